#!/usr/bin/env python3
"""Regenerates the fixtures of `bwbble map -X` (a read's other placements: the tags X0 / X1 / XA) from the REAL reference - run where the
reference is built, like make_golden_map.py, whose rep.fa index these files sit on.  Only data lands in tests/golden:

  rep_sa.npy        the reference's SA(i) for every row i of the rep.fa index (53 305 values, <u4), dumped by a throw-away harness that is
                    written to a temporary directory and linked against the reference's own objects in oracle/_ref/obj (as make_golden.py
                    does for the rank vectors).  The judge of every text position the tests expect on this index.
  rep_gap.fq        reads of 100 bases cut from the planted repeat units of rep.fa (make_golden_map.make_genome) with one base inserted or
  rep_gap_n4.aln    deleted, alternating strands; and the reference's `align -n 4 -o 1` on them: gapped hits at several loci
  alt_hits.aln      hit lists on the rep index that no search produces (written by this script: our data), every looked-up row inside the
  alt_hits.fq.gz    index; make_alt_hits() lists the cases, check() asserts them.  The reads' bases only travel to the SAM line.

A read of alt_hits is left with no hits only where its PRIMARY is undefined in the reference, by make_golden_map's rule: its position
outside every annotated sequence, or top2 < 0 with top1 == 1 or top1 < 0.  At most 5 % of the reads may end like that.
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bwbble")
REF_OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")

from golden import make_golden_map as mgm  # noqa: E402
from golden.make_golden import REF_SRC  # noqa: E402  (where the reference's headers lie)
from golden.make_golden_map import M, I, D, hit, read_len  # noqa: E402

# calls the reference's own load_bwt and SA (bwt.h): one 32-bit value per row
HARNESS = r"""
#include <stdio.h>
#include <stdint.h>
#include "bwt.h"
int main(int argc, char** argv) {
	if (argc < 3) return 2;
	bwt_t* BWT = load_bwt(argv[1], 1);
	FILE* o = fopen(argv[2], "wb");
	if (!o) return 2;
	for (bwtint_t i = 0; i < BWT->length; i++) { uint32_t v = (uint32_t) SA(BWT, i); fwrite(&v, 4, 1, o); }
	fclose(o);
	return 0;
}
"""
GAP_SEED, ALT_SEED, ALT_RANDOM_READS = 20261018, 20261019, 150
NS = (1, 5, 255)  # the values of -X whose boundaries the fixture holds


def make_rep_sa(tmp):
    hsrc, hbin, out = os.path.join(tmp, "sa_harness.c"), os.path.join(tmp, "sa_harness"), os.path.join(tmp, "sa.u32")
    open(hsrc, "w").write(HARNESS)
    objs = sorted(os.path.join(REF_OBJ, o) for o in os.listdir(REF_OBJ) if o.endswith(".o") and o != "main.o")
    mgm.run(["gcc", "-w", "-O2", "-std=gnu99", "-fopenmp", "-I", REF_SRC, hsrc] + objs + ["-o", hbin, "-lm", "-lz", "-lpthread"])
    mgm.run([hbin, os.path.join(HERE, "rep.fa.bwt"), out])
    sa = np.fromfile(out, dtype="<u4")
    assert len(sa) == int(np.fromfile(os.path.join(HERE, "rep.fa.bwt"), dtype="<u8", count=1)[0])
    np.save(os.path.join(HERE, "rep_sa.npy"), sa)
    return sa


def make_rep_gap(rng):
    """reads from the planted units with one inserted or one deleted base in their middle, both strands -> FASTQ text"""
    recs, text, where, split = mgm.make_genome(random.Random(20261016))  # (the genome of rep.fa, drawn again)
    fa = "".join(ln for ln in open(os.path.join(HERE, "rep.fa")).read().split("\n") if not ln.startswith(">"))
    assert fa == text, "rep.fa is not the genome make_golden_map draws"
    plan = [("u1" + "abc"[k % 3]) for k in range(12)] + [("u3" + "ab"[k % 2]) for k in range(10)] + ["u4"] * 8 + ["u3m1"] * 4 + ["u2"] * 6
    rng.shuffle(plan)
    out = []
    for i, tag in enumerate(plan):
        o = where[tag] + rng.randrange(0, mgm.UNIT - mgm.READ + 1)
        at = rng.randrange(30, 70)
        if i % 2:  # one base inserted into the read (the read keeps 100 bases)
            read = text[o:o + at] + rng.choice("ACGT") + text[o + at:o + mgm.READ - 1]
        else:      # one base of the text left out
            read = text[o:o + at] + text[o + at + 1:o + mgm.READ + 1]
        assert len(read) == mgm.READ
        strand = (i // 2) % 2
        if strand:
            read = read[::-1].translate(mgm.COMP)
        qual = "".join(rng.choice("ABCDEFGHIJ0123456789") for _ in range(mgm.READ))
        out.append(f"@gap{i}_{tag}_{'ins' if i % 2 else 'del'}_{'-' if strand else '+'}\n{read}\n+\n{qual}\n")
    return "".join(out)


def check_rep_gap(here=HERE):
    import alt_model
    import oracle_lib
    reads = oracle_lib.parse_aln(open(os.path.join(here, "rep_gap_n4.aln"), "rb").read())
    good = [e for e in reads if 2 <= alt_model.placements(e) <= 6 and any(x["gapo"] for x in e)]
    assert len(good) >= 10, f"only {len(good)} reads with 2 <= T <= 6 and a gapped hit"
    return reads


def make_alt_hits(rng, fsa, ann):
    """-> (FASTQ text, hit lists, reads left without hits).  fsa: alt_model.FullSA of rep_sa.npy; ann: [(start, end)]"""
    import map_model
    length = fsa.length
    sa0 = int(fsa.isa[0])

    def pos_of(row, ref_len):
        rp = int(fsa.sa[row])
        fwd = rp > (length - 1) // 2
        pos = (length - 1) - rp - 1 - ref_len + 1 if fwd else rp
        return fwd, pos, any(a <= pos <= b for a, b in ann)

    def row_where(ref_len=100, fwd=None, width=1, pred=lambda r: True):
        """a random row L with [L, L + width) inside the index, the row itself inside a record and, if asked, on that strand"""
        span = width if width < length // 2 else 1  # (the rows of a hit too wide for any list are never looked up)
        for _ in range(200000):
            row = rng.randrange(1, length - span)
            f, _, ok = pos_of(row, ref_len)
            if ok and (fwd is None or f == fwd) and pred(row):
                return row
        raise AssertionError("no such row")

    plain = lambda n=100: [(M, n)]
    gap = [(M, 30), (D, 2), (M, 30), (I, 1), (M, 39)]
    eight = [(M, 10), (I, 1), (M, 5), (D, 2), (M, 7), (I, 3), (D, 4), (M, 9), (I, 2), (M, 6), (D, 1), (M, 8), (I, 25), (M, 11), (D, 3), (M, 20)]
    at = lambda segs, row, **kw: hit(segs, row, **kw)
    rnd = lambda segs=None, width=1, **kw: hit(segs or plain(), row_where(width=width), width=width, **kw)
    reads = []
    # T on both sides of the list's limit for -X 1, 5 and 255: from hits one row wide, from one wide hit, and mixed
    for N in NS:
        for T in (N + 1, N + 2):
            reads.append([rnd(mm=1)] + [rnd(score=6, mm=2) for _ in range(min(T - 1, 7))] + ([rnd(width=T - 8, score=6, mm=2)] if T > 8 else []))
            reads.append([rnd(width=T, mm=1)])
            reads.append([rnd(width=T - 1, mm=1), rnd(gap, score=14)])
    for ents in reads:
        assert sum(e["U"] - e["L"] + 1 for e in ents) in {N + d for N in NS for d in (1, 2)}
    # a wide primary: the items start with the rest of the first hit's rows; and a wide hit in the middle of the list
    reads.append([rnd(width=3), rnd(gap, score=14), rnd(score=6, mm=2)])
    reads.append([rnd(gap, width=4, score=14), rnd(score=17, mm=1, segs=gap)])
    reads.append([rnd(), rnd(gap, width=3, score=14), rnd(score=6, mm=2)])
    reads.append([rnd(mm=1), rnd(score=6, mm=2), rnd(gap, width=2, score=14), rnd(score=9, mm=3), rnd(gap, score=14)])
    reads.append([rnd(), rnd(width=100, score=3), rnd(gap, width=100, score=14), rnd(score=6, mm=2)])  # 202 placements: listed by -X 255 only
    # eight gap runs on an ITEM, on both strands, in both orders of the path
    for segs in (eight, eight[::-1]):
        for fwd in (True, False):
            h = hit(segs, 1, score=70)
            h["L"] = h["U"] = row_where(h["aln_length"], fwd)
            reads.append([hit(plain(read_len(h)), row_where(read_len(h)), mm=1), h])
            reads.append([hit(plain(read_len(h)), row_where(read_len(h)), width=2, mm=1), h, hit(plain(read_len(h)), row_where(read_len(h)), score=6, mm=2)])
    # item rows that are special for the walk: the sentinel row, multiples of 32, length - 1, and their neighbours
    for row in (sa0, sa0 - 1, sa0 + 1, length - 1, length - 2, 32, 64, 31, 33, 1, (sa0 // 32) * 32, (sa0 // 32 + 1) * 32):
        reads.append([rnd(mm=1), at(gap, row, score=14)])
    reads.append([rnd(), at(plain(), sa0 - 1, width=3, score=3)])         # a wide hit across the sentinel row
    reads.append([rnd(), at(plain(), length - 3, width=3, score=3)])      # ... and up to the last row of the index
    reads.append([rnd(), at(plain(), 30, width=5, score=3)])              # ... and across a sampled row
    # no list: widths of 2^32 and more (the 64-bit sum), a sum that only saturates, U < L
    reads.append([rnd(width=2**32, mm=1)])
    reads.append([rnd(width=2**32 + 1, mm=1), rnd(score=6)])              # 2 placements if the widths were summed in 32 bits
    reads.append([rnd(mm=1), rnd(width=2**32 + 2, score=6)])              # 3 placements if ...
    reads.append([rnd(width=2), rnd(width=2**32, score=6)])               # 2 placements if ...
    reads.append([rnd(width=2, mm=1), at(plain(), 1, width=2**64 - 2, score=6)])  # the sum itself overflows 64 bits
    reads.append([rnd(mm=1), rnd(width=2**63, score=6), rnd(width=2**63, score=6)])
    for bad in ((500, 499), (500, 100), (2**40, 5)):                      # U < L on a later hit: saturated, whatever stands before
        h = rnd(score=6)
        h["L"], h["U"] = bad
        reads.append([rnd(mm=1), h])
        reads.append([rnd(width=2, mm=1), h, rnd(score=6)])
    # an item whose position lies in no annotation record: a forward-strand row so close to the end of the text that the position is
    # negative (and wraps), and the row of the separator between the two strands; between two items that are listed
    beyond = int(fsa.isa[length - 1 - 10])
    middle = int(fsa.isa[(length - 1) // 2])
    assert not pos_of(beyond, 100)[2] and not pos_of(middle, 100)[2]
    reads.append([rnd(mm=1), at(plain(), beyond, score=6, mm=2)])
    reads.append([rnd(mm=1), rnd(score=6, mm=2), at(plain(), beyond, score=6, mm=2), rnd(gap, score=14)])
    reads.append([rnd(mm=1), at(plain(), middle, score=6, mm=2), rnd(score=6, mm=2)])
    # reads without hits
    for _ in range(4):
        reads.append([])
    # random lists: 0-6 hits of 1-5 rows, paths and rows drawn independently
    for _ in range(ALT_RANDOM_READS):
        rlen = rng.choice([30, 64, 65, 100, 128, 129, 150, 200])
        ents = []
        for _ in range(rng.choice([0, 1, 1, 2, 2, 3, 4, 6])):
            w = rng.choice([1, 1, 1, 1, 2, 2, 3, 5])
            ents.append(hit(mgm.random_path(rng, rlen), rng.randrange(1, length - w), width=w, score=rng.choice([0, 3, 3, 6, 300]), mm=rng.randrange(0, 7)))
        reads.append(ents)
    for ents in reads:  # every hit of a read describes the same read
        assert len({read_len(e) for e in ents}) <= 1
    lens = [read_len(ents[0]) if ents else rng.choice([30, 100, 250]) for ents in reads]
    order = list(range(len(reads)))
    rng.shuffle(order)
    reads, lens = [reads[k] for k in order], [lens[k] for k in order]
    dropped = 0
    for r, ents in enumerate(reads):
        if ents and primary_undefined(ents, pos_of):
            reads[r] = []
            dropped += 1
    assert dropped <= 0.05 * len(reads), f"{dropped} of {len(reads)} reads left out"
    fq = []
    for r, n in enumerate(lens):
        fq.append(f"@a{r}\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{''.join(rng.choice('ABCDEFGHIJ0123456789') for _ in range(n))}\n")
    return "".join(fq), reads, dropped


def primary_undefined(ents, pos_of):
    """make_golden_map's rule: the primary outside every annotated sequence, or a MAPQ the reference computes from log() of a negative number"""
    import map_model
    e0 = ents[0]
    top1 = map_model.wrap32(sum(e["U"] - e["L"] + 1 for e in ents if e["score"] <= e0["score"]))
    top2 = map_model.wrap32(sum(e["U"] - e["L"] + 1 for e in ents if e["score"] > e0["score"]))
    ref_len = e0["aln_length"] - sum(s >> 2 for s in e0["states"] if (s & 3) == I)
    return not pos_of(e0["L"], ref_len)[2] or (top2 < 0 and (top1 == 1 or top1 < 0))


def unpack_alt(dst, here=HERE):
    """writes alt_hits.fq out into dst (the host tools read plain files) -> its path"""
    path = os.path.join(str(dst), "alt_hits.fq")
    with open(path, "wb") as f:
        f.write(gzip.open(os.path.join(here, "alt_hits.fq.gz"), "rb").read())
    return path


def check(here=HERE):
    """the cases alt_hits exists for, asserted on the files (tests/test_alt_host.py does the same on the committed ones) -> the hit lists"""
    import alt_model
    import oracle_lib
    reads = oracle_lib.parse_aln(open(os.path.join(here, "alt_hits.aln"), "rb").read())
    fq_lens = [len(ln) for ln in mgm.read_text(os.path.join(here, "alt_hits.fq.gz")).split("\n")[1::4]]
    assert len(reads) == len(fq_lens) and 150 <= len(reads) <= 400
    fsa = alt_model.rep_sa(here)
    length, sa0 = fsa.length, int(fsa.isa[0])
    ann = alt_model.read_ann(os.path.join(here, "rep.fa.ann"))
    T = [alt_model.placements(e) for e in reads]
    w = lambda e: e["U"] - e["L"] + 1
    for r, ents in enumerate(reads):
        assert all(read_len(e) == fq_lens[r] and e["aln_length"] <= 255 and e["gapo"] == len(mgm.runs_of(e)) <= 8 for e in ents), r
    # T equal to N + 1 and to N + 2
    for N in NS:
        assert N + 1 in T and N + 2 in T, N
        assert any(t == N + 1 and len(e) > 1 for t, e in zip(T, reads)) and any(t == N + 2 and len(e) > 1 for t, e in zip(T, reads)), N
    # a wide primary; a wide hit in the middle of the list
    assert any(2 <= t <= 6 and w(e[0]) > 1 and len(e) > 1 for t, e in zip(T, reads))
    assert any(2 <= t <= 6 and len(e) >= 3 and w(e[0]) == 1 and any(w(x) > 1 for x in e[1:-1]) for t, e in zip(T, reads))
    assert any(6 < t <= 256 and len(e) >= 3 and any(w(x) > 1 for x in e[1:-1]) for t, e in zip(T, reads))
    # the items at -X 255: their rows, strands, runs and records
    off, alts, _ = alt_model.expected_alts(reads, 255, fsa)
    rows = [row for e in reads for _, row in alt_model.item_rows(e, 255)]
    assert len(rows) == len(alts) >= 500
    live = (alts["gap_run"] != 0xFFFF).sum(axis=1)
    rev = (alts["flags"] & 2) != 0
    assert ((live == 8) & rev).sum() >= 2 and ((live == 8) & ~rev).sum() >= 2
    assert {sa0, length - 1, 32, 64} <= set(rows) and any(r % 32 == 0 and r not in (32, 64) for r in rows)
    assert {sa0 - 1, sa0 + 1, 31, 33, 1} <= set(rows)
    inside = np.array([any(s <= int(p) <= e for _, s, e in ann) for p in alts["pos"]])
    assert 1 <= (~inside).sum() <= 0.05 * len(alts) + 3
    assert any((~inside[int(a):int(b)]).any() and inside[int(a):int(b)].any() for a, b in zip(off[:-1], off[1:]))  # left out between listed ones
    assert (alts["pos"] >= 2**63).any()  # a position that wrapped
    assert {0, 1} <= set(int(h) for h in alts["hit"]) and max(int(h) for h in alts["hit"]) >= 5
    # no list: widths of 2^32 and more, U < L
    assert any(any(2**32 <= w(x) for x in e if x["U"] >= x["L"]) for e in reads)
    assert any(2 <= sum(w(x) for x in e) % 2**32 <= 6 and t >= 2**32 for t, e in zip(T, reads) if all(x["U"] >= x["L"] for x in e))  # a 32-bit sum would list
    assert any(t == alt_model.SAT and all(x["U"] >= x["L"] for x in e) for t, e in zip(T, reads))  # the 64-bit sum saturates
    assert sum(1 for e in reads if any(x["U"] < x["L"] for x in e)) >= 3
    assert all(alt_model.n_items(e, 255) == 0 for e in reads if any(x["U"] < x["L"] or w(x) >= 2**32 for x in e))
    # reads without hits; every looked-up row inside the index; every primary defined
    assert sum(1 for e in reads if not e) >= 4
    assert all(e[0]["L"] < length for e in reads if e) and all(r < length for r in rows)

    def pos_of(row, ref_len):
        rp = int(fsa.sa[row])
        pos = (length - 1) - rp - 1 - ref_len + 1 if rp > (length - 1) // 2 else rp
        return rp > (length - 1) // 2, pos, any(s <= pos <= e for _, s, e in ann)
    assert not any(primary_undefined(e, pos_of) for e in reads if e)
    return reads


def main():
    if not os.path.exists(REF_BIN) or not os.path.isdir(REF_OBJ):
        sys.exit("oracle/_ref is missing: the fixtures can only be regenerated where the reference is present (make -C oracle ref)")
    import alt_model
    with tempfile.TemporaryDirectory() as tmp:
        sa = make_rep_sa(tmp)
        fa = os.path.join(HERE, "rep.fa")
        fq, aln = os.path.join(HERE, "rep_gap.fq"), os.path.join(HERE, "rep_gap_n4.aln")
        open(fq, "w").write(make_rep_gap(random.Random(GAP_SEED)))
        if os.path.exists(aln):
            os.remove(aln)
        mgm.run([REF_BIN, "align", "-n", "4", "-o", "1", fa, fq, aln])
    gap_reads = check_rep_gap()
    fsa = alt_model.FullSA(sa)
    ann = mgm.read_ann(os.path.join(HERE, "rep.fa.ann"))
    text, reads, dropped = make_alt_hits(random.Random(ALT_SEED), fsa, ann)
    open(os.path.join(HERE, "alt_hits.aln"), "wb").write(mgm.serialize_aln(reads))
    with open(os.path.join(HERE, "alt_hits.fq.gz"), "wb") as f:
        f.write(gzip.compress(text.encode(), 9, mtime=0))
    check()
    from collections import Counter
    print("rep_gap_n4: T of the reads", sorted(Counter(alt_model.placements(e) for e in gap_reads).items()))
    print(f"alt_hits: {len(reads)} reads, {sum(1 for e in reads if e)} with hits, {dropped} left out ({100 * dropped / len(reads):.1f} %)")


if __name__ == "__main__":
    main()
