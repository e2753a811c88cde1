#!/usr/bin/env python3
"""Regenerates the `rep` fixtures of tests/golden from the REAL reference (run in the build container only, like make_golden.py).

The synthetic toy genome has no repeats: every mapped read of the toy fixtures has exactly one hit of interval width 1, so of mapq's six
outcomes (align.c:738-746) the toy .sam files only ever show two (37 and unmapped).  The sums over a read's hit list - the part of
eval_aln that `bwbble map` computes on the GPU - need a genome with planted repeats:

  rep.fa      two records, 26 650 random A/C/G/T characters holding four 150-base units:
                U1  three verbatim copies                               -> top1 = 3               MAPQ 0, first hit with U > L
                U2  the unit, a one-mismatch copy, a two-mismatch copy  -> top1 = 1, top2 = 1     MAPQ 23
                U3  two verbatim copies and a one-mismatch copy         -> top1 = 2: MAPQ 0; read from the copy: top2 = 2, MAPQ 20
                U4  the unit and five one-mismatch copies               -> top1 = 1, top2 = 5     MAPQ 16
  rep.fq      104 reads of 100 bases: cut from the units and from unique text with 0-3 substitutions, alternating strands (unique text
              with three substitutions: MAPQ 25 under `aln2sam -n 3`, 37 under the default 6), and four random reads (unmapped)
  rep.fa.bwt, rep.fa.ann          the reference's `index`
  rep_n3.aln                      the reference's `align -n 3`
  rep_n3.sam, rep_n3_q3.sam       the reference's `aln2sam` with its default -n 6, and with -n 3

Only data lands in tests/golden; the .ref file that `index` also writes is removed (as for toy.fa).  The script asserts that what the
reference wrote covers the MAPQ outcomes listed above; tests/test_map_host.py asserts the same on the committed files.

The hits the search finds on such a genome still leave most of eval_aln's input space alone (paths of 100 positions with a run or two,
sums of a handful of rows).  The reference's `aln2sam` takes any .aln file, so the second fixture hands it hit lists nobody searched for:

  synth_hits.fq.gz  random reads of 30-250 bases on the rep.fa index (their bases only travel to the SAM line)
  synth_hits.aln    0-17 made-up hits per read, in the reference's .aln format (written by this script: our data): up to eight gap runs
                    anywhere on the path, interval widths up to 2^32 + 1, first rows that are special for the invPsi walk - make_synth()
                    lists the cases, check_synth() asserts them
  synth_hits_n6.sam.gz, synth_hits_n3.sam.gz    the reference's `aln2sam` on them with its default -n 6, and with -n 3
  (the three text files are 340 KB of random bases and qualities that nobody reads: committed gzipped, with a zero time stamp;
  unpack_synth() writes them out for the tools, which take plain files)

A read is left with no hits (itself a case) where the reference's behaviour is undefined: its first hit's position outside every
annotated sequence (print_aln2sam indexes seq_anns[-1]), or top2 < 0 with top1 == 1 or top1 < 0 (mapq takes log() of a negative number
and converts NaN to int).  At most 5 % of the generated reads may end like that.
"""
import gzip
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bwbble")
UNIT, READ = 150, 100
COMP = str.maketrans("ACGT", "TGCA")


def run(cmd):
    print("+", " ".join(cmd))
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)


def mutate(rng, s, positions):
    s = list(s)
    for p in positions:
        s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
    return "".join(s)


def make_genome(rng):
    """-> (records [(name, text)], the whole text, {tag: offset in it} of every planted unit copy, where the second record starts)"""
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    u1, u2, u3, u4 = (rnd(UNIT) for _ in range(4))
    # (a copy's mismatches lie in 55..94: inside every 100-base window cut at offset 0..50 of the unit)
    copies = [("u1a", u1), ("u1b", u1), ("u1c", u1),
              ("u2", u2), ("u2m1", mutate(rng, u2, [70])), ("u2m2", mutate(rng, u2, [62, 88])),
              ("u3a", u3), ("u3b", u3), ("u3m1", mutate(rng, u3, [75])),
              ("u4", u4)] + [(f"u4m{k}", mutate(rng, u4, [56 + 7 * k])) for k in range(5)]
    rng.shuffle(copies)
    total = 26650
    filler = total - UNIT * len(copies)
    cuts = sorted(rng.sample(range(400, filler - 400, 50), len(copies)))  # filler characters in front of each copy
    text, where, prev = [], {}, 0
    for (tag, seq), cut in zip(copies, cuts):
        text.append(rnd(cut - prev))
        prev = cut
        where[tag] = sum(len(t) for t in text)
        text.append(seq)
    text.append(rnd(filler - prev))
    text = "".join(text)
    assert len(text) == total
    split = 14000
    while any(off - READ < split < off + UNIT + READ for off in where.values()):
        split += 10
    recs = [("rep1", text[:split]), ("rep2", text[split:])]
    return recs, text, where, split


def make_reads(rng, text, where, split):
    planted = sorted(where.values())

    def unique_offset():
        while True:
            o = rng.randrange(0, len(text) - READ)
            if all(o + READ + 20 < p or o > p + UNIT + 20 for p in planted) and not (split - READ - 20 < o < split + 20):
                return o

    plan = ([("u1" + "abc"[k % 3], k % 2) for k in range(20)] + [("u3" + "ab"[k % 2], 0) for k in range(20)] +
            [("u4", 0)] * 5 + [("u3m1", 0)] * 5 + [("u2", 0)] * 10 + [("uniq", k % 4) for k in range(40)])
    rng.shuffle(plan)
    out = []
    for i, (tag, nsub) in enumerate(plan):
        o = unique_offset() if tag == "uniq" else where[tag] + rng.randrange(0, UNIT - READ + 1)
        read = mutate(rng, text[o:o + READ], [(10, 45, 80)[k] + rng.randrange(0, 8) for k in range(nsub)])
        strand = i % 2
        if strand:
            read = read[::-1].translate(COMP)
        qual = "".join(rng.choice("ABCDEFGHIJ0123456789") for _ in range(READ))
        out.append(f"@rep{i}_{tag}_s{nsub}_{'-' if strand else '+'}\n{read}\n+\n{qual}\n")
    for k in range(4):
        read = "".join(rng.choice("ACGT") for _ in range(READ))
        out.insert(rng.randrange(0, len(out)), f"@rnd{k}\n{read}\n+\n{'5' * READ}\n")
    return "".join(out)


def read_text(path):
    return gzip.open(path, "rt").read() if path.endswith(".gz") else open(path).read()


def sam_records(path):
    return [ln.split("\t") for ln in read_text(path).split("\n") if ln and not ln.startswith("@")]


SYNTH_TEXT = ("synth_hits.fq", "synth_hits_n6.sam", "synth_hits_n3.sam")


def unpack_synth(dst, here=HERE):
    """writes the gzipped text files of the synth_hits fixture out into dst (the host tools read plain files) -> dst"""
    for name in SYNTH_TEXT:
        with open(os.path.join(str(dst), name), "wb") as f:
            f.write(gzip.open(os.path.join(here, name + ".gz"), "rb").read())
    return str(dst)


def check(here=HERE):
    """the outcomes the fixture exists for (also asserted by tests/test_map_host.py on the committed files)"""
    d, q3 = sam_records(os.path.join(here, "rep_n3.sam")), sam_records(os.path.join(here, "rep_n3_q3.sam"))
    mq = [(int(r[1]), int(r[4])) for r in d]
    assert any(f != 4 and q == 0 for f, q in mq), "no MAPQ 0 on a mapped read"
    assert any(q == 23 for _, q in mq) and any(0 < q < 23 for _, q in mq) and any(q == 37 for _, q in mq)
    assert any(int(r[4]) == 25 for r in q3)
    assert {0, 16} <= {f for f, _ in mq}
    return mq


# ---- synthetic hit lists ------------------------------------------------------------------------------------------------------------
M, I, D = 0, 1, 2
SYNTH_SEED, SYNTH_RANDOM_READS = 20261017, 320


def read_ann(path):
    """[(start_index, end_index)] of a .ann file (both inclusive, the way print_aln2sam compares, align.c:567)"""
    return [(int(f[1]), int(f[2])) for f in (ln.rsplit(None, 2) for ln in open(path).read().split("\n")[1:]) if len(f) == 3]


def hit(segs, L, width=1, score=3, mm=0):
    """one hit in oracle_lib.parse_aln's form from its path as (state, count) segments in the .aln file's order"""
    merged = []
    for st, cnt in segs:
        if merged and merged[-1][0] == st:
            merged[-1] = (st, merged[-1][1] + cnt)
        else:
            merged.append((st, cnt))
    alen = sum(c for _, c in merged)
    assert alen <= 255 and all(c <= 127 for st, c in merged if st)
    return dict(score=score, L=L, U=L + width - 1, mm=mm, gapo=sum(1 for st, _ in merged if st), gape=sum(c - 1 for st, c in merged if st),
                aln_length=alen, states=[st | (c << 2) for st, c in merged])


def read_len(h):
    return sum(s >> 2 for s in h["states"] if (s & 3) != D)


def runs_of(h, align_time=False):
    """[(start, len, state)] of a hit's gap runs on the file's path, or on the align-time path (the file's reversed: what k_place maps)"""
    out, pos = [], 0
    for s in h["states"]:
        st, cnt = s & 3, s >> 2
        if st:
            out.append((h["aln_length"] - pos - cnt if align_time else pos, cnt, st))
        pos += cnt
    return out


def random_path(rng, rlen):
    """a path of rlen read bases with 0-8 runs (the experiment's distribution); an insertion may sit directly next to a deletion"""
    nruns = rng.choice([0, 0, 1, 1, 2, 3, 5, 8])
    runs = [(rng.choice([I, D]), rng.choice([1, 1, 2, 3, 7, 20])) for _ in range(nruns)]
    m_total = rlen - sum(c for st, c in runs if st == I)
    if m_total < nruns + 1 or rlen + sum(c for st, c in runs if st == D) > 255:
        return [(M, rlen)]
    cuts = sorted(rng.sample(range(1, m_total), nruns)) if nruns else []
    if nruns >= 2 and runs[0][0] != runs[1][0] and rng.random() < 0.3:
        cuts[1] = cuts[0]  # no match between the first two runs
    ms = [b - a for a, b in zip([0] + cuts, cuts + [m_total])]
    segs = []
    for k, m in enumerate(ms):
        if m:
            segs.append((M, m))
        if k < nruns:
            segs.append(runs[k])
    return segs


def make_synth(rng, orc, idx, ann, through_sentinel=True):
    """-> (FASTQ text, hit lists, number of reads left without hits by the two conditions of the module's docstring).  Works on any index;
    through_sentinel=False leaves out the rows whose walk passes through the sentinel row, which are found by drawing rows: a matter of
    thousands of draws on rep.fa's 53 305 rows, hopeless on millions"""
    import map_model
    length, sa0 = int(idx.contents.length), int(idx.contents.sa0_index)
    walks = {}

    def walk(row):
        if row not in walks:
            walks[row] = map_model.walk_rows(orc, idx, row)
        return walks[row]

    def placed(row, ref_len):
        rows = walk(row)
        rp = (int(idx.contents.SA[rows[-1] // 32]) + len(rows) - 1) % length
        pos = (length - 1) - rp - 1 - ref_len + 1 if rp > (length - 1) // 2 else rp
        return rp > (length - 1) // 2, any(a <= pos <= b for a, b in ann)

    def row_where(pred, ref_len=100, fwd=None):
        """a random row that satisfies pred(row, its walk), lands inside an annotated sequence and, if asked, on that strand"""
        for _ in range(200000):
            row = rng.randrange(1, length)
            f, ok = placed(row, ref_len)
            if ok and (fwd is None or f == fwd) and pred(row, walk(row)):
                return row
        raise AssertionError("no such row")

    anyrow = lambda ref_len=100, fwd=None: row_where(lambda r, w: True, ref_len, fwd)
    plain = lambda n: [(M, n)]
    reads = []  # hit lists
    # read lengths on both sides of the words of the 256-bit insertion map, no gap
    for n in (30, 63, 64, 65, 127, 128, 129, 191, 192, 193, 250):
        reads.append([hit(plain(n), anyrow(n))])
    # gap runs: 1, 2, 3, 5 and 8 of them; insertions and deletions mixed, an insertion next to a deletion, run lengths 1 and 25
    eight = [(M, 10), (I, 1), (M, 5), (D, 2), (M, 7), (I, 3), (D, 4), (M, 9), (I, 2), (M, 6), (D, 1), (M, 8), (I, 25), (M, 11), (D, 3), (M, 20)]
    five = [(M, 20), (D, 1), (M, 30), (I, 20), (M, 3), (I, 1), (M, 40), (D, 5), (I, 2), (M, 30)]
    for segs in ([(M, 40), (I, 2), (M, 58)], [(M, 40), (D, 2), (M, 20), (I, 1), (M, 39)], [(M, 10), (I, 3), (M, 10), (D, 3), (M, 10), (I, 4), (M, 60)],
                 five, five[::-1], eight, eight[::-1]):
        for fwd in (True, False):
            h = hit(segs, 1)
            h["L"] = h["U"] = anyrow(h["aln_length"], fwd)
            reads.append([h])
    # a run at path position 0 and one that ends at aln_length (both orientations: the path and its reverse)
    for segs in ([(I, 2), (M, 50), (D, 3)], [(D, 3), (M, 50), (I, 2)]):
        reads.append([hit(segs, anyrow(60))])
    # runs across bits 64, 128 and 192 of the map: on the file's path, and (the reverse) on the align-time path k_place maps; insertions,
    # then the same with deletions on top of which nothing lies
    cross = [(M, 60), (I, 10), (M, 54), (I, 8), (M, 56), (I, 8), (M, 30)]
    for segs in (cross, cross[::-1], [(st and D, c) for st, c in cross], [(st and D, c) for st, c in cross[::-1]]):
        reads.append([hit(segs, anyrow(220))])
    # an insertion run that fills a whole word of the map (bits 64..127 and more), and one that ends exactly at a word's last bit
    for segs in ([(M, 60), (I, 100), (M, 40)], [(M, 40), (I, 100), (M, 60)], [(M, 64), (I, 64), (M, 64)], [(M, 100), (I, 28), (D, 64), (M, 50)]):
        reads.append([hit(segs, anyrow(150))])
    # top2 of 0 (above), 1, 254, 255, 256 and 20 000 with top1 = 1: a table value each, the clamp at 255 on both sides
    for t2 in ([1], [254], [255], [256], [100, 154], [200, 55], [20000], [1, 1, 1]):
        reads.append([hit(plain(100), anyrow(), mm=1)] + [hit(plain(100), anyrow(), width=w, score=6, mm=2) for w in t2])
    # sums that wrap (align.c:773,776 add 64-bit widths into ints)
    big = lambda w, score, **kw: hit(plain(100), anyrow(), width=w, score=score, **kw)
    reads.append([big(2**32 + 1, 3, mm=1)])                          # top1 = 1 only through wrapping, top2 = 0: 37
    reads.append([big(2**32 + 1, 3, mm=2), big(3, 6)])               # the same with top2 = 3
    reads.append([big(2**32, 3)])                                    # top1 wraps to 0 on a mapped read: 23
    reads.append([big(2**31, 3), big(2**31, 3)])                     # the same from two hits
    reads.append([big(2**31, 3)])                                    # top1 negative, top2 = 0
    reads.append([big(2**32 - 1, 3), big(5, 6)])                     # top1 = -1, top2 = 5
    reads.append([big(1, 3), big(2**32, 6)])                         # top2 wraps to 0: 37
    reads.append([big(1, 3), big(2**31, 6), big(2**31, 6), big(7, 6)])  # top2 wraps to 7
    reads.append([big(2, 3), big(2**31, 6)])                         # top2 negative behind a repeat: 0
    reads.append([big(1, 3), big(2**32 + 254, 6)])                   # top2 = 254 through wrapping
    # a later hit that scores below the first one counts for top1
    reads.append([big(1, 6), big(5, 3)])
    reads.append([big(1, 6, mm=1), big(1, 9), big(1, 3), big(1, 6)])
    # scores above 255 (bwb_aln.score is 16 bits wide)
    reads.append([big(1, 300, mm=2), big(4, 310), big(1, 256)])
    reads.append([big(1, 255), big(2, 256)])
    # nine and seventeen hits: more than one pass of the octet's stride, every lane with a different width
    reads.append([big(1, 3, mm=1)] + [big(k + 1, 6) for k in range(8)])
    reads.append([big(1, 3, mm=1)] + [big(k + 1, 6) for k in range(16)])
    reads.append([big(1, 3)] + [big(1 << k, 3 + 3 * (k % 2)) for k in range(16)])
    # num_mm == 3 on a unique read: 25 under -n 3, 37 under -n 6; and num_mm == 6
    reads.append([big(1, 9, mm=3)])
    reads.append([big(1, 18, mm=6), big(3, 21)])
    # first rows that are special for the walk, on whichever strand they lie, with a deletion so that ref_len differs from the read's length
    gap = [(M, 30), (D, 2), (M, 30), (I, 1), (M, 39)]
    for row in (sa0, sa0 - 1, sa0 + 1, length - 1, 1, 31, 32, 33, length - 2):
        reads.append([hit(gap, row)])
    for fwd in (True, False):
        reads.append([hit(gap, row_where(lambda r, w: len(w) == 1, fwd=fwd))])                      # a sampled row: no step
        reads.append([hit(gap, row_where(lambda r, w: len(w) == 32, fwd=fwd))])                     # 31 steps
        reads.append([hit(gap, row_where(lambda r, w: r % 32 == 1, fwd=fwd))])                      # 32 k + 1
        reads.append([hit(gap, row_where(lambda r, w: r % 32 == 31, fwd=fwd))])
    if through_sentinel:
        for _ in range(3):
            reads.append([hit(gap, row_where(lambda r, w: sa0 in w[1:-1]))])                        # the walk passes through the sentinel row
        reads.append([hit(gap, row_where(lambda r, w: len(w) > 1 and w[1] == sa0))])
    # random hit lists: lengths, paths, widths and rows drawn independently
    for _ in range(SYNTH_RANDOM_READS):
        rlen = rng.choice([30, 64, 65, 100, 128, 129, 150, 192, 200, 250])
        ents = []
        for _ in range(rng.choice([0, 1, 1, 2, 3, 9, 17])):
            w = rng.choice([1, 1, 1, 2, 3, 100, 254, 255, 256, 2**31 - 1, 2**32, 2**32 + 1])
            ents.append(hit(random_path(rng, rlen), rng.randrange(1, length), width=w, score=rng.choice([0, 3, 3, 6, 300]), mm=rng.randrange(0, 7)))
        reads.append(ents)
    # every hit of a read describes the same read: the designed lists above use one length per list already
    for ents in reads:
        assert len({read_len(e) for e in ents}) <= 1
    lens = [read_len(ents[0]) if ents else rng.choice([30, 100, 250]) for ents in reads]
    order = list(range(len(reads)))
    rng.shuffle(order)
    reads, lens = [reads[k] for k in order], [lens[k] for k in order]
    # the two conditions under which the reference's output is undefined
    dropped = 0
    for r, ents in enumerate(reads):
        if not ents:
            continue
        e0 = ents[0]
        top1 = map_model.wrap32(sum(e["U"] - e["L"] + 1 for e in ents if e["score"] <= e0["score"]))
        top2 = map_model.wrap32(sum(e["U"] - e["L"] + 1 for e in ents if e["score"] > e0["score"]))
        ref_len = e0["aln_length"] - sum(s >> 2 for s in e0["states"] if (s & 3) == I)
        if not placed(e0["L"], ref_len)[1] or (top2 < 0 and (top1 == 1 or top1 < 0)):
            reads[r] = []
            dropped += 1
    assert dropped <= 0.05 * len(reads), f"{dropped} of {len(reads)} reads left out"
    fq = []
    for r, n in enumerate(lens):
        fq.append(f"@s{r}\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{''.join(rng.choice('ABCDEFGHIJ0123456789') for _ in range(n))}\n")
    return "".join(fq), reads, dropped


def serialize_aln(reads):
    """the bytes of a .aln file (alns2alnf_bin, align.c:345-382) from hits in parse_aln's form"""
    import struct
    b = bytearray()
    for ents in reads:
        b += struct.pack("<i", len(ents))
        for e in ents:
            b += struct.pack("<iQQiiiii", e["score"], e["L"], e["U"], e["mm"], e["gapo"], e["gape"], e["aln_length"], len(e["states"]))
            b += struct.pack(f"<{len(e['states'])}i", *e["states"])
    return bytes(b)


def check_synth(orc, idx, here=HERE):
    """the cases synth_hits exists for, asserted on the files (tests/test_map_host.py does the same on the committed ones); -> the hit lists"""
    import map_model
    import oracle_lib
    reads = oracle_lib.parse_aln(open(os.path.join(here, "synth_hits.aln"), "rb").read())
    n6, n3 = sam_records(os.path.join(here, "synth_hits_n6.sam.gz")), sam_records(os.path.join(here, "synth_hits_n3.sam.gz"))
    fq_lens = [len(ln) for ln in read_text(os.path.join(here, "synth_hits.fq.gz")).split("\n")[1::4]]
    assert len(reads) == len(n6) == len(n3) == len(fq_lens) and 350 <= len(reads) <= 450
    length, sa0 = int(idx.contents.length), int(idx.contents.sa0_index)
    ann = read_ann(os.path.join(here, "rep.fa.ann"))
    mapped = [(r, ents) for r, ents in enumerate(reads) if ents]
    assert 0 < len(reads) - len(mapped) and all((int(n6[r][1]) == 4) == (not ents) for r, ents in enumerate(reads))
    firsts = [ents[0] for _, ents in mapped]
    for r, ents in mapped:
        assert all(read_len(e) == fq_lens[r] and e["aln_length"] <= 255 and e["gapo"] == len(runs_of(e)) <= 8 for e in ents), r
    # read lengths around the words of the insertion map
    got_lens = {fq_lens[r] for r, _ in mapped}
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193, 250} <= got_lens and min(got_lens) <= 30
    assert max(e["aln_length"] for e in firsts) >= 250
    # gap runs of the first hits
    nruns = {len(runs_of(e)) for e in firsts}
    assert {0, 1, 2, 3, 5, 8} <= nruns
    assert any({st for _, _, st in runs_of(e)} == {I, D} for e in firsts)
    assert any(a[2] != b[2] and a[0] + a[1] == b[0] for e in firsts for a, b in zip(runs_of(e), runs_of(e)[1:]))  # I next to D
    for at in (False, True):  # the file's orientation and k_place's
        for bit in (64, 128, 192):
            assert any(s < bit < s + n and st == I for e in firsts for s, n, st in runs_of(e, at)), (at, bit)
            assert any(s < bit < s + n and st == D for e in firsts for s, n, st in runs_of(e, at)), (at, bit)
        assert any(s == 0 for e in firsts for s, n, st in runs_of(e, at))
        assert any(s + n == e["aln_length"] for e in firsts for s, n, st in runs_of(e, at))
        assert any(s <= 64 and s + n >= 128 and st == I for e in firsts for s, n, st in runs_of(e, at))  # a whole word of the map
    assert any(n == 1 for e in firsts for _, n, _ in runs_of(e)) and any(n >= 20 for e in firsts for _, n, _ in runs_of(e))
    assert sum(1 for e in firsts if len(runs_of(e)) == 8) >= 4
    # sums: what the model makes of them, and the MAPQ the REFERENCE printed
    want, _ = map_model.expected_places(orc, idx, reads, 6)
    w = lambda e: e["U"] - e["L"] + 1
    t = [(int(want["top1"][r]), int(want["top2"][r]), ents, int(n6[r][4]), int(n3[r][4])) for r, ents in mapped]
    import math
    for t2 in (1, 254, 255, 256):
        q = 23 - int(4.343 * math.log(min(t2, 255)) + 0.5)
        assert any(a == 1 and b == t2 and e[0]["mm"] not in (3, 6) and q6 == q3 == max(q, 0) for a, b, e, q6, q3 in t), t2
    assert any(a == 1 and b == 0 and e[0]["mm"] not in (3, 6) and q6 == q3 == 37 for a, b, e, q6, q3 in t)
    assert any(a == 1 and b > 10000 and e[0]["mm"] not in (3, 6) and q6 == q3 == 0 for a, b, e, q6, q3 in t)
    assert any(a == 1 and w(e[0]) == 2**32 + 1 and q6 == 37 for a, b, e, q6, q3 in t)       # top1 = 1 only through wrapping
    assert any(a == 0 and q6 == 23 for a, b, e, q6, q3 in t)                                  # top1 wrapped to 0 on a mapped read
    assert any(a < 0 for a, b, e, q6, q3 in t)
    assert any(a == 1 and b == 0 and sum(w(x) for x in e[1:] if x["score"] > e[0]["score"]) >= 2**32 and q6 == 37 for a, b, e, q6, q3 in t)
    assert any(b < 0 for a, b, e, q6, q3 in t)
    assert not any(b < 0 and (a == 1 or a < 0) for a, b, e, q6, q3 in t)                      # undefined in the reference
    assert any(any(x["score"] < e[0]["score"] for x in e[1:]) and a == sum(w(x) for x in e if x["score"] <= e[0]["score"]) > 1 for a, b, e, q6, q3 in t)
    assert {9, 17} <= {len(e) for a, b, e, q6, q3 in t}
    assert any(e[0]["score"] > 255 for a, b, e, q6, q3 in t) and any(x["score"] > 255 for a, b, e, q6, q3 in t for x in e[1:])
    assert any(a == 1 and b == 0 and e[0]["mm"] == 3 and (q6, q3) == (37, 25) for a, b, e, q6, q3 in t)
    assert any(a == 1 and b > 0 and e[0]["mm"] == 6 and q6 == 25 and q3 < 23 for a, b, e, q6, q3 in t)
    # first rows and their walks
    rows = {e["L"] for e in firsts}
    assert {sa0, sa0 - 1, sa0 + 1, length - 1} <= rows
    walks = {row: map_model.walk_rows(orc, idx, row) for row in rows}
    assert any(len(wk) == 1 for wk in walks.values()) and any(len(wk) == 32 for wk in walks.values())
    assert any(row % 32 == 1 for row in rows) and any(row % 32 == 31 for row in rows)
    assert any(sa0 in wk[1:-1] for wk in walks.values()) and any(len(wk) > 1 and wk[1] == sa0 for wk in walks.values())
    assert {0, 16} <= {int(n6[r][1]) for r, _ in mapped}
    for r, _ in mapped:  # inside an annotated sequence
        assert any(a <= int(want["pos"][r]) <= b for a, b in ann), r
    return reads


def main_synth():
    import oracle_lib
    orc = oracle_lib.load()
    idx = orc.load_index(os.path.join(HERE, "rep.fa.bwt"), load_sa=True)
    rng = random.Random(SYNTH_SEED)
    fq, reads, dropped = make_synth(rng, orc, idx, read_ann(os.path.join(HERE, "rep.fa.ann")))
    import tempfile
    fa, aln = os.path.join(HERE, "rep.fa"), os.path.join(HERE, "synth_hits.aln")
    open(aln, "wb").write(serialize_aln(reads))
    with tempfile.TemporaryDirectory() as tmp:
        fqp = os.path.join(tmp, "synth_hits.fq")
        open(fqp, "w").write(fq)
        run([REF_BIN, "aln2sam", fa, fqp, aln, os.path.join(tmp, "synth_hits_n6.sam")])
        run([REF_BIN, "aln2sam", "-n", "3", fa, fqp, aln, os.path.join(tmp, "synth_hits_n3.sam")])
        for name in SYNTH_TEXT:
            with open(os.path.join(HERE, name + ".gz"), "wb") as f:
                f.write(gzip.compress(open(os.path.join(tmp, name), "rb").read(), 9, mtime=0))
    check_synth(orc, idx)
    print(f"synth_hits: {len(reads)} reads, {sum(1 for e in reads if e)} with hits, {dropped} left out ({100 * dropped / len(reads):.1f} %)")


def main():
    if not os.path.exists(REF_BIN):
        sys.exit("oracle/_ref/bwbble is missing: the fixtures can only be regenerated where the reference is present (make -C oracle ref)")
    rng = random.Random(20261016)
    recs, text, where, split = make_genome(rng)
    fa, fq = os.path.join(HERE, "rep.fa"), os.path.join(HERE, "rep.fq")
    with open(fa, "w") as f:
        for name, seq in recs:
            f.write(f">{name}\n")
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
    open(fq, "w").write(make_reads(rng, text, where, split))
    run([REF_BIN, "index", fa])
    os.remove(fa + ".ref")
    aln = os.path.join(HERE, "rep_n3.aln")
    if os.path.exists(aln):
        os.remove(aln)
    run([REF_BIN, "align", "-n", "3", fa, fq, aln])
    run([REF_BIN, "aln2sam", fa, fq, aln, os.path.join(HERE, "rep_n3.sam")])
    run([REF_BIN, "aln2sam", "-n", "3", fa, fq, aln, os.path.join(HERE, "rep_n3_q3.sam")])
    mq = check()
    from collections import Counter
    print("flag / MAPQ counts:", sorted(Counter(mq).items()))
    main_synth()


if __name__ == "__main__":
    main()
