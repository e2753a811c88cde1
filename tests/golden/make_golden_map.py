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
"""
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
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


def sam_records(path):
    return [ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("@")]


def check(here=HERE):
    """the outcomes the fixture exists for (also asserted by tests/test_map_host.py on the committed files)"""
    d, q3 = sam_records(os.path.join(here, "rep_n3.sam")), sam_records(os.path.join(here, "rep_n3_q3.sam"))
    mq = [(int(r[1]), int(r[4])) for r in d]
    assert any(f != 4 and q == 0 for f, q in mq), "no MAPQ 0 on a mapped read"
    assert any(q == 23 for _, q in mq) and any(0 < q < 23 for _, q in mq) and any(q == 37 for _, q in mq)
    assert any(int(r[4]) == 25 for r in q3)
    assert {0, 16} <= {f for f, _ in mq}
    return mq


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


if __name__ == "__main__":
    main()
