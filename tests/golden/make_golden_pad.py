#!/usr/bin/env python3
"""Regenerates the fixtures of `bwbble sampad` / `map -B` / `aln2sam -B` (bubble hits in reference coordinates: the tags bC:Z: / bP:Z:)
from the REAL reference - run where the reference is built, like make_golden_map.py.  The judge of every expected byte is the reference's
own sam_pad: this script compiles mg-ref/sam_pad.cpp with g++ into a temporary directory (nothing of it is kept) and uses
oracle/_ref/bwbble for align / aln2sam like the other make_golden*.py.  Only data lands in tests/golden:

  pad_toy.data            bubble.data for the four bubbles of toy.fa, derived from their headers `>bubbleK chrN p` and the generator's shape
                          (bwbble_amd/tools/bwb_synth.c: 124 characters before 0-based position p of the chromosome, 1-5 inserted bases, 124
                          characters from p on): the chromosome's full header, then `p-123  124  p+1  123  0  ins`
  pad_bub.fq.gz           reads cut from the four bubble records (IUPAC codes resolved to one of their bases), 100 and 60 bases long, at every
                          third offset plus every offset from 121 to 124 + ins + 2, every second one reverse-complemented; and 60 plain
                          100-base reads from chr1-3
  pad_bub_n3.aln.gz       the reference's `align -n 3` on them,
  pad_bub_n3.sam.gz       its `aln2sam`,
  pad_bub_n3.pad.sam.gz   and its `sam_pad` with pad_toy.data
  pad_synth.data          a hand-built table and SAM file that hold what the aligner never produces - alt_len 0 with ref_len 0 / 1 / 5,
  pad_synth.sam           B_minus_A 0, D_minus_C -1, A and C above 2^32, a header with spaces; for every bubble POS at 0, 1, B, B + 1, B + alt,
  pad_synth.pad.sam       B + alt + 1, B + alt + D + 1, B + alt + D + 2 and far beyond; the names `bubble`, `bubbles1 q`, `mybubble1`, `*`;
                          bubble names with and without trailing words; a line with X0 / X1 / XA tags; a last line without a newline -
                          and what the reference's sam_pad makes of them

check() asserts that the aligned fixture reaches every branch of the rule on both strands (tests/test_pad_host.py asserts the same on the
committed files).  The gzip members carry a zero time stamp, so that a rerun gives the same bytes.
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bwbble")

from golden.make_golden import REF_SRC  # noqa: E402  (mg-aligner of the reference; mg-ref lies next to it)
import pad_model  # noqa: E402

SEED = 20261019
FLANK = 124
IUPAC = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = str.maketrans("ACGT", "TGCA")


def run(cmd):
    print("+", " ".join(cmd))
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)


def put_gz(path, data):
    with open(path, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
        g.write(data)


def fasta_records(path):
    recs = []
    for ln in open(path).read().split("\n"):
        if ln.startswith(">"):
            recs.append([ln[1:], []])
        elif ln:
            recs[-1][1].append(ln)
    return [(h, "".join(parts)) for h, parts in recs]


def toy_table(recs):
    """bubble.data text for the bubble records of toy.fa, and the inserted length of every bubble"""
    chrom = {h.split()[0]: h for h, _ in recs if not h.startswith("bubble")}
    lines, ins_of = [], []
    for h, seq in recs:
        if not h.startswith("bubble"):
            continue
        name, ch, p = h.split()
        assert int(name[6:]) == len(ins_of)
        p, ins = int(p), len(seq) - 2 * FLANK
        assert 1 <= ins <= 5
        lines += [chrom[ch], f"{p - FLANK + 1}\t{FLANK}\t{p + 1}\t{FLANK - 1}\t0\t{ins}"]
        ins_of.append(ins)
    return "\n".join(lines) + "\n", ins_of


def make_reads(rng, recs, ins_of):
    resolve = lambda s: "".join(c if c in "ACGT" else rng.choice(IUPAC[c.upper()]) for c in s)
    out = []
    bubbles = [(h, seq) for h, seq in recs if h.startswith("bubble")]
    for (h, seq), ins in zip(bubbles, ins_of):
        for ln in (100, 60):
            offs = sorted(set(range(0, len(seq) - ln + 1, 3)) | {o for o in range(FLANK - 3, FLANK + ins + 3) if o <= len(seq) - ln})
            for o in offs:
                read = resolve(seq[o:o + ln])
                strand = len(out) % 2
                if strand:
                    read = read[::-1].translate(COMP)
                qual = "".join(rng.choice("ABCDEFGHIJ0123456789") for _ in range(ln))
                out.append(f"@{h.split()[0]}_o{o}_l{ln}_{'-' if strand else '+'}\n{read}\n+\n{qual}\n")
    plain = [(h, seq) for h, seq in recs if not h.startswith("bubble")]
    for k in range(60):
        h, seq = plain[k % len(plain)]
        o = rng.randrange(0, len(seq) - 100)
        read = resolve(seq[o:o + 100])
        if k % 2:
            read = read[::-1].translate(COMP)
        out.append(f"@{h.split()[0]}_o{o}_plain{k}\n{read}\n+\n{'5' * 100}\n")
    return "".join(out)


# (ann, A, B_minus_A, C, D_minus_C, ref_len, alt_len)
SYNTH_BUBBLES = [
    ("chrS synthetic seed=1 with spaces", 100, 10, 111, 10, 0, 3),      # an insertion
    ("chrD", 1000, 20, 1025, 20, 5, 0),                                 # alt_len 0, ref_len 5: a deletion
    ("chrM mixed", 5000, 124, 5125, 123, 1, 2),
    ("chrZ", 1, 0, 1, 5, 0, 4),                                         # B_minus_A 0: at the head of the chromosome
    ("chrE tail", 200, 7, 207, -1, 0, 2),                               # D_minus_C -1: at its end
    ("chrBig", 2**32 + 17, 124, 2**32 + 17 + 124 + 3, 123, 3, 0),       # A and C above 2^32
    ("chrBig", 2**35 + 5, 3, 2**35 + 8, 2, 0, 0),                       # alt_len 0, ref_len 0
    ("chrO one", 300, 5, 306, 4, 1, 0),                                 # alt_len 0, ref_len 1
]


def make_synth():
    data = "".join(f"{b[0]}\n{b[1]}\t{b[2]}\t{b[3]}\t{b[4]}\t{b[5]}\t{b[6]}\n" for b in SYNTH_BUBBLES)
    lines = ["@SQ\tSN:chrS synthetic seed=1 with spaces\tLN:1000", "@SQ\tSN:bubble0 chrS 101\tLN:23", "@PG\tID:bwbble\tPN:bwbble\tVN:0.1-r01"]
    seq, qual = "ACGTACGTAC", "IIIIIIIIII"
    n = 0

    def rec(rname, pos, extra=""):
        nonlocal n
        lines.append(f"s{n}\t{16 if n % 2 else 0}\t{rname}\t{pos}\t37\t10M\t*\t0\t0\t{seq}\t{qual}{extra}")
        n += 1

    for k, (_, A, B, C, D, ref_len, alt_len) in enumerate(SYNTH_BUBBLES):
        for i, pos in enumerate((0, 1, B, B + 1, B + alt_len, B + alt_len + 1, B + alt_len + D + 1, B + alt_len + D + 2, 1000000)):
            rec(f"bubble{k}" if i % 2 else f"bubble{k} chr{k} {A}", pos)
    rec("bubble0", -1)
    rec("bubble", 3)            # no number: bubble 0
    rec("bubbles1 q", 12)       # atoll("s1") == 0: bubble 0
    rec("bubble+2", 125)        # atoll("+2") == 2
    rec("bubble07 x", 2)        # leading zero: bubble 7
    rec("mybubble1", 5)
    rec("chrS synthetic seed=1 with spaces", 77)
    lines.append(f"u{n}\t4\t*\t0\t0\t*\t*\t0\t0\t{seq}\t{qual}")
    rec("bubble2 chr2 5000", 126, "\tX0:i:1\tX1:i:2\tXA:Z:bubble1 chr1 1000,+21,10M,0;chrD,-1030,10M,1;")
    rec("bubble4", 9)           # the last line: no newline after it
    return data, "\n".join(lines)


def check(here=HERE):
    """the branches the aligned fixture exists for, on both strands"""
    bubbles = pad_model.load_bubbles(os.path.join(here, "pad_toy.data"))
    census = pad_model.classify(pad_model.read_bytes(os.path.join(here, "pad_bub_n3.pad.sam.gz")), bubbles)
    for case in ("left", "right", "range"):
        for strand in ("fwd", "rev"):
            assert census.get((case, strand), 0) >= 8, (case, strand, census)
    assert census.get(("plain", None), 0) >= 50 and census.get(("unmapped", None), 0) >= 1, census
    return census


def main():
    if not os.path.isdir(REF_SRC) or not os.path.exists(REF_BIN):
        sys.exit("the reference is not built here (oracle/_ref): these fixtures can only be regenerated where it is")
    tmp = tempfile.mkdtemp(prefix="bwb_pad_")
    sam_pad = os.path.join(tmp, "sam_pad")
    run(["g++", "-O2", "-w", "-o", sam_pad, os.path.join(os.path.dirname(REF_SRC.rstrip("/")), "mg-ref", "sam_pad.cpp")])

    recs = fasta_records(os.path.join(HERE, "toy.fa"))
    data, ins_of = toy_table(recs)
    open(os.path.join(HERE, "pad_toy.data"), "w").write(data)
    fq = make_reads(random.Random(SEED), recs, ins_of)
    fqp, aln, sam, pad = (os.path.join(tmp, n) for n in ("pad_bub.fq", "pad_bub_n3.aln", "pad_bub_n3.sam", "pad_bub_n3.pad.sam"))
    open(fqp, "w").write(fq)
    fa = os.path.join(HERE, "toy.fa")
    run([REF_BIN, "align", "-n", "3", fa, fqp, aln])
    run([REF_BIN, "aln2sam", fa, fqp, aln, sam])
    run([sam_pad, os.path.join(HERE, "pad_toy.data"), sam, pad])
    for p in (fqp, aln, sam, pad):
        put_gz(os.path.join(HERE, os.path.basename(p) + ".gz"), open(p, "rb").read())

    sdata, ssam = make_synth()
    open(os.path.join(HERE, "pad_synth.data"), "w").write(sdata)
    open(os.path.join(HERE, "pad_synth.sam"), "w").write(ssam)
    run([sam_pad, os.path.join(HERE, "pad_synth.data"), os.path.join(HERE, "pad_synth.sam"), os.path.join(HERE, "pad_synth.pad.sam")])
    print(fq.count("\n") // 4, "reads;", check())


if __name__ == "__main__":
    main()
