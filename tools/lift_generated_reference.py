#!/usr/bin/env python3
"""Where the REFERENCE's own `index` + `align -n 3` + `aln2sam` place the reads of the generated multi-genome of tests/lift_model.py, on the
CPU: the check behind the condition of tests/test_gpu_lift.py that no error-free read is left undecided - every one must lie where it was cut
from its bubble record or, a read inside one flank, on the chromosome's copy of it -, once with the generator as the tests use it (two-base
IUPAC codes in the flanks) and once with three-base codes as well, which is why the generator does not write those.
usage: tools/lift_generated_reference.py <a bwbble binary built from the reference> [work directory]"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import lift_model  # noqa: E402


def census(ref, work, code_bases):
    g = lift_model.genome(code_bases=code_bases)
    reads = lift_model.reads(g)
    fa, fq, aln, sam = (os.path.join(work, n) for n in ("gen.fa", "gen.fq", "gen.aln", "gen.sam"))
    open(fa, "w").write(g["fasta"])
    open(fq, "w").write(lift_model.fastq(reads))
    for f in (aln, sam):
        if os.path.exists(f):
            os.remove(f)
    for cmd in (["index", fa], ["align", "-n", "3", fa, fq, aln], ["aln2sam", fa, fq, aln, sam]):
        subprocess.run([ref] + cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    lines = [ln.rstrip("\n").split("\t") for ln in open(sam) if ln[0] != "@"]
    assert len(lines) == len(reads)
    out = {"error-free reads": 0, "on their bubble record": 0, "on the chromosome's copy of the flank": 0, "undecided": 0, "of them unmapped": 0, "reads with an edit": 0, "of them unmapped ": 0}
    for f, (name, k, o, ln, strand, edit, seq, cig) in zip(lines, reads):
        if edit is not None:
            out["reads with an edit"] += 1
            out["of them unmapped "] += f[1] == "4"
            continue
        out["error-free reads"] += 1
        want = lift_model.judge(g["records"][k][2], o + 1, cig)
        on_bubble = f[2] == g["records"][k][0] and int(f[3]) == o + 1 and f[5] == f"{ln}M"
        on_chrom = want[1] == f"{ln}M" and f[2] == g["names"][0] and int(f[3]) == want[0] and f[5] == f"{ln}M"
        out["on their bubble record"] += on_bubble
        out["on the chromosome's copy of the flank"] += on_chrom and not on_bubble
        out["undecided"] += not (on_bubble or on_chrom)
        out["of them unmapped"] += f[1] == "4"
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        work = sys.argv[2] if len(sys.argv) > 2 else tmp
        os.makedirs(work, exist_ok=True)
        for what, code_bases in (("two-base codes (the tests' generator)", (2,)), ("two- and three-base codes", (2, 3))):
            print(what + ":", "  ".join(f"{k.strip()} {v}" for k, v in census(sys.argv[1], work, code_bases).items()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
