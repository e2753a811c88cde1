#!/usr/bin/env python3
"""Regenerates the fixtures that pin the oracle to the REAL reference on a text dense in IUPAC codes (tests/ovf_model.py:
golden_fixture) - run where the reference is built (make -C oracle ref).  Lists of 15 625 SA intervals in calculate_d, reads with more
than a thousand hits, reads whose placement needs two gap opens: input of a kind the other golden files do not hold.  Only data lands in tests/golden, gzipped with a zero time
stamp so that a second run writes the same bytes:

  ovf.fa.gz            the FASTA (ordinary record, the two de Bruijn records, the families f330 and f1300) - our data
  ovf.fq.gz            the reads (ovf_model.golden_reads: the fixture's, and GAPPED) - our data
  ovf.fa.bwt.gz        what the reference's `index` writes for it
  ovf.fa.ann
  ovf_<config>.aln.gz  the reference's `align` (-t 1) with CONFIGS[config]
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bwbble")

CONFIGS = {"n0": ["-n", "0"], "n2": ["-n", "2"], "n3gap": ["-n", "3", "-o", "2", "-e", "3"]}
FILES = ["ovf.fa.gz", "ovf.fq.gz", "ovf.fa.bwt.gz", "ovf.fa.ann"] + [f"ovf_{c}.aln.gz" for c in sorted(CONFIGS)]


def texts():
    """(FASTA text, FASTQ text) of the fixture"""
    import ovf_model
    fx = ovf_model.golden_fixture()
    reads = ovf_model.golden_reads(fx)
    return fx.fasta(), "".join(f"@{n}\n{s}\n+\n{'I' * len(s)}\n" for n, s in reads.items())


def unpack(dst, here=HERE):
    """writes ovf.fa, ovf.fq, ovf.fa.bwt and ovf.fa.ann out into dst (the tools read plain files) -> the FASTA's path"""
    for name in ("ovf.fa", "ovf.fq", "ovf.fa.bwt"):
        with open(os.path.join(str(dst), name), "wb") as f:
            f.write(gzip.open(os.path.join(here, name + ".gz"), "rb").read())
    shutil.copy(os.path.join(here, "ovf.fa.ann"), os.path.join(str(dst), "ovf.fa.ann"))
    return os.path.join(str(dst), "ovf.fa")


def put_gz(path, data):
    with open(path, "wb") as f:
        f.write(gzip.compress(data, 9, mtime=0))


def main(out=HERE):
    if not os.path.exists(REF_BIN):
        sys.exit("oracle/_ref is missing: the fixtures can only be regenerated where the reference is present (make -C oracle ref)")
    fa_text, fq_text = texts()
    with tempfile.TemporaryDirectory() as tmp:
        fa, fq = os.path.join(tmp, "ovf.fa"), os.path.join(tmp, "ovf.fq")
        open(fa, "w").write(fa_text)
        open(fq, "w").write(fq_text)
        subprocess.run([REF_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
        put_gz(os.path.join(out, "ovf.fa.gz"), fa_text.encode())
        put_gz(os.path.join(out, "ovf.fq.gz"), fq_text.encode())
        put_gz(os.path.join(out, "ovf.fa.bwt.gz"), open(fa + ".bwt", "rb").read())
        shutil.copy(fa + ".ann", os.path.join(out, "ovf.fa.ann"))
        for name, flags in sorted(CONFIGS.items()):
            aln = os.path.join(tmp, name + ".aln")
            subprocess.run([REF_BIN, "align", "-t", "1"] + flags + [fa, fq, aln], check=True, stdout=subprocess.DEVNULL)
            put_gz(os.path.join(out, f"ovf_{name}.aln.gz"), open(aln, "rb").read())
    for name in FILES:
        print(f"{name}: {os.path.getsize(os.path.join(out, name))} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
