#!/usr/bin/env python3
"""Regenerates tests/golden/params_*.aln[.gz] from the REAL reference (run in the build container only): the reference's own
align_reads_inexact with max_best and no_indel_length away from their defaults.

`bwbble align` has no flag for either field (main.c:100-117), so the reference binary cannot produce these: a throw-away harness
(written to a temp dir, never committed) is linked with the reference's own object files (oracle/_ref/obj, all but main.o).  It loads the
index, parses the FASTQ with fastq2reads, sets the two fields and -n / -o / -e on a defaulted aln_params_t and calls the serial
align_reads_inexact (n_threads = 1).  Inputs are fixtures already here (rep.fa, toy.fa; rep.fq, rep_gap.fq, gapo.fq, toy.fq).

Only DATA lands in tests/golden/: the .aln bytes the reference wrote.  tests/test_oracle_golden_params.py holds the oracle to them.
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = "/root/reference/mg-aligner"
REF_OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")

# name: (FASTA, FASTQ, `align` flags, fields without a flag, gzip the output)
CONFIGS = {
    # max_best: the search ends at the first hit above the best score once more than max_best best hits are known
    # (inexact_match.c:339-340, 353-354).  rep.fa is repeat-rich: 40 / 20 records of rep.fq differ from rep_n3.aln at 0 / 1, none at 3
    "rep_mb0": ("rep.fa", "rep.fq", ["-n", "3"], dict(max_best=0), False),
    "rep_mb1": ("rep.fa", "rep.fq", ["-n", "3"], dict(max_best=1), False),
    "rep_mb3": ("rep.fa", "rep.fq", ["-n", "3"], dict(max_best=3), False),
    # (the flags of rep_gap_n4.aln, the default-valued run of the same reads: 28 / 28 / 16 / 4 of its 40 records differ at -1 / 0 / 1 / 3)
    "repgap_mbneg": ("rep.fa", "rep_gap.fq", ["-n", "4", "-o", "1"], dict(max_best=-1), False),
    "repgap_mb0": ("rep.fa", "rep_gap.fq", ["-n", "4", "-o", "1"], dict(max_best=0), False),
    "repgap_mb1": ("rep.fa", "rep_gap.fq", ["-n", "4", "-o", "1"], dict(max_best=1), False),
    "repgap_mb3": ("rep.fa", "rep_gap.fq", ["-n", "4", "-o", "1"], dict(max_best=3), False),
    # no_indel_length: no gap is opened or extended closer than this (+ the gaps so far) to either end of the read (:423-425).
    # toy.fq has reads whose gapped hits come and go with it (17, 16, 16, 15, 14, 12 gapped hits at -2, 0, 2, 3, the default 5, 12); a record
    # changes between -2 and 0, between 2 and 3, and between 3 and 12 (0, 1 and 2 give the same bytes).  Larger than the other fixtures: gzipped
    "toy_nilneg": ("toy.fa", "toy.fq", ["-n", "3"], dict(no_indel_length=-2), True),
    "toy_nil0": ("toy.fa", "toy.fq", ["-n", "3"], dict(no_indel_length=0), True),
    "toy_nil2": ("toy.fa", "toy.fq", ["-n", "3"], dict(no_indel_length=2), True),
    "toy_nil3": ("toy.fa", "toy.fq", ["-n", "3"], dict(no_indel_length=3), True),
    "toy_nil12": ("toy.fa", "toy.fq", ["-n", "3"], dict(no_indel_length=12), True),
    # two gap opens, three extensions: the bound grows with the gaps so far, and a record changes at every step from -2 to 3
    "toy_o2e3_nilneg": ("toy.fa", "toy.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(no_indel_length=-2), True),
    "toy_o2e3_nil0": ("toy.fa", "toy.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(no_indel_length=0), True),
    "toy_o2e3_nil1": ("toy.fa", "toy.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(no_indel_length=1), True),
    "toy_o2e3_nil2": ("toy.fa", "toy.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(no_indel_length=2), True),
    "toy_o2e3_nil3": ("toy.fa", "toy.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(no_indel_length=3), True),
    "toy_o2e3_mb0_nil2": ("toy.fa", "toy.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(max_best=0, no_indel_length=2), True),
    # reads with 2 .. 6 indels (the flags of gapo_o5.aln, the default-valued run): 2 / 5 of its records differ at 8 / 12
    "gapo_o5e2_nil8": ("toy.fa", "gapo.fq", ["-n", "5", "-o", "5", "-e", "2"], dict(no_indel_length=8), False),
    "gapo_o5e2_nil12": ("toy.fa", "gapo.fq", ["-n", "5", "-o", "5", "-e", "2"], dict(no_indel_length=12), False),
    # past half a read: no indel anywhere, no gapped hit left
    "gapo_o2e3_nil60": ("toy.fa", "gapo.fq", ["-n", "4", "-o", "2", "-e", "3"], dict(no_indel_length=60), False),
    "repgap_nil60": ("rep.fa", "rep_gap.fq", ["-n", "4", "-o", "1"], dict(no_indel_length=60), False),
}


def fixture_path(name):
    return os.path.join(HERE, f"params_{name}.aln" + (".gz" if CONFIGS[name][4] else ""))


def fixture_bytes(name):
    path = fixture_path(name)
    return gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()


HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bwt.h"
#include "align.h"
#include "inexact_match.h"
#include "io.h"
/* params_harness <bwt> <fastq> <out.aln> <max_diff> <max_gapo> <max_gape> <max_best> <no_indel_length> */
int main(int argc, char** argv) {
	if (argc != 9) return 2;
	aln_params_t p;
	memset(&p, 0, sizeof p);
	set_default_aln_params(&p);
	p.max_diff = atoi(argv[4]);
	if (strcmp(argv[5], "-")) p.max_gapo = atoi(argv[5]);
	if (strcmp(argv[6], "-")) p.max_gape = atoi(argv[6]);
	p.max_best = atoi(argv[7]);
	p.no_indel_length = atoi(argv[8]);
	p.n_threads = 1;
	bwt_t* BWT = load_bwt(argv[1], 0);
	reads_t* reads = fastq2reads(argv[2]);
	remove(argv[3]); /* (the reference appends) */
	return align_reads_inexact(BWT, reads, NULL, &p, argv[3]);
}
"""

DEFAULTS = dict(max_best=30, no_indel_length=5)


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit("reference sources not present; golden vectors can only be regenerated in the build container")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, stdout=subprocess.DEVNULL)
    tmp = tempfile.mkdtemp(prefix="bwb_golden_params_")
    hsrc, hbin = os.path.join(tmp, "params_harness.c"), os.path.join(tmp, "params_harness")
    open(hsrc, "w").write(HARNESS)
    objs = sorted(os.path.join(REF_OBJ, o) for o in os.listdir(REF_OBJ) if o.endswith(".o") and o != "main.o")
    subprocess.run(["gcc", "-w", "-O2", "-std=gnu99", "-fopenmp", "-I", REF_SRC, hsrc] + objs + ["-o", hbin, "-lm", "-lz", "-lpthread"], check=True)
    for name, (fa, fq, flags, fields, gz) in CONFIGS.items():
        f = dict(zip(flags[::2], flags[1::2]))
        assert set(f) <= {"-n", "-o", "-e"} and set(fields) <= set(DEFAULTS)
        v = dict(DEFAULTS, **fields)
        out = os.path.join(tmp, name + ".aln")
        cmd = [hbin, os.path.join(HERE, fa + ".bwt"), os.path.join(HERE, fq), out, f["-n"], f.get("-o", "-"), f.get("-e", "-"),
               str(v["max_best"]), str(v["no_indel_length"])]
        print("+", " ".join(cmd))
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        data = open(out, "rb").read()
        if gz:
            with open(fixture_path(name), "wb") as fh, gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as z:
                z.write(data)
        else:
            open(fixture_path(name), "wb").write(data)
    print("golden parameter vectors written to", HERE)


if __name__ == "__main__":
    main()
