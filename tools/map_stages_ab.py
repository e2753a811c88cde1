#!/usr/bin/env python3
"""`bwbble map` with every result-stream stage (-X 5 -B -J -R -D -A -I -G) on the 3.3 M-character fixture of tests/mid_model.py, this tree's build
against another build's - the parent commit's -, alternating, two runs each: the log lines of the stages with their counts, the kernel times each
line reports, and the bytes of the SAM and the three tables.  With `trace`: one more run per build under rocprofv3 --kernel-trace --stats, and the
kernel call counts by name compared.  With `q`: -b 20 -Y on the command line too (the fixture's reads carry quality lines), and the log line of
k_pile_q among the stage lines.  The fixture (genome, index, .ref, bubble table, reads: the CPU half of mid_model.build) is made in <dir>
unless it is there already, so it can be prepared on a machine without a GPU.
usage: tools/map_stages_ab.py <dir> prepare
       tools/map_stages_ab.py <dir> <the other build's bwbble_amd/bin> [q] [trace]  (profiles/stage_fold.txt, profiles/pile_fold.txt: one run's output each)"""
import csv
import glob
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bwbble_amd as bw
import mid_model

STAGES = ("placements on the GPU", "other placements on the GPU", "placements joined by locus", "placements lifted", "NM and MD", "allele counts at", "read support per indel bubble on",
          "genotype calls on the GPU")
STAGE_Q = "base qualities in the counts on the GPU (k_pile_q)"
TIME = re.compile(r"\b(kernels?|k_pile|k_indel) (\d+\.\d+) ms")


def prepare(d):
    fa, fq, data = (os.path.join(d, n) for n in ("g.fa", "g.fq", "g.data"))
    if not os.path.exists(fq + ".ok"):
        os.makedirs(d, exist_ok=True)
        subprocess.run([bw.SYNTH_BIN, "genome", fa] + mid_model.GENOME, check=True)
        for tool in ("index", "fasta2ref"):
            subprocess.run([bw.HOST_BIN, tool, fa], check=True, stdout=subprocess.DEVNULL)
        names, start, end = bw.read_ann(fa + ".ann")
        open(data, "w").write(mid_model.bubble_table(names, start, end))
        subprocess.run([bw.SYNTH_BIN, "reads", fa, fq] + mid_model.SYNTH_READS, check=True)
        with open(fq, "a") as f:
            f.write("".join(f"@{name}\n{seq}\n+\n{'2' * len(seq)}\n" for name, seq in mid_model.reads(mid_model.fasta_records(open(fa).read()))))
        open(fq + ".ok", "w").write("ok\n")
    return fa, fq, data


def digest(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    d = os.path.abspath(sys.argv[1])
    fa, fq, data = prepare(d)
    if sys.argv[2] == "prepare":
        return 0
    out = {e: os.path.join(d, "out." + e) for e in ("sam", "a.tsv", "i.tsv", "g.tsv")}
    args = ["map"] + mid_model.ALIGN + ["-X", "5", "-B", data, "-J", "-R", "-D", "-A", out["a.tsv"], "-a", str(mid_model.MIN_MAPQ), "-I", out["i.tsv"], "-w", str(mid_model.ANCHOR),
                                        "-G", out["g.tsv"], fa, fq, out["sam"]]
    opts = sys.argv[3:]
    stages = STAGES
    if "q" in opts:
        args[1:1] = ["-b", "20", "-Y"]
        stages += (STAGE_Q,)
    builds = {"parent": os.path.join(sys.argv[2], "bwbble"), "this": bw.HOST_BIN}
    counts, files, times = {}, {}, {}
    for run in range(2):
        for name, exe in builds.items():
            r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if r.returncode != 0:
                print(name, "FAILED", r.returncode, r.stdout[-2000:])
                return 1
            lines = [ln for ln in r.stdout.split("\n") if ln.startswith(stages)]
            print(f"--- {name}, run {run + 1}: {len(lines)} of {len(stages)} stage lines")
            print("\n".join(lines))
            counts.setdefault(name, set()).add("\n".join(re.sub(r"\d+\.\d+", "#", ln) for ln in lines))  # (every figure that is not a time or a rate is an integer)
            files.setdefault(name, set()).add(" ".join(f"{e} {os.path.getsize(p)} bytes {digest(p)}" for e, p in out.items()))
            for ln in lines:
                times.setdefault(ln[:24], {}).setdefault(name, []).append(sum(float(m[1]) for m in TIME.findall(ln)))
    print("every count of the log lines equal, across runs and builds:", len(counts["this"] | counts["parent"]) == 1)
    print("the SAM and the three tables identical, across runs and builds:", len(files["this"] | files["parent"]) == 1, " ", next(iter(files["this"])))
    for stage, t in times.items():
        lo, hi = min(t["parent"]), max(t["parent"])
        print(f"{stage:24s} kernel ms  parent {t['parent'][0]:.3f} {t['parent'][1]:.3f}  this {t['this'][0]:.3f} {t['this'][1]:.3f}  "
              f"{'within' if all(lo <= v <= hi for v in t['this']) else 'OUTSIDE'} the parent's spread")
    if "trace" in opts:
        calls = {}
        for name, exe in builds.items():
            td = os.path.join(d, "trace_" + name)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "run", "--", exe] + args, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT,
                           check=True, timeout=600)
            (stats,) = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
            calls[name] = {row["Name"]: int(row["Calls"]) for row in csv.DictReader(open(stats))}
        print("kernel calls by name under rocprofv3 --kernel-trace --stats equal:", calls["this"] == calls["parent"])
        print("  ".join(f"{k.split('(')[0]} {v}" for k, v in sorted(calls["this"].items())))
        if calls["this"] != calls["parent"]:
            print("parent:", "  ".join(f"{k.split('(')[0]} {v}" for k, v in sorted(calls["parent"].items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
