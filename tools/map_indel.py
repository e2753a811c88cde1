#!/usr/bin/env python3
"""What `map -I` costs: indel_begin (the host's sort of the eligible bubbles, the upload of the table and the zeroed counters) and k_indel beside
k_pile, k_locus and k_place on one 2.5 M-read slot of the GRCh37-scale index of bench.py (the stats of the same calls), plain and with the joined
MAPQ of `-X 5 -B -J`; the reads counted, the adds and the candidates examined; the eligible bubbles at an anchor of 1 and the table's bytes; the
read-back of the counters; and the wall time of this tree's plain `map -n 3` against another build's - the parent commit's - on the same reads,
three runs each, alternating, with the SAM bytes compared; then `map -n 3 -B t -I` and `map -X 5 -B -J -I` once each (their log lines carry the
host sort's and the writer's time).  The input is that of tools/map_pile.py.
usage: tools/map_indel.py <the other build's bwbble_amd/bin> [output file]     (profiles/map_indel.txt is to be one run's output)"""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench
import bwbble_amd as bw

OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.getcwd(), "map_indel.txt")
N_READS = 2_500_000
ANCHOR = 1


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    a = bench.parse_args([])
    t0 = time.time()
    fa = bench.build_genome(a, bw)
    say(f"index ready in {time.time() - t0:.0f} s: {os.path.basename(fa)}")
    fq = os.path.join(a.workdir, f"pad_measure_{N_READS}.fq")
    if not os.path.exists(fq + ".ok"):
        subprocess.run([bw.SYNTH_BIN, "reads", fa, fq, str(N_READS), "100", "777", "1.0", "0.1", "0.0"], check=True)
        open(fq + ".ok", "w").write("ok\n")
    names, start, end = bw.read_ann(fa + ".ann")
    data = os.path.join(a.workdir, "pad_measure.data")
    header = {n.split()[0]: n for n in names if not n.startswith("bubble")}
    with open(data, "w") as f:
        for n, s, e in zip(names, start, end):
            if n.startswith("bubble"):
                _, ch, p = n.split()
                p, ins = int(p), int(e - s) + 1 - 248
                f.write(f"{header[ch]}\n{p - 123}\t124\t{p + 1}\t123\t0\t{ins}\n")
    anns, recs = bw.read_bubble_data(data)
    bub_of = bw.bubble_of(names, len(recs))
    chrom = bw.bubble_chrom_of(names, anns)
    say(f"records {len(names)}  bubbles {len(recs)}")

    seqs, lens = bw.load_fastq_codes(fq)
    b = bw.BwtFile(fa + ".bwt", load_sa=True)
    ctx = bw.Context(b)
    ctx.set_sa(b.SA)
    ctx.set_loci(start, end, bub_of, recs)
    ctx.set_bubble_chrom(chrom)
    have_text = os.path.exists(fa + ".ref")  # (k_pile on the same records for comparison, where `bwbble fasta2ref` has left the text)
    if have_text:
        ctx.set_text(bw.read_ref(fa))
        ctx.pile_begin()
    begins = []
    for _ in range(3):
        t0 = time.time()
        n_elig = ctx.indel_begin(ANCHOR)
        begins.append(round(time.time() - t0, 3))
    say(json.dumps({"anchor": ANCHOR, "bubbles": int(len(recs)), "eligible": int(n_elig), "indel_begin_s (sort, upload, memset)": begins,
                    "table_bytes": int(n_elig) * 16 + int(len(recs)), "counter_bytes": int(len(recs)) * 16}))
    out = {"reads": int(len(lens))}
    for key, joined in (("plain", False), ("joined", True)):
        t0 = time.time()
        ctx.align(bw.params(["-n", "3"]), seqs, lens)  # (a submission is counted once: one batch per form)
        t_align = time.time() - t0
        ctx.indel_reset()
        ctx.locus(6)
        _, lms = ctx.locus_stats()
        if joined:
            ctx.join(6, 5)
        _, _, pms = ctx.place_stats()
        kms = None
        if have_text:
            ctx.pile_reset()
            ctx.batch_pile(6, 5, False, joined, 0)
            kms = round(ctx.pile_stats()[2], 3)
        counted = ctx.batch_indel(6, 5, joined, 0)
        n_reads, n_adds, n_cand, ms = ctx.indel_stats()
        t0 = time.time()
        table = ctx.indel_counts(0, len(recs))
        t_fetch = time.time() - t0
        assert counted == n_reads and int(table.sum(dtype=np.uint64)) == n_adds, (counted, n_reads, n_adds)
        out[key] = {"align_s": round(t_align, 1), "k_place_ms": round(pms, 3), "k_locus_ms": round(lms, 3), "k_pile_ms": kms, "k_indel_ms": round(ms, 3), "reads_counted": int(n_reads),
                    "adds": int(n_adds), "candidates": int(n_cand), "bubbles_with_a_count": int(table.any(axis=1).sum()), "columns": [int(v) for v in table.sum(axis=0, dtype=np.uint64)],
                    "read_back_s": round(t_fetch, 3)}
    say(json.dumps(out))
    ctx.close()
    del ctx

    # wall time from process start to exit: the other build's map and this tree's, alternately, three times; the bytes must be the same
    new, old = bw.HOST_BIN, os.path.join(sys.argv[1], "bwbble")
    sam, tsv = os.path.join(a.workdir, "indel_measure.sam"), os.path.join(a.workdir, "indel_measure.tsv")
    runs = [("parent map", [old, "map", "-n", "3", fa, fq, sam]), ("map", [new, "map", "-n", "3", fa, fq, sam])] * 3
    runs += [("map -B", [new, "map", "-n", "3", "-B", data, fa, fq, sam]), ("map -B -I", [new, "map", "-n", "3", "-B", data, "-I", tsv, fa, fq, sam]),
             ("map -X 5 -B -J", [new, "map", "-n", "3", "-X", "5", "-B", data, "-J", fa, fq, sam]), ("map -X 5 -B -J -I", [new, "map", "-n", "3", "-X", "5", "-B", data, "-J", "-I", tsv, fa, fq, sam])]
    sums, times = {}, {}
    for name, cmd in runs:
        if not os.path.exists(cmd[0]):
            say(name, "binary missing")
            continue
        t0 = time.time()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        dt = time.time() - t0
        if r.returncode != 0:
            say(name, "FAILED", r.returncode, r.stdout[-1500:])
            return 1
        lines = [ln for ln in r.stdout.split("\n") if "placements on the GPU" in ln or "read support per indel bubble" in ln]
        sums.setdefault(name, set()).add(digest(sam))
        times.setdefault(name, []).append(dt)
        more = f"  table {os.path.getsize(tsv)} bytes  sha256 {digest(tsv)}" if "-I" in cmd else ""
        say(f"{name}: {dt:.2f} s  sam {os.path.getsize(sam)} bytes  sha256 {digest(sam)}{more}  | {' | '.join(lines)}")
    if "parent map" in sums:
        say("plain map writes the parent's bytes:", sums["map"] == sums["parent map"] and len(sums["map"]) == 1)
        lo, hi = min(times["parent map"]), max(times["parent map"])
        say(f"plain map: this tree {min(times['map']):.2f}-{max(times['map']):.2f} s (median {statistics.median(times['map']):.2f}), the parent {lo:.2f}-{hi:.2f} s: "
            f"the median lies {'inside' if lo <= statistics.median(times['map']) <= hi else ('BELOW' if statistics.median(times['map']) < lo else 'ABOVE')} the parent's spread")
    say("map -I writes the SAM bytes of the run without:", sums.get("map -B -I") == sums.get("map -B"), " with -X 5 -J:", sums.get("map -X 5 -B -J -I") == sums.get("map -X 5 -B -J"))
    for p in (sam, tsv):
        if os.path.exists(p):
            os.remove(p)
    return 0


if __name__ == "__main__":
    sys.exit(main())
