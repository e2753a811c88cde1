#!/usr/bin/env python3
"""What `map -A` costs: pile_begin (kernels k_site_count + k_scan_sums + k_site_add: the site index and the zeroed counters) and k_pile beside
k_place and k_md_count + k_md on one 2.5 M-read slot of the GRCh37-scale index of bench.py (the stats of the same calls), plain and on the lifted
and joined records of `-X 5 -B -J -R`; the reads counted, the adds and the sites touched; the read-back of the counters; and the wall time of this
tree's plain `map -n 3` against another build's - the parent commit's - on the same reads, three runs each, alternating, with the SAM bytes
compared; then `map -n 3 -A` and `map -X 5 -B -J -R -A` once each.  The input is that of tools/map_md.py.
usage: tools/map_pile.py <the other build's bwbble_amd/bin> [output file]     (profiles/map_pile.txt is one run's output)"""
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

OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.getcwd(), "map_pile.txt")
N_READS = 2_500_000
PIECE = 1 << 20  # sites per read-back, as in `map`


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


def fetch(ctx, n_sites):
    """the counters in bounded pieces -> (sites touched, sum, seconds)"""
    t0 = time.time()
    touched = total = 0
    for s0 in range(0, n_sites, PIECE):
        part = ctx.pile_counts(s0, min(PIECE, n_sites - s0))
        touched += int(part.any(axis=1).sum())
        total += int(part.sum(dtype=np.uint64))
    return touched, total, time.time() - t0


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
    if not os.path.exists(fa + ".ref"):  # (`bwbble index` of bench.py keeps none; fasta2ref rewrites the same .ann beside it)
        t0 = time.time()
        subprocess.run([bw.HOST_BIN, "fasta2ref", fa], check=True, stdout=subprocess.DEVNULL)
        say(f"fasta2ref: {time.time() - t0:.0f} s")
        assert bw.read_ann(fa + ".ann")[0] == names
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
    codes = bw.read_ref(fa)
    ctx.set_text(codes)
    n_fwd = int(len(codes))
    del codes
    begins = []
    for _ in range(3):
        t0 = time.time()
        n_sites = ctx.pile_begin()
        begins.append(round(time.time() - t0, 3))
    say(json.dumps({"text_characters": n_fwd, "n_sites": int(n_sites), "pile_begin_s": begins, "site_index_bytes": (n_fwd + 31) // 32 * 4, "counter_bytes": int(n_sites) * 16}))
    out = {"reads": int(len(lens))}
    for key, (lifted, joined) in (("plain", (False, False)), ("lifted_joined", (True, True))):
        t0 = time.time()
        ctx.align(bw.params(["-n", "3"]), seqs, lens)  # (a submission is piled once: one batch per form)
        t_align = time.time() - t0
        ctx.pile_reset()
        if joined:
            ctx.join(6, 5)
            ctx.lift(6, 5)
        ctx.batch_md(6, 5, lifted)
        _, _, mms = ctx.md_stats()
        _, _, pms = ctx.place_stats()
        counted = ctx.batch_pile(6, 5, lifted, joined, 0)
        n_reads, n_adds, ms = ctx.pile_stats()
        touched, total, t_fetch = fetch(ctx, n_sites)
        assert counted == n_reads and total == n_adds, (counted, n_reads, total, n_adds)
        out[key] = {"align_s": round(t_align, 1), "k_place_ms": round(pms, 3), "k_md_ms": round(mms, 3), "k_pile_ms": round(ms, 3), "reads_counted": int(n_reads), "adds": int(n_adds),
                    "sites_touched": touched, "read_back_s": round(t_fetch, 3)}
    say(json.dumps(out))
    ctx.close()
    del ctx

    # wall time from process start to exit: the other build's map and this tree's, alternately, three times; the bytes must be the same
    new, old = bw.HOST_BIN, os.path.join(sys.argv[1], "bwbble")
    sam, tsv = os.path.join(a.workdir, "pile_measure.sam"), os.path.join(a.workdir, "pile_measure.tsv")
    full = ["-X", "5", "-B", data, "-J", "-R"]
    runs = [("parent map", [old, "map", "-n", "3", fa, fq, sam]), ("map", [new, "map", "-n", "3", fa, fq, sam])] * 3
    runs += [("map -A", [new, "map", "-n", "3", "-A", tsv, fa, fq, sam]), ("map -X 5 -B -J -R", [new, "map", "-n", "3"] + full + [fa, fq, sam]),
             ("map -X 5 -B -J -R -A", [new, "map", "-n", "3"] + full + ["-A", tsv, fa, fq, sam])]
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
        lines = [ln for ln in r.stdout.split("\n") if "placements on the GPU" in ln or "allele counts" in ln]
        sums.setdefault(name, set()).add(digest(sam))
        times.setdefault(name, []).append(dt)
        more = f"  counts {os.path.getsize(tsv)} bytes  sha256 {digest(tsv)}" if "-A" in cmd else ""
        say(f"{name}: {dt:.2f} s  sam {os.path.getsize(sam)} bytes  sha256 {digest(sam)}{more}  | {' | '.join(lines)}")
    if "parent map" in sums:
        say("plain map writes the parent's bytes:", sums["map"] == sums["parent map"] and len(sums["map"]) == 1)
        say(f"plain map: this tree {min(times['map']):.2f}-{max(times['map']):.2f} s, the parent {min(times['parent map']):.2f}-{max(times['parent map']):.2f} s: "
            f"{'inside' if statistics.median(times['map']) <= max(times['parent map']) else 'ABOVE'} the parent's spread")
    say("map -A writes the SAM bytes of map:", sums.get("map -A") == sums.get("map"), " with -X 5 -B -J -R:", sums.get("map -X 5 -B -J -R -A") == sums.get("map -X 5 -B -J -R"))
    for p in (sam, tsv):
        if os.path.exists(p):
            os.remove(p)
    return 0


if __name__ == "__main__":
    sys.exit(main())
