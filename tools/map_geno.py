#!/usr/bin/env python3
"""What `map -G` costs: the geno kernels (k_geno_count + scan + k_geno_emit over every site, k_geno_bubbles over every bubble, in pieces of 2^20:
the stats of the same calls) on the counters one 2.5 M-read slot of the GRCh37-scale index of bench.py leaves behind, the called entries and the
bytes that come back for them beside the dense read-back of -A's counters, the seconds of putting the whole tables back (what the last of several
workers does); and the wall time of this tree's plain `map -n 3` against another build's - the parent commit's - on the same reads, three runs
each, alternating, with the SAM bytes compared; then `map -n 3 -A`, `map -n 3 -G`, `map -X 5 -B -J -R -G` and the last with two workers once each.
The input is that of tools/map_pile.py.
usage: tools/map_geno.py <the other build's bwbble_amd/bin> [output file]     (profiles/map_geno.txt is one run's output)"""
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

OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.getcwd(), "map_geno.txt")
N_READS = 2_500_000
PIECE = 1 << 20  # entries per call, as in `map`


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
    if not os.path.exists(fa + ".ref"):
        t0 = time.time()
        subprocess.run([bw.HOST_BIN, "fasta2ref", fa], check=True, stdout=subprocess.DEVNULL)
        say(f"fasta2ref: {time.time() - t0:.0f} s")
    data = os.path.join(a.workdir, "pad_measure.data")
    header = {n.split()[0]: n for n in names if not n.startswith("bubble")}
    with open(data, "w") as f:
        for n, s, e in zip(names, start, end):
            if n.startswith("bubble"):
                _, ch, p = n.split()
                p, ins = int(p), int(e - s) + 1 - 248
                f.write(f"{header[ch]}\n{p - 123}\t124\t{p + 1}\t123\t0\t{ins}\n")
    anns, recs = bw.read_bubble_data(data)
    say(f"records {len(names)}  bubbles {len(recs)}")

    seqs, lens = bw.load_fastq_codes(fq)
    b = bw.BwtFile(fa + ".bwt", load_sa=True)
    ctx = bw.Context(b)
    ctx.set_sa(b.SA)
    ctx.set_loci(start, end, bw.bubble_of(names, len(recs)), recs)
    ctx.set_bubble_chrom(bw.bubble_chrom_of(names, anns))
    ctx.set_text(bw.read_ref(fa))
    n_sites, n_bub = ctx.pile_begin(), len(recs)
    n_elig = ctx.indel_begin(1)
    ctx.geno_begin(PIECE)
    ctx.align(bw.params(["-n", "3"]), seqs, lens)
    ctx.batch_pile(6, 0, False, False, 0)
    ctx.batch_indel(6, 0, False, 0)
    out = {"n_sites": int(n_sites), "bubbles": n_bub, "eligible": int(n_elig), "reads": int(len(lens))}
    for d in (1, 2):
        t0, ms, called, calls = time.time(), 0.0, 0, 0
        for s0 in range(0, n_sites, PIECE):
            called += len(ctx.geno_sites(s0, min(PIECE, n_sites - s0), 20, d))
            ms += ctx.geno_stats()[2]
            calls += 1
        t_sites, t0, bms, bcalled = time.time() - t0, time.time(), 0.0, 0
        for s0 in range(0, n_bub, PIECE):
            bcalled += len(ctx.geno_bubbles(s0, min(PIECE, n_bub - s0), 20, d))
            bms += ctx.geno_stats()[2]
            calls += 1
        out[f"min_depth_{d}"] = {"site_kernels_ms": round(ms, 3), "sites_called": called, "sites_wall_s": round(t_sites, 3), "bubble_kernels_ms": round(bms, 3), "bubbles_called": bcalled,
                                 "bubbles_wall_s": round(time.time() - t0, 3), "bytes_back": called * 64 + bcalled * 48 + calls * 8, "dense_counter_bytes": int(n_sites) * 16 + n_bub * 16}
    # the tables fetched and put back whole, in pieces: what the last of several workers uploads before it calls
    parts = [ctx.pile_counts(s0, min(PIECE, n_sites - s0)) for s0 in range(0, n_sites, PIECE)]
    t0 = time.time()
    for k, part in enumerate(parts):
        ctx.pile_put(k * PIECE, part)
    ctx.indel_put(0, ctx.indel_counts(0, n_bub))
    out["put_back_s"] = round(time.time() - t0, 3)
    out["put_back_bytes"] = int(n_sites) * 16 + n_bub * 16
    say(json.dumps(out))
    ctx.close()
    del ctx, parts

    new, old = bw.HOST_BIN, os.path.join(sys.argv[1], "bwbble")
    sam, tsv = os.path.join(a.workdir, "geno_measure.sam"), os.path.join(a.workdir, "geno_measure.tsv")
    full = ["-X", "5", "-B", data, "-J", "-R"]
    runs = [("parent map", [old, "map", "-n", "3", fa, fq, sam], {}), ("map", [new, "map", "-n", "3", fa, fq, sam], {})] * 3
    runs += [("map -A", [new, "map", "-n", "3", "-A", tsv, fa, fq, sam], {}), ("map -G", [new, "map", "-n", "3", "-G", tsv, fa, fq, sam], {}),
             ("map -X 5 -B -J -R -G", [new, "map", "-n", "3"] + full + ["-G", tsv, fa, fq, sam], {}),
             ("map -g 2 -X 5 -B -J -R -G", [new, "map", "-n", "3", "-g", "2"] + full + ["-G", tsv, fa, fq, sam], {"BWB_DEVICE_MAP": "0,0"})]
    sums, times, files = {}, {}, {}
    for name, cmd, env in runs:
        if not os.path.exists(cmd[0]):
            say(name, "binary missing")
            continue
        t0 = time.time()
        r = subprocess.run(cmd, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        dt = time.time() - t0
        if r.returncode != 0:
            say(name, "FAILED", r.returncode, r.stdout[-1500:])
            return 1
        lines = [ln for ln in r.stdout.split("\n") if "genotype calls" in ln or "allele counts written" in ln]
        sums.setdefault(name, set()).add(digest(sam))
        times.setdefault(name, []).append(dt)
        more = ""
        if name not in ("map", "parent map"):
            files[name] = digest(tsv)
            more = f"  file {os.path.getsize(tsv)} bytes  sha256 {files[name]}"
        say(f"{name}: {dt:.2f} s  sam {os.path.getsize(sam)} bytes  sha256 {digest(sam)}{more}  | {' | '.join(lines)}")
    if "parent map" in sums:
        say("plain map writes the parent's bytes:", sums["map"] == sums["parent map"] and len(sums["map"]) == 1)
        say(f"plain map: this tree {min(times['map']):.2f}-{max(times['map']):.2f} s, the parent {min(times['parent map']):.2f}-{max(times['parent map']):.2f} s: "
            f"{'inside' if statistics.median(times['map']) <= max(times['parent map']) else 'ABOVE'} the parent's spread")
    say("map -G writes the SAM bytes of map:", sums.get("map -G") == sums.get("map"), " one and two workers write one calls file and one SAM file:",
        sums.get("map -g 2 -X 5 -B -J -R -G") == sums.get("map -X 5 -B -J -R -G") and files.get("map -g 2 -X 5 -B -J -R -G") == files.get("map -X 5 -B -J -R -G"))
    for p in (sam, tsv):
        if os.path.exists(p):
            os.remove(p)
    return 0


if __name__ == "__main__":
    sys.exit(main())
