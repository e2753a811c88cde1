#!/usr/bin/env python3
"""What `map -X 5 -B -J -R` costs and changes: kernels k_lift_count + scan + k_lift beside k_place, k_place_alt, k_locus and the join kernels on
one 2.5 M-read slot of the GRCh37-scale index of bench.py (6.85 G rows, 1.29 M bubble records: the stats of the same calls) with the numbers
of placements lifted and not liftable and the bytes that come back for them, and the wall time of this tree's plain `map -n 3` against
another build's - the parent commit's - on the same reads, three runs each, alternating, with the SAM bytes compared; then
`map -X 5 -B -J` and `map -X 5 -B -J -R` once each.  The input is that of tools/map_locus.py and tools/map_join.py.
usage: tools/map_lift.py <the other build's bwbble_amd/bin> [output file]     (profiles/map_lift.txt is one run's output)"""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench
import bwbble_amd as bw

OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.getcwd(), "map_lift.txt")
N_READS = 2_500_000


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
    # bubble.data of the synthetic multi-genome, from its .ann (bwb_synth: 124 + ins + 124 around 0-based position p)
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
    t0 = time.time()
    ctx.align(bw.params(["-n", "3"]), seqs, lens)
    say(f"align of {len(lens)} reads: {time.time() - t0:.1f} s")
    places, alt_off, alts, loci, joins = ctx.join(6, 5)
    _, _, pms = ctx.place_stats()
    items, _, ams = ctx.place_alt_stats()
    _, lms = ctx.locus_stats()
    _, _, jms = ctx.join_stats()
    kinds, off, words = ctx.lift(6, 5)
    lifted, unliftable, fms = ctx.lift_stats()
    n = len(places)
    shapes = {}
    for q in (kinds == bw.LIFT_LIFTED).nonzero()[0][:200000]:
        s = "".join("MID?S"[op] for _, op in bw.lift_record(words, off[q])[2])
        shapes[s] = shapes.get(s, 0) + 1
    say(json.dumps({"reads": n, "items": int(items), "k_place_ms": round(pms, 3), "k_place_alt_ms": round(ams, 3), "k_locus_ms": round(lms, 3), "k_join_ms": round(jms, 3),
                    "k_lift_ms": round(fms, 3), "placements": len(kinds), "lifted": int(lifted), "not_liftable": int(unliftable),
                    "primaries_lifted": int((kinds[:n] == bw.LIFT_LIFTED).sum()), "items_lifted": int((kinds[n:] == bw.LIFT_LIFTED).sum()),
                    "d2h_bytes": int(len(kinds) + 8 * len(off) + 16 * len(words)), "record_bytes": int(16 * len(words)), "shapes": dict(sorted(shapes.items(), key=lambda kv: -kv[1])[:8])}))
    again = ctx.lift(6, 5)  # (cached records)
    assert again[0].tobytes() == kinds.tobytes() and again[2].tobytes() == words.tobytes()
    ctx.close()
    del ctx

    # wall time from process start to exit: the other build's map and this tree's, alternately, three times; the bytes must be the same
    new, old = bw.HOST_BIN, os.path.join(sys.argv[1], "bwbble")
    sam = os.path.join(a.workdir, "lift_measure.sam")
    runs = [("parent map", [old, "map", "-n", "3", fa, fq, sam]), ("map", [new, "map", "-n", "3", fa, fq, sam])] * 3
    runs += [("map -X 5 -B -J", [new, "map", "-n", "3", "-X", "5", "-B", data, "-J", fa, fq, sam]), ("map -X 5 -B -J -R", [new, "map", "-n", "3", "-X", "5", "-B", data, "-J", "-R", fa, fq, sam])]
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
        lines = [ln for ln in r.stdout.split("\n") if "placements on the GPU" in ln or "joined by locus" in ln or "lifted to chromosome" in ln]
        sums.setdefault(name, set()).add(digest(sam))
        times.setdefault(name, []).append(dt)
        say(f"{name}: {dt:.2f} s  sam {os.path.getsize(sam)} bytes  sha256 {digest(sam)}  | {' | '.join(lines)}")
    if "parent map" in sums:
        say("plain map writes the parent's bytes:", sums["map"] == sums["parent map"] and len(sums["map"]) == 1)
        say(f"plain map: this tree's median {statistics.median(times['map']):.2f} s, the parent's slowest run {max(times['parent map']):.2f} s: "
            f"{'within' if statistics.median(times['map']) <= max(times['parent map']) else 'ABOVE'} the bar")
    if os.path.exists(sam):
        os.remove(sam)
    return 0


if __name__ == "__main__":
    sys.exit(main())
