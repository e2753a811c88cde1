#!/usr/bin/env python3
"""What `map -B` costs: kernel k_locus beside k_place on one 2.5 M-read slot of the GRCh37-scale index of bench.py (6.85 G rows, 1.29 M bubble
records: place_stats and locus_stats of the same call), and the wall time of this tree's `map -n 3 -B` against another build's - the parent
commit's - `map -n 3` on the same reads, alternating, with `bwbble sampad` of the plain SAM compared byte for byte with `map -B`'s.
bubble.data is derived from the synthetic multi-genome's .ann (bwbble_amd/tools/bwb_synth.c: 124 + ins + 124 around position p).
usage: tools/map_locus.py <the other build's bwbble_amd/bin> [output file]     (profiles/map_locus.txt is one run's output)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench
import bwbble_amd as bw

OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.getcwd(), "map_locus.txt")
N_READS = 2_500_000


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    a = bench.parse_args([])
    t0 = time.time()
    fa = bench.build_genome(a, bw)
    say(f"index ready in {time.time() - t0:.0f} s: {fa}")
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
    say(f"records {len(names)}  bubbles {len(recs)}")

    seqs, lens = bw.load_fastq_codes(fq)
    b = bw.BwtFile(fa + ".bwt", load_sa=True)
    t0 = time.time()
    ctx = bw.Context(b)
    ctx.set_sa(b.SA)
    ctx.set_loci(start, end, bub_of, recs)
    say(f"context + SA + tables in {time.time() - t0:.1f} s")
    t0 = time.time()
    ctx.align(bw.params(["-n", "3"]), seqs, lens)
    say(f"align of {len(lens)} reads: {time.time() - t0:.1f} s")
    places, loci = ctx.locus(6)
    pn, psteps, pms = ctx.place_stats()
    ln, lms = ctx.locus_stats()
    say(json.dumps({"reads": int(pn), "k_place_ms": round(pms, 3), "k_place_steps": int(psteps), "k_locus_reads": int(ln), "k_locus_ms": round(lms, 3),
                    "mapped": int((places["flags"] & 1).sum()), "on_bubbles": int((loci["bubble"] >= 0).sum()), "ranges": int((loci["kind"] == 2).sum())}))
    places2, loci2 = ctx.locus(6)  # (cached records)
    assert loci2.tobytes() == loci.tobytes()
    ctx.close()
    del ctx

    # wall time from process start to exit: the other build's map, this tree's map, this tree's map -B; then the other build's and map -B again
    new, old = bw.HOST_BIN, os.path.join(sys.argv[1], "bwbble")
    sam = os.path.join(a.workdir, "pad_measure.sam")
    runs = [("parent map", [old, "map", "-n", "3", fa, fq, sam]), ("map", [new, "map", "-n", "3", fa, fq, sam]),
            ("map -B", [new, "map", "-n", "3", "-B", data, fa, fq, sam])]
    sizes = {}
    for rnd in range(2):
        for name, cmd in runs:
            if rnd == 1 and name == "map":
                continue
            if not os.path.exists(cmd[0]):
                say(name, "binary missing")
                continue
            t0 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            dt = time.time() - t0
            if r.returncode != 0:
                say(name, "FAILED", r.returncode, r.stdout[-1500:])
                return 1
            line = [ln for ln in r.stdout.split("\n") if "placements on the GPU" in ln]
            sizes[name] = os.path.getsize(sam)
            say(f"round {rnd} {name}: {dt:.2f} s  sam {sizes[name]} bytes  | {line[0] if line else ''}")
            if name == "map":
                os.replace(sam, sam + ".plain")
            elif name == "map -B" and rnd == 0:
                pad = sam + ".sampad"
                t0 = time.time()
                subprocess.run([new, "sampad", data, sam + ".plain", pad], check=True, stdout=subprocess.DEVNULL)
                same = subprocess.run(["cmp", "-s", pad, sam]).returncode == 0
                say(f"sampad of map's SAM: {time.time() - t0:.2f} s  equal to map -B: {same}")
    for f in (sam, sam + ".plain", sam + ".sampad"):
        if os.path.exists(f):
            os.remove(f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
