#!/usr/bin/env python3
"""What `map -D` costs: kernels k_md_count + scan + k_md beside k_place, k_locus and the lift kernels on one 2.5 M-read slot of the GRCh37-scale
index of bench.py (6.85 G rows, 1.29 M bubble records: the stats of the same calls), plain and on the lifted records of `-X 5 -B -J -R`; the
seconds and bytes of the .ref read and of set_text; the bytes -D brings back for the slot; and the wall time of this tree's plain `map -n 3`
against another build's - the parent commit's - on the same reads, three runs each, alternating, with the SAM bytes compared; then
`map -n 3 -D` and `map -X 5 -B -J -R [-D]` once each.  The input is that of tools/map_lift.py; <fasta>.ref is written with `bwbble fasta2ref`
outside every timed region when it is absent.
usage: tools/map_md.py <the other build's bwbble_amd/bin> [output file]     (profiles/map_md.txt is one run's output)"""
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

OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.getcwd(), "map_md.txt")
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
    names, start, end = bw.read_ann(fa + ".ann")
    if not os.path.exists(fa + ".ref"):  # (`bwbble index` of bench.py keeps none; fasta2ref rewrites the same .ann beside it)
        t0 = time.time()
        subprocess.run([bw.HOST_BIN, "fasta2ref", fa], check=True, stdout=subprocess.DEVNULL)
        say(f"fasta2ref: {time.time() - t0:.0f} s")
        assert bw.read_ann(fa + ".ann")[0] == names
    # bubble.data of the synthetic multi-genome, from its .ann (bwb_synth: 124 + ins + 124 around 0-based position p)
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
    codes = bw.read_ref(fa)
    t_read = time.time() - t0
    t0 = time.time()
    ctx.set_text(codes)
    t_set = time.time() - t0
    say(json.dumps({"text_characters": int(len(codes)), "ref_read_s": round(t_read, 2), "set_text_s": round(t_set, 2), "packed_bytes": int((len(codes) + 31) // 32 * 16)}))
    del codes
    t0 = time.time()
    ctx.align(bw.params(["-n", "3"]), seqs, lens)
    say(f"align of {len(lens)} reads: {time.time() - t0:.1f} s")
    ctx.join(6, 5)
    _, _, pms = ctx.place_stats()
    _, lms = ctx.locus_stats()
    kinds, _, _ = ctx.lift(6, 5)
    _, _, fms = ctx.lift_stats()
    out = {"reads": int(len(lens)), "k_place_ms": round(pms, 3), "k_locus_ms": round(lms, 3), "k_lift_ms": round(fms, 3)}
    for lifted in (False, True):
        recs_md, off, text = ctx.batch_md(6, 5, lifted)
        n_ok, n_bytes, ms = ctx.md_stats()
        key = "lifted" if lifted else "plain"
        out[key] = {"k_md_ms": round(ms, 3), "reads_tagged": int(n_ok), "too_long": int((recs_md["kind"] == bw.MD_TOO_LONG).sum()), "md_bytes": int(n_bytes),
                    "d2h_bytes": int(recs_md.nbytes + off.nbytes + len(text)), "nm_sum": int(recs_md["nm"].sum()), "md_with_a_deletion": int(text.count(b"^"))}
    out["primaries_lifted"] = int((kinds[:len(lens)] == bw.LIFT_LIFTED).sum())
    say(json.dumps(out))
    ctx.close()
    del ctx

    # wall time from process start to exit: the other build's map and this tree's, alternately, three times; the bytes must be the same
    new, old = bw.HOST_BIN, os.path.join(sys.argv[1], "bwbble")
    sam = os.path.join(a.workdir, "md_measure.sam")
    full = ["-X", "5", "-B", data, "-J", "-R"]
    runs = [("parent map", [old, "map", "-n", "3", fa, fq, sam]), ("map", [new, "map", "-n", "3", fa, fq, sam])] * 3
    runs += [("map -D", [new, "map", "-n", "3", "-D", fa, fq, sam]), ("map -X 5 -B -J -R", [new, "map", "-n", "3"] + full + [fa, fq, sam]),
             ("map -X 5 -B -J -R -D", [new, "map", "-n", "3"] + full + ["-D", fa, fq, sam])]
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
        lines = [ln for ln in r.stdout.split("\n") if "placements on the GPU" in ln or "NM and MD" in ln]
        sums.setdefault(name, set()).add(digest(sam))
        times.setdefault(name, []).append(dt)
        say(f"{name}: {dt:.2f} s  sam {os.path.getsize(sam)} bytes  sha256 {digest(sam)}  | {' | '.join(lines)}")
    if "parent map" in sums:
        say("plain map writes the parent's bytes:", sums["map"] == sums["parent map"] and len(sums["map"]) == 1)
        say(f"plain map: this tree {min(times['map']):.2f}-{max(times['map']):.2f} s, the parent {min(times['parent map']):.2f}-{max(times['parent map']):.2f} s: "
            f"{'inside' if statistics.median(times['map']) <= max(times['parent map']) else 'ABOVE'} the parent's spread")
    if os.path.exists(sam):
        os.remove(sam)
    return 0


if __name__ == "__main__":
    sys.exit(main())
