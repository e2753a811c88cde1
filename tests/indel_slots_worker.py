"""Worker of tests/test_gpu_indel.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the product or the TEST build.
The generated genome of tests/lift_model.py is indexed here and the reads of tests/indel_model.py are mapped on it (`-n 3 -o 1`, so that the
reads with an inserted or a deleted base are found): batch_indel plain and joined (-X 5) on one batch, then slot_indel in chunks of 197 reads
through the eight slots and round again with every wave parked after 150 loop iterations (BWB_SLICE_ITERS, set by the test), before and after
slot_result - a second slot_indel on the same submission adds nothing - against tests/indel_model.py fed the ORACLE's hits: the table of the
stream is the table of the one batch.
usage: indel_slots_worker.py <work directory>"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alt_model  # noqa: E402
import bwbble_amd as bw  # noqa: E402
import indel_model  # noqa: E402
import join_model  # noqa: E402
import lift_model  # noqa: E402
import map_model  # noqa: E402
import oracle_lib  # noqa: E402
import pad_model  # noqa: E402

work = sys.argv[1]
g = lift_model.genome()
gen_reads = indel_model.reads(g)
fa, fq = os.path.join(work, "gen.fa"), os.path.join(work, "gen.fq")
open(fa, "w").write(g["fasta"])
open(fq, "w").write(indel_model.fastq(gen_reads))
subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL, timeout=300)
names, start, end = bw.read_ann(fa + ".ann")
bubbles = g["bubbles"]
bub_of = pad_model.bubble_of(names, bubbles)
chrom = join_model.chrom_of(names, bubbles)
W, FLAGS = 5, ["-n", "3", "-o", "1"]

orc = oracle_lib.load()
idx = orc.load_index(fa + ".bwt", load_sa=True)
b = bw.BwtFile(fa + ".bwt", load_sa=True)
ctx = bw.Context(b)
ctx.set_sa(b.SA)
ctx.set_loci(start, end, bub_of, pad_model.bubble_records(bubbles))
ctx.set_bubble_chrom(chrom)
n_elig = ctx.indel_begin(W)
assert n_elig == sum(indel_model.eligible(v, W) for v in bubbles) == len(bubbles) - 1
seqs, lens = bw.encode_reads(bw.read_fastq(fq))
p = bw.params(FLAGS)

# the model fed the oracle's hits: placement records, their loci, join records (-X 5)
data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(FLAGS))
reads = oracle_lib.parse_aln(data)
places, _ = map_model.expected_places(orc, idx, reads, 6)
loci = pad_model.expected_loci(places, start, end, bub_of, bubbles)
off, alts, _ = alt_model.expected_alts(reads, 5, alt_model.OracleSA(orc, idx))
joins, _ = join_model.expected_joins(places, off, alts, join_model.suboptimal(reads, off, alts), start, end, bub_of, bubbles, chrom, 6)
MODES = {"plain": (False, 0), "plain, MAPQ 1": (False, 1), "joined, MAPQ 1": (True, 1)}


def want_of(lo, hi, joined, q):
    return indel_model.count(indel_model.from_records(places[lo:hi], loci[lo:hi], joins["mapq"][lo:hi] if joined else None, lens[lo:hi]), bubbles, chrom, W, q)


wants = {m: want_of(0, len(lens), *MODES[m]) for m in MODES}
# every error-free read the name judge calls clean is counted where the judge says (the oracle places it where it was cut: the census of test_indel_host.py)
judged = indel_model.judged_table([r for r in gen_reads if r[6] is None], bubbles, W)
assert (wants["plain"][0][:, :2] >= judged[:, :2]).all() and wants["plain"][0][:, 2:].any() and judged[:, :2].sum() > 1000
# the joined MAPQ lets the reads in a flank count that two placements held at 0
assert wants["joined, MAPQ 1"][1] > wants["plain, MAPQ 1"][1] and wants["plain"][1] > wants["plain, MAPQ 1"][1]
# the table is equal plain and joined wherever the joined MAPQ does not cross -a
assert np.array_equal(want_of(0, len(lens), True, 0)[0], wants["plain"][0])

for m, (joined, q) in MODES.items():
    ctx.indel_reset()
    ctx.align(p, seqs, lens)
    counted = ctx.batch_indel(6, 5, joined, q)
    want, n_reads, n_adds = wants[m]
    got = ctx.indel_counts(0, len(bubbles))
    assert np.array_equal(got, want), (m, got.tolist(), want.tolist())
    st = ctx.indel_stats()
    assert counted == n_reads and st[:2] == (n_reads, n_adds) and st[2] >= n_adds and st[3] > 0, (m, counted, st, n_reads, n_adds)
    assert ctx.batch_indel(6, 5, joined, q) == 0 and ctx.batch_indel(6, 5, not joined, 0) == 0  # (a submission is counted once)
    assert np.array_equal(ctx.indel_counts(0, len(bubbles)), want), m
assert bw.aln_bytes(*ctx.result()) == data

# streamed, with parked reads: slot_indel before slot_result on even slots and after it on odd ones, and once more behind
cuts = list(range(0, len(lens), 197)) + [len(lens)]
assert len(cuts) - 1 > bw.MAX_SLOTS
for m in ("joined, MAPQ 1", "plain"):
    joined, q = MODES[m]
    ctx.indel_reset()
    seen = counted = 0

    def collect(j):
        global seen, counted
        slot, (lo, hi) = j % bw.MAX_SLOTS, (cuts[j], cuts[j + 1])
        if slot % 2 == 0:
            got = ctx.slot_indel(slot, 6, 5, joined, q)
            ctx.slot_result(slot)
        else:
            ctx.slot_result(slot)
            got = ctx.slot_indel(slot, 6, 5, joined, q)
        _, n_reads, n_adds = want_of(lo, hi, joined, q)
        assert got == n_reads and ctx.indel_stats()[:2] == (n_reads, n_adds), (m, j, got, n_reads)
        assert ctx.slot_indel(slot, 6, 5, joined, q) == 0 and ctx.slot_indel(slot, 6, 5, False, 0) == 0, j
        seen += 1
        counted += got

    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if j >= bw.MAX_SLOTS:
            collect(j - bw.MAX_SLOTS)
        ctx.slot_upload(j % bw.MAX_SLOTS, p, seqs[lo:hi], lens[lo:hi])
        ctx.slot_submit(j % bw.MAX_SLOTS)
    for j in range(max(0, len(cuts) - 1 - bw.MAX_SLOTS), len(cuts) - 1):
        collect(j)
    want, n_reads, _ = wants[m]
    got = ctx.indel_counts(0, len(bubbles))
    assert seen == len(cuts) - 1 and counted == n_reads
    assert np.array_equal(got, want), (m, "streamed", got.tolist(), want.tolist())  # the table of the one batch
assert ctx.stats().n_parked_reads > 0
ctx.close()
print(f"INDEL-SLOTS-OK {seen} chunks, {counted} reads counted, {os.path.basename(bw.LIB_PATH)}")
