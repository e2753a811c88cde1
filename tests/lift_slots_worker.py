"""Worker of tests/test_gpu_lift.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the product or the TEST
build.  The pad_bub reads on the toy index: batch_lift, then slot_lift in chunks of 97 reads through the eight slots and round again with
every wave parked after 150 loop iterations (BWB_SLICE_ITERS, set by the test), before and after slot_join / slot_result, against
tests/lift_model.py fed the ORACLE's hits; lift_stats against the model's counts.
usage: lift_slots_worker.py <directory with the unpacked pad_bub files>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alt_model  # noqa: E402
import bwbble_amd as bw  # noqa: E402
import join_model  # noqa: E402
import lift_model  # noqa: E402
import map_model  # noqa: E402
import oracle_lib  # noqa: E402
import pad_model  # noqa: E402

golden = os.path.join(ROOT, "tests", "golden")
bwt = os.path.join(golden, "toy.fa.bwt")
orc = oracle_lib.load()
idx = orc.load_index(bwt, load_sa=True)
sa = alt_model.OracleSA(orc, idx)
names, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
anns, recs = bw.read_bubble_data(os.path.join(golden, "pad_toy.data"))
bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
bub_of = pad_model.bubble_of(names, bubbles)
chrom = join_model.chrom_of(names, bubbles)


def want_of(seqs, lens, max_mm, max_alt):
    """the model fed the oracle's hits -> (kinds, records, the oracle's .aln bytes); max_alt 0: the primaries alone"""
    data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(["-n", "3"]))
    reads = oracle_lib.parse_aln(data)
    places, _ = map_model.expected_places(orc, idx, reads, max_mm)
    off, alts = np.zeros(len(places) + 1, dtype=np.uint64), np.zeros(0, dtype=bw.ALT_DTYPE)
    if max_alt:
        off, alts, _ = alt_model.expected_alts(reads, max_alt, sa)
    as_places = np.zeros(len(alts), dtype=bw.PLACE_DTYPE)
    as_places["pos"], as_places["flags"] = alts["pos"], alts["flags"]
    kinds, want = lift_model.expected_records(places, pad_model.expected_loci(places, start, end, bub_of, bubbles), off, alts,
                                              pad_model.expected_loci(as_places, start, end, bub_of, bubbles), bubbles, chrom)
    return kinds, want, data


def same(got, want, what):
    diff = lift_model.compare_records(got, want[0], want[1])
    assert diff is None, (what, diff)


seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(sys.argv[1], "pad_bub.fq")))
b = bw.BwtFile(bwt, load_sa=True)
ctx = bw.Context(b)
ctx.set_sa(b.SA)
ctx.set_loci(start, end, bub_of, recs)
ctx.set_bubble_chrom(chrom)
p = bw.params(["-n", "3"])

# one batch: -Q 6 and 3, -X 5, 1 and none
ctx.align(p, seqs, lens)
lifted_primaries = 0
for max_mm, max_alt in ((6, 5), (3, 5), (6, 1), (6, 0)):
    want = want_of(seqs, lens, max_mm, max_alt)
    same(ctx.lift(max_mm, max_alt), want, ("batch", max_mm, max_alt))
    lifted, unliftable, ms = ctx.lift_stats()
    assert (lifted, unliftable) == (int((want[0] == bw.LIFT_LIFTED).sum()), int((want[0] == bw.LIFT_UNLIFTABLE).sum())) and ms > 0, ctx.lift_stats()
    lifted_primaries = int((want[0][:len(lens)] == bw.LIFT_LIFTED).sum())
assert lifted_primaries == 447, lifted_primaries
assert bw.aln_bytes(*ctx.result()) == want[2]

# streamed, with parked reads: slot_lift before slot_join / slot_result on even slots and after them on odd ones, and once more behind them
seqs, lens = np.concatenate([seqs, seqs[:330]]), np.concatenate([lens, lens[:330]])
cuts = list(range(0, len(lens), 97)) + [len(lens)]
wants = [want_of(seqs[lo:hi], lens[lo:hi], 6, 5) for lo, hi in zip(cuts[:-1], cuts[1:])]
assert len(wants) > bw.MAX_SLOTS
seen = lifted_all = 0


def collect(j):
    global seen, lifted_all
    slot, want = j % bw.MAX_SLOTS, wants[j]
    if slot % 2 == 0:
        got = ctx.slot_lift(slot)
        joined = ctx.slot_join(slot)
        off, alns = ctx.slot_result(slot)
    else:
        off, alns = ctx.slot_result(slot)
        joined = ctx.slot_join(slot)
        got = ctx.slot_lift(slot)
    same(got, want, ("slot", j))
    assert ctx.lift_stats()[0] == int((want[0] == bw.LIFT_LIFTED).sum()), j
    assert bw.aln_bytes(off, alns) == want[2], j
    assert len(got[0]) == len(joined[0]) + len(joined[2]), j
    same(ctx.slot_lift(slot), want, ("slot again", j))
    seen += 1
    lifted_all += int((want[0] == bw.LIFT_LIFTED).sum())


for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
    if j >= bw.MAX_SLOTS:
        collect(j - bw.MAX_SLOTS)
    ctx.slot_upload(j % bw.MAX_SLOTS, p, seqs[lo:hi], lens[lo:hi])
    ctx.slot_submit(j % bw.MAX_SLOTS)
for j in range(max(0, len(wants) - bw.MAX_SLOTS), len(wants)):
    collect(j)
assert seen == len(wants) and lifted_all >= 447
assert ctx.stats().n_parked_reads > 0
ctx.close()
print(f"LIFT-SLOTS-OK {seen} chunks, {lifted_all} lifted placements, {os.path.basename(bw.LIB_PATH)}")
