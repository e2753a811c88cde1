"""Worker of tests/test_gpu_join.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the product or the TEST
build (bwbble_amd/libbwbble_hip_test.so: 2^13-block superblocks, biased stored positions).  The pad_bub reads on the toy index: batch_join,
then slot_join in chunks of 97 reads through the eight slots and round again with every wave parked after 150 loop iterations
(BWB_SLICE_ITERS, set by the test), against tests/join_model.py fed the ORACLE's hits; join_stats against the model's counts.
usage: join_slots_worker.py <directory with the unpacked pad_bub files>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alt_model  # noqa: E402
import bwbble_amd as bw  # noqa: E402
import join_model  # noqa: E402
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
    """the model fed the oracle's hits -> (places, alt_off, alts, loci, joins, joined items, the oracle's .aln bytes)"""
    data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(["-n", "3"]))
    reads = oracle_lib.parse_aln(data)
    places, _ = map_model.expected_places(orc, idx, reads, max_mm)
    off, alts, _ = alt_model.expected_alts(reads, max_alt, sa)
    loci = pad_model.expected_loci(places, start, end, bub_of, bubbles)
    joins, total = join_model.expected_joins(places, off, alts, join_model.suboptimal(reads, off, alts), start, end, bub_of, bubbles, chrom, max_mm)
    return places, off, alts, loci, joins, total, data


def same(got, want, what):
    for g, w, name in zip(got, want[:5], ("places", "alt_off", "alts", "loci", "joins")):
        assert g.tobytes() == np.asarray(w, dtype=g.dtype).tobytes(), (what, name, join_model.first_difference(g, w) if name == "joins" else "")


seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(sys.argv[1], "pad_bub.fq")))
b = bw.BwtFile(bwt, load_sa=True)
ctx = bw.Context(b)
ctx.set_sa(b.SA)
ctx.set_loci(start, end, bub_of, recs)
ctx.set_bubble_chrom(chrom)
p = bw.params(["-n", "3"])

# one batch: -Q 6 and 3, -X 5 and 1; the records of the other calls unchanged beside them
ctx.align(p, seqs, lens)
raised = 0
for max_mm, max_alt in ((6, 5), (3, 5), (6, 1)):
    want = want_of(seqs, lens, max_mm, max_alt)
    same(ctx.join(max_mm, max_alt), want, ("batch", max_mm, max_alt))
    items, joined, ms = ctx.join_stats()
    assert (items, joined) == (len(want[2]), want[5]) and ms > 0, (ctx.join_stats(), len(want[2]), want[5])
    assert ctx.place(max_mm).tobytes() == want[0].tobytes() and ctx.locus(max_mm)[1].tobytes() == want[3].tobytes()
    raised = max(raised, int(((want[0]["mapq"] == 0) & (want[4]["mapq"] > 0)).sum()))
assert raised >= 100, raised
assert bw.aln_bytes(*ctx.result()) == want[6]

# streamed, with parked reads: slot_join before slot_result on even slots and after it on odd ones, and once more behind the other record calls
seqs, lens = np.concatenate([seqs, seqs[:330]]), np.concatenate([lens, lens[:330]])
cuts = list(range(0, len(lens), 97)) + [len(lens)]
wants = [want_of(seqs[lo:hi], lens[lo:hi], 6, 5) for lo, hi in zip(cuts[:-1], cuts[1:])]
assert len(wants) > bw.MAX_SLOTS
seen = joined_all = 0


def collect(j):
    global seen, joined_all
    slot, want = j % bw.MAX_SLOTS, wants[j]
    if slot % 2 == 0:
        got = ctx.slot_join(slot)
        off, alns = ctx.slot_result(slot)
    else:
        off, alns = ctx.slot_result(slot)
        got = ctx.slot_join(slot)
    same(got, want, ("slot", j))
    assert ctx.join_stats()[:2] == (len(want[2]), want[5]), j
    assert bw.aln_bytes(off, alns) == want[6], j
    assert ctx.slot_place_alt(slot, 6, 5)[2].tobytes() == want[2].tobytes() and ctx.slot_locus(slot)[1].tobytes() == want[3].tobytes(), j
    same(ctx.slot_join(slot), want, ("slot again", j))
    seen += 1
    joined_all += want[5]


for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
    if j >= bw.MAX_SLOTS:
        collect(j - bw.MAX_SLOTS)
    ctx.slot_upload(j % bw.MAX_SLOTS, p, seqs[lo:hi], lens[lo:hi])
    ctx.slot_submit(j % bw.MAX_SLOTS)
for j in range(max(0, len(wants) - bw.MAX_SLOTS), len(wants)):
    collect(j)
assert seen == len(wants) and joined_all >= 260
assert ctx.stats().n_parked_reads > 0
ctx.close()
print(f"JOIN-SLOTS-OK {seen} chunks, {joined_all} joined items, {os.path.basename(bw.LIB_PATH)}")
