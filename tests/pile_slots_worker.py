"""Worker of tests/test_gpu_pile.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the product or the TEST build.
First a text of 40 001 characters, which the test build uploads in two chunks (one for the product): its site index at every position, and
reads laid across the chunk's edge.  Then the pad_bub reads on the toy index: batch_pile plain, lifted and joined (-X 5) on one batch of 901
reads, then slot_pile in chunks of 97 reads through the eight slots and round again with every wave parked after 150 loop iterations
(BWB_SLICE_ITERS, set by the test), before and after slot_md / slot_result - a second slot_pile on the same submission adds nothing - against
tests/pile_model.py fed the ORACLE's hits: the table of the stream is the table of the one batch.
usage: pile_slots_worker.py <directory with the unpacked pad_bub files>"""
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
import md_model  # noqa: E402
import oracle_lib  # noqa: E402
import pad_model  # noqa: E402
import pile_model  # noqa: E402

golden = os.path.join(ROOT, "tests", "golden")
bwt = os.path.join(golden, "toy.fa.bwt")
orc = oracle_lib.load()
idx = orc.load_index(bwt, load_sa=True)
text, names, starts = pile_model.fasta_text(open(os.path.join(golden, "toy.fa")).read())
_, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
anns, recs = bw.read_bubble_data(os.path.join(golden, "pad_toy.data"))
bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
bub_of = pad_model.bubble_of(names, bubbles)
chrom = join_model.chrom_of(names, bubbles)

b = bw.BwtFile(bwt, load_sa=True)
ctx = bw.Context(b)

# a text that the test build uploads in two chunks (2^15 characters each): the index over both, reads across the edge and on the last characters
rng = np.random.default_rng(40)
long_text = "".join(rng.choice(list("ACGT" * 6 + md_model.LETTERS[1:]), 40_000)) + "R"
ctx.set_text(pile_model.codes(long_text))
n_long = ctx.pile_begin()
where_long = pile_model.site_of(long_text)
assert n_long == int(where_long.max()) + 1 > 10_000 and 0 < where_long[:1 << 15].max() < n_long - 1  # sites in both chunks
assert np.array_equal(ctx.pile_site_of(np.arange(len(long_text))), where_long)
where = [0, 31, 32, 1 << 15, (1 << 15) - 1, (1 << 15) - 50, (1 << 15) - 99, (1 << 15) - 100, len(long_text) - 100, len(long_text) - 99] + rng.integers(0, len(long_text) - 100, 200).tolist()
placed = [(int(p), bool(k & 1), "100M") for k, p in enumerate(where)]
pl = lift_model.place_records(placed)
sq = rng.integers(0, 5, (len(pl), 100)).astype(np.uint8)
sq[8, 99] = 0  # (the read on the text's last 100 characters: an A on the last site)
ln = np.full(len(pl), 100, dtype=np.uint16)
want, n_reads, n_adds = pile_model.expected_counts(long_text, sq, ln, pl)
ctx.pile_records(sq, ln, pl)
assert np.array_equal(ctx.pile_counts(0, n_long), want) and ctx.pile_stats()[:2] == (n_reads, n_adds) and n_reads == len(pl) - 1 and want[-1].sum() == 1

seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(sys.argv[1], "pad_bub.fq")))
seqs, lens = np.concatenate([seqs, seqs[:330]]), np.concatenate([lens, lens[:330]])
ctx.set_text(pile_model.codes(text))  # (a second call replaces the text and forgets the index)
n_sites = ctx.pile_begin()
assert n_sites == len(pile_model.sites(text)) == 2454
ctx.set_sa(b.SA)
ctx.set_loci(start, end, bub_of, recs)
ctx.set_bubble_chrom(chrom)
p = bw.params(["-n", "3"])

# the model fed the oracle's hits: placement records, lift records of the primaries, join records (-X 5)
data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(["-n", "3"]))
reads = oracle_lib.parse_aln(data)
places, _ = map_model.expected_places(orc, idx, reads, 6)
loci = pad_model.expected_loci(places, start, end, bub_of, bubbles)
kinds, lrecs = lift_model.expected_records(places, loci, np.zeros(len(places) + 1, dtype=np.uint64), np.zeros(0, dtype=bw.ALT_DTYPE), [], bubbles, chrom)
off, alts, _ = alt_model.expected_alts(reads, 5, alt_model.OracleSA(orc, idx))
joins, _ = join_model.expected_joins(places, off, alts, join_model.suboptimal(reads, off, alts), start, end, bub_of, bubbles, chrom, 6)
MODES = {"plain": (False, False, 0), "plain, MAPQ 37": (False, False, 37), "lifted": (True, False, 0), "joined, MAPQ 37": (False, True, 37), "lifted and joined, MAPQ 37": (True, True, 37)}


def want_of(lo, hi, lifted, joined, min_mapq):
    return pile_model.expected_counts(text, seqs[lo:hi], lens[lo:hi], places[lo:hi], kinds[lo:hi] if lifted else None, lrecs[lo:hi] if lifted else None, starts,
                                      joins["mapq"][lo:hi] if joined else None, min_mapq)


wants = {m: want_of(0, len(lens), *MODES[m]) for m in MODES}
assert len({w[0].tobytes() for w in wants.values()}) == len(MODES)  # every mode has a table of its own

# one batch per mode (a submission is piled once)
for m, (lifted, joined, q) in MODES.items():
    ctx.pile_reset()
    ctx.align(p, seqs, lens)
    counted = ctx.batch_pile(6, 5, lifted, joined, q)
    want, n_reads, n_adds = wants[m]
    got = ctx.pile_counts(0, n_sites)
    assert np.array_equal(got, want), (m, np.flatnonzero((got != want).any(axis=1))[:5])
    assert counted == n_reads and ctx.pile_stats()[:2] == (n_reads, n_adds) and ctx.pile_stats()[2] > 0, (m, counted, ctx.pile_stats(), n_reads, n_adds)
    assert ctx.batch_pile(6, 5, lifted, joined, q) == 0 and ctx.batch_pile(6, 5, not lifted, joined, 0) == 0
    assert np.array_equal(ctx.pile_counts(0, n_sites), want), m
assert bw.aln_bytes(*ctx.result()) == data

# streamed, with parked reads: slot_pile before slot_md / slot_result on even slots and after them on odd ones, and once more behind them
cuts = list(range(0, len(lens), 97)) + [len(lens)]
assert len(cuts) - 1 > bw.MAX_SLOTS
for m in ("lifted and joined, MAPQ 37", "plain"):
    lifted, joined, q = MODES[m]
    ctx.pile_reset()
    seen = counted = 0

    def collect(j):
        global seen, counted
        slot, (lo, hi) = j % bw.MAX_SLOTS, (cuts[j], cuts[j + 1])
        if slot % 2 == 0:
            got = ctx.slot_pile(slot, 6, 5, lifted, joined, q)
            ctx.slot_md(slot, 6, 5, lifted)
            ctx.slot_result(slot)
        else:
            ctx.slot_result(slot)
            ctx.slot_md(slot, 6, 5, lifted)
            got = ctx.slot_pile(slot, 6, 5, lifted, joined, q)
        _, n_reads, n_adds = want_of(lo, hi, lifted, joined, q)
        assert got == n_reads and ctx.pile_stats()[:2] == (n_reads, n_adds), (m, j, got, n_reads)
        assert ctx.slot_pile(slot, 6, 5, lifted, joined, q) == 0 and ctx.slot_pile(slot, 6, 5, False, False, 0) == 0, j
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
    got = ctx.pile_counts(0, n_sites)
    assert seen == len(cuts) - 1 and counted == n_reads
    assert np.array_equal(got, want), (m, "streamed", np.flatnonzero((got != want).any(axis=1))[:5])  # the table of the one batch
assert ctx.stats().n_parked_reads > 0
ctx.close()
print(f"PILE-SLOTS-OK {seen} chunks, {counted} reads counted, {os.path.basename(bw.LIB_PATH)}")
