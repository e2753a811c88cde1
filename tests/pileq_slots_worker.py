"""Worker of tests/test_gpu_pileq.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the product or the TEST build.
The pad_bub reads on the toy index under rewritten quality lines (tests/pileq_model.py: requal_fastq): batch_pile_q plain, lifted and joined (-X 5)
on one batch of 901 reads, then slot_quals / slot_pile_q in chunks of 97 reads through the eight slots and round again with every wave parked
after 150 loop iterations (BWB_SLICE_ITERS, set by the test), before and after slot_md / slot_result - a second slot_pile_q, and a slot_pile after
it, on the same submission add nothing - against tests/pileq_model.py fed the ORACLE's hits: the counters and the quality sums of the stream are
those of the one batch.
usage: pileq_slots_worker.py <directory with the unpacked pad_bub files>"""
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
import pile_model  # noqa: E402
import pileq_model  # noqa: E402

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

fq = os.path.join(sys.argv[1], "pad_bub.fq")
seqs, lens = bw.encode_reads(bw.read_fastq(fq))
lines = pileq_model.requal_fastq(open(fq, "rb").read(), 12)[0].split(b"\n")[3::4]  # the rewritten quality lines, in file order
assert len(lines) == len(lens) and all(len(q) == n for q, n in zip(lines, lens))
quals = np.full(seqs.shape, 255, dtype=np.uint8)
for r, q in enumerate(lines):
    quals[r, :len(q)] = np.frombuffer(q, dtype=np.uint8)
seqs, lens, quals = np.concatenate([seqs, seqs[:330]]), np.concatenate([lens, lens[:330]]), np.concatenate([quals, quals[:330]])

b = bw.BwtFile(bwt, load_sa=True)
ctx = bw.Context(b)
ctx.set_text(pile_model.codes(text))
n_sites = ctx.pile_begin()
assert n_sites == len(pile_model.sites(text)) == 2454
ctx.pileq_begin(True)
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
# (lifted, joined, min MAPQ, min base quality, err_cap)
MODES = {"plain, -b 20": (False, False, 0, 20, 0), "plain, -Y at E 93": (False, False, 0, 0, 93), "lifted, -b 1 -Y at E 4": (True, False, 0, 1, 4),
         "lifted and joined, MAPQ 37, -b 20 -Y at E 30": (True, True, 37, 20, 30)}


def want_of(lo, hi, lifted, joined, min_mapq, m, E):
    return pileq_model.expected_q(text, seqs[lo:hi], quals[lo:hi], lens[lo:hi], places[lo:hi], kinds[lo:hi] if lifted else None, lrecs[lo:hi] if lifted else None, starts,
                                  joins["mapq"][lo:hi] if joined else None, min_mapq, m, E)


def tables():
    return ctx.pile_counts(0, n_sites), ctx.pileq_sums(0, n_sites)


wants = {m: want_of(0, len(lens), *MODES[m]) for m in MODES}
assert len({w[0].tobytes() + w[1].tobytes() for w in wants.values()}) == len(MODES)  # every mode has tables of its own

# one batch per mode (a submission is piled once)
for m, (lifted, joined, q, mb, E) in MODES.items():
    ctx.pile_reset()
    ctx.upload(p, seqs, lens)
    ctx.slot_quals(0, quals)
    ctx.run()
    counted = ctx.batch_pile_q(6, 5, lifted, joined, q, mb, E)
    wc, ws, n_reads, n_adds, n_drop = wants[m]
    gc, gs = tables()
    assert np.array_equal(gc, wc), (m, np.flatnonzero((gc != wc).any(axis=1))[:5])
    assert np.array_equal(gs, ws), (m, np.flatnonzero((gs != ws).any(axis=1))[:5])
    assert counted == n_reads and ctx.pileq_stats()[:3] == (n_reads, n_adds, n_drop) and ctx.pileq_stats()[3] > 0, (m, counted, ctx.pileq_stats(), n_reads, n_adds, n_drop)
    assert ctx.batch_pile_q(6, 5, lifted, joined, q, mb, E) == 0 and ctx.batch_pile(6, 5, not lifted, joined, 0) == 0
    assert all(np.array_equal(g, w) for g, w in zip(tables(), (wc, ws))), m
assert bw.aln_bytes(*ctx.result()) == data

# streamed, with parked reads: slot_pile_q before slot_md / slot_result on even slots and after them on odd ones, and once more behind them
cuts = list(range(0, len(lens), 97)) + [len(lens)]
assert len(cuts) - 1 > bw.MAX_SLOTS
for m in ("lifted and joined, MAPQ 37, -b 20 -Y at E 30", "plain, -b 20"):
    lifted, joined, q, mb, E = MODES[m]
    ctx.pile_reset()
    seen = counted = 0

    def collect(j):
        global seen, counted
        slot, (lo, hi) = j % bw.MAX_SLOTS, (cuts[j], cuts[j + 1])
        if slot % 2 == 0:
            got = ctx.slot_pile_q(slot, 6, 5, lifted, joined, q, mb, E)
            ctx.slot_md(slot, 6, 5, lifted)
            ctx.slot_result(slot)
        else:
            ctx.slot_result(slot)
            ctx.slot_md(slot, 6, 5, lifted)
            got = ctx.slot_pile_q(slot, 6, 5, lifted, joined, q, mb, E)
        _, _, n_reads, n_adds, n_drop = want_of(lo, hi, lifted, joined, q, mb, E)
        assert got == n_reads and ctx.pileq_stats()[:3] == (n_reads, n_adds, n_drop), (m, j, got, n_reads)
        assert ctx.slot_pile_q(slot, 6, 5, lifted, joined, q, mb, E) == 0 and ctx.slot_pile(slot, 6, 5, False, False, 0) == 0, j
        seen += 1
        counted += got

    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if j >= bw.MAX_SLOTS:
            collect(j - bw.MAX_SLOTS)
        ctx.slot_upload(j % bw.MAX_SLOTS, p, seqs[lo:hi], lens[lo:hi])
        ctx.slot_quals(j % bw.MAX_SLOTS, quals[lo:hi])
        ctx.slot_submit(j % bw.MAX_SLOTS)
    for j in range(max(0, len(cuts) - 1 - bw.MAX_SLOTS), len(cuts) - 1):
        collect(j)
    wc, ws, n_reads, _, _ = wants[m]
    gc, gs = tables()
    assert seen == len(cuts) - 1 and counted == n_reads
    assert np.array_equal(gc, wc) and np.array_equal(gs, ws), (m, "streamed", np.flatnonzero((gc != wc).any(axis=1))[:5], np.flatnonzero((gs != ws).any(axis=1))[:5])  # the tables of the one batch
assert ctx.stats().n_parked_reads > 0
ctx.close()
print(f"PILEQ-SLOTS-OK {seen} chunks, {counted} reads counted, {os.path.basename(bw.LIB_PATH)}")
