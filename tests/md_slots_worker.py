"""Worker of tests/test_gpu_md.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the product or the TEST build.
First a text of 40 000 characters, which the test build uploads in two chunks (one for the product), with reads laid across the chunk's edge.
Then the pad_bub reads on the toy index: batch_md plain and lifted, then slot_md in chunks of 97 reads through the eight slots and round again
with every wave parked after 150 loop iterations (BWB_SLICE_ITERS, set by the test), before and after slot_lift / slot_result, against
tests/md_model.py fed the ORACLE's hits; md_stats against the model's counts.
usage: md_slots_worker.py <directory with the unpacked pad_bub files>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import join_model  # noqa: E402
import lift_model  # noqa: E402
import map_model  # noqa: E402
import md_model  # noqa: E402
import oracle_lib  # noqa: E402
import pad_model  # noqa: E402

golden = os.path.join(ROOT, "tests", "golden")
bwt = os.path.join(golden, "toy.fa.bwt")
orc = oracle_lib.load()
idx = orc.load_index(bwt, load_sa=True)
text, names, starts = md_model.fasta_text(open(os.path.join(golden, "toy.fa")).read())
_, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
anns, recs = bw.read_bubble_data(os.path.join(golden, "pad_toy.data"))
bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
bub_of = pad_model.bubble_of(names, bubbles)
chrom = join_model.chrom_of(names, bubbles)


def same(got, want, what):
    diff = md_model.compare_records(got, want)
    assert diff is None, (what, diff)


def want_of(seqs, lens, max_mm, lifted):
    """the model fed the oracle's hits -> (records, md_off, MD bytes), and the oracle's .aln bytes"""
    data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(["-n", "3"]))
    places, _ = map_model.expected_places(orc, idx, oracle_lib.parse_aln(data), max_mm)
    kinds = lrecs = None
    if lifted:
        kinds, lrecs = lift_model.expected_records(places, pad_model.expected_loci(places, start, end, bub_of, bubbles), np.zeros(len(places) + 1, dtype=np.uint64),
                                                   np.zeros(0, dtype=bw.ALT_DTYPE), [], bubbles, chrom)
    return md_model.expected_records(text, seqs, lens, places, kinds, lrecs, starts), data


b = bw.BwtFile(bwt, load_sa=True)
ctx = bw.Context(b)

# a text that the test build uploads in two chunks (2^15 characters each): reads across the edge, and on the text's last characters
rng = np.random.default_rng(40)
long_text = "".join(rng.choice(list("ACGT" * 6 + md_model.LETTERS[1:]), 40_000)) + "$"
ctx.set_text(md_model.codes(long_text))
where = [0, 31, 32, 1 << 15, (1 << 15) - 1, (1 << 15) - 50, (1 << 15) - 99, (1 << 15) - 100, len(long_text) - 100, len(long_text) - 99] + rng.integers(0, len(long_text) - 100, 200).tolist()
placed = [(int(p), bool(k & 1), "100M") for k, p in enumerate(where)]
pl = lift_model.place_records(placed)
sq = np.full((len(pl), 100), 4, dtype=np.uint8)
for r, (p, rev, _) in enumerate(placed):
    s = "".join((md_model.MEMBERS[c] or "A")[0] for c in long_text[p:p + 100]).ljust(100, "A")
    s = s[:r % 100] + "N" + s[r % 100 + 1:]
    sq[r] = ["AGCTN".index(c) for c in (s[::-1].translate(md_model.COMP) if rev else s)]
ln = np.full(len(pl), 100, dtype=np.uint16)
want = md_model.expected_records(long_text, sq, ln, pl)
same(ctx.md_records(sq, ln, pl), want, "two chunks")
assert (want[0]["kind"] == bw.MD_OK).sum() == len(pl) - 1 and want[0]["kind"][9] == bw.MD_NONE

seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(sys.argv[1], "pad_bub.fq")))
ctx.set_text(md_model.codes(text))  # (a second call replaces the text)
ctx.set_sa(b.SA)
ctx.set_loci(start, end, bub_of, recs)
ctx.set_bubble_chrom(chrom)
p = bw.params(["-n", "3"])

# one batch: -Q 6 and 3, plain and lifted (behind lift() with another max_alt and before it)
ctx.align(p, seqs, lens)
for max_mm, lifted in ((6, False), (6, True), (3, True), (3, False)):
    want, data = want_of(seqs, lens, max_mm, lifted)
    same(ctx.batch_md(max_mm, 5, lifted), want, ("batch", max_mm, lifted))
    n_ok, n_bytes, ms = ctx.md_stats()
    assert (n_ok, n_bytes) == (int((want[0]["kind"] == bw.MD_OK).sum()), len(want[2])) and ms > 0, ctx.md_stats()
    assert n_ok == 569
    same(ctx.batch_md(max_mm, 0 if lifted else 5, lifted), want, ("batch again", max_mm, lifted))
assert bw.aln_bytes(*ctx.result()) == data

# streamed, with parked reads: slot_md before slot_lift / slot_result on even slots and after them on odd ones, and once more behind them
seqs, lens = np.concatenate([seqs, seqs[:330]]), np.concatenate([lens, lens[:330]])
cuts = list(range(0, len(lens), 97)) + [len(lens)]
wants = [(want_of(seqs[lo:hi], lens[lo:hi], 6, True), want_of(seqs[lo:hi], lens[lo:hi], 6, False)[0]) for lo, hi in zip(cuts[:-1], cuts[1:])]
assert len(wants) > bw.MAX_SLOTS
seen = tagged = 0


def collect(j):
    global seen, tagged
    slot, ((want, data), plain) = j % bw.MAX_SLOTS, wants[j]
    if slot % 2 == 0:
        got = ctx.slot_md(slot, 6, 5, True)
        ctx.slot_lift(slot)
        off, alns = ctx.slot_result(slot)
    else:
        off, alns = ctx.slot_result(slot)
        ctx.slot_lift(slot)
        got = ctx.slot_md(slot, 6, 5, True)
    same(got, want, ("slot", j))
    assert ctx.md_stats()[:2] == (int((want[0]["kind"] == bw.MD_OK).sum()), len(want[2])), j
    assert bw.aln_bytes(off, alns) == data, j
    same(ctx.slot_md(slot, 6, 5, False), plain, ("slot, not lifted", j))
    same(ctx.slot_md(slot, 6, 5, True), want, ("slot again", j))
    seen += 1
    tagged += int((want[0]["kind"] == bw.MD_OK).sum())


for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
    if j >= bw.MAX_SLOTS:
        collect(j - bw.MAX_SLOTS)
    ctx.slot_upload(j % bw.MAX_SLOTS, p, seqs[lo:hi], lens[lo:hi])
    ctx.slot_submit(j % bw.MAX_SLOTS)
for j in range(max(0, len(wants) - bw.MAX_SLOTS), len(wants)):
    collect(j)
assert seen == len(wants) and tagged >= 569
assert ctx.stats().n_parked_reads > 0
ctx.close()
print(f"MD-SLOTS-OK {seen} chunks, {tagged} tagged reads, {os.path.basename(bw.LIB_PATH)}")
