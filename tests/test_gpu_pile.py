"""Allele counts at the text's IUPAC sites (`bwbble map -A`, kernels k_site_count / k_site_add / k_site_of / k_pile) on the GPU, judged by
tests/pile_model.py: the site index at every position of a constructed text; Context.pile_records on injected records - every read base on every
text code at both parities, windows at every offset of a 32-character word, read lengths up to 255, CIGARs with up to eight gap runs, both strands,
lifted records, MAPQ thresholds -; 70 000 reads on one site; more reads than twice the grid's lanes; the pad_bub reads in one batch and streamed
through the slots (tests/pile_slots_worker.py); the state and argument errors; and the command line against the model's bytes and against `align`
+ `aln2sam -A`."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bwbble_amd as bw
import lift_model
import md_model
import pad_model
import pile_model
from test_gpu_join import VARIANTS, model, pad_text, toy_tables  # noqa: F401 (fixtures)
from test_gpu_map import cli, compute_units
from test_gpu_md import base_texts, cases, md_dir, tagged, toy  # noqa: F401 (fixtures, and the shapes of the md tests)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, S = bw.LIFT_M, bw.LIFT_I, bw.LIFT_D, bw.LIFT_S
Q = 20  # the MAPQ threshold of the injected records: their own MAPQ is Q - 1, Q or Q + 1


@pytest.fixture(scope="module")
def text():
    """3 201 characters in two records, no multiple of 32: the first and the last character are sites; word 3 has sites at nibbles 0, 7, 8, 15, 16
    and 31 only, word 4 has 32 sites, word 5 none; every code beside every other at both parities; `$` at an even and at an odd position"""
    rng = np.random.default_rng(16)
    body = "".join(rng.choice(list("ACGT" * 8 + md_model.LETTERS[1:]), 3000 - 47))
    t = "K" + md_model.LETTERS[1:] * 3 + body + "$"
    w3 = "".join("K" if k in (0, 7, 8, 15, 16, 31) else "ACGT"[k % 4] for k in range(32))
    t = t[:96] + w3 + ("KSBYMHVRDW" * 4)[:32] + "ACGT" * 8 + t[192:]
    t = t[:1400] + "$" + t[1401:]
    t = t + "ACGT" * 50 + "W"
    assert len(t) == 3201 and len(t) % 32 and t[1400] == t[2999] == "$" and t[0] in pile_model.SITE_LETTERS and t[-1] in pile_model.SITE_LETTERS
    return t


@pytest.fixture(scope="module")
def ctx(built, golden, text):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    c.set_text(pile_model.codes(text))
    c.n_sites = c.pile_begin()
    h = text.index("$") + 1
    c.set_loci(np.array([0, h], dtype=np.uint64), np.array([h - 1, len(text) - 1], dtype=np.uint64), np.array([-1, -1], dtype=np.int32), np.zeros(0, dtype=bw.BUBBLE_DTYPE))
    c.starts = [0, h]
    yield c
    c.close()


def test_site_index_at_every_position(ctx, text, golden):
    want = pile_model.site_of(text)
    assert ctx.n_sites == len(pile_model.sites(text)) == int(want.max()) + 1 > 500
    words = [[k for k in range(32) if 32 * w + k < len(text) and text[32 * w + k] in pile_model.SITE_LETTERS] for w in range((len(text) + 31) // 32)]
    assert words[3] == [0, 7, 8, 15, 16, 31] and len(words[4]) == 32 and words[5] == [] and want[0] == 0 and want[-1] == ctx.n_sites - 1
    got = ctx.pile_site_of(np.arange(len(text)))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    rng = np.random.default_rng(1)
    some = rng.integers(0, len(text), 100_000)  # more queries than one pass of the grid
    assert np.array_equal(ctx.pile_site_of(some), want[some])
    assert len(ctx.pile_site_of(np.zeros(0, dtype=np.uint64))) == 0
    with pytest.raises(bw.BwbError, match="error -1.*outside the text"):
        ctx.pile_site_of([len(text)])
    # a text with no site: nothing to count, and every position says so
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    try:
        plain = "ACGTN$" * 100 + "ACG"
        c.set_text(pile_model.codes(plain))
        assert c.pile_begin() == 0
        assert (c.pile_site_of(np.arange(len(plain))) == -1).all()
        c.pile_records(np.zeros((3, 50), dtype=np.uint8), np.full(3, 50, dtype=np.uint16), lift_model.place_records([(5, False, "50M"), (100, True, "50M"), (553, False, "50M")]))
        assert c.pile_stats()[:2] == (3, 0) and c.pile_counts(0, 0).shape == (0, 4)
        with pytest.raises(bw.BwbError, match="error -1.*pile_counts"):
            c.pile_counts(0, 1)
    finally:
        c.close()


def records(ctx, text, cs):
    """the cases of the md tests on both strands, a few of them unmapped, with MAPQ Q - 1, Q and Q + 1 -> what pile_records takes, and the python lift records"""
    rows = [(c, rev) for c in cs for rev in (False, True)]
    seqs, lens = np.full((len(rows), 255), 4, dtype=np.uint8), np.zeros(len(rows), dtype=np.uint16)
    placed, kinds, lrecs = [], np.zeros(len(rows), dtype=np.uint8), [None] * len(rows)
    for r, ((start, cig, seq, lops), rev) in enumerate(rows):
        up = seq[::-1].translate(md_model.COMP) if rev else seq
        seqs[r, :len(up)], lens[r] = ["AGCTN".index(c) for c in up], len(up)
        if lops is None:
            placed.append((start, rev, cig))
        else:  # (the placement itself lies somewhere else: on a bubble record)
            placed.append((7, rev, f"{len(seq)}M"))
            seqid = 1 if start >= ctx.starts[1] else 0
            kinds[r], lrecs[r] = bw.LIFT_LIFTED, (start - ctx.starts[seqid] + 1, seqid, lops)
    places = lift_model.place_records(placed)
    places["flags"][::37] = 0
    places["mapq"] = Q - 1 + (np.arange(len(rows)) // 2) % 3  # (both strands of a case share it)
    return rows, seqs, lens, places, kinds, lrecs


@pytest.fixture(scope="module")
def injected(ctx, text):
    return records(ctx, text, cases(text))


def counts_of(ctx):
    return ctx.pile_counts(0, ctx.n_sites)


def test_pile_records_equals_the_model_on_injected_records(ctx, text, injected):
    rows, seqs, lens, places, kinds, lrecs = injected
    lift = md_model.pack_lift(kinds, lrecs)
    override = ((places["mapq"].astype(np.int64) - (Q - 1) + 1) % 3 + Q - 1).astype(np.uint8)  # another of Q - 1, Q, Q + 1 for every read
    total = np.zeros((ctx.n_sites, 4), dtype=np.uint32)
    for min_mapq, mapq in ((0, None), (Q, None), (Q + 1, None), (Q, override), (Q - 1, override)):
        want, reads, adds = pile_model.expected_counts(text, seqs, lens, places, kinds, lrecs, ctx.starts, mapq, min_mapq)
        ctx.pile_reset()
        ctx.pile_records(seqs, lens, places, *lift, mapq=mapq, min_mapq=min_mapq)
        got = counts_of(ctx)
        assert np.array_equal(got, want), (min_mapq, mapq is not None, np.flatnonzero((got != want).any(axis=1))[:5])
        n_reads, n_adds, ms = ctx.pile_stats()
        assert (n_reads, n_adds) == (reads, adds) and ms > 0 and adds == int(want.sum())
        total += want
        if min_mapq == 0:
            everyone = (want, reads)
    # the thresholds bite: Q - 1 is left out at Q, Q at Q + 1, and the override stands in for the record's own
    by_mapq = [pile_model.expected_counts(text, seqs, lens, places, kinds, lrecs, ctx.starts, None, q)[1] for q in (Q - 1, Q, Q + 1, Q + 2)]
    assert by_mapq[0] == everyone[1] > by_mapq[1] > by_mapq[2] > by_mapq[3] == 0
    assert pile_model.expected_counts(text, seqs, lens, places, kinds, lrecs, ctx.starts, override, Q)[0].tolist() != pile_model.expected_counts(text, seqs, lens, places, kinds, lrecs, ctx.starts, None, Q)[0].tolist()
    # what the cases cover: all 5 x 16 pairs of a read base and a text code at even and at odd text positions, on either strand, under an M of a read that counts;
    # reads of 1..255 bases; lifted records with I, S and D; the long gaps, unmapped reads and a read N on a site contribute nothing
    placements = pile_model.record_placements(seqs, lens, places, kinds, lrecs, ctx.starts)
    mapped = np.flatnonzero(places["flags"] & bw.PLACE_MAPPED)
    assert len(placements) == len(mapped)
    for strand in (False, True):
        covered = set()
        for r, (start, ops, seq, _) in zip(mapped, placements):
            if rows[r][1] == strand and md_model.md(text, start, ops, seq)[0] == md_model.OK:
                i, t = 0, start
                for n, op in ops:
                    if op == "M":
                        covered |= {(seq[i + k], text[t + k], (t + k) & 1) for k in range(n)}
                    i += n if op in "MIS" else 0
                    t += n if op in "MD" else 0
        assert covered == {(b, c, par) for b, c in md_model.ALL_PAIRS for par in (0, 1)}, (strand, sorted({(b, c, par) for b, c in md_model.ALL_PAIRS for par in (0, 1)} - covered)[:8])
    assert set(lens.tolist()) >= {1, 2, 31, 32, 33, 100, 255}
    lifted_ops = {op for r in mapped if kinds[r] == bw.LIFT_LIFTED for _, op in lrecs[r][2]}
    assert lifted_ops >= {M, I, D, S} and any(n == (1 << 28) - 1 for r in mapped if kinds[r] == bw.LIFT_LIFTED for n, _ in lrecs[r][2])
    assert any(seq[i] == "N" and text[start + i] in pile_model.SITE_LETTERS for start, ops, seq, _ in placements if ops == [(len(seq), "M")] and 0 <= start and start + len(seq) <= len(text) for i in range(len(seq)))
    assert everyone[1] < len(mapped) < len(rows)
    # without the lift arguments the lifted reads are walked where their own records say
    ctx.pile_reset()
    ctx.pile_records(seqs, lens, places)
    assert np.array_equal(counts_of(ctx), pile_model.expected_counts(text, seqs, lens, places)[0])


def test_two_calls_accumulate_reset_zeroes_and_sub_ranges(ctx, text, injected):
    rows, seqs, lens, places, kinds, lrecs = injected
    lift = md_model.pack_lift(kinds, lrecs)
    want = pile_model.expected_counts(text, seqs, lens, places, kinds, lrecs, ctx.starts)[0]
    half = len(lens) // 2 // 2 * 2
    ctx.pile_reset()
    assert not counts_of(ctx).any()
    ctx.pile_records(seqs[:half], lens[:half], places[:half])
    first = counts_of(ctx)
    assert np.array_equal(first, pile_model.expected_counts(text, seqs[:half], lens[:half], places[:half])[0]) and first.any()
    ctx.pile_records(seqs, lens, places, *lift)
    assert np.array_equal(counts_of(ctx), first + want)
    ctx.pile_records(seqs[:0], lens[:0], places[:0])  # (no read: no launch, nothing changes)
    assert np.array_equal(counts_of(ctx), first + want)
    n = ctx.n_sites
    for lo, k in ((0, 1), (0, 7), (n - 1, 1), (n - 9, 9), (n, 0), (0, 0), (n // 2, 33)):
        assert np.array_equal(ctx.pile_counts(lo, k), (first + want)[lo:lo + k]), (lo, k)
    for lo, k in ((0, n + 1), (n, 1), (n + 1, 0), (1, n), ((1 << 64) - 1, 2)):
        with pytest.raises(bw.BwbError, match="error -1.*pile_counts"):
            ctx.pile_counts(lo, k)
    ctx.pile_reset()
    assert not counts_of(ctx).any()


def test_seventy_thousand_reads_on_one_site(ctx, text):
    """every read's span covers the site at position 96 (the first nibble of word 3): its counter is exactly 70 000, split by base as the model says -
    what an add that is not atomic loses"""
    site = 96
    assert text[site] == "K"
    rng = np.random.default_rng(3)
    templates = []
    for k in range(70):
        ln = 33 + k % 5
        start = site - (k * 7) % ln
        templates.append((start, bool(k & 1), f"{ln}M", "".join(rng.choice(list("ACGT"), ln))))
    times = 1000
    seqs, lens = np.full((70, 40), 4, dtype=np.uint8), np.zeros(70, dtype=np.uint16)
    for r, (start, rev, cig, seq) in enumerate(templates):
        up = seq[::-1].translate(md_model.COMP) if rev else seq
        seqs[r, :len(up)], lens[r] = ["AGCTN".index(c) for c in up], len(up)
    places = lift_model.place_records([(s, rev, cig) for s, rev, cig, _ in templates])
    want, reads, adds = pile_model.expected_counts(text, seqs, lens, places)
    k = int(pile_model.site_of(text)[site])
    assert reads == 70 and want[k].sum() == 70 and (want[k] > 0).all()
    ctx.pile_reset()
    ctx.pile_records(np.tile(seqs, (times, 1)), np.tile(lens, times), np.tile(places, times))
    got = counts_of(ctx)
    assert got[k].sum() == 70_000 and np.array_equal(got[k], want[k] * times)
    assert np.array_equal(got, want * times) and ctx.pile_stats()[:2] == (70_000, adds * times)


def test_pile_records_strides_over_twice_the_lanes_of_the_grid(ctx, text, injected):
    """more than twice 8 * CUs * 256 reads - the short ones of the injected records, 33 bytes apart -, so that every lane takes a third"""
    rows, seqs, lens, places, kinds, lrecs = injected
    short = np.flatnonzero((lens <= 33) & (kinds == 0))
    seqs, lens, places = np.ascontiguousarray(seqs[short, :33]), lens[short], places[short]
    want, reads, adds = pile_model.expected_counts(text, seqs, lens, places, min_mapq=Q)
    lanes = 8 * compute_units() * 256
    times = 2 * lanes // len(lens) + 1
    assert times * len(lens) > 2 * lanes and reads > 100 and adds > 100
    ctx.pile_reset()
    ctx.pile_records(np.tile(seqs, (times, 1)), np.tile(lens, times), np.tile(places, times), min_mapq=Q)
    assert np.array_equal(counts_of(ctx), want * np.uint32(times)) and ctx.pile_stats()[:2] == (reads * times, adds * times)


def test_md_pile_and_pile_q_walk_the_same_reads_at_the_edges_of_the_gate(built, golden, text, ctx, injected):
    """k_md_count, k_pile and k_pile_q share one gate (md_gate): the reads md_records calls MD_OK are the reads pile_records and pile_records_q
    count.  The injected reads of 1..255 bases and the lifted ones, plus records on every edge of the gate, each on both strands: a span of
    MD_MAX_SPAN and one more, the last text character reached and passed by one, ops that consume one base less and one more than the read has,
    lift headers with 0 and 21 ops, a record number that is the table's size, a lift record one word short of its ops, an unmapped read.  All
    of the refused ones are refused before a text or read byte is fetched: the header's fields and the ops' sums alone decide."""
    import pileq_model
    from test_gpu_md import read_for
    rows, seqs, lens, places, kinds, lrecs = injected
    keep = [r for r, ((start, cig, seq, lops), _) in enumerate(rows) if lops is not None or (start == 600 and cig == f"{len(seq)}M")]
    assert {1, 255} <= set(lens[keep].tolist()) and (kinds[keep] == bw.LIFT_LIFTED).any() and (kinds[keep] == 0).any()
    n, h, rng, span = len(text), ctx.starts[1], np.random.default_rng(9), bw.MD_MAX_SPAN
    m50 = [(50, "M")]
    edges = [("unmapped", (300, "50M", read_for(text, 300, m50, rng), None)),
             ("span 4096", (100, None, "ACGT" * 5, [(10, M), (span - 20, D), (10, M)])),
             ("span 4097", (100, None, "ACGT" * 5, [(10, M), (span - 19, D), (10, M)])),
             ("ends at the text's end", (n - 50, "50M", read_for(text, n - 50, m50, rng), None)),
             ("ends one past it", (n - 49, "50M", "ACGT" * 12 + "AC", None)),
             ("lifted, ends at the text's end", (n - 40, None, read_for(text, n - 40, [(10, "M"), (20, "D"), (10, "M")], rng), [(10, M), (20, D), (10, M)])),
             ("lifted, ends one past it", (n - 39, None, "ACGT" * 5, [(10, M), (20, D), (10, M)])),
             ("ops one base short", (300, "49M", "ACGT" * 12 + "AC", None)),
             ("ops one base over", (300, "51M", "ACGT" * 12 + "AC", None)),
             ("lifted, ops one base short", (300, None, "ACGT" * 12 + "AC", [(49, M)])),
             ("lifted, ops one base over", (300, None, "ACGT" * 12 + "AC", [(51, M)])),
             ("header with no op", (300, None, "ACGT" * 5, [])),
             ("header with 21 ops", (300, None, read_for(text, 300, [(42, "M")], rng), [(2, M)] * 21)),
             ("record number n_seq", (300, None, read_for(text, 300, m50, rng), [(50, M)])),
             ("lifted, as it should be", (h + 300, None, read_for(text, h + 300, m50, rng), [(20, M), (30, M)])),
             ("one word short", (300, None, read_for(text, 300, m50, rng), [(10, M)] * 5))]
    names = [name for name, _ in edges for _ in (False, True)]
    _, e_seqs, e_lens, e_places, e_kinds, e_lrecs = records(ctx, text, [c for _, c in edges])
    e_places["flags"] |= bw.PLACE_MAPPED  # (records() leaves a few unmapped by their row number: here the one that says so is)
    seqs, lens, places = np.concatenate([seqs[keep], e_seqs]), np.concatenate([lens[keep], e_lens]), np.concatenate([places[keep], e_places])
    kinds, lrecs = np.concatenate([kinds[keep], e_kinds]), [lrecs[r] for r in keep] + e_lrecs
    at = {name: [len(keep) + i for i, nm in enumerate(names) if nm == name] for name in dict(edges)}
    assert len(lens) < 100 and all(len(v) == 2 for v in at.values())
    for r in at["record number n_seq"]:
        lrecs[r] = (lrecs[r][0], 2, lrecs[r][2])
    for r in at["unmapped"]:
        places["flags"][r] = 0
    k_arr, off, words = md_model.pack_lift(kinds, lrecs)
    for r in sorted(at["one word short"], reverse=True):  # (three words each: the header and five ops; the last is taken away)
        assert int(off[r + 1] - off[r]) == 3
        words = np.delete(words, int(off[r + 1]) - 1, axis=0)
        off[r + 1:] -= 1
    assert int(off[-1]) == len(words)
    # what the model is told: a lift record that does not fit its own words, has no or too many ops or names no record of the table is walked by nobody
    nobody = at["header with 21 ops"] + at["record number n_seq"] + at["one word short"] + at["header with no op"]
    told = places.copy()
    told["flags"][nobody] = 0
    want = md_model.expected_records(text, seqs, lens, told, kinds, lrecs, ctx.starts)
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    try:
        c.set_text(pile_model.codes(text))
        n_sites = c.pile_begin()
        c.pileq_begin()
        c.set_loci(np.array([0, h], dtype=np.uint64), np.array([h - 1, n - 1], dtype=np.uint64), np.array([-1, -1], dtype=np.int32), np.zeros(0, dtype=bw.BUBBLE_DTYPE))
        got = c.md_records(seqs, lens, places, k_arr, off, words)
        assert md_model.compare_records(got, want) is None, md_model.compare_records(got, want)
        kind = got[0]["kind"]
        ok = np.flatnonzero(kind == bw.MD_OK)
        for name, rs in at.items():
            expect = bw.MD_TOO_LONG if name == "span 4097" else bw.MD_OK if name in ("ends at the text's end", "lifted, ends at the text's end", "lifted, as it should be") else bw.MD_NONE
            assert kind[rs].tolist() == [expect, expect], (name, kind[rs])
        assert len(ok) > 20 and len(lens) - len(ok) >= 30
        # the model over exactly the reads of kind MD_OK: it counts every one of them, and the kernels count those and no other
        sub = (seqs[ok], lens[ok], places[ok], kinds[ok], [lrecs[r] for r in ok], ctx.starts)
        counts, reads, adds = pile_model.expected_counts(text, *sub)
        assert reads == len(ok) and adds > 100
        c.pile_records(seqs, lens, places, k_arr, off, words, min_mapq=0)
        assert c.pile_stats()[:2] == (len(ok), adds) and np.array_equal(c.pile_counts(0, n_sites), counts)
        quals = np.full(seqs.shape, ord("I"), dtype=np.uint8)
        counts_q, _, reads_q, adds_q, dropped = pileq_model.expected_q(text, seqs[ok], quals[ok], *sub[1:])
        assert (reads_q, adds_q, dropped) == (len(ok), adds, 0) and np.array_equal(counts_q, counts)
        c.pile_reset()
        c.pile_records_q(seqs, quals, lens, places, k_arr, off, words, min_mapq=0)
        assert c.pileq_stats()[:3] == (len(ok), adds, 0) and np.array_equal(c.pile_counts(0, n_sites), counts)
        assert c.pile_stats()[:2] == (len(ok), adds)  # (the plain form's figures: its own last launch)
        # the context is usable afterwards
        c.pile_reset()
        c.pile_records(seqs[ok], lens[ok], places[ok], *md_model.pack_lift(kinds[ok], sub[4]))
        assert c.pile_stats()[:2] == (len(ok), adds) and np.array_equal(c.pile_counts(0, n_sites), counts)
    finally:
        c.close()


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_pile_and_slot_pile_equal_the_model_fed_the_oracles_hits(built, pad_text, lib):
    """a text uploaded in two chunks by the test build, its site index at every position; the pad_bub reads in one batch - plain, lifted, joined -
    and through all eight slots with parked reads: the same table, the model's"""
    env = dict(os.environ, BWB_SLICE_ITERS="150")
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pile_slots_worker.py"), pad_text], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PILE-SLOTS-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


def test_pile_errors_leave_the_context_usable(built, golden, pad_text, toy_tables, toy):
    t = toy_tables
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    c = bw.Context(b)
    one = (seqs[:1], lens[:1], lift_model.place_records([(5, False, f"{int(lens[0])}M")]))
    lifted_one = md_model.pack_lift([bw.LIFT_LIFTED], [(6, 0, [(int(lens[0]), M)])])
    plain_calls = (lambda: c.batch_pile(), lambda: c.slot_pile(0))
    lifted_calls = (lambda: c.batch_pile(6, 5, True), lambda: c.slot_pile(0, 6, 5, True), lambda: c.batch_pile(6, 5, False, True), lambda: c.slot_pile(0, 6, 5, False, True))
    try:
        with pytest.raises(bw.BwbError, match="error -4.*set_text"):
            c.pile_begin()
        c.set_text(pile_model.codes(toy.text))
        for call in plain_calls + lifted_calls + (lambda: c.pile_records(*one), lambda: c.pile_counts(0, 0), lambda: c.pile_reset(), lambda: c.pile_site_of([0])):
            with pytest.raises(bw.BwbError, match="error -4.*pile_begin"):
                call()
        n_sites = c.pile_begin()
        assert n_sites == 2454 == len(pile_model.sites(toy.text))
        c.align(bw.params(["-n", "3"]), seqs, lens)
        assert c.pile_stats() == (0, 0, 0.0)
        c.pile_records(*one)  # (needs no SA and no batch)
        want_one = pile_model.expected_counts(toy.text, *one)[0]
        assert np.array_equal(c.pile_counts(0, n_sites), want_one) and c.pile_stats()[0] == 1
        for call in plain_calls + lifted_calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
                call()
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            c.pile_records(*one, *lifted_one)
        c.set_sa(b.SA)
        for call in lifted_calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
                call()
        c.set_loci(t.start, t.end, t.bub_of, t.recs)
        for call in lifted_calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
                call()
        c.set_bubble_chrom(t.chrom)
        with pytest.raises(bw.BwbError, match="error -4.*max_alt"):
            c.batch_pile(6, 0, False, True)
        for bad in (lambda: c.batch_pile(6, 5, False, False, 256), lambda: c.batch_pile(6, 5, False, False, -1), lambda: c.slot_pile(0, 6, 256), lambda: c.slot_pile(0, 6, -1),
                    lambda: c.slot_pile(-1), lambda: c.slot_pile(bw.MAX_SLOTS), lambda: c.pile_records(*one, min_mapq=256)):
            with pytest.raises(bw.BwbError, match="error -1"):
                bad()
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            c.slot_pile(3)
        two = (seqs[:2], lens[:2], lift_model.place_records([(5, False, "100M")] * 2))
        for bad_off in ([1, 2, 2], [0, 2, 1]):
            with pytest.raises(bw.BwbError, match="error -1.*pile_records"):
                c.pile_records(*two, np.array([1, 0], dtype=np.uint8), np.array(bad_off, dtype=np.uint64), lifted_one[2][:bad_off[-1]])
        # none of that has counted anything; a lift record of a record the table does not have, or one that does not fit its words, counts nothing either
        for seqid, n_ops in ((len(t.start), 1), (0, 9)):
            words = lifted_one[2].copy()
            words[0][2], words[0][3] = seqid, n_ops
            c.pile_records(*one, lifted_one[0], lifted_one[1], words)
            assert c.pile_stats()[:2] == (0, 0)
        assert np.array_equal(c.pile_counts(0, n_sites), want_one)
        c.pile_reset()
        counted = c.batch_pile()
        assert counted == 569 == c.pile_stats()[0] and c.pile_counts(0, n_sites).sum() == c.pile_stats()[1] == 556
        assert c.batch_pile() == 0 and c.batch_pile(6, 5, True, True) == 0 and c.pile_counts(0, n_sites).sum() == 556  # (a submission is piled once)
        c.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            c.batch_pile()
        c.run()
        assert 0 < c.batch_pile(6, 5, True, True) <= 10
        # a later set_text forgets the index and the counters
        c.set_text(pile_model.codes(toy.text))
        with pytest.raises(bw.BwbError, match="error -4.*pile_begin"):
            c.pile_counts(0, 0)
        assert c.pile_begin() == n_sites and not c.pile_counts(0, n_sites).any()
    finally:
        c.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def want_tsv(base, toy, min_mapq=0):
    table, reads, adds = pile_model.pile_sam(base, toy.text, toy.names, toy.starts, min_mapq)
    return pile_model.tsv(toy.text, toy.names, toy.starts, table), reads, adds


@pytest.mark.parametrize("variant", ["one_chunk", "chunks_of_97", "two_workers", "four_workers"])
def test_cli_map_with_counts_writes_the_models_bytes(md_dir, golden, pad_text, model, toy_tables, toy, variant):
    extra, env = dict(VARIANTS, four_workers=(["-g", "4"], {"BWB_DEVICE_MAP": "0,0,0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}))[variant]
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    out, counts = md_dir / f"pile_{variant}.sam", md_dir / f"pile_{variant}.tsv"
    # map -n 3 -A f
    base = base_texts(model, pad_text, toy_tables)["plain"][1]
    log = cli(["map", "-n", "3", "-A", counts] + extra + [md_dir / "toy.fa", fq, out], env)
    want, reads, adds = want_tsv(base, toy)
    assert open(counts, "rb").read() == want and open(out, "rb").read() == base
    assert f"allele counts at the text's IUPAC sites on the GPU: sites 2454  reads counted {reads}  adds {adds} " in log and reads == 569
    # map -n 3 -X 5 -B t -J -R -D -A f -a 1
    opts, base = base_texts(model, pad_text, toy_tables)["XBJR"]
    opts = [data if o == "DATA" else o for o in opts]
    log = cli(["map", "-n", "3"] + opts + ["-D", "-A", counts, "-a", "1"] + extra + [md_dir / "toy.fa", fq, out], env)
    want1, reads1, adds1 = want_tsv(base, toy, 1)
    assert open(counts, "rb").read() == want1 and open(out, "rb").read() == tagged(base, toy)[0]
    assert f"reads counted {reads1}  adds {adds1} " in log and 0 < reads1 <= reads and want1 != want
    # and without -A: nothing built, uploaded or launched
    log = cli(["map", "-n", "3"] + extra + [md_dir / "toy.fa", fq, out], env)
    assert open(out, "rb").read() == base_texts(model, pad_text, toy_tables)["plain"][1] and "allele counts" not in log


def test_cli_align_then_aln2sam_with_counts(md_dir, golden, pad_text, model, toy_tables, toy, tmp_path):
    fa, fq, aln, out = md_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "t.aln", tmp_path / "t.sam"
    cli(["align", "-n", "3", fa, fq, aln])
    for key, more in (("plain", []), ("XBJR", ["-D"]), ("BR", []), ("XB", [])):
        opts, base = base_texts(model, pad_text, toy_tables)[key]
        opts = [os.path.join(golden, "pad_toy.data") if o == "DATA" else o for o in opts]
        for q in (1, 37):
            cli(["aln2sam"] + opts + more + ["-A", tmp_path / "a.tsv", "-a", q, fa, fq, aln, out])
            cli(["map", "-n", "3"] + opts + more + ["-A", tmp_path / "m.tsv", "-a", q, fa, fq, tmp_path / "m.sam"])
            got = open(tmp_path / "a.tsv", "rb").read()
            assert got == open(tmp_path / "m.tsv", "rb").read() == want_tsv(base, toy, q)[0], (key, q)
            assert open(out, "rb").read() == open(tmp_path / "m.sam", "rb").read() == (tagged(base, toy)[0] if more else base)


def test_cli_map_with_counts_on_records_out_of_text_order(md_dir, golden, pad_text, model, toy_tables, toy, tmp_path):
    """an .ann whose records do not ascend: with -R the lift records come from the host's rule and so do the counts, and the log says so; without
    -R the kernel needs no record table"""
    for ext in ("", ".bwt", ".ref"):
        shutil.copy(md_dir / ("toy.fa" + ext), tmp_path / ("toy.fa" + ext))
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    out, counts = tmp_path / "out.sam", tmp_path / "counts.tsv"
    opts, base = base_texts(model, pad_text, toy_tables)["XBJR"]
    opts = [os.path.join(golden, "pad_toy.data") if o == "DATA" else o for o in opts]
    log = cli(["map", "-n", "3"] + opts + ["-A", counts, "-a", "1", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    want, reads, adds = want_tsv(base, toy, 1)
    assert open(counts, "rb").read() == want
    assert f"allele counts at the text's IUPAC sites on the host (the .ann records are not ascending and disjoint): sites 2454  reads counted {reads}  adds {adds}" in log
    log = cli(["map", "-n", "3", "-A", counts, tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    assert open(counts, "rb").read() == want_tsv(base_texts(model, pad_text, toy_tables)["plain"][1], toy)[0]
    assert "allele counts at the text's IUPAC sites on the GPU: sites 2454  reads counted 569" in log
