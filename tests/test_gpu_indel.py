"""Ref / alt read support per indel bubble (`bwbble map -I`, kernel k_indel) on the GPU, judged by tests/indel_model.py: Context.indel_records on
injected placement records over constructed record and bubble tables - the eligibility edges, windows at every edge, D and I at and beside lo
and hi, CIGARs of up to eight gap runs, both strands, 300 bubbles that share a left flank, two chromosomes with bubbles at equal positions, a
refused bubble beside good ones, MAPQ thresholds with and without the override -; tables of 0, 1 and around every power of two up to 257
entries, one chromosome of three without any; 70 000 reads on one bubble; more reads than twice the grid's
lanes; the generated genome mapped in one batch and streamed through the slots (tests/indel_slots_worker.py); the state and argument errors;
and the command line against the model's bytes and against `align` + `aln2sam -I`."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import bwbble_amd as bw
import indel_model
import join_model
import lift_model
import pad_model
from test_gpu_join import REC_LEN, VARIANTS, model, pad_text, table, toy_tables  # noqa: F401 (fixtures)
from test_gpu_lift import gapped
from test_gpu_map import cli, compute_units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 4  # the anchor of the injected tables

# the eligibility edges at anchor 4, every shape of allele and gap, and a multi-allelic site; each of them three times, so that with table() the
# copies lie on chromosomes 0, 1 and 2 at equal positions
EDGES = [(b"e", 1000, 20, 1020, 19, 0, 3), (b"e", 1000, 20, 1025, 19, 5, 0), (b"e", 1000, 20, 1021, 30, 1, 1), (b"e", 1000, 20, 1020, 19, 0, 5),
         (b"e", 1300, W, 1304, W - 1, 0, 1), (b"e", 1300, W - 1, 1303, W - 1, 0, 1), (b"e", 1300, W, 1304, W - 2, 0, 1),
         (b"e", 1, W, 5, 10, 0, 1), (b"e", 0, W, 4, 10, 0, 1), (b"e", 1500, 10, 1509, 10, 0, 2), (b"e", 1600, 40, 1770, 40, 130, 0),
         (b"e", 1900, 10, 1910 + (1 << 28) - 1, 10, 0, 0), (b"e", 2000, 10, 2010 + (1 << 28), 10, 0, 0), (b"e", 2100, 10, 2110, 10, 0, -1)]


@pytest.fixture(scope="module")
def bubbles():
    return [b for b in EDGES for _ in range(3)] + lift_model.genome()["bubbles"]


@pytest.fixture(scope="module")
def toy_ctx(built, golden):
    ctx = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    yield ctx
    ctx.close()


def relative(bubbles, seed=4):
    """[(on the bubble's record | on its chromosome, bubble, pos1, reverse, CIGAR)]: per bubble, on either record, reads whose first M lies one
    before, at and one behind lo and whose last M lies one before, at and one behind hi; D on lo, D on hi, I just inside and just outside the
    window at either end, D inside; CIGARs of one to eight gap runs over the window"""
    rng = np.random.default_rng(seed)
    out = []
    for b, bub in enumerate(bubbles):
        for own, (lo, hi) in zip((True, False), indel_model.windows(bub, W)):
            if hi - lo > 200 or lo < 1:
                lo, hi = max(lo, 1), max(lo, 1) + 30  # (a window no read can contain: reads at its lower edge, which count nothing)
            n = hi - lo + 1
            cigs = [(lo + a, f"{n - a + z}M") for a in (-1, 0, 1) for z in (-1, 0, 1) if n - a + z > 0]
            cigs += [(lo - 5, f"5M1D{n + 4}M"), (lo - 5, f"{4 + n}M1D5M"), (lo - 5, f"6M1I{n + 4}M"), (lo - 5, f"5M1I{n + 5}M"), (lo - 5, f"{4 + n}M1I6M"), (lo - 5, f"{5 + n}M1I5M"),
                     (lo - 5, f"7M1D{n + 2}M"), (lo - 5, f"4M1D{n + 5}M"), (lo - 5, f"{5 + n}M1D4M"), (lo - 3, f"2I{n + 6}M3I")]
            cigs += [(lo - 3, gapped(rng, k, n + 6)) for k in range(1, 9)] + [(lo - 30, gapped(rng, k, 90)) for k in (1, 4, 8)]
            for pos1, cig in cigs:
                if pos1 >= 1:
                    out.append((own, b, pos1, bool(rng.integers(0, 2)), cig))
    return out


def injected(t, rel, seed, mapq=None):
    """the relative placements put on the first record of their bubble, or on its chromosome's record; a few unmapped, a few in no record"""
    rng = np.random.default_rng(seed)
    first = {}
    for i in np.flatnonzero(t.bub_of >= 0):
        first.setdefault(int(t.bub_of[i]), int(i))
    placed = []
    for own, b, pos1, rev, cig in rel:
        i = first.get(b) if own else int(t.chrom[b])
        if i is not None and pos1 + 260 < REC_LEN:
            placed.append((int(t.start[i]) + pos1 - 1, rev, cig))
    placed += [(int(t.start[0]) - 1, False, "100M"), (int(t.end[-1]) + 1, True, "50M1I49M"), (int(t.end[0]) + 2, False, "30M")]
    placed = [placed[i] for i in rng.permutation(len(placed))]
    places = lift_model.place_records(placed)
    places["flags"][rng.integers(0, len(places), max(1, len(places) // 50))] = 0
    if mapq is not None:
        places["mapq"] = rng.choice(mapq, len(places))
    return places


def expected(t, bubbles, places, mapq=None, min_mapq=0, w=W):
    loci = pad_model.expected_loci(places, t.start, t.end, t.bub_of, bubbles)
    return indel_model.count(indel_model.from_records(places, loci, mapq), bubbles, t.chrom, w, min_mapq)


def load(ctx, t, bubbles, w=W):
    ctx.set_loci(t.start, t.end, t.bub_of, pad_model.bubble_records(bubbles))
    ctx.set_bubble_chrom(t.chrom)
    return ctx.indel_begin(w)


@pytest.fixture(scope="module")
def rel(bubbles):
    return relative(bubbles)


@pytest.mark.parametrize("n_seq", [1, 2, 3, 7, 8, 9, 1_300_000])
def test_indel_records_equals_the_model_on_injected_records(toy_ctx, bubbles, rel, n_seq):
    """record tables around the powers of two of k_locus's step count and one of the GRCh37 shape"""
    t = table(n_seq, len(bubbles))
    places = injected(t, rel, n_seq)
    want, reads, adds = expected(t, bubbles, places)
    n_elig = load(toy_ctx, t, bubbles)
    assert n_elig == sum(indel_model.eligible(b, W) for b in bubbles)
    assert [indel_model.eligible(b, W) for b in EDGES] == [True] * 5 + [False, False, True, False, False, True, True, False, False]
    toy_ctx.indel_records(places)
    got = toy_ctx.indel_counts(0, len(bubbles))
    assert np.array_equal(got, want), (n_seq, np.flatnonzero((got != want).any(axis=1))[:5], got[(got != want).any(axis=1)][:3], want[(got != want).any(axis=1)][:3])
    st = toy_ctx.indel_stats()
    assert st[:2] == (reads, adds) and st[2] >= adds and st[3] > 0 and adds == int(want.sum())
    if n_seq > 9:  # a record of every bubble: every class for either allele, the refused and ineligible bubbles untouched, and the copies apart
        assert (want.sum(axis=0) > 0).all() and (places["flags"] == 0).any()
        elig = np.array([indel_model.eligible(b, W) for b in bubbles])
        assert not want[~elig].any() and want[elig][:, 1].all()
        for k in (0, 3, 6, 12, 21):  # the three copies of a bubble, on chromosomes 0, 3 and 6 at equal positions: each is counted, from its own chromosome's reads
            assert want[k][0] > 0 and want[k + 1][0] > 0 and want[k + 2][0] > 0 and len({int(t.chrom[k + i]) for i in range(3)}) == 3
    if n_seq == 1:
        assert not want[:, 1].any() and not want[:, 3].any()  # one record: a chromosome, no read on a bubble record


def test_three_hundred_bubbles_share_a_left_flank(toy_ctx):
    """every one of them is a candidate of a read that begins before the flank: the loop is bounded by the table, not by a constant"""
    bubbles = [(b"m", 1000, 20, 1020 + k % 3, 30, k % 3, k % 4) for k in range(300)]
    t = table(4, len(bubbles))
    t.chrom[:] = 0
    placed = [(int(t.start[0]) + 1000, False, "60M"), (int(t.start[0]) + 1010, True, "10M1I30M"), (int(t.start[0]) + 1015, False, "5M"), (int(t.start[0]) + 900, False, "200M"),
              (int(t.start[3]) + 1010, False, "40M")] * 3
    places = lift_model.place_records(placed)
    want, reads, adds = expected(t, bubbles, places)
    assert load(toy_ctx, t, bubbles) == 300
    toy_ctx.indel_records(places)
    got = toy_ctx.indel_counts(0, 300)
    assert np.array_equal(got, want) and (want[:, 0] >= 6).all() and (want[:, 2] >= 3).all() and not want[:, 1].any()
    assert toy_ctx.indel_stats()[:3] == (reads, adds, 300 * 12)  # (the reads on chromosome 3 have no candidate; the 5M read begins at every lo and ends before every hi: a candidate each time, never counted)


def edge_bubbles(n_elig):
    """a list with exactly n_elig bubbles eligible at anchor W and, in every fourth place and behind them, bubbles that are not (a left flank one
    short; flanks that overlap: refused); with table() bubble b lies on chromosome record 3 * (b % 3), at a position that ascends with b // 3"""
    out, made = [], 0
    while made < n_elig or len(out) < 2:
        A, k = 200 + 20 * (len(out) // 3), len(out)
        if k % 4 == 1 or made == n_elig:
            out.append((b"x", A, W - 1, A + W - 1, 9, 0, 1) if k % 8 == 1 else (b"x", A, 10, A + 9, 9, 0, 2))
        else:
            out.append((b"t", A, 10, A + 10 + made % 2, 9, made % 2, 1 + made % 3))
            made += 1
    return out


def edge_reads(t, bubbles, seed):
    """per chromosome record 0, 3 and 6, on alternating strands: with entries - a read that begins before the first entry's lo, one whose window is
    the first entry's and one whose window is the last entry's, one behind the last entry, one that spans the last entry, a CIGAR of three gap runs
    over the first window, one with a D inside it, and reads of 250 positions over the whole stretch; without entries - reads where the other
    chromosomes have theirs"""
    rng = np.random.default_rng(seed)
    by_chrom = {}
    for k, b in enumerate(bubbles):
        if indel_model.eligible(b, W):
            by_chrom.setdefault(int(t.chrom[k]), []).append(indel_model.windows(b, W)[1])
    placed, census = [], {"chromosomes with entries": 0, "without": 0}

    def put(rec, pos1, cig):
        placed.append((int(t.start[rec]) + pos1 - 1, len(placed) % 2 == 1, cig))

    for rec in (0, 3, 6):
        wins = sorted(by_chrom.get(rec, []))
        for pos1 in range(1, 200 + 20 * (len(bubbles) // 3) + 60, 200):
            put(rec, pos1, "250M")
        if not wins:
            census["without"] += 1
            put(rec, 191, "60M")
            put(rec, 206, "9M")
            continue
        census["chromosomes with entries"] += 1
        (lo0, hi0), (lo1, hi1) = wins[0], wins[-1]
        put(rec, lo0 - 5, "60M")
        put(rec, lo0, f"{hi0 - lo0 + 1}M")
        put(rec, lo1, f"{hi1 - lo1 + 1}M")
        put(rec, hi1 + 1, "50M")
        put(rec, lo1 - 20, "60M")
        put(rec, lo0 - 3, gapped(rng, 3, hi0 - lo0 + 7))
        put(rec, lo0 - 5, "7M1D50M")  # (a D inside the first window: gapped, whatever the CIGAR before drew)
    return lift_model.place_records(placed), census


@pytest.mark.parametrize("none_on_record_3", [False, True])
@pytest.mark.parametrize("n_tab", [0, 1, 2, 3, 4, 7, 8, 9, 255, 256, 257])
def test_table_sizes_at_and_beside_the_powers_of_two(toy_ctx, n_tab, none_on_record_3):
    """the bisection's step count is chosen so that 2^trips > n_tab: tables of no entry, one, a power of two and one either side, spread over
    chromosome records 0, 3 and 6 - or over 0 and 6 only, so that the chromosome in the middle owns no entry and two bubbles of record 0 share a
    lo -, with bubbles that are not eligible between the others"""
    bubbles = edge_bubbles(n_tab)
    t = table(9, len(bubbles))
    if none_on_record_3:
        t.chrom[t.chrom == 3] = 0
    places, census = edge_reads(t, bubbles, n_tab)
    want, reads, adds = expected(t, bubbles, places)
    assert load(toy_ctx, t, bubbles) == n_tab == sum(indel_model.eligible(b, W) for b in bubbles) < len(bubbles)
    toy_ctx.indel_records(places)
    got = toy_ctx.indel_counts(0, len(bubbles))
    assert np.array_equal(got, want), (n_tab, np.flatnonzero((got != want).any(axis=1))[:5], got[(got != want).any(axis=1)][:3], want[(got != want).any(axis=1)][:3])
    st = toy_ctx.indel_stats()
    assert st[:2] == (reads, adds) and st[2] >= adds and reads == len(places)
    elig = np.array([indel_model.eligible(b, W) for b in bubbles])
    assert not want[~elig].any() and want[elig][:, 0].all()  # every entry is counted by a read on its chromosome, the first and the last of each among them
    assert census["chromosomes with entries"] + census["without"] == 3 and (census["without"] > 0) == (none_on_record_3 or n_tab < 4)
    assert n_tab < 4 or census["chromosomes with entries"] == (2 if none_on_record_3 else 3)
    if n_tab == 0:
        assert st[2] == 0 and not want.any()
    else:
        assert want[:, 2].any()


def test_mapq_threshold_with_and_without_the_override(toy_ctx, bubbles, rel):
    t = table(200, len(bubbles))
    places = injected(t, rel, 7, mapq=[19, 20, 21])
    load(toy_ctx, t, bubbles)
    seen = []
    for override in (None, np.random.default_rng(2).choice(np.array([19, 20, 21], dtype=np.uint8), len(places))):
        for q in (0, 20, 21, 22):
            toy_ctx.indel_reset()
            toy_ctx.indel_records(places, override, q)
            want, reads, adds = expected(t, bubbles, places, override, q)
            assert np.array_equal(toy_ctx.indel_counts(0, len(bubbles)), want) and (toy_ctx.indel_stats()[:2] == (reads, adds) or adds == 0 == reads)
            seen.append(int(want.sum()))
    assert seen[0] > seen[1] > seen[2] > seen[3] == 0 and seen[4] == seen[0] and seen[5] != seen[1] and seen[7] == 0


def test_two_calls_accumulate_reset_zeroes_and_sub_ranges(toy_ctx, bubbles, rel):
    t = table(200, len(bubbles))
    places = injected(t, rel, 8)
    n = len(bubbles)
    load(toy_ctx, t, bubbles)
    want = expected(t, bubbles, places)[0]
    half = len(places) // 2
    toy_ctx.indel_records(places[:half])
    toy_ctx.indel_records(places[half:])
    assert np.array_equal(toy_ctx.indel_counts(0, n), want)
    toy_ctx.indel_records(places)
    assert np.array_equal(toy_ctx.indel_counts(0, n), 2 * want)
    assert np.array_equal(toy_ctx.indel_counts(0, 3), 2 * want[:3]) and np.array_equal(toy_ctx.indel_counts(n - 2, 2), 2 * want[-2:]) and toy_ctx.indel_counts(n, 0).shape == (0, 4)
    for first, k in ((n, 1), (0, n + 1), (n + 1, 0)):
        with pytest.raises(bw.BwbError, match="error -1.*indel_counts"):
            toy_ctx.indel_counts(first, k)
    toy_ctx.indel_records(places[:0])  # (no reads: no launch, the figures stay)
    toy_ctx.indel_reset()
    assert not toy_ctx.indel_counts(0, n).any()
    # another anchor: a table and counters of its own
    for w in (1, 10, 255):
        assert load(toy_ctx, t, bubbles, w) == sum(indel_model.eligible(b, w) for b in bubbles)
        toy_ctx.indel_records(places)
        assert np.array_equal(toy_ctx.indel_counts(0, n), expected(t, bubbles, places, w=w)[0]), w


def test_seventy_thousand_reads_on_one_bubble(toy_ctx):
    """more adds to one counter than a 16-bit count holds: ref is exactly 70 000, and so is alt"""
    bubbles = [(b"one", 1000, 50, 1052, 50, 2, 3)]
    t = table(3, 1)
    rng = np.random.default_rng(70)
    n = 70_000
    on_chrom = lift_model.place_records([(int(t.start[0]) + 1049 - 1 - int(o), bool(o & 1), "60M") for o in rng.integers(0, 50, n)])
    on_record = lift_model.place_records([(int(t.start[1]) + 50 - 1 - int(o), bool(o & 1), "60M") for o in rng.integers(0, 50, n)])
    assert load(toy_ctx, t, bubbles, 1) == 1
    toy_ctx.indel_records(np.concatenate([on_chrom, on_record]))
    assert toy_ctx.indel_counts(0, 1).tolist() == [[n, n, 0, 0]] and toy_ctx.indel_stats()[:3] == (2 * n, 2 * n, 2 * n)
    assert expected(t, bubbles, np.concatenate([on_chrom[:50], on_record[:50]]), w=1)[0].tolist() == [[50, 50, 0, 0]]


def test_indel_records_strides_over_twice_the_lanes_of_the_grid(toy_ctx, bubbles, rel):
    """the production path of the loop: more than twice 8 * CUs * 256 reads, so that every lane takes a third"""
    t = table(1_300_000, len(bubbles))
    places = injected(t, rel, 9)
    want, reads, adds = expected(t, bubbles, places)
    times = (2 * 8 * compute_units() * 256) // len(places) + 1
    load(toy_ctx, t, bubbles)
    toy_ctx.indel_records(np.tile(places, times))
    assert times * len(places) > 2 * 8 * compute_units() * 256
    assert np.array_equal(toy_ctx.indel_counts(0, len(bubbles)), want * np.uint32(times)) and toy_ctx.indel_stats()[:2] == (reads * times, adds * times)


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_indel_and_slot_indel_equal_the_model_fed_the_oracles_hits(built, tmp_path, lib):
    """the generated genome indexed and mapped, `-n 3 -o 1`, in one batch - plain and joined - and through all eight slots with parked reads: the
    same table, the model's"""
    env = dict(os.environ, BWB_SLICE_ITERS="150")
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "indel_slots_worker.py"), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "INDEL-SLOTS-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


def test_indel_errors_leave_the_context_usable(built, golden, pad_text, toy_tables):
    t = toy_tables
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    c = bw.Context(b)
    one = lift_model.place_records([(5, False, "100M")])
    calls = (lambda: c.batch_indel(), lambda: c.slot_indel(0), lambda: c.batch_indel(6, 5, True), lambda: c.slot_indel(0, 6, 5, True))
    try:
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            c.indel_begin(1)
        c.set_loci(t.start, t.end, t.bub_of, t.recs)
        with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
            c.indel_begin(1)
        c.set_bubble_chrom(t.chrom)
        for w in (0, 256, -1):
            with pytest.raises(bw.BwbError, match="error -1.*anchor"):
                c.indel_begin(w)
        for call in calls + (lambda: c.indel_records(one), lambda: c.indel_counts(0, 0), lambda: c.indel_reset()):
            with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
                call()
        n_bub = len(t.recs)
        assert 0 < c.indel_begin(1) <= n_bub and c.indel_stats() == (0, 0, 0, 0.0)
        c.align(bw.params(["-n", "3"]), seqs, lens)
        c.indel_records(one)  # (needs no SA and no batch)
        assert c.indel_stats()[0] == 1
        for call in calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
                call()
        c.set_sa(b.SA)
        with pytest.raises(bw.BwbError, match="error -4.*max_alt"):
            c.batch_indel(6, 0, True)
        for bad in (lambda: c.batch_indel(6, 5, False, 256), lambda: c.batch_indel(6, 5, False, -1), lambda: c.slot_indel(0, 6, 256), lambda: c.slot_indel(0, 6, -1),
                    lambda: c.slot_indel(-1), lambda: c.slot_indel(bw.MAX_SLOTS), lambda: c.indel_records(one, None, 256)):
            with pytest.raises(bw.BwbError, match="error -1"):
                bad()
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            c.slot_indel(3)
        # none of that has counted anything
        c.indel_reset()
        counted = c.batch_indel()
        total = int(c.indel_counts(0, n_bub).sum())
        assert 500 < counted == c.indel_stats()[0] <= len(lens) and total == c.indel_stats()[1] > 0
        assert c.batch_indel() == 0 and c.batch_indel(6, 5, True, 0) == 0 and int(c.indel_counts(0, n_bub).sum()) == total  # (a submission is counted once)
        c.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            c.batch_indel()
        c.run()
        assert 0 < c.batch_indel(6, 5, True, 0) <= 10
        # a later set_loci or set_bubble_chrom forgets the table and the counters
        c.set_bubble_chrom(t.chrom)
        with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
            c.indel_counts(0, 0)
        assert c.indel_begin(10) <= n_bub and not c.indel_counts(0, n_bub).any()
        c.set_loci(t.start, t.end, t.bub_of, t.recs)
        with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
            c.indel_records(one)
    finally:
        c.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gen_dir(built, tmp_path_factory):
    """the generated genome, indexed, with the reads of indel_model"""
    d = tmp_path_factory.mktemp("indel_cli")
    g = lift_model.genome()
    (d / "gen.fa").write_text(g["fasta"])
    (d / "gen.data").write_bytes(g["data"])
    (d / "gen.fq").write_text(indel_model.fastq(indel_model.reads(g)))
    cli(["index", d / "gen.fa"])
    cli(["fasta2ref", d / "gen.fa"])
    names, start, end = bw.read_ann(d / "gen.fa.ann")
    return types.SimpleNamespace(dir=d, g=g, names=list(names), bub_of=pad_model.bubble_of(names, g["bubbles"]), chrom=join_model.chrom_of(names, g["bubbles"]))


def want_of(gd, sam, w, q=0):
    counts, reads, adds = indel_model.count(indel_model.from_sam(sam, gd.names, gd.bub_of), gd.g["bubbles"], gd.chrom, w, q)
    return indel_model.table_bytes(gd.g["bubbles"], counts), reads, adds


FULL = ["-X", "5", "-J", "-R", "-D"]


@pytest.mark.parametrize("variant", ["one_chunk", "two_workers", "four_workers"])
def test_cli_map_with_indel_support_writes_the_models_bytes(gen_dir, variant):
    """the table is the model's fed the SAM text of the same run; the SAM and -A bytes are those of the run without -I; with and without -R one table"""
    extra, env = dict(VARIANTS, four_workers=(["-g", "4"], {"BWB_DEVICE_MAP": "0,0,0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}))[variant]
    d = gen_dir.dir
    fa, fq, data = d / "gen.fa", d / "gen.fq", d / "gen.data"
    out, base, ind, cnt, cnt0 = (d / f"{variant}.{e}" for e in ("sam", "base.sam", "tsv", "a.tsv", "a0.tsv"))
    if variant == "one_chunk":  # map -n 3 -B t -I f
        cli(["map", "-n", "3", "-o", "1", "-B", data] + extra + [fa, fq, base], env)
        log = cli(["map", "-n", "3", "-o", "1", "-B", data, "-I", ind] + extra + [fa, fq, out], env)
        sam = open(out, "rb").read()
        want, reads, adds = want_of(gen_dir, sam, 1)
        assert sam == open(base, "rb").read() and open(ind, "rb").read() == want and want.count(b"\n") == 9
        assert f"read support per indel bubble on the GPU: anchor 1  eligible bubbles 8  refused and skipped 0  reads counted {reads}  adds {adds} " in log and "k_indel" in log
        assert "read support" not in cli(["map", "-n", "3", "-o", "1", "-B", data] + extra + [fa, fq, base], env)  # without -I nothing is built, uploaded or launched
    # map -n 3 -X 5 -B t -J -R -D -A c -I f -a 1 -w 5
    cli(["map", "-n", "3", "-o", "1", "-B", data] + FULL + ["-A", cnt0, "-a", "1"] + extra + [fa, fq, base], env)
    log = cli(["map", "-n", "3", "-o", "1", "-B", data] + FULL + ["-A", cnt, "-I", ind, "-a", "1", "-w", "5"] + extra + [fa, fq, out], env)
    sam = open(out, "rb").read()
    want, reads, adds = want_of(gen_dir, sam, 5, 1)
    assert sam == open(base, "rb").read() and open(cnt, "rb").read() == open(cnt0, "rb").read()
    assert open(ind, "rb").read() == want and f"anchor 5  eligible bubbles 8  refused and skipped 0  reads counted {reads}  adds {adds} " in log and b"\t8\n" in want
    if variant == "one_chunk":  # the same table without -R
        cli(["map", "-n", "3", "-o", "1", "-B", data, "-X", "5", "-J", "-I", ind, "-a", "1", "-w", "5"] + extra + [fa, fq, out], env)
        assert open(ind, "rb").read() == want


def test_cli_align_then_aln2sam_with_indel_support(gen_dir, tmp_path):
    d = gen_dir.dir
    fa, fq, data, aln = d / "gen.fa", d / "gen.fq", d / "gen.data", tmp_path / "t.aln"
    cli(["align", "-n", "3", "-o", "1", fa, fq, aln])
    for opts in (["-B", data], ["-B", data] + FULL[:-1]):
        for q, w in ((1, 5), (37, 30)):
            cli(["aln2sam", "-n", "6"] + opts + ["-I", tmp_path / "a.tsv", "-a", q, "-w", w, fa, fq, aln, tmp_path / "a.sam"])
            cli(["map", "-n", "3", "-o", "1"] + opts + ["-I", tmp_path / "m.tsv", "-a", q, "-w", w, fa, fq, tmp_path / "m.sam"])
            sam = open(tmp_path / "a.sam", "rb").read()
            assert sam == open(tmp_path / "m.sam", "rb").read()
            assert open(tmp_path / "a.tsv", "rb").read() == open(tmp_path / "m.tsv", "rb").read() == want_of(gen_dir, sam, w, q)[0], (opts, q, w)


def test_cli_map_with_indel_support_on_records_out_of_text_order(gen_dir, tmp_path):
    """an .ann whose records do not ascend: the loci come from the host's resolver and so does the table, and the log says so"""
    d = gen_dir.dir
    for ext in ("", ".bwt", ".ref"):
        shutil.copy(d / ("gen.fa" + ext), tmp_path / ("gen.fa" + ext))
    lines = open(d / "gen.fa.ann").read().split("\n")
    lines[2], lines[4] = lines[4], lines[2]  # two bubble records change places
    (tmp_path / "gen.fa.ann").write_text("\n".join(lines))
    names, _, _ = bw.read_ann(tmp_path / "gen.fa.ann")
    gd = types.SimpleNamespace(g=gen_dir.g, names=list(names), bub_of=pad_model.bubble_of(names, gen_dir.g["bubbles"]), chrom=join_model.chrom_of(names, gen_dir.g["bubbles"]))
    log = cli(["map", "-n", "3", "-o", "1", "-B", d / "gen.data", "-I", tmp_path / "i.tsv", "-w", "5", tmp_path / "gen.fa", d / "gen.fq", tmp_path / "o.sam"])
    want, reads, adds = want_of(gd, open(tmp_path / "o.sam", "rb").read(), 5)
    assert open(tmp_path / "i.tsv", "rb").read() == want and want.count(b"\n") == 9
    assert f"read support per indel bubble on the host (the .ann records are not ascending and disjoint): anchor 5  eligible bubbles 8  refused and skipped 0  reads counted {reads}  adds {adds}" in log
