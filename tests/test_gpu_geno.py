"""Genotype calls at the IUPAC sites and the indel bubbles (`bwbble map -G`, kernels k_geno_count / k_geno_emit / k_geno_bubbles) on the GPU, judged
by tests/geno_model.py: the inverse of the site index on constructed texts - every site must come back with its position and code -; the calls on
counts injected with pile_put / indel_put, every crafted vector on every code; ranges and pieces; more sites than the grid has lanes; the put /
counts round trip; bubble tables of 0 to 257 entries with ineligible bubbles beside eligible ones; the state and argument errors; and the command
line on the diploid sample against the bytes of the CPU-only chain, with one, two and four workers."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bwbble_amd as bw
import geno_model
import indel_model
import lift_model
import pad_model
import pile_model
from test_geno_host import crafted_text
from test_gpu_join import table
from test_gpu_map import cli, compute_units
from test_gpu_pile import text  # noqa: F401 (fixture: the constructed text of 3 201 characters)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(built, golden):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    yield c
    c.close()


def begin(ctx, text, piece=None):
    """the text, its site index and zeroed counters, and scratch for `piece` sites (None: all of them) -> the text positions of the sites"""
    where = pile_model.sites(text)
    ctx.set_text(pile_model.codes(text))
    assert ctx.pile_begin() == len(where)
    ctx.geno_begin(max(1, len(where)) if piece is None else piece)
    return where


def words(n_words, sites_in, tail=0, seed=0):
    """a text of n_words words of 32 characters (+ tail characters): the words listed in sites_in hold random sites, the others none"""
    rng = np.random.default_rng(seed)
    out = []
    for w in range(n_words):
        if w in sites_in:
            out.append("".join(rng.choice(list("ACGT" + pile_model.SITE_LETTERS * 2), 32)))
        else:
            out.append("".join(rng.choice(list("ACGTN"), 32)))
    return "".join(out) + "ACGT"[:tail]


def inverse_texts(text):
    t = {"constructed": text,
         "no_site_in_the_last_three_words": "K" + words(9, {0, 2, 5})[1:] + words(3, set(), 7),
         "five_empty_words_in_the_middle": words(4, {0, 1, 2, 3}, seed=1) + words(5, set()) + words(4, {0, 1, 3}, seed=2) + "W",
         "one_word": "ACGTKACGTNNSACGTBY$W",
         "one_site": "ACGT" * 20 + "R" + "ACGT" * 30}
    for nw in (15, 16, 17):
        t[f"{nw}_words"] = words(nw, set(range(0, nw, 2)) | {nw - 1}, seed=nw)
    t["16_words_and_one_character"] = words(16, {0, 15}, seed=3) + "D"
    return t


def test_every_site_comes_back_with_its_position_and_code(ctx, text):
    """the inverse of the site index: with a count at every site, geno_sites returns every site in order, where the model says it lies; and
    k_site_of maps the returned positions back"""
    texts = inverse_texts(text)
    w = [[k for k in range(32) if 32 * i + k < len(text) and text[32 * i + k] in pile_model.SITE_LETTERS] for i in range((len(text) + 31) // 32)]
    assert w[3] == [0, 7, 8, 15, 16, 31] and len(w[4]) == 32 and w[5] == [] and text[0] in pile_model.SITE_LETTERS and text[-1] in pile_model.SITE_LETTERS
    for name, t in texts.items():
        where = begin(ctx, t)
        n = len(where)
        assert n > 0, name
        counts = np.ones((n, 4), dtype=np.uint32)
        ctx.pile_put(0, counts)
        got = ctx.geno_sites(0, n)
        want = geno_model.site_records(t, counts)
        assert len(got) == n and got.tobytes() == want.tobytes(), (name, np.flatnonzero(got["pos"] != want["pos"])[:5])
        assert got["pos"].tolist() == where and [pile_model.NT16[c] for c in got["code"]] == [t[p] for p in where], name
        assert np.array_equal(ctx.pile_site_of(got["pos"]), np.arange(n)), name
        assert ctx.geno_stats()[0] == n and ctx.geno_stats()[2] > 0
    assert (len(texts["15_words"]), len(texts["16_words"]), len(texts["17_words"]), len(texts["16_words_and_one_character"])) == (480, 512, 544, 513)
    # a text without sites: nothing to call
    begin(ctx, "ACGTN$" * 100 + "ACG")
    assert len(ctx.geno_sites(0, 0)) == 0
    with pytest.raises(bw.BwbError, match="error -1.*geno_sites"):
        ctx.geno_sites(0, 1)


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_a_text_uploaded_in_two_chunks(built, lib):
    env = dict(os.environ)
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "geno_sites_worker.py"), "2" if lib == "testlib" else "1"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0 and "GENO-SITES-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


def test_calls_on_injected_counts(ctx):
    """every crafted vector on every code, each group under its own E and d: the model's records byte for byte"""
    t, per_site = crafted_text()
    where = begin(ctx, t)
    assert len(where) == len(per_site) > 300
    counts = np.array([v for _, _, v in per_site], dtype=np.uint32)
    ctx.pile_put(0, counts)
    assert np.array_equal(ctx.pile_counts(0, len(where)), counts)
    groups = sorted({(e, d) for e, d, _ in per_site})
    assert {e for e, _ in groups} >= {4, 20, 93} and {d for _, d in groups} >= {1, 7, (1 << 31) - 1}
    for E, D in groups:
        got = ctx.geno_sites(0, len(where), E, D)
        want = geno_model.site_records(t, counts, E, D)
        assert got.tobytes() == want.tobytes(), (E, D, len(got), len(want), [(g, w) for g, w in zip(got.tolist(), want.tolist()) if g != w][:3])
        assert ctx.geno_stats()[0] == len(want)
    assert {int(c) for c in want["code"]} == {pile_model.NT16.index(c) for c in pile_model.SITE_LETTERS}


def test_ranges_and_pieces(ctx):
    """n = 1, 7, the piece and the whole table, at both ends; a range without a called site; pieces of 1 000 concatenated"""
    rng = np.random.default_rng(8)
    t = "".join(rng.choice(list("ACGT" * 5 + pile_model.NT16[1:]), 20011))
    n = len(pile_model.sites(t))
    assert n > 4000
    counts = rng.integers(0, 40, (n, 4)).astype(np.uint32)
    counts[rng.random(n) < 0.3] = 0
    counts[2000:2300] = 0
    counts[0] = counts[n - 1] = (3, 0, 2, 1)
    counts[1999] = counts[2300] = (1, 1, 0, 0)
    begin(ctx, t, n)
    ctx.pile_put(0, counts)
    whole = geno_model.site_records(t, counts, 20, 2)
    assert ctx.geno_sites(0, n, 20, 2).tobytes() == whole.tobytes()
    for first, k in ((0, 1), (0, 7), (n - 1, 1), (n - 7, 7), (n, 0), (0, 0), (2000, 300), (1999, 302), (n // 2, 1000)):
        want = geno_model.site_records(t, counts, 20, 2, first, k)
        got = ctx.geno_sites(first, k, 20, 2)
        assert got.tobytes() == want.tobytes(), (first, k)
        assert (len(want) == 0) == ((first, k) in ((n, 0), (0, 0), (2000, 300)))
    begin(ctx, t, 1000)
    ctx.pile_put(0, counts)
    with pytest.raises(bw.BwbError, match="error -1.*piece"):
        ctx.geno_sites(0, 1001, 20, 2)
    pieces = [ctx.geno_sites(s, min(1000, n - s), 20, 2) for s in range(0, n, 1000)]
    assert np.concatenate(pieces).tobytes() == whole.tobytes() and ctx.geno_sites(n - 1000, 1000, 20, 2).tobytes() == geno_model.site_records(t, counts, 20, 2, n - 1000, 1000).tobytes()


def test_more_sites_than_the_grid_has_lanes(ctx):
    """one call over more sites than 8 blocks per CU have lanes: every lane takes several sites; K everywhere, so that numpy can restate the rule"""
    lanes = compute_units() * 8 * 256
    n = 2 * lanes + 777
    rng = np.random.default_rng(5)
    body = np.where(rng.random(n + n // 3) < 0.75, "K", "A")
    t = "".join(body.tolist())
    where = np.array(pile_model.sites(t), dtype=np.uint64)
    n = len(where)
    assert n > lanes and n <= 1 << 24
    begin(ctx, t, n)
    counts = rng.integers(0, 12, (n, 4)).astype(np.uint32)
    counts[rng.random(n) < 0.25] = 0
    ctx.pile_put(0, counts)
    E, D = 20, 3
    got = ctx.geno_sites(0, n, E, D)
    print(f"k_geno_count + scan + k_geno_emit: {n} sites in one call, {len(got)} called, kernels {ctx.geno_stats()[2]:.3f} ms")
    c = counts.astype(np.int64)
    depth = c.sum(axis=1)
    called = depth >= D
    n0, n1 = c[:, 2], c[:, 3]  # K: G, T
    raw = np.stack([E * (depth - n0), 3 * (n0 + n1) + E * (depth - n0 - n1), E * (depth - n1)], axis=1)[called]
    gt = raw.argmin(axis=1)
    pl = raw - raw.min(axis=1, keepdims=True)
    gq = np.minimum(99, np.sort(pl, axis=1)[:, 1])
    assert len(got) == int(called.sum()) and np.array_equal(got["pos"], where[called]) and np.array_equal(got["site"], np.flatnonzero(called))
    assert np.array_equal(got["n"], counts[called]) and np.array_equal(got["gt"], gt) and np.array_equal(got["gq"], gq) and np.array_equal(got["pl"][:, :3], pl)
    assert not got["pl"][:, 3:].any() and (got["n_geno"] == 3).all() and (got["code"] == 2).all() and not got["reserved"].any()


def test_put_and_counts_round_trip(ctx, text):
    where = begin(ctx, text)
    n = len(where)
    rng = np.random.default_rng(2)
    v = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    ctx.pile_put(0, v)
    assert np.array_equal(ctx.pile_counts(0, n), v)
    ctx.pile_put(0, v[:1] + 1)
    ctx.pile_put(n - 3, v[:3])
    ctx.pile_put(n, np.zeros((0, 4), dtype=np.uint32))
    v[n - 3:] = v[:3].copy()
    v[0] += 1
    assert np.array_equal(ctx.pile_counts(0, n), v) and np.array_equal(ctx.pile_counts(n - 3, 3), v[n - 3:])
    # after real adds a put overwrites: three reads of 50 bases over the text's first sites
    ctx.pile_reset()
    ctx.pile_records(np.zeros((3, 50), dtype=np.uint8), np.full(3, 50, dtype=np.uint16), lift_model.place_records([(0, False, "50M"), (1, False, "50M"), (0, True, "50M")]))
    added = ctx.pile_counts(0, n)
    assert added.any() and ctx.pile_stats()[1] == int(added.sum())
    ctx.pile_put(0, v[:40])
    assert np.array_equal(ctx.pile_counts(0, 40), v[:40]) and np.array_equal(ctx.pile_counts(40, n - 40), added[40:])
    for first, k in ((0, n + 1), (n, 1), (n + 1, 0), ((1 << 64) - 1, 2)):
        with pytest.raises(bw.BwbError, match="error -1.*pile_put"):
            ctx.pile_put(first, np.zeros((k, 4), dtype=np.uint32))


W = 4
EDGES = [(b"e", 1000, 20, 1020, 19, 0, 3), (b"e", 1300, W, 1304, W - 1, 0, 1), (b"e", 1300, W - 1, 1303, W - 1, 0, 1), (b"e", 1300, W, 1304, W - 2, 0, 1), (b"e", 1, W, 5, 10, 0, 1),
         (b"e", 0, W, 4, 10, 0, 1), (b"e", 1500, 10, 1509, 10, 0, 2), (b"e", 1600, 40, 1770, 40, 130, 0)]  # the eligibility edges of tests/test_gpu_indel.py at anchor 4


def load(ctx, t, bubbles, w):
    ctx.set_loci(t.start, t.end, t.bub_of, pad_model.bubble_records(bubbles))
    ctx.set_bubble_chrom(t.chrom)
    return ctx.indel_begin(w)


@pytest.mark.parametrize("n_bub", [0, 1, 2, 255, 256, 257])
def test_bubble_tables(ctx, text, n_bub):
    """ineligible bubbles beside eligible ones, with counters in all of them: only the eligible ones are called; put / counts round trip; ranges"""
    assert [indel_model.eligible(b, W) for b in EDGES] == [True, True, False, False, True, False, False, True]
    bubbles = [EDGES[(k * 3) % len(EDGES)] for k in range(n_bub)]
    if n_bub:
        t = table(9, n_bub)
    else:
        t = types.SimpleNamespace(start=np.array([1000], dtype=np.uint64), end=np.array([6999], dtype=np.uint64), bub_of=np.array([-1], dtype=np.int32), chrom=np.zeros(0, dtype=np.int32))
    n_elig = load(ctx, t, bubbles, W)
    assert n_elig == sum(indel_model.eligible(b, W) for b in bubbles)
    begin(ctx, text, 100)  # (geno_begin behind indel_begin: min(100, n_bub) bubbles per call)
    rng = np.random.default_rng(n_bub)
    counts = rng.integers(0, 25, (n_bub, 4)).astype(np.uint32)
    if n_bub > 2:
        counts[::5] = 0
        counts[7] = 0xFFFFFFFF
    ctx.indel_put(0, counts)
    assert np.array_equal(ctx.indel_counts(0, n_bub), counts)
    piece = max(1, min(100, n_bub))
    for E, D in ((20, 1), (4, 30), (93, 2)):
        want = geno_model.bubble_records(bubbles, counts, W, E, D)
        got = [ctx.geno_bubbles(s, min(piece, n_bub - s), E, D) for s in range(0, n_bub, piece)]
        got = np.concatenate(got) if got else np.zeros(0, dtype=bw.GENO_BUBBLE_DTYPE)
        assert got.tobytes() == want.tobytes(), (E, D, len(got), len(want))
        assert all(indel_model.eligible(bubbles[int(b)], W) for b in got["bubble"])
        for first, k in ((0, min(1, n_bub)), (max(0, n_bub - 7), min(7, n_bub)), (n_bub, 0)):
            assert ctx.geno_bubbles(first, k, E, D).tobytes() == geno_model.bubble_records(bubbles, counts, W, E, D, first, k).tobytes(), (first, k)
    if n_bub:
        with pytest.raises(bw.BwbError, match="error -1.*geno_bubbles"):
            ctx.geno_bubbles(0, piece + 1)
    with pytest.raises(bw.BwbError, match="error -1.*geno_bubbles"):
        ctx.geno_bubbles(n_bub, 1)
    with pytest.raises(bw.BwbError, match="error -1.*indel_put"):
        ctx.indel_put(n_bub, np.zeros((1, 4), dtype=np.uint32))
    # the anchor decides: at 5 the bubbles with a flank of 4 are no longer eligible, whatever their counters hold
    if n_bub > 2:
        assert load(ctx, t, bubbles, W + 1) < n_elig
        ctx.geno_begin(n_bub)
        ctx.indel_put(0, counts)
        assert ctx.geno_bubbles(0, n_bub).tobytes() == geno_model.bubble_records(bubbles, counts, W + 1).tobytes()


def test_state_and_argument_errors(built, golden, text):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    one = np.ones((1, 4), dtype=np.uint32)
    try:
        with pytest.raises(bw.BwbError, match="error -4.*pile_begin"):
            c.geno_begin(10)
        with pytest.raises(bw.BwbError, match="error -4.*pile_begin"):
            c.pile_put(0, one)
        with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
            c.indel_put(0, one)
        with pytest.raises(bw.BwbError, match="error -4.*geno_begin"):
            c.geno_sites(0, 0)
        with pytest.raises(bw.BwbError, match="error -4.*geno_begin"):
            c.geno_bubbles(0, 0)
        c.set_text(pile_model.codes(text))
        n = c.pile_begin()
        for bad in (0, (1 << 24) + 1):
            with pytest.raises(bw.BwbError, match="error -1.*piece"):
                c.geno_begin(bad)
        with pytest.raises(bw.BwbError, match="error -4.*geno_begin"):
            c.geno_sites(0, 1)
        c.geno_begin(1 << 10)
        assert c.geno_stats() == (0, 0, 0.0)
        with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
            c.geno_bubbles(0, 0)
        for err, d in ((3, 1), (94, 1), (-1, 1), (20, 0), (20, -5), (20, 1 << 31)):
            with pytest.raises(bw.BwbError, match="error -1.*geno_sites"):
                c.geno_sites(0, 1, err, d)
        for first, k in ((0, n + 1), (n, 1), (n + 1, 0), ((1 << 64) - 1, 2), (0, (1 << 10) + 1)):
            with pytest.raises(bw.BwbError, match="error -1.*geno_sites"):
                c.geno_sites(first, k)
        # the context is still usable, and the edges of the arguments are taken
        c.pile_put(0, one)
        assert len(c.geno_sites(0, 1, 4, 1)) == 1 and len(c.geno_sites(0, 1, 93, (1 << 31) - 1)) == 0 and len(c.geno_sites(0, min(n, 1 << 10), 93, 1)) == 1
        # indel_begin behind geno_begin: the bubble output was never sized
        t = table(9, 5)
        assert load(c, t, EDGES[:5], W) == 3
        with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
            c.geno_bubbles(0, 1)
        c.geno_begin(3)
        c.indel_put(0, np.ones((5, 4), dtype=np.uint32))
        assert len(c.geno_bubbles(0, 3)) == 2 and len(c.geno_bubbles(3, 2)) == 1
        for err, d in ((3, 1), (94, 1), (20, 0), (20, 1 << 31)):
            with pytest.raises(bw.BwbError, match="error -1.*geno_bubbles"):
                c.geno_bubbles(0, 1, err, d)
        for first, k in ((0, 4), (5, 1), (6, 0)):
            with pytest.raises(bw.BwbError, match="error -1.*geno_bubbles"):
                c.geno_bubbles(first, k)
        # a later pile_begin, set_text or indel_begin forgets what geno_begin sized
        c.indel_begin(W)
        with pytest.raises(bw.BwbError, match="error -4.*indel_begin"):
            c.geno_bubbles(0, 1)
        assert len(c.geno_sites(0, 1)) == 1
        c.pile_begin()
        with pytest.raises(bw.BwbError, match="error -4.*geno_begin"):
            c.geno_sites(0, 1)
    finally:
        c.close()


# ---- the command line --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(built, oracle, tmp_path_factory):
    """the diploid sample and what the CPU-only chain makes of it (tests/geno_model.py: build_chain)"""
    return geno_model.build_chain(tmp_path_factory.mktemp("geno_cli"), oracle)


MAP = ["map", "-n", "3", "-o", "1", "-X", "5"]
RUNS = {
    "one_worker": ([], {}),
    "chunks_of_97": ([], {"BWB_CHUNK": "97"}),
    "two_workers": (["-g", "2"], {"BWB_DEVICE_MAP": "0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}),
    "four_workers": (["-g", "4"], {"BWB_DEVICE_MAP": "0,0,0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1", "BWB_DEBUG": "1"}),
    "count_piece_7": ([], {"BWB_COUNT_PIECE": "7", "BWB_DEBUG": "1"}),
}


@pytest.mark.parametrize("run", list(RUNS))
def test_cli_map_writes_the_chains_calls(chain, run):
    """`map -n 3 -o 1 -X 5 -B t -J -R -G f -a 1 -w 5`: the bytes of the CPU-only chain in every run; the SAM, -A and -I bytes are those of the run without -G"""
    extra, env = RUNS[run]
    d = chain.dir
    p = lambda n: os.path.join(d, f"{run}.{n}")
    flags = ["-B", chain.data, "-J", "-R", "-A", p("a.tsv"), "-I", p("i.tsv"), "-a", "1", "-w", "5"]
    log = cli(MAP + flags + ["-G", p("calls.tsv")] + extra + [chain.fa, chain.fq, p("sam")], env)
    rd = lambda n: open(p(n), "rb").read()
    assert rd("calls.tsv") == chain.calls, pad_model.first_difference(rd("calls.tsv"), chain.calls)
    assert (rd("sam"), rd("a.tsv"), rd("i.tsv")) == (chain.base, chain.a_tsv, chain.i_tsv)
    sites, bubs = (sum(ln.startswith(k) for ln in chain.calls.split(b"\n")) for k in (b"S\t", b"I\t"))
    assert f"genotype calls on the GPU (worker " in log and f"sites called {sites}  bubbles called {bubs}  kernels " in log, log[-2000:]
    if run == "one_worker":  # without -G: the same three files, and nothing of it is built, uploaded or launched
        log0 = cli(MAP + flags + extra + [chain.fa, chain.fq, p("sam")], env)
        assert (rd("sam"), rd("a.tsv"), rd("i.tsv")) == (chain.base, chain.a_tsv, chain.i_tsv) and "genotype" not in log0
        assert "tables put back in 0 pieces" in log
    if run == "four_workers":  # one worker called, after the host's sums were put back over its counters
        called = [ln for ln in log.split("\n") if "genotypes called by this worker, the last of 4" in ln]
        assert len(called) == 1 and " 2 pieces of tables put back" in called[0], log[-3000:]
    if run == "count_piece_7":
        called = [ln for ln in log.split("\n") if "genotypes called by this worker, the last of 1" in ln]
        n_sites = len(pile_model.sites(pile_model.fasta_text(chain.g["fasta"])[0]))
        pieces = (n_sites + 6) // 7 + (len(chain.g["bubbles"]) + 6) // 7
        assert len(called) == 1 and " 0 pieces of tables put back" in called[0] and f" {pieces} pieces called" in called[0] and pieces >= 10, log[-3000:]


def test_cli_map_with_calls_alone(chain):
    """`map -G f` (sites only, the reads where they lie) and `map -B t -G f` without -A and -I: what `align` + `aln2sam ... -G f` write"""
    d = chain.dir
    p = lambda n: os.path.join(d, f"alone.{n}")
    cli(["align", "-n", "3", "-o", "1", chain.fa, chain.fq, p("aln")])
    for opts in ([], ["-B", chain.data], ["-X", "5", "-B", chain.data, "-J", "-R", "-a", "1", "-w", "5"]):
        log = cli(["map", "-n", "3", "-o", "1"] + opts + ["-G", p("m.tsv")] + [chain.fa, chain.fq, p("m.sam")])
        cli(["map", "-n", "3", "-o", "1"] + opts[:-4 if "-a" in opts else None] + [chain.fa, chain.fq, p("m0.sam")])  # (-a and -w are refused without -A, -I or -G)
        cli(["aln2sam", "-n", "6"] + opts + ["-G", p("a.tsv"), "-q", "20", "-d", "1", chain.fa, chain.fq, p("aln"), p("a.sam")])
        m, a = open(p("m.tsv"), "rb").read(), open(p("a.tsv"), "rb").read()
        assert m == a and m.startswith(geno_model.HEADER) and m.count(b"\nS\t") > 20, (opts, pad_model.first_difference(m, a))
        assert (b"\nI\t" in m) == bool(opts) and open(p("m.sam"), "rb").read() == open(p("m0.sam"), "rb").read() == open(p("a.sam"), "rb").read()
        assert "genotype calls on the GPU" in log
        if len(opts) > 2:
            assert m == chain.calls
