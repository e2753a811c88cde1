"""Base qualities in the allele counts and the genotype calls (`bwbble map -b m` / `-Y`, kernels k_pile_q / k_geno_emit_q) on the GPU, judged by
tests/pileq_model.py: Context.pile_records_q on the injected records of the pile tests under per-read quality ramps - a base on a site at m - 1, m
and m + 1, the quality bytes 0, 32, 33, 126 and 255, reads of 1 and 255 bases, stride > len -; the counter edges - 70 000 reads on one site, a
column that wraps, more reads than twice the grid's lanes, two calls, reset, sub-ranges -; Context.geno_sites_q on injected counters and sums; the
pad_bub reads in one batch and streamed through the slots (tests/pileq_slots_worker.py); the state and argument errors; and the command line
against the CPU-only chain's bytes and against `align` + `aln2sam`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bwbble_amd as bw
import geno_model
import lift_model
import md_model
import pad_model
import pile_model
import pileq_model
from test_geno_host import crafted_text
from test_gpu_join import VARIANTS, model, pad_text, toy_tables  # noqa: F401 (fixtures)
from test_gpu_map import cli, compute_units
from test_gpu_md import base_texts, cases, md_dir, toy  # noqa: F401 (fixtures, and the shapes of the md tests)
from test_gpu_pile import Q, records, text  # noqa: F401 (fixture: the constructed text of 3 201 characters; the injected records)
from test_md_host import fx, ref, write_inputs  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = (0, 32, 33, 126, 255)


@pytest.fixture(scope="module")
def ctx(built, golden, text):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    c.set_text(pile_model.codes(text))
    c.n_sites = c.pile_begin()
    c.pileq_begin(True)
    c.geno_begin(c.n_sites)
    h = text.index("$") + 1
    c.set_loci(np.array([0, h], dtype=np.uint64), np.array([h - 1, len(text) - 1], dtype=np.uint64), np.array([-1, -1], dtype=np.int32), np.zeros(0, dtype=bw.BUBBLE_DTYPE))
    c.starts = [0, h]
    yield c
    c.close()


def ramps(lens, stride, m, seed):
    """(n, stride) quality bytes in FASTQ order: per read a ramp that differs from its own reverse, running through m - 1, m, m + 1 (as bytes 33 + Q) with the
    edge bytes sprinkled in; the bytes behind a read's length are 255 (they belong to no base)"""
    rng = np.random.default_rng(seed)
    q = np.full((len(lens), stride), 255, dtype=np.uint8)
    around = [33 + v for v in (m - 1, m, m + 1) if 0 <= v <= 93]
    for r, n in enumerate(lens):
        n = int(n)
        line = [(around + list(EDGE))[(r + i // 2) % (len(around) + len(EDGE))] if (i + r) % 2 else 33 + (5 * r + 7 * i) % 94 for i in range(n)]
        if n > 1 and line == line[::-1]:
            line[0], line[-1] = 34, 120
        q[r, :n] = line
    return q


def tables(ctx):
    return ctx.pile_counts(0, ctx.n_sites), ctx.pileq_sums(0, ctx.n_sites)


@pytest.fixture(scope="module")
def injected(ctx, text):
    return records(ctx, text, cases(text))


def test_pile_records_q_equals_the_model_on_injected_records(ctx, text, injected):
    """the -D / -A cases on both strands - windows at every word offset, CIGARs of up to eight gap runs, I beside D, S at either end, lifted records,
    reads of 1 and 255 bases in rows of 255 bytes (stride > len) - under min_baseq 0, 1, 20, 93 and err_cap 0, 4, 20, 93"""
    rows, seqs, lens, places, kinds, lrecs = injected
    lift = md_model.pack_lift(kinds, lrecs)
    assert seqs.shape[1] == 255 and set(lens.tolist()) >= {1, 255} and (lens < 255).any()
    seen_q = set()
    for m, E, min_mapq in ((0, 0, 0), (1, 0, 0), (20, 0, 0), (93, 0, 0), (0, 4, 0), (1, 20, Q), (20, 20, 0), (93, 93, 0), (20, 93, Q + 1)):
        quals = ramps(lens, 255, m or 20, 100 + m)
        wc, ws, reads, adds, dropped = pileq_model.expected_q(text, seqs, quals, lens, places, kinds, lrecs, ctx.starts, None, min_mapq, m, E)
        ctx.pile_reset()
        ctx.pile_records_q(seqs, quals, lens, places, *lift, min_mapq=min_mapq, min_baseq=m, err_cap=E)
        gc, gs = tables(ctx)
        assert np.array_equal(gc, wc), (m, E, np.flatnonzero((gc != wc).any(axis=1))[:5])
        assert np.array_equal(gs, ws), (m, E, np.flatnonzero((gs != ws).any(axis=1))[:5])
        st = ctx.pileq_stats()
        assert st[:3] == (reads, adds, dropped) and st[3] > 0 and adds == int(wc.sum()) > 0 and (E == 0) == (not ws.any())
        if m:
            assert dropped > 0
            # bases on a site at m - 1, m and m + 1, and the edge bytes, among the bases of the reads that count
            for start, ops, seq, _, qual in pileq_model.record_placements_q(seqs, quals, lens, places, kinds, lrecs, ctx.starts):
                if md_model.md(text, start, ops, seq)[0] != md_model.OK:
                    continue
                i, t = 0, start
                for n, op in ops:
                    if op == "M":
                        seen_q |= {(m, qual[i + k]) for k in range(n) if text[t + k] in pile_model.SITE_LETTERS and seq[i + k] in "ACGT"}
                    i += n if op in "MIS" else 0
                    t += n if op in "MD" else 0
        if (m, E) == (0, 0):  # min_baseq = 0, err_cap = 0: pile_records on the same records
            ctx.pile_reset()
            ctx.pile_records(seqs, lens, places, *lift, min_mapq=min_mapq)
            assert np.array_equal(ctx.pile_counts(0, ctx.n_sites), gc) and ctx.pile_stats()[:2] == (reads, adds) and dropped == 0
    for m in (1, 20, 93):
        assert {(m, 33 + v) for v in (m - 1, m, m + 1) if v <= 93} | {(m, b) for b in EDGE} <= seen_q, m
    # the quality line the wrong way round gives another table: the orientation is checked
    quals = ramps(lens, 255, 20, 120)
    flipped = quals.copy()
    for r, n in enumerate(lens):
        flipped[r, :n] = quals[r, :n][::-1]
    a, b = (pileq_model.expected_q(text, seqs, q, lens, places, kinds, lrecs, ctx.starts, None, 0, 20, 30)[:2] for q in (quals, flipped))
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])


def test_counter_edges(ctx, text, injected):
    """70 000 reads on one site: exact sums; a column put to 0xFFFFFFF0 and piled wraps; two calls accumulate; pile_reset zeroes both tables;
    sub-ranges of pileq_sums at both ends"""
    site = 96
    rng = np.random.default_rng(3)
    templates = []
    for k in range(70):
        ln = 33 + k % 5
        templates.append((site - (k * 7) % ln, bool(k & 1), f"{ln}M", "".join(rng.choice(list("ACGT"), ln))))
    seqs, lens = np.full((70, 40), 4, dtype=np.uint8), np.zeros(70, dtype=np.uint16)
    for r, (start, rev, cig, seq) in enumerate(templates):
        up = seq[::-1].translate(md_model.COMP) if rev else seq
        seqs[r, :len(up)], lens[r] = ["AGCTN".index(c) for c in up], len(up)
    places = lift_model.place_records([(s, rev, cig) for s, rev, cig, _ in templates])
    quals = ramps(lens, 40, 20, 7)
    wc, ws, reads, adds, dropped = pileq_model.expected_q(text, seqs, quals, lens, places, min_baseq=2, err_cap=40)
    k = int(pile_model.site_of(text)[site])
    assert reads == 70 and 0 < wc[k].sum() <= 70 and ws[k].sum() > 4 * wc[k].sum()
    times = 1000
    ctx.pile_reset()
    ctx.pile_records_q(np.tile(seqs, (times, 1)), np.tile(quals, (times, 1)), np.tile(lens, times), np.tile(places, times), min_baseq=2, err_cap=40)
    gc, gs = tables(ctx)
    assert np.array_equal(gc, wc * np.uint32(times)) and np.array_equal(gs, ws * np.uint32(times)) and ctx.pileq_stats()[:3] == (70_000, adds * times, dropped * times)
    # a second call accumulates into both
    ctx.pile_records_q(seqs, quals, lens, places, min_baseq=2, err_cap=40)
    gc2, gs2 = tables(ctx)
    assert np.array_equal(gc2, wc * np.uint32(times + 1)) and np.array_equal(gs2, ws * np.uint32(times + 1))
    # wrap: the site's columns at 0xFFFFFFF0, then one call
    n = ctx.n_sites
    put = np.zeros((n, 4), dtype=np.uint32)
    put[k] = 0xFFFFFFF0
    ctx.pileq_put(0, put)
    ctx.pile_put(0, put)
    ctx.pile_records_q(seqs, quals, lens, places, min_baseq=2, err_cap=40)
    gc, gs = tables(ctx)
    assert np.array_equal(gs, put + ws) and np.array_equal(gc, put + wc) and (gs[k] < 0xFFFFFFF0).any()  # (uint32 sums wrap as the table does)
    for lo, cnt in ((0, 1), (0, 7), (n - 1, 1), (n - 9, 9), (n, 0), (0, 0), (k, 1), (n // 2, 33)):
        assert np.array_equal(ctx.pileq_sums(lo, cnt), gs[lo:lo + cnt]), (lo, cnt)
    for lo, cnt in ((0, n + 1), (n, 1), (n + 1, 0), (1, n), ((1 << 64) - 1, 2)):
        with pytest.raises(bw.BwbError, match="error -1.*pileq_sums"):
            ctx.pileq_sums(lo, cnt)
    for lo, cnt in ((n, 1), (n - 1, 2), (1, n), ((1 << 64) - 1, 2)):
        with pytest.raises(bw.BwbError, match="error -1.*pileq_put"):
            ctx.pileq_put(lo, np.zeros((cnt, 4), dtype=np.uint32))
    ctx.pile_reset()
    assert not any(t.any() for t in tables(ctx))
    # more reads than twice the grid's lanes
    rows, s2, l2, p2, kinds, lrecs = injected
    short = np.flatnonzero((l2 <= 33) & (kinds == 0))
    s2, l2, p2 = np.ascontiguousarray(s2[short, :33]), l2[short], p2[short]
    q2 = ramps(l2, 33, 20, 9)
    wc, ws, reads, adds, dropped = pileq_model.expected_q(text, s2, q2, l2, p2, min_mapq=Q, min_baseq=20, err_cap=30)
    lanes = 8 * compute_units() * 256
    times = 2 * lanes // len(l2) + 1
    assert times * len(l2) > 2 * lanes and reads > 100 and adds > 100 and dropped > 100
    ctx.pile_records_q(np.tile(s2, (times, 1)), np.tile(q2, (times, 1)), np.tile(l2, times), np.tile(p2, times), min_mapq=Q, min_baseq=20, err_cap=30)
    gc, gs = tables(ctx)
    assert np.array_equal(gc, wc * np.uint32(times)) and np.array_equal(gs, ws * np.uint32(times)) and ctx.pileq_stats()[:3] == (reads * times, adds * times, dropped * times)
    ctx.pile_reset()


def begin(c, t, piece=None):
    where = pile_model.sites(t)
    c.set_text(pile_model.codes(t))
    assert c.pile_begin() == len(where)
    c.pileq_begin(True)
    c.geno_begin(max(1, len(where)) if piece is None else piece)
    return where


@pytest.fixture(scope="module")
def gctx(built, golden):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    yield c
    c.close()


def member_cols(letter):
    return [geno_model.COLS.index(c) for c in geno_model.MEMBERS[letter]]


def test_weighted_calls_on_injected_counts_and_sums(gctx):
    """the crafted vectors of geno_model with s_i = E n_i: geno_sites' records plus qs; vectors where the weights flip the winner; every two-way
    tie; S above 2^32 through wrapped columns; a PL saturated; depth d - 1 and d"""
    c = gctx
    t, per_site = crafted_text()
    where = begin(c, t)
    counts = np.array([v for _, _, v in per_site], dtype=np.uint32)
    c.pile_put(0, counts)
    groups = sorted({(e, d) for e, d, _ in per_site})
    n_exact = 0
    for E, D in groups:
        sums = (counts.astype(np.uint64) * E % (1 << 32)).astype(np.uint32)  # (a column of 0xFFFFFFFF bases wraps, as the table does)
        c.pileq_put(0, sums)
        got = c.geno_sites_q(0, len(where), E, D)
        want = pileq_model.site_records_q(t, counts, sums, D)
        assert got.tobytes() == want.tobytes(), (E, D, len(got), len(want))
        plain = c.geno_sites(0, len(where), E, D)
        exact = np.array([(int(r["n"].astype(np.uint64).max()) * E) < (1 << 32) for r in plain], dtype=bool)  # where no sum wrapped: the existing rule, number for number
        assert len(plain) == len(got)
        n_exact += int(exact.sum())
        for f in bw.GENO_SITE_DTYPE.names:
            assert np.array_equal(got[f][exact], plain[f][exact]), (E, D, f)
        assert np.array_equal(got["qs"], sums[got["site"].astype(np.int64)]) and c.geno_stats()[0] == len(want)
    assert n_exact > 1000
    # crafted for the weights, on the text's first sites of each code (counts, sums by column) - `what` names the property asserted below
    letters = [t[p] for p in where]
    counts[:], sums = 0, np.zeros_like(counts)
    crafted = {}

    def put(letter, what, n, s, other=(0, 0)):
        site = next(k for k, ltr in enumerate(letters) if ltr == letter and k not in crafted.values())
        cols = member_cols(letter)
        for col, a, b in zip(cols, n, s):
            counts[site, col], sums[site, col] = a, b
        free = next(col for col in range(4) if col not in cols)
        counts[site, free], sums[site, free] = other
        crafted[(letter, what)] = site
    for letter in geno_model.MEMBERS:
        k = len(member_cols(letter))
        z = [0] * (k - 2)
        put(letter, "flip", [3, 2] + z, [12, 80] + z)             # three Q4 bases of a0 against two Q40 of a1: a1/a1 by weight, a0/a1 by count at E = 40
        put(letter, "wrapped", [0xFFFFFFFF, 0xFFFFFFFF] + z, [0xFFFFFFFF, 0xFFFFFFF0] + z, (0xFFFFFFFF, 0xFFFFFFFF))  # S above 2^32
        put(letter, "pl_saturated", [0xFFFFFFFF, 0] + z, [0xFFFFFFFF, 0] + z)      # raw(1,1) - raw(0,0) = s_0; the het's H n_0 saturates
        put(letter, "depth_below", [3, 2] + z, [30, 20] + z)
        put(letter, "depth_at", [3, 3] + z, [30, 30] + z)
    c.pile_put(0, counts)
    c.pileq_put(0, sums)
    got = c.geno_sites_q(0, len(where), 40, 1)
    want = pileq_model.site_records_q(t, counts, sums, 1)
    assert got.tobytes() == want.tobytes() and len(got) == len(crafted)
    by_site = {int(r["site"]): r for r in got}
    for letter in geno_model.MEMBERS:
        r = by_site[crafted[(letter, "flip")]]
        al = [int(r["n"][col]) for col in member_cols(letter)]
        assert int(r["gt"]) == 2 and geno_model.rule(al, sum(al), 40)[0] == 1, letter   # the weights flip the winner
        r = by_site[crafted[(letter, "wrapped")]]
        assert int(r["qs"].astype(np.uint64).sum()) > (1 << 32)
        r = by_site[crafted[(letter, "pl_saturated")]]
        assert int(r["gt"]) == 0 and int(r["pl"].max()) == geno_model.PL_MAX and int(r["gq"]) == 99
    at6 = c.geno_sites_q(0, len(where), 40, 6)
    assert {crafted[(ltr, "depth_at")] for ltr in geno_model.MEMBERS} <= {int(s) for s in at6["site"]}
    assert not {crafted[(ltr, "depth_below")] for ltr in geno_model.MEMBERS} & {int(s) for s in at6["site"]}
    # every two-way tie of the weighted costs, searched for over small counts and weights (a base weighs 4..12): the first genotype in VCF order
    # wins, GQ 0.  The weights allow all 3 pairs of two alleles' genotypes and all 15 of three alleles' - also the three the counts alone cannot tie
    import random
    for letter in ("K", "B"):
        k = len(member_cols(letter))
        ng = geno_model.n_geno(k)
        found = {}
        rnd = random.Random(k)
        for _ in range(200_000):
            if len(found) == ng * (ng - 1) // 2:
                break
            n = [rnd.randrange(6) for _ in range(k)]
            s = [rnd.randrange(4 * a, 12 * a + 1) if a else 0 for a in n]
            o = rnd.randrange(3)
            so = rnd.randrange(4 * o, 12 * o + 1) if o else 0
            S = sum(s) + so
            raw = [S - s[x] if x == y else 3 * (n[x] + n[y]) + S - s[x] - s[y] for x, y in geno_model.GENOTYPES[:ng]]
            low = [j for j in range(ng) if raw[j] == min(raw)]
            if len(low) == 2 and tuple(low) not in found:
                found[tuple(low)] = (n, s, (o, so))
        assert len(found) == ng * (ng - 1) // 2 >= geno_model.TWO_WAY_TIES[k], (letter, sorted(found))
        site = next(i for i, ltr in enumerate(letters) if ltr == letter)
        for pair, (n, s, other) in found.items():
            counts[:], sums[:] = 0, 0
            cols = member_cols(letter)
            for col, a, b in zip(cols, n, s):
                counts[site, col], sums[site, col] = a, b
            free = next(col for col in range(4) if col not in cols)
            counts[site, free], sums[site, free] = other
            c.pile_put(0, counts)
            c.pileq_put(0, sums)
            got = c.geno_sites_q(site, 1, 20, 1)
            assert got.tobytes() == pileq_model.site_records_q(t, counts, sums, 1, site, 1).tobytes() and len(got) == 1
            assert int(got[0]["gt"]) == pair[0] and int(got[0]["gq"]) == 0 and int(got[0]["pl"][pair[1]]) == 0, (letter, pair)


def test_ranges_and_pieces_of_the_weighted_calls(gctx):
    """n = 1, 7, the piece and the whole table, at both ends; pieces of 1 000 concatenated"""
    c = gctx
    rng = np.random.default_rng(8)
    t = "".join(rng.choice(list("ACGT" * 5 + pile_model.NT16[1:]), 20011))
    n = len(pile_model.sites(t))
    counts = rng.integers(0, 40, (n, 4)).astype(np.uint32)
    counts[rng.random(n) < 0.3] = 0
    counts[2000:2300] = 0
    counts[0] = counts[n - 1] = (3, 0, 2, 1)
    sums = (counts * rng.integers(4, 41, (n, 4))).astype(np.uint32)
    begin(c, t, n)
    c.pile_put(0, counts)
    c.pileq_put(0, sums)
    whole = pileq_model.site_records_q(t, counts, sums, 2)
    assert c.geno_sites_q(0, n, 20, 2).tobytes() == whole.tobytes() and len(whole) > 2000
    for first, k in ((0, 1), (0, 7), (n - 1, 1), (n - 7, 7), (n, 0), (0, 0), (2000, 300), (1999, 302), (n // 2, 1000)):
        assert c.geno_sites_q(first, k, 20, 2).tobytes() == pileq_model.site_records_q(t, counts, sums, 2, first, k).tobytes(), (first, k)
    begin(c, t, 1000)
    c.pile_put(0, counts)
    c.pileq_put(0, sums)
    parts = [c.geno_sites_q(s0, min(1000, n - s0), 20, 2) for s0 in range(0, n, 1000)]
    assert np.concatenate(parts).tobytes() == whole.tobytes() and len(parts) > 4
    with pytest.raises(bw.BwbError, match="error -1.*geno_sites_q"):
        c.geno_sites_q(0, 1001, 20, 2)
    for first, k in ((0, n + 1), (n, 1), ((1 << 64) - 1, 2)):
        with pytest.raises(bw.BwbError, match="error -1.*geno_sites_q"):
            c.geno_sites_q(first, k, 20, 2)


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_slots_equal_the_model_fed_the_oracles_hits(built, pad_text, lib):
    """the pad_bub reads with rewritten qualities in one batch - plain, lifted, joined - and through all eight slots with parked reads: the stream's
    tables are the batch's, the model's; a second slot_pile_q, and a slot_pile after a slot_pile_q, add nothing"""
    env = dict(os.environ, BWB_SLICE_ITERS="150")
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pileq_slots_worker.py"), pad_text], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "PILEQ-SLOTS-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


def test_errors_leave_the_context_usable(built, golden, pad_text, toy):
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    quals = ramps(lens, seqs.shape[1], 20, 1)
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    c = bw.Context(b)
    one = (seqs[:1], quals[:1], lens[:1], lift_model.place_records([(5, False, f"{int(lens[0])}M")]))
    p = bw.params(["-n", "3"])
    try:
        c.set_text(pile_model.codes(toy.text))
        with pytest.raises(bw.BwbError, match="error -4.*pile_begin"):
            c.pileq_begin(True)
        n_sites = c.pile_begin()
        c.set_sa(b.SA)
        for call in (lambda: c.slot_quals(0, quals), lambda: c.slot_pile_q(0), lambda: c.batch_pile_q(), lambda: c.pile_records_q(*one)):
            with pytest.raises(bw.BwbError, match="error -4.*pileq_begin"):
                call()
        for call in (lambda: c.pileq_sums(0, 0), lambda: c.pileq_put(0, np.zeros((0, 4), dtype=np.uint32))):
            with pytest.raises(bw.BwbError, match="error -4.*pileq_begin"):
                call()
        c.pileq_begin(False)
        c.geno_begin(n_sites)
        for call in (lambda: c.pileq_sums(0, 0), lambda: c.pile_records_q(*one, err_cap=20), lambda: c.geno_sites_q(0, 1)):
            with pytest.raises(bw.BwbError, match="error -4.*weighted"):
                call()
        c.pile_records_q(*one, min_baseq=20)  # (unweighted needs no sums)
        assert c.pileq_stats()[0] == 1
        c.pileq_begin(True)
        with pytest.raises(bw.BwbError, match="error -4.*geno_begin"):
            c.geno_sites_q(0, 1)  # (the output was sized for the 64-byte records: geno_begin comes after the weighted pileq_begin)
        c.geno_begin(n_sites)
        assert len(c.geno_sites_q(0, n_sites)) == len(c.geno_sites(0, n_sites)) > 0  # (the one read counted above)
        for bad in (lambda: c.pile_records_q(*one, min_baseq=94), lambda: c.pile_records_q(*one, min_baseq=-1), lambda: c.pile_records_q(*one, err_cap=3), lambda: c.pile_records_q(*one, err_cap=94),
                    lambda: c.pile_records_q(*one, err_cap=-4), lambda: c.slot_pile_q(0, min_baseq=94), lambda: c.batch_pile_q(err_cap=1), lambda: c.slot_pile_q(-1), lambda: c.slot_pile_q(bw.MAX_SLOTS),
                    lambda: c.slot_quals(bw.MAX_SLOTS, quals), lambda: c.geno_sites_q(0, 1, 3), lambda: c.geno_sites_q(0, 1, 20, 0)):
            with pytest.raises(bw.BwbError, match="error -1"):
                bad()
        with pytest.raises(bw.BwbError, match="error -4.*no upload"):
            c.slot_quals(0, quals)
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            c.slot_pile_q(3)
        c.upload(p, seqs, lens)
        with pytest.raises(bw.BwbError, match="error -1.*stride"):
            c.slot_quals(0, quals, stride=seqs.shape[1] + 1)
        c.run()
        with pytest.raises(bw.BwbError, match="error -4.*slot_quals"):
            c.batch_pile_q(min_baseq=20, err_cap=30)  # (a batch without qualities)
        c.pile_reset()
        c.slot_quals(0, quals)
        counted = c.batch_pile_q(min_baseq=20, err_cap=30)
        reads, adds, dropped, ms = c.pileq_stats()
        assert counted == reads == 569 and adds + dropped == 556 and dropped > 0 and c.pile_counts(0, n_sites).sum() == adds
        sums = c.pileq_sums(0, n_sites)
        assert 4 * adds <= int(sums.sum()) <= 30 * adds
        assert c.batch_pile_q(min_baseq=20, err_cap=30) == 0 and c.batch_pile() == 0 and c.pile_counts(0, n_sites).sum() == adds  # (a submission is piled once: the flag is shared)
        c.upload(p, seqs[:10], lens[:10])
        c.run()
        with pytest.raises(bw.BwbError, match="error -4.*slot_quals"):
            c.batch_pile_q()  # (the upload forgot the qualities)
        assert c.batch_pile() > 0 and c.batch_pile_q() == 0  # (and slot_pile's flag holds for slot_pile_q)
        # pile_reset zeroes the sums too; a later pile_begin forgets pileq_begin
        c.pile_reset()
        assert not c.pileq_sums(0, n_sites).any()
        assert c.pile_begin() == n_sites
        with pytest.raises(bw.BwbError, match="error -4.*pileq_begin"):
            c.pileq_sums(0, 0)
        c.pile_records(one[0], one[2], one[3])
        assert c.pile_stats()[0] == 1
    finally:
        c.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def qfq(pad_text, md_dir):
    """the pad_bub reads with rewritten quality lines"""
    data, quals = pileq_model.requal_fastq(open(os.path.join(pad_text, "pad_bub.fq"), "rb").read(), 12)
    open(md_dir / "q.fq", "wb").write(data)
    return md_dir / "q.fq", quals


FULL = ["-J", "-R", "-D"]
RUNS = dict(VARIANTS, four_workers=(["-g", "4"], {"BWB_DEVICE_MAP": "0,0,0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1", "BWB_DEBUG": "1"}), count_piece_7=([], {"BWB_COUNT_PIECE": "7"}))


@pytest.fixture(scope="module")
def chain(md_dir, golden, qfq, fx):
    """the CPU-only chain on the same reads: the models' placement records and items through `places2sam`, with and without -b 20 -Y -q 30"""
    fq, _ = qfq
    pf, af = write_inputs(fx, md_dir)
    data = os.path.join(golden, "pad_toy.data")
    p = lambda n: str(md_dir / f"chain.{n}")
    out = {}
    for what, more in (("plain", []), ("q", ["-q", "30", "-b", "20", "-Y"])):
        cli(["places2sam", "-B", data] + FULL + ["-A", p("a"), "-a", "1", "-I", p("i"), "-w", "5", "-G", p("g")] + more + [md_dir / "toy.fa", fq, pf, p("sam"), af])
        out[what] = {n: open(p(n), "rb").read() for n in ("sam", "a", "i", "g")}
    assert out["plain"]["sam"] == out["q"]["sam"] and out["plain"]["i"] == out["q"]["i"] and out["plain"]["a"] != out["q"]["a"] and out["q"]["g"].startswith(pileq_model.HEADER_Q)
    return out


@pytest.mark.parametrize("run", list(RUNS))
def test_cli_map_writes_the_chains_bytes(md_dir, golden, qfq, chain, run):
    """`map -n 3 -o 1 -X 5 -B t -J -R -D -A a -I i -G f -a 1 -w 5 -b 20 -Y -q 30` in one chunk, in chunks of 97, with two and four workers and with
    BWB_COUNT_PIECE=7: the CPU-only chain's bytes; the SAM and -I bytes of the run without -b -Y"""
    extra, env = RUNS[run]
    fq, _ = qfq
    p = lambda n: str(md_dir / f"cli_{run}.{n}")
    base = ["map", "-n", "3", "-o", "1", "-X", "5", "-B", os.path.join(golden, "pad_toy.data")] + FULL + ["-A", p("a"), "-I", p("i"), "-G", p("g"), "-a", "1", "-w", "5"]
    log = cli(base + ["-b", "20", "-Y", "-q", "30"] + extra + [md_dir / "toy.fa", fq, p("sam")], env)
    got = {n: open(p(n), "rb").read() for n in ("sam", "a", "i", "g")}
    for n in got:
        assert got[n] == chain["q"][n], (n, pad_model.first_difference(got[n], chain["q"][n]))
    assert "base qualities in the counts on the GPU (k_pile_q): minimum 20  bases dropped " in log and "quality sums kept (-Y)" in log, log[-2000:]
    if run in ("one_chunk", "four_workers"):  # without -b -Y (and with -b 0): every file of the parent's command, nothing of it uploaded or launched
        for more in ([], ["-b", "0"]):
            log0 = cli(base + more + extra + [md_dir / "toy.fa", fq, p("sam")], env)
            assert {n: open(p(n), "rb").read() for n in got} == chain["plain"] and "base qualities" not in log0
    if run == "four_workers":
        called = [ln for ln in log.split("\n") if "genotypes called by this worker, the last of 4" in ln]
        assert len(called) == 1 and " 3 pieces of tables put back" in called[0], log[-3000:]  # counters, sums, bubbles


def test_cli_map_with_a_minimum_base_quality_alone_and_aln2sam(md_dir, golden, qfq, toy, tmp_path):
    """`map -n 3 -A a -b 20`: the model's counts of the SAM text it writes; and `align` + `aln2sam ... -b m -Y -G f` writes `map`'s files"""
    fq, quals = qfq
    fa = md_dir / "toy.fa"
    log = cli(["map", "-n", "3", "-A", tmp_path / "a.tsv", "-b", "20", fa, fq, tmp_path / "m.sam"])
    sam = open(tmp_path / "m.sam", "rb").read()
    counts, _, reads, adds, dropped = pileq_model.pile_sam_q(sam, toy.text, toy.names, toy.starts, 0, 20, 0)
    assert open(tmp_path / "a.tsv", "rb").read() == pile_model.tsv(toy.text, toy.names, toy.starts, counts)
    assert f"reads counted {reads}  adds {adds} " in log and f"minimum 20  bases dropped {dropped}  quality sums not kept" in log and dropped > 0
    cli(["align", "-n", "3", "-o", "1", fa, fq, tmp_path / "t.aln"])
    data = os.path.join(golden, "pad_toy.data")
    for opts in (["-A", "A", "-b", "1"], ["-G", "G", "-q", "93", "-Y"], ["-X", "5", "-B", data, "-J", "-R", "-D", "-A", "A", "-I", "I", "-G", "G", "-a", "1", "-w", "5", "-b", "20", "-Y", "-q", "30"]):
        files = [o for o in opts if o in ("A", "I", "G")]
        for tool, tail in (("m", ["map", "-n", "3", "-o", "1"]), ("a", ["aln2sam"])):
            cli(tail + [str(tmp_path / f"{tool}.{o}") if o in files else o for o in opts] + [fa, fq] + ([tmp_path / "t.aln"] if tool == "a" else []) + [tmp_path / f"{tool}.sam"])
        for f in files + ["sam"]:
            m, a = open(tmp_path / f"m.{f}", "rb").read(), open(tmp_path / f"a.{f}", "rb").read()
            assert m == a and len(m) > 100, (opts, f, pad_model.first_difference(m, a))
