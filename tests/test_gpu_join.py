"""A read's placements counted by locus on the GPU (`map -X N -B table -J`): kernels k_join_items / k_join_reads through
Context.join_records on injected records - record tables of every shape of the search, the pad_synth bubble table, reads with 0 .. 255 items
of every relation to their primary - against the Python restatement of the rule (tests/join_model.py; pinned to the truth in the pad_bub
reads' names by tests/test_join_host.py); through Context.join / slot_join on the pad_bub reads, on the product and on the test build, against
the model fed the ORACLE's hits (tests/join_slots_worker.py); the state and argument errors; and the command line."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import join_model
import map_model
import oracle_lib
import pad_model
from test_gpu_map import cli, compute_units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_LEN, REC_GAP, REC_BASE = 6000, 5, 1000  # the injected tables: records of 6000 positions (every small coordinate of pad_synth.data is a position of a chromosome record), 5 apart


@pytest.fixture(scope="module")
def synth_bubbles(golden):
    return pad_model.load_bubbles(os.path.join(golden, "pad_synth.data"))


@pytest.fixture(scope="module")
def toy_ctx(built, golden):
    ctx = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    yield ctx
    ctx.close()


def table(n_seq, n_bub):
    """n_seq disjoint records in text order: every third one (0, 3, ..) a chromosome, the others bubble records with the bubbles taken in turn;
    bubble b lies on chromosome record 3 * (b % chromosomes) - two bubbles of the table share a chromosome as soon as there are fewer of them"""
    start = REC_BASE + np.arange(n_seq, dtype=np.uint64) * np.uint64(REC_LEN + REC_GAP)
    end = start + np.uint64(REC_LEN - 1)
    i = np.arange(n_seq)
    bub_of = np.where(i % 3 == 0, -1, (i - i // 3 - 1) % n_bub).astype(np.int32)
    n_chrom = (n_seq + 2) // 3
    chrom = (3 * (np.arange(n_bub) % min(n_chrom, 3))).astype(np.int32)
    return types.SimpleNamespace(start=start, end=end, bub_of=bub_of, chrom=chrom)


def candidates(t, bubbles, rng):
    """text positions worth placing a read at: in every sampled bubble record the loci at which sam_pad's rule changes its answer; in every
    sampled chromosome record the coordinates those answers name (and their neighbours); the ends of records, gaps, beyond the table"""
    n = len(t.start)
    recs = sorted(set(range(min(n, 12))) | {n // 2, n - 1} | set(int(v) for v in rng.integers(0, n, 6)))
    coords = {1, 2, REC_LEN}
    loci = {1, 2, REC_LEN - 1, REC_LEN}
    for _, A, B, C, D, ref_len, alt_len in bubbles:
        loci |= {B, B + 1, B + alt_len, B + alt_len + 1, B + alt_len + 2, B + alt_len + D + 1, B + alt_len + D + 2}
        coords |= {A, A + 1, A + B - 1, A + B, A + B + 1, A + B + ref_len - 1, A + B + ref_len, C, C + 1, C + D}
    pos = [0, REC_BASE - 1, int(t.end[-1]) + 1, int(t.end[-1]) + 10**9]
    for i in recs:
        s = int(t.start[i])
        pos += [int(t.end[i]) + 1] + [s + v - 1 for v in sorted(loci if t.bub_of[i] >= 0 else coords) if 1 <= v <= REC_LEN]
    return np.array(sorted(set(pos)), dtype=np.uint64)


# reads 0 .. 6 of every injected set, one per branch of mapq: (top1, top2, num_mm, [(the item lies where the primary lies, it is suboptimal)]) -> MAPQ with -Q 6 / 3
BRANCHES = [
    (2, 0, 0, [(True, False)]),                                                # one best placement left, nothing else: 37
    (2, 0, 3, [(True, False)]),                                                # ... at the mismatch limit 3: 37 / 25
    (2, 0, 6, [(True, False)]),                                                # ... at the mismatch limit 6: 25 / 37
    (2, 3, 0, [(True, False), (False, True), (False, True), (False, True)]),   # three suboptimal placements elsewhere: 23 - (int)(4.343 ln 3 + .5) = 18
    (1, 2, 0, [(True, True), (True, True)]),                                   # both suboptimal placements joined: 37
    (3, 0, 0, [(True, False), (False, False)]),                                # two best placements left: 0
    (2, 2, 0, [(True, False), (True, True), (False, True)]),                   # one suboptimal placement left: 23
]
BRANCH_MAPQ = {6: [37, 37, 25, 18, 37, 0, 23], 3: [37, 25, 37, 18, 37, 0, 23]}


def injected(t, bubbles, seed, n_reads=600):
    """reads with 0 .. 12 items, one with 255 and one with 255 copies of its primary: the items drawn from the candidates of the primary's
    chromosome four times in five, the strand mostly the primary's; top1 / top2 the counts eval_aln would have summed plus a few more; and
    the seven reads of BRANCHES in front"""
    rng = np.random.default_rng(seed)
    cand = candidates(t, bubbles, rng)
    has, c, _, _, _ = join_model.loci4(cand, np.full(len(cand), bw.PLACE_MAPPED, dtype=np.uint8), t.start, t.end, t.bub_of, bubbles, t.chrom)
    by_chrom = {int(k): cand[has & (c == k)] for k in np.unique(c[has])}
    places = np.zeros(n_reads, dtype=bw.PLACE_DTYPE)
    places["pos"] = cand[rng.integers(0, len(cand), n_reads)]
    places["flags"] = np.where(rng.integers(0, 16, n_reads) == 0, 0, bw.PLACE_MAPPED).astype(np.uint8) | np.where(rng.integers(0, 2, n_reads) == 0, bw.PLACE_REVERSE, 0).astype(np.uint8)
    places["num_mm"] = rng.integers(0, 7, n_reads)
    places["pos"][n_reads // 2], places["flags"][n_reads // 2] = t.start[0] + np.uint64(1), bw.PLACE_MAPPED  # (the read with 255 copies of its primary)
    places["score"], places["aln_length"], places["ref_len"] = 3, 100, 100
    cnt = rng.choice([0, 0, 1, 1, 2, 3, 5, 12], n_reads)
    cnt[7], cnt[n_reads // 2] = 255, 255
    cnt[:len(BRANCHES)] = [len(items) for _, _, _, items in BRANCHES]
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(cnt)
    alts = np.zeros(int(off[-1]), dtype=bw.ALT_DTYPE)
    owner = np.repeat(np.arange(n_reads), cnt)
    ph, pc, _, _, _ = join_model.loci4(places["pos"], places["flags"], t.start, t.end, t.bub_of, bubbles, t.chrom)
    for q, r in enumerate(owner):
        pool = by_chrom[int(pc[r])] if ph[r] and rng.integers(0, 5) else cand
        alts["pos"][q] = places["pos"][r] if r == n_reads // 2 else pool[rng.integers(0, len(pool))]
    alts["flags"] = (places["flags"][owner] & bw.PLACE_REVERSE) ^ np.where(rng.integers(0, 6, len(alts)) == 0, bw.PLACE_REVERSE, 0).astype(np.uint8)
    alts["flags"] |= np.where(rng.integers(0, 40, len(alts)) == 0, 0, bw.PLACE_MAPPED).astype(np.uint8)
    alts["flags"][owner == n_reads // 2] = places["flags"][n_reads // 2] | bw.PLACE_MAPPED
    alts["hit"], alts["aln_length"] = rng.integers(0, 4, len(alts)), 100
    sub = (rng.integers(0, 3, len(alts)) == 0).astype(np.uint8)
    sub[owner == n_reads // 2] = 0
    extra = rng.choice([0, 0, 0, 1, 300], n_reads)
    places["top1"] = 1 + np.bincount(owner[sub == 0], minlength=n_reads) + np.where(rng.integers(0, 4, n_reads) == 0, extra, 0)
    places["top2"] = np.bincount(owner[sub != 0], minlength=n_reads) + np.where(rng.integers(0, 4, n_reads) == 0, extra, 0)
    for r, (top1, top2, num_mm, items) in enumerate(BRANCHES):  # on chromosome record 0, the items that do not join 99 positions further on
        places["pos"][r], places["flags"][r], places["top1"][r], places["top2"][r], places["num_mm"][r] = t.start[0] + np.uint64(1), bw.PLACE_MAPPED, top1, top2, num_mm
        q = int(off[r])
        alts["pos"][q:q + len(items)] = [int(t.start[0]) + (1 if here else 100) for here, _ in items]
        alts["flags"][q:q + len(items)], sub[q:q + len(items)] = bw.PLACE_MAPPED, [s for _, s in items]
    places["mapq"] = [map_model.mapq(int(a), int(b), int(m), 6) for a, b, m in zip(places["top1"], places["top2"], places["num_mm"])]
    return places, off, alts, sub


def same_joins(got, want, what=""):
    assert join_model.first_difference(got, want) is None, (what, join_model.first_difference(got, want))
    assert got.tobytes() == want.tobytes(), what


def relations(t, bubbles, places, off, alts):
    """the census of the injected items: which relation to its primary each one has"""
    owner, joined = join_model.item_classes(places, off, alts, t.start, t.end, t.bub_of, bubbles, t.chrom)
    as_places = np.zeros(len(alts), dtype=bw.PLACE_DTYPE)
    as_places["pos"], as_places["flags"] = alts["pos"], alts["flags"]
    il, pl = pad_model.expected_loci(as_places, t.start, t.end, t.bub_of, bubbles), pad_model.expected_loci(places, t.start, t.end, t.bub_of, bubbles)[owner]
    hi, ci, si, loi, hii = join_model.loci4(alts["pos"], alts["flags"], t.start, t.end, t.bub_of, bubbles, t.chrom)
    hp, cp, sp, lop, hip = (a[owner] for a in join_model.loci4(places["pos"], places["flags"], t.start, t.end, t.bub_of, bubbles, t.chrom))
    point = lambda lc: (lc["seqid"] >= 0) & (lc["kind"] != bw.LOCUS_RANGE)
    rng_ = lambda lc: lc["kind"] == bw.LOCUS_RANGE
    empty = lambda lc: rng_(lc) & (lc["ref_hi"] < lc["ref_lo"])
    overlap = hi & hp & (loi <= hip) & (lop <= hii)
    return {
        "same point": int((joined & point(il) & point(pl)).sum()),
        "point in a range": int((joined & (point(il) ^ point(pl)) & ~empty(il) & ~empty(pl)).sum()),
        "range and range": int((joined & rng_(il) & rng_(pl)).sum()),
        "an empty range": int((joined & (empty(il) | empty(pl))).sum()),
        "a chromosome and a bubble record": int((joined & ((il["bubble"] >= 0) ^ (pl["bubble"] >= 0))).sum()),
        "above 2^32": int((joined & (loi > 2**32)).sum()),
        "the other strand": int((overlap & (ci == cp) & (si != sp)).sum()),
        "another chromosome, the same numbers": int((overlap & (ci != cp) & (si == sp)).sum()),
        "the same chromosome, elsewhere": int((hi & hp & (ci == cp) & (si == sp) & ~overlap).sum()),
        "in no record": int((~hi).sum()),
    }


@pytest.mark.parametrize("max_mm", [6, 3])
@pytest.mark.parametrize("n_seq", [1, 2, 3, 7, 8, 9, 1_300_000])
def test_join_records_equals_the_model_on_injected_records(toy_ctx, synth_bubbles, n_seq, max_mm):
    """record tables around the powers of two of the search's step count and one of the GRCh37 shape; the pad_synth bubbles (alt_len 0, ref_len
    0 / 1 / 5, B_minus_A 0, D_minus_C -1, A and C above 2^32)"""
    t = table(n_seq, len(synth_bubbles))
    places, off, alts, sub = injected(t, synth_bubbles, n_seq)
    want, total = join_model.expected_joins(places, off, alts, sub, t.start, t.end, t.bub_of, synth_bubbles, t.chrom, max_mm)
    toy_ctx.set_loci(t.start, t.end, t.bub_of, pad_model.bubble_records(synth_bubbles))
    toy_ctx.set_bubble_chrom(t.chrom)
    same_joins(toy_ctx.join_records(places, off, alts, sub, max_mm), want, n_seq)
    items, joined, ms = toy_ctx.join_stats()
    assert (items, joined) == (len(alts), total) and ms > 0
    assert want["joined"].max() == 255 and (np.diff(off) == 255).sum() == 2 and ((off[:-1] // 256) != ((off[1:] - 1) // 256))[np.diff(off) > 0].any()  # a read's items straddle a block
    census = relations(t, synth_bubbles, places, off, alts)
    always = ["same point", "the other strand", "the same chromosome, elsewhere", "in no record"]
    if n_seq >= 7:  # several chromosomes and bubble records; from nine records on, one of a bubble above 2^32
        always += ["point in a range", "range and range", "an empty range", "a chromosome and a bubble record", "another chromosome, the same numbers"]
        always += ["above 2^32"] if n_seq >= 9 else []
    assert all(census[k] >= 1 for k in always), census
    # every branch of mapq on a read that joined something: more than one best placement left, the mismatch limit, nothing else, something else
    j = want["joined"] > 0
    got_q = set(want["mapq"][j].tolist())
    assert want["mapq"][:len(BRANCHES)].tolist() == BRANCH_MAPQ[max_mm] and j[:len(BRANCHES)].all() and {0, 18, 23, 25, 37} <= got_q, got_q
    assert (want["mapq"][j] != places["mapq"][j]).any() and (want["top2"][j] < places["top2"][j]).any() and (want["top1"][j] < places["top1"][j]).any()
    unmapped = (places["flags"] & bw.PLACE_MAPPED) == 0
    none = (np.diff(off) == 0) & ~unmapped
    assert none.any() and (want["mapq"][none] == places["mapq"][none]).all()  # verbatim, whatever max_mm says
    assert unmapped.any() and want[unmapped].tobytes() == bytes(16 * int(unmapped.sum()))


@pytest.fixture(scope="module")
def grch37_shape(synth_bubbles):
    t = table(1_300_000, len(synth_bubbles))
    places, off, alts, sub = injected(t, synth_bubbles, 37, n_reads=4099)
    want, total = join_model.expected_joins(places, off, alts, sub, t.start, t.end, t.bub_of, synth_bubbles, t.chrom, 6)
    return types.SimpleNamespace(t=t, places=places, off=off, alts=alts, sub=sub, want=want, total=total)


def load(ctx, g, bubbles):
    ctx.set_loci(g.t.start, g.t.end, g.t.bub_of, pad_model.bubble_records(bubbles))
    ctx.set_bubble_chrom(g.t.chrom)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_join_records_on_a_few_reads(toy_ctx, synth_bubbles, grch37_shape, n):
    """less than a wave, exactly one, one more; and none (no launch)"""
    g = grch37_shape
    load(toy_ctx, g, synth_bubbles)
    k = int(g.off[n])
    same_joins(toy_ctx.join_records(g.places[:n], g.off[:n + 1], g.alts[:k], g.sub[:k]), g.want[:n], n)
    items, joined, ms = toy_ctx.join_stats()
    assert (items, joined) == (k, int(g.want["joined"][:n].sum())) and (ms > 0) == (n > 0)


def test_join_records_without_items(toy_ctx, synth_bubbles, grch37_shape):
    """no item anywhere: only k_join_reads runs, every record is its placement record's"""
    g = grch37_shape
    load(toy_ctx, g, synth_bubbles)
    got = toy_ctx.join_records(g.places, np.zeros(len(g.places) + 1, dtype=np.uint64), g.alts[:0], g.sub[:0])
    mapped = (g.places["flags"] & bw.PLACE_MAPPED) != 0
    for f in ("top1", "top2", "mapq"):
        assert (got[f] == np.where(mapped, g.places[f], 0)).all(), f
    assert not got["joined"].any() and toy_ctx.join_stats()[:2] == (0, 0)


def test_join_records_strides_over_more_reads_and_items_than_the_grid_has_lanes(toy_ctx, synth_bubbles, grch37_shape):
    """the production path of both loops: more than twice 8 * CUs * 256 reads (and more items than that), so that every lane takes a third"""
    g = grch37_shape
    cus = compute_units()
    times = (2 * 8 * cus * 256) // len(g.places) + 1
    n = times * len(g.places)
    assert n > 2 * 8 * cus * 256 and times * len(g.alts) > 2 * 8 * cus * 256
    load(toy_ctx, g, synth_bubbles)
    off = np.concatenate([[0], np.cumsum(np.tile(np.diff(g.off), times))]).astype(np.uint64)
    got = toy_ctx.join_records(np.tile(g.places, times), off, np.tile(g.alts, times), np.tile(g.sub, times))
    same_joins(got, np.tile(g.want, times), f"{n} reads on {cus} CUs")
    assert toy_ctx.join_stats()[:2] == (times * len(g.alts), times * g.total)


# ---- the pad_bub reads on the toy index -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pad_text(tmp_path_factory):
    return pad_model.unpack(tmp_path_factory.mktemp("joingpu"))


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_join_and_slot_join_equal_the_model_fed_the_oracles_hits(built, pad_text, lib):
    """one batch with -Q 6 / 3 and -X 5 / 1, then through all eight slots with parked reads - on the product and on the test build"""
    env = dict(os.environ, BWB_SLICE_ITERS="150")
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_slots_worker.py"), pad_text], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "JOIN-SLOTS-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


@pytest.fixture(scope="module")
def toy_tables(golden):
    names, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
    anns, recs = bw.read_bubble_data(os.path.join(golden, "pad_toy.data"))
    bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
    return types.SimpleNamespace(names=names, start=start, end=end, bub_of=pad_model.bubble_of(names, bubbles), bubbles=bubbles, recs=recs, chrom=join_model.chrom_of(names, bubbles))


@pytest.fixture(scope="module")
def model(golden, oracle, pad_text, toy_tables):
    """the model's records of the pad_bub reads from the REFERENCE's hits (-X 5), and the text it predicts"""
    t = toy_tables
    idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(pad_text, "pad_bub_n3.aln"), "rb").read())
    places, _ = map_model.expected_places(oracle, idx, reads, 6)
    off, alts, _ = alt_model.expected_alts(reads, 5, alt_model.OracleSA(oracle, idx))
    sub = join_model.suboptimal(reads, off, alts)
    joins, total = join_model.expected_joins(places, off, alts, sub, t.start, t.end, t.bub_of, t.bubbles, t.chrom, 6)
    with_x = alt_model.expected_sam(open(os.path.join(pad_text, "pad_bub_n3.sam")).read(), places, off, alts, alt_model.read_ann(os.path.join(golden, "toy.fa.ann"))).encode()
    padded = pad_model.pad_sam(with_x, t.bubbles)
    return types.SimpleNamespace(places=places, off=off, alts=alts, sub=sub, joins=joins, total=total, padded=padded, text=join_model.apply_to_sam(padded, places, joins))


def test_join_errors_leave_the_context_usable(built, golden, pad_text, toy_tables, model):
    t = toy_tables
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    ctx = bw.Context(b)
    try:
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            ctx.set_bubble_chrom(t.chrom)
        for call in (lambda: ctx.join(), lambda: ctx.slot_join(0), lambda: ctx.join_records(model.places, model.off, model.alts, model.sub)):
            with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
                call()
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        for call in (lambda: ctx.join(), lambda: ctx.slot_join(0), lambda: ctx.join_records(model.places, model.off, model.alts, model.sub)):
            with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
                call()
        # another number of bubbles, a record outside the table, below it, a bubble record: refused, and still no table
        for bad in (t.chrom[:3], np.append(t.chrom, 0), np.where(np.arange(4) == 1, len(t.start), t.chrom), np.where(np.arange(4) == 1, -1, t.chrom), np.where(np.arange(4) == 2, 5, t.chrom)):
            with pytest.raises(bw.BwbError, match="error -1.*set_bubble_chrom"):
                ctx.set_bubble_chrom(bad)
        with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
            ctx.join()
        ctx.set_bubble_chrom(t.chrom)
        same_joins(ctx.join_records(model.places, model.off, model.alts, model.sub), model.joins)  # (needs no SA and no batch)
        for call in (lambda: ctx.join(), lambda: ctx.slot_join(0)):
            with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
                call()
        ctx.set_sa(b.SA)
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            ctx.slot_join(3)
        for slot in (-1, bw.MAX_SLOTS):
            with pytest.raises(bw.BwbError, match="error -1"):
                ctx.slot_join(slot)
        for max_alt in (0, 256, -1):
            with pytest.raises(bw.BwbError, match="error -1.*max_alt"):
                ctx.slot_join(0, 6, max_alt)
            with pytest.raises(bw.BwbError, match="error -1.*max_alt"):
                ctx.join(6, max_alt)
        # offsets that do not start at 0, descend, or give a read 256 items
        one = np.zeros(1, dtype=bw.PLACE_DTYPE)
        for bad_off, k in (([1, 2], 2), ([0, 3, 2], 2), ([0, 256], 256)):
            with pytest.raises(bw.BwbError, match="error -1.*join_records"):
                ctx.join_records(np.repeat(one, len(bad_off) - 1), bad_off, np.zeros(k, dtype=bw.ALT_DTYPE), np.zeros(k, dtype=np.uint8))
        got = ctx.join()
        assert got[0].tobytes() == model.places.tobytes() and np.array_equal(got[1], model.off) and got[2].tobytes() == model.alts.tobytes()
        same_joins(got[4], model.joins)
        assert ctx.join_stats()[:2] == (len(model.alts), model.total)
        # set_loci forgets the chromosomes; a new batch invalidates the slot's records
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
            ctx.join()
        ctx.set_bubble_chrom(t.chrom)
        ctx.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            ctx.join()
        ctx.run()
        same_joins(ctx.join()[4], model.joins[:10])
    finally:
        ctx.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def map_dir(built, golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("mapjoin")
    for ext in ("", ".bwt", ".ann"):
        shutil.copy(os.path.join(golden, "toy.fa" + ext), d / ("toy.fa" + ext))
    return d


VARIANTS = {
    "one_chunk": ([], {}),
    "chunks_of_97": ([], {"BWB_CHUNK": "97"}),
    "two_workers": (["-g", "2"], {"BWB_DEVICE_MAP": "0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cli_map_with_join_writes_the_models_text(map_dir, golden, pad_text, model, variant):
    extra, env = VARIANTS[variant]
    out = map_dir / f"join_{variant}.sam"
    log = cli(["map", "-n", "3", "-X", "5", "-B", os.path.join(golden, "pad_toy.data"), "-J"] + extra + [map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out], env)
    assert open(out, "rb").read() == model.text
    assert f"placements joined by locus on the GPU: items {len(model.alts)}  joined {model.total}  reads with another MAPQ {int((model.joins['mapq'] != model.places['mapq']).sum())}" in log
    assert ("GPUs: 2" in log) == (variant == "two_workers")


def test_cli_align_then_aln2sam_with_join(map_dir, golden, pad_text, model, tmp_path):
    fa, fq, aln, out = map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "t.aln", tmp_path / "t.sam"
    cli(["align", "-n", "3", fa, fq, aln])
    cli(["aln2sam", "-X", "5", "-B", os.path.join(golden, "pad_toy.data"), "-J", fa, fq, aln, out])
    assert open(out, "rb").read() == model.text


def test_cli_map_with_join_and_another_mismatch_limit_equals_aln2sam(map_dir, golden, pad_text, model, tmp_path):
    """-Q 0 / -n 0 and -X 1: parity of the two paths away from the defaults (a joined read without a mismatch is at the limit: 25, not 37)"""
    fa, fq, data = map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    aln, one, two = tmp_path / "t.aln", tmp_path / "one.sam", tmp_path / "two.sam"
    cli(["map", "-n", "3", "-Q", "0", "-X", "1", "-B", data, "-J", fa, fq, one])
    cli(["align", "-n", "3", fa, fq, aln])
    cli(["aln2sam", "-n", "0", "-X", "1", "-B", data, "-J", fa, fq, aln, two])
    got = open(one, "rb").read()
    assert got == open(two, "rb").read() and got != model.text and got.count(b"\tbJ:i:1") == model.total


def test_cli_map_without_join_writes_todays_bytes(map_dir, golden, pad_text, model):
    out = map_dir / "nojoin.sam"
    log = cli(["map", "-n", "3", "-X", "5", "-B", os.path.join(golden, "pad_toy.data"), map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    assert open(out, "rb").read() == model.padded and "joined by locus" not in log
    cli(["map", "-n", "3", "-B", os.path.join(golden, "pad_toy.data"), map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    assert open(out, "rb").read() == open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read()


def test_cli_map_with_join_on_records_out_of_text_order(golden, pad_text, model, tmp_path):
    """an .ann whose records do not ascend: loci and joins are resolved on the host, the log says so, the lines are the same"""
    for ext in ("", ".bwt"):
        shutil.copy(os.path.join(golden, "toy.fa" + ext), tmp_path / ("toy.fa" + ext))
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    out = tmp_path / "out.sam"
    log = cli(["map", "-n", "3", "-X", "5", "-B", os.path.join(golden, "pad_toy.data"), "-J", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"@")]
    assert body(open(out, "rb").read()) == body(model.text)
    assert "on the host and joined there" in log and f"placements joined by locus on the host: joined {model.total}" in log


def test_cli_map_refuses_a_bubble_without_its_chromosome(golden, pad_text, tmp_path):
    for ext in ("", ".bwt"):
        shutil.copy(os.path.join(golden, "toy.fa" + ext), tmp_path / ("toy.fa" + ext))
    (tmp_path / "toy.fa.ann").write_text(open(os.path.join(golden, "toy.fa.ann")).read().replace("chr3 synthetic", "chrX synthetic"))
    out = tmp_path / "out.sam"
    r = subprocess.run([bw.HOST_BIN, "map", "-n", "3", "-X", "5", "-B", os.path.join(golden, "pad_toy.data"), "-J", str(tmp_path / "toy.fa"), os.path.join(pad_text, "pad_bub.fq"), str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "bubble 0" in r.stdout and "0 .ann records are named \"chr3\"" in r.stdout and not out.exists()
