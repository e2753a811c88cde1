"""kl_search with max_best and no_indel_length away from their defaults, on the reads of tests/params_model.py (tests/test_params_host.py proves
on the CPU that each value decides records of these reads, and where).  The two fields are launch arguments that `bwbble align` has no flag for;
a caller of the C-ABI sets them.  Each has its sites in bwb_lane.h: the break of a popped hit and of an exact tail (`num_best > max_best`,
num_best grown by an interval's width or by the summed width of a tail's list), and `allow_indels`.  Every value of the sweeps, under every
kl_search instantiation (32- / 64-bit positions, 16- / 32-byte entries, both alphabets), in one launch and with every wave parked after 3, 5 and 7
loop iterations (num_best, the lowered max_diff and the best score cross park / resume), with the calculate_d table (K = 6), on the pool's
floor with a batch that overflows it (the re-run classes), on the test build,
streamed with a change of one field between uploads, and through k_place: .aln bytes and the visit / pop / push counters equal to the CPU
oracle's (which tests/test_oracle_golden_params.py pins to the real reference at such values)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bwbble_amd as bw
import map_model
import oracle_lib
import params_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DTAB_K = 6  # (the default, 12, is for indexes of billions of rows)
CONTEXTS = {  # name: (environment of the context, the full sweeps?, reads get parked?)
    "plain": ({}, True, False),
    "pos64": ({"BWB_FORCE_POS64": "1"}, True, False),
    "slice3": ({"BWB_SLICE_ITERS": "3"}, False, True),
    "slice7": ({"BWB_SLICE_ITERS": "7"}, False, True),
    "pos64slice": ({"BWB_FORCE_POS64": "1", "BWB_SLICE_ITERS": "5"}, False, True),
    "dtab": ({"BWB_DTAB": "1", "BWB_DTAB_K": str(DTAB_K)}, False, False),
}
KNOBS = ("BWB_FORCE_POS64", "BWB_SLICE_ITERS", "BWB_POOL_GB", "BWB_DTAB", "BWB_DTAB_K")


@pytest.fixture(scope="module")
def pf(built, oracle, tmp_path_factory):
    fx = pm.ParamsFixture()
    fa = str(tmp_path_factory.mktemp("params") / "params.fa")
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    seqs, lens = fx.batch()
    idx = oracle.load_index(fa + ".bwt", load_sa=True)
    want = {}  # the oracle's answer per parameter set: computed once, shared by every context

    def expected(flags, **fields):
        k = pm.key(flags, fields)
        if k not in want:
            data, ost, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(list(flags), **fields))
            want[k] = (data, ost.visits_single + ost.visits_alphabet, ost.heap_pops, ost.heap_pushes)
        return want[k]

    return fx, fa, seqs, lens, expected, idx


@contextlib.contextmanager
def context(bwt, env, sa=False):
    """a context whose knobs are in the environment for as long as it lives: the library reads some when the context is created (slices, 64-bit
    positions, BWB_DTAB) and others later - BWB_POOL_GB whenever it sizes the pool for an upload, BWB_DTAB_K when the first idle submit builds the
    table.  Whatever an enclosing context set is put back afterwards."""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    c = None
    try:
        b = bw.BwtFile(bwt, load_sa=sa)
        c = bw.Context(b)
        if sa:
            c.set_sa(b.SA)
        yield c
    finally:
        if c is not None:
            c.close()
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module", params=list(CONTEXTS))
def ctx(request, pf):
    env, full, parks = CONTEXTS[request.param]
    with context(pf[1] + ".bwt", env) as c:
        yield c, full, parks


def check(pf, c, flags, **fields):
    _, _, seqs, lens, expected, _ = pf
    data, visits, pops, pushes = expected(flags, **fields)
    off, alns = c.align(bw.params(list(flags), **fields), seqs, lens)
    assert bw.aln_bytes(off, alns) == data, (flags, fields)
    st = c.stats()
    assert st.visits_single + st.visits_alphabet == visits, (flags, fields)
    assert st.heap_pops == pops and st.heap_pushes == pushes, (flags, fields)
    if os.environ.get("BWB_DTAB") == "1":  # (the table's context: it was built, with the K asked for; "-n 0" included)
        assert c.dtab_info()["K"] == DTAB_K
    return st


def test_max_best_sweep(pf, ctx):
    """-n 2, every value from -1 to 34 and 2^31 - 1 (parked contexts: both sides of every family's threshold): every family's flip"""
    c, full, parks = ctx
    for mb in pm.MAX_BEST_SWEEP if full else pm.MAX_BEST_EDGES:
        st = check(pf, c, ("-n", "2"), max_best=mb)
        if parks:
            assert st.n_parked_reads > len(pf[3])
    assert pf[4](("-n", "2"), max_best=0)[0] != pf[4](("-n", "2"), max_best=1)[0]


@pytest.mark.parametrize("flags", pm.BEST_FLAG_SETS, ids="".join)
def test_max_best_under_other_parameters(pf, ctx, flags):
    """no difference allowed (one tail from the root: nothing to break), one (a substituted read's best hit arrives through an exact tail, the
    gapped variant after it where a gap open is cheap), -S, -P, and the 32-byte entries of -o 2 and of penalties above 63 in both alphabets"""
    c, full, parks = ctx
    for mb in pm.MAX_BEST_EDGES if full else pm.MAX_BEST_FEW:
        st = check(pf, c, flags, max_best=mb)
        if parks:
            assert st.n_parked_reads > 0
    if flags != ("-n", "0"):  # (a value that breaks, one that does not)
        assert pf[4](flags, max_best=0)[0] != pf[4](flags, max_best=pm.MAX_BEST_MAX)[0]


@pytest.mark.parametrize("flags", pm.INDEL_FLAG_SETS, ids="".join)
def test_no_indel_length_sweep(pf, ctx, flags):
    c, full, parks = ctx
    for v in pm.NO_INDEL_SWEEP if full else pm.NO_INDEL_FEW:
        st = check(pf, c, flags, no_indel_length=v)
        if parks:
            assert st.n_parked_reads > 0
    assert pf[4](flags, no_indel_length=0)[0] != pf[4](flags, no_indel_length=25)[0]


def test_both_fields_together(pf, ctx):
    c, _, parks = ctx
    for mb, v in ((2, 0), (3, 8), (33, 2), (-1, -3)):
        st = check(pf, c, ("-n", "2", "-o", "2", "-e", "2"), max_best=mb, no_indel_length=v)
        if parks:
            assert st.n_parked_reads > len(pf[3])


def test_the_table_context_uses_its_table(pf):
    """BWB_DTAB=1 with K = 6: the same visits of kl_calc_d as without a table, fewer buckets fetched"""
    loads = {}
    for on in ("1", "0"):
        with context(pf[1] + ".bwt", {"BWB_DTAB": on, "BWB_DTAB_K": str(DTAB_K)}) as c:
            st = check(pf, c, ("-n", "2"), max_best=3)
            assert c.dtab_info()["K"] == (DTAB_K if on == "1" else 0)
            loads[on] = (st.bucket_loads_calc_d, st.visits_calc_d)
    assert loads["1"][1] == loads["0"][1] and loads["1"][0] < loads["0"][0], loads


POOL_COPIES = 240  # 65 760 reads at once on the 256 MB floor of the chunk pool: tens of thousands of them run out of chunks and are re-run
POOL_CASES = ((("-n", "2"), dict(max_best=3)), (("-n", "2"), dict(max_best=2)), (("-n", "2", "-M", "70", "-O", "66", "-E", "64"), dict(max_best=33)),
              (("-n", "3", "-o", "1", "-e", "3"), dict(no_indel_length=0)), (("-n", "3", "-o", "1", "-e", "3"), dict(no_indel_length=6)))


@pytest.mark.parametrize("env", [{}, {"BWB_SLICE_ITERS": "40"}], ids=["plain", "slice40"])
def test_starved_pool_reruns(pf, env):
    """BWB_POOL_GB=0 (the pool's floor) and the batch 240 times over: reads that find the pool empty are abandoned and run again in the
    re-run classes, where num_best, the lowered max_diff and the best score start afresh.  The batch by itself is checked against the oracle
    on this context; the large batch must give the same records and counters, copy after copy (a read's record depends on no other read:
    all are longer than the seed), and must have overflowed."""
    _, fa, seqs, lens, expected, _ = pf
    big_seqs, big_lens = np.tile(seqs, (POOL_COPIES, 1)), np.tile(lens, POOL_COPIES)
    with context(fa + ".bwt", dict(env, BWB_POOL_GB="0")) as c:
        for flags, fields in POOL_CASES:
            data, visits, pops, pushes = expected(flags, **fields)
            off1, alns1 = c.align(bw.params(list(flags), **fields), seqs, lens)
            st1 = c.stats()
            assert bw.aln_bytes(off1, alns1) == data, (flags, fields)
            assert (st1.visits_single + st1.visits_alphabet, st1.heap_pops, st1.heap_pushes) == (visits, pops, pushes), (flags, fields)
            off, alns = c.align(bw.params(list(flags), **fields), big_seqs, big_lens)
            st = c.stats()
            assert st.n_overflow_reads > 0, (flags, fields)
            assert np.array_equal(np.diff(off), np.tile(np.diff(off1), POOL_COPIES)), (flags, fields)
            assert alns.tobytes() == alns1.tobytes() * POOL_COPIES, (flags, fields)
            assert st.heap_pops == POOL_COPIES * st1.heap_pops and st.heap_pushes == POOL_COPIES * st1.heap_pushes, (flags, fields)
            assert st.visits_single + st.visits_alphabet == POOL_COPIES * (st1.visits_single + st1.visits_alphabet), (flags, fields)
            if env:
                assert st.n_parked_reads > 0


def test_params_on_the_test_build(pf):
    """the same reads on the test library (`make testlib`: 64-bit positions stored with a bias beyond 2^32), in its own process because the
    library is bound at import; parked every 5 iterations"""
    bw.build(testlib=True)
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(BWB_LIB=bw.TEST_LIB_PATH, BWB_FORCE_POS64="1", BWB_SLICE_ITERS="5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "params_worker.py"), pf[1]], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "PARAMS-OK" in r.stdout, r.stdout[-3000:]


STREAM = ((dict(max_best=0), dict(max_best=3), dict(max_best=8), dict(max_best=33)),
          (dict(no_indel_length=0), dict(no_indel_length=3), dict(no_indel_length=6), dict(no_indel_length=9)))


@pytest.mark.parametrize("fields", STREAM, ids=["max_best", "no_indel_length"])
def test_streamed_uploads_that_differ_in_one_field(pf, fields):
    """consecutive slot_uploads whose parameters differ in one field only, every wave parked after 7 iterations so that reads of the batch before
    are parked when the next upload arrives: the parameters are launch arguments, the upload must flush, and each batch equals its own oracle
    result"""
    _, fa, seqs, lens, expected, _ = pf
    flags = ("-n", "2", "-o", "2", "-e", "2")
    with context(fa + ".bwt", {"BWB_SLICE_ITERS": "7"}) as c:
        for rnd in range(2):  # (the second round reuses the slots)
            for slot, f in enumerate(fields):
                c.slot_upload(slot, bw.params(list(flags), **f), seqs, lens)
                c.slot_submit(slot)
            for slot, f in enumerate(fields):
                off, alns = c.slot_result(slot)
                assert bw.aln_bytes(off, alns) == expected(flags, **f)[0], (rnd, f)
        c.flush()
        assert c.stats().n_parked_reads > 0
        assert len({expected(flags, **f)[0] for f in fields}) == len(fields)


def test_place_with_gap_runs_next_to_a_path_end(pf, oracle):
    """no_indel_length = 0: hits whose gap run lies closer to an end of the path than any CLI run can produce, through k_place (eval_aln + mapq on
    the GPU) against tests/map_model.py applied to the oracle's hits"""
    fx, fa, _, _, _, idx = pf
    seqs, lens = fx.batch(list(fx.indel1) + list(fx.indel2))
    with context(fa + ".bwt", {}, sa=True) as c:
        for flags in (("-n", "1"), ("-n", "2", "-o", "2", "-e", "2")):
            data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(list(flags), no_indel_length=0))
            hits = oracle_lib.parse_aln(data)
            ends = [pm.gap_ends(h) for r in hits for h in r if h["gapo"]]
            assert sum(e[0] < 5 for e in ends) >= 5 and sum(e[1] < 5 for e in ends) >= 5
            off, alns = c.align(bw.params(list(flags), no_indel_length=0), seqs, lens)
            assert bw.aln_bytes(off, alns) == data
            for max_mm in (6, 3):
                want, steps = map_model.expected_places(oracle, idx, hits, max_mm)
                got = c.place(max_mm)
                assert map_model.first_difference(got, want) is None, (flags, max_mm, map_model.first_difference(got, want))
                assert got.tobytes() == want.tobytes()
                assert c.place_stats()[:2] == (len(lens), steps)
            assert (want["num_gapo"] > 0).sum() >= 20
