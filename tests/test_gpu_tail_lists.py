"""kl_search's exact-tail interval lists on the reads of tests/tail_model.py (tests/test_tail_lists_host.py proves on the CPU which list lengths
they walk and end with): the search stores only the intervals it reads back - a list's first interval and its tail travel in registers,
slot 0 of a list is never written (bwb_lane.h: list_add<P, true>) - so every reader of a list is run here at every list length, from the root
(-n 0), from popped entries (-n 1, -n 2, gapped), through the seeding path (-P) and with the single-genome alphabet (-S); in one launch, and
with every wave parked after 3, 5 and 7 loop iterations, so that reads are parked and resumed at every position of a list, the first included.
.aln bytes and the visit / pop / push counters equal to the CPU oracle's."""
import os
import subprocess
import sys

import pytest

import bwbble_amd as bw
import tail_model as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tail(built, oracle, tmp_path_factory):
    fx = tm.TailFixture()
    fa = str(tmp_path_factory.mktemp("tail") / "tail.fa")
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    seqs, lens = bw.encode_reads([fx.reads[n] for n in fx.names])
    idx = oracle.load_index(fa + ".bwt")
    want = {}  # the oracle's answer per parameter set: computed once, shared by the four contexts

    def expected(flags):
        if flags not in want:
            data, ost, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(list(flags)))
            want[flags] = (data, ost.visits_single + ost.visits_alphabet, ost.heap_pops, ost.heap_pushes)
        return want[flags]

    return fa, seqs, lens, expected


@pytest.fixture(scope="module", params=[None, "3", "5", "7"], ids=lambda v: f"slice{v}" if v else "plain")
def ctx(request, tail):
    """a context per BWB_SLICE_ITERS (the library reads it when a context is created)"""
    old = os.environ.pop("BWB_SLICE_ITERS", None)
    if request.param:
        os.environ["BWB_SLICE_ITERS"] = request.param
    try:
        c = bw.Context(tail[0] + ".bwt")
    finally:
        os.environ.pop("BWB_SLICE_ITERS", None)
        if old is not None:
            os.environ["BWB_SLICE_ITERS"] = old
    yield c, request.param
    c.close()


@pytest.mark.parametrize("flags", tm.FLAG_SETS, ids="".join)
def test_tail_lists_match_oracle(tail, ctx, flags):
    _, seqs, lens, expected = tail
    c, sliced = ctx
    data, visits, pops, pushes = expected(flags)
    off, alns = c.align(bw.params(list(flags)), seqs, lens)
    assert bw.aln_bytes(off, alns) == data
    st = c.stats()
    assert st.visits_single + st.visits_alphabet == visits
    assert st.heap_pops == pops and st.heap_pushes == pushes
    if sliced:
        assert st.n_parked_reads > len(lens) and st.launches_search > 10  # every read was parked, many times over


def test_tail_lists_on_the_test_build(tail):
    """the same reads on the test library (`make testlib`: 64-bit positions stored with a bias beyond 2^32, so an interval's high words matter),
    in its own process because the library is bound at import; parked every 5 iterations"""
    bw.build(testlib=True)
    env = dict(os.environ, BWB_LIB=bw.TEST_LIB_PATH, BWB_FORCE_POS64="1", BWB_SLICE_ITERS="5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_lists_worker.py"), tail[0]], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and f"TAIL-LISTS-OK {len(tm.FLAG_SETS)} parameter sets" in r.stdout, r.stdout[-3000:]
