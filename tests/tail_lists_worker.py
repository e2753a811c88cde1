"""Worker of tests/test_gpu_tail_lists.py: runs in its own process so that bwbble_amd binds the TEST build of the library
(BWB_LIB=bwbble_amd/libbwbble_hip_test.so: biased 64-bit stored positions) instead of the product's.
usage: tail_lists_worker.py <tail.fa (indexed)>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import oracle_lib  # noqa: E402
import tail_model as tm  # noqa: E402

fa = sys.argv[1]
assert os.path.samefile(bw.LIB_PATH, bw.TEST_LIB_PATH), "the worker must run on the test build"
fx = tm.TailFixture()
assert open(fa).read() == fx.fasta()
orc = oracle_lib.load()
idx = orc.load_index(fa + ".bwt")
ctx = bw.Context(fa + ".bwt")
seqs, lens = bw.encode_reads([fx.reads[n] for n in fx.names])
n_checked = 0
for flags in tm.FLAG_SETS:
    off, alns = ctx.align(bw.params(list(flags)), seqs, lens)
    want, ost, _ = orc.align_encoded(idx, seqs, lens, orc.params(list(flags)))
    assert bw.aln_bytes(off, alns) == want, flags
    st = ctx.stats()
    assert st.visits_single + st.visits_alphabet == ost.visits_single + ost.visits_alphabet, flags
    assert st.heap_pops == ost.heap_pops and st.heap_pushes == ost.heap_pushes, flags
    assert st.n_parked_reads > len(lens), flags
    n_checked += 1
ctx.close()
print(f"TAIL-LISTS-OK {n_checked} parameter sets")
