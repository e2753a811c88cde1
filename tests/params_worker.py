"""Worker of tests/test_gpu_params.py: runs in its own process so that bwbble_amd binds the TEST build of the library
(BWB_LIB=bwbble_amd/libbwbble_hip_test.so: biased 64-bit stored positions) instead of the product's.
usage: params_worker.py <params.fa (indexed)>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import oracle_lib  # noqa: E402
import params_model as pm  # noqa: E402

fa = sys.argv[1]
assert os.path.samefile(bw.LIB_PATH, bw.TEST_LIB_PATH), "the worker must run on the test build"
fx = pm.ParamsFixture()
assert open(fa).read() == fx.fasta()
orc = oracle_lib.load()
idx = orc.load_index(fa + ".bwt")
ctx = bw.Context(fa + ".bwt")
seqs, lens = fx.batch()
cases = [(("-n", "2"), dict(max_best=mb)) for mb in pm.MAX_BEST_EDGES]
cases += [(f, dict(max_best=mb)) for f in (("-n", "1", "-O", "4"), ("-n", "2", "-o", "2"), ("-S", "-n", "2"), ("-S", "-n", "2", "-o", "2")) for mb in (2, 3)]
cases += [(f, dict(no_indel_length=v)) for f in (("-n", "1"), ("-n", "2", "-o", "2", "-e", "2"), ("-S", "-n", "2")) for v in (0, 2, 6)]
for flags, fields in cases:
    off, alns = ctx.align(bw.params(list(flags), **fields), seqs, lens)
    want, ost, _ = orc.align_encoded(idx, seqs, lens, orc.params(list(flags), **fields))
    assert bw.aln_bytes(off, alns) == want, (flags, fields)
    st = ctx.stats()
    assert st.visits_single + st.visits_alphabet == ost.visits_single + ost.visits_alphabet, (flags, fields)
    assert st.heap_pops == ost.heap_pops and st.heap_pushes == ost.heap_pushes, (flags, fields)
    assert st.n_parked_reads > 0, (flags, fields)
ctx.close()
print(f"PARAMS-OK {len(cases)} parameter sets")
