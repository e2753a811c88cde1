"""Worker of tests/test_gpu_map.py: runs in its own process so that bwbble_amd binds the TEST build of the library
(BWB_LIB=bwbble_amd/libbwbble_hip_test.so: 2^13-block superblocks, biased stored positions).  Placement records of a few thousand
reads on a 6 M-row index against eval_aln of the oracle's hits.
usage: map_c3_worker.py <genome.fa (indexed)> <workdir>"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import map_model  # noqa: E402
import oracle_lib  # noqa: E402

fa, work = sys.argv[1], sys.argv[2]
assert os.path.samefile(bw.LIB_PATH, bw.TEST_LIB_PATH), "the worker must run on the test build"
orc = oracle_lib.load()
idx = orc.load_index(fa + ".bwt", load_sa=True)
b = bw.BwtFile(fa + ".bwt", load_sa=True)
assert (b.length + 127) // 128 > 5 * 8192, "the index must span several 2^13-block superblocks"
ctx = bw.Context(b)
ctx.set_sa(b.SA)
fq = os.path.join(work, "mapc3.fq")
subprocess.run([bw.SYNTH_BIN, "reads", fa, fq, "3000", "100", "21", "1.5", "2.0", "1.0"], check=True)
seqs, lens = bw.load_fastq_codes(fq)
n_mapped = 0
for flags in (["-n", "3"], ["-n", "3", "-o", "2"]):
    ctx.align(bw.params(flags), seqs, lens)
    data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(flags))
    want, steps = map_model.expected_places(orc, idx, oracle_lib.parse_aln(data), 6)
    got = ctx.place(6)
    assert map_model.first_difference(got, want) is None, (flags, map_model.first_difference(got, want))
    assert got.tobytes() == want.tobytes()
    assert ctx.place_stats()[:2] == (len(lens), steps), (ctx.place_stats(), steps)
    n_mapped += int((want["flags"] & 1).sum())
ctx.close()
assert n_mapped > 4000
print(f"MAP-C3-OK {n_mapped} mapped reads")
