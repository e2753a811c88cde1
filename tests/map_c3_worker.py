"""Worker of tests/test_gpu_map.py: runs in its own process so that bwbble_amd binds the TEST build of the library
(BWB_LIB=bwbble_amd/libbwbble_hip_test.so: 2^13-block superblocks, biased stored positions).  Placement records of a few thousand
reads on a 6 M-row index against eval_aln of the oracle's hits; and of 200 000 made-up hit lists (the generator of the synth_hits fixture
run on this index, tests/golden/make_golden_map.py) through place_hits against eval_aln of the same lists with the oracle's walk.
usage: map_c3_worker.py <genome.fa (indexed)> <workdir>"""
import os
import random
import subprocess
import sys

import numpy as np

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
# injected hit lists: eight gap runs, wrapping sums, special first rows - and the grid-stride loop - across superblock rows
from golden.make_golden_map import make_synth, read_ann  # noqa: E402
_, hits, _ = make_synth(random.Random(33), orc, idx, read_ann(fa + ".ann"), through_sentinel=False)
want, steps = map_model.expected_places(orc, idx, hits, 6)
off, alns = map_model.aln_records(hits, random.Random(34))
times = 200_000 // len(hits) + 1
toff = np.zeros(len(hits) * times + 1, dtype=np.uint64)
toff[1:] = np.cumsum(np.tile(np.diff(off), times))
got = ctx.place_hits(toff, np.tile(alns, times), 6)
assert map_model.first_difference(got[:len(hits)], want) is None, map_model.first_difference(got[:len(hits)], want)
assert got.tobytes() == np.tile(want, times).tobytes()
assert ctx.place_stats()[:2] == (len(hits) * times, steps * times), (ctx.place_stats(), steps * times)
n_synth = int((want["flags"] & 1).sum())
assert n_synth > 300 and {int(idx.contents.sa0_index), int(idx.contents.length) - 1} <= {e[0]["L"] for e in hits if e}
ctx.close()
assert n_mapped > 4000
print(f"MAP-C3-OK {n_mapped} mapped reads, {n_synth} of {len(hits)} synthetic hit lists placed {times} times")
