"""Worker of tests/test_gpu_alt.py: runs in its own process so that bwbble_amd binds the TEST build of the library
(BWB_LIB=bwbble_amd/libbwbble_hip_test.so: 2^13-block superblocks, biased stored positions).  The other placements of a few thousand
reads on a 6 M-row multi-genome index (a read next to an indel site lies in the chromosome and in the bubble) against the model fed the
oracle's hits and the oracle's walk; and of made-up hit lists with rows all over the index, through place_hits_alt.
usage: alt_c3_worker.py <genome.fa (indexed)> <workdir>"""
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import alt_model  # noqa: E402
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
sa = alt_model.OracleSA(orc, idx)
fq = os.path.join(work, "altc3.fq")
subprocess.run([bw.SYNTH_BIN, "reads", fa, fq, "3000", "100", "23", "1.5", "2.0", "1.0"], check=True)
seqs, lens = bw.load_fastq_codes(fq)
flags = ["-n", "3"]
ctx.align(bw.params(flags), seqs, lens)
data, _, _ = orc.align_encoded(idx, seqs, lens, orc.params(flags))
reads = oracle_lib.parse_aln(data)
n_items = 0
for max_alt in (1, 5):
    off, alts, steps = alt_model.expected_alts(reads, max_alt, sa)
    places, goff, galts = ctx.place_alt(6, max_alt)
    assert places.tobytes() == ctx.place(6).tobytes()
    assert np.array_equal(goff, off) and alt_model.first_difference(galts, alts) is None, (max_alt, alt_model.first_difference(galts, alts))
    assert galts.tobytes() == alts.tobytes()
    assert ctx.place_alt_stats()[:2] == (len(alts), steps), (ctx.place_alt_stats(), len(alts), steps)
    n_items = len(alts)
assert n_items >= 20, n_items  # reads at the bubbles
# made-up hit lists: rows all over the index (every superblock), 1-4 hits of 1-3 rows, gapped paths
from golden.make_golden_map import hit, random_path  # noqa: E402
rng = random.Random(35)
length = int(idx.contents.length)
hits = []
for _ in range(1500):
    ents = []
    for _ in range(rng.choice([0, 1, 2, 2, 3, 4])):
        w = rng.choice([1, 1, 2, 3])
        ents.append(hit(random_path(rng, 100), rng.randrange(1, length - w), width=w, score=rng.choice([3, 6]), mm=rng.randrange(0, 4)))
    hits.append(ents)
hits.append([hit([(0, 100)], int(idx.contents.sa0_index) - 1, width=3), hit([(0, 100)], length - 2, width=2, score=6)])
off, alts, steps = alt_model.expected_alts(hits, 5, sa)
hoff, halns = map_model.aln_records(hits, random.Random(36))
_, goff, galts = ctx.place_hits_alt(hoff, halns, 6, 5)
assert np.array_equal(goff, off) and alt_model.first_difference(galts, alts) is None, alt_model.first_difference(galts, alts)
assert galts.tobytes() == alts.tobytes() and ctx.place_alt_stats()[:2] == (len(alts), steps)
assert len(alts) > 1000 and len({int(p) >> 20 for p in alts["pos"]}) >= 3
ctx.close()
print(f"ALT-C3-OK {n_items} items of {len(lens)} reads, {len(alts)} items of {len(hits)} made-up hit lists")
