"""Worker of tests/test_gpu_geno.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the TEST build stages 2^15
characters per chunk of set_text, so that the 40 001 characters here arrive in two.  Every site of the uploaded text must come back from
geno_sites with its position and code (the inverse of the site index), in pieces of 1 000 and in one piece, and k_site_of must map the returned
positions back to the site numbers.
usage: geno_sites_worker.py <chunks expected>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import geno_model  # noqa: E402
import pile_model  # noqa: E402

rng = np.random.default_rng(40001)
text = "".join(rng.choice(list("ACGT" * 6 + pile_model.NT16[1:]), 40000)) + "W"
shift = 15 if os.path.basename(bw.LIB_PATH) == "libbwbble_hip_test.so" else 25
assert (len(text) + (1 << shift) - 1) >> shift == int(sys.argv[1]), len(text)
where = pile_model.sites(text)
ctx = bw.Context(os.path.join(ROOT, "tests", "golden", "toy.fa.bwt"))
ctx.set_text(pile_model.codes(text))
n = ctx.pile_begin()
assert n == len(where) > 10000 and where[-1] == 40000
counts = rng.integers(0, 30, (n, 4)).astype(np.uint32)
counts[rng.random(n) < 0.2] = 0
ctx.pile_put(0, counts)
want = geno_model.site_records(text, counts, 20, 1)
ctx.geno_begin(n)
whole = ctx.geno_sites(0, n, 20, 1)
assert whole.tobytes() == want.tobytes(), np.flatnonzero(whole != want)[:5] if len(whole) == len(want) else (len(whole), len(want))
assert np.array_equal(ctx.pile_site_of(whole["pos"]), whole["site"].astype(np.int64))
ctx.geno_begin(1000)
pieces = [ctx.geno_sites(s, min(1000, n - s), 20, 1) for s in range(0, n, 1000)]
assert np.concatenate(pieces).tobytes() == want.tobytes()
ctx.close()
print(f"GENO-SITES-OK {len(text)} characters, {n} sites, {len(want)} called, {os.path.basename(bw.LIB_PATH)}")
