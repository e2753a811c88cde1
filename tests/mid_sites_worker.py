"""Worker of tests/test_gpu_mid_stream.py: runs in its own process so that bwbble_amd binds the library BWB_LIB names - the TEST build, which
stages 2^15 characters per chunk of set_text, so that the 3 302 441 characters of the mid-size genome arrive in 101 chunks.  The site index over
the uploaded text is compared with a numpy cumulative count at every position (mid_model.check_site_index).
usage: mid_sites_worker.py <fasta with its .ann and .ref> <chunks expected>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import mid_model  # noqa: E402

codes = bw.read_ref(sys.argv[1])
assert (len(codes) + (1 << 15) - 1) >> 15 == int(sys.argv[2]), len(codes)
ctx = bw.Context(os.path.join(ROOT, "tests", "golden", "toy.fa.bwt"))
n_sites = mid_model.check_site_index(ctx, codes)
ctx.close()
print(f"MID-SITES-OK {len(codes)} characters, {n_sites} sites, {os.path.basename(bw.LIB_PATH)}")
