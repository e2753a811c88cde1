"""Worker of tests/test_gpu_index_shapes.py: runs in its own process so that bwbble_amd binds the TEST build of the library
(BWB_LIB=bwbble_amd/libbwbble_hip_test.so: 2^13-block superblocks = 2^20 characters, 2^10-block upload chunks).
Two crafted code strings of a little over 2^21 characters - three superblocks, seventeen upload chunks:
  A  16 * 1024 + 1 blocks (a last chunk of ONE block, its word count clipped by num_words), the sentinel exactly on a superblock start
     (row 2^20: the first row of a chunk as well), code 13 first in the third superblock;
  B  exactly 17 * 1024 blocks of 128 characters, the sentinel one row before the superblock start, a '$' (code 0, counted) on the superblock
     start itself, code 5 first in the third superblock.
rank16 and wave_children around every superblock start and at random positions, against tests/idx_model.py.
usage: idx_shapes_worker.py <workdir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwbble_amd as bw  # noqa: E402
import idx_model as im  # noqa: E402
import oracle_lib  # noqa: E402

work = sys.argv[1]
assert os.path.samefile(bw.LIB_PATH, bw.TEST_LIB_PATH), "the worker must run on the test build"
orc = oracle_lib.load()
SB = 1 << 20  # characters per superblock of the test build
n_idx = n_pos = n_pairs = 0
for tag, nblk, tail, sa0, first3 in (("A", 16 * 1024 + 1, 91, SB, 13), ("B", 17 * 1024, 128, SB - 1, 5)):
    n = (nblk - 1) * 128 + tail
    codes = im.rand_below(31 + n_idx, n, 16).astype(np.uint8)
    codes[SB] = 0          # A: the sentinel; B: a '$' that the superblock's base row must count
    codes[2 * SB] = first3
    codes[sa0] = 0
    m = im.from_codes(codes, sa0).attach(orc, os.path.join(work, f"big{tag}.bwt"))
    assert m.num_occ == nblk and (nblk + 8191) // 8192 == 3 and (tag != "A" or m.num_words < nblk * 16)
    ctx = bw.Context(m)
    rng = im.Rng(41 + n_idx)
    pos = [2**64 - 1, n - 1, 0, n - 2, sa0 - 1, sa0, sa0 + 1]
    for b in (SB, 2 * SB):
        pos += [p for p in (b - 129, b - 128, b - 65, b - 64, b - 1, b, b + 1, b + 63, b + 64, b + 127, b + 128) if p < n]
    for ch in (1, 2, 8, 9, 16):  # the first and last rows of upload chunks (2^10 blocks)
        pos += [p for p in (ch * 1024 * 128 - 1, ch * 1024 * 128) if p < n]
    pos = np.array(pos + [int(v) for v in rng.below(n, 4000)], dtype=np.uint64)
    exact, alpha = im.rank_exact(m, pos), im.rank_alpha(m, pos)
    for inc in (0, 1):
        assert np.array_equal(ctx.rank16(pos, inc=inc, exact=True)[:, 1:], exact[:, 1:] + np.uint64(inc)), (tag, inc, "exact")
        assert np.array_equal(ctx.rank16(pos, inc=inc)[:, 1:], alpha[:, 1:] + np.uint64(inc)), (tag, inc, "alpha")
    n_pos += len(pos)
    # waves whose pairs straddle the superblock starts (rows_differ) among ordinary lanes; the named waves of the small test as well
    waves = im.named_waves(n, seed=13)
    for w in waves:
        w.alpha = rng.below(2, 64) == 1
    edge = []
    for b in (SB, 2 * SB):  # the sides right at the boundary, lane by lane: (b - 1 - k, b + k), and sides ON the first row of the superblock
        k = np.arange(64)
        edge.append(im.Wave(f"straddle_{b}", b - 1 - k, b + k, alpha=k % 2 == 1))
        far = min(b + 300, n - 2 - 128)  # (A's third superblock is 91 characters: its ordinary lanes lie before the boundary)
        edge.append(im.Wave(f"straddle_every_4th_{b}", np.where(k % 4 == 0, b - 1 - k, far - 100 + k), np.where(k % 4 == 0, b + k // 2, far + 2 * k), alpha=k % 3 == 0))
        edge.append(im.Wave(f"on_the_start_{b}", np.where(k % 2 == 0, b - 1, b), b + k, alpha=k % 4 < 2))
    rnd = [im.random_wave(n, rng, f"random_{k}", hot=(SB, 2 * SB)) for k in range(200)]
    n_pairs += im.check_children(ctx, m, waves + edge + rnd, bits=64 if os.environ.get("BWB_FORCE_POS64") else 32)
    ctx.close()
    orc.lib.bwb_or_free_index(m.oracle_index)
    os.unlink(m.path)
    n_idx += 1
print(f"IDX-SHAPES-OK {n_idx} indexes, {n_pos} rank positions, {n_pairs} pairs")
