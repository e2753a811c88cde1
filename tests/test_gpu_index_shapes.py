"""Rank, locate and interval children at the edges of the index's and the wave's shape - against tests/idx_model.py (anchored to the
indexer and the oracle on the CPU by tests/test_idx_host.py).  Everything is bit-exact integer comparison.

* rank family: CRAFTED code strings of every length residue around the 64-character bucket and the 128-character block, with the sentinel row
  on block starts, bucket starts, in the last block, on the last row - shapes the indexer never makes (it writes odd lengths and puts the
  sentinel where the sort puts suffix 0).  k_rank16 at every position, and wave_children (bwb_hip_children) with every position on either side;
* real BWTs of the same residues and sentinel placements (idx_model.REAL_SHAPES): locate of all rows, calculate_d, the search's bytes and
  work counters, placement records;
* wave_children by itself on waves built for its rare paths: further gather rounds, the rows_differ recomputation, idle lanes;
* the test build (2^13-block superblocks, 2^10-block upload chunks) in a child process: tests/idx_shapes_worker.py.
Each family runs with 32-bit and with 64-bit positions (BWB_FORCE_POS64 is read when a context is created)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bwbble_amd as bw
import idx_model as im
import map_model as mm
import oracle_lib
from ovf_model import IUPAC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS = [pytest.param(False, id="pos32"), pytest.param(True, id="pos64")]


def set_pos(monkeypatch, pos64):
    if pos64:
        monkeypatch.setenv("BWB_FORCE_POS64", "1")
    else:
        monkeypatch.delenv("BWB_FORCE_POS64", raising=False)
    monkeypatch.setenv("BWB_POOL_GB", "1")  # (several contexts per process: include/bwbble_hip.h)


# ---- rank on crafted code strings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos64", POS)
@pytest.mark.parametrize("content", im.CONTENTS)
def test_rank_at_every_position_of_crafted_strings(content, pos64, oracle, monkeypatch, tmp_path):
    set_pos(monkeypatch, pos64)
    n_idx = 0
    for n, sa0, c in im.rank_family():
        if c != content:
            continue
        m = im.from_codes(im.crafted(n, sa0, c), sa0).attach(oracle, str(tmp_path / "c.bwt"))
        ctx = bw.Context(m)
        pos = np.concatenate([[im.NEG], np.arange(n, dtype=np.uint64)])
        exact, alpha = im.rank_exact(m, pos), im.rank_alpha(m, pos)
        for inc in (0, 1):
            assert np.array_equal(ctx.rank16(pos, inc=inc, exact=True)[:, 1:], exact[:, 1:] + np.uint64(inc)), (n, sa0, c, inc, "exact")
            assert np.array_equal(ctx.rank16(pos, inc=inc)[:, 1:], alpha[:, 1:] + np.uint64(inc)), (n, sa0, c, inc, "alpha")
        # the lane rank (wave_children): every position as side L of (p + 1, length - 1) and as side U of (0, p) - a U bucket of the lane's
        # own -, and both sides on p; exact and O_alphabet lanes alternate
        p = pos.astype(np.int64)  # (-1 first)
        last = np.full(len(p), n - 1)
        w = im.Wave(f"n={n} sa0={sa0} {c}", np.concatenate([p, np.full(len(p), -1), p]), np.concatenate([last, np.maximum(p, 0), np.maximum(p, 0)]))
        w.alpha = np.arange(len(w.iL)) % 2 == 1
        im.check_children(ctx, m, [w], bits=64 if pos64 else 32, allow_undefined=n <= 3)
        w.alpha = ~w.alpha
        im.check_children(ctx, m, [w], bits=64 if pos64 else 32, allow_undefined=n <= 3)
        ctx.close()
        oracle.lib.bwb_or_free_index(m.oracle_index)
        n_idx += 1
    assert n_idx >= 2 * len(im.RANK_LENGTHS) - 1


# ---- real BWTs ----------------------------------------------------------------------------------------------------------------
_BASE = {"A": 0, "G": 1, "C": 2, "T": 3}


def shape_reads(seq, seed):
    """a few dozen reads (A0 G1 C2 T3 N4): substrings of the record of 12, 13, 32, 33, 50 and 70 bases - an IUPAC character gives one of its bases -
    half of them with one or two substitutions, one with an N; random reads where the record is shorter; and a read of 255 bases, longer than
    the text of the two small shapes"""
    rng = im.Rng(seed)
    reads = []
    for rl in (12, 13, 32, 33, 50, 70):
        for k in range(5):
            if rl <= len(seq):
                s0 = rng.below(len(seq) - rl + 1)
                r = [_BASE[IUPAC[ch][rng.below(len(IUPAC[ch]))]] if ch in IUPAC else 4 for ch in seq[s0:s0 + rl]]
            else:
                r = [int(v) for v in rng.below(4, rl)]
            for _ in range(k % 3):  # 0, 1, 2 substitutions
                q = rng.below(rl)
                r[q] = (r[q] + 1 + rng.below(3)) % 4 if r[q] < 4 else 0
            if k == 4 and rl == 50:
                r[rng.below(rl)] = 4
            reads.append(r if k % 2 == 0 else [3 - b if b < 4 else 4 for b in r[::-1]])  # (every second one from the other strand)
    reads.append([int(v) for v in rng.below(4, 255)])
    lens = np.array([len(r) for r in reads], dtype=np.uint16)
    seqs = np.full((len(reads), 255), 4, dtype=np.uint8)
    for i, r in enumerate(reads):
        seqs[i, :len(r)] = r
    return seqs, lens


SEARCH_FLAGS = (["-n", "0"], ["-n", "2"], ["-n", "3", "-o", "1"], ["-S", "-n", "2"], ["-P", "-n", "2"])


def check_search(ctx, oracle, idx, flags, seqs, lens):
    off, alns = ctx.align(bw.params(flags), seqs, lens)
    want, ost, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    assert bw.aln_bytes(off, alns) == want, flags
    st = ctx.stats()
    assert st.visits_single + st.visits_alphabet == ost.visits_single + ost.visits_alphabet, flags
    assert st.heap_pops == ost.heap_pops and st.heap_pushes == ost.heap_pushes, flags
    return want


@pytest.mark.parametrize("pos64", POS)
@pytest.mark.parametrize("shape", im.REAL_SHAPES, ids=[s[0] for s in im.REAL_SHAPES])
def test_locate_calc_d_and_search_on_real_bwts(shape, pos64, built, oracle, monkeypatch, tmp_path):
    name, bases, seed, trim, claims = shape
    set_pos(monkeypatch, pos64)
    records = im.real_records(bases, seed)
    seq = records[-1]
    m = im.from_text(im.real_text(bases, seed, trim))
    assert m.length == claims["length"] and m.sa0 == claims["sa0"]
    path = str(tmp_path / "s.fa.bwt")
    if trim:  # an even length: the indexer makes none
        m.write(path)
    else:
        with open(path[:-4], "w") as f:
            f.write("".join(f">s{i}\n{r}\n" for i, r in enumerate(records)))
        subprocess.run([bw.HOST_BIN, "index", path[:-4]], check=True, stdout=subprocess.DEVNULL)
    b = bw.BwtFile(path, load_sa=True)
    assert b.length == m.length and b.sa0_index == m.sa0
    idx = oracle.load_index(path, load_sa=True)
    ctx = bw.Context(b)
    ctx.set_sa(b.SA)
    # locate: every row, against the sort
    rows = np.arange(m.length, dtype=np.uint64)
    assert np.array_equal(ctx.locate(rows), m.sa)
    assert ctx.locate_stats()[:2] == (m.length, int(im.walk_steps(m).sum()))
    # calculate_d
    seqs, lens = shape_reads(seq, seed)
    for flags in ([], ["-S"]):
        D, Ds = ctx.calc_d(bw.params(flags), seqs, lens)
        p = oracle.params(flags)
        for r in range(len(lens)):
            ln = int(lens[r])
            assert np.array_equal(D[r, :ln + 1], oracle.calculate_d(idx, seqs[r, :ln], p)), (flags, r)
            if ln > p.seed_length:
                assert np.array_equal(Ds[r], oracle.calculate_d(idx, seqs[r, :p.seed_length], p)), (flags, r)
    # the search: bytes and work counters
    n_hits = 0
    for flags in SEARCH_FLAGS:
        want = check_search(ctx, oracle, idx, flags, seqs, lens)
        if flags == ["-n", "2"] and not trim:  # placement records: map_model speaks of the indexer's texts (forward half, reverse half)
            hits = oracle_lib.parse_aln(want)
            wantp, steps = mm.expected_places(oracle, idx, hits)
            got = ctx.place()
            assert mm.first_difference(got, wantp) is None, mm.first_difference(got, wantp)
            assert ctx.place_stats()[:2] == (len(lens), steps)
        n_hits += len(want) > 4 * len(lens)
    assert n_hits == len(SEARCH_FLAGS)  # (reads do hit)
    ctx.close()
    monkeypatch.setenv("BWB_DTAB", "1")
    monkeypatch.setenv("BWB_DTAB_K", "7")
    ctx = bw.Context(b)
    check_search(ctx, oracle, idx, ["-n", "2"], seqs, lens)
    assert ctx.dtab_info()["K"] == 7
    ctx.close()
    oracle.lib.bwb_or_free_index(idx)


# ---- wave_children by itself --------------------------------------------------------------------------------------------------
def wave_index(kind, oracle, tmp_path):
    if kind == "crafted":  # about 40 blocks, the sentinel on a block start, quirk codes on some block starts
        n, sa0 = 40 * 128 + 37, 17 * 128
        codes = im.crafted(n, sa0, "uniform", seed=7)
        codes[128:n:256] = [5, 9, 11, 13] * 5
        codes[sa0] = 0
        m = im.from_codes(codes, sa0)
    else:
        _, bases, seed, trim, _ = next(s for s in im.REAL_SHAPES if s[0] == "res65_blk")
        m = im.from_text(im.real_text(bases, seed, trim))
    return m.attach(oracle, str(tmp_path / "w.bwt"))


@pytest.mark.parametrize("pos64", POS)
@pytest.mark.parametrize("kind", ["crafted", "real"])
def test_wave_children_on_constructed_waves(kind, pos64, oracle, monkeypatch, tmp_path):
    """Pair q is lane q % 64 of wave q / 64 (include/bwbble_hip.h), so 64 consecutive pairs are one wave."""
    set_pos(monkeypatch, pos64)
    m = wave_index(kind, oracle, tmp_path)
    n = m.length
    ctx = bw.Context(m)
    waves = im.named_waves(n, seed=11)
    own = {w.name: w.own_u_rows(n) for w in waves}  # the waves are what they are called: U buckets of their own -> gather rounds of 24
    assert own["one_bucket"] == 0 and own["all_split"] == 64 and [own[f"own_{k}"] for k in (24, 25, 48, 49)] == [24, 25, 48, 49]
    assert own["every_second_idle"] == 32 and own["only_lane_63"] == 1 and own["block_halves"] == 64 and own["bucket_edge"] == 64
    mixed = im.Rng(5).below(2, 64) == 1
    bits = 64 if pos64 else 32
    total = 0
    for alpha in (False, True, mixed):  # exact, O_alphabet, and both kinds of lane in one wave
        for w in waves:
            w.alpha = np.broadcast_to(np.asarray(alpha), (64,)).copy()
        total += im.check_children(ctx, m, waves, bits=bits)
    # n pairs that do not fill their last wave
    rng = im.Rng(23)
    rnd = [im.random_wave(n, rng, f"random_{k}") for k in range(200)]
    for tail in (1, 63, 65, 257):
        total += im.check_children(ctx, m, rnd[:5], tail=tail, bits=bits)
    total += im.check_children(ctx, m, rnd, bits=bits)  # 200 random waves: every kind of lane mixed
    assert total == 3 * 64 * len(waves) + 1 + 63 + 65 + 257 + 200 * 64
    with pytest.raises(bw.BwbError):
        ctx.children([n + 1], [0])
    with pytest.raises(bw.BwbError):
        ctx.children([0], [n])
    ctx.close()


# ---- the test build: superblock rows and a chunked upload ---------------------------------------------------------------------
@pytest.mark.parametrize("pos64", POS)
def test_superblock_starts_and_chunked_upload_in_the_test_build(pos64, built, oracle, tmp_path):
    bw.build(testlib=True)
    env = dict(os.environ, BWB_LIB=bw.TEST_LIB_PATH, BWB_POOL_GB="1")
    env.pop("BWB_FORCE_POS64", None)
    if pos64:
        env["BWB_FORCE_POS64"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "idx_shapes_worker.py"), str(tmp_path)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "IDX-SHAPES-OK 2 indexes" in r.stdout, r.stdout[-3000:]
