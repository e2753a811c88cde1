"""CPU-only: the index model of tests/idx_model.py against the product's indexer and the oracle, and the claims of its shape tables.

* from_text on the indexer's text gives the bytes `bwbble index` writes (and, for rep.fa, the committed golden file): the model is anchored
  to the product's indexer, and through the golden files to the reference;
* occ equals the oracle's O() at every position, and the oracle's SA walk finds the sort's suffix array through the model's files;
* the oracle's O_alphabet on from_codes files equals a direct restatement on every crafted shape of the rank family;
* the shape tables hold the residues and sentinel placements they claim."""
import os
import subprocess

import numpy as np
import pytest

import bwbble_amd as bw
import idx_model as im

ODD_SHAPES = [s for s in im.REAL_SHAPES if s[3] == 0]


def fasta_records(path):
    recs, cur = [], None
    for ln in open(path):
        if ln.startswith(">"):
            cur = []
            recs.append(cur)
        else:
            cur.append(ln.strip())
    return ["".join(r) for r in recs]


@pytest.fixture(scope="module")
def rep_model(golden):
    return im.from_text(im.fasta_text(fasta_records(os.path.join(golden, "rep.fa"))))


def test_from_text_gives_the_golden_rep_index(rep_model, golden):
    assert rep_model.tobytes() == open(os.path.join(golden, "rep.fa.bwt"), "rb").read()


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=[s[0] for s in ODD_SHAPES])
def test_from_text_gives_the_indexers_bytes(shape, built, tmp_path):
    name, bases, seed, trim, _ = shape
    fa = str(tmp_path / "s.fa")
    with open(fa, "w") as f:
        for k, seq in enumerate(im.real_records(bases, seed)):
            f.write(f">s{k}\n" + "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + "\n")
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    assert im.from_text(im.real_text(bases, seed, trim)).tobytes() == open(fa + ".bwt", "rb").read()


def _occ_vs_oracle(oracle, m, path):
    m.attach(oracle, path)
    want = im.occ(m.codes, m.sa0)
    for c in range(16):
        got = np.array([oracle.lib.bwb_or_O(m.oracle_index, c, i) for i in range(m.length)], dtype=np.uint64)
        assert np.array_equal(got, want[:, c]), c
    assert [oracle.lib.bwb_or_O(m.oracle_index, c, 2**64 - 1) for c in range(16)] == [0] * 16


def test_occ_equals_the_oracle_at_every_position_of_rep(rep_model, oracle, tmp_path):
    _occ_vs_oracle(oracle, rep_model, str(tmp_path / "rep.bwt"))


@pytest.mark.parametrize("shape", im.REAL_SHAPES, ids=[s[0] for s in im.REAL_SHAPES])
def test_real_shapes_hold_their_claims_and_agree_with_the_oracle(shape, oracle, tmp_path):
    name, bases, seed, trim, claims = shape
    m = im.from_text(im.real_text(bases, seed, trim))
    got = im.shape_claims(m)
    assert {k: got[k] for k in claims} == claims
    assert (m.length % 2 == 0) == bool(trim)
    _occ_vs_oracle(oracle, m, str(tmp_path / "m.bwt"))
    # the oracle's invPsi walk through the model's file: the suffix array of the sort, in the model's count of steps
    sa = np.array([oracle.lib.bwb_or_SA(m.oracle_index, r) for r in range(m.length)], dtype=np.uint64)
    assert np.array_equal(sa, m.sa)
    steps = im.walk_steps(m)
    assert steps.max() < m.length and np.all(steps[::32] == 0)
    r = int(np.argmax(steps))  # the longest walk, replayed
    k, row = 0, r
    while row % 32:
        row = oracle.lib.bwb_or_invPsi(m.oracle_index, row)
        k += 1
    assert k == steps[r]


def test_real_shape_table_covers_the_edges():
    cl = [s[4] for s in im.REAL_SHAPES]
    assert {c["res"] for c in cl} >= {0, 1, 63, 64, 65, 127}
    assert any(c["length"] < 128 for c in cl) and any(129 <= c["length"] <= 256 for c in cl)
    for key in ("blk_start", "bkt_start", "last_blk", "low"):
        assert any(c.get(key) for c in cl), key
        assert key == "low" or any(c.get(key) and c.get("zero_after") for c in cl), key  # ... with a counted '$' row behind the sentinel in its bucket
    assert any(c.get("blk_start") and c.get("zero_next") for c in cl)
    assert any(c.get("last_blk") and c["length"] > 128 for c in cl)


def test_rank_family_covers_the_edges():
    fam = im.rank_family()
    assert len(set(fam)) == len(fam)
    assert {n % 128 for n, _, _ in fam if n >= 640} == {0, 1, 63, 64, 65, 127}
    assert {n for n, _, _ in fam} == set(im.RANK_LENGTHS) and {2, 3, 127, 128, 129, 255, 256, 257} <= set(im.RANK_LENGTHS)
    for n in im.RANK_LENGTHS:
        for c in im.CONTENTS:
            rows = [r for m, r, cc in fam if m == n and cc == c]
            assert len(rows) >= (2 if n > 2 else 1), (n, c)  # (two rows only: the sentinel can only be on row 1)
            if n > 128:
                assert any(r % 128 == 0 for r in rows), (n, c)
        rows = {r for m, r, cc in fam if m == n and cc == "uniform"}
        assert rows == set(im.sentinel_rows(n)) and (n - 1) in rows
        assert {r for r in (1, 31, 32, 63, 64, 127, 128, 192) if r < n} <= rows
        assert (n - 1) // 128 * 128 in rows or n <= 128
    # the contents are what they are called
    m = im.crafted(641, 128, "zero_first")
    assert np.all(m[::128] == 0)
    for j in im.QUIRK:
        c = im.crafted(641, 640, f"first{j}")
        assert np.all(c[:640:128] == j) and c[640] == 0
    assert len(np.unique(np.delete(im.crafted(257, 31, "single", seed=4), 31))) == 1
    assert len(np.unique(im.crafted(640, 1, "uniform"))) == 16


@pytest.mark.parametrize("content", im.CONTENTS)
def test_oracle_O_alphabet_equals_the_restatement_on_crafted_strings(content, oracle, tmp_path):
    for n, sa0, c in im.rank_family():
        if c != content:
            continue
        m = im.from_codes(im.crafted(n, sa0, c), sa0).attach(oracle, str(tmp_path / "c.bwt"))
        assert bw.BwtFile(m.path).length == n and m.num_occ == (n + 127) // 128 and m.num_words == (n + 7) // 8
        pos = np.concatenate([[im.NEG], np.arange(n, dtype=np.uint64)])
        assert np.array_equal(im.rank_alpha(m, pos)[:, 1:], im.rank_alpha_restated(m, pos)[:, 1:]), (n, sa0, c)
        ex = im.rank_exact(m, pos)
        assert np.array_equal(ex[0], m.C[:16]) and np.array_equal(ex[-1], m.C[1:]), (n, sa0, c)
        assert np.array_equal(oracle.O_single(m.oracle_index, pos[::7])[:, 1:] + m.C[None, 1:16], ex[::7, 1:]), (n, sa0, c)
        oracle.lib.bwb_or_free_index(m.oracle_index)


def test_children_of_the_root_are_the_C_intervals(oracle, tmp_path):
    m = im.from_codes(im.crafted(705, 640, "first9"), 640).attach(oracle, str(tmp_path / "c.bwt"))
    for alpha in (False, True):
        L, U, mask = im.children(m, [0], [m.length - 1], alpha)
        assert np.array_equal(L[0, 1:], m.C[1:16] + np.uint64(1)) and np.array_equal(U[0, 1:], m.C[2:17])
        assert int(mask[0]) == sum(1 << j for j in range(1, 16) if m.C[j + 1] > m.C[j])
