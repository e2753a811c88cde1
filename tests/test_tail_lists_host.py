"""The exact-tail fixture (tests/tail_model.py) holds what tests/test_gpu_tail_lists.py relies on - checked here on the CPU, with the model
of tests/ovf_model.py and with the oracle, so that the GPU test cannot pass vacuously: kl_search keeps a list's first interval and its tail in
registers and stores only the intervals in between (bwb_lane.h: list_add<P, true>), so every list length from one to nine and a long one
must occur, in the steps and at the hits, and adjacent intervals must merge somewhere.  CPU only."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bwbble_amd as bw
import oracle_lib
import ovf_model as om
import tail_model as tm

LENGTHS = set(range(1, 10))  # 1: the tail alone; 2: first + tail, no load; 3 .. 5: the remainder loop; 6 .. 9: one trip of the four-at-a-time loop + remainders 0 .. 3
LONG = 13                    # ... and two trips and more


@pytest.fixture(scope="module")
def tail(built, oracle, tmp_path_factory):
    fx = tm.TailFixture()
    fa = str(tmp_path_factory.mktemp("tail") / "tail.fa")
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    return fx, fx.text(), oracle.load_index(fa + ".bwt")


def walk(oracle, idx, read):
    """the exact search of `read` with the ORACLE's rank function, as exact_match_bounded walks it (the reverse complement from its last base
    = the read's complement from its first): per step (intervals of the list, appends that merged into the tail), until a list is empty"""
    x = idx.contents
    cur, out = [(0, x.length - 1)], []
    for ch in reversed(om.revcomp(read)):
        nxt, merged = [], 0
        for lo, hi in cur:
            for c in (om.CODES.index(k) for k in om.COMPAT[ch]):
                L = x.C[c] + oracle.lib.bwb_or_O(idx, c, C.c_uint64(lo - 1 & (1 << 64) - 1)) + 1
                U = x.C[c] + oracle.lib.bwb_or_O(idx, c, hi)
                if L <= U:
                    if nxt and L == nxt[-1][1] + 1:
                        nxt[-1] = (nxt[-1][0], U)
                        merged += 1
                    else:
                        nxt.append((L, U))
        if not nxt:
            break
        out.append((len(nxt), merged))
        cur = nxt
    return out


def test_fixture_is_small():
    fx = tm.TailFixture()
    assert sum(len(s) + 1 for _, s in fx.records) < 10000 and len(fx.names) <= 256
    assert all(38 <= len(fx.reads[n]) <= 42 for n in fx.names) and all(set(fx.reads[n]) <= set("ACGT") for n in fx.names)
    assert [r[2] for r in tm.RUNS] == ["AR", "CYS"] and all(set(r[2]) <= set(om.COMPAT[r[1]]) for r in tm.RUNS)


def test_model_list_lengths_cover_every_case(tail):
    fx, tx, _ = tail
    lists = {n: tx.tail_lists(fx.reads[n]) for n in fx.runs + fx.families + fx.plain}
    steps = {d for tl in lists.values() for d in tl}
    assert LENGTHS <= steps and max(steps) >= LONG, sorted(steps)
    finals = {tl[-1] for n, tl in lists.items() if len(tl) == len(fx.reads[n])}  # (the search reached the read's end: every interval is a hit)
    assert LENGTHS <= finals and max(finals) >= LONG, sorted(finals)
    # -P: the list after the first twelve steps is what the seeding path turns into heap entries
    seeded = {tl[tm.PRECALC - 1] for tl in lists.values() if len(tl) >= tm.PRECALC}
    assert {1, 2} <= seeded and max(seeded) >= 3
    # the first step from the whole index merges: the codes compatible with a base that are present in the text are more than their runs
    present = np.unique(tx.c)
    for b in "ACGT":
        codes = [c for c in present if tx.member[b][c]]
        assert len({int(tx.run[b][c]) for c in codes}) < len(codes), b
    # the run reads climb through the de Bruijn records' lists and come out with one hit
    for n in fx.runs:
        assert max(lists[n]) >= 16 and lists[n][-1] == 1 and len(lists[n]) == len(fx.reads[n]), (n, lists[n])


def test_oracle_walk_agrees_and_covers_every_case(tail, oracle):
    """the same from the index itself, rank by rank (merges included: never more intervals than the model's distinct strings), and the hits
    of -n 0 are the intervals of the last list"""
    fx, tx, idx = tail
    names = fx.runs + fx.families + fx.plain
    walks = {n: walk(oracle, idx, fx.reads[n]) for n in names}
    for n in names:
        want = tx.tail_lists(fx.reads[n])
        assert len(walks[n]) == len(want) and all(g <= w for (g, _), w in zip(walks[n], want)), (n, walks[n], want)
    steps = {g for w in walks.values() for g, _ in w}
    assert LENGTHS <= steps and max(steps) >= LONG, sorted(steps)
    assert all(w[0][1] > 0 for w in walks.values())                       # the first step from the whole index merges
    assert sum(m > 0 for w in walks.values() for _, m in w[1:]) > 0       # ... and so does a later one, onto a tail in the middle of a list
    seqs, lens = bw.encode_reads([fx.reads[n] for n in names])
    data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(["-n", "0"]))
    hits = dict(zip(names, (len(e) for e in oracle_lib.parse_aln(data))))
    assert all(hits[n] == (walks[n][-1][0] if len(walks[n]) == len(fx.reads[n]) else 0) for n in names)
    assert LENGTHS <= set(hits.values()) and max(hits.values()) >= LONG, sorted(set(hits.values()))
    seeded = {w[tm.PRECALC - 1][0] for w in walks.values() if len(w) >= tm.PRECALC}
    assert {1, 2} <= seeded and max(seeded) >= 3


@pytest.mark.parametrize("flags", tm.FLAG_SETS, ids="".join)
def test_every_parameter_set_has_work_of_its_kind(tail, oracle, flags):
    """tails that start from popped entries, gapped hits (the hit loop that looks for duplicates), hits under -P and -S"""
    fx, _, idx = tail
    seqs, lens = bw.encode_reads([fx.reads[n] for n in fx.names])
    data, st, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    hits = oracle_lib.parse_aln(data)
    assert sum(len(e) for e in hits) > 20
    if "-n0" not in "".join(flags):
        assert st.heap_pops > 10 * len(fx.names)
        assert sum(1 for e in hits for h in e if h["gapo"]) > 0
        if "-S" not in flags:
            assert max(len(e) for e in hits if e and e[0]["gapo"]) >= 6  # gapped entries that end in lists beyond first + tail + remainder
