"""The fixture of tests/params_model.py holds what tests/test_gpu_params.py relies on - proved here on the CPU, with the oracle and with a count
straight from the text, so that the GPU test cannot pass vacuously: max_best and no_indel_length each DECIDE records of these reads, at the
values the model says.  These are conditions on the inputs: where one fails, the input changes, not the condition.  CPU only."""
import subprocess

import pytest

import bwbble_amd as bw
import oracle_lib
import params_model as pm

# the max_best families under: two differences (a best hit with none or one arrives in popped entries; the next score's through exact tails,
# or - a difference at the base consumed last - popped), and one difference with a gap open that costs less than two mismatches (the best hit
# of a read with a substitution of its own arrives through an exact tail, the gapped variant after it through another)
BEST_FLAGS = (("-n", "2"), ("-n", "1", "-O", "4"))


@pytest.fixture(scope="module")
def fixture(built, oracle, tmp_path_factory):
    fx = pm.ParamsFixture()
    fa = str(tmp_path_factory.mktemp("params") / "params.fa")
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    return fx, fx.text(), oracle.load_index(fa + ".bwt")


def records(oracle, idx, fx, names, flags, **fields):
    seqs, lens = fx.batch(names)
    data, st, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(list(flags), **fields))
    return oracle_lib.parse_aln(data), st


def test_fixture_is_small():
    fx = pm.ParamsFixture()
    assert sum(len(s) + 1 for _, s in fx.records) < 40000 and len(fx.names) <= 320
    assert all(40 <= len(r) <= 60 and set(r) <= set("ACGT") for r in fx.reads.values())
    assert not set("BDHVN") & set("".join(s for _, s in fx.records))  # (no code the inexact search cannot step over: the count below is exact)
    assert len(fx.best_names) == 6 * (3 * len(pm.COPIES) + len(pm.IUPAC_COPIES)) and len(fx.indel1) == 72


@pytest.mark.parametrize("flags", BEST_FLAGS, ids="".join)
def test_every_family_flips_at_the_threshold_counted_from_the_text(fixture, oracle, flags):
    """a sweep of max_best from -1 to T + 2 (here: to 36 for all) changes a family read's record at exactly one value, T = the number of its
    best placements; below it the record holds one score, from it on two"""
    fx, tx, idx = fixture
    names = fx.best_names
    sweep = list(range(-1, 37))
    recs = {mb: records(oracle, idx, fx, names, flags, max_best=mb)[0] for mb in sweep}
    T = {}
    for j, n in enumerate(names):
        flips = [mb for mb in sweep[1:] if recs[mb][j] != recs[mb - 1][j]]
        T[n] = pm.threshold(tx, fx.reads[n], int(flags[1]))[0]
        assert flips == [T[n]], (n, flips, T[n])
        assert len({h["score"] for h in recs[T[n] - 1][j]}) == 1 and len({h["score"] for h in recs[T[n]][j]}) == 2, n
        best = min(h["score"] for h in recs[36][j])
        assert sum(h["U"] - h["L"] + 1 for h in recs[36][j] if h["score"] == best) == T[n], n
    assert recs[-1] == recs[0] and recs[36] == records(oracle, idx, fx, names, flags, max_best=pm.MAX_BEST_MAX)[0]
    # every R on either side of the default, at every site; the IUPAC families' best hits are lists (and their thresholds summed widths)
    for R in pm.COPIES:
        assert all(T[f"r{R}{s}"] == R and T[f"r{R}{s}_rc"] == R for s in pm.SITES)
    for j, n in enumerate(names):
        if n[0] == "u":
            best = [h for h in recs[36][j] if h["score"] == recs[36][j][0]["score"]]
            assert len(best) >= 2, (n, best)
    lists = {len([h for h in recs[36][names.index(n)] if h["score"] == recs[36][names.index(n)][0]["score"]]) for n in names if n[0] == "u"}
    assert len(lists) >= 4 and max(lists) >= 6, sorted(lists)
    wide = [n for j, n in enumerate(names) if n[0] == "r" and "_q" in n and recs[36][j][0]["U"] - recs[36][j][0]["L"] + 1 > 1]
    assert len(wide) == 4 * 3 * (len(pm.COPIES) - 1)  # every substituted read of a family with R > 1: its best hit is one interval R wide


def test_the_default_lies_inside_the_sweep(fixture, oracle):
    """max_best = 30: the families of 31 and 33 copies stop, those of 8 and fewer do not"""
    fx, _, idx = fixture
    names = [f"r{R}{s}" for R in (8, 31, 33) for s in pm.SITES]
    recs, _ = records(oracle, idx, fx, names, ("-n", "2"))
    assert [len(r) for r in recs] == [3] * 3 + [1] * 6


def test_no_indel_length_decides_at_every_step(fixture, oracle):
    """one indel at distance d from an end, -n 1: at every step of no_indel_length from 1 to 9 some read gains or loses its gapped hit;
    0 and 1 differ in the pushes only; at 0 there are hits whose gap run lies within 5 path positions of either end of the path"""
    fx, _, idx = fixture
    names = list(fx.indel1)
    gapped, pushes, near = {}, {}, {}
    for v in range(-1, 11):
        recs, st = records(oracle, idx, fx, names, ("-n", "1"), no_indel_length=v)
        gapped[v] = {n for n, r in zip(names, recs) if any(h["gapo"] for h in r)}
        pushes[v] = st.heap_pushes
        ends = [pm.gap_ends(h) for r in recs for h in r if h["gapo"]]
        near[v] = (sum(e[0] < 5 for e in ends), sum(e[1] < 5 for e in ends))
    for v in range(2, 10):
        assert gapped[v] != gapped[v - 1], v
    assert gapped[0] == gapped[1] and pushes[0] != pushes[1]
    assert gapped[-1] == gapped[0] and pushes[-1] == pushes[0]  # (fewer than zero bases are never left)
    assert len(gapped[0]) > 50 and len(gapped[10]) < 6
    assert near[0][0] >= 5 and near[0][1] >= 5 and near[5][0] + near[5][1] < near[0][0] + near[0][1], near


@pytest.mark.parametrize("flags", [("-n", "2", "-o", "2", "-e", "2"), ("-n", "3", "-o", "1", "-e", "3")], ids="".join)
def test_a_second_gap_moves_the_bound_by_one(fixture, oracle, flags):
    """the `+ num_gapo + num_gape` of the bound: reads with a second indel (two opens) or a two-base gap (an extension) at distance d from an
    end change at a step of no_indel_length at which the one-indel reads of the same kind, side and d do not"""
    fx, _, idx = fixture
    names = list(fx.indel1) + list(fx.indel2)
    recs = {v: records(oracle, idx, fx, names, flags, no_indel_length=v)[0] for v in range(-1, 12)}
    steps = {n: {v for v in range(0, 12) if recs[v][j] != recs[v - 1][j]} for j, n in enumerate(names)}
    own = {}
    for n, (kind, side, d) in fx.indel2.items():
        k1 = "del" if kind == "del2" else kind
        if steps[n] - steps[f"i1_{k1}_{side}{d}"] - steps[f"i1_{k1}_{side}{d}_rc"]:
            own.setdefault((kind, side), []).append(d)
    kinds = ("del", "ins", "del2") if "-o2" in "".join(flags) else ("del2",)  # (one gap open: only the extension is a second gap)
    for kind in kinds:
        for side in ("head", "tail"):
            assert len(own.get((kind, side), [])) >= 3, (kind, side, own)
    two = [h for j, n in enumerate(names) if n in fx.indel2 for h in recs[0][j] if h["gapo"] + h["gape"] >= 2]
    assert len(two) >= 10
