"""The overflow fixture (tests/ovf_model.py) holds what tests/test_gpu_overflow.py relies on - checked here on the CPU, with the model and
the oracle, so that the GPU tests cannot pass vacuously - and the oracle is pinned to the real reference on a text of this kind
(tests/golden/make_golden_ovf.py).  CPU only."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bwbble_amd as bw
import oracle_lib
import ovf_model as om
from golden import make_golden_ovf as mgo

ALIGN_FLAGS = (["-n", "0"], ["-n", "2"], ["-n", "3", "-o", "2", "-e", "3"], ["-P", "-n", "2"])


@pytest.fixture(scope="module")
def ovf(built, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("ovf")
    fx = om.Fixture()
    fa = str(d / "ovf.fa")
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    return fx, fx.text(), oracle.load_index(fa + ".bwt")


def codes(read):
    seqs, _ = bw.encode_reads([read])
    return seqs[0, :len(read)]


def n_hits(oracle, idx, fx, names, flags):
    seqs, lens = bw.encode_reads([fx.reads[n] for n in names])
    data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    return dict(zip(names, (len(e) for e in oracle_lib.parse_aln(data))))


def rank_walk(oracle, idx, read, steps):
    """list lengths of the first `steps` steps of calculate_d on `read` from the ORACLE's rank function: one backward step per base over every
    interval of the list, children in code order, an interval that starts where the last one ended merged into it (align.c:93-110)"""
    x = idx.contents
    cur, out = [(0, x.length - 1)], []
    for ch in reversed(read[-steps:]):
        nxt = []
        for lo, hi in cur:
            for c in (om.CODES.index(k) for k in om.COMPAT[ch]):
                L = x.C[c] + oracle.lib.bwb_or_O(idx, c, C.c_uint64(lo - 1 & (1 << 64) - 1)) + 1
                U = x.C[c] + oracle.lib.bwb_or_O(idx, c, hi)
                if L <= U:
                    if nxt and L == nxt[-1][1] + 1:
                        nxt[-1] = (nxt[-1][0], U)
                    else:
                        nxt.append((L, U))
        out.append(len(nxt))
        cur = nxt
    return out


def test_generator_is_its_own():
    """the streams must not move with a library's version: known values of the generator, and the de Bruijn records"""
    rng = om.Lcg(1)
    assert [rng.next(), rng.next()] == [1357874332, 515420022] and om.Lcg(2).next() == 999454233
    assert om.Lcg(7).bases(12) == "CGTCTGAGCATC" and set(om.Lcg(7).bases(400)) == set("ACGT")
    for letters, order in ((om.A5, 6), (om.C3, 9)):
        s = om.de_bruijn(letters, order)
        assert len(s) == len(letters) ** order + order - 1
        assert len({s[i:i + order] for i in range(len(s) - order + 1)}) == len(letters) ** order
    assert om.COMPAT["A"] == "MHVRDWA" and sorted(om.COMPAT["C"]) == sorted("CYMSBHV") and set(om.A5) <= set(om.COMPAT["A"])
    assert om.revcomp("ARMC$") == "$GKYT"


def test_model_widths_equal_the_oracles_calculate_d(ovf, oracle):
    """the model's num_diff and interval width of every step, straight from the text, against calculate_d on the index: for the read and for
    its seed (restarts included: the short reads carry substitutions)"""
    fx, tx, idx = ovf
    p = oracle.params()
    names = om.CALCD_READS + ["p0", "p1", "q0", "q1", "q2", "q3", "f188", "f1300", "b1024"]
    restarts = 0
    for n in names:
        r = fx.reads[n]
        for part in (r, r[:om.SEED]):
            D = oracle.calculate_d(idx, codes(part), p)
            st = tx.steps(part)
            assert [(int(a), int(b)) for a, b in D[:len(part)]] == [(z, w) for z, w, _ in st], n
            restarts += st[-1][0]
    assert restarts > 0


def test_model_list_lengths_equal_a_walk_with_the_oracles_ranks(ovf, oracle):
    """distinct compatible strings (the model) = intervals of the list (rank by rank on the index, merges included) through the peak of a
    read of every class, in the read and in the seed, and of a family's read through all its steps"""
    fx, tx, idx = ovf
    for n, part, steps in (("e2a", fx.reads["e2a"], 9), ("e1a", fx.reads["e1a"], 11), ("e0b", fx.reads["e0b"], 11),
                           ("s2b", fx.reads["s2b"][:om.SEED], 9), ("s1a", fx.reads["s1a"][:om.SEED], 11),
                           ("p3", fx.reads["p3"], 12), ("p4rc", om.revcomp(fx.reads["p4"]), 12),
                           ("f1300", fx.reads["f1300"], 60)):
        want = [d for _, _, d in tx.steps(part)[:steps]]
        got = rank_walk(oracle, idx, part, steps)
        # (two strings that follow each other in a list and in the index as well are merged too - it happens in the short lists of the later
        # steps, and only ever makes fewer intervals.  The classes are asserted an eighth of a capacity away from it: a list of a quarter of
        # the smallest capacity or more must be modelled within a sixty-fourth)
        assert all(g <= w and (w < om.LCAP[0] // 4 or w - g <= w // 64) for g, w in zip(got, want)), (n, got, want)
        if n[0] in "es":
            assert max(got) == max(want), n
        assert max(want) == max(d for _, _, d in tx.steps(part)), n  # (the walk went through the peak)


def test_overflow_fixture_holds_every_case_it_exists_for(ovf, oracle):
    fx, tx, idx = ovf
    eighth = lambda n: om.clear_of(n, om.LCAP, om.LIST_SLACK)
    # interval lists: a peak in each class, in the read phase (e) and in the seed phase (s); everything else quiet
    for cls in (0, 1, 2):
        for t in "ab":
            own, seed = tx.peak(fx.reads[f"e{cls}{t}"])
            assert om.list_class(own) == cls and eighth(own) and seed <= om.QUIET, (cls, t, own, seed)
            own, seed = tx.peak(fx.reads[f"s{cls}{t}"])
            assert om.list_class(seed) == cls and eighth(seed) and own <= om.QUIET, (cls, t, own, seed)
    assert max(tx.peak(fx.reads["e2a"])) >= 5 ** 6 and max(tx.peak(fx.reads["s1a"])) >= 3 ** 8
    # the class-0 peaks are no small lists either: beyond half of the capacity
    assert all(max(tx.peak(fx.reads[f"{k}0{t}"])) > om.LCAP[0] // 2 for k in "es" for t in "ab")
    plain = [n for n in fx.reads if n[0] == "p"]
    short = [n for n in fx.reads if n[0] == "q"]
    assert len(plain) >= 24 and len(short) >= 36
    assert all(max(tx.peak(fx.reads[n])) <= om.QUIET for n in plain + short + list(om.FAMILIES))
    assert all(om.SEED < len(fx.reads[n]) for n in plain) and all(20 <= len(fx.reads[n]) <= om.SEED for n in short)
    assert any(len(fx.reads[n]) == om.SEED for n in short)
    # every long read lies in the ordinary record (or its reverse complement): one exact hit
    hits = n_hits(oracle, idx, fx, om.CALCD_READS + plain, ["-n", "0"])
    assert set(hits.values()) == {1}
    # hit lists: a family in each class, an eighth clear of 256 and 1 024 wherever a test asserts its class
    fam = {tuple(f): n_hits(oracle, idx, fx, list(om.FAMILIES), f) for f in ALIGN_FLAGS}
    n0, n2 = fam[("-n", "0")], fam[("-n", "2")]
    assert [om.hits_class(n0[k]) for k in ("f188", "f330", "f1300")] == [0, 1, 2]
    assert [om.hits_class(n2[k]) for k in ("f188", "f330", "f1300")] == [0, 0, 1]
    for f in ALIGN_FLAGS:
        assert all(om.clear_of(fam[tuple(f)][k], om.ACAP) for k in ("f188", "f330", "f1300")), (f, fam[tuple(f)])
    assert n0["f188"] <= 200
    # the reads that need gaps: hits only where two gap opens / three differences are allowed, hundreds of them in the families, and every
    # count an eighth clear of the hit-list capacities
    gap = {tuple(f): n_hits(oracle, idx, fx, list(om.GAPPED), f) for f in ALIGN_FLAGS}
    assert all(om.clear_of(h, om.ACAP) for f in gap for h in gap[f].values()), gap
    g3 = gap[("-n", "3", "-o", "2", "-e", "3")]
    assert all(g3.values()) and not any(n0[k] if k in n0 else gap[("-n", "0")][k] for k in om.GAPPED)
    assert sum(gap[("-n", "2")][k] == 0 for k in om.GAPPED) >= 6 and any(om.hits_class(h) == 1 for h in g3.values())
    # (with differences allowed the exact tails start from one interval of the heap: their lists stay below the family's size)
    assert all(om.FAMILIES[k][2] + om.LIST_SLACK <= om.LCAP[0] - om.LCAP[0] // 8 for k in om.FAMILIES)
    # the boundary reads: exactly the hits of their names
    assert {k: n0[k] for k in n0 if k[0] == "b"} == {f"b{v}": v for v in (255, 256, 257, 1023, 1024, 1025)}
    # the batches of the calculate_d and inheritance tests
    mixed = om.mixed_batch(fx)
    assert set(om.CALCD_READS) <= set(mixed) and mixed[0][0] == "p" and len(set(mixed)) == len(mixed)
    inh = om.inherit_batch(fx)
    assert inh[22] == "e2a" and all(n[0] == "q" for n in inh[23:31]) and {"s2a", "e1b", "s1a", "e0a"} <= set(inh)
    # ... short reads whose own list leaves class 0: the peak of the read they are the end of, behind a source of class 0, a smaller and a larger one
    for n, cls in (("t2", 2), ("t1", 1)):
        own, seed = tx.peak(fx.reads[n])
        assert len(fx.reads[n]) <= om.SEED and seed == 0 and om.list_class(own) == cls and eighth(own), (n, own)
    pairs = set()
    for i, n in enumerate(inh):
        if n[0] == "t":
            src = next(m for m in reversed(inh[:i]) if len(fx.reads[m]) > om.SEED)
            pairs.add((n, int(src[1]) if src[0] in "es" else 0))
    assert {("t2", 0), ("t2", 1), ("t1", 2), ("t1", 0)} <= pairs
    cls = om.inherit_classes(fx, inh)
    assert [cls[i] for i in (22, 23, 30, 31)] == [2, 2, 2, 0] and cls.count(1) >= 8 and cls.count(2) >= 16
    # the hit log: totals that make it grow once, and twice
    for name, growths in (("class0", 1), ("rerun1", 1), ("rerun2", 1), ("twice", 2), ("survive", 1)):
        names = om.log_case(name)
        cap = om.log_cap(len(names))
        total = sum(n0.get(n, 1) for n in names)
        assert cap == om.LOG_MIN and len(names) <= 8192
        assert cap * om.LOG_GROWTH ** (growths - 1) + cap // 64 < total <= cap * om.LOG_GROWTH ** growths, (name, total)
    assert max(n0[n] for n, _ in om.LOG_CASES["class0"]) <= 200
    # ... rerun1 fills it in class 1, rerun2 in class 2 and not before; survive: the log is full only for the last reads
    r1 = dict(om.LOG_CASES["rerun1"])
    assert r1["p0"] < om.LOG_MIN < r1["p0"] + r1["f330"] * n0["f330"] and om.hits_class(n0["f330"]) == 1
    assert om.hits_class(n0["f1300"]) == 2
    sv = om.LOG_CASES["survive"]
    assert sv[0][1] + (sv[1][1] - 30) * n0["f188"] < om.LOG_MIN


def test_big_family_leaves_class_one_in_the_exact_search(built, oracle, tmp_path):
    fx = om.big_fixture()
    fa = str(tmp_path / "big.fa")
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    idx = oracle.load_index(fa + ".bwt")
    assert idx.contents.length < 1000000
    r = fx.reads["big"]
    fx.reads["big_rc"] = om.revcomp(r)
    hits = n_hits(oracle, idx, fx, ["big", "big_rc"], ["-n", "0"])
    # one hit per interval of the exact search's last list (merged intervals: fewer than the model's distinct strings)
    tx = fx.text()
    for name, n in hits.items():
        assert om.LCAP[1] + om.LCAP[1] // 8 <= n <= tx.tail_lists(fx.reads[name])[-1] and om.hits_class(n) == 2 and om.clear_of(n, om.ACAP)
    assert max(tx.peak(fx.reads["p0"])) <= om.QUIET


def test_inheritance_fixture_discriminates(ovf, oracle):
    """the short reads' results depend on whose D_seed they see"""
    fx, tx, idx = ovf
    seqs, lens = bw.encode_reads([fx.reads[n] for n in om.inherit_batch(fx)])
    p = oracle.params(["-n", "2"])
    assert oracle.align_encoded(idx, seqs, lens, p, fresh_dseed=1)[0] != oracle.align_encoded(idx, seqs, lens, p, fresh_dseed=0)[0]


# -- the oracle against the real reference on this kind of text ------------------------------------------------------------------------

def test_golden_files_are_what_the_generator_writes(golden):
    fa, fq = mgo.texts()
    assert gzip.open(os.path.join(golden, "ovf.fa.gz"), "rb").read() == fa.encode()
    assert gzip.open(os.path.join(golden, "ovf.fq.gz"), "rb").read() == fq.encode()
    limit = os.path.getsize(os.path.join(golden, "rep_sa.npy"))
    assert all(os.path.getsize(os.path.join(golden, f)) <= limit for f in mgo.FILES)


@pytest.mark.parametrize("name", sorted(mgo.CONFIGS))
def test_oracle_matches_reference_on_iupac_dense_text(oracle, golden, tmp_path, name):
    """lists of 15 625 intervals in calculate_d, reads with 300 and 1 300 hits on both strands, reads that need two gap opens or three
    differences: the reference's bytes"""
    fa = mgo.unpack(tmp_path)
    want = gzip.open(os.path.join(golden, f"ovf_{name}.aln.gz"), "rb").read()
    out = str(tmp_path / "o.aln")
    oracle.align_fastq(fa + ".bwt", str(tmp_path / "ovf.fq"), out, oracle.params(mgo.CONFIGS[name]))
    assert open(out, "rb").read() == want
    hits = oracle_lib.parse_aln(want)
    most = max(len(e) for e in hits)
    assert most > (om.ACAP[1] if name == "n0" else om.ACAP[0])
    if name == "n3gap":  # the gapped setting finds what -n 2 (one gap open, two differences) cannot: in the ordinary record and in the families
        assert want != gzip.open(os.path.join(golden, "ovf_n2.aln.gz"), "rb").read()
        by_name = dict(zip(om.golden_reads(om.golden_fixture()), hits))
        two = [n for n in om.GAPPED if by_name[n] and all(e["gapo"] == 2 for e in by_name[n])]
        assert {"g_del_ins", "g_del_del", "g_ins_ins", "g_f330_del_ins", "g_f330rc_ins_ins"} <= set(two)
        assert all(e["gape"] == 1 and e["gapo"] == 1 for e in by_name["g_del2"]) and all(e["mm"] == 3 for e in by_name["g_sub3"])
        assert all(by_name[n] for n in om.GAPPED) and max(len(by_name[n]) for n in two) > 100


def test_product_index_matches_reference_on_iupac_dense_text(built, golden, tmp_path):
    (tmp_path / "ref").mkdir()
    ref = mgo.unpack(tmp_path / "ref")
    fa = str(tmp_path / "ovf.fa")
    open(fa, "wb").write(open(ref, "rb").read())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    assert open(fa + ".bwt", "rb").read() == open(ref + ".bwt", "rb").read()
    assert open(fa + ".ann", "rb").read() == open(ref + ".ann", "rb").read()
