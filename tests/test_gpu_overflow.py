"""The re-runs of reads that exceed a per-read capacity - SA-interval list, hit list, the slot's hit log - on the constructed texts of
tests/ovf_model.py (tests/test_ovf_host.py proves on the CPU that the reads overflow what their names say).  Every case: .aln bytes (or
hit records) and the visit / pop / push counters equal to the CPU oracle's; where a class is asserted, n_overflow_reads and
launches_calc_d equal to the model's prediction."""
import os
import subprocess

import numpy as np
import pytest

import bwbble_amd as bw
import map_model
import oracle_lib
import ovf_model as om

pytestmark = pytest.mark.gpu


def build_index(fx, d, name):
    fa = str(d / name)
    open(fa, "w").write(fx.fasta())
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    return fa + ".bwt"


@pytest.fixture(scope="module")
def ovf(built, oracle, tmp_path_factory):
    fx = om.Fixture()
    bwt = build_index(fx, tmp_path_factory.mktemp("ovf"), "ovf.fa")
    return fx, bwt, oracle.load_index(bwt)


@pytest.fixture(scope="module")
def ctx(ovf):
    c = bw.Context(ovf[1])
    yield c
    c.close()


def encode(fx, names):
    return bw.encode_reads([fx.reads[n] for n in names])


def check(ctx, oracle, idx, flags, seqs, lens):
    off, alns = ctx.align(bw.params(flags), seqs, lens)
    want, ost, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    assert bw.aln_bytes(off, alns) == want
    st = ctx.stats()
    assert st.visits_single + st.visits_alphabet == ost.visits_single + ost.visits_alphabet
    assert st.heap_pops == ost.heap_pops and st.heap_pushes == ost.heap_pushes
    return st


D_OVERFLOWS = [n for n in om.CALCD_READS if n[1] != "0"]  # the reads whose calculate_d leaves class 0 (half of them leave class 1 too)
ALIGN_FLAGS = (["-n", "0"], ["-n", "2"], ["-n", "3", "-o", "2", "-e", "3"], ["-P", "-n", "2"])


def test_calc_d_lists_of_every_class_match_oracle(ovf, ctx, oracle):
    """D and D_seed of reads whose list peaks in class 0, 1 and 2, at the read's end and inside the seed, among plain reads: the class loop
    of bwb_hip_calc_d (one launch per class)"""
    fx, _, idx = ovf
    names = om.mixed_batch(fx)
    seqs, lens = encode(fx, names)
    p = bw.params(["-n", "2"])
    D, Ds = ctx.calc_d(p, seqs, lens)
    assert ctx.stats().launches_calc_d == 3
    op = oracle.params(["-n", "2"])
    for i, n in enumerate(names):
        ln = int(lens[i])
        assert np.array_equal(D[i, :ln + 1], oracle.calculate_d(idx, seqs[i, :ln], op)), n
        assert np.array_equal(Ds[i, :om.SEED + 1], oracle.calculate_d(idx, seqs[i, :om.SEED], op)), n


@pytest.mark.parametrize("flags", ALIGN_FLAGS, ids=lambda f: "".join(f))
def test_calc_d_overflows_are_rerun_in_their_class(ovf, ctx, oracle, flags):
    """ST_D_OVF from kl_calc_d (read phase and seed phase), the dfail branch of kl_search, and both kernels again in class 1 and class 2;
    among them the reads that only two gap opens or three differences place (some with hundreds of such hits: their hit list overflows)"""
    fx, _, idx = ovf
    names = om.mixed_batch(fx) + list(om.GAPPED)
    seqs, lens = encode(fx, names)
    st = check(ctx, oracle, idx, flags, seqs, lens)
    hits = [len(e) for e in oracle_lib.parse_aln(oracle.align_encoded(idx, seqs, lens, oracle.params(flags))[0])]
    gapped = hits[-len(om.GAPPED):]
    assert len(D_OVERFLOWS) == 8 and st.n_overflow_reads == 8 + sum(om.hits_class(h) > 0 for h in gapped)
    assert st.launches_calc_d == 3  # class 0, class 1 (eight reads), class 2 (four)
    if "-o" in flags:
        assert all(gapped) and sum(om.hits_class(h) > 0 for h in gapped) >= 1


def test_short_reads_inherit_dseed_from_a_read_that_overflows(ovf, ctx, oracle):
    """k_dseed_inherit hands ST_D_OVF on as ST_D_WAIT: a read no longer than the seed waits for the class in which its source's calculate_d
    fits - its own is not run again (the counters would show it), unless it overflowed as well; in one batch, and streamed in batches of
    23 reads whose carried read is the one that overflows"""
    fx, _, idx = ovf
    names = om.inherit_batch(fx)
    seqs, lens = encode(fx, names)
    for flags in (["-n", "2"], ["-n", "3", "-k", "1"]):
        st = check(ctx, oracle, idx, flags, seqs, lens)  # (the serial oracle: fresh_dseed = 0)
        assert st.n_overflow_reads == sum(k > 0 for k in om.inherit_classes(fx, names)) and st.launches_calc_d == 3
        fresh, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags), fresh_dseed=1)
        stale, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags), fresh_dseed=0)
        assert fresh != stale
        p = bw.params(flags)
        got, last = b"", None
        ctx.flush()
        for lo in range(0, len(lens), 23):
            hi = min(lo + 23, len(lens))
            ctx.slot_upload(0, p, seqs[lo:hi], lens[lo:hi], carry=last)
            ctx.slot_submit(0)
            off, alns = ctx.slot_result(0)
            got += bw.aln_bytes(off, alns)
            for i in range(lo, hi):
                if lens[i] > p.seed_length:
                    last = seqs[i, :lens[i]].copy()
        assert got == stale


@pytest.mark.parametrize("flags", ALIGN_FLAGS, ids=lambda f: "".join(f))
def test_hit_lists_of_every_class(ovf, ctx, oracle, flags):
    """183 / 319 / 1 351 hits at -n 0 (class 0 / 1 / 2), 50 / 103 / 380 at -n 2 (0 / 0 / 1): as many reads leave class 0 as the oracle's hit
    counts say (tests/test_ovf_host.py: each an eighth of a capacity away from it, for every flag set)"""
    fx, _, idx = ovf
    names = [n for n in fx.reads if n[0] == "p"][:12] + ["f188", "f330", "f1300"]
    seqs, lens = encode(fx, names)
    st = check(ctx, oracle, idx, flags, seqs, lens)
    hits = [len(e) for e in oracle_lib.parse_aln(oracle.align_encoded(idx, seqs, lens, oracle.params(flags))[0])]
    assert st.n_overflow_reads == sum(om.hits_class(h) > 0 for h in hits)
    assert flags != ["-n", "0"] or [om.hits_class(h) for h in hits[-3:]] == [0, 1, 2]


def test_hit_counts_at_the_capacities(ovf, ctx, oracle):
    """exactly 255, 256, 257 and 1 023, 1 024, 1 025 hits (beside the 4-way unrolled add_aln loops): bytes only"""
    fx, _, idx = ovf
    names = [n for n in om.FAMILIES if n[0] == "b"]
    seqs, lens = encode(fx, names)
    off, alns = ctx.align(bw.params(["-n", "0"]), seqs, lens)
    assert [int(b - a) for a, b in zip(off[:-1], off[1:])] == [int(n[1:]) for n in names]
    assert bw.aln_bytes(off, alns) == oracle.align_encoded(idx, seqs, lens, oracle.params(["-n", "0"]))[0]
    check(ctx, oracle, idx, ["-n", "2"], seqs, lens)


def test_exact_search_list_beyond_class_one(built, oracle, tmp_path):
    """a family of 10 600: the read's lists - calculate_d's and the exact search's - and its hit list all leave class 1"""
    fx = om.big_fixture()
    bwt = build_index(fx, tmp_path, "big.fa")
    idx = oracle.load_index(bwt)
    fx.reads["big_rc"] = om.revcomp(fx.reads["big"])
    c = bw.Context(bwt)
    try:
        names = [n for n in fx.reads if n[0] == "p"] + ["big", "big_rc"]
        st = check(c, oracle, idx, ["-n", "0"], *encode(fx, names))
        assert st.n_overflow_reads == 2 and st.launches_calc_d == 3
        check(c, oracle, idx, ["-n", "2"], *encode(fx, names))
    finally:
        c.close()


@pytest.fixture(scope="module")
def log_ctx(ovf):
    c = bw.Context(ovf[1])
    yield c
    c.close()


@pytest.mark.parametrize("slot,case,growths", [(1, "class0", 1), (2, "rerun1", 1), (3, "rerun2", 1), (4, "twice", 2), (5, "survive", 1)])
def test_hit_log_grows_and_keeps_its_records(ovf, log_ctx, oracle, slot, case, growths):
    """ST_OUT_OVF: in class 0, inside the class-1 and class-2 re-runs, twice, and for the last reads only - each case in a slot of its own
    (a slot's log never shrinks).  The batches repeat a few reads: every copy's records must equal the oracle's for its read."""
    fx, _, idx = ovf
    names = om.log_case(case)
    seqs, lens = encode(fx, names)
    log_ctx.slot_upload(slot, bw.params(["-n", "0"]), seqs, lens)
    log_ctx.slot_submit(slot)
    off, alns = log_ctx.slot_result(slot)
    assert len(alns) > om.log_cap(len(names)) * om.LOG_GROWTH ** (growths - 1)  # the log grew (twice)
    assert len(off) == len(names) + 1
    # the first copy of every read: the oracle's bytes; every other copy: the records of the first (serialising 270 000 hits would take long)
    first, fields = {}, [f for f in bw.ALN_DTYPE.names if not f.startswith("reserved")]
    for i, n in enumerate(names):
        got = alns[int(off[i]):int(off[i + 1])]
        if n not in first:
            want, _, _ = oracle.align_encoded(idx, seqs[i:i + 1], lens[i:i + 1], oracle.params(["-n", "0"]))
            assert bw.aln_bytes(np.array([0, len(got)], dtype=np.uint64), got) == want, (i, n)
            first[n] = got
        else:
            assert len(got) == len(first[n]) and all(np.array_equal(got[f], first[n][f]) for f in fields), (i, n)


@pytest.mark.parametrize("env", [{"BWB_FORCE_POS64": "1"}, {"BWB_DTAB": "1", "BWB_DTAB_K": "7"}], ids=["pos64", "dtab7"])
def test_overflow_reruns_with_other_machinery(ovf, oracle, monkeypatch, env):
    """64-bit positions; the calculate_d table with K = 7, whose AAAAAAA entry is longer than class 0 and class 1 hold (from_table falls
    back there and is taken in class 2: fewer buckets loaded by kl_calc_d than without the table, for the same visits)"""
    fx, bwt, idx = ovf
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = bw.Context(bwt)
    try:
        names = om.mixed_batch(fx) + ["f188", "f330", "f1300"]
        seqs, lens = encode(fx, names)
        st = check(c, oracle, idx, ["-n", "2"], seqs, lens)
        assert st.n_overflow_reads == len(D_OVERFLOWS) + 1 and st.launches_calc_d == 3
        st = check(c, oracle, idx, ["-n", "0"], seqs, lens)
        assert st.n_overflow_reads == len(D_OVERFLOWS) + 2
        check(c, oracle, idx, ["-n", "2"], *encode(fx, om.inherit_batch(fx)))
        if "BWB_DTAB" in env:
            # the reads that end in AAAAAAA alone: their first seven steps come from the table only in class 2
            e2 = encode(fx, ["e2a", "e2b"] * 8)
            with_tab = check(c, oracle, idx, ["-n", "2"], *e2)
            monkeypatch.setenv("BWB_DTAB", "0")
            plain = bw.Context(bwt)
            try:
                without = check(plain, oracle, idx, ["-n", "2"], *e2)
            finally:
                plain.close()
            assert with_tab.launches_calc_d == without.launches_calc_d == 3 and with_tab.visits_calc_d == without.visits_calc_d
            assert with_tab.bucket_loads_calc_d < without.bucket_loads_calc_d
    finally:
        c.close()


def test_overflow_reruns_while_other_slots_hold_parked_reads(ovf, oracle, monkeypatch):
    """BWB_SLICE_ITERS=150, every slot submitted before the first result is taken: the reads of slot 0 that overflow are re-run while the
    heavy reads of the later slots (a family's read at -n 2: tens of thousands of heap entries) are parked - the draining launch at the top
    of rerun_overflows finishes those before class 1 takes the chunk pool.  Every slot's bytes, and the counters of all of them."""
    fx, bwt, idx = ovf
    monkeypatch.setenv("BWB_SLICE_ITERS", "150")
    flags = ["-n", "2"]
    p = bw.params(flags)
    base = om.mixed_batch(fx)
    batches = [base[j:] + base[:j] + ["f188", "f330", "f1300"] * 4 for j in range(bw.MAX_SLOTS)]
    want, tot = [], [0, 0, 0]
    for names in batches:
        data, ost, _ = oracle.align_encoded(idx, *encode(fx, names), oracle.params(flags))
        want.append(data)
        tot = [tot[0] + ost.visits_single + ost.visits_alphabet, tot[1] + ost.heap_pops, tot[2] + ost.heap_pushes]
    c = bw.Context(bwt)
    try:
        for j, names in enumerate(batches):
            c.slot_upload(j, p, *encode(fx, names))
            c.slot_submit(j)
        got = [bw.aln_bytes(*c.slot_result(j)) for j in range(len(batches))]
        c.flush()
        assert got == want
        st = c.stats()
        assert [st.visits_single + st.visits_alphabet, st.heap_pops, st.heap_pushes] == tot
        assert st.n_parked_reads > 0 and st.n_overflow_reads == len(batches) * (len(D_OVERFLOWS) + 4)
    finally:
        c.close()


def test_overflows_in_batches_uploaded_ahead(ovf, oracle, monkeypatch):
    """BWB_CALCD_AHEAD=2: kl_calc_d and k_dseed_inherit of the batches ahead run on the second stream; the inheritance batch in batches of 23
    reads, all uploaded before the first submit, each with its carried read (the first one's overflows): the serial oracle's bytes"""
    fx, bwt, idx = ovf
    monkeypatch.setenv("BWB_CALCD_AHEAD", "2")
    names = om.inherit_batch(fx)
    seqs, lens = encode(fx, names)
    flags = ["-n", "2"]
    want, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    p = bw.params(flags)
    cuts = list(range(0, len(lens), 23)) + [len(lens)]
    assert 3 < len(cuts) - 1 <= bw.MAX_SLOTS
    c = bw.Context(bwt)
    try:
        last = None
        for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            c.slot_upload(j, p, seqs[lo:hi], lens[lo:hi], carry=last)
            for i in range(lo, hi):
                if lens[i] > p.seed_length:
                    last = seqs[i, :lens[i]].copy()
        got = b""
        for j in range(len(cuts) - 1):
            c.slot_submit(j)
        for j in range(len(cuts) - 1):
            got += bw.aln_bytes(*c.slot_result(j))
        assert got == want
        st = c.stats()
        assert st.n_overflow_reads == sum(k > 0 for k in om.inherit_classes(fx, names)) and st.launches_calc_d > len(cuts) - 1
    finally:
        c.close()


def test_cli_align_of_the_overflow_reads(ovf, oracle, tmp_path):
    """`bwbble align` in chunks of 97 reads on a FASTQ of every kind of overflowing read: the bytes of the oracle's align_fastq"""
    fx, bwt, _ = ovf
    names = om.mixed_batch(fx) + om.inherit_batch(fx) + ["f188", "f330", "f1300", "b257", "b1025"]
    fq, got, want = str(tmp_path / "ovf.fq"), str(tmp_path / "got.aln"), str(tmp_path / "want.aln")
    open(fq, "w").write(fx.fastq(names))
    assert len(names) > 97
    for flags in (["-n", "0"], ["-n", "2"]):
        r = subprocess.run([bw.HOST_BIN, "align"] + flags + [bwt[:-len(".bwt")], fq, got], env=dict(os.environ, BWB_CHUNK="97"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        oracle.align_fastq(bwt, fq, want, oracle.params(flags))
        assert open(got, "rb").read() == open(want, "rb").read() and os.path.getsize(want) > 10000


def test_place_after_a_log_growth(ovf, oracle):
    """k_place reads the slot's hit log where grow_log left it (inside the class-1 re-run): eval_aln of the oracle's hits"""
    fx, bwt, _ = ovf
    names = om.log_case("rerun1")
    seqs, lens = encode(fx, names)
    idx = oracle.load_index(bwt, load_sa=True)
    b = bw.BwtFile(bwt, load_sa=True)
    c = bw.Context(b)
    try:
        c.set_sa(b.SA)
        off, alns = c.align(bw.params(["-n", "0"]), seqs, lens)
        assert len(alns) > om.log_cap(len(names))
        data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(["-n", "0"]))
        want, _ = map_model.expected_places(oracle, idx, oracle_lib.parse_aln(data), 6)
        got = c.place(6)
        assert map_model.first_difference(got, want) is None, map_model.first_difference(got, want)
        assert got.tobytes() == want.tobytes() and (want["top1"] > om.ACAP[0]).any()
    finally:
        c.close()
