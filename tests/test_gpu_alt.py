"""`bwbble map -X` on the GPU: kernels k_alt_count / the scan / k_place_alt through Context.place_alt, place_hits_alt and slot_place_alt
against the Python restatement (tests/alt_model.py) fed with the ORACLE's hits or the fixtures' - never the library's own hits - and
positions from the reference's SA() (rep_sa.npy) or the oracle's walk; items compared as bytes, the work as exact invPsi step counts.
Then the command line: `map -X`, `aln2sam -X`, and `map` without -X."""
import os
import random
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import map_model
import oracle_lib
from golden.make_golden import ALIGN_CONFIGS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 4, 5, 255)

ALT_CONFIGS = {
    "rep_n3": ("rep.fa", "rep.fq", ["-n", "3"]),
    "rep_gap_n4": ("rep.fa", "rep_gap.fq", ["-n", "4", "-o", "1"]),
    "toy_n4gap": ("toy.fa", "toy.fq", ALIGN_CONFIGS["n4gap"]),
    "toy_s2": ("toy.fa", "toy.fq", ["-S", "-n", "2"]),
}


def sa_context(bwt_path):
    b = bw.BwtFile(bwt_path, load_sa=True)
    ctx = bw.Context(b)
    ctx.set_sa(b.SA)
    return ctx


def same_alts(got, want, what=""):
    goff, galts = got
    woff, walts = want
    assert np.array_equal(goff, woff), (what, "alt_off differs")
    assert alt_model.first_difference(galts, walts) is None, (what, alt_model.first_difference(galts, walts))
    assert galts.tobytes() == walts.tobytes(), what


@pytest.mark.parametrize("name", list(ALT_CONFIGS))
def test_place_alt_equals_the_model_on_the_oracles_hits(built, golden, oracle, name):
    fa, fq, flags = ALT_CONFIGS[name]
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, fq)))
    idx = oracle.load_index(os.path.join(golden, fa + ".bwt"), load_sa=True)
    data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    reads = oracle_lib.parse_aln(data)
    if name in ("rep_n3", "rep_gap_n4"):  # the oracle's hits are the reference's
        assert data == open(os.path.join(golden, name + ".aln"), "rb").read()
    sa = alt_model.rep_sa(golden) if fa == "rep.fa" else alt_model.OracleSA(oracle, idx)
    ctx = sa_context(os.path.join(golden, fa + ".bwt"))
    try:
        ctx.align(bw.params(flags), seqs, lens)
        plain = ctx.place(6)
        for max_alt in NS:
            off, alts, steps = alt_model.expected_alts(reads, max_alt, sa)
            places, goff, galts = ctx.place_alt(6, max_alt)
            same_alts((goff, galts), (off, alts), (name, max_alt))
            items, st, ms = ctx.place_alt_stats()
            assert (items, st) == (len(alts), steps) and ms > 0
            assert places.tobytes() == plain.tobytes() == ctx.place(6).tobytes()
        if name == "rep_n3":
            assert [int((np.diff(alt_model.expected_alts(reads, n, sa)[0]) > 0).sum()) for n in NS] == [10, 55, 60, 60]
        if name == "rep_gap_n4":
            assert (alts["num_gapo"] > 0).sum() >= 20 and len(set(alts["flags"])) == 2
    finally:
        ctx.close()


# ---- injected hit lists (tests/golden/alt_hits.*, made by tests/golden/make_golden_alt.py) ---------------------------------------

@pytest.fixture(scope="module")
def hits(golden):
    """the fixture's hit lists as bwb_aln records, the model's places and, per N, (alt_off, items, steps)"""
    reads = oracle_lib.parse_aln(open(os.path.join(golden, "alt_hits.aln"), "rb").read())
    off, alns = map_model.aln_records(reads)
    sa = alt_model.rep_sa(golden)
    return types.SimpleNamespace(reads=reads, off=off, alns=alns, sa=sa, want={n: alt_model.expected_alts(reads, n, sa) for n in NS})


@pytest.fixture()
def rep_ctx(built, golden):
    ctx = sa_context(os.path.join(golden, "rep.fa.bwt"))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("max_alt", NS)
def test_place_hits_alt_equals_the_model(rep_ctx, hits, max_alt):
    off, alts, steps = hits.want[max_alt]
    places, goff, galts = rep_ctx.place_hits_alt(hits.off, hits.alns, 6, max_alt)
    same_alts((goff, galts), (off, alts), max_alt)
    assert rep_ctx.place_alt_stats()[:2] == (len(alts), steps)
    assert places.tobytes() == rep_ctx.place_hits(hits.off, hits.alns, 6).tobytes()
    if max_alt == 255:
        assert len(alts) >= 500 and int(np.diff(off).max()) == 255


@pytest.mark.parametrize("order", ["reverse", "seed1", "seed2"])
def test_place_hits_alt_does_not_depend_on_the_order_of_the_gap_runs(rep_ctx, hits, order):
    off, alns = map_model.aln_records(hits.reads, "reverse" if order == "reverse" else random.Random(int(order[4:])))
    assert (alns["gap_run"] != hits.alns["gap_run"]).any(axis=1).sum() >= 30
    _, goff, galts = rep_ctx.place_hits_alt(off, alns, 6, 255)
    same_alts((goff, galts), hits.want[255][:2], order)


def compute_units():
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       check=True, stdout=subprocess.PIPE, text=True, timeout=300)
    return int(r.stdout.split()[-1])


def test_place_hits_alt_strides_over_more_items_than_the_grid_has_octets(rep_ctx, hits):
    """more reads than 2 * 8 * CUs * 32 by tiling the fixture: the counts' scan runs over hundreds of blocks, the binary search over a long
    offset array, and every octet of k_place_alt's grid takes several items"""
    cus = compute_units()
    times = (2 * 8 * cus * 32) // len(hits.reads) + 1
    n = times * len(hits.reads)
    assert n > 2 * 8 * cus * 32
    cnt = np.diff(hits.off)
    toff = np.zeros(n + 1, dtype=np.uint64)
    toff[1:] = np.cumsum(np.tile(cnt, times))
    off, alts, steps = hits.want[5]
    assert len(alts) * times > 2 * 8 * cus * 32  # items as well
    woff = np.zeros(n + 1, dtype=np.uint64)
    woff[1:] = np.cumsum(np.tile(np.diff(off), times))
    places, goff, galts = rep_ctx.place_hits_alt(toff, np.tile(hits.alns, times), 6, 5)
    same_alts((goff, galts), (woff, np.tile(alts, times)), f"{n} reads on {cus} CUs")
    assert rep_ctx.place_alt_stats()[:2] == (len(alts) * times, steps * times)
    assert len(places) == n


@pytest.mark.parametrize("n", [0, 1, 33])
def test_place_hits_alt_on_a_few_reads(rep_ctx, hits, n):
    first = [r for r, e in enumerate(hits.reads) if alt_model.n_items(e, 5)][0]  # (so that one read is a read with items)
    off, alts, _ = hits.want[5]
    places, goff, galts = rep_ctx.place_hits_alt(hits.off[first:first + n + 1], hits.alns, 6, 5)
    lo, hi = int(off[first]), int(off[first + n])
    same_alts((goff, galts), (off[first:first + n + 1] - off[first], alts[lo:hi]), n)
    assert len(places) == n and len(goff) == n + 1 and rep_ctx.place_alt_stats()[0] == hi - lo
    if n:
        assert len(galts) > 0


def test_slot_place_alt_through_all_slots_with_parked_reads(built, golden, oracle, monkeypatch):
    """chunks of 23 reads of rep.fq through the eight slots and round again, every wave parked after 150 loop iterations; slot_place_alt
    before slot_result on even slots and after it on odd ones"""
    monkeypatch.setenv("BWB_SLICE_ITERS", "150")
    flags = ["-n", "3"]
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, "rep.fq")))
    seqs, lens = np.concatenate([seqs, seqs]), np.concatenate([lens, lens])
    idx = oracle.load_index(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    sa = alt_model.rep_sa(golden)
    cuts = list(range(0, len(lens), 23)) + [len(lens)]
    want = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        data, _, _ = oracle.align_encoded(idx, seqs[lo:hi], lens[lo:hi], oracle.params(flags))
        reads = oracle_lib.parse_aln(data)
        want.append((map_model.expected_places(oracle, idx, reads, 6)[0], alt_model.expected_alts(reads, 5, sa), data))
    assert len(want) > bw.MAX_SLOTS
    ctx = sa_context(os.path.join(golden, "rep.fa.bwt"))
    p = bw.params(flags)
    seen = 0

    def collect(j):
        nonlocal seen
        slot = j % bw.MAX_SLOTS
        if slot % 2 == 0:
            places, goff, galts = ctx.slot_place_alt(slot, 6, 5)
            off, alns = ctx.slot_result(slot)
        else:
            off, alns = ctx.slot_result(slot)
            places, goff, galts = ctx.slot_place_alt(slot, 6, 5)
        wp, (woff, walts, steps), wbytes = want[j]
        assert places.tobytes() == wp.tobytes(), j
        same_alts((goff, galts), (woff, walts), j)
        assert ctx.place_alt_stats()[:2] == (len(walts), steps)
        assert bw.aln_bytes(off, alns) == wbytes, j
        again = ctx.slot_place_alt(slot, 6, 5)  # asked again: the same records
        assert again[0].tobytes() == wp.tobytes() and again[2].tobytes() == walts.tobytes()
        assert ctx.slot_place(slot).tobytes() == wp.tobytes()
        fewer = ctx.slot_place_alt(slot, 6, 1)  # another limit: computed anew
        same_alts(fewer[1:], alt_model.expected_alts(oracle_lib.parse_aln(wbytes), 1, sa)[:2], (j, 1))
        seen += 1

    try:
        for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            if j >= bw.MAX_SLOTS:
                collect(j - bw.MAX_SLOTS)
            ctx.slot_upload(j % bw.MAX_SLOTS, p, seqs[lo:hi], lens[lo:hi])
            ctx.slot_submit(j % bw.MAX_SLOTS)
        for j in range(max(0, len(want) - bw.MAX_SLOTS), len(want)):
            collect(j)
        assert seen == len(want)
        assert ctx.stats().n_parked_reads > 0
        assert sum(len(w[1][1]) for w in want) == 2 * 125  # rep.fq twice: 10 + 2 * 45 + 5 * 5 items each time
    finally:
        ctx.close()


def test_place_alt_errors_leave_the_context_usable(built, golden, hits):
    b = bw.BwtFile(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    ctx = bw.Context(b)
    off, alts, _ = hits.want[5]
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, "rep.fq")))
    try:
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        for call in (lambda: ctx.place_hits_alt(hits.off, hits.alns), lambda: ctx.place_alt(), lambda: ctx.slot_place_alt(0)):
            with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
                call()
        ctx.set_sa(b.SA)
        for bad in (0, 256, -1, 1000):
            for call in (lambda: ctx.place_hits_alt(hits.off, hits.alns, 6, bad), lambda: ctx.place_alt(6, bad), lambda: ctx.slot_place_alt(0, 6, bad)):
                with pytest.raises(bw.BwbError, match="error -1.*max_alt"):
                    call()
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            ctx.slot_place_alt(3)
        with pytest.raises(bw.BwbError, match="error -1"):
            ctx.slot_place_alt(bw.MAX_SLOTS)
        rep_items = ctx.place_alt(6, 5)[2]
        assert len(rep_items) == 125
        # an item whose row is not a row of the index: flagged, reported, nothing looked up
        target = [r for r, e in enumerate(hits.reads) if len(e) >= 2 and alt_model.n_items(e, 5)][3]
        k = int(hits.off[target]) + 1
        for row in (b.length, 2**63):
            alns = hits.alns.copy()
            alns["L"][k], alns["U"][k] = row, row
            with pytest.raises(bw.BwbError, match="error -4.*outside the index"):
                ctx.place_hits_alt(hits.off, alns, 6, 5)
            assert len(ctx.place_hits(hits.off, alns, 6)) == len(hits.reads)  # (k_place only looks up the first hit's row)
            same_alts(ctx.place_hits_alt(hits.off, hits.alns, 6, 5)[1:], (off, alts), row)
        bad_off = hits.off.copy()
        bad_off[7], bad_off[8] = bad_off[8] + 1, bad_off[7]
        with pytest.raises(bw.BwbError, match="error -1.*not ascending"):
            ctx.place_hits_alt(bad_off, hits.alns, 6, 5)
        with pytest.raises(ValueError):
            ctx.place_hits_alt(hits.off, hits.alns[:-1], 6, 5)
        same_alts(ctx.place_hits_alt(hits.off, hits.alns, 6, 5)[1:], (off, alts))
        assert ctx.place_alt(6, 5)[2].tobytes() == rep_items.tobytes()  # the slot is untouched by all this
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def mid(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("altmid")
    fa = str(d / "g.fa")
    subprocess.run([bw.SYNTH_BIN, "genome", fa, "3000000", "5", "1200", "77"], check=True)
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    return d, fa


def test_place_alt_on_the_small_superblock_build(mid):
    """the walk across superblock rows and with biased stored positions (the test build): a fresh process bound to libbwbble_hip_test.so"""
    d, fa = mid
    bw.build(testlib=True)
    env = dict(os.environ, BWB_LIB=bw.TEST_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "alt_c3_worker.py"), fa, str(d)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "ALT-C3-OK" in r.stdout, r.stdout[-3000:]


# ---- the command line ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def map_dir(built, golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("altmap")
    for ext in ("", ".bwt", ".ann"):
        shutil.copy(os.path.join(golden, "rep.fa" + ext), d / ("rep.fa" + ext))
    return d


def cli(args, env=None, timeout=600):
    r = subprocess.run([bw.HOST_BIN] + [str(a) for a in args], env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def model_text(golden, oracle, aln_bytes, base_text, max_mm, max_alt):
    idx = oracle.load_index(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(aln_bytes)
    places, _ = map_model.expected_places(oracle, idx, reads, max_mm)
    off, alts, _ = alt_model.expected_alts(reads, max_alt, alt_model.rep_sa(golden))
    return alt_model.expected_sam(base_text, places, off, alts, alt_model.read_ann(os.path.join(golden, "rep.fa.ann")))


VARIANTS = {
    "one_chunk": ([], {}),
    "chunks_of_23": (["-g", "1"], {"BWB_CHUNK": "23"}),
    "two_workers": (["-g", "2"], {"BWB_DEVICE_MAP": "0,0", "BWB_CHUNK": "23", "BWB_POOL_GB": "1"}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cli_map_x5_on_rep(map_dir, golden, oracle, variant):
    """map -n 3 -X 5: columns 1-11 are the golden rep_n3.sam's, the whole file is the model's text, and it is what align + aln2sam -X 5
    write (the invariant that defines map); map without -X still writes the golden file"""
    extra, env = VARIANTS[variant]
    fa, fq = map_dir / "rep.fa", os.path.join(golden, "rep.fq")
    gold = open(os.path.join(golden, "rep_n3.sam")).read()
    out, aln, two, plain = (map_dir / f"{variant}.{x}" for x in ("x5.sam", "aln", "two.sam", "plain.sam"))
    log = cli(["map", "-n", "3", "-X", "5"] + extra + [fa, fq, out], env)
    got = open(out).read()
    body = lambda t: [ln for ln in t.split("\n") if ln and not ln.startswith("@")]
    assert ["\t".join(ln.split("\t")[:11]) for ln in body(got)] == body(gold)
    assert got == model_text(golden, oracle, open(os.path.join(golden, "rep_n3.aln"), "rb").read(), gold, 6, 5)
    assert sum(1 for ln in body(got) if "\tXA:Z:" in ln) == 60
    assert "other placements on the GPU (-X 5): items 125 " in log and ("GPUs: 2" in log) == (variant == "two_workers")
    cli(["align", "-n", "3"] + extra + [fa, fq, aln], env)
    cli(["aln2sam", "-X", "5", fa, fq, aln, two])
    assert open(two).read() == got
    log = cli(["map", "-n", "3"] + extra + [fa, fq, plain], env)
    assert open(plain).read() == gold and "other placements" not in log


@pytest.mark.parametrize("max_alt,max_mm", [(4, 3), (1, 6), (255, 6)])
def test_cli_map_other_limits_and_mapq_option(map_dir, golden, oracle, max_alt, max_mm):
    """-X 4 drops exactly the five reads with six placements; -Q and -X together: map == align + aln2sam -n Q -X N == the model"""
    fa, fq = map_dir / "rep.fa", os.path.join(golden, "rep.fq")
    gold = open(os.path.join(golden, "rep_n3_q3.sam" if max_mm == 3 else "rep_n3.sam")).read()
    out, aln, two = (map_dir / f"n{max_alt}.{x}" for x in ("sam", "aln", "two.sam"))
    cli(["map", "-n", "3", "-Q", max_mm, "-X", max_alt, fa, fq, out])
    got = open(out).read()
    assert got == model_text(golden, oracle, open(os.path.join(golden, "rep_n3.aln"), "rb").read(), gold, max_mm, max_alt)
    assert sum(1 for ln in got.split("\n") if "\tXA:Z:" in ln) == {1: 10, 4: 55, 255: 60}[max_alt]
    cli(["align", "-n", "3", fa, fq, aln])
    cli(["aln2sam", "-n", max_mm, "-X", max_alt, fa, fq, aln, two])
    assert open(two).read() == got


def test_cli_gapped_reads_and_the_made_up_hit_lists(map_dir, golden, oracle, tmp_path):
    """map -X on the gapped reads == the model on the reference's .aln; aln2sam -X 255 on alt_hits.aln (the host's own enumeration of the
    rows, the items through bwb_hip_locate) == the model: an item in no record left out, lists of 255 items"""
    from golden.make_golden_alt import unpack_alt
    fa = map_dir / "rep.fa"
    out, base = tmp_path / "gap.sam", tmp_path / "gap_plain.sam"
    cli(["map", "-n", "4", "-o", "1", "-X", "5", fa, os.path.join(golden, "rep_gap.fq"), out])
    cli(["map", "-n", "4", "-o", "1", fa, os.path.join(golden, "rep_gap.fq"), base])
    got = open(out).read()
    assert got == model_text(golden, oracle, open(os.path.join(golden, "rep_gap_n4.aln"), "rb").read(), open(base).read(), 6, 5)
    assert sum(1 for ln in got.split("\n") if "\tXA:Z:" in ln and ("I" in ln.split("\tXA:Z:")[1] or "D" in ln.split("\tXA:Z:")[1])) >= 10
    fq = unpack_alt(tmp_path, golden)
    aln = os.path.join(golden, "alt_hits.aln")
    for max_alt in (5, 255):
        out, base = tmp_path / f"hits{max_alt}.sam", tmp_path / "hits_plain.sam"
        cli(["aln2sam", "-X", max_alt, fa, fq, aln, out])
        cli(["aln2sam", fa, fq, aln, base])
        assert open(out).read() == model_text(golden, oracle, open(aln, "rb").read(), open(base).read(), 6, max_alt)
