"""`bwbble map` on the GPU: kernel k_place through Context.place / slot_place against the Python restatement of eval_aln
(tests/map_model.py) fed with the ORACLE's hits - never the library's own slot_result -, the streaming interface with parked and resumed
reads, the state errors, the command line against the reference's golden .sam files and against this build's align + aln2sam, and the
walk on the small-superblock test build.  And k_place on hit lists the search would never hand it (Context.place_hits on the synth_hits
fixture, whose judge is the reference's aln2sam): eight gap runs in every order, sums that wrap, special first rows, 200 000 reads."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bwbble_amd as bw
import map_model
import oracle_lib
from golden.make_golden import ALIGN_CONFIGS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLACE_CONFIGS = {
    "toy_n3": ("toy.fa", "toy.fq", ["-n", "3"]),
    "toy_n4gap": ("toy.fa", "toy.fq", ALIGN_CONFIGS["n4gap"]),
    "ragged_n5": ("toy.fa", "ragged.fq", ALIGN_CONFIGS["n5"]),
    "toy_s2": ("toy.fa", "toy.fq", ["-S", "-n", "2"]),
    "rep_n3": ("rep.fa", "rep.fq", ["-n", "3"]),
}


def sa_context(bwt_path):
    b = bw.BwtFile(bwt_path, load_sa=True)
    ctx = bw.Context(b)
    ctx.set_sa(b.SA)
    return ctx


def oracle_places(oracle, idx, flags, seqs, lens, max_mm):
    data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(flags))
    return map_model.expected_places(oracle, idx, oracle_lib.parse_aln(data), max_mm), data


@pytest.mark.parametrize("name", list(PLACE_CONFIGS))
def test_place_equals_eval_aln_of_the_oracles_hits(built, golden, oracle, name):
    fa, fq, flags = PLACE_CONFIGS[name]
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, fq)))
    idx = oracle.load_index(os.path.join(golden, fa + ".bwt"), load_sa=True)
    ctx = sa_context(os.path.join(golden, fa + ".bwt"))
    try:
        ctx.align(bw.params(flags), seqs, lens)
        for max_mm in (6, 3):
            (want, steps), _ = oracle_places(oracle, idx, flags, seqs, lens, max_mm)
            got = ctx.place(max_mm)
            assert map_model.first_difference(got, want) is None, (max_mm, map_model.first_difference(got, want))
            assert got.tobytes() == want.tobytes()
            n, st, ms = ctx.place_stats()
            assert (n, st) == (len(lens), steps) and ms > 0
        if name == "rep_n3":  # the sums the toy genome never needs
            assert (want["top1"] > 1).any() and (want["top2"] > 1).any() and len(set(want["mapq"])) >= 6
        if "gap" in name:
            assert (want["num_gapo"] > 0).any() and (want["ref_len"] != want["aln_length"]).any()
    finally:
        ctx.close()


def test_slot_place_through_all_slots_with_parked_reads(built, golden, oracle, monkeypatch):
    """chunks of 97 reads through the eight slots and round again, every wave parked after 150 loop iterations; slot_place before
    slot_result on even slots and after it on odd ones: the records are the one-batch records, slot_result's bytes the oracle's"""
    monkeypatch.setenv("BWB_SLICE_ITERS", "150")
    flags = ["-n", "3"]
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, "toy.fq")))
    seqs, lens = np.concatenate([seqs, seqs[:300]]), np.concatenate([lens, lens[:300]])
    idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    cuts = list(range(0, len(lens), 97)) + [len(lens)]
    want = [oracle_places(oracle, idx, flags, seqs[lo:hi], lens[lo:hi], 6) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert len(want) > bw.MAX_SLOTS
    ctx = sa_context(os.path.join(golden, "toy.fa.bwt"))
    p = bw.params(flags)
    seen = 0

    def collect(j):
        nonlocal seen
        slot = j % bw.MAX_SLOTS
        if slot % 2 == 0:
            places = ctx.slot_place(slot)
            off, alns = ctx.slot_result(slot)
        else:
            off, alns = ctx.slot_result(slot)
            places = ctx.slot_place(slot)
        (wp, _), wbytes = want[j]
        assert map_model.first_difference(places, wp) is None, (j, map_model.first_difference(places, wp))
        assert bw.aln_bytes(off, alns) == wbytes, j
        assert ctx.slot_place(slot).tobytes() == wp.tobytes()  # asked again: the same records
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
    finally:
        ctx.close()


def test_place_state_errors_leave_the_context_usable(built, golden, oracle):
    fa = os.path.join(golden, "rep.fa.bwt")
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, "rep.fq")))
    b = bw.BwtFile(fa, load_sa=True)
    ctx = bw.Context(b)
    try:
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        with pytest.raises(bw.BwbError, match="set_sa"):
            ctx.place()
        with pytest.raises(bw.BwbError, match="set_sa"):
            ctx.slot_place(0)
        ctx.set_sa(b.SA)
        with pytest.raises(bw.BwbError, match="not been submitted"):
            ctx.slot_place(3)
        with pytest.raises(bw.BwbError):
            ctx.slot_place(bw.MAX_SLOTS)
        with pytest.raises(bw.BwbError):
            ctx.slot_place(-1)
        idx = oracle.load_index(fa, load_sa=True)
        (want, _), data = oracle_places(oracle, idx, ["-n", "3"], seqs, lens, 6)
        assert ctx.place().tobytes() == want.tobytes()
        assert bw.aln_bytes(*ctx.result()) == data
        # a new batch invalidates the slot's records: place before run is a state error again
        ctx.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            ctx.place()
        ctx.run()
        assert ctx.place().tobytes() == want[:10].tobytes()
    finally:
        ctx.close()


# ---- k_place on injected hit lists (tests/golden/synth_hits.*, made by tests/golden/make_golden_map.py with the reference as judge) ----------

@pytest.fixture(scope="module")
def synth(golden, oracle):
    """the fixture's hit lists as bwb_aln records, and what eval_aln makes of them under aln2sam's -n 6 and -n 3 (records, invPsi steps)"""
    import types
    idx = oracle.load_index(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(golden, "synth_hits.aln"), "rb").read())
    off, alns = map_model.aln_records(reads)
    return types.SimpleNamespace(reads=reads, off=off, alns=alns, want={mm: map_model.expected_places(oracle, idx, reads, mm) for mm in (6, 3)})


@pytest.fixture(scope="module")
def synth_text(tmp_path_factory):
    """the fixture's text files (committed gzipped) as plain files: synth_hits.fq, synth_hits_n6.sam, synth_hits_n3.sam"""
    from golden.make_golden_map import unpack_synth
    return unpack_synth(tmp_path_factory.mktemp("synth"))


@pytest.fixture()
def rep_ctx(built, golden):
    ctx = sa_context(os.path.join(golden, "rep.fa.bwt"))
    yield ctx
    ctx.close()


def same_places(got, want, what=""):
    assert map_model.first_difference(got, want) is None, (what, map_model.first_difference(got, want))
    assert got.tobytes() == want.tobytes(), what


def tiled(off, alns, times):
    """the hit lists `times` times over"""
    cnt = np.diff(off)
    toff = np.zeros(len(cnt) * times + 1, dtype=np.uint64)
    toff[1:] = np.cumsum(np.tile(cnt, times))
    return toff, np.tile(alns, times)


def compute_units():
    """the device's CU count, asked in a child process (k_place's grid is min(ceil(n / 32), 8 * CUs) blocks)"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       check=True, stdout=subprocess.PIPE, text=True, timeout=300)
    return int(r.stdout.split()[-1])


@pytest.mark.parametrize("max_mm", [6, 3])
def test_place_hits_equals_the_model_and_the_references_sam(rep_ctx, golden, synth, synth_text, tmp_path, max_mm):
    """k_place on the synthetic hit lists == the model's records and step count; and the kernel's records through the formatter == the
    SAM the REFERENCE wrote for these hit lists (no model in that loop)"""
    want, steps = synth.want[max_mm]
    got = rep_ctx.place_hits(synth.off, synth.alns, max_mm)
    same_places(got, want)
    n, st, ms = rep_ctx.place_stats()
    assert (n, st) == (len(synth.reads), steps) and ms > 0
    pf, out = tmp_path / "places.bin", tmp_path / "out.sam"
    got.tofile(pf)
    subprocess.run([bw.HOST_BIN, "places2sam", os.path.join(golden, "rep.fa"), os.path.join(synth_text, "synth_hits.fq"), str(pf), str(out)], check=True, stdout=subprocess.DEVNULL)
    assert open(out, "rb").read() == open(os.path.join(synth_text, f"synth_hits_n{max_mm}.sam"), "rb").read()


@pytest.mark.parametrize("order", ["reverse", "seed1", "seed2", "seed3"])
def test_place_hits_does_not_depend_on_the_order_of_the_gap_runs(rep_ctx, synth, order):
    """every hit's runs reversed / shuffled inside gap_run[]: the sorting network gets its eight live inputs in other orders, the insertion
    map is built from disjoint runs - the records are the same"""
    import random
    off, alns = map_model.aln_records(synth.reads, "reverse" if order == "reverse" else random.Random(int(order[4:])))
    changed = (alns["gap_run"] != synth.alns["gap_run"]).any(axis=1)
    first = np.zeros(len(alns), dtype=bool)
    first[off[:-1][np.diff(off) > 0].astype(np.int64)] = True
    assert (changed & first).sum() >= 30  # first hits are the ones k_place sorts
    same_places(rep_ctx.place_hits(off, alns, 6), synth.want[6][0], order)


def test_place_hits_strides_over_more_reads_than_the_grid_has_octets(rep_ctx, synth):
    """the production path of k_place's loop: more than twice 8 * CUs * 32 reads, so that every octet takes a third read"""
    cus = compute_units()
    times = max(200_000, 2 * 8 * cus * 32 + 1) // len(synth.reads) + 1
    n = times * len(synth.reads)
    assert n > 2 * 8 * cus * 32 and n >= 200_000
    off, alns = tiled(synth.off, synth.alns, times)
    want, steps = synth.want[6]
    got = rep_ctx.place_hits(off, alns, 6)
    same_places(got, np.tile(want, times), f"{n} reads on {cus} CUs")
    assert rep_ctx.place_stats()[:2] == (n, steps * times)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33])
def test_place_hits_on_a_few_reads(rep_ctx, synth, n):
    """less than a block, exactly one, one more; and none (no launch)"""
    mapped = [r for r, e in enumerate(synth.reads) if e]
    first = mapped[0]  # (so that one read is a read with hits)
    want, _ = synth.want[6]
    got = rep_ctx.place_hits(synth.off[first:first + n + 1], synth.alns, 6)
    same_places(got, want[first:first + n], n)
    assert len(got) == n and rep_ctx.place_stats()[0] == n
    if n:
        assert got["flags"][0] & bw.PLACE_MAPPED


def test_place_hits_errors_leave_the_context_usable(built, golden, synth):
    """hits the kernel must not follow (a first row outside the index) come back as a state error, a hit list that does not ascend is refused
    on the host; after each the context places the fixture"""
    b = bw.BwtFile(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    ctx = bw.Context(b)
    want, _ = synth.want[6]
    try:
        with pytest.raises(bw.BwbError, match="set_sa"):
            ctx.place_hits(synth.off, synth.alns)
        ctx.set_sa(b.SA)
        target = int(synth.off[[r for r, e in enumerate(synth.reads) if e][5]])
        for row in (b.length, 2**63):
            alns = synth.alns.copy()
            alns["L"][target], alns["U"][target] = row, row
            with pytest.raises(bw.BwbError, match="error -4.*outside the hit log or the index"):
                ctx.place_hits(synth.off, alns)
            same_places(ctx.place_hits(synth.off, synth.alns), want, row)
        off = synth.off.copy()
        off[7], off[8] = off[8] + 1, off[7]
        assert (np.diff(off.astype(np.int64)) < 0).any()
        with pytest.raises(bw.BwbError, match="error -1.*not ascending"):
            ctx.place_hits(off, synth.alns)
        with pytest.raises(ValueError):
            ctx.place_hits(synth.off, synth.alns[:-1])
        same_places(ctx.place_hits(synth.off, synth.alns), want)
        # and the slot interface is untouched by all this
        seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(golden, "rep.fq")))
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        a = ctx.place().tobytes()
        ctx.place_hits(synth.off, synth.alns, 3)
        assert ctx.place().tobytes() == a and ctx.place_stats()[0] == len(synth.reads)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def map_dir(built, golden, tmp_path_factory):
    """the two golden indexes in a directory of the test's own (`-P` writes <fasta>.pre next to the index)"""
    d = tmp_path_factory.mktemp("map")
    for fa in ("toy.fa", "rep.fa"):
        for ext in ("", ".bwt", ".ann"):
            shutil.copy(os.path.join(golden, fa + ext), d / (fa + ext))
    return d


def cli(args, env=None, timeout=600):
    r = subprocess.run([bw.HOST_BIN] + [str(a) for a in args], env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


# golden .sam: (index, reads, the options its .aln was made with + map's -Q)
SAM_CASES = {
    "toy_n3": ("toy.fa", "toy.fq", ["-n", "3"]),
    "ragged_n4gap": ("toy.fa", "ragged.fq", ALIGN_CONFIGS["n4gap"]),
    "wgsim100_n2": ("toy.fa", "wgsim100.fq", ["-n", "2"]),
    "sim_chr21_N100_n2": ("toy.fa", "sim_chr21_N100.fastq", ["-n", "2"]),
    "rep_n3": ("rep.fa", "rep.fq", ["-n", "3"]),
    "rep_n3_q3": ("rep.fa", "rep.fq", ["-n", "3", "-Q", "3"]),
}
VARIANTS = {
    "one_chunk": ([], {}),
    "chunks_of_97": ([], {"BWB_CHUNK": "97"}),
    "two_workers": (["-g", "2"], {"BWB_DEVICE_MAP": "0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SAM_CASES))
def test_cli_map_writes_the_reference_sam(map_dir, golden, name, variant):
    fa, fq, flags = SAM_CASES[name]
    extra, env = VARIANTS[variant]
    out = map_dir / f"{name}_{variant}.sam"
    log = cli(["map"] + flags + extra + [map_dir / fa, os.path.join(golden, fq), out], env)
    assert open(out, "rb").read() == open(os.path.join(golden, name + ".sam"), "rb").read()
    assert "placements on the GPU" in log and ("GPUs: 2" in log) == (variant == "two_workers")
    assert not [f for f in os.listdir(map_dir) if f.endswith(".aln")]  # one process, no .aln on disk


@pytest.mark.parametrize("name,fq,flags,env", [("n0", "toy.fq", ["-n", "0"], {}), ("p2", "ragged.fq", ["-P", "-n", "2"], {"BWB_CHUNK": "97"}),
                                               ("short", "short.fq", ["-n", "3", "-k", "1"], {"BWB_CHUNK": "7"})])
def test_cli_map_equals_align_then_aln2sam(map_dir, golden, tmp_path, name, fq, flags, env):
    """the contract: map OPTS = align OPTS + aln2sam of this build (-n 0: the CLI default; -P; reads not longer than the seed at chunk heads)"""
    fa, fqp = map_dir / "toy.fa", os.path.join(golden, fq)
    one, aln, two = tmp_path / "map.sam", tmp_path / "t.aln", tmp_path / "two.sam"
    cli(["map"] + flags + [fa, fqp, one], env)
    cli(["align"] + flags + [fa, fqp, aln], env)
    cli(["aln2sam", fa, fqp, aln, two])
    assert open(one, "rb").read() == open(two, "rb").read()
    assert os.path.getsize(one) > 1000


@pytest.mark.parametrize("max_mm", [6, 3])
def test_cli_aln2sam_of_the_synthetic_hits_writes_the_reference_sam(map_dir, golden, synth_text, max_mm):
    """the host's own eval_aln (place_from_alns) and the .aln loader on paths of eight runs and sums that wrap"""
    out = map_dir / f"synth_aln2sam_{max_mm}.sam"
    cli(["aln2sam"] + (["-n", "3"] if max_mm == 3 else []) + [map_dir / "rep.fa", os.path.join(synth_text, "synth_hits.fq"), os.path.join(golden, "synth_hits.aln"), out])
    assert open(out, "rb").read() == open(os.path.join(synth_text, f"synth_hits_n{max_mm}.sam"), "rb").read()


@pytest.fixture(scope="module")
def mid(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("mapmid")
    fa = str(d / "g.fa")
    subprocess.run([bw.SYNTH_BIN, "genome", fa, "3000000", "5", "1200", "77"], check=True)
    subprocess.run([bw.HOST_BIN, "index", fa], check=True, stdout=subprocess.DEVNULL)
    return d, fa


@pytest.mark.parametrize("extra_env", [{"BWB_FORCE_POS64": "1"}, {}])
def test_place_on_the_small_superblock_build(mid, extra_env):
    """the walk across superblock rows and with biased stored positions (the test build, as tests/test_gpu_c3_paths.py), for both position
    widths of the search kernels: a fresh process bound to libbwbble_hip_test.so"""
    d, fa = mid
    bw.build(testlib=True)
    env = dict(os.environ, BWB_LIB=bw.TEST_LIB_PATH, **extra_env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "map_c3_worker.py"), fa, str(d)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "MAP-C3-OK" in r.stdout, r.stdout[-3000:]
