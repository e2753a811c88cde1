"""`bwbble map` on the GPU: kernel k_place through Context.place / slot_place against the Python restatement of eval_aln
(tests/map_model.py) fed with the ORACLE's hits - never the library's own slot_result -, the streaming interface with parked and resumed
reads, the state errors, the command line against the reference's golden .sam files and against this build's align + aln2sam, and the
walk on the small-superblock test build."""
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
