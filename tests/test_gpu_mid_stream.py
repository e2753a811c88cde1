"""`bwbble map` with -J, -R, -D, -A and -I together on the mid-size fixture of tests/mid_model.py (3 302 441 characters of text on 5 chromosomes,
1 200 bubbles, 9 600 searched reads), held to the bytes of the CPU-only chain that tests/test_mid_host.py judges: one chunk, chunks of 997 reads,
four workers, and the counters read back in pieces of 1 000 (BWB_COUNT_PIECE); the -I table without -R and the -A table of a plain run; the site
index (`k_site_count` / `k_scan_sums` / `k_site_add`) at every position of the real text - 404 blocks, two turns of the carry loop - on the
product and, uploaded in 101 chunks, on the test build (tests/mid_sites_worker.py), and of a constructed text whose block sums of 8 192 lie on
both sides of the carry loop's turn, with reads piled on it; and the toy's `map -A -I` with the counters read back seven at a time."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bwbble_amd as bw
import lift_model
import mid_model
import pad_model
import pile_model
from test_gpu_map import cli
from test_gpu_md import md_dir  # noqa: F401 (fixture)
from test_gpu_join import pad_text  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ["-X", "5", "-J", "-R", "-D"]


@pytest.fixture(scope="module")
def mid(built, oracle, tmp_path_factory):
    return mid_model.build(tmp_path_factory.mktemp("mid_stream"), oracle)


VARIANTS = {
    "one_chunk": ([], {}),
    "chunks_of_997": ([], {"BWB_CHUNK": "997"}),
    "four_workers": (["-g", "4"], {"BWB_DEVICE_MAP": "0,0,0,0", "BWB_CHUNK": "997", "BWB_POOL_GB": "1"}),
    "count_piece_1000": ([], {"BWB_COUNT_PIECE": "1000", "BWB_DEBUG": "1"}),  # 1 200 bubbles in two pieces, the text's sites in some forty
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_map_writes_the_chains_bytes(mid, variant):
    """map -n 3 -o 1 -X 5 -B t -J -R -D -A a -a 1 -I i -w 5: the SAM, the counts and the table of the CPU chain, and the models' figures in the log"""
    extra, env = VARIANTS[variant]
    j = mid_model.judged(mid)
    out, a, i = (os.path.join(mid.dir, f"{variant}.{e}") for e in ("sam", "a.tsv", "i.tsv"))
    log = cli(["map"] + mid_model.ALIGN + ["-B", mid.data] + ALL + ["-A", a, "-a", mid_model.MIN_MAPQ, "-I", i, "-w", mid_model.ANCHOR] + extra + [mid.fa, mid.fq, out], env)
    got = open(out, "rb").read()
    assert got == mid.full, pad_model.first_difference(got, mid.full)
    assert open(a, "rb").read() == mid.a_tsv and open(i, "rb").read() == mid.i_tsv
    n_sites = mid_model.site_numbers(bw.read_ref(mid.fa))[1]
    assert f"placements lifted to chromosome coordinates on the GPU: lifted {j.n_lifted}  not liftable 0 " in log
    assert f"allele counts at the text's IUPAC sites on the GPU: sites {n_sites}  reads counted {j.pile_reads}  adds {j.pile_adds} " in log
    assert f"read support per indel bubble on the GPU: anchor 5  eligible bubbles {j.eligible}  refused and skipped 0  reads counted {j.indel_reads}  adds {j.indel_adds} " in log
    assert ("GPUs: 4" in log) == (variant == "four_workers")
    if variant == "count_piece_1000":
        assert f"the counters of {n_sites} sites read back in {(n_sites + 999) // 1000} pieces" in log and n_sites > 30_000
        assert "the counters of 1200 bubbles read back in 2 pieces" in log


def test_indel_table_without_lift_and_counts_of_a_plain_run(mid):
    """-I needs no -R: the same table; and `map -n 3 -o 1 -A a` with no other flag counts what pile_model counts on that run's own SAM text"""
    out, a, i = (os.path.join(mid.dir, f"plain.{e}") for e in ("sam", "a.tsv", "i.tsv"))
    cli(["map"] + mid_model.ALIGN + ["-B", mid.data, "-X", "5", "-J", "-I", i, "-a", mid_model.MIN_MAPQ, "-w", mid_model.ANCHOR, mid.fa, mid.fq, out])
    assert open(i, "rb").read() == mid.i_tsv and open(out, "rb").read() == mid.base
    log = cli(["map"] + mid_model.ALIGN + ["-A", a, mid.fa, mid.fq, out])
    table, reads, adds = pile_model.pile_sam(open(out, "rb").read(), mid.text, mid.names, mid.starts)
    assert open(a, "rb").read() == pile_model.tsv(mid.text, mid.names, mid.starts, table)
    assert f"reads counted {reads}  adds {adds} " in log and reads > 9000 and len(table) > 5000


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_site_index_of_the_real_text(mid, golden, lib):
    """3 302 441 positions, 404 blocks: the carry loop of k_scan_sums takes its second turn; on the test build the text arrives in 101 chunks"""
    codes = bw.read_ref(mid.fa)
    assert len(codes) == 3_302_441 and (len(codes) + 8191) // 8192 == 404
    if lib == "product":
        ctx = bw.Context(os.path.join(golden, "toy.fa.bwt"))
        try:
            assert mid_model.check_site_index(ctx, codes) > 30_000
        finally:
            ctx.close()
        return
    bw.build(testlib=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mid_sites_worker.py"), mid.fa, "101"], env=dict(os.environ, BWB_LIB=bw.TEST_LIB_PATH),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "MID-SITES-OK" in r.stdout and "libbwbble_hip_test.so" in r.stdout, r.stdout[-3000:]


def test_site_index_with_a_carry_that_matters(built, golden):
    """block sums of 8 192 on both sides of the turn of k_scan_sums' carry loop, a block without a site, 258 blocks: the index at every position,
    then 2 000 reads of 40 bases - a good part of them around the turn, one on the text's last characters - piled against the model"""
    codes = mid_model.carry_text()
    turn = 65536 * 32
    want, n_sites = mid_model.site_numbers(codes)
    sums = np.add.reduceat(np.isin(codes, mid_model.SITE_CODES).astype(np.int64), np.arange(0, len(codes), 8192))
    assert len(sums) == 258 and sums[255] == sums[256] == 8192 and (sums == 0).any() and len(codes) % 32 == 5
    text = np.frombuffer(pile_model.NT16.encode(), dtype=np.uint8)[codes].tobytes().decode()
    rng = np.random.default_rng(5)
    where = np.concatenate([rng.integers(0, len(codes) - 40, 1200), rng.integers(turn - 9000, turn + 9000, 797), [0, turn - 20, len(codes) - 40]])
    places = lift_model.place_records([(int(p), bool(k & 1), "40M") for k, p in enumerate(where)])
    seqs, lens = rng.integers(0, 5, (len(where), 40)).astype(np.uint8), np.full(len(where), 40, dtype=np.uint16)
    ctx = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    try:
        assert mid_model.check_site_index(ctx, codes) == n_sites
        counts, reads, adds = pile_model.expected_counts(text, seqs, lens, places)
        ctx.pile_records(seqs, lens, places)
        got = ctx.pile_counts(0, n_sites)
        assert np.array_equal(got, counts), np.flatnonzero((got != counts).any(axis=1))[:5]
        assert ctx.pile_stats()[:2] == (reads, adds) and reads == 2000
        k = int(want[turn])
        assert counts[k - 8192:k].any() and counts[k:k + 8192].any() and counts[-5:].any()  # either side of the turn, and the last word's sites
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", ["one_worker", "four_workers", "piece_below_1"])
def test_toy_counters_read_back_seven_at_a_time(md_dir, golden, pad_text, variant):
    """BWB_COUNT_PIECE=7 on the toy (2 454 sites: 351 read-backs per worker; below 1 it is 1: 4 read-backs of a bubble each): the bytes of the run without the knob"""
    extra, env = {"one_worker": ([], {}), "four_workers": (["-g", "4"], {"BWB_DEVICE_MAP": "0,0,0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}), "piece_below_1": ([], {})}[variant]
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    cmd = lambda tag: ["map", "-n", "3", "-X", "5", "-B", data, "-J", "-R", "-A", md_dir / f"{variant}.{tag}.a.tsv", "-I", md_dir / f"{variant}.{tag}.i.tsv", "-w", "5"] + extra + [md_dir / "toy.fa", fq, md_dir / f"{variant}.{tag}.sam"]
    cli(cmd("whole"), env)
    log = cli(cmd("pieces"), dict(env, BWB_COUNT_PIECE="0" if variant == "piece_below_1" else "7", BWB_DEBUG="1"))
    sites, bubs = (2454, 4) if variant == "piece_below_1" else (351, 1)
    workers = 4 if variant == "four_workers" else 1
    assert log.count(f"the counters of 2454 sites read back in {sites} pieces") == log.count(f"the counters of 4 bubbles read back in {bubs} pieces") == workers
    for e in ("sam", "a.tsv", "i.tsv"):
        whole, pieces = open(md_dir / f"{variant}.whole.{e}", "rb").read(), open(md_dir / f"{variant}.pieces.{e}", "rb").read()
        assert whole == pieces and whole.count(b"\n") > 1, e
