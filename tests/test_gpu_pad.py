"""Bubble hits in reference coordinates on the GPU: kernel k_locus through Context.locus_places on injected placement records and record
tables of every shape of its search, through Context.locus / slot_locus on the pad_bub reads against the Python restatement of the
reference's sam_pad (tests/pad_model.py, pinned to the reference's bytes by tests/test_pad_host.py) fed with the ORACLE's placements -
never the library's own -, the state and argument errors, and the command line against the golden padded SAM and against `bwbble sampad`.

k_locus reads no index memory (placement records, the record table, the bubble table), so the small-superblock test build
(libbwbble_hip_test.so) would run the very same code: no worker for it here."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import bwbble_amd as bw
import map_model
import oracle_lib
import pad_model
from test_gpu_map import cli, compute_units, sa_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_LEN, REC_GAP, REC_BASE = 300, 5, 1000  # the injected tables: records of 300 positions, 5 apart, the first one at 1000


@pytest.fixture(scope="module")
def synth_bubbles(golden):
    return pad_model.load_bubbles(os.path.join(golden, "pad_synth.data"))


@pytest.fixture(scope="module")
def toy_ctx(built, golden):
    ctx = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    yield ctx
    ctx.close()


def table(n_seq, n_bub):
    """n_seq disjoint records in text order; record 2 of every nine is a plain one, the others are bubble records, the bubbles taken in turn"""
    start = REC_BASE + np.arange(n_seq, dtype=np.uint64) * np.uint64(REC_LEN + REC_GAP)
    end = start + np.uint64(REC_LEN - 1)
    i = np.arange(n_seq)
    bub_of = np.where(i % 9 == 2, -1, (i - (i + 6) // 9) % max(n_bub, 1)).astype(np.int32)
    return start, end, bub_of


def boundary_loci(bubbles):
    """every locus at which sam_pad's rule changes its answer for some bubble of the table, as far as a record holds it"""
    loci = {1, 2, REC_LEN - 1, REC_LEN}
    for _, A, B, C, D, ref_len, alt_len in bubbles:
        loci |= {B, B + 1, B + alt_len, B + alt_len + 1, B + alt_len + D + 1, B + alt_len + D + 2}
    return sorted(v for v in loci if 1 <= v <= REC_LEN)


def injected_places(start, end, bubbles, rng):
    """positions at the first and last character of the first, middle and last record, one past the last record, before the first, in a gap
    between two records, and every boundary locus of the bubble rule on a sample of records - each as a mapped and as an unmapped read"""
    n = len(start)
    recs = sorted({0, n // 2, n - 1} | (set(range(n)) if n <= 9 else set(int(v) for v in rng.integers(0, n, 16))))
    pos = [0, REC_BASE - 1, int(end[-1]) + 1, int(end[-1]) + 10**9]
    for i in recs:
        pos += [int(start[i]), int(end[i])]
        if i + 1 < n:
            pos += [int(end[i]) + 1, int(start[i + 1]) - 1]
        pos += [int(start[i]) + v - 1 for v in boundary_loci(bubbles)]
    places = np.zeros(2 * len(pos), dtype=bw.PLACE_DTYPE)
    places["pos"] = np.repeat(np.array(pos, dtype=np.uint64), 2)
    places["flags"] = np.tile(np.array([bw.PLACE_MAPPED, 0], dtype=np.uint8), len(pos))
    places["flags"][::4] |= bw.PLACE_REVERSE
    places["mapq"], places["aln_length"], places["ref_len"] = 37, 100, 100  # (fields k_locus does not read)
    return places


def same_loci(got, want, what=""):
    assert pad_model.first_difference(got, want) is None, (what, pad_model.first_difference(got, want))
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("n_seq", [1, 2, 3, 7, 8, 9, 1_300_000])
def test_locus_places_equals_the_model_on_injected_places(toy_ctx, synth_bubbles, n_seq):
    """record tables around the powers of two of the search's step count and one of the GRCh37 shape, the pad_synth bubble table (alt_len 0,
    ref_len 0 / 1 / 5, B_minus_A 0, D_minus_C -1, A and C above 2^32)"""
    start, end, bub_of = table(n_seq, len(synth_bubbles))
    places = injected_places(start, end, synth_bubbles, np.random.default_rng(n_seq))
    want = pad_model.expected_loci(places, start, end, bub_of, synth_bubbles)
    assert {bw.LOCUS_POINT, bw.LOCUS_RANGE, 0} <= set(want["kind"].tolist()) and (want["seqid"] < 0).sum() > len(want) // 2 - 1
    assert n_seq < 3 or ((want["seqid"] >= 0) & (want["bubble"] < 0)).any()
    toy_ctx.set_loci(start, end, bub_of, pad_model.bubble_records(synth_bubbles))
    same_loci(toy_ctx.locus_places(places), want, n_seq)
    n, ms = toy_ctx.locus_stats()
    assert n == len(places) and ms > 0
    if n_seq == 9:  # every bubble of the table has a record, and every answer of the rule is above 2^32 somewhere
        assert set(want["bubble"].tolist()) == set(range(-1, len(synth_bubbles))) and (want["ref_lo"] > 2**32).any() and (want["ref_hi"] < want["ref_lo"]).any()


def test_locus_places_without_a_bubble_table(toy_ctx):
    """n_bub == 0 with every record a plain one is allowed"""
    start, end, _ = table(5, 0)
    none = np.full(5, -1, dtype=np.int32)
    places = injected_places(start, end, [], np.random.default_rng(5))
    toy_ctx.set_loci(start, end, none, np.zeros(0, dtype=bw.BUBBLE_DTYPE))
    same_loci(toy_ctx.locus_places(places), pad_model.expected_loci(places, start, end, none, []))


@pytest.fixture(scope="module")
def grch37_shape(synth_bubbles):
    """4 099 placement records on the 1.3 M-record table, and what the model makes of them"""
    start, end, bub_of = table(1_300_000, len(synth_bubbles))
    rng = np.random.default_rng(37)
    places = np.zeros(4099, dtype=bw.PLACE_DTYPE)
    places["pos"] = rng.integers(0, int(end[-1]) + 400, len(places)).astype(np.uint64)
    places["flags"] = np.where(rng.integers(0, 8, len(places)) == 0, 0, bw.PLACE_MAPPED).astype(np.uint8)
    want = pad_model.expected_loci(places, start, end, bub_of, synth_bubbles)
    return types.SimpleNamespace(start=start, end=end, bub_of=bub_of, places=places, want=want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_locus_places_on_a_few_reads(toy_ctx, synth_bubbles, grch37_shape, n):
    """less than a wave, exactly one, one more; and none (no launch)"""
    g = grch37_shape
    toy_ctx.set_loci(g.start, g.end, g.bub_of, pad_model.bubble_records(synth_bubbles))
    same_loci(toy_ctx.locus_places(g.places[:n]), g.want[:n], n)
    assert toy_ctx.locus_stats()[0] == n and (toy_ctx.locus_stats()[1] > 0) == (n > 0)


def test_locus_places_strides_over_more_reads_than_the_grid_has_lanes(toy_ctx, synth_bubbles, grch37_shape):
    """the production path of k_locus's loop: more than twice 8 * CUs * 256 reads, so that every lane takes a third read"""
    g = grch37_shape
    cus = compute_units()
    times = max(200_000, 2 * 8 * cus * 256 + 1) // len(g.places) + 1
    n = times * len(g.places)
    assert n > 2 * 8 * cus * 256 and n >= 200_000
    toy_ctx.set_loci(g.start, g.end, g.bub_of, pad_model.bubble_records(synth_bubbles))
    got = toy_ctx.locus_places(np.tile(g.places, times))
    same_loci(got, np.tile(g.want, times), f"{n} reads on {cus} CUs")
    assert toy_ctx.locus_stats()[0] == n


# ---- the pad_bub reads on the toy index -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def toy_tables(golden):
    names, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
    anns, recs = bw.read_bubble_data(os.path.join(golden, "pad_toy.data"))
    bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
    return types.SimpleNamespace(start=start, end=end, bub_of=pad_model.bubble_of(names, bubbles), bubbles=bubbles, recs=recs)


@pytest.fixture(scope="module")
def pad_text(tmp_path_factory):
    return pad_model.unpack(tmp_path_factory.mktemp("padgpu"))


@pytest.fixture(scope="module")
def bub_reads(pad_text):
    return bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))


def oracle_loci(oracle, idx, t, seqs, lens, max_mm):
    """the model fed the oracle's placements -> (places, loci, the oracle's .aln bytes)"""
    data, _, _ = oracle.align_encoded(idx, seqs, lens, oracle.params(["-n", "3"]))
    places, _ = map_model.expected_places(oracle, idx, oracle_lib.parse_aln(data), max_mm)
    return places, pad_model.expected_loci(places, t.start, t.end, t.bub_of, t.bubbles), data


def test_locus_equals_the_model_fed_the_oracles_places(built, golden, oracle, toy_tables, bub_reads):
    seqs, lens = bub_reads
    t = toy_tables
    idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    ctx = sa_context(os.path.join(golden, "toy.fa.bwt"))
    try:
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        for max_mm in (6, 3):
            wp, wl, _ = oracle_loci(oracle, idx, t, seqs, lens, max_mm)
            places, loci = ctx.locus(max_mm)
            assert places.tobytes() == wp.tobytes()
            same_loci(loci, wl, max_mm)
            assert ctx.locus_stats()[0] == len(lens) and ctx.place().tobytes() == wp.tobytes()
        assert (wl["kind"] == bw.LOCUS_RANGE).sum() >= 16 and (wl["kind"] == bw.LOCUS_POINT).sum() >= 300 and (wl["seqid"] < 0).any()
    finally:
        ctx.close()


def test_slot_locus_through_all_slots_with_parked_reads(built, golden, oracle, toy_tables, bub_reads, monkeypatch):
    """chunks of 97 reads through the eight slots and round again, every wave parked after 150 loop iterations; slot_locus before slot_result
    on even slots and after it on odd ones, and once more after slot_place_alt: the same bytes"""
    monkeypatch.setenv("BWB_SLICE_ITERS", "150")
    seqs, lens = bub_reads
    seqs, lens = np.concatenate([seqs, seqs[:330]]), np.concatenate([lens, lens[:330]])
    t = toy_tables
    idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    cuts = list(range(0, len(lens), 97)) + [len(lens)]
    want = [oracle_loci(oracle, idx, t, seqs[lo:hi], lens[lo:hi], 6) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert len(want) > bw.MAX_SLOTS
    ctx = sa_context(os.path.join(golden, "toy.fa.bwt"))
    ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
    p = bw.params(["-n", "3"])
    seen = 0

    def collect(j):
        nonlocal seen
        slot = j % bw.MAX_SLOTS
        wp, wl, wbytes = want[j]
        if slot % 2 == 0:
            places, loci = ctx.slot_locus(slot)
            off, alns = ctx.slot_result(slot)
        else:
            off, alns = ctx.slot_result(slot)
            places, loci = ctx.slot_locus(slot)
        same_loci(loci, wl, j)
        assert places.tobytes() == wp.tobytes() and bw.aln_bytes(off, alns) == wbytes, j
        assert ctx.slot_place_alt(slot, 6, 5)[0].tobytes() == wp.tobytes()
        again = ctx.slot_locus(slot)
        assert again[0].tobytes() == wp.tobytes() and again[1].tobytes() == wl.tobytes(), j
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


def test_locus_errors_leave_the_context_usable(built, golden, oracle, toy_tables, bub_reads):
    seqs, lens = bub_reads[0][:120], bub_reads[1][:120]
    t = toy_tables
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    ctx = bw.Context(b)
    try:
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            ctx.locus()
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            ctx.slot_locus(0)
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            ctx.locus_places(np.zeros(3, dtype=bw.PLACE_DTYPE))
        # an unsorted table, overlapping records, an empty record, bubble numbers outside the table: refused, and still no tables
        for s, e, bo in ((t.start[::-1], t.end[::-1], t.bub_of[::-1]), (t.start, t.end + np.uint64(1), t.bub_of),
                         (t.start, np.where(np.arange(len(t.end)) == 2, t.start - np.uint64(1), t.end), t.bub_of),
                         (t.start, t.end, np.where(t.bub_of == 3, 4, t.bub_of)), (t.start, t.end, np.where(t.bub_of == 3, -2, t.bub_of)),
                         (t.start[:0], t.end[:0], t.bub_of[:0])):
            with pytest.raises(bw.BwbError, match="error -1.*set_loci"):
                ctx.set_loci(s, e, bo, t.recs)
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            ctx.locus()
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
            ctx.locus()
        with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
            ctx.slot_locus(0)
        ctx.set_sa(b.SA)
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            ctx.slot_locus(3)
        for slot in (-1, bw.MAX_SLOTS):
            with pytest.raises(bw.BwbError, match="error -1"):
                ctx.slot_locus(slot)
        idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
        wp, wl, data = oracle_loci(oracle, idx, t, seqs, lens, 6)
        places, loci = ctx.locus()
        assert places.tobytes() == wp.tobytes()
        same_loci(loci, wl)
        assert bw.aln_bytes(*ctx.result()) == data
        # a refused table leaves the resident one in place; a new batch invalidates the slot's records
        with pytest.raises(bw.BwbError, match="error -1.*set_loci"):
            ctx.set_loci(t.start, t.end, np.where(t.bub_of == 0, 9, t.bub_of), t.recs)
        ctx.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            ctx.locus()
        ctx.run()
        same_loci(ctx.locus()[1], wl[:10])
        same_loci(ctx.locus_places(wp), wl)
    finally:
        ctx.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def map_dir(built, golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("mappad")
    for ext in ("", ".bwt", ".ann"):
        shutil.copy(os.path.join(golden, "toy.fa" + ext), d / ("toy.fa" + ext))
    return d


VARIANTS = {
    "one_chunk": ([], {}),
    "chunks_of_97": ([], {"BWB_CHUNK": "97"}),
    "two_workers": (["-g", "2"], {"BWB_DEVICE_MAP": "0,0", "BWB_CHUNK": "97", "BWB_POOL_GB": "1"}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cli_map_with_the_bubble_table_writes_the_references_padded_sam(map_dir, golden, pad_text, variant):
    extra, env = VARIANTS[variant]
    out = map_dir / f"pad_{variant}.sam"
    log = cli(["map", "-n", "3", "-B", os.path.join(golden, "pad_toy.data")] + extra + [map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out], env)
    assert open(out, "rb").read() == open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read()
    assert "loci resolved 571  k_locus" in log and ("GPUs: 2" in log) == (variant == "two_workers")


def test_cli_align_then_aln2sam_with_the_bubble_table(map_dir, golden, pad_text, tmp_path):
    fa, fq, aln, out = map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "t.aln", tmp_path / "t.sam"
    cli(["align", "-n", "3", fa, fq, aln])
    cli(["aln2sam", "-B", os.path.join(golden, "pad_toy.data"), fa, fq, aln, out])
    assert open(out, "rb").read() == open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read()


@pytest.mark.parametrize("flags", [["-n", "3", "-X", "5"], ["-S"]], ids=["n3_x5", "single_genome"])
def test_cli_map_with_the_bubble_table_equals_sampad_of_map(map_dir, golden, pad_text, tmp_path, flags):
    """the tags come last, behind XA; and on the single-genome alphabet"""
    fa, fq, data = map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    one, plain, two = tmp_path / "b.sam", tmp_path / "plain.sam", tmp_path / "padded.sam"
    cli(["map"] + flags + ["-B", data, fa, fq, one])
    cli(["map"] + flags + [fa, fq, plain])
    cli(["sampad", data, plain, two])
    got = open(one, "rb").read()
    assert got == open(two, "rb").read() and got != open(plain, "rb").read() and b"\tbP:Z:" in got
    if "-X" in flags:
        assert any(b"\tXA:Z:" in ln and ln.index(b"\tXA:Z:") < ln.index(b"\tbC:Z:") for ln in got.split(b"\n") if b"\tbC:Z:" in ln)
