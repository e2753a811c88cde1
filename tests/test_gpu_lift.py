"""Placements on bubble records in chromosome coordinates (`bwbble map -B table -R`, kernels k_lift_count / k_lift) on the GPU, judged by
tests/lift_model.py: Context.lift_records on injected records - record tables of every shape of the search, the pad_synth bubbles and the
generator's, every position at which a zone begins or ends, CIGARs with up to eight gap runs, both strands, reads with 0 .. 255 items -; the
pad_bub reads in one batch and streamed through the slots (tests/lift_slots_worker.py); the state and argument errors; the command line
against the model's text; and a generated multi-genome, indexed and mapped, whose lifted lines the records' cmap judges."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import bwbble_amd as bw
import lift_model
import pad_model
from test_gpu_join import VARIANTS, map_dir, model, pad_text, table, toy_tables  # noqa: F401 (fixtures)
from test_gpu_map import cli, compute_units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = (b"chrFar", 100, 10, 110 + (1 << 28) - 1, 10, 0, 0)  # the longest gap the rule takes: a D that no neighbour is merged into


@pytest.fixture(scope="module")
def bubbles(golden):
    return pad_model.load_bubbles(os.path.join(golden, "pad_synth.data")) + lift_model.genome()["bubbles"] + [FAR]


@pytest.fixture(scope="module")
def toy_ctx(built, golden):
    ctx = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    yield ctx
    ctx.close()


def gapped(rng, runs, total):
    """a CIGAR of `runs` gap runs (I and D, now and then one behind the other) in about `total` positions"""
    ops, left = [], total
    for k in range(runs):
        m = int(rng.integers(1, max(2, left // (2 * (runs - k)))))
        ops.append(f"{m}M")
        kind = "ID"[int(rng.integers(0, 2))]
        ops.append(f"{int(rng.integers(1, 4))}{kind}")
        if k + 1 < runs and rng.integers(0, 4) == 0:
            continue  # the next run follows without an M between them
        left -= m + 3
    if ops[-1][-1] in "ID":
        ops.append(f"{int(rng.integers(1, 9))}M")
    merged = []  # (two runs of one kind would print as one)
    for n, op in lift_model.parse_cigar("".join(ops)):
        if merged and merged[-1][1] == op:
            merged[-1] = (merged[-1][0] + n, op)
        else:
            merged.append((n, op))
    return lift_model.cigar_text(merged)


def relative_placements(bubbles, seed=3):
    """[(bubble, pos1, reverse, CIGAR)]: per bubble the printed positions at which a zone begins or ends, with plain and gapped CIGARs, and
    the placements the rule treats specially"""
    rng = np.random.default_rng(seed)
    out = []
    for b, (_, A, Bm, C, Dm, _, alt) in enumerate(bubbles):
        reclen = Bm + alt + Dm + 1
        plain = ["1M", "100M", "60M"] + [gapped(rng, k, 90) for k in range(1, 9)]
        # (0 is the text position before the record's first: it lies in the space between two records of the injected tables, so k_locus gives
        # the placement no record and the kernels must leave it alone - a printed position below 1 cannot reach lift_walk on a bubble)
        for pos1 in sorted({0, 1, 2, Bm, Bm + 1, Bm + alt, Bm + alt + 1, reclen, reclen + 1} | {v for v in (reclen - 99, reclen - 59, Bm - 50, Bm - 98, Bm + alt - 30) if v >= 1}):
            for cig in ["1M", "100M"] + [plain[int(i)] for i in rng.integers(2, len(plain), 4)]:
                out.append((b, pos1, bool(rng.integers(0, 2)), cig))
        a = min(5, Bm)
        lead = f"{a}M" if a else ""
        special = [(Bm - a + 1, f"{lead}2I6M"), (Bm - a + 1, f"{lead}2I1D6M")]                  # an I run that ends at the allele's edge
        if 0 < alt < 128:
            special += [(Bm - a + 1, f"{lead}{alt}D7M"), (Bm + 1, f"{alt}M"), (Bm + 1, "1M")]  # a D run over the whole allele; a span inside it only
        for k in (1, 7, 100):
            special += [(reclen - k + 2, f"{k}M"), (reclen - k + 1, f"{k}M")]                   # leaves the record by one; ends on its last character
        for pos1, cig in special:
            if pos1 >= 1:  # (an offset that would lie before the record)
                out += [(b, pos1, False, cig), (b, pos1, True, cig)]
    return out


def injected(t, rel, n_reads, seed):
    """the relative placements put on records of table t - the first and the last record of every bubble - and dealt out as n_reads primaries
    and their items: reads with 0 .. 12 items, one with 255; a few unmapped, a few in the space between two records"""
    rng = np.random.default_rng(seed)
    recs = {}
    for i in np.flatnonzero(t.bub_of >= 0)[:40].tolist() + np.flatnonzero(t.bub_of >= 0)[-40:].tolist():
        recs.setdefault(int(t.bub_of[i]), []).append(i)
    placed = []
    for b, pos1, rev, cig in rel:
        for i in sorted(set(recs.get(b, [])[:1] + recs.get(b, [])[-1:])):
            placed.append((int(t.start[i]) + pos1 - 1, rev, cig))
    chrom_recs = np.flatnonzero(t.bub_of < 0)
    placed += [(int(t.start[i]) + 10, False, "100M") for i in chrom_recs[:3]] + [(int(t.start[0]) - 1, False, "100M"), (int(t.end[-1]) + 1, True, "50M1I49M")]
    order = rng.permutation(len(placed))
    placed = [placed[i] for i in order]
    n_reads = min(n_reads, max(1, len(placed) // 4))
    places = lift_model.place_records(placed[:n_reads])
    places["flags"][rng.integers(0, n_reads, max(1, n_reads // 50))] = 0
    rest = placed[n_reads:]
    cnt = rng.choice([0, 0, 0, 1, 1, 2, 3, 12], n_reads)
    if n_reads > 8 and len(rest) >= 255:
        cnt[7] = 255
    for r in range(n_reads - 1, -1, -1):  # (no more items than there are placements left: the last reads give theirs up)
        if cnt.sum() <= len(rest):
            break
        cnt[r] = 0 if r != 7 else cnt[r]
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(cnt)
    alts = lift_model.alt_records(rest[:int(off[-1])])
    if len(alts):
        alts["flags"][rng.integers(0, len(alts), max(1, len(alts) // 50))] &= ~np.uint8(bw.PLACE_MAPPED)
    return places, off, alts


def expected(t, bubbles, places, off, alts):
    as_places = np.zeros(len(alts), dtype=bw.PLACE_DTYPE)
    as_places["pos"], as_places["flags"] = alts["pos"], alts["flags"]
    return lift_model.expected_records(places, pad_model.expected_loci(places, t.start, t.end, t.bub_of, bubbles), off, alts,
                                       pad_model.expected_loci(as_places, t.start, t.end, t.bub_of, bubbles), bubbles, t.chrom)


def load(ctx, t, bubbles):
    ctx.set_loci(t.start, t.end, t.bub_of, pad_model.bubble_records(bubbles))
    ctx.set_bubble_chrom(t.chrom)


def same(got, want, what=""):
    diff = lift_model.compare_records(got, want[0], want[1])
    assert diff is None, (what, diff)


@pytest.fixture(scope="module")
def rel(bubbles):
    return relative_placements(bubbles)


@pytest.mark.parametrize("n_seq", [1, 2, 3, 7, 8, 9, 1_300_000])
def test_lift_records_equals_the_model_on_injected_records(toy_ctx, bubbles, rel, n_seq):
    """record tables around the powers of two of the search's step count and one of the GRCh37 shape"""
    t = table(n_seq, len(bubbles))
    places, off, alts = injected(t, rel, 700, n_seq)
    want = expected(t, bubbles, places, off, alts)
    load(toy_ctx, t, bubbles)
    same(toy_ctx.lift_records(places, off, alts), want, n_seq)
    lifted, unliftable, ms = toy_ctx.lift_stats()
    assert (lifted, unliftable) == (int((want[0] == bw.LIFT_LIFTED).sum()), int((want[0] == bw.LIFT_UNLIFTABLE).sum())) and ms > 0
    if n_seq >= 2:
        assert (want[0] == bw.LIFT_LIFTED).any() and (want[0] == bw.LIFT_UNLIFTABLE).any() and len(alts)
    if n_seq > 9:  # a record of every bubble: every outcome and every shape of the rule, among primaries and among items
        n = len(places)
        for part in (want[0][:n], want[0][n:]):
            assert {bw.LIFT_NONE, bw.LIFT_LIFTED, bw.LIFT_UNLIFTABLE} <= set(part.tolist())
        shapes = {"".join("MID?S"[op] for _, op in r[2]) for r in want[1] if r}
        assert {"M", "MIM", "MDM", "MIDM", "SM", "MS"} <= shapes and any(len(s) >= 12 for s in shapes), shapes
        assert any(n_ops == (1 << 28) - 1 for r in want[1] if r for n_ops, op in r[2] if op == bw.LIFT_D)
        assert (np.diff(off) == 255).any() and max(r[0] for r in want[1] if r) > 2**32
    if n_seq == 1:
        assert not want[0].any()  # one record: a chromosome, nothing to lift


@pytest.fixture(scope="module")
def grch37_shape(bubbles, rel):
    t = table(1_300_000, len(bubbles))
    places, off, alts = injected(t, rel, 1500, 37)
    return types.SimpleNamespace(t=t, places=places, off=off, alts=alts, want=expected(t, bubbles, places, off, alts))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_lift_records_on_a_few_reads(toy_ctx, bubbles, grch37_shape, n):
    """less than a wave, exactly one, one more; and none (no launch)"""
    g = grch37_shape
    load(toy_ctx, g.t, bubbles)
    k = int(g.off[n])
    want = (np.concatenate([g.want[0][:n], g.want[0][len(g.places):len(g.places) + k]]), g.want[1][:n] + g.want[1][len(g.places):len(g.places) + k])
    same(toy_ctx.lift_records(g.places[:n], g.off[:n + 1], g.alts[:k]), want, n)
    assert toy_ctx.lift_stats()[0] == int((want[0] == bw.LIFT_LIFTED).sum()) and (toy_ctx.lift_stats()[2] > 0) == (n > 0)


def test_lift_records_strides_over_more_placements_than_the_grid_has_lanes(toy_ctx, bubbles, grch37_shape):
    """the production path of both loops: more than twice 8 * CUs * 256 placements, so that every lane takes a third"""
    g = grch37_shape
    cus = compute_units()
    n_q = len(g.places) + len(g.alts)
    times = (2 * 8 * cus * 256) // n_q + 1
    load(toy_ctx, g.t, bubbles)
    off = np.concatenate([[0], np.cumsum(np.tile(np.diff(g.off), times))]).astype(np.uint64)
    got = toy_ctx.lift_records(np.tile(g.places, times), off, np.tile(g.alts, times))
    n = len(g.places)
    want = (np.concatenate([np.tile(g.want[0][:n], times), np.tile(g.want[0][n:], times)]), g.want[1][:n] * times + g.want[1][n:] * times)
    assert times * n_q > 2 * 8 * cus * 256
    same(got, want, f"{times * n_q} placements on {cus} CUs")


# ---- the pad_bub reads on the toy index -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_lift_and_slot_lift_equal_the_model_fed_the_oracles_hits(built, pad_text, lib):
    """one batch with -Q 6 / 3 and -X 5 / 1 / none, then through all eight slots with parked reads - on the product and on the test build"""
    env = dict(os.environ, BWB_SLICE_ITERS="150")
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lift_slots_worker.py"), pad_text], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "LIFT-SLOTS-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


def test_lift_errors_leave_the_context_usable(built, golden, pad_text, toy_tables, model):
    t = toy_tables
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    ctx = bw.Context(b)
    as_places = np.zeros(len(model.alts), dtype=bw.PLACE_DTYPE)
    as_places["pos"], as_places["flags"] = model.alts["pos"], model.alts["flags"]
    want = lift_model.expected_records(model.places, pad_model.expected_loci(model.places, t.start, t.end, t.bub_of, t.bubbles), model.off, model.alts,
                                       pad_model.expected_loci(as_places, t.start, t.end, t.bub_of, t.bubbles), t.bubbles, t.chrom)
    calls = (lambda: ctx.lift(), lambda: ctx.slot_lift(0), lambda: ctx.lift_records(model.places, model.off, model.alts))
    try:
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        for call in calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
                call()
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        for call in calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
                call()
        ctx.set_bubble_chrom(t.chrom)
        same(ctx.lift_records(model.places, model.off, model.alts), want)  # (needs no SA and no batch)
        for call in calls[:2]:
            with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
                call()
        ctx.set_sa(b.SA)
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            ctx.slot_lift(3)
        for slot in (-1, bw.MAX_SLOTS):
            with pytest.raises(bw.BwbError, match="error -1"):
                ctx.slot_lift(slot)
        for max_alt in (256, -1):
            with pytest.raises(bw.BwbError, match="error -1.*max_alt"):
                ctx.slot_lift(0, 6, max_alt)
            with pytest.raises(bw.BwbError, match="error -1.*max_alt"):
                ctx.lift(6, max_alt)
        one = np.zeros(1, dtype=bw.PLACE_DTYPE)
        for bad_off, k in (([1, 2], 2), ([0, 3, 2], 2)):
            with pytest.raises(bw.BwbError, match="error -1.*lift_records"):
                ctx.lift_records(np.repeat(one, len(bad_off) - 1), bad_off, np.zeros(k, dtype=bw.ALT_DTYPE))
        same(ctx.lift(), want)
        assert ctx.lift_stats()[:2] == (int((want[0] == bw.LIFT_LIFTED).sum()), 0)
        # a table the rule refuses: every refusal names bubble 2; -B and -J still take the table; a good table again and the records are back
        for col, value, why in ((2, 11061, "overlap"), (2, 11062 + (1 << 28), "2\\^28"), (5, -1, "alt_len"), (1, -1, "B_minus_A is negative"), (3, -2, "D_minus_C is below -1")):
            recs = t.recs.copy()
            recs[2][bw.BUBBLE_DTYPE.names[col]] = value
            ctx.set_loci(t.start, t.end, t.bub_of, recs)
            ctx.set_bubble_chrom(t.chrom)
            for call in calls:
                with pytest.raises(bw.BwbError, match="error -1.*bubble 2: .*" + why):
                    call()
            assert len(ctx.locus()[1]) == len(model.places)
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
            ctx.lift()
        ctx.set_bubble_chrom(t.chrom)
        same(ctx.lift(), want)
        ctx.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            ctx.lift()
        ctx.run()
        assert len(ctx.lift(6, 0)[0]) == 10
    finally:
        ctx.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def lifted_text(text, t):
    return lift_model.lift_sam(text, t.bubbles, t.names, t.chrom)


FLAGS = {"B": ([], "plain"), "XB": (["-X", "5"], "padded"), "XBJ": (["-X", "5", "-J"], "text")}


def base_text(model, pad_text, which):
    return open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read() if which == "plain" else getattr(model, which)


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("variant", ["one_chunk", "two_workers"])
def test_cli_map_with_lift_writes_the_models_text(map_dir, golden, pad_text, model, toy_tables, variant, flags):
    extra, env = VARIANTS[variant]
    opts, which = FLAGS[flags]
    out = map_dir / f"lift_{variant}_{flags}.sam"
    data = os.path.join(golden, "pad_toy.data")
    joins = [o for o in opts if o == "-J"]
    log = cli(["map", "-n", "3"] + [o for o in opts if o != "-J"] + ["-B", data] + joins + ["-R"] + extra + [map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out], env)
    want, lifted, unliftable = lifted_text(base_text(model, pad_text, which), toy_tables)
    assert open(out, "rb").read() == want
    assert f"placements lifted to chromosome coordinates on the GPU: lifted {lifted}  not liftable {unliftable}" in log and lifted >= 447


def test_cli_align_then_aln2sam_with_lift(map_dir, golden, pad_text, model, toy_tables, tmp_path):
    fa, fq, aln, out = map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "t.aln", tmp_path / "t.sam"
    data = os.path.join(golden, "pad_toy.data")
    cli(["align", "-n", "3", fa, fq, aln])
    for opts, which in FLAGS.values():
        cli(["aln2sam"] + opts + ["-B", data, "-R", fa, fq, aln, out])
        assert open(out, "rb").read() == lifted_text(base_text(model, pad_text, which), toy_tables)[0], opts


def test_cli_map_without_lift_writes_todays_bytes(map_dir, golden, pad_text, model):
    out = map_dir / "nolift.sam"
    data = os.path.join(golden, "pad_toy.data")
    for opts, which in FLAGS.values():
        log = cli(["map", "-n", "3"] + opts[:2] + ["-B", data] + opts[2:] + [map_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
        assert open(out, "rb").read() == base_text(model, pad_text, which) and "lifted" not in log


def test_cli_map_with_lift_on_records_out_of_text_order(golden, pad_text, model, toy_tables, tmp_path):
    """an .ann whose records do not ascend: loci, joins and lifts are resolved on the host, the log says so, the lines are the same"""
    for ext in ("", ".bwt"):
        shutil.copy(os.path.join(golden, "toy.fa" + ext), tmp_path / ("toy.fa" + ext))
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    out = tmp_path / "out.sam"
    log = cli(["map", "-n", "3", "-X", "5", "-B", os.path.join(golden, "pad_toy.data"), "-J", "-R", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"@")]
    want, lifted, _ = lifted_text(model.text, toy_tables)
    assert body(open(out, "rb").read()) == body(want)
    assert f"lifted to chromosome coordinates on the host (the .ann records are not ascending and disjoint): lifted {lifted}" in log


def test_cli_map_refuses_a_table_the_rule_cannot_use(golden, pad_text, map_dir, tmp_path):
    lines = open(os.path.join(golden, "pad_toy.data")).read().split("\n")
    lines[5] = lines[5].replace("11062", "11061")
    (tmp_path / "t.data").write_text("\n".join(lines))
    out = tmp_path / "out.sam"
    r = subprocess.run([bw.HOST_BIN, "map", "-n", "3", "-B", str(tmp_path / "t.data"), "-R", str(map_dir / "toy.fa"), os.path.join(pad_text, "pad_bub.fq"), str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode != 0 and "bubble 2 " in r.stdout and "(-R)" in r.stdout and not out.exists()


# ---- a generated multi-genome, indexed and mapped ---------------------------------------------------------------------------------------

def test_generated_genome_mapped_and_lifted(built, tmp_path):
    """`bwbble index`, then `map -n 3 -o 1 -X 5 -B t -R` on the generator's reads: every line with a bO tag is what the cmap of the record it
    names dictates; every read cut without errors across an allele is lifted to the POS and CIGAR its cut position dictates - the reads the
    judge cannot decide (unmapped, or placed elsewhere with an equal score) number ZERO; every other error-free read lies where it was cut"""
    g = lift_model.genome()
    reads = lift_model.reads(g)
    (tmp_path / "gen.fa").write_text(g["fasta"])
    (tmp_path / "gen.data").write_bytes(g["data"])
    (tmp_path / "gen.fq").write_text(lift_model.fastq(reads))
    cli(["index", tmp_path / "gen.fa"])
    log = cli(["map", "-n", "3", "-o", "1", "-X", "5", "-B", tmp_path / "gen.data", "-R", tmp_path / "gen.fa", tmp_path / "gen.fq", tmp_path / "out.sam"])
    lines = [ln.split("\t") for ln in open(tmp_path / "out.sam").read().split("\n") if ln and ln[0] != "@"]
    assert len(lines) == len(reads) and "lifted to chromosome coordinates on the GPU" in log
    record_of = {r[0].split()[0]: k for k, r in enumerate(g["records"])}
    tagged = across = undecided = 0
    for f, (name, k, o, ln, strand, edit, seq, cig) in zip(lines, reads):
        assert f[0] == name
        if f[-1].startswith("bO:Z:"):
            rec, pos1, orig = f[-1][5:].rsplit(",", 2)
            assert lift_model.judge(g["records"][record_of[rec]][2], int(pos1), orig) == (int(f[3]), f[5]), name
            assert f[2] == g["names"][0]
            tagged += 1
        if edit is not None:
            continue
        want = lift_model.judge(g["records"][k][2], o + 1, cig)
        crosses = want[1] != f"{ln}M"
        across += crosses
        if f[1] == "4" or (f[2], int(f[3]), f[5]) != (g["names"][0], want[0], want[1]):
            undecided += 1
            print("undecided:", name, f[1:6], want)
        elif crosses:
            assert f[-1].startswith("bO:Z:") and lift_model.mismatches(g["chrom"], int(f[3]), f[5], f[9]) == 0, name
    assert across >= 300 and tagged >= across
    assert undecided == 0
