"""NM:i and MD:Z against the text (`bwbble map -D`, kernels k_text_pack / k_md_count / k_md) on the GPU, judged by tests/md_model.py:
Context.md_records on injected records over a constructed text - every read base on every text code, windows at every offset of a 32-character
word, the text's first and last characters, read lengths up to 255, CIGARs with up to eight gap runs, both strands, lifted records -; the pad_bub
reads in one batch and streamed through the slots (tests/md_slots_worker.py); the state and argument errors; and the command line against the
model's text and against `align` + `aln2sam -D`."""
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import bwbble_amd as bw
import lift_model
import md_model
import pad_model
from test_gpu_join import VARIANTS, model, pad_text, toy_tables  # noqa: F401 (fixtures)
from test_gpu_lift import gapped
from test_gpu_map import cli, compute_units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, S = bw.LIFT_M, bw.LIFT_I, bw.LIFT_D, bw.LIFT_S


@pytest.fixture(scope="module")
def text():
    """3 200 characters in two records: every code beside every other at both parities, stretches of plain bases, IUPAC codes now and then"""
    rng = np.random.default_rng(16)
    body = "".join(rng.choice(list("ACGT" * 8 + md_model.LETTERS[1:]), 3000 - 47))
    t = "T" + md_model.LETTERS[1:] * 3 + body + "$"
    t = t[:1400] + "$" + t[1401:]
    return t + "ACGT" * 50 + "$"


@pytest.fixture(scope="module")
def ctx(built, golden, text):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    c.set_text(md_model.codes(text))
    h = text.index("$") + 1
    c.set_loci(np.array([0, h], dtype=np.uint64), np.array([h - 1, len(text) - 1], dtype=np.uint64), np.array([-1, -1], dtype=np.int32), np.zeros(0, dtype=bw.BUBBLE_DTYPE))
    c.starts = [0, h]
    yield c
    c.close()


def read_for(text, start, ops, rng, mismatches=()):
    """SEQ as SAM prints it for ops [(len, op)] at `start`: a member of every text code under M (A where there is none), random bases elsewhere,
    and another base at the given SEQ offsets"""
    seq, t = [], start
    for n, op in ops:
        if op == "M":
            seq += [(md_model.MEMBERS.get(text[t + k] if 0 <= t + k < len(text) else "A") or "A")[0] for k in range(n)]
        elif op in "IS":
            seq += list(rng.choice(list("ACGT"), n))
        t += n if op in "MD" else 0
    for i in mismatches:
        seq[i] = "N" if seq[i] == "T" else "ACGT"[("ACGT".index(seq[i]) + 1) % 4]
    return "".join(seq)


def cases(text):
    """[(start, CIGAR, SEQ, lifted ops or None)]: what the kernels can get wrong"""
    rng = np.random.default_rng(5)
    n = len(text)
    # every read base x every text code at both parities; `$`, a code of its own (it matches nothing and prints N), under every base too: the one
    # at the even position 1400 and the one at the odd position 2999, in the middle and at either end of a window
    out = [(k, "15M", b * 15, None) for b in "ACGTN" for k in (1, 2, 16, 17, 1386, 1393, 1400, 2985, 2992, 2999)]
    for off in range(32):                                                                               # every offset of a 32-character word; one and two words crossed
        for ln in (20, 33, 70):
            out.append((64 + off, f"{ln}M", read_for(text, 64 + off, [(ln, "M")], rng, (0, ln - 1) if off % 3 == 0 else ()), None))
    out += [(0, "9M", read_for(text, 0, [(9, "M")], rng), None), (n - 9, "9M", read_for(text, n - 9, [(9, "M")], rng), None),  # the first and the last character
            (n - 8, "9M", "A" * 9, None), (n, "1M", "A", None), (n - 5, "3M3D1M", "ACGT", None), (n - 6, "3M2D1M", "ACGT", None)]  # leaving the text by one
    at = n - 201  # the plain stretch
    for ln in (1, 2, 31, 32, 33, 100, 255):
        out.append((600, f"{ln}M", read_for(text, 600, [(ln, "M")], rng, (ln // 2,)), None))
    for mm in ((0,), (119,), (50, 51), (9, 19), (10, 110), (20, 119), (99,), (100,), (0, 1, 2), (117, 118, 119)):  # first, last, adjacent; runs of 9, 10, 99, 100
        out.append((at, "120M", read_for(text, at, [(120, "M")], rng, mm), None))
    for cig, mm in (("10M2D10M", (10,)), ("10M2I3D10M", ()), ("10M3D2I10M", ()), ("5M1D1I1D5M", ()), ("10M2D10M", (9,))):  # D then a mismatch; I beside D
        out.append((at, cig, read_for(text, at, md_model.parse_cigar(cig), rng, mm), None))
    for runs in range(1, 9):                                                                            # up to eight gap runs
        for _ in range(4):
            cig = gapped(rng, runs, 90)
            p = int(rng.integers(1, n - 300))
            ops = md_model.parse_cigar(cig)
            out.append((p, cig, read_for(text, p, ops, rng, tuple(rng.integers(0, sum(k for k, op in ops if op in "MI"), 2))), None))
    far = (1 << 28) - 1
    for pos, lops in ((700, [(40, M), (3, I), (57, M)]), (1405, [(5, S), (95, M)]), (1500, [(90, M), (10, S)]), (800, [(30, M), (2, I), (130, D), (68, M)]), (1401, [(50, M), (7, D), (50, M)]),
                      (100, [(1, M), (far, D), (1, D), (2, M)]), (100, [(10, M), (md_model.MAX_SPAN - 19, D), (10, M)]), (n - 99, [(100, M)])):
        ops = [(k, "MID?S"[op]) for k, op in lops]
        out.append((pos, None, read_for(text, pos, ops, rng, (1,) if lops[0][0] > 1 and lops[0][1] == M else ()), lops))
    return out


def records(ctx, text, cs):
    """the cases on both strands, a few of them unmapped -> what md_records takes, and the model's answer"""
    rows = [(c, rev) for c in cs for rev in (False, True)]
    seqs, lens = np.full((len(rows), 255), 4, dtype=np.uint8), np.zeros(len(rows), dtype=np.uint16)
    placed, kinds, lrecs = [], np.zeros(len(rows), dtype=np.uint8), [None] * len(rows)
    for r, ((start, cig, seq, lops), rev) in enumerate(rows):
        up = seq[::-1].translate(md_model.COMP) if rev else seq
        seqs[r, :len(up)], lens[r] = ["AGCTN".index(c) for c in up], len(up)
        if lops is None:
            placed.append((start, rev, cig))
        else:  # (the placement itself lies somewhere else: on a bubble record)
            placed.append((7, rev, f"{len(seq)}M"))
            seqid = 1 if start >= ctx.starts[1] else 0
            kinds[r], lrecs[r] = bw.LIFT_LIFTED, (start - ctx.starts[seqid] + 1, seqid, lops)
    places = lift_model.place_records(placed)
    places["flags"][::37] = 0
    want = md_model.expected_records(text, seqs, lens, places, kinds, lrecs, ctx.starts)
    return seqs, lens, places, md_model.pack_lift(kinds, lrecs), want


def same(got, want, what=""):
    diff = md_model.compare_records(got, want)
    assert diff is None, (what, diff)


@pytest.fixture(scope="module")
def injected(ctx, text):
    return records(ctx, text, cases(text))


def test_md_records_equals_the_model_on_injected_records(ctx, text, injected):
    seqs, lens, places, lift, want = injected
    same(ctx.md_records(seqs, lens, places, *lift), want)
    n_ok, n_bytes, ms = ctx.md_stats()
    assert (n_ok, n_bytes) == (int((want[0]["kind"] == bw.MD_OK).sum()), len(want[2])) and ms > 0
    kinds = want[0]["kind"]
    assert (kinds == bw.MD_TOO_LONG).sum() >= 2 and (kinds == bw.MD_NONE).sum() >= 10 and (kinds == bw.MD_OK).sum() > 300
    mds = [want[2][int(want[1][r]):int(want[1][r + 1])].decode() for r in range(len(kinds))]
    numbers = {int(v) for m in mds for v in re.findall(r"\d+", m)}
    assert {0, 9, 10, 99, 100} <= numbers and any("^" in m for m in mds) and any(re.search(r"[A-Z]0[A-Z]", m) for m in mds) and any(re.search(r"\^[A-Z]+0[A-Z]", m) for m in mds)
    assert any(m.startswith("0") and len(m) > 1 for m in mds) and max(len(m) for m in mds) >= 130 and set(lens.tolist()) >= {1, 2, 31, 32, 33, 100, 255}
    rows = [(c, rev) for c in cases(text) for rev in (False, True)]
    # all 5 x 16 pairs of a read base and a text code meet under an M of a read that gets its tags, on either strand
    assert text[1400] == text[2999] == "$"
    for strand in (False, True):
        covered = set()
        for r, ((start, cig, seq, lops), rev) in enumerate(rows):
            if rev == strand and kinds[r] == bw.MD_OK:
                covered |= md_model.pairs(text, start, md_model.parse_cigar(cig) if lops is None else [(k, "MID?S"[op]) for k, op in lops], seq)
        assert covered == md_model.ALL_PAIRS, (strand, sorted(md_model.ALL_PAIRS - covered))
    # the judge, on what the kernel wrote
    got = ctx.md_records(seqs, lens, places, *lift)
    for r, ((start, cig, seq, lops), rev) in enumerate(rows):
        if got[0][r]["kind"] == bw.MD_OK:
            ops = md_model.parse_cigar(cig) if lops is None else [(k, "MID?S"[op]) for k, op in lops]
            assert md_model.judge(text, start, ops, seq, int(got[0][r]["nm"]), got[2][int(got[1][r]):int(got[1][r + 1])].decode()) is None, (r, start, cig, lops)
    # without the lift arguments the lifted reads are walked where their own records say
    plain = md_model.expected_records(text, seqs, lens, places)
    same(ctx.md_records(seqs, lens, places), plain, "no lift records")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_md_records_on_a_few_reads(ctx, text, injected, n):
    """less than a wave, exactly one, one more; and none (no launch)"""
    seqs, lens, places, _, _ = injected
    same(ctx.md_records(seqs[:n], lens[:n], places[:n]), md_model.expected_records(text, seqs[:n], lens[:n], places[:n]), n)
    assert (ctx.md_stats()[2] > 0) == (n > 0)


def test_md_records_strides_over_more_reads_than_the_grid_has_lanes(ctx, text, injected):
    """70 000 reads of up to 255 bases, lifted records among them, every one compared"""
    seqs, lens, places, lift, want = injected
    n = len(lens)
    times = 70_000 // n + 1
    assert times * n >= 70_000
    kinds, off, words = lift
    step = np.diff(off)
    got = ctx.md_records(np.tile(seqs, (times, 1)), np.tile(lens, times), np.tile(places, times), np.tile(kinds, times),
                         np.concatenate([[0], np.cumsum(np.tile(step, times))]).astype(np.uint64), np.tile(words, (times, 1)))
    md_len = np.tile(want[0]["md_len"].astype(np.uint64), times)
    same(got, (np.tile(want[0], times), np.concatenate([[0], np.cumsum(md_len)]).astype(np.uint64), want[2] * times), f"{times * n} reads")


def test_md_records_strides_over_twice_the_lanes_of_the_grid(ctx, text, injected):
    """the production path of both loops: more than twice 8 * CUs * 256 reads - the short ones of the injected records, 33 bytes apart -, so that
    every lane takes a third"""
    seqs, lens, places, _, _ = injected
    short = np.flatnonzero(lens <= 33)
    seqs, lens, places = np.ascontiguousarray(seqs[short, :33]), lens[short], places[short]
    want = md_model.expected_records(text, seqs, lens, places)
    lanes = 8 * compute_units() * 256
    times = 2 * lanes // len(lens) + 1
    got = ctx.md_records(np.tile(seqs, (times, 1)), np.tile(lens, times), np.tile(places, times))
    off = np.concatenate([[0], np.cumsum(np.tile(want[0]["md_len"].astype(np.uint64), times))]).astype(np.uint64)
    assert times * len(lens) > 2 * lanes and (want[0]["kind"] == bw.MD_OK).sum() > 100 and (want[0]["kind"] == bw.MD_NONE).any()
    assert got[0].tobytes() == np.tile(want[0], times).tobytes() and np.array_equal(got[1], off) and got[2] == want[2] * times
    assert ctx.md_stats()[:2] == (times * int((want[0]["kind"] == bw.MD_OK).sum()), times * len(want[2]))


def test_set_text_refuses_a_code_above_15(built, golden, text):
    c = bw.Context(os.path.join(golden, "toy.fa.bwt"))
    try:
        codes = md_model.codes(text).copy()
        one = (np.zeros((1, 4), dtype=np.uint8), np.array([4], dtype=np.uint16), lift_model.place_records([(5, False, "4M")]))
        for at in (0, 31, 33, len(codes) - 1):
            bad = codes.copy()
            bad[at] = 16
            with pytest.raises(bw.BwbError, match="error -1.*above 15"):
                c.set_text(bad)
            with pytest.raises(bw.BwbError, match="error -4.*set_text"):
                c.md_records(*one)
        with pytest.raises(bw.BwbError, match="error -1"):
            c.set_text(np.zeros(0, dtype=np.uint8))
        c.set_text(codes)
        same(c.md_records(*one), md_model.expected_records(text, *one))
    finally:
        c.close()


@pytest.mark.parametrize("lib", ["product", "testlib"])
def test_md_and_slot_md_equal_the_model_fed_the_oracles_hits(built, pad_text, lib):
    """a text uploaded in two chunks; one batch with -Q 6 / 3, plain and lifted; then through all eight slots with parked reads - on the product
    and on the test build"""
    env = dict(os.environ, BWB_SLICE_ITERS="150")
    if lib == "testlib":
        bw.build(testlib=True)
        env["BWB_LIB"] = bw.TEST_LIB_PATH
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "md_slots_worker.py"), pad_text], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "MD-SLOTS-OK" in r.stdout, r.stdout[-3000:]
    assert ("libbwbble_hip_test.so" in r.stdout) == (lib == "testlib")


def test_md_errors_leave_the_context_usable(built, golden, pad_text, toy_tables):
    t = toy_tables
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    toy_text, names, starts = md_model.fasta_text(open(os.path.join(golden, "toy.fa")).read())
    b = bw.BwtFile(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    c = bw.Context(b)
    one = (seqs[:1], lens[:1], lift_model.place_records([(5, False, f"{int(lens[0])}M")]))
    lifted_one = md_model.pack_lift([bw.LIFT_LIFTED], [(6, 0, [(int(lens[0]), M)])])
    slot_calls = (lambda: c.batch_md(), lambda: c.slot_md(0), lambda: c.batch_md(6, 5, True), lambda: c.slot_md(0, 6, 5, True))
    try:
        c.set_text(md_model.codes(toy_text))
        c.align(bw.params(["-n", "3"]), seqs, lens)
        assert c.md_stats() == (0, 0, 0.0)  # (a batch without an md call launches nothing)
        want_one = md_model.expected_records(toy_text, *one)
        same(c.md_records(*one), want_one)  # (needs no SA and no batch)
        for call in slot_calls:
            with pytest.raises(bw.BwbError, match="error -4.*set_sa"):
                call()
        with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
            c.md_records(*one, *lifted_one)
        c.set_sa(b.SA)
        for call in slot_calls[2:]:
            with pytest.raises(bw.BwbError, match="error -4.*set_loci"):
                call()
        c.set_loci(t.start, t.end, t.bub_of, t.recs)
        for call in slot_calls[2:]:
            with pytest.raises(bw.BwbError, match="error -4.*set_bubble_chrom"):
                call()
        same(c.md_records(*one, *lifted_one), want_one, "a lift record that says what the placement says")
        with pytest.raises(bw.BwbError, match="error -4.*not been submitted"):
            c.slot_md(3)
        for slot in (-1, bw.MAX_SLOTS):
            with pytest.raises(bw.BwbError, match="error -1"):
                c.slot_md(slot)
        two = (seqs[:2], lens[:2], lift_model.place_records([(5, False, "100M")] * 2))
        for bad_off in ([1, 2, 2], [0, 2, 1]):
            with pytest.raises(bw.BwbError, match="error -1.*md_records"):
                c.md_records(*two, np.array([1, 0], dtype=np.uint8), np.array(bad_off, dtype=np.uint64), lifted_one[2][:bad_off[-1]])
        # a lift record of a record the table does not have, and one that does not fit its words: no tags, nothing read
        for seqid, n_ops in ((len(t.start), 1), (0, 9)):
            words = lifted_one[2].copy()
            words[0][2], words[0][3] = seqid, n_ops
            assert c.md_records(*one, lifted_one[0], lifted_one[1], words)[0][0]["kind"] == bw.MD_NONE
        got = c.batch_md()
        assert len(got[0]) == len(lens) and (got[0]["kind"] == bw.MD_OK).sum() == 569 == c.md_stats()[0]
        c.set_bubble_chrom(t.chrom)
        lifted = c.batch_md(6, 5, True)
        assert (lifted[0]["kind"] == bw.MD_OK).sum() == 569 and lifted[2] != got[2]
        c.upload(bw.params(["-n", "3"]), seqs[:10], lens[:10])
        with pytest.raises(bw.BwbError):
            c.batch_md()
        c.run()
        assert len(c.batch_md()[0]) == 10 and c.batch_md()[2] == got[2][:int(got[1][10])]
    finally:
        c.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def md_dir(built, golden, tmp_path_factory):
    """toy.fa with its index, and the .ref `bwbble fasta2ref` writes"""
    d = tmp_path_factory.mktemp("mapmd")
    shutil.copy(os.path.join(golden, "toy.fa"), d / "toy.fa")
    cli(["fasta2ref", d / "toy.fa"])
    assert open(d / "toy.fa.ann").read() == open(os.path.join(golden, "toy.fa.ann")).read()
    shutil.copy(os.path.join(golden, "toy.fa.bwt"), d / "toy.fa.bwt")
    return d


@pytest.fixture(scope="module")
def toy(golden):
    text, names, starts = md_model.fasta_text(open(os.path.join(golden, "toy.fa")).read())
    return types.SimpleNamespace(text=text, names=names, starts=starts)


def tagged(base, toy):
    want, census = md_model.tag_sam(base, toy.text, toy.names, toy.starts)
    bad, _ = md_model.judge_sam(want, toy.text, toy.names, toy.starts)
    assert not bad and census[md_model.NONE] == census[md_model.TOO_LONG] == 0
    return want, census[md_model.OK]


def base_texts(model, pad_text, toy_tables):
    t = toy_tables
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read()
    return {"plain": ([], plain), "XBJR": (["-X", "5", "-B", "DATA", "-J", "-R"], lift_model.lift_sam(model.text, t.bubbles, t.names, t.chrom)[0]),
            "BR": (["-B", "DATA", "-R"], lift_model.lift_sam(open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read(), t.bubbles, t.names, t.chrom)[0]),
            "XB": (["-X", "5", "-B", "DATA"], model.padded)}


@pytest.mark.parametrize("flags", ["plain", "XBJR", "BR", "XB"])
@pytest.mark.parametrize("variant", ["one_chunk", "two_workers"])
def test_cli_map_with_md_writes_the_models_text(md_dir, golden, pad_text, model, toy_tables, toy, variant, flags):
    extra, env = VARIANTS[variant]
    opts, base = base_texts(model, pad_text, toy_tables)[flags]
    opts = [os.path.join(golden, "pad_toy.data") if o == "DATA" else o for o in opts]
    out = md_dir / f"md_{variant}_{flags}.sam"
    log = cli(["map", "-n", "3"] + opts + ["-D"] + extra + [md_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out], env)
    want, n_ok = tagged(base, toy)
    got = open(out, "rb").read()
    assert got == want, pad_model.first_difference(got, want)
    assert f"NM and MD against the text on the GPU: reads {n_ok} " in log and n_ok == 569
    # and without -D: the bytes of today, nothing loaded or launched
    log = cli(["map", "-n", "3"] + opts + extra + [md_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out], env)
    assert open(out, "rb").read() == base and "NM and MD" not in log


def test_cli_align_then_aln2sam_with_md(md_dir, golden, pad_text, model, toy_tables, toy, tmp_path):
    fa, fq, aln, out = md_dir / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "t.aln", tmp_path / "t.sam"
    cli(["align", "-n", "3", fa, fq, aln])
    for opts, base in base_texts(model, pad_text, toy_tables).values():
        opts = [os.path.join(golden, "pad_toy.data") if o == "DATA" else o for o in opts]
        cli(["aln2sam"] + opts + ["-D", fa, fq, aln, out])
        assert open(out, "rb").read() == tagged(base, toy)[0], opts


def test_cli_map_with_md_on_records_out_of_text_order(md_dir, golden, pad_text, model, toy_tables, toy, tmp_path):
    """an .ann whose records do not ascend: with -R the lift records come from the host's rule and so do NM and MD, and the log says so; without
    -R the kernels need no record table"""
    for ext in ("", ".bwt", ".ref"):
        shutil.copy(md_dir / ("toy.fa" + ext), tmp_path / ("toy.fa" + ext))
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    out = tmp_path / "out.sam"
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"@")]
    opts, base = base_texts(model, pad_text, toy_tables)["XBJR"]
    opts = [os.path.join(golden, "pad_toy.data") if o == "DATA" else o for o in opts]
    log = cli(["map", "-n", "3"] + opts + ["-D", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    assert body(open(out, "rb").read()) == body(tagged(base, toy)[0])
    assert "NM and MD against the text on the host (the .ann records are not ascending and disjoint): reads 569" in log
    log = cli(["map", "-n", "3", "-D", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), out])
    assert body(open(out, "rb").read()) == body(tagged(base_texts(model, pad_text, toy_tables)["plain"][1], toy)[0])
    assert "NM and MD against the text on the GPU: reads 569" in log
