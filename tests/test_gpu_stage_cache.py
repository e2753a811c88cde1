"""What a slot's cached stage records answer after something they depend on has changed (bwb_hip.hip: StageCache): other arguments on the same
submission, a replaced bubble table, a replaced text, a re-uploaded batch.  One context on the toy index, the 571 pad_bub reads in one batch
(-n 3); every answer is judged by the Python models (pad_model, join_model, lift_model, md_model) fed the REFERENCE's hits for the arguments and
the tables of that very call - so a record that was kept where it had to be made again shows as the model's records for the earlier call."""
import os
import types

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import join_model
import lift_model
import map_model
import md_model
import oracle_lib
import pad_model
from test_gpu_join import pad_text, toy_tables  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def want_of(orc, idx, sa, reads, seqs, lens, t, recs, text, starts, max_mm, max_alt):
    """the models' records of these reads for (max_mm, max_alt) under the bubble table recs (BUBBLE_DTYPE) and the text"""
    bubbles = [(b[0],) + tuple(int(v) for v in r) for b, r in zip(t.bubbles, recs)]
    places, _ = map_model.expected_places(orc, idx, reads, max_mm)
    off, alts, _ = alt_model.expected_alts(reads, max_alt, sa)
    loci = pad_model.expected_loci(places, t.start, t.end, t.bub_of, bubbles)
    joins, _ = join_model.expected_joins(places, off, alts, join_model.suboptimal(reads, off, alts), t.start, t.end, t.bub_of, bubbles, t.chrom, max_mm)
    as_places = np.zeros(len(alts), dtype=bw.PLACE_DTYPE)
    as_places["pos"], as_places["flags"] = alts["pos"], alts["flags"]
    kinds, lrecs = lift_model.expected_records(places, loci, off, alts, pad_model.expected_loci(as_places, t.start, t.end, t.bub_of, bubbles), bubbles, t.chrom)
    n = len(places)
    return types.SimpleNamespace(places=places, loci=loci, off=off, alts=alts, joins=joins, kinds=kinds, lrecs=lrecs,
                                 md=md_model.expected_records(text, seqs, lens, places), md_lifted=md_model.expected_records(text, seqs, lens, places, kinds[:n], lrecs[:n], starts))


def differ(a, b):
    """the stages of which two expectations do not agree"""
    out = set()
    if a.places.tobytes() != b.places.tobytes() or a.loci.tobytes() != b.loci.tobytes():
        out.add("locus")
    if a.joins.tobytes() != b.joins.tobytes() or a.alts.tobytes() != b.alts.tobytes():
        out.add("join")
    if len(a.kinds) != len(b.kinds) or (a.kinds != b.kinds).any() or a.lrecs != b.lrecs:
        out.add("lift")
    if md_model.compare_records(a.md_lifted, b.md_lifted) is not None:
        out.add("md_lifted")
    if md_model.compare_records(a.md, b.md) is not None:
        out.add("md")
    return out


def check(ctx, w, max_mm, max_alt, what):
    """locus, join, lift and both kinds of batch_md for these arguments against the expectation w"""
    places, loci = ctx.locus(max_mm)
    assert places.tobytes() == w.places.tobytes() and loci.tobytes() == w.loci.tobytes(), (what, "locus", pad_model.first_difference(loci, w.loci))
    if max_alt:  # (join takes 1 .. 255)
        for g, x, name in zip(ctx.join(max_mm, max_alt), (w.places, w.off, w.alts, w.loci, w.joins), ("places", "alt_off", "alts", "loci", "joins")):
            assert g.tobytes() == np.asarray(x, dtype=g.dtype).tobytes(), (what, "join", name)
    assert lift_model.compare_records(ctx.lift(max_mm, max_alt), w.kinds, w.lrecs) is None, (what, "lift", lift_model.compare_records(ctx.lift(max_mm, max_alt), w.kinds, w.lrecs))
    for lifted, want in ((True, w.md_lifted), (False, w.md)):
        diff = md_model.compare_records(ctx.batch_md(max_mm, max_alt, lifted), want)
        assert diff is None, (what, "md", lifted, diff)


def test_stage_records_follow_their_arguments_tables_text_and_batch(built, golden, oracle, pad_text, toy_tables):
    t = toy_tables
    bwt = os.path.join(golden, "toy.fa.bwt")
    idx = oracle.load_index(bwt, load_sa=True)
    sa = alt_model.OracleSA(oracle, idx)
    reads = oracle_lib.parse_aln(open(os.path.join(pad_text, "pad_bub_n3.aln"), "rb").read())
    seqs, lens = bw.encode_reads(bw.read_fastq(os.path.join(pad_text, "pad_bub.fq")))
    text, _, starts = md_model.fasta_text(open(os.path.join(golden, "toy.fa")).read())
    want = lambda recs, txt, max_mm, max_alt, k=len(lens): want_of(oracle, idx, sa, reads[:k], seqs[:k], lens[:k], t, recs, txt, starts, max_mm, max_alt)
    # On these reads the models predict the SAME records for (6, 5) and (3, 1): no primary has three mismatches and a unique best hit, and no read
    # has 3 .. 6 placements.  What tells two calls apart here is max_mm 0 (MAPQ 25 for a unique read without a mismatch: placement and join records)
    # and max_alt 0 (the primaries alone: lift records), so the sequence asks those too; NM and MD depend on neither.
    w65, w31, w01, w60 = want(t.recs, text, 6, 5), want(t.recs, text, 3, 1), want(t.recs, text, 0, 1), want(t.recs, text, 6, 0)
    assert {"locus", "join"} <= differ(w65, w01) and "lift" in differ(w65, w60)

    # another table: C of the bubble with the most lifted primaries, seven positions on - its right flank lands elsewhere, its deletion is longer
    n = len(lens)
    busiest = int(np.bincount(w65.loci["bubble"][w65.kinds[:n] == bw.LIFT_LIFTED]).argmax())
    recs2 = t.recs.copy()
    recs2[busiest]["C"] += 7
    v65 = want(recs2, text, 6, 5)
    assert {"lift", "md_lifted"} <= differ(w65, v65)

    # another text: a base under the first forward primary with MD tags that lies on no bubble, changed to a base the read does not have there
    r = int(np.flatnonzero((w65.md[0]["kind"] == bw.MD_OK) & (w65.loci["bubble"] < 0) & (w65.loci["seqid"] >= 0) & ((w65.places["flags"] & bw.PLACE_REVERSE) == 0))[0])
    at = int(w65.places["pos"][r]) + 2
    text2 = text[:at] + ("A" if text[at] != "A" else "C") + text[at + 1:]
    u65 = want(recs2, text2, 6, 5)
    assert {"md", "md_lifted"} <= differ(v65, u65) and differ(v65, u65) <= {"md", "md_lifted"}

    b = bw.BwtFile(bwt, load_sa=True)
    ctx = bw.Context(b)
    try:
        ctx.set_sa(b.SA)
        ctx.set_text(md_model.codes(text))
        ctx.set_loci(t.start, t.end, t.bub_of, t.recs)
        ctx.set_bubble_chrom(t.chrom)
        p = bw.params(["-n", "3"])
        ctx.align(p, seqs, lens)
        # keys: one submission asked with other arguments, and with the first ones again
        check(ctx, w65, 6, 5, "first (6, 5)")
        check(ctx, w31, 3, 1, "(3, 1) behind (6, 5)")
        check(ctx, w65, 6, 5, "(6, 5) behind (3, 1)")
        check(ctx, w01, 0, 1, "(0, 1) behind (6, 5)")
        check(ctx, w60, 6, 0, "(6, 0) behind (0, 1)")
        check(ctx, w65, 6, 5, "(6, 5) behind (6, 0)")
        # replaced tables: a valid table that differs in one field
        ctx.set_loci(t.start, t.end, t.bub_of, recs2)
        ctx.set_bubble_chrom(t.chrom)
        check(ctx, v65, 6, 5, "another bubble table")
        # replaced text
        ctx.set_text(md_model.codes(text2))
        check(ctx, u65, 6, 5, "another text")
        # re-upload: ten reads in the slot that held 571
        ctx.upload(p, seqs[:10], lens[:10])
        ctx.run()
        check(ctx, want(recs2, text2, 6, 5, 10), 6, 5, "ten reads")
    finally:
        ctx.close()
