"""A read's placements counted by locus (`-J`) without a GPU: the model (tests/join_model.py) against the truth the pad_bub reads carry in
their names, the counts that make the fixture worth testing with, the SAM formatter and the host's rule fed with the model's records
(`places2sam -B -J`), the refusals, and the layout of the new record of the C-ABI.  Every input of the model derives from the reference:
its hits (pad_bub_n3.aln), its SAM text, the oracle's SA, and the models pinned to its bytes."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import join_model
import map_model
import oracle_lib
import pad_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the model finds on the fixture with -X 5 (and with -X 1 and -X 255: no read of it has more than two placements at one locus)
ITEMS, JOINED_READS, JOINED_PER_STRAND, MAPQ_RAISED_FROM_0 = 272, 260, 130, 259


def run(args, **kw):
    return subprocess.run([bw.HOST_BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


@pytest.fixture(scope="module")
def pad_text(tmp_path_factory):
    return pad_model.unpack(tmp_path_factory.mktemp("join"))


@pytest.fixture(scope="module")
def fx(golden, oracle, pad_text):
    """the pad_bub reads: the reference's hits -> the model's placement records, items (-X 5), suboptimal bytes and join records"""
    idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(pad_text, "pad_bub_n3.aln"), "rb").read())
    places, _ = map_model.expected_places(oracle, idx, reads, 6)
    off, alts, _ = alt_model.expected_alts(reads, 5, alt_model.OracleSA(oracle, idx))
    names, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
    bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
    t = types.SimpleNamespace(names=names, start=start, end=end, bubbles=bubbles, bub_of=pad_model.bubble_of(names, bubbles), chrom=join_model.chrom_of(names, bubbles))
    sub = join_model.suboptimal(reads, off, alts)
    joins, total = join_model.expected_joins(places, off, alts, sub, t.start, t.end, t.bub_of, t.bubbles, t.chrom, 6)
    qnames = [ln[1:].split()[0] for ln in open(os.path.join(pad_text, "pad_bub.fq")).read().split("\n")[0::4] if ln]
    return types.SimpleNamespace(reads=reads, places=places, off=off, alts=alts, sub=sub, joins=joins, total=total, t=t, qnames=qnames)


def test_joined_reads_lie_where_their_names_say(fx):
    """a read named bubbleK_oO_lL_+/- was cut at offset O of bubble K = 124 flanking bases, the inserted allele, 124 more, around position p of
    the chromosome its header names: its first base is the chromosome's p - 123 + O in the left flank and p + 1 + (O - 124 - ins) in the right
    one.  For every such read the model joins: the primary's locus starts there, and of the primary and its joined item one lies on the
    chromosome's own record, the other on bubble K's"""
    t = fx.t
    owner, joined = join_model.item_classes(fx.places, fx.off, fx.alts, t.start, t.end, t.bub_of, t.bubbles, t.chrom)
    _, cp, _, lop, _ = join_model.loci4(fx.places["pos"], fx.places["flags"], t.start, t.end, t.bub_of, t.bubbles, t.chrom)
    record_of = lambda pos: int(np.searchsorted(t.start, np.uint64(pos), side="right")) - 1
    bubble_record = {int(b): i for i, b in enumerate(t.bub_of) if b >= 0}
    checked = {"left": 0, "right": 0}
    for q in np.flatnonzero(joined):
        r = int(owner[q])
        m = re.fullmatch(r"bubble(\d+)_o(\d+)_l(\d+)_([+-])", fx.qnames[r])
        if not m:
            continue
        K, O = int(m.group(1)), int(m.group(2))
        _, chrom_name, p = t.names[bubble_record[K]].split()
        ins = t.bubbles[K][6]
        if O < 124:
            want, side = int(p) - 123 + O, "left"
        elif O >= 124 + ins:
            want, side = int(p) + 1 + (O - 124 - ins), "right"
        else:
            continue
        chrom_record = [i for i, n in enumerate(t.names) if n.split()[0] == chrom_name]
        assert len(chrom_record) == 1 and int(cp[r]) == chrom_record[0] == int(t.chrom[K]), fx.qnames[r]
        assert int(lop[r]) == want, (fx.qnames[r], int(lop[r]), want)
        assert {record_of(fx.places["pos"][r]), record_of(fx.alts["pos"][q])} == {chrom_record[0], bubble_record[K]}, fx.qnames[r]
        checked[side] += 1
    assert checked["left"] >= 50 and checked["right"] >= 50, checked


def test_fixture_is_worth_joining(fx):
    """at least 8 joined reads on each strand and at least 100 reads raised from MAPQ 0 - and the exact counts the documents quote"""
    j = fx.joins["joined"] > 0
    rev = (fx.places["flags"] & bw.PLACE_REVERSE) != 0
    raised = (fx.places["mapq"] == 0) & (fx.joins["mapq"] > 0)
    assert (j & ~rev).sum() >= 8 and (j & rev).sum() >= 8 and raised.sum() >= 100
    assert (len(fx.alts), int(j.sum()), int((j & ~rev).sum()), int((j & rev).sum()), int(raised.sum())) == (ITEMS, JOINED_READS, JOINED_PER_STRAND, JOINED_PER_STRAND, MAPQ_RAISED_FROM_0)
    assert fx.total == int(fx.joins["joined"].sum()) == JOINED_READS
    assert (fx.sub != 0).any() and (fx.joins["top2"] < fx.places["top2"]).any()  # a joined suboptimal item: top2 falls, not top1
    # the reads on a bubble record (the lines with a bC tag in the reference's padded SAM): 447, 195 of them at MAPQ 0, all 195 raised
    on_bubble = pad_model.expected_loci(fx.places, fx.t.start, fx.t.end, fx.t.bub_of, fx.t.bubbles)["bubble"] >= 0
    mapped = (fx.places["flags"] & bw.PLACE_MAPPED) != 0
    assert (int(on_bubble.sum()), int((on_bubble & mapped & (fx.places["mapq"] == 0)).sum()), int((on_bubble & raised).sum()), int((~on_bubble & raised).sum())) == (447, 195, 195, 64)


def test_bubble_placed_count_is_the_references(pad_text):
    lines = [ln.split(b"\t") for ln in open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read().split(b"\n") if b"\tbC:Z:" in ln]
    assert (len(lines), sum(1 for f in lines if f[4] == b"0")) == (447, 195)


def test_no_mapq_falls_and_reads_without_items_keep_theirs(fx):
    assert (fx.joins["mapq"] >= fx.places["mapq"]).all()
    none = np.diff(fx.off) == 0
    assert none.sum() > 100 and (fx.joins["joined"][none] == 0).all()
    for f in ("top1", "top2", "mapq"):
        assert (fx.joins[f][none] == fx.places[f][none]).all(), f
    unmapped = (fx.places["flags"] & bw.PLACE_MAPPED) == 0
    assert unmapped.any() and fx.joins[unmapped].tobytes() == bytes(16 * int(unmapped.sum()))
    assert (np.diff(fx.off) <= 1).all()  # no read of this fixture has more than one item: the same records for every -X


def model_text(fx, golden, pad_text):
    """the reference's SAM with the model's X tags, its padded form, the MAPQ column and bJ applied; without them it is the reference's padded SAM"""
    ann = alt_model.read_ann(os.path.join(golden, "toy.fa.ann"))
    with_x = alt_model.expected_sam(open(os.path.join(pad_text, "pad_bub_n3.sam")).read(), fx.places, fx.off, fx.alts, ann).encode()
    padded = pad_model.pad_sam(with_x, fx.t.bubbles)
    strip = lambda b: re.sub(rb"\tX0:i:[^\n]*?(?=\tbC:Z:|\n)", b"", b)
    assert strip(padded) == open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read()
    return padded, join_model.apply_to_sam(padded, fx.places, fx.joins)


def test_formatter_writes_the_models_text(built, golden, pad_text, fx, tmp_path):
    """`places2sam -B -J` fed the model's records == the model's text; without -J today's bytes; bJ is the last tag, behind bP"""
    pf, af, out = tmp_path / "places.bin", tmp_path / "alts.bin", tmp_path / "out.sam"
    fx.places.tofile(pf)
    af.write_bytes(join_model.alts_file_bytes(fx.off, fx.alts, fx.sub))
    fa, fq, data = os.path.join(golden, "toy.fa"), os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    padded, want = model_text(fx, golden, pad_text)
    r = run(["places2sam", "-B", data, "-J", fa, fq, pf, out, af])
    assert r.returncode == 0, r.stdout
    got = open(out, "rb").read()
    assert got == want
    lines = [ln for ln in got.split(b"\n") if b"\tbJ:i:" in ln]
    assert len(lines) == JOINED_READS and all(re.search(rb"\tbJ:i:1$", ln) for ln in lines)
    assert any(b"\tbP:Z:" in ln and ln.index(b"\tbP:Z:") < ln.index(b"\tbJ:i:") for ln in lines) and any(b"\tbP:Z:" not in ln for ln in lines)
    r = run(["places2sam", "-B", data, fa, fq, pf, out, af])
    assert r.returncode == 0 and open(out, "rb").read() == padded


def test_host_rule_on_records_out_of_text_order(built, golden, pad_text, fx, tmp_path):
    """an .ann whose records do not ascend (what `map -B -J` resolves on the host): the same lines"""
    pf, af, out = tmp_path / "places.bin", tmp_path / "alts.bin", tmp_path / "out.sam"
    fx.places.tofile(pf)
    af.write_bytes(join_model.alts_file_bytes(fx.off, fx.alts, fx.sub))
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), "-J", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), pf, out, af])
    assert r.returncode == 0, r.stdout
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"@")]
    assert body(open(out, "rb").read()) == body(model_text(fx, golden, pad_text)[1])


def test_join_without_its_inputs_is_refused(built, golden, pad_text, fx, tmp_path):
    """-J without -X or without -B: an error that names what is missing, exit 1, no file - before anything is loaded, so without a GPU"""
    fa, fq, data = os.path.join(golden, "toy.fa"), os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    aln, out, pf = os.path.join(pad_text, "pad_bub_n3.aln"), tmp_path / "x.sam", tmp_path / "places.bin"
    fx.places.tofile(pf)
    for cmd, tail in ((["map", "-n", "3"], [fa, fq, out]), (["aln2sam"], [fa, fq, aln, out])):
        for flags, missing, present in ((["-J"], ["-X", "-B"], []), (["-X", "5", "-J"], ["-B"], ["-X"]), (["-B", data, "-J"], ["-X"], ["-B"])):
            r = run(cmd + flags + tail)
            assert r.returncode == 1 and "-J needs" in r.stdout, r.stdout
            said = r.stdout.split("-J needs")[1]
            assert all(m in said for m in missing) and not any(p in said for p in present), r.stdout
            assert not out.exists()
    r = run(["places2sam", "-B", data, "-J", fa, fq, pf, out])  # no items file
    assert r.returncode == 1 and "-J needs -X" in r.stdout and not out.exists()
    r = run(["places2sam", "-J", fa, fq, pf, out, pf])
    assert r.returncode == 1 and "-B" in r.stdout.split("-J needs")[1] and not out.exists()
    # an items file without the suboptimal bytes
    af = tmp_path / "alts.bin"
    af.write_bytes(alt_model.alts_file_bytes(fx.off, fx.alts))
    r = run(["places2sam", "-B", data, "-J", fa, fq, pf, out, af])
    assert r.returncode != 0 and "suboptimal byte" in r.stdout


BAD_CHROMOSOMES = {
    "missing": (lambda ann, data: (ann.replace("chr3 synthetic", "chrX synthetic"), data), "bubble 0", "0 .ann records are named \"chr3\""),
    "ambiguous": (lambda ann, data: (ann.replace("chr1 synthetic", "chr2 other"), data), "bubble 1", "2 .ann records are named \"chr2\""),
    "a_bubble_record": (lambda ann, data: (ann, data.replace("chr1 synthetic seed=7", "bubble2 synthetic seed=7")), "bubble 3", "is itself a bubble record"),
}


@pytest.mark.parametrize("name", list(BAD_CHROMOSOMES))
def test_bubble_without_one_chromosome_record_is_refused_and_named(built, golden, pad_text, fx, tmp_path, name):
    edit, which, why = BAD_CHROMOSOMES[name]
    ann, data = edit(open(os.path.join(golden, "toy.fa.ann")).read(), open(os.path.join(golden, "pad_toy.data")).read())
    (tmp_path / "toy.fa.ann").write_text(ann)
    (tmp_path / "t.data").write_text(data)
    pf, af, out = tmp_path / "places.bin", tmp_path / "alts.bin", tmp_path / "out.sam"
    fx.places.tofile(pf)
    af.write_bytes(join_model.alts_file_bytes(fx.off, fx.alts, fx.sub))
    fq = os.path.join(pad_text, "pad_bub.fq")
    r = run(["places2sam", "-B", tmp_path / "t.data", "-J", tmp_path / "toy.fa", fq, pf, out, af])
    assert r.returncode != 0 and which in r.stdout and why in r.stdout, r.stdout
    assert not out.exists()
    r = run(["places2sam", "-B", tmp_path / "t.data", tmp_path / "toy.fa", fq, pf, out, af])  # without -J the table is good enough
    assert r.returncode == 0, r.stdout
    names = [ln.split("\t")[0] for ln in ann.split("\n")[1:] if ln]
    anns, _ = bw.read_bubble_data(tmp_path / "t.data")
    with pytest.raises(ValueError, match=which):
        bw.bubble_chrom_of(names, anns)


def test_python_helper_equals_the_model(golden, fx):
    anns, _ = bw.read_bubble_data(os.path.join(golden, "pad_toy.data"))
    assert bw.bubble_chrom_of(fx.t.names, anns).tolist() == fx.t.chrom.tolist() == [2, 1, 1, 0]


def test_usage_names_the_flag(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-J]" in r.stdout and "bJ:i:" in r.stdout
    assert "-J" in run(["aln2sam"]).stdout and "[-J]" in run(["places2sam"]).stdout


def test_join_layout_matches_the_header(built, tmp_path):
    """bwb_join as the C compiler sees it == JOIN_DTYPE: size and every field's offset"""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bwb_join));']
    for f in bw.JOIN_DTYPE.names:
        lines.append(f'printf("{f} %zu\\n", offsetof(bwb_join, {f}));')
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["size"]) == bw.JOIN_DTYPE.itemsize == 16
    for f in bw.JOIN_DTYPE.names:
        assert int(got[f]) == bw.JOIN_DTYPE.fields[f][1], f
    assert sum(bw.JOIN_DTYPE.fields[f][0].itemsize for f in bw.JOIN_DTYPE.names) == 16
