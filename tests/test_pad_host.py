"""Bubble hits in reference coordinates without a GPU: `bwbble sampad` and the Python model against the bytes the REFERENCE's sam_pad wrote
(tests/golden/make_golden_pad.py), the branches the fixture exists for, the SAM formatter with tags fed with placement records computed in
Python (`places2sam -B`: the formatter of `map -B` and the host's resolver), the refusals where the reference's behaviour is undefined, and
the layout of the two new records of the C-ABI."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bwbble_amd as bw
import map_model
import oracle_lib
import pad_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pad_text(tmp_path_factory):
    """the pad_bub fixture (committed gzipped) as plain files"""
    return pad_model.unpack(tmp_path_factory.mktemp("pad"))


def run(args, **kw):
    return subprocess.run([bw.HOST_BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


def cases(golden, pad_text):
    return {"synth": (os.path.join(golden, "pad_synth.data"), os.path.join(golden, "pad_synth.sam"), os.path.join(golden, "pad_synth.pad.sam")),
            "bub_n3": (os.path.join(golden, "pad_toy.data"), os.path.join(pad_text, "pad_bub_n3.sam"), os.path.join(pad_text, "pad_bub_n3.pad.sam"))}


@pytest.mark.parametrize("name", ["synth", "bub_n3"])
def test_sampad_writes_the_references_bytes(built, golden, pad_text, tmp_path, name):
    data, sam, want = cases(golden, pad_text)[name]
    out = tmp_path / "out.sam"
    r = run(["sampad", data, sam, out])
    assert r.returncode == 0, r.stdout
    assert open(out, "rb").read() == open(want, "rb").read()


@pytest.mark.parametrize("name", ["synth", "bub_n3"])
def test_model_writes_the_references_bytes(golden, pad_text, name):
    """this pins the model, which then judges the GPU's records"""
    data, sam, want = cases(golden, pad_text)[name]
    assert pad_model.pad_sam(open(sam, "rb").read(), pad_model.load_bubbles(data)) == open(want, "rb").read()


def test_synthetic_fixture_ends_without_a_newline_and_its_output_with_one(golden):
    assert not open(os.path.join(golden, "pad_synth.sam"), "rb").read().endswith(b"\n")
    out = open(os.path.join(golden, "pad_synth.pad.sam"), "rb").read()
    assert out.endswith(b"\n") and b"bP:Z:207-206\n" in out and b"bP:Z:5124-5124\n" in out  # a range below itself (ref_len 0), and one of one position
    assert max(int(ln.rsplit(b"bP:Z:", 1)[1].split(b"-")[0]) for ln in out.split(b"\n") if b"bP:Z:" in ln) > 2**35


def test_fixture_reaches_every_branch_on_both_strands(golden, pad_text):
    """the committed pad_bub files: at least 8 reads on the left flank, the right flank and in between (a range), forward and reverse; at
    least 50 mapped reads off the bubbles; an unmapped read"""
    bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
    census = pad_model.classify(open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read(), bubbles)
    for case in ("left", "right", "range"):
        for strand in ("fwd", "rev"):
            assert census.get((case, strand), 0) >= 8, (case, strand, census)
    assert census.get(("plain", None), 0) >= 50, census
    assert census.get(("unmapped", None), 0) >= 1, census


@pytest.fixture(scope="module")
def bub_places(golden, oracle, pad_text, tmp_path_factory):
    """placement records computed in Python from the reference's .aln and the oracle's SA, in a file"""
    idx = oracle.load_index(os.path.join(golden, "toy.fa.bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(pad_text, "pad_bub_n3.aln"), "rb").read())
    places, _ = map_model.expected_places(oracle, idx, reads, 6)
    pf = tmp_path_factory.mktemp("places") / "places.bin"
    places.tofile(pf)
    return places, pf


def test_formatter_with_tags_writes_the_references_padded_sam(built, golden, pad_text, bub_places, tmp_path):
    """`places2sam -B` (sam_format_reads with locus records from the host resolver) -> the reference's aln2sam + sam_pad, byte for byte; and
    without -B the reference's aln2sam alone"""
    _, pf = bub_places
    fa, fq = os.path.join(golden, "toy.fa"), os.path.join(pad_text, "pad_bub.fq")
    out = tmp_path / "out.sam"
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), fa, fq, pf, out])
    assert r.returncode == 0, r.stdout
    assert open(out, "rb").read() == open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read()
    r = run(["places2sam", fa, fq, pf, out])
    assert r.returncode == 0, r.stdout
    assert open(out, "rb").read() == open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read()


def test_host_resolver_on_records_out_of_text_order(built, golden, pad_text, bub_places, tmp_path):
    """an .ann whose records are not ascending takes the linear search (what `map -B` falls back to): the same lines"""
    _, pf = bub_places
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    out = tmp_path / "out.sam"
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), pf, out])
    assert r.returncode == 0, r.stdout
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"@")]
    assert body(open(out, "rb").read()) == body(open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read())


def test_model_loci_give_the_references_tags(golden, pad_text, bub_places):
    """expected_loci (the judge of kernel k_locus) on the same records: its record names, positions and tags are the padded SAM's"""
    places, _ = bub_places
    names, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
    bubbles = pad_model.load_bubbles(os.path.join(golden, "pad_toy.data"))
    loci = pad_model.expected_loci(places, start, end, pad_model.bubble_of(names, bubbles), bubbles)
    assert (pad_model.bubble_of(names, bubbles) == bw.bubble_of(names, len(bubbles))).all()
    recs = [ln.split(b"\t") for ln in open(os.path.join(pad_text, "pad_bub_n3.pad.sam"), "rb").read().split(b"\n") if ln and ln[:1] != b"@"]
    assert len(recs) == len(loci)
    for f, lc in zip(recs, loci):
        if int(f[1]) & 4:
            assert (lc["seqid"], lc["pos1"], lc["bubble"], lc["kind"]) == (-1, 0, -1, 0)
            continue
        assert names[lc["seqid"]].encode() == f[2] and lc["pos1"] == int(f[3])
        tail = b"\t".join(f[11:])
        if lc["bubble"] < 0:
            assert tail == b"" and lc["kind"] == 0
        else:
            bp = b"%d" % lc["ref_lo"] if lc["kind"] == bw.LOCUS_POINT else b"%d-%d" % (lc["ref_lo"], lc["ref_hi"])
            assert tail == b"bC:Z:" + bubbles[lc["bubble"]][0] + b"\tbP:Z:" + bp


def test_python_reader_of_the_bubble_table(golden, tmp_path):
    anns, recs = bw.read_bubble_data(os.path.join(golden, "pad_synth.data"))
    want = pad_model.load_bubbles(os.path.join(golden, "pad_synth.data"))
    assert [a.encode() for a in anns] == [b[0] for b in want] and recs.tobytes() == pad_model.bubble_records(want).tobytes()
    (tmp_path / "odd.data").write_text("chr1\n1 2 3 4 5 6\nchr2\n")
    with pytest.raises(ValueError, match="odd"):
        bw.read_bubble_data(tmp_path / "odd.data")
    with pytest.raises(ValueError, match="outside"):
        bw.bubble_of(["chr1", "bubble9 chr1 5"], 4)


REFUSED_TABLES = {
    "odd_line_count": ("chr1 x\n1\t2\t3\t4\t0\t1\nchr2 y\n", "odd number of lines", "line 3"),
    "five_numbers": ("chr1 x\n1\t2\t3\t4\t0\t1\nchr2 y\n5\t6\t7\t8\t0\n", "six integers", "line 4"),
    "not_a_number": ("chr1 x\n1\t2\tthree\t4\t0\t1\n", "six integers", "line 2"),
}


@pytest.mark.parametrize("name", list(REFUSED_TABLES))
def test_refused_bubble_tables(built, golden, tmp_path, name):
    text, what, where = REFUSED_TABLES[name]
    data, out = tmp_path / "bad.data", tmp_path / "out.sam"
    data.write_text(text)
    r = run(["sampad", data, os.path.join(golden, "pad_synth.sam"), out])
    assert r.returncode != 0 and what in r.stdout and where in r.stdout, r.stdout
    assert not out.exists()


def test_refused_sam_lines(built, golden, tmp_path):
    """a bubble outside the table and a line without a POS field: non-zero exit, the line named, no output file left behind"""
    data, out = os.path.join(golden, "pad_toy.data"), tmp_path / "out.sam"
    head = "@PG\tID:x\nr0\t0\tbubble3 chr1 56976\t5\t37\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n"
    for bad, what in (("r1\t0\tbubble9 chr1 7\t5\t37\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n", "outside the table of 4 bubbles"),
                      ("r1\t0\tbubble-1\t5\t37\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n", "outside the table of 4 bubbles"),
                      ("r1\t0\tbubble1\n", "fewer than four fields"), ("\n", "fewer than four fields")):
        sam = tmp_path / "in.sam"
        sam.write_text(head + bad)
        r = run(["sampad", data, sam, out])
        assert r.returncode != 0 and what in r.stdout and "line 3" in r.stdout, r.stdout
        assert not out.exists()
    sam.write_text(head)
    assert run(["sampad", data, sam, out]).returncode == 0 and open(out, "rb").read().endswith(b"\tbC:Z:chr1 synthetic seed=7\tbP:Z:56857\n")


def test_record_naming_a_bubble_outside_the_table_is_refused_at_load_time(built, golden, pad_text, bub_places, tmp_path):
    """`bubble9` in the .ann with four bubbles in the table: -B stops before any SAM file exists, naming the record"""
    _, pf = bub_places
    ann = open(os.path.join(golden, "toy.fa.ann")).read().replace("bubble3 chr1", "bubble9 chr1")
    (tmp_path / "toy.fa.ann").write_text(ann)
    out = tmp_path / "out.sam"
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), pf, out])
    assert r.returncode != 0 and "record 6" in r.stdout and "bubble9 chr1 56976" in r.stdout and "outside the table of 4 bubbles" in r.stdout, r.stdout
    assert not out.exists()


def test_usage_names_the_new_command_and_flag(built):
    assert "sampad" in run([]).stdout
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "-B <bubble.data>" in r.stdout
    assert "-B" in run(["aln2sam"]).stdout
    assert "Usage: bwbble sampad <bubble.data>" in run(["sampad"]).stdout


def test_map_with_a_refused_table_leaves_no_file(built, golden, tmp_path):
    """the table is loaded before anything else: this needs no GPU"""
    for ext in ("", ".bwt", ".ann"):
        shutil.copy(os.path.join(golden, "toy.fa" + ext), tmp_path / ("toy.fa" + ext))
    (tmp_path / "bad.data").write_text("chr1\n1 2 3\n")
    out = tmp_path / "x.sam"
    for cmd in (["map", "-n", "3", "-B", tmp_path / "bad.data", tmp_path / "toy.fa", os.path.join(golden, "toy.fq"), out],
                ["aln2sam", "-B", tmp_path / "bad.data", tmp_path / "toy.fa", os.path.join(golden, "toy.fq"), os.path.join(golden, "toy_n3.aln"), out]):
        r = run(cmd)
        assert r.returncode != 0 and "six integers" in r.stdout, r.stdout
        assert not out.exists()


def test_bubble_and_locus_layouts_match_the_header(built, tmp_path):
    """bwb_bubble / bwb_locus as the C compiler sees them == BUBBLE_DTYPE / LOCUS_DTYPE: size and every field's offset"""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {']
    for st, dt in (("bwb_bubble", bw.BUBBLE_DTYPE), ("bwb_locus", bw.LOCUS_DTYPE)):
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f in dt.names:
            lines.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    lines += ['printf("point %d\\n", BWB_LOCUS_POINT);', 'printf("range %d\\n", BWB_LOCUS_RANGE);', 'return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    for st, dt, size in (("bwb_bubble", bw.BUBBLE_DTYPE, 40), ("bwb_locus", bw.LOCUS_DTYPE, 32)):
        assert int(got[st]) == dt.itemsize == size
        for f in dt.names:
            assert int(got[f"{st}.{f}"]) == dt.fields[f][1], (st, f)
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == size  # every byte of the record belongs to a field
    assert (int(got["point"]), int(got["range"])) == (bw.LOCUS_POINT, bw.LOCUS_RANGE)
