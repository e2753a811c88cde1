"""`bwbble map -X` / `aln2sam -X` without a GPU: the fixtures of tests/golden/make_golden_alt.py, the bwb_alt record's layout, the SAM
formatter fed with placement records and items computed in Python (tests/alt_model.py) from the reference's .aln files and the
reference's SA() values (developer command `places2sam` with its sixth argument), and the command line's -X."""
import os
import subprocess

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import map_model
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alt_hits_fixture_holds_every_case_it_exists_for(golden):
    """T = N + 1 and N + 2 for N = 1, 5, 255; wide primaries and wide middle hits; items with eight runs on both strands; item rows that are
    special for the walk; widths of 2^32 and more and U < L; an item in no record; reads without hits - make_golden_alt.check"""
    from golden.make_golden_alt import check
    reads = check(golden)
    assert len(reads) >= 150


def test_rep_gap_fixture_has_gapped_hits_at_several_loci(golden):
    from golden.make_golden_alt import check_rep_gap
    reads = check_rep_gap(golden)
    assert len(reads) == 40 and len(open(os.path.join(golden, "rep_gap.fq")).read().split("\n")) == 161


def test_rep_n3_counts_are_the_ones_the_tags_are_specified_with(golden):
    """60 of the 104 reads of rep_n3.aln have 2 <= T <= 6 (10 with 2, 45 with 3, 5 with 6), 45 of them through a hit wider than one row:
    -X 5 lists all of them, -X 4 drops exactly the five with T = 6"""
    from collections import Counter
    reads = oracle_lib.parse_aln(open(os.path.join(golden, "rep_n3.aln"), "rb").read())
    T = [alt_model.placements(e) for e in reads]
    assert len(reads) == 104
    assert Counter(t for t in T if 2 <= t <= 6) == {2: 10, 3: 45, 6: 5}
    assert sum(1 for t, e in zip(T, reads) if 2 <= t <= 6 and any(x["U"] > x["L"] for x in e)) == 45
    assert sum(1 for e in reads if alt_model.n_items(e, 5)) == 60 and sum(1 for e in reads if alt_model.n_items(e, 4)) == 55


def test_rep_sa_equals_the_oracles_walk_on_every_row(golden, oracle):
    """rep_sa.npy (the reference's SA() on every row) == the oracle's invPsi walk to the sampled SA of the .bwt file; and the step counts
    the model derives from the full suffix array alone == the lengths of those walks"""
    idx = oracle.load_index(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    sa = np.load(os.path.join(golden, "rep_sa.npy"))
    assert sa.dtype == np.dtype("<u4") and len(sa) == int(idx.contents.length)
    fsa = alt_model.FullSA(sa)
    assert int(fsa.isa[0]) == int(idx.contents.sa0_index)
    for row in range(len(sa)):
        assert int(oracle.lib.bwb_or_SA(idx, row)) == int(sa[row]), row
    osa = alt_model.OracleSA(oracle, idx)
    for row in list(range(0, 200)) + list(range(int(idx.contents.sa0_index) - 40, int(idx.contents.sa0_index) + 40)) + list(range(len(sa) - 100, len(sa))):
        assert fsa(row) == osa(row), row


def test_alt_record_layout_matches_the_header(built, tmp_path):
    """bwb_alt as the C compiler sees it == ALT_DTYPE: size and every field's offset"""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bwb_alt));']
    for f in bw.ALT_DTYPE.names:
        lines.append(f'printf("{f} %zu\\n", offsetof(bwb_alt, {f}));')
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["size"]) == bw.ALT_DTYPE.itemsize == 32
    for f in bw.ALT_DTYPE.names:
        assert int(got[f]) == bw.ALT_DTYPE.fields[f][1], f
    assert sum(bw.ALT_DTYPE.fields[f][0].itemsize for f in bw.ALT_DTYPE.names) == 32


def test_model_saturates_and_stops_at_the_limit():
    h = lambda L, U: dict(L=L, U=U)
    assert alt_model.placements([]) == 0 and alt_model.placements([h(5, 5)]) == 1 and alt_model.placements([h(5, 7), h(1, 1)]) == 4
    assert alt_model.placements([h(1, 2**64 - 1), h(1, 1)]) == alt_model.SAT and alt_model.placements([h(5, 5), h(7, 6)]) == alt_model.SAT
    assert alt_model.placements([h(0, 2**32)]) == 2**32 + 1
    ents = [h(5, 7), h(1, 1), h(9, 10)]  # T = 6
    assert [alt_model.n_items(ents, n) for n in (1, 4, 5, 6, 255)] == [0, 0, 5, 5, 5]
    assert alt_model.item_rows(ents, 5) == [(0, 6), (0, 7), (1, 1), (2, 9), (2, 10)]
    assert alt_model.n_items([h(5, 5)], 5) == 0  # one placement: nothing else to list
    assert alt_model.cigar(10, [2 | (3 << 8), 7 | (1 << 8) | 0x8000] + [0xFFFF] * 6, False) == "2M1D2M3I2M"
    assert alt_model.cigar(10, [2 | (3 << 8), 7 | (1 << 8) | 0x8000] + [0xFFFF] * 6, True) == "2M3I2M1D2M"


# name: (index, reads, .aln, base .sam (None: `places2sam` without items), aln2sam's -n)
CASES = {
    "rep_n3": ("rep.fa", "rep.fq", "rep_n3.aln", "rep_n3.sam", 6),
    "rep_n3_q3": ("rep.fa", "rep.fq", "rep_n3.aln", "rep_n3_q3.sam", 3),
    "rep_gap_n4": ("rep.fa", "rep_gap.fq", "rep_gap_n4.aln", None, 6),
    "alt_hits": ("rep.fa", "alt_hits.fq", "alt_hits.aln", None, 6),
}


def places2sam(golden, fa, fq, places, out, alts=None):
    subprocess.run([bw.HOST_BIN, "places2sam", os.path.join(golden, fa), fq, str(places), str(out)] + ([str(alts)] if alts else []), check=True, stdout=subprocess.DEVNULL)
    return open(out, "rb").read()


@pytest.mark.parametrize("max_alt", [1, 4, 5, 255])
@pytest.mark.parametrize("name", list(CASES))
def test_formatter_writes_the_models_tags(built, golden, oracle, tmp_path, name, max_alt):
    """placement records and items computed in Python from the reference's hits and SA values -> `places2sam` with the items file == the
    reference's SAM line (golden file, or the formatter's own text without items) + the model's tags; columns 1-11 unchanged"""
    fa, fq, aln, sam, max_mm = CASES[name]
    fqp = os.path.join(golden, fq)
    if name == "alt_hits":
        from golden.make_golden_alt import unpack_alt
        fqp = unpack_alt(tmp_path, golden)
    idx = oracle.load_index(os.path.join(golden, fa + ".bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(golden, aln), "rb").read())
    places, _ = map_model.expected_places(oracle, idx, reads, max_mm)
    off, alts, _ = alt_model.expected_alts(reads, max_alt, alt_model.rep_sa(golden))
    pf, af = tmp_path / "places.bin", tmp_path / "alts.bin"
    places.tofile(pf)
    af.write_bytes(alt_model.alts_file_bytes(off, alts))
    plain = places2sam(golden, fa, fqp, pf, tmp_path / "plain.sam")
    if sam:  # without the items file: today's bytes
        assert plain == open(os.path.join(golden, sam), "rb").read()
    got = places2sam(golden, fa, fqp, pf, tmp_path / "x.sam", af).decode()
    want = alt_model.expected_sam(plain.decode(), places, off, alts, alt_model.read_ann(os.path.join(golden, fa + ".ann")))
    assert got == want
    body = lambda t: [ln for ln in t.split("\n") if ln and not ln.startswith("@")]
    assert ["\t".join(ln.split("\t")[:11]) for ln in body(got)] == body(plain.decode())
    mapped = [ln for ln in body(got) if ln.split("\t")[1] != "4"]
    assert mapped and all(ln.split("\t")[11].startswith("X0:i:") and ln.split("\t")[12].startswith("X1:i:") for ln in mapped)
    assert all(len(ln.split("\t")) == 11 for ln in body(got) if ln.split("\t")[1] == "4")
    with_xa = sum(1 for ln in body(got) if "\tXA:Z:" in ln)
    assert with_xa == sum(1 for e in reads if alt_model.n_items(e, max_alt))
    if name.startswith("rep_n3"):
        assert with_xa == {1: 10, 4: 55, 5: 60, 255: 60}[max_alt]
    if name == "alt_hits" and max_alt == 255:  # an item in no record is left out, the ones around it stay
        assert any(ln.split("\tXA:Z:")[1].count(";") < n for ln, n in zip((l for l in body(got) if "\tXA:Z:" in l), (c for c in np.diff(off) if c)))
        assert any("," + "-" in ln and ",+" in ln for ln in body(got))


def test_places2sam_refuses_an_items_file_that_does_not_fit(built, golden, oracle, tmp_path):
    idx = oracle.load_index(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(golden, "rep_n3.aln"), "rb").read())
    places, _ = map_model.expected_places(oracle, idx, reads, 6)
    off, alts, _ = alt_model.expected_alts(reads, 5, alt_model.rep_sa(golden))
    pf, af = tmp_path / "places.bin", tmp_path / "alts.bin"
    places.tofile(pf)
    af.write_bytes(alt_model.alts_file_bytes(off, alts)[:-32])
    r = subprocess.run([bw.HOST_BIN, "places2sam", os.path.join(golden, "rep.fa"), os.path.join(golden, "rep.fq"), str(pf), str(tmp_path / "o.sam"), str(af)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "does not hold the records" in r.stdout


def test_usage_texts_name_the_option_and_bad_values_are_refused(built, golden, tmp_path):
    r = subprocess.run([bw.HOST_BIN, "map", "-n", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 1 and "Usage: bwbble map" in r.stdout and "-X" in r.stdout and "XA:Z:" in r.stdout
    r = subprocess.run([bw.HOST_BIN, "aln2sam"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 1 and "Usage: bwbble aln2sam" in r.stdout and "-X" in r.stdout
    fa, fq, aln = os.path.join(golden, "rep.fa"), os.path.join(golden, "rep.fq"), os.path.join(golden, "rep_n3.aln")
    for cmd in (["map", "-n", "3"], ["aln2sam"]):
        for bad in ("0", "256", "-1", "5x", ""):
            out = tmp_path / "o.sam"
            args = [bw.HOST_BIN] + cmd + ["-X", bad, fa, fq] + ([aln] if cmd[0] == "aln2sam" else []) + [str(out)]
            r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 1 and "-X takes a number from 1 to 255" in r.stdout, (cmd, bad, r.stdout[-300:])
            assert not out.exists()
