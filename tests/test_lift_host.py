"""Placements on bubble records in chromosome coordinates (`-R`) without a GPU: the model (tests/lift_model.py) on the pad_bub lines - the
census the documents quote, and the mismatch count of every lifted line against the chromosome -, the model against the judge that knows
the records' cmap only, the SAM formatter and the host's rule fed with the model's records (`places2sam -B -R`), the refusals, and the
layout of the new record of the C-ABI."""
import os
import re
import subprocess
import types
from collections import Counter

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import join_model
import lift_model
import map_model
import oracle_lib
import pad_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = {"MIM": 221, "M": 195, "SM": 24, "MS": 7}  # the 447 bubble-placed lines of pad_bub_n3.sam


def run(args, **kw):
    return subprocess.run([bw.HOST_BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


@pytest.fixture(scope="module")
def pad_text(tmp_path_factory):
    return pad_model.unpack(tmp_path_factory.mktemp("lift"))


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
    joins, _ = join_model.expected_joins(places, off, alts, sub, t.start, t.end, t.bub_of, t.bubbles, t.chrom, 6)
    return types.SimpleNamespace(reads=reads, places=places, off=off, alts=alts, sub=sub, joins=joins, t=t)


def toy_chromosomes(golden):
    out, name = {}, None
    for ln in open(os.path.join(golden, "toy.fa")).read().split("\n"):
        if ln.startswith(">"):
            name = ln[1:]
            out[name] = []
        elif name:
            out[name].append(ln)
    return {k: "".join(v) for k, v in out.items()}


def shape(cigar):
    return "".join(op for _, op in lift_model.parse_cigar(cigar))


def test_census_and_mismatches_of_the_pad_bub_lines(golden, pad_text, fx):
    """all 447 bubble-placed lines lift, with the shapes the documents quote; and for every one the mismatches of SEQ under the lifted M ops
    against the chromosome of toy.fa equal the mismatches of the original line against the bubble record"""
    text = open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read()
    got, lifted, unliftable = lift_model.lift_sam(text, fx.t.bubbles, fx.t.names, fx.t.chrom)
    seqs = toy_chromosomes(golden)
    before = [ln.split(b"\t") for ln in text.split(b"\n") if ln and ln[:1] != b"@"]
    after = [ln.split(b"\t") for ln in got.split(b"\n") if ln and ln[:1] != b"@"]
    assert len(before) == len(after) and (lifted, unliftable) == (447, 0)
    census = Counter()
    for b, a in zip(before, after):
        if not a[-1].startswith(b"bO:Z:"):
            assert a == b
            continue
        census[shape(a[5].decode())] += 1
        rec, pos1, cig = a[-1][5:].decode().rsplit(",", 2)
        assert (rec, pos1, cig) == (b[2].decode().split()[0], b[3].decode(), b[5].decode())
        seq = a[9].decode()
        on_record = lift_model.mismatches(seqs[b[2].decode()], int(pos1), cig, seq)
        on_chromosome = lift_model.mismatches(seqs[a[2].decode()], int(a[3]), a[5].decode(), seq)
        assert on_record == on_chromosome, a[0]
        assert a[:2] + a[4:5] + a[6:11] == b[:2] + b[4:5] + b[6:11]
    assert dict(census) == CENSUS
    # the flanks of the four toy bubbles are the chromosome's at the table's coordinates, and no record skips anything
    for k, (ann, A, Bm, C, Dm, _, alt) in enumerate(fx.t.bubbles):
        rec = seqs[next(n for n in fx.t.names if n.startswith(f"bubble{k} "))]
        chrom = seqs[ann.decode()]
        assert C - A - Bm == 0 and rec[:Bm] == chrom[A - 1:A - 1 + Bm] and rec[Bm + alt:Bm + alt + Dm + 1] == chrom[C - 1:C + Dm]


@pytest.fixture(scope="module")
def gen():
    g = lift_model.genome()
    return g, lift_model.reads(g)


def test_model_equals_the_cmap_judge_on_generated_reads(gen):
    """every generated read at the position it was cut from: the rule's POS and CIGAR are what the record's cmap dictates, an error-free read
    has no mismatch against the chromosome under its M ops, and every bubble kind and CIGAR shape of the rule occurs"""
    g, reads = gen
    gaps = sorted({b[3] - b[1] - b[2] for b in g["bubbles"]})
    assert gaps == [0, 1, 2, 7, 130] and any(b[4] == -1 for b in g["bubbles"]) and any(b[2] < 124 for b in g["bubbles"])
    assert any(b[3] - b[1] - b[2] == 1 and b[5] == 0 for b in g["bubbles"])  # the `.` allele: gap 1, ref_len 0
    assert any(c not in "ACGT" for c in g["chrom"]) and not any("N" in r[6] for r in reads)
    shapes = Counter()
    for name, k, o, ln, strand, edit, seq, cig in reads:
        got = lift_model.lift(g["bubbles"][k], o + 1, cig)
        assert got == lift_model.judge(g["records"][k][2], o + 1, cig), name
        shapes[shape(got[1]) if got else None] += 1
        if got and edit is None:
            assert lift_model.mismatches(g["chrom"], got[0], got[1], seq) == 0, name
    for s in ("M", "MIM", "MDM", "MIDM", "SM", "MS"):
        assert shapes[s] >= 8, (s, shapes)
    assert shapes[None] == 0 and {r[3] for r in reads} == {60, 100} and {r[4] for r in reads} == {"+", "-"}


def test_rule_edges():
    """a span inside the allele alone, a span that leaves the record by one, position 0, a D run over the whole allele, an I run that ends at
    the allele's edge, and a gap longer than a gap run can say"""
    b = (b"c", 100, 10, 111, 10, 0, 3)  # pad_synth's first bubble: gap 1, ref_len 0; reclen 24
    assert lift_model.lift(b, 11, "3M") is None and lift_model.lift(b, 12, "1M") is None
    assert lift_model.lift(b, 5, "20M") == (104, "6M3I1D11M") and lift_model.lift(b, 5, "21M") is None and lift_model.lift(b, 0, "5M") is None
    assert lift_model.lift(b, 1, "10M3D11M") == (100, "10M1D11M")
    assert lift_model.lift(b, 8, "3M2I3M4M") == (107, "3M5I1D4M")
    assert lift_model.lift(b, 11, "3M2M") == (111, "3S2M") and lift_model.lift(b, 9, "2M3M") == (108, "2M3S")
    assert lift_model.lift(b, 14, "5M") == (111, "5M") and lift_model.lift(b, 13, "6M") == (111, "1S5M")
    far = (b"c", 100, 10, 110 + (1 << 28) - 1, 10, 0, 0)
    assert lift_model.lift(far, 10, "1M1D2M") == (109, f"1M{(1 << 28) - 1}D1D2M") and lift_model.refusal(far) is None


def test_host_rule_called_by_itself_on_positions_no_locus_gives(built, tmp_path):
    """`pad.c: lift_resolve` in a program of its own, with the same compiler flags as the tool plus the address and undefined-behaviour
    sanitizers: a printed position below 1 - which neither k_locus nor locus_resolve ever gives a placement on a bubble record, so the tools
    and the kernels cannot be fed it - is not liftable; and the rule's edge cases give the model's answers"""
    b = (b"c", 100, 10, 111, 10, 0, 3)
    cases = [(0, "5M"), (-3, "5M"), (1, "5M"), (5, "20M"), (5, "21M"), (11, "3M"), (11, "3M2M"), (8, "3M2I3M4M"), (1, "10M3D11M"), (13, "6M")]
    rows = []
    for pos1, cig in cases:
        for rev in (0, 1):
            alen, runs = lift_model.gap_runs(cig, bool(rev))
            rows.append(f"{{ {pos1}, {rev}, {alen}, {{ {', '.join(str(r) for r in runs)} }} }}")
    src = tmp_path / "rule.c"
    src.write_text("""
#include <stdarg.h>
#include "bwb_host.h"
void bwb_die(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); exit(1); }
int sam_mapq(int top1, int top2, int num_mm, int max_mm) { (void)top1; (void)top2; (void)num_mm; (void)max_mm; return 0; }
static const struct { long long pos1; int rev; unsigned alen; uint16_t runs[8]; } cases[] = { %s };
int main(void) {
	const bwb_bubble b = { .A = 100, .B_minus_A = 10, .C = 111, .D_minus_C = 10, .ref_len = 0, .alt_len = 3 };
	for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); k++) {
		bwb_lift hdr;
		uint32_t ops[BWB_LIFT_MAX_OPS];
		const int n = lift_resolve(&b, 7, cases[k].pos1, cases[k].rev, cases[k].alen, cases[k].runs, &hdr, ops);
		if (!n) { printf("none\\n"); continue; }
		printf("%%lld %%d ", (long long)hdr.pos, (int)hdr.seqid);
		for (int i = 0; i < n; i++) printf("%%u%%c", ops[i] >> 4, "MID?S"[ops[i] & 15]);
		printf("\\n");
	}
	return 0;
}
""" % ",\n".join(rows))
    exe = tmp_path / "rule"
    host = os.path.join(ROOT, "bwbble_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", host,
                    str(src), os.path.join(host, "pad.c"), "-o", str(exe), "-lm"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    got = r.stdout.split("\n")[:-1]
    want = []
    for pos1, cig in cases:
        m = lift_model.lift(b, pos1, cig)
        want += ["none" if m is None else f"{m[0]} 7 {m[1]}"] * 2
    assert got == want and want[:4] == ["none"] * 4 and want[4] != "none"


def write_inputs(fx, tmp_path):
    pf, af = tmp_path / "places.bin", tmp_path / "alts.bin"
    fx.places.tofile(pf)
    af.write_bytes(join_model.alts_file_bytes(fx.off, fx.alts, fx.sub))
    return pf, af


def model_texts(fx, golden, pad_text):
    """the reference's SAM with the model's X tags, padded (-B) and joined (-J): the three texts -R is applied to"""
    ann = alt_model.read_ann(os.path.join(golden, "toy.fa.ann"))
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam")).read()
    with_x = alt_model.expected_sam(plain, fx.places, fx.off, fx.alts, ann).encode()
    padded_x = pad_model.pad_sam(with_x, fx.t.bubbles)
    return pad_model.pad_sam(plain.encode(), fx.t.bubbles), padded_x, join_model.apply_to_sam(padded_x, fx.places, fx.joins)


def test_formatter_writes_the_models_text(built, golden, pad_text, fx, tmp_path):
    """`places2sam -B -R` without items, with items, and with -J: the model's text; without -R the bytes it writes today; bO is the last tag"""
    pf, af = write_inputs(fx, tmp_path)
    out = tmp_path / "out.sam"
    fa, fq, data = os.path.join(golden, "toy.fa"), os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    padded, padded_x, joined = model_texts(fx, golden, pad_text)
    lift = lambda text: lift_model.lift_sam(text, fx.t.bubbles, fx.t.names, fx.t.chrom)[0]
    for flags, items, base in ((["-B", data], [], padded), (["-B", data], [af], padded_x), (["-B", data, "-J"], [af], joined)):
        r = run(["places2sam"] + flags + ["-R", fa, fq, pf, out] + items)
        assert r.returncode == 0, r.stdout
        got = open(out, "rb").read()
        assert got == lift(base), flags
        tagged = [ln for ln in got.split(b"\n") if b"\tbO:Z:" in ln]
        assert len(tagged) == 447 and all(re.search(rb"\tbO:Z:bubble\d,\d+,[0-9MID]+$", ln) for ln in tagged)
        assert all(ln.index(b"\tbP:Z:") < ln.index(b"\tbO:Z:") for ln in tagged)
        assert not any(ln.split(b"\t")[2].startswith(b"bubble") for ln in got.split(b"\n") if ln and ln[:1] != b"@")
        r = run(["places2sam"] + flags + [fa, fq, pf, out] + items)
        assert r.returncode == 0 and open(out, "rb").read() == base
    assert any(b"\tbJ:i:" in ln and ln.index(b"\tbJ:i:") < ln.index(b"\tbO:Z:") for ln in lift(joined).split(b"\n") if b"\tbO:Z:" in ln)
    # an item on a bubble record is written on the chromosome as well: no item names a bubble record any more
    assert b",bubble" not in b"".join(re.findall(rb"XA:Z:[^\t\n]*", b"," + lift(padded_x).replace(b"XA:Z:", b"XA:Z:,").replace(b";", b";,")))
    assert b"bubble" in b"".join(re.findall(rb"XA:Z:[^\t\n]*", padded_x))


def test_host_rule_on_records_out_of_text_order(built, golden, pad_text, fx, tmp_path):
    """an .ann whose records do not ascend (what `map -B -R` resolves on the host): the same lines"""
    pf, af = write_inputs(fx, tmp_path)
    out = tmp_path / "out.sam"
    lines = open(os.path.join(golden, "toy.fa.ann")).read().split("\n")
    lines[1], lines[5] = lines[5], lines[1]  # chr1 and bubble1 change places
    (tmp_path / "toy.fa.ann").write_text("\n".join(lines))
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), "-J", "-R", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), pf, out, af])
    assert r.returncode == 0, r.stdout
    body = lambda b: [ln for ln in b.split(b"\n") if not ln.startswith(b"@")]
    want = lift_model.lift_sam(model_texts(fx, golden, pad_text)[2], fx.t.bubbles, fx.t.names, fx.t.chrom)[0]
    assert body(open(out, "rb").read()) == body(want)


def test_host_rule_on_the_generated_genome(built, gen, tmp_path):
    """the generated reads placed where they were cut, through `fasta2ref` and `places2sam -B -R`: every line is lifted to the POS and CIGAR the
    judge derives from the record's cmap, on the chromosome's name, with the original placement in bO - the host's rule on every bubble kind,
    both strands, and reads with an inserted or a deleted base"""
    g, reads = gen
    (tmp_path / "gen.fa").write_text(g["fasta"])
    (tmp_path / "gen.data").write_bytes(g["data"])
    (tmp_path / "gen.fq").write_text(lift_model.fastq(reads))
    assert run(["fasta2ref", tmp_path / "gen.fa"]).returncode == 0
    names, start, _ = bw.read_ann(tmp_path / "gen.fa.ann")
    assert names == g["names"]
    places = lift_model.place_records([(int(start[1 + k]) + o, strand == "-", cig) for _, k, o, _, strand, _, _, cig in reads])
    places.tofile(tmp_path / "places.bin")
    r = run(["places2sam", "-B", tmp_path / "gen.data", "-R", tmp_path / "gen.fa", tmp_path / "gen.fq", tmp_path / "places.bin", tmp_path / "out.sam"])
    assert r.returncode == 0, r.stdout
    lines = [ln.split("\t") for ln in open(tmp_path / "out.sam").read().split("\n") if ln and ln[0] != "@"]
    assert len(lines) == len(reads)
    for f, (name, k, o, ln, strand, edit, seq, cig) in zip(lines, reads):
        pos, cigar = lift_model.judge(g["records"][k][2], o + 1, cig)
        assert (f[0], f[2], int(f[3]), f[5], f[9]) == (name, g["names"][0], pos, cigar, seq), name
        assert f[-1] == f"bO:Z:bubble{k},{o + 1},{cig}" and f[1] == ("16" if strand == "-" else "0"), name


BAD_TABLES = {  # the toy table with one number of bubble 2 changed: (column, value, what the message says)
    "gap_negative": (2, 11061, "overlap"),
    "gap_too_long": (2, 11062 + (1 << 28), "2^28"),
    "alt_len_negative": (5, -1, "alt_len"),
    "Bm_negative": (1, -1, "B_minus_A is negative"),
    "Dm_below_minus_one": (3, -2, "D_minus_C is below -1"),
}


@pytest.mark.parametrize("name", list(BAD_TABLES))
def test_refused_tables_name_their_bubble_and_leave_no_file(built, golden, pad_text, fx, tmp_path, name):
    col, value, why = BAD_TABLES[name]
    lines = open(os.path.join(golden, "pad_toy.data")).read().split("\n")
    nums = lines[5].split("\t")
    nums[col] = str(value)
    lines[5] = "\t".join(nums)
    (tmp_path / "t.data").write_text("\n".join(lines))
    bad = pad_model.load_bubbles(tmp_path / "t.data")
    assert [lift_model.refusal(b) for b in bad] == [None, None, True, None]
    pf, af = write_inputs(fx, tmp_path)
    out = tmp_path / "out.sam"
    fa, fq = os.path.join(golden, "toy.fa"), os.path.join(pad_text, "pad_bub.fq")
    r = run(["places2sam", "-B", tmp_path / "t.data", "-R", fa, fq, pf, out, af])
    assert r.returncode != 0 and "bubble 2 " in r.stdout and why in r.stdout and "(-R)" in r.stdout, r.stdout
    assert not out.exists()
    r = run(["places2sam", "-B", tmp_path / "t.data", fa, fq, pf, out, af])  # without -R the table is good enough
    assert r.returncode == 0, r.stdout


def test_bubble_without_a_chromosome_record_is_refused_with_R_too(built, golden, pad_text, fx, tmp_path):
    (tmp_path / "toy.fa.ann").write_text(open(os.path.join(golden, "toy.fa.ann")).read().replace("chr3 synthetic", "chrX synthetic"))
    pf, af = write_inputs(fx, tmp_path)
    out = tmp_path / "out.sam"
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), "-R", tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), pf, out])
    assert r.returncode != 0 and "bubble 0" in r.stdout and "0 .ann records are named \"chr3\"" in r.stdout and "(-R)" in r.stdout, r.stdout
    assert not out.exists()


def test_lift_without_the_table_is_refused(built, golden, pad_text, fx, tmp_path):
    """-R without -B: an error that names what is missing, exit 1, no file - before anything is loaded, so without a GPU"""
    fa, fq = os.path.join(golden, "toy.fa"), os.path.join(pad_text, "pad_bub.fq")
    aln, out, pf = os.path.join(pad_text, "pad_bub_n3.aln"), tmp_path / "x.sam", tmp_path / "places.bin"
    fx.places.tofile(pf)
    for cmd in (["map", "-n", "3", "-R", fa, fq, out], ["map", "-n", "3", "-X", "5", "-R", fa, fq, out], ["aln2sam", "-R", fa, fq, aln, out], ["places2sam", "-R", fa, fq, pf, out]):
        r = run(cmd)
        assert r.returncode == 1 and "-R needs -B" in r.stdout, r.stdout
        assert not out.exists()


def test_usage_names_the_flag(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-R]" in r.stdout and "bO:Z:" in r.stdout
    assert "-R" in run(["aln2sam"]).stdout and "[-R]" in run(["places2sam"]).stdout


def test_lift_layout_matches_the_header(built, tmp_path):
    """bwb_lift as the C compiler sees it == LIFT_DTYPE: size and every field's offset; and the op codes"""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bwb_lift));']
    for f in bw.LIFT_DTYPE.names:
        lines.append(f'printf("{f} %zu\\n", offsetof(bwb_lift, {f}));')
    lines.append('printf("codes %d,%d,%d,%d,%d,%d,%d,%d\\n", BWB_LIFT_M, BWB_LIFT_I, BWB_LIFT_D, BWB_LIFT_S, BWB_LIFT_MAX_OPS, BWB_LIFT_NONE, BWB_LIFT_LIFTED, BWB_LIFT_UNLIFTABLE);')
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["size"]) == bw.LIFT_DTYPE.itemsize == 16
    for f in bw.LIFT_DTYPE.names:
        assert int(got[f]) == bw.LIFT_DTYPE.fields[f][1], f
    assert sum(bw.LIFT_DTYPE.fields[f][0].itemsize for f in bw.LIFT_DTYPE.names) == 16
    assert got["codes"] == ",".join(str(v) for v in (bw.LIFT_M, bw.LIFT_I, bw.LIFT_D, bw.LIFT_S, bw.LIFT_MAX_OPS, bw.LIFT_NONE, bw.LIFT_LIFTED, bw.LIFT_UNLIFTABLE))
    assert (bw.LIFT_M, bw.LIFT_I, bw.LIFT_D, bw.LIFT_S, bw.LIFT_MAX_OPS) == (0, 1, 2, 4, 20)
