"""NM:i and MD:Z against the text (`-D`) without a GPU: the model and the judge that knows no emission order (tests/md_model.py) on the
reference's golden lines, plain and lifted, and on the generated genome of lift_model; the SAM formatter and the host's rule
(`places2sam ... -D` after `fasta2ref`) against the model's text, byte for byte; the refusals; the usage texts; the layout of the new record
of the C-ABI; and `md.c: md_resolve` in a program of its own under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, **kw):
    return subprocess.run([bw.HOST_BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


@pytest.fixture(scope="module")
def pad_text(tmp_path_factory):
    return pad_model.unpack(tmp_path_factory.mktemp("md"))


@pytest.fixture(scope="module")
def toy(golden):
    """the text of toy.fa from this side's own parser"""
    text, names, starts = md_model.fasta_text(open(os.path.join(golden, "toy.fa")).read())
    return types.SimpleNamespace(text=text, names=names, starts=starts)


@pytest.fixture(scope="module")
def ref(built, golden, tmp_path_factory):
    """toy.fa with the .ref and .ann `bwbble fasta2ref` writes beside it"""
    d = tmp_path_factory.mktemp("ref")
    shutil.copy(os.path.join(golden, "toy.fa"), d / "toy.fa")
    r = run(["fasta2ref", d / "toy.fa"])
    assert r.returncode == 0, r.stdout
    return str(d / "toy.fa")


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
    toy_reads = oracle_lib.parse_aln(open(os.path.join(golden, "toy_n3.aln"), "rb").read())
    toy_places, _ = map_model.expected_places(oracle, idx, toy_reads, 6)
    return types.SimpleNamespace(reads=reads, places=places, off=off, alts=alts, sub=sub, joins=joins, t=t, toy_places=toy_places)


def mapped_lines(sam):
    return [ln.split(b"\t") for ln in sam.split(b"\n") if ln and ln[:1] != b"@" and ln.split(b"\t")[1] != b"4"]


def both_judges(sam, toy):
    """the model's tags on SAM bytes, the judge on the tagged bytes -> (tagged bytes, census)"""
    tagged, census = md_model.tag_sam(sam, toy.text, toy.names, toy.starts)
    bad, n = md_model.judge_sam(tagged, toy.text, toy.names, toy.starts)
    assert not bad and n == census[md_model.OK], bad[:3]
    return tagged, census


def test_text_parser_agrees_with_the_ann_file(golden, toy):
    names, start, end = bw.read_ann(os.path.join(golden, "toy.fa.ann"))
    assert toy.names == names and toy.starts == [int(s) for s in start]
    assert all(toy.text[int(e)] == "$" for e in end) and toy.text.count("$") == len(names)
    assert any(c not in "ACGT$" for c in toy.text)  # the toy multi-genome holds IUPAC codes


def test_model_and_judge_on_the_golden_lines(golden, pad_text, fx, toy):
    """toy_n3.sam and the 571 pad_bub reads, plain and lifted: no mapped primary is NONE or TOO_LONG, the judge accepts every line, and on the
    unlifted lines the mismatches under M are the search's num_mm and NM is its mm + gapo + gape"""
    for sam, places, mapped in ((open(os.path.join(golden, "toy_n3.sam"), "rb").read(), fx.toy_places, 584), (open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read(), fx.places, 569)):
        _, census = both_judges(sam, toy)
        assert census == {md_model.NONE: 0, md_model.OK: mapped, md_model.TOO_LONG: 0}
        recs = [p for p in places if p["flags"] & bw.PLACE_MAPPED]
        lines = mapped_lines(sam)
        assert len(recs) == len(lines) == mapped
        for f, p in zip(lines, recs):
            _, nm, _, mm = md_model.line_md(f, toy.text, toy.names, toy.starts)
            assert mm == int(p["num_mm"]) and nm == int(p["num_mm"]) + int(p["num_gapo"]) + int(p["num_gape"]), f[0]
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read()
    lifted, n_lifted, _ = lift_model.lift_sam(pad_model.pad_sam(plain, fx.t.bubbles), fx.t.bubbles, fx.t.names, fx.t.chrom)
    tagged, census = both_judges(lifted, toy)
    assert n_lifted == 447 and census == {md_model.NONE: 0, md_model.OK: 569, md_model.TOO_LONG: 0}
    # a lifted line that carries the allele counts its I: NM is the mismatches under M and the inserted bases, and MD has no word for them
    with_i = [f for f in mapped_lines(tagged) if b"I" in f[5] and f[-1].startswith(b"bO:Z:")]
    assert len(with_i) == 221
    for f in with_i:
        ins = sum(n for n, op in md_model.parse_cigar(f[5].decode()) if op == "I")
        assert int(f[11][5:]) == ins + len(re.findall(r"(?<!\^)(?<![A-Z])[A-Z]", f[12][5:].decode())), f[0]


@pytest.fixture(scope="module")
def gen(built, tmp_path_factory):
    """the generated genome of lift_model with its reads placed where they were cut, after `fasta2ref`"""
    d = tmp_path_factory.mktemp("gen")
    g = lift_model.genome()
    reads = lift_model.reads(g)
    (d / "gen.fa").write_text(g["fasta"])
    (d / "gen.data").write_bytes(g["data"])
    (d / "gen.fq").write_text(lift_model.fastq(reads))
    assert run(["fasta2ref", d / "gen.fa"]).returncode == 0
    text, names, starts = md_model.fasta_text(g["fasta"])
    _, start, _ = bw.read_ann(d / "gen.fa.ann")
    assert names == g["names"] and starts == [int(s) for s in start]
    lift_model.place_records([(starts[1 + k] + o, strand == "-", cig) for _, k, o, _, strand, _, _, cig in reads]).tofile(d / "places.bin")
    return types.SimpleNamespace(g=g, reads=reads, dir=d, text=text, names=names, starts=starts)


def test_host_rule_on_the_generated_genome(gen):
    """every generated read, on its bubble record (`places2sam -D`) and lifted (`places2sam -B -R -D`): NM and MD are the model's, the judge
    accepts them, and the deletions of 1, 7 and 130, insertions, both strands and reads with an edited base all occur"""
    d = gen.dir
    seen = set()
    for flags in ([], ["-B", d / "gen.data", "-R"]):
        r = run(["places2sam"] + flags + ["-D", d / "gen.fa", d / "gen.fq", d / "places.bin", d / "out.sam"])
        assert r.returncode == 0, r.stdout
        lines = mapped_lines(open(d / "out.sam", "rb").read())
        assert len(lines) == len(gen.reads)
        for f, (name, k, o, ln, strand, edit, seq, cig) in zip(lines, gen.reads):
            if flags:
                pos, cigar = lift_model.lift(gen.g["bubbles"][k], o + 1, cig)
                start = gen.starts[0] + pos - 1
            else:
                cigar, start = cig, gen.starts[1 + k] + o
            ops = md_model.parse_cigar(cigar)
            kind, nm, mdt, mm = md_model.md(gen.text, start, ops, seq)
            assert kind == md_model.OK and (f[0].decode(), f[5].decode(), f[9].decode()) == (name, cigar, seq), name
            assert (f[11], f[12]) == (b"NM:i:%d" % nm, b"MD:Z:" + mdt.encode()), (name, f[11], f[12], nm, mdt)
            assert md_model.judge(gen.text, start, ops, seq, nm, mdt) is None, name
            if edit is None:
                assert mm == 0, name  # an error-free read has no mismatch, on the record and on the chromosome
            seen |= {("D", n) for n, op in ops if op == "D"} | {(op, strand) for _, op in ops} | {("edit", edit)}
            seen |= {("md^", len(m)) for m in re.findall(r"\^([A-Z]+)", mdt)}
    for want in (("D", 1), ("D", 7), ("D", 130), ("md^", 1), ("md^", 7), ("md^", 130), ("I", "+"), ("I", "-"), ("S", "+"), ("M", "-"), ("edit", "I"), ("edit", "D")):
        assert want in seen, want


def write_inputs(fx, tmp_path):
    pf, af = tmp_path / "places.bin", tmp_path / "alts.bin"
    fx.places.tofile(pf)
    af.write_bytes(join_model.alts_file_bytes(fx.off, fx.alts, fx.sub))
    return pf, af


def test_formatter_writes_the_models_text(ref, golden, pad_text, fx, toy, tmp_path):
    """`places2sam [-B t [-J] [-R]] -D`: the model's tags on the model's text, byte for byte, NM and MD directly behind QUAL; without -D the
    bytes it writes today"""
    pf, af = write_inputs(fx, tmp_path)
    out = tmp_path / "out.sam"
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    ann = alt_model.read_ann(os.path.join(golden, "toy.fa.ann"))
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam")).read()
    with_x = alt_model.expected_sam(plain, fx.places, fx.off, fx.alts, ann).encode()
    padded, padded_x = pad_model.pad_sam(plain.encode(), fx.t.bubbles), pad_model.pad_sam(with_x, fx.t.bubbles)
    joined = join_model.apply_to_sam(padded_x, fx.places, fx.joins)
    lift = lambda text: lift_model.lift_sam(text, fx.t.bubbles, fx.t.names, fx.t.chrom)[0]
    cases = (([], [], plain.encode()), ([], [af], with_x), (["-B", data], [], padded), (["-B", data], [af], padded_x), (["-B", data, "-J"], [af], joined),
             (["-B", data, "-R"], [], lift(padded)), (["-B", data, "-R"], [af], lift(padded_x)), (["-B", data, "-J", "-R"], [af], lift(joined)))
    for flags, items, base in cases:
        want, census = both_judges(base, toy)
        assert census[md_model.OK] == 569
        r = run(["places2sam"] + flags + ["-D", ref, fq, pf, out] + items)
        assert r.returncode == 0, r.stdout
        got = open(out, "rb").read()
        assert got == want, (flags, pad_model.first_difference(got, want))
        assert all(f[11].startswith(b"NM:i:") and f[12].startswith(b"MD:Z:") for f in mapped_lines(got))
        r = run(["places2sam"] + flags + [ref, fq, pf, out] + items)
        assert r.returncode == 0 and open(out, "rb").read() == base, flags
    # the XA items keep the search's NM
    assert re.findall(rb"XA:Z:[^\t\n]*", want) == re.findall(rb"XA:Z:[^\t\n]*", base)


@pytest.mark.parametrize("what", ["missing", "short", "long"])
def test_a_text_that_is_not_there_stops_the_run_and_leaves_no_file(ref, pad_text, fx, tmp_path, what):
    """.ref missing, or not 2 x n_fwd bytes: every command with -D names `bwbble fasta2ref`, exits 1 and leaves no SAM file"""
    for f in (".ann",) + ((".ref",) if what != "missing" else ()):
        shutil.copy(ref + f, tmp_path / ("toy.fa" + f))
    if what != "missing":
        n = os.path.getsize(tmp_path / "toy.fa.ref")
        with open(tmp_path / "toy.fa.ref", "r+b") as f:
            f.truncate(n - 1 if what == "short" else n + 2)
    fa, fq, out = tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "out.sam"
    pf, _ = write_inputs(fx, tmp_path)
    for cmd in (["places2sam", "-D", fa, fq, pf, out], ["aln2sam", "-D", fa, fq, os.path.join(pad_text, "pad_bub_n3.aln"), out], ["map", "-n", "3", "-D", fa, fq, out]):
        r = run(cmd)
        assert r.returncode == 1 and "bwbble fasta2ref" in r.stdout and "toy.fa.ref" in r.stdout, r.stdout
        assert ("missing" in r.stdout) == (what == "missing") and not out.exists()


def test_usage_names_the_flag(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-D]" in r.stdout and "NM:i:" in r.stdout and "MD:Z:" in r.stdout and "fasta2ref" in r.stdout
    assert "-D" in run(["aln2sam"]).stdout and "MD:Z:" in run(["aln2sam"]).stdout and "[-R] [-D]" in run(["places2sam"]).stdout


def test_md_layout_matches_the_header(built, tmp_path):
    """bwb_md as the C compiler sees it == MD_DTYPE: size and every field's offset; and the kinds"""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bwb_md));']
    for f in bw.MD_DTYPE.names:
        lines.append(f'printf("{f} %zu\\n", offsetof(bwb_md, {f}));')
    lines.append('printf("codes %d,%d,%d,%d\\n", BWB_MD_NONE, BWB_MD_OK, BWB_MD_TOO_LONG, BWB_MD_MAX_SPAN);')
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["size"]) == bw.MD_DTYPE.itemsize == 8
    for f in bw.MD_DTYPE.names:
        assert int(got[f]) == bw.MD_DTYPE.fields[f][1], f
    assert sum(bw.MD_DTYPE.fields[f][0].itemsize for f in bw.MD_DTYPE.names) == 8
    assert got["codes"] == ",".join(str(v) for v in (bw.MD_NONE, bw.MD_OK, bw.MD_TOO_LONG, bw.MD_MAX_SPAN)) == "0,1,2,4096"
    assert (md_model.NONE, md_model.OK, md_model.TOO_LONG, md_model.MAX_SPAN) == (bw.MD_NONE, bw.MD_OK, bw.MD_TOO_LONG, bw.MD_MAX_SPAN)


def edge_cases():
    """(text, [(start, CIGAR, SEQ as printed)]): a text of every code, and placements at the rule's edges"""
    text = "$" + md_model.LETTERS[1:] * 3 + "ACGT" * 40 + "$" + "ACGTRYKM" * 30 + "$"
    n = len(text)
    at = text.index("ACGT" * 40)
    exact = lambda a, ln: "".join(c if c in "ACGT" else md_model.MEMBERS[c][:1] or "A" for c in text[a:a + ln])
    flip = lambda s, i: s[:i] + ("C" if s[i] != "C" else "G") + s[i + 1:]
    # every read base x every text code, `$` among them, at both parities: the all-codes stretch from its `$` and from one behind it, and the
    # other two `$` - at an even and at an odd position - from the middle and at the end of a window
    cases = [(k, "15M", b * 15) for b in "ACGTN" for k in (0, 1, 2, text.index("$", 1) - 7, n - 15)]
    cases += [(0, "5M", "AAAAA"), (n - 5, "5M", "AAAAA"), (n - 4, "5M", "AAAAA"), (-1, "5M", "AAAAA"), (n, "1M", "A"), (n - 3, "2M2D", "AA")]  # position 0, the last, leaving by one
    for ln in (1, 2, 31, 32, 33, 100, 255):
        cases.append((at, f"{ln}M", exact(at, ln)[:ln] if ln <= 160 else "A" * ln))
    s = exact(at, 120)
    cases += [(at, "120M", flip(s, 0)), (at, "120M", flip(s, 119)), (at, "120M", flip(flip(s, 50), 51)), (at, "120M", flip(flip(s, 9), 19)), (at, "120M", flip(flip(s, 10), 110)),
              (at, "120M", flip(flip(s, 20), 120 - 1)), (at, "110M", flip(s[:110], 9)), (at, "110M", flip(s[:110], 10)), (at, "110M", flip(s[:110], 99)), (at, "110M", flip(s[:110], 100))]
    cases += [(at, "10M2D10M", s[:10] + flip(s[12:22], 0)), (at, "10M2I3D10M", s[:10] + "GG" + s[13:23]), (at, "10M3D2I10M", s[:10] + "GG" + s[13:23]), (at, "5M1D1I1D5M", s[:5] + "T" + s[7:12]),
              (at, "3S10M2S", "TTT" + s[:10] + "GG"), (at, "4M1I4M1D4M1I4M1D4M1I4M1D4M1I4M1D4M", "ACGTTACGTCGTATACGTCGTATACGTCGTATACGTCGTA"),
              (at, f"2M{md_model.MAX_SPAN - 3}D1M", "ACA"), (at, f"2M{md_model.MAX_SPAN - 2}D1M", "ACA"), (at, f"1M{(1 << 28) - 1}D1M", "AA"), (at, "5M", "ACGTA"[:4])]
    return text, cases


def test_host_rule_called_by_itself_under_the_sanitizers(built, tmp_path):
    """`md.c: md_resolve` in a program of its own, with the tool's compiler flags plus the address and undefined-behaviour sanitizers, on the
    edge cases - counted first, then written into a buffer of exactly the counted size, on both strands: the model's kind, NM and bytes"""
    text, cases = edge_cases()
    rows, want = [], []
    for start, cig, seq in cases:
        ops = md_model.parse_cigar(cig)
        for rev in (0, 1):
            fwd = seq[::-1].translate(md_model.COMP) if rev else seq  # the read as uploaded
            rows.append('{ %d, %d, %d, "%s", %d, { %s } }' % (start, rev, len(fwd), "".join(str("AGCTN".index(c)) for c in fwd), len(ops),
                                                               ", ".join(f"{(n << 4) | 'MID?S'.index(op)}u" for n, op in ops)))
            kind, nm, mdt, _ = md_model.md(text, start, ops, seq)
            want.append(f"{kind} {nm} {mdt}" if kind == md_model.OK else f"{kind}")
    src = tmp_path / "rule.c"
    src.write_text("""
#include <stdarg.h>
#include <string.h>
#include "bwb_host.h"
void bwb_die(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); exit(1); }
static const struct { long long start; int rev; unsigned len; const char *seq; unsigned n_ops; uint32_t ops[24]; } cases[] = { %s };
static const uint8_t text[] = { %s };
int main(void) {
	for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); k++) {
		uint8_t *seq = (uint8_t *)malloc(cases[k].len ? cases[k].len : 1);
		for (unsigned i = 0; i < cases[k].len; i++) seq[i] = (uint8_t)(cases[k].seq[i] - '0');
		bwb_md rec, again;
		const int kind = md_resolve(text, sizeof(text), seq, cases[k].len, cases[k].rev, cases[k].start, cases[k].ops, cases[k].n_ops, &rec, NULL, 0);
		if (kind != BWB_MD_OK) { printf("%%d\\n", kind); free(seq); continue; }
		char *md = (char *)malloc(rec.md_len ? rec.md_len : 1);
		if (md_resolve(text, sizeof(text), seq, cases[k].len, cases[k].rev, cases[k].start, cases[k].ops, cases[k].n_ops, &again, md, rec.md_len) != kind || memcmp(&rec, &again, sizeof(rec))) return 2;
		printf("%%d %%u %%.*s\\n", kind, rec.nm, (int)rec.md_len, md);
		free(md); free(seq);
	}
	return 0;
}
""" % (",\n".join(rows), ", ".join(str(c) for c in md_model.codes(text))))
    exe = tmp_path / "rule"
    host = os.path.join(ROOT, "bwbble_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", host,
                    str(src), os.path.join(host, "md.c"), "-o", str(exe), "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    got = r.stdout.split("\n")[:-1]
    assert got == want, [(c, g, w) for c, g, w in zip([c for c in cases for _ in (0, 1)], got, want) if g != w][:3]
    kinds = [w.split()[0] for w in want]
    assert kinds.count("0") >= 8 and kinds.count("2") == 4 and any("^" in w for w in want) and any(w.endswith(" 100") or " 100" in w for w in want)
    covered = set().union(*(md_model.pairs(text, start, md_model.parse_cigar(cig), seq) for start, cig, seq in cases))
    assert covered == md_model.ALL_PAIRS and text.index("$", 1) % 2 == 0 and (len(text) - 1) % 2 == 1, sorted(md_model.ALL_PAIRS - covered)
    # the judge on what the rule said
    for (start, cig, seq), w in zip([c for c in cases for _ in (0, 1)], want):
        if w[0] == "1":
            _, nm, mdt = w.split()
            assert md_model.judge(text, start, md_model.parse_cigar(cig), seq, int(nm), mdt) is None, (start, cig, seq, w)
