"""Allele counts at the text's IUPAC sites (`-A`) without a GPU: the model against the judge that knows no walk and no site numbering
(tests/pile_model.py) on the reference's golden lines, on the pad_bub reads plain and lifted, and on the generated genome of lift_model, with the
census; the host's rule and the writer (`places2sam ... -A f -a m`) against the model's bytes; the refusals; the usage texts; and `pile.c:
pile_host` in a program of its own under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import join_model
import lift_model
import md_model
import pad_model
import pile_model
from test_md_host import fx, gen, pad_text, ref, run, toy, write_inputs  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def census(text, table):
    """(sites counted, member bases, other bases) of a table {text position: [A, C, G, T]}"""
    member = sum(v[k] for pos, v in table.items() for k in range(4) if "ACGT"[k] in md_model.MEMBERS[text[pos]])
    return len(table), member, sum(sum(v) for v in table.values()) - member


def both(sam, fasta, text, names, starts, min_mapq=0):
    """the model's table of SAM bytes, after the judge has agreed with what the writer makes of it"""
    table, reads, adds = pile_model.pile_sam(sam, text, names, starts, min_mapq)
    written = pile_model.parse_tsv(pile_model.tsv(text, names, starts, table))
    judged = pile_model.judge_sam(sam, fasta, min_mapq)
    assert written == judged, sorted(set(written) ^ set(judged))[:5] or [k for k in written if written[k] != judged[k]][:5]
    assert adds == sum(sum(v) for v in table.values()) == sum(sum(v[1]) for v in judged.values())
    return table, reads


def lifted_text(plain, t):
    return lift_model.lift_sam(pad_model.pad_sam(plain, t.bubbles), t.bubbles, t.names, t.chrom)[0]


def test_model_and_judge_on_the_golden_lines(golden, pad_text, fx, toy):
    """toy_n3.sam and the 571 pad_bub reads, plain and lifted: the plain pileup equals the model at -a 0, 1, 37 and 255, and the census"""
    fasta = open(os.path.join(golden, "toy.fa")).read()
    assert (toy.text, toy.names, toy.starts) == pile_model.fasta_text(fasta)  # the two parsers agree
    assert len(pile_model.sites(toy.text)) == 2454
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read()
    texts = {"toy_n3": open(os.path.join(golden, "toy_n3.sam"), "rb").read(), "pad_bub": plain, "pad_bub lifted": lifted_text(plain, fx.t)}
    tables = {}
    for what, sam in texts.items():
        for q in (0, 1, 37, 255):
            table, reads = both(sam, fasta, toy.text, toy.names, toy.starts, q)
            if q == 0:
                tables[what] = table
                print(what, "reads", reads, "sites, member bases, other bases:", census(toy.text, table))
            if q == 255:
                assert not table and reads == 0
    assert {k: (census(toy.text, v), ) for k, v in tables.items()} == {"toy_n3": ((624, 707, 6),), "pad_bub": ((80, 556, 0),), "pad_bub lifted": ((77, 556, 0),)}
    for what, table in tables.items():  # (the pad_bub reads carry no base that is no member of its site's code; the reference's own reads do)
        sites, member, other = census(toy.text, table)
        assert sites > 0 and member > 0 and (other > 0) == (what == "toy_n3")
    assert tables["pad_bub"] != tables["pad_bub lifted"]
    # lifted, every count lies on a chromosome or on a bubble's own allele-only placement; the sums agree since I counts nothing and a flank base is a flank base
    assert sum(map(sum, tables["pad_bub"].values())) >= sum(map(sum, tables["pad_bub lifted"].values()))


def gen_sam(gen, lifted):
    """SAM lines of the generated reads where they were cut (or lifted by lift_model.lift): what a mapper that found them would print"""
    out = []
    for name, k, o, ln, strand, edit, seq, cig in gen.reads:
        rname, pos, cigar = gen.names[1 + k].split()[0], o + 1, cig
        if lifted:
            got = lift_model.lift(gen.g["bubbles"][k], o + 1, cig)
            if got is not None:
                rname, (pos, cigar) = gen.names[0].split()[0], got
        out.append("\t".join([name, "16" if strand == "-" else "0", rname, str(pos), str(20 + len(out) % 30), cigar, "*", "0", "0", seq, "I" * len(seq)]))
    return ("\n".join(out) + "\n").encode()


def test_model_and_judge_on_the_generated_genome(gen):
    tables = {}
    for lifted in (False, True):
        for q in (0, 35):
            table, reads = both(gen_sam(gen, lifted), gen.g["fasta"], gen.text, gen.names, gen.starts, q)
            if q == 0:
                tables[lifted] = table
                print("generated, lifted" if lifted else "generated", "reads", reads, "sites, member bases, other bases:", census(gen.text, table))
                assert reads == len(gen.reads)
            else:
                assert 0 < reads < len(gen.reads)
    for table in tables.values():
        sites, member, other = census(gen.text, table)
        assert sites > 0 and member > 0
    assert tables[False] != tables[True]
    # lifted, the flanks' counts land on the chromosome's own sites
    assert all(pos < gen.starts[1] for pos in tables[True]) and all(pos >= gen.starts[1] for pos in tables[False])


def test_host_rule_on_the_generated_genome(gen):
    """`places2sam [-B t -R] -A`: every generated read on its bubble record and lifted - the model's bytes"""
    d = gen.dir
    for flags, lifted in (([], False), (["-B", d / "gen.data", "-R"], True)):
        r = run(["places2sam"] + flags + ["-A", d / "counts.tsv", d / "gen.fa", d / "gen.fq", d / "places.bin", d / "out.sam"])
        assert r.returncode == 0, r.stdout
        sam = open(d / "out.sam", "rb").read()
        table, reads, adds = pile_model.pile_sam(sam, gen.text, gen.names, gen.starts)
        assert reads == len(gen.reads) and f"reads counted {reads}  adds {adds}" in r.stdout
        assert open(d / "counts.tsv", "rb").read() == pile_model.tsv(gen.text, gen.names, gen.starts, table)
        # (the placements file carries MAPQ 0: the table is the one of the lines above whatever their MAPQ column says)
        assert table == pile_model.pile(gen.text, [(s, ops, seq, 0) for s, ops, seq, _ in pile_model.sam_placements(gen_sam(gen, lifted), gen.names, gen.starts)])[0]


def test_writer_and_host_rule_write_the_models_bytes(ref, golden, pad_text, fx, toy, tmp_path):
    """`places2sam [-B t [-J] [-R]] [-D] -A f [-a m]` for -a 0, 1, 37, 255: the model's counts file byte for byte, and the SAM bytes of the run without -A"""
    pf, af = write_inputs(fx, tmp_path)
    out, counts = tmp_path / "out.sam", tmp_path / "counts.tsv"
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    ann = alt_model.read_ann(os.path.join(golden, "toy.fa.ann"))
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam")).read()
    padded_x = pad_model.pad_sam(alt_model.expected_sam(plain, fx.places, fx.off, fx.alts, ann).encode(), fx.t.bubbles)
    joined = join_model.apply_to_sam(padded_x, fx.places, fx.joins)
    lift = lambda text: lift_model.lift_sam(text, fx.t.bubbles, fx.t.names, fx.t.chrom)[0]
    cases = (([], [], plain.encode()), (["-B", data, "-R"], [], lift(pad_model.pad_sam(plain.encode(), fx.t.bubbles))), (["-B", data, "-J"], [af], joined),
             (["-B", data, "-J", "-R"], [af], lift(joined)), (["-B", data, "-J", "-R", "-D"], [af], None))
    seen = {}
    for flags, items, base in cases:
        if base is None:  # with -D the lines gain tags; the counts are those without
            base_counts = seen[("-B", data, "-J", "-R")]
        for q in (0, 1, 37, 255):
            r = run(["places2sam"] + flags + ["-A", counts] + (["-a", q] if q else []) + [ref, fq, pf, out] + items)
            assert r.returncode == 0, r.stdout
            got = open(counts, "rb").read()
            if base is None:
                assert got == base_counts[q]
                continue
            table, reads, adds = pile_model.pile_sam(base, toy.text, toy.names, toy.starts, q)
            want = pile_model.tsv(toy.text, toy.names, toy.starts, table)
            assert got == want, (flags, q, pad_model.first_difference(got, want))
            assert f"reads counted {reads}  adds {adds}" in r.stdout and open(out, "rb").read() == base
            seen.setdefault(tuple(flags), {})[q] = got
    for by_q in seen.values():
        assert by_q[255] == pile_model.HEADER.encode() and len({by_q[q] for q in (0, 1, 37, 255)}) >= 2
    assert seen[()][0] != seen[("-B", data, "-R")][0]  # lifted, the flanks count on the chromosome
    assert seen[("-B", data, "-J")][37] != seen[()][37]  # the joined MAPQ is the one -a sees


@pytest.mark.parametrize("what", ["missing", "short", "a_without_A", "a_256", "a_minus", "unwritable"])
def test_refusals_leave_no_file(ref, pad_text, fx, tmp_path, what):
    for f in (".ann",) + ((".ref",) if what != "missing" else ()):
        shutil.copy(ref + f, tmp_path / ("toy.fa" + f))
    if what == "short":
        with open(tmp_path / "toy.fa.ref", "r+b") as f:
            f.truncate(os.path.getsize(tmp_path / "toy.fa.ref") - 1)
    fa, fq, out, counts = tmp_path / "toy.fa", os.path.join(pad_text, "pad_bub.fq"), tmp_path / "out.sam", tmp_path / "counts.tsv"
    opts = {"a_without_A": ["-a", "3"], "a_256": ["-A", counts, "-a", "256"], "a_minus": ["-A", counts, "-a", "-1"], "unwritable": ["-A", tmp_path / "no_such_dir" / "counts.tsv"]}.get(what, ["-A", counts])
    pf, _ = write_inputs(fx, tmp_path)
    for cmd in (["places2sam"] + opts + [fa, fq, pf, out], ["aln2sam"] + opts + [fa, fq, os.path.join(pad_text, "pad_bub_n3.aln"), out], ["map", "-n", "3"] + opts + [fa, fq, out]):
        r = run(cmd)
        assert r.returncode == 1 and not out.exists() and not counts.exists(), r.stdout
        if what in ("missing", "short"):
            assert "-A needs the text" in r.stdout and "bwbble fasta2ref" in r.stdout and "toy.fa.ref" in r.stdout, r.stdout
        elif what == "a_without_A":
            assert "-a needs -A" in r.stdout, r.stdout
        elif what in ("a_256", "a_minus"):
            assert "0..255" in r.stdout, r.stdout
        else:
            assert "Cannot open the counts file" in r.stdout, r.stdout


def test_usage_names_the_flags(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-A <counts.tsv> [-a <int>]]" in r.stdout and "record<TAB>pos<TAB>code<TAB>A<TAB>C<TAB>G<TAB>T" in r.stdout
    assert "-A, -a" in run(["aln2sam"]).stdout and "[-A <counts.tsv>] [-a <MAPQ>]" in run(["places2sam"]).stdout


def edge_cases():
    """(text, [(start, CIGAR, SEQ as printed, MAPQ)]): a text of every code with sites at both ends of a 32-character word, and placements at the rule's edges"""
    text = "K" + md_model.LETTERS[1:] * 3 + "ACGT" * 40 + "$" + "ACGTRYKM" * 30 + "W"
    n = len(text)
    at = text.index("ACGT" * 40)
    two = text.index("$", 1) + 1
    cases = [(k, "15M", b * 15, 30) for b in "ACGTN" for k in (0, 1, 2, n - 15)]                      # every read base on every code
    cases += [(0, "5M", "AAAAA", 30), (n - 5, "5M", "AAAAA", 30), (n - 4, "5M", "AAAAA", 30), (-1, "5M", "AAAAA", 30), (n, "1M", "A", 30)]  # the first and last site; leaving by one
    cases += [(two + o, f"{ln}M", "ACGT" * 64, 30) for o in range(0, 40, 7) for ln in (1, 31, 33, 70)]
    cases = [(s, c, q[:sum(k for k, op in md_model.parse_cigar(c) if op in "MIS")], m) for s, c, q, m in cases]
    cases += [(two, "10M2D10M", "ACGTACGTAC" + "GTACGTACGT", 30), (two, "10M2I3D10M", "A" * 22, 30), (two, "3S10M2S", "T" * 15, 30), (two + 3, "4M1I4M1D4M1I4M1D4M1I4M1D4M1I4M1D4M", "C" * 40, 30),
              (at, f"2M{md_model.MAX_SPAN - 3}D1M", "ACA", 30), (at, f"2M{md_model.MAX_SPAN - 2}D1M", "ACA", 30), (two, f"1M{(1 << 28) - 1}D1M", "AA", 30), (two, "5M", "ACGT", 30),
              (two, "40M", "G" * 40, 9), (two, "40M", "G" * 40, 10), (two, "40M", "G" * 40, 11)]  # MAPQ below, at and above the threshold
    return text, cases


def test_host_rule_called_by_itself_under_the_sanitizers(built, tmp_path):
    """`pile.c: pile_host` in a program of its own, with the tool's compiler flags plus the address and undefined-behaviour sanitizers, on the edge
    cases, both strands, min MAPQ 10: the model's table, reads and adds"""
    text, cases = edge_cases()
    rows, placements = [], []
    for start, cig, seq, mapq in cases:
        for rev in (0, 1):
            fwd = seq[::-1].translate(md_model.COMP) if rev else seq  # the read as uploaded
            ops = md_model.parse_cigar(cig)
            rows.append('{ %d, %d, %d, %d, "%s", %d, { %s } }' % (start, rev, mapq, len(fwd), "".join(str("AGCTN".index(c)) for c in fwd), len(ops),
                                                                   ", ".join(f"{(k << 4) | 'MID?S'.index(op)}u" for k, op in ops)))
            placements.append((start, ops, seq, mapq))
    table, reads, adds = pile_model.pile(text, placements, 10)
    want = pile_model.table_array(text, table)
    src = tmp_path / "rule.c"
    src.write_text("""
#include <stdarg.h>
#include <string.h>
#include "bwb_host.h"
void bwb_die(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); exit(1); }
static const struct { long long start; int rev, mapq; unsigned len; const char *seq; unsigned n_ops; uint32_t ops[24]; } cases[] = { %s };
static uint8_t text[] = { %s };
enum { N = sizeof(cases) / sizeof(cases[0]) };
int main(void) {
	/* every case as a lifted primary of record 0, which begins at text position 0: the ops as they are, from position start + 1 */
	md_text_t t = { .codes = text, .n_fwd = sizeof(text), .ready = 1 };
	seq_annotation_t rec = { .name = "all", .start_index = 0, .end_index = sizeof(text) - 1 };
	fasta_annotations_t ann = { .num_seq = 1, .seq_anns = &rec };
	bwb_place *pl = (bwb_place *)calloc(N, sizeof(bwb_place));
	uint8_t *seq = (uint8_t *)calloc(N, 255), *kind = (uint8_t *)malloc(N);
	uint16_t *len = (uint16_t *)calloc(N, 2);
	uint64_t *off = (uint64_t *)calloc(N + 1, 8);
	bwb_lift *recs = (bwb_lift *)calloc(N * 7, sizeof(bwb_lift));
	for (size_t k = 0; k < N; k++) {
		for (unsigned i = 0; i < cases[k].len; i++) seq[k * 255 + i] = (uint8_t)(cases[k].seq[i] - '0');
		len[k] = (uint16_t)cases[k].len;
		pl[k].flags = BWB_PLACE_MAPPED | (cases[k].rev ? BWB_PLACE_REVERSE : 0);
		pl[k].mapq = (uint8_t)cases[k].mapq;
		pl[k].pos = 3; pl[k].aln_length = (uint16_t)cases[k].len;
		for (int g = 0; g < BWB_MAX_GAP_RUNS; g++) pl[k].gap_run[g] = 0xFFFF;
		kind[k] = BWB_LIFT_LIFTED;
		bwb_lift *r = recs + off[k];
		r->pos = cases[k].start + 1; r->seqid = 0; r->n_ops = (uint8_t)cases[k].n_ops;
		memcpy(r + 1, cases[k].ops, cases[k].n_ops * 4);
		off[k + 1] = off[k] + 1 + (cases[k].n_ops + 3) / 4;
	}
	pile_t *p = pile_open(NULL, 10);
	pile_set_text(p, &t, 1);
	const uint64_t reads = pile_host(p, pl, N, seq, 255, len, kind, off, recs, NULL, &ann);
	printf("%%llu %%llu %%llu %%llu\\n", (unsigned long long)p->n_sites, (unsigned long long)reads, (unsigned long long)p->reads, (unsigned long long)p->adds);
	for (uint64_t s = 0; s < p->n_sites; s++) printf("%%u %%u %%u %%u\\n", p->counts[4 * s], p->counts[4 * s + 1], p->counts[4 * s + 2], p->counts[4 * s + 3]);
	/* and as placements of their own (no lift records): ungapped reads from pl.pos, with the join records' MAPQ in place of the placements' */
	bwb_join *joins = (bwb_join *)calloc(N, sizeof(bwb_join));
	for (size_t k = 0; k < N; k++) { joins[k].mapq = (uint8_t)(k %% 2 ? 10 : 9); pl[k].mapq = 60; }
	pile_t *q = pile_open(NULL, 10);
	pile_set_text(q, &t, 1);
	printf("%%llu\\n", (unsigned long long)pile_host(q, pl, N, seq, 255, len, NULL, NULL, NULL, joins, &ann));
	pile_free(p); pile_free(q);
	free(pl); free(seq); free(kind); free(len); free(off); free(recs); free(joins);
	return 0;
}
""" % (",\n".join(rows), ", ".join(str(c) for c in pile_model.codes(text))))
    exe = tmp_path / "rule"
    host = os.path.join(ROOT, "bwbble_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", host,
                    str(src), os.path.join(host, "pile.c"), os.path.join(host, "md.c"), "-o", str(exe), "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.split("\n")[:-1]
    assert lines[0] == f"{len(want)} {reads} {reads} {adds}", (lines[0], len(want), reads, adds)
    got = np.array([[int(x) for x in ln.split()] for ln in lines[1:1 + len(want)]], dtype=np.uint32)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:5]
    # the census of the cases: every code under every base, the first and the last character are sites, MAPQ 9 is left out, the long gaps count nothing
    assert text[0] in pile_model.SITE_LETTERS and text[-1] in pile_model.SITE_LETTERS and want[0].sum() > 0 and want[-1].sum() > 0
    letters = np.array([text[i] for i in pile_model.sites(text)])
    assert len(want) == len(letters) and reads < len(placements) - 8
    assert all((want[letters == c] > 0).any(axis=0).all() for c in pile_model.SITE_LETTERS)  # all 40 pairs of a read base and a site's code
    assert pile_model.pile(text, [p for p in placements if p[3] == 9], 10)[1] == 0 < pile_model.pile(text, [p for p in placements if p[3] == 10], 10)[1]
    # the second call: reads of 1..70 bases at text position 3, counted when their join record says MAPQ 10
    second = [(3, [(len(seq), "M")], seq, 10 if k % 2 else 9) for k, (_, _, seq, _) in enumerate(placements)]
    assert int(lines[-1]) == pile_model.pile(text, second, 10)[1] > 0
