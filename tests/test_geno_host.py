"""Genotype calls at the IUPAC sites and the indel bubbles (`-G`) without a GPU: the crafted count vectors and what they cover; the rule against the
judge that adds one base at a time (tests/geno_model.py), fed by the plain pileup of pile_model and the name judge of indel_model; the host's rule
and the writer (`places2sam ... -G f -q e -d n`) against the model's bytes on the generated genome, the pad_bub reads plain, lifted and joined, and
the reference-derived placements of toy_n3; the refusals; the usage texts; the records' layout; `geno.c: geno_host` in a program of its own under
the address and undefined-behaviour sanitizers; and the truth census of a diploid sample."""
import os
import subprocess
import types

import numpy as np
import pytest

import bwbble_amd as bw
import geno_model
import indel_model
import lift_model
import pad_model
import pile_model
from test_indel_host import gen  # noqa: F401 (fixture)
from test_md_host import fx, pad_text, ref, run, toy, write_inputs  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crafted_vectors_cover_the_rule():
    """per code: every genotype the winner, every two-way tie that exists and the all-equal tie, GQ 98 / 99 / capped, the depth edge, E = 4, 20, 93,
    the PL edges with counters up to 0xFFFFFFFF, other bases only (geno_model.check_crafted asserts each); and the judge agrees wherever the
    bases can be laid out one by one"""
    vectors = geno_model.check_crafted()
    assert set(vectors) == set(geno_model.MEMBERS) and len(vectors) == 10
    judged = 0
    for letter, vs in vectors.items():
        assert {e for _, e, _, _ in vs} >= {4, 20, 93} and {d for _, _, d, _ in vs} >= {1, 7, (1 << 31) - 1}
        for what, err, d, v in vs:
            if sum(v) > 500:
                continue
            mem = geno_model.MEMBERS[letter]
            al = [v[geno_model.COLS.index(c)] for c in mem]
            if sum(v):
                assert geno_model.judge(geno_model.expand(v, letter), len(mem), err) == geno_model.rule(al, sum(v), err), (letter, what)
                judged += 1
    assert judged >= 20 * len(vectors)


def judged_sites(sam, fasta, err, min_depth, min_mapq=0):
    """the plain pileup of pile_model.judge_sam, called one base at a time -> {(record, pos): (letter, AD, other, GT letters, GQ, PLs)}"""
    out = {}
    for key, (letter, v) in pile_model.judge_sam(sam, fasta, min_mapq).items():
        if sum(v) < min_depth:
            continue
        mem = geno_model.MEMBERS[letter]
        gt, gq, pl = geno_model.judge(geno_model.expand(v, letter), len(mem), err)
        x, y = geno_model.GENOTYPES[gt]
        al = [v[geno_model.COLS.index(c)] for c in mem]
        out[key] = (letter, al, sum(v) - sum(al), f"{mem[x]}/{mem[y]}", gq, pl)
    return out


def written_sites(data):
    return {(f[1], f[2]): (f[3], f[5], f[6], f[7], f[8], f[9]) for f in geno_model.parse_calls(data) if f[0] == "S"}


def written_bubbles(data):
    return {int(f[3]): (f[5], f[6], f[7], f[8], f[9]) for f in geno_model.parse_calls(data) if f[0] == "I"}


def judged_bubbles(counts, bubbles, w, err, min_depth):
    """a table of the name judge, called one read at a time -> {bubble: (AD, other, GT, GQ, PLs)}"""
    out = {}
    for b, v in enumerate(counts):
        v = [int(x) for x in v]
        if not indel_model.eligible(bubbles[b], w) or sum(v) < min_depth:
            continue
        gt, gq, pl = geno_model.judge([0] * v[0] + [1] * v[1] + [None] * (v[2] + v[3]), 2, err)
        x, y = geno_model.GENOTYPES[gt]
        out[b] = (v[:2], v[2] + v[3], f"{'RV'[x]}/{'RV'[y]}", gq, pl)
    return out


def model_bytes(sam, text, names, starts, bubbles, indel_counts, w, err, min_depth, min_mapq=0):
    """the calls file of SAM bytes by the models: pile_model's table of them, the given indel table (None: no bubble lines)"""
    table, _, _ = pile_model.pile_sam(sam, text, names, starts, min_mapq)
    sites = geno_model.site_records(text, pile_model.table_array(text, table), err, min_depth)
    bubs = geno_model.bubble_records(bubbles, indel_counts, w, err, min_depth) if indel_counts is not None else ()
    return geno_model.calls_bytes(text, names, starts, sites, bubbles, bubs), sites, bubs


@pytest.mark.parametrize("err,min_depth,w", [(None, None, None), (4, 1, 5), (93, 3, 30), (20, 40, 1), (20, (1 << 31) - 1, 1)])
def test_host_rule_and_writer_on_the_generated_genome(gen, err, min_depth, w):
    """`places2sam -B t [-R] -A a -I i -G f [-q e] [-d n] [-w w]`: the model's bytes, plain and lifted; both judges agree with every line; the SAM, -A
    and -I bytes are those of the run without -G"""
    d = gen.dir
    E, D, W = err or 20, min_depth or 1, w or 1
    text, names, starts = pile_model.fasta_text(gen.g["fasta"])
    opts = (["-w", W] if w else []) + ["-G", d / "calls.tsv"] + (["-q", E] if err else []) + (["-d", D] if min_depth else [])
    tail = [d / "gen.fa", d / "gen.fq", d / "places.bin"]
    for lift in ([], ["-R"]):
        base = ["places2sam", "-B", d / "gen.data"] + lift + ["-A", d / "a.tsv", "-I", d / "i.tsv"] + (["-w", W] if w else [])
        assert run(base + tail + [d / "plain.sam"]).returncode == 0
        plain = [open(d / n, "rb").read() for n in ("plain.sam", "a.tsv", "i.tsv")]
        r = run(["places2sam", "-B", d / "gen.data"] + lift + ["-A", d / "a.tsv", "-I", d / "i.tsv"] + opts + tail + [d / "out.sam"])
        assert r.returncode == 0, r.stdout
        assert [open(d / n, "rb").read() for n in ("out.sam", "a.tsv", "i.tsv")] == plain
        got = open(d / "calls.tsv", "rb").read()
        counts, _, _ = indel_model.count(indel_model.truth(gen.g, gen.reads), gen.g["bubbles"], gen.chrom, W)
        want, sites, bubs = model_bytes(plain[0], text, names, starts, gen.g["bubbles"], counts, W, E, D)
        assert got == want, (lift, pad_model.first_difference(got, want))
        assert f"error phred {E}  minimum depth {D}  sites called {len(sites)}  bubbles called {len(bubs)}  lines written {len(sites) + len(bubs)}" in r.stdout, r.stdout
        # the second judges: the plain pileup and the name judge, one base and one read at a time
        assert written_sites(got) == judged_sites(plain[0], gen.g["fasta"], E, D)
        assert written_bubbles(got) == judged_bubbles(indel_model.judged_table(gen.reads, gen.g["bubbles"], W), gen.g["bubbles"], W, E, D)
        # -G alone writes the same file
        r = run(["places2sam", "-B", d / "gen.data"] + lift + opts + tail + [d / "alone.sam"])
        assert r.returncode == 0 and open(d / "calls.tsv", "rb").read() == want and open(d / "alone.sam", "rb").read() == plain[0], r.stdout
    if D == (1 << 31) - 1:
        assert want == geno_model.HEADER
    elif D == 1 and E == 20:
        # (reads were cut from both alleles of every bubble, so the calls are R/V - but for del130, whose site no read of 100 bases spans)
        assert len(sites) > 10 and len(bubs) == 8 and {int(g) for g in bubs["gt"]} == {1, 2}


def test_sites_only_without_the_table(gen):
    """`places2sam -G f` without -B: site lines only, of the reads on their own records; -w and -a are accepted"""
    d = gen.dir
    text, names, starts = pile_model.fasta_text(gen.g["fasta"])
    tail = [d / "gen.fa", d / "gen.fq", d / "places.bin"]
    assert run(["places2sam"] + tail + [d / "p.sam"]).returncode == 0
    for q in (0, 37, 38):  # (the placement records carry MAPQ 37)
        r = run(["places2sam", "-a", q, "-w", 9, "-G", d / "s.tsv"] + tail + [d / "s.sam"])
        assert r.returncode == 0, r.stdout
        want, sites, _ = model_bytes(open(d / "p.sam", "rb").read(), text, names, starts, None, None, 1, 20, 1, q)
        assert open(d / "s.tsv", "rb").read() == want and open(d / "s.sam", "rb").read() == open(d / "p.sam", "rb").read()
        assert (len(sites) > 0) == (q <= 37) and b"\nI\t" not in want


def test_pad_bub_reads_plain_lifted_and_joined(ref, golden, pad_text, fx, toy, tmp_path):
    """the pad_bub reads on pad_toy.data: `places2sam -B t [-J] [-R] -G f -q e -d n -w w -a m` writes the model's bytes fed the SAM text of the run
    without -G and the model's own locus and join records"""
    pf, af = write_inputs(fx, tmp_path)
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    t = fx.t
    loci = pad_model.expected_loci(fx.places, t.start, t.end, t.bub_of, t.bubbles)
    seen = set()
    for flags, joined in ((["-B", data], False), (["-B", data, "-R"], False), (["-B", data, "-J"], True), (["-B", data, "-J", "-R"], True)):
        items = [af] if joined else []
        assert run(["places2sam"] + flags + [ref, fq, pf, tmp_path / "plain.sam"] + items).returncode == 0
        plain = open(tmp_path / "plain.sam", "rb").read()
        for E, D, w, q in ((20, 1, 1, 0), (7, 2, 10, 20), (93, 1, 5, 0)):
            r = run(["places2sam"] + flags + ["-a", q, "-w", w, "-G", tmp_path / "g.tsv", "-q", E, "-d", D, ref, fq, pf, tmp_path / "o.sam"] + items)
            assert r.returncode == 0, r.stdout
            counts, _, _ = indel_model.count(indel_model.from_records(fx.places, loci, fx.joins["mapq"] if joined else None), t.bubbles, t.chrom, w, q)
            want, sites, bubs = model_bytes(plain, toy.text, toy.names, toy.starts, t.bubbles, counts, w, E, D, q)
            got = open(tmp_path / "g.tsv", "rb").read()
            assert got == want, (flags, E, D, w, q, pad_model.first_difference(got, want))
            assert open(tmp_path / "o.sam", "rb").read() == plain and len(sites) > 0 and len(bubs) > 0
            assert written_sites(got) == judged_sites(plain, open(os.path.join(golden, "toy.fa")).read(), E, D, q)
            seen.add((tuple(flags), got))
    assert len({g for _, g in seen}) >= 6  # lifted, the flanks' bases count on the chromosome; the joined MAPQ is the one -a sees


def test_toy_n3_placements(ref, golden, fx, toy, tmp_path):
    """the reference-derived placements of toy_n3 (no table): site lines, with three-member codes among them, at E = 4, 20 and 93"""
    pf = tmp_path / "toy_places.bin"
    fx.toy_places.tofile(pf)
    fq = os.path.join(golden, "toy.fq")
    assert run(["places2sam", ref, fq, pf, tmp_path / "plain.sam"]).returncode == 0
    plain = open(tmp_path / "plain.sam", "rb").read()
    fasta = open(os.path.join(golden, "toy.fa")).read()
    for E, D in ((4, 1), (20, 1), (93, 2)):
        r = run(["places2sam", "-G", tmp_path / "g.tsv", "-q", E, "-d", D, ref, fq, pf, tmp_path / "o.sam"])
        assert r.returncode == 0, r.stdout
        want, sites, _ = model_bytes(plain, toy.text, toy.names, toy.starts, None, None, 1, E, D)
        got = open(tmp_path / "g.tsv", "rb").read()
        assert got == want, pad_model.first_difference(got, want)
        assert open(tmp_path / "o.sam", "rb").read() == plain and written_sites(got) == judged_sites(plain, fasta, E, D)
        if D == 1:
            assert len(sites) == 624 and {int(n) for n in sites["n_geno"]} == {3, 6} and any(f[6] for f in geno_model.parse_calls(got))  # (the census of test_pile_host: 624 sites, 6 other bases)


@pytest.mark.parametrize("what", ["q_without_G", "d_without_G", "q_3", "q_94", "q_text", "d_0", "d_2p31", "d_text", "a_alone", "w_alone", "unwritable"])
def test_refusals_leave_no_file(ref, golden, pad_text, fx, tmp_path, what):
    fq, out, calls = os.path.join(pad_text, "pad_bub.fq"), tmp_path / "out.sam", tmp_path / "calls.tsv"
    data = os.path.join(golden, "pad_toy.data")
    opts = {"q_without_G": ["-q", 20], "d_without_G": ["-d", 2], "q_3": ["-G", calls, "-q", 3], "q_94": ["-G", calls, "-q", 94], "q_text": ["-G", calls, "-q", "2o"],
            "d_0": ["-G", calls, "-d", 0], "d_2p31": ["-G", calls, "-d", 1 << 31], "d_text": ["-G", calls, "-d", "x"], "a_alone": ["-a", 3], "w_alone": ["-w", 3],
            "unwritable": ["-G", tmp_path / "no_such_dir" / "calls.tsv"]}[what]
    want = {"q_without_G": "-q needs -G", "d_without_G": "-d needs -G", "a_alone": "-a needs -A", "w_alone": "-w needs -I", "unwritable": "Cannot open the calls file"}.get(what, "4..93" if what[0] == "q" else "1..2147483647")
    pf, _ = write_inputs(fx, tmp_path)
    for cmd in (["places2sam", "-B", data] + opts + [ref, fq, pf, out], ["aln2sam", "-B", data] + opts + [ref, fq, os.path.join(pad_text, "pad_bub_n3.aln"), out],
                ["map", "-n", "3", "-B", data] + opts + [ref, fq, out]):
        r = run(cmd)
        assert r.returncode == 1 and not out.exists() and not calls.exists(), (cmd[0], r.stdout)
        assert want in r.stdout, (cmd[0], r.stdout)


def test_a_run_that_stops_later_leaves_no_calls_file(ref, golden, pad_text, fx, tmp_path):
    """the calls file is opened first; a counts file that cannot be opened, and a table -R refuses, stop the run and remove it"""
    pf, _ = write_inputs(fx, tmp_path)
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    r = run(["places2sam", "-B", data, "-A", tmp_path / "no_such_dir" / "c.tsv", "-G", tmp_path / "g.tsv", ref, fq, pf, tmp_path / "o.sam"])
    assert r.returncode == 1 and not (tmp_path / "g.tsv").exists() and not (tmp_path / "o.sam").exists(), r.stdout
    r = run(["places2sam", "-G", tmp_path / "g.tsv", tmp_path / "no.fa", fq, pf, tmp_path / "o.sam"])
    assert r.returncode != 0 and not (tmp_path / "g.tsv").exists(), r.stdout


def test_usage_names_the_flags(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-G <calls.tsv> [-q <int>] [-d <int>]]" in r.stdout and "#kind<TAB>record<TAB>pos<TAB>id<TAB>alleles<TAB>AD<TAB>other<TAB>GT<TAB>GQ<TAB>PL" in r.stdout
    assert "-G, -q, -d" in run(["aln2sam"]).stdout and "[-G <calls.tsv>] [-q <err>] [-d <depth>]" in run(["places2sam"]).stdout


def test_layout_of_the_records(built, tmp_path):
    """bwb_geno_site and bwb_geno_bubble as the C compiler sees them == the dtypes"""
    src = tmp_path / "layout.c"
    fields = [("bwb_geno_site", bw.GENO_SITE_DTYPE), ("bwb_geno_bubble", bw.GENO_BUBBLE_DTYPE)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {']
    for s, dt in fields:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in dt.names]
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    for s, dt in fields:
        assert int(got[s]) == dt.itemsize, s
        for f in dt.names:
            assert int(got[f"{s}.{f}"]) == dt.fields[f][1], (s, f)
    assert (int(got["bwb_geno_site"]), int(got["bwb_geno_bubble"])) == (64, 48)


def crafted_text():
    """a text that holds every code once per crafted vector of that code, the ten letters in turn with plain bases between -> (text, [(E, d, counters)] per site)"""
    vectors = geno_model.check_crafted()
    per_site = []
    text = []
    todo = {letter: list(vs) for letter, vs in vectors.items()}
    k = 0
    while any(todo.values()):
        for letter in geno_model.MEMBERS:
            if todo[letter]:
                what, err, d, v = todo[letter].pop(0)
                text.append(letter + "ACGTN"[k % 5] * (k % 3))
                per_site.append((err, d, v))
                k += 1
    return "".join(text) + "$", per_site


def test_host_rule_called_by_itself_under_the_sanitizers(built, tmp_path):
    """`geno.c: geno_host` and `geno_write` in a program of its own, with the tool's compiler flags plus the address and undefined-behaviour
    sanitizers: every crafted vector on every code, each under its own E and d, and a bubble table with ineligible bubbles beside eligible ones"""
    text, per_site = crafted_text()
    codes = pile_model.codes(text)
    groups = sorted({(e, d) for e, d, _ in per_site})
    w = 4
    bubbles = [(b"c0 x", 100, 20, 120, 19, 0, 3), (b"c0 x", 300, w - 1, 303, w - 1, 0, 1), (b"c0 x", 300, w, 304, w - 1, 0, 1), (b"c0 x", 500, 10, 509, 10, 0, 2), (b"c0 x", 600, 20, 625, 19, 5, 0)]
    bcounts = [[5, 0, 1, 0], [9, 9, 9, 9], [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], [7, 7, 0, 0], [6, 6, 0, 1]]
    src = tmp_path / "rule.c"
    src.write_text("""
#include <stdarg.h>
#include <string.h>
#include "bwb_host.h"
void bwb_die(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); exit(1); }
int sam_mapq(int top1, int top2, int num_mm, int max_mm) { (void)top1; (void)top2; (void)num_mm; (void)max_mm; return 0; } /* (pad.c: join_resolve, not called here) */
static uint8_t codes[] = { %s };
static uint32_t counts[][4] = { %s };
static const struct { int err; long long d; } groups[] = { %s };
static bwb_bubble bubs[] = { %s };
static uint32_t bcounts[][4] = { %s };
static int32_t chrom_of[] = { %s };
static char *anns[] = { %s };
enum { N = sizeof(codes), NS = sizeof(counts) / sizeof(counts[0]), NG = sizeof(groups) / sizeof(groups[0]), NB = sizeof(bubs) / sizeof(bubs[0]) };
int main(int argc, char **argv) {
	(void)argc;
	md_text_t text = { .codes = codes, .n_fwd = N };
	bubble_table_t t = { .n = NB, .b = bubs, .ann = anns };
	seq_annotation_t sa = { .start_index = 0, .end_index = N - 1 };
	strcpy(sa.name, "crafted text");
	fasta_annotations_t ann = { .num_seq = 1, .seq_anns = &sa };
	for (size_t k = 0; k < NG; k++) {
		pile_t *p = pile_open(NULL, 0);
		pile_set_text(p, &text, 0);
		if (p->n_sites != NS) return 2;
		memcpy(p->counts, counts, sizeof(counts));
		indel_t *q = indel_open(NULL, 0, %d);
		indel_set_table(q, &t, chrom_of);
		memcpy(q->counts, bcounts, sizeof(bcounts));
		char name[512];
		snprintf(name, sizeof(name), "%%s.%%zu", argv[1], k);
		geno_t *g = geno_open(name, groups[k].err, groups[k].d);
		geno_host(g, p, k %% 2 ? NULL : q);
		printf("%%llu %%llu ", (unsigned long long)g->n_sites, (unsigned long long)g->n_bubs);
		printf("%%llu\\n", (unsigned long long)geno_write(g, &ann, &t));
		geno_free(g); pile_free(p); indel_free(q);
	}
	return 0;
}
""" % (", ".join(str(int(c)) for c in codes), ", ".join("{ %du, %du, %du, %du }" % tuple(v) for _, _, v in per_site), ", ".join("{ %d, %dLL }" % g for g in groups),
       ", ".join("{ %dLL, %dLL, %dLL, %dLL, %d, %d }" % b[1:] for b in bubbles), ", ".join("{ %du, %du, %du, %du }" % tuple(v) for v in bcounts), ", ".join("0" for _ in bubbles),
       ", ".join('"%s"' % b[0].decode() for b in bubbles), w))
    exe = tmp_path / "rule"
    host = os.path.join(ROOT, "bwbble_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", host,
                    str(src), os.path.join(host, "geno.c"), os.path.join(host, "pile.c"), os.path.join(host, "md.c"), os.path.join(host, "indel.c"), os.path.join(host, "pad.c"), "-o", str(exe), "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe), str(tmp_path / "calls")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    counts = np.array([v for _, _, v in per_site], dtype=np.uint32)
    assert [indel_model.eligible(b, w) for b in bubbles] == [True, False, True, False, True]
    names, starts = ["crafted text"], [0]
    called_own = 0
    for k, (E, D) in enumerate(groups):
        sites = geno_model.site_records(text, counts, E, D)
        bubs = geno_model.bubble_records(bubbles, np.array(bcounts, dtype=np.uint32), w, E, D) if k % 2 == 0 else np.zeros(0, dtype=bw.GENO_BUBBLE_DTYPE)
        want = geno_model.calls_bytes(text, names, starts, sites, bubbles, bubs)
        got = open(f"{tmp_path / 'calls'}.{k}", "rb").read()
        assert got == want, (E, D, pad_model.first_difference(got, want))
        assert r.stdout.split("\n")[k] == f"{len(sites)} {len(bubs)} {len(sites) + len(bubs)}"
        own = [s for s, (e, d, _) in enumerate(per_site) if (e, d) == (E, D)]  # the vectors made for this E and d: called or not as their depth says
        assert {int(s) for s in sites["site"]} >= {s for s in own if sum(per_site[s][2]) >= D}
        called_own += len(own)
        assert not ({1, 3} & {int(b) for b in bubs["bubble"]})  # an ineligible bubble is never called, whatever its counters hold
    assert called_own == len(per_site)


# ---- the truth census ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(built, oracle, tmp_path_factory):
    return geno_model.build_chain(tmp_path_factory.mktemp("geno_chain"), oracle)


# what tools/geno_generated_reference.py prints: the sample's 1 721 reads through the oracle's `align -n 3 -o 1`, the models' records and
# `places2sam -B t -J -R -a 1 -w 5 -G`
CENSUS = {"sites with a genotype": 27, "sites called": 27, "sites with GQ >= 20": 26, "site disagreements": 0, "called on a bubble record's allele": 0,
          "eligible bubbles": 8, "bubbles called": 8, "bubbles with GQ >= 20": 8, "bubble disagreements": 1}
# The one disagreement: bubble 4 deletes 130 bases, so its window on the chromosome is 130 + 2 x 5 positions wide and no read of 100 bases covers it -
# -I can count no ref read there (tests/test_indel_host.py says the same of its reads), and the sample's R/V is called V/V from alt reads alone.
DISAGREEMENTS = [("I", 4, 2101, "V/V", "R/V", [0, 23], 0, 69)]


def test_truth_census_of_the_diploid_sample(chain):
    figures, wrong = geno_model.census(chain)
    print(figures, wrong)
    assert figures == CENSUS and wrong == DISAGREEMENTS, (figures, wrong)
    assert 2 * figures["sites with GQ >= 20"] >= figures["sites with a genotype"] and 2 * figures["bubbles with GQ >= 20"] >= figures["eligible bubbles"]
    assert len(chain.sample.reads) == 1721 and set(chain.sample.bubbles) == {0, 1, 2} and len(set(chain.sample.sites.values())) > 6
    # the chain's calls are the model's fed the chain's own SAM text, and -G changes no other file
    assert chain.calls_sam == chain.base
    bub_of = pad_model.bubble_of(chain.names, chain.g["bubbles"])
    chrom = np.zeros(len(chain.g["bubbles"]), dtype=np.int32)
    counts, _, _ = indel_model.count(indel_model.from_sam(chain.base, chain.names, bub_of), chain.g["bubbles"], chrom, geno_model.ANCHOR, geno_model.MIN_MAPQ)
    assert indel_model.table_bytes(chain.g["bubbles"], counts) == chain.i_tsv
    text, names, starts = pile_model.fasta_text(chain.g["fasta"])
    want, _, _ = model_bytes(chain.base, text, names, starts, chain.g["bubbles"], counts, geno_model.ANCHOR, 20, 1, geno_model.MIN_MAPQ)
    assert chain.calls == want, pad_model.first_difference(chain.calls, want)
    assert written_sites(chain.calls) == judged_sites(chain.base, chain.g["fasta"], 20, 1, geno_model.MIN_MAPQ)
