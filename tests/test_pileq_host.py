"""Base qualities in the allele counts and the genotype calls (`-b m`, `-Y`) without a GPU: the model against the plain pileup that reads the QUAL
column of the SAM line itself (tests/pileq_model.py) on the reference's golden lines, on the pad_bub reads plain, lifted and joined, and on the
generated genome, under FASTQ quality lines rewritten by a seeded generator; the host's rule and the writers (`places2sam ... -b m -Y -G f`) against
the model's bytes; `-b 0` without `-Y` and qualities that all reach E against the run without the flags; the refusals; the usage texts; the layout of
the new record; `pile.c: pile_host_q` and the weighted `geno.c: geno_host` in a program of their own under the address and undefined-behaviour
sanitizers; and the truth census of a diploid sample whose read errors carry a low quality."""
import os
import subprocess

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import geno_model
import indel_model
import join_model
import lift_model
import md_model
import pad_model
import pile_model
import pileq_model
from test_md_host import fx, gen, pad_text, ref, run, toy, write_inputs  # noqa: F401 (fixtures)
from test_pile_host import edge_cases, gen_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((0, 0), (1, 0), (20, 0), (93, 0), (0, 4), (0, 20), (20, 30), (0, 93))  # (-b m, -Y's E or 0)


def keyed(text, names, starts, counts, sums):
    """the model's tables by (record, 1-based position), as the judge keys its own: through the counts file's writer and parser"""
    c = pile_model.parse_tsv(pile_model.tsv(text, names, starts, counts))
    s = pile_model.parse_tsv(pile_model.tsv(text, names, starts, sums))
    return {k: (v[0], v[1], s[k][1] if k in s else [0, 0, 0, 0]) for k, v in c.items()}


def both(sam, fasta, text, names, starts, min_mapq, m, E):
    """the model's tables of SAM bytes, after the judge has agreed"""
    counts, sums, reads, adds, dropped = pileq_model.pile_sam_q(sam, text, names, starts, min_mapq, m, E)
    judged = pileq_model.judge_sam_q(sam, fasta, min_mapq, m, E)
    assert keyed(text, names, starts, counts, sums) == {k: v[:3] for k, v in judged.items()}, (min_mapq, m, E)
    assert adds == sum(sum(v[1]) for v in judged.values()) and all(len(v[3]) == sum(v[1]) for v in judged.values())
    return counts, sums, reads, adds, dropped


def judged_calls(judged, min_depth):
    """the judge's pileup called one base at a time -> {(record, pos): (letter, AD, other, GT letters, GQ, PLs, QS)}"""
    out = {}
    for key, (letter, v, u, bases) in judged.items():
        if sum(v) < min_depth:
            continue
        mem = geno_model.MEMBERS[letter]
        gt, gq, pl = pileq_model.judge_q([(mem.index(b) if b in mem else None, q) for b, q in bases], len(mem))
        x, y = geno_model.GENOTYPES[gt]
        al = [v[geno_model.COLS.index(c)] for c in mem]
        out[key] = (letter, al, sum(v) - sum(al), f"{mem[x]}/{mem[y]}", gq, pl, [u[geno_model.COLS.index(c)] for c in mem])
    return out


def check_texts(texts, fasta, text, names, starts, mapqs):
    seen = {}
    for what, sam in texts.items():
        for q in mapqs:
            plain = pile_model.pile_sam(sam, text, names, starts, q)
            for m, E in SETTINGS:
                counts, sums, reads, adds, dropped = both(sam, fasta, text, names, starts, q, m, E)
                assert reads == plain[1] and adds + dropped == plain[2]  # -b drops bases, never reads
                if m == 0:
                    assert counts == plain[0] and dropped == 0
                assert bool(sums) == bool(E and adds)
                if E:
                    assert all(4 * n <= s <= E * n for pos in counts for n, s in zip(counts[pos], sums[pos]))
                seen[(what, q, m, E)] = (counts, sums, dropped)
    return seen


def test_model_and_judge_on_the_golden_lines(golden, pad_text, fx, toy):
    """toy_n3.sam and the pad_bub reads plain, lifted and joined, QUAL rewritten: the plain pileup that reads QUAL equals the model at every
    setting; a wrong orientation of the quality line does not"""
    fasta = open(os.path.join(golden, "toy.fa")).read()
    _, tq = pileq_model.requal_fastq(open(os.path.join(golden, "toy.fq"), "rb").read(), 11)
    _, pq = pileq_model.requal_fastq(open(os.path.join(pad_text, "pad_bub.fq"), "rb").read(), 12)
    every = b"".join(tq.values()) + b"".join(pq.values())
    assert all(c in every for c in pileq_model.EDGE_BYTES) and all(q != q[::-1] for q in list(tq.values()) + list(pq.values()) if len(q) > 1)
    plain = open(os.path.join(pad_text, "pad_bub_n3.sam"), "rb").read()
    ann = alt_model.read_ann(os.path.join(golden, "toy.fa.ann"))
    padded_x = pad_model.pad_sam(alt_model.expected_sam(plain.decode(), fx.places, fx.off, fx.alts, ann).encode(), fx.t.bubbles)
    joined = join_model.apply_to_sam(padded_x, fx.places, fx.joins)
    lift = lambda t: lift_model.lift_sam(t, fx.t.bubbles, fx.t.names, fx.t.chrom)[0]
    texts = {"toy_n3": pileq_model.requal_sam(open(os.path.join(golden, "toy_n3.sam"), "rb").read(), tq), "pad_bub": pileq_model.requal_sam(plain, pq),
             "pad_bub lifted": pileq_model.requal_sam(lift(pad_model.pad_sam(plain, fx.t.bubbles)), pq), "pad_bub joined": pileq_model.requal_sam(joined, pq),
             "pad_bub joined and lifted": pileq_model.requal_sam(lift(joined), pq)}
    seen = check_texts(texts, fasta, toy.text, toy.names, toy.starts, (0, 37))
    for what in texts:
        assert seen[(what, 0, 20, 0)][2] > 0 and seen[(what, 0, 93, 0)][2] > seen[(what, 0, 20, 0)][2] > seen[(what, 0, 1, 0)][2] > 0, what
        assert seen[(what, 0, 0, 20)][1] != seen[(what, 0, 0, 93)][1] != seen[(what, 0, 0, 4)][1]
    # the quality line laid the wrong way round under the reverse strand's reads: other tables
    flipped = pileq_model.requal_sam(plain, {k: v[::-1] for k, v in pq.items()})
    assert any(int(ln.split(b"\t")[1]) & 16 for ln in plain.split(b"\n")[:-1] if ln[:1] != b"@")
    assert pileq_model.pile_sam_q(flipped, toy.text, toy.names, toy.starts, 0, 20, 30)[:2] != seen[("pad_bub", 0, 20, 30)][:2]


def test_model_and_judge_on_the_generated_genome(gen):
    _, q = pileq_model.requal_fastq(open(gen.dir / "gen.fq", "rb").read(), 13)
    texts = {lifted: pileq_model.requal_sam(gen_sam(gen, lifted), q) for lifted in (False, True)}
    seen = check_texts(texts, gen.g["fasta"], gen.text, gen.names, gen.starts, (0, 35))
    assert seen[(False, 0, 20, 30)][:2] != seen[(True, 0, 20, 30)][:2] and seen[(True, 0, 20, 0)][2] > 0


def requalled(src, dst, seed, fixed=None):
    data, quals = pileq_model.requal_fastq(open(src, "rb").read(), seed, fixed)
    open(dst, "wb").write(data)
    return quals


def test_writers_and_host_rule_write_the_models_bytes(ref, golden, pad_text, fx, toy, tmp_path):
    """`places2sam [-B t [-J] [-R]] -A a -I i -G f [-b m] [-Y] [-q E]` on the pad_bub reads under rewritten qualities: the model's counts and calls
    files byte for byte at -b 0, 1, 20, 93 and -Y with -q 4, 20, 93; the second judge on every S line; the SAM and -I bytes of the run without
    the flags; -b 0 without -Y changes no byte of any file"""
    pf, af = write_inputs(fx, tmp_path)
    fq, data = tmp_path / "q.fq", os.path.join(golden, "pad_toy.data")
    quals = requalled(os.path.join(pad_text, "pad_bub.fq"), fq, 12)
    fasta = open(os.path.join(golden, "toy.fa")).read()
    t = fx.t
    loci = pad_model.expected_loci(fx.places, t.start, t.end, t.bub_of, t.bubbles)
    w, D, a = 5, 2, 1
    differ = set()
    for flags, joined in (([], False), (["-B", data, "-R"], False), (["-B", data, "-J", "-R"], True)):
        items = [af] if joined else []
        # (places2sam takes its flags in one order: -A -a -I -w -G -q -d -b -Y)
        outs = lambda E=0: ["-A", tmp_path / "a.tsv", "-a", a] + (["-I", tmp_path / "i.tsv"] if flags else []) + ["-w", w, "-G", tmp_path / "g.tsv"] + (["-q", E] if E else []) + ["-d", D]
        names = ["o.sam", "a.tsv", "g.tsv"] + (["i.tsv"] if flags else [])
        files = lambda: [open(tmp_path / n, "rb").read() for n in names]
        assert run(["places2sam"] + flags + outs() + [ref, fq, pf, tmp_path / "o.sam"] + items).returncode == 0
        base = files()
        # what SAM prints under the bases is the rewritten line, reversed on the reverse strand
        assert run(["places2sam"] + flags + [ref, os.path.join(pad_text, "pad_bub.fq"), pf, tmp_path / "orig.sam"] + items).returncode == 0
        assert base[0] == pileq_model.requal_sam(open(tmp_path / "orig.sam", "rb").read(), quals)
        r = run(["places2sam"] + flags + outs() + ["-b", 0, ref, fq, pf, tmp_path / "o.sam"] + items)
        assert r.returncode == 0 and files() == base and "base qualities" not in r.stdout, r.stdout
        bub_counts = indel_model.count(indel_model.from_records(fx.places, loci, fx.joins["mapq"] if joined else None), t.bubbles, t.chrom, w, a)[0] if flags else None
        for m, E in SETTINGS:
            r = run(["places2sam"] + flags + outs(E) + ["-b", m] + (["-Y"] if E else []) + [ref, fq, pf, tmp_path / "o.sam"] + items)
            assert r.returncode == 0, r.stdout
            got = files()
            assert got[0] == base[0] and got[3:] == base[3:]  # SAM and -I: not affected
            counts, sums, reads, adds, dropped = pileq_model.pile_sam_q(base[0], toy.text, toy.names, toy.starts, a, m, E)
            assert got[1] == pile_model.tsv(toy.text, toy.names, toy.starts, counts), (flags, m, E)
            assert f"reads counted {reads}  adds {adds}" in r.stdout and (not (m or E) or f"minimum {m}  bases dropped {dropped}" in r.stdout), r.stdout
            ca, sa = pileq_model.table_arrays(toy.text, counts, sums)
            bubs = geno_model.bubble_records(t.bubbles, bub_counts, w, E or 20, D) if flags else ()
            if E:
                sites = pileq_model.site_records_q(toy.text, ca, sa, D)
                want = pileq_model.calls_bytes_q(toy.text, toy.names, toy.starts, sites, t.bubbles, bubs)
                assert got[2] == want, (flags, m, E, pad_model.first_difference(got[2], want))
                judged = judged_calls(pileq_model.judge_sam_q(base[0], fasta, a, m, E), D)
                assert {(f[1], f[2]): (f[3], f[5], f[6], f[7], f[8], f[9], f[10]) for f in pileq_model.parse_calls_q(got[2]) if f[0] == "S"} == judged
                assert all(f[10] is None for f in pileq_model.parse_calls_q(got[2]) if f[0] == "I") and (not flags or b"\nI\t" in got[2])
                differ.add(got[2])
            else:
                want = geno_model.calls_bytes(toy.text, toy.names, toy.starts, geno_model.site_records(toy.text, ca, 20, D), t.bubbles, bubs)
                assert got[2] == want, (flags, m, pad_model.first_difference(got[2], want))
            assert (got[1] == base[1]) == (m == 0)
    assert len(differ) >= 9


@pytest.mark.parametrize("E,byte", [(20, b"5"), (20, b"I"), (40, b"I"), (93, b"~"), (93, b"\x7f"), (4, b"%")])
def test_qualities_that_all_reach_E_give_the_unweighted_calls(ref, golden, pad_text, fx, toy, tmp_path, E, byte):
    """every quality >= E: s_x = E n_x, and -Y writes the GT, GQ and PL of the run without it, number for number, with QS = E x AD"""
    assert pileq_model.base_q(byte[0]) >= E
    pf, af = write_inputs(fx, tmp_path)
    fq, data = tmp_path / "q.fq", os.path.join(golden, "pad_toy.data")
    requalled(os.path.join(pad_text, "pad_bub.fq"), fq, 0, lambda name, n: byte * n)
    cmd = lambda more, f: ["places2sam", "-B", data, "-J", "-R", "-w", 5, "-G", tmp_path / f, "-q", E] + more + [ref, fq, pf, tmp_path / "o.sam", af]
    assert run(cmd([], "plain.tsv")).returncode == 0 and run(cmd(["-b", E, "-Y"], "y.tsv")).returncode == 0
    plain = geno_model.parse_calls(open(tmp_path / "plain.tsv", "rb").read())
    weighted = pileq_model.parse_calls_q(open(tmp_path / "y.tsv", "rb").read())
    assert [f[:10] for f in weighted] == plain and len(plain) > 50
    assert all(f[10] == [E * n for n in f[5]] for f in weighted if f[0] == "S") and any(f[0] == "I" for f in weighted)


@pytest.mark.parametrize("what", ["b_alone", "b_with_I_only", "b_94", "b_minus", "b_text", "Y_alone", "Y_with_A_only", "unwritable_A", "unwritable_G"])
def test_refusals_leave_no_file(ref, golden, pad_text, fx, tmp_path, what):
    fq, out, counts, calls, ind = os.path.join(pad_text, "pad_bub.fq"), tmp_path / "out.sam", tmp_path / "counts.tsv", tmp_path / "calls.tsv", tmp_path / "i.tsv"
    data = os.path.join(golden, "pad_toy.data")
    opts = {"b_alone": ["-b", 20], "b_with_I_only": ["-I", ind, "-b", 20], "b_94": ["-A", counts, "-b", 94], "b_minus": ["-G", calls, "-b", -1], "b_text": ["-A", counts, "-b", "2o"],
            "Y_alone": ["-Y"], "Y_with_A_only": ["-A", counts, "-Y"], "unwritable_A": ["-A", tmp_path / "no_such_dir" / "c.tsv", "-b", 20],
            "unwritable_G": ["-G", tmp_path / "no_such_dir" / "g.tsv", "-b", 20, "-Y"]}[what]
    want = {"b_alone": "-b needs -A", "b_with_I_only": "-b needs -A", "Y_alone": "-Y needs -G", "Y_with_A_only": "-Y needs -G", "unwritable_A": "Cannot open the counts file",
            "unwritable_G": "Cannot open the calls file"}.get(what, "0..93")
    pf, _ = write_inputs(fx, tmp_path)
    for cmd in (["places2sam", "-B", data] + opts + [ref, fq, pf, out], ["aln2sam", "-B", data] + opts + [ref, fq, os.path.join(pad_text, "pad_bub_n3.aln"), out],
                ["map", "-n", "3", "-B", data] + opts + [ref, fq, out]):
        r = run(cmd)
        assert r.returncode == 1 and not any(p.exists() for p in (out, counts, calls, ind)), (cmd[0], r.stdout)
        assert want in r.stdout, (cmd[0], r.stdout)


def test_usage_names_the_flags(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-G <calls.tsv> [-q <int>] [-d <int>]] [-b <int>] [-Y]" in r.stdout and "-I is not affected" in r.stdout and "last column QS" in r.stdout
    assert "-b, -Y" in run(["aln2sam"]).stdout and "-I is not affected" in run(["aln2sam"]).stdout and "[-b <baseq>] [-Y]" in run(["places2sam"]).stdout


def test_layout_of_the_record(built, tmp_path):
    """bwb_geno_site_q as the C compiler sees it == the dtype: the 64 bytes of bwb_geno_site, then qs"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwbble_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(bwb_geno_site_q), offsetof(bwb_geno_site_q, site), '
                   'offsetof(bwb_geno_site_q, qs), sizeof(bwb_geno_site)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    dt = bw.GENO_SITE_Q_DTYPE
    assert got == [dt.itemsize, 0, dt.fields["qs"][1], bw.GENO_SITE_DTYPE.itemsize] == [80, 0, 64, 64]
    assert all(dt.fields[f][1] == bw.GENO_SITE_DTYPE.fields[f][1] for f in bw.GENO_SITE_DTYPE.names)


def test_host_rule_called_by_itself_under_the_sanitizers(built, tmp_path):
    """`pile.c: pile_host_q`, the weighted `geno.c: geno_host` and `geno_write` in a program of their own, with the tool's compiler flags plus the
    address and undefined-behaviour sanitizers, on the edge cases of test_pile_host under every quality byte 0..255, both strands, min MAPQ 10,
    -b 20 -Y with E = 30: the model's counts, sums, reads, adds, dropped bases and calls file; and -b 0 without -Y through the same function"""
    text, cases = edge_cases()
    rows, placements, qbytes, qoff = [], [], bytearray(), []
    for start, cig, seq, mapq in cases:
        for rev in (0, 1):
            fwd = seq[::-1].translate(md_model.COMP) if rev else seq  # the read as uploaded
            ops = md_model.parse_cigar(cig)
            line = bytes((7 * len(rows) + 3 * i * i + (37 if rev else 0)) % 256 for i in range(len(fwd)))  # the quality line in FASTQ order: every byte value occurs
            rows.append('{ %d, %d, %d, %d, "%s", %d, { %s } }' % (start, rev, mapq, len(fwd), "".join(str("AGCTN".index(c)) for c in fwd), len(ops),
                                                                   ", ".join(f"{(k << 4) | 'MID?S'.index(op)}u" for k, op in ops)))
            qoff.append(len(qbytes))
            qbytes += line
            placements.append((start, ops, seq, mapq, line[::-1] if rev else line))
    assert set(qbytes) == set(range(256))
    m, E, D = 20, 30, 2
    counts, sums, reads, adds, dropped = pileq_model.pile_q(text, placements, 10, m, E)
    ca, sa = pileq_model.table_arrays(text, counts, sums)
    plain = pile_model.pile(text, [p[:4] for p in placements], 10)
    assert dropped > 0 and adds + dropped == plain[2] and reads == plain[1]
    two = text.index("$") + 1
    src = tmp_path / "rule.c"
    src.write_text("""
#include <stdarg.h>
#include <string.h>
#include "bwb_host.h"
void bwb_die(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); exit(1); }
int sam_mapq(int top1, int top2, int num_mm, int max_mm) { (void)top1; (void)top2; (void)num_mm; (void)max_mm; return 0; } /* (pad.c: join_resolve, not called here) */
static const struct { long long start; int rev, mapq; unsigned len; const char *seq; unsigned n_ops; uint32_t ops[24]; } cases[] = { %s };
static uint8_t text[] = { %s };
static const uint8_t quals[] = { %s };
static const size_t qoff[] = { %s };
enum { N = sizeof(cases) / sizeof(cases[0]) };
int main(int argc, char **argv) {
	(void)argc;
	/* every case as a lifted primary of record 0, which begins at text position 0: the ops as they are, from position start + 1 */
	md_text_t t = { .codes = text, .n_fwd = sizeof(text), .ready = 1 };
	seq_annotation_t rec[2] = { { .name = "one", .start_index = 0, .end_index = %d }, { .name = "two", .start_index = %d, .end_index = sizeof(text) - 1 } };
	fasta_annotations_t ann = { .num_seq = 2, .seq_anns = rec };
	bwb_place *pl = (bwb_place *)calloc(N, sizeof(bwb_place));
	uint8_t *seq = (uint8_t *)calloc(N, 255), *kind = (uint8_t *)malloc(N);
	uint16_t *len = (uint16_t *)calloc(N, 2);
	uint64_t *off = (uint64_t *)calloc(N + 1, 8);
	bwb_lift *recs = (bwb_lift *)calloc(N * 7, sizeof(bwb_lift));
	/* (the quality lines in a buffer of exactly their bytes: a byte read beyond a line's end at the buffer's end is the sanitizer's to find) */
	char *qtext = (char *)malloc(sizeof(quals));
	memcpy(qtext, quals, sizeof(quals));
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
	p->min_baseq = %d; p->err_cap = %d;
	pile_set_text(p, &t, 1);
	const uint64_t reads = pile_host_q(p, pl, N, seq, 255, len, qtext, qoff, kind, off, recs, NULL, &ann);
	printf("%%llu %%llu %%llu %%llu %%llu\\n", (unsigned long long)p->n_sites, (unsigned long long)reads, (unsigned long long)p->reads, (unsigned long long)p->adds, (unsigned long long)p->dropped);
	for (uint64_t s = 0; s < p->n_sites; s++) printf("%%u %%u %%u %%u %%u %%u %%u %%u\\n", p->counts[4 * s], p->counts[4 * s + 1], p->counts[4 * s + 2], p->counts[4 * s + 3],
	                                                 p->qsum[4 * s], p->qsum[4 * s + 1], p->qsum[4 * s + 2], p->qsum[4 * s + 3]);
	geno_t *g = geno_open(argv[1], p->err_cap, %d);
	g->weighted = 1;
	geno_host(g, p, NULL);
	printf("%%llu ", (unsigned long long)g->n_sites);
	printf("%%llu\\n", (unsigned long long)geno_write(g, &ann, NULL));
	/* -b 0 without -Y through the same function: no quality is read (none is given) and the table is pile_host's */
	pile_t *q = pile_open(NULL, 10), *q0 = pile_open(NULL, 10);
	pile_set_text(q, &t, 1); pile_set_text(q0, &t, 1);
	const uint64_t ra = pile_host_q(q, pl, N, seq, 255, len, NULL, NULL, kind, off, recs, NULL, &ann), rb = pile_host(q0, pl, N, seq, 255, len, kind, off, recs, NULL, &ann);
	printf("%%d\\n", ra == rb && q->adds == q0->adds && !q->qsum && !q->dropped && !memcmp(q->counts, q0->counts, (size_t)q->n_sites * 16));
	geno_free(g); pile_free(p); pile_free(q); pile_free(q0);
	free(pl); free(seq); free(kind); free(len); free(off); free(recs); free(qtext);
	return 0;
}
""" % (",\n".join(rows), ", ".join(str(c) for c in pile_model.codes(text)), ", ".join(str(b) for b in qbytes), ", ".join(str(o) for o in qoff), two - 1, two, m, E, D))
    exe = tmp_path / "rule"
    host = os.path.join(ROOT, "bwbble_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", host,
                    str(src), os.path.join(host, "geno.c"), os.path.join(host, "pile.c"), os.path.join(host, "md.c"), os.path.join(host, "indel.c"), os.path.join(host, "pad.c"), "-o", str(exe), "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe), str(tmp_path / "calls.tsv")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.split("\n")[:-1]
    assert lines[0] == f"{len(ca)} {reads} {reads} {adds} {dropped}", (lines[0], len(ca), reads, adds, dropped)
    got = np.array([[int(x) for x in ln.split()] for ln in lines[1:1 + len(ca)]], dtype=np.uint32)
    assert np.array_equal(got[:, :4], ca) and np.array_equal(got[:, 4:], sa), np.flatnonzero((got != np.hstack([ca, sa])).any(axis=1))[:5]
    model_text = text + "$"  # (the records as the model's writer finds them: up to a `$`)
    sites = pileq_model.site_records_q(model_text, ca, sa, D)
    want = pileq_model.calls_bytes_q(model_text, ["one", "two"], [0, two], sites)
    assert open(tmp_path / "calls.tsv", "rb").read() == want and lines[1 + len(ca)] == f"{len(sites)} {len(sites)}" and len(sites) > 20
    assert lines[-1] == "1"
    # the weights flip calls here: some site's GT differs from the unweighted rule's on the same counts
    plain_gt = {int(r["site"]): int(r["gt"]) for r in geno_model.site_records(model_text, ca, E, D)}
    assert any(plain_gt[int(r["site"])] != int(r["gt"]) for r in sites)


# ---- the truth census: read errors at a low quality -------------------------------------------------------------------------------------------

ERR_SEED, ERR_EVERY, Q_ERR, Q_GOOD = 5, 23, 5, 35


@pytest.fixture(scope="module")
def chains(built, oracle, tmp_path_factory):
    """the diploid sample of geno_model with seeded substitution errors written into the reads at Q 5, every other base at Q 35, mapped without a
    GPU (the oracle's align, the models' records, places2sam) with and without -Y"""
    import random
    import types

    import map_model
    import oracle_lib
    d = str(tmp_path_factory.mktemp("pileq_chain"))
    path = lambda n: os.path.join(d, n)
    g = lift_model.genome()
    sample = geno_model.diploid(g)
    rnd = random.Random(ERR_SEED)
    fq, n_err = [], 0
    for name, seq in sample.reads:
        seq, qual = list(seq), [chr(33 + Q_GOOD)] * len(seq)
        for i in range(len(seq)):
            if rnd.randrange(ERR_EVERY) == 0:
                seq[i], qual[i] = rnd.choice([c for c in "ACGT" if c != seq[i]]), chr(33 + Q_ERR)
                n_err += 1
        fq.append(f"@{name}\n{''.join(seq)}\n+\n{''.join(qual)}\n")
    fa, fqp, data, aln = path("dip.fa"), path("dip.fq"), path("dip.data"), path("dip.aln")
    open(fa, "w").write(g["fasta"])
    open(data, "wb").write(g["data"])
    open(fqp, "w").write("".join(fq))
    assert run(["index", fa]).returncode == 0 and run(["fasta2ref", fa]).returncode == 0
    n, _, _ = oracle.align_fastq(fa + ".bwt", fqp, aln, oracle.params(geno_model.ALIGN + ["-t", str(min(16, os.cpu_count() or 1))]))
    hits = oracle_lib.parse_aln(open(aln, "rb").read())
    idx = oracle.load_index(fa + ".bwt", load_sa=True)
    places, _ = map_model.expected_places(oracle, idx, hits, geno_model.MAX_MM)
    off, alts, _ = alt_model.expected_alts(hits, geno_model.MAX_ALT, alt_model.OracleSA(oracle, idx))
    sub = join_model.suboptimal(hits, off, alts)
    oracle.lib.bwb_or_free_index(idx)
    places.tofile(path("places.bin"))
    open(path("alts.bin"), "wb").write(join_model.alts_file_bytes(off, alts, sub))
    out = {}
    for what, more in (("plain", []), ("weighted", ["-Y"]), ("filtered", ["-b", 10]), ("filtered and weighted", ["-b", 10, "-Y"])):
        r = run(["places2sam", "-B", data, "-J", "-R", "-a", geno_model.MIN_MAPQ, "-w", geno_model.ANCHOR, "-G", path("calls.tsv")] + more + [fa, fqp, path("places.bin"), path("o.sam"), path("alts.bin")])
        assert r.returncode == 0, r.stdout
        calls = open(path("calls.tsv"), "rb").read()
        if "-Y" in more:
            calls = geno_model.HEADER + b"".join(ln.rsplit(b"\t", 1)[0] + b"\n" for ln in calls.split(b"\n")[1:-1])
        out[what] = types.SimpleNamespace(g=g, sample=sample, calls=calls)
    return out, n_err, n


# (sites called, sites wrong, sites wrong among GQ >= 20, sites with GQ >= 20), measured on the reads above - 1 721 reads, 7 425 error bases, one about
# every 23rd base - against the unweighted rule on the same reads; not chosen in advance.  All four runs give the same figures: at 25 x per haplotype
# a site's few error bases outweigh its true alleles under neither rule, so -Y equals the unweighted rule on wrong calls among GQ >= 20 (none), and
# the one wrong call, below GQ 20, stays wrong under -Y and under -b 10.
CENSUS_FIGURES = {"plain": (27, 1, 0, 24), "weighted": (27, 1, 0, 24), "filtered": (27, 1, 0, 24), "filtered and weighted": (27, 1, 0, 24)}


def wrong_calls(m):
    """(sites called, sites wrong, sites wrong among GQ >= 20, sites with GQ >= 20) of a chain's S lines against the drawn genotypes"""
    g, sample = m.g, m.sample
    chrom_name = g["names"][0].split()[0]
    cmaps = {r[0].split()[0]: r[2] for r in g["records"]}
    called = wrong = wrong20 = conf = 0
    for kind, rec, pos, ident, alleles, ad, other, gt, gq, pl in geno_model.parse_calls(m.calls):
        at = (pos if rec == chrom_name else cmaps[rec][pos - 1]) if kind == "S" else None
        if at is None or at not in sample.sites:
            continue
        called += 1
        conf += gq >= 20
        wrong += gt != sample.sites[at]
        wrong20 += gt != sample.sites[at] and gq >= 20
    return called, wrong, wrong20, conf


def test_truth_census_with_errors_at_a_low_quality(chains):
    out, n_err, n_reads = chains
    figures = {what: wrong_calls(m) for what, m in out.items()}
    print("reads", n_reads, "error bases", n_err, "(sites called, wrong, wrong among GQ >= 20, GQ >= 20):", figures)
    assert (n_reads, n_err) == (1721, 7425)
    assert figures == CENSUS_FIGURES, figures
    # -Y is at least as good as the unweighted rule on wrong calls among GQ >= 20, on the same reads
    assert figures["weighted"][2] <= figures["plain"][2] and figures["filtered and weighted"][2] <= figures["filtered"][2]

