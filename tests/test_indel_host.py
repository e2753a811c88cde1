"""Ref / alt read support per indel bubble (`-I`) without a GPU: the model against the judge that walks no CIGAR (tests/indel_model.py) on the
generated genome, with the census of the reference's own placements; the host's rule and the writer (`places2sam -B t ... -I f -w n -a m`)
against the model's bytes on the generated genome and on the pad_bub reads; the refusals; the usage texts; the layout of the records the
kernel reads; and `indel.c: indel_host` in a program of its own under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import bwbble_amd as bw
import indel_model
import lift_model
import md_model
import pad_model
from test_md_host import fx, pad_text, ref, run, toy, write_inputs  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bwbble")


@pytest.fixture(scope="module")
def gen(built, tmp_path_factory):
    """the generated genome of lift_model with the reads of indel_model placed where they were cut, after `fasta2ref`"""
    d = tmp_path_factory.mktemp("indel_gen")
    g = lift_model.genome()
    reads = indel_model.reads(g)
    (d / "gen.fa").write_text(g["fasta"])
    (d / "gen.data").write_bytes(g["data"])
    (d / "gen.fq").write_text(indel_model.fastq(reads))
    assert run(["fasta2ref", d / "gen.fa"]).returncode == 0
    names, start, end = bw.read_ann(d / "gen.fa.ann")
    assert list(names) == g["names"]
    indel_model.truth_records(g, reads, start).tofile(d / "places.bin")
    chrom = np.zeros(len(g["bubbles"]), dtype=np.int32)
    return types.SimpleNamespace(g=g, reads=reads, dir=d, names=g["names"], start=start, end=end, chrom=chrom, bub_of=pad_model.bubble_of(g["names"], g["bubbles"]))


def test_model_against_the_name_judge():
    """the expected table of the generated genome at w = 1, 5 and 30: the CIGAR walk equals the interval arithmetic on the names"""
    g = lift_model.genome()
    reads = indel_model.reads(g)
    bubbles = g["bubbles"]
    kinds = [b[0] for b in lift_model.BUBBLES]
    chrom = [0] * len(bubbles)
    assert len(reads) == 3004 and {r[6] for r in reads} == {None, "I", "D"} and {r[5] for r in reads} == {"+", "-"} and {r[4] for r in reads} == {100, 60}
    tables = {}
    for w in indel_model.ANCHORS + (61,):
        counts, n_reads, adds = indel_model.count(indel_model.truth(g, reads), bubbles, chrom, w)
        want = indel_model.judged_table(reads, bubbles, w)
        assert np.array_equal(counts, want), (w, np.flatnonzero((counts != want).any(axis=1)))
        assert n_reads == len(reads) and adds == int(counts.sum())
        tables[w] = counts
        print("anchor", w, "adds", adds, counts.tolist())
        # tail has no right flank (D_minus_C = -1): no line at any anchor
        assert not counts[kinds.index("tail")].any() and not indel_model.eligible(bubbles[kinds.index("tail")], w)
        text = indel_model.table_bytes(bubbles, counts)
        assert text.startswith(indel_model.HEADER) and text.count(b"\n") == 1 + int(counts.any(axis=1).sum())
    head = bubbles[kinds.index("head")]
    # head's left flank is the 60 bases before it: it is eligible up to an anchor of 60 and has its line there; from 61 on it has none
    assert head[2] == 60 and indel_model.eligible(head, 30) and indel_model.eligible(head, 60) and not indel_model.eligible(head, 61)
    assert tables[30][kinds.index("head")].any() and not tables[61].any()
    # every eligible bubble has clean reads for both alleles at 1 and 5 (the reads of 100 bases cannot contain the 130 deleted bases and two anchors)
    for w in (1, 5):
        for k, kind in enumerate(kinds):
            if kind != "tail":
                assert tables[w][k][indel_model.ALT] > 0 and (tables[w][k][indel_model.REF] > 0) == (kind != "del130"), (w, kind)
    # the gapped classes come from the edited reads, at the anchor they were made for
    assert tables[5][:, indel_model.REF_GAPPED].sum() > 0 and tables[5][:, indel_model.ALT_GAPPED].sum() > 0 and not tables[1][:, 2:].any()
    assert (tables[1] >= tables[5]).all() or tables[5][:, 2:].any()


def test_classes_of_the_rule():
    """the classes one by one on a window 10 .. 14"""
    c = indel_model.classify
    assert c(1, "20M", 10, 14) == 1 and c(10, "5M", 10, 14) == 1 and c(11, "5M", 10, 14) == 0 and c(10, "4M", 10, 14) == 0 and c(9, "5M", 10, 14) == 0
    assert c(1, "9M1D10M", 10, 14) == 0 and c(1, "13M1D6M", 10, 14) == 0          # D on lo, D on hi
    assert c(1, "10M1D9M", 10, 14) == 2 and c(1, "12M2D6M", 10, 14) == 0           # D inside; a D that ends on hi
    assert c(1, "10M1I10M", 10, 14) == 2 and c(1, "13M1I7M", 10, 14) == 2          # I just inside at either end
    assert c(1, "9M1I11M", 10, 14) == 1 and c(1, "14M1I6M", 10, 14) == 1           # I just outside
    assert c(1, "8M1D11M", 10, 14) == 1 and c(1, "14M1D6M", 10, 14) == 1           # D just outside
    assert c(8, "2I7M", 10, 14) == 1 and c(10, "5M3I", 10, 14) == 1 and c(1, "3M1I2M1D1M1I3M1D8M", 10, 14) == 2


def model_of(gen, w, min_mapq=0):
    return indel_model.count(indel_model.truth(gen.g, gen.reads), gen.g["bubbles"], gen.chrom, w, min_mapq)


@pytest.mark.parametrize("w", [None, 1, 5, 30, 61, 255])
def test_host_rule_and_writer_on_the_generated_genome(gen, w):
    """`places2sam -B t [-R] -I f [-w n]`: the model's bytes, with and without -R; the SAM bytes are those of the run without -I"""
    d = gen.dir
    anchor = 1 if w is None else w
    counts, reads, adds = model_of(gen, anchor)
    want = indel_model.table_bytes(gen.g["bubbles"], counts)
    assert np.array_equal(counts, indel_model.judged_table(gen.reads, gen.g["bubbles"], anchor))
    for lift in ([], ["-R"]):
        base = ["places2sam", "-B", d / "gen.data"] + lift
        tail = [d / "gen.fa", d / "gen.fq", d / "places.bin"]
        assert run(base + tail + [d / "plain.sam"]).returncode == 0
        r = run(base + ["-I", d / "indels.tsv"] + (["-w", w] if w is not None else []) + tail + [d / "out.sam"])
        assert r.returncode == 0, r.stdout
        got = open(d / "indels.tsv", "rb").read()
        assert got == want, (lift, pad_model.first_difference(got, want))
        assert f"anchor {anchor}  eligible bubbles {sum(indel_model.eligible(b, anchor) for b in gen.g['bubbles'])}  refused and skipped 0  reads counted {reads}  adds {adds}" in r.stdout, r.stdout
        assert open(d / "out.sam", "rb").read() == open(d / "plain.sam", "rb").read()
        # the model fed the SAM text that was written says the same
        again, _, _ = indel_model.count(indel_model.from_sam(open(d / "out.sam", "rb").read(), gen.names, gen.bub_of), gen.g["bubbles"], gen.chrom, anchor)
        assert np.array_equal(again, counts)
    if anchor >= 61:
        assert want == indel_model.HEADER


def test_min_mapq_on_the_generated_genome(gen):
    """-a: the placement records carry MAPQ 37 - one below, at, one above"""
    d = gen.dir
    for q, some in ((36, True), (37, True), (38, False)):
        r = run(["places2sam", "-B", d / "gen.data", "-a", q, "-I", d / "q.tsv", "-w", 5, d / "gen.fa", d / "gen.fq", d / "places.bin", d / "q.sam"])
        assert r.returncode == 0, r.stdout
        counts, reads, _ = model_of(gen, 5, q)
        assert open(d / "q.tsv", "rb").read() == indel_model.table_bytes(gen.g["bubbles"], counts) and bool(counts.any()) == some == (reads > 0)


def test_refused_bubbles_are_skipped(gen, tmp_path):
    """a bubble whose flanks overlap (gap < 0) beside the good ones: -R stops at it, -I skips it, counts the others and says how many"""
    bubbles = list(gen.g["bubbles"])
    _, A, Bm, C, Dm, ref_len, alt = bubbles[2]
    bubbles[2] = (bubbles[2][0], A, Bm, A + Bm - 1, Dm, ref_len, alt)
    data = tmp_path / "bad.data"
    data.write_bytes(b"".join(b[0] + b"\n" + b"\t".join(b"%d" % v for v in b[1:]) + b"\n" for b in bubbles))
    d = gen.dir
    r = run(["places2sam", "-B", data, "-I", tmp_path / "i.tsv", d / "gen.fa", d / "gen.fq", d / "places.bin", tmp_path / "o.sam"])
    assert r.returncode == 0 and "refused and skipped 1 " in r.stdout, r.stdout
    counts, _, _ = indel_model.count(indel_model.truth(gen.g, gen.reads), bubbles, gen.chrom, 1)
    assert not counts[2].any() and counts[[0, 1, 3]].any(axis=1).all()
    assert open(tmp_path / "i.tsv", "rb").read() == indel_model.table_bytes(bubbles, counts)
    r = run(["places2sam", "-B", data, "-R", "-I", tmp_path / "j.tsv", d / "gen.fa", d / "gen.fq", d / "places.bin", tmp_path / "p.sam"])
    assert r.returncode == 1 and not (tmp_path / "j.tsv").exists(), r.stdout


def test_pad_bub_reads_plain_and_joined(ref, golden, pad_text, fx, tmp_path):
    """the pad_bub reads on pad_toy.data (`-n 3 -X 5 -B -J`), -a 0 and 20, anchors 1 and 10: the host's bytes are the model's fed the model's own
    placement, locus and join records; and the reads' names (bubble<k>_o<offset>_l<length>) say which of them contain their bubble's window"""
    pf, af = write_inputs(fx, tmp_path)
    fq, data = os.path.join(pad_text, "pad_bub.fq"), os.path.join(golden, "pad_toy.data")
    t = fx.t
    loci = pad_model.expected_loci(fx.places, t.start, t.end, t.bub_of, t.bubbles)
    names = [ln[1:].strip() for ln in open(fq).read().split("\n")[0::4] if ln]
    assert len(names) == len(fx.places)
    seen = set()
    for joined in (False, True):
        for q in (0, 20):
            for w in (1, 10):
                mapq = fx.joins["mapq"] if joined else None
                counts, reads, adds = indel_model.count(indel_model.from_records(fx.places, loci, mapq), t.bubbles, t.chrom, w, q)
                out = tmp_path / "i.tsv"
                r = run(["places2sam", "-B", data] + (["-J"] if joined else []) + ["-a", q, "-I", out, "-w", w, ref, fq, pf, tmp_path / "o.sam"] + ([af] if joined else []))
                assert r.returncode == 0, r.stdout
                got, want = open(out, "rb").read(), indel_model.table_bytes(t.bubbles, counts)
                assert got == want, (joined, q, w, pad_model.first_difference(got, want))
                assert f"reads counted {reads}  adds {adds}" in r.stdout
                seen.add((joined, q, w, want))
                if q == 0 and not joined:
                    # the name judge: an error-free read placed on its own bubble's record at its offset is clean for alt exactly when it contains the window
                    alt = np.zeros(len(t.bubbles), dtype=np.int64)
                    for name, pl, lc in zip(names, fx.places, loci):
                        m = re.match(r"bubble(\d+)_o(\d+)_l(\d+)_[+-]$", name)
                        if not m:
                            continue
                        k, o, ln = (int(v) for v in m.groups())
                        if int(lc["bubble"]) == k and int(lc["pos1"]) == o + 1 and int(pl["aln_length"]) == ln and (pl["gap_run"] == 0xFFFF).all() and indel_model.eligible(t.bubbles[k], w):
                            lo, hi = indel_model.windows(t.bubbles[k], w)[0]
                            alt[k] += o + 1 <= lo and hi <= o + ln
                    assert alt.sum() > 0 and (counts[:, indel_model.ALT] >= alt).all()
    # the anchor changes the table; a read that contains its bubble's allele and an anchor on either side lies nowhere else, so neither -a 20 nor the joined MAPQ does
    assert len({s[3] for s in seen}) == len({s[3] for s in seen if not s[0] and not s[1]}) == 2


@pytest.mark.parametrize("what", ["I_without_B", "w_without_I", "w_0", "w_256", "w_text", "a_alone", "unwritable"])
def test_refusals_leave_no_file(ref, golden, pad_text, fx, tmp_path, what):
    fq, out, ind = os.path.join(pad_text, "pad_bub.fq"), tmp_path / "out.sam", tmp_path / "indels.tsv"
    data = os.path.join(golden, "pad_toy.data")
    opts = {"I_without_B": ["-I", ind], "w_without_I": ["-B", data, "-w", 5], "w_0": ["-B", data, "-I", ind, "-w", 0], "w_256": ["-B", data, "-I", ind, "-w", 256],
            "w_text": ["-B", data, "-I", ind, "-w", "5x"], "a_alone": ["-B", data, "-a", 3], "unwritable": ["-B", data, "-I", tmp_path / "no_such_dir" / "indels.tsv"]}[what]
    pf, _ = write_inputs(fx, tmp_path)
    for cmd in (["places2sam"] + opts + [ref, fq, pf, out], ["aln2sam"] + opts + [ref, fq, os.path.join(pad_text, "pad_bub_n3.aln"), out], ["map", "-n", "3"] + opts + [ref, fq, out]):
        r = run(cmd)
        assert r.returncode == 1 and not out.exists() and not ind.exists(), (cmd[0], r.stdout)
        want = {"I_without_B": "-I needs -B", "w_without_I": "-w needs -I", "a_alone": "-a needs -A", "unwritable": "Cannot open the indel support file"}.get(what, "1..255")
        assert want in r.stdout, (cmd[0], r.stdout)


def test_an_unwritable_counts_file_leaves_no_indel_file(ref, golden, pad_text, fx, tmp_path):
    """-A and -I together: the file that was opened first is removed when the second cannot be"""
    pf, _ = write_inputs(fx, tmp_path)
    r = run(["places2sam", "-B", os.path.join(golden, "pad_toy.data"), "-A", tmp_path / "c.tsv", "-I", tmp_path / "no_such_dir" / "i.tsv", ref, os.path.join(pad_text, "pad_bub.fq"), pf, tmp_path / "o.sam"])
    assert r.returncode == 1 and not (tmp_path / "c.tsv").exists() and not (tmp_path / "o.sam").exists(), r.stdout


def test_usage_names_the_flags(built):
    r = run(["map", "-n", "3"])
    assert r.returncode == 1 and "[-I <indels.tsv> [-w <int>]]" in r.stdout and "bubble<TAB>chrom<TAB>pos<TAB>ref_len<TAB>alt_len<TAB>ref<TAB>alt<TAB>ref_gapped<TAB>alt_gapped" in r.stdout
    assert "-I, -w" in run(["aln2sam"]).stdout and "[-a <MAPQ>] [-I <indels.tsv>] [-w <anchor>]" in run(["places2sam"]).stdout


def test_layout_of_the_records_the_kernel_reads(built, tmp_path):
    """k_indel takes bwb_place, bwb_locus, bwb_join and bwb_bubble apart by 16-byte words: the fields it reads lie where the dtypes say"""
    src = tmp_path / "layout.c"
    fields = [("bwb_place", bw.PLACE_DTYPE, ("pos", "mapq", "flags", "aln_length", "gap_run")), ("bwb_locus", bw.LOCUS_DTYPE, ("seqid", "pos1", "bubble")),
              ("bwb_join", bw.JOIN_DTYPE, ("mapq",)), ("bwb_bubble", bw.BUBBLE_DTYPE, ("A", "B_minus_A", "C", "D_minus_C", "ref_len", "alt_len"))]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {']
    for s, dt, names in fields:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in names]
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    for s, dt, names in fields:
        assert int(got[s]) == dt.itemsize, s
        for f in names:
            assert int(got[f"{s}.{f}"]) == dt.fields[f][1], (s, f)
    assert (int(got["bwb_place"]), int(got["bwb_locus"]), int(got["bwb_join"]), int(got["bwb_bubble"])) == (48, 32, 16, 40)
    assert int(got["bwb_place.mapq"]) == 18 and int(got["bwb_place.flags"]) == 19 and int(got["bwb_place.aln_length"]) == 24 and int(got["bwb_place.gap_run"]) == 32


def edge_cases():
    """(bubbles, chrom_of, [(record, pos1, reverse, CIGAR, MAPQ)]) on records 0, 1 (chromosomes) and 2 + b (bubble b's): the rule's edges"""
    w = 4
    bubbles = [(b"c0", 100, 20, 120, 19, 0, 3),           # a pure insertion of 3 on chromosome 0: windows 17 .. 27 and 116 .. 123
               (b"c0", 100, 20, 125, 19, 5, 0),           # a deletion of 5 at the same position (a multi-allelic site): 17 .. 24 and 116 .. 128
               (b"c1", 100, 20, 120, 19, 0, 3),           # the first again on chromosome 1
               (b"c0", 300, w, 304, w - 1, 0, 1),         # Bm == w and Dm + 1 == w: eligible
               (b"c0", 300, w - 1, 303, w - 1, 0, 1),     # Bm one below
               (b"c0", 300, w, 304, w - 2, 0, 1),         # Dm + 1 one below
               (b"c0", 1, w, 5, 10, 0, 1),                # A + Bm - w == 1: eligible
               (b"c0", 0, w, 4, 10, 0, 1),                # ... == 0: not
               (b"c0", 500, 10, 509, 10, 0, 2),           # the flanks overlap: refused
               (b"c0", 600, 10, 610 + (1 << 28) - 1, 10, 0, 0),  # the longest gap the rule takes
               (b"c0", 700, 10, 710 + (1 << 28), 10, 0, 0)]      # one longer: refused
    chrom = [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    cases = []
    for rec in (0, 1):
        for pos1 in (115, 116, 117):      # the first M one before, at and one behind lo
            for ln in (7, 8, 9, 12, 13, 14):  # the last M one before, at and one behind either hi
                cases.append((rec, pos1, ln & 1, f"{ln}M", 30))
        cases += [(rec, 110, 0, c, 30) for c in ("6M1D20M", "13M1D10M", "18M1D10M", "7M1I20M", "6M1I20M", "14M1I10M", "13M1I10M", "8M2D18M", "5M1D1M1I3M1D2M1I20M", "4M1I1M1D1M1I1M1D1M1I1M1D1M1I1M1D20M")]
        cases += [(rec, 1, 0, "30M", 30), (rec, 1, 1, "8M", 30), (rec, 2, 0, "20M", 30), (rec, 296, 0, "12M", 30), (rec, 297, 1, "11M", 30), (rec, 100, 0, "30M", 9), (rec, 100, 1, "30M", 10), (rec, 100, 0, "30M", 11)]
    for b, (_, A, Bm, C, Dm, _, alt) in enumerate(bubbles):
        reclen = Bm + alt + Dm + 1
        for pos1, cig in ((1, f"{reclen}M"), (2, f"{max(1, reclen - 1)}M"), (1, f"{max(1, reclen - 1)}M"), (max(1, Bm - w + 1), f"{alt + 2 * w}M"), (max(1, Bm - w + 1), f"{w}M1I{alt + w}M"),
                          (max(1, Bm - w + 1), f"{w}M1D{alt + w}M"), (max(1, Bm - w), f"1M1I{alt + 2 * w}M"), (max(1, Bm - w + 2), f"{alt + 2 * w}M")):
            cases += [(2 + b, pos1, 0, cig, 30), (2 + b, pos1, 1, cig, 30)]
    return w, bubbles, chrom, cases


def test_host_rule_called_by_itself_under_the_sanitizers(built, tmp_path):
    """`indel.c: indel_host` in a program of its own, with the tool's compiler flags plus the address and undefined-behaviour sanitizers, on the
    edge cases, min MAPQ 10: the model's table, reads and adds; then with join records whose MAPQ decides"""
    w, bubbles, chrom, cases = edge_cases()
    placements = [(rec, rec - 2 if rec >= 2 else -1, pos1, cig, mapq, None) for rec, pos1, _, cig, mapq in cases]
    want, reads, adds = indel_model.count(placements, bubbles, chrom, w, 10)
    rows = []
    for rec, pos1, rev, cig, mapq in cases:
        alen, runs = lift_model.gap_runs(cig, bool(rev))
        rows.append("{ %d, %d, %d, %d, %d, { %s } }" % (rec, pos1, rev, mapq, alen, ", ".join(str(v) for v in runs)))
    src = tmp_path / "rule.c"
    src.write_text("""
#include <stdarg.h>
#include <string.h>
#include "bwb_host.h"
void bwb_die(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); exit(1); }
int sam_mapq(int top1, int top2, int num_mm, int max_mm) { (void)top1; (void)top2; (void)num_mm; (void)max_mm; return 0; } /* (pad.c: join_resolve, not called here) */
static const struct { int rec, pos1, rev, mapq, alen; uint16_t runs[8]; } cases[] = { %s };
static bwb_bubble bubs[] = { %s };
static int32_t chrom_of[] = { %s };
static char *anns[] = { %s };
enum { N = sizeof(cases) / sizeof(cases[0]), NB = sizeof(bubs) / sizeof(bubs[0]) };
int main(void) {
	bubble_table_t t = { .n = NB, .b = bubs, .ann = anns };
	bwb_place *pl = (bwb_place *)calloc(N, sizeof(bwb_place));
	bwb_locus *loci = (bwb_locus *)calloc(N, sizeof(bwb_locus));
	bwb_join *joins = (bwb_join *)calloc(N, sizeof(bwb_join));
	for (size_t k = 0; k < N; k++) {
		pl[k].flags = BWB_PLACE_MAPPED | (cases[k].rev ? BWB_PLACE_REVERSE : 0);
		pl[k].mapq = (uint8_t)cases[k].mapq; pl[k].aln_length = (uint16_t)cases[k].alen;
		memcpy(pl[k].gap_run, cases[k].runs, 16);
		loci[k].seqid = cases[k].rec; loci[k].pos1 = cases[k].pos1; loci[k].bubble = cases[k].rec >= 2 ? cases[k].rec - 2 : -1;
		joins[k].mapq = (uint8_t)(k %% 2 ? 10 : 9);
	}
	indel_t *p = indel_open(NULL, 10, %d);
	indel_set_table(p, &t, chrom_of);
	const uint64_t reads = indel_host(p, pl, loci, N, NULL, NULL);
	printf("%%llu %%llu %%llu %%llu %%llu\\n", (unsigned long long)p->n_tab, (unsigned long long)p->n_refused, (unsigned long long)reads, (unsigned long long)p->adds, (unsigned long long)p->cands);
	for (size_t b = 0; b < NB; b++) printf("%%u %%u %%u %%u\\n", p->counts[4 * b], p->counts[4 * b + 1], p->counts[4 * b + 2], p->counts[4 * b + 3]);
	indel_t *q = indel_open(NULL, 10, %d);
	indel_set_table(q, &t, chrom_of);
	pl[0].flags = 0; loci[1].seqid = -1; /* an unmapped read; a read in no record */
	printf("%%llu\\n", (unsigned long long)indel_host(q, pl, loci, N, NULL, joins));
	for (size_t b = 0; b < NB; b++) printf("%%u %%u %%u %%u\\n", q->counts[4 * b], q->counts[4 * b + 1], q->counts[4 * b + 2], q->counts[4 * b + 3]);
	indel_free(p); indel_free(q);
	free(pl); free(loci); free(joins);
	return 0;
}
""" % (",\n".join(rows), ", ".join("{ %dLL, %dLL, %dLL, %dLL, %d, %d }" % b[1:] for b in bubbles), ", ".join(str(c) for c in chrom), ", ".join('"%s x"' % b[0].decode() for b in bubbles), w, w))
    exe = tmp_path / "rule"
    host = os.path.join(ROOT, "bwbble_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", host,
                    str(src), os.path.join(host, "indel.c"), os.path.join(host, "pad.c"), "-o", str(exe), "-lm", "-lpthread"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.split("\n")[:-1]
    n_elig = sum(indel_model.eligible(b, w) for b in bubbles)
    head = [int(x) for x in lines[0].split()]
    assert head[:4] == [n_elig, 2, reads, adds] and head[4] >= adds, (lines[0], n_elig, reads, adds)
    nb = len(bubbles)
    got = np.array([[int(x) for x in ln.split()] for ln in lines[1:1 + nb]], dtype=np.uint32)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    # the census of the cases
    assert [indel_model.eligible(b, w) for b in bubbles] == [True, True, True, True, False, False, True, False, False, True, False]
    assert want[0].all() and want[1][[0, 1, 2]].all() and want[2][0] and want[3][1] and want[6][1] and not want[[4, 5, 7, 8, 10]].any()
    assert want[0][0] != want[1][0] and want[0][0] == want[2][0]  # two bubbles at one position differ by their hi; two chromosomes with bubbles at equal positions do not mix
    # the second call: MAPQ 10 from every second join record, one read unmapped, one in no record
    second = [None if k == 0 else (-1 if k == 1 else p[0], p[1], p[2], p[3], 10 if k % 2 else 9, None) for k, p in enumerate(placements)]
    want2, reads2, _ = indel_model.count(second, bubbles, chrom, w, 10)
    assert int(lines[1 + nb]) == reads2 and 0 < reads2 < reads
    assert np.array_equal(np.array([[int(x) for x in ln.split()] for ln in lines[2 + nb:2 + 2 * nb]], dtype=np.uint32), want2)


def census(ref_bin, work):
    """where the reference's own `index` + `align -n 3 -o 1` + `aln2sam` place the generated reads: every error-free read that the name judge
    calls clean for some bubble, at some anchor of the tests, must lie on the record it was cut from, at its offset, ungapped"""
    g = lift_model.genome()
    reads = indel_model.reads(g)
    fa, fq, aln, sam = (os.path.join(work, n) for n in ("gen.fa", "gen.fq", "gen.aln", "gen.sam"))
    open(fa, "w").write(g["fasta"])
    open(fq, "w").write(indel_model.fastq(reads))
    for cmd in (["index", fa], ["align", "-n", "3", "-o", "1", fa, fq, aln], ["aln2sam", fa, fq, aln, sam]):
        subprocess.run([ref_bin] + cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    lines = [ln.rstrip("\n").split("\t") for ln in open(sam) if ln[0] != "@"]
    assert len(lines) == len(reads)
    out = {"error-free reads": 0, "clean for a bubble": 0, "of them placed where they were cut": 0, "exceptions": 0, "reads with an edit": 0, "of them unmapped": 0}
    for f, r in zip(lines, reads):
        if r[6] is not None:
            out["reads with an edit"] += 1
            out["of them unmapped"] += f[1] == "4"
            continue
        out["error-free reads"] += 1
        if not any(indel_model.judge(r[0], g["bubbles"], w) for w in indel_model.ANCHORS):
            continue
        out["clean for a bubble"] += 1
        rec = g["names"][0] if r[1] == "c" else g["records"][r[2]][0]
        ok = f[1] != "4" and f[2].split()[0] == rec.split()[0] and int(f[3]) == r[3] + 1 and f[5] == f"{r[4]}M"
        out["of them placed where they were cut"] += ok
        out["exceptions"] += not ok
    return out


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="no reference binary under oracle/_ref")
def test_census_of_the_references_placements(tmp_path):
    got = census(REF_BIN, str(tmp_path))
    print(got)
    assert got["exceptions"] == 0 and got["clean for a bubble"] == got["of them placed where they were cut"] > 0, got
    assert got == CENSUS, got


# the reference's `index` + `align -n 3 -o 1` + `aln2sam` on the generated reads (tools/indel_generated_reference.py prints it)
CENSUS = {"error-free reads": 2756, "clean for a bubble": 1278, "of them placed where they were cut": 1278, "exceptions": 0, "reads with an edit": 248, "of them unmapped": 0}
