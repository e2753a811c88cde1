"""`bwbble map` without a GPU: the placement record's layout, the SAM formatter fed with placement records computed in Python from the
reference's golden .aln files (developer command `places2sam`), the repeat-rich fixtures, the streaming reader's name / quality offsets
and the command line's error paths."""
import os
import shutil
import subprocess

import pytest

import bwbble_amd as bw
import map_model
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (index, reads, golden .aln, golden .sam, aln2sam's -n)
CASES = {
    "toy_n3": ("toy.fa", "toy.fq", "toy_n3.aln", "toy_n3.sam", 6),
    "ragged_n4gap": ("toy.fa", "ragged.fq", "ragged_n4gap.aln", "ragged_n4gap.sam", 6),
    "wgsim100_n2": ("toy.fa", "wgsim100.fq", "wgsim100_n2.aln", "wgsim100_n2.sam", 6),
    "sim_chr21_N100_n2": ("toy.fa", "sim_chr21_N100.fastq", "sim_chr21_N100_n2.aln", "sim_chr21_N100_n2.sam", 6),
    "rep_n3": ("rep.fa", "rep.fq", "rep_n3.aln", "rep_n3.sam", 6),
    "rep_n3_q3": ("rep.fa", "rep.fq", "rep_n3.aln", "rep_n3_q3.sam", 3),
    # hit lists nobody searched for, judged by the reference's aln2sam (tests/golden/make_golden_map.py): the model's sums wrap like its ints
    "synth_hits_n6": ("rep.fa", "synth_hits.fq", "synth_hits.aln", "synth_hits_n6.sam", 6),
    "synth_hits_n3": ("rep.fa", "synth_hits.fq", "synth_hits.aln", "synth_hits_n3.sam", 3),
}


def test_place_record_layout_matches_the_header(built, tmp_path):
    """bwb_place as the C compiler sees it == PLACE_DTYPE: size and every field's offset"""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bwbble_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bwb_place));']
    for f in bw.PLACE_DTYPE.names:
        lines.append(f'printf("{f} %zu\\n", offsetof(bwb_place, {f}));')
    lines += ['printf("flag_mapped %d\\n", BWB_PLACE_MAPPED);', 'printf("flag_reverse %d\\n", BWB_PLACE_REVERSE);', 'return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["size"]) == bw.PLACE_DTYPE.itemsize == 48
    for f in bw.PLACE_DTYPE.names:
        assert int(got[f]) == bw.PLACE_DTYPE.fields[f][1], f
    assert (int(got["flag_mapped"]), int(got["flag_reverse"])) == (bw.PLACE_MAPPED, bw.PLACE_REVERSE)
    # every byte of the record belongs to a field
    assert sum(bw.PLACE_DTYPE.fields[f][0].itemsize for f in bw.PLACE_DTYPE.names) == 48


@pytest.mark.parametrize("name", list(CASES))
def test_formatter_writes_the_reference_sam_from_placement_records(built, golden, oracle, tmp_path, name):
    text = golden
    if name.startswith("synth_hits"):  # (its text files are committed gzipped)
        from golden.make_golden_map import unpack_synth
        text = unpack_synth(tmp_path)
    """placement records computed HERE, in Python, from the reference's .aln and the oracle's SA -> `places2sam` (sam_format_reads, the
    formatter of `map`) -> the reference's .sam, byte for byte"""
    fa, fq, aln, sam, max_mm = CASES[name]
    idx = oracle.load_index(os.path.join(golden, fa + ".bwt"), load_sa=True)
    reads = oracle_lib.parse_aln(open(os.path.join(golden, aln), "rb").read())
    places, _ = map_model.expected_places(oracle, idx, reads, max_mm)
    pf, out = tmp_path / "places.bin", tmp_path / "out.sam"
    places.tofile(pf)
    subprocess.run([bw.HOST_BIN, "places2sam", os.path.join(golden, fa), os.path.join(text, fq), str(pf), str(out)], check=True, stdout=subprocess.DEVNULL)
    assert open(out, "rb").read() == open(os.path.join(text, sam), "rb").read()


def test_repeat_fixture_reaches_every_mapq_outcome(golden):
    """the committed rep_* files: MAPQ 0 on a mapped read, 23, a value strictly between, 37 and - with `aln2sam -n 3` - 25; both strands; a
    first hit whose interval is wider than one row; reads with more than one hit (the toy fixtures have none of these)"""
    from golden.make_golden_map import sam_records
    d, q3 = sam_records(os.path.join(golden, "rep_n3.sam")), sam_records(os.path.join(golden, "rep_n3_q3.sam"))
    assert len(d) == len(q3) == 104
    mq = [(int(r[1]), int(r[4])) for r in d]
    assert any(f != 4 and q == 0 for f, q in mq)
    assert any(q == 23 for _, q in mq)
    assert any(0 < q < 23 for _, q in mq)
    assert any(q == 37 for _, q in mq)
    assert any(int(r[4]) == 25 for r in q3) and not any(q == 25 for _, q in mq)
    assert {f for f, _ in mq} == {0, 16, 4}
    reads = oracle_lib.parse_aln(open(os.path.join(golden, "rep_n3.aln"), "rb").read())
    assert len(reads) == 104
    assert any(e and e[0]["U"] > e[0]["L"] for e in reads)
    assert sum(1 for e in reads if len(e) > 1) >= 10
    assert any(sum(1 for x in e if x["score"] > e[0]["score"]) >= 2 for e in reads)  # top2 summed over several entries


def test_synthetic_hits_fixture_holds_every_case_it_exists_for(golden, oracle):
    """the committed synth_hits files: read lengths around 64 / 128 / 192, 0-8 gap runs across the words of k_place's insertion map in both
    orientations, sums at the clamp and wrapped to 1, 0 and below, later hits below the first, 9 and 17 hits, first rows that are special
    for the walk - every assertion of make_golden_map.check_synth, with the MAPQ values taken from the reference's SAM"""
    from golden.make_golden_map import check_synth
    idx = oracle.load_index(os.path.join(golden, "rep.fa.bwt"), load_sa=True)
    check_synth(oracle, idx, golden)


def test_model_sums_wrap_like_the_references_ints():
    assert [map_model.wrap32(v) for v in (0, 1, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**32 + 1, 3 * 2**31)] == [0, 1, 2**31 - 1, -2**31, -1, 0, 1, -2**31]


@pytest.mark.parametrize("order", ["natural", "reverse", "shuffled"])
def test_hit_records_rebuilt_from_the_aln_file_serialise_to_its_bytes(golden, order):
    """map_model.aln_records (file order -> the bwb_aln records kl_search emits, align-time order) is the inverse of the serialiser: aln_bytes
    of the rebuilt records == synth_hits.aln byte for byte, whatever the order of the runs inside gap_run[]; and the rep fixture's"""
    import random
    for name in ("synth_hits.aln", "rep_n3.aln", "ragged_n4gap.aln"):
        data = open(os.path.join(golden, name), "rb").read()
        permute = {"natural": None, "reverse": "reverse", "shuffled": random.Random(5)}[order]
        off, alns = map_model.aln_records(oracle_lib.parse_aln(data), permute)
        assert bw.aln_bytes(off, alns) == data, name
        if name == "synth_hits.aln" and order != "natural":  # the order did change
            nat = map_model.aln_records(oracle_lib.parse_aln(data))[1]
            assert (alns["gap_run"] != nat["gap_run"]).any(axis=1).sum() > 50


def test_mapq_table_fits_a_byte():
    """mapq's table entries: (int)(4.343 * log(n) + 0.5) for n = 1..255 stays within 0..24, so it fits the byte table k_place reads"""
    import math
    assert all(0 <= int(4.343 * math.log(n) + 0.5) <= 24 for n in range(1, 256))
    assert map_model.mapq(1, 1, 0, 6) == 23 and map_model.mapq(1, 2, 0, 6) == 20 and map_model.mapq(1, 5, 0, 6) == 16 and map_model.mapq(1, 255, 0, 6) == 0


def _nasty_fastq(path, n=300, seed=19):
    """'@' and '+' inside names and at the start of quality lines, '+name' separators, blank lines, ragged lengths, no final newline"""
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.choice([1, 2, 17, 36, 100, 151])
        seq = "".join(rng.choice("ACGTNacgt") for _ in range(ln))
        qual = rng.choice("@+I5") + "".join(rng.choice("@+IJ5#") for _ in range(ln - 1))
        name = f"r{i}" + rng.choice(["", " @x", " +y", "/1 len=+@", "@" + "n" * 300])
        sep = "+" + (name if rng.random() < 0.3 else "")
        out.append(f"@{name}\n{seq}\n{sep}\n{qual}\n" + ("\n" if rng.random() < 0.1 else ""))
    text = "".join(out)
    open(path, "w").write(text[:-1] if text.endswith("\n") else text)


@pytest.mark.parametrize("region,threads,chunk", [("64", "3", 7), ("1000", "16", 1), ("100000000", "8", 13)])
def test_streaming_reader_finds_names_and_qualities(built, golden, tmp_path, monkeypatch, region, threads, chunk):
    """fq_open_text (the stream of `map`): every chunk's name offsets, name lengths and quality offsets point at what the whole-file
    reader (fastq2reads, which aln2sam uses) finds - on the golden files and on a FASTQ built to mislead"""
    nasty = tmp_path / "nasty.fq"
    _nasty_fastq(str(nasty))
    monkeypatch.setenv("BWB_FQ_REGION", region)
    monkeypatch.setenv("BWB_FQ_THREADS", threads)
    for fq in [os.path.join(golden, f) for f in ("wgsim100.fq", "ragged.fq", "sim_chr21_N100.fastq", "rep.fq")] + [str(nasty)]:
        whole, parts = tmp_path / "whole.tsv", tmp_path / "parts.tsv"
        subprocess.run([bw.HOST_BIN, "dumpreads", fq, str(whole)], check=True, stdout=subprocess.DEVNULL)
        subprocess.run([bw.HOST_BIN, "dumpreads", fq, str(parts), str(chunk), "text"], check=True, stdout=subprocess.DEVNULL)
        assert open(parts, "rb").read() == open(whole, "rb").read(), fq


def test_map_usage(built):
    r = subprocess.run([bw.HOST_BIN, "map", "-n", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 1 and "Usage: bwbble map" in r.stdout and "-Q" in r.stdout
    r = subprocess.run([bw.HOST_BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert "map " in r.stdout


def test_map_without_gpu_fails_loudly_and_leaves_no_file(built, golden, tmp_path):
    if bw.device_count() > 0:
        pytest.skip("a GPU is present")
    for ext in ("", ".bwt", ".ann"):
        shutil.copy(os.path.join(golden, "rep.fa" + ext), tmp_path / ("rep.fa" + ext))
    out = tmp_path / "x.sam"
    r = subprocess.run([bw.HOST_BIN, "map", "-n", "3", "-Q", "3", str(tmp_path / "rep.fa"), os.path.join(golden, "rep.fq"), str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "no HIP device" in r.stdout
    assert not out.exists()
