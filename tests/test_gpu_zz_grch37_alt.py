"""`bwbble map -X` at GRCh37 INDEX SIZE (6.85 G BWT rows: 64-bit rows and SA values in k_place_alt, 1.3 M annotation records in the
formatter's lookup), on the index tests/test_gpu_zz_grch37.py builds (the file name sorts after it).  The tags are judged by the model
(tests/alt_model.py) fed with this build's .aln - whose bytes that file compares with the reference at this size - and with text
positions from Context.locate: kernel k_locate, independent of k_place_alt and pinned by the parity tests."""
import os
import subprocess
import time

import numpy as np
import pytest

import alt_model
import bwbble_amd as bw
import map_model
import oracle_lib
from test_gpu_zz_grch37 import grch37, sam_body  # noqa: F401  (the module's fixture: the index is built once per box)

pytestmark = pytest.mark.gpu


class LocateSA:
    """sa(row) for the model: the text positions of all rows asked for up front, by Context.locate"""

    def __init__(self, ctx, length, rows):
        rows = sorted(set(rows))
        pos = ctx.locate(np.array(rows, dtype=np.uint64)) if rows else []
        self.length, self.pos = length, {r: int(p) for r, p in zip(rows, pos)}

    def __call__(self, row):
        return self.pos[row], 0


def test_map_x5_matches_the_model_at_grch37_size(grch37, tmp_path):
    """map -n 3 -X 5 over 4 000 C3 reads: columns 1-11 are map's without -X; the tags are the model's from `align -n 3`'s hits and
    k_locate's positions; reads at the bubbles list their other placement"""
    fa = grch37
    n_reads = 4_000
    fq = str(tmp_path / "alt.fq")
    subprocess.run([bw.SYNTH_BIN, "reads", fa, fq, str(n_reads), "100", "8181", "1.0", "0.1", "0.0"], check=True)
    plain, tagged, aln = (str(tmp_path / x) for x in ("plain.sam", "x5.sam", "reads.aln"))
    t0 = time.time()
    for args in (["map", "-n", "3", fa, fq, plain], ["map", "-n", "3", "-X", "5", fa, fq, tagged], ["align", "-n", "3", fa, fq, aln]):
        r = subprocess.run([bw.HOST_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-3000:]
    print(f"[grch37] map, map -X 5 and align of {n_reads} reads: {time.time() - t0:.1f} s")
    got, base = sam_body(tagged), sam_body(plain)
    assert len(got) == len(base) == n_reads
    assert [b"\t".join(ln.split(b"\t")[:11]) for ln in got] == base
    hits = oracle_lib.parse_aln(open(aln, "rb").read())
    assert len(hits) == n_reads
    b = bw.BwtFile(fa + ".bwt", load_sa=True)
    ctx = bw.Context(b)
    try:
        ctx.set_sa(b.SA)
        sa = LocateSA(ctx, b.length, [row for e in hits for _, row in alt_model.item_rows(e, 5)])
        off, alts, _ = alt_model.expected_alts(hits, 5, sa)
        # the records themselves, in process: the library's own hit log of these reads
        seqs, lens = bw.load_fastq_codes(fq)
        ctx.align(bw.params(["-n", "3"]), seqs, lens)
        places, goff, galts = ctx.place_alt(6, 5)
        assert np.array_equal(goff, off) and alt_model.first_difference(galts, alts) is None, alt_model.first_difference(galts, alts)
        assert galts.tobytes() == alts.tobytes() and places.tobytes() == ctx.place(6).tobytes()
    finally:
        ctx.close()
    ann = alt_model.read_ann(fa + ".ann")
    want = alt_model.expected_sam(open(plain).read(), places, off, alts, ann)
    assert open(tagged).read() == want
    listed = [ln for ln in got if b"\tXA:Z:" in ln]
    assert len(alts) >= 1 and len(listed) >= 1
    if b.length > 2**32:  # 64-bit rows among the items' (a smaller index, BWB_TEST_GRCH37_FWD, has none)
        rows = np.array([row for e in hits for _, row in alt_model.item_rows(e, 5)], dtype=np.uint64)
        assert (rows >= 2**32).any()
    print(f"[grch37] -X 5: {len(alts)} items on {len(listed)} of {n_reads} reads")
