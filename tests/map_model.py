"""What eval_aln + mapq (mg-aligner/align.c:738-812) make of a read's hits, restated in Python for the tests of `bwbble map`
(tests/test_map_host.py, tests/test_gpu_map.py): placement records (bwbble_amd.PLACE_DTYPE) from hits in the form oracle_lib.parse_aln
gives - so from a golden .aln of the reference or from the oracle's bytes, never from the library under test - and the oracle's
invPsi / SA (oracle/bwb_oracle.c)."""
import ctypes as C
import math
import random

import numpy as np

import bwbble_amd as bw


def wrap32(x):
    """what a C int holds after `+=` of 64-bit interval widths (align.c:773,776: read_t.aln_top1_count / aln_top2_count are ints)"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def mapq(top1, top2, num_mm, max_mm):  # align.c:738-746 (top2 < 0 with top1 == 1 or < 0: log() of a negative number there - undefined, an error here)
    if top1 == 0:
        return 23
    if top1 > 1:
        return 0
    if num_mm == max_mm:
        return 25
    if top2 == 0:
        return 37
    n = 255 if top2 >= 255 else top2
    q = int(4.343 * math.log(n) + 0.5)
    return 0 if 23 < q else 23 - q


def gap_runs(states):
    """bwb_aln.gap_run encoding of a path given as the .aln file's (state | count << 2) pairs, in the file's order: that is the order in
    which the reference's loader fills aln_path (align.c:466-476), the orientation eval_aln and the CIGAR code work on"""
    runs, pos = [], 0
    for s in states:
        st, cnt = s & 3, s >> 2
        if st:
            runs.append((pos & 0xFF) | ((cnt & 0x7F) << 8) | (0x8000 if st == 2 else 0))
        pos += cnt
    assert len(runs) <= 8
    return runs + [0xFFFF] * (8 - len(runs))


def aln_records(reads, permute=None):
    """The inverse of gap_runs: hits in the form oracle_lib.parse_aln gives (paths in the .aln file's order) -> (aln_off, records of
    bwbble_amd.ALN_DTYPE) as kl_search would have emitted them.  The search writes the path in align-time order, which the file holds from
    its end to its start (align.c:363-373): a run (start, len) of the file's path is (aln_length - start - len, len) there.  permute: the
    order of the runs inside gap_run[] - None: ascending by align-time start; "reverse": descending; a random.Random: shuffled by it."""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(ents) for ents in reads])
    alns = np.zeros(int(off[-1]), dtype=bw.ALN_DTYPE)
    k = 0
    for ents in reads:
        for e in ents:
            alen = e["aln_length"]
            runs = []
            for run in gap_runs(e["states"]):
                if run != 0xFFFF:
                    start, ln = run & 0xFF, (run >> 8) & 0x7F
                    assert 0 <= alen - start - ln <= 0xFF
                    runs.append((alen - start - ln) | (run & 0xFF00))
            runs.sort(key=lambda v: v & 0xFF)
            if permute == "reverse":
                runs.reverse()
            elif isinstance(permute, random.Random):
                permute.shuffle(runs)
            else:
                assert permute is None
            rec = alns[k]
            rec["L"], rec["U"], rec["score"] = e["L"], e["U"], e["score"]
            rec["num_mm"], rec["num_gapo"], rec["num_gape"], rec["aln_length"] = e["mm"], e["gapo"], e["gape"], alen
            rec["gap_run"] = runs + [0xFFFF] * (8 - len(runs))
            k += 1
    return off, alns


def walk_rows(orc, idx, row):
    """the rows the invPsi walk from `row` visits, the start and the sampled row it ends on included (bwt.c:311-329)"""
    orc.lib.bwb_or_invPsi.restype = C.c_uint64
    orc.lib.bwb_or_invPsi.argtypes = [C.c_void_p, C.c_uint64]
    rows = [row]
    while rows[-1] % 32:
        rows.append(int(orc.lib.bwb_or_invPsi(idx, rows[-1])))
    return rows


def sa_walk(orc, idx, row):
    """(SA[row], steps): bwt.c:311-329 with the oracle's invPsi, until a row divisible by 32; the step through the sentinel row counts"""
    rows = walk_rows(orc, idx, row)
    j = len(rows) - 1
    return (int(idx.contents.SA[rows[-1] // 32]) + j) % int(idx.contents.length), j


def expected_places(orc, idx, reads, max_mm=6):
    """reads: per read a list of hits (dicts of oracle_lib.parse_aln); idx: an oracle index loaded WITH its SA -> (records, invPsi steps)"""
    length = int(idx.contents.length)
    out = np.zeros(len(reads), dtype=bw.PLACE_DTYPE)
    steps = 0
    for r, ents in enumerate(reads):
        if not ents:
            continue
        e0 = ents[0]
        top1 = wrap32(sum(e["U"] - e["L"] + 1 for e in ents if e["score"] <= e0["score"]))  # sums of C ints, align.c:773,776
        top2 = wrap32(sum(e["U"] - e["L"] + 1 for e in ents if e["score"] > e0["score"]))
        ref_len = e0["aln_length"] - sum(s >> 2 for s in e0["states"] if (s & 3) == 1)  # get_aln_length, align.c:748-757
        rp, j = sa_walk(orc, idx, e0["L"])
        steps += j
        if rp > (length - 1) // 2:  # align.c:790-795
            flags, pos = bw.PLACE_MAPPED, (length - 1) - rp - 1 - ref_len + 1
        else:
            flags, pos = bw.PLACE_MAPPED | bw.PLACE_REVERSE, rp
        rec = out[r]
        rec["pos"], rec["top1"], rec["top2"], rec["score"] = pos, top1, top2, e0["score"]
        rec["mapq"], rec["flags"] = mapq(top1, top2, e0["mm"], max_mm), flags
        rec["num_mm"], rec["num_gapo"], rec["num_gape"] = e0["mm"], e0["gapo"], e0["gape"]
        rec["aln_length"], rec["ref_len"] = e0["aln_length"], ref_len
        rec["gap_run"] = gap_runs(e0["states"])
    return out, steps


def first_difference(got, want):
    """a readable account of where two record arrays differ (for assertion messages)"""
    if len(got) != len(want):
        return f"{len(got)} records, {len(want)} expected"
    for r in range(len(got)):
        for f in bw.PLACE_DTYPE.names:
            if not np.array_equal(got[r][f], want[r][f]):
                return f"read {r} field {f}: got {got[r][f]} want {want[r][f]}"
    return None
