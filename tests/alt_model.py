"""A read's other placements (`bwbble map -X N`: the tags X0 / X1 / XA) restated in Python for tests/test_alt_host.py and
tests/test_gpu_alt.py, from hits in the form oracle_lib.parse_aln gives - a golden .aln of the reference or the oracle's bytes.

  placements   the rows e[0].L .. e[0].U, then e[1].L .. e[1].U, ... of a read's hits in discovery order; placement 0 is the primary
  T            their number: unsigned 64-bit, saturating; a hit with U < L saturates it
  items        with 2 <= T <= N + 1 the placements 1 .. T - 1, otherwise none (BWA's rule: too many placements, no list)

Every item is what eval_aln / print_aln2sam (align.c:786-801, :588-609) make of the primary, applied to the item's own hit and row.
Positions never come from the library under test: on the rep index they come from rep_sa.npy (the REFERENCE's SA() for every row), on
any other index from the oracle's invPsi walk (map_model.sa_walk)."""
import os

import numpy as np

import bwbble_amd as bw
import map_model

SAT = 2**64 - 1


def placements(ents):
    """T of a read's hit list"""
    T = 0
    for e in ents:
        if e["U"] < e["L"]:
            return SAT
        T = min(SAT, T + e["U"] - e["L"] + 1)
    return T


def n_items(ents, max_alt):
    T = placements(ents)
    return T - 1 if 2 <= T <= max_alt + 1 else 0


def item_rows(ents, max_alt):
    """[(hit, row)] of a read's items, in order"""
    c, out, k = n_items(ents, max_alt), [], 0
    for h, e in enumerate(ents if c else []):
        for row in range(e["L"], e["U"] + 1):
            k += 1
            if k > 1:
                out.append((h, row))
    assert len(out) == c
    return out


class FullSA:
    """sa(row) -> (SA[row], invPsi steps of the walk from row to the next row divisible by 32) from the suffix array of every row alone:
    the walk's k-th row is the row of suffix SA[row] - k (bwt.c:311-329; the step through the sentinel row takes suffix 0 to length - 1)"""

    def __init__(self, sa):
        self.sa = np.asarray(sa, dtype=np.int64)
        self.length = len(self.sa)
        self.isa = np.empty(self.length, dtype=np.int64)
        self.isa[self.sa] = np.arange(self.length)
        assert (np.sort(self.sa) == np.arange(self.length)).all()

    def __call__(self, row):
        p = int(self.sa[row])
        j = 0
        while int(self.isa[(p - j) % self.length]) % 32:
            j += 1
        return p, j


class OracleSA:
    """the same from the oracle's invPsi and the index's sampled SA (idx loaded WITH its SA)"""

    def __init__(self, orc, idx):
        self.orc, self.idx, self.length, self.memo = orc, idx, int(idx.contents.length), {}

    def __call__(self, row):
        if row not in self.memo:
            self.memo[row] = map_model.sa_walk(self.orc, self.idx, row)
        return self.memo[row]


def rep_sa(golden):
    return FullSA(np.load(os.path.join(golden, "rep_sa.npy")))


def expected_alts(reads, max_alt, sa):
    """-> (alt_off uint64[n + 1], items as bw.ALT_DTYPE, invPsi steps); sa: FullSA or OracleSA of the index the hits are on"""
    length = sa.length
    cnt = [n_items(ents, max_alt) for ents in reads]
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(cnt, dtype=np.uint64) if cnt else []
    alts = np.zeros(int(off[-1]), dtype=bw.ALT_DTYPE)
    steps, q = 0, 0
    for ents, c in zip(reads, cnt):
        if not c:
            continue
        for h, row in item_rows(ents, max_alt):
            e = ents[h]
            ref_len = e["aln_length"] - sum(s >> 2 for s in e["states"] if (s & 3) == 1)  # get_aln_length, align.c:748-757
            runs = map_model.gap_runs(e["states"])
            rp, j = sa(row)
            steps += j
            rec = alts[q]
            if rp > (length - 1) // 2:  # align.c:790-795 (the position is a bwtint_t there: a negative one wraps)
                rec["flags"], rec["pos"] = bw.PLACE_MAPPED, ((length - 1) - rp - 1 - ref_len + 1) % 2**64
            else:
                rec["flags"], rec["pos"] = bw.PLACE_MAPPED | bw.PLACE_REVERSE, rp
            rec["hit"], rec["num_mm"], rec["num_gapo"], rec["num_gape"] = h, e["mm"], e["gapo"], e["gape"]
            rec["aln_length"], rec["gap_run"] = e["aln_length"], runs
            q += 1
    assert q == len(alts)
    return off, alts, steps


class Ann(list):
    """[(name, start_index, end_index)] of a .ann file (both ends inclusive, the way print_aln2sam compares, align.c:567); find(pos): the
    first record that contains pos, like the reference's linear scan (align.c:796-801) - by bisection when the records ascend, as
    fasta2ref writes them (a GRCh37-scale multi-genome has 1.3 M of them)"""

    def find(self, pos):
        if not hasattr(self, "_starts"):
            self._starts = [s for _, s, _ in self]
            self._sorted = all(a[2] < b[1] for a, b in zip(self, self[1:]))
        if self._sorted:
            import bisect
            k = bisect.bisect_right(self._starts, pos) - 1
            return self[k] if k >= 0 and self[k][1] <= pos <= self[k][2] else None
        return next((rec for rec in self if rec[1] <= pos <= rec[2]), None)


def read_ann(path):
    out = Ann()
    for ln in open(path).read().split("\n")[1:]:
        f = ln.split("\t")
        if len(f) == 3:
            out.append((f[0], int(f[1]), int(f[2])))
    return out


def cigar(aln_length, gap_run, reverse):
    """print_aln2sam's CIGAR (align.c:588-609) of a path given as bwb_place.gap_run: the path walked from its end to its start, after it
    was reversed for the reverse strand"""
    path = [0] * aln_length
    for run in gap_run:
        run = int(run)
        if run != 0xFFFF:
            start, ln = run & 0xFF, (run >> 8) & 0x7F
            for i in range(start, min(start + ln, aln_length)):
                path[i] = 2 if run >> 15 else 1
    if reverse:
        path.reverse()
    out, i = [], aln_length - 1
    while i >= 0:
        j = i
        while j >= 0 and path[j] == path[i]:
            j -= 1
        out.append(f"{i - j}{'MID'[path[i]]}")
        i = j
    return "".join(out)


def tags(place, items, ann):
    """the text a mapped read's SAM line gains after the quality column; items: the read's ALT_DTYPE records (may be empty)"""
    t = f"\tX0:i:{int(place['top1'])}\tX1:i:{int(place['top2'])}"
    if len(items):
        t += "\tXA:Z:"
    for a in items:
        pos = int(a["pos"])
        rec = ann.find(pos)
        if rec is None:
            continue  # in no annotation record: left out (the primary dies there; an alternative must not)
        rev = bool(a["flags"] & bw.PLACE_REVERSE)
        nm = int(a["num_mm"]) + int(a["num_gapo"]) + int(a["num_gape"])
        t += f"{rec[0]},{'-' if rev else '+'}{pos - rec[1] + 1},{cigar(int(a['aln_length']), a['gap_run'], rev)},{nm};"
    return t


def expected_sam(base_text, places, alt_off, alts, ann):
    """base_text: the SAM text without -X (columns 1-11 of every read, header lines) -> the text with -X"""
    out, r = [], 0
    for ln in base_text.split("\n")[:-1]:
        if ln.startswith("@"):
            out.append(ln)
            continue
        if places[r]["flags"] & bw.PLACE_MAPPED:
            assert ln.split("\t")[1] != "4"
            ln += tags(places[r], alts[int(alt_off[r]):int(alt_off[r + 1])], ann)
        else:
            assert ln.split("\t")[1] == "4" and alt_off[r] == alt_off[r + 1]
        out.append(ln)
        r += 1
    assert r == len(places) and base_text.endswith("\n")
    return "\n".join(out) + "\n"


def alts_file_bytes(alt_off, alts):
    """the sixth argument of `places2sam`: u64 alt_off[n + 1], then the records"""
    return np.asarray(alt_off, dtype="<u8").tobytes() + np.asarray(alts, dtype=bw.ALT_DTYPE).tobytes()


def first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} items, {len(want)} expected"
    for q in range(len(got)):
        for f in bw.ALT_DTYPE.names:
            if not np.array_equal(got[q][f], want[q][f]):
                return f"item {q} field {f}: got {got[q][f]} want {want[q][f]}"
    return None
