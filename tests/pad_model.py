"""What the reference's sam_pad (mg-ref/sam_pad.cpp:27-94) makes of a SAM file and a bubble table, restated in Python for the tests of
`bwbble sampad` / `map -B` / `aln2sam -B` (tests/test_pad_host.py, tests/test_gpu_pad.py): padded SAM text from SAM text, and locus
records (bwbble_amd.LOCUS_DTYPE) from placement records + .ann + bubble.data.  Pinned to the reference's own output on the golden files
(tests/golden/pad_*.pad.sam*) on the CPU, then the judge of the GPU's records.  Never fed anything the library computed, except where a
test says so."""
import gzip
import os
import re

import numpy as np

import bwbble_amd as bw

MASK = (1 << 64) - 1


def wrap64(x):
    """what a C long long holds (two's complement; the reference's sums have no other defined meaning)"""
    x &= MASK
    return x - (1 << 64) if x >= (1 << 63) else x


def atoll(text):
    """C's atoll on a byte string: leading white space, an optional sign, decimal digits; 0 without digits"""
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?[0-9]+)", text)
    return wrap64(int(m.group(1))) if m else 0


def load_bubbles(path):
    """bubble.data -> [(ann bytes, A, B_minus_A, C, D_minus_C, ref_len, alt_len)], the k-th pair of lines is bubble k"""
    lines = read_bytes(path).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 2 == 0, "half a pair"
    out = []
    for ann, nums in zip(lines[0::2], lines[1::2]):
        v = [int(x) for x in nums.split()[:6]]
        assert len(v) == 6
        out.append((ann,) + tuple(v))
    return out


def which_bubble(rname):
    """sam_pad.cpp:67-72: None unless RNAME starts with `bubble`, else atoll of its first word after the word's first six characters"""
    if not rname.startswith(b"bubble"):
        return None
    return atoll(rname.split()[0][6:])


def locus_of(bubble, locus):
    """sam_pad.cpp:75-87 -> (kind, lo, hi)"""
    _, A, B, C, D, ref_len, alt_len = bubble
    right = wrap64(B + alt_len + 1)
    if 1 <= locus <= B:
        v = wrap64(A + locus - 1)
        return bw.LOCUS_POINT, v, v
    if right <= locus <= wrap64(right + D):
        v = wrap64(locus + C - right)
        return bw.LOCUS_POINT, v, v
    return bw.LOCUS_RANGE, wrap64(A + B), wrap64(A + B + ref_len - 1)


def tags(bubble, locus):
    kind, lo, hi = locus_of(bubble, locus)
    return b"\tbC:Z:" + bubble[0] + b"\tbP:Z:" + (b"%d" % lo if kind == bw.LOCUS_POINT else b"%d-%d" % (lo, hi))


def pad_sam(sam, bubbles):
    """process_sam (sam_pad.cpp:47-94): SAM bytes -> padded SAM bytes; every line ends in a newline, also a last one that had none"""
    lines = sam.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out = []
    for ln in lines:
        if ln[:1] != b"@":
            f = ln.split(b"\t")
            assert len(f) >= 4, "fewer than four fields: undefined in the reference"
            w = which_bubble(f[2])
            if w is not None:
                assert 0 <= w < len(bubbles), "a bubble outside the table: undefined in the reference"
                ln = ln + tags(bubbles[w], atoll(f[3]))
        out.append(ln + b"\n")
    return b"".join(out)


def bubble_of(names, bubbles):
    """which_bubble of every .ann record name, -1: not a bubble record"""
    out = np.full(len(names), -1, dtype=np.int32)
    for i, name in enumerate(names):
        w = which_bubble(name.encode() if isinstance(name, str) else name)
        if w is not None:
            assert 0 <= w < len(bubbles)
            out[i] = w
    return out


def bubble_records(bubbles):
    rec = np.zeros(len(bubbles), dtype=bw.BUBBLE_DTYPE)
    for k, b in enumerate(bubbles):
        rec[k] = b[1:]
    return rec


def expected_loci(places, start, end, bub_of, bubbles):
    """placement records + the .ann records' first / last positions + their bubble numbers + the bubble table -> LOCUS_DTYPE records: the
    record that contains the position (none for an unmapped read or a position in no record), the position SAM prints, and on a bubble
    record what sam_pad makes of that printed position"""
    start = np.asarray(start, dtype=np.uint64)
    end = np.asarray(end, dtype=np.uint64)
    out = np.zeros(len(places), dtype=bw.LOCUS_DTYPE)
    out["seqid"], out["bubble"] = -1, -1
    pos = places["pos"].astype(np.uint64)
    i = np.searchsorted(start, pos, side="right").astype(np.int64) - 1
    ok = ((places["flags"] & bw.PLACE_MAPPED) != 0) & (i >= 0)
    ic = np.maximum(i, 0)
    ok &= pos <= end[ic]
    out["seqid"][ok] = ic[ok]
    out["pos1"][ok] = (pos[ok] - start[ic[ok]] + np.uint64(1)).astype(np.uint32).view(np.int32)
    bub = np.where(ok, np.asarray(bub_of, dtype=np.int32)[ic], -1)
    out["bubble"] = bub
    for r in np.flatnonzero(bub >= 0):
        out["kind"][r], out["ref_lo"][r], out["ref_hi"][r] = locus_of(bubbles[int(bub[r])], int(out["pos1"][r]))
    return out


def first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} records, {len(want)} expected"
    for r in np.flatnonzero(got != want)[:1]:
        return f"read {r}: got {got[r]} want {want[r]}"
    return None


def read_bytes(path):
    return gzip.open(path, "rb").read() if str(path).endswith(".gz") else open(path, "rb").read()


PAD_TEXT = ("pad_bub.fq", "pad_bub_n3.aln", "pad_bub_n3.sam", "pad_bub_n3.pad.sam")


def unpack(dst, here=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")):
    """writes the gzipped files of the pad_bub fixture out into dst (the host tools read plain files) -> dst"""
    for name in PAD_TEXT:
        with open(os.path.join(str(dst), name), "wb") as f:
            f.write(read_bytes(os.path.join(here, name + ".gz")))
    return str(dst)


def classify(pad_sam_bytes, bubbles):
    """the fixture's census: {(case, strand): reads} over the bubble reads with case in left / right / range and strand in fwd / rev, plus
    ("plain", None) for mapped reads off the bubbles and ("unmapped", None)"""
    census = {}
    for ln in pad_sam_bytes.split(b"\n"):
        if not ln or ln[:1] == b"@":
            continue
        f = ln.split(b"\t")
        flag = int(f[1])
        w = which_bubble(f[2])
        if flag & 4:
            key = ("unmapped", None)
        elif w is None:
            key = ("plain", None)
        else:
            _, A, B, C, D, ref_len, alt_len = bubbles[w]
            locus = atoll(f[3])
            case = "left" if 1 <= locus <= B else ("right" if B + alt_len + 1 <= locus <= B + alt_len + D + 1 else "range")
            key = (case, "rev" if flag & 16 else "fwd")
        census[key] = census.get(key, 0) + 1
    return census
