"""A read's placements counted by locus (`bwbble map -X N -B table -J`) restated in Python for tests/test_join_host.py and
tests/test_gpu_join.py.  The rule (include/bwbble_hip.h, bwb_join):

  placement   the primary (PLACE_DTYPE) or one of the read's items (ALT_DTYPE, alt_model.expected_alts)
  locus       (c, s, lo, hi) of a mapped placement that lies in an .ann record: s the PLACE_REVERSE bit; on a non-bubble record i, c = i and
              lo = hi = the position SAM prints; on a record of bubble b, c = chrom_of[b] and lo .. hi = what pad_model.locus_of (pinned to
              the reference's sam_pad) makes of the printed position; hi' = max(hi, lo)
  joined      an item whose locus has the primary's c and s and lo_item <= hi'_primary and lo_primary <= hi'_item
  suboptimal  an item whose hit's score is greater than the first hit's (eval_aln, align.c:771-779)
  per read    joined = the joined items; top1' = top1 - (joined, not suboptimal); top2' = top2 - (joined, suboptimal), as C ints;
              mapq' = map_model.mapq(top1', top2', num_mm, max_mm) for a read WITH items, the record's own MAPQ otherwise; all zero unmapped

Fed the reference's hits (golden .aln files), the oracle's SA and the models that are pinned to the reference (map_model, alt_model,
pad_model) - never anything the library computed."""
import numpy as np

import bwbble_amd as bw
import map_model
import pad_model


def chrom_of(names, bubbles):
    """the .ann record of the chromosome every bubble lies on: the ONE record whose name's first word is the first word of the bubble's
    header line (bubbles as pad_model.load_bubbles gives them); it must not be a bubble record"""
    out = np.zeros(len(bubbles), dtype=np.int32)
    for b, bub in enumerate(bubbles):
        w = bub[0].split()[0] if bub[0].split() else b""
        hits = [i for i, n in enumerate(names) if ((n.encode() if isinstance(n, str) else n).split() or [b""])[0] == w]
        assert len(hits) == 1, (b, bub[0], hits)
        assert pad_model.which_bubble(names[hits[0]].encode() if isinstance(names[hits[0]], str) else names[hits[0]]) is None, (b, bub[0])
        out[b] = hits[0]
    return out


def loci4(pos, flags, start, end, bub_of, bubbles, chrom):
    """(has, c, s, lo, hi') of placements given by text position and flags"""
    as_places = np.zeros(len(pos), dtype=bw.PLACE_DTYPE)
    as_places["pos"], as_places["flags"] = pos, flags
    lc = pad_model.expected_loci(as_places, start, end, bub_of, bubbles)
    has = lc["seqid"] >= 0
    on_bubble = lc["bubble"] >= 0
    chrom = np.asarray(chrom, dtype=np.int64)
    c = np.where(on_bubble, chrom[np.maximum(lc["bubble"], 0)] if len(chrom) else 0, lc["seqid"]).astype(np.int64)
    lo = np.where(on_bubble, lc["ref_lo"], lc["pos1"].astype(np.int64))
    hi = np.where(on_bubble, lc["ref_hi"], lc["pos1"].astype(np.int64))
    return has, c, (np.asarray(flags) & bw.PLACE_REVERSE) != 0, lo, np.maximum(hi, lo)


def item_classes(places, alt_off, alts, start, end, bub_of, bubbles, chrom):
    """per item: joined to its read's primary or not"""
    cnt = np.diff(np.asarray(alt_off, dtype=np.uint64)).astype(np.int64)
    owner = np.repeat(np.arange(len(places)), cnt)
    hp, cp, sp, lop, hip = (a[owner] for a in loci4(places["pos"], places["flags"], start, end, bub_of, bubbles, chrom))
    hi_, ci, si, loi, hii = loci4(alts["pos"], alts["flags"], start, end, bub_of, bubbles, chrom)
    return owner, hp & hi_ & (cp == ci) & (sp == si) & (loi <= hip) & (lop <= hii)


def expected_joins(places, alt_off, alts, alt_sub, start, end, bub_of, bubbles, chrom, max_mm=6):
    """-> (JOIN_DTYPE records, joined items in all)"""
    n = len(places)
    owner, joined = item_classes(places, alt_off, alts, start, end, bub_of, bubbles, chrom)
    sub = np.asarray(alt_sub, dtype=np.uint8) != 0
    best = np.bincount(owner[joined & ~sub], minlength=n).astype(np.int64)
    subopt = np.bincount(owner[joined & sub], minlength=n).astype(np.int64)
    out = np.zeros(n, dtype=bw.JOIN_DTYPE)
    out["top1"] = ((places["top1"].astype(np.int64) - best) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # C ints
    out["top2"] = ((places["top2"].astype(np.int64) - subopt) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    out["mapq"] = places["mapq"]
    out["joined"] = best + subopt
    cnt = np.diff(np.asarray(alt_off, dtype=np.uint64)).astype(np.int64)
    for r in np.flatnonzero(cnt > 0):
        out["mapq"][r] = map_model.mapq(int(out["top1"][r]), int(out["top2"][r]), int(places["num_mm"][r]), max_mm)
    unmapped = (places["flags"] & bw.PLACE_MAPPED) == 0
    out[unmapped] = np.zeros(1, dtype=bw.JOIN_DTYPE)[0]
    return out, int((best + subopt)[~unmapped].sum())


def suboptimal(reads, alt_off, alts):
    """the suboptimal byte of every item from the reads' hits (oracle_lib.parse_aln): hit `hit`'s score against hit 0's"""
    sub = np.zeros(len(alts), dtype=np.uint8)
    for r, ents in enumerate(reads):
        for q in range(int(alt_off[r]), int(alt_off[r + 1])):
            sub[q] = ents[int(alts[q]["hit"])]["score"] > ents[0]["score"]
    return sub


def apply_to_sam(text, places, joins):
    """SAM bytes with the X and b tags -> the bytes `-J` writes: the MAPQ column from the join records, and bJ:i:<joined> last on the line of
    a read with joined items"""
    out, r = [], 0
    for ln in text.split(b"\n")[:-1]:
        if ln[:1] != b"@":
            if places[r]["flags"] & bw.PLACE_MAPPED:
                f = ln.split(b"\t")
                assert int(f[4]) == int(places[r]["mapq"])
                f[4] = b"%d" % int(joins[r]["mapq"])
                ln = b"\t".join(f) + (b"\tbJ:i:%d" % int(joins[r]["joined"]) if joins[r]["joined"] else b"")
            r += 1
        out.append(ln)
    assert r == len(places) and text.endswith(b"\n")
    return b"\n".join(out) + b"\n"


def alts_file_bytes(alt_off, alts, alt_sub):
    """the items file of `places2sam -J`: alt_model.alts_file_bytes, then one byte per item"""
    import alt_model
    return alt_model.alts_file_bytes(alt_off, alts) + np.asarray(alt_sub, dtype=np.uint8).tobytes()


def first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} records, {len(want)} expected"
    for r in np.flatnonzero(got != want)[:1]:
        return f"read {r}: got {got[r]} want {want[r]}"
    return None
