"""Ref / alt read support per indel bubble (`bwbble map -B table -I file`) restated in Python for tests/test_indel_host.py and
tests/test_gpu_indel.py.  Three things, none of them fed anything the library computed:

  the rule       eligible() / windows() / classify() / count(): include/bwbble_hip.h (bwb_hip_indel_begin) on printed positions and CIGAR texts,
                 base by base, every eligible bubble tried for every chromosome read (no sorted table, no bisection); table_bytes() is the writer
  a generator    lift_model.genome() unchanged, and reads(): error-free reads cut from every bubble record and from the chromosome around every
                 bubble's site, and reads with one inserted or one deleted base inside and just outside the window; the names say where they
                 were cut
  a judge        judge(): walks no CIGAR - from a read's name alone (record or chromosome, offset, length, edit) it decides by interval
                 arithmetic which windows the read contains
"""
import random
import re

import numpy as np

import bwbble_amd as bw
import lift_model

REF, ALT, REF_GAPPED, ALT_GAPPED = 0, 1, 2, 3
HEADER = b"#bubble\tchrom\tpos\tref_len\talt_len\tref\talt\tref_gapped\talt_gapped\n"
ANCHORS = (1, 5, 30)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def eligible(bubble, w):
    _, A, Bm, C, Dm, _, alt = bubble
    return lift_model.refusal(bubble) is None and Bm >= w and Dm + 1 >= w and A + Bm - w >= 1


def windows(bubble, w):
    """((lo, hi) on the bubble's own record, (lo, hi) on its chromosome's record), 1-based"""
    _, A, Bm, C, Dm, _, alt = bubble
    return (Bm - w + 1, Bm + alt + w), (A + Bm - w, C + w - 1)


def classify(pos1, cigar, lo, hi):
    """0 not covering, 1 clean, 2 gapped: the printed CIGAR expanded to one entry per op position"""
    if lo < pos1 or hi >= pos1 + sum(n for n, op in lift_model.parse_cigar(cigar) if op in "MD"):
        return 0  # (the window leaves the positions the read consumes)
    consumed, inserts, x, step = {}, [], pos1, 0  # x -> (op, step); the steps at which an I lies
    for n, op in lift_model.parse_cigar(cigar):
        for _ in range(n):
            if op == "I":
                inserts.append(step)
            else:
                consumed[x] = (op, step)
                x += 1
            step += 1
    if consumed.get(lo, ("", 0))[0] != "M" or consumed.get(hi, ("", 0))[0] != "M":
        return 0
    clean = all(consumed[v][0] == "M" for v in range(lo, hi + 1)) and not any(consumed[lo][1] < s < consumed[hi][1] for s in inserts)
    return 1 if clean else 2


def read_length(cigar):
    return sum(n for n, op in lift_model.parse_cigar(cigar) if op in "MI")


def count(placements, bubbles, chrom_of, w, min_mapq=0):
    """placements: [(seqid | -1, bubble | -1, pos1, CIGAR text, MAPQ, read length | None)] of mapped primaries (None: an unmapped read)
    -> ((n_bub, 4) uint32 counters, reads counted, adds)"""
    counts = np.zeros((len(bubbles), 4), dtype=np.uint32)
    ok = [k for k, b in enumerate(bubbles) if eligible(b, w)]
    reads = adds = 0
    for p in placements:
        if p is None:
            continue
        seqid, b, pos1, cigar, mapq, length = p
        if seqid < 0 or mapq < min_mapq or (length is not None and read_length(cigar) != length):
            continue
        reads += 1
        if b >= 0:
            todo = [(b, windows(bubbles[b], w)[0], ALT)] if b in ok else []
        else:
            todo = [(k, windows(bubbles[k], w)[1], REF) for k in ok if int(chrom_of[k]) == seqid]
        for k, (lo, hi), col in todo:
            cls = classify(pos1, cigar, lo, hi)
            if cls:
                counts[k][col + (2 if cls == 2 else 0)] += 1
                adds += 1
    return counts, reads, adds


def from_records(places, loci, mapq=None, lens=None):
    """PLACE_DTYPE + LOCUS_DTYPE records (pad_model.expected_loci) -> count()'s placements"""
    import alt_model
    out = []
    for r, (pl, lc) in enumerate(zip(places, loci)):
        if not pl["flags"] & bw.PLACE_MAPPED:
            out.append(None)
            continue
        cig = alt_model.cigar(int(pl["aln_length"]), pl["gap_run"], bool(pl["flags"] & bw.PLACE_REVERSE))
        out.append((int(lc["seqid"]), int(lc["bubble"]), int(lc["pos1"]), cig, int(pl["mapq"] if mapq is None else mapq[r]), None if lens is None else int(lens[r])))
    return out


def from_sam(text, names, bubble_of):
    """SAM bytes as `map` / `aln2sam` write them -> count()'s placements: RNAME, POS, CIGAR and MAPQ of every line, as it was placed - with -R
    a lifted line carries them in its bO tag"""
    first = {lift_model.first_word(n): i for i, n in enumerate(names)}
    out = []
    for ln in text.split(b"\n")[:-1]:
        if ln[:1] == b"@":
            continue
        f = ln.split(b"\t")
        if int(f[1]) & 4:
            out.append(None)
            continue
        rname, pos, cig = f[2].decode(), int(f[3]), f[5].decode()
        for tag in f[11:]:
            if tag.startswith(b"bO:Z:"):
                rname, pos, cig = tag[5:].decode().split(",")
                pos = int(pos)
        i = first[lift_model.first_word(rname)]
        out.append((i, int(bubble_of[i]), pos, cig, int(f[4]), len(f[9])))
    return out


def table_bytes(bubbles, counts):
    out = [HEADER]
    for k, (b, v) in enumerate(zip(bubbles, counts)):
        if any(int(x) for x in v):
            out.append(b"%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (k, lift_model.first_word(b[0]).encode(), b[1] + b[2], b[5], b[6], v[0], v[1], v[2], v[3]))
    return b"".join(out)


# ---- the generator ----------------------------------------------------------------------------------------------------------------------

def _copy(rnd, text):
    return "".join(rnd.choice(lift_model.IUPAC[c]) for c in text)


def reads(g, seed=9, anchors=ANCHORS, edit_anchor=5):
    """[(name, where, bubble, offset, length, strand, edit, SEQ on the forward strand, CIGAR)]: where "b" - cut from bubble k's record - or "c" -
    cut from the chromosome around bubble k's site; offset 0-based in that text.  Error-free reads of 100 and 60 bases at every offset at which
    the read's first base lies within 3 of a window's lo or its last within 3 of a window's hi (the windows of every anchor), and at every third
    offset otherwise; then reads with one inserted (I<a>) or one deleted (D<a>) base behind their first a bases, placed 3 before lo, 1 behind
    lo, 1 before hi and 3 behind hi of the window at edit_anchor"""
    rnd = random.Random(seed)
    out = []
    for k, bub in enumerate(g["bubbles"]):
        _, A, Bm, C, Dm, _, alt = bub
        for where, text, span in (("b", g["records"][k][1], (0, len(g["records"][k][1]))), ("c", g["chrom"], (max(0, A + Bm - 140), min(len(g["chrom"]), C + 140)))):
            wins = [windows(bub, w)[0 if where == "b" else 1] for w in anchors]
            for ln in (100, 60):
                for o in range(span[0], span[1] - ln + 1):
                    near = any(abs(o + 1 - lo) <= 3 or abs(o + ln - hi) <= 3 for lo, hi in wins)
                    if not (near or o % 3 == 0):
                        continue
                    strand = "+-"[(o + ln) & 1]
                    out.append((f"i{where}{k}_o{o}_l{ln}_{strand}", where, k, o, ln, strand, None, _copy(rnd, text[o:o + ln]), f"{ln}M"))
                lo, hi = windows(bub, edit_anchor)[0 if where == "b" else 1]
                for x, a in ((lo - 3, 12), (lo + 1, 12), (hi - 1, ln - 13), (hi + 3, ln - 13)):
                    for edit in "ID":
                        # D: text position x (1-based) is deleted; I: a base is inserted before text position x
                        o = x - 1 - a
                        last = o + ln + (1 if edit == "D" else -1)
                        if o < 0 or last > len(text) or x < 1:
                            continue
                        if edit == "I":
                            seq = _copy(rnd, text[o:o + a]) + rnd.choice("ACGT") + _copy(rnd, text[o + a:o + ln - 1])
                            cig = f"{a}M1I{ln - 1 - a}M"
                        else:
                            seq = _copy(rnd, text[o:o + a] + text[o + a + 1:o + ln + 1])
                            cig = f"{a}M1D{ln - a}M"
                        assert len(seq) == ln
                        out.append((f"i{where}{k}_o{o}_l{ln}_+_{edit}{a}", where, k, o, ln, "+", edit, seq, cig))
    return out


def fastq(read_list):
    """a read of the reverse strand is written reverse-complemented, so that it maps there"""
    return "".join(f"@{r[0]}\n{r[7][::-1].translate(lift_model.COMP) if r[5] == '-' else r[7]}\n+\n{'I' * r[4]}\n" for r in read_list)


def truth(g, read_list, mapq=37):
    """count()'s placements of the reads where they were cut: record 0 is the chromosome, record 1 + k bubble k's"""
    return [((0, -1) if r[1] == "c" else (1 + r[2], r[2])) + (r[3] + 1, r[8], mapq, r[4]) for r in read_list]


def truth_records(g, read_list, start):
    """the same as PLACE_DTYPE records on an .ann whose record i begins at text position start[i]"""
    return lift_model.place_records([(int(start[0 if r[1] == "c" else 1 + r[2]]) + r[3], r[5] == "-", r[8]) for r in read_list])


# ---- the judge --------------------------------------------------------------------------------------------------------------------------

NAME = re.compile(r"i([bc])(\d+)_o(\d+)_l(\d+)_([+-])(?:_([ID])(\d+))?$")


def judge(name, bubbles, w):
    """[(bubble, column)] the read adds to, from its name alone.  An error-free read occupies the text positions o + 1 .. o + l; it is clean for
    a window it contains and nothing otherwise.  A read with a deleted base occupies one position more and is gapped when the deleted position
    lies inside the window (not covering when it is lo or hi); one with an inserted base occupies one less and is gapped when the bases on
    either side of the insertion both lie inside the window"""
    where, k, o, ln, _, edit, a = NAME.match(name).groups()
    k, o, ln = int(k), int(o), int(ln)
    first, last = o + 1, o + ln + {None: 0, "D": 1, "I": -1}[edit]
    out = []
    for j, b in enumerate(bubbles):
        if not eligible(b, w) or (where == "b" and j != k):
            continue
        lo, hi = windows(b, w)[0 if where == "b" else 1]
        if not (first <= lo and hi <= last):
            continue
        gapped = False
        if edit == "D":
            x = o + int(a) + 1
            if x in (lo, hi):
                continue
            gapped = lo < x < hi
        elif edit == "I":
            gapped = lo <= o + int(a) and o + int(a) + 1 <= hi
        out.append((j, (ALT if where == "b" else REF) + (2 if gapped else 0)))
    return out


def judged_table(read_list, bubbles, w):
    counts = np.zeros((len(bubbles), 4), dtype=np.uint32)
    for r in read_list:
        for j, col in judge(r[0], bubbles, w):
            counts[j][col] += 1
    return counts
