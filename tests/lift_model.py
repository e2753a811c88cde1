"""Placements on bubble records in chromosome coordinates (`bwbble map -B table -R`) restated in Python for tests/test_lift_host.py and
tests/test_gpu_lift.py.  Three things, none of them fed anything the library computed:

  the rule       lift(): include/bwbble_hip.h (bwb_lift) on a printed position and a CIGAR text, base by base; lift_sam() applies it to SAM text
  a generator    genome(): one chromosome of a few kb with IUPAC codes in the flanks, and bubble records built the way the reference's comb
                 builds them (124-base flanks, cut by the chromosome's ends) with their bubble.data and, for every record character, the
                 chromosome coordinate it copies (cmap, None inside the alternate allele); reads(): reads cut from the records
  a judge        judge(): POS and CIGAR re-derived from cmap alone - no A / Bm / C arithmetic -, and mismatches() against the chromosome
"""
import itertools
import random
import re

import numpy as np

import bwbble_amd as bw

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG",
         "N": "ACGT"}
COMP = str.maketrans("ACGTRYSWKMBDHVN", "TGCAYRSWMKVHDBN")
FLANK = 124


def parse_cigar(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDS])", text)]


def cigar_text(ops):
    return "".join(f"{n}{op}" for n, op in ops)


def _finish(steps):
    """the walk's steps [(kind, chromosome coordinate | None, length)] - one per base, and one for the positions a record skips - ->
    (POS, ops) or None: soft clips, dropped edge deletions, neighbours merged while the sum stays below 2^28"""
    ms = [i for i, (k, _, _) in enumerate(steps) if k == "M"]
    if not ms:
        return None
    head, body, tail = steps[:ms[0]], steps[ms[0]:ms[-1] + 1], steps[ms[-1] + 1:]
    ops = []
    clip = sum(n for k, _, n in head if k == "I")
    if clip:
        ops.append((clip, "S"))
    for k, _, n in body:
        if ops and ops[-1][1] == k and ops[-1][0] + n < 1 << 28:
            ops[-1] = (ops[-1][0] + n, k)
        else:
            ops.append((n, k))
    clip = sum(n for k, _, n in tail if k == "I")
    if clip:
        ops.append((clip, "S"))
    return body[0][1], ops


def refusal(bubble):
    """why -R refuses a bubble (pad_model.load_bubbles tuple), None: it does not"""
    _, A, Bm, C, Dm, _, alt = bubble
    gap = C - A - Bm
    if Bm < 0 or Dm < -1 or alt < 0 or gap < 0 or gap >= 1 << 28:
        return True
    return None


def lift(bubble, pos1, cigar):
    """the rule: bubble = (ann, A, Bm, C, Dm, ref_len, alt_len), pos1 the printed position on the bubble record, cigar the printed CIGAR text
    -> (POS, CIGAR text) on the chromosome, or None when the placement is not liftable"""
    _, A, Bm, C, Dm, _, alt = bubble
    reclen, right, gap = Bm + alt + Dm + 1, Bm + alt + 1, C - A - Bm
    ops = parse_cigar(cigar)
    span = sum(n for n, op in ops if op in "MD")
    if pos1 < 1 or pos1 + span - 1 > reclen:
        return None
    per_base, x = [], pos1
    for n, op in ops:
        for _ in range(n):
            if op == "I":
                per_base.append(("I", None, 1))
                continue
            if x == right and x > pos1 and gap > 0:
                per_base.append(("D", None, gap))
            in_allele = Bm < x < right
            where = None if in_allele else (A + x - 1 if x <= Bm else C + x - right)
            if op == "M":
                per_base.append(("I", None, 1) if in_allele else ("M", where, 1))
            elif not in_allele:
                per_base.append(("D", None, 1))
            x += 1
    got = _finish(per_base)
    return None if got is None or len(got[1]) > bw.LIFT_MAX_OPS else (got[0], cigar_text(got[1]))


def first_word(name):
    name = name.decode() if isinstance(name, bytes) else name
    return name.split()[0] if name.split() else ""


def bubble_number(rname):
    """the bubble of an RNAME / item name, None: not a bubble record (sam_pad's rule, pad_model.which_bubble)"""
    import pad_model
    return pad_model.which_bubble(rname if isinstance(rname, bytes) else rname.encode())


def lift_sam(text, bubbles, names, chrom):
    """SAM bytes as `map [-X N] -B table [-J]` writes them -> the bytes with -R: the lines on a bubble record lifted and tagged bO (last),
    the XA items on a bubble record lifted; names: the .ann names, chrom[b]: the chromosome's record of bubble b.  Also returns the number
    of placements lifted and of those on a bubble record that are not liftable"""
    out, lifted, unliftable = [], 0, 0
    for ln in text.split(b"\n")[:-1]:
        if ln[:1] != b"@":
            f = ln.split(b"\t")
            tail = b""
            b = bubble_number(f[2]) if f[1] != b"4" else None
            if b is not None:
                got = lift(bubbles[b], int(f[3]), f[5].decode())
                if got is None:
                    unliftable += 1
                else:
                    lifted += 1
                    tail = b"\tbO:Z:%s,%s,%s" % (first_word(f[2]).encode(), f[3], f[5])
                    f[2], f[3], f[5] = names[int(chrom[b])].encode(), b"%d" % got[0], got[1].encode()
            for i in range(11, len(f)):
                if f[i].startswith(b"XA:Z:"):
                    items = []
                    for item in f[i][5:].split(b";")[:-1]:
                        name, pos, cig, nm = item.rsplit(b",", 3)
                        ib = bubble_number(name)
                        if ib is not None:
                            got = lift(bubbles[ib], int(pos[1:]), cig.decode())
                            if got is None:
                                unliftable += 1
                            else:
                                lifted += 1
                                name, pos, cig = names[int(chrom[ib])].encode(), pos[:1] + b"%d" % got[0], got[1].encode()
                        items.append(b",".join((name, pos, cig, nm)) + b";")
                    f[i] = b"XA:Z:" + b"".join(items)
            ln = b"\t".join(f) + tail
        out.append(ln)
    return b"\n".join(out) + b"\n", lifted, unliftable


def expected_records(places, loci, alt_off, alts, item_loci, bubbles, chrom):
    """the rule on records: placement records and their LOCUS_DTYPE records (pad_model.expected_loci), items and theirs -> (kinds, [None |
    (pos, seqid, [(len, op)])]) over the placements: the primaries, then the items"""
    import alt_model
    code = {"M": bw.LIFT_M, "I": bw.LIFT_I, "D": bw.LIFT_D, "S": bw.LIFT_S}
    kinds, recs = [], []
    for rec, lc in itertools.chain(zip(places, loci), zip(alts, item_loci)):
        b = int(lc["bubble"])
        if b < 0 or int(lc["seqid"]) < 0:
            kinds.append(bw.LIFT_NONE)
            recs.append(None)
            continue
        rev = bool(rec["flags"] & bw.PLACE_REVERSE)
        got = lift(bubbles[b], int(lc["pos1"]), alt_model.cigar(int(rec["aln_length"]), rec["gap_run"], rev))
        kinds.append(bw.LIFT_LIFTED if got else bw.LIFT_UNLIFTABLE)
        recs.append((got[0], int(chrom[b]), [(n, code[op]) for n, op in parse_cigar(got[1])]) if got else None)
    return np.array(kinds, dtype=np.uint8), recs


def compare_records(got, want_kinds, want_recs):
    """got: (kinds, lift_off, words) of Context.slot_lift / lift_records -> None, or the first difference"""
    kinds, off, words = got
    if len(kinds) != len(want_kinds) or len(off) != len(kinds) + 1:
        return f"{len(kinds)} placements, {len(want_kinds)} expected"
    bad = np.flatnonzero(kinds != want_kinds)
    if len(bad):
        return f"placement {bad[0]}: kind {kinds[bad[0]]}, expected {want_kinds[bad[0]]} ({want_recs[bad[0]]})"
    at = 0
    for q, rec in enumerate(want_recs):
        if int(off[q]) != at:
            return f"placement {q}: record at word {int(off[q])}, expected {at}"
        if rec is None:
            continue
        size = 1 + (len(rec[2]) + 3) // 4
        have = bw.lift_record(words, at)
        pad = words[at + 1:at + size].reshape(-1)[len(rec[2]):]
        if have != rec or pad.any() or words[at][3] >> 8:
            return f"placement {q}: {have}, expected {rec}"
        at += size
    return None if int(off[-1]) == at == len(words) else f"{int(off[-1])} words, expected {at}"


# ---- the generator ---------------------------------------------------------------------------------------------------------------------

BUBBLES = (  # (name, position p of the last base before the allele, reference bases replaced, alternate bases, ref_len written)
    ("ins1", 400, 0, "T", 0), ("ins5", 800, 0, "GATTC", 0), ("del1", 1200, 1, "", 1), ("del7", 1600, 7, "", 7), ("del130", 2100, 130, "", 130),
    ("complex", 2700, 2, "CAG", 2), ("dot", 3100, 1, "ACG", 0), ("head", 60, 0, "GG", 0), ("tail", None, 0, "TTA", 0),
)


def genome(seed=11, length=3600, code_bases=(2,)):
    """-> dict: chrom (text, IUPAC codes included), records [(name, text, cmap)], bubbles (pad_model.load_bubbles tuples), data (bubble.data
    bytes), fasta (the multi-genome's text), names (the .ann names in text order)
    code_bases: the sizes of the IUPAC sets the flanks' codes are drawn from"""
    rnd = random.Random(seed)
    chrom = [rnd.choice("ACGT") for _ in range(length)]
    bubbles, records = [], []
    for k, (_, p, ref, alt, ref_len) in enumerate(BUBBLES):
        if p is None:  # the allele behind the chromosome's last base: no right flank, D_minus_C = -1
            p = length
        A = max(1, p - FLANK + 1)
        Bm = p - A + 1
        C = p + 1 + ref
        Dm = min(FLANK - 1, length - C)
        for where in (A + 7, A + Bm - 3, C + 2, C + Dm - 5):  # a few IUPAC codes in the flanks
            if 1 <= where <= length and chrom[where - 1] in "ACGT" and rnd.random() < 0.7:
                chrom[where - 1] = rnd.choice([c for c, s in IUPAC.items() if chrom[where - 1] in s and len(s) in code_bases])  # (two-base codes: the reference's search often misses a read on a code of three bases, tools/lift_generated_reference.py)
        bubbles.append((b"chrG generated seed=%d" % seed, A, Bm, C, Dm, ref_len, len(alt)))
        # a read that reaches one base beyond a flank must not lie as well on the chromosome itself: the chromosome's base behind the left
        # flank differs from the record's, and so does the one before the right flank
        avoid = {}
        if p + 1 <= length:
            avoid.setdefault(p + 1, set()).add(alt[0] if alt else chrom[C - 1] if C <= length else "")
        if C - 1 >= 1:
            avoid.setdefault(C - 1, set()).add(alt[-1] if alt else chrom[p - 1])
        for where, not_these in avoid.items():
            if chrom[where - 1] in not_these:
                chrom[where - 1] = next(c for c in "ACGT" if c not in not_these and (alt or (c != chrom[p - 1] and (C > length or c != chrom[C - 1]))))
    text = "".join(chrom)
    for k, ((_, _, _, alt, _), (_, A, Bm, C, Dm, _, _)) in enumerate(zip(BUBBLES, bubbles)):
        rec = text[A - 1:A - 1 + Bm] + alt + text[C - 1:C + Dm]
        cmap = list(range(A, A + Bm)) + [None] * len(alt) + list(range(C, C + Dm + 1))
        assert len(rec) == len(cmap) == Bm + len(alt) + Dm + 1
        records.append((f"bubble{k} chrG {A + Bm - 1}", rec, cmap))
    name = f"chrG generated seed={seed}"
    fasta = f">{name}\n" + "\n".join(text[i:i + 60] for i in range(0, length, 60)) + "\n"
    for rname, rec, _ in records:
        fasta += f">{rname}\n" + "\n".join(rec[i:i + 60] for i in range(0, len(rec), 60)) + "\n"
    data = b"".join(b[0] + b"\n" + b"\t".join(b"%d" % v for v in b[1:]) + b"\n" for b in bubbles)
    return {"chrom": text, "records": records, "bubbles": bubbles, "data": data, "fasta": fasta, "names": [name] + [r[0] for r in records]}


def boundaries(bubble):
    """the 0-based record offsets where a zone begins"""
    _, _, Bm, _, Dm, _, alt = bubble
    return [0, Bm, Bm + alt, Bm + alt + Dm + 1]


def reads(g, seed=5):
    """[(name, bubble, offset, length, strand, edit, SEQ as SAM prints it on the forward strand, CIGAR on the record)]: reads of 100 and 60 bases cut
    from every record at every third offset and at every offset within 3 of a zone boundary, without N (an IUPAC code of the record becomes
    one base of its set), on both strands; and a second set with one inserted or one deleted base, at least 6 from either end, near a boundary"""
    rnd = random.Random(seed)
    out = []
    for k, (_, rec, _) in enumerate(g["records"]):
        edges = boundaries(g["bubbles"][k])
        for ln in (100, 60):
            for o in range(0, len(rec) - ln + 1):
                near = any(abs(o - e) <= 3 or abs(o + ln - e) <= 3 for e in edges)
                if not (near or o % 3 == 0):
                    continue
                seq = "".join(rnd.choice(IUPAC[c]) for c in rec[o:o + ln])
                strand = "+-"[(o + ln) & 1]
                out.append((f"g{k}_o{o}_l{ln}_{strand}", k, o, ln, strand, None, seq, f"{ln}M"))
            for e in edges[1:3]:  # one inserted / one deleted base beside the allele's edges
                for shift in (-9, 8):
                    for edit in ("I", "D"):
                        at = e + shift  # record offset of the edit
                        o = max(0, min(at - 30, len(rec) - ln - 1))
                        a = at - o
                        if not (6 <= a <= ln - 7) or o + ln + 1 > len(rec):
                            continue
                        if edit == "I":
                            seq = "".join(rnd.choice(IUPAC[c]) for c in rec[o:o + ln - 1])
                            seq = seq[:a] + rnd.choice("ACGT") + seq[a:]
                            cig = f"{a}M1I{ln - 1 - a}M"
                        else:
                            seq = "".join(rnd.choice(IUPAC[c]) for c in rec[o:o + a] + rec[o + a + 1:o + ln + 1])
                            cig = f"{a}M1D{ln - a}M"
                        out.append((f"g{k}_o{o}_l{ln}_{edit}{a}_+", k, o, ln, "+", edit, seq, cig))
    return out


def fastq(read_list):
    """the FASTQ of reads(): a read of the reverse strand is written reverse-complemented, so that it maps there"""
    out = []
    for name, _, _, ln, strand, _, seq, _ in read_list:
        out.append(f"@{name}\n{seq[::-1].translate(COMP) if strand == '-' else seq}\n+\n{'I' * ln}\n")
    return "".join(out)


# ---- the judge -------------------------------------------------------------------------------------------------------------------------

def judge(cmap, pos1, cigar):
    """POS and CIGAR of a placement at pos1 of a record with the CIGAR `cigar`, from the record's cmap alone: a base on a character that copies
    a chromosome position is M there, any other an insertion; a deleted character that copies one is D; and where the chromosome positions of
    two consumed characters are not neighbours, the positions between them are deleted.  None: no M, or the span leaves the record"""
    per_base, x, prev = [], pos1, None
    span = sum(n for n, op in parse_cigar(cigar) if op in "MD")
    if pos1 < 1 or pos1 + span - 1 > len(cmap):
        return None
    for n, op in parse_cigar(cigar):
        for _ in range(n):
            if op == "I":
                per_base.append(("I", None, 1))
                continue
            c = cmap[x - 1]
            x += 1
            if c is None:
                if op == "M":
                    per_base.append(("I", None, 1))
                continue
            if prev is not None and c - prev > 1:
                per_base.append(("D", None, c - prev - 1))
            prev = c
            per_base.append(("M", c, 1) if op == "M" else ("D", None, 1))
    got = _finish(per_base)
    return None if got is None else (got[0], cigar_text(got[1]))


def mismatches(chrom, pos, cigar, seq):
    """the bases of SEQ under the M ops of a lifted line that the chromosome's text does not allow (a code matches the bases of its set)"""
    mm, c, i = 0, pos, 0
    for n, op in parse_cigar(cigar):
        if op == "M":
            mm += sum(1 for k in range(n) if seq[i + k] not in IUPAC.get(chrom[c + k - 1], ""))
            c, i = c + n, i + n
        elif op in "IS":
            i += n
        else:
            c += n
    assert i == len(seq)
    return mm


def gap_runs(cigar, reverse):
    """(aln_length, gap_run[8]) of a CIGAR text as bwb_place holds it: runs on the path aln2sam sees - the text order reversed on the forward
    strand - ascending by start, 0xFFFF for the unused ones"""
    ops = parse_cigar(cigar)
    alen = sum(n for n, _ in ops)
    runs, t = [], 0
    for n, op in ops:
        if op in "ID":
            runs.append(((t if reverse else alen - t - n) & 0xFF) | (n << 8) | (0x8000 if op == "D" else 0))
        t += n
    assert len(runs) <= 8 and all(n < 128 for n, op in ops if op in "ID") and alen < 256
    return alen, sorted(runs, key=lambda r: r & 0xFF) + [0xFFFF] * (8 - len(runs))


def place_records(placements):
    """[(text position, reverse, CIGAR text)] -> PLACE_DTYPE records of mapped, unique reads"""
    out = np.zeros(len(placements), dtype=bw.PLACE_DTYPE)
    for r, (pos, reverse, cigar) in enumerate(placements):
        alen, runs = gap_runs(cigar, reverse)
        out[r]["pos"], out[r]["flags"] = pos, bw.PLACE_MAPPED | (bw.PLACE_REVERSE if reverse else 0)
        out[r]["top1"], out[r]["mapq"], out[r]["aln_length"], out[r]["gap_run"] = 1, 37, alen, runs
        out[r]["ref_len"] = alen - sum(n for n, op in parse_cigar(cigar) if op == "I")
        out[r]["num_gapo"] = sum(1 for _, op in parse_cigar(cigar) if op in "ID")
    return out


def alt_records(placements):
    """the same as ALT_DTYPE records"""
    out = np.zeros(len(placements), dtype=bw.ALT_DTYPE)
    for r, (pos, reverse, cigar) in enumerate(placements):
        alen, runs = gap_runs(cigar, reverse)
        out[r]["pos"], out[r]["flags"] = pos, bw.PLACE_MAPPED | (bw.PLACE_REVERSE if reverse else 0)
        out[r]["aln_length"], out[r]["gap_run"] = alen, runs
        out[r]["num_gapo"] = sum(1 for _, op in parse_cigar(cigar) if op in "ID")
    return out
