"""Allele counts at the text's IUPAC sites (`bwbble map -A`) restated in Python for tests/test_pile_host.py and tests/test_gpu_pile.py.  Nothing here
is fed anything the library computed: the text comes from parsing the FASTA with this file's own nt16 table, the ops from md_model / lift_model.

  the rule      pile(): include/bwbble_hip.h (bwb_hip_pile_begin) on placements (text position, ops, SEQ, MAPQ) -> {text position: [A, C, G, T]};
                pile_sam() applies it to SAM text, expected_counts() to records as Context.pile_records takes them; tsv() is the writer
  a judge       judge_sam(): knows no walk, no text and no site numbering - a plain SAM-specification pileup of RNAME, POS, CIGAR, SEQ and MAPQ
                onto (record, position), on the FASTA's own records, keeping the positions whose FASTA letter is one of the ten
"""
import numpy as np

import bwbble_amd as bw
import md_model

NT16 = "$TKGSBYCMHNVRDWA"  # this file's own table of the text's codes 0..15
SITE_LETTERS = "KSBYMHVRDW"  # the ten codes with two or three members: 2 4 5 6 8 9 11 12 13 14
COLS = "ACGT"
HEADER = "#record\tpos\tcode\tA\tC\tG\tT\n"
assert [NT16.index(c) for c in SITE_LETTERS] == [2, 4, 5, 6, 8, 9, 11, 12, 13, 14]


def fasta_text(fasta):
    """the forward text in letters, as the index holds it -> (text, names, first positions); parsed here, with NT16"""
    text, names, starts, at = [], [], [], 0
    for rec in fasta.split(">")[1:]:
        head, _, body = rec.partition("\n")
        seq = "".join(c if c in NT16[1:] else "N" for c in body.replace("\n", "").upper()) + "$"
        names.append(head[:256])
        starts.append(at)
        text.append(seq)
        at += len(seq)
    return "".join(text), names, starts


def codes(text):
    lut = np.zeros(256, dtype=np.uint8)
    for k, c in enumerate(NT16):
        lut[ord(c)] = k
    return lut[np.frombuffer(text.encode(), dtype=np.uint8)]


def sites(text):
    """the text positions that are sites, in text order: site number k is sites(text)[k]"""
    return [i for i, c in enumerate(text) if c in SITE_LETTERS]


def site_of(text):
    """per text position its site number, or -1"""
    out, k = np.full(len(text), -1, dtype=np.int64), 0
    for i, c in enumerate(text):
        if c in SITE_LETTERS:
            out[i], k = k, k + 1
    return out


def pile(text, placements, min_mapq=0):
    """placements: (0-based text position, [(len, op)], SEQ as SAM prints it, MAPQ) of the mapped primaries -> ({text position: [A, C, G, T]},
    reads counted, adds).  A placement counts when md_model's kind is OK and its MAPQ is at least min_mapq."""
    table, reads, adds = {}, 0, 0
    for start, ops, seq, mapq in placements:
        if mapq < min_mapq or md_model.md(text, start, ops, seq)[0] != md_model.OK:
            continue
        reads += 1
        i, t = 0, start
        for n, op in ops:
            if op == "M":
                for k in range(n):
                    if text[t + k] in SITE_LETTERS and seq[i + k] in COLS:
                        table.setdefault(t + k, [0, 0, 0, 0])[COLS.index(seq[i + k])] += 1
                        adds += 1
            i += n if op in "MIS" else 0
            t += n if op in "MD" else 0
    return table, reads, adds


def table_array(text, table):
    """the table as the device holds it: (n_sites, 4) uint32 in site order"""
    where = site_of(text)
    out = np.zeros((int((where >= 0).sum()), 4), dtype=np.uint32)
    for pos, v in table.items():
        out[where[pos]] = np.array(v, dtype=np.uint64) % (1 << 32)
    return out


def sam_placements(sam, names, starts):
    """the mapped lines of SAM bytes as pile() takes them: RNAME's first position + POS - 1, CIGAR, SEQ, MAPQ"""
    first = {n: s for n, s in zip(names, starts)}  # (RNAME is the whole name here; a lifted line prints the first word)
    first.update({n.split()[0]: s for n, s in zip(names, starts)})
    out = []
    for ln in sam.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        if ln[:1] != b"@" and not int(f[1]) & 4:
            out.append((first[f[2].decode()] + int(f[3]) - 1, md_model.parse_cigar(f[5].decode()), f[9].decode(), int(f[4])))
    return out


def pile_sam(sam, text, names, starts, min_mapq=0):
    return pile(text, sam_placements(sam, names, starts), min_mapq)


def tsv(text, names, starts, table):
    """the counts file: the header, then one line per site with a counter that is not zero, in text order; a site in no record is left out"""
    out = [HEADER]
    ends = [s + text.index("$", s) - s for s in starts]  # the record's `$`
    for pos in sorted(table):
        v = table[pos]
        if not any(v):
            continue
        for name, s, e in zip(names, starts, ends):
            if s <= pos <= e:
                out.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\n" % (name.split()[0], pos - s + 1, text[pos], *[x % (1 << 32) for x in v]))
                break
    return "".join(out).encode()


def parse_tsv(data):
    """counts file bytes -> {(record, 1-based position): (letter, [A, C, G, T])}"""
    lines = data.decode().split("\n")
    assert lines[0] + "\n" == HEADER and lines[-1] == "", lines[:1]
    out = {}
    for ln in lines[1:-1]:
        f = ln.split("\t")
        assert len(f) == 7 and (f[0], int(f[1])) not in out, ln
        out[(f[0], int(f[1]))] = (f[2], [int(x) for x in f[3:]])
    return out


# ---- the second judge: a plain pileup --------------------------------------------------------------------------------------------------

def judge_sam(sam, fasta, min_mapq=0):
    """SAM bytes and the FASTA -> {(RNAME, POS): (FASTA letter, [A, C, G, T])} for the positions with one of the ten letters that a read base
    A / C / G / T covers under an M; SEQ laid under the CIGAR as the SAM specification says, on the record RNAME names"""
    recs = {}
    for rec in fasta.split(">")[1:]:
        head, _, body = rec.partition("\n")
        recs[head] = recs[head.split()[0]] = body.replace("\n", "").upper()
    out = {}
    for ln in sam.split(b"\n"):
        f = ln.split(b"\t")
        if not ln or ln[:1] == b"@" or int(f[1]) & 4 or int(f[4]) < min_mapq:
            continue
        ref, pos, seq, i = recs[f[2].decode()], int(f[3]), f[9].decode(), 0
        digits = ""
        for ch in f[5].decode():
            if ch.isdigit():
                digits += ch
                continue
            n, digits = int(digits), ""
            if ch == "M":
                for k in range(n):
                    letter = ref[pos - 1 + k]
                    if letter in "KSBYMHVRDW" and seq[i + k] in "ACGT":
                        out.setdefault((f[2].decode().split()[0], pos + k), (letter, [0, 0, 0, 0]))[1]["ACGT".index(seq[i + k])] += 1
            if ch in "MIS":
                i += n
            if ch in "MD":
                pos += n
        assert i == len(seq), f[0]
    return out


# ---- records: what Context.pile_records takes ---------------------------------------------------------------------------------------------

def record_placements(seqs, lens, places, lift_kinds=None, lift_recs=None, starts=None, mapq=None):
    """read codes, PLACE_DTYPE records, lift records as md_model.expected_records takes them, and the MAPQ override -> pile()'s placements"""
    import alt_model
    out = []
    for r, p in enumerate(places):
        if not (p["flags"] & bw.PLACE_MAPPED) or lens[r] > 255:
            continue
        rev = bool(p["flags"] & bw.PLACE_REVERSE)
        if lift_kinds is not None and lift_kinds[r] == bw.LIFT_LIFTED:
            pos, seqid, lops = lift_recs[r]
            start, ops = int(starts[seqid]) + pos - 1, [(n, "MID?S"[op]) for n, op in lops]
        else:
            start, ops = int(p["pos"]), md_model.parse_cigar(alt_model.cigar(int(p["aln_length"]), p["gap_run"], rev))
        out.append((start, ops, md_model.printed_seq(seqs[r], int(lens[r]), rev), int(mapq[r]) if mapq is not None else int(p["mapq"])))
    return out


def expected_counts(text, seqs, lens, places, lift_kinds=None, lift_recs=None, starts=None, mapq=None, min_mapq=0):
    """-> ((n_sites, 4) uint32 counters, reads counted, adds)"""
    table, reads, adds = pile(text, record_placements(seqs, lens, places, lift_kinds, lift_recs, starts, mapq), min_mapq)
    return table_array(text, table), reads, adds
