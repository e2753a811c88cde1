"""NM:i and MD:Z against the text (`bwbble map -D`) restated in Python for tests/test_md_host.py and tests/test_gpu_md.py.  Nothing here is fed
anything the library computed: the text comes from parsing the FASTA with this file's own nt16 table, and POS / CIGAR / SEQ from SAM lines.

  the rule      md(): include/bwbble_hip.h (bwb_md) on a text position, CIGAR ops and SEQ, base by base; tag_sam() applies it to SAM text
  a judge       judge(): knows no emission order - it expands MD to one item per reference position by the SAM specification's meaning, lays
                it under the CIGAR, and checks every item against the text: a letter must be the text's letter and the read base no member of
                it, a matched base must be a member, a deleted letter must be the text's, and NM must equal the recount
"""
import re

import numpy as np

import bwbble_amd as bw

LETTERS = "$TKGSBYCMHNVRDWA"  # the text's codes 0..15 (nt16)
MEMBERS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG",
           "N": "", "$": ""}  # the read bases a text letter matches: N and the separator match nothing
NONE, OK, TOO_LONG, MAX_SPAN = 0, 1, 2, 4096
READ_BASES = "AGCTN"  # read->seq codes
COMP = str.maketrans("ACGTN", "TGCAN")


def parse_cigar(text):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDS])", text)]


def fasta_text(fasta):
    """the forward text as the index holds it, in letters: every record's sequence in upper case, anything that is no IUPAC letter as N, and
    `$` behind every record -> (text, names, first positions)"""
    text, names, starts, at = [], [], [], 0
    for rec in fasta.split(">")[1:]:
        head, _, body = rec.partition("\n")
        seq = "".join(c if c in LETTERS[1:] else "N" for c in body.replace("\n", "").upper()) + "$"
        names.append(head[:256])
        starts.append(at)
        text.append(seq)
        at += len(seq)
    return "".join(text), names, starts


def codes(text):
    """the text as the one-byte codes of <fasta>.ref"""
    lut = np.zeros(256, dtype=np.uint8)
    for k, c in enumerate(LETTERS):
        lut[ord(c)] = k
    return lut[np.frombuffer(text.encode(), dtype=np.uint8)]


def printed(letter):
    return "N" if letter == "$" else letter


def md(text, start, ops, seq):
    """the rule: ops [(len, op)] from the 0-based text position start, seq as SAM prints it -> (kind, NM, MD text, mismatches)"""
    span = sum(n for n, op in ops if op in "MD")
    if span > MAX_SPAN:
        return TOO_LONG, 0, "", 0
    if start < 0 or start + span > len(text) or sum(n for n, op in ops if op in "MIS") != len(seq):
        return NONE, 0, "", 0
    out, run, mm, gaps, i, t, prev = [], 0, 0, 0, 0, start, None
    for n, op in ops:
        if op == "M":
            for _ in range(n):
                if seq[i] in MEMBERS[text[t]]:
                    run += 1
                else:
                    out.append(f"{run}{printed(text[t])}")
                    run, mm = 0, mm + 1
                i, t = i + 1, t + 1
        elif op == "D":
            if prev != "D":
                out.append(f"{run}^")
                run = 0
            out.append("".join(printed(c) for c in text[t:t + n]))
            t, gaps = t + n, gaps + n
        else:
            i += n
            gaps += n if op == "I" else 0
        prev = op
    out.append(str(run))
    return OK, mm + gaps, "".join(out), mm


def pairs(text, start, ops, seq):
    """the (read base, text letter) pairs that meet under the M ops of a placement of kind OK (none for another kind): what a set of cases covers"""
    if md(text, start, ops, seq)[0] != OK:
        return set()
    out, i, t = set(), 0, start
    for n, op in ops:
        if op == "M":
            out |= {(seq[i + k], text[t + k]) for k in range(n)}
        i += n if op in "MIS" else 0
        t += n if op in "MD" else 0
    return out


ALL_PAIRS = {(b, c) for b in "ACGTN" for c in LETTERS}  # 5 x 16: `$` is a code of its own - it matches nothing and prints N


def judge(text, start, ops, seq, nm, md_text):
    """None, or what is wrong with (NM, MD) for this placement - by the SAM specification's meaning of MD, not by the order the rule emits in"""
    if not re.fullmatch(r"\d+(?:(?:[A-Z]|\^[A-Z]+)\d+)*", md_text):
        return f"MD {md_text!r} is not <number>((<letter>|^<letters>)<number>)*"
    items = []  # one per reference position: "=" matched, ("X", letter) mismatched, ("^", letter) deleted
    for num, dele, letter in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md_text):
        items += ["="] * int(num) if num else [("^", c) for c in dele] if dele else [("X", letter)]
    i, t, k, recount = 0, start, 0, 0
    for n, op in ops:
        if op in "IS":
            i += n
            recount += n if op == "I" else 0
            continue
        for _ in range(n):
            if k >= len(items):
                return f"MD ends at reference position {t - start} of the alignment"
            it, k = items[k], k + 1
            if op == "D":
                if it == "=" or it[0] != "^" or it[1] != printed(text[t]):
                    return f"deleted position {t}: MD has {it}, the text {text[t]}"
                recount += 1
            elif it == "=":
                if seq[i] not in MEMBERS[text[t]]:
                    return f"position {t}: MD says match, but {seq[i]} is no member of {text[t]}"
            else:
                if it[0] != "X" or it[1] != printed(text[t]):
                    return f"position {t}: MD has {it}, the text {text[t]}"
                if seq[i] in MEMBERS[text[t]]:
                    return f"position {t}: MD says mismatch, but {seq[i]} is a member of {text[t]}"
                recount += 1
            i += op == "M"
            t += 1
    if k != len(items) or i != len(seq):
        return f"MD describes {len(items)} reference positions, the CIGAR {k}; {i} of {len(seq)} read bases"
    return None if recount == nm else f"NM {nm}, recount {recount}"


def line_md(f, text, names, starts):
    """the rule on the fields of a mapped SAM line as it is printed (plain or lifted): RNAME's first position + POS - 1, CIGAR, SEQ"""
    return md(text, starts[names.index(f[2].decode())] + int(f[3]) - 1, parse_cigar(f[5].decode()), f[9].decode())


def tag_sam(sam, text, names, starts):
    """SAM bytes without -D -> the bytes with -D: NM:i and MD:Z directly behind QUAL on every mapped line of kind OK; and the census
    {kind: lines} of the mapped lines"""
    out, census = [], {NONE: 0, OK: 0, TOO_LONG: 0}
    for ln in sam.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        if ln[:1] != b"@" and f[1] != b"4":
            kind, nm, mdt, _ = line_md(f, text, names, starts)
            census[kind] += 1
            if kind == OK:
                f[11:11] = [b"NM:i:%d" % nm, b"MD:Z:" + mdt.encode()]
                ln = b"\t".join(f)
        out.append(ln)
    return b"\n".join(out) + b"\n", census


def judge_sam(sam, text, names, starts):
    """the judge on every mapped line of SAM bytes written with -D -> [(QNAME, what is wrong)], and the number of lines judged"""
    bad, n = [], 0
    for ln in sam.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        if ln[:1] == b"@" or f[1] == b"4":
            continue
        n += 1
        if not (f[11].startswith(b"NM:i:") and f[12].startswith(b"MD:Z:")):
            bad.append((f[0], "no NM / MD behind QUAL"))
            continue
        why = judge(text, starts[names.index(f[2].decode())] + int(f[3]) - 1, parse_cigar(f[5].decode()), f[9].decode(), int(f[11][5:]), f[12][5:].decode())
        if why:
            bad.append((f[0], why))
    return bad, n


# ---- records: what Context.md_records / slot_md return -----------------------------------------------------------------------------------

def printed_seq(row, ln, reverse):
    s = "".join(READ_BASES[c] for c in row[:ln])
    return s[::-1].translate(COMP) if reverse else s


def expected_records(text, seqs, lens, places, lift_kinds=None, lift_recs=None, starts=None):
    """the rule on records: read codes, PLACE_DTYPE records and - lift_kinds[r] == LIFT_LIFTED: lift_recs[r] = (pos, seqid, [(len, op code)]) as
    lift_model.expected_records gives them, starts = the records' first positions - lift records -> (MD_DTYPE records, md_off, MD bytes)"""
    import alt_model
    recs, off, parts = np.zeros(len(places), dtype=bw.MD_DTYPE), np.zeros(len(places) + 1, dtype=np.uint64), []
    for r, p in enumerate(places):
        kind, nm, mdt = NONE, 0, ""
        if p["flags"] & bw.PLACE_MAPPED and lens[r] <= 255:
            rev = bool(p["flags"] & bw.PLACE_REVERSE)
            if lift_kinds is not None and lift_kinds[r] == bw.LIFT_LIFTED:
                pos, seqid, lops = lift_recs[r]
                start, ops = int(starts[seqid]) + pos - 1, [(n, "MID?S"[op]) for n, op in lops]
            else:
                start, ops = int(p["pos"]), parse_cigar(alt_model.cigar(int(p["aln_length"]), p["gap_run"], rev))
            kind, nm, mdt, _ = md(text, start, ops, printed_seq(seqs[r], int(lens[r]), rev))
        recs[r]["kind"], recs[r]["nm"], recs[r]["md_len"] = kind, nm, len(mdt)
        off[r + 1] = off[r] + len(mdt)
        parts.append(mdt)
    return recs, off, "".join(parts).encode()


def pack_lift(kinds, lift_recs):
    """(kinds, lift_off, words) as Context.slot_lift returns them, from python records: a header word and the ops, four to a 16-byte word"""
    off, words = np.zeros(len(kinds) + 1, dtype=np.uint64), []
    for r, k in enumerate(kinds):
        if k == bw.LIFT_LIFTED:
            pos, seqid, ops = lift_recs[r]
            hdr = np.zeros(1, dtype=bw.LIFT_DTYPE)
            hdr["pos"], hdr["seqid"], hdr["n_ops"] = pos, seqid, len(ops)
            body = np.zeros((len(ops) + 3) // 4 * 4, dtype=np.uint32)
            body[:len(ops)] = [(n << 4) | op for n, op in ops]
            words += [hdr.view(np.uint32).reshape(1, 4), body.reshape(-1, 4)]
        off[r + 1] = sum(len(w) for w in words)
    return np.asarray(kinds, dtype=np.uint8), off, np.concatenate(words) if words else np.zeros((0, 4), dtype=np.uint32)


def compare_records(got, want):
    """None, or the first difference between two (recs, md_off, text)"""
    if len(got[0]) != len(want[0]):
        return f"{len(got[0])} records, {len(want[0])} expected"
    for r in range(len(want[0])):
        g, w = got[0][r], want[0][r]
        gt, wt = got[2][int(got[1][r]):int(got[1][r + 1])], want[2][int(want[1][r]):int(want[1][r + 1])]
        if g.tobytes() != w.tobytes() or int(got[1][r]) != int(want[1][r]) or gt != wt:
            return f"read {r}: {g} at {int(got[1][r])} {gt!r}, expected {w} at {int(want[1][r])} {wt!r}"
    return None if int(got[1][-1]) == int(want[1][-1]) and got[2] == want[2] else f"{int(got[1][-1])} MD bytes, expected {int(want[1][-1])}"
