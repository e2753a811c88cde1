"""Base qualities in the allele counts and the genotype calls (`bwbble map -b m` / `-Y`; include/bwbble_hip.h: bwb_hip_pileq_begin) restated in
Python for tests/test_pileq_host.py and tests/test_gpu_pileq.py.  Nothing here is fed anything the library computed.

  the rule      pile_q(): pile_model.pile() with a quality byte under every printed base -> counts, quality sums, reads, adds, dropped bases;
                rule_q(): the weighted costs from counts and sums by the closed formulas; site_records_q() / calls_bytes_q(): records and file
  a judge       judge_sam_q(): pile_model.judge_sam() extended to read the QUAL column of the SAM line itself - no walk, no text, no site
                numbering, no strand: SAM prints QUAL under SEQ; judge_q(): the costs one base at a time
  qualities     requal_fastq() rewrites a FASTQ's quality lines with a seeded generator, requal_sam() says what SAM must print under them
"""
import random

import numpy as np

import bwbble_amd as bw
import geno_model
import md_model
import pile_model

MAX_Q, MIN_W, H = 93, 4, geno_model.H
COLS = "ACGT"
HEADER_Q = geno_model.HEADER[:-1] + b"\tQS\n"


def base_q(c):
    """the quality of a QUAL byte"""
    return 0 if c < 33 else min(c - 33, MAX_Q)


def weight(c, err_cap):
    return min(max(base_q(c), MIN_W), err_cap)


def pile_q(text, placements, min_mapq=0, min_baseq=0, err_cap=0):
    """placements: (0-based text position, [(len, op)], SEQ as SAM prints it, MAPQ, QUAL bytes as SAM prints them) ->
    ({text position: [A, C, G, T]} counts, the same of quality sums (empty without err_cap), reads counted, adds, bases dropped by min_baseq)"""
    counts, sums, reads, adds, dropped = {}, {}, 0, 0, 0
    for start, ops, seq, mapq, qual in placements:
        if mapq < min_mapq or md_model.md(text, start, ops, seq)[0] != md_model.OK:
            continue
        assert len(qual) == len(seq)
        reads += 1
        i, t = 0, start
        for n, op in ops:
            if op == "M":
                for k in range(n):
                    if text[t + k] in pile_model.SITE_LETTERS and seq[i + k] in COLS:
                        if base_q(qual[i + k]) < min_baseq:
                            dropped += 1
                            continue
                        col = COLS.index(seq[i + k])
                        counts.setdefault(t + k, [0, 0, 0, 0])[col] += 1
                        if err_cap:
                            sums.setdefault(t + k, [0, 0, 0, 0])[col] += weight(qual[i + k], err_cap)
                        adds += 1
            i += n if op in "MIS" else 0
            t += n if op in "MD" else 0
    return counts, sums, reads, adds, dropped


def sam_placements_q(sam, names, starts):
    """pile_model.sam_placements() with the line's QUAL column"""
    quals = [ln.split(b"\t")[10] for ln in sam.split(b"\n")[:-1] if ln[:1] != b"@" and not int(ln.split(b"\t")[1]) & 4]
    return [p + (q,) for p, q in zip(pile_model.sam_placements(sam, names, starts), quals)]


def pile_sam_q(sam, text, names, starts, min_mapq=0, min_baseq=0, err_cap=0):
    return pile_q(text, sam_placements_q(sam, names, starts), min_mapq, min_baseq, err_cap)


def judge_sam_q(sam, fasta, min_mapq=0, min_baseq=0, err_cap=0):
    """SAM bytes and the FASTA -> {(RNAME, POS): (FASTA letter, [A, C, G, T] counts, [A, C, G, T] quality sums, [(letter, weight)] base by base)}:
    the plain SAM-specification pileup of pile_model.judge_sam with QUAL laid under SEQ, byte for base"""
    recs = {}
    for rec in fasta.split(">")[1:]:
        head, _, body = rec.partition("\n")
        recs[head] = recs[head.split()[0]] = body.replace("\n", "").upper()
    out = {}
    for ln in sam.split(b"\n"):
        f = ln.split(b"\t")
        if not ln or ln[:1] == b"@" or int(f[1]) & 4 or int(f[4]) < min_mapq:
            continue
        ref, pos, seq, qual, i = recs[f[2].decode()], int(f[3]), f[9].decode(), f[10], 0
        assert len(qual) == len(seq), f[0]
        digits = ""
        for ch in f[5].decode():
            if ch.isdigit():
                digits += ch
                continue
            n, digits = int(digits), ""
            if ch == "M":
                for k in range(n):
                    letter, c = ref[pos - 1 + k], qual[i + k]
                    q = 0 if c < 33 else c - 33 if c - 33 < 93 else 93
                    if letter in "KSBYMHVRDW" and seq[i + k] in "ACGT" and q >= min_baseq:
                        e = out.setdefault((f[2].decode().split()[0], pos + k), (letter, [0, 0, 0, 0], [0, 0, 0, 0], []))
                        wq = sorted((4, q, err_cap))[1] if err_cap else 0  # (E >= 4: the middle one is min(max(q, 4), E))
                        e[1]["ACGT".index(seq[i + k])] += 1
                        e[2]["ACGT".index(seq[i + k])] += wq
                        e[3].append((seq[i + k], wq))
            if ch in "MIS":
                i += n
            if ch in "MD":
                pos += n
        assert i == len(seq), f[0]
    return out


def table_arrays(text, counts, sums):
    """the two tables as the device holds them: (n_sites, 4) uint32 each, wrapping"""
    return pile_model.table_array(text, counts), pile_model.table_array(text, sums)


# ---- the weighted calls -----------------------------------------------------------------------------------------------------------------------

def rule_q(n, s, S):
    """n, s: the k = 2 or 3 alleles' counts and quality sums; S: the sum of all four quality columns -> (GT, GQ, PLs)"""
    raw = []
    for x, y in geno_model.GENOTYPES[:geno_model.n_geno(len(n))]:
        raw.append(S - s[x] if x == y else H * (n[x] + n[y]) + (S - s[x] - s[y]))
    return geno_model.finish(raw)


def judge_q(bases, k):
    """bases: (allele index below k or None, the base's weight q) one at a time -> (GT, GQ, PLs): a genotype pays q for a base it does not carry,
    a heterozygous one H for a base it carries"""
    cost = [0] * geno_model.n_geno(k)
    for b, q in bases:
        for j, (x, y) in enumerate(geno_model.GENOTYPES[:geno_model.n_geno(k)]):
            if x == y:
                cost[j] += 0 if b == x else q
            else:
                cost[j] += H if b in (x, y) else q
    return geno_model.finish(cost)


def site_records_q(text, counts, qsum, min_depth=1, first=0, n=None):
    """the text in letters, the (n_sites, 4) counters and quality sums -> the bw.GENO_SITE_Q_DTYPE records of the called sites among first .. first + n - 1"""
    where = pile_model.sites(text)
    n = len(where) - first if n is None else n
    out = []
    for s in range(first, first + n):
        v, u = [int(x) for x in counts[s]], [int(x) for x in qsum[s]]
        if sum(v) < min_depth:
            continue
        letter = text[where[s]]
        mem = geno_model.MEMBERS[letter]
        gt, gq, pl = rule_q([v[COLS.index(c)] for c in mem], [u[COLS.index(c)] for c in mem], sum(u))
        out.append((where[s], s, v, pile_model.NT16.index(letter), geno_model.n_geno(len(mem)), gt, gq, 0, pl + [0] * (6 - len(pl)), u))
    return np.array(out, dtype=bw.GENO_SITE_Q_DTYPE)


def calls_bytes_q(text, names, starts, site_recs, bubbles=None, bubble_recs=()):
    """the calls file under -Y: geno_model.calls_bytes() with the last column QS - the alleles' quality sums on S lines, `.` on I lines"""
    plain = geno_model.calls_bytes(text, names, starts, site_recs, bubbles, bubble_recs).split(b"\n")[1:-1]
    ends = [text.index("$", s) for s in starts]
    kept = [r for r in site_recs if any(s <= int(r["pos"]) <= e for s, e in zip(starts, ends))]  # (calls_bytes leaves a site in no record out)
    out = [HEADER_Q]
    for k, ln in enumerate(plain):
        if k < len(kept):
            mem = geno_model.MEMBERS[pile_model.NT16[int(kept[k]["code"])]]
            out.append(ln + b"\t" + ",".join(str(int(kept[k]["qs"][COLS.index(c)])) for c in mem).encode() + b"\n")
        else:
            out.append(ln + b"\t.\n")
    return b"".join(out)


def parse_calls_q(data):
    """calls file bytes under -Y -> geno_model.parse_calls()'s tuples, each with its QS ([sums] or None) appended"""
    lines = data.split(b"\n")
    assert lines[0] + b"\n" == HEADER_Q and lines[-1] == b"", lines[:1]
    qs = [ln.rsplit(b"\t", 1)[1] for ln in lines[1:-1]]
    plain = geno_model.parse_calls(geno_model.HEADER + b"".join(ln.rsplit(b"\t", 1)[0] + b"\n" for ln in lines[1:-1]))
    return [p + (None if q == b"." else [int(x) for x in q.split(b",")],) for p, q in zip(plain, qs)]


# ---- qualities ----------------------------------------------------------------------------------------------------------------------------------

EDGE_BYTES = b"!#~ \x7f"  # Q 0, Q 2, Q 93, a byte below `!` (Q 0) and a byte above `~` (Q 94 -> 93)


def requal_fastq(fastq, seed, fixed=None):
    """FASTQ bytes with every quality line rewritten -> (bytes, {read name: its quality line}).  Each line is a ramp that differs from its own
    reverse - so that a wrong orientation cannot pass - with seeded noise on it, and the edge bytes are sprinkled over the lines.  fixed: a
    function (name, length) -> the line, instead of the generator (the all-high lines of the equivalence test)"""
    rnd = random.Random(seed)
    lines = fastq.split(b"\n")
    out, quals = [], {}
    for k in range(0, len(lines) - 1, 4):
        name, n = lines[k][1:].split()[0], len(lines[k + 1])
        if fixed:
            q = fixed(name, n)
        else:
            lo, hi = rnd.randrange(33, 60), rnd.randrange(61, 127)
            q = bytearray(min(126, max(33, lo + (hi - lo) * i // max(n - 1, 1) + rnd.randrange(-3, 4))) for i in range(n))
            for _ in range(1 + n // 16):
                q[rnd.randrange(n)] = rnd.choice(EDGE_BYTES)
            if q[0] == 64:
                q[0] = 65  # (no line starts with `@`)
            if n > 1 and bytes(q) == bytes(q[::-1]):
                q[0], q[-1] = 34, 90
            q = bytes(q)
        assert len(q) == n and b"\n" not in q and b"\t" not in q
        out += [lines[k], lines[k + 1], lines[k + 2], q]
        quals[name] = q
    return b"\n".join(out) + b"\n", quals


def requal_sam(sam, quals):
    """SAM bytes with the QUAL column a reader of the rewritten FASTQ must print: the read's line, reversed on the reverse strand"""
    out = []
    for ln in sam.split(b"\n")[:-1]:
        if ln[:1] != b"@":
            f = ln.split(b"\t")
            q = quals[f[0]]
            f[10] = q[::-1] if int(f[1]) & 16 else q
            ln = b"\t".join(f)
        out.append(ln)
    return b"\n".join(out) + b"\n"


# ---- records: what Context.pile_records_q takes -------------------------------------------------------------------------------------------------

def record_placements_q(seqs, quals, lens, places, lift_kinds=None, lift_recs=None, starts=None, mapq=None):
    """pile_model.record_placements() with the reads' quality bytes ((n, stride) uint8 in FASTQ order): printed reversed on the reverse strand"""
    out = []
    base = {id_: p for id_, p in zip([r for r, p in enumerate(places) if (p["flags"] & bw.PLACE_MAPPED) and lens[r] <= 255],
                                     pile_model.record_placements(seqs, lens, places, lift_kinds, lift_recs, starts, mapq))}
    for r, p in base.items():
        q = bytes(bytearray(int(x) for x in quals[r][:int(lens[r])]))
        out.append(p + (q[::-1] if places[r]["flags"] & bw.PLACE_REVERSE else q,))
    return out


def expected_q(text, seqs, quals, lens, places, lift_kinds=None, lift_recs=None, starts=None, mapq=None, min_mapq=0, min_baseq=0, err_cap=0):
    """-> ((n_sites, 4) counters, (n_sites, 4) quality sums, reads counted, adds, dropped)"""
    counts, sums, reads, adds, dropped = pile_q(text, record_placements_q(seqs, quals, lens, places, lift_kinds, lift_recs, starts, mapq), min_mapq, min_baseq, err_cap)
    return pile_model.table_array(text, counts), pile_model.table_array(text, sums), reads, adds, dropped
