"""The genotype calls of `-G` (include/bwbble_hip.h: bwb_hip_geno_begin) in plain Python, twice.

rule() is the rule from counts, as the kernels and host/geno.c have it: the raw costs of the genotypes in VCF order by the closed formulas.
judge() knows no closed form: it takes the bases one at a time - allele index or None for a base that is no allele - and adds to every
genotype what that base costs under it.  Both use Python's integers; nothing here is floating point.

The records are those of bw.GENO_SITE_DTYPE / bw.GENO_BUBBLE_DTYPE; calls_bytes() is the calls file.  crafted() makes, per code, the count vectors
the tests inject: every genotype the winner, every tie, the GQ and PL edges, the depth edge.
"""
import os

import numpy as np

import bwbble_amd as bw
import indel_model
import pile_model

H = 3
PL_MAX = (1 << 32) - 1
COLS = "ACGT"
MEMBERS = {"K": "GT", "S": "CG", "B": "CGT", "Y": "CT", "M": "AC", "H": "ACT", "V": "ACG", "R": "AG", "D": "AGT", "W": "AT"}  # in column order
GENOTYPES = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))  # VCF order; two alleles have the first three
HEADER = b"#kind\trecord\tpos\tid\talleles\tAD\tother\tGT\tGQ\tPL\n"
assert set(MEMBERS) == set(pile_model.SITE_LETTERS) and all("".join(sorted(m)) == m for m in MEMBERS.values())


def n_geno(k):
    return 6 if k == 3 else 3


def finish(raw):
    """raw costs -> (GT, GQ, PLs): the first smallest, the distance to the next, the differences saturated"""
    gt = raw.index(min(raw))
    gq = min(99, min(r - raw[gt] for j, r in enumerate(raw) if j != gt))
    return gt, gq, [min(r - raw[gt], PL_MAX) for r in raw]


def rule(n, depth, err):
    """n: the k = 2 or 3 alleles' counts; depth: all bases -> (GT, GQ, PLs)"""
    raw = []
    for x, y in GENOTYPES[:n_geno(len(n))]:
        raw.append(err * (depth - n[x]) if x == y else H * (n[x] + n[y]) + err * (depth - n[x] - n[y]))
    return finish(raw)


def judge(bases, k, err):
    """bases: an iterable of allele indices below k, or None for a base that is none of them -> (GT, GQ, PLs), one base at a time"""
    cost = [0] * n_geno(k)
    for b in bases:
        for j, (x, y) in enumerate(GENOTYPES[:n_geno(k)]):
            if x == y:
                cost[j] += 0 if b == x else err
            else:
                cost[j] += H if b in (x, y) else err
    return finish(cost)


def expand(counts4, letter):
    """a site's four counters -> judge()'s bases"""
    mem = MEMBERS[letter]
    out = []
    for col, v in zip(COLS, counts4):
        out += [mem.index(col) if col in mem else None] * int(v)
    return out


def site_records(text, counts, err=20, min_depth=1, first=0, n=None):
    """the text in letters and the (n_sites, 4) counters -> the records of the called sites among first .. first + n - 1"""
    where = pile_model.sites(text)
    n = len(where) - first if n is None else n
    out = []
    for s in range(first, first + n):
        v = [int(x) for x in counts[s]]
        depth = sum(v)
        if depth < min_depth:
            continue
        letter = text[where[s]]
        al = [v[COLS.index(c)] for c in MEMBERS[letter]]
        gt, gq, pl = rule(al, depth, err)
        out.append((where[s], s, v, pile_model.NT16.index(letter), n_geno(len(al)), gt, gq, 0, pl + [0] * (6 - len(pl))))
    return np.array(out, dtype=bw.GENO_SITE_DTYPE)


def bubble_records(bubbles, counts, w, err=20, min_depth=1, first=0, n=None):
    """the bubble table and the (n_bub, 4) counters -> the records of the called bubbles: eligible at anchor w, depth >= min_depth"""
    n = len(bubbles) - first if n is None else n
    out = []
    for b in range(first, first + n):
        v = [int(x) for x in counts[b]]
        depth = sum(v)
        if not indel_model.eligible(bubbles[b], w) or depth < min_depth:
            continue
        gt, gq, pl = rule(v[:2], depth, err)
        out.append((b, v, gt, gq, 0, pl, [0, 0, 0]))
    return np.array(out, dtype=bw.GENO_BUBBLE_DTYPE)


def calls_bytes(text, names, starts, site_recs, bubbles=None, bubble_recs=()):
    """the calls file: the header, the called sites in text order (one in no record is left out), the called bubbles in bubble order"""
    out = [HEADER]
    ends = [text.index("$", s) for s in starts]
    for r in site_recs:
        pos = int(r["pos"])
        letter = pile_model.NT16[int(r["code"])]
        mem = MEMBERS[letter]
        v = [int(x) for x in r["n"]]
        al = [v[COLS.index(c)] for c in mem]
        for name, s, e in zip(names, starts, ends):
            if s <= pos <= e:
                x, y = GENOTYPES[int(r["gt"])]
                out.append(b"S\t%s\t%d\t%s\t%s\t%s\t%d\t%s/%s\t%d\t%s\n" % (name.split()[0].encode(), pos - s + 1, letter.encode(), ",".join(mem).encode(), ",".join(str(a) for a in al).encode(),
                                                                     sum(v) - sum(al), mem[x].encode(), mem[y].encode(), int(r["gq"]), ",".join(str(int(p)) for p in r["pl"][:n_geno(len(mem))]).encode()))
                break
    for r in bubble_recs:
        b = bubbles[int(r["bubble"])]
        v = [int(x) for x in r["n"]]
        x, y = GENOTYPES[int(r["gt"])]
        out.append(b"I\t%s\t%d\t%d\tR,V\t%d,%d\t%d\t%s/%s\t%d\t%s\n" % (b[0].split()[0], b[1] + b[2], int(r["bubble"]), v[0], v[1], v[2] + v[3], b"RV"[x:x + 1], b"RV"[y:y + 1], int(r["gq"]),
                                                                  ",".join(str(int(p)) for p in r["pl"]).encode()))
    return b"".join(out)


def parse_calls(data):
    """calls file bytes -> [(kind, record, pos, id, alleles, AD, other, GT, GQ, PLs)]"""
    lines = data.split(b"\n")
    assert lines[0] + b"\n" == HEADER and lines[-1] == b"", lines[:1]
    out = []
    for ln in lines[1:-1]:
        f = ln.decode().split("\t")
        assert len(f) == 10, ln
        out.append((f[0], f[1], int(f[2]), f[3], f[4].split(","), [int(x) for x in f[5].split(",")], int(f[6]), f[7], int(f[8]), [int(x) for x in f[9].split(",")]))
    return out


# ---- the crafted count vectors ------------------------------------------------------------------------------------------------------------

def _cols(letter, al, other=0):
    """allele counts in member order (+ `other` on the first column that is no member) -> the four counters"""
    mem = MEMBERS[letter]
    v = [0, 0, 0, 0]
    for c, a in zip(mem, al):
        v[COLS.index(c)] = a
    v[[c not in mem for c in COLS].index(True)] += other
    return v


def crafted(letter):
    """[(what, E, d, [A, C, G, T])]: the vectors of one code.  `what` names the property; check_crafted() asserts that the model shows it."""
    k = len(MEMBERS[letter])
    out = []
    z = [0] * k

    def unit(i, v=1):
        u = list(z)
        u[i] = v
        return u
    for j, (x, y) in enumerate(GENOTYPES[:n_geno(k)]):  # every genotype the winner: 12 bases of x, or 6 of x and 6 of y
        al = list(z)
        if x == y:
            al[x] = 12
        else:
            al[x] = al[y] = 6
        # (a het of n + n bases costs 2 H n, either hom E n: below E = 7 no het can win, so the hets are asked for at 7 in place of 4)
        for err in (4 if x == y else 7, 20, 93):
            out.append((f"win{j}", err, 1, _cols(letter, al, 1)))
    # every two-way tie: two genotypes share the smallest cost and every other one costs more; the first in order wins (searched for, see _tie)
    for ja in range(n_geno(k)):
        for jb in range(ja + 1, n_geno(k)):
            found = _tie(k, ja, jb)
            if found:
                out.append((f"tie_{ja}_{jb}", found[0], 1, _cols(letter, found[1], found[2])))
    out.append(("tie_all", 20, 1, _cols(letter, z, 5)))  # other bases only: every genotype costs 5 E; a0/a0 with GQ 0
    out.append(("other_only", 93, 1, _cols(letter, z, 1)))
    # GQ 98, 99 and capped.  98: a het of 14 + 14 bases at E = 13 costs 84, either hom 182.  99 and 102: 33 and 34 bases of a0 at H = 3
    al = list(z)
    al[0] = al[1] = 14
    out.append(("gq98", 13, 1, _cols(letter, al)))
    out.append(("gq99", 20, 1, _cols(letter, unit(0, 33))))    # raw(0,1) - raw(0,0) = 99
    out.append(("gq_capped", 20, 1, _cols(letter, unit(0, 34))))   # 102 -> 99
    al = list(z)
    al[0], al[1] = 40, 9                                            # het (0,1): raw(0,1) = 147, raw(0,0) = 9 E = 180 (E = 20), raw(1,1) = 800: GQ 33
    out.append(("het_gq", 20, 1, _cols(letter, al)))
    # depth d - 1 and d
    out.append(("depth_below", 20, 7, _cols(letter, unit(k - 1, 5), 1)))
    out.append(("depth_at", 20, 7, _cols(letter, unit(k - 1, 5), 2)))
    out.append(("depth_zero", 20, 1, [0, 0, 0, 0]))
    # a PL at 2^32 - 2, at 2^32 - 1 and one beyond, saturated: raw(0,1) - raw(0,0) = H n_0 - (E - H) n_1
    for want, name in ((PL_MAX - 1, "pl_max_minus_1"), (PL_MAX, "pl_max"), (PL_MAX + 1, "pl_saturated")):
        out.append((name, *_search_pl(letter, want)))
    out.append(("counters_full", 93, 1, [0xFFFFFFFF] * 4))
    out.append(("counters_full_d", 4, (1 << 31) - 1, [0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF]))
    return out


# Two alleles: all 3 pairs.  Three alleles: 12 of the 15 - a hom x cannot tie alone with the het (y, z) that lacks it: hom x is the cheapest hom only
# when n_x >= n_y, n_z, and het (y, z) <= het (x, y) needs n_z >= n_x (E > H), so n_z = n_x and hom z ties as well.
TWO_WAY_TIES = {2: 3, 3: 12}
_TIES = {}


def _tie(k, ja, jb):
    """(E, allele counts, other) under which exactly the genotypes ja < jb share the smallest cost, or None when no counts up to 8 do"""
    if k not in _TIES:
        import itertools
        found = {}
        for err in (4, 5, 6, 7, 9, 12, 20):
            for al in itertools.product(range(9), repeat=k):
                for other in (0, 1):
                    pl = rule(list(al), sum(al) + other, err)[2]
                    zero = [j for j, p in enumerate(pl) if p == 0]
                    if len(zero) == 2:
                        found.setdefault(tuple(zero), (err, list(al), other))
        _TIES[k] = found
    return _TIES[k].get((ja, jb))


def _search_pl(letter, want):
    """(E, d, counters) under which a0/a0 wins and the het (0, 1) costs exactly `want` more: H n_0 - (E - H) n_1 = want"""
    for err in range(4, 94):
        for n1 in range(4):
            n0, rest = divmod(want + (err - H) * n1, H)
            if rest == 0 and n1 < n0 <= 0xFFFFFFFF:
                return err, 1, _cols(letter, [n0, n1] + [0] * (len(MEMBERS[letter]) - 2))
    raise AssertionError(want)


def check_crafted():
    """the coverage the vectors claim, asserted on the model: -> {letter: vectors}"""
    all_vectors = {}
    for letter, mem in MEMBERS.items():
        k = len(mem)
        vs = crafted(letter)
        seen = {}
        for what, err, d, v in vs:
            al = [v[COLS.index(c)] for c in mem]
            depth = sum(v)
            gt, gq, pl = rule(al, depth, err)
            seen[what] = (gt, gq, pl, depth, d)
            if what.startswith("win"):
                assert gt == int(what[3:]) and gq > 0, (letter, what, err, gt, gq)
            if what.startswith("tie_") and what != "tie_all":
                ja, jb = (int(x) for x in what[4:].split("_"))
                assert ja < jb and [j for j, p in enumerate(pl) if p == 0] == [ja, jb] and gt == ja and gq == 0, (letter, what, pl)
            if what in ("tie_all", "other_only"):
                assert gt == 0 and gq == 0 and set(pl) == {0} and sum(al) == 0
        assert {seen[f"win{j}"][0] for j in range(n_geno(k))} == set(range(n_geno(k)))
        ties = {w for w in seen if w.startswith("tie_") and w != "tie_all"}
        assert len(ties) == TWO_WAY_TIES[k], (letter, sorted(ties))
        assert seen["gq98"][0] == 1 and seen["gq98"][1] == 98
        assert seen["gq99"][1] == 99 and min(p for p in seen["gq99"][2] if p) == 99 and seen["gq_capped"][1] == 99 and min(p for p in seen["gq_capped"][2] if p) == 102
        assert seen["het_gq"][0] == 1 and seen["het_gq"][1] == 33
        assert seen["depth_below"][3] == seen["depth_below"][4] - 1 and seen["depth_at"][3] == seen["depth_at"][4]
        for what, true in (("pl_max_minus_1", PL_MAX - 1), ("pl_max", PL_MAX), ("pl_saturated", PL_MAX + 1)):
            err, _, v = next((e, d, v) for w, e, d, v in vs if w == what)
            n0, n1 = (v[COLS.index(c)] for c in mem[:2])
            assert H * n0 - (err - H) * n1 == true and seen[what][0] == 0 and seen[what][2][1] == min(true, PL_MAX), (letter, what)
        assert seen["pl_saturated"][1] == 99 and seen["counters_full"][3] == 4 * 0xFFFFFFFF and max(seen["counters_full"][2]) == PL_MAX
        all_vectors[letter] = vs
    return all_vectors


# ---- the diploid sample and the CPU-only chain ---------------------------------------------------------------------------------------------

SAMPLE_SEED, SAMPLE_STEP, SAMPLE_LEN = 21, 4, 100  # a read of 100 bases from every 4th offset of either haplotype: 25 x per haplotype
ALIGN = ["-n", "3", "-o", "1"]
MAX_MM, MAX_ALT, MIN_MAPQ, ANCHOR = 6, 5, 1, 5
COMP = str.maketrans("ACGT", "TGCA")


def diploid(g, seed=SAMPLE_SEED, step=SAMPLE_STEP, length=SAMPLE_LEN):
    """a diploid sample over lift_model.genome(): per IUPAC site of the chromosome a genotype drawn among the code's members, per bubble R/R, R/V or
    V/V; error-free reads from both haplotypes on both strands -> namespace: reads [(name, SEQ as written)], sites {1-based chromosome position:
    "x/y" in member order}, bubbles [0 R/R | 1 R/V | 2 V/V]"""
    import random
    import types
    rnd = random.Random(seed)
    chrom = g["chrom"]
    drawn = {i + 1: (rnd.choice(MEMBERS[c]), rnd.choice(MEMBERS[c])) for i, c in enumerate(chrom) if c in MEMBERS}
    bub_gt = [rnd.choice((0, 1, 2)) for _ in g["bubbles"]]
    het_on = [rnd.choice((0, 1)) for _ in bub_gt]  # the haplotype that carries V of an R/V bubble
    carries = [[gt == 2 or (gt == 1 and h == on) for h in (0, 1)] for gt, on in zip(bub_gt, het_on)]
    order = sorted(range(len(g["bubbles"])), key=lambda k: g["bubbles"][k][1] + g["bubbles"][k][2])
    haps, seen = [], {}
    for h in (0, 1):
        seq, i = [], 0
        for k in order:
            _, A, Bm, C, Dm, _, alt = g["bubbles"][k]
            p = A + Bm - 1
            seq += [(chrom[x], x + 1) for x in range(i, p)]
            i = p
            if carries[k][h]:
                seq += [(c, None) for c in g["records"][k][1][Bm:Bm + alt]]
                i = C - 1
        seq += [(chrom[x], x + 1) for x in range(i, len(chrom))]
        for c, pos in seq:
            if pos in drawn:
                seen.setdefault(pos, set()).add(h)
        haps.append("".join(drawn[pos][h] if pos in drawn else c for c, pos in seq))
    sites = {}
    for pos, pair in drawn.items():
        if seen.get(pos) == {0, 1}:  # (a site inside bases that a haplotype's V allele replaces has no genotype to compare with)
            mem = MEMBERS[chrom[pos - 1]]
            x, y = sorted(pair, key=mem.index)
            sites[pos] = f"{x}/{y}"
    reads = []
    for h, hap in enumerate(haps):
        offs = list(range(h * 2, len(hap) - length + 1, step))
        if offs[-1] != len(hap) - length:
            offs.append(len(hap) - length)
        for n, o in enumerate(offs):
            strand = "+-"[(n + h) & 1]
            seq = hap[o:o + length]
            reads.append((f"d{h}_o{o}_{strand}", seq[::-1].translate(COMP) if strand == "-" else seq))
    return types.SimpleNamespace(reads=reads, sites=sites, bubbles=bub_gt, haps=haps)


def build_chain(d, oracle=None):
    """the sample mapped without a GPU, written into d: the oracle's `align -n 3 -o 1` -> the models' placement records, items (-X 5) and suboptimal
    bytes -> `places2sam -B t -J -R -a 1 -w 5 [-A a -I i] [-G calls]` -> namespace of paths, tables, truth and bytes"""
    import subprocess
    import types

    import alt_model
    import join_model
    import lift_model
    import map_model
    import oracle_lib
    d = str(d)
    path = lambda n: os.path.join(d, n)

    def tool(args):
        r = subprocess.run([bw.HOST_BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        return r.stdout
    g = lift_model.genome()
    sample = diploid(g)
    fa, fq, data, aln = path("dip.fa"), path("dip.fq"), path("dip.data"), path("dip.aln")
    open(fa, "w").write(g["fasta"])
    open(data, "wb").write(g["data"])
    open(fq, "w").write("".join(f"@{name}\n{seq}\n+\n{'I' * len(seq)}\n" for name, seq in sample.reads))
    tool(["index", fa])
    tool(["fasta2ref", fa])
    orc = oracle or oracle_lib.load()
    n, _, _ = orc.align_fastq(fa + ".bwt", fq, aln, orc.params(ALIGN + ["-t", str(min(16, os.cpu_count() or 1))]))
    assert n == len(sample.reads)
    hits = oracle_lib.parse_aln(open(aln, "rb").read())
    idx = orc.load_index(fa + ".bwt", load_sa=True)
    places, _ = map_model.expected_places(orc, idx, hits, MAX_MM)
    off, alts, _ = alt_model.expected_alts(hits, MAX_ALT, alt_model.OracleSA(orc, idx))
    sub = join_model.suboptimal(hits, off, alts)
    orc.lib.bwb_or_free_index(idx)
    places.tofile(path("places.bin"))
    open(path("alts.bin"), "wb").write(join_model.alts_file_bytes(off, alts, sub))
    flags = ["places2sam", "-B", data, "-J", "-R"]
    tail = [fa, fq, path("places.bin")]
    tool(flags + ["-A", path("a.tsv"), "-a", MIN_MAPQ, "-I", path("i.tsv"), "-w", ANCHOR] + tail + [path("base.sam"), path("alts.bin")])
    log = tool(flags + ["-a", MIN_MAPQ, "-w", ANCHOR, "-G", path("calls.tsv")] + tail + [path("calls.sam"), path("alts.bin")])
    tool(flags + ["-a", MIN_MAPQ, "-G", path("sites.tsv")] + tail[:0] + [fa, fq, path("places.bin"), path("sites.sam"), path("alts.bin")])
    rd = lambda n: open(path(n), "rb").read()
    names, start, end = bw.read_ann(fa + ".ann")
    return types.SimpleNamespace(dir=d, fa=fa, fq=fq, data=data, g=g, sample=sample, names=list(names), start=start, log=log, base=rd("base.sam"), a_tsv=rd("a.tsv"), i_tsv=rd("i.tsv"),
                                 calls=rd("calls.tsv"), calls_sam=rd("calls.sam"))


def census(m):
    """the calls of the chain against the drawn genotypes -> (figures, [disagreements])"""
    g, sample = m.g, m.sample
    chrom_name = g["names"][0].split()[0]
    cmaps = {r[0].split()[0]: r[2] for r in g["records"]}
    out = {"sites with a genotype": len(sample.sites), "sites called": 0, "sites with GQ >= 20": 0, "site disagreements": 0, "called on a bubble record's allele": 0,
           "eligible bubbles": sum(indel_model.eligible(b, ANCHOR) for b in g["bubbles"]), "bubbles called": 0, "bubbles with GQ >= 20": 0, "bubble disagreements": 0}
    wrong = []
    for kind, rec, pos, ident, alleles, ad, other, gt, gq, pl in parse_calls(m.calls):
        if kind == "S":
            at = pos if rec == chrom_name else cmaps[rec][pos - 1]
            if at is None or at not in sample.sites:
                out["called on a bubble record's allele"] += 1
                continue
            out["sites called"] += 1
            if gq >= 20:
                out["sites with GQ >= 20"] += 1
                if gt != sample.sites[at]:
                    out["site disagreements"] += 1
                    wrong.append(("S", rec, pos, gt, sample.sites[at], ad, other, gq))
        else:
            out["bubbles called"] += 1
            if gq >= 20:
                out["bubbles with GQ >= 20"] += 1
                want = ("R/R", "R/V", "V/V")[sample.bubbles[int(ident)]]
                if gt != want:
                    out["bubble disagreements"] += 1
                    wrong.append(("I", int(ident), pos, gt, want, ad, other, gq))
    return out, wrong
