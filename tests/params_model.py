"""A small text and reads on which max_best and no_indel_length DECIDE something (bwb_params mirrors aln_params_t; `bwbble align` has no flag
for either field, a caller of the C-ABI sets them): built with tests/ovf_model.py, proved on the CPU by tests/test_params_host.py, run on the
GPU by tests/test_gpu_params.py.

max_best (inexact_match.c:339-340 for a popped hit, :353-354 for an exact tail; kl_search has one copy of each): the hits at the best score
add their interval widths to num_best; the first hit at another score ends the read's search if num_best > max_best.  So a read whose best
placements number T and that has one more placement within reach keeps ONE score's hits for max_best < T and the others as well from
max_best = T on.  T is counted here straight from the text (`threshold`), without any index.
  * plain families: R copies of a random unit between distinct spacers, two copies of the unit with one base replaced (at the read's first
    base, in the middle or at its last base: one end is the base the search consumes last, a hit popped with no base left; the others end in
    an exact tail), and the unit's own-substitution reads with one base deleted: a gapped placement, the only kind that scores above a
    one-mismatch best hit when no second difference is allowed (-n 1) - and the loop goes on to it only where it scores no more than
    mm_score above the best hit (:309-311), so these reads decide under a cheap gap open (-n 1 -O 4);
  * IUPAC families: the unit written k times over two-base codes that hold its bases - the best hits are a LIST of intervals, whose
    summed width is T;
  * per family the reads: the unit (best hit exact: popped entries, one interval R wide or one entry per interval), the unit with a
    substitution of its own at each of the two other sites (-n 2: the R copies arrive in one popped hit R wide; -n 1: through an exact tail whose
    list's summed width is what num_best grows by), and the reverse complement of each.

no_indel_length (:423-425): no gap is opened or extended while fewer than no_indel_length + (gaps so far) bases are left, or consumed.
  * reads of a plain random record with one deleted or one inserted base at distance d = 0 .. 8 from the head and from the tail, both strands;
  * reads with a second indel (two opens: -o 2) or a two-base gap (an extension: -e) at distance d from an end: their bound is one higher.
"""
import numpy as np

import ovf_model as om

READ_LEN = 50
SEED = 9
COPIES = (1, 2, 3, 4, 5, 8, 31, 33)       # R: around the default 30 as well
SITES = {"first": 0, "mid": 24, "last": READ_LEN - 1}
IUPAC_COPIES = (2, 3, 4, 5, 6, 7, 8, 9)   # k: intervals of the best hits' list (fewer where two variants merge)
ORDINARY = 3000
DIST = tuple(range(9))                    # d
DEL_AT = 23                               # the base a gapped variant lacks: far from both ends
MAX_BEST_MAX = 2**31 - 1
MAX_BEST_SWEEP = tuple(range(-1, 35)) + (MAX_BEST_MAX,)
NO_INDEL_SWEEP = (-3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 25, 300)  # 25: half a read - no indel anywhere
# what the GPU runs (tests/test_gpu_params.py, tests/params_worker.py).  The coarser sweeps keep both sides of every family's threshold.
MAX_BEST_EDGES = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30, 31, 32, 33, 34, MAX_BEST_MAX)
MAX_BEST_FEW = (0, 2, 3, 8, 9, 32, 33, MAX_BEST_MAX)
NO_INDEL_FEW = (-3, 0, 1, 2, 5, 6, 9, 25)
BEST_FLAG_SETS = (("-n", "0"), ("-n", "1"), ("-n", "1", "-O", "4"), ("-S", "-n", "2"), ("-P", "-n", "2"), ("-n", "2", "-o", "2"),
                  ("-S", "-n", "2", "-o", "2"), ("-n", "2", "-M", "70", "-O", "66", "-E", "64"))  # the last three: 32-byte heap entries
INDEL_FLAG_SETS = (("-n", "1"), ("-n", "2", "-o", "2", "-e", "2"), ("-n", "3", "-o", "1", "-e", "3"), ("-S", "-n", "2"), ("-P", "-n", "2"),
                   ("-n", "2", "-o", "1", "-e", "2", "-M", "70", "-O", "66", "-E", "64"), ("-S", "-n", "2", "-o", "2", "-e", "2"))


def key(flags, fields):
    return tuple(flags), tuple(sorted(fields.items()))


def _sub(read, at, step=1):
    """`read` with the base at `at` replaced by the step-th next of ACGT"""
    return read[:at] + "ACGT"[("ACGT".index(read[at]) + step) % 4] + read[at + 1:]


def _delete(read, at):
    return read[:at] + read[at + 1:]


TWO_BASE = {b: "".join(c for c in om.COMPAT[b] if len(om.IUPAC[c]) == 2) for b in "ACGT"}


def _two_base_variants(rng, unit, k):
    """k copies of `unit` with one to three bases written as a two-base code that holds them (like ovf_model.variants, but: the three-base
    codes B D H V are no children of the inexact search - O_alphabet does not count them, bwt.c:760-790 - only of the exact one; and the
    sites of the substitutions and of the deletion keep their base)"""
    free = [p for p in range(len(unit)) if p not in SITES.values() and p != DEL_AT]
    out = []
    for _ in range(k):
        v = list(unit)
        for _ in range(1 + rng.below(3)):
            p = rng.pick(free)
            v[p] = rng.pick(TWO_BASE[unit[p]])
        out.append("".join(v))
    return out


class ParamsFixture:
    """records: [(name, sequence)] of the FASTA; reads: name -> bases.  best_names: the reads of the max_best families (fam[name] = family);
    indel1 / indel2: the no_indel_length reads, name -> (kind, side, d)"""

    def __init__(self):
        rng = om.Lcg(SEED)
        self.records, self.reads, self.fam = [], {}, {}
        self.best_names, self.indel1, self.indel2 = [], {}, {}
        spacers = set()

        def spacer():
            while True:
                s = rng.bases(7)
                if s not in spacers:
                    spacers.add(s)
                    return s

        def family_reads(fam, unit, site):
            """the unit, its substituted reads at the other sites with their gapped variants (returned: what goes into the text), each in both
            strands.  No substituted read at the family's own site: it would lie one mismatch from the unit AND from both variants, all R + 2 of
            them best hits, and nothing but its gapped variant would be left to arrive after them."""
            extra = []
            self.reads[fam] = unit
            self.reads[fam + "_rc"] = om.revcomp(unit)
            names = [fam, fam + "_rc"]
            for s2, at in SITES.items():
                if s2 == site:
                    continue
                q = _sub(unit, at, 2)
                self.reads[f"{fam}_q{s2}"] = q
                self.reads[f"{fam}_q{s2}_rc"] = om.revcomp(q)
                names += [f"{fam}_q{s2}", f"{fam}_q{s2}_rc"]
                extra.append(_delete(q, DEL_AT))
            for n in names:
                self.fam[n] = fam
            self.best_names += names
            return extra

        for R in COPIES:
            for site, at in SITES.items():
                fam = f"r{R}{site}"
                unit = rng.bases(READ_LEN)
                parts = [unit] * R + [_sub(unit, at, 1), _sub(unit, at, 3)] + family_reads(fam, unit, site)
                self.records.append((fam, "".join(p + spacer() for p in parts)))
        for j, k in enumerate(IUPAC_COPIES):
            site = list(SITES)[j % 3]
            fam = f"u{k}{site}"
            unit = rng.bases(READ_LEN)
            parts = _two_base_variants(rng, unit, k) + [_sub(unit, SITES[site], 1), _sub(unit, SITES[site], 3)] + family_reads(fam, unit, site)
            self.records.append((fam, "".join(p + spacer() for p in parts)))
        ordn = rng.bases(ORDINARY)
        self.records.append(("ordinary", ordn))
        # one indel at distance d from an end: `del` lacks the source's base there, `ins` has one more in front of it
        k = 0
        for kind in ("del", "ins"):
            for side in ("head", "tail"):
                for d in DIST:
                    o = 20 + 57 * k
                    k += 1
                    at = d if side == "head" else READ_LEN - 1 - d
                    src = ordn[o:o + READ_LEN + 1]
                    r = om._edit(src, dels=(at,))[:READ_LEN] if kind == "del" else om._edit(src, ins=(at,))[:READ_LEN]
                    for strand in ("", "_rc"):
                        n = f"i1_{kind}_{side}{d}{strand}"
                        self.reads[n] = om.revcomp(r) if strand else r
                        self.indel1[n] = (kind, side, d)
        # a second difference of the gap kind: another indel of the same kind in the middle (two opens), or the neighbouring base as well (an extension)
        k = 0
        for kind in ("del", "ins", "del2"):
            for side in ("head", "tail"):
                for d in DIST[2:]:
                    o = 30 + 61 * k
                    k += 1
                    at = d if side == "head" else READ_LEN - 1 - d
                    src = ordn[o:o + READ_LEN + 3]
                    if kind == "del":
                        r = om._edit(src, dels=(at, 26))
                    elif kind == "ins":
                        r = om._edit(src, ins=(at, 26))
                    else:
                        r = om._edit(src, dels=(at, at + 1) if side == "head" else (at - 1, at))
                    r = r[:READ_LEN]
                    n = f"i2_{kind}_{side}{d}" + ("_rc" if k % 2 else "")
                    self.reads[n] = om.revcomp(r) if k % 2 else r
                    self.indel2[n] = (kind, side, d)
        assert max(30 + 61 * k, 20 + 57 * 36) + READ_LEN + 3 < ORDINARY
        self.names = list(self.reads)

    def fasta(self):
        return "".join(f">{n}\n{s}\n" for n, s in self.records)

    def text(self):
        return om.Text(self.records)

    def batch(self, names=None):
        """names -> the reads as the C-ABI and the oracle take them"""
        import bwbble_amd as bw
        return bw.encode_reads([self.reads[n] for n in (self.names if names is None else names)])


def mismatches(tx, read):
    """per window of the text (both strands, as indexed) the number of read bases the text's code is not compatible with; windows that
    hold an end of a record ('$') can hold no hit: -1"""
    n = len(tx.c) - len(read) + 1
    mm = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for i, ch in enumerate(read):
        w = tx.c[i:i + n]
        mm += ~tx.member[ch][w]
        bad |= w == 0
    mm[bad] = -1
    return mm


def threshold(tx, read, max_diff):
    """(T, more): the read's placements with the fewest mismatches - what num_best has grown to when the first hit at another score arrives -
    and whether substitutions alone give such a hit (one mismatch more, within max_diff); None when no placement has max_diff mismatches or
    fewer.  (A gap open costs more than a mismatch under every parameter set the tests use these reads with, and every read has a placement
    without a gap and with one mismatch at the most: its best hits are never gapped.)"""
    mm = mismatches(tx, read)
    ok = mm[mm >= 0]
    best = int(ok.min())
    if best > max_diff:
        return None
    return int((ok == best).sum()), best + 1 <= max_diff and bool((ok == best + 1).any())


def gap_ends(hit):
    """a hit of oracle_lib.parse_aln -> (path positions before its first gap run, after its last), None for a hit without a gap"""
    path = []
    for v in hit["states"]:
        path += [v & 3] * (v >> 2)
    gaps = [i for i, s in enumerate(path) if s != 0]
    return (gaps[0], len(path) - 1 - gaps[-1]) if gaps else None
