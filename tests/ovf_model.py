"""Texts and reads CONSTRUCTED so that the per-read capacities of the GPU path overflow, and an independent model of when they do
(tests/test_ovf_host.py checks every property on the CPU, tests/test_gpu_overflow.py runs them; tests/golden/make_golden_ovf.py pins
the oracle to the real reference on a reduced text of the same kind).  Product and test code only.

A read base is compatible with 7 of the 16 text codes (A with A R M W D H V).  calculate_d and the exact tail keep one SA interval per
DISTINCT compatible string of the text, so
  * a de Bruijn sequence of order k over m compatible letters gives a read that ends in k + 1 equal bases a list of m^k intervals, and
  * K copies of a read R with one to three bases replaced by other compatible codes give R one hit per distinct variant.
The random numbers come from the generator below (the streams of `random` and numpy are not promised across versions).
"""
import numpy as np

# The capacities of the three scratch classes and of the hit log.  Source: ensure_class (lcap, acap of class 0 / 1 / 2) and slot_upload
# (the log: max(8 * reads, 65 536) records; grow_log multiplies by 4) in bwbble_amd/csrc/bwb_hip.hip; a list is full at T + 15 > cap
# (list_full, bwb_lane.h) and the hit that finds n_alns >= acap overflows.  Stated here once: the tests take them from here.
LCAP = (4096, 8192, 1 << 20)
ACAP = (256, 1024, 1 << 16)
LIST_SLACK = 15
LOG_MIN, LOG_PER_READ, LOG_GROWTH = 1 << 16, 8, 4
SEED = 32  # set_default_aln_params: seed_length

CODES = "$TKGSBYCMHNVRDWA"  # the index's code of a character = its position here (index.c: nt16); SA order and child order follow it
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
COMPAT = {b: "".join(c for c in CODES if c in IUPAC and b in IUPAC[c]) for b in "ACGT"}  # N matches no read base
_COMPL = str.maketrans("ACGTRYSWKMBDHVN$", "TGCAYRSWMKVHDBN$")
_M64 = (1 << 64) - 1


class Lcg:
    """64-bit linear congruential generator (Knuth's MMIX constants), the high bits returned"""

    def __init__(self, seed):
        self.s = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & _M64
        for _ in range(4):
            self.next()

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & _M64
        return self.s >> 33

    def below(self, n):
        return self.next() % n

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def bases(self, n):
        return "".join("ACGT"[self.below(4)] for _ in range(n))


def revcomp(s):
    return s.translate(_COMPL)[::-1]


def de_bruijn(letters, order):
    """every `order`-mer over `letters` exactly once, as a linear string of len(letters)^order + order - 1 characters"""
    m, a, out = len(letters), [0] * (len(letters) * order), []

    def db(t, p):
        if t > order:
            if order % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, m):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = "".join(letters[i] for i in out)
    return s + s[:order - 1]


def list_class(n):
    """the smallest scratch class whose interval lists hold a list that grows to n intervals"""
    return next(k for k in range(3) if n + LIST_SLACK <= LCAP[k])


def hits_class(n):
    return next(k for k in range(3) if n <= ACAP[k])


def clear_of(n, caps, slack=0):
    """n lies at least one eighth of a capacity away from every capacity of `caps` (on the side it is on)"""
    return all(n + slack <= c - c // 8 or n >= c + c // 8 for c in caps[:2])


def log_cap(n_reads):
    return max(LOG_PER_READ * n_reads, LOG_MIN)


class Text:
    """the text `bwbble index` indexes for these FASTA records: every record with its '$', then the reverse complement of all of it"""

    def __init__(self, records):
        fwd = "".join(seq + "$" for _, seq in records)
        self.s = fwd + revcomp(fwd)
        lut = np.zeros(256, dtype=np.uint8)
        for i, ch in enumerate(CODES):
            lut[ord(ch)] = i
        self.c = lut[np.frombuffer(self.s.encode(), dtype=np.uint8)].astype(np.int64)
        self.member = {b: np.array([ch in COMPAT[b] for ch in CODES]) for b in "ACGT"}
        self.first = {}
        # The intervals of the codes c and c' that follow each other among the codes PRESENT in the text touch, so add_sa_interval
        # (align.c:93-110) merges them: the first step's list has one interval per RUN of compatible codes (A's seven are one run in a text
        # without N), and every later list one per distinct string with the LAST character replaced by its run.  (Longer strings are appended
        # in the order of their reversed spelling, in which two neighbours lie in different parts of the index: no other merges - the walk of
        # tests/test_ovf_host.py confirms it rank by rank.)
        present = np.unique(self.c)
        self.run = {}
        for b in "ACGT":
            ids, k, last = np.zeros(16, dtype=np.int64), -1, False
            for code in present:
                if self.member[b][code]:
                    k += not last
                    ids[code] = k
                last = bool(self.member[b][code])
            self.run[b] = ids

    def steps(self, read):
        """calculate_d on `read`, straight from the text: per step k (the read's last k + 1 bases, restarts as inexact_match.c:240-244) the tuple
        (num_diff, width = occurrences of compatible strings, intervals of the list = distinct compatible strings up to the last character's run)"""
        z, out = 0, []
        pos = cls = None  # None: the whole index
        for ch in reversed(read):
            if ch not in self.member:
                pos = np.zeros(0, dtype=np.int64)
            elif pos is None:
                if ch not in self.first:  # (the first step from the whole index: the same for every read)
                    at = np.flatnonzero(self.member[ch][self.c])
                    self.first[ch] = (at,) + np.unique(self.run[ch][self.c[at]], return_inverse=True)
                pos, uniq, cls = self.first[ch]
            else:
                cand, old = pos[pos > 0] - 1, cls[pos > 0]
                keep = self.member[ch][self.c[cand]]
                pos, old = cand[keep], old[keep]
                uniq, cls = np.unique(self.c[pos] + 16 * old, return_inverse=True)
            if len(pos) == 0:
                z += 1
                pos = cls = None
                out.append((z, len(self.c) + 1, 1))  # (the index has one row more than the text has characters: the end of the text)
            else:
                out.append((z, len(pos), len(uniq)))
        return out

    def peak(self, read):
        """(longest list of the read's calculate_d, longest list of its seed's)"""
        return (max(s[2] for s in self.steps(read)), max(s[2] for s in self.steps(read[:SEED])) if len(read) > SEED else 0)

    def tail_lists(self, read):
        """the list lengths of the exact search of `read` (`-n 0`: exact_match_bounded from the whole index, on the read's reverse complement as
        inexact_match sees it): the distinct compatible strings of every suffix of the reverse complement - as many as of the read's prefix
        of that length, the text holds both strands -, up to the step that finds none"""
        out = []
        for z, _, d in self.steps(revcomp(read)):
            if z:
                break
            out.append(d)
        return out


def variants(rng, read, k, least=1):
    """k copies of `read` with `least` to three bases replaced by another compatible code (prefix-stable: the first j of k + 1 are the same)"""
    out = []
    for _ in range(k):
        v = list(read)
        for _ in range(least + rng.below(4 - least)):
            p = rng.below(len(read))
            v[p] = rng.pick([c for c in COMPAT[read[p]] if c != read[p]])
        out.append("".join(v))
    return out


def family(seed, length, k, least=1):
    """(the read, the FASTA record that holds its k variants with two or three random bases between them)"""
    rng = Lcg(seed)
    read = rng.bases(length)
    parts = []
    for v in variants(rng, read, k, least):
        parts += [v, rng.bases(2 + rng.below(2))]
    return read, "".join(parts)


# (a list counts strings up to their last character's run: a run of k + 1 equal bases meets m^k intervals in a de Bruijn record of order k)
A5 = "MRDWA"                # 5^6 = 15 625 intervals at the seventh A: beyond class 1
C3 = "CYS"                  # 3^8 = 6 561 at the ninth C: beyond class 0, inside class 1; 3^7 = 2 187 at the eighth: inside class 0
RUN2, RUN1, RUN0 = "A" * 7, "C" * 9, "T" + "C" * 8
READ_LEN = 60

# name -> (seed, read length, copies).  The copies of the boundary families were chosen so that the ORACLE reports exactly the number of
# hits in the name at -n 0 (test_ovf_host.py asserts it); f188 / f330 / f1300 are the class-0 / 1 / 2 hit lists, an eighth clear of 256 and 1 024.
FAMILIES = {
    "f188": (101, 60, 200), "f330": (102, 60, 350), "f1300": (103, 60, 1700),
    "b255": (111, 40, 276), "b256": (112, 40, 287), "b257": (113, 40, 286),
    "b1023": (114, 40, 1369), "b1024": (115, 40, 1242), "b1025": (116, 40, 1314),
}
BIG = ("big", 121, 40, 10600, 2)  # the exact tail's list beyond class 1 (and the hit list beyond class 1 as well)


SHORT_OVERFLOWS = {"t2": "e2a", "t1": "e1b"}
QUIET = LCAP[0] - LCAP[0] // 8 - LIST_SLACK  # a list this long or shorter is an eighth of class 0's capacity clear of it


def _site(rng, run, at):
    """a READ_LEN-base read with `run` at offset `at`, random bases elsewhere (none that lengthens the run)"""
    s = list(rng.bases(READ_LEN))
    s[at:at + len(run)] = run
    for p in (at - 1, at + len(run)):
        if 0 <= p < READ_LEN and s[p] == run[-1]:
            s[p] = "G"
    return "".join(s)


def _edit(read, dels=(), ins=(), subs=()):
    """`read` with the bases at `dels` removed, a base inserted before each of `ins`, the bases at `subs` replaced (positions of `read`;
    the new base is the next of ACGT, so nothing here is random)"""
    nxt = dict(zip("ACGT", "CGTA"))
    out = []
    for i, ch in enumerate(read):
        if i in ins:
            out.append(nxt[ch])
        if i not in dels:
            out.append(nxt[ch] if i in subs else ch)
    return "".join(out)


# reads that have no exact hit and whose best placement needs gaps: name -> (source read, dels, ins, subs).  Two gap
# opens or three differences: what `-n 3 -o 2 -e 3` finds and `-n 2` (one gap open) cannot.
GAPPED = {
    "g_del_ins": ("p0", (38,), (50,), ()), "g_del_del": ("p1", (36, 48), (), ()), "g_ins_ins": ("p2", (), (37, 49), ()),
    "g_del2": ("p3", (40, 41), (), ()), "g_sub3": ("p4", (), (), (35, 44, 53)), "g_del_sub2": ("p5", (42,), (), (36, 52)),
    "g_f330_del_ins": ("f330", (36,), (48,), ()), "g_f1300_del2": ("f1300", (40, 41), (), ()), "g_f1300_sub3": ("f1300", (), (), (34, 43, 52)),
    "g_f330rc_ins_ins": ("f330_rc", (), (38, 50), ()),
}


class Fixture:
    """records: [(name, sequence)] of the FASTA; reads: name -> bases.  Read names: e<class> / s<class> + a letter: the list of the read's
    own calculate_d (e: the run ends the read) or of its seed's (s: the run ends the seed, position 31) peaks in that class, the other
    phase's list stays QUIET; p<j>: plain reads of the ordinary record, both phases QUIET; q<j>: reads no longer than the seed, with one or
    two substitutions, QUIET; and the names of `families`.  In a text this dense in IUPAC codes a random read's list reaches thousands of
    intervals by itself, so every read is drawn again until the model finds its lists where its name says (on the text before the reads
    are planted; tests/test_ovf_host.py asserts it on the final one)."""

    def __init__(self, families=tuple(FAMILIES), plain=40, short=40, ordinary=20000, seed=7, dense=True):
        rng = Lcg(seed)
        ordn = list(rng.bases(ordinary))
        self.records = [("ordinary", None)]
        if dense:
            self.records += [("dbA5", de_bruijn(A5, 6)), ("dbC3", de_bruijn(C3, 9))]
        self.reads = {}
        fam = {}
        for name in families:
            fam[name], rec = family(*(FAMILIES[name] if name in FAMILIES else BIG[1:]))
            self.records.append((name, rec))
        self.records[0] = ("ordinary", "".join(ordn))
        t0 = Text(self.records)
        slot = iter(range(100, ordinary - READ_LEN, 2 * READ_LEN))
        for cls, run in ((2, RUN2), (1, RUN1), (0, RUN0)) if dense else ():
            for kind, at in (("e", READ_LEN - len(run)), ("s", SEED - len(run))):
                for t in "ab":
                    for attempt in range(200):
                        s = _site(rng, run, at)
                        pk = t0.peak(s)
                        if pk[kind == "e"] <= QUIET - 64 and list_class(pk[kind == "s"]) == cls:
                            break
                    else:
                        raise AssertionError(f"no read of kind {kind}{cls} found")
                    o = next(slot)
                    ordn[o:o + READ_LEN] = s
                    self.reads[f"{kind}{cls}{t}"] = s
        ordn = "".join(ordn)
        self.records[0] = ("ordinary", ordn)
        j = 0
        while j < plain:
            o = rng.below(len(ordn) - READ_LEN)
            s = ordn[o:o + READ_LEN] if j % 2 == 0 else revcomp(ordn[o:o + READ_LEN])
            if max(t0.peak(s)) <= QUIET - 64:
                self.reads[f"p{j}"] = s
                j += 1
        j = 0
        while j < short:
            ln = 20 + rng.below(SEED - 20 + 1)
            o = rng.below(len(ordn) - ln)
            s = list(ordn[o:o + ln])
            for _ in range(1 + rng.below(2)):
                p = rng.below(ln)
                s[p] = rng.pick([b for b in "ACGT" if b != s[p]])
            if max(t0.peak("".join(s))) <= QUIET - 64:
                self.reads[f"q{j}"] = "".join(s)
                j += 1
        if dense:  # short reads whose OWN list overflows: the last 30 bases of a read whose list peaks at its end (the same peak, no seed)
            for n, src in SHORT_OVERFLOWS.items():
                self.reads[n] = self.reads[src][-30:]
        self.reads.update(fam)
        for n, (src, dels, ins, subs) in GAPPED.items():  # (a source read ..._rc: the reverse complement of that read)
            base = self.reads.get(src[:-3] if src.endswith("_rc") else src)
            if base is not None:
                self.reads[n] = _edit(revcomp(base) if src.endswith("_rc") else base, dels, ins, subs)

    def fasta(self):
        return "".join(f">{n}\n{s}\n" for n, s in self.records)

    def fastq(self, names):
        return "".join(f"@{n}\n{self.reads[n]}\n+\n{'I' * len(self.reads[n])}\n" for n in names)

    def text(self):
        return Text(self.records)


def big_fixture():
    """a text of its own for the family whose exact-tail list leaves class 1 (kept apart: the main text stays under a million rows)"""
    return Fixture(families=(BIG[0],), plain=16, short=0, ordinary=4000, seed=8, dense=False)


CALCD_READS = [f"{p}{c}{t}" for c in (0, 1, 2) for p in "es" for t in "ab"]


def golden_fixture():
    """the reduced text on which tests/golden/make_golden_ovf.py runs the real reference: the calculate_d overflows and the families of
    about 300 and 1 300 variants"""
    return Fixture(families=("f330", "f1300"), plain=8, short=8, ordinary=6000, seed=11)


def golden_reads(fx):
    """the reads of the golden FASTQ, in file order: name -> bases (the fixture's, GAPPED among them, then the families' other strand)"""
    out = dict(fx.reads)
    for n in ("f330", "f1300"):
        out[n + "_rc"] = revcomp(fx.reads[n])
    return out


def mixed_batch(fx):
    """the reads whose calculate_d overflows scattered among the plain ones -> names"""
    special = CALCD_READS
    plain = [n for n in fx.reads if n[0] == "p"]
    out = []
    for j, n in enumerate(plain):
        out.append(n)
        if j % 2 == 0 and j // 2 < len(special):
            out.append(special[j // 2])
    return out + special[(len(plain) + 1) // 2:]


def inherit_batch(fx):
    """reads no longer than the seed behind a long read whose calculate_d overflows (class 2 and 1, in the read and in the seed phase) or
    does not; read 22 is e2a and reads 23.. are short: streamed in batches of 23 reads, the CARRIED read is one that overflows.  Then short
    reads whose OWN calculate_d overflows (t1, t2), behind a source that fits class 0, that leaves it later than they do, and earlier"""
    q = [n for n in fx.reads if n[0] == "q"]
    p = [n for n in fx.reads if n[0] == "p"]
    out = p[:22] + ["e2a"] + q[:8] + [p[22], "s2a"] + q[8:14] + ["e1b"] + q[14:20] + [p[23]] + q[20:26] + ["s1a"] + q[26:34] + ["e0a"] + q[34:]
    out += [p[24], "t2", q[0], "t1", "s2b", "t1", q[1], "e1a", "t2", q[2], "t1"]
    assert out[22] == "e2a" and len(q) >= 36
    return out


def inherit_classes(fx, names):
    """per read of an inheritance batch: the class in which it is searched = the larger of its own list's class and, for a read no longer
    than the seed, of the class of the last longer read before it (whose D_seed it takes).  From the names: e / s / t + class."""
    own = lambda n: int(n[1]) if n[0] in "est" else 0
    out, src = [], 0
    for n in names:
        if len(fx.reads[n]) > SEED:
            src = own(n)
            out.append(src)
        else:
            out.append(max(own(n), src))
    return out


# Batches that fill the hit log: name -> [(read, copies)], in this order.  Every read at -n 0; a slot's log never shrinks, so each wants a
# slot (or a context) that held no larger batch before.
LOG_CASES = {
    "class0": [("f188", 400)],                 # no read beyond 200 hits: ST_OUT_OVF in class 0 alone
    "rerun1": [("p0", 16), ("f330", 230)],     # the log fills inside the class-1 re-run
    "rerun2": [("p0", 16), ("f1300", 60)],     # ... inside the class-2 re-run
    "twice": [("f1300", 200)],                 # more than four times the log: it grows twice
    "survive": [("p0", 40), ("f188", 370)],    # only the last reads find it full: what is in the log must survive the copy
}


def log_case(name):
    return [n for n, k in LOG_CASES[name] for _ in range(k)]
