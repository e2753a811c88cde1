"""An index model for tests: the reference-format .bwt contents of ANY code string, a real BWT of a small text by plain suffix
sorting, exact prefix counts and the children of SA intervals - numpy only, no GPU (tests/test_idx_host.py checks it against
`bwbble index` and the oracle on the CPU; tests/test_gpu_index_shapes.py and tests/idx_shapes_worker.py run the GPU against it).
Written from the format as bwbble_amd/host/index.c (construct_bwt) and bwt_io.c (store_bwt) describe it.  Product and test code only.

Occ is defined on any string of 4-bit codes with one sentinel row, so `from_codes` reaches every length and every sentinel row - the
indexer only makes odd lengths (2 * seqLen + 1) and puts the sentinel where the sort puts suffix 0.
The random numbers come from the generator below (the streams of `random` and numpy are not promised across versions).
"""
import numpy as np

NEG = np.uint64(2**64 - 1)          # position -1
QUIRK = (5, 9, 11, 13)              # the codes O_alphabet does not count (B H V D)
CODES = "$TKGSBYCMHNVRDWA"          # index.c: nt16
COMPL = np.array([0, 15, 8, 7, 4, 11, 12, 3, 2, 13, 10, 5, 6, 9, 14, 1], dtype=np.uint8)  # index.c: iupacCompl
_BASE_CODES = np.array([15, 3, 7, 1], dtype=np.uint8)  # A G C T in read order (A0 G1 C2 T3)


def rand_u64(seed, n, stream=0):
    """n 64-bit values of a counter-based generator (splitmix64's finaliser over seed, stream and the index)"""
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xD1B54A32D192ED03 + stream * 0x2545F4914F6CDD1D + 1) & (2**64 - 1))
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def rand_below(seed, n, bound, stream=0):
    return (rand_u64(seed, n, stream) >> np.uint64(11)) % np.uint64(bound)


class Model:
    """what a .bwt file holds (hdr, C, bwt, O: the arrays bwbble_amd.Context takes; SA: the samples), the code string and, for a real BWT, the full SA"""

    def __init__(self, codes, sa0, sa=None):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = len(codes)
        assert n >= 2 and 0 <= sa0 < n and codes.max() < 16 and codes[sa0] == 0
        self.codes, self.sa0, self.length, self.sa = codes, int(sa0), n, sa
        self.num_words, self.num_sa, self.num_occ = (n + 7) // 8, (n + 31) // 32, (n + 127) // 128
        self.hdr = np.array([n, self.num_words, self.num_sa, self.num_occ, sa0], dtype="<u8")
        counted = np.delete(codes, sa0)
        self.C = np.zeros(17, dtype="<u8")
        self.C[1:] = np.cumsum(np.bincount(counted, minlength=16))
        padded = np.zeros(self.num_words * 8, dtype=np.uint32)
        padded[:n] = codes
        self.bwt = np.zeros(self.num_words, dtype="<u4")
        for k in range(8):  # first character in bits 31-28
            self.bwt |= padded[k::8] << np.uint32(28 - 4 * k)
        # O rows: inclusive of position 128 k, the sentinel row skipped, '$' separators counted as code 0
        self.O = np.ascontiguousarray(occ_at(codes, sa0, np.arange(0, n, 128, dtype=np.uint64))).astype("<u8").reshape(-1)
        self.SA = np.zeros(self.num_sa, dtype="<u8") if sa is None else np.ascontiguousarray(sa[::32], dtype="<u8")
        self.path = self.oracle_index = None

    def tobytes(self):
        return b"".join(a.tobytes() for a in (self.hdr, self.C, self.bwt, self.O, self.SA))

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self.tobytes())
        self.path = path
        return path

    def attach(self, oracle, path):
        """writes the file and loads it into the oracle: the reference for O_alphabet's view"""
        self._oracle = oracle
        self.oracle_index = oracle.load_index(self.write(path), load_sa=self.sa is not None)
        return self


def from_codes(codes, sa0):
    return Model(codes, sa0)


def suffix_array(text):
    """rows 0..n of the plain suffix order, the end of the text smaller than every character: row 0 is the empty suffix"""
    b = np.ascontiguousarray(text, dtype=np.uint8).tobytes()
    return np.array([len(b)] + sorted(range(len(b)), key=lambda i: b[i:]), dtype=np.int64)


def from_text(text):
    """the BWT of a text of codes in the indexer's conventions (construct_bwt): sa0_index is the row of suffix 0, stored as code 0"""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    sa = suffix_array(text)
    codes = text[sa - 1]  # (sa == 0 reads text[-1]: overwritten next)
    sa0 = int(np.flatnonzero(sa == 0)[0])
    codes[sa0] = 0
    return Model(codes, sa0, sa.astype(np.uint64))


def fasta_text(records):
    """the text `bwbble index` makes of FASTA records (fasta2ref): every record and its '$', then the reverse complement of all of it"""
    lut = np.full(256, 10, dtype=np.uint8)
    for i, ch in enumerate(CODES):
        lut[ord(ch)] = i
    fwd = np.concatenate([np.append(lut[np.frombuffer(s.upper().encode(), dtype=np.uint8)], np.uint8(0)) for s in records])
    return np.concatenate([fwd, COMPL[fwd[::-1]]])


def random_dna(seed, n, iupac_per_64=6):
    """n characters, mostly A C G T with a few of every other code: the BWT then holds all sixteen"""
    r = rand_below(seed, n, 64)
    s = rand_below(seed, n, 4, stream=1)
    o = rand_below(seed, n, 11, stream=2)
    other = "KSBYMHNVRDW"
    return "".join("ACGT"[int(b)] if int(x) >= iupac_per_64 else other[int(k)] for x, b, k in zip(r, s, o))


def occ_at(codes, sa0, pos):
    """Occ(c, pos) for c = 0..15: #c among codes[0 .. pos] without the sentinel row, 0 for pos == -1; one cumsum per code"""
    pos = np.asarray(pos, dtype=np.uint64)
    neg = pos == NEG
    p = np.where(neg, 0, pos).astype(np.int64)
    out = np.zeros((len(pos), 16), dtype=np.uint64)
    live = np.ones(len(codes), dtype=bool)
    live[sa0] = False
    for c in range(16):
        cs = np.cumsum((codes == c) & live)
        out[:, c] = np.where(neg, 0, cs[p])
    return out


def occ(codes, sa0):
    """the whole table: row i = Occ(., i)"""
    return occ_at(codes, sa0, np.arange(len(codes), dtype=np.uint64))


def rank_exact(m, pos):
    """C[j] + Occ(j, pos): what O() gives, with -1 and length - 1 as in bwt.c (C[j] and C[j + 1])"""
    return m.C[None, :16] + occ_at(m.codes, m.sa0, pos)


def rank_alpha_restated(m, pos):
    """O_alphabet restated: exact, but the codes 5, 9, 11, 13 of a regular position are C[j] - [first character of the 128-character block == j]"""
    pos = np.asarray(pos, dtype=np.uint64)
    out = rank_exact(m, pos)
    regular = (pos != NEG) & (pos != np.uint64(m.length - 1))
    first = m.codes[(np.where(regular, pos, 0).astype(np.int64) // 128) * 128]
    for j in QUIRK:
        out[:, j] = np.where(regular, m.C[j] - (first == j).astype(np.uint64), out[:, j])
    return out


def rank_alpha(m, pos):
    """O_alphabet as the oracle computes it (pinned to the reference by tests/test_oracle_golden.py); needs attach()"""
    out = m._oracle.O_alphabet(m.oracle_index, pos, 0)
    out[:, 0] = 0
    return out


def children(m, iL, iU, alpha, bits=64):
    """child j of [iL, iU] = [v(j, iL - 1) + 1, v(j, iU)], j = 1..15 (column 0 is zero), v = exact rank or O_alphabet's view per pair;
    returns (L, U, mask): mask bit j = L <= U.  bits: the width of a position in the kernels (32 for an index of fewer than 2^32 - 1 rows):
    O_alphabet's C[j] - 1 is -1 in that width when no smaller code occurs at all (C[j] == 0: crafted strings only, a real text has its '$')"""
    iL, iU = np.asarray(iL, dtype=np.uint64), np.asarray(iU, dtype=np.uint64)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=bool), iL.shape)
    with np.errstate(over="ignore"):
        pL = iL - np.uint64(1)  # 0 -> -1
    vL, vU = rank_exact(m, pL), rank_exact(m, iU)
    if alpha.any():
        aL, aU = rank_alpha(m, pL), rank_alpha(m, iU)
        vL, vU = np.where(alpha[:, None], aL, vL), np.where(alpha[:, None], aU, vU)
    L, U = vL + np.uint64(1), vU.copy()
    if bits == 32:
        L, U = L & np.uint64(0xFFFFFFFF), U & np.uint64(0xFFFFFFFF)
    L[:, 0] = 0
    U[:, 0] = 0
    ne = L <= U
    ne[:, 0] = False
    mask = (ne.astype(np.uint32) << np.arange(16, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    return L, U, mask


def walk_steps(m):
    """invPsi steps from every row to the next sampled one (row % 32 == 0), the step through the sentinel row included: what locate_stats counts"""
    n = m.length
    isa = np.zeros(n, dtype=np.int64)
    isa[m.sa.astype(np.int64)] = np.arange(n)
    lf = isa[(m.sa.astype(np.int64) - 1) % n]  # the row of the suffix one character earlier; suffix 0 goes to row 0 (the empty suffix, SA = n - 1)
    rows, steps = np.arange(n), np.zeros(n, dtype=np.int64)
    while True:
        act = rows % 32 != 0
        if not act.any():
            return steps
        rows[act] = lf[rows[act]]
        steps[act] += 1


# ---- crafted code strings -----------------------------------------------------------------------------------------------------
RANK_LENGTHS = (2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 640, 641, 703, 704, 705, 767)
CONTENTS = ("uniform", "single", "zero_first", "first5", "first9", "first11", "first13")


def sentinel_rows(length):
    """the sentinel placements of the rank family that exist for the length (row 0 holds the last character of a text, never the sentinel)"""
    last_blk, last_bkt = (length - 1) // 128 * 128, (length - 1) // 64 * 64
    rows = {1, 31, 32, 63, 64, 127, 128, 192, last_blk, last_bkt, length - 1}
    return sorted(r for r in rows if 1 <= r < length)


def crafted(length, sa0, content, seed=1):
    """a code string of the family: `content` of CONTENTS, then code 0 on the sentinel row"""
    if content == "single":
        codes = np.full(length, 1 + seed % 15, dtype=np.uint8)
    else:
        codes = rand_below(seed * 1000003 + length, length, 16).astype(np.uint8)
        if content == "zero_first":
            codes[::128] = 0
        elif content.startswith("first"):
            codes[::128] = int(content[5:])
    codes[sa0] = 0
    return codes


def rank_family():
    """(length, sentinel row, content): every length with every sentinel placement that exists for it on uniform contents, and every other
    content with two placements per length - a block start where there is one (the quirk codes and code 0 sit on block starts), and the last row.
    The product is pruned on the content axis only: a content changes the characters, not the geometry."""
    fam = []
    for n in RANK_LENGTHS:
        rows = sentinel_rows(n)
        two = sorted({max([r for r in rows if r % 128 == 0], default=rows[0]), n - 1, rows[0] if n % 128 == 1 else n - 1})
        for c in CONTENTS:
            fam += [(n, r, c) for r in (rows if c == "uniform" else two)]
    return fam


# ---- real BWTs ----------------------------------------------------------------------------------------------------------------
# One FASTA record of `bases` characters from random_dna(seed, bases) (or several: real_records).  `bwbble index` makes the text fwd $ revcomp(fwd $): 2 * bases + 2
# characters, an odd BWT length 2 * bases + 3.  trim = 1: the text without its last character, an even length the indexer never makes - built with
# from_text, like the two small ones are in the GPU test where the file has to come from the model anyway.
# The seeds were found once by search on the CPU (tests/test_idx_host.py: find_seed) and are asserted there with every claim of the table.
# (`bwbble index` accepts every FASTA, down to one base: no shape had to be made with from_text because the indexer rejected it.)
#    name                  bases seed trim   claims: BWT length, length % 128, sentinel row and where that is
REAL_SHAPES = (
    ("even0_lastblk",        703,   1, 1, dict(length=1408, res=0, sa0=1328, last_blk=True)),
    ("res1_blk",             639, 609, 0, dict(length=1281, res=1, sa0=1152, blk_start=True)),   # the last block is one row: length - 1 on a block start
    ("res63_bkt",            670,  87, 0, dict(length=1343, res=63, sa0=832, bkt_start=True)),   # length - 1 is the last character of a first bucket
    ("even64_low",           671,  18, 1, dict(length=1344, res=64, sa0=9, low=True)),           # the last block's second bucket lies past the text
    ("res65_blk",            671, 107, 0, dict(length=1345, res=65, sa0=384, blk_start=True)),   # length - 1 is the first character of a second bucket
    ("res127_bkt",           702, 247, 0, dict(length=1407, res=127, sa0=448, bkt_start=True)),
    ("tiny_low",              40,   7, 0, dict(length=83, res=83, sa0=8, low=True, last_blk=True)),   # one block
    ("two_blocks_lastblk",   100,   1, 0, dict(length=203, res=75, sa0=185, last_blk=True)),     # between 129 and 256 rows
    # several records with a common head: counted '$' rows right behind the sentinel row - in its bucket (zero_after) or in the second bucket
    # of its block (zero_next).  Only there does the count of code 0 - the sentinel-at-block-start exception of the re-layout, the walk's
    # correction for the sentinel row - reach a result: code 0 is never a child, and only the invPsi walk steps through a '$'
    ("multi_blk_zero_after", (8, 90), 36, 0, dict(length=1457, res=49, sa0=256, blk_start=True, zero_after=4)),
    ("multi_bkt_zero_after", (8, 90), 145, 0, dict(length=1457, res=49, sa0=1216, bkt_start=True, zero_after=2)),
    ("multi_blk_zero_next", (70, 30), 157, 0, dict(length=4341, res=117, sa0=4096, blk_start=True, zero_after=5, zero_next=2)),
    ("multi_lastblk_zero_after", (8, 90), 16, 0, dict(length=1457, res=49, sa0=1426, last_blk=True, zero_after=2)),
)


def real_records(bases, seed):
    """one record of `bases` characters, or for bases = (k, each) k records that begin with the same 14 characters: the suffixes that start at the
    records sort next to each other, so the rows around the sentinel row (suffix 0, the first record) hold the '$' in front of the others -
    code 0 rows that are counted, beside the one that is not"""
    if isinstance(bases, int):
        return [random_dna(seed, bases)]
    k, each = bases
    head = random_dna(seed, 14, iupac_per_64=0)
    return [head + random_dna(seed * 64 + i + 1, each - 14) for i in range(k)]


def real_text(bases, seed, trim):
    t = fasta_text(real_records(bases, seed))
    return t[:len(t) - trim] if trim else t


def shape_claims(m):
    """the properties the table speaks of"""
    n, s = m.length, m.sa0
    zeros = np.flatnonzero(m.codes == 0)
    return dict(length=n, res=n % 128, sa0=s, blk_start=s % 128 == 0, bkt_start=s % 64 == 0 and s % 128 != 0,
                last_blk=s // 128 == (n - 1) // 128, low=s < 32,
                zero_after=int(np.sum((zeros > s) & (zeros < s + 64 - s % 64))),          # counted code 0 rows behind the sentinel in its bucket
                zero_next=int(np.sum((zeros >= s + 64 - s % 64) & (zeros < s + 128 - s % 128))))  # ... and in the second bucket of its block


# ---- waves for wave_children --------------------------------------------------------------------------------------------------
# A wave is 64 pairs in lane order (bwb_hip_children: pair q is lane q % 64 of wave q / 64).  Side L of a pair is the position iL - 1, side U
# the position iU; a "regular" position is 0 .. length - 2 (-1 and length - 1 touch no bucket).  Buckets are 64 characters.
class Rng:
    """a stream of the counter-based generator above"""

    def __init__(self, seed):
        self.seed, self.k = seed, 0

    def below(self, bound, n=None):
        self.k += 1
        v = rand_below(self.seed, 1 if n is None else n, bound, stream=self.k).astype(np.int64)
        return int(v[0]) if n is None else v

    def perm(self, n):
        self.k += 1
        return np.argsort(rand_u64(self.seed, n, stream=self.k), kind="stable")


class Wave:
    def __init__(self, name, pL, pU, need=True, alpha=False):
        """pL, pU: the two POSITIONS of every lane (-1 allowed for pL)"""
        self.name = name
        self.iL = (np.asarray(pL, dtype=np.int64) + 1).astype(np.uint64)
        self.iU = np.asarray(pU, dtype=np.int64).astype(np.uint64)
        n = len(self.iL)
        self.need = np.broadcast_to(np.asarray(need, dtype=bool), (n,)).copy()
        self.alpha = np.broadcast_to(np.asarray(alpha, dtype=bool), (n,)).copy()

    def own_u_rows(self, length):
        """lanes that fetch a U bucket of their own: needed, side U regular and not in side L's bucket (side L regular)"""
        pL, pU = self.iL.astype(np.int64) - 1, self.iU.astype(np.int64)
        regL, regU = (pL >= 0) & (pL != length - 1), pU != length - 1
        return int(np.sum(self.need & regU & ~(regL & (pL // 64 == pU // 64))))


def _in_bucket(rng, length, b, n):
    """n regular positions of bucket b"""
    hi = min(64 * b + 64, length - 1)
    return 64 * b + rng.below(hi - 64 * b, n)


def _split_pairs(rng, length, n):
    """n pairs whose sides lie in different buckets, side L first"""
    nb = (length - 2) // 64 + 1  # buckets that hold a regular position
    bl = rng.below(nb - 1, n)
    bu = bl + 1 + (rng.below(nb, n) % (nb - 1 - bl))
    return (np.array([_in_bucket(rng, length, int(b), 1)[0] for b in bl]), np.array([_in_bucket(rng, length, int(b), 1)[0] for b in bu]))


def _same_pairs(rng, length, n, b=None):
    """n pairs inside one bucket (each its own unless b is given), side L not behind side U"""
    nb = (length - 2) // 64 + 1
    bs = np.full(n, b) if b is not None else rng.below(nb, n)
    a = np.array([_in_bucket(rng, length, int(x), 1)[0] for x in bs])
    c = np.array([_in_bucket(rng, length, int(x), 1)[0] for x in bs])
    return np.minimum(a, c), np.maximum(a, c)


def named_waves(length, seed):
    """the waves the issue of the direct wave_children test lists, for an index of `length` rows (at least three buckets); alpha is set by the caller"""
    rng = Rng(seed)
    nb = (length - 2) // 64 + 1
    assert nb >= 3
    out = []
    out.append(Wave("one_bucket", *_same_pairs(rng, length, 64, b=rng.below(nb - 1))))
    out.append(Wave("all_split", *_split_pairs(rng, length, 64)))
    for k in (24, 25, 48, 49):  # lanes with a U bucket of their own, the rest with both sides in one bucket, in shuffled lane order
        sL, sU = _split_pairs(rng, length, k)
        tL, tU = _same_pairs(rng, length, 64 - k)
        p = rng.perm(64)
        out.append(Wave(f"own_{k}", np.concatenate([sL, tL])[p], np.concatenate([sU, tU])[p]))
    sL, sU = _split_pairs(rng, length, 64)
    out.append(Wave("every_second_idle", sL, sU, need=np.arange(64) % 2 == 0))
    out.append(Wave("only_lane_63", sL, sU, need=np.arange(64) == 63))
    sL, sU = _split_pairs(rng, length, 64)
    root = np.isin(np.arange(64), (0, 5, 31, 32, 63))
    out.append(Wave("root_among_regular", np.where(root, -1, sL), np.where(root, length - 1, sU)))
    third = np.arange(64) % 3
    tL, tU = _same_pairs(rng, length, 64)
    out.append(Wave("iL0_or_iU_last", np.where(third == 0, -1, np.where(third == 1, sL, tL)), np.where(third == 0, sU, np.where(third == 1, length - 1, tU))))
    # both sides in one 128-character block, in its two buckets (blocks whose second bucket holds a regular position)
    nblk2 = (length - 2 - 64) // 128 + 1
    blk = rng.below(nblk2, 64)
    out.append(Wave("block_halves", 128 * blk + rng.below(64, 64), np.array([_in_bucket(rng, length, 2 * int(b) + 1, 1)[0] for b in blk])))
    # the last character of a bucket and the first of the next
    edge = 64 * (1 + rng.below(nb - 1, 64))
    out.append(Wave("bucket_edge", edge - 1, edge))
    out.append(Wave("empty_intervals", tL, tL))  # iL = iU + 1: both sides on one position, no child
    return out


def random_wave(length, rng, name, hot=()):
    """lanes of every kind mixed; `hot`: positions (superblock starts) some pairs straddle"""
    nb = (length - 2) // 64 + 1
    kind = rng.below(16, 64)
    sL, sU = _split_pairs(rng, length, 64)
    tL, tU = _same_pairs(rng, length, 64)
    pL = np.where(kind < 6, tL, sL)
    pU = np.where(kind < 6, tU, sU)
    pL = np.where((kind == 12) | (kind == 13), -1, pL)
    pU = np.where((kind == 13) | (kind == 14), length - 1, pU)
    if len(hot):
        h = np.asarray(hot, dtype=np.int64)[rng.below(len(hot), 64)]
        st = kind == 11
        pL = np.where(st, np.maximum(h - 1 - rng.below(130, 64), 0), pL)
        pU = np.where(st, np.minimum(h + rng.below(130, 64), length - 2), pU)
    return Wave(name, pL, pU, need=kind != 15, alpha=rng.below(2, 64) == 1)


def check_children(ctx, m, waves, tail=None, bits=64, allow_undefined=False):
    """runs the waves (each a multiple of 64 pairs, except the last) in one call and compares every child and mask with children(); returns the pair count"""
    iL, iU = np.concatenate([w.iL for w in waves]), np.concatenate([w.iU for w in waves])
    need, alpha = np.concatenate([w.need for w in waves]), np.concatenate([w.alpha for w in waves])
    if tail is not None:
        iL, iU, need, alpha = iL[:tail], iU[:tail], need[:tail], alpha[:tail]
    names = np.concatenate([[w.name] * len(w.iL) for w in waves])[:len(iL)]
    L, U, mask = ctx.children(iL, iU, need=need, alpha=alpha)
    wL, wU, wmask = children(m, iL, iU, alpha, bits)
    # O_alphabet's value of a code 5, 9, 11, 13 is C[j] - [first character of the block == j]: -1 where C[j] == 0, a text without any smaller
    # code - not even a '$', which no indexed text is.  L and U are compared as they wrap in the kernels' width; whether such a child counts as
    # empty is not defined by anything (the reference would walk into [0, 2^64 - 1]), so its mask bit is left out - only where the caller allows
    # it: the rank family's strings of two or three characters.  The wave tests run on indexes where every C[j] > 0: the rule holds in full.
    undefined = sum(1 << j for j in QUIRK if m.C[j] == 0)
    assert allow_undefined or undefined == 0
    keep = np.where(alpha, ~np.uint32(undefined), ~np.uint32(0))
    bad = (need[:, None] & ((L != wL) | (U != wU))).any(axis=1) | ((mask & keep) != (np.where(need, wmask, 0) & keep))
    if bad.any():
        q = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{int(bad.sum())} of {len(iL)} pairs differ; first: wave {names[q]} pair {q} (lane {q % 64}) iL={int(iL[q])} iU={int(iU[q])} need={bool(need[q])} "
                             f"alpha={bool(alpha[q])}\n got L={L[q, 1:]} U={U[q, 1:]} mask={int(mask[q]):#x}\nwant L={wL[q, 1:]} U={wU[q, 1:]} mask={int(wmask[q]):#x}")
    return len(iL)
