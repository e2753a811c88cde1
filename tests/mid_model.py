"""A mid-size fixture with known truth for tests/test_mid_host.py and tests/test_gpu_mid_stream.py: the 3 M-character generated genome of the
`mid` fixtures (5 chromosomes, 1 200 insertion bubbles; 3 302 441 characters of text, 404 blocks of the site index), its bubble table, 6 000
`bwb_synth` reads whose names say where they were cut and 3 600 reads cut here across the bubbles - and what the CPU-only chain makes of them:

  the oracle's `align -n 3 -o 1`  ->  oracle_lib.parse_aln  ->  map_model.expected_places / alt_model.expected_alts (-X 5) / join_model.suboptimal
  ->  `places2sam -B t -J` (base), `... -R` (lifted) and `... -R -D -A a.tsv -a 1 -I i.tsv -w 5` (full)

No GPU is involved; the GPU tests hold `bwbble map` to these bytes, the CPU tests hold the chain to the Python models and to the reads' names.

  build(dir)    everything above, written into dir -> a namespace of paths, tables and bytes
  judged(m)     the Python models on the chain's bytes, computed once per namespace: the lifted and tagged text, the -A and -I tables and
                the figures `map` logs
  reads()       the generator: random.Random(3); every IUPAC code resolved to a random member; a `-` read is written reverse-complemented;
                the names carry kind, bubble and strand
"""
import os
import random
import subprocess
import types

import numpy as np

import alt_model
import bwbble_amd as bw
import indel_model
import join_model
import lift_model
import map_model
import md_model
import oracle_lib
import pad_model
import pile_model

GENOME = ["3000000", "5", "1200", "77"]                       # bwb_synth genome: characters, chromosomes, bubbles, seed
SYNTH_READS = ["6000", "100", "4242", "1.0", "2.0", "0.5"]  # bwb_synth reads: number, length, seed, % substitutions, % reads with an indel, % reads with an N
ALIGN = ["-n", "3", "-o", "1"]
MAX_MM, MAX_ALT, MIN_MAPQ, ANCHOR = 6, 5, 1, 5
FLANK = 124
ALT_OFFSETS = (40, 70, 100, 120)
COMP = str.maketrans("ACGT", "TGCA")


def fasta_records(fasta):
    return [(head, body.replace("\n", "").upper()) for head, _, body in (rec.partition("\n") for rec in fasta.split(">")[1:])]


def bubble_table(names, start, end):
    """the rule of tools/map_indel.py: `>bubbleK chrN p` with record length L -> the chromosome's header line, then p-123 124 p+1 123 0 L-248"""
    header = {n.split()[0]: n for n in names if not n.startswith("bubble")}
    out = []
    for n, s, e in zip(names, start, end):
        if n.startswith("bubble"):
            _, ch, p = n.split()
            p, ins = int(p), int(e) - int(s) + 1 - 2 * FLANK
            out.append(f"{header[ch]}\n{p - FLANK + 1}\t{FLANK}\t{p + 1}\t{FLANK - 1}\t0\t{ins}\n")
    return "".join(out)


def reads(records, seed=3):
    """[(name, SEQ as written)]: for bubble k with k % 3 == 0 the alt reads - 100 bases of the record from offsets 40, 70, 100 and 120; with
    k % 3 == 1 the record's characters 40 .. 149 with the base at read offset 81 deleted and with one inserted there, the chromosome's from
    p - 124 + 40 with the base at read offset 80 deleted and with one inserted there, each cut to 100, and the chromosome's 100 unedited"""
    rnd = random.Random(seed)
    chrom = {h.split()[0]: s for h, s in records if not h.startswith("bubble")}
    out = []

    def emit(kind, k, src, edit=None, at=0):
        seq = [rnd.choice(lift_model.IUPAC[c]) for c in src]
        if edit == "D":
            del seq[at]
        elif edit == "I":
            seq.insert(at, rnd.choice("ACGT"))
        seq = "".join(seq[:100])
        strand = rnd.choice("+-")
        assert len(seq) == 100
        out.append((f"{kind}_b{k}_{strand}", seq[::-1].translate(COMP) if strand == "-" else seq))

    for head, rec in records:
        if not head.startswith("bubble"):
            continue
        word, ch, p = head.split()
        k, p = int(word[6:]), int(p)
        if k % 3 == 0:
            for o in ALT_OFFSETS:
                emit(f"alt{o}", k, rec[o:o + 100])
        elif k % 3 == 1:
            c0 = p - FLANK + 40
            emit("adel", k, rec[40:150], "D", 81)
            emit("ains", k, rec[40:150], "I", 81)
            emit("rdel", k, chrom[ch][c0:c0 + 110], "D", 80)
            emit("rins", k, chrom[ch][c0:c0 + 110], "I", 80)
            emit("ref", k, chrom[ch][c0:c0 + 100])
    return out


def _tool(args):
    r = subprocess.run([bw.HOST_BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def build(d, oracle=None):
    d = str(d)
    path = lambda n: os.path.join(d, n)
    fa, fq, data, aln = path("g.fa"), path("g.fq"), path("g.data"), path("g.aln")
    subprocess.run([bw.SYNTH_BIN, "genome", fa] + GENOME, check=True)
    _tool(["index", fa])
    _tool(["fasta2ref", fa])
    names, start, end = bw.read_ann(fa + ".ann")
    open(data, "w").write(bubble_table(names, start, end))
    fasta = open(fa).read()
    subprocess.run([bw.SYNTH_BIN, "reads", fa, fq] + SYNTH_READS, check=True)
    gen = reads(fasta_records(fasta))
    with open(fq, "a") as f:
        f.write("".join(f"@{name}\n{seq}\n+\n{'2' * len(seq)}\n" for name, seq in gen))
    n_synth, n_reads = int(SYNTH_READS[0]), int(SYNTH_READS[0]) + len(gen)

    # the judge: the oracle's hits, the models' records, the host's writer
    orc = oracle or oracle_lib.load()
    n, _, _ = orc.align_fastq(fa + ".bwt", fq, aln, orc.params(ALIGN + ["-t", str(min(16, os.cpu_count() or 1))]))
    assert n == n_reads, (n, n_reads)
    hits = oracle_lib.parse_aln(open(aln, "rb").read())
    idx = orc.load_index(fa + ".bwt", load_sa=True)
    places, _ = map_model.expected_places(orc, idx, hits, MAX_MM)
    off, alts, _ = alt_model.expected_alts(hits, MAX_ALT, alt_model.OracleSA(orc, idx))
    sub = join_model.suboptimal(hits, off, alts)
    orc.lib.bwb_or_free_index(idx)
    places.tofile(path("places.bin"))
    open(path("alts.bin"), "wb").write(join_model.alts_file_bytes(off, alts, sub))
    tail = [fa, fq, path("places.bin")]
    logs = {}
    logs["base"] = _tool(["places2sam", "-B", data, "-J"] + tail + [path("base.sam"), path("alts.bin")])
    logs["lifted"] = _tool(["places2sam", "-B", data, "-J", "-R"] + tail + [path("lifted.sam"), path("alts.bin")])
    logs["full"] = _tool(["places2sam", "-B", data, "-J", "-R", "-D", "-A", path("a.tsv"), "-a", MIN_MAPQ, "-I", path("i.tsv"), "-w", ANCHOR] + tail + [path("full.sam"), path("alts.bin")])
    rd = lambda n: open(path(n), "rb").read()

    bubbles = pad_model.load_bubbles(data)
    first = {n.split()[0]: i for i, n in enumerate(names)}
    chrom = np.array([first[b[0].split()[0].decode()] for b in bubbles], dtype=np.int32)
    text, tnames, tstarts = md_model.fasta_text(fasta)
    assert tnames == list(names) and tstarts == [int(s) for s in start]
    return types.SimpleNamespace(dir=d, fa=fa, fq=fq, data=data, names=list(names), start=start, end=end, bubbles=bubbles, bub_of=pad_model.bubble_of(names, bubbles), chrom=chrom,
                                 text=text, starts=tstarts, gen=gen, n_synth=n_synth, n_reads=n_reads, places=places, off=off, alts=alts, sub=sub, logs=logs,
                                 base=rd("base.sam"), lifted=rd("lifted.sam"), full=rd("full.sam"), a_tsv=rd("a.tsv"), i_tsv=rd("i.tsv"))


SITE_CODES = [pile_model.NT16.index(c) for c in pile_model.SITE_LETTERS]
PLAIN_CODES = [pile_model.NT16.index(c) for c in "ACGTN"]


def site_numbers(codes):
    """per text position its site number, or -1: a cumulative count over the one-byte codes"""
    site = np.isin(codes, SITE_CODES)
    return np.where(site, np.cumsum(site, dtype=np.int64) - 1, -1), int(site.sum())


def check_site_index(ctx, codes):
    """set_text + pile_begin on a context, then k_site_of at every position of the text against site_numbers() -> the number of sites"""
    want, n_sites = site_numbers(codes)
    ctx.set_text(codes)
    assert ctx.pile_begin() == n_sites
    got = ctx.pile_site_of(np.arange(len(codes), dtype=np.uint64))
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])
    return n_sites


CARRY_WORDS = 65536 + 300  # k_site_count takes one block per 256 words of 32 characters; k_scan_sums takes 256 blocks per turn of its carry loop


def carry_text(seed=404):
    """codes of (65 536 + 300) * 32 + 5 characters, 258 blocks of the site index: words 65 280 .. 65 791 - the last block of the carry loop's first
    turn and the first of its second - hold site codes only (block sums of 8 192 on both sides of the turn); words 20 100 .. 20 699 hold none
    (a block sum of 0 among them); the rest is random with about 30 % site codes"""
    rng = np.random.default_rng(seed)
    n = CARRY_WORDS * 32 + 5
    codes = np.where(rng.random(n) < 0.3, rng.choice(SITE_CODES, n), rng.choice(PLAIN_CODES, n)).astype(np.uint8)
    codes[65280 * 32:65792 * 32] = rng.choice(SITE_CODES, 512 * 32)
    codes[20100 * 32:20700 * 32] = rng.choice(PLAIN_CODES, 600 * 32)
    return codes


def judged(m):
    """the Python models on the chain's bytes -> a namespace: lifted / n_lifted / unliftable (lift_model), tagged (md_model), a_tsv / pile_reads /
    pile_adds (pile_model, -a 1), counts / i_tsv / indel_reads / indel_adds (indel_model, -w 5 -a 1); computed once"""
    if getattr(m, "_judged", None) is None:
        lifted, n_lifted, unliftable = lift_model.lift_sam(m.base, m.bubbles, m.names, m.chrom)
        tagged, census = md_model.tag_sam(m.lifted, m.text, m.names, m.starts)
        table, pile_reads, pile_adds = pile_model.pile_sam(m.lifted, m.text, m.names, m.starts, MIN_MAPQ)
        counts, indel_reads, indel_adds = indel_model.count(indel_model.from_sam(m.full, m.names, m.bub_of), m.bubbles, m.chrom, ANCHOR, MIN_MAPQ)
        m._judged = types.SimpleNamespace(lifted=lifted, n_lifted=n_lifted, unliftable=unliftable, tagged=tagged, census=census, table=table,
                                          a_tsv=pile_model.tsv(m.text, m.names, m.starts, table), pile_reads=pile_reads, pile_adds=pile_adds, counts=counts,
                                          i_tsv=indel_model.table_bytes(m.bubbles, counts), indel_reads=indel_reads, indel_adds=indel_adds,
                                          eligible=sum(indel_model.eligible(b, ANCHOR) for b in m.bubbles))
    return m._judged
