"""A small text and reads whose EXACT-TAIL interval lists have every length that matters to kl_search (bwb_lane.h: list_add<P, true> stores only
the displaced tails that land in slots >= 1; a list's first interval and its tail travel in registers): built with tests/ovf_model.py,
checked on the CPU by tests/test_tail_lists_host.py, run on the GPU by tests/test_gpu_tail_lists.py.

  * de Bruijn records over two and three letters compatible with one base, each followed by a plain stretch: a read that starts with a run
    of that base and goes on into the stretch walks lists of 2, 4, 8, 16 (3, 9, 27) intervals, which then collapse to one - and it has a hit;
  * families (ovf_model.family): k variants of a read in the text give that read a list that grows, step by step, to one interval per
    distinct variant: the final lists of 1 .. 9 and of 13 and more intervals, and most lengths in between on the way;
  * the same reads with one substitution, with a deletion, with an insertion: the tails that start from popped entries (-n 1, -n 2), gapped
    ones among them (the hit loop that looks for duplicates)."""
import ovf_model as om

READ_LEN = 40
SEED = 5
FAMILY_COPIES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 20, 24)  # variants of the family's read in the text
# (two variants that follow each other in the index merge into one interval: some families end a little below their size, so a few more)
MORE_FAMILIES = (("g6", 206, 6), ("g7", 207, 7), ("g13", 213, 13))
ORDINARY = 1600
PRECALC = 12  # -P: the heap starts from the list of the read's first twelve bases (bwb_lane.h: PRECALC_LEN)
# -n 0: the whole search is one tail from the root; -n 1 / -n 2: tails from popped entries (one gap open by default), two gap opens: more gapped
# entries at the hits; -P: the seeding path; -S: the single-genome alphabet
FLAG_SETS = (("-n", "0"), ("-n", "1"), ("-n", "2"), ("-n", "2", "-o", "2", "-e", "2"), ("-P", "-n", "0"), ("-P", "-n", "2"), ("-S", "-n", "1"))
STRETCH = READ_LEN
# (letters compatible with the run's base; the stretch that follows starts with a base none of them is compatible with)
RUNS = (("dbA2", "A", "AR", 5, "T"), ("dbC3", "C", "CYS", 4, "A"))


class TailFixture:
    def __init__(self):
        rng = om.Lcg(SEED)
        self.records = [("ordinary", rng.bases(ORDINARY))]
        self.reads = {}
        self.families, self.runs, self.plain = [], [], []
        for name, base, letters, order, stop in RUNS:
            stretch = stop + rng.bases(STRETCH - 1)
            db = om.de_bruijn(letters, order)
            self.records.append((name, db + stretch))
            # (a run of the base meets the record's k-mers over `letters`; only the one in front of the stretch goes on: a single hit)
            for run in range(2, order + 1):
                n = f"{name}_r{run}"
                self.reads[n] = (base * run + stretch)[:READ_LEN]
                self.runs.append(n)
        for n, seed, k in tuple((f"f{k}", 100 + k, k) for k in FAMILY_COPIES) + MORE_FAMILIES:
            read, rec = om.family(seed, READ_LEN, k)
            self.records.append((n, rec))
            self.reads[n] = read
            self.reads[n + "_rc"] = om.revcomp(read)
            self.families += [n, n + "_rc"]
        ordn = self.records[0][1]
        for j in range(12):
            o = rng.below(len(ordn) - READ_LEN)
            n = f"p{j}"
            self.reads[n] = ordn[o:o + READ_LEN] if j % 2 == 0 else om.revcomp(ordn[o:o + READ_LEN])
            self.plain.append(n)
        # one difference, at the far end / in the middle / near the start of the search (which walks the read from its first base)
        self.edited = []
        for src in [f"f{k}" for k in FAMILY_COPIES] + ["f9_rc", "f16_rc", "p0", "p1", "dbA2_r5", "dbC3_r4"]:
            r = self.reads[src]
            for tag, kw in (("s8", dict(subs=(8,))), ("s20", dict(subs=(20,))), ("s33", dict(subs=(33,))),
                            ("d25", dict(dels=(25,))), ("i14", dict(ins=(14,))), ("s12s30", dict(subs=(12, 30)))):
                n = f"{src}_{tag}"
                self.reads[n] = om._edit(r, **kw)
                self.edited.append(n)
        self.names = list(self.reads)
        assert len(self.names) <= 256

    def fasta(self):
        return "".join(f">{n}\n{s}\n" for n, s in self.records)

    def text(self):
        return om.Text(self.records)
