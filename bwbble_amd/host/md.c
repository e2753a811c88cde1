/*
 * md.c - `-D`: NM:i and MD:Z of a read's line against the text the index was built from (no counterpart in the reference).
 *
 * The text is <seq_fasta>.ref as fasta2ref writes it (index.c): one code per byte, the forward text of n_fwd characters - the first number of
 * the .ann file - and then its reverse complement.  It holds IUPAC codes, and a read base that is a MEMBER of a code is a match, as in the
 * search; so no stock tool can add the two tags afterwards.  md_resolve is the rule of include/bwbble_hip.h (bwb_md) on one read - what the
 * kernels k_md_count / k_md compute -, md_place_ops turns a placement's printed CIGAR into the ops it walks, md_host runs it over a set of
 * reads the way bwb_hip_slot_md lays the result out (aln2sam, places2sam, and map on an .ann that is not ascending and disjoint).
 */
#define _GNU_SOURCE
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include "bwb_host.h"

static double md_wall(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

/* reads the forward half into t->codes and publishes it (also the job `map` gives the .bwt loader, behind the sampled SA) */
void md_text_read(void *text) {
	md_text_t *t = (md_text_t *)text;
	const double t0 = md_wall();
	FILE *f = fopen(t->refFname, "rb");
	if (!f) { perror(t->refFname); bwb_die("%s: Cannot open the text: %s (`bwbble fasta2ref <seq_fasta>` writes it)", t->flag, t->refFname); }
	if (fread(t->codes, 1, t->n_fwd, f) != t->n_fwd) bwb_die("%s: %s ends before its %llu forward characters", t->flag, t->refFname, (unsigned long long)t->n_fwd);
	fclose(f);
	t->seconds = md_wall() - t0;
	__atomic_store_n(&t->ready, 1, __ATOMIC_RELEASE);
}

/* the forward half of <fastaFname>.ref.  Checked before anything is read: the file is there and holds 2 x n_fwd bytes */
md_text_t *md_text_open(const char *fastaFname, int deferred) { return md_text_open_for(fastaFname, deferred, "-D"); }

/* flag: the option that asks for the text, for the messages (-D, or -A without it) */
md_text_t *md_text_open_for(const char *fastaFname, int deferred, const char *flag) {
	const size_t L = strlen(fastaFname) + 8;
	char *annFname = (char *)malloc(L), *refFname = (char *)malloc(L);
	snprintf(annFname, L, "%s.ann", fastaFname);
	snprintf(refFname, L, "%s.ref", fastaFname);
	FILE *af = fopen(annFname, "r");
	unsigned long long n_fwd = 0;
	if (!af || fscanf(af, "%llu", &n_fwd) != 1 || !n_fwd) bwb_die("%s: Cannot read the text length from %s", flag, annFname);
	fclose(af);
	struct stat st;
	if (stat(refFname, &st) != 0) bwb_die("%s needs the text %s: it is missing (`bwbble fasta2ref %s` writes it)", flag, refFname, fastaFname);
	if ((unsigned long long)st.st_size != 2 * n_fwd)
		bwb_die("%s needs the text %s: it holds %lld bytes, not 2 x %llu as %s says (`bwbble fasta2ref %s` writes it)", flag, refFname, (long long)st.st_size, n_fwd, annFname, fastaFname);
	md_text_t *t = (md_text_t *)calloc(1, sizeof(*t));
	t->n_fwd = n_fwd;
	t->refFname = refFname;
	t->flag = flag;
	t->codes = (uint8_t *)malloc(n_fwd);
	if (!t->codes) bwb_die("%s: no memory for the %llu characters of %s", flag, n_fwd, refFname);
	free(annFname);
	if (!deferred) md_text_read(t);
	return t;
}

/* (every GPU worker of `map` waits for the one text, the way it waits for the sampled SA) */
void md_text_wait(md_text_t *t) {
	if (!t) return;
	while (!__atomic_load_n(&t->ready, __ATOMIC_ACQUIRE)) { struct timespec ts = { 0, 200000 }; nanosleep(&ts, NULL); }
}

void md_text_free(md_text_t *t) {
	if (!t) return;
	free(t->codes); free(t->refFname); free(t);
}

/* the printed CIGAR of a placement (sam_put_cigar) as ops of a lift record, neighbours merged: at most 17 */
unsigned md_place_ops(unsigned alen, const uint16_t *gap_run, int reverse, uint32_t *ops) {
	unsigned n = 0;
	for (unsigned t = 0; t < alen; t++) {
		const unsigned op = lift_op_at(gap_run, alen, reverse, t);
		if (n && (ops[n - 1] & 15u) == op) ops[n - 1] += 1u << 4;
		else if (n < 2 * BWB_MAX_GAP_RUNS + 1) ops[n++] = (1u << 4) | op;
		else return 0; /* (more runs than eight gap runs can make: not reached) */
	}
	return n;
}

typedef struct { char *md; size_t cap, n; } md_out_t;
static inline void md_put(md_out_t *o, char ch) { if (o->md && o->n < o->cap) o->md[o->n] = ch; o->n++; }
static inline void md_number(md_out_t *o, unsigned v) {
	char d[12];
	const int k = snprintf(d, sizeof(d), "%u", v);
	for (int i = 0; i < k; i++) md_put(o, d[i]);
}
/* io.h:29,109: bit j = code j is a member of read base c (A0 G1 C2 T3), as the kernels' member_mask */
static const uint32_t md_member[4] = { 0xFB00u, 0x383Cu, 0x0BF0u, 0x6266u };

/* The rule on one read: seq / len as uploaded (read->seq codes), the strand, the ops (len << 4 | op) from text position start.  Fills rec;
 * with md, writes at most cap bytes of the MD text (rec->md_len is the exact length either way).  Returns the kind. */
int md_resolve(const uint8_t *text, uint64_t n_fwd, const uint8_t *seq, unsigned len, int reverse, int64_t start, const uint32_t *ops, unsigned n_ops, bwb_md *rec, char *md, size_t cap) {
	memset(rec, 0, sizeof(*rec));
	uint64_t span = 0, on_read = 0;
	for (unsigned i = 0; i < n_ops; i++) {
		const unsigned op = ops[i] & 15u;
		if (op == BWB_LIFT_M || op == BWB_LIFT_D) span += ops[i] >> 4;
		if (op != BWB_LIFT_D) on_read += ops[i] >> 4;
	}
	if (span > BWB_MD_MAX_SPAN) { rec->kind = BWB_MD_TOO_LONG; return BWB_MD_TOO_LONG; }
	if (start < 0 || (uint64_t)start > n_fwd || span > n_fwd - (uint64_t)start || on_read != len) return BWB_MD_NONE;
	md_out_t o = { .md = md, .cap = cap, .n = 0 };
	unsigned ri = 0, run = 0, mm = 0, gaps = 0, in_del = 0;
	uint64_t tp = (uint64_t)start;
	for (unsigned i = 0; i < n_ops; i++) {
		const unsigned op = ops[i] & 15u, count = ops[i] >> 4;
		if (op == BWB_LIFT_M) {
			for (unsigned k = 0; k < count; k++, ri++, tp++) {
				const unsigned raw = reverse ? seq[len - 1 - ri] : seq[ri];
				const unsigned b = reverse ? (raw > 3 ? 4u : 3u - raw) : raw; /* read->rc */
				const unsigned c = text[tp] & 15u;
				if (b < 4 && ((md_member[b] >> c) & 1u)) run++;
				else { md_number(&o, run); md_put(&o, "NTKGSBYCMHNVRDWA"[c]); run = 0; mm++; }
			}
		} else if (op == BWB_LIFT_D) {
			if (!in_del) { md_number(&o, run); md_put(&o, '^'); run = 0; }
			for (unsigned k = 0; k < count; k++, tp++) md_put(&o, "NTKGSBYCMHNVRDWA"[text[tp] & 15u]);
			gaps += count;
		} else {
			ri += count;
			if (op == BWB_LIFT_I) gaps += count;
		}
		in_del = op == BWB_LIFT_D;
	}
	md_number(&o, run);
	rec->nm = mm + gaps;
	rec->md_len = (uint16_t)o.n;
	rec->kind = BWB_MD_OK;
	return BWB_MD_OK;
}

/* -D on the host: the md records of n reads laid out as bwb_hip_slot_md returns them (lift_kind NULL: no read is lifted); with all cores */
md_set_t *md_host(const bwb_place *pl, size_t n, const uint8_t *seq, uint32_t stride, const uint16_t *len, const uint8_t *lift_kind, const uint64_t *lift_off,
                  const bwb_lift *lift_recs, const fasta_annotations_t *ann, const md_text_t *t) {
	md_set_t *ms = (md_set_t *)calloc(1, sizeof(*ms));
	ms->recs = (bwb_md *)calloc(n ? n : 1, sizeof(bwb_md));
	ms->off = (uint64_t *)calloc(n + 1, 8);
	for (int pass = 0; pass < 2; pass++) {
		uint64_t ok = 0, too_long = 0;
#pragma omp parallel for schedule(static) reduction(+ : ok, too_long) num_threads(bwb_host_team())
		for (long r = 0; r < (long)n; r++) {
			if (pass && ms->recs[r].kind != BWB_MD_OK) continue;
			if (!(pl[r].flags & BWB_PLACE_MAPPED)) continue;
			uint32_t own[2 * BWB_MAX_GAP_RUNS + 1];
			const uint32_t *ops = own;
			unsigned n_ops;
			int64_t start = (int64_t)pl[r].pos;
			if (lift_kind && lift_kind[r] == BWB_LIFT_LIFTED) {
				const bwb_lift *rec = lift_recs + lift_off[r];
				if (rec->seqid < 0 || rec->seqid >= ann->num_seq) continue;
				ops = (const uint32_t *)(rec + 1); n_ops = rec->n_ops;
				start = (int64_t)(ann->seq_anns[rec->seqid].start_index + (uint64_t)rec->pos - 1u);
			} else n_ops = md_place_ops(pl[r].aln_length, pl[r].gap_run, (pl[r].flags & BWB_PLACE_REVERSE) != 0, own);
			bwb_md rec;
			const int kind = md_resolve(t->codes, t->n_fwd, seq + (size_t)r * stride, len[r], (pl[r].flags & BWB_PLACE_REVERSE) != 0, start, ops, n_ops, &rec,
			                            pass ? ms->text + ms->off[r] : NULL, pass ? (size_t)(ms->off[r + 1] - ms->off[r]) : 0);
			if (!pass) {
				ms->recs[r] = rec;
				ms->off[r + 1] = rec.md_len;
				ok += kind == BWB_MD_OK; too_long += kind == BWB_MD_TOO_LONG;
			}
		}
		if (!pass) {
			ms->n_ok = ok; ms->n_too_long = too_long;
			for (size_t r = 0; r < n; r++) ms->off[r + 1] += ms->off[r];
			ms->text = (char *)malloc(ms->off[n] ? (size_t)ms->off[n] : 1);
		}
	}
	return ms;
}

void md_free(md_set_t *ms) {
	if (!ms) return;
	free(ms->recs); free(ms->off); free(ms->text); free(ms);
}
