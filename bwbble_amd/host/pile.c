/*
 * pile.c - `-A <counts.tsv>`: allele counts at the text's IUPAC sites (no counterpart in the reference).
 *
 * A site is a position of the forward text whose code has two or three members; the rule is in include/bwbble_hip.h (bwb_hip_pile_begin).
 * `map` sums the counts on the GPU (kernel k_pile) and fetches them when the stream ends; pile_host is the same rule on the host over a set of
 * reads laid out the way md_host takes them (aln2sam, places2sam, and map with the host's lift or join records).  The table lives here either
 * way: n_sites x (A, C, G, T) uint32 counters that wrap, sites numbered in text order.  pile_write enumerates the sites by scanning the text's
 * bytes - no site list travels from the device - and writes one line per site with a counter that is not zero.
 * -b / -Y (include/bwbble_hip.h: bwb_hip_pileq_begin): min_baseq drops the bases below it, and with err_cap a second table of the same shape,
 * qsum, takes min(max(Q, 4), err_cap) for every base counted; the qualities are the FASTQ's lines, byte i under read base i.
 * The counts file is opened before anything is loaded, so that a path that cannot be written stops the run there; a run that ends through
 * bwb_die (exit) before pile_write has finished leaves no counts file behind.
 */
#define _GNU_SOURCE
#include <string.h>
#include "bwb_host.h"

#define PILE_SITE_CODES 0x7B74u /* bit c: code c is K 2, S 4, B 5, Y 6, M 8, H 9, V 11, R 12, D 13 or W 14 */

static char *pile_unfinished; /* the counts file of a run that has not written it yet: removed at exit */
static void pile_at_exit(void) { if (pile_unfinished) remove(pile_unfinished); }

pile_t *pile_open(const char *countsFname, int min_mapq) {
	pile_t *p = (pile_t *)calloc(1, sizeof(*p));
	p->min_mapq = min_mapq;
	if (countsFname) {
		p->fname = strdup(countsFname);
		p->f = fopen(countsFname, "w");
		if (!p->f) { perror(countsFname); bwb_die("-A: Cannot open the counts file: %s!", countsFname); }
		static int registered;
		if (!registered) { atexit(pile_at_exit); registered = 1; }
		pile_unfinished = p->fname;
	}
	return p;
}

/* the text is in memory: counts its sites, makes the zeroed table and - index != 0, for pile_host - the sites below every 32 characters */
void pile_set_text(pile_t *p, const md_text_t *t, int index) {
	p->text = t;
	const uint64_t n_words = (t->n_fwd + 31) / 32;
	if (index) p->base = (uint32_t *)malloc((n_words ? n_words : 1) * sizeof(uint32_t));
	uint64_t n = 0;
	uint32_t *base = p->base;
#pragma omp parallel for schedule(static) reduction(+ : n) num_threads(bwb_host_team())
	for (long w = 0; w < (long)n_words; w++) {
		const uint64_t e = ((uint64_t)w + 1) * 32 < t->n_fwd ? ((uint64_t)w + 1) * 32 : t->n_fwd;
		uint32_t k = 0;
		for (uint64_t i = (uint64_t)w * 32; i < e; i++) k += (PILE_SITE_CODES >> (t->codes[i] & 15u)) & 1u;
		if (base) base[w] = k;
		n += k;
	}
	if (base && n <= 0xFFFFFFFFull) { /* the words' counts -> the sites below every word */
		uint32_t below = 0;
		for (uint64_t w = 0; w < n_words; w++) { const uint32_t k = base[w]; base[w] = below; below += k; }
	}
	if (n > 0xFFFFFFFFull) bwb_die("-A: the text has %llu IUPAC sites, more than 2^32 - 1", (unsigned long long)n);
	p->n_sites = n;
	p->counts = (uint32_t *)calloc(n ? (size_t)n * 4 : 1, sizeof(uint32_t));
	if (p->err_cap) p->qsum = (uint32_t *)calloc(n ? (size_t)n * 4 : 1, sizeof(uint32_t)); /* -Y */
	if (!p->counts || (p->err_cap && !p->qsum)) bwb_die("-A: no memory for the counters of %llu sites", (unsigned long long)n);
}

/* the site number of a site's position (pile_host; needs the index of pile_set_text) */
static inline uint64_t pile_site(const pile_t *p, uint64_t i) {
	uint64_t s = p->base[i >> 5];
	for (uint64_t k = i & ~(uint64_t)31; k < i; k++) s += (PILE_SITE_CODES >> (p->text->codes[k] & 15u)) & 1u;
	return s;
}

/* The rule on a set of reads, laid out as for md_host; joins NULL: MAPQ is the placement's; read r's quality line is qtext + qual_off[r] (only
 * read with -b above 0 or -Y).  Adds into the table with all cores (the adds commute); returns the reads counted and adds the adds to p->adds,
 * the bases -b dropped to p->dropped. */
uint64_t pile_host_q(pile_t *p, const bwb_place *pl, size_t n, const uint8_t *seq, uint32_t stride, const uint16_t *len, const char *qtext, const size_t *qual_off,
                     const uint8_t *lift_kind, const uint64_t *lift_off, const bwb_lift *lift_recs, const bwb_join *joins, const fasta_annotations_t *ann) {
	const unsigned min_baseq = (unsigned)p->min_baseq, err_cap = (unsigned)p->err_cap;
	const int with_q = min_baseq || err_cap;
	if (with_q && !(qtext && qual_off)) bwb_die("-b / -Y: the reads carry no qualities");
	uint64_t dropped = 0;
	const uint8_t *text = p->text->codes;
	const uint64_t n_fwd = p->text->n_fwd;
	uint64_t reads = 0, adds = 0;
#pragma omp parallel for schedule(static) reduction(+ : reads, adds, dropped) num_threads(bwb_host_team())
	for (long r = 0; r < (long)n; r++) {
		if (!(pl[r].flags & BWB_PLACE_MAPPED) || len[r] > 255 || len[r] > stride) continue;
		if ((int)(joins ? joins[r].mapq : pl[r].mapq) < p->min_mapq) continue;
		const int reverse = (pl[r].flags & BWB_PLACE_REVERSE) != 0;
		uint32_t own[2 * BWB_MAX_GAP_RUNS + 1];
		const uint32_t *ops = own;
		unsigned n_ops;
		int64_t start = (int64_t)pl[r].pos;
		if (lift_kind && lift_kind[r] == BWB_LIFT_LIFTED) {
			const bwb_lift *rec = lift_recs + lift_off[r];
			if (rec->seqid < 0 || rec->seqid >= ann->num_seq) continue;
			ops = (const uint32_t *)(rec + 1); n_ops = rec->n_ops;
			start = (int64_t)(ann->seq_anns[rec->seqid].start_index + (uint64_t)rec->pos - 1u);
		} else n_ops = md_place_ops(pl[r].aln_length, pl[r].gap_run, reverse, own);
		uint64_t span = 0, on_read = 0;
		for (unsigned i = 0; i < n_ops; i++) {
			const unsigned op = ops[i] & 15u;
			if (op == BWB_LIFT_M || op == BWB_LIFT_D) span += ops[i] >> 4;
			if (op != BWB_LIFT_D) on_read += ops[i] >> 4;
		}
		if (span > BWB_MD_MAX_SPAN || start < 0 || (uint64_t)start > n_fwd || span > n_fwd - (uint64_t)start || on_read != len[r]) continue;
		const uint8_t *s = seq + (size_t)r * stride;
		const uint8_t *ql = with_q ? (const uint8_t *)qtext + qual_off[r] : NULL;
		unsigned ri = 0;
		uint64_t tp = (uint64_t)start;
		for (unsigned i = 0; i < n_ops; i++) {
			const unsigned op = ops[i] & 15u, count = ops[i] >> 4;
			if (op == BWB_LIFT_M) {
				for (unsigned k = 0; k < count; k++, ri++, tp++) {
					if (!((PILE_SITE_CODES >> (text[tp] & 15u)) & 1u)) continue;
					const unsigned idx = reverse ? len[r] - 1u - ri : ri;
					const unsigned raw = s[idx];
					if (raw > 3) continue; /* a read N */
					unsigned Q = 0;
					if (with_q) {
						Q = ql[idx] < 33 ? 0u : (ql[idx] - 33u > 93u ? 93u : ql[idx] - 33u);
						if (Q < min_baseq) { dropped++; continue; }
					}
					const unsigned b = reverse ? 3u - raw : raw; /* A0 G1 C2 T3 as SAM prints it */
					const unsigned col = (b == 1 || b == 2) ? 3u - b : b; /* A C G T */
					uint32_t *dst = p->counts + pile_site(p, tp) * 4 + col;
#pragma omp atomic
					*dst += 1u;
					if (err_cap) {
						uint32_t *qd = p->qsum + (dst - p->counts);
						const uint32_t q = Q < 4 ? 4u : Q > err_cap ? err_cap : Q;
#pragma omp atomic
						*qd += q;
					}
					adds++;
				}
			} else if (op == BWB_LIFT_D) tp += count;
			else ri += count;
		}
		reads++;
	}
	p->reads += reads; p->adds += adds; p->dropped += dropped;
	return reads;
}

/* the rule without qualities (a table without -b and -Y) */
uint64_t pile_host(pile_t *p, const bwb_place *pl, size_t n, const uint8_t *seq, uint32_t stride, const uint16_t *len, const uint8_t *lift_kind, const uint64_t *lift_off,
                   const bwb_lift *lift_recs, const bwb_join *joins, const fasta_annotations_t *ann) {
	return pile_host_q(p, pl, n, seq, stride, len, NULL, NULL, lift_kind, lift_off, lift_recs, joins, ann);
}

/* a worker's counters of the sites first .. first + n - 1 (bwb_hip_pile_counts), added into the table */
void pile_add(pile_t *p, uint64_t first, uint64_t n, const uint32_t *counts) {
	uint32_t *dst = p->counts + first * 4;
	for (uint64_t k = 0; k < n * 4; k++) dst[k] += counts[k];
}

/* a worker's quality sums of the same sites (bwb_hip_pileq_sums) */
void pile_add_q(pile_t *p, uint64_t first, uint64_t n, const uint32_t *sums) {
	uint32_t *dst = p->qsum + first * 4;
	for (uint64_t k = 0; k < n * 4; k++) dst[k] += sums[k];
}

typedef struct { uint64_t start; int rec; } pile_rec_t;
static int pile_rec_cmp(const void *a, const void *b) {
	const pile_rec_t *x = (const pile_rec_t *)a, *y = (const pile_rec_t *)b;
	return x->start < y->start ? -1 : x->start > y->start ? 1 : x->rec - y->rec;
}

/* `#record<TAB>pos<TAB>code<TAB>A<TAB>C<TAB>G<TAB>T`, then one line per site with a counter that is not zero, in text order: the first word of
 * the .ann record's name, the 1-based position in the record, the text's letter and the four counts.  A site in no record is left out.
 * Returns the sites written; the file is complete and closed after this. */
uint64_t pile_write(pile_t *p, const fasta_annotations_t *ann) {
	const md_text_t *t = p->text;
	/* the records by their first position (an .ann need not ascend) */
	pile_rec_t *order = (pile_rec_t *)malloc((ann->num_seq > 0 ? (size_t)ann->num_seq : 1) * sizeof(pile_rec_t));
	for (int i = 0; i < ann->num_seq; i++) order[i] = (pile_rec_t){ ann->seq_anns[i].start_index, i };
	qsort(order, (size_t)ann->num_seq, sizeof(pile_rec_t), pile_rec_cmp);
	fprintf(p->f, "#record\tpos\tcode\tA\tC\tG\tT\n");
	uint64_t site = 0, written = 0;
	int at = 0; /* the first record in `order` that does not end below i */
	for (uint64_t i = 0; i < t->n_fwd; i++) {
		const unsigned c = t->codes[i] & 15u;
		if (!((PILE_SITE_CODES >> c) & 1u)) continue;
		const uint32_t *v = p->counts + site * 4;
		site++;
		if (!(v[0] | v[1] | v[2] | v[3])) continue;
		while (at < ann->num_seq && ann->seq_anns[order[at].rec].end_index < i) at++;
		if (at >= ann->num_seq || ann->seq_anns[order[at].rec].start_index > i) continue;
		const seq_annotation_t *a = &ann->seq_anns[order[at].rec];
		fprintf(p->f, "%.*s\t%llu\t%c\t%u\t%u\t%u\t%u\n", (int)strcspn(a->name, " \t"), a->name, (unsigned long long)(i - a->start_index + 1), "NTKGSBYCMHNVRDWA"[c], v[0], v[1], v[2], v[3]);
		written++;
	}
	if (site != p->n_sites) bwb_die("-A: the text has %llu sites, %llu were counted before", (unsigned long long)site, (unsigned long long)p->n_sites);
	free(order);
	if (fflush(p->f) || ferror(p->f) || fclose(p->f)) bwb_die("-A: Cannot write to the counts file: %s!", p->fname);
	p->f = NULL;
	pile_unfinished = NULL;
	return written;
}

void pile_free(pile_t *p) {
	if (!p) return;
	if (p->f) fclose(p->f);
	if (p->fname && pile_unfinished == p->fname) { remove(p->fname); pile_unfinished = NULL; }
	free(p->fname); free(p->base); free(p->counts); free(p->qsum); free(p);
}
