/*
 * indel.c - `-I <indels.tsv>`: ref / alt read support per indel bubble (no counterpart in the reference).
 *
 * The rule is in include/bwbble_hip.h (bwb_hip_indel_begin) and restated here: bubble b = (A, Bm, C, Dm, ref_len, alt_len), gap = C - A - Bm,
 * anchor w.  b is ELIGIBLE when lift_bubble_refusal(b) is NULL, Bm >= w, Dm + 1 >= w and A + Bm - w >= 1.  Its window on its own record is
 * [Bm - w + 1, Bm + alt_len + w], on the chromosome's record [A + Bm - w, C + w - 1], both in the 1-based coordinates bwb_locus.pos1 has.  A
 * mapped primary in a record, whose printed ops consume the read and whose MAPQ (the join record's when there is one) reaches min_mapq, is
 * classed against a window by walking its printed CIGAR with x from pos1 (M and D consume x, I does not): COVERING when lo and hi are each
 * consumed by an M, CLEAN when also every x of the window is an M's and no I lies between the two, else GAPPED.  A read on b's record adds to
 * alt / alt_gapped of b; a read on a chromosome record c to ref / ref_gapped of every eligible bubble with chrom_of == c.
 * `map` sums the counts on the GPU (kernel k_indel) and fetches them when the stream ends; indel_host is the same rule on the host (aln2sam,
 * places2sam, and map on an .ann that is not ascending and disjoint).  The table lives here either way: n x (ref, alt, ref_gapped, alt_gapped)
 * uint32 counters that wrap.  The eligible bubbles are sorted by (chrom_of, A + Bm - w, bubble number) with qsort, so that a chromosome read
 * finds its candidates by bisection: those whose lo lies within its first and last M.
 * The file is opened before anything is loaded, so that a path that cannot be written stops the run there; a run that ends through bwb_die
 * (exit) before indel_write has finished leaves no file behind.
 */
#define _GNU_SOURCE
#include <string.h>
#include <time.h>
#include "bwb_host.h"

static char *indel_unfinished; /* the file of a run that has not written it yet: removed at exit */
static void indel_at_exit(void) { if (indel_unfinished) remove(indel_unfinished); }

indel_t *indel_open(const char *indelFname, int min_mapq, int anchor) {
	indel_t *p = (indel_t *)calloc(1, sizeof(*p));
	p->min_mapq = min_mapq;
	p->anchor = anchor;
	if (indelFname) {
		p->fname = strdup(indelFname);
		p->f = fopen(indelFname, "w");
		if (!p->f) { perror(indelFname); bwb_die("-I: Cannot open the indel support file: %s!", indelFname); }
		static int registered;
		if (!registered) { atexit(indel_at_exit); registered = 1; }
		indel_unfinished = p->fname;
	}
	return p;
}

int indel_eligible(const bwb_bubble *b, int anchor) {
	if (lift_bubble_refusal(b)) return 0;
	return b->B_minus_A >= anchor && b->D_minus_C + 1 >= anchor && (int64_t)((uint64_t)b->A + (uint64_t)b->B_minus_A - (uint64_t)anchor) >= 1;
}

static int indel_entry_cmp(const void *a, const void *b) {
	const indel_entry_t *x = (const indel_entry_t *)a, *y = (const indel_entry_t *)b;
	if (x->chrom != y->chrom) return x->chrom < y->chrom ? -1 : 1;
	if (x->lo != y->lo) return x->lo < y->lo ? -1 : 1;
	return x->bubble < y->bubble ? -1 : x->bubble > y->bubble;
}

/* the eligible bubbles of the table, sorted, and the zeroed counters */
void indel_set_table(indel_t *p, const bubble_table_t *t, const int32_t *chrom_of) {
	p->bub = t;
	p->elig = (uint8_t *)calloc(t->n > 0 ? (size_t)t->n : 1, 1);
	p->tab = (indel_entry_t *)malloc((t->n > 0 ? (size_t)t->n : 1) * sizeof(indel_entry_t));
	p->n_tab = 0;
	for (int64_t k = 0; k < t->n; k++) {
		if (lift_bubble_refusal(&t->b[k])) { p->n_refused++; continue; }
		if (!indel_eligible(&t->b[k], p->anchor)) continue;
		p->elig[k] = 1;
		p->tab[p->n_tab++] = (indel_entry_t){ (int64_t)((uint64_t)t->b[k].A + (uint64_t)t->b[k].B_minus_A - (uint64_t)p->anchor), chrom_of[k], (uint32_t)k };
	}
	struct timespec t0, t1;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	qsort(p->tab, (size_t)p->n_tab, sizeof(indel_entry_t), indel_entry_cmp);
	clock_gettime(CLOCK_MONOTONIC, &t1);
	p->sort_s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
	p->counts = (uint32_t *)calloc(t->n > 0 ? (size_t)t->n * 4 : 1, sizeof(uint32_t));
	if (!p->counts) bwb_die("-I: no memory for the counters of %lld bubbles", (long long)t->n);
}

/* the class of one placement against the window lo .. hi (lo < hi): 0 not covering, 1 clean, 2 gapped */
unsigned indel_resolve(int64_t pos1, int reverse, unsigned alen, const uint16_t *gap_run, int64_t lo, int64_t hi) {
	int64_t x = pos1;
	int at_lo = 0, at_hi = 0, dirty = 0;
	for (unsigned t = 0; t < alen && x <= hi; t++) {
		const unsigned op = lift_op_at(gap_run, alen, reverse, t);
		if (op == BWB_LIFT_I) { if (at_lo) dirty = 1; continue; } /* (the M at hi ends the walk) */
		if (x >= lo) {
			if (op == BWB_LIFT_M) { if (x == lo) at_lo = 1; if (x == hi) at_hi = 1; }
			else dirty = 1;
		}
		x++;
	}
	return at_lo && at_hi ? (dirty ? 2u : 1u) : 0u;
}

/* The rule on a set of reads (len NULL: no read lengths to compare; joins NULL: MAPQ is the placement's).  Adds into the table with all cores
 * (the adds commute); returns the reads counted. */
uint64_t indel_host(indel_t *p, const bwb_place *pl, const bwb_locus *loci, size_t n, const uint16_t *len, const bwb_join *joins) {
	const int64_t w = p->anchor;
	uint64_t reads = 0, adds = 0, cands = 0;
#pragma omp parallel for schedule(static) reduction(+ : reads, adds, cands) num_threads(bwb_host_team())
	for (long r = 0; r < (long)n; r++) {
		if (!(pl[r].flags & BWB_PLACE_MAPPED) || loci[r].seqid < 0) continue;
		if ((int)(joins ? joins[r].mapq : pl[r].mapq) < p->min_mapq) continue;
		const int reverse = (pl[r].flags & BWB_PLACE_REVERSE) != 0;
		const unsigned alen = pl[r].aln_length;
		const int64_t pos1 = loci[r].pos1;
		int64_t x = pos1, xf = 0, xl = -1;
		unsigned on_read = 0;
		int any = 0;
		for (unsigned t = 0; t < alen; t++) {
			const unsigned op = lift_op_at(pl[r].gap_run, alen, reverse, t);
			on_read += op != BWB_LIFT_D;
			if (op == BWB_LIFT_I) continue;
			if (op == BWB_LIFT_M) { if (!any) { xf = x; any = 1; } xl = x; }
			x++;
		}
		if (len && on_read != len[r]) continue;
		reads++;
		const int32_t b = loci[r].bubble;
		if (b >= 0) {
			if (!p->elig[b]) continue;
			const bwb_bubble *e = &p->bub->b[b];
			cands++;
			const unsigned cls = indel_resolve(pos1, reverse, alen, pl[r].gap_run, e->B_minus_A - w + 1, e->B_minus_A + e->alt_len + w);
			if (cls) {
				uint32_t *dst = p->counts + (size_t)b * 4 + (cls == 1 ? 1 : 3);
#pragma omp atomic
				*dst += 1u;
				adds++;
			}
			continue;
		}
		if (!any) continue;
		const int32_t c = loci[r].seqid;
		uint64_t at = 0, len2 = p->n_tab; /* the first entry not below (c, xf) */
		while (len2) {
			const uint64_t half = len2 >> 1;
			const indel_entry_t *k = &p->tab[at + half];
			if (k->chrom < c || (k->chrom == c && k->lo < xf)) { at += half + 1; len2 -= half + 1; } else len2 = half;
		}
		for (; at < p->n_tab; at++) {
			const indel_entry_t *k = &p->tab[at];
			if (k->chrom != c || k->lo > xl) break;
			cands++;
			const int64_t hi = (int64_t)((uint64_t)p->bub->b[k->bubble].C + (uint64_t)w - 1u);
			if (hi > xl) continue;
			const unsigned cls = indel_resolve(pos1, reverse, alen, pl[r].gap_run, k->lo, hi);
			if (cls) {
				uint32_t *dst = p->counts + (size_t)k->bubble * 4 + (cls == 1 ? 0 : 2);
#pragma omp atomic
				*dst += 1u;
				adds++;
			}
		}
	}
	p->reads += reads; p->adds += adds; p->cands += cands;
	return reads;
}

/* a worker's counters of the bubbles first .. first + n - 1 (bwb_hip_indel_counts), added into the table */
void indel_add(indel_t *p, uint64_t first, uint64_t n, const uint32_t *counts) {
	uint32_t *dst = p->counts + first * 4;
	for (uint64_t k = 0; k < n * 4; k++) dst[k] += counts[k];
}

/* `#bubble<TAB>chrom<TAB>pos<TAB>ref_len<TAB>alt_len<TAB>ref<TAB>alt<TAB>ref_gapped<TAB>alt_gapped`, then one line per bubble with a counter that
 * is not zero, in bubble-number order: the bubble's number, the first word of its header line in bubble.data, A + Bm, the two lengths and the
 * four counts.  Returns the lines written; the file is complete and closed after this. */
uint64_t indel_write(indel_t *p) {
	const bubble_table_t *t = p->bub;
	fprintf(p->f, "#bubble\tchrom\tpos\tref_len\talt_len\tref\talt\tref_gapped\talt_gapped\n");
	uint64_t written = 0;
	for (int64_t k = 0; k < t->n; k++) {
		const uint32_t *v = p->counts + (size_t)k * 4;
		if (!(v[0] | v[1] | v[2] | v[3])) continue;
		const bwb_bubble *b = &t->b[k];
		fprintf(p->f, "%lld\t%.*s\t%lld\t%d\t%d\t%u\t%u\t%u\t%u\n", (long long)k, (int)strcspn(t->ann[k], " \t"), t->ann[k],
		        (long long)((uint64_t)b->A + (uint64_t)b->B_minus_A), b->ref_len, b->alt_len, v[0], v[1], v[2], v[3]);
		written++;
	}
	if (fflush(p->f) || ferror(p->f) || fclose(p->f)) bwb_die("-I: Cannot write to the indel support file: %s!", p->fname);
	p->f = NULL;
	indel_unfinished = NULL;
	return written;
}

void indel_free(indel_t *p) {
	if (!p) return;
	if (p->f) fclose(p->f);
	if (p->fname && indel_unfinished == p->fname) { remove(p->fname); indel_unfinished = NULL; }
	free(p->fname); free(p->elig); free(p->tab); free(p->counts); free(p);
}
