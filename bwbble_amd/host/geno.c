/*
 * geno.c - `-G <calls.tsv>`: genotype calls at the text's IUPAC sites and at the indel bubbles (no counterpart in the reference).
 *
 * The rule is in include/bwbble_hip.h (bwb_hip_geno_begin) and restated here; integer arithmetic only.  E is the error phred (-q, 4..93), d the
 * minimum depth (-d), H = 3.  A site's alleles are the members of its code in the column order A, C, G, T, n_i their pile counters, depth the sum
 * of all four columns; a bubble's alleles are R and V, n_R = ref, n_V = alt, depth = ref + alt + ref_gapped + alt_gapped.  An entry is called when
 * depth >= d.  Over the genotypes in VCF order - (0,0), (0,1), (1,1), (0,2), (1,2), (2,2); two alleles have the first three -
 *   raw(x,x) = E (depth - n_x)      raw(x,y) = H (n_x + n_y) + E (depth - n_x - n_y)
 * GT is the first with the smallest raw, GQ = min(99, the next smallest minus it), PL_j = min(raw_j - raw_GT, 2^32 - 1).
 * -Y (bwb_hip_pileq_begin): the sites' raw costs come from the pile's quality sums instead - geno_rule_q -, the bubbles' stay; the file gains a
 * last column QS, the alleles' sums on S lines and `.` on I lines.
 * `map` has the last worker call on the GPU (kernels k_geno_count / k_geno_emit / k_geno_bubbles) and hands the records to geno_take_*; geno_host
 * makes the same records from the host's tables (aln2sam, places2sam, and map where -A / -I count on the host).  geno_write copies what the
 * records say: the record of a site's position by bisection over the .ann starts, no second scan of the .ref.
 * The file is opened before anything is loaded, so that a path that cannot be written stops the run there; a run that ends through bwb_die
 * (exit) before geno_write has finished leaves no file behind.
 */
#define _GNU_SOURCE
#include <string.h>
#include "bwb_host.h"

#define GENO_SITE_CODES 0x7B74u /* pile.c: PILE_SITE_CODES */
static const uint8_t geno_members[16] = { 0, 0, 12, 0, 6, 14, 10, 0, 3, 11, 0, 7, 5, 13, 9, 0 }; /* the members of a code as columns: bit 0 A, 1 C, 2 G, 3 T */

static char *geno_unfinished; /* the file of a run that has not written it yet: removed at exit */
static void geno_at_exit(void) { if (geno_unfinished) remove(geno_unfinished); }

geno_t *geno_open(const char *genoFname, int err, int64_t min_depth) {
	geno_t *g = (geno_t *)calloc(1, sizeof(*g));
	g->err = err;
	g->min_depth = min_depth;
	if (genoFname) {
		g->fname = strdup(genoFname);
		g->f = fopen(genoFname, "w");
		if (!g->f) { perror(genoFname); bwb_die("-G: Cannot open the calls file: %s!", genoFname); }
		static int registered;
		if (!registered) { atexit(geno_at_exit); registered = 1; }
		geno_unfinished = g->fname;
	}
	return g;
}

static const uint8_t gx[6] = { 0, 0, 1, 0, 1, 2 }, gy[6] = { 0, 1, 1, 2, 2, 2 }; /* the genotypes in VCF order */

/* GT, GQ and the PLs from the raw costs of the ng genotypes; pl has 6 entries, the unused ones 0 */
static void geno_pick(const uint64_t *raw, unsigned ng, uint8_t *gt, uint8_t *gq, uint32_t *pl) {
	unsigned best = 0;
	for (unsigned j = 1; j < ng; j++) if (raw[j] < raw[best]) best = j;
	uint64_t second = UINT64_MAX;
	for (unsigned j = 0; j < ng; j++) if (j != best && raw[j] - raw[best] < second) second = raw[j] - raw[best];
	*gt = (uint8_t)best;
	*gq = (uint8_t)(second > 99 ? 99 : second);
	for (unsigned j = 0; j < 6; j++) {
		const uint64_t d = j < ng ? raw[j] - raw[best] : 0;
		pl[j] = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
	}
}

/* the rule from counts: n[0 .. k), k = 2 or 3 */
void geno_rule(const uint32_t *n, unsigned k, uint64_t depth, unsigned err, uint8_t *gt, uint8_t *gq, uint32_t *pl) {
	const unsigned ng = k == 3 ? 6 : 3;
	uint64_t raw[6];
	for (unsigned j = 0; j < ng; j++) {
		const uint64_t nx = n[gx[j]], ny = n[gy[j]];
		raw[j] = gx[j] == gy[j] ? (uint64_t)err * (depth - nx) : 3u * (nx + ny) + (uint64_t)err * (depth - nx - ny);
	}
	geno_pick(raw, ng, gt, gq, pl);
}

/* -Y, the weighted rule (include/bwbble_hip.h: bwb_hip_pileq_begin): s[0 .. k) the alleles' quality sums, S the sum of all four columns;
 *   raw(x,x) = S - s_x      raw(x,y) = H (n_x + n_y) + (S - s_x - s_y)      in uint64 */
void geno_rule_q(const uint32_t *n, const uint32_t *s, unsigned k, uint64_t S, uint8_t *gt, uint8_t *gq, uint32_t *pl) {
	const unsigned ng = k == 3 ? 6 : 3;
	uint64_t raw[6];
	for (unsigned j = 0; j < ng; j++) {
		const uint64_t nx = n[gx[j]], ny = n[gy[j]], sx = s[gx[j]], sy = s[gy[j]];
		raw[j] = gx[j] == gy[j] ? S - sx : 3u * (nx + ny) + (S - sx - sy);
	}
	geno_pick(raw, ng, gt, gq, pl);
}

/* called entries' records, in ascending order over the calls (what bwb_hip_geno_sites / bwb_hip_geno_bubbles return for one piece): kept for the writer */
void geno_take_sites(geno_t *g, const bwb_geno_site *recs, uint64_t n) {
	if (g->n_sites + n > g->cap_sites) {
		g->cap_sites = (g->n_sites + n) * 2;
		g->sites = (bwb_geno_site *)realloc(g->sites, (size_t)g->cap_sites * sizeof(bwb_geno_site));
		if (g->weighted) g->qs = (uint32_t *)realloc(g->qs, (size_t)g->cap_sites * 16);
		if (!g->sites || (g->weighted && !g->qs)) bwb_die("-G: no memory for the records of %llu called sites", (unsigned long long)g->cap_sites);
	}
	if (n && recs) memcpy(g->sites + g->n_sites, recs, (size_t)n * sizeof(bwb_geno_site));
	g->n_sites += n;
}
/* -Y: the 80-byte records - the site's record, then its four quality sums (room first, then record by record) */
void geno_take_sites_q(geno_t *g, const bwb_geno_site_q *recs, uint64_t n) {
	const uint64_t at = g->n_sites;
	geno_take_sites(g, NULL, n);
	for (uint64_t q = 0; q < n; q++) { g->sites[at + q] = recs[q].site; memcpy(g->qs + (at + q) * 4, recs[q].qs, 16); }
}
void geno_take_bubbles(geno_t *g, const bwb_geno_bubble *recs, uint64_t n) {
	if (g->n_bubs + n > g->cap_bubs) {
		g->cap_bubs = (g->n_bubs + n) * 2;
		g->bubs = (bwb_geno_bubble *)realloc(g->bubs, (size_t)g->cap_bubs * sizeof(bwb_geno_bubble));
		if (!g->bubs) bwb_die("-G: no memory for the records of %llu called bubbles", (unsigned long long)g->cap_bubs);
	}
	if (n) memcpy(g->bubs + g->n_bubs, recs, (size_t)n * sizeof(bwb_geno_bubble));
	g->n_bubs += n;
}

/* the kernels on the host: the records of the called sites of the pile's table (NULL: none) and of the called bubbles of the indel table (NULL:
 * none), in the kernels' layout */
void geno_host(geno_t *g, const pile_t *pile, const indel_t *indel) {
	if (pile && pile->text) {
		const md_text_t *t = pile->text;
		uint64_t site = 0;
		for (uint64_t i = 0; i < t->n_fwd; i++) {
			const unsigned c = t->codes[i] & 15u;
			if (!((GENO_SITE_CODES >> c) & 1u)) continue;
			const uint32_t *v = pile->counts + site * 4;
			const uint64_t depth = (uint64_t)v[0] + v[1] + v[2] + v[3], s = site++;
			if (depth < (uint64_t)g->min_depth) continue;
			bwb_geno_site_q rq;
			bwb_geno_site *r = &rq.site;
			memset(&rq, 0, sizeof(rq));
			const uint32_t *u = g->weighted ? pile->qsum + s * 4 : rq.qs;
			uint32_t n[3] = { 0, 0, 0 }, e[3] = { 0, 0, 0 };
			unsigned k = 0;
			for (unsigned col = 0; col < 4; col++) if ((geno_members[c] >> col) & 1u) { n[k] = v[col]; e[k++] = u[col]; }
			r->pos = i; r->site = s; memcpy(r->n, v, 16);
			r->code = (uint8_t)c; r->n_geno = k == 3 ? 6 : 3;
			if (g->weighted) {
				memcpy(rq.qs, u, 16);
				geno_rule_q(n, e, k, (uint64_t)u[0] + u[1] + u[2] + u[3], &r->gt, &r->gq, r->pl);
				geno_take_sites_q(g, &rq, 1);
			} else {
				geno_rule(n, k, depth, (unsigned)g->err, &r->gt, &r->gq, r->pl);
				geno_take_sites(g, r, 1);
			}
		}
	}
	if (indel && indel->bub) {
		for (int64_t b = 0; b < indel->bub->n; b++) {
			const uint32_t *v = indel->counts + (size_t)b * 4;
			const uint64_t depth = (uint64_t)v[0] + v[1] + v[2] + v[3];
			if (!indel->elig[b] || depth < (uint64_t)g->min_depth) continue;
			bwb_geno_bubble r;
			memset(&r, 0, sizeof(r));
			uint32_t pl[6];
			r.bubble = (uint32_t)b; memcpy(r.n, v, 16);
			geno_rule(v, 2, depth, (unsigned)g->err, &r.gt, &r.gq, pl);
			memcpy(r.pl, pl, 12);
			geno_take_bubbles(g, &r, 1);
		}
	}
}

typedef struct { uint64_t start; int rec; } geno_rec_t;
static int geno_rec_cmp(const void *a, const void *b) {
	const geno_rec_t *x = (const geno_rec_t *)a, *y = (const geno_rec_t *)b;
	return x->start < y->start ? -1 : x->start > y->start ? 1 : x->rec - y->rec;
}

/* `#kind<TAB>record<TAB>pos<TAB>id<TAB>alleles<TAB>AD<TAB>other<TAB>GT<TAB>GQ<TAB>PL`, then one line per called site in text order - S, the first word of
 * the .ann record's name, the 1-based position in the record, the text's letter, the members, their counts, the other bases, GT in letters, GQ,
 * the PLs in genotype order; a site in no record is left out, as in -A - and one line per called bubble in bubble order: I, chrom and pos = A + Bm
 * as -I prints them, the bubble's number, R,V, ref,alt, ref_gapped + alt_gapped, GT, GQ, the three PLs.  bub NULL: no bubble lines.  Returns the
 * lines written; the file is complete and closed after this. */
uint64_t geno_write(geno_t *g, const fasta_annotations_t *ann, const bubble_table_t *bub) {
	geno_rec_t *order = (geno_rec_t *)malloc((ann->num_seq > 0 ? (size_t)ann->num_seq : 1) * sizeof(geno_rec_t));
	for (int i = 0; i < ann->num_seq; i++) order[i] = (geno_rec_t){ ann->seq_anns[i].start_index, i };
	qsort(order, (size_t)ann->num_seq, sizeof(geno_rec_t), geno_rec_cmp);
	fprintf(g->f, "#kind\trecord\tpos\tid\talleles\tAD\tother\tGT\tGQ\tPL%s\n", g->weighted ? "\tQS" : "");
	uint64_t written = 0;
	for (uint64_t q = 0; q < g->n_sites; q++) {
		const bwb_geno_site *r = &g->sites[q];
		/* the last record in `order` that starts at or below the position */
		int lo = 0, hi = ann->num_seq;
		while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (order[mid].start <= r->pos) lo = mid + 1; else hi = mid; }
		/* (records that start at the same position: pile_write takes the first of them that does not end below it) */
		int at = -1;
		for (int k = lo - 1; k >= 0 && order[k].start == order[lo - 1].start; k--) if (ann->seq_anns[order[k].rec].end_index >= r->pos) at = k;
		if (at < 0) continue;
		const seq_annotation_t *a = &ann->seq_anns[order[at].rec];
		const unsigned mem = geno_members[r->code & 15u];
		char al[3]; uint32_t n[3] = { 0, 0, 0 }, e[3] = { 0, 0, 0 }; unsigned k = 0;
		for (unsigned col = 0; col < 4; col++) if ((mem >> col) & 1u) { al[k] = "ACGT"[col]; e[k] = g->weighted ? g->qs[q * 4 + col] : 0; n[k++] = r->n[col]; }
		if (k < 2) continue; /* (no record of a kernel's or of geno_host's) */
		const uint64_t depth = (uint64_t)r->n[0] + r->n[1] + r->n[2] + r->n[3];
		fprintf(g->f, "S\t%.*s\t%llu\t%c\t", (int)strcspn(a->name, " \t"), a->name, (unsigned long long)(r->pos - a->start_index + 1), "NTKGSBYCMHNVRDWA"[r->code & 15u]);
		if (k == 3) fprintf(g->f, "%c,%c,%c\t%u,%u,%u\t%llu\t", al[0], al[1], al[2], n[0], n[1], n[2], (unsigned long long)(depth - n[0] - n[1] - n[2]));
		else fprintf(g->f, "%c,%c\t%u,%u\t%llu\t", al[0], al[1], n[0], n[1], (unsigned long long)(depth - n[0] - n[1]));
		const unsigned j = r->gt < 6 ? r->gt : 0;
		fprintf(g->f, "%c/%c\t%u\t", al[gx[j] < k ? gx[j] : 0], al[gy[j] < k ? gy[j] : 0], r->gq);
		for (unsigned p = 0; p < (k == 3 ? 6u : 3u); p++) fprintf(g->f, "%s%u", p ? "," : "", r->pl[p]);
		for (unsigned p = 0; g->weighted && p < k; p++) fprintf(g->f, "%s%u", p ? "," : "\t", e[p]); /* -Y: QS, the alleles' quality sums */
		fputc('\n', g->f);
		written++;
	}
	for (uint64_t q = 0; bub && q < g->n_bubs; q++) {
		const bwb_geno_bubble *r = &g->bubs[q];
		if ((int64_t)r->bubble >= bub->n) continue;
		const bwb_bubble *b = &bub->b[r->bubble];
		const unsigned j = r->gt < 3 ? r->gt : 0;
		fprintf(g->f, "I\t%.*s\t%lld\t%u\tR,V\t%u,%u\t%llu\t%c/%c\t%u\t%u,%u,%u%s\n", (int)strcspn(bub->ann[r->bubble], " \t"), bub->ann[r->bubble],
		        (long long)((uint64_t)b->A + (uint64_t)b->B_minus_A), r->bubble, r->n[0], r->n[1], (unsigned long long)((uint64_t)r->n[2] + r->n[3]), "RRV"[j], "RVV"[j], r->gq,
		        r->pl[0], r->pl[1], r->pl[2], g->weighted ? "\t." : "");
		written++;
	}
	free(order);
	if (fflush(g->f) || ferror(g->f) || fclose(g->f)) bwb_die("-G: Cannot write to the calls file: %s!", g->fname);
	g->f = NULL;
	geno_unfinished = NULL;
	return written;
}

void geno_free(geno_t *g) {
	if (!g) return;
	if (g->f) fclose(g->f);
	if (g->fname && geno_unfinished == g->fname) { remove(g->fname); geno_unfinished = NULL; }
	free(g->fname); free(g->sites); free(g->qs); free(g->bubs); free(g);
}
