/*
 * pad.c - bubble hits in reference coordinates: what the reference's `sam_pad` (mg-ref/sam_pad.cpp:27-94) appends to the SAM lines of reads
 * placed on a `>bubbleN chr pos` record - the tags bC:Z:<chromosome header> and bP:Z:<position | lo-hi> - from the bubble table that
 * `comb` writes next to the multi-genome (bubble.data, mg-ref/comb.cpp:245-253: two lines per bubble, the k-th pair is bubble k).
 *
 * Three users of one rule: `bwbble sampad` (the text tool, a drop-in for the reference's, streamed line by line), the host resolver
 * locus_resolve (aln2sam -B, places2sam -B, and map -B on an .ann whose records are not ascending and disjoint), and kernel k_locus
 * (map -B: the same arithmetic on the GPU, next to k_place).  Where the reference's behaviour is undefined - a table with half a pair, a
 * numbers line without six integers, a bubble number outside the table, a SAM line without a POS field - this build stops with a message
 * that names the place.
 *
 * -J (no counterpart in the reference): bubble_chrom_of and join_resolve - which of a read's other placements lie where its primary lies,
 * once both are in chromosome coordinates, and the read's counts and MAPQ without them (include/bwbble_hip.h: bwb_join).
 *
 * -R (no counterpart either): lift_check_table, lift_resolve and lift_host - RNAME, POS and CIGAR of a placement on a bubble record rewritten
 * to the chromosome's, the alternate allele as an insertion and the positions the record skips as a deletion (include/bwbble_hip.h: bwb_lift).
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <errno.h>
#include <limits.h>
#include <string.h>
#include <sys/types.h>
#include "bwb_host.h"

/* one line of f without its '\n' (getline(3) keeps the buffer); -1 at the end of the file */
static ssize_t pad_line(char **buf, size_t *cap, FILE *f) {
	ssize_t n = getline(buf, cap, f);
	if (n > 0 && (*buf)[n - 1] == '\n') (*buf)[--n] = 0;
	return n;
}

bubble_table_t *load_bubbles(const char *dataFname) { /* read_in_bubbles, sam_pad.cpp:27-45 */
	FILE *f = fopen(dataFname, "r");
	if (!f) { perror(dataFname); bwb_die("load_bubbles: Cannot open the bubble table: %s!", dataFname); }
	bubble_table_t *t = (bubble_table_t *)calloc(1, sizeof(*t));
	size_t cap_n = 0, lcap = 0, line_no = 0;
	char *line = NULL;
	ssize_t n;
	while ((n = pad_line(&line, &lcap, f)) >= 0) {
		line_no++;
		if ((size_t)t->n == cap_n) {
			cap_n = cap_n ? cap_n * 2 : 1024;
			t->b = (bwb_bubble *)realloc(t->b, cap_n * sizeof(bwb_bubble));
			t->ann = (char **)realloc(t->ann, cap_n * sizeof(char *));
		}
		char *ann = strdup(line);
		if (pad_line(&line, &lcap, f) < 0)
			bwb_die("load_bubbles: %s has an odd number of lines: line %zu (\"%s\") has no numbers line after it", dataFname, line_no, ann);
		line_no++;
		long long v[6];
		const char *q = line;
		for (int k = 0; k < 6; k++) { /* `stream >> A >> ... >> alt_len`: white space, then a signed decimal number */
			char *end;
			errno = 0;
			v[k] = strtoll(q, &end, 10);
			if (end == q || errno || (k >= 4 && (v[k] < INT_MIN || v[k] > INT_MAX)))
				bwb_die("load_bubbles: %s line %zu (bubble %lld): expected six integers A B-A C D-C ref_len alt_len, got \"%s\"", dataFname, line_no, (long long)t->n, line);
			q = end;
		}
		t->b[t->n] = (bwb_bubble){ .A = v[0], .B_minus_A = v[1], .C = v[2], .D_minus_C = v[3], .ref_len = (int32_t)v[4], .alt_len = (int32_t)v[5] };
		t->ann[t->n] = ann;
		t->n++;
	}
	free(line);
	fclose(f);
	return t;
}

void free_bubbles(bubble_table_t *t) {
	if (!t) return;
	for (int64_t k = 0; k < t->n; k++) free(t->ann[k]);
	free(t->ann); free(t->b); free(t);
}

/* sam_pad.cpp:67-72 on one RNAME: -1 when it does not START with "bubble", else atoll of its first white-space delimited word after the
 * word's first six characters ("bubble" alone and "bubbles1 q" are bubble 0) */
int64_t bubble_number(const char *name) {
	if (strncmp(name, "bubble", 6)) return -1;
	char word[32];
	size_t k = 0;
	for (const char *q = name + 6; *q && !isspace((unsigned char)*q) && k + 1 < sizeof(word); q++) word[k++] = *q;
	word[k] = 0;
	const long long v = strtoll(word, NULL, 10); /* (a number that does not fit saturates: outside every table) */
	return v < 0 ? INT64_MIN : (int64_t)v;       /* (a negative number is no index: never -1, which means `not a bubble`) */
}

int32_t *ann_bubble_of(const fasta_annotations_t *ann, const bubble_table_t *t) {
	int32_t *bo = (int32_t *)malloc(((size_t)ann->num_seq ? (size_t)ann->num_seq : 1) * sizeof(int32_t));
	for (int i = 0; i < ann->num_seq; i++) {
		const int64_t w = bubble_number(ann->seq_anns[i].name);
		if (w != -1 && (w < 0 || w >= t->n || w > INT32_MAX))
			bwb_die("bubble table: record %d (\"%s\") names a bubble outside the table of %lld bubbles", i, ann->seq_anns[i].name, (long long)t->n);
		bo[i] = (int32_t)w;
	}
	return bo;
}

/* sam_pad.cpp:75-87: the SAM POS `locus` on bubble b -> a position of the chromosome or, inside the alternate allele and beyond the
 * record, the range of the reference allele (its upper end one below its lower end when ref_len == 0).  64-bit signed like the
 * reference's long long; sums wrap instead of overflowing. */
void bubble_locus(const bwb_bubble *b, int64_t locus, bwb_locus *out) {
	const uint64_t B = (uint64_t)b->B_minus_A, right = B + (uint64_t)(int64_t)b->alt_len + 1u;
	if (locus >= 1 && locus <= b->B_minus_A) {
		out->kind = BWB_LOCUS_POINT;
		out->ref_lo = out->ref_hi = (int64_t)((uint64_t)b->A + (uint64_t)locus - 1u);
	} else if (locus >= (int64_t)right && locus <= (int64_t)(right + (uint64_t)b->D_minus_C)) {
		out->kind = BWB_LOCUS_POINT;
		out->ref_lo = out->ref_hi = (int64_t)((uint64_t)locus + (uint64_t)b->C - right);
	} else {
		out->kind = BWB_LOCUS_RANGE;
		out->ref_lo = (int64_t)(B + (uint64_t)b->A);
		out->ref_hi = (int64_t)(B + (uint64_t)b->A + (uint64_t)(int64_t)b->ref_len - 1u);
	}
}

/* the record that contains aln_pos, -1: none (align.c:796-801 scans linearly; a multi-genome has a record per bubble - 1.3 M at GRCh37
 * scale - and the records are disjoint and in text order, so a binary search finds the same one) */
int ann_find_record(const fasta_annotations_t *ann, int ann_sorted, uint64_t aln_pos) {
	if (ann_sorted) {
		int lo = 0, hi = ann->num_seq - 1;
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ann->seq_anns[mid].start_index <= aln_pos) lo = mid; else hi = mid - 1; }
		if (ann->num_seq > 0 && aln_pos >= ann->seq_anns[lo].start_index && aln_pos <= ann->seq_anns[lo].end_index) return lo;
		return -1;
	}
	for (int i = 0; i < ann->num_seq; i++)
		if (aln_pos >= ann->seq_anns[i].start_index && aln_pos <= ann->seq_anns[i].end_index) return i;
	return -1;
}

/* (text position, annotation table, bubble table) -> locus record: what kernel k_locus computes for `map -B` */
void locus_resolve(const bwb_place *pl, const fasta_annotations_t *ann, int ann_sorted, const int32_t *bubble_of, const bubble_table_t *t, bwb_locus *out) {
	memset(out, 0, sizeof(*out));
	out->seqid = -1; out->bubble = -1;
	if (!(pl->flags & BWB_PLACE_MAPPED)) return;
	const int seqid = ann_find_record(ann, ann_sorted, pl->pos);
	if (seqid < 0) return;
	out->seqid = seqid;
	out->pos1 = (int32_t)(uint32_t)(pl->pos - ann->seq_anns[seqid].start_index + 1);
	out->bubble = bubble_of[seqid];
	if (out->bubble >= 0) bubble_locus(&t->b[out->bubble], (int64_t)out->pos1, out);
}

/* the two tags of a locus record on a bubble, without a terminator; returns the end of the text */
char *locus_put_tags(char *o, const bwb_locus *lc, const bubble_table_t *t) {
	o += sprintf(o, "\tbC:Z:%s\tbP:Z:", t->ann[lc->bubble]);
	if (lc->kind == BWB_LOCUS_POINT) return o + sprintf(o, "%lld", (long long)lc->ref_lo);
	return o + sprintf(o, "%lld-%lld", (long long)lc->ref_lo, (long long)lc->ref_hi);
}

/* ---- -J: a read's placements counted by locus (include/bwbble_hip.h: bwb_join; kernels k_join_items / k_join_reads) -------------------- */

/* the first white-space delimited word of a name */
typedef struct { const char *w; size_t len; int rec; } name_word_t;
static name_word_t first_word(const char *s, int rec) {
	while (*s && isspace((unsigned char)*s)) s++;
	size_t n = 0;
	while (s[n] && !isspace((unsigned char)s[n])) n++;
	return (name_word_t){ .w = s, .len = n, .rec = rec };
}
static int word_cmp(const void *a, const void *b) {
	const name_word_t *x = (const name_word_t *)a, *y = (const name_word_t *)b;
	const int c = memcmp(x->w, y->w, x->len < y->len ? x->len : y->len);
	return c ? c : (x->len > y->len) - (x->len < y->len);
}

/* chrom_of[k]: the .ann record of the chromosome bubble k lies on - the one record whose name's first word is the first word of the bubble's
 * header line in bubble.data.  None, several, or a record that is itself a bubble record: refused, naming the bubble. */
int32_t *bubble_chrom_of(const fasta_annotations_t *ann, const int32_t *bubble_of, const bubble_table_t *t, const char *flag) {
	const size_t n_rec = ann->num_seq > 0 ? (size_t)ann->num_seq : 0;
	name_word_t *words = (name_word_t *)malloc((n_rec ? n_rec : 1) * sizeof(name_word_t));
	for (size_t i = 0; i < n_rec; i++) words[i] = first_word(ann->seq_anns[i].name, (int)i);
	qsort(words, n_rec, sizeof(name_word_t), word_cmp);
	int32_t *chrom_of = (int32_t *)malloc((t->n ? (size_t)t->n : 1) * sizeof(int32_t));
	for (int64_t k = 0; k < t->n; k++) {
		const name_word_t key = first_word(t->ann[k], -1);
		size_t lo = 0, hi = n_rec; /* the first record whose word is not below the key */
		while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (word_cmp(&words[mid], &key) < 0) lo = mid + 1; else hi = mid; }
		size_t same = 0;
		while (lo + same < n_rec && word_cmp(&words[lo + same], &key) == 0) same++;
		if (same != 1)
			bwb_die("bubble table: bubble %lld (\"%s\"): %zu .ann records are named \"%.*s\", one chromosome record is needed (%s)", (long long)k, t->ann[k], same, (int)key.len, key.w, flag);
		if (bubble_of[words[lo].rec] != -1)
			bwb_die("bubble table: bubble %lld (\"%s\"): .ann record %d (\"%s\") is itself a bubble record (%s)", (long long)k, t->ann[k], words[lo].rec, ann->seq_anns[words[lo].rec].name, flag);
		chrom_of[k] = words[lo].rec;
	}
	free(words);
	return chrom_of;
}

/* (c, lo, hi') of a placement from its locus record; 0: it has none */
static int join_locus(const bwb_locus *lc, const int32_t *chrom_of, int32_t *c, int64_t *lo, int64_t *hi) {
	if (lc->seqid < 0) return 0;
	if (lc->bubble >= 0) { *c = chrom_of[lc->bubble]; *lo = lc->ref_lo; *hi = lc->ref_hi; }
	else { *c = lc->seqid; *lo = *hi = (int64_t)lc->pos1; }
	if (*hi < *lo) *hi = *lo; /* a pure insertion's empty range counts as its left edge */
	return 1;
}

/* one read: its placement record, that record's locus, its items and their suboptimal bytes -> its join record: what the two kernels compute
 * for `map -J` */
void join_resolve(const bwb_place *pl, const bwb_locus *lc, const bwb_alt *items, const uint8_t *sub, uint64_t n_items, const fasta_annotations_t *ann, int ann_sorted,
                  const int32_t *bubble_of, const int32_t *chrom_of, const bubble_table_t *t, int max_mm, bwb_join *out) {
	memset(out, 0, sizeof(*out));
	if (!(pl->flags & BWB_PLACE_MAPPED)) return;
	int32_t cp = 0, ci = 0;
	int64_t lop = 0, hip = 0, loi = 0, hii = 0;
	const int has_p = join_locus(lc, chrom_of, &cp, &lop, &hip);
	uint32_t best = 0, subopt = 0;
	for (uint64_t k = 0; k < n_items && has_p; k++) {
		const bwb_place as_place = { .pos = items[k].pos, .flags = items[k].flags };
		bwb_locus il;
		locus_resolve(&as_place, ann, ann_sorted, bubble_of, t, &il);
		if (!join_locus(&il, chrom_of, &ci, &loi, &hii) || ci != cp || ((items[k].flags ^ pl->flags) & BWB_PLACE_REVERSE) || loi > hip || lop > hii) continue;
		if (sub[k]) subopt++; else best++;
	}
	out->top1 = (int32_t)((uint32_t)pl->top1 - best);
	out->top2 = (int32_t)((uint32_t)pl->top2 - subopt);
	out->mapq = n_items ? (uint8_t)sam_mapq(out->top1, out->top2, pl->num_mm, max_mm) : pl->mapq;
	out->joined = (uint8_t)(best + subopt);
}

/* ---- -R: a placement on a bubble record in chromosome coordinates (include/bwbble_hip.h: bwb_lift; kernels k_lift_count / k_lift) ---------- */

/* 0: the rule can use bubble b; else why not (the five refusals of -R) */
const char *lift_bubble_refusal(const bwb_bubble *b) {
	const __int128 gap = (__int128)b->C - (__int128)b->A - (__int128)b->B_minus_A;
	if (b->B_minus_A < 0) return "B_minus_A is negative";
	if (b->D_minus_C < -1) return "D_minus_C is below -1";
	if (b->alt_len < 0) return "alt_len is negative";
	if (gap < 0) return "its flanks overlap on the chromosome (C - A - B_minus_A is negative)";
	if (gap >= ((__int128)1 << 28)) return "its flanks lie 2^28 positions or more apart";
	return NULL;
}

void lift_check_table(const bubble_table_t *t) {
	for (int64_t k = 0; k < t->n; k++) {
		const char *why = lift_bubble_refusal(&t->b[k]);
		if (why) bwb_die("bubble table: bubble %lld (\"%s\"): %s (-R)", (long long)k, t->ann[k], why);
	}
}

/* 0 left flank, 1 alternate allele, 2 right flank, of a record position x >= 1 that the span check has kept inside the record */
static inline int lift_zone(const bwb_bubble *b, int64_t x) { return x <= b->B_minus_A ? 0 : (x - b->B_minus_A <= (int64_t)b->alt_len ? 1 : 2); }

typedef struct { uint32_t *ops; unsigned n, kind; uint64_t len; } lift_out_t;
static inline void lift_put(lift_out_t *o) {
	if (o->kind == 0xFFu) return;
	if (o->n < BWB_LIFT_MAX_OPS) o->ops[o->n] = (uint32_t)(o->len << 4) | o->kind;
	o->n++;
}
static inline void lift_emit(lift_out_t *o, unsigned kind, uint64_t len) {
	if (kind == o->kind && o->len + len < ((uint64_t)1 << 28)) { o->len += len; return; }
	lift_put(o);
	o->kind = kind; o->len = len;
}

/* The rule on one placement of bubble b (a table lift_check_table has passed): printed position pos1, strand, path length and gap runs as
 * bwb_place / bwb_alt hold them -> the record's header and ops.  Returns the number of ops, 0: not liftable (the span leaves the record, or
 * no M remains).  What kernels k_lift_count / k_lift compute. */
int lift_resolve(const bwb_bubble *b, int32_t chrom, int64_t pos1, int reverse, unsigned alen, const uint16_t *gap_run, bwb_lift *hdr, uint32_t *ops) {
	const int64_t gap = (int64_t)((uint64_t)b->C - (uint64_t)b->A - (uint64_t)b->B_minus_A);
	/* first pass: the span on the record, and the first and last M that stays an M */
	int64_t x = pos1, first = -1, last = -1, x_first = 0;
	for (unsigned t = 0; t < alen; t++) {
		const unsigned op = lift_op_at(gap_run, alen, reverse, t);
		if (op == BWB_LIFT_I) continue;
		if (op == BWB_LIFT_M && x >= 1 && lift_zone(b, x) != 1) { if (first < 0) { first = t; x_first = x; } last = t; }
		x++;
	}
	const int64_t end = x - 1; /* the last record position consumed */
	/* (pos1 < 1: the rule's own condition, kept for a caller of this function - a locus on a bubble record always has pos1 >= 1) */
	if (pos1 < 1 || first < 0) return 0;
	if (end > b->B_minus_A && end - b->B_minus_A > (int64_t)b->alt_len && end - b->B_minus_A - (int64_t)b->alt_len - 1 > b->D_minus_C) return 0;
	lift_out_t o = { .ops = ops, .n = 0, .kind = 0xFFu, .len = 0 };
	uint64_t lead = 0, trail = 0;
	x = pos1;
	for (unsigned t = 0; t < alen; t++) {
		const unsigned op = lift_op_at(gap_run, alen, reverse, t);
		unsigned kind = BWB_LIFT_I;
		if (op != BWB_LIFT_I) {
			const int z = lift_zone(b, x);
			/* the walk enters the right flank: the positions the record skips, behind the allele's I */
			if (z == 2 && x - b->B_minus_A == (int64_t)b->alt_len + 1 && x > pos1 && gap > 0 && (int64_t)t > first && (int64_t)t <= last) lift_emit(&o, BWB_LIFT_D, (uint64_t)gap);
			kind = op == BWB_LIFT_M ? (z == 1 ? BWB_LIFT_I : BWB_LIFT_M) : (z == 1 ? 0xFFu : BWB_LIFT_D);
			x++;
		}
		if (kind == 0xFFu) continue;
		if ((int64_t)t < first) lead += kind == BWB_LIFT_I;
		else if ((int64_t)t > last) trail += kind == BWB_LIFT_I;
		else {
			if ((int64_t)t == first && lead) lift_emit(&o, BWB_LIFT_S, lead);
			lift_emit(&o, kind, 1);
		}
	}
	lift_put(&o);
	if (trail) { o.kind = BWB_LIFT_S; o.len = trail; lift_put(&o); }
	if (o.n > BWB_LIFT_MAX_OPS) return 0; /* (17 runs and the three the allele adds: not reached) */
	memset(hdr, 0, sizeof(*hdr));
	const int64_t right = b->B_minus_A + (int64_t)b->alt_len + 1;
	hdr->pos = x_first <= b->B_minus_A ? (int64_t)((uint64_t)b->A + (uint64_t)x_first - 1u) : (int64_t)((uint64_t)b->C + (uint64_t)(x_first - right));
	hdr->seqid = chrom;
	hdr->n_ops = (uint8_t)o.n;
	return (int)o.n;
}

/* -R on the host (aln2sam, places2sam, and map on an .ann that is not ascending and disjoint): the lift records of n reads and their items
 * (alt_off NULL: none), laid out as bwb_hip_slot_lift returns them; with all cores */
lift_set_t *lift_host(const bwb_place *pl, const bwb_locus *loci, size_t n, const uint64_t *alt_off, const bwb_alt *alts, const fasta_annotations_t *ann, int ann_sorted,
                      const int32_t *bubble_of, const int32_t *chrom_of, const bubble_table_t *t) {
	const size_t n_items = alt_off ? (size_t)alt_off[n] : 0, nq = n + n_items;
	lift_set_t *ls = (lift_set_t *)calloc(1, sizeof(*ls));
	ls->kind = (uint8_t *)calloc(nq ? nq : 1, 1);
	ls->off = (uint64_t *)calloc(nq + 1, 8);
	for (int pass = 0; pass < 2; pass++) {
		uint64_t lifted = 0, unliftable = 0;
#pragma omp parallel for schedule(static) reduction(+ : lifted, unliftable) num_threads(bwb_host_team())
		for (long q = 0; q < (long)nq; q++) {
			if (pass && ls->kind[q] != BWB_LIFT_LIFTED) continue;
			bwb_locus il;
			const bwb_locus *lc = &il;
			const uint16_t *runs;
			unsigned alen;
			int reverse;
			if ((size_t)q < n) { lc = &loci[q]; runs = pl[q].gap_run; alen = pl[q].aln_length; reverse = (pl[q].flags & BWB_PLACE_REVERSE) != 0; }
			else {
				const bwb_alt *a = &alts[(size_t)q - n];
				const bwb_place as_place = { .pos = a->pos, .flags = a->flags };
				locus_resolve(&as_place, ann, ann_sorted, bubble_of, t, &il);
				runs = a->gap_run; alen = a->aln_length; reverse = (a->flags & BWB_PLACE_REVERSE) != 0;
			}
			if (lc->bubble < 0) continue;
			bwb_lift hdr;
			uint32_t ops[BWB_LIFT_MAX_OPS];
			const int n_ops = lift_resolve(&t->b[lc->bubble], chrom_of[lc->bubble], (int64_t)lc->pos1, reverse, alen, runs, &hdr, ops);
			if (!pass) {
				ls->kind[q] = n_ops ? BWB_LIFT_LIFTED : BWB_LIFT_UNLIFTABLE;
				ls->off[q + 1] = n_ops ? 1 + ((uint64_t)n_ops + 3) / 4 : 0;
				lifted += n_ops != 0; unliftable += n_ops == 0;
			} else {
				bwb_lift *dst = ls->recs + ls->off[q];
				memset(dst, 0, (size_t)(ls->off[q + 1] - ls->off[q]) * sizeof(bwb_lift));
				dst[0] = hdr;
				memcpy(dst + 1, ops, (size_t)n_ops * 4);
			}
		}
		if (!pass) {
			ls->n_lifted = lifted; ls->n_unliftable = unliftable;
			for (size_t q = 0; q < nq; q++) ls->off[q + 1] += ls->off[q];
			ls->recs = (bwb_lift *)malloc((ls->off[nq] ? (size_t)ls->off[nq] : 1) * sizeof(bwb_lift));
		}
	}
	return ls;
}

void lift_free(lift_set_t *ls) {
	if (!ls) return;
	free(ls->kind); free(ls->off); free(ls->recs); free(ls);
}

/* `bwbble sampad <bubble.data> <in.sam> <out.sam>`: process_sam (sam_pad.cpp:47-94), one line in memory at a time.  A refused line leaves
 * no output file behind. */
void sam_pad(const char *dataFname, const char *inFname, const char *outFname) {
	bubble_table_t *t = load_bubbles(dataFname);
	FILE *in = fopen(inFname, "r");
	if (!in) { perror(inFname); bwb_die("sampad: Cannot open SAM file: %s!", inFname); }
	FILE *out = fopen(outFname, "w");
	if (!out) { perror(outFname); bwb_die("sampad: Cannot open SAM file: %s!", outFname); }
#define SAMPAD_REFUSE(...) do { fclose(out); remove(outFname); bwb_die(__VA_ARGS__); } while (0)
	size_t ann_max = 0;
	for (int64_t k = 0; k < t->n; k++) if (strlen(t->ann[k]) > ann_max) ann_max = strlen(t->ann[k]);
	char *line = NULL, *tags = (char *)malloc(ann_max + 64);
	size_t lcap = 0, line_no = 0, padded = 0;
	ssize_t n;
	while ((n = pad_line(&line, &lcap, in)) >= 0) {
		line_no++;
		int ok = fwrite(line, 1, (size_t)n, out) == (size_t)n;
		if (n == 0 || line[0] != '@') {
			char *f[4] = { line, NULL, NULL, NULL }; /* QNAME, FLAG, RNAME, POS */
			for (int k = 1; k < 4 && f[k - 1]; k++) { char *tab = strchr(f[k - 1], '\t'); f[k] = tab ? tab + 1 : NULL; }
			if (!f[3]) SAMPAD_REFUSE("sampad: %s line %zu has fewer than four fields", inFname, line_no);
			f[3][-1] = 0; /* RNAME ends here (the line has been written) */
			const int64_t w = bubble_number(f[2]);
			if (w != -1) {
				if (w < 0 || w >= t->n) SAMPAD_REFUSE("sampad: %s line %zu: \"%s\" names a bubble outside the table of %lld bubbles", inFname, line_no, f[2], (long long)t->n);
				bwb_locus lc = { .bubble = (int32_t)w };
				bubble_locus(&t->b[w], strtoll(f[3], NULL, 10), &lc); /* atoll(POS) */
				const size_t tn = (size_t)(locus_put_tags(tags, &lc, t) - tags);
				ok = ok && fwrite(tags, 1, tn, out) == tn;
				padded++;
			}
		}
		if (!ok || fputc('\n', out) == EOF) SAMPAD_REFUSE("sampad: Cannot write to the SAM file: %s!", outFname);
	}
	free(line); free(tags);
	fclose(in);
	if (fclose(out)) { remove(outFname); bwb_die("sampad: Cannot write to the SAM file: %s!", outFname); }
#undef SAMPAD_REFUSE
	printf("Processed %zu lines, %zu on bubbles.\n", line_no, padded);
	free_bubbles(t);
}
