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
int32_t *bubble_chrom_of(const fasta_annotations_t *ann, const int32_t *bubble_of, const bubble_table_t *t) {
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
			bwb_die("bubble table: bubble %lld (\"%s\"): %zu .ann records are named \"%.*s\", one chromosome record is needed (-J)", (long long)k, t->ann[k], same, (int)key.len, key.w);
		if (bubble_of[words[lo].rec] != -1)
			bwb_die("bubble table: bubble %lld (\"%s\"): .ann record %d (\"%s\") is itself a bubble record (-J)", (long long)k, t->ann[k], words[lo].rec, ann->seq_anns[words[lo].rec].name);
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
