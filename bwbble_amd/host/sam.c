/*
 * sam.c - `bwbble aln2sam`: .aln + FASTQ -> SAM, same text as the reference (mg-aligner/align.c:494-556 alns2sam,
 * :562-652 print_aln2sam, :738-812 mapq / eval_aln).
 *
 * The only index work here is SA(aln.L) for the reported hit of every mapped read (align.c:786), an invPsi
 * walk of up to 31 dependent rank queries (bwt.c:311-329).  It runs on the GPU for all reads at once
 * (bwb_hip_locate); MAPQ (the only floating point in the tool), CIGAR and text stay on the host.
 *
 * Two halves since `bwbble map`: place_from_alns (eval_aln of one read -> a bwb_place record) and sam_format_reads (records + names, bases,
 * qualities, annotations -> text).  `map` gets its records from the GPU (kernel k_place) and shares the formatter; `places2sam` feeds it
 * from a file for the CPU tests.
 */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include "bwb_host.h"

#define SAM_FSU 4
#define SAM_FSR 16

int sam_mapq(int top1, int top2, int num_mm, int max_mm) { /* align.c:738-746 */
	if (top1 == 0) return 23;
	if (top1 > 1) return 0;
	if (num_mm == max_mm) return 25;
	if (top2 == 0) return 37;
	int n = top2 >= 255 ? 255 : top2;
	int q = (int)(4.343 * log(n) + 0.5);
	return 23 < q ? 0 : 23 - q;
}

/* eval_aln (align.c:760-812) on the host: the placement record of one read from its .aln hits and SA(e[0].L).  The same arithmetic as
 * kernel k_place (`bwbble map` gets these records from the GPU, where the hits lie). */
void place_from_alns(const bwb_aln *e, uint64_t ne, uint64_t ref_pos, uint64_t bwt_length, int max_mm, bwb_place *out) {
	memset(out, 0, sizeof(*out));
	if (ne == 0) return; /* unmapped */
	int top1 = 0, top2 = 0;
	const int best_score = e[0].score;
	for (uint64_t i = 0; i < ne; i++) {
		if (e[i].score > best_score) top2 += (int)(e[i].U - e[i].L + 1);
		else top1 += (int)(e[i].U - e[i].L + 1);
	}
	unsigned char path[272];
	const int alen = aln_path_bytes(&e[0], path);
	int ref_len = alen;                                                          /* get_aln_length :748-757 */
	for (int i = 0; i < alen; i++) if (path[i] == 1) ref_len--;
	out->flags = BWB_PLACE_MAPPED;
	if (ref_pos > (bwt_length - 1) / 2) out->pos = ((bwt_length - 1) - ref_pos - 1) - (uint64_t)ref_len + 1;
	else { out->flags |= BWB_PLACE_REVERSE; out->pos = ref_pos; }
	out->top1 = top1; out->top2 = top2;
	out->score = e[0].score;
	out->mapq = (uint8_t)sam_mapq(top1, top2, e[0].num_mm, max_mm);
	out->num_mm = e[0].num_mm; out->num_gapo = e[0].num_gapo; out->num_gape = e[0].num_gape;
	out->aln_length = (uint16_t)alen; out->ref_len = (uint16_t)ref_len;
	memcpy(out->gap_run, e[0].gap_run, sizeof(out->gap_run));
}

/* the same for one of the read's other placements (`aln2sam -X`): hit number `hit` of the read and SA(its row), like kernel k_place_alt */
void alt_from_aln(const bwb_aln *e, unsigned hit, uint64_t ref_pos, uint64_t bwt_length, bwb_alt *out) {
	memset(out, 0, sizeof(*out));
	unsigned char path[272];
	const int alen = aln_path_bytes(e, path);
	int ref_len = alen;
	for (int i = 0; i < alen; i++) if (path[i] == 1) ref_len--;
	out->flags = BWB_PLACE_MAPPED;
	if (ref_pos > (bwt_length - 1) / 2) out->pos = ((bwt_length - 1) - ref_pos - 1) - (uint64_t)ref_len + 1;
	else { out->flags |= BWB_PLACE_REVERSE; out->pos = ref_pos; }
	out->hit = (uint8_t)hit;
	out->num_mm = e->num_mm; out->num_gapo = e->num_gapo; out->num_gape = e->num_gape;
	out->aln_length = (uint16_t)alen;
	memcpy(out->gap_run, e->gap_run, sizeof(out->gap_run));
}

/* the number of a read's placements - the rows of all its hits - as the X tags count them: 64-bit and saturating, a hit with U < L saturates */
uint64_t alt_placements(const bwb_aln *e, uint64_t ne) {
	uint64_t T = 0;
	for (uint64_t i = 0; i < ne; i++) {
		const uint64_t w = e[i].U - e[i].L + 1;
		if (e[i].U < e[i].L || w == 0 || T + w < T) return UINT64_MAX;
		T += w;
	}
	return T;
}

void sam_write_header(FILE *sam, const fasta_annotations_t *ann) {
	for (int i = 0; i < ann->num_seq; i++)                                           /* align.c:522-525 */
		fprintf(sam, "@SQ\tSN:%s\tLN:%d\n", ann->seq_anns[i].name, (int)(ann->seq_anns[i].end_index - ann->seq_anns[i].start_index + 1));
	fprintf(sam, "@PG\tID:bwbble\tPN:bwbble\tVN:0.1-r01\n");
}

int sam_ann_sorted(const fasta_annotations_t *ann) { /* records as fasta2ref writes them: increasing, disjoint */
	for (int i = 1; i < ann->num_seq; i++) if (ann->seq_anns[i].start_index <= ann->seq_anns[i - 1].end_index) return 0;
	return 1;
}

/* CIGAR of a path given by its length and gap runs (as bwb_place.gap_run), reversed for the reverse strand: runs of the path walked from
 * its end to its start (align.c:588-609); returns the end of the text */
static char *sam_put_cigar(char *o, uint16_t aln_length, const uint16_t *gap_run, int strand) {
	unsigned char path[272];
	bwb_aln e0;
	memset(&e0, 0, sizeof(e0));
	e0.aln_length = aln_length;
	memcpy(e0.gap_run, gap_run, sizeof(e0.gap_run));
	const int alen = aln_path_bytes(&e0, path);
	if (strand) for (int i = 0; i < alen >> 1; i++) { unsigned char t = path[alen - 1 - i]; path[alen - 1 - i] = path[i]; path[i] = t; }
	int i = alen - 1;
	while (i >= 0) {
		int j = i;
		while (j >= 0 && path[j] == path[i]) j--;
		o += sprintf(o, "%d%c", i - j, "MID"[path[i]]);
		i = j;
	}
	return o;
}

/* CIGAR of a lift record (-R): its ops as they lie; returns the end of the text */
static char *sam_put_lifted_cigar(char *o, const bwb_lift *rec) {
	const uint32_t *ops = (const uint32_t *)(rec + 1);
	for (unsigned i = 0; i < rec->n_ops; i++) o += sprintf(o, "%u%c", ops[i] >> 4, "MID?S???????????"[ops[i] & 15u]);
	return o;
}

/* print_aln2sam (align.c:562-652) for reads [r0, r1) of rd: placement records + names / bases / qualities + annotations -> SAM text in a
 * malloc'ed buffer.  Shared by aln2sam (records from place_from_alns), map (records from the GPU) and places2sam (records from a file). */
char *sam_format_reads(const sam_reads_t *rd, size_t r0, size_t r1, const fasta_annotations_t *ann, int ann_sorted, size_t *out_len) {
	size_t cap = 0;
	for (size_t r = r0; r < r1; r++) cap += (size_t)rd->name_len[r] + 2 * (size_t)rd->len[r] + MAX_SEQ_NAME_LEN + 160 + 8 * (size_t)rd->pl[r].num_gapo;
	if (rd->alt_off) { /* the tags: X0 and X1 (two ints), and per item a name, a position, a CIGAR of up to 17 runs and NM */
		cap += (r1 - r0) * 48;
		for (uint64_t k = rd->alt_off[r0]; k < rd->alt_off[r1]; k++) cap += MAX_SEQ_NAME_LEN + 64 + 8 * (size_t)rd->alts[k].num_gapo;
	}
	if (rd->joins) cap += (r1 - r0) * 12; /* -J: "\tbJ:i:255" */
	if (rd->lift_kind) { /* -R: a lifted placement prints another name, a 64-bit position and up to 20 ops; a primary also the tag bO with its own CIGAR */
		for (size_t r = r0; r < r1; r++) if (rd->lift_kind[r] == BWB_LIFT_LIFTED) cap += 2 * MAX_SEQ_NAME_LEN + 480 + 8 * (size_t)rd->pl[r].num_gapo;
		if (rd->alt_off) for (uint64_t k = rd->alt_off[r0]; k < rd->alt_off[r1]; k++) if (rd->lift_kind[rd->lift_n + k] == BWB_LIFT_LIFTED) cap += MAX_SEQ_NAME_LEN + 320;
	}
	if (rd->md) cap += (r1 - r0) * 32 + (size_t)(rd->md_off[r1] - rd->md_off[r0]); /* -D: "\tNM:i:<32-bit>\tMD:Z:" and the MD bytes */
	if (rd->loci) /* -B: on a bubble record the chromosome's header and one or two 64-bit numbers */
		for (size_t r = r0; r < r1; r++) if (rd->loci[r].bubble >= 0) cap += strlen(rd->bubbles->ann[rd->loci[r].bubble]) + 64;
	char *o = (char *)malloc(cap ? cap : 1), *o0 = o;
	for (size_t r = r0; r < r1; r++) {
		const bwb_place *pl = &rd->pl[r];
		const int len = rd->len[r];
		const uint8_t *seq = rd->seq + (size_t)r * rd->stride;
		const char *name = rd->text + rd->name_off[r];
		const char *qual = rd->text + rd->qual_off[r];
		memcpy(o, name, rd->name_len[r]); o += rd->name_len[r];
		if (!(pl->flags & BWB_PLACE_MAPPED)) { /* unmapped, align.c:629-651 (aln_strand is 0 for a read that was never evaluated) */
			o += sprintf(o, "\t%d\t*\t0\t0\t*\t*\t0\t0\t", SAM_FSU);
			for (int i = 0; i < len; i++) o[i] = "AGCTN"[seq[i]];
			o += len; *o++ = '\t';
			memcpy(o, qual, (size_t)len); o += len; *o++ = '\n';
			continue;
		}
		const int strand = (pl->flags & BWB_PLACE_REVERSE) != 0;
		const uint64_t aln_pos = pl->pos;
		/* -B: the read's record and POS were resolved with its locus (kernel k_locus for `map`, locus_resolve otherwise) */
		const int seqid = rd->loci ? rd->loci[r].seqid : ann_find_record(ann, ann_sorted, aln_pos);
		if (seqid < 0 || seqid >= ann->num_seq) bwb_die("alns2sam: read %zu maps outside every annotated sequence", rd->first + r); /* the reference indexes seq_anns[-1] here */
		/* -R: a lifted placement lies on the chromosome of its bubble */
		const bwb_lift *lifted = rd->lift_kind && rd->lift_kind[r] == BWB_LIFT_LIFTED ? rd->lift_recs + rd->lift_off[r] : NULL;
		if (lifted) {
			if (lifted->seqid < 0 || lifted->seqid >= ann->num_seq) bwb_die("alns2sam: read %zu is lifted to a record outside the annotations", rd->first + r);
			o += sprintf(o, "\t%d\t%s\t%lld\t%d\t", strand ? SAM_FSR : 0, ann->seq_anns[lifted->seqid].name, (long long)lifted->pos, rd->joins ? (int)rd->joins[r].mapq : (int)pl->mapq);
			o = sam_put_lifted_cigar(o, lifted);
		} else {
			o += sprintf(o, "\t%d\t%s\t%d\t%d\t", strand ? SAM_FSR : 0, ann->seq_anns[seqid].name, rd->loci ? (int)rd->loci[r].pos1 : (int)(aln_pos - ann->seq_anns[seqid].start_index + 1), rd->joins ? (int)rd->joins[r].mapq : (int)pl->mapq);
			o = sam_put_cigar(o, pl->aln_length, pl->gap_run, strand);
		}
		memcpy(o, "\t*\t0\t0\t", 7); o += 7;
		if (strand) for (int k = 0; k < len; k++) { const int c = seq[len - 1 - k]; o[k] = "AGCTN"[c > 3 ? 4 : 3 - c]; } /* read->rc */
		else for (int k = 0; k < len; k++) o[k] = "AGCTN"[seq[k]];
		o += len; *o++ = '\t';
		if (strand) for (int k = 0; k < len; k++) o[k] = qual[len - 1 - k];
		else memcpy(o, qual, (size_t)len);
		o += len;
		if (rd->md && rd->md[r].kind == BWB_MD_OK) { /* -D: directly behind QUAL, the bytes the kernel (or md_resolve) wrote */
			o += sprintf(o, "\tNM:i:%u\tMD:Z:", rd->md[r].nm);
			memcpy(o, rd->md_text + rd->md_off[r], rd->md[r].md_len); o += rd->md[r].md_len;
		}
		if (rd->alt_off) { /* -X: the two counters as they are, and the read's other placements (an item outside every record is left out) */
			o += sprintf(o, "\tX0:i:%d\tX1:i:%d", (int)pl->top1, (int)pl->top2);
			if (rd->alt_off[r + 1] > rd->alt_off[r]) { memcpy(o, "\tXA:Z:", 6); o += 6; }
			for (uint64_t k = rd->alt_off[r]; k < rd->alt_off[r + 1]; k++) {
				const bwb_alt *a = &rd->alts[k];
				const int sid = ann_find_record(ann, ann_sorted, a->pos);
				if (sid < 0) continue;
				const bwb_lift *li = rd->lift_kind && rd->lift_kind[rd->lift_n + k] == BWB_LIFT_LIFTED ? rd->lift_recs + rd->lift_off[rd->lift_n + k] : NULL;
				if (li && li->seqid >= 0 && li->seqid < ann->num_seq) {
					o += sprintf(o, "%s,%c%lld,", ann->seq_anns[li->seqid].name, (a->flags & BWB_PLACE_REVERSE) ? '-' : '+', (long long)li->pos);
					o = sam_put_lifted_cigar(o, li);
					o += sprintf(o, ",%d;", (int)a->num_mm + (int)a->num_gapo + (int)a->num_gape);
					continue;
				}
				o += sprintf(o, "%s,%c%d,", ann->seq_anns[sid].name, (a->flags & BWB_PLACE_REVERSE) ? '-' : '+', (int)(a->pos - ann->seq_anns[sid].start_index + 1));
				o = sam_put_cigar(o, a->aln_length, a->gap_run, (a->flags & BWB_PLACE_REVERSE) != 0);
				o += sprintf(o, ",%d;", (int)a->num_mm + (int)a->num_gapo + (int)a->num_gape);
			}
		}
		if (rd->loci && rd->loci[r].bubble >= 0) o = locus_put_tags(o, &rd->loci[r], rd->bubbles); /* last on the line, like sam_pad's */
		if (rd->joins && rd->joins[r].joined) o += sprintf(o, "\tbJ:i:%d", (int)rd->joins[r].joined); /* -J: behind them */
		if (lifted) { /* -R: where the read was placed - the bubble record's first word, POS and CIGAR there; last */
			const char *bn = ann->seq_anns[seqid].name;
			size_t wl = 0;
			while (bn[wl] && bn[wl] != ' ' && bn[wl] != '\t') wl++;
			o += sprintf(o, "\tbO:Z:%.*s,%d,", (int)wl, bn, rd->loci ? (int)rd->loci[r].pos1 : (int)(aln_pos - ann->seq_anns[seqid].start_index + 1));
			o = sam_put_cigar(o, pl->aln_length, pl->gap_run, strand);
		}
		*o++ = '\n';
	}
	*out_len = (size_t)(o - o0);
	return o0;
}

/* SA lookups of a contiguous share of the rows on one GPU (the index is replicated, like in align) */
typedef struct { int device; const bwt_t *BWT; const uint64_t *rows; uint64_t *pos; size_t n; uint64_t steps; double kernel_ms; } locate_job_t;
static void *locate_worker(void *arg) {
	locate_job_t *j = (locate_job_t *)arg;
	bwb_hip_ctx *ctx = NULL;
	const bwtint_t hdr[5] = { j->BWT->length, j->BWT->num_words, j->BWT->num_sa, j->BWT->num_occ, j->BWT->sa0_index };
	if (bwb_hip_ctx_create(j->device, hdr, j->BWT->C, j->BWT->bwt, j->BWT->O, &ctx) || bwb_hip_set_sa(ctx, j->BWT->SA, j->BWT->num_sa) ||
	    bwb_hip_locate(ctx, j->rows, j->n, j->pos))
		bwb_die("alns2sam: GPU %d: %s", j->device, bwb_hip_last_error());
	bwb_hip_locate_stats(ctx, NULL, &j->steps, &j->kernel_ms);
	bwb_hip_ctx_destroy(ctx);
	return NULL;
}

/* the carrier of a whole file's reads (aln2sam, places2sam): the records so far; host_chain adds the rest */
static sam_reads_t sam_reads_of(const reads_t *reads, size_t n, const bwb_place *pl, const uint64_t *alt_off, const bwb_alt *alts) {
	return (sam_reads_t){ .pl = pl, .seq = reads->seq, .stride = reads->stride, .len = reads->len, .text = reads->raw,
	                      .name_off = reads->name_off, .qual_off = reads->qual_off, .name_len = reads->name_len, .first = 0, .alt_off = alt_off, .alts = alts, .lift_n = n };
}

void alns2sam(char *fastaFname, char *readsFname, char *alnsFname, char *samFname, int is_multiref, int n_gpus, const map_opts_t *o) {
	(void)is_multiref;
	printf("**** BWBBLE Alignment Evaluation/SAM File Generation ****\n");
	const int max_alt = o->max_alt;
	host_outs_t out;
	host_outs_open(&out, o);
	md_text_t *text = host_text_open(fastaFname, o, &out, 0); /* (before anything is loaded or created) */
	size_t Ln = strlen(fastaFname) + 8;
	char *bwtFname = (char *)malloc(Ln), *annFname = (char *)malloc(Ln);
	snprintf(bwtFname, Ln, "%s.bwt", fastaFname);
	snprintf(annFname, Ln, "%s.ann", fastaFname);
	bwt_t *BWT = load_bwt(bwtFname, 1);
	fasta_annotations_t *ann = annf2ann(annFname);
	host_tables_t T;
	host_tables_load(&T, ann, o, out.indel != NULL);
	alns_batch_t *alns = alnsf2alns_bin(alnsFname);
	reads_t *reads = fastq2reads(readsFname);
	FILE *sam = fopen(samFname, "w");
	if (!sam) { perror(samFname); bwb_die("alns2sam: Cannot open SAM file: %s!", samFname); }
	sam_write_header(sam, ann);

	const size_t n = reads->count < alns->n_reads ? reads->count : alns->n_reads;    /* align.c:535-537 */
	/* SA(aln.L) of the first entry of every mapped read, on the GPU */
	/* -X: the rows of the reads' other placements ride along behind the primaries' (the same rows kernel k_place_alt walks from for `map -X`) */
	uint64_t *alt_off = NULL;
	bwb_alt *alts = NULL;
	if (max_alt) {
		alt_off = (uint64_t *)calloc(n + 1, 8);
		for (size_t r = 0; r < n; r++) {
			const uint64_t T = alt_placements(alns->alns + alns->aln_off[r], alns->aln_off[r + 1] - alns->aln_off[r]);
			alt_off[r + 1] = alt_off[r] + (T >= 2 && T <= (uint64_t)max_alt + 1 ? T - 1 : 0);
		}
		alts = (bwb_alt *)malloc((alt_off[n] ? alt_off[n] : 1) * sizeof(bwb_alt));
	}
	const size_t n_alt = max_alt ? (size_t)alt_off[n] : 0, n_rows = n + n_alt;
	uint64_t *rows = (uint64_t *)malloc((n_rows ? n_rows : 1) * 8), *pos = (uint64_t *)malloc((n_rows ? n_rows : 1) * 8);
	size_t *which = (size_t *)malloc((n ? n : 1) * sizeof(size_t));
	size_t nm = 0;
	for (size_t r = 0; r < n; r++)
		if (alns->aln_off[r + 1] > alns->aln_off[r]) { rows[nm] = alns->alns[alns->aln_off[r]].L; which[nm] = r; nm++; }
	const size_t n_prim = nm;
	for (size_t r = 0; r < n && n_alt; r++) { /* placements 1 .. T - 1: the rest of the first hit's rows, then the later hits' */
		if (alt_off[r + 1] == alt_off[r]) continue;
		const bwb_aln *e = alns->alns + alns->aln_off[r];
		uint64_t left = alt_off[r + 1] - alt_off[r];
		for (uint64_t h = 0; left; h++)
			for (uint64_t row = e[h].L + (h == 0); row <= e[h].U && left; row++, left--) rows[nm++] = row;
	}
	if (nm) {
		const int ndev = bwb_hip_device_count();
		if (ndev < 1) bwb_die("alns2sam: no HIP device found (SA lookups run on the GPU)");
		if (n_gpus < 1) n_gpus = 1;
		if (n_gpus > ndev) bwb_die("alns2sam: -g %d asked for, %d HIP device(s) available", n_gpus, ndev);
		if ((size_t)n_gpus > nm) n_gpus = (int)nm;
		locate_job_t jobs[64];
		pthread_t th[64];
		if (n_gpus > 64) n_gpus = 64;
		for (int g = 0; g < n_gpus; g++) { /* contiguous shares, like the read chunks of align (inexact_match.c:115-116) */
			const size_t lo = (size_t)g * nm / (size_t)n_gpus, hi = (size_t)(g + 1) * nm / (size_t)n_gpus;
			jobs[g] = (locate_job_t){ .device = g, .BWT = BWT, .rows = rows + lo, .pos = pos + lo, .n = hi - lo };
			if (pthread_create(&th[g], NULL, locate_worker, &jobs[g])) bwb_die("alns2sam: cannot start a host thread");
		}
		for (int g = 0; g < n_gpus; g++) pthread_join(th[g], NULL);
		uint64_t steps = 0; double kms = 0;
		for (int g = 0; g < n_gpus; g++) { steps += jobs[g].steps; if (jobs[g].kernel_ms > kms) kms = jobs[g].kernel_ms; }
		printf("SA lookups on the GPU: rows %zu  rank-block visits %llu  kernel %.3f ms  (%.2f G visits/s)\n", nm, (unsigned long long)steps, kms, kms > 0 ? steps / kms / 1e6 : 0.0);
	}
	uint64_t *ref_pos = (uint64_t *)calloc(n ? n : 1, 8);
	for (size_t k = 0; k < n_prim; k++) ref_pos[which[k]] = pos[k];
	for (size_t r = 0, k = n_prim; r < n && n_alt; r++) { /* the items, beside place_from_alns below: the same walk over the same rows */
		if (alt_off[r + 1] == alt_off[r]) continue;
		const bwb_aln *e = alns->alns + alns->aln_off[r];
		uint64_t q = alt_off[r];
		for (uint64_t h = 0; q < alt_off[r + 1]; h++)
			for (uint64_t row = e[h].L + (h == 0); row <= e[h].U && q < alt_off[r + 1]; row++, q++) alt_from_aln(&e[h], (unsigned)h, pos[k++], BWT->length, &alts[q]);
	}
	/* eval_aln for every read, then the text */
	bwb_place *pl = (bwb_place *)malloc((n ? n : 1) * sizeof(bwb_place));
#pragma omp parallel for schedule(static) num_threads(bwb_host_team())
	for (long r = 0; r < (long)n; r++)
		place_from_alns(alns->alns + alns->aln_off[r], alns->aln_off[r + 1] - alns->aln_off[r], ref_pos[r], BWT->length, o->max_mm, &pl[r]);
	const int ann_sorted = T.ann_sorted;
	sam_reads_t rd = sam_reads_of(reads, n, pl, alt_off, alts);
	host_recs_t own;
	host_chain(&rd, n, &T, o, text, NULL, alns->alns, alns->aln_off, 1, &own); /* (-J: an item's suboptimal byte from the hits' scores) */
	/* The text: blocks of reads are formatted into memory by all cores and written in order (round 5: one thread's fprintf calls were
	 * the wall time of aln2sam on a 10 M-read file, not the SA lookups). */
	const size_t BLK = SAM_BLOCK_READS;
	const size_t nblk = (n + BLK - 1) / BLK;
	const size_t WAVE = 64; /* blocks formatted before the writer writes them */
	char **bufs = (char **)calloc(WAVE, sizeof(char *));
	size_t *lens = (size_t *)calloc(WAVE, sizeof(size_t));
	for (size_t b0 = 0; b0 < nblk; b0 += WAVE) {
		const size_t nb_ = nblk - b0 < WAVE ? nblk - b0 : WAVE;
#pragma omp parallel for schedule(dynamic, 1) num_threads(bwb_host_team())
		for (long bi = 0; bi < (long)nb_; bi++) {
			const size_t r0 = (b0 + (size_t)bi) * BLK, r1 = r0 + BLK < n ? r0 + BLK : n;
			bufs[bi] = sam_format_reads(&rd, r0, r1, ann, ann_sorted, &lens[bi]);
		}
		for (size_t bi = 0; bi < nb_; bi++) {
			if (lens[bi] && fwrite(bufs[bi], 1, lens[bi], sam) != lens[bi]) bwb_die("alns2sam: Cannot write to the SAM file: %s!", samFname);
			free(bufs[bi]); bufs[bi] = NULL;
		}
	}
	free(bufs); free(lens);
	printf("Processed %zu reads.\n", n);
	free(rows); free(pos); free(which); free(ref_pos);
	free(bwtFname); free(annFname);
	fclose(sam);
	host_tail(&out, &rd, n, &T, text);
	free(pl); free(alt_off); free(alts);
	host_recs_free(&own); host_tables_free(&T); host_outs_free(&out); md_text_free(text);
	free_bwt(BWT); free_reads(reads); free_alns_batch(alns); free_ann(ann);
}

/* developer command (CPU only, for the tests): raw bwb_place records from a file through the host's chain and sam_format_reads - the formatter
 * `map` uses, on a machine without a GPU */
void places2sam(char *fastaFname, char *readsFname, char *placesFname, char *samFname, char *altsFname, const map_opts_t *o) {
	host_outs_t out;
	host_outs_open(&out, o);
	size_t Ln = strlen(fastaFname) + 8;
	char *annFname = (char *)malloc(Ln);
	snprintf(annFname, Ln, "%s.ann", fastaFname);
	fasta_annotations_t *ann = annf2ann(annFname);
	host_tables_t T;
	host_tables_load(&T, ann, o, out.indel != NULL);
	md_text_t *text = host_text_open(fastaFname, o, &out, 0);
	reads_t *reads = fastq2reads(readsFname);
	FILE *pf = fopen(placesFname, "rb");
	if (!pf) { perror(placesFname); bwb_die("places2sam: Cannot open the placements file: %s!", placesFname); }
	bwb_place *pl = (bwb_place *)malloc(((size_t)reads->count ? reads->count : 1) * sizeof(bwb_place));
	const size_t got = fread(pl, sizeof(bwb_place), reads->count, pf);
	fclose(pf);
	const size_t n = got < reads->count ? got : reads->count;
	/* optional: u64 alt_off[n + 1], then alt_off[n] bwb_alt records (what slot_place_alt returns) - the X tags */
	uint64_t *alt_off = NULL;
	bwb_alt *alts = NULL;
	uint8_t *alt_sub = NULL; /* -J: behind the records, one byte per item - not zero: the item is suboptimal */
	if (altsFname) {
		FILE *af = fopen(altsFname, "rb");
		if (!af) { perror(altsFname); bwb_die("places2sam: Cannot open the alternatives file: %s!", altsFname); }
		alt_off = (uint64_t *)malloc((n + 1) * 8);
		if (fread(alt_off, 8, n + 1, af) != n + 1) bwb_die("places2sam: %s is shorter than %zu + 1 offsets", altsFname, n);
		for (size_t r = 0; r < n; r++) if (alt_off[r + 1] < alt_off[r]) bwb_die("places2sam: %s: the offsets do not ascend", altsFname);
		alts = (bwb_alt *)malloc((alt_off[n] ? alt_off[n] : 1) * sizeof(bwb_alt));
		if (alt_off[0] != 0 || fread(alts, sizeof(bwb_alt), alt_off[n], af) != alt_off[n]) bwb_die("places2sam: %s does not hold the records its offsets name", altsFname);
		if (o->join) {
			alt_sub = (uint8_t *)malloc(alt_off[n] ? alt_off[n] : 1);
			if (fread(alt_sub, 1, alt_off[n], af) != alt_off[n]) bwb_die("places2sam: %s does not hold one suboptimal byte per item behind its records (-J)", altsFname);
		}
		fclose(af);
	}
	FILE *sam = fopen(samFname, "w");
	if (!sam) { perror(samFname); bwb_die("places2sam: Cannot open SAM file: %s!", samFname); }
	sam_write_header(sam, ann);
	sam_reads_t rd = sam_reads_of(reads, n, pl, alt_off, alts);
	host_recs_t own;
	host_chain(&rd, n, &T, o, text, alt_sub, NULL, NULL, 0, &own);
	for (size_t r0 = 0; r0 < n; r0 += SAM_BLOCK_READS) {
		size_t len = 0;
		char *buf = sam_format_reads(&rd, r0, r0 + SAM_BLOCK_READS < n ? r0 + SAM_BLOCK_READS : n, ann, T.ann_sorted, &len);
		if (len && fwrite(buf, 1, len, sam) != len) bwb_die("places2sam: Cannot write to the SAM file: %s!", samFname);
		free(buf);
	}
	printf("Processed %zu reads.\n", n);
	fclose(sam);
	host_tail(&out, &rd, n, &T, text);
	free(pl); free(annFname); free(alt_off); free(alts); free(alt_sub);
	host_recs_free(&own); host_tables_free(&T); host_outs_free(&out); md_text_free(text);
	free_reads(reads); free_ann(ann);
}
