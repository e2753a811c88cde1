/*
 * bwb_host.h - host side (C) of the MI355X BWBBLE aligner: the reference's own data types and
 * entry points for the `index | align | aln2sam` path, re-implemented from scratch, with the
 * alignment loop handed to libbwbble_hip.so through include/bwbble_hip.h.
 *
 * Names follow the reference (mg-aligner/{bwt.h,io.h,align.h,inexact_match.h}) so that the seam is
 * obvious: align_reads_inexact_gpu_stream() stands where align_reads_inexact_parallel() (inexact_match.h:40) is
 * selected in align_reads() (align.c:72-76); it takes the FASTQ's NAME instead of the loaded reads_t - the file is streamed
 * through a reader thread while the index is still on its way to the GPU (align_gpu.c).  The drop-in binding with the
 * reference's exact signature, for a maintainer who keeps the reference's host code, is integration/align_gpu.c.
 */
#ifndef BWB_HOST_H
#define BWB_HOST_H
#include <stdint.h>
#include <stdlib.h>
#include <unistd.h>
#include <stdio.h>
#include "bwbble_hip.h"

typedef uint64_t bwtint_t;

#define OCC_INTERVAL 128        /* bwt.h:14 */
#define SA_INTERVAL 32          /* bwt.h:16 */
#define ALPHABET_SIZE 16        /* io.h:27 */
#define MAX_SEQ_NAME_LEN 256    /* io.h:10 */

/* bwt_t (bwt.h:19-40) minus the 64 K-entry LUT (popcounts are used instead) */
typedef struct {
	bwtint_t length, num_words;
	uint32_t *bwt;
	bwtint_t C[ALPHABET_SIZE + 1];
	bwtint_t *O;
	bwtint_t num_occ;
	bwtint_t *SA;
	bwtint_t num_sa;
	bwtint_t sa0_index;
	/* load_bwt_start: the arrays are filled by loader threads while the GPUs already take the index in */
	volatile uint64_t blocks_ready;   /* leading 128-character blocks whose bwt words and O rows are in memory (release/acquire) */
	void *loader;                     /* opaque: the loader threads (NULL: everything is loaded) */
	double load_seconds;              /* load_bwt_start to the last byte of the file in memory */
	volatile int sa_ready;            /* loadSA: SA is in memory (release/acquire; the loader reads it first - `map` uploads it before the chunk pool is sized) */
} bwt_t;

/* reads_t/read_t (io.h:151-194) in structure-of-arrays form: codes are read->seq (A0 G1 C2 T3 N4) */
typedef struct {
	unsigned int count, max_len;
	uint32_t stride;            /* bytes per read in seq */
	uint8_t *seq;               /* [count][stride] */
	uint16_t *len;
	char *raw;                  /* the FASTQ text; names and qualities point into it */
	size_t *name_off, *qual_off;
	uint16_t *name_len;
} reads_t;

typedef struct {                /* seq_annotation_t / fasta_annotations_t (io.h:196-207) */
	char name[MAX_SEQ_NAME_LEN + 1];
	bwtint_t start_index, end_index;
} seq_annotation_t;
typedef struct { int num_seq; seq_annotation_t *seq_anns; } fasta_annotations_t;

typedef bwb_params aln_params_t; /* align.h:48-79 */

/* alignments of a batch as loaded from / written to .aln (align.c:345-382,430-483) */
typedef struct {
	size_t n_reads;
	uint64_t *aln_off;          /* n_reads + 1 */
	bwb_aln *alns;
} alns_batch_t;

void bwb_die(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));

/* bwt_io.c */
void store_bwt(const bwt_t *BWT, const char *bwtFname);                /* bwt.c:66-82 */
bwt_t *load_bwt(const char *bwtFname, int loadSA);                     /* bwt.c:90-125 */
double bwt_load_seconds(const bwt_t *B);
bwt_t *load_bwt_start(const char *bwtFname, int loadSA);               /* returns after the header: the arrays fill in the background (blocks_ready) */
bwt_t *load_bwt_start_job(const char *bwtFname, int loadSA, void (*job)(void *), void *job_arg); /* the same; one loader thread also runs job(job_arg) behind the sampled SA (`map -D`: md_text_read) */
void load_bwt_wait(bwt_t *BWT);                                        /* until the whole file is in memory */
void free_bwt(bwt_t *BWT);

/* index.c */
int index_bwt(const char *fastaFname, const char *extSAFname);         /* bwt.c:29-63 */
void fasta2ref(const char *fastaFname, const char *refFname, const char *annFname, unsigned char **seq, bwtint_t *totalSeqLen); /* io.c:190-321 */
bwt_t *construct_bwt(unsigned char *seq, bwtint_t length, const char *extSAFname); /* bwt.c:161-218; extSAFname: esa2bwt bwt.c:132-158 */
fasta_annotations_t *annf2ann(const char *annFname);                   /* io.c:324-349 */
void free_ann(fasta_annotations_t *a);

/* reads.c */
reads_t *fastq2reads(const char *readsFname);                          /* io.c:410-515 */
void free_reads(reads_t *reads);
/* the same parser as a stream: `align` takes the FASTQ in chunks, chunk k+1 is parsed while chunk k is on the GPUs */
typedef struct fq_stream fq_stream;
typedef struct {
	uint32_t n, stride, max_len;  /* reads in the chunk; bytes per read in seq (the chunk's longest read, at least 1) */
	uint8_t *seq;                 /* [n][stride] read->seq codes (A0 G1 C2 T3 N4), malloc'ed: the consumer frees it */
	uint16_t *len;                /* [n], malloc'ed */
	/* only from a stream opened with fq_open_text (`map`; NULL otherwise): where each read's name and qualities lie in `text`, the stream's
	 * mapping of the FASTQ - valid until fq_close, so the stream stays open until the last chunk's SAM text is formatted */
	const char *text;
	size_t *name_off, *qual_off;  /* [n], malloc'ed */
	uint16_t *name_len;           /* [n], malloc'ed (at most MAX_SEQ_NAME_LEN, io.c:439) */
} fq_chunk_t;
fq_stream *fq_open(const char *readsFname);
fq_stream *fq_open_text(const char *readsFname);                       /* the same; its chunks also carry name / quality offsets */
int fq_next_chunk(fq_stream *s, uint32_t max_reads, fq_chunk_t *out); /* 0 at the end of the file */
void fq_close(fq_stream *s);

/* aln_io.c */
void alns2alnf_bin(const bwb_aln *alns, uint64_t n, FILE *alnFile);    /* align.c:345-382, one read */
unsigned char *alns2alnf_buf(const bwb_aln *alns, const uint64_t *aln_off, uint32_t n_reads, size_t *len); /* the same bytes for a chunk of reads, as one buffer */
alns_batch_t *alnsf2alns_bin(const char *alnFname);                    /* align.c:430-483 */
void free_alns_batch(alns_batch_t *b);
int aln_path_bytes(const bwb_aln *a, unsigned char *path /* >= 272 bytes */); /* edit path from the gap runs; returns aln_length */

/* align_gpu.c */
/* reads per GPU batch (BWB_CHUNK).  Batches are streamed as slices that park their unfinished reads for the next slice, so the
 * size no longer decides how much of the GPU idles at the end of a batch; it trades launch overhead against the balance
 * between GPUs and the memory of a slot (about 1 KB per read).
 * Test knobs beside it: BWB_FQ_REGION (reads.c: bytes per region of the FASTQ scan) and BWB_COUNT_PIECE (align_gpu.c: the sites of -A, or the
 * bubbles of -I, whose counters a worker of `map` reads back at a time; default 2^20, a value below 1 is 1). */
#define GPU_CHUNK_DEFAULT (1u << 21)
void set_default_aln_params(aln_params_t *params);                     /* align.c:22-38 */
int align_reads(char *fastaFname, char *readsFname, char *alnsFname, aln_params_t *params, int n_gpus); /* align.c:40-87 */
int align_reads_inexact_gpu_stream(bwt_t *BWT, const char *readsFname, aln_params_t *params, char *alnFname, int n_gpus); /* the GPU's align_reads_inexact_parallel (inexact_match.h:40) over a streamed FASTQ */
/* what the command line asks of the result stream: `map`, `aln2sam` and `places2sam` share the record; main.c fills it letter by letter
 * (map_option) and checks and completes it (map_opts_finish) before any of them runs */
typedef struct {
	int max_mm;                  /* map -Q, aln2sam -n: the mismatch count at which a unique hit gets MAPQ 25 (6; places2sam has no flag for it) */
	int max_alt;                 /* -X: 1..255, X0:i / X1:i and up to that many other placements as XA:Z: (0: no tags) */
	const char *bubbleFname;     /* -B: the bubble table, bubble.data - the tags bC:Z: / bP:Z: (NULL: no tags) */
	int join;                    /* -J: a read's placements counted by locus, MAPQ without the joined ones and the tag bJ:i:; needs -X and -B */
	int lift;                    /* -R: placements on a bubble record written in chromosome coordinates, the tag bO:Z:; needs -B */
	int md;                      /* -D: the tags NM:i / MD:Z against the text of <seq_fasta>.ref */
	const char *countsFname;     /* -A: the file of the allele counts at the text's IUPAC sites (NULL: no counts) */
	int min_mapq;                /* -a: the least MAPQ that -A, -I and -G count, 0..255 (-1 until finished: not given, then 0) */
	const char *indelFname;      /* -I: the file of the read support per indel bubble (NULL: no table); needs -B */
	int anchor;                  /* -w: the flank bases a read must cover on either side for -I and -G, 1..255 (0 until finished: not given, then 1) */
	int min_baseq;               /* -b: the least base quality that -A and -G count, 0..93 (-1 until finished: not given, then 0) */
	int weighted;                /* -Y: the genotype calls of -G weighted by the base qualities, the column QS; needs -G */
	const char *genoFname;       /* -G: the file of the genotype calls from both tables (NULL: no calls) */
	int geno_err;                /* -q: the error phred of -G, 4..93 (0 until finished: not given, then 20) */
	int64_t geno_depth;          /* -d: the minimum depth of a call of -G, 1..2^31 - 1 (0 until finished: not given, then 1) */
} map_opts_t;
int map_reads(char *fastaFname, char *readsFname, char *samFname, aln_params_t *params, const map_opts_t *opts, int n_gpus); /* `bwbble map`: align + aln2sam in one pass, the hits evaluated on the GPU */

/* precalc.c */
void precalc_sa_intervals(bwt_t *BWT, const aln_params_t *params, const char *preFname); /* align.c:200-224: writes <fasta>.pre */
int check_precalc_file(const char *preFname); /* the walk of load_precalc_sa_intervals (align.c:226-238) over an existing table: 0 = complete */

/* sam.c */
void alns2sam(char *fastaFname, char *readsFname, char *alnsFname, char *samFname, int is_multiref, int n_gpus, const map_opts_t *opts); /* align.c:494-556 */
/* the two halves of alns2sam: eval_aln of one read on the host, and the text of a block of reads from placement records (which `map` gets
 * from the GPU instead, bwb_hip_slot_place) */
#define SAM_BLOCK_READS ((size_t)1 << 14)                              /* reads formatted by one thread at a time */
typedef struct {
	const bwb_place *pl;                                               /* [n] */
	const uint8_t *seq; uint32_t stride; const uint16_t *len;          /* read->seq codes */
	const char *text; const size_t *name_off, *qual_off; const uint16_t *name_len; /* names and qualities: offsets into text */
	size_t first;                                                      /* number of read 0 in the file (error messages) */
	const uint64_t *alt_off; const bwb_alt *alts;                      /* -X (NULL: no tags): read r's other placements are alts[alt_off[r] .. alt_off[r + 1]) */
	const bwb_locus *loci; const struct bubble_table *bubbles;         /* -B (NULL: no tags): read r's record and POS come from loci[r], and on a bubble record the tags bC / bP */
	const bwb_join *joins;                                             /* -J (NULL: pl's MAPQ, no tag): read r's MAPQ comes from joins[r], and with joined items the tag bJ */
	/* -R (lift_kind NULL: as placed): placement q - read q's primary, or lift_n + k for item alts[k] - with lift_kind[q] == BWB_LIFT_LIFTED prints
	 * RNAME, POS and CIGAR of the record at lift_recs + lift_off[q], and a lifted primary the tag bO */
	const uint8_t *lift_kind; const uint64_t *lift_off; const bwb_lift *lift_recs; size_t lift_n;
	/* -D (md NULL: no tags): read r with md[r].kind == BWB_MD_OK gains NM:i:md[r].nm and MD:Z: with the bytes md_text[md_off[r] .. md_off[r + 1]), behind QUAL */
	const bwb_md *md; const uint64_t *md_off; const char *md_text;
} sam_reads_t;
int sam_mapq(int top1, int top2, int num_mm, int max_mm);               /* align.c:738-746 */
void place_from_alns(const bwb_aln *e, uint64_t ne, uint64_t ref_pos, uint64_t bwt_length, int max_mm, bwb_place *out);
void alt_from_aln(const bwb_aln *e, unsigned hit, uint64_t ref_pos, uint64_t bwt_length, bwb_alt *out); /* one of the other placements, from its hit and SA(its row) */
uint64_t alt_placements(const bwb_aln *e, uint64_t ne);               /* the rows of all hits: 64-bit, saturating */
void sam_write_header(FILE *sam, const fasta_annotations_t *ann);
int sam_ann_sorted(const fasta_annotations_t *ann);
char *sam_format_reads(const sam_reads_t *rd, size_t r0, size_t r1, const fasta_annotations_t *ann, int ann_sorted, size_t *out_len);
void places2sam(char *fastaFname, char *readsFname, char *placesFname, char *samFname, char *altsFname, const map_opts_t *opts); /* developer command: records from a file (altsFname: NULL or the items; with -J the items file ends with one suboptimal byte per item) */

/* pad.c: bubble hits in reference coordinates (the reference's mg-ref/sam_pad.cpp) */
typedef struct bubble_table {                                          /* bubble.data (mg-ref/comb.cpp:245-253): the k-th pair of lines is bubble k */
	int64_t n;
	bwb_bubble *b;                                                     /* [n] */
	char **ann;                                                        /* [n] the chromosome header as comb wrote it: the bC tag */
} bubble_table_t;
bubble_table_t *load_bubbles(const char *dataFname);                   /* sam_pad.cpp:27-45; half a pair or a numbers line without six integers is refused */
void free_bubbles(bubble_table_t *t);
int64_t bubble_number(const char *name);                               /* sam_pad.cpp:67-72: -1 unless the name starts with "bubble" */
int32_t *ann_bubble_of(const fasta_annotations_t *ann, const bubble_table_t *t); /* [num_seq] bubble_number of every record (malloc'ed); one outside the table is refused */
void bubble_locus(const bwb_bubble *b, int64_t locus, bwb_locus *out); /* sam_pad.cpp:75-87: kind, ref_lo, ref_hi */
int ann_find_record(const fasta_annotations_t *ann, int ann_sorted, uint64_t aln_pos); /* the record that contains aln_pos, -1: none */
void locus_resolve(const bwb_place *pl, const fasta_annotations_t *ann, int ann_sorted, const int32_t *bubble_of, const bubble_table_t *t, bwb_locus *out); /* kernel k_locus on the host */
char *locus_put_tags(char *o, const bwb_locus *lc, const bubble_table_t *t);
int32_t *bubble_chrom_of(const fasta_annotations_t *ann, const int32_t *bubble_of, const bubble_table_t *t, const char *flag); /* -J, -R (flag: the one the message names): [t->n] the chromosome's record of every bubble (malloc'ed); none, several or a bubble record is refused */
void join_resolve(const bwb_place *pl, const bwb_locus *lc, const bwb_alt *items, const uint8_t *sub, uint64_t n_items, const fasta_annotations_t *ann, int ann_sorted,
                  const int32_t *bubble_of, const int32_t *chrom_of, const bubble_table_t *t, int max_mm, bwb_join *out); /* kernels k_join_items + k_join_reads on the host, one read */
/* -R: placements on a bubble record in chromosome coordinates (include/bwbble_hip.h: bwb_lift) */
const char *lift_bubble_refusal(const bwb_bubble *b);                  /* NULL, or why the rule refuses the bubble */
void lift_check_table(const bubble_table_t *t);                        /* a refused bubble stops the run and is named */
int lift_resolve(const bwb_bubble *b, int32_t chrom, int64_t pos1, int reverse, unsigned alen, const uint16_t *gap_run, bwb_lift *hdr, uint32_t *ops /* BWB_LIFT_MAX_OPS */); /* kernels k_lift_count + k_lift on the host, one placement; returns the ops, 0: not liftable */
typedef struct { uint8_t *kind; uint64_t *off; bwb_lift *recs; uint64_t n_lifted, n_unliftable; } lift_set_t; /* what bwb_hip_slot_lift returns, malloc'ed */
lift_set_t *lift_host(const bwb_place *pl, const bwb_locus *loci, size_t n, const uint64_t *alt_off, const bwb_alt *alts, const fasta_annotations_t *ann, int ann_sorted,
                      const int32_t *bubble_of, const int32_t *chrom_of, const bubble_table_t *t);
void lift_free(lift_set_t *ls);
/* the op of text position t of a placement's CIGAR: the path byte aln_path_bytes gives (a later run wins), walked as sam_put_cigar walks it
 * (lift_resolve and md_place_ops) */
static inline unsigned lift_op_at(const uint16_t *gap_run, unsigned alen, int reverse, unsigned t) {
	const unsigned p = reverse ? t : alen - 1 - t;
	unsigned op = 0;
	for (int k = 0; k < BWB_MAX_GAP_RUNS; k++) {
		const unsigned run = gap_run[k];
		if (run != 0xFFFFu && p - (run & 0xFFu) < ((run >> 8) & 0x7Fu)) op = (run >> 15) ? BWB_LIFT_D : BWB_LIFT_I;
	}
	return op;
}

/* md.c: -D, NM:i and MD:Z against the text of <seq_fasta>.ref (include/bwbble_hip.h: bwb_md) */
typedef struct md_text { uint8_t *codes; uint64_t n_fwd; double seconds; char *refFname; volatile int ready; const char *flag; } md_text_t; /* the forward text, one code per byte; ready: the bytes are in memory (release/acquire) */
md_text_t *md_text_open(const char *fastaFname, int deferred);        /* a missing .ref or one that is not 2 x n_fwd bytes stops the run and names `bwbble fasta2ref`; deferred: the bytes are not read here but by md_text_read */
md_text_t *md_text_open_for(const char *fastaFname, int deferred, const char *flag); /* the same; flag: the option the messages name ("-D", "-A") */
void md_text_read(void *text);                                         /* reads the n_fwd bytes of a deferred text (a job of the .bwt loader: load_bwt_start_job) */
void md_text_wait(md_text_t *t);                                       /* until the n_fwd bytes are in memory */
void md_text_free(md_text_t *t);
unsigned md_place_ops(unsigned alen, const uint16_t *gap_run, int reverse, uint32_t *ops /* 2 * BWB_MAX_GAP_RUNS + 1 */); /* the printed CIGAR as ops of a lift record: len << 4 | op */
int md_resolve(const uint8_t *text, uint64_t n_fwd, const uint8_t *seq, unsigned len, int reverse, int64_t start, const uint32_t *ops, unsigned n_ops,
               bwb_md *rec, char *md, size_t cap); /* kernels k_md_count + k_md on the host, one read: seq as uploaded, the ops from text position start; md NULL: counted only; returns the kind */
typedef struct { bwb_md *recs; uint64_t *off; char *text; uint64_t n_ok, n_too_long; } md_set_t; /* what bwb_hip_slot_md returns, malloc'ed */
md_set_t *md_host(const bwb_place *pl, size_t n, const uint8_t *seq, uint32_t stride, const uint16_t *len, const uint8_t *lift_kind, const uint64_t *lift_off,
                  const bwb_lift *lift_recs, const fasta_annotations_t *ann, const md_text_t *t);
void md_free(md_set_t *ms);

/* pile.c: -A, allele counts at the text's IUPAC sites (include/bwbble_hip.h: bwb_hip_pile_begin) */
typedef struct pile {
	char *fname; FILE *f; int min_mapq;                               /* the counts file, open since before anything was loaded (NULL: none, a table in memory only); -a */
	const md_text_t *text; uint64_t n_sites; uint32_t *base;          /* the text, its sites, and - for pile_host - the sites below every 32 characters */
	uint32_t *counts; uint64_t reads, adds;                           /* n_sites x (A, C, G, T), wrapping; what pile_host has counted */
	int min_baseq, err_cap;                                           /* -b: the least base quality that counts, 0..93; -Y: -q's E, the cap of a base's weight (0: no -Y), set before pile_set_text */
	uint32_t *qsum; uint64_t dropped;                                 /* -Y (NULL: none): n_sites x (A, C, G, T) quality sums, wrapping; the bases -b has dropped in pile_host */
} pile_t;
pile_t *pile_open(const char *countsFname, int min_mapq);             /* a path that cannot be written stops the run; until pile_write has finished, a run that exits leaves no file */
void pile_set_text(pile_t *p, const md_text_t *t, int index);         /* counts the sites of the text in memory and makes the zeroed table; index: also what pile_host needs */
uint64_t pile_host(pile_t *p, const bwb_place *pl, size_t n, const uint8_t *seq, uint32_t stride, const uint16_t *len, const uint8_t *lift_kind, const uint64_t *lift_off,
                   const bwb_lift *lift_recs, const bwb_join *joins, const fasta_annotations_t *ann); /* kernel k_pile on the host: adds into the table, returns the reads counted (joins NULL: the placements' MAPQ) */
uint64_t pile_host_q(pile_t *p, const bwb_place *pl, size_t n, const uint8_t *seq, uint32_t stride, const uint16_t *len, const char *qtext, const size_t *qual_off,
                     const uint8_t *lift_kind, const uint64_t *lift_off, const bwb_lift *lift_recs, const bwb_join *joins, const fasta_annotations_t *ann); /* the same with the qualities, kernel k_pile_q on the host: read r's quality line is qtext + qual_off[r] (read only with -b above 0 or -Y) */
void pile_add(pile_t *p, uint64_t first, uint64_t n, const uint32_t *counts); /* adds a context's counters of n sites from `first` (bwb_hip_pile_counts) */
void pile_add_q(pile_t *p, uint64_t first, uint64_t n, const uint32_t *sums); /* the same for its quality sums (bwb_hip_pileq_sums) */
uint64_t pile_write(pile_t *p, const fasta_annotations_t *ann);       /* the header line and one line per site with a counter that is not zero; closes the file; returns the lines */
void pile_free(pile_t *p);

/* indel.c: -I, ref / alt read support per indel bubble (include/bwbble_hip.h: bwb_hip_indel_begin) */
typedef struct { int64_t lo; int32_t chrom; uint32_t bubble; } indel_entry_t; /* an eligible bubble: A + Bm - w, chrom_of, its number */
typedef struct indel {
	char *fname; FILE *f; int min_mapq, anchor;                       /* the file, open since before anything was loaded (NULL: none, a table in memory only); -a; -w */
	const bubble_table_t *bub; uint8_t *elig;                         /* the bubble table and, per bubble, whether it is eligible at this anchor */
	indel_entry_t *tab; uint64_t n_tab, n_refused; double sort_s;     /* the eligible bubbles ascending by (chrom, lo, bubble); the bubbles lift_bubble_refusal refuses; qsort's seconds */
	uint32_t *counts; uint64_t reads, adds, cands;                    /* n x (ref, alt, ref_gapped, alt_gapped), wrapping; what indel_host has counted */
} indel_t;
indel_t *indel_open(const char *indelFname, int min_mapq, int anchor); /* a path that cannot be written stops the run; until indel_write has finished, a run that exits leaves no file */
int indel_eligible(const bwb_bubble *b, int anchor);
void indel_set_table(indel_t *p, const bubble_table_t *t, const int32_t *chrom_of); /* the sorted table of the eligible bubbles and the zeroed counters */
unsigned indel_resolve(int64_t pos1, int reverse, unsigned alen, const uint16_t *gap_run, int64_t lo, int64_t hi); /* one placement against one window: 0 not covering, 1 clean, 2 gapped */
uint64_t indel_host(indel_t *p, const bwb_place *pl, const bwb_locus *loci, size_t n, const uint16_t *len, const bwb_join *joins); /* kernel k_indel on the host: adds into the table, returns the reads counted (joins NULL: the placements' MAPQ) */
void indel_add(indel_t *p, uint64_t first, uint64_t n, const uint32_t *counts); /* adds a context's counters of n bubbles from `first` (bwb_hip_indel_counts) */
uint64_t indel_write(indel_t *p);                                     /* the header line and one line per bubble with a counter that is not zero; closes the file; returns the lines */
void indel_free(indel_t *p);

/* geno.c: -G, genotype calls at the IUPAC sites and the indel bubbles (include/bwbble_hip.h: bwb_hip_geno_begin) */
typedef struct geno {
	char *fname; FILE *f; int err; int64_t min_depth;                  /* the calls file, open since before anything was loaded (NULL: none, records in memory only); -q; -d */
	bwb_geno_site *sites; uint64_t n_sites, cap_sites;                /* the called sites' records, in site order */
	int weighted; uint32_t *qs;                                       /* -Y: the weighted rule and the column QS; the sites' quality sums, four per record of `sites` */
	bwb_geno_bubble *bubs; uint64_t n_bubs, cap_bubs;                 /* the called bubbles' records, in bubble order */
	int worker; uint64_t pieces, put_pieces; double kernel_ms, put_s, call_s; /* map: the worker that called, its geno_sites / geno_bubbles calls, its pile_put / indel_put calls, the kernels' time summed, the seconds of both */
} geno_t;
geno_t *geno_open(const char *genoFname, int err, int64_t min_depth); /* a path that cannot be written stops the run; until geno_write has finished, a run that exits leaves no file */
void geno_rule(const uint32_t *n, unsigned k, uint64_t depth, unsigned err, uint8_t *gt, uint8_t *gq, uint32_t *pl /* 6 */); /* the rule from the k = 2 or 3 alleles' counts and the depth */
void geno_rule_q(const uint32_t *n, const uint32_t *s, unsigned k, uint64_t S, uint8_t *gt, uint8_t *gq, uint32_t *pl /* 6 */); /* -Y: the weighted rule from the alleles' counts and quality sums and the sum of all four columns */
void geno_take_sites(geno_t *g, const bwb_geno_site *recs, uint64_t n); /* keeps a piece's records for the writer (bwb_hip_geno_sites) */
void geno_take_sites_q(geno_t *g, const bwb_geno_site_q *recs, uint64_t n); /* -Y: the same with the records' quality sums (bwb_hip_geno_sites_q) */
void geno_take_bubbles(geno_t *g, const bwb_geno_bubble *recs, uint64_t n); /* (bwb_hip_geno_bubbles) */
void geno_host(geno_t *g, const pile_t *pile, const indel_t *indel);  /* the geno kernels on the host: the same records from the host's tables (either may be NULL) */
uint64_t geno_write(geno_t *g, const fasta_annotations_t *ann, const bubble_table_t *bub); /* the header line, the called sites, the called bubbles (bub NULL: none); closes the file; returns the lines */
void geno_free(geno_t *g);
void sam_pad(const char *dataFname, const char *inFname, const char *outFname); /* `bwbble sampad`: sam_pad.cpp:47-94 over SAM text */

/* host_chain.c: the host's rules behind the placement records, stage by stage - loci, joins, lifts, NM / MD, then the tables of -A, -I and -G.
 * `aln2sam` and `places2sam` run the whole chain; `map` runs a stage here where it cannot run it on the GPU (align_gpu.c).  The chunk's or
 * file's records ride in a sam_reads_t: a stage reads what the stages before it put there. */
typedef struct { pile_t *pile; indel_t *indel; geno_t *geno; } host_outs_t; /* the output trio; -G keeps the tables of -A and (with -B) -I in memory without their files */
void host_outs_open(host_outs_t *out, const map_opts_t *opts);       /* before anything is loaded: a path that cannot be written stops the run */
void host_outs_free(host_outs_t *out);
/* the text of <seq_fasta>.ref that -D, -A and -G need (NULL: none of them), named after the first of them in its messages: a missing .ref, or one of
 * another size than the .ann says, stops the run; deferred: md_text_open's */
md_text_t *host_text_open(const char *fastaFname, const map_opts_t *opts, const host_outs_t *out, int deferred);
typedef struct {                                                     /* what the rules resolve against */
	const fasta_annotations_t *ann; int ann_sorted;
	bubble_table_t *bub;                                              /* -B (NULL: none) */
	int32_t *bubble_of, *chrom_of;                                    /* every .ann record's bubble number; -J, -R, -I, -G with -B: the chromosome's record of every bubble (NULL: not needed) */
} host_tables_t;
void host_tables_load(host_tables_t *T, const fasta_annotations_t *ann, const map_opts_t *opts, int indel); /* aln2sam, places2sam: the table, the records' bubbles, -R's check, the bubbles' chromosomes (indel: a table of -I is kept) */
void host_tables_free(host_tables_t *T);                             /* (not ann: the caller's) */
typedef struct { bwb_locus *loci; bwb_join *joins; lift_set_t *lift; md_set_t *md; } host_recs_t; /* what the host's stages allocated for a sam_reads_t */
void host_recs_free(host_recs_t *own);
bwb_locus *host_loci(const sam_reads_t *rd, size_t n, const host_tables_t *T); /* -B: the locus record of every placement record, with all cores (malloc'ed) */
/* -J: the join record of every read, with all cores (malloc'ed).  sub: one byte per item, not zero for a suboptimal one; NULL: from the reads'
 * hits - read r's are hits[hit_off[r] ..) - an item is suboptimal when its hit's score is greater than the first hit's (align.c:771-779) */
bwb_join *host_joins(const sam_reads_t *rd, size_t n, const host_tables_t *T, int max_mm, const uint8_t *sub, const bwb_aln *hits, const uint64_t *hit_off);
void sam_reads_set_lift(sam_reads_t *rd, const lift_set_t *ls);     /* -R's records into the carrier, whose lift_n is its number of reads (NULL: as placed) */
void sam_reads_set_md(sam_reads_t *rd, const md_set_t *ms);          /* -D's (NULL: no tags) */
/* the four stages in order, as the options ask; rd gains the records, own what has to be freed.  sub / hits / hit_off: host_joins's; log: the lines of -R and -D */
void host_chain(sam_reads_t *rd, size_t n, const host_tables_t *T, const map_opts_t *opts, const md_text_t *text, const uint8_t *sub, const bwb_aln *hits, const uint64_t *hit_off, int log, host_recs_t *own);
/* the tail, when the SAM file is complete: the host's rules of -A and -I on the same records, the calls of -G from both tables, each file written and its log line */
void host_tail(host_outs_t *out, const sam_reads_t *rd, size_t n, const host_tables_t *T, const md_text_t *text);

/* The OpenMP teams of the host stages of `align` / `aln2sam` (base encoding, .aln serialisation, SAM text) have at most 32 threads unless
 * OMP_NUM_THREADS says otherwise: on the GPU box (2 x 64 cores, 256 hardware threads) a team of 256 - every hardware thread spinning in
 * libgomp's barriers next to its sibling - parsed 8.8 M reads/s and serialised 8.5 M records/s where 32 threads do 33 M and 240 M
 * (tools/r5_hostbox.sh, profiles/r5_host_stage_threads.txt), and `align -g 8` runs one serialising team per GPU worker.  A clause on
 * every region, not omp_set_num_threads(): the regions run in pthreads, which do not inherit the caller's setting.  `index` keeps the
 * default team. */
static inline int bwb_host_team(void) {
	const char *e = getenv("OMP_NUM_THREADS");
	if (e && atoi(e) > 0) return atoi(e);
	const long nc = sysconf(_SC_NPROCESSORS_ONLN);
	return nc < 1 ? 1 : (nc < 32 ? (int)nc : 32);
}

#endif
