/*
 * align_gpu.c - `bwbble align` driver: align_reads (mg-aligner/align.c:40-87) and the GPU replacement for
 * align_reads_inexact_parallel (mg-aligner/inexact_match.c:92-168).
 *
 * Same contract as the reference pair (inexact_match.h:39-40): the caller owns BWT, reads and params; one
 * .aln record per read is appended in input order (empty records included); returns 0; errors printf + exit(1).
 * The FM-index is replicated on every GPU; reads are cut into contiguous chunks that the per-GPU host threads
 * pull from a shared queue (the per-read work is heavy-tailed) and a writer emits them in order.
 * No collective is involved.  There is NO CPU alignment path: without a GPU this exits with an error.
 *
 * `bwbble map` (map_reads) is the same pipeline with another last stage: a finished chunk is not copied back hit by hit and serialised as
 * .aln records, its reads are evaluated on the GPU (bwb_hip_slot_place: eval_aln + mapq, one 48-byte record per read) and the worker's
 * team formats the chunk's SAM text (sam.c) - the bytes `align` + `aln2sam` write, from one process, one index load and no .aln file.
 */
#define _GNU_SOURCE
#include <pthread.h>
#include <sched.h>
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "bwb_host.h"

static double wall(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

void set_default_aln_params(aln_params_t *p) { bwb_default_params(p); } /* align.c:22-38 */

/* One chunk of the FASTQ on its way through the pipeline: parsed by the reader thread (several scanner threads: reads.c), aligned by one
 * of the GPU workers - which also turns the hits into the chunk's .aln bytes (aln_io.c: alns2alnf_buf) -, written by the main thread in
 * file order with one write per chunk. */
typedef struct chunk {
	size_t idx;
	fq_chunk_t fq;                 /* the reads (freed once the chunk is uploaded) */
	uint8_t *carry; uint32_t carry_len; /* the last read before the chunk that computes a D_seed (NULL: none), a copy */
	unsigned char *buf; size_t buf_len; uint32_t n; /* the chunk's .aln records, serialised by the worker that received its hits */
	char **sam; size_t *sam_len; size_t n_sam;      /* map: the chunk's SAM text instead, in blocks of SAM_BLOCK_READS reads */
	size_t first_read;                              /* number of the chunk's first read in the file */
	int ready;
	struct chunk *next;            /* production order */
} chunk_t;

/* what `map` adds to the pipeline (NULL: align) */
typedef struct {
	int max_mm; int max_alt /* -X (0: no tags) */; const fasta_annotations_t *ann; int ann_sorted;
	/* -B (bub NULL: no tags): the bubble table, every .ann record's bubble number, and - when the records are ascending and disjoint, so that
	 * kernel k_locus can search them (gpu_loci) - their first and last positions as the arrays bwb_hip_set_loci takes */
	const bubble_table_t *bub; const int32_t *bubble_of; int gpu_loci; const uint64_t *rec_start, *rec_end;
	const int32_t *chrom_of;  /* -J, -R (NULL: neither): the chromosome's record of every bubble; needs bub */
	int join;                 /* -J: a read's placements counted by locus; needs max_alt and bub */
	int lift;                 /* -R: placements on a bubble record written in chromosome coordinates; needs bub */
	md_text_t *text;          /* -D, -A (NULL: neither): the forward text of <seq_fasta>.ref */
	int md;                   /* -D: the tags NM:i / MD:Z against the text */
	pile_t *pile;             /* -A (NULL: no counts): the allele counts at the text's IUPAC sites; on the GPU unless pile_on_host */
	int pile_on_host;         /* -A with the host's lift or join records (-R / -J on an .ann that is not ascending and disjoint): the host's rule */
	indel_t *indel;           /* -I (NULL: no table): the read support per indel bubble; needs bub and chrom_of; on the GPU when gpu_loci, else the host's rule */
	geno_t *geno;             /* -G (NULL: no calls): the genotype calls from both tables - pile is there then, and with bub indel; each half on the GPU where its counters are */
} map_t;

typedef struct {
	pthread_mutex_t mu;
	pthread_cond_t cv_work, cv_done, cv_space;
	chunk_t *first, *last;         /* every chunk not yet written, in order */
	chunk_t *unclaimed;            /* the first chunk no worker has taken yet */
	size_t n_parsed, n_written, max_ahead;
	int reader_done;
	int n_workers, n_finished;     /* map -G: the workers, and those whose counters have all been summed on the host; the one that completes the count calls the genotypes */
	uint64_t n_reads;
	/* reader */
	const char *readsFname;
	const aln_params_t *params;
	uint32_t chunk_reads;
	double t_first_chunk;
	const map_t *map;
	fq_stream *fs;                 /* map: the open stream - the chunks' names and qualities point into its mapping of the FASTQ */
} pipe_t;

typedef struct {
	int gpu, device; /* worker number; HIP device it drives */
	bwt_t *BWT;
	aln_params_t *params;
	pipe_t *pp;
	bwb_stats total;
	double kernel_ms, t_ctx, t_pool, t_first_submit; /* index upload; the chunk pool's hipMalloc; worker start to the first slice queued */
	unsigned long long pool_bytes;
	unsigned long long n_reads; /* reads of the chunks this worker took */
	double place_ms; unsigned long long place_steps; /* map: k_place, summed over the chunks */
	double alt_ms; unsigned long long alt_steps, alt_items; /* map -X: k_alt_count + scan + k_place_alt, summed over the chunks */
	double locus_ms; unsigned long long locus_reads; /* map -B: k_locus, summed over the chunks */
	double join_ms; unsigned long long join_items, join_joined, join_mapq; /* map -J: k_join_items + k_join_reads, summed over the chunks; reads whose MAPQ changed */
	double lift_ms; unsigned long long lift_lifted, lift_unliftable, lift_bytes; /* map -R: k_lift_count + scan + k_lift, summed over the chunks; what came back for them */
	double md_ms, text_s; unsigned long long md_reads, md_bytes, md_back; /* map -D: k_md_count + scan + k_md, summed over the chunks; set_text's seconds; reads tagged, MD bytes, what came back */
	double pile_ms, pile_begin_s, pile_fetch_s; unsigned long long pile_reads, pile_adds; /* map -A: k_pile, summed over the chunks; pile_begin's and the final read-back's seconds; reads counted, adds */
	double indel_ms, indel_begin_s, indel_fetch_s; unsigned long long indel_reads, indel_adds, indel_cands; /* map -I: k_indel, summed over the chunks; indel_begin's and the final read-back's seconds; reads counted, adds, candidates */
} worker_t;

/* The reader: chunk k+1 is parsed (record boundaries by one sequential scan, bases encoded by all cores: reads.c) while chunk k is on
 * the GPUs.  It also names, for every chunk, the last read before it that computes a D_seed - longer than the seed, not dropped by
 * -P - whose bounds a short read at the head of the chunk sees, like in the reference's serial loop (inexact_match.c:35,62-65; the
 * look-back has no bound: the read is carried along as a copy). */
static void *reader_thread(void *arg) {
	pipe_t *pp = (pipe_t *)arg;
	fq_stream *fs = pp->map ? fq_open_text(pp->readsFname) : fq_open(pp->readsFname);
	uint8_t *last_src = NULL; uint32_t last_len = 0;
	const aln_params_t *params = pp->params;
	const double t0 = wall();
	for (;;) {
		pthread_mutex_lock(&pp->mu);
		while (pp->n_parsed - pp->n_written >= pp->max_ahead) pthread_cond_wait(&pp->cv_space, &pp->mu);
		pthread_mutex_unlock(&pp->mu);
		chunk_t *c = (chunk_t *)calloc(1, sizeof(chunk_t));
		if (!fq_next_chunk(fs, pp->chunk_reads, &c->fq)) { free(c); break; }
		if (last_src) { c->carry = (uint8_t *)malloc(last_len); memcpy(c->carry, last_src, last_len); c->carry_len = last_len; }
		for (uint32_t q = c->fq.n; q-- > 0;) { /* the chunk's last D_seed source, if it has one */
			const uint32_t lq = c->fq.len[q];
			const uint8_t *sq = c->fq.seq + (size_t)q * c->fq.stride;
			int ok = params->seed_length && lq > (uint32_t)params->seed_length && lq <= 255;
			if (ok && params->use_precalc) { if (lq < 12) ok = 0; for (int k = 0; ok && k < 12; k++) if (sq[k] > 3) ok = 0; }
			if (ok) { last_src = (uint8_t *)realloc(last_src, lq); memcpy(last_src, sq, lq); last_len = lq; break; }
		}
		pthread_mutex_lock(&pp->mu);
		c->idx = pp->n_parsed++;
		c->first_read = pp->n_reads;
		pp->n_reads += c->fq.n;
		if (c->idx == 0) pp->t_first_chunk = wall() - t0;
		if (pp->last) pp->last->next = c; else pp->first = c;
		pp->last = c;
		if (!pp->unclaimed) pp->unclaimed = c;
		pthread_cond_broadcast(&pp->cv_work);
		pthread_mutex_unlock(&pp->mu);
	}
	pthread_mutex_lock(&pp->mu);
	pp->reader_done = 1;
	pthread_cond_broadcast(&pp->cv_work);
	pthread_cond_broadcast(&pp->cv_done);
	pthread_mutex_unlock(&pp->mu);
	free(last_src);
	if (pp->map) pp->fs = fs; /* (closed by the writer's thread after the last chunk's text is formatted) */
	else fq_close(fs);
	return NULL;
}

/* the chunk's output is complete: wakes the writer */
static void chunk_ready(pipe_t *pp, chunk_t *c) {
	pthread_mutex_lock(&pp->mu);
	c->ready = 1;
	pthread_cond_broadcast(&pp->cv_done);
	pthread_mutex_unlock(&pp->mu);
}

/* hands the finished chunk in `slot` to the writer */
static void retire(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c) {
	bwb_result r;
	if (bwb_hip_slot_result(ctx, slot, &r)) bwb_die("align_reads_inexact_gpu: GPU %d: %s", w->gpu, bwb_hip_last_error());
	c->n = r.n_reads;
	c->buf = alns2alnf_buf(r.alns, r.aln_off, r.n_reads, &c->buf_len); /* (with all cores; the library's result buffers stay valid until the slot is uploaded again) */
	chunk_ready(w->pp, c);
}

/* map: the same hand-over with the chunk's SAM text.  The reads are evaluated where their hits lie (kernel k_place); what comes back is one
 * placement record per read, and the worker's team formats the text. */
static void retire_map(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c) {
	const map_t *m = w->pp->map;
	const bwb_place *pl = NULL;
	uint32_t n = 0;
	const uint64_t *alt_off = NULL;
	const bwb_alt *alts = NULL;
	if (m->max_alt ? bwb_hip_slot_place_alt(ctx, slot, m->max_mm, m->max_alt, &pl, &alt_off, &alts, &n) : bwb_hip_slot_place(ctx, slot, m->max_mm, &pl, &n))
		bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
	{ uint64_t st = 0; double ms = 0; bwb_hip_place_stats(ctx, NULL, &st, &ms); w->place_ms += ms; w->place_steps += st; }
	if (m->max_alt) { uint64_t it = 0, st = 0; double ms = 0; bwb_hip_place_alt_stats(ctx, &it, &st, &ms); w->alt_ms += ms; w->alt_steps += st; w->alt_items += it; }
	/* -B: the loci of the same records, resolved where they lie (kernel k_locus behind k_place on the result stream; the slot's placement
	 * records are cached, so nothing is evaluated twice); on an .ann that is not ascending and disjoint, by the host's resolver */
	const bwb_locus *loci = NULL;
	bwb_locus *host_loci = NULL;
	if (m->bub && m->gpu_loci) {
		if (bwb_hip_slot_locus(ctx, slot, m->max_mm, &pl, &loci, &n)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		uint64_t nr = 0; double ms = 0;
		bwb_hip_locus_stats(ctx, &nr, &ms);
		w->locus_ms += ms; w->locus_reads += nr;
	} else if (m->bub) {
		loci = host_loci = (bwb_locus *)malloc((n ? n : 1) * sizeof(bwb_locus));
#pragma omp parallel for schedule(static) num_threads(bwb_host_team())
		for (long r = 0; r < (long)n; r++) locus_resolve(&pl[r], m->ann, m->ann_sorted, m->bubble_of, m->bub, &host_loci[r]);
	}
	/* -J: the items that lie where the primary lies, from the items and loci the slot already holds (kernels k_join_items / k_join_reads behind
	 * k_locus on the result stream); with the host's loci, the host's rule - the suboptimal bit then needs the hits' scores (slot_result) */
	const bwb_join *joins = NULL;
	bwb_join *host_joins = NULL;
	if (m->join && m->gpu_loci) {
		if (bwb_hip_slot_join(ctx, slot, m->max_mm, m->max_alt, &pl, &alt_off, &alts, &loci, &joins, &n)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		uint64_t it = 0, jn = 0; double ms = 0;
		bwb_hip_join_stats(ctx, &it, &jn, &ms);
		w->join_ms += ms; w->join_items += it; w->join_joined += jn;
	} else if (m->join) {
		bwb_result res;
		if (bwb_hip_slot_result(ctx, slot, &res)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		uint8_t *sub = (uint8_t *)malloc(alt_off[n] ? alt_off[n] : 1);
		joins = host_joins = (bwb_join *)malloc((n ? n : 1) * sizeof(bwb_join));
#pragma omp parallel for schedule(static) num_threads(bwb_host_team())
		for (long r = 0; r < (long)n; r++) {
			for (uint64_t q = alt_off[r]; q < alt_off[r + 1]; q++) sub[q] = res.alns[res.aln_off[r] + alts[q].hit].score > res.alns[res.aln_off[r]].score;
			join_resolve(&pl[r], &loci[r], alts + alt_off[r], sub + alt_off[r], alt_off[r + 1] - alt_off[r], m->ann, m->ann_sorted, m->bubble_of, m->chrom_of, m->bub, m->max_mm, &host_joins[r]);
		}
		free(sub);
	}
	if (joins) { /* the log line's counts, with the team */
		unsigned long long changed = 0, joined = 0;
#pragma omp parallel for schedule(static) reduction(+ : changed, joined) num_threads(bwb_host_team())
		for (long r = 0; r < (long)n; r++) { changed += joins[r].mapq != pl[r].mapq; joined += joins[r].joined; }
		w->join_mapq += changed;
		if (!m->gpu_loci) w->join_joined += joined; /* (on the GPU path join_stats has counted them) */
	}
	/* -R: RNAME, POS and CIGAR of the placements on bubble records, from the records and loci the slot already holds (kernels k_lift_count / k_lift
	 * behind them on the result stream); with the host's loci, the host's rule */
	const uint8_t *lift_kind = NULL;
	const uint64_t *lift_off = NULL;
	const bwb_lift *lift_recs = NULL;
	lift_set_t *host_lift = NULL;
	if (m->lift && m->gpu_loci) {
		uint64_t nq = 0, nl = 0, nu = 0; double ms = 0;
		if (bwb_hip_slot_lift(ctx, slot, m->max_mm, m->max_alt, &lift_kind, &lift_off, &lift_recs, &nq)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		bwb_hip_lift_stats(ctx, &nl, &nu, &ms);
		w->lift_ms += ms; w->lift_lifted += nl; w->lift_unliftable += nu;
		w->lift_bytes += nq + (nq + 1) * 8 + lift_off[nq] * sizeof(bwb_lift);
	} else if (m->lift) {
		host_lift = lift_host(pl, loci, n, alt_off, alts, m->ann, m->ann_sorted, m->bubble_of, m->chrom_of, m->bub);
		lift_kind = host_lift->kind; lift_off = host_lift->off; lift_recs = host_lift->recs;
		w->lift_lifted += host_lift->n_lifted; w->lift_unliftable += host_lift->n_unliftable;
	}
	/* -D: NM and the MD text of every mapped read against the text in HBM (kernels k_md_count / k_md behind them on the result stream, on the
	 * slot's resident reads); with the host's lift records, the host's rule */
	const bwb_md *md_recs = NULL;
	const uint64_t *md_off = NULL;
	const char *md_text = NULL;
	md_set_t *host_md = NULL;
	if (m->md && !host_lift) {
		uint64_t nr = 0, nb = 0; double ms = 0;
		if (bwb_hip_slot_md(ctx, slot, m->max_mm, m->max_alt, m->lift, &md_recs, &md_off, &md_text, &n)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		bwb_hip_md_stats(ctx, &nr, &nb, &ms); /* (the figures of the last call that LAUNCHED: this one, since a chunk's slot is asked once - a second slot_md on it would return its cached records and leave them) */
		w->md_ms += ms; w->md_reads += nr; w->md_bytes += nb;
		w->md_back += (unsigned long long)n * sizeof(bwb_md) + ((unsigned long long)n + 1) * 8 + md_off[n];
	} else if (m->md) {
		host_md = md_host(pl, n, c->fq.seq, c->fq.stride, c->fq.len, lift_kind, lift_off, lift_recs, m->ann, m->text);
		md_recs = host_md->recs; md_off = host_md->off; md_text = host_md->text;
		w->md_reads += host_md->n_ok; w->md_bytes += host_md->off[n];
	}
	/* -A: the allele counts of the slot's reads, added to the context's counters (kernel k_pile behind them on the result stream, on the slot's
	 * resident reads and cached records; nothing per read comes back); with the host's lift or join records, the host's rule into the table itself */
	if (m->pile && !m->pile_on_host) {
		uint64_t nr = 0, na = 0; double ms = 0;
		if (bwb_hip_slot_pile(ctx, slot, m->max_mm, m->max_alt, m->lift, m->join, m->pile->min_mapq, &nr)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		if (n) { bwb_hip_pile_stats(ctx, NULL, &na, &ms); w->pile_ms += ms; w->pile_reads += nr; w->pile_adds += na; } /* (a chunk without reads launches nothing) */
	} else if (m->pile) {
		pthread_mutex_lock(&w->pp->mu); /* (pile_host adds with the whole team: one worker at a time) */
		pile_host(m->pile, pl, n, c->fq.seq, c->fq.stride, c->fq.len, lift_kind, lift_off, lift_recs, joins, m->ann);
		pthread_mutex_unlock(&w->pp->mu);
	}
	/* -I: the read support per indel bubble of the slot's reads, added to the context's counters (kernel k_indel behind them on the result stream,
	 * on the slot's cached placement, locus and join records; nothing per read comes back); with the host's loci, the host's rule into the table itself */
	if (m->indel && m->gpu_loci) {
		uint64_t nr = 0, na = 0, nc = 0; double ms = 0;
		if (bwb_hip_slot_indel(ctx, slot, m->max_mm, m->max_alt, m->join, m->indel->min_mapq, &nr)) bwb_die("map_reads: GPU %d: %s", w->gpu, bwb_hip_last_error());
		if (n) { bwb_hip_indel_stats(ctx, NULL, &na, &nc, &ms); w->indel_ms += ms; w->indel_reads += nr; w->indel_adds += na; w->indel_cands += nc; } /* (a chunk without reads launches nothing) */
	} else if (m->indel) {
		pthread_mutex_lock(&w->pp->mu); /* (indel_host adds with the whole team: one worker at a time) */
		indel_host(m->indel, pl, loci, n, c->fq.len, joins);
		pthread_mutex_unlock(&w->pp->mu);
	}
	const sam_reads_t rd = { .pl = pl, .seq = c->fq.seq, .stride = c->fq.stride, .len = c->fq.len, .text = c->fq.text,
	                         .name_off = c->fq.name_off, .qual_off = c->fq.qual_off, .name_len = c->fq.name_len, .first = c->first_read,
	                         .alt_off = alt_off, .alts = alts, .loci = loci, .bubbles = m->bub, .joins = joins,
	                         .lift_kind = lift_kind, .lift_off = lift_off, .lift_recs = lift_recs, .lift_n = n,
	                         .md = md_recs, .md_off = md_off, .md_text = md_text };
	c->n = n;
	c->n_sam = ((size_t)n + SAM_BLOCK_READS - 1) / SAM_BLOCK_READS;
	c->sam = (char **)calloc(c->n_sam ? c->n_sam : 1, sizeof(char *));
	c->sam_len = (size_t *)calloc(c->n_sam ? c->n_sam : 1, sizeof(size_t));
#pragma omp parallel for schedule(dynamic, 1) num_threads(bwb_host_team())
	for (long bi = 0; bi < (long)c->n_sam; bi++) {
		const size_t r0 = (size_t)bi * SAM_BLOCK_READS, r1 = r0 + SAM_BLOCK_READS < n ? r0 + SAM_BLOCK_READS : n;
		c->sam[bi] = sam_format_reads(&rd, r0, r1, m->ann, m->ann_sorted, &c->sam_len[bi]);
	}
	free(host_loci); free(host_joins); lift_free(host_lift); md_free(host_md);
	free(c->fq.seq); free(c->fq.len); free(c->fq.name_off); free(c->fq.qual_off); free(c->fq.name_len);
	c->fq.seq = NULL; c->fq.len = NULL; c->fq.name_off = NULL; c->fq.qual_off = NULL; c->fq.name_len = NULL;
	chunk_ready(w->pp, c);
}

/* the CPUs of the GPU's NUMA node, when the machine has several nodes: the worker thread, its pinned staging buffers (first touched
 * by it) and the copies into them stay next to the GPU's PCIe root */
static void pin_to_device_node(int device, int dbg) {
	const int node = bwb_hip_device_numa_node(device);
	if (node < 0) return;
	char path[96], buf[4096];
	snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
	FILE *f = fopen(path, "r");
	if (!f) return;
	if (!fgets(buf, sizeof(buf), f)) { fclose(f); return; }
	fclose(f);
	cpu_set_t set; CPU_ZERO(&set);
	int any = 0;
	for (char *q = buf; *q;) {
		char *end;
		long a = strtol(q, &end, 10), b = a;
		if (end == q) break;
		if (*end == '-') { q = end + 1; b = strtol(q, &end, 10); }
		for (long k = a; k <= b && k < CPU_SETSIZE; k++) { CPU_SET((int)k, &set); any = 1; }
		q = *end == ',' ? end + 1 : end;
		if (*q == '\n') break;
	}
	if (any && pthread_setaffinity_np(pthread_self(), sizeof(set), &set) == 0 && dbg) fprintf(stderr, "[bwb host] device %d: worker thread on NUMA node %d (cpus %s", device, node, buf);
}

/* counters (of -A's sites, of -I's bubbles) per read-back of a worker: 2^20, 16 MB.  BWB_COUNT_PIECE: a test knob - pieces of a few counters
 * make the loops below take many turns on a small text; a value below 1 is 1 */
static uint64_t count_piece(void) {
	const char *e = getenv("BWB_COUNT_PIECE");
	if (!e) return (uint64_t)1 << 20;
	const long long v = strtoll(e, NULL, 10);
	return v < 1 ? 1 : (uint64_t)v;
}

/* -G: the entries per geno_sites / geno_bubbles call - count_piece(), at most the library's 2^24 and no more than the larger table has */
static uint32_t geno_piece(const map_t *m) {
	uint64_t most = m->pile->n_sites;
	if (m->indel && m->gpu_loci && (uint64_t)m->bub->n > most) most = (uint64_t)m->bub->n;
	uint64_t p = count_piece();
	if (p > most) p = most;
	if (p > ((uint64_t)1 << 24)) p = (uint64_t)1 << 24;
	return p < 1 ? 1u : (uint32_t)p;
}

/* One host thread per GPU.  Chunks are streamed through the slots of the context: while the search slice of chunk j runs,
 * chunk j+1 is already uploaded and queued behind it and the hits of chunk j-1 are on their way back; a slice parks its
 * unfinished reads for the next one instead of draining (include/bwbble_hip.h), so the GPU never runs a batch's tail alone. */
static void *gpu_worker(void *arg) {
	worker_t *w = (worker_t *)arg;
	pipe_t *pp = w->pp;
	bwb_hip_ctx *ctx = NULL;
	const int dbg = getenv("BWB_DEBUG") != NULL;
	pin_to_device_node(w->device, dbg);
	double tq = wall();
	const bwtint_t hdr[5] = { w->BWT->length, w->BWT->num_words, w->BWT->num_sa, w->BWT->num_occ, w->BWT->sa0_index };
	/* The index goes to the GPU - on a thread of the library - while the loader threads are still reading the tail of the .bwt file
	 * (bwt_io.c), and while this thread already uploads its first chunk: that first slot_upload sizes and allocates the context's scratch
	 * and its heap chunk pool (seconds of hipMalloc at GRCh37 scale, which rounds 3-5 paid AFTER the index upload); slot_submit waits for
	 * the index by itself. */
	if (bwb_hip_ctx_create_async(w->device, hdr, w->BWT->C, w->BWT->bwt, w->BWT->O, w->BWT->loader ? &w->BWT->blocks_ready : NULL, &ctx))
		bwb_die("align_reads_inexact_gpu: GPU %d: %s", w->device, bwb_hip_last_error());
	if (dbg) fprintf(stderr, "[bwb host] worker %d: context created at +%.3f s (index upload under way)\n", w->gpu, wall() - tq);
	if (pp->map) {
		/* The sampled SA (length / 32 x 8 bytes: 1.7 GB at GRCh37 scale) goes to HBM BEFORE the first slot_upload sizes the chunk pool from
		 * what is free - the loader reads it first (bwt_io.c) - and while the library's thread uploads the index: set_sa uses a stream of
		 * its own for that (bwb_hip.hip). */
		while (!__atomic_load_n(&w->BWT->sa_ready, __ATOMIC_ACQUIRE)) { struct timespec ts = { 0, 200000 }; nanosleep(&ts, NULL); }
		if (bwb_hip_set_sa(ctx, w->BWT->SA, w->BWT->num_sa)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
		if (dbg) fprintf(stderr, "[bwb host] worker %d: sampled SA resident at +%.3f s\n", w->gpu, wall() - tq);
		/* -B: the record and bubble tables of k_locus (every worker's context gets them; 30 MB at GRCh37 scale) */
		if (pp->map->bub && pp->map->gpu_loci &&
		    bwb_hip_set_loci(ctx, pp->map->rec_start, pp->map->rec_end, pp->map->bubble_of, (uint32_t)pp->map->ann->num_seq, pp->map->bub->b, (uint32_t)pp->map->bub->n))
			bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
		/* -J, -R: the chromosome's record of every bubble, beside them */
		if (pp->map->chrom_of && pp->map->gpu_loci && bwb_hip_set_bubble_chrom(ctx, pp->map->chrom_of, (uint32_t)pp->map->bub->n))
			bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
		/* -I: the sorted table of the eligible bubbles (16 bytes each, one more per bubble) and the zeroed counters (16 bytes per bubble), before the pool is sized as well */
		if (pp->map->indel && pp->map->gpu_loci) {
			const double t0 = wall();
			uint64_t n_elig = 0;
			if (bwb_hip_indel_begin(ctx, pp->map->indel->anchor, &n_elig)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
			w->indel_begin_s = wall() - t0;
			if (n_elig != pp->map->indel->n_tab) bwb_die("map_reads: GPU %d finds %llu eligible bubbles, the host %llu", w->device, (unsigned long long)n_elig, (unsigned long long)pp->map->indel->n_tab);
		}
		/* -D: the forward text (n_fwd / 2 bytes in HBM: 1.7 GB at GRCh37 scale), before the first slot_upload sizes the chunk pool as well; its
		 * bytes are read by the .bwt loader behind the SA (bwt_io.c: load_bwt_start_job, md.c: md_text_read).  Not with the host's lift records: the host's rule then */
		md_text_wait(pp->map->text);
		if (pp->map->pile) { /* -A: the host's own count of the sites, which every context's must equal, and the table (the first worker here makes them) */
			pthread_mutex_lock(&pp->mu);
			if (!pp->map->pile->text) pile_set_text(pp->map->pile, pp->map->text, pp->map->pile_on_host);
			pthread_mutex_unlock(&pp->mu);
		}
		const int pile_gpu = pp->map->pile && !pp->map->pile_on_host;
		if ((pp->map->md && !(pp->map->lift && !pp->map->gpu_loci)) || pile_gpu) {
			const double t0 = wall();
			if (bwb_hip_set_text(ctx, pp->map->text->codes, pp->map->text->n_fwd)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
			w->text_s = wall() - t0;
			if (dbg) fprintf(stderr, "[bwb host] worker %d: text resident at +%.3f s\n", w->gpu, wall() - tq);
		}
		/* -A: the site index (n_fwd / 8 bytes) and the zeroed counters (16 bytes per site) behind the text, before the pool is sized as well */
		if (pile_gpu) {
			const double t0 = wall();
			uint64_t n_sites = 0;
			if (bwb_hip_pile_begin(ctx, &n_sites)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
			w->pile_begin_s = wall() - t0;
			if (n_sites != pp->map->pile->n_sites) bwb_die("map_reads: GPU %d counts %llu IUPAC sites in the text, the host's scan of the .ref %llu", w->device, (unsigned long long)n_sites, (unsigned long long)pp->map->pile->n_sites);
		}
		/* -G: the scratch and the pinned output of one piece of calls (92 bytes per site of the piece, 48 more per bubble), in every context - which worker
		 * finishes last is not known yet -, before the pool is sized as well */
		if (pp->map->geno && pile_gpu && bwb_hip_geno_begin(ctx, geno_piece(pp->map))) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
	}
	void (*const hand_over)(worker_t *, bwb_hip_ctx *, int, chunk_t *) = pp->map ? retire_map : retire;
	enum { NS = BWB_MAX_SLOTS }; /* chunks in flight: the heaviest reads of a chunk take several slices' time (they are parked and resumed), and
	                                a slot can be uploaded again only when its chunk is complete */
	chunk_t *in_slot[NS];
	size_t j = 0, retired = 0; /* chunks this worker has submitted / handed to the writer */
	for (;;) {
		pthread_mutex_lock(&pp->mu);
		/* nothing to take: with chunks of its own in flight the worker hands its oldest one over instead of waiting (the reader may
		 * be held back by exactly that chunk: it parses at most max_ahead chunks beyond the one being written) */
		while (!pp->unclaimed && !pp->reader_done && retired == j) pthread_cond_wait(&pp->cv_work, &pp->mu);
		chunk_t *c = pp->unclaimed;
		if (c) pp->unclaimed = c->next;
		const int done = !c && pp->reader_done;
		pthread_mutex_unlock(&pp->mu);
		if (!c) {
			if (retired < j) { hand_over(w, ctx, (int)(retired % NS), in_slot[retired % NS]); retired++; continue; }
			if (done) break;
			continue;
		}
		const int slot = (int)(j % NS);
		if (j >= NS && retired + NS <= j) { hand_over(w, ctx, slot, in_slot[slot]); retired++; } /* the slot's previous chunk: NS - 1 slices stay queued while the host waits */
		if (bwb_hip_slot_upload(ctx, slot, w->params, c->fq.seq, c->fq.len, c->fq.n, c->fq.stride, c->carry, c->carry_len))
			bwb_die("align_reads_inexact_gpu: GPU %d: %s", w->device, bwb_hip_last_error());
		if (j == 0) { /* the first chunk is staged, scratch and pool exist: now the index must be complete */
			if (bwb_hip_ctx_index_wait(ctx, &w->t_ctx)) bwb_die("align_reads_inexact_gpu: GPU %d: %s", w->device, bwb_hip_last_error());
			uint64_t pb = 0;
			bwb_hip_setup_times(ctx, NULL, &w->t_pool, &pb);
			w->pool_bytes = pb;
			if (dbg) fprintf(stderr, "[bwb host] worker %d (device %d): index upload %.3f s, chunk pool %.1f GB allocated in %.3f s, first chunk staged at +%.3f s\n", w->gpu, w->device, w->t_ctx,
			                 (double)pb / (1u << 30), w->t_pool, wall() - tq);
		}
		if (bwb_hip_slot_submit(ctx, slot))
			bwb_die("align_reads_inexact_gpu: GPU %d: %s", w->device, bwb_hip_last_error());
		if (j == 0) w->t_first_submit = wall() - tq;
		if (!pp->map) { free(c->fq.seq); free(c->fq.len); c->fq.seq = NULL; c->fq.len = NULL; } /* (staged by the library: the caller's buffers are free; map prints the bases) */
		free(c->carry); c->carry = NULL;
		in_slot[slot] = c;
		w->n_reads += c->fq.n;
		j++;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: chunk %zu (%u reads) submitted at +%.3f s\n", w->gpu, c->idx, c->fq.n, wall() - tq);
	}
	/* -A: the stream has ended and every chunk of this worker is retired - its counters come back in bounded pieces and are summed on the host */
	if (pp->map && pp->map->pile && !pp->map->pile_on_host) {
		const double t0 = wall();
		const uint64_t PIECE = count_piece(), n_sites = pp->map->pile->n_sites; /* sites per read-back */
		uint32_t *buf = (uint32_t *)malloc((size_t)(n_sites < PIECE ? n_sites : PIECE) * 16 + 16);
		uint64_t turns = 0;
		for (uint64_t s0 = 0; s0 < n_sites; s0 += PIECE, turns++) {
			const uint64_t ns = n_sites - s0 < PIECE ? n_sites - s0 : PIECE;
			if (bwb_hip_pile_counts(ctx, s0, ns, buf)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
			pthread_mutex_lock(&pp->mu);
			pile_add(pp->map->pile, s0, ns, buf);
			pthread_mutex_unlock(&pp->mu);
		}
		free(buf);
		w->pile_fetch_s = wall() - t0;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: the counters of %llu sites read back in %llu pieces\n", w->gpu, (unsigned long long)n_sites, (unsigned long long)turns);
	}
	/* -I: the same for the bubbles' counters */
	if (pp->map && pp->map->indel && pp->map->gpu_loci) {
		const double t0 = wall();
		const uint64_t PIECE = count_piece(), n_bub = (uint64_t)pp->map->bub->n;
		uint32_t *buf = (uint32_t *)malloc((size_t)(n_bub < PIECE ? n_bub : PIECE) * 16 + 16);
		uint64_t turns = 0;
		for (uint64_t s0 = 0; s0 < n_bub; s0 += PIECE, turns++) {
			const uint64_t ns = n_bub - s0 < PIECE ? n_bub - s0 : PIECE;
			if (bwb_hip_indel_counts(ctx, s0, ns, buf)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
			pthread_mutex_lock(&pp->mu);
			indel_add(pp->map->indel, s0, ns, buf);
			pthread_mutex_unlock(&pp->mu);
		}
		free(buf);
		w->indel_fetch_s = wall() - t0;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: the counters of %llu bubbles read back in %llu pieces\n", w->gpu, (unsigned long long)n_bub, (unsigned long long)turns);
	}
	/* -G: this worker's counters are in the host's sums.  The worker that completes the count calls the genotypes on its own context: with several
	 * workers it first puts the host's summed tables back over its counters, with one its counters are the sums already and nothing is uploaded.  Then
	 * the sites and the bubbles are walked in pieces; what comes back is the called entries' records alone, which geno.c keeps for the writer. */
	if (pp->map && pp->map->geno) {
		const map_t *m = pp->map;
		geno_t *G = m->geno;
		pthread_mutex_lock(&pp->mu);
		const int last = ++pp->n_finished == pp->n_workers;
		pthread_mutex_unlock(&pp->mu);
		const int sites_gpu = !m->pile_on_host, bubs_gpu = sites_gpu && m->indel && m->gpu_loci;
		if (last && sites_gpu) {
			const uint64_t PIECE = count_piece(), GP = geno_piece(m), n_sites = m->pile->n_sites, n_bub = bubs_gpu ? (uint64_t)m->bub->n : 0;
			double t0 = wall();
			if (pp->n_workers > 1) {
				for (uint64_t s0 = 0; s0 < n_sites; s0 += PIECE, G->put_pieces++)
					if (bwb_hip_pile_put(ctx, s0, n_sites - s0 < PIECE ? n_sites - s0 : PIECE, m->pile->counts + s0 * 4)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
				for (uint64_t s0 = 0; s0 < n_bub; s0 += PIECE, G->put_pieces++)
					if (bwb_hip_indel_put(ctx, s0, n_bub - s0 < PIECE ? n_bub - s0 : PIECE, m->indel->counts + s0 * 4)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
			}
			G->put_s = wall() - t0;
			t0 = wall();
			double ms = 0;
			for (uint64_t s0 = 0; s0 < n_sites; s0 += GP, G->pieces++) {
				const bwb_geno_site *recs = NULL; uint64_t k = 0;
				if (bwb_hip_geno_sites(ctx, s0, n_sites - s0 < GP ? n_sites - s0 : GP, G->err, G->min_depth, &recs, &k)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
				bwb_hip_geno_stats(ctx, NULL, NULL, &ms);
				G->kernel_ms += ms;
				geno_take_sites(G, recs, k);
			}
			const uint64_t GB = GP < n_bub ? GP : n_bub;
			for (uint64_t s0 = 0; s0 < n_bub; s0 += GB, G->pieces++) {
				const bwb_geno_bubble *recs = NULL; uint64_t k = 0;
				if (bwb_hip_geno_bubbles(ctx, s0, n_bub - s0 < GB ? n_bub - s0 : GB, G->err, G->min_depth, &recs, &k)) bwb_die("map_reads: GPU %d: %s", w->device, bwb_hip_last_error());
				bwb_hip_geno_stats(ctx, NULL, NULL, &ms);
				G->kernel_ms += ms;
				geno_take_bubbles(G, recs, k);
			}
			G->call_s = wall() - t0;
			G->worker = w->gpu;
			if (dbg) fprintf(stderr, "[bwb host] worker %d: genotypes called by this worker, the last of %d: %llu pieces of tables put back in %.3f s, %llu pieces called in %.3f s: sites %llu  bubbles %llu  kernels %.3f ms\n",
			                 w->gpu, pp->n_workers, (unsigned long long)G->put_pieces, G->put_s, (unsigned long long)G->pieces, G->call_s, (unsigned long long)G->n_sites, (unsigned long long)G->n_bubs, G->kernel_ms);
		}
	}
	bwb_stats st;
	if (bwb_hip_flush(ctx) || bwb_hip_get_stats(ctx, &st)) bwb_die("align_reads_inexact_gpu: GPU %d: %s", w->device, bwb_hip_last_error());
	w->total = st;
	w->kernel_ms = st.ms_calc_d + st.ms_search;
	bwb_hip_ctx_destroy(ctx);
	if (dbg) fprintf(stderr, "[bwb host] worker %d: done %.3f s\n", w->gpu, wall() - tq);
	return NULL;
}

/* The GPU replacement for align_reads_inexact_parallel, as a pipeline: reader thread (FASTQ -> chunks) | one worker per GPU | this
 * thread (ordered writer, inexact_match.c:154-162).  `reads` is the FASTQ's NAME: the file is streamed, not loaded (the reference's
 * reads_t holds the whole file in memory before the first read is aligned). */
static int run_stream(bwt_t *BWT, const char *readsFname, aln_params_t *params, FILE *alnFile, const char *alnFname, int n_gpus, const map_t *map);
int align_reads_inexact_gpu_stream(bwt_t *BWT, const char *readsFname, aln_params_t *params, char *alnFname, int n_gpus) {
	printf("BWBBLE Inexact Alignment (MI355X)...\n");
	FILE *alnFile = fopen(alnFname, "a+b");                                   /* inexact_match.c:94 */
	if (!alnFile) { perror(alnFname); bwb_die("align_reads_inexact: Cannot open ALN file: %s!", alnFname); }
	return run_stream(BWT, readsFname, params, alnFile, alnFname, n_gpus, NULL);
}

/* the pipeline; alnFile is the open output (.aln records, or with `map` the SAM file after its header lines) and is closed here */
static int run_stream(bwt_t *BWT, const char *readsFname, aln_params_t *params, FILE *alnFile, const char *alnFname, int n_gpus, const map_t *map) {
	if (bwb_hip_abi_version() != BWB_HIP_ABI_VERSION) bwb_die("align_reads_inexact_gpu: libbwbble_hip.so implements C-ABI version %d, this binary was compiled against %d", bwb_hip_abi_version(), BWB_HIP_ABI_VERSION);
	const int ndev = bwb_hip_device_count();
	if (ndev < 1) bwb_die("align_reads_inexact_gpu: no HIP device found (this build has no CPU alignment path)");
	/* BWB_DEVICE_MAP=d0,d1,...: worker g drives HIP device d_g (default g).  Several workers on one device are allowed - that
	 * is how the multi-worker path (shared queue, ordered writer) is tested on a one-GPU box. */
	int devmap[64];
	int nmap = 0;
	if (getenv("BWB_DEVICE_MAP")) {
		const char *q = getenv("BWB_DEVICE_MAP");
		while (*q && nmap < 64) {
			char *end;
			const long d = strtol(q, &end, 10);
			if (end == q) break;
			if (d < 0 || d >= ndev) bwb_die("align_reads_inexact_gpu: BWB_DEVICE_MAP names device %ld, only %d present", d, ndev);
			devmap[nmap++] = (int)d;
			q = *end == ',' ? end + 1 : end;
		}
	}
	if (n_gpus < 1) n_gpus = 1;
	if (n_gpus > (nmap ? nmap : ndev)) bwb_die("align_reads_inexact_gpu: -g %d asked for, %d HIP device(s) available", n_gpus, nmap ? nmap : ndev);
	pipe_t pp;
	memset(&pp, 0, sizeof(pp));
	pthread_mutex_init(&pp.mu, NULL);
	pthread_cond_init(&pp.cv_work, NULL); pthread_cond_init(&pp.cv_done, NULL); pthread_cond_init(&pp.cv_space, NULL);
	pp.readsFname = readsFname; pp.params = params; pp.map = map;
	pp.n_workers = n_gpus;
	pp.chunk_reads = GPU_CHUNK_DEFAULT;
	if (getenv("BWB_CHUNK")) pp.chunk_reads = (uint32_t)strtoul(getenv("BWB_CHUNK"), NULL, 10);
	if (pp.chunk_reads < 1) pp.chunk_reads = 1;
	pp.max_ahead = (size_t)n_gpus * (BWB_MAX_SLOTS + 2); /* chunks parsed beyond the one being written: every worker's slots and two to take */
	worker_t *ws = (worker_t *)calloc((size_t)n_gpus, sizeof(worker_t));
	pthread_t *th = (pthread_t *)calloc((size_t)n_gpus, sizeof(pthread_t));
	pthread_t rth;
	const double t0 = wall();
	if (pthread_create(&rth, NULL, reader_thread, &pp)) bwb_die("align_reads_inexact_gpu: cannot start the reader thread");
	for (int g = 0; g < n_gpus; g++) {
		ws[g] = (worker_t){ .gpu = g, .device = nmap ? devmap[g] : g, .BWT = BWT, .params = params, .pp = &pp };
		if (pthread_create(&th[g], NULL, gpu_worker, &ws[g])) bwb_die("align_reads_inexact_gpu: cannot start a host thread");
	}
	/* ordered writer (the reference writes after each batch, inexact_match.c:154-162), woken when a chunk's hits have arrived */
	size_t processed = 0;
	const int dbg = getenv("BWB_DEBUG") != NULL;
	for (;;) {
		pthread_mutex_lock(&pp.mu);
		while (!(pp.first && pp.first->ready) && !(pp.reader_done && !pp.first)) pthread_cond_wait(&pp.cv_done, &pp.mu);
		chunk_t *c = pp.first;
		if (c) { pp.first = c->next; if (!pp.first) pp.last = NULL; }
		pthread_mutex_unlock(&pp.mu);
		if (!c) break;
		if (c->buf_len && fwrite(c->buf, 1, c->buf_len, alnFile) != c->buf_len) bwb_die("align_reads_inexact: Cannot write to the ALN file: %s!", alnFname);
		for (size_t bi = 0; bi < c->n_sam; bi++) {
			if (c->sam_len[bi] && fwrite(c->sam[bi], 1, c->sam_len[bi], alnFile) != c->sam_len[bi]) bwb_die("map_reads: Cannot write to the SAM file: %s!", alnFname);
			free(c->sam[bi]);
		}
		free(c->sam); free(c->sam_len);
		processed += c->n;
		printf("Processed %zu reads. Elapsed: %.2f sec\n", processed, wall() - t0);
		if (dbg) fprintf(stderr, "[bwb host] writer: chunk %zu written at +%.3f s\n", c->idx, wall() - t0);
		free(c->buf); free(c);
		pthread_mutex_lock(&pp.mu);
		pp.n_written++;
		pthread_cond_broadcast(&pp.cv_space);
		pthread_mutex_unlock(&pp.mu);
	}
	pthread_join(rth, NULL);
	if (pp.fs) fq_close(pp.fs);
	bwb_stats tot; memset(&tot, 0, sizeof(tot));
	double kms = 0, tctx = 0, tpool = 0, tfirst = 0;
	unsigned long long pool_bytes = 0;
	for (int g = 0; g < n_gpus; g++) {
		pthread_join(th[g], NULL);
		tot.visits_single += ws[g].total.visits_single; tot.visits_alphabet += ws[g].total.visits_alphabet;
		tot.heap_pops += ws[g].total.heap_pops; tot.n_alignments += ws[g].total.n_alignments; tot.n_overflow_reads += ws[g].total.n_overflow_reads;
		if (ws[g].kernel_ms > kms) kms = ws[g].kernel_ms;
		if (ws[g].t_ctx > tctx) tctx = ws[g].t_ctx;
		if (ws[g].t_pool > tpool) tpool = ws[g].t_pool;
		if (ws[g].t_first_submit > tfirst) tfirst = ws[g].t_first_submit;
		if (ws[g].pool_bytes > pool_bytes) pool_bytes = ws[g].pool_bytes;
		if (n_gpus > 1) /* one line per worker: an uneven node (a slow link, a busy socket) shows here, not in the total */
			printf("  GPU %d (device %d, NUMA node %d): reads %llu  kernel %.1f ms  index to HBM %.2f sec  launches %llu  parked reads %llu  re-run reads %llu\n", g, ws[g].device,
			       bwb_hip_device_numa_node(ws[g].device), (unsigned long long)ws[g].n_reads, ws[g].kernel_ms, ws[g].t_ctx,
			       (unsigned long long)ws[g].total.launches_search, (unsigned long long)ws[g].total.n_parked_reads, (unsigned long long)ws[g].total.n_overflow_reads);
	}
	const double dt = wall() - t0;
	printf("GPUs: %d  reads: %llu  wall: %.3f sec (%.0f reads/s incl. index upload)  kernel: %.1f ms  index to HBM: %.2f sec  first chunk parsed after: %.2f sec  rank-block visits: %llu  hits: %llu  re-run reads: %llu\n",
	       n_gpus, (unsigned long long)pp.n_reads, dt, pp.n_reads / (dt > 0 ? dt : 1), kms, tctx, pp.t_first_chunk, (unsigned long long)(tot.visits_single + tot.visits_alphabet),
	       (unsigned long long)tot.n_alignments, (unsigned long long)tot.n_overflow_reads);
	if (map) {
		double pms = 0; unsigned long long pst = 0;
		for (int g = 0; g < n_gpus; g++) { pst += ws[g].place_steps; if (ws[g].place_ms > pms) pms = ws[g].place_ms; }
		printf("placements on the GPU: reads %llu  rank-block visits %llu  kernel %.3f ms", (unsigned long long)pp.n_reads, pst, pms);
		if (map->bub && map->gpu_loci) { /* -B: the loci of the same reads */
			double lms = 0; unsigned long long lrd = 0;
			for (int g = 0; g < n_gpus; g++) { lrd += ws[g].locus_reads; if (ws[g].locus_ms > lms) lms = ws[g].locus_ms; }
			printf("  loci resolved %llu  k_locus %.3f ms", lrd, lms);
		} else if (map->bub) printf("  loci resolved %llu on the host%s (the .ann records are not ascending and disjoint)", (unsigned long long)pp.n_reads, map->join ? " and joined there" : "");
		printf("\n");
		if (map->join) { /* -J */
			double jms = 0; unsigned long long jit = 0, jjn = 0, jmq = 0;
			for (int g = 0; g < n_gpus; g++) { jit += ws[g].join_items; jjn += ws[g].join_joined; jmq += ws[g].join_mapq; if (ws[g].join_ms > jms) jms = ws[g].join_ms; }
			if (map->gpu_loci) printf("placements joined by locus on the GPU: items %llu  joined %llu  reads with another MAPQ %llu  kernels %.3f ms\n", jit, jjn, jmq, jms);
			else printf("placements joined by locus on the host: joined %llu  reads with another MAPQ %llu\n", jjn, jmq);
		}
		if (map->lift) { /* -R */
			double lms = 0; unsigned long long ll = 0, lu = 0, lb = 0;
			for (int g = 0; g < n_gpus; g++) { ll += ws[g].lift_lifted; lu += ws[g].lift_unliftable; lb += ws[g].lift_bytes; if (ws[g].lift_ms > lms) lms = ws[g].lift_ms; }
			if (map->gpu_loci) printf("placements lifted to chromosome coordinates on the GPU: lifted %llu  not liftable %llu  kernels %.3f ms  bytes to the host %llu\n", ll, lu, lms, lb);
			else printf("placements lifted to chromosome coordinates on the host (the .ann records are not ascending and disjoint): lifted %llu  not liftable %llu\n", ll, lu);
		}
		if (map->md) { /* -D */
			double mms = 0, ts = 0; unsigned long long mr = 0, mb = 0, bk = 0;
			for (int g = 0; g < n_gpus; g++) { mr += ws[g].md_reads; mb += ws[g].md_bytes; bk += ws[g].md_back; if (ws[g].md_ms > mms) mms = ws[g].md_ms; if (ws[g].text_s > ts) ts = ws[g].text_s; }
			if (!(map->lift && !map->gpu_loci))
				printf("NM and MD against the text on the GPU: reads %llu  MD bytes %llu  kernels %.3f ms  bytes to the host %llu  text %llu characters read in %.3f s, set in %.3f s\n", mr, mb, mms, bk,
				       (unsigned long long)map->text->n_fwd, map->text->seconds, ts);
			else printf("NM and MD against the text on the host (the .ann records are not ascending and disjoint): reads %llu  MD bytes %llu\n", mr, mb);
		}
		if (map->pile) { /* -A */
			double pms = 0, bs = 0, fs = 0; unsigned long long pr = 0, pa = 0;
			for (int g = 0; g < n_gpus; g++) { pr += ws[g].pile_reads; pa += ws[g].pile_adds; if (ws[g].pile_ms > pms) pms = ws[g].pile_ms; if (ws[g].pile_begin_s > bs) bs = ws[g].pile_begin_s; if (ws[g].pile_fetch_s > fs) fs = ws[g].pile_fetch_s; }
			if (!map->pile_on_host)
				printf("allele counts at the text's IUPAC sites on the GPU: sites %llu  reads counted %llu  adds %llu  k_pile %.3f ms  site index and counters %llu bytes, built in %.3f s  counters read back in %.3f s\n",
				       (unsigned long long)map->pile->n_sites, pr, pa, pms, (unsigned long long)((map->text->n_fwd + 31) / 32 * 4 + map->pile->n_sites * 16), bs, fs);
			else printf("allele counts at the text's IUPAC sites on the host (the .ann records are not ascending and disjoint): sites %llu  reads counted %llu  adds %llu\n",
			            (unsigned long long)map->pile->n_sites, (unsigned long long)map->pile->reads, (unsigned long long)map->pile->adds);
		}
		if (map->indel) { /* -I */
			double ims = 0, bs = 0, fs = 0; unsigned long long ir = 0, ia = 0, ic = 0;
			for (int g = 0; g < n_gpus; g++) { ir += ws[g].indel_reads; ia += ws[g].indel_adds; ic += ws[g].indel_cands; if (ws[g].indel_ms > ims) ims = ws[g].indel_ms; if (ws[g].indel_begin_s > bs) bs = ws[g].indel_begin_s; if (ws[g].indel_fetch_s > fs) fs = ws[g].indel_fetch_s; }
			if (map->gpu_loci)
				printf("read support per indel bubble on the GPU: anchor %d  eligible bubbles %llu  refused and skipped %llu  reads counted %llu  adds %llu  candidates %llu  k_indel %.3f ms  table and counters %llu bytes, sorted in %.3f s, resident in %.3f s  counters read back in %.3f s\n",
				       map->indel->anchor, (unsigned long long)map->indel->n_tab, (unsigned long long)map->indel->n_refused, ir, ia, ic, ims,
				       (unsigned long long)(map->indel->n_tab * 16 + (uint64_t)map->bub->n * 17), map->indel->sort_s, bs, fs);
			else printf("read support per indel bubble on the host (the .ann records are not ascending and disjoint): anchor %d  eligible bubbles %llu  refused and skipped %llu  reads counted %llu  adds %llu  candidates %llu\n",
			            map->indel->anchor, (unsigned long long)map->indel->n_tab, (unsigned long long)map->indel->n_refused, (unsigned long long)map->indel->reads, (unsigned long long)map->indel->adds, (unsigned long long)map->indel->cands);
		}
		if (map->geno && !map->pile_on_host) /* -G */
			printf("genotype calls on the GPU (worker %d): error phred %d  minimum depth %lld  sites called %llu%s  bubbles called %llu  kernels %.3f ms  pieces %llu  bytes to the host %llu  tables put back in %llu pieces, %.3f s  called in %.3f s\n",
			       map->geno->worker, map->geno->err, (long long)map->geno->min_depth, (unsigned long long)map->geno->n_sites, map->indel && !map->gpu_loci ? " (the bubbles follow on the host)" : "",
			       (unsigned long long)map->geno->n_bubs, map->geno->kernel_ms, (unsigned long long)map->geno->pieces,
			       (unsigned long long)(map->geno->n_sites * sizeof(bwb_geno_site) + map->geno->n_bubs * sizeof(bwb_geno_bubble) + map->geno->pieces * 8), (unsigned long long)map->geno->put_pieces, map->geno->put_s, map->geno->call_s);
		if (map->max_alt) {
			double ams = 0; unsigned long long ast = 0, ait = 0;
			for (int g = 0; g < n_gpus; g++) { ast += ws[g].alt_steps; ait += ws[g].alt_items; if (ws[g].alt_ms > ams) ams = ws[g].alt_ms; }
			printf("other placements on the GPU (-X %d): items %llu (%.3f per read)  rank-block visits %llu  kernels %.3f ms\n", map->max_alt, ait,
			       pp.n_reads ? (double)ait / (double)pp.n_reads : 0.0, ast, ams);
		}
	}
	/* where the start-up went (the three overlap): the .bwt file in memory | the index in HBM | the chunk pool's hipMalloc | first slice queued */
	printf("start-up: .bwt read %.2f sec | index to HBM %.2f sec | chunk pool %.1f GB in %.2f sec | first slice queued after %.2f sec\n",
	       bwt_load_seconds(BWT), tctx, (double)pool_bytes / (1u << 30), tpool, tfirst);
	free(ws); free(th);
	pthread_mutex_destroy(&pp.mu); pthread_cond_destroy(&pp.cv_work); pthread_cond_destroy(&pp.cv_done); pthread_cond_destroy(&pp.cv_space);
	fclose(alnFile);
	return 0;
}

/* -P (align.c:59-65): the first run on an index leaves <fasta>.pre behind (precalc.c: written, never read).  A file that is there -
 * load_precalc_sa_intervals (align.c:226-238) would read it - only has its shape checked (precalc.c); without one the index is waited
 * for, the table built, and *t (the caller's start time, of the index load so far) restarted. */
static void ensure_precalc(bwt_t *BWT, const char *fastaFname, aln_params_t *params, double *t) {
	const size_t L = strlen(fastaFname) + 8;
	char *preFname = (char *)malloc(L);
	snprintf(preFname, L, "%s.pre", fastaFname);
	FILE *pf = fopen(preFname, "r");
	if (pf) {
		fclose(pf);
		if (check_precalc_file(preFname)) fprintf(stderr, "warning: %s is not a complete table of 16777216 interval lists (a run of the reference would fail on it): delete it to have it rebuilt\n", preFname);
	} else {
		load_bwt_wait(BWT);
		printf("Total BWT loading time: %.2f sec\n", wall() - *t);
		*t = wall();
		precalc_sa_intervals(BWT, params, preFname);
		printf("Total pre-calculated intervals time: %.2f sec\n", wall() - *t);
	}
	free(preFname);
}

int align_reads(char *fastaFname, char *readsFname, char *alnsFname, aln_params_t *params, int n_gpus) { /* align.c:40-87 */
	printf("**** BWBBLE Read Alignment ****\n");
	size_t L = strlen(fastaFname) + 8;
	char *bwtFname = (char *)malloc(L);
	snprintf(bwtFname, L, "%s.bwt", fastaFname);
	remove(alnsFname); /* align.c:48 */
	double t = wall();
	/* The reference loads the index, then all reads, then aligns (align.c:50-76).  Here the three overlap: loader threads read the .bwt
	 * file while every GPU worker already uploads its head (bwt_io.c, bwb_hip_ctx_create_streamed), and the reader thread parses the
	 * FASTQ chunk by chunk while the GPUs align the chunks before. */
	bwt_t *BWT = load_bwt_start(bwtFname, 0);
	if (params->use_precalc) ensure_precalc(BWT, fastaFname, params, &t);
	t = wall();
	align_reads_inexact_gpu_stream(BWT, readsFname, params, alnsFname, n_gpus);   /* the seam: align.c:72-76 */
	printf("Total read alignment time (index and read loading overlapped): %.2f sec\n", wall() - t);
	free_bwt(BWT);
	free(bwtFname);
	return 0;
}

/* `bwbble map`: align_reads + alns2sam in one pass.  The .bwt is loaded once, with its SA; the SAM header is written before the first chunk. */
int map_reads(char *fastaFname, char *readsFname, char *samFname, aln_params_t *params, int max_mm, int max_alt, const char *bubbleFname, int join, int lift, int md, const char *countsFname, int min_mapq, const char *indelFname, int anchor, const char *genoFname, int geno_err, int64_t geno_depth, int n_gpus) {
	printf("**** BWBBLE Read Mapping (align + aln2sam in one pass) ****\n");
	/* -A: the counts file is opened before anything is loaded; until it is written, a run that stops leaves none behind */
	pile_t *pile = countsFname || genoFname ? pile_open(countsFname, min_mapq) : NULL; /* (-G: the table without a file) */
	indel_t *indel = indelFname || (genoFname && bubbleFname) ? indel_open(indelFname, min_mapq, anchor) : NULL; /* -I (main.c: only with -B): the same; -G with -B: the table without a file */
	geno_t *geno = genoFname ? geno_open(genoFname, geno_err, geno_depth) : NULL; /* -G: the same */
	/* -B: the table first (a refused table stops the run before anything is created) */
	bubble_table_t *bub = bubbleFname ? load_bubbles(bubbleFname) : NULL;
	if (lift && bub) lift_check_table(bub); /* -R (main.c: only with -B): a bubble the rule refuses is named here */
	/* -D: a missing <seq_fasta>.ref, or one of another size than the .ann says, stops the run here; the .bwt loader reads its forward half, behind the sampled SA */
	md_text_t *text = md || pile ? md_text_open_for(fastaFname, 1, md ? "-D" : countsFname ? "-A" : "-G") : NULL; /* (-A loads it the same way, with or without -D) */
	/* before anything is created: without a GPU no SAM file is left behind */
	if (bwb_hip_device_count() < 1) bwb_die("align_reads_inexact_gpu: no HIP device found (this build has no CPU alignment path)");
	size_t L = strlen(fastaFname) + 8;
	char *bwtFname = (char *)malloc(L), *annFname = (char *)malloc(L);
	snprintf(bwtFname, L, "%s.bwt", fastaFname);
	snprintf(annFname, L, "%s.ann", fastaFname);
	double t = wall();
	bwt_t *BWT = load_bwt_start_job(bwtFname, 1, text ? md_text_read : NULL, text);
	fasta_annotations_t *ann = annf2ann(annFname);
	/* -B: every record's bubble number, before the SAM file exists (a record that names a bubble outside the table leaves none behind) */
	int32_t *bubble_of = bub ? ann_bubble_of(ann, bub) : NULL;
	/* -J (main.c: only with -X and -B): the chromosome's record of every bubble; one without a chromosome leaves no SAM file behind either */
	join = join && bub && max_alt; lift = lift && bub;
	int32_t *chrom_of = join || lift || indel ? bubble_chrom_of(ann, bubble_of, bub, join ? "-J" : lift ? "-R" : indelFname ? "-I" : "-G") : NULL;
	if (indel) indel_set_table(indel, bub, chrom_of); /* -I: the eligible bubbles, sorted; a refused bubble is skipped, not named */
	uint64_t *rec_start = NULL, *rec_end = NULL;
	int gpu_loci = bub && ann->num_seq > 0 && sam_ann_sorted(ann) && bub->n <= INT32_MAX;
	if (bub) {
		const size_t n_rec = ann->num_seq > 0 ? (size_t)ann->num_seq : 1;
		rec_start = (uint64_t *)malloc(n_rec * 8);
		rec_end = (uint64_t *)malloc(n_rec * 8);
		for (int i = 0; i < ann->num_seq; i++) {
			rec_start[i] = ann->seq_anns[i].start_index; rec_end[i] = ann->seq_anns[i].end_index;
			if (rec_start[i] > rec_end[i]) gpu_loci = 0; /* (an empty record: sam_ann_sorted does not look for it, bwb_hip_set_loci refuses it) */
		}
	}
	if (params->use_precalc) ensure_precalc(BWT, fastaFname, params, &t);
	FILE *sam = fopen(samFname, "w");
	if (!sam) { perror(samFname); bwb_die("map_reads: Cannot open SAM file: %s!", samFname); }
	sam_write_header(sam, ann);
	const map_t m = { .max_mm = max_mm, .max_alt = max_alt, .ann = ann, .ann_sorted = sam_ann_sorted(ann),
	                  .bub = bub, .bubble_of = bubble_of, .gpu_loci = gpu_loci, .rec_start = rec_start, .rec_end = rec_end, .chrom_of = chrom_of, .join = join, .lift = lift, .text = text,
	                  .md = md, .pile = pile, .pile_on_host = pile && bub && !gpu_loci && (lift || join), .indel = indel, .geno = geno };

	t = wall();
	printf("BWBBLE Inexact Alignment (MI355X)...\n");
	run_stream(BWT, readsFname, params, sam, samFname, n_gpus, &m);
	if (pile && pile->f) { /* -A: the SAM file is complete (run_stream has closed it) */
		const double tw = wall();
		const unsigned long long lines = pile_write(pile, ann);
		printf("allele counts written: %llu sites with a count in %.3f s\n", lines, wall() - tw);
	}
	if (indel && indel->f) { /* -I: likewise */
		const double tw = wall();
		const unsigned long long lines = indel_write(indel);
		printf("read support per indel bubble written: %llu bubbles with a count in %.3f s\n", lines, wall() - tw);
	}
	if (geno) { /* -G: last; what was counted on the host is called there, by the same rule */
		const double tw = wall();
		if (m.pile_on_host || (indel && !gpu_loci)) {
			const unsigned long long s0 = geno->n_sites, b0 = geno->n_bubs;
			geno_host(geno, m.pile_on_host ? pile : NULL, indel && !gpu_loci ? indel : NULL);
			printf("genotype calls on the host (the .ann records are not ascending and disjoint): sites called %llu  bubbles called %llu\n", (unsigned long long)geno->n_sites - s0, (unsigned long long)geno->n_bubs - b0);
		}
		const unsigned long long lines = geno_write(geno, ann, bub);
		printf("genotype calls written: %llu lines in %.3f s\n", lines, wall() - tw);
	}
	printf("Total read mapping time (index and read loading overlapped): %.2f sec\n", wall() - t);
	free_bwt(BWT); free_ann(ann);
	free(bwtFname); free(annFname);
	free(bubble_of); free(chrom_of); free(rec_start); free(rec_end); free_bubbles(bub); pile_free(pile); indel_free(indel); geno_free(geno); md_text_free(text);
	return 0;
}
