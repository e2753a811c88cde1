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
	host_recs_t host;                               /* map: what the host's stages allocated for the chunk's records, until its text is formatted */
	size_t first_read;                              /* number of the chunk's first read in the file */
	int ready;
	struct chunk *next;            /* production order */
} chunk_t;

/* what `map` adds to the pipeline (NULL: align) */
typedef struct {
	int max_mm; int max_alt /* -X (0: no tags) */;
	/* the .ann records; -B (T.bub NULL: no tags): the bubble table and every record's bubble number; -J, -R, -I (T.chrom_of NULL: none of them):
	 * the chromosome's record of every bubble */
	host_tables_t T;
	/* -B: when the records are ascending and disjoint, so that kernel k_locus can search them (gpu_loci) - their first and last positions as
	 * the arrays bwb_hip_set_loci takes */
	int gpu_loci; const uint64_t *rec_start, *rec_end;
	int join;                 /* -J: a read's placements counted by locus; needs max_alt and bub */
	int lift;                 /* -R: placements on a bubble record written in chromosome coordinates; needs bub */
	md_text_t *text;          /* -D, -A (NULL: neither): the forward text of <seq_fasta>.ref */
	int md;                   /* -D: the tags NM:i / MD:Z against the text */
	pile_t *pile;             /* -A (NULL: no counts): the allele counts at the text's IUPAC sites; on the GPU unless pile_on_host */
	int pile_q;               /* -b above 0 or -Y: the pile reads the base qualities - on the GPU k_pile_q on the slot's quality bytes, and with -Y the sums of the weighted calls */
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
	double quals_s; unsigned long long quals_bytes, pile_dropped; /* map -b / -Y: packing and staging the chunks' quality lines, their bytes; the bases -b dropped */
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

/* a C-ABI call of a worker: on failure the run ends with the caller's prefix, the worker's number (retire, retire_map: w->gpu) or its device
 * (gpu_worker: w->device), and the library's message */
static void gpu_ok(int failed, const char *who, int id) {
	if (failed) bwb_die("%s: GPU %d: %s", who, id, bwb_hip_last_error());
}

/* hands the finished chunk in `slot` to the writer */
static void retire(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c) {
	bwb_result r;
	gpu_ok(bwb_hip_slot_result(ctx, slot, &r), "align_reads_inexact_gpu", w->gpu);
	c->n = r.n_reads;
	c->buf = alns2alnf_buf(r.alns, r.aln_off, r.n_reads, &c->buf_len); /* (with all cores; the library's result buffers stay valid until the slot is uploaded again) */
	chunk_ready(w->pp, c);
}

/* map: the stages of a finished chunk on the result stream, one per flag.  Each takes the worker, its context, the slot, the chunk and the
 * carrier of the chunk's records (rd: a stage reads what the stages before it put there), holds the GPU's branch and the host's - the slot's
 * records are cached, so nothing is evaluated twice; what the host allocates the chunk keeps (c->host) - and adds to the worker's figures. */

/* the reads are evaluated where their hits lie (kernel k_place; -X: with their other placements): one placement record per read comes back */
static void stage_place(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	gpu_ok(m->max_alt ? bwb_hip_slot_place_alt(ctx, slot, m->max_mm, m->max_alt, &rd->pl, &rd->alt_off, &rd->alts, &c->n) : bwb_hip_slot_place(ctx, slot, m->max_mm, &rd->pl, &c->n), "map_reads", w->gpu);
	rd->lift_n = c->n;
	{ uint64_t st = 0; double ms = 0; bwb_hip_place_stats(ctx, NULL, &st, &ms); w->place_ms += ms; w->place_steps += st; }
	if (m->max_alt) { uint64_t it = 0, st = 0; double ms = 0; bwb_hip_place_alt_stats(ctx, &it, &st, &ms); w->alt_ms += ms; w->alt_steps += st; w->alt_items += it; }
}

/* -B: the loci of the same records, resolved where they lie (kernel k_locus behind k_place); on an .ann that is not ascending and disjoint, by
 * the host's resolver */
static void stage_locus(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	if (!m->gpu_loci) { rd->loci = c->host.loci = host_loci(rd, c->n, &m->T); return; }
	uint64_t nr = 0; double ms = 0;
	gpu_ok(bwb_hip_slot_locus(ctx, slot, m->max_mm, &rd->pl, &rd->loci, &c->n), "map_reads", w->gpu);
	bwb_hip_locus_stats(ctx, &nr, &ms);
	w->locus_ms += ms; w->locus_reads += nr;
}

/* -J: the items that lie where the primary lies, from the items and loci the slot already holds (kernels k_join_items / k_join_reads behind
 * k_locus); with the host's loci, the host's rule - the suboptimal byte then needs the hits' scores (slot_result) */
static void stage_join(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	if (m->gpu_loci) {
		uint64_t it = 0, jn = 0; double ms = 0;
		gpu_ok(bwb_hip_slot_join(ctx, slot, m->max_mm, m->max_alt, &rd->pl, &rd->alt_off, &rd->alts, &rd->loci, &rd->joins, &c->n), "map_reads", w->gpu);
		bwb_hip_join_stats(ctx, &it, &jn, &ms);
		w->join_ms += ms; w->join_items += it; w->join_joined += jn;
	} else {
		bwb_result res;
		gpu_ok(bwb_hip_slot_result(ctx, slot, &res), "map_reads", w->gpu);
		rd->joins = c->host.joins = host_joins(rd, c->n, &m->T, m->max_mm, NULL, res.alns, res.aln_off);
	}
	unsigned long long changed = 0, joined = 0; /* the log line's counts, with the team */
#pragma omp parallel for schedule(static) reduction(+ : changed, joined) num_threads(bwb_host_team())
	for (long r = 0; r < (long)c->n; r++) { changed += rd->joins[r].mapq != rd->pl[r].mapq; joined += rd->joins[r].joined; }
	w->join_mapq += changed;
	if (!m->gpu_loci) w->join_joined += joined; /* (on the GPU path join_stats has counted them) */
}

/* -R: RNAME, POS and CIGAR of the placements on bubble records, from the records and loci the slot already holds (kernels k_lift_count / k_lift
 * behind them); with the host's loci, the host's rule */
static void stage_lift(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	if (m->gpu_loci) {
		uint64_t nq = 0, nl = 0, nu = 0; double ms = 0;
		gpu_ok(bwb_hip_slot_lift(ctx, slot, m->max_mm, m->max_alt, &rd->lift_kind, &rd->lift_off, &rd->lift_recs, &nq), "map_reads", w->gpu);
		bwb_hip_lift_stats(ctx, &nl, &nu, &ms);
		w->lift_ms += ms; w->lift_lifted += nl; w->lift_unliftable += nu;
		w->lift_bytes += nq + (nq + 1) * 8 + rd->lift_off[nq] * sizeof(bwb_lift);
	} else {
		c->host.lift = lift_host(rd->pl, rd->loci, c->n, rd->alt_off, rd->alts, m->T.ann, m->T.ann_sorted, m->T.bubble_of, m->T.chrom_of, m->T.bub);
		sam_reads_set_lift(rd, c->host.lift);
		w->lift_lifted += c->host.lift->n_lifted; w->lift_unliftable += c->host.lift->n_unliftable;
	}
}

/* -D: NM and the MD text of every mapped read against the text in HBM (kernels k_md_count / k_md behind them, on the slot's resident reads);
 * with the host's lift records, the host's rule */
static void stage_md(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	if (!c->host.lift) {
		uint64_t nr = 0, nb = 0; double ms = 0;
		gpu_ok(bwb_hip_slot_md(ctx, slot, m->max_mm, m->max_alt, m->lift, &rd->md, &rd->md_off, &rd->md_text, &c->n), "map_reads", w->gpu);
		bwb_hip_md_stats(ctx, &nr, &nb, &ms); /* (the figures of the last call that LAUNCHED: this one, since a chunk's slot is asked once - a second slot_md on it would return its cached records and leave them) */
		w->md_ms += ms; w->md_reads += nr; w->md_bytes += nb;
		w->md_back += (unsigned long long)c->n * sizeof(bwb_md) + ((unsigned long long)c->n + 1) * 8 + rd->md_off[c->n];
	} else {
		c->host.md = md_host(rd->pl, c->n, rd->seq, rd->stride, rd->len, rd->lift_kind, rd->lift_off, rd->lift_recs, m->T.ann, m->text);
		sam_reads_set_md(rd, c->host.md);
		w->md_reads += c->host.md->n_ok; w->md_bytes += c->host.md->off[c->n];
	}
}

/* -A: the allele counts of the slot's reads, added to the context's counters (kernel k_pile behind them, on the slot's resident reads and
 * cached records; nothing per read comes back); with the host's lift or join records, the host's rule into the table itself */
static void stage_pile(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	if (!m->pile_on_host) {
		uint64_t nr = 0, na = 0, nd = 0; double ms = 0;
		if (m->pile_q) gpu_ok(bwb_hip_slot_pile_q(ctx, slot, m->max_mm, m->max_alt, m->lift, m->join, m->pile->min_mapq, m->pile->min_baseq, m->pile->err_cap, &nr), "map_reads", w->gpu);
		else gpu_ok(bwb_hip_slot_pile(ctx, slot, m->max_mm, m->max_alt, m->lift, m->join, m->pile->min_mapq, &nr), "map_reads", w->gpu);
		if (c->n) { /* (a chunk without reads launches nothing) */
			if (m->pile_q) bwb_hip_pileq_stats(ctx, NULL, &na, &nd, &ms); else bwb_hip_pile_stats(ctx, NULL, &na, &ms);
			w->pile_ms += ms; w->pile_reads += nr; w->pile_adds += na; w->pile_dropped += nd;
		}
	} else {
		pthread_mutex_lock(&w->pp->mu); /* (pile_host adds with the whole team: one worker at a time) */
		pile_host_q(m->pile, rd->pl, c->n, rd->seq, rd->stride, rd->len, rd->text, rd->qual_off, rd->lift_kind, rd->lift_off, rd->lift_recs, rd->joins, m->T.ann);
		pthread_mutex_unlock(&w->pp->mu);
	}
}

/* -I: the read support per indel bubble of the slot's reads, added to the context's counters (kernel k_indel behind them, on the slot's cached
 * placement, locus and join records; nothing per read comes back); with the host's loci, the host's rule into the table itself */
static void stage_indel(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c, sam_reads_t *rd) {
	const map_t *m = w->pp->map;
	if (m->gpu_loci) {
		uint64_t nr = 0, na = 0, nc = 0; double ms = 0;
		gpu_ok(bwb_hip_slot_indel(ctx, slot, m->max_mm, m->max_alt, m->join, m->indel->min_mapq, &nr), "map_reads", w->gpu);
		if (c->n) { bwb_hip_indel_stats(ctx, NULL, &na, &nc, &ms); w->indel_ms += ms; w->indel_reads += nr; w->indel_adds += na; w->indel_cands += nc; } /* (a chunk without reads launches nothing) */
	} else {
		pthread_mutex_lock(&w->pp->mu); /* (indel_host adds with the whole team: one worker at a time) */
		indel_host(m->indel, rd->pl, rd->loci, c->n, rd->len, rd->joins);
		pthread_mutex_unlock(&w->pp->mu);
	}
}

/* map: the same hand-over with the chunk's SAM text: the records of the stages the flags ask for, then the worker's team formats the text */
static void retire_map(worker_t *w, bwb_hip_ctx *ctx, int slot, chunk_t *c) {
	const map_t *m = w->pp->map;
	sam_reads_t rd = { .seq = c->fq.seq, .stride = c->fq.stride, .len = c->fq.len, .text = c->fq.text, .name_off = c->fq.name_off, .qual_off = c->fq.qual_off,
	                   .name_len = c->fq.name_len, .first = c->first_read, .bubbles = m->T.bub };
	stage_place(w, ctx, slot, c, &rd);
	if (m->T.bub) stage_locus(w, ctx, slot, c, &rd);
	if (m->join) stage_join(w, ctx, slot, c, &rd);
	if (m->lift) stage_lift(w, ctx, slot, c, &rd);
	if (m->md) stage_md(w, ctx, slot, c, &rd);
	if (m->pile) stage_pile(w, ctx, slot, c, &rd);
	if (m->indel) stage_indel(w, ctx, slot, c, &rd);
	const size_t n = c->n;
	c->n_sam = (n + SAM_BLOCK_READS - 1) / SAM_BLOCK_READS;
	c->sam = (char **)calloc(c->n_sam ? c->n_sam : 1, sizeof(char *));
	c->sam_len = (size_t *)calloc(c->n_sam ? c->n_sam : 1, sizeof(size_t));
#pragma omp parallel for schedule(dynamic, 1) num_threads(bwb_host_team())
	for (long bi = 0; bi < (long)c->n_sam; bi++) {
		const size_t r0 = (size_t)bi * SAM_BLOCK_READS, r1 = r0 + SAM_BLOCK_READS < n ? r0 + SAM_BLOCK_READS : n;
		c->sam[bi] = sam_format_reads(&rd, r0, r1, m->T.ann, m->T.ann_sorted, &c->sam_len[bi]);
	}
	host_recs_free(&c->host);
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
	if (m->indel && m->gpu_loci && (uint64_t)m->T.bub->n > most) most = (uint64_t)m->T.bub->n;
	uint64_t p = count_piece();
	if (p > most) p = most;
	if (p > ((uint64_t)1 << 24)) p = (uint64_t)1 << 24;
	return p < 1 ? 1u : (uint32_t)p;
}

/* the piece-walker of the counters' loops: the size of the piece of n entries that starts at `first` - at most `piece` -, 0 behind the last.
 * `for (s0 = 0; (ns = piece_at(s0, n, piece)); s0 += ns)` walks the n entries and takes no turn on none */
static uint64_t piece_at(uint64_t first, uint64_t n, uint64_t piece) {
	return first >= n ? 0 : (n - first < piece ? n - first : piece);
}

/* map: what the worker's context holds before the stream starts.  In this order, and all of it before the first slot_upload: that sizes the
 * chunk pool from what is free afterwards */
static void worker_map_setup(worker_t *w, bwb_hip_ctx *ctx, double tq, int dbg) {
	const map_t *m = w->pp->map;
	/* The sampled SA (length / 32 x 8 bytes: 1.7 GB at GRCh37 scale) - the loader reads it first (bwt_io.c) - goes up while the library's thread
	 * uploads the index: set_sa uses a stream of its own for that (bwb_hip.hip). */
	while (!__atomic_load_n(&w->BWT->sa_ready, __ATOMIC_ACQUIRE)) { struct timespec ts = { 0, 200000 }; nanosleep(&ts, NULL); }
	gpu_ok(bwb_hip_set_sa(ctx, w->BWT->SA, w->BWT->num_sa), "map_reads", w->device);
	if (dbg) fprintf(stderr, "[bwb host] worker %d: sampled SA resident at +%.3f s\n", w->gpu, wall() - tq);
	/* -B: the record and bubble tables of k_locus (every worker's context gets them; 30 MB at GRCh37 scale) */
	if (m->T.bub && m->gpu_loci)
		gpu_ok(bwb_hip_set_loci(ctx, m->rec_start, m->rec_end, m->T.bubble_of, (uint32_t)m->T.ann->num_seq, m->T.bub->b, (uint32_t)m->T.bub->n), "map_reads", w->device);
	/* -J, -R: the chromosome's record of every bubble, beside them */
	if (m->T.chrom_of && m->gpu_loci) gpu_ok(bwb_hip_set_bubble_chrom(ctx, m->T.chrom_of, (uint32_t)m->T.bub->n), "map_reads", w->device);
	/* -I: the sorted table of the eligible bubbles (16 bytes each, one more per bubble) and the zeroed counters (16 bytes per bubble) */
	if (m->indel && m->gpu_loci) {
		const double t0 = wall();
		uint64_t n_elig = 0;
		gpu_ok(bwb_hip_indel_begin(ctx, m->indel->anchor, &n_elig), "map_reads", w->device);
		w->indel_begin_s = wall() - t0;
		if (n_elig != m->indel->n_tab) bwb_die("map_reads: GPU %d finds %llu eligible bubbles, the host %llu", w->device, (unsigned long long)n_elig, (unsigned long long)m->indel->n_tab);
	}
	/* -D: the forward text (n_fwd / 2 bytes in HBM: 1.7 GB at GRCh37 scale); its bytes are read by the .bwt loader behind the SA (bwt_io.c:
	 * load_bwt_start_job, md.c: md_text_read).  Not with the host's lift records: the host's rule then */
	md_text_wait(m->text);
	if (m->pile) { /* -A: the host's own count of the sites, which every context's must equal, and the table (the first worker here makes them) */
		pthread_mutex_lock(&w->pp->mu);
		if (!m->pile->text) pile_set_text(m->pile, m->text, m->pile_on_host);
		pthread_mutex_unlock(&w->pp->mu);
	}
	const int pile_gpu = m->pile && !m->pile_on_host;
	if ((m->md && !(m->lift && !m->gpu_loci)) || pile_gpu) {
		const double t0 = wall();
		gpu_ok(bwb_hip_set_text(ctx, m->text->codes, m->text->n_fwd), "map_reads", w->device);
		w->text_s = wall() - t0;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: text resident at +%.3f s\n", w->gpu, wall() - tq);
	}
	/* -A: the site index (n_fwd / 8 bytes) and the zeroed counters (16 bytes per site) behind the text */
	if (pile_gpu) {
		const double t0 = wall();
		uint64_t n_sites = 0;
		gpu_ok(bwb_hip_pile_begin(ctx, &n_sites), "map_reads", w->device);
		w->pile_begin_s = wall() - t0;
		if (n_sites != m->pile->n_sites) bwb_die("map_reads: GPU %d counts %llu IUPAC sites in the text, the host's scan of the .ref %llu", w->device, (unsigned long long)n_sites, (unsigned long long)m->pile->n_sites);
	}
	/* -b / -Y: from here on every slot keeps its reads' quality bytes; -Y: the quality sums (16 bytes per site) beside the counters.  Before geno_begin,
	 * which then sizes its output for the 80-byte records */
	if (pile_gpu && m->pile_q) gpu_ok(bwb_hip_pileq_begin(ctx, m->pile->err_cap != 0), "map_reads", w->device);
	/* -G: the scratch and the pinned output of one piece of calls (92 bytes per site of the piece, 48 more per bubble), in every context - which worker
	 * finishes last is not known yet */
	if (m->geno && pile_gpu) gpu_ok(bwb_hip_geno_begin(ctx, geno_piece(m)), "map_reads", w->device);
}

/* map -b / -Y: the chunk's quality lines packed like its reads - one byte per base in FASTQ order, the chunk's stride per read - and handed to the
 * slot behind its upload (the library stages them: the buffer is free at once) */
static void slot_quals_up(worker_t *w, bwb_hip_ctx *ctx, int slot, const chunk_t *c) {
	const double t0 = wall();
	const size_t stride = c->fq.stride;
	uint8_t *q = (uint8_t *)calloc((size_t)c->fq.n * stride + 1, 1);
	if (!q) bwb_die("map_reads: no memory for the qualities of %u reads", c->fq.n);
#pragma omp parallel for schedule(static) num_threads(bwb_host_team())
	for (long r = 0; r < (long)c->fq.n; r++) memcpy(q + (size_t)r * stride, c->fq.text + c->fq.qual_off[r], c->fq.len[r] <= stride ? c->fq.len[r] : stride);
	gpu_ok(bwb_hip_slot_quals(ctx, slot, q, c->fq.stride), "map_reads", w->device);
	free(q);
	w->quals_s += wall() - t0; w->quals_bytes += (unsigned long long)c->fq.n * stride;
}

/* The stream.  Chunks go through the slots of the context: while the search slice of chunk j runs, chunk j+1 is already uploaded and queued
 * behind it and the hits of chunk j-1 are on their way back; a slice parks its unfinished reads for the next one instead of draining
 * (include/bwbble_hip.h), so the GPU never runs a batch's tail alone. */
static void worker_stream(worker_t *w, bwb_hip_ctx *ctx, double tq, int dbg) {
	pipe_t *pp = w->pp;
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
		gpu_ok(bwb_hip_slot_upload(ctx, slot, w->params, c->fq.seq, c->fq.len, c->fq.n, c->fq.stride, c->carry, c->carry_len), "align_reads_inexact_gpu", w->device);
		if (pp->map && pp->map->pile_q && !pp->map->pile_on_host) slot_quals_up(w, ctx, slot, c);
		if (j == 0) { /* the first chunk is staged, scratch and pool exist: now the index must be complete */
			gpu_ok(bwb_hip_ctx_index_wait(ctx, &w->t_ctx), "align_reads_inexact_gpu", w->device);
			uint64_t pb = 0;
			bwb_hip_setup_times(ctx, NULL, &w->t_pool, &pb);
			w->pool_bytes = pb;
			if (dbg) fprintf(stderr, "[bwb host] worker %d (device %d): index upload %.3f s, chunk pool %.1f GB allocated in %.3f s, first chunk staged at +%.3f s\n", w->gpu, w->device, w->t_ctx,
			                 (double)pb / (1u << 30), w->t_pool, wall() - tq);
		}
		gpu_ok(bwb_hip_slot_submit(ctx, slot), "align_reads_inexact_gpu", w->device);
		if (j == 0) w->t_first_submit = wall() - tq;
		if (!pp->map) { free(c->fq.seq); free(c->fq.len); c->fq.seq = NULL; c->fq.len = NULL; } /* (staged by the library: the caller's buffers are free; map prints the bases) */
		free(c->carry); c->carry = NULL;
		in_slot[slot] = c;
		w->n_reads += c->fq.n;
		j++;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: chunk %zu (%u reads) submitted at +%.3f s\n", w->gpu, c->idx, c->fq.n, wall() - tq);
	}
}

/* map -A, -I: the stream has ended and every chunk of this worker is retired - its counters (bubbles: those of -I's n bubbles, else those of
 * -A's n sites) come back in bounded pieces and are summed on the host; returns the pieces */
enum { BACK_SITES, BACK_BUBBLES, BACK_QSUMS }; /* -A's counters, -I's, -Y's quality sums */
static uint64_t counters_back(worker_t *w, bwb_hip_ctx *ctx, int which, uint64_t n) {
	pipe_t *pp = w->pp;
	const uint64_t PIECE = count_piece();
	uint32_t *buf = (uint32_t *)malloc((size_t)(n < PIECE ? n : PIECE) * 16 + 16);
	uint64_t turns = 0, ns;
	for (uint64_t s0 = 0; (ns = piece_at(s0, n, PIECE)); s0 += ns, turns++) {
		gpu_ok(which == BACK_BUBBLES ? bwb_hip_indel_counts(ctx, s0, ns, buf) : which == BACK_QSUMS ? bwb_hip_pileq_sums(ctx, s0, ns, buf) : bwb_hip_pile_counts(ctx, s0, ns, buf), "map_reads", w->device);
		pthread_mutex_lock(&pp->mu);
		if (which == BACK_BUBBLES) indel_add(pp->map->indel, s0, ns, buf); else if (which == BACK_QSUMS) pile_add_q(pp->map->pile, s0, ns, buf); else pile_add(pp->map->pile, s0, ns, buf);
		pthread_mutex_unlock(&pp->mu);
	}
	free(buf);
	return turns;
}
static void worker_map_counters(worker_t *w, bwb_hip_ctx *ctx, int dbg) {
	const map_t *m = w->pp->map;
	if (m->pile && !m->pile_on_host) {
		const double t0 = wall();
		uint64_t turns = counters_back(w, ctx, BACK_SITES, m->pile->n_sites);
		if (m->pile->err_cap) turns += counters_back(w, ctx, BACK_QSUMS, m->pile->n_sites); /* -Y: the quality sums beside them */
		w->pile_fetch_s = wall() - t0;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: the counters of %llu sites read back in %llu pieces\n", w->gpu, (unsigned long long)m->pile->n_sites, (unsigned long long)turns);
	}
	if (m->indel && m->gpu_loci) {
		const double t0 = wall();
		const uint64_t turns = counters_back(w, ctx, BACK_BUBBLES, (uint64_t)m->T.bub->n);
		w->indel_fetch_s = wall() - t0;
		if (dbg) fprintf(stderr, "[bwb host] worker %d: the counters of %llu bubbles read back in %llu pieces\n", w->gpu, (unsigned long long)m->T.bub->n, (unsigned long long)turns);
	}
}

/* map -G: this worker's counters are in the host's sums.  The worker that completes the count calls the genotypes on its own context: with several
 * workers it first puts the host's summed tables back over its counters, with one its counters are the sums already and nothing is uploaded.  Then
 * the sites and the bubbles are walked in pieces; what comes back is the called entries' records alone, which geno.c keeps for the writer. */
static void worker_map_genotypes(worker_t *w, bwb_hip_ctx *ctx, int dbg) {
	pipe_t *pp = w->pp;
	const map_t *m = pp->map;
	geno_t *G = m->geno;
	pthread_mutex_lock(&pp->mu);
	const int last = ++pp->n_finished == pp->n_workers;
	pthread_mutex_unlock(&pp->mu);
	const int sites_gpu = !m->pile_on_host, bubs_gpu = sites_gpu && m->indel && m->gpu_loci;
	if (!last || !sites_gpu) return;
	const uint64_t PIECE = count_piece(), GP = geno_piece(m), n_sites = m->pile->n_sites, n_bub = bubs_gpu ? (uint64_t)m->T.bub->n : 0;
	uint64_t ns;
	double t0 = wall();
	if (pp->n_workers > 1) {
		for (uint64_t s0 = 0; (ns = piece_at(s0, n_sites, PIECE)); s0 += ns, G->put_pieces++)
			gpu_ok(bwb_hip_pile_put(ctx, s0, ns, m->pile->counts + s0 * 4), "map_reads", w->device);
		for (uint64_t s0 = 0; G->weighted && (ns = piece_at(s0, n_sites, PIECE)); s0 += ns, G->put_pieces++)
			gpu_ok(bwb_hip_pileq_put(ctx, s0, ns, m->pile->qsum + s0 * 4), "map_reads", w->device);
		for (uint64_t s0 = 0; (ns = piece_at(s0, n_bub, PIECE)); s0 += ns, G->put_pieces++)
			gpu_ok(bwb_hip_indel_put(ctx, s0, ns, m->indel->counts + s0 * 4), "map_reads", w->device);
	}
	G->put_s = wall() - t0;
	t0 = wall();
	double ms = 0;
	for (uint64_t s0 = 0; (ns = piece_at(s0, n_sites, GP)); s0 += ns, G->pieces++) {
		const bwb_geno_site *recs = NULL; const bwb_geno_site_q *recs_q = NULL; uint64_t k = 0;
		if (G->weighted) gpu_ok(bwb_hip_geno_sites_q(ctx, s0, ns, G->err, G->min_depth, &recs_q, &k), "map_reads", w->device);
		else gpu_ok(bwb_hip_geno_sites(ctx, s0, ns, G->err, G->min_depth, &recs, &k), "map_reads", w->device);
		bwb_hip_geno_stats(ctx, NULL, NULL, &ms);
		G->kernel_ms += ms;
		if (G->weighted) geno_take_sites_q(G, recs_q, k); else geno_take_sites(G, recs, k);
	}
	for (uint64_t s0 = 0; (ns = piece_at(s0, n_bub, GP)); s0 += ns, G->pieces++) {
		const bwb_geno_bubble *recs = NULL; uint64_t k = 0;
		gpu_ok(bwb_hip_geno_bubbles(ctx, s0, ns, G->err, G->min_depth, &recs, &k), "map_reads", w->device);
		bwb_hip_geno_stats(ctx, NULL, NULL, &ms);
		G->kernel_ms += ms;
		geno_take_bubbles(G, recs, k);
	}
	G->call_s = wall() - t0;
	G->worker = w->gpu;
	if (dbg) fprintf(stderr, "[bwb host] worker %d: genotypes called by this worker, the last of %d: %llu pieces of tables put back in %.3f s, %llu pieces called in %.3f s: sites %llu  bubbles %llu  kernels %.3f ms\n",
	                 w->gpu, pp->n_workers, (unsigned long long)G->put_pieces, G->put_s, (unsigned long long)G->pieces, G->call_s, (unsigned long long)G->n_sites, (unsigned long long)G->n_bubs, G->kernel_ms);
}

/* One host thread per GPU: the context, for `map` what it holds beside the index, the stream, for `map` the counters and the calls */
static void *gpu_worker(void *arg) {
	worker_t *w = (worker_t *)arg;
	bwb_hip_ctx *ctx = NULL;
	const int dbg = getenv("BWB_DEBUG") != NULL;
	pin_to_device_node(w->device, dbg);
	const double tq = wall();
	const bwtint_t hdr[5] = { w->BWT->length, w->BWT->num_words, w->BWT->num_sa, w->BWT->num_occ, w->BWT->sa0_index };
	/* The index goes to the GPU - on a thread of the library - while the loader threads are still reading the tail of the .bwt file
	 * (bwt_io.c), and while this thread already uploads its first chunk: that first slot_upload sizes and allocates the context's scratch
	 * and its heap chunk pool (seconds of hipMalloc at GRCh37 scale, which rounds 3-5 paid AFTER the index upload); slot_submit waits for
	 * the index by itself. */
	gpu_ok(bwb_hip_ctx_create_async(w->device, hdr, w->BWT->C, w->BWT->bwt, w->BWT->O, w->BWT->loader ? &w->BWT->blocks_ready : NULL, &ctx), "align_reads_inexact_gpu", w->device);
	if (dbg) fprintf(stderr, "[bwb host] worker %d: context created at +%.3f s (index upload under way)\n", w->gpu, wall() - tq);
	if (w->pp->map) worker_map_setup(w, ctx, tq, dbg);
	worker_stream(w, ctx, tq, dbg);
	if (w->pp->map) worker_map_counters(w, ctx, dbg);
	if (w->pp->map && w->pp->map->geno) worker_map_genotypes(w, ctx, dbg);
	bwb_stats st;
	gpu_ok(bwb_hip_flush(ctx) || bwb_hip_get_stats(ctx, &st), "align_reads_inexact_gpu", w->device);
	w->total = st;
	w->kernel_ms = st.ms_calc_d + st.ms_search;
	bwb_hip_ctx_destroy(ctx);
	if (dbg) fprintf(stderr, "[bwb host] worker %d: done %.3f s\n", w->gpu, wall() - tq);
	return NULL;
}

/* the summary's figures: worker w folded into the total t - times by maximum (the workers run side by side), counts by sum */
static void max_of(double *t, double v) { if (v > *t) *t = v; }
static void fold_worker(worker_t *t, const worker_t *w) {
	max_of(&t->kernel_ms, w->kernel_ms); max_of(&t->t_ctx, w->t_ctx); max_of(&t->t_pool, w->t_pool); max_of(&t->t_first_submit, w->t_first_submit);
	if (w->pool_bytes > t->pool_bytes) t->pool_bytes = w->pool_bytes;
	t->total.visits_single += w->total.visits_single; t->total.visits_alphabet += w->total.visits_alphabet;
	t->total.heap_pops += w->total.heap_pops; t->total.n_alignments += w->total.n_alignments; t->total.n_overflow_reads += w->total.n_overflow_reads;
	max_of(&t->place_ms, w->place_ms); t->place_steps += w->place_steps;
	max_of(&t->alt_ms, w->alt_ms); t->alt_steps += w->alt_steps; t->alt_items += w->alt_items;
	max_of(&t->locus_ms, w->locus_ms); t->locus_reads += w->locus_reads;
	max_of(&t->join_ms, w->join_ms); t->join_items += w->join_items; t->join_joined += w->join_joined; t->join_mapq += w->join_mapq;
	max_of(&t->lift_ms, w->lift_ms); t->lift_lifted += w->lift_lifted; t->lift_unliftable += w->lift_unliftable; t->lift_bytes += w->lift_bytes;
	max_of(&t->md_ms, w->md_ms); max_of(&t->text_s, w->text_s); t->md_reads += w->md_reads; t->md_bytes += w->md_bytes; t->md_back += w->md_back;
	max_of(&t->pile_ms, w->pile_ms); max_of(&t->pile_begin_s, w->pile_begin_s); max_of(&t->pile_fetch_s, w->pile_fetch_s); t->pile_reads += w->pile_reads; t->pile_adds += w->pile_adds;
	max_of(&t->quals_s, w->quals_s); t->quals_bytes += w->quals_bytes; t->pile_dropped += w->pile_dropped;
	max_of(&t->indel_ms, w->indel_ms); max_of(&t->indel_begin_s, w->indel_begin_s); max_of(&t->indel_fetch_s, w->indel_fetch_s);
	t->indel_reads += w->indel_reads; t->indel_adds += w->indel_adds; t->indel_cands += w->indel_cands;
}

/* map: one line per stage of the result stream, from the folded workers; a stage that ran on the host says so and why */
static void print_map_summary(const map_t *map, const worker_t *t, uint64_t n_reads) {
	printf("placements on the GPU: reads %llu  rank-block visits %llu  kernel %.3f ms", (unsigned long long)n_reads, t->place_steps, t->place_ms);
	if (map->T.bub && map->gpu_loci) printf("  loci resolved %llu  k_locus %.3f ms", t->locus_reads, t->locus_ms); /* -B: the loci of the same reads */
	else if (map->T.bub) printf("  loci resolved %llu on the host%s (the .ann records are not ascending and disjoint)", (unsigned long long)n_reads, map->join ? " and joined there" : "");
	printf("\n");
	if (map->join && map->gpu_loci) printf("placements joined by locus on the GPU: items %llu  joined %llu  reads with another MAPQ %llu  kernels %.3f ms\n", t->join_items, t->join_joined, t->join_mapq, t->join_ms);
	else if (map->join) printf("placements joined by locus on the host: joined %llu  reads with another MAPQ %llu\n", t->join_joined, t->join_mapq);
	if (map->lift && map->gpu_loci) printf("placements lifted to chromosome coordinates on the GPU: lifted %llu  not liftable %llu  kernels %.3f ms  bytes to the host %llu\n", t->lift_lifted, t->lift_unliftable, t->lift_ms, t->lift_bytes);
	else if (map->lift) printf("placements lifted to chromosome coordinates on the host (the .ann records are not ascending and disjoint): lifted %llu  not liftable %llu\n", t->lift_lifted, t->lift_unliftable);
	if (map->md && !(map->lift && !map->gpu_loci))
		printf("NM and MD against the text on the GPU: reads %llu  MD bytes %llu  kernels %.3f ms  bytes to the host %llu  text %llu characters read in %.3f s, set in %.3f s\n", t->md_reads, t->md_bytes, t->md_ms, t->md_back,
		       (unsigned long long)map->text->n_fwd, map->text->seconds, t->text_s);
	else if (map->md) printf("NM and MD against the text on the host (the .ann records are not ascending and disjoint): reads %llu  MD bytes %llu\n", t->md_reads, t->md_bytes);
	if (map->pile && !map->pile_on_host)
		printf("allele counts at the text's IUPAC sites on the GPU: sites %llu  reads counted %llu  adds %llu  k_pile %.3f ms  site index and counters %llu bytes, built in %.3f s  counters read back in %.3f s\n",
		       (unsigned long long)map->pile->n_sites, t->pile_reads, t->pile_adds, t->pile_ms, (unsigned long long)((map->text->n_fwd + 31) / 32 * 4 + map->pile->n_sites * 16), t->pile_begin_s, t->pile_fetch_s);
	else if (map->pile) printf("allele counts at the text's IUPAC sites on the host (the .ann records are not ascending and disjoint): sites %llu  reads counted %llu  adds %llu\n",
		                   (unsigned long long)map->pile->n_sites, (unsigned long long)map->pile->reads, (unsigned long long)map->pile->adds);
	if (map->pile && !map->pile_on_host && map->pile_q)
		printf("base qualities in the counts on the GPU (k_pile_q): minimum %d  bases dropped %llu  quality sums %s  quality bytes to the slots %llu, packed and staged in %.3f s\n",
		       map->pile->min_baseq, t->pile_dropped, map->pile->err_cap ? "kept (-Y)" : "not kept", t->quals_bytes, t->quals_s);
	if (map->indel && map->gpu_loci)
		printf("read support per indel bubble on the GPU: anchor %d  eligible bubbles %llu  refused and skipped %llu  reads counted %llu  adds %llu  candidates %llu  k_indel %.3f ms  table and counters %llu bytes, sorted in %.3f s, resident in %.3f s  counters read back in %.3f s\n",
		       map->indel->anchor, (unsigned long long)map->indel->n_tab, (unsigned long long)map->indel->n_refused, t->indel_reads, t->indel_adds, t->indel_cands, t->indel_ms,
		       (unsigned long long)(map->indel->n_tab * 16 + (uint64_t)map->T.bub->n * 17), map->indel->sort_s, t->indel_begin_s, t->indel_fetch_s);
	else if (map->indel) printf("read support per indel bubble on the host (the .ann records are not ascending and disjoint): anchor %d  eligible bubbles %llu  refused and skipped %llu  reads counted %llu  adds %llu  candidates %llu\n",
		                    map->indel->anchor, (unsigned long long)map->indel->n_tab, (unsigned long long)map->indel->n_refused, (unsigned long long)map->indel->reads, (unsigned long long)map->indel->adds, (unsigned long long)map->indel->cands);
	if (map->geno && !map->pile_on_host) /* -G */
		printf("genotype calls on the GPU (worker %d): error phred %d  minimum depth %lld  sites called %llu%s  bubbles called %llu  kernels %.3f ms  pieces %llu  bytes to the host %llu  tables put back in %llu pieces, %.3f s  called in %.3f s\n",
		       map->geno->worker, map->geno->err, (long long)map->geno->min_depth, (unsigned long long)map->geno->n_sites, map->indel && !map->gpu_loci ? " (the bubbles follow on the host)" : "",
		       (unsigned long long)map->geno->n_bubs, map->geno->kernel_ms, (unsigned long long)map->geno->pieces,
		       (unsigned long long)(map->geno->n_sites * (map->geno->weighted ? sizeof(bwb_geno_site_q) : sizeof(bwb_geno_site)) + map->geno->n_bubs * sizeof(bwb_geno_bubble) + map->geno->pieces * 8), (unsigned long long)map->geno->put_pieces, map->geno->put_s, map->geno->call_s);
	if (map->max_alt)
		printf("other placements on the GPU (-X %d): items %llu (%.3f per read)  rank-block visits %llu  kernels %.3f ms\n", map->max_alt, t->alt_items,
		       n_reads ? (double)t->alt_items / (double)n_reads : 0.0, t->alt_steps, t->alt_ms);
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
	worker_t tot; /* the workers folded once: times by maximum, counts by sum */
	memset(&tot, 0, sizeof(tot));
	for (int g = 0; g < n_gpus; g++) {
		pthread_join(th[g], NULL);
		fold_worker(&tot, &ws[g]);
		if (n_gpus > 1) /* one line per worker: an uneven node (a slow link, a busy socket) shows here, not in the total */
			printf("  GPU %d (device %d, NUMA node %d): reads %llu  kernel %.1f ms  index to HBM %.2f sec  launches %llu  parked reads %llu  re-run reads %llu\n", g, ws[g].device,
			       bwb_hip_device_numa_node(ws[g].device), (unsigned long long)ws[g].n_reads, ws[g].kernel_ms, ws[g].t_ctx,
			       (unsigned long long)ws[g].total.launches_search, (unsigned long long)ws[g].total.n_parked_reads, (unsigned long long)ws[g].total.n_overflow_reads);
	}
	const double dt = wall() - t0;
	printf("GPUs: %d  reads: %llu  wall: %.3f sec (%.0f reads/s incl. index upload)  kernel: %.1f ms  index to HBM: %.2f sec  first chunk parsed after: %.2f sec  rank-block visits: %llu  hits: %llu  re-run reads: %llu\n",
	       n_gpus, (unsigned long long)pp.n_reads, dt, pp.n_reads / (dt > 0 ? dt : 1), tot.kernel_ms, tot.t_ctx, pp.t_first_chunk, (unsigned long long)(tot.total.visits_single + tot.total.visits_alphabet),
	       (unsigned long long)tot.total.n_alignments, (unsigned long long)tot.total.n_overflow_reads);
	if (map) print_map_summary(map, &tot, pp.n_reads);
	/* where the start-up went (the three overlap): the .bwt file in memory | the index in HBM | the chunk pool's hipMalloc | first slice queued */
	printf("start-up: .bwt read %.2f sec | index to HBM %.2f sec | chunk pool %.1f GB in %.2f sec | first slice queued after %.2f sec\n",
	       bwt_load_seconds(BWT), tot.t_ctx, (double)tot.pool_bytes / (1u << 30), tot.t_pool, tot.t_first_submit);
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
int map_reads(char *fastaFname, char *readsFname, char *samFname, aln_params_t *params, const map_opts_t *o, int n_gpus) {
	printf("**** BWBBLE Read Mapping (align + aln2sam in one pass) ****\n");
	/* -A, -I, -G: the files are opened before anything is loaded; until they are written, a run that stops leaves none behind */
	host_outs_t out;
	host_outs_open(&out, o);
	pile_t *pile = out.pile;
	indel_t *indel = out.indel;
	geno_t *geno = out.geno;
	/* -B: the table first (a refused table stops the run before anything is created) */
	bubble_table_t *bub = o->bubbleFname ? load_bubbles(o->bubbleFname) : NULL;
	if (o->lift && bub) lift_check_table(bub); /* -R (main.c: only with -B): a bubble the rule refuses is named here */
	/* -D: a missing <seq_fasta>.ref, or one of another size than the .ann says, stops the run here; the .bwt loader reads its forward half, behind the sampled SA */
	md_text_t *text = host_text_open(fastaFname, o, &out, 1); /* (-A loads it the same way, with or without -D) */
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
	const int join = o->join && bub && o->max_alt, lift = o->lift && bub;
	int32_t *chrom_of = join || lift || indel ? bubble_chrom_of(ann, bubble_of, bub, join ? "-J" : lift ? "-R" : o->indelFname ? "-I" : "-G") : NULL;
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
	const map_t m = { .max_mm = o->max_mm, .max_alt = o->max_alt, .T = { .ann = ann, .ann_sorted = sam_ann_sorted(ann), .bub = bub, .bubble_of = bubble_of, .chrom_of = chrom_of },
	                  .gpu_loci = gpu_loci, .rec_start = rec_start, .rec_end = rec_end, .join = join, .lift = lift, .text = text,
	                  .md = o->md, .pile = pile, .pile_on_host = pile && bub && !gpu_loci && (lift || join), .pile_q = pile && (pile->min_baseq || pile->err_cap), .indel = indel, .geno = geno };

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
	free(bubble_of); free(chrom_of); free(rec_start); free(rec_end); free_bubbles(bub); host_outs_free(&out); md_text_free(text);
	return 0;
}
