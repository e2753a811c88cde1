/*
 * bwbble_hip.h - C-ABI of the MI355X (gfx950) read-alignment library, libbwbble_hip.so.
 *
 * This is the drop-in boundary for BWBBLE's `align` hot path.  The reference has no plugin/FFI
 * layer; its seam is the function pair selected in align_reads (mg-aligner/align.c:72-76):
 *
 *     int align_reads_inexact[_parallel](bwt_t*, reads_t*, sa_intv_list_t*, aln_params_t*, char* alnFname);
 *                                                               (mg-aligner/inexact_match.h:39-40)
 *
 * A maintainer adds `align_reads_inexact_gpu()` with that same signature next to them (see
 * INTEGRATION.md and bwbble_amd/host/align_gpu.c) and it calls the entry points below.  Plain
 * pointers and sizes only; every function returns 0 on success or a negative BWB_E_* code, never
 * exits the process (the reference printf+exit(1)s; the host wrapper keeps that behaviour), and
 * bwb_hip_last_error() gives the message.  Calls on distinct contexts are thread-safe (one host
 * thread per GPU); a context must not be used from two threads at once.
 */
#ifndef BWBBLE_HIP_H
#define BWBBLE_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BWB_OK 0
#define BWB_E_ARG (-1)         /* bad argument / unsupported parameter combination */
#define BWB_E_HIP (-2)         /* HIP runtime error (no device, out of memory, launch failure) */
#define BWB_E_OVERFLOW (-3)    /* a read exceeded the largest per-read scratch class */
#define BWB_E_STATE (-4)       /* call order violated (e.g. run before upload) */

/* mirror of aln_params_t (mg-aligner/align.h:48-79): same fields, same order, same meaning.
 * Defaults are set_default_aln_params (mg-aligner/align.c:22-38). n_threads is ignored by the GPU. */
typedef struct {
	int32_t max_diff, max_gapo, max_gape, max_entries;
	int32_t mm_score, gapo_score, gape_score;
	int32_t seed_length, max_diff_seed, max_best, no_indel_length;
	int32_t matched_Ncontig, use_precalc, is_multiref, n_threads;
} bwb_params;

/* One alignment hit = one aln_t (mg-aligner/align.h:81-90) in fixed 48-byte form (ABI version 3; 32 bytes with four runs before).
 * The edit path is all STATE_M except for <= 8 gap runs (one per gap open: -o up to 8):
 * run = start_index_in_path | (run_length << 8) | (is_deletion << 15); unused runs are 0xFFFF. */
#define BWB_MAX_GAP_RUNS 8
typedef struct {
	uint64_t L, U;           /* SA interval */
	uint16_t score;          /* aln_t.score: the full int aln_score(num_mm, num_gapo, num_gape) (inexact_match.c:332,348); up to 1 024 heap
	                            buckets are accepted, so it does not fit the 8 bits it had in ABI version 1 */
	uint8_t num_mm, num_gapo, num_gape, reserved;
	uint16_t aln_length;     /* 8-bit wrapped like aln_entry_t.aln_length (align.h:104) */
	uint16_t gap_run[BWB_MAX_GAP_RUNS];
	uint64_t reserved2;      /* (zero; the record is three 16-byte words) */
} bwb_aln;

/* Results of one batch: read r owns alns[aln_off[r] .. aln_off[r+1]) in discovery order
 * (== the order of alns->entries in the reference, align.c:286-297). Owned by the context;
 * valid until the next bwb_hip_batch_* call on it. */
typedef struct {
	uint32_t n_reads;
	const uint64_t *aln_off;     /* n_reads + 1 */
	const bwb_aln *alns;
} bwb_result;

/* Work/timing counters since the last bwb_hip_reset_stats / bwb_hip_batch_run (SURVEY.md 8(d) counting rules) */
typedef struct {
	uint64_t visits_single;      /* rank-block visits made for the 7-code exact steps (calculate_d, exact tail) */
	uint64_t visits_calc_d;      /* the part of visits_single made by the calculate_d kernel */
	uint64_t visits_alphabet;    /* rank-block visits made for O_alphabet (2 per expansion unless special-cased) */
	uint64_t heap_pops, heap_pushes;
	uint64_t n_alignments;
	uint64_t n_overflow_reads;   /* reads re-run with a larger scratch class (still on the GPU) */
	uint64_t n_parked_reads;     /* reads that were parked at the end of a slice and resumed by the next launch */
	uint64_t bucket_loads_search; /* 128-byte device buckets the search kernel fetched (a same-bucket L-1/U pair counts once) */
	uint64_t bucket_loads_calc_d; /* the same for the calculate_d kernel */
	uint64_t lane_iterations, wave_iterations; /* search loop iterations of busy lanes / of waves: their ratio = lanes busy of 64 */
	uint64_t heap_entries_stored, heap_entries_loaded; /* heap entries the search kernel wrote to / read from its chunk pool (deletion children
	                                                      travel as one group entry and a match child that is popped next stays in registers: fewer than pushes) */
	uint64_t record_loads;       /* 16-byte records (four read positions each: D, D_seed, bases) the search kernel loaded */
	double ms_calc_d;            /* HIP-event time of the calculate_d kernel(s) that have finished */
	double ms_search;            /* HIP-event time of the inexact-search kernel(s) that have finished, all passes */
	double ms_total;             /* batch_run: wall time of the call */
	uint32_t launches_calc_d, launches_search;
} bwb_stats;

typedef struct bwb_hip_ctx bwb_hip_ctx;

/* Version of this interface: 3 since bwb_aln holds eight gap runs in 48 bytes (round 5; 2: bwb_aln.score 16 bits wide, round 4).  A binding compiled against another version must not
 * be used with the library: compare BWB_HIP_ABI_VERSION with bwb_hip_abi_version() at start-up. */
#define BWB_HIP_ABI_VERSION 3
int bwb_hip_abi_version(void);

int bwb_hip_device_count(void);
int bwb_hip_device_numa_node(int device);                    /* NUMA node of the device's PCIe root, -1 = unknown / single node */
const char *bwb_hip_last_error(void);
void bwb_default_params(bwb_params *p);                       /* align.c:22-38 */

/* Creates a context on `device` and builds the device FM-index from the reference's in-memory
 * bwt_t arrays (mg-aligner/bwt.h:19-40, file layout bwt.c:66-82):
 *   hdr = {length, num_words, num_sa, num_occ, sa0_index}, C[17], bwt[num_words], O[num_occ*16].
 * The index is re-laid-out on the GPU into 128-byte rank buckets of 64 BWT characters (2 bytes of device memory per BWT
 * character); the host arrays are not referenced after return.  One context per device is the intended use: with the first batch a context sizes its heap
 * chunk pool from what the device has free (minus a reserve for the re-run classes and further slots), so a second context
 * on the same device - tests do that - should be given a budget with the environment variable BWB_POOL_GB. */
int bwb_hip_ctx_create(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt,
                       const uint64_t *O, bwb_hip_ctx **out);
/* The same while the host arrays are still being filled (`bwbble align` reads the 12 GB .bwt of a GRCh37-scale index with several
 * threads while the GPUs already take it in): *blocks_ready = number of leading 128-character blocks whose bwt words [16 k, 16 k + 16)
 * and O rows k are in memory, advanced by the caller's loader with release semantics; the upload of a chunk waits for it.  NULL =
 * everything is there (= bwb_hip_ctx_create).  Several contexts (one per GPU) may follow the same counter. */
int bwb_hip_ctx_create_streamed(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt,
                                const uint64_t *O, const volatile uint64_t *blocks_ready, bwb_hip_ctx **out);
/* The same, returning as soon as the context exists: the index upload runs on a thread of the library, so the caller can already
 * slot_upload its first batch - which also sizes and allocates the context's scratch and heap chunk pool, seconds of hipMalloc at GRCh37
 * scale - while the index is still on its way.  The host arrays (and *blocks_ready) must stay valid until bwb_hip_ctx_index_wait has
 * returned; every entry point that launches a kernel waits by itself (slot_submit, batch_run, calc_d, rank16, rank_bench, locate), and so
 * does ctx_destroy.  index_wait reports an upload error (the message through bwb_hip_last_error) and, optionally, the upload's seconds.
 * (Added in round 6 without a version change: no structure or existing entry point changed.) */
int bwb_hip_ctx_create_async(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt,
                             const uint64_t *O, const volatile uint64_t *blocks_ready, bwb_hip_ctx **out);
int bwb_hip_ctx_index_wait(bwb_hip_ctx *ctx, double *seconds);
/* where a context's start-up time went: seconds of the index upload (-1 while it is running), seconds spent in the hipMalloc of the heap
 * chunk pool and the pool's size (any pointer may be NULL) */
int bwb_hip_setup_times(bwb_hip_ctx *ctx, double *index_seconds, double *pool_seconds, uint64_t *pool_bytes);
/* The calculate_d table of the context: the state of calculate_d (inexact_match.c:171-254) after its first K steps for every
 * K-mer, from which kl_calc_d starts a read and its seed.  Built by the first slot_submit / batch_run whose batch has at least 200 000 reads
 * (environment: BWB_DTAB=1 always, 0 never; BWB_DTAB_K: K, default and maximum 12); K = 0: none.  Results do not depend on it. */
int bwb_hip_dtab_info(bwb_hip_ctx *ctx, int *K, double *build_seconds, uint64_t *bytes);
void bwb_hip_ctx_destroy(bwb_hip_ctx *ctx);

/* Replaces align_reads_inexact[_parallel] for one batch (inexact_match.c:25-168): calculate_d x2 +
 * inexact_match for n_reads reads. reads_fwd holds read->seq codes (A0 G1 C2 T3 N4, io.h:112-130),
 * `stride` bytes per read; the reverse complement (read->rc, io.c:502-504) is formed on the GPU.
 * == batch_upload + batch_run + batch_result. */
int bwb_hip_align_batch(bwb_hip_ctx *ctx, const bwb_params *p, const uint8_t *reads_fwd, const uint16_t *lens,
                        uint32_t n_reads, uint32_t stride, bwb_result *out);

/* The same in three steps, so that a caller can time the GPU work with inputs resident in HBM. */
int bwb_hip_batch_upload(bwb_hip_ctx *ctx, const bwb_params *p, const uint8_t *reads_fwd, const uint16_t *lens,
                         uint32_t n_reads, uint32_t stride);
int bwb_hip_batch_run(bwb_hip_ctx *ctx);                       /* kernels only; blocks until done; resets the statistics first */
int bwb_hip_batch_result(bwb_hip_ctx *ctx, bwb_result *out);  /* D2H copy of the hits */
int bwb_hip_get_stats(bwb_hip_ctx *ctx, bwb_stats *out);
int bwb_hip_reset_stats(bwb_hip_ctx *ctx);

/* Streaming form of the same (what `bwbble align` uses for a FASTQ of many batches, inexact_match.c:103-165): up to
 * BWB_MAX_SLOTS batches are resident per context.  slot_upload copies the reads to HBM on a copy stream (the caller's
 * buffers are free when it returns); slot_submit queues calculate_d and one slice of the search for that slot and returns at
 * once - a slice does not drain: the reads still under way when the slot's cursor runs out are parked and resumed by the
 * next submitted slot's slice, so the heavy tail of one batch overlaps the bulk of the next; slot_wait blocks until every
 * read of the slot is done (launching a draining slice if nothing else is queued); slot_result = slot_wait + D2H of the
 * hits on a result stream, valid until the slot is uploaded again; flush = wait for every slot.  All slots in flight use
 * the same parameters (a slot_upload with different ones flushes first).  Same result bytes as align_batch.
 *
 * Reads that are not longer than the seed (len <= seed_length): the reference computes D_seed only for longer reads
 * (inexact_match.c:62-64) yet inexact_match consults it for every read (:321-328), so its serial path (-t 1) gives a short
 * read the bounds of the last longer read before it in the file (zeros if there is none; with -t N it depends on the thread
 * that happens to process the read).  The library reproduces the serial behaviour: inside a batch it knows the order; for
 * the head of a batch the caller passes that last longer read of the earlier batches as carry_seq/carry_len (read->seq
 * codes; NULL/0 = none, which is also what batch_upload/align_batch assume). */
#define BWB_MAX_SLOTS 8
int bwb_hip_slot_upload(bwb_hip_ctx *ctx, int slot, const bwb_params *p, const uint8_t *reads_fwd, const uint16_t *lens,
                        uint32_t n_reads, uint32_t stride, const uint8_t *carry_seq, uint32_t carry_len);
int bwb_hip_slot_submit(bwb_hip_ctx *ctx, int slot);
int bwb_hip_slot_wait(bwb_hip_ctx *ctx, int slot);
int bwb_hip_slot_result(bwb_hip_ctx *ctx, int slot, bwb_result *out);
int bwb_hip_flush(bwb_hip_ctx *ctx);

/* calculate_d for the uploaded batch (inexact_match.c:171-254): D and D_seed of every read as
 * (num_diff, sa_intv_width) int32 pairs, out_D[n_reads][max_len+1][2], out_Dseed[n_reads][seed_length+1][2]
 * (rows beyond a read's length are 0; D_seed rows are 0 when len <= seed_length). For parity tests. */
int bwb_hip_calc_d(bwb_hip_ctx *ctx, int32_t *out_D, int32_t *out_Dseed);

/* O_alphabet (bwt.c:374-438) for n positions: out[q][j] = C[j] + Occ(j, pos[q]) + inc with the
 * reference's three-base-code behaviour when exact==0, or the exact count for all 15 codes
 * (== C[j] + O(j,pos) + inc, bwt.c:348-372) when exact!=0. out[q][0] is 0. pos may be (uint64_t)-1. */
int bwb_hip_rank16(bwb_hip_ctx *ctx, const uint64_t *pos, size_t n, int inc, int exact, uint64_t *out);

/* The children of n SA intervals [iL[q], iU[q]] as the alignment kernels compute them (wave_children, bwb_lane.h): child j = 1..15 is
 * [C[j] + Occ(j, iL - 1) + 1, C[j] + Occ(j, iU)], out_L[q][j - 1] / out_U[q][j - 1]; out_mask[q] has bit j set when child j is not empty (L <= U).
 * flags[q] bit 0 = need: the lane asks for its children (clear: an idle lane of a busy wave - mask 0, L and U 0); bit 1 = alpha: Occ as O_alphabet
 * sees it (bwt.c:374-438: the codes 5, 9, 11, 13 of a regular position are C[j] - [first character of the block == j]), exact otherwise.
 * iL <= length (iL - 1 is a position, -1 for iL == 0), iU < length: the root interval is (0, length - 1).
 * LANE ORDER: pair q runs as lane q % 64 of wave q / 64 - a wave gathers the buckets of its 64 pairs together, so the caller decides which pairs
 * share a bucket, how many need a second one (more than 24 take further gather rounds) and which lanes are idle; the last wave is padded with
 * idle lanes.  For parity tests, like calc_d and rank16.  (Added without a version change: no structure or existing entry point changed.) */
int bwb_hip_children(bwb_hip_ctx *ctx, const uint64_t *iL, const uint64_t *iU, const uint8_t *flags, size_t n,
                     uint64_t *out_L, uint64_t *out_U, uint32_t *out_mask);

/* Rank micro-benchmark: `n` pseudo-random Occ16 queries (seeded), repeated `iters` times with
 * everything resident; returns kernel milliseconds per iteration and a checksum of the results. */
int bwb_hip_rank_bench(bwb_hip_ctx *ctx, size_t n, int iters, uint64_t seed, double *ms_per_iter, uint64_t *checksum);
/* The same queries with the layout the alignment kernels use: one query per lane, every lane gathers its own 128-byte
 * bucket and ranks all 15 codes (the octet version above splits one bucket over 8 lanes). Same checksum. */
int bwb_hip_rank_bench_lane(bwb_hip_ctx *ctx, size_t n, int iters, uint64_t seed, double *ms_per_iter, uint64_t *checksum);

/* SA[i] for n suffix-array rows via the invPsi walk (bwt.c:311-329); needs the sampled SA
 * (bwt.c:80) uploaded with bwb_hip_set_sa. Used by aln2sam (align.c:760-812). */
int bwb_hip_set_sa(bwb_hip_ctx *ctx, const uint64_t *SA, uint64_t num_sa);
int bwb_hip_locate(bwb_hip_ctx *ctx, const uint64_t *rows, size_t n, uint64_t *out_pos);
/* the last bwb_hip_locate call on the context: rows looked up, invPsi steps taken (each one rank-block visit: a 128-byte bucket) and the
 * kernel's HIP-event time - what `bwbble aln2sam` and bench.py report (any pointer may be NULL) */
int bwb_hip_locate_stats(bwb_hip_ctx *ctx, uint64_t *rows, uint64_t *steps, double *kernel_ms);

/* What eval_aln + mapq (align.c:738-812) make of one read's hits - everything print_aln2sam needs except the names - computed on the GPU
 * where the hits lie (kernel k_place), so that a caller who wants SAM text copies 48 bytes per read instead of every hit.  An unmapped read
 * (no hits) is all zero.  (Added without a version change, like ctx_create_async: no structure or existing entry point changed.) */
#define BWB_PLACE_MAPPED 1     /* flags bit 0: the read has a hit */
#define BWB_PLACE_REVERSE 2    /* flags bit 1: aln_strand == 1, printed as SAM flag 16 */
typedef struct {
	uint64_t pos;            /* read_t.aln_pos: 0-based position in the indexed text (align.c:790-795) */
	int32_t top1, top2;      /* summed interval widths of the hits with the first hit's score or less / of the others (align.c:771-779): each
	                            64-bit width is added into an int there, so the sums wrap modulo 2^32 and may be zero or negative on a mapped read.
	                            With top2 < 0 and top1 == 1 or < 0 the reference's MAPQ is undefined (log() of a negative number, NaN
	                            converted to int, align.c:744); this library then reads its table at 0 */
	uint16_t score;          /* of the first hit, like everything below */
	uint8_t mapq;
	uint8_t flags;
	uint8_t num_mm, num_gapo, num_gape, reserved;
	uint16_t aln_length;
	uint16_t ref_len;        /* aln_length minus the path's insertions (get_aln_length, align.c:748-757) */
	uint32_t reserved2;
	uint16_t gap_run[BWB_MAX_GAP_RUNS]; /* the first hit's gap runs (encoded like bwb_aln.gap_run) on the path AS aln2sam SEES IT: reversed, the way the
	                            .aln loader rebuilds it (align.c:466-476) - the CIGAR; ascending by start, unused runs (0xFFFF) last */
} bwb_place;

/* slot_wait + k_place over the slot + D2H of n_reads records in read order into pinned memory of the slot, valid until the slot is uploaded
 * again.  max_mm is mapq's (aln2sam's -n, default 6 - not align's).  Needs the sampled SA (bwb_hip_set_sa; BWB_E_STATE without).  Independent
 * of slot_result: either, both, in any order.  The kernel runs on the context's result stream, not behind the slices queued on the kernel
 * stream.  batch_place is the one-batch form (slot 0 after batch_run), place_stats reports the last place call. */
int bwb_hip_slot_place(bwb_hip_ctx *ctx, int slot, int max_mm, const bwb_place **out, uint32_t *n_reads);
int bwb_hip_batch_place(bwb_hip_ctx *ctx, int max_mm, const bwb_place **out, uint32_t *n_reads);
int bwb_hip_place_stats(bwb_hip_ctx *ctx, uint64_t *reads, uint64_t *steps, double *kernel_ms);
/* The same kernel on a hit list of the caller's instead of a slot's hit log: read r owns alns[aln_off[r] .. aln_off[r + 1]) in discovery
 * order (a bwb_aln is exactly one record of the log; only alns[aln_off[0] .. aln_off[n_reads]) is read); n_reads records go to out, place_stats reports the call.  Needs set_sa; touches no slot.
 * BWB_E_ARG when aln_off does not ascend; BWB_E_STATE when a first hit's L is not a row of the index (nothing of that read is looked up).
 * For parity tests, like calc_d and rank16.  (Added without a version change: no structure or existing entry point changed.) */
int bwb_hip_place_hits(bwb_hip_ctx *ctx, const bwb_aln *alns, const uint64_t *aln_off, uint32_t n_reads, int max_mm, bwb_place *out);

/* A read's OTHER placements (`bwbble map -X N`: the X0 / X1 / XA tags).  A read's placements are the rows L .. U of its first hit, then of its
 * second, and so on in discovery order; placement 0 is the one bwb_place describes.  T = their number (64-bit, saturating; a hit with U < L
 * saturates it).  With 2 <= T <= max_alt + 1 the read owns the T - 1 items alts[alt_off[r] .. alt_off[r + 1]), placements 1 .. T - 1 in that
 * order; otherwise none (BWA's rule: too many placements, no list).  Every item is evaluated like the primary (align.c:786-801) from its own
 * hit and row.  Computed on the GPU per ITEM, not per read: kernels k_alt_count, an exclusive scan, k_place_alt - the buffers hold the items
 * there are, never n_reads * max_alt.  (Added without a version change: no structure or existing entry point changed.) */
typedef struct {            /* 32 bytes */
	uint64_t pos;           /* as bwb_place.pos */
	uint8_t flags;          /* BWB_PLACE_MAPPED | BWB_PLACE_REVERSE */
	uint8_t hit;            /* index of the hit in the read's list */
	uint8_t num_mm, num_gapo, num_gape, reserved;
	uint16_t aln_length;
	uint16_t gap_run[BWB_MAX_GAP_RUNS]; /* as bwb_place.gap_run */
} bwb_alt;
/* slot_place, then the items of the slot's reads: places as slot_place gives them, alt_off[n_reads + 1] and the items in pinned memory of the
 * slot, valid until the slot is uploaded again.  max_alt outside 1..255: BWB_E_ARG; no sampled SA: BWB_E_STATE; an item whose row is not a
 * row of the index: BWB_E_STATE (nothing is looked up for it).  The context stays usable after each.  batch_place_alt is the one-batch form,
 * place_alt_stats reports the last place_alt call: items, invPsi steps, kernel milliseconds (count + scan + k_place_alt). */
int bwb_hip_slot_place_alt(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off,
                           const bwb_alt **alts, uint32_t *n_reads);
int bwb_hip_batch_place_alt(bwb_hip_ctx *ctx, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off,
                            const bwb_alt **alts, uint32_t *n_reads);
int bwb_hip_place_alt_stats(bwb_hip_ctx *ctx, uint64_t *items, uint64_t *steps, double *kernel_ms);
/* The same on a hit list of the caller's (see place_hits): n_reads records go to out; alt_off and alts point into memory of the context, valid
 * until the next place_hits_alt call on it.  For parity tests. */
int bwb_hip_place_hits_alt(bwb_hip_ctx *ctx, const bwb_aln *alns, const uint64_t *aln_off, uint32_t n_reads, int max_mm, int max_alt,
                           bwb_place *out, const uint64_t **alt_off, const bwb_alt **alts);

/* Bubble hits in reference coordinates (`bwbble map -B`: the tags bC:Z: / bP:Z: that the reference's sam_pad appends, mg-ref/sam_pad.cpp:47-94).
 * A multi-genome holds one `>bubbleN chr pos` record per indel; bubble.data (mg-ref/comb.cpp:245-253) says where its two flanks lie on the
 * chromosome.  Kernel k_locus resolves every read of a slot next to k_place: the .ann record that contains the read's text position (a binary
 * search of a uniform number of steps over the records' first positions), the position SAM prints, and on a bubble record with B = B_minus_A
 * and the printed position as `locus`, in 64-bit signed arithmetic:
 *     1 <= locus <= B                                         -> the point A + locus - 1
 *     B + alt_len + 1 <= locus <= B + alt_len + D_minus_C + 1 -> the point locus + C - (B + alt_len + 1)
 *     anything else                                           -> the range A + B .. A + B + ref_len - 1 (its upper end one below its lower end
 *                                                                when ref_len == 0)
 * (Added without a version change: no structure or existing entry point changed.) */
typedef struct { int64_t A, B_minus_A, C, D_minus_C; int32_t ref_len, alt_len; } bwb_bubble;
#define BWB_LOCUS_POINT 1
#define BWB_LOCUS_RANGE 2
typedef struct {                 /* 32 bytes, two 16-byte words */
	int32_t seqid;               /* .ann record that contains bwb_place.pos; -1: none / unmapped */
	int32_t pos1;                /* what SAM POS prints: (int)(pos - start + 1); 0 unmapped */
	int32_t bubble;              /* index into the bubble table; -1: not a bubble record */
	uint8_t kind, reserved[3];   /* 0 none, BWB_LOCUS_POINT, BWB_LOCUS_RANGE */
	int64_t ref_lo, ref_hi;      /* bP: lo == hi for a point */
} bwb_locus;
/* Uploads the tables once per context: record i of the .ann file spans the text positions start[i] .. end[i] and is bubble bubble_of[i] (-1: not a
 * bubble record).  BWB_E_ARG when the records are not ascending and disjoint (start[i] <= end[i] < start[i + 1]), when there is none, or when a
 * bubble_of lies outside -1 .. n_bub - 1; n_bub == 0 with every bubble_of -1 is allowed.  A second call replaces the tables. */
int bwb_hip_set_loci(bwb_hip_ctx *ctx, const uint64_t *start, const uint64_t *end, const int32_t *bubble_of, uint32_t n_seq,
                     const bwb_bubble *bubbles, uint32_t n_bub);
/* slot_place (or its cached records), then k_locus over the slot's device-resident placement records on the result stream and D2H of n_reads
 * locus records in read order into pinned memory of the slot, valid until the slot is uploaded again.  The same records whether it is called
 * before or after slot_place / slot_place_alt / slot_result.  BWB_E_STATE without set_loci, without set_sa, or on a slot that has not been
 * submitted; the context stays usable after each.  batch_locus is the one-batch form (slot 0 after batch_run). */
int bwb_hip_slot_locus(bwb_hip_ctx *ctx, int slot, int max_mm, const bwb_place **places, const bwb_locus **loci, uint32_t *n_reads);
int bwb_hip_batch_locus(bwb_hip_ctx *ctx, int max_mm, const bwb_place **places, const bwb_locus **loci, uint32_t *n_reads);
/* The same kernel on n placement records of the caller's (like place_hits): n locus records go to out.  Needs set_loci; touches no slot.
 * For parity tests. */
int bwb_hip_locus_places(bwb_hip_ctx *ctx, const bwb_place *places, uint32_t n, bwb_locus *out);
/* the last locus call on the context: reads resolved and the kernel's HIP-event time (any pointer may be NULL) */
int bwb_hip_locus_stats(bwb_hip_ctx *ctx, uint64_t *reads, double *kernel_ms);

/* A read's placements counted by LOCUS (`bwbble map -X N -B table -J`).  A read beside an indel site lies twice in a multi-genome's text - in
 * the chromosome and in a flank of the `>bubbleN` record that copies it - and eval_aln counts two placements (MAPQ 0).  A PLACEMENT is the
 * primary (bwb_place) or one of the read's items (bwb_alt).  Its locus is (c, s, lo, hi): s the BWB_PLACE_REVERSE bit; on a non-bubble
 * record i, c = i and lo = hi = the position SAM prints (bwb_locus.pos1, widened to 64 bits); on a record of bubble b, c = chrom_of[b] and
 * lo .. hi = ref_lo .. ref_hi of bwb_locus; an unmapped placement or one in no record has no locus.  With hi' = max(hi, lo) - the empty range of
 * a pure insertion counts as its left edge - an item is JOINED to the primary when both have a locus, c and s are equal, and
 * lo_item <= hi'_primary && lo_primary <= hi'_item (signed 64-bit).  Items are compared with the primary only.  An item is SUBOPTIMAL when
 * its hit's score is greater than the first hit's (the comparison of eval_aln, align.c:771-779).  Per read:
 *     joined = the number of joined items
 *     top1   = bwb_place.top1 - (joined items that are not suboptimal),  top2 = bwb_place.top2 - (joined suboptimal items)  (32-bit, wrapping)
 *     mapq   = the reference's formula (align.c:738-746) on these counts
 * A read without items keeps top1, top2 and mapq of its bwb_place verbatim; an unmapped read is all zero.  Two kernels behind k_place_alt and
 * k_locus on the result stream: k_join_items (one lane per item: its locus, compared with the primary's; one class byte) and k_join_reads
 * (one lane per read: the sums of its class bytes, one 16-byte record).  (Added without a version change: no structure or existing entry
 * point changed.) */
typedef struct { int32_t top1, top2; uint8_t mapq, joined; uint16_t reserved; uint32_t reserved2; } bwb_join; /* 16 bytes */
/* After set_loci: the .ann record of the chromosome every bubble lies on (what -J and -R both need).  BWB_E_STATE without set_loci; BWB_E_ARG when n_bub is not set_loci's,
 * or a value lies outside 0 .. n_seq - 1 or names a bubble record.  set_loci forgets it. */
int bwb_hip_set_bubble_chrom(bwb_hip_ctx *ctx, const int32_t *chrom_of, uint32_t n_bub);
/* slot_place_alt and slot_locus (or their cached records), then the two kernels over what they left in device memory, and D2H of n_reads join
 * records in read order into pinned memory of the slot, valid until the slot is uploaded again.  The same records whether it is called before
 * or after slot_place_alt / slot_locus / slot_result.  BWB_E_ARG for max_alt outside 1..255; BWB_E_STATE without set_sa, set_loci or
 * set_bubble_chrom, or on a slot that has not been submitted; the context stays usable after each.  batch_join is the one-batch form. */
int bwb_hip_slot_join(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off,
                      const bwb_alt **alts, const bwb_locus **loci, const bwb_join **joins, uint32_t *n_reads);
int bwb_hip_batch_join(bwb_hip_ctx *ctx, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off,
                       const bwb_alt **alts, const bwb_locus **loci, const bwb_join **joins, uint32_t *n_reads);
/* The same kernels (and k_locus) on records of the caller's: read r owns alts[alt_off[r] .. alt_off[r + 1]), at most 255 of them, alt_off[0] == 0;
 * alt_sub[q] != 0 says that item q is suboptimal.  n join records go to out.  Needs set_loci and set_bubble_chrom; touches no slot; locus_stats
 * then reports its k_locus launch.  BWB_E_ARG when alt_off does not fit that description.  For parity tests. */
int bwb_hip_join_records(bwb_hip_ctx *ctx, const bwb_place *places, uint32_t n, const uint64_t *alt_off, const bwb_alt *alts,
                         const uint8_t *alt_sub, int max_mm, bwb_join *out);
/* the last join call on the context that launched the kernels: items compared, items joined and the two kernels' HIP-event time (any pointer
 * may be NULL).  A slot_join that returns the slot's cached records launches nothing and leaves these figures as they were. */
int bwb_hip_join_stats(bwb_hip_ctx *ctx, uint64_t *items, uint64_t *joined, double *kernel_ms);

/* A placement on a bubble record in CHROMOSOME coordinates (`bwbble map -B table -R`): RNAME, POS and CIGAR rewritten, the alternate allele as
 * an insertion and the positions the record skips as a deletion.  Bubble b = (A, Bm = B_minus_A, C, Dm = D_minus_C, ref_len, alt_len) has a
 * record of reclen = Bm + alt_len + Dm + 1 characters whose 1-based coordinate x lies in one of three zones:
 *     L  1 .. Bm                          the chromosome's A + x - 1
 *     V  Bm + 1 .. Bm + alt_len           no chromosome position (the alternate allele)
 *     R  Bm + alt_len + 1 .. reclen       the chromosome's C + x - (Bm + alt_len + 1)
 * gap = C - A - Bm is the number of chromosome positions between the flanks.  It is NOT ref_len: comb gives an allele written `.` a length of 1
 * in C and of 0 in ref_len, and the flanks' coordinates are what place the M bases.
 * A placement with printed position pos1 (bwb_locus.pos1) and the CIGAR SAM prints (the M / I / D ops of its gap runs in text order, on either
 * strand) is LIFTABLE when pos1 >= 1 and pos1 + (the M and D lengths) - 1 <= reclen and an M remains below.  The ops are walked with x running
 * from pos1:  I stays I;  M on an x in L or R stays M, on an x in V it becomes I;  D on an x in L or R stays D, on an x in V it disappears;  when
 * the walk consumes x = Bm + alt_len + 1 after a smaller x and gap > 0, D x gap comes first (so: the allele's I, then the D);  before the first
 * and behind the last M, I becomes S (a soft clip) and D is dropped;  POS is the chromosome position of the first M;  neighbouring ops of one
 * kind are merged (while the sum stays below 2^28).  At most BWB_LIFT_MAX_OPS ops remain: 17 runs and the three the allele adds.
 * The index space is the PLACEMENTS of n_reads reads: q < n_reads is read q's primary (bwb_place), n_reads + j is item j (bwb_alt).  Per
 * placement one kind byte - BWB_LIFT_NONE: not on a bubble record, or unmapped; BWB_LIFT_LIFTED; BWB_LIFT_UNLIFTABLE: on a bubble record, printed
 * as it is - and for a lifted one a record of 16-byte words at recs + lift_off[q]: the header below, then n_ops ops as uint32 = len << 4 | op,
 * padded with zeros to a multiple of four.  lift_off has one entry per placement and one more; the buffers hold the records there are.
 * Kernels k_lift_count (one lane per placement: the kind byte and the record's size), the exclusive scan of k_place_alt, and k_lift, behind
 * k_place_alt / k_locus on the result stream.  (Added without a version change: no structure or existing entry point changed.) */
#define BWB_LIFT_M 0
#define BWB_LIFT_I 1
#define BWB_LIFT_D 2
#define BWB_LIFT_S 4
#define BWB_LIFT_MAX_OPS 20
#define BWB_LIFT_NONE 0
#define BWB_LIFT_LIFTED 1
#define BWB_LIFT_UNLIFTABLE 2
typedef struct { int64_t pos; int32_t seqid; uint8_t n_ops, reserved[3]; } bwb_lift; /* 16 bytes: POS, the chromosome's .ann record, the ops that follow */
/* slot_locus and, with max_alt 1..255, slot_place_alt (or their cached records; max_alt 0: the primaries alone), then the kernels over what they
 * left in device memory, and D2H into pinned memory of the slot, valid until the next slot_lift on that slot or its next upload.  *n_placements = n_reads + the items.
 * The same records whether it is called before or after slot_place_alt / slot_locus / slot_join / slot_result.  BWB_E_ARG for max_alt outside
 * 0..255 and for a bubble table the rule refuses - gap < 0, gap >= 2^28, alt_len < 0, Bm < 0 or Dm < -1; the message names the bubble -;
 * BWB_E_STATE without set_sa, set_loci or set_bubble_chrom, or on a slot that has not been submitted; the context stays usable after each.
 * batch_lift is the one-batch form. */
int bwb_hip_slot_lift(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, const uint8_t **kinds, const uint64_t **lift_off, const bwb_lift **recs,
                      uint64_t *n_placements);
int bwb_hip_batch_lift(bwb_hip_ctx *ctx, int max_mm, int max_alt, const uint8_t **kinds, const uint64_t **lift_off, const bwb_lift **recs,
                       uint64_t *n_placements);
/* The same kernels (and k_locus for the primaries) on records of the caller's: read r owns alts[alt_off[r] .. alt_off[r + 1]), alt_off[0] == 0.
 * kinds, lift_off and recs point into memory of the context, valid until the next lift_records call on it.  Needs set_loci and set_bubble_chrom;
 * touches no slot.  BWB_E_ARG when alt_off does not ascend or n + the items exceed 2^31 - 1.  For parity tests. */
int bwb_hip_lift_records(bwb_hip_ctx *ctx, const bwb_place *places, uint32_t n, const uint64_t *alt_off, const bwb_alt *alts,
                         const uint8_t **kinds, const uint64_t **lift_off, const bwb_lift **recs);
/* the last lift call on the context that launched the kernels: placements lifted, placements on a bubble record that are not liftable, and the
 * kernels' HIP-event time (any pointer may be NULL) */
int bwb_hip_lift_stats(bwb_hip_ctx *ctx, uint64_t *lifted, uint64_t *unliftable, double *kernel_ms);

/* NM:i and MD:Z of a read's line (`bwbble map -D`), computed against the TEXT the index was built from - which holds IUPAC codes, so that no
 * stock tool can add the two tags afterwards.  The text is <seq_fasta>.ref as `bwbble index` / `fasta2ref` write it: one code per byte
 * (0 `$`, 1 T, 2 K, 3 G, 4 S, 5 B, 6 Y, 7 C, 8 M, 9 H, 10 N, 11 V, 12 R, 13 D, 14 W, 15 A), the forward text of n_fwd characters - the first
 * number of the .ann file - and then its reverse complement; only the forward half is used.
 * The rule, for one read:
 *   SEQ     the read as SAM prints it: reversed and complemented when BWB_PLACE_REVERSE.
 *   ops     the placement's printed CIGAR (the M / I / D ops of its gap runs in text order), from text position bwb_place.pos; or, for a primary
 *           whose lift kind is BWB_LIFT_LIFTED, the ops of its lift record (M / I / D / S), from text position start[rec.seqid] + rec.pos - 1.
 *   kind    BWB_MD_NONE for an unmapped read;  else BWB_MD_TOO_LONG when span = the M and D lengths exceeds BWB_MD_MAX_SPAN (only a lifted
 *           record with a long gap gets there: the rule of bwb_lift admits a D of 2^28 - 1);  else BWB_MD_NONE when the span leaves
 *           [0, n_fwd), when the M, I and S lengths are not the read's length, or when a lift record names no record of the table;  else
 *           BWB_MD_OK.  Only BWB_MD_OK has nm and md_len; the line of any other kind is printed as without -D.
 *   walk    with a match run `run` = 0:
 *           M  per base: a match when the read base is A / G / C / T and the text's code is one of the codes that base is a member of (the
 *              search's own rule; the codes 0 `$` and 10 `N` match nothing, and a read N matches nothing): run + 1.  Otherwise `run` in
 *              decimal and the text's letter - "NTKGSBYCMHNVRDWA"[code] - are written, run = 0, mm + 1.
 *           D  `run` in decimal, `^` and the text's letters over the deletion; run = 0.  (A D directly behind a D continues its letters.)
 *           I  consumes read bases only.     S  consumes read bases only and counts for nothing.
 *           at the end: `run` in decimal.
 *   NM      mm + the I lengths + the D lengths.
 * This is the SAM specification's MD, so `10^AC0T5` and a leading `0` fall out by themselves.  MD and NM for XA items are not computed.
 * Per read one bwb_md record, and for kind BWB_MD_OK the md_len ASCII bytes md_text[md_off[r] .. md_off[r + 1]) (no terminator); md_off has one
 * entry per read and one more; the buffers hold the bytes there are.  Kernels k_md_count (one lane per read, grid-strided: kind, NM and the
 * exact length), the exclusive scan of k_place_alt, and k_md (writes the bytes), behind k_place / k_lift on the result stream; they fetch the text,
 * packed to 4 bits per character by k_text_pack, in aligned 16-byte words of 32 characters.  (Added without a version change: no structure or
 * existing entry point changed.) */
#define BWB_MD_NONE 0
#define BWB_MD_OK 1
#define BWB_MD_TOO_LONG 2
#define BWB_MD_MAX_SPAN 4096
typedef struct { uint32_t nm; uint16_t md_len; uint8_t kind, reserved; } bwb_md; /* 8 bytes */
/* Uploads the forward text (codes[0 .. n_fwd), one code per byte) and packs it on the device, staged in chunks: n_fwd / 2 bytes stay resident.
 * Call it before the first slot_upload sizes the context's pool.  BWB_E_ARG for a code above 15 (no text is set then) or n_fwd == 0.  A second
 * call replaces the text. */
int bwb_hip_set_text(bwb_hip_ctx *ctx, const uint8_t *codes, uint64_t n_fwd);
/* slot_place (or its cached records) and, with lifted != 0, slot_lift (max_alt as given to it, so that cached records are used), then the kernels
 * over the slot's reads - still resident from its upload - and D2H into pinned memory of the slot, valid until the next slot_md on that slot or
 * its next upload.  BWB_E_STATE without set_text, without set_sa, on a slot that has not been submitted, or with lifted != 0 without set_loci /
 * set_bubble_chrom; the context stays usable after each.  batch_md is the one-batch form (slot 0 after batch_run). */
int bwb_hip_slot_md(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, int lifted, const bwb_md **recs, const uint64_t **md_off,
                    const char **md_text, uint32_t *n_reads);
int bwb_hip_batch_md(bwb_hip_ctx *ctx, int max_mm, int max_alt, int lifted, const bwb_md **recs, const uint64_t **md_off, const char **md_text,
                     uint32_t *n_reads);
/* The same kernels on records of the caller's: read r is reads_fwd[r * stride .. + lens[r]) (read->seq codes, lens[r] <= stride, at most 255)
 * with the placement places[r].  kinds / lift_off / lift_recs (all three or none): read r's lift kind, and the 16-byte words of its record at
 * lift_recs + lift_off[r] as slot_lift lays them out; lift_off has n + 1 ascending entries.  recs, md_off and md_text point into memory of the
 * context, valid until the next md_records call on it.  Needs set_text, and set_loci with the lift arguments (BWB_E_STATE); touches no slot.
 * For parity tests. */
int bwb_hip_md_records(bwb_hip_ctx *ctx, const uint8_t *reads_fwd, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n,
                       const uint8_t *kinds, const uint64_t *lift_off, const bwb_lift *lift_recs, const bwb_md **recs, const uint64_t **md_off,
                       const char **md_text);
/* the last md call on the context that launched the kernels: reads of kind BWB_MD_OK, the MD bytes written, and the kernels' HIP-event time
 * (any pointer may be NULL) */
int bwb_hip_md_stats(bwb_hip_ctx *ctx, uint64_t *reads, uint64_t *md_bytes, double *kernel_ms);

/* Allele counts at the text's IUPAC sites (`bwbble map -A`): which allele of each known variant the reads carry, summed on the device over
 * every read of a run - the first stage that is a reduction ACROSS reads.  No pileup tool can make the table afterwards: it has neither the
 * text nor the member rule, and without -R the reads on bubble records lie in coordinates nothing else understands.
 * The rule:
 *   sites   a SITE is a position i in [0, n_fwd) of the forward text (bwb_hip_set_text) whose code has two or three members: 2 K, 4 S, 5 B, 6 Y,
 *           8 M, 9 H, 11 V, 12 R, 13 D, 14 W.  `$`, N and the four plain bases are no sites.  Sites are numbered in text order: site(i) = the
 *           number of sites below i.  n_sites is 64-bit here; a text with more than 2^32 - 1 sites is refused (BWB_E_ARG).
 *   reads   read r counts when its bwb_md kind under the same `lifted` argument would be BWB_MD_OK - mapped, the span within [0, n_fwd) and at
 *           most BWB_MD_MAX_SPAN, the ops consuming exactly the read - and its MAPQ is at least min_mapq: bwb_join.mapq when the call is
 *           `joined`, else bwb_place.mapq.  Primaries only.
 *   counts  the ops are those bwb_md walks, from the same start: the printed CIGAR from bwb_place.pos, or for a primary whose lift kind is
 *           BWB_LIFT_LIFTED the ops of its lift record from start[rec.seqid] + rec.pos - 1.  For every M base whose text position is a site and
 *           whose read base (SEQ as SAM prints it) is A, C, G or T: counts[site][column] += 1, the columns A, C, G, T by the printed letter.  A
 *           base that is no member of the code counts under its own letter (a novel allele or an error: the table is there to show it).  A read
 *           N, and the ops I, S and D, count nothing.  The counters are uint32 and wrap modulo 2^32.
 *   where   with `lifted` a read on a bubble record is walked on the chromosome: its flank bases land on the chromosome's sites, the allele's
 *           bases (I) nowhere.  Without it the read counts on the bubble record's own positions.
 * The adds are integer and commute: the table does not depend on chunking, slot order, parked reads or the number of contexts whose tables are
 * summed.  Kernels: k_site_count (one lane per 16-byte word of the packed text: the word's site mask and popcount, scanned into one uint32 per
 * word, n_fwd / 8 bytes resident), k_pile (one lane per read behind k_place / k_lift / the join kernels on the result stream; relaxed
 * agent-scope atomic adds), k_site_of (test entry).  (Added without a version change: no structure or existing entry point changed.) */
/* After set_text and before the first slot_upload sizes the pool: builds the site index, allocates and zeroes n_sites x 4 counters.  BWB_E_STATE
 * without a text.  *n_sites may be 0: the pile calls then count nothing.  A later set_text forgets the index and the counters. */
int bwb_hip_pile_begin(bwb_hip_ctx *ctx, uint64_t *n_sites);
/* slot_place, then slot_lift with lifted != 0 and slot_join with joined != 0 (their cached records where they exist), then k_pile over the
 * slot's n_reads resident reads (a carried read has no record).  Nothing per read comes back; *reads_counted (may be NULL) = the reads this
 * call counted.  A SUBMISSION IS PILED ONCE: a second slot_pile on the same submission returns BWB_OK, launches nothing and reports 0; the flag
 * clears at the slot's next upload.  BWB_E_ARG for min_mapq or max_alt outside 0..255.  BWB_E_STATE without pile_begin, without set_sa, on a
 * slot that has not been submitted, with lifted != 0 without set_loci / set_bubble_chrom, and with joined != 0 without them or with
 * max_alt == 0; the context stays usable after each.  batch_pile is the one-batch form (slot 0 after batch_run). */
int bwb_hip_slot_pile(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, int lifted, int joined, int min_mapq, uint64_t *reads_counted);
int bwb_hip_batch_pile(bwb_hip_ctx *ctx, int max_mm, int max_alt, int lifted, int joined, int min_mapq, uint64_t *reads_counted);
/* The same kernel on records of the caller's, laid out as for md_records; mapq: NULL, or one value per read that stands in for the joined MAPQ.
 * Accumulates into the context's counters; touches no slot.  Needs pile_begin, and set_loci with the lift arguments (BWB_E_STATE). */
int bwb_hip_pile_records(bwb_hip_ctx *ctx, const uint8_t *reads_fwd, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n,
                         const uint8_t *kinds, const uint64_t *lift_off, const bwb_lift *lift_recs, const uint8_t *mapq, int min_mapq);
/* Synchronises the result stream and copies the 4 n counters of the sites first .. first + n - 1 to out (A, C, G, T per site).  BWB_E_ARG when
 * the range leaves n_sites; BWB_E_STATE without pile_begin. */
int bwb_hip_pile_counts(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, uint32_t *out);
/* zeroes the counters */
int bwb_hip_pile_reset(bwb_hip_ctx *ctx);
/* the site number of each text position pos[q] < n_fwd (BWB_E_ARG beyond), or -1 where it is no site: for parity tests, like rank16 */
int bwb_hip_pile_site_of(bwb_hip_ctx *ctx, const uint64_t *pos, size_t n, int64_t *site);
/* the last pile call on the context that launched the kernel: reads counted, adds made, and the kernel's HIP-event time (any pointer may be
 * NULL) */
int bwb_hip_pile_stats(bwb_hip_ctx *ctx, uint64_t *reads, uint64_t *adds, double *kernel_ms);

/* Ref / alt read support per indel bubble (`bwbble map -B table -I <indels.tsv>`): how many reads carry a bubble's alternate allele and how
 * many the chromosome's own, summed on the device over every read of a run - the second reduction across reads, beside the pile family.  No
 * stock tool can make the table afterwards: an alt-supporting read lies on a bubble record, a ref-supporting read at a site only bubble.data
 * names, and the MAPQ that decides is -J's.
 * The rule.  Bubble b = (A, Bm, C, Dm, ref_len, alt_len) with gap = C - A - Bm, c = chrom_of[b] and the zones L / V / R of bwb_lift; w is the
 * ANCHOR, 1..255: the flank bases a read must cover with M on either side.
 *   eligible  b is eligible when the rule of bwb_lift does not refuse it (Bm >= 0, Dm >= -1, alt_len >= 0, 0 <= gap < 2^28) and Bm >= w,
 *             Dm + 1 >= w and A + Bm - w >= 1.  An ineligible bubble is never counted, for either allele.  A table with refused bubbles does
 *             not stop anything: they are skipped.
 *   windows   in the 1-based coordinates of the record the read lies on (bwb_locus.pos1):
 *             on b's own record       [lo, hi] = [Bm - w + 1, Bm + alt_len + w]
 *             on the chromosome's c   [lo, hi] = [A + Bm - w, C + w - 1]
 *   reads     a read counts when it is mapped and its locus has seqid >= 0, its printed ops consume exactly the read's length (M and I; the
 *             records form has no reads and does not ask), and its MAPQ is at least min_mapq: bwb_join.mapq when the call is `joined`, else
 *             bwb_place.mapq.  Primaries only.  The ops are always the placement's PRINTED CIGAR - lift_op_at over gap_run, walked with x from
 *             pos1; M and D consume x, I does not -, never the lift record: the table is the same with and without -R.
 *   classes   of a read against a window: COVERING - lo and hi are each consumed by an M; CLEAN - covering, every x in [lo, hi] is consumed by
 *             an M, and no I lies between the M at lo and the M at hi; GAPPED - covering, not clean.  A read that is not covering adds nothing.
 *   counters  four uint32 per bubble, in the order ref, alt, ref_gapped, alt_gapped; they wrap modulo 2^32.  A read whose locus lies on b's
 *             record is classed against b's own window only: alt += 1 when clean, alt_gapped += 1 when gapped.  A read on a non-bubble record
 *             c is classed against the window of EVERY eligible bubble with chrom_of == c: ref += 1 or ref_gapped += 1.  Mismatches under M
 *             do not matter.
 * Not here: other bubbles' sites inside a bubble record's flanks, XA items, base qualities (the rule looks at ops, not at bases: -b and -Y below do not change it), genotypes, left-alignment (a read that fits both
 * alleles equally well counts for whichever placement is its primary).
 * The adds are integer and commute: the table does not depend on chunking, slot order, parked reads or the number of contexts whose tables are
 * summed.  Kernel k_indel: one lane per read behind k_place / k_locus / the join kernels on the result stream; a read on a chromosome bisects
 * a table of the eligible bubbles sorted by (chrom_of, A + Bm - w, bubble number) - 16 bytes per bubble, built on the host by indel_begin - and
 * walks the candidates whose lo lies within its first and last M; relaxed agent-scope atomic adds.  (Added without a version change: no
 * structure or existing entry point changed.) */
/* After set_loci and set_bubble_chrom and before the first slot_upload sizes the pool: builds and uploads the sorted table of the bubbles
 * eligible at this anchor, allocates and zeroes n_bub x 4 counters.  *n_eligible may be 0.  BWB_E_STATE without set_loci or set_bubble_chrom;
 * BWB_E_ARG for an anchor outside 1..255.  A later set_loci or set_bubble_chrom forgets the table and the counters. */
int bwb_hip_indel_begin(bwb_hip_ctx *ctx, int anchor, uint64_t *n_eligible);
/* slot_locus, and slot_join with joined != 0 (their cached records where they exist), then k_indel over the slot's n_reads resident reads.
 * Nothing per read comes back; *reads_counted (may be NULL) = the reads this call counted.  A SUBMISSION IS COUNTED ONCE: a second slot_indel
 * on the same submission returns BWB_OK, launches nothing and reports 0; the flag clears at the slot's next upload.  BWB_E_ARG for min_mapq or
 * max_alt outside 0..255.  BWB_E_STATE without indel_begin, without set_sa, on a slot that has not been submitted, and with joined != 0 and
 * max_alt == 0; the context stays usable after each.  batch_indel is the one-batch form (slot 0 after batch_run). */
int bwb_hip_slot_indel(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, int joined, int min_mapq, uint64_t *reads_counted);
int bwb_hip_batch_indel(bwb_hip_ctx *ctx, int max_mm, int max_alt, int joined, int min_mapq, uint64_t *reads_counted);
/* The same kernel on n placement records of the caller's (k_locus runs on them first, as in lift_records); mapq: NULL, or one value per read
 * that stands in for the joined MAPQ.  Accumulates into the context's counters; touches no slot.  Needs indel_begin (BWB_E_STATE). */
int bwb_hip_indel_records(bwb_hip_ctx *ctx, const bwb_place *places, uint32_t n, const uint8_t *mapq, int min_mapq);
/* Synchronises the result stream and copies the 4 n counters of the bubbles first .. first + n - 1 to out (ref, alt, ref_gapped, alt_gapped
 * per bubble).  BWB_E_ARG when the range leaves the bubble table; BWB_E_STATE without indel_begin. */
int bwb_hip_indel_counts(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, uint32_t *out);
/* zeroes the counters */
int bwb_hip_indel_reset(bwb_hip_ctx *ctx);
/* the last indel call on the context that launched the kernel: reads counted, adds made, candidate windows examined (a chromosome read's
 * table entries with lo within its M span, a bubble read's own eligible window) and the kernel's HIP-event time (any pointer may be NULL) */
int bwb_hip_indel_stats(bwb_hip_ctx *ctx, uint64_t *reads, uint64_t *adds, uint64_t *candidates, double *kernel_ms);

/* Genotype calls at IUPAC sites and indel bubbles (`bwbble map -G <calls.tsv>`): the last link behind the pile and indel counters - a genotype,
 * a quality and phred-scaled likelihoods for every known SNP site and indel bubble the reads cover.  No stock tool can make the call afterwards:
 * the text holds IUPAC codes and no reference base, the alt-supporting reads of an indel lie on bubble records, and the MAPQ that decides is -J's.
 * The rule - stated here once; the kernels, host/geno.c and tests/geno_model.py implement it and agree bit for bit.  Integer arithmetic only.
 *   parameters  E, the error phred, 4..93 (-q, default 20); d, the minimum depth, 1..2^31 - 1 (-d, default 1); H = 3, the cost of a base under a
 *               heterozygous genotype that carries it (10 log10 2, rounded).
 *   site        one of the pile family's sites, in the same numbering.  Its alleles are the members of the text's code in the column order A, C,
 *               G, T: a0 < a1 (< a2), k = 2 or 3.  n_i = the pile counter of a_i's column; depth = the sum of all four columns, in 64 bits (the
 *               counters are uint32 and wrap, as they do); other = depth - sum n_i.  The site is CALLED when depth >= d.
 *   genotypes   in VCF order, j = (0,0), (0,1), (1,1), (0,2), (1,2), (2,2); a two-member code has the first three.
 *                 raw(x,x) = E (depth - n_x)          raw(x,y) = H (n_x + n_y) + E (depth - n_x - n_y)          in uint64
 *               GT = the first j with the smallest raw; GQ = min(99, the smallest raw over j != GT, minus raw_GT); PL_j = min(raw_j - raw_GT,
 *               2^32 - 1).  A site whose bases are all non-members is still called: a0/a0 with GQ 0 - the table shows it, as the pile shows such
 *               bases.
 *   bubble      only the bubbles ELIGIBLE at indel_begin's anchor.  The alleles are R (the chromosome's) and V (the record's): n_R = ref, n_V =
 *               alt, the clean counts; other = ref_gapped + alt_gapped, depth = n_R + n_V + other, both in 64 bits.  Called when depth >= d, by
 *               the same formulas over R/R, R/V, V/V.  Bubbles that share a site are called each on its own, biallelic, with the shared ref count,
 *               exactly as the indel family counts them.
 * Which reads count is entirely the pile and indel families' rule; nothing here walks a read.  Base qualities: bwb_hip_pileq_begin, below.  Not here: priors, multi-allelic
 * indel sites, XA items, left-alignment, and VCF itself - the text has no reference allele to put in REF.
 * Kernels: k_geno_count (one lane per site of a range: the inverse of the site index - the site's word by bisection over the one uint32 per word,
 * its character as the r-th set bit of the word's site mask - and the four counters in one 16-byte load), the scan of the alt family, k_geno_emit
 * (the call, and the called sites' records compacted in site order); k_geno_bubbles, count and emit pass, for a range of bubbles.  On the result
 * stream.  (Added without a version change: no structure or existing entry point changed.) */
typedef struct {
	uint64_t pos;           /* 0-based position in the forward text */
	uint64_t site;          /* the site's number */
	uint32_t n[4];          /* the counters: A, C, G, T */
	uint8_t code, n_geno;   /* the text's code there; 3 or 6 genotypes */
	uint8_t gt, gq;         /* GT as the index j in VCF order; GQ 0..99 */
	uint32_t reserved;      /* 0 */
	uint32_t pl[6];         /* PL per genotype, unused entries 0 */
} bwb_geno_site;            /* 64 bytes */
typedef struct {
	uint32_t bubble;        /* the bubble's number */
	uint32_t n[4];          /* the counters: ref, alt, ref_gapped, alt_gapped */
	uint8_t gt, gq;         /* 0 R/R, 1 R/V, 2 V/V; GQ 0..99 */
	uint16_t reserved;      /* 0 */
	uint32_t pl[3];
	uint32_t pad[3];        /* 0 */
} bwb_geno_bubble;          /* 48 bytes */
/* After pile_begin (BWB_E_STATE without) and, where bubbles are to be called, after indel_begin; before the first slot_upload sizes the pool:
 * allocates the scratch and the pinned output for `piece` sites (1..2^24, else BWB_E_ARG) and, when indel_begin has run, for min(piece, n_bub)
 * bubbles.  A later pile_begin, set_text or indel_begin forgets what was sized for the tables they replace. */
int bwb_hip_geno_begin(bwb_hip_ctx *ctx, uint32_t piece);
/* The mirrors of pile_counts / indel_counts, with their argument checks: overwrite the 4 n counters from `first` with the caller's.  `map` needs
 * them when several workers' counters must meet on one device, the tests to inject crafted counts. */
int bwb_hip_pile_put(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, const uint32_t *counts);
int bwb_hip_indel_put(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, const uint32_t *counts);
/* Calls the sites (the bubbles) first .. first + n - 1, n <= piece (for bubbles min(piece, n_bub)): *out = the *n_out called entries' records in
 * ascending order, in pinned memory of the context's that stays valid until the next call of the same function.  BWB_E_ARG for err outside 4..93,
 * min_depth outside 1..2^31 - 1, a range that leaves the table or exceeds the piece.  BWB_E_STATE without geno_begin, and for bubbles without
 * an indel_begin before it. */
int bwb_hip_geno_sites(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, int err, int64_t min_depth, const bwb_geno_site **out, uint64_t *n_out);
int bwb_hip_geno_bubbles(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, int err, int64_t min_depth, const bwb_geno_bubble **out, uint64_t *n_out);
/* the entries the last geno_sites and the last geno_bubbles call that launched have called, and the HIP-event time of the kernels of whichever
 * of the two launched last (any pointer may be NULL) */
int bwb_hip_geno_stats(bwb_hip_ctx *ctx, uint64_t *sites_called, uint64_t *bubbles_called, double *kernel_ms);

/* Base qualities in the allele counts and the genotype calls (`bwbble map -b <m>` and `-Y`): a minimum base quality for the pile family, and a
 * quality-weighted rule beside the geno family's.  Nobody can apply either afterwards, for the reasons the two families give.  The rule - stated
 * here once; the kernels, host/pile.c + host/geno.c and tests/pileq_model.py implement it and agree bit for bit.  Integer arithmetic only.
 *   quality     the quality of a read base is taken from the QUAL byte SAM prints under it: for the read base at index i of the read as uploaded
 *               (i = ri on the forward strand, len - 1 - ri on the reverse one - the index k_pile uses for the base) it is byte i of the FASTQ's
 *               quality line.  For a byte c, Q = 0 when c < 33, else min(c - 33, 93).  I and S ops consume quality bytes as they consume bases.
 *   -b m        m = min_baseq, 0..93.  Everything of the pile family's rule stands - which reads count, which ops are walked, from where, which
 *               column, -a, -J's MAPQ, -R's walk - with one more condition: an M base on a site adds to counts[site][column] only when Q >= m.
 *               The indel family is not affected: its rule looks at ops, not at bases.
 *   -Y          err_cap = E, the geno family's error phred, 4..93.  A second table beside the counters, qsum[site][A|C|G|T], uint32, wrapping
 *               modulo 2^32: every base that adds 1 to a counter (after -b) adds q = min(max(Q, 4), E) to qsum in the same column; q lies in
 *               4..E.  The floor of 4 is E's own lower bound: a base costs a homozygous genotype that lacks it no less than H = 3, its cost
 *               under a heterozygous one that carries it.
 *   calls       for a site with the alleles a0 < a1 (< a2): n_i and depth as in the geno family, s_i the qsum column of a_i, S the sum of all
 *               four qsum columns in 64 bits;
 *                 raw(x,x) = S - s_x          raw(x,y) = H (n_x + n_y) + (S - s_x - s_y)          in uint64
 *               and GT, GQ, PL and CALLED (depth >= d) from raw exactly as there.  When every counted base has Q >= E, s_x = E n_x and the
 *               calls are the geno family's, number for number.  Bubbles have no per-base evidence: they are called by the geno family's rule.
 * Not here: quality-aware indel support, base qualities capped by MAPQ, the qualities of XA items, priors, VCF.
 * Kernels: k_pile_q beside k_pile (the same lanes and walk; the quality byte is loaded only when a base falls on a site, as the read base is;
 * relaxed agent-scope atomic adds to counts and qsum) and k_geno_emit_q beside k_geno_emit (behind the same k_geno_count and scan; counters and
 * sums in one 16-byte load each).  (Added without a version change: no structure or existing entry point changed.) */
typedef struct {
	bwb_geno_site site;     /* as from bwb_hip_geno_sites, GT / GQ / PL by the weighted rule */
	uint32_t qs[4];         /* the quality sums: A, C, G, T */
} bwb_geno_site_q;          /* 80 bytes */
/* After pile_begin (BWB_E_STATE without) and before the first slot_upload sizes the pool: from now on every slot keeps n_reads x stride quality
 * bytes beside its reads, and - weighted != 0 - allocates and zeroes the n_sites x 4 quality sums.  A later pile_begin or set_text forgets it. */
int bwb_hip_pileq_begin(bwb_hip_ctx *ctx, int weighted);
/* The quality bytes of the slot's resident reads, laid out like slot_upload's reads_fwd (one byte per base in FASTQ order, `stride` bytes per read):
 * staged and copied on the copy stream; the caller's buffer is free on return.  After the slot's slot_upload and before its pile call; the slot's
 * next slot_upload forgets them.  BWB_E_STATE without pileq_begin or on a slot without an upload; BWB_E_ARG when stride is not the upload's. */
int bwb_hip_slot_quals(bwb_hip_ctx *ctx, int slot, const uint8_t *quals, uint32_t stride);
/* slot_pile's chain - slot_place, slot_lift, slot_join or their cached records - then k_pile_q.  err_cap == 0: unweighted (counts only); 4..93:
 * weighted with that E, which needs pileq_begin(weighted != 0).  A SUBMISSION IS PILED ONCE: slot_pile and slot_pile_q share the flag.  slot_pile's
 * errors, and BWB_E_ARG for min_baseq outside 0..93 or err_cap outside {0, 4..93}; BWB_E_STATE without pileq_begin, for err_cap != 0 without the
 * sums, and without the slot's qualities; the context stays usable after each.  batch_pile_q is the one-batch form (slot 0 after batch_run). */
int bwb_hip_slot_pile_q(bwb_hip_ctx *ctx, int slot, int max_mm, int max_alt, int lifted, int joined, int min_mapq, int min_baseq, int err_cap, uint64_t *reads_counted);
int bwb_hip_batch_pile_q(bwb_hip_ctx *ctx, int max_mm, int max_alt, int lifted, int joined, int min_mapq, int min_baseq, int err_cap, uint64_t *reads_counted);
/* pile_records with the reads' quality bytes (laid out like reads_fwd), min_baseq and err_cap: accumulates into the counters and the sums. */
int bwb_hip_pile_records_q(bwb_hip_ctx *ctx, const uint8_t *reads_fwd, const uint8_t *quals, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n,
                           const uint8_t *kinds, const uint64_t *lift_off, const bwb_lift *lift_recs, const uint8_t *mapq, int min_mapq, int min_baseq, int err_cap);
/* The mirrors of pile_counts and pile_put for the 4 n quality sums of the sites first .. first + n - 1, with their argument checks; BWB_E_STATE
 * without a weighted pileq_begin.  pile_reset zeroes the sums with the counters. */
int bwb_hip_pileq_sums(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, uint32_t *out);
int bwb_hip_pileq_put(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, const uint32_t *sums);
/* the last pile_q call on the context that launched the kernel: reads counted, adds made, bases dropped by min_baseq, and the kernel's HIP-event
 * time (any pointer may be NULL) */
int bwb_hip_pileq_stats(bwb_hip_ctx *ctx, uint64_t *reads, uint64_t *adds, uint64_t *dropped, double *kernel_ms);
/* geno_sites by the weighted rule, from the counters and the sums: geno_begin's piece - a geno_begin that comes after pileq_begin(weighted != 0)
 * sizes scratch and output for the 80-byte records -, the same pinned-output discipline (*out shares geno_sites' memory), geno_stats as there.
 * err is checked as there; the sums carry it from the pile's err_cap.  geno_sites' errors, and BWB_E_STATE without a weighted pileq_begin before
 * geno_begin. */
int bwb_hip_geno_sites_q(bwb_hip_ctx *ctx, uint64_t first, uint64_t n, int err, int64_t min_depth, const bwb_geno_site_q **out, uint64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
