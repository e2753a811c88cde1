/*
 * bwb_kernels.h - shared kernel-side types and the utility kernels (gfx950).  Included by bwb_hip.hip.
 *
 *   k_relayout, k_relayout64   reference .bwt arrays -> 128-byte rank buckets of 64 characters (bwb_device.h)
 *   k_rank16     O_alphabet / O for a list of positions (parity tests), octet-cooperative rank
 *   k_rank_bench random-position rank micro-benchmark (octet-cooperative rank)
 *   k_locate     SA[row] by the invPsi walk (aln2sam)
 *   k_gather     per-read hit lists -> read order
 *   k_place      eval_aln + mapq for every read of a slot (`bwbble map`): one 48-byte placement record per read
 *   k_locus      the .ann record of every placement record and, on a bubble record, its reference coordinates (`bwbble map -B`)
 *   k_join_items, k_join_reads   a read's other placements that lie where its primary lies, and its MAPQ without them (`bwbble map -J`)
 *   k_lift_count, k_lift         a placement on a bubble record in the chromosome's coordinates: POS and CIGAR (`bwbble map -R`)
 *   k_text_pack, k_md_count, k_md   the forward text at 4 bits per character, and a read's NM and MD text against it (`bwbble map -D`)
 *   k_site_count, k_site_add, k_site_of, k_pile   the rank structure over the text's IUPAC sites, and the reads' allele counts at them (`bwbble map -A`)
 *   k_indel                      ref / alt read support per indel bubble, against a sorted table of the eligible bubbles (`bwbble map -I`)
 *   k_pile_q, k_geno_emit_q      the allele counts with a minimum base quality and the quality sums, and the genotype calls weighted by them (`bwbble map -b / -Y`)
 * The alignment kernels themselves (kl_calc_d, kl_search: one read per lane) are in bwb_lane.h.
 */
#pragma once
#include "bwb_device.h"

#define BWB_BLOCK 256
#define BWB_OCTS_PER_BLOCK 32
#define NONE32 0xFFFFFFFFu
#define BAD_LEN 0xFFFFu   /* lens[] marker of a read the kernels cannot represent (> 255 bases; < 12 with -P): it gets an empty record */
#define ST_OK 0
#define ST_SCRATCH_OVF 1  /* heap arena / interval list / hit list too small: re-run in a bigger class */
#define ST_OUT_OVF 2      /* the slot's hit log is full: host grows it and re-runs the read */
#define ST_D_OVF 3        /* kl_calc_d: SA-interval list too small; kl_search leaves the read to the re-run of both kernels in a bigger class */
#define ST_D_WAIT 4       /* k_dseed_inherit: the read's own calculate_d is done, the read its D_seed comes from is ST_D_OVF; kl_search leaves it too */

struct KParams {
	int max_diff, max_gapo, max_gape, max_entries;
	int mm_score, gapo_score, gape_score;
	int seed_length, max_diff_seed, max_best, no_indel_length;
	int num_buckets;
	int use_precalc; /* -P: the heap starts from the exact matches of the last 12 bases of rc (inexact_match.c:269-279) */
	int multiref;   /* 0: single-genome mode (-S): 4-letter children A,G,C,T in rows 1..4, 1-to-1 exact matching */
};

/* one resident batch of reads (a "slot" of the context): inputs, what kl_calc_d hands to kl_search, per-read status */
struct Batch {
	const uint8_t *reads;     /* [n][stride] read->seq codes */
	const uint16_t *lens;
	uint32_t n_reads, stride;
	uint8_t *dbuf;            /* [n][dstride]: what kl_calc_d hands to kl_search, one 16-byte RECORD PER FOUR READ POSITIONS (rec_put / rec_get below),
	                             then the read's N count (dstride-4) and its calculate_d work (dstride-8) */
	uint32_t dstride;
	uint8_t *status;          /* per read */
	uint32_t *dbg_iters;      /* optional (BWB_DEBUG_ITERS): loop iterations spent on each read */
};

struct OutBuf {
	uint4 *alns;              /* the slot's hit log, 48-byte records (bwb_aln: three uint4) */
	unsigned long long *count;
	uint64_t cap;
	uint64_t *off;            /* per read: first record */
	uint32_t *n;              /* per read: #records */
};

/* what kl_search needs to know about a slot: several slots are alive at once, because a read that is parked at the end of
 * a slice (see Work) belongs to an earlier batch than the reads the next slice starts */
struct SlotDesc {
	Batch b;
	OutBuf out;
	unsigned int *done;       /* reads of the slot that have been finished by kl_search (any status) */
};

/* the work of one launch */
struct Work {
	const uint32_t *worklist; /* read ids to process (NULL = 0..n_work-1) */
	uint32_t n_work;
	uint32_t *counter;        /* work-stealing cursor */
	uint32_t slot;            /* the slot those reads belong to */
	uint32_t suspend;         /* kl_search: when the cursor runs out a wave parks the reads it is working on in the lanes' save
	                             area and leaves (the next launch resumes them) instead of draining with ever fewer busy lanes */
	uint32_t slice_iters;     /* kl_search, test knob: park after this many loop iterations of a wave as well (0 = off) */
	uint32_t resume;          /* kl_search: lanes look for a parked read in their save area first */
};

enum { STAT_VIS_SINGLE = 0, STAT_VIS_ALPHA, STAT_POPS, STAT_PUSHES, STAT_ALNS, STAT_N, STAT_N_MAX, STAT_VIS_CALCD,
       STAT_BKT_SEARCH /* 128-byte buckets fetched by kl_search */, STAT_BKT_CALCD, STAT_PARKED /* reads parked at the end of a slice */,
       STAT_ENT_ST /* heap entries kl_search stored */, STAT_ENT_LD /* ... loaded */, STAT_REC_LD /* per-position records it loaded */,
       STAT_WAVE_ITERS = 16, STAT_WAVE_ITERS_CALCD = 17, STAT_LOCATE_STEPS = 18 /* k_locate: invPsi steps */, STAT_STAMPS = 24, STAT_HIST = 40 /* BWB_HIST diagnostic build */, STAT_BBPROF = 104 /* tools/bbprof.py: one 64-bit counter per basic block */,
#ifdef BWB_BBPROF
       STAT_WORDS = 104 + 2048 };
#else
       STAT_WORDS = 104 };
#endif

template <typename P> struct Intv { P L, U; };

/* The per-position data of a read, as kl_calc_d leaves it for kl_search.  An entry at read position i (aln_entry_t.i) consults
 * D[i-1], D[i-2] (inexact_match.c:317,399-405), D_seed[si-1], D_seed[si-2] with si = i - (len - seed_length) (:321-328,408-415) and the
 * base seq[len - i] it extends with.  One byte per D value: min(num_diff, 127) | 0x80 when sa_intv_width equals the previous
 * position's (the only way the width is ever used, :402-403,411-412).  Record m (16 bytes) serves the FOUR positions i = 4m .. 4m+3:
 *   bytes 0..5    D[k]   for k = 4m-2 .. 4m+3        (k < 0: 0)
 *   bytes 6..7    the bases of i = 4m .. 4m+3, 4 bits each (i & 3 = nibble)
 *   bytes 8..13   DS[k]  for the same k, DS[k] = D_seed[k - (len - seed_length)] - the seed's bounds moved to the read's positions
 *   bytes 14..15  m (the record's tag: kl_search keeps the record in registers and checks it against i >> 2)
 * so consecutive records overlap by two D bytes, and a search that walks down a read - a popped entry's match child is at i - 1 and is
 * popped next in 55 % of the pops - loads a record once per four positions (round 3: an 8-byte record per position, 0.8 loads per loop
 * iteration, 70 % of the kernel's metadata read requests). */
#define REC_BYTES 16
__host__ __device__ __forceinline__ uint32_t rec_count(uint32_t len) { return (len >> 2) + 1u; }
/* the byte D[k] (arr = 0) or DS[k] (arr = 8), k >= -2: in record (k + 2) >> 2, and again in the record before it when it is one of a record's first two */
/* (nrec = rec_count(len): the byte of the read's LAST position k = len - 1 has no record of its own when len % 4 == 3 - no entry sits beyond
 * position len - and is only written into the record before, where the entries at position len look for it; round 4 wrote it one record past
 * the read's records, into the per-read tail that holds calculate_d's work counter: ADVICE r4) */
__device__ __forceinline__ void rec_put(uint8_t *recs, uint32_t nrec, int arr, int k, uint32_t v) {
	const int m = (k + 2) >> 2, t = (k + 2) & 3;
	if ((uint32_t)m < nrec) recs[REC_BYTES * m + arr + t] = (uint8_t)v;
	if (t < 2 && m > 0) recs[REC_BYTES * (m - 1) + arr + 4 + t] = (uint8_t)v;
}
__device__ __forceinline__ uint32_t rec_get(const uint8_t *recs, int arr, int k) { return recs[REC_BYTES * ((k + 2) >> 2) + arr + ((k + 2) & 3)]; }

/* io.h:29,109: read base c (A0 G1 C2 T3) is compatible with code j iff gray(c) & grayVal[j]; N(10) excluded
 * (nucl_bases_table io.h:102-106).  Bit j of the mask = code j is a member. */
/* -S: child row j = 1..4 is base j-1 (A G C T), i.e. code nt4_gray[j-1] = 15, 3, 7, 1 (io.h:108, bwt.c:440-463) */
__device__ __forceinline__ uint32_t single_mask_codes(int c) { return c == 0 ? 1u << 15 : (c == 1 ? 1u << 3 : (c == 2 ? 1u << 7 : 1u << 1)); }
__device__ __forceinline__ uint32_t member_mask(int c) {
	/* A {8,9,11,12,13,14,15}  G {2,3,4,5,11,12,13}  C {4,5,6,7,8,9,11}  T {1,2,5,6,9,13,14} */
	return c == 0 ? 0xFB00u : (c == 1 ? 0x383Cu : (c == 2 ? 0x0BF0u : 0x6266u));
}

template <typename P> __device__ __forceinline__ void load_base(P *s_base, const DevIndex &ix) {
	for (int t = threadIdx.x; t < BWB_BASE_ROWS * 16; t += BWB_BLOCK) s_base[t] = (P)ix.base[t >> 4][t & 15];
	__syncthreads();
}
/* the base table (exact counts: O(), bwt.c:348-372), then its superblock rows once more as O_alphabet sees them (bwt.c:423-437): the codes
 * 5, 9, 11, 13 - never counted there - have C[j] - 1, to which the rank adds 1 - [first char of the block == j] (bwb_lane.h: side_finish);
 * the special positions -1 and length-1 are exact in that view too: they use the first table's rows */
template <typename P> __device__ __forceinline__ void load_base2(P *s_base, const DevIndex &ix) {
	for (int t = threadIdx.x; t < BWB_BASE_ROWS * 16; t += BWB_BLOCK) {
		const int row = t >> 4, j = t & 15;
		const P v = (P)ix.base[row][j];
		s_base[t] = v;
		if (row < BWB_NSB_MAX) s_base[BWB_BASE_ROWS * 16 + t] = ((0x2A20u >> j) & 1u) ? (P)(ix.base[BWB_ROW_NEG][j] - 1) : v;
	}
	__syncthreads();
}

/* ============================================================================================
 * Index re-layout: reference arrays (bwt words io.c:590-609, O rows bwt.c:280-291) -> buckets
 * One thread per 16-byte slice. blk0 = first block of this chunk; bwt/O point at the chunk.
 * ========================================================================================== */
__global__ void k_relayout(const uint32_t *bwt, const uint64_t *O, uint64_t blk0, uint64_t nblk_chunk, uint64_t nwords_chunk, uint64_t sa0_index,
                           const uint64_t *sbcount /* [NSB][16] exclusive counts at superblock starts */, uint4 *buckets) {
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nblk_chunk * 8) return;
	const uint64_t lb = t >> 3, blk = blk0 + lb;
	const int sl = (int)(t & 7);
	const uint64_t w0 = lb * 16;
	uint4 o;
	if (sl < 4) {
		const uint32_t first = w0 < nwords_chunk ? (bwt[w0] >> 28) : 0u;
		const uint64_t *row = O + lb * 16;
		const uint64_t *sb = sbcount + (blk >> BWB_SB_SHIFT) * 16;
		const int cs[4] = { 2 * sl, 2 * sl + 1, 2 * sl + 8, 2 * sl + 9 };
		uint32_t v[4];
		for (int q = 0; q < 4; q++) {
			const int c = cs[q];
			/* O rows are inclusive of position 128k and skip the sentinel row (bwt.c:284-288) */
			const bool counted = first == (uint32_t)c && !(c == 0 && blk * 128 == sa0_index);
			v[q] = (uint32_t)(row[c] - (counted ? 1u : 0u) - sb[c]);
		}
		o = make_uint4(v[0], v[1], v[2], v[3]);
	} else {
		const int w = sl - 4;
		uint32_t p[4] = { 0, 0, 0, 0 };
		for (int q = 0; q < 4; q++) {
			const uint64_t wi = w0 + 4 * w + q;
			const uint32_t word = wi < nwords_chunk ? bwt[wi] : 0u;
			for (int n = 0; n < 8; n++) {
				const uint32_t code = (word >> (28 - 4 * n)) & 15u; /* first char in bits 31-28, io.c:597 */
				const int j = 8 * q + n;
				p[0] |= (code & 1u) << j; p[1] |= ((code >> 1) & 1u) << j; p[2] |= ((code >> 2) & 1u) << j; p[3] |= ((code >> 3) & 1u) << j;
			}
		}
		o = make_uint4(p[0], p[1], p[2], p[3]);
	}
	buckets[lb * 8 + sl] = o; /* (chunk-local: the 128-character form only lives in a staging buffer, k_relayout64 below makes the index) */
}

/* The index proper (bwb_device.h): 64-character buckets, derived from a chunk of 128-character ones.  One thread per new bucket. */
__device__ __forceinline__ void sub_counts16(const uint4 p, uint32_t out[16]) {
	const uint32_t a[4] = { ~p.x & ~p.y, p.x & ~p.y, ~p.x & p.y, p.x & p.y };
	const uint32_t b[4] = { ~p.z & ~p.w, p.z & ~p.w, ~p.z & p.w, p.z & p.w };
	for (int c = 0; c < 16; c++) out[c] = (uint32_t)__popc(a[c & 3] & b[c >> 2]);
}
__global__ void k_relayout64(const uint4 *b128, uint64_t nblk128, uint4 *b64) {
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nblk128 * 2) return;
	const uint4 *src = b128 + (t >> 1) * 8;
	const int half = (int)(t & 1);
	uint4 cnt[4] = { src[0], src[1], src[2], src[3] };
	const uint4 s4 = src[4];
	const uint4 pa = src[4 + 2 * half], pb = src[5 + 2 * half];
	const uint32_t first = (s4.x & 1u) | ((s4.y & 1u) << 1) | ((s4.z & 1u) << 2) | ((s4.w & 1u) << 3);
	uint32_t m0[16];
	sub_counts16(pa, m0);
	if (half) {
		uint32_t h0[16], h1[16];
		sub_counts16(src[4], h0); sub_counts16(src[5], h1);
		for (int s = 0; s < 4; s++) {
			cnt[s].x += h0[2 * s] + h1[2 * s]; cnt[s].y += h0[2 * s + 1] + h1[2 * s + 1];
			cnt[s].z += h0[2 * s + 8] + h1[2 * s + 8]; cnt[s].w += h0[2 * s + 9] + h1[2 * s + 9];
		}
	}
	uint32_t mid[4];
	for (int s = 0; s < 4; s++) mid[s] = m0[2 * s] | (m0[2 * s + 1] << 8) | (m0[2 * s + 8] << 16) | (m0[2 * s + 9] << 24);
	uint4 *dst = b64 + t * 8;
	dst[0] = cnt[0]; dst[1] = cnt[1]; dst[2] = cnt[2]; dst[3] = cnt[3];
	dst[4] = pa; dst[5] = pb;
	dst[6] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
	dst[7] = make_uint4(first, 0u, 0u, 0u);
}

/* O_alphabet / exact Occ16 for a list of positions: one octet per query */
__global__ __launch_bounds__(BWB_BLOCK) void k_rank16(DevIndex ix, const uint64_t *pos, uint64_t n, int inc, int exact, uint64_t *out) {
	__shared__ uint64_t s_base[BWB_BASE_ROWS * 16];
	load_base<uint64_t>(s_base, ix);
	const int lane = threadIdx.x & 63, ol = lane & 7;
	const uint64_t noct = (uint64_t)gridDim.x * BWB_OCTS_PER_BLOCK;
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_OCTS_PER_BLOCK + (threadIdx.x >> 3); q < n; q += noct) {
		RankReq<uint64_t> ra;
		rank_issue<uint64_t>(ix.buckets, ix.length - 1, pos[q], ol, ra);
		uint64_t v0, v1;
		if (exact) rank_finish<uint64_t, false>(ra, s_base, ol, lane, v0, v1);
		else rank_finish<uint64_t, true>(ra, s_base, ol, lane, v0, v1);
		out[q * 16 + 2 * ol] = ol == 0 ? 0 : v0 + inc;
		out[q * 16 + 2 * ol + 1] = v1 + inc;
	}
}

/* Rank micro-benchmark: pseudo-random positions, 4 independent visits in flight per octet */
template <typename P>
__global__ __launch_bounds__(BWB_BLOCK) void k_rank_bench(DevIndex ix, uint64_t n, uint64_t seed, unsigned long long *checksum) {
	__shared__ P s_base[BWB_BASE_ROWS * 16];
	load_base<P>(s_base, ix);
	const int lane = threadIdx.x & 63, ol = lane & 7;
	const uint64_t noct = (uint64_t)gridDim.x * BWB_OCTS_PER_BLOCK;
	unsigned long long acc = 0;
	for (uint64_t q = ((uint64_t)blockIdx.x * BWB_OCTS_PER_BLOCK + (threadIdx.x >> 3)) * 4; q < n; q += noct * 4) {
		RankReq<P> rq[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			uint64_t x = (q + u) * 0x9E3779B97F4A7C15ull + seed;
			x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
			rank_issue<P>(ix.buckets, (P)(ix.length - 1), (P)(x % (ix.length - 1)), ol, rq[u]);
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			P v0, v1;
			rank_finish<P, false>(rq[u], s_base, ol, lane, v0, v1);
			acc += (ol == 0 ? 0ull : (unsigned long long)v0) + 3ull * v1; /* codes 1..15 (code 0 = '$' is never a child) */
		}
	}
	acc += __shfl_xor(acc, 1); acc += __shfl_xor(acc, 2); acc += __shfl_xor(acc, 4);
	if (ol == 0 && acc) atomicAdd(checksum, acc);
}

/* gathers the per-read hit lists into read order */
__global__ void k_gather(const uint4 *log, const uint64_t *off, const uint32_t *n, const uint64_t *dst_off, uint32_t n_reads, uint4 *dst) {
	const uint32_t rid = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
	if (rid >= n_reads) return;
	const int ol = threadIdx.x & 7;
	const uint64_t so = off[rid] * 2, d = dst_off[rid] * 2;
	const uint32_t cnt = n[rid] * 2;
	for (uint32_t t = ol; t < cnt; t += 8) dst[d + t] = log[so + t];
}

/* D_seed of a read that is not longer than the seed.  The reference computes D_seed only when len > seed_length
 * (inexact_match.c:62-64) but inexact_match reads it regardless (:321-328,408-415): the serial path (-t 1, one buffer for the
 * whole file, :35) therefore sees the bounds of the LAST LONGER READ BEFORE IT in the file - zeros when there is none.
 * src[r] names that read (host: slot_upload); the records carry the seed's bounds at the read's own positions (rec_put), so read r
 * takes the byte of position k + len_q - len_r of read q.  Runs after kl_calc_d. */
__global__ void k_dseed_inherit(Batch b, const uint32_t *src, uint32_t n) {
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n) return;
	const uint32_t q = src[r];
	if (q == NONE32) return;
	/* its source waits for a larger scratch class: so does this read (its own calculate_d is not repeated, unless that overflowed as well) */
	if (b.status[q] == ST_D_OVF) { if (b.status[r] != ST_D_OVF) b.status[r] = ST_D_WAIT; return; }
	const int lr = b.lens[r], lq = b.lens[q];
	uint8_t *rr = b.dbuf + (size_t)r * b.dstride;
	const uint8_t *rq = b.dbuf + (size_t)q * b.dstride;
	/* DS of read r at position k (of r) = DS of read q at position k + len_q - len_r (of q): the same seed index */
	for (int k = -2; k < lr; k++) rec_put(rr, rec_count((uint32_t)lr), 8, k, rec_get(rq, 8, k + lq - lr));
	if (b.status[r] == ST_D_WAIT) b.status[r] = ST_OK; /* (a re-run class has made the source fit: the search may have the read now) */
}

/* The invPsi walk from row i to the next sampled row (bwt.c:311-329, SA_INTERVAL = 32, bwt.h:16), by one octet: returns that row and adds
 * the steps taken to j (each one rank-block visit, the step through the sentinel row included).  SA[i0] = (SA[row >> 5] + j) % length.
 * Shared by k_locate and k_place. */
__device__ __forceinline__ uint64_t sa_walk(const DevIndex &ix, const uint64_t *s_base, uint64_t sa0_index, uint64_t i, int lane, int ol, uint64_t &j) {
	while ((i & 31) != 0) {
		if (i == sa0_index) { i = 0; j++; continue; } /* invPsi bwt.c:312-314 */
		RankReq<uint64_t> ra;
		rank_issue<uint64_t>(ix.buckets, ix.length - 1, i, ol, ra);
		/* B(i), bwt.c:337-345: bit (i&31) of the planes held by lane 4 + ((i&63)>>5) */
		const uint4 cq = ra.regular ? ra.q : ix.buckets[(i >> BKT_SHIFT) * 8 + ol]; /* i == length-1 is not ranked via its bucket */
		const int off = (int)(i & BKT_MASK), srcl = (lane & ~7) + 4 + (off >> 5), bit = off & 31;
		const uint32_t code_here = ((cq.x >> bit) & 1u) | (((cq.y >> bit) & 1u) << 1) | (((cq.z >> bit) & 1u) << 2) | (((cq.w >> bit) & 1u) << 3);
		const uint32_t code = oct_bcast(code_here, srcl);
		uint64_t v0, v1;
		rank_finish<uint64_t, false>(ra, s_base, ol, lane, v0, v1);
		/* C[c] + O(c,i): held by lane c>>1.  The sentinel row is stored as code 0 but is not a '$' (bwt.c:364) */
		const uint64_t mine = (code & 1u) ? v1 : v0;
		uint64_t nxt = oct_bcast(mine, (lane & ~7) + (int)(code >> 1));
		if (code == 0 && ra.regular && sa0_index >= (i & ~127ull) && sa0_index <= i) nxt--;
		i = nxt;
		j++;
	}
	return i;
}

/* SA[row] by the invPsi walk: one octet per row */
__global__ __launch_bounds__(BWB_BLOCK) void k_locate(DevIndex ix, const uint64_t *SA, uint64_t sa0_index, const uint64_t *rows, uint64_t n, uint64_t *out, unsigned long long *stats) {
	__shared__ uint64_t s_base[BWB_BASE_ROWS * 16];
	load_base<uint64_t>(s_base, ix);
	const int lane = threadIdx.x & 63, ol = lane & 7;
	const uint64_t noct = (uint64_t)gridDim.x * BWB_OCTS_PER_BLOCK;
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_OCTS_PER_BLOCK + (threadIdx.x >> 3); q < n; q += noct) {
		uint64_t j = 0;
		const uint64_t i = sa_walk(ix, s_base, sa0_index, rows[q], lane, ol, j);
		if (ol == 0) { out[q] = (SA[i >> 5] + j) % ix.length; if (j) atomicAdd(&stats[STAT_LOCATE_STEPS], (unsigned long long)j); } /* (j: invPsi steps = rank-block visits, the step through the sentinel row included) */
	}
}

/* get_aln_length (align.c:748-757) of a hit from its gap runs rw[] (four words of two runs, as the hit log holds them): aln_length minus the
 * path positions below aln_length that are insertions.  The runs are applied in order like aln_path_bytes does (a later run overwrites an
 * earlier one), on a 256-bit map: aln_length is 8-bit wrapped.  Shared by k_place and k_place_alt. */
__device__ __forceinline__ uint32_t place_ref_len(uint32_t alen, const uint32_t rw[4]) {
	uint64_t ins[4] = { 0, 0, 0, 0 };
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint32_t run = (rw[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
		if (run == 0xFFFFu) continue;
		const uint32_t start = run & 0xFFu, len = (run >> 8) & 0x7Fu, del = run >> 15;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const int lo = (int)start - 64 * q, hi = lo + (int)len; /* bits [lo, hi) of word q */
			const int a = lo < 0 ? 0 : lo, b = hi > 64 ? 64 : hi;
			if (a >= b) continue;
			const uint64_t m = (b - a == 64 ? ~0ull : ((1ull << (b - a)) - 1ull)) << a;
			ins[q] = del ? (ins[q] & ~m) : (ins[q] | m);
		}
	}
	uint32_t n_ins = 0;
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const int top = (int)alen - 64 * q;
		if (top <= 0) continue;
		n_ins += (uint32_t)__popcll(top >= 64 ? ins[q] : (ins[q] & ((1ull << top) - 1ull)));
	}
	return alen - n_ins;
}
/* The gap runs as aln2sam sees them: the .aln file holds the path from its end to its start (align.c:363-373) and the loader
 * fills it in that order (align.c:466-476), so eval_aln and the CIGAR code work on the align-time path REVERSED.  A run
 * (start, len) of a path of alen positions becomes (alen - start - len, len); ascending by start, unused runs last. */
__device__ __forceinline__ void place_runs(uint32_t alen, const uint32_t rw[4], uint32_t rr[8]) {
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint32_t run = (rw[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
		rr[k] = run == 0xFFFFu ? 0xFFFFu : (((alen - (run & 0xFFu) - ((run >> 8) & 0x7Fu)) & 0xFFu) | (run & 0xFF00u));
	}
	if ((rw[0] & rw[1] & rw[2] & rw[3]) != 0xFFFFFFFFu) { /* (a sorting network of 19 exchanges; most hits have no gap at all) */
#define PLACE_CE(a, b) { const uint32_t ka = rr[a] == 0xFFFFu ? 0x1FFu : (rr[a] & 0xFFu), kb = rr[b] == 0xFFFFu ? 0x1FFu : (rr[b] & 0xFFu); if (ka > kb) { const uint32_t t = rr[a]; rr[a] = rr[b]; rr[b] = t; } }
		PLACE_CE(0, 2) PLACE_CE(1, 3) PLACE_CE(4, 6) PLACE_CE(5, 7) PLACE_CE(0, 4) PLACE_CE(1, 5) PLACE_CE(2, 6) PLACE_CE(3, 7)
		PLACE_CE(0, 1) PLACE_CE(2, 3) PLACE_CE(4, 5) PLACE_CE(6, 7) PLACE_CE(2, 4) PLACE_CE(3, 5) PLACE_CE(1, 4) PLACE_CE(3, 6)
		PLACE_CE(1, 2) PLACE_CE(3, 4) PLACE_CE(5, 6)
#undef PLACE_CE
	}
}

/* mapq, align.c:738-746: all integer, qtab[n] = (int)(4.343 * log(n) + 0.5) tabulated by the host (k_place, k_join_reads) */
__device__ __forceinline__ uint32_t place_mapq(int top1, int top2, int num_mm, int max_mm, const uint8_t *qtab) {
	if (top1 == 0) return 23u;
	if (top1 > 1) return 0u;
	if (num_mm == max_mm) return 25u;
	if (top2 == 0) return 37u;
	const uint32_t q = qtab[top2 >= 255 ? 255 : (top2 < 0 ? 0 : top2)];
	return 23 < q ? 0u : 23 - q;
}

/* eval_aln + mapq (align.c:738-812) for every read of a slot, where its hits lie: one octet per read -> one 48-byte bwb_place record
 * (include/bwbble_hip.h) in read order.  log/off/n are the slot's hit log (bwb_aln: three uint4 per hit, a read's hits contiguous and in
 * discovery order).  All integer: qtab[n] = (int)(4.343 * log(n) + 0.5), tabulated by the host (the only floating point of mapq). */
#define PLACE_F_MAPPED 1u
#define PLACE_F_REVERSE 2u
#define PLACE_F_BAD 0x80u  /* the read's hits lie outside the log / its row outside the index: nothing was read (the host reports it) */
__global__ __launch_bounds__(BWB_BLOCK) void k_place(DevIndex ix, const uint64_t *SA, uint64_t sa0_index, const uint4 *log, uint64_t log_n, const uint64_t *off, const uint32_t *n,
                                                      uint32_t n_reads, int max_mm, const uint8_t *qtab, uint4 *out, unsigned long long *steps) {
	__shared__ uint64_t s_base[BWB_BASE_ROWS * 16];
	load_base<uint64_t>(s_base, ix);
	const int lane = threadIdx.x & 63, ol = lane & 7;
	const uint32_t noct = gridDim.x * BWB_OCTS_PER_BLOCK;
	for (uint32_t r = blockIdx.x * BWB_OCTS_PER_BLOCK + (threadIdx.x >> 3); r < n_reads; r += noct) {
		const uint32_t ne = n[r];
		const uint64_t o = ne ? off[r] : 0;
		uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, w2 = w0; /* n == 0: unmapped, everything zero */
		if (ne && (o > log_n || ne > log_n - o)) w1.x = PLACE_F_BAD << 24;
		else if (ne) {
			const uint4 *e = log + o * 3;
			const uint4 e0 = e[0], e1 = e[1], e2 = e[2]; /* L, U | score16 mm go | ge - alen16 | runs 0..3 | runs 4..7, - */
			const uint32_t best = e1.x & 0xFFFFu;
			/* top1 / top2 (align.c:771-779): the octet strides over the hits; 32-bit sums like read_t's ints */
			uint32_t t1 = 0, t2 = 0;
			for (uint32_t t = (uint32_t)ol; t < ne; t += 8) {
				const uint4 a = e[(size_t)t * 3], b = e[(size_t)t * 3 + 1];
				const uint32_t w = a.z - a.x + 1u; /* (int)(U - L + 1) */
				if ((b.x & 0xFFFFu) > best) t2 += w; else t1 += w;
			}
			t1 += __shfl_xor(t1, 1); t1 += __shfl_xor(t1, 2); t1 += __shfl_xor(t1, 4);
			t2 += __shfl_xor(t2, 1); t2 += __shfl_xor(t2, 2); t2 += __shfl_xor(t2, 4);
			const uint64_t L = (uint64_t)e0.x | ((uint64_t)e0.y << 32);
			const uint32_t num_mm = (e1.x >> 16) & 0xFFu, alen = e1.y >> 16;
			const uint32_t rw[4] = { e1.z, e1.w, e2.x, e2.y };
			const uint32_t ref_len = place_ref_len(alen, rw);
			uint32_t rr[8];
			place_runs(alen, rw, rr);
			if (L >= ix.length) w1.x = PLACE_F_BAD << 24;
			else {
				uint64_t j = 0;
				const uint64_t i = sa_walk(ix, s_base, sa0_index, L, lane, ol, j);
				const uint64_t rp = (SA[i >> 5] + j) % ix.length;
				if (ol == 0 && j) atomicAdd(steps, (unsigned long long)j);
				/* strand and text position, align.c:790-799 */
				uint32_t flags = PLACE_F_MAPPED;
				uint64_t pos;
				if (rp > (ix.length - 1) / 2) pos = ((ix.length - 1) - rp - 1) - (uint64_t)ref_len + 1;
				else { flags |= PLACE_F_REVERSE; pos = rp; }
				const uint32_t mq = place_mapq((int)t1, (int)t2, (int)num_mm, max_mm, qtab);
				w0 = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), t1, t2);
				w1 = make_uint4(best | (mq << 16) | (flags << 24), (e1.x >> 16) | ((e1.y & 0xFFu) << 16), alen | (ref_len << 16), 0u);
				w2 = make_uint4(rr[0] | (rr[1] << 16), rr[2] | (rr[3] << 16), rr[4] | (rr[5] << 16), rr[6] | (rr[7] << 16));
			}
		}
		uint4 *dst = out + (size_t)r * 3;
		if (ol == 0) dst[0] = w0;
		else if (ol == 1) dst[1] = w1;
		else if (ol == 2) dst[2] = w2;
	}
}

/* ---- bubble hits in reference coordinates (`map -B`: the bC / bP tags) ----------------------------------------------------------
 * For every placement record: the .ann record that contains its text position, the position SAM prints, and on a `>bubbleN` record what
 * the reference's sam_pad makes of that position (include/bwbble_hip.h: bwb_locus; mg-ref/sam_pad.cpp:75-87).  One read per LANE - there is
 * no bucket to gather, so not the octet layout - in a grid-stride loop.  The search is the branch-free lower bound: `trips` =
 * ceil(log2(n_seq)) steps for every lane (a kernel argument, so the loop is uniform: selects, no divergent while), the candidates
 * [lo, lo + len) shrinking to one record; every start[] it reads lies inside the table (lo + len <= n_seq throughout, half < len).  The
 * first positions of 1.3 M records are 10 MB: they stay in the Infinity Cache.  bub[] holds the bwb_bubble records as five 64-bit words
 * (A, B_minus_A, C, D_minus_C, ref_len | alt_len << 32); bubble_of[] was checked against its size on the host (bwb_hip_set_loci).  The
 * sums wrap (unsigned arithmetic, compared as signed) like the host's bubble_locus. */
struct Locus { uint32_t seqid /* 0xFFFFFFFF: none */, pos1; int32_t b; uint32_t kind; uint64_t lo, hi; };
__device__ __forceinline__ Locus locus_at(uint64_t pos, bool mapped, const uint64_t *start, const uint64_t *end, const int32_t *bubble_of, uint32_t n_seq, uint32_t trips,
                                          const uint64_t *bub) {
	uint32_t lo = 0, len = n_seq;
	for (uint32_t t = 0; t < trips; t++) {
		const uint32_t half = len >> 1, mid = lo + half;
		lo = start[mid] <= pos ? mid : lo;
		len -= half;
	}
	const uint64_t s = start[lo];
	const bool in = mapped && pos >= s && pos <= end[lo];
	const int32_t b = in ? bubble_of[lo] : -1;
	const uint32_t pos1 = in ? (uint32_t)(pos - s + 1) : 0u;
	uint32_t kind = 0;
	uint64_t rlo = 0, rhi = 0;
	if (b >= 0) {
		const uint64_t *q = bub + (size_t)b * 5;
		const uint64_t A = q[0], B = q[1], C = q[2], D = q[3], la = q[4];
		const uint64_t ref_len = (uint64_t)(int64_t)(int32_t)(uint32_t)la, alt_len = (uint64_t)(int64_t)(int32_t)(uint32_t)(la >> 32);
		const int64_t locus = (int64_t)(int32_t)pos1;
		const uint64_t right = B + alt_len + 1u;
		const bool left_flank = locus >= 1 && locus <= (int64_t)B;
		const bool right_flank = locus >= (int64_t)right && locus <= (int64_t)(right + D);
		const uint64_t point = left_flank ? A + (uint64_t)locus - 1u : (uint64_t)locus + C - right;
		const bool is_point = left_flank || right_flank;
		kind = is_point ? 1u : 2u;
		rlo = is_point ? point : A + B;
		rhi = is_point ? point : A + B + ref_len - 1u;
	}
	return Locus{ in ? lo : 0xFFFFFFFFu, pos1, b, kind, rlo, rhi };
}
__global__ __launch_bounds__(BWB_BLOCK) void k_locus(const uint4 *places, uint32_t n_reads, const uint64_t *start, const uint64_t *end, const int32_t *bubble_of,
                                                      uint32_t n_seq, uint32_t trips, const uint64_t *bub, uint4 *out) {
	const uint32_t stride = gridDim.x * BWB_BLOCK;
	for (uint32_t r = blockIdx.x * BWB_BLOCK + threadIdx.x; r < n_reads; r += stride) {
		const uint4 p0 = places[(size_t)r * 3], p1 = places[(size_t)r * 3 + 1];
		const Locus lc = locus_at((uint64_t)p0.x | ((uint64_t)p0.y << 32), ((p1.x >> 24) & PLACE_F_MAPPED) != 0, start, end, bubble_of, n_seq, trips, bub);
		uint4 *dst = out + (size_t)r * 2;
		dst[0] = make_uint4(lc.seqid, lc.pos1, (uint32_t)lc.b, lc.kind);
		dst[1] = make_uint4((uint32_t)lc.lo, (uint32_t)(lc.lo >> 32), (uint32_t)lc.hi, (uint32_t)(lc.hi >> 32));
	}
}

/* ---- a read's other placements (`map -X N`: the X0 / X1 / XA tags) -----------------------------------------------------------
 * A read's PLACEMENTS are the rows e[0].L .. e[0].U, then e[1].L .. e[1].U, and so on through its hits in discovery order; placement 0 is
 * what k_place reports.  T = the number of placements, 64-bit and saturating (a hit with U < L saturates it).  With 2 <= T <= N + 1 the read
 * lists the placements 1 .. T - 1 as items (BWA's rule: too many placements, no list), one 32-byte bwb_alt record each
 * (include/bwbble_hip.h).  The work is per item, not per read - most reads own none, a few own up to 255 - so: k_alt_count (items per
 * read), an exclusive scan of the counts (k_scan_blocks / k_scan_sums / k_scan_add), and k_place_alt with one octet per ITEM. */

/* cnt[r] = (2 <= T <= max_alt + 1) ? T - 1 : 0.  One thread per read; the sum stops as soon as it exceeds max_alt + 1, so a thread reads at
 * most max_alt + 2 hits.  A read whose hits lie outside the log gets no items (k_place flags the read itself). */
__global__ __launch_bounds__(BWB_BLOCK) void k_alt_count(const uint4 *log, uint64_t log_n, const uint64_t *off, const uint32_t *n, uint32_t n_reads, uint32_t max_alt, uint32_t *cnt) {
	const uint32_t r = blockIdx.x * BWB_BLOCK + threadIdx.x;
	if (r >= n_reads) return;
	const uint32_t ne = n[r];
	const uint64_t o = ne ? off[r] : 0;
	uint64_t T = 0;
	if (ne && !(o > log_n || ne > log_n - o)) {
		const uint4 *e = log + o * 3;
		for (uint32_t t = 0; t < ne && T <= (uint64_t)max_alt + 1; t++) {
			const uint4 a = e[(size_t)t * 3];
			const uint64_t L = (uint64_t)a.x | ((uint64_t)a.y << 32), U = (uint64_t)a.z | ((uint64_t)a.w << 32);
			const uint64_t w = U - L + 1; /* (0 for the interval of every row: saturated as well) */
			if (U < L || w == 0 || T + w < T) T = ~0ull; else T += w;
		}
	}
	cnt[r] = (T >= 2 && T <= (uint64_t)max_alt + 1) ? (uint32_t)(T - 1) : 0u;
}

/* Exclusive scan of cnt[0 .. n) into off[0 .. n], off[n] = the total.  k_scan_blocks: every block scans BWB_BLOCK counts - inclusive scan
 * of each wave by shuffles, the waves' sums through LDS - and leaves the block-local exclusive values in off[] and its sum in bsum[];
 * k_scan_sums (one block) turns bsum[] into the blocks' offsets and writes the total; k_scan_add adds them.  No host round trip. */
__global__ __launch_bounds__(BWB_BLOCK) void k_scan_blocks(const uint32_t *cnt, uint32_t n, uint64_t *off, uint64_t *bsum) {
	__shared__ uint32_t s_wave[BWB_BLOCK / 64];
	const uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint32_t v = i < n ? cnt[i] : 0u;
	uint32_t inc = v; /* (a block's sum is at most 256 * 255) */
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d); if (lane >= d) inc += t; }
	if (lane == 63) s_wave[wv] = inc;
	__syncthreads();
	uint32_t before = 0, total = 0;
#pragma unroll
	for (int k = 0; k < BWB_BLOCK / 64; k++) { if (k < wv) before += s_wave[k]; total += s_wave[k]; }
	if (i < n) off[i] = (uint64_t)(before + inc - v);
	if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(BWB_BLOCK) void k_scan_sums(uint64_t *bsum, uint32_t nblk, uint64_t *total_out) {
	__shared__ uint64_t s_wave[BWB_BLOCK / 64];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	uint64_t carry = 0;
	for (uint32_t b0 = 0; b0 < nblk; b0 += BWB_BLOCK) { /* (every thread of the block takes every turn of this loop: the barriers are uniform) */
		const uint32_t i = b0 + threadIdx.x;
		const uint64_t v = i < nblk ? bsum[i] : 0ull;
		uint64_t inc = v;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) { const uint64_t t = __shfl_up(inc, d); if (lane >= d) inc += t; }
		if (lane == 63) s_wave[wv] = inc;
		__syncthreads();
		uint64_t before = 0, total = 0;
#pragma unroll
		for (int k = 0; k < BWB_BLOCK / 64; k++) { if (k < wv) before += s_wave[k]; total += s_wave[k]; }
		if (i < nblk) bsum[i] = carry + before + inc - v;
		carry += total;
		__syncthreads();
	}
	if (threadIdx.x == 0) *total_out = carry;
}
__global__ __launch_bounds__(BWB_BLOCK) void k_scan_add(uint64_t *off, uint32_t n, const uint64_t *bsum) {
	const uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x;
	if (i < n) off[i] += bsum[blockIdx.x];
}

/* eval_aln (align.c:786-801) of item q = placement q - alt_off[r] + 1 of read r, the read found by binary search in alt_off[0 .. n_reads]:
 * hit h and row L_h + d by a linear scan over the read's hits (at most max_alt + 1 of them come before the last placement), the same walk,
 * strand rule and position formula as the primary's, that hit's ref_len and reversed gap runs.  One octet per item, grid-strided.  An item
 * whose row is not a row of the index, or whose hit is not where the counts said, is flagged PLACE_F_BAD and counted in ctl[1]; nothing is
 * looked up for it.  ctl[0]: invPsi steps, added once per wave. */
__global__ __launch_bounds__(BWB_BLOCK) void k_place_alt(DevIndex ix, const uint64_t *SA, uint64_t sa0_index, const uint4 *log, uint64_t log_n, const uint64_t *off, const uint32_t *n,
                                                          uint32_t n_reads, const uint64_t *alt_off, uint64_t n_items, uint4 *out, unsigned long long *ctl) {
	__shared__ uint64_t s_base[BWB_BASE_ROWS * 16];
	load_base<uint64_t>(s_base, ix);
	const int lane = threadIdx.x & 63, ol = lane & 7;
	const uint64_t noct = (uint64_t)gridDim.x * BWB_OCTS_PER_BLOCK;
	unsigned long long my_steps = 0, my_bad = 0; /* of this octet's items (kept by its lane 0) */
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_OCTS_PER_BLOCK + (threadIdx.x >> 3); q < n_items; q += noct) {
		/* the last read r with alt_off[r] <= q (reads without items share their successor's offset: the last one is the owner) */
		uint32_t lo = 0, hi = n_reads - 1;
		while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if (alt_off[mid] <= q) lo = mid; else hi = mid - 1; }
		const uint32_t r = lo, ne = n[r];
		const uint64_t o = ne ? off[r] : 0;
		uint64_t k = q - alt_off[r] + 1; /* the placement: the primary is skipped */
		uint4 w0 = make_uint4(0u, 0u, PLACE_F_BAD, 0u), w1 = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
		bool found = false;
		uint32_t h = 0;
		uint64_t row = 0;
		if (ne && !(o > log_n || ne > log_n - o)) {
			const uint4 *e = log + o * 3;
			for (; h < ne && h < 256; h++) {
				const uint4 a = e[(size_t)h * 3];
				const uint64_t L = (uint64_t)a.x | ((uint64_t)a.y << 32), U = (uint64_t)a.z | ((uint64_t)a.w << 32);
				if (U < L) break;
				const uint64_t w = U - L + 1;
				if (w == 0 || k < w) { row = L + k; found = row >= L && row < ix.length; break; }
				k -= w;
			}
		}
		if (found) {
			const uint4 *e = log + (o + h) * 3;
			const uint4 e1 = e[1], e2 = e[2];
			const uint32_t alen = e1.y >> 16;
			const uint32_t rw[4] = { e1.z, e1.w, e2.x, e2.y };
			const uint32_t ref_len = place_ref_len(alen, rw);
			uint32_t rr[8];
			place_runs(alen, rw, rr);
			uint64_t j = 0;
			const uint64_t i = sa_walk(ix, s_base, sa0_index, row, lane, ol, j);
			const uint64_t rp = (SA[i >> 5] + j) % ix.length;
			if (ol == 0) my_steps += j;
			uint32_t flags = PLACE_F_MAPPED;
			uint64_t pos;
			if (rp > (ix.length - 1) / 2) pos = ((ix.length - 1) - rp - 1) - (uint64_t)ref_len + 1;
			else { flags |= PLACE_F_REVERSE; pos = rp; }
			/* pos | flags hit mm go | ge - alen16 || the runs */
			w0 = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), flags | (h << 8) | (e1.x & 0xFFFF0000u), (e1.y & 0xFFu) | (alen << 16));
			w1 = make_uint4(rr[0] | (rr[1] << 16), rr[2] | (rr[3] << 16), rr[4] | (rr[5] << 16), rr[6] | (rr[7] << 16));
		} else if (ol == 0) my_bad++;
		uint4 *dst = out + q * 2;
		if (ol == 0) dst[0] = w0;
		else if (ol == 1) dst[1] = w1;
	}
	/* one atomic per wave: the eight octets' counts (held by their lanes 0; the other lanes hold zeros) summed by shuffles */
	my_steps += __shfl_xor(my_steps, 8); my_steps += __shfl_xor(my_steps, 16); my_steps += __shfl_xor(my_steps, 32);
	my_bad += __shfl_xor(my_bad, 8); my_bad += __shfl_xor(my_bad, 16); my_bad += __shfl_xor(my_bad, 32);
	if (lane == 0) {
		if (my_steps) atomicAdd(&ctl[0], my_steps);
		if (my_bad) atomicAdd(&ctl[1], my_bad);
	}
}

/* ---- a read's placements counted by locus (`map -X N -B table -J`) -------------------------------------------------------------
 * The rule is in include/bwbble_hip.h (bwb_join).  Per ITEM like k_place_alt, and for the same reason; nothing is gathered, so one item per
 * LANE like k_locus.  k_join_items: the item's owner by the branch-free lower bound over alt_off[0 .. n_reads) - the last read whose offset
 * is <= q: reads without items share their successor's offset -, `owner_trips` = ceil(log2(n_reads)) steps for every lane; the item's own
 * locus by k_locus's search and rule (locus_at); the primary's from the bwb_locus record k_locus left for the read; one class byte.  The
 * suboptimal bit: the score of hit `hit` in the hit log against the primary's (bwb_place.score is the first hit's), or with alt_sub != NULL
 * the caller's byte (bwb_hip_join_records).  chrom_of[] was checked against the record table on the host (bwb_hip_set_bubble_chrom). */
#define JOIN_C_JOINED 1u
#define JOIN_C_SUB 2u
/* (c, lo, hi') of a placement from its locus record; false: it has none */
__device__ __forceinline__ bool join_locus(uint32_t seqid, uint32_t pos1, int32_t b, uint64_t rlo, uint64_t rhi, const int32_t *chrom_of, int32_t &c, int64_t &lo, int64_t &hi) {
	const bool has = seqid != 0xFFFFFFFFu, bubble = has && b >= 0;
	c = bubble ? chrom_of[b] : (int32_t)seqid;
	lo = bubble ? (int64_t)rlo : (int64_t)(int32_t)pos1;
	hi = bubble ? (int64_t)rhi : lo;
	hi = hi < lo ? lo : hi; /* a pure insertion's empty range counts as its left edge */
	return has;
}
__global__ __launch_bounds__(BWB_BLOCK) void k_join_items(const uint4 *places, uint32_t n_reads, uint32_t owner_trips, const uint64_t *alt_off, const uint4 *alts, uint64_t n_items,
                                                           const uint4 *loci, const uint64_t *start, const uint64_t *end, const int32_t *bubble_of, uint32_t n_seq, uint32_t trips,
                                                           const uint64_t *bub, const int32_t *chrom_of, const uint4 *log, uint64_t log_n, const uint64_t *off, const uint32_t *n,
                                                           const uint8_t *alt_sub, uint8_t *cls) {
	const uint64_t stride = (uint64_t)gridDim.x * BWB_BLOCK;
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_items; q += stride) {
		uint32_t r = 0, len = n_reads;
		for (uint32_t t = 0; t < owner_trips; t++) {
			const uint32_t half = len >> 1, mid = r + half;
			r = alt_off[mid] <= q ? mid : r;
			len -= half;
		}
		const uint4 a0 = alts[q * 2]; /* pos | flags hit mm go | ge - alen16 */
		const uint32_t hit = (a0.z >> 8) & 0xFFu;
		const Locus il = locus_at((uint64_t)a0.x | ((uint64_t)a0.y << 32), (a0.z & PLACE_F_MAPPED) != 0, start, end, bubble_of, n_seq, trips, bub);
		const uint4 p1 = places[(size_t)r * 3 + 1], l0 = loci[(size_t)r * 2], l1 = loci[(size_t)r * 2 + 1];
		int32_t ci, cp;
		int64_t loi, hii, lop, hip;
		const bool has_i = join_locus(il.seqid, il.pos1, il.b, il.lo, il.hi, chrom_of, ci, loi, hii);
		const bool has_p = join_locus(l0.x, l0.y, (int32_t)l0.z, (uint64_t)l1.x | ((uint64_t)l1.y << 32), (uint64_t)l1.z | ((uint64_t)l1.w << 32), chrom_of, cp, lop, hip);
		const bool joined = has_i && has_p && ci == cp && (((p1.x >> 24) ^ a0.z) & PLACE_F_REVERSE) == 0 && loi <= hip && lop <= hii;
		bool sub;
		if (alt_sub) sub = alt_sub[q] != 0;
		else {
			const uint32_t ne = n[r];
			const uint64_t o = ne ? off[r] : 0;
			sub = hit < ne && o < log_n && hit < log_n - o && (log[(o + hit) * 3 + 1].x & 0xFFFFu) > (p1.x & 0xFFFFu);
		}
		cls[q] = (uint8_t)((joined ? JOIN_C_JOINED : 0u) | (sub ? JOIN_C_SUB : 0u));
	}
}

/* One lane per read, grid-strided: the sums of the read's class bytes (contiguous, at most 255; most reads have none) -> one 16-byte bwb_join.
 * A read without items keeps its record's counts and MAPQ; with items the MAPQ is the reference's formula on the new counts (place_mapq and
 * the table of k_place). */
__global__ __launch_bounds__(BWB_BLOCK) void k_join_reads(const uint4 *places, uint32_t n_reads, const uint64_t *alt_off, const uint8_t *cls, int max_mm, const uint8_t *qtab, uint4 *out) {
	const uint32_t stride = gridDim.x * BWB_BLOCK;
	for (uint32_t r = blockIdx.x * BWB_BLOCK + threadIdx.x; r < n_reads; r += stride) {
		const uint4 p0 = places[(size_t)r * 3], p1 = places[(size_t)r * 3 + 1];
		const uint64_t q0 = alt_off[r], q1 = alt_off[r + 1];
		uint32_t best = 0, subopt = 0;
		for (uint64_t q = q0; q < q1; q++) {
			const uint32_t c = cls[q];
			best += c == JOIN_C_JOINED;
			subopt += c == (JOIN_C_JOINED | JOIN_C_SUB);
		}
		const uint32_t top1 = p0.z - best, top2 = p0.w - subopt;
		const uint32_t mq = q1 > q0 ? place_mapq((int)top1, (int)top2, (int)(p1.y & 0xFFu), max_mm, qtab) : (p1.x >> 16) & 0xFFu;
		const bool mapped = ((p1.x >> 24) & PLACE_F_MAPPED) != 0;
		out[r] = mapped ? make_uint4(top1, top2, mq | ((best + subopt) << 8), 0u) : make_uint4(0u, 0u, 0u, 0u);
	}
}

/* ---- a placement on a bubble record in chromosome coordinates (`map -B table -R`) ----------------------------------------------------
 * The rule is in include/bwbble_hip.h (bwb_lift).  One lane per PLACEMENT, grid-strided: q < n_reads is read q's primary - its record, strand
 * and gap runs from bwb_place, its bubble and printed position from the bwb_locus record k_locus left -, n_reads + j is item j - its locus by
 * k_locus's search and rule (locus_at, as in k_join_items).  Most placements lie on no bubble record and leave after one load.  The walk
 * (lift_walk) takes the CIGAR one text position at a time - at most 8 gap runs are compared per position - twice: once for the span and the first
 * and last M that stays an M, once to emit.  k_lift_count keeps the kind byte and the record's size in 16-byte words; the scan of k_place_alt
 * turns the sizes into lift_off[]; k_lift walks the lifted placements again and writes header and ops, four ops per store. */
struct LiftBub { int64_t A, Bm, C, Dm, alt, gap; };
__device__ __forceinline__ LiftBub lift_bubble(const uint64_t *bub, int32_t b) {
	const uint64_t *q = bub + (size_t)b * 5;
	const uint64_t la = q[4];
	LiftBub v;
	v.A = (int64_t)q[0]; v.Bm = (int64_t)q[1]; v.C = (int64_t)q[2]; v.Dm = (int64_t)q[3];
	v.alt = (int64_t)(int32_t)(uint32_t)(la >> 32);
	v.gap = (int64_t)(q[2] - q[0] - q[1]);
	return v;
}
/* the op of text position t: the path byte the host's aln_path_bytes gives (a later run wins), walked as sam_put_cigar walks it */
__device__ __forceinline__ uint32_t lift_op_at(const uint4 runs, uint32_t alen, bool reverse, uint32_t t) {
	const uint32_t p = reverse ? t : alen - 1u - t;
	const uint32_t rw[4] = { runs.x, runs.y, runs.z, runs.w };
	uint32_t op = 0;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint32_t run = (rw[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
		if (run != 0xFFFFu && p - (run & 0xFFu) < ((run >> 8) & 0x7Fu)) op = (run >> 15) ? 2u : 1u;
	}
	return op;
}
__device__ __forceinline__ int lift_zone(const LiftBub &b, int64_t x) { return x <= b.Bm ? 0 : (x - b.Bm <= b.alt ? 1 : 2); }
/* the ops as they are emitted: merged with their neighbour, four to a 16-byte word (dst NULL: counted only) */
struct LiftOut {
	uint4 *dst; uint32_t cap /* 16-byte words at dst */; uint4 w; uint32_t n, kind; uint64_t len;
	__device__ __forceinline__ void put() {
		if (kind == 0xFFu) return;
		if (dst && n < 20u) {
			const uint32_t v = (uint32_t)(len << 4) | kind, c = n & 3u;
			w.x = c == 0 ? v : w.x; w.y = c == 1 ? v : w.y; w.z = c == 2 ? v : w.z; w.w = c == 3 ? v : w.w;
			if (c == 3) { if (1u + (n >> 2) < cap) dst[1 + (n >> 2)] = w; w = make_uint4(0u, 0u, 0u, 0u); }
		}
		n++;
	}
	__device__ __forceinline__ void emit(uint32_t k, uint64_t l) {
		if (k == kind && len + l < (1ull << 28)) { len += l; return; }
		put();
		kind = k; len = l;
	}
};
/* -> the number of ops, 0: not liftable; with dst the record is written there (header seqid = chrom) */
__device__ __forceinline__ uint32_t lift_walk(const LiftBub &b, int64_t pos1, bool reverse, uint32_t alen, const uint4 runs, int32_t chrom, uint4 *dst, uint32_t cap) {
	int64_t x = pos1, first = -1, last = -1, x_first = 0;
	for (uint32_t t = 0; t < alen; t++) {
		const uint32_t op = lift_op_at(runs, alen, reverse, t);
		if (op == 1u) continue;
		if (op == 0u && x >= 1 && lift_zone(b, x) != 1) { if (first < 0) { first = (int64_t)t; x_first = x; } last = (int64_t)t; }
		x++;
	}
	const int64_t end = x - 1;
	/* (pos1 < 1: the rule's own condition, as in the host's lift_resolve - locus_at gives a placement on a bubble record pos1 >= 1) */
	if (pos1 < 1 || first < 0) return 0u;
	if (end > b.Bm && end - b.Bm > b.alt && end - b.Bm - b.alt - 1 > b.Dm) return 0u;
	LiftOut o;
	o.dst = dst; o.cap = cap; o.w = make_uint4(0u, 0u, 0u, 0u); o.n = 0; o.kind = 0xFFu; o.len = 0;
	uint64_t lead = 0, trail = 0;
	x = pos1;
	for (uint32_t t = 0; t < alen; t++) {
		const uint32_t op = lift_op_at(runs, alen, reverse, t);
		uint32_t kind = 1u;
		if (op != 1u) {
			const int z = lift_zone(b, x);
			if (z == 2 && x - b.Bm == b.alt + 1 && x > pos1 && b.gap > 0 && (int64_t)t > first && (int64_t)t <= last) o.emit(2u, (uint64_t)b.gap);
			kind = op == 0u ? (z == 1 ? 1u : 0u) : (z == 1 ? 0xFFu : 2u);
			x++;
		}
		if (kind == 0xFFu) continue;
		if ((int64_t)t < first) lead += kind == 1u;
		else if ((int64_t)t > last) trail += kind == 1u;
		else {
			if ((int64_t)t == first && lead) o.emit(4u, lead);
			o.emit(kind, 1);
		}
	}
	o.put();
	if (trail) { o.kind = 4u; o.len = trail; o.put(); }
	if (o.n > 20u) return 0u; /* (17 runs and the three the allele adds: not reached) */
	if (dst) {
		if ((o.n & 3u) && 1u + (o.n >> 2) < cap) dst[1 + (o.n >> 2)] = o.w;
		const uint64_t pos = x_first <= b.Bm ? (uint64_t)b.A + (uint64_t)x_first - 1u : (uint64_t)b.C + (uint64_t)(x_first - (b.Bm + b.alt + 1));
		dst[0] = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), (uint32_t)chrom, o.n);
	}
	return o.n;
}
/* placement q: its bubble (-1: none), printed position, strand, path length and gap runs */
struct LiftPlacement { int32_t b; int64_t pos1; bool reverse; uint32_t alen; uint4 runs; };
__device__ __forceinline__ LiftPlacement lift_placement(uint64_t q, const uint4 *places, uint32_t n_reads, const uint4 *loci, const uint4 *alts, const uint64_t *start, const uint64_t *end,
                                                        const int32_t *bubble_of, uint32_t n_seq, uint32_t trips, const uint64_t *bub) {
	LiftPlacement v;
	if (q < n_reads) {
		const uint4 l0 = loci[q * 2];
		v.b = l0.x != 0xFFFFFFFFu ? (int32_t)l0.z : -1;
		v.pos1 = (int64_t)(int32_t)l0.y;
		if (v.b >= 0) {
			const uint4 p1 = places[q * 3 + 1];
			v.reverse = ((p1.x >> 24) & PLACE_F_REVERSE) != 0;
			v.alen = p1.z & 0xFFFFu;
			v.runs = places[q * 3 + 2];
		}
	} else {
		const uint64_t j = q - n_reads;
		const uint4 a0 = alts[j * 2];
		const Locus il = locus_at((uint64_t)a0.x | ((uint64_t)a0.y << 32), (a0.z & PLACE_F_MAPPED) != 0, start, end, bubble_of, n_seq, trips, bub);
		v.b = il.seqid != 0xFFFFFFFFu ? il.b : -1;
		v.pos1 = (int64_t)(int32_t)il.pos1;
		v.reverse = (a0.z & PLACE_F_REVERSE) != 0;
		v.alen = a0.w >> 16;
		if (v.b >= 0) v.runs = alts[j * 2 + 1];
	}
	return v;
}
__global__ __launch_bounds__(BWB_BLOCK) void k_lift_count(const uint4 *places, uint32_t n_reads, const uint4 *loci, const uint4 *alts, uint64_t n_q, const uint64_t *start, const uint64_t *end,
                                                           const int32_t *bubble_of, uint32_t n_seq, uint32_t trips, const uint64_t *bub, uint8_t *kind, uint32_t *words) {
	const uint64_t stride = (uint64_t)gridDim.x * BWB_BLOCK;
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_q; q += stride) {
		const LiftPlacement v = lift_placement(q, places, n_reads, loci, alts, start, end, bubble_of, n_seq, trips, bub);
		uint32_t k = 0, wn = 0;
		if (v.b >= 0) {
			const uint32_t n_ops = lift_walk(lift_bubble(bub, v.b), v.pos1, v.reverse, v.alen, v.runs, 0, nullptr, 0u);
			k = n_ops ? 1u : 2u;
			wn = n_ops ? 1u + ((n_ops + 3u) >> 2) : 0u;
		}
		kind[q] = (uint8_t)k;
		words[q] = wn;
	}
}
__global__ __launch_bounds__(BWB_BLOCK) void k_lift(const uint4 *places, uint32_t n_reads, const uint4 *loci, const uint4 *alts, uint64_t n_q, const uint64_t *start, const uint64_t *end,
                                                     const int32_t *bubble_of, uint32_t n_seq, uint32_t trips, const uint64_t *bub, const int32_t *chrom_of, const uint8_t *kind,
                                                     const uint64_t *lift_off, uint4 *out) {
	const uint64_t stride = (uint64_t)gridDim.x * BWB_BLOCK;
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_q; q += stride) {
		if (kind[q] != 1u) continue;
		const LiftPlacement v = lift_placement(q, places, n_reads, loci, alts, start, end, bubble_of, n_seq, trips, bub);
		if (v.b < 0) continue;
		const uint64_t o = lift_off[q];
		const uint64_t cap = lift_off[q + 1] - o; /* (k_lift_count sized it from the same walk; nothing is stored beyond it) */
		if (cap < 2u || cap > 6u) continue;
		lift_walk(lift_bubble(bub, v.b), v.pos1, v.reverse, v.alen, v.runs, chrom_of[v.b], out + o, (uint32_t)cap);
	}
}

/* ---- NM:i and MD:Z of a read's line against the text (`map -D`) ---------------------------------------------------------------------
 * The rule is in include/bwbble_hip.h (bwb_md).  The text lies in device memory at 4 bits per character: character i is nibble i & 7 of the
 * 32-bit word i >> 3, so that an aligned 16-byte word holds 32 characters.  k_text_pack makes that of a staged chunk of one-byte codes: one
 * lane per 16-byte word, the 32 codes by two 16-byte loads (the last word of the text, which may hold fewer, byte by byte; what lies beyond
 * the text is 0); a code above 15 sets *bad. */
__device__ __forceinline__ uint32_t text_pack4(uint32_t v) { return (v & 0xFu) | ((v >> 4) & 0xF0u) | ((v >> 8) & 0xF00u) | ((v >> 12) & 0xF000u); }
__global__ __launch_bounds__(BWB_BLOCK) void k_text_pack(const uint8_t *codes /* 16-byte aligned */, uint64_t n_chunk, uint4 *packed, uint32_t *bad) {
	const uint64_t stride = (uint64_t)gridDim.x * BWB_BLOCK, n_words = (n_chunk + 31u) >> 5;
	for (uint64_t w = (uint64_t)blockIdx.x * BWB_BLOCK + threadIdx.x; w < n_words; w += stride) {
		uint32_t src[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
		if (w * 32u + 32u <= n_chunk) {
			const uint4 a = ((const uint4 *)codes)[w * 2u], b = ((const uint4 *)codes)[w * 2u + 1u];
			src[0] = a.x; src[1] = a.y; src[2] = a.z; src[3] = a.w; src[4] = b.x; src[5] = b.y; src[6] = b.z; src[7] = b.w;
		} else
			for (uint64_t i = w * 32u; i < n_chunk; i++) src[(i & 31u) >> 2] |= (uint32_t)codes[i] << ((i & 3u) * 8u);
		uint32_t over = 0;
#pragma unroll
		for (int k = 0; k < 8; k++) over |= src[k] & 0xF0F0F0F0u;
		if (over) atomicOr(bad, 1u);
		packed[w] = make_uint4(text_pack4(src[0]) | (text_pack4(src[1]) << 16), text_pack4(src[2]) | (text_pack4(src[3]) << 16),
		                       text_pack4(src[4]) | (text_pack4(src[5]) << 16), text_pack4(src[6]) | (text_pack4(src[7]) << 16));
	}
}

/* One lane per READ, grid-strided.  A lane walks its read's ops - the printed CIGAR of its placement one path position at a time (lift_op_at, as
 * k_lift walks it), or the ops of its lift record - with the read base from the slot's resident reads and the text's code from the 16-byte word
 * the lane holds in registers: a read of 100 bases loads four or five of them.  k_md_count walks for the kind, NM and the exact length of the MD
 * text; the scan of k_place_alt turns the lengths into md_off[]; k_md walks the reads of kind BWB_MD_OK again and stores the bytes.  Every text
 * position fetched lies in [0, n_fwd) - k_md_count has checked the span before either kernel walks -, every read base in [0, len), and k_md
 * stores nothing beyond the length k_md_count left. */
#define MD_NONE 0u
#define MD_OK 1u
#define MD_TOO_LONG 2u
#define MD_MAX_SPAN 4096u
/* eight letters as the bytes of one 64-bit constant, the first lowest: a register, not a table in memory */
__host__ __device__ constexpr uint64_t md_letters8(const char (&s)[9]) {
	return (uint64_t)(uint8_t)s[0] | (uint64_t)(uint8_t)s[1] << 8 | (uint64_t)(uint8_t)s[2] << 16 | (uint64_t)(uint8_t)s[3] << 24 | (uint64_t)(uint8_t)s[4] << 32 |
	       (uint64_t)(uint8_t)s[5] << 40 | (uint64_t)(uint8_t)s[6] << 48 | (uint64_t)(uint8_t)s[7] << 56;
}
static_assert((md_letters8("NTKGSBYC") & 0xFF) == 'N' && (md_letters8("MHNVRDWA") >> 16 & 0xFF) == 'N' && (md_letters8("MHNVRDWA") >> 56) == 'A', "code 0 prints N, code 10 N, code 15 A");
struct MdWalk {
	const uint4 *text; uint64_t cur; uint4 w;             /* the packed text and the word held */
	const uint8_t *seq; uint32_t len; bool reverse;       /* the read as uploaded */
	char *dst; uint32_t cap, n;                           /* the MD text (dst NULL: counted only) */
	uint32_t ri, run, mm, gaps; uint64_t tp; bool in_del;
	__device__ __forceinline__ uint32_t code() {
		const uint64_t wi = tp >> 5;
		if (wi != cur) { w = text[wi]; cur = wi; }
		const uint32_t k = (uint32_t)tp & 31u;
		const uint64_t lo = (uint64_t)w.x | ((uint64_t)w.y << 32), hi = (uint64_t)w.z | ((uint64_t)w.w << 32); /* (two shifts and a select: a component chosen by index goes through scratch) */
		tp++;
		return (uint32_t)((k < 16u ? lo : hi) >> ((k & 15u) * 4u)) & 15u;
	}
	__device__ __forceinline__ uint32_t base() { /* SEQ as SAM prints it: read->rc on the reverse strand */
		const uint32_t c = reverse ? seq[len - 1u - ri] : seq[ri];
		ri++;
		return reverse ? (c > 3u ? 4u : 3u - c) : c;
	}
	__device__ __forceinline__ void put(uint32_t ch) { if (dst && n < cap) dst[n] = (char)ch; n++; }
	__device__ __forceinline__ void letter(uint32_t c) { /* "NTKGSBYCMHNVRDWA"[c] */
		put((uint32_t)((c < 8u ? md_letters8("NTKGSBYC") : md_letters8("MHNVRDWA")) >> ((c & 7u) * 8u)) & 0xFFu);
	}
	__device__ __forceinline__ void number(uint32_t v) {
		if (v >= 10000u) put('0' + v / 10000u % 10u);
		if (v >= 1000u) put('0' + v / 1000u % 10u);
		if (v >= 100u) put('0' + v / 100u % 10u);
		if (v >= 10u) put('0' + v / 10u % 10u);
		put('0' + v % 10u);
	}
	__device__ __forceinline__ void step(uint32_t op, uint32_t count) { /* op: 0 M, 1 I, 2 D, 4 S */
		if (op == 0u) {
			for (uint32_t k = 0; k < count; k++) {
				const uint32_t b = base(), c = code();
				if (b < 4u && ((member_mask((int)b) >> c) & 1u)) run++;
				else { number(run); letter(c); run = 0; mm++; }
			}
		} else if (op == 2u) {
			if (!in_del) { number(run); put('^'); run = 0; }
			for (uint32_t k = 0; k < count; k++) letter(code());
			gaps += count;
		} else {
			ri += count;
			if (op == 1u) gaps += count;
		}
		in_del = op == 2u;
	}
};
/* read q's ops: kind 1 with a record (hdr: pos, seqid, n_ops; its ops in the words behind) or the placement's own */
struct MdRead { bool mapped, reverse, lifted; uint32_t alen, n_ops; uint4 runs; const uint4 *rec; int64_t start; };
__device__ __forceinline__ MdRead md_read(uint32_t q, const uint4 *places, const uint8_t *lift_kind, const uint64_t *lift_off, const uint4 *lift_recs, const uint64_t *lstart, uint32_t n_seq) {
	MdRead v;
	const uint4 p0 = places[(size_t)q * 3], p1 = places[(size_t)q * 3 + 1];
	v.mapped = ((p1.x >> 24) & PLACE_F_MAPPED) != 0;
	v.reverse = ((p1.x >> 24) & PLACE_F_REVERSE) != 0;
	v.alen = p1.z & 0xFFFFu;
	v.runs = places[(size_t)q * 3 + 2];
	v.start = (int64_t)((uint64_t)p0.x | ((uint64_t)p0.y << 32));
	v.lifted = lift_kind && lift_kind[q] == 1u;
	v.n_ops = 0; v.rec = nullptr;
	if (v.lifted) {
		const uint64_t o = lift_off[q], words = lift_off[q + 1] - o;
		const uint4 hdr = words ? lift_recs[o] : make_uint4(0u, 0u, 0xFFFFFFFFu, 0xFFu);
		const uint32_t n_ops = hdr.w & 0xFFu;
		/* (a record that does not fit its own words, or names no record of the table: walked by nobody) */
		if (n_ops < 1u || n_ops > 20u || 1u + ((n_ops + 3u) >> 2) > words || hdr.z >= n_seq) v.mapped = false;
		else {
			v.n_ops = n_ops; v.rec = lift_recs + o;
			v.start = (int64_t)(lstart[hdr.z] + ((uint64_t)hdr.x | ((uint64_t)hdr.y << 32)) - 1u);
		}
	}
	return v;
}
__device__ __forceinline__ uint32_t md_rec_op(const uint4 *rec, uint32_t i) {
	return ((const uint32_t *)(rec + 1))[i];
}
/* the read's ops in order, f(op, count): the words of its lift record, or its printed CIGAR one text position at a time */
template <typename F> __device__ __forceinline__ void md_ops(const MdRead &v, F &&f) {
	if (v.lifted) for (uint32_t i = 0; i < v.n_ops; i++) { const uint32_t op = md_rec_op(v.rec, i); f(op & 15u, op >> 4); }
	else for (uint32_t t = 0; t < v.alen; t++) f(lift_op_at(v.runs, v.alen, v.reverse, t), 1u);
}
/* the walker's step (MdWalk, PileWalk<Q>) over the read's ops */
template <typename W> __device__ __forceinline__ void md_walk(W &m, const MdRead &v) {
	md_ops(v, [&](uint32_t op, uint32_t count) { m.step(op, count); });
}
/* May read v be walked?  The gate of every kernel that walks (k_md_count writes the kind, k_md walks the reads it left MD_OK, the pile kernels
 * count exactly those): a mapped read of at most 255 bases that fits the slot's stride, whose ops - the span on the text and the read bases they
 * consume - stay within MD_MAX_SPAN, within [0, n_fwd) from the start, and consume the read exactly.  Nothing of the text or the read is fetched
 * here; a read that is not MD_OK has none of either fetched by anybody. */
__device__ __forceinline__ uint32_t md_gate(const MdRead &v, uint32_t len, uint32_t stride, uint64_t n_fwd) {
	if (!(v.mapped && len <= 255u && len <= stride)) return MD_NONE;
	uint64_t span = 0, on_read = 0;
	md_ops(v, [&](uint32_t op, uint32_t count) { if (op == 0u || op == 2u) span += count; if (op != 2u) on_read += count; });
	/* (the kind as two selects, not a return per kind: that form cost the pile kernels registers) */
	const bool fits = v.start >= 0 && (uint64_t)v.start <= n_fwd && span <= n_fwd - (uint64_t)v.start && on_read == len;
	return span > MD_MAX_SPAN ? MD_TOO_LONG : fits ? MD_OK : MD_NONE;
}
__device__ __forceinline__ MdWalk md_begin(const uint4 *text, const uint8_t *seq, uint32_t len, const MdRead &v, char *dst, uint32_t cap) {
	MdWalk m;
	m.text = text; m.cur = ~0ull; m.w = make_uint4(0u, 0u, 0u, 0u);
	m.seq = seq; m.len = len; m.reverse = v.reverse;
	m.dst = dst; m.cap = cap; m.n = 0;
	m.ri = 0; m.run = 0; m.mm = 0; m.gaps = 0; m.tp = (uint64_t)v.start; m.in_del = false;
	return m;
}
__global__ __launch_bounds__(BWB_BLOCK) void k_md_count(const uint8_t *reads, const uint16_t *lens, uint32_t stride, const uint4 *places, uint32_t n_reads, const uint8_t *lift_kind,
                                                         const uint64_t *lift_off, const uint4 *lift_recs, const uint64_t *lstart, uint32_t n_seq, const uint4 *text, uint64_t n_fwd,
                                                         uint2 *recs, uint32_t *md_len) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	for (uint32_t q = blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_reads; q += gstride) {
		const MdRead v = md_read(q, places, lift_kind, lift_off, lift_recs, lstart, n_seq);
		const uint32_t len = lens[q];
		const uint32_t kind = md_gate(v, len, stride, n_fwd);
		uint32_t nm = 0, bytes = 0;
		if (kind == MD_OK) {
			MdWalk m = md_begin(text, reads + (size_t)q * stride, len, v, nullptr, 0u);
			md_walk(m, v);
			m.number(m.run);
			nm = m.mm + m.gaps; bytes = m.n;
		}
		recs[q] = make_uint2(nm, bytes | (kind << 16));
		md_len[q] = bytes;
	}
}
__global__ __launch_bounds__(BWB_BLOCK) void k_md(const uint8_t *reads, const uint16_t *lens, uint32_t stride, const uint4 *places, uint32_t n_reads, const uint8_t *lift_kind,
                                                   const uint64_t *lift_off, const uint4 *lift_recs, const uint64_t *lstart, uint32_t n_seq, const uint4 *text, const uint2 *recs,
                                                   const uint64_t *md_off, char *out) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	for (uint32_t q = blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_reads; q += gstride) {
		if (((recs[q].y >> 16) & 0xFFu) != MD_OK) continue;
		const MdRead v = md_read(q, places, lift_kind, lift_off, lift_recs, lstart, n_seq);
		const uint64_t o = md_off[q], cap = md_off[q + 1] - o; /* (k_md_count sized it from the same walk; nothing is stored beyond it) */
		if (!v.mapped || cap > 0xFFFFu) continue;
		MdWalk m = md_begin(text, reads + (size_t)q * stride, lens[q], v, out + o, (uint32_t)cap);
		md_walk(m, v);
		m.number(m.run);
	}
}

/* ---- allele counts at the text's IUPAC sites (`map -A`) -----------------------------------------------------------------------------
 * The rule is in include/bwbble_hip.h (bwb_hip_pile_begin).  A SITE is a text position whose code has two or three members; sites are numbered
 * in text order.  The rank structure over them is one uint32 per 16-byte word of the packed text: site_base[w] = the sites below character
 * 32 w, so that position i is site site_base[i >> 5] + popcount(site mask of its word & the bits below i & 31).
 * k_site_count: one lane per 16-byte word - its 32-bit site mask, the popcount, the block's exclusive scan (the scheme of k_scan_blocks, fused
 * behind the popcount so that no count array exists) into site_base[] and the block's sum into bsum[]; k_scan_sums turns bsum[] into the blocks'
 * offsets and the 64-bit total; k_site_add adds them.  What lies behind the text in its last word is code 0, no site. */
#define PILE_SITE_CODES 0x7B74u /* bit c: code c is K 2, S 4, B 5, Y 6, M 8, H 9, V 11, R 12, D 13 or W 14 */
static_assert(PILE_SITE_CODES == (1u << 2 | 1u << 4 | 1u << 5 | 1u << 6 | 1u << 8 | 1u << 9 | 1u << 11 | 1u << 12 | 1u << 13 | 1u << 14), "the ten codes with two or three members");
__device__ __forceinline__ uint32_t site_mask8(uint32_t x) { /* bit k: nibble k of x is a site's code */
	uint32_t m = 0;
#pragma unroll
	for (int k = 0; k < 8; k++) m |= ((PILE_SITE_CODES >> ((x >> (4 * k)) & 15u)) & 1u) << k;
	return m;
}
__device__ __forceinline__ uint32_t site_mask32(const uint4 w) { return site_mask8(w.x) | (site_mask8(w.y) << 8) | (site_mask8(w.z) << 16) | (site_mask8(w.w) << 24); }
__global__ __launch_bounds__(BWB_BLOCK) void k_site_count(const uint4 *text, uint32_t n_words, uint32_t *site_base, uint64_t *bsum) {
	__shared__ uint32_t s_wave[BWB_BLOCK / 64];
	const uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint32_t v = i < n_words ? (uint32_t)__popc(site_mask32(text[i])) : 0u;
	uint32_t inc = v; /* (a block's sum is at most 256 * 32) */
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d); if (lane >= d) inc += t; }
	if (lane == 63) s_wave[wv] = inc;
	__syncthreads();
	uint32_t before = 0, total = 0;
#pragma unroll
	for (int k = 0; k < BWB_BLOCK / 64; k++) { if (k < wv) before += s_wave[k]; total += s_wave[k]; }
	if (i < n_words) site_base[i] = before + inc - v;
	if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
/* (the caller has refused a total above 2^32 - 1 before this runs: no sum wraps) */
__global__ __launch_bounds__(BWB_BLOCK) void k_site_add(uint32_t *site_base, uint32_t n_words, const uint64_t *bsum) {
	const uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x;
	if (i < n_words) site_base[i] += (uint32_t)bsum[blockIdx.x];
}
/* test entry: the site number of every queried text position (< n_fwd, checked by the caller), or -1 */
__global__ __launch_bounds__(BWB_BLOCK) void k_site_of(const uint4 *text, const uint32_t *site_base, const uint64_t *pos, uint64_t n, int64_t *site) {
	const uint64_t stride = (uint64_t)gridDim.x * BWB_BLOCK;
	for (uint64_t q = (uint64_t)blockIdx.x * BWB_BLOCK + threadIdx.x; q < n; q += stride) {
		const uint64_t wi = pos[q] >> 5;
		const uint32_t k = (uint32_t)pos[q] & 31u, mask = site_mask32(text[wi]);
		site[q] = (mask >> k) & 1u ? (int64_t)((uint64_t)site_base[wi] + (uint32_t)__popc(mask & ((1u << k) - 1u))) : -1;
	}
}

/* The block's sums of N per-lane figures, added to stats[0 .. N) once per block: shuffles over the wave's 64 lanes, the waves' sums through LDS
 * (N * BWB_BLOCK / 64 * 8 bytes), then thread 0 adds what is not zero.  EVERY thread of the block must get here - there is a barrier inside -,
 * so the callers' loops have no barrier, return or break past it: they fall through to this call. */
template <int N> __device__ __forceinline__ void block_sums_to(unsigned long long (&mine)[N], unsigned long long *stats) {
	__shared__ unsigned long long s_sum[N][BWB_BLOCK / 64];
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
		for (int k = 0; k < N; k++) mine[k] += __shfl_down(mine[k], d);
	}
	if ((threadIdx.x & 63) == 0) {
#pragma unroll
		for (int k = 0; k < N; k++) s_sum[k][threadIdx.x >> 6] = mine[k];
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long sum[N];
#pragma unroll
		for (int k = 0; k < N; k++) sum[k] = 0;
#pragma unroll
		for (int i = 0; i < BWB_BLOCK / 64; i++) {
#pragma unroll
			for (int k = 0; k < N; k++) sum[k] += s_sum[k][i];
		}
#pragma unroll
		for (int k = 0; k < N; k++) if (sum[k]) atomicAdd(stats + k, sum[k]);
	}
}

/* k_pile, k_pile_q: one lane per READ, grid-strided; the walk of k_md_count - md_read, md_gate, the same ops from the same start, the text in
 * 16-byte words held in registers - with one add where k_md compares: for every M base that lies on a site and is A, C, G or T,
 * counts[site * 4 + column] += 1, the columns A, C, G, T by the letter SAM prints.  The site mask is computed once per word held; site_base[] is
 * loaded only when a base falls on a site, and the read base only then.  A read counts when its kind is BWB_MD_OK (md_gate) and its MAPQ - the
 * placement's, or mapq[q * mapq_stride] (the join record's, or the caller's override) - is at least min_mapq; the MAPQ is tested ahead of the
 * gate, so a filtered read costs no op decoding.  The adds are relaxed, agent-scope atomics to scattered counters (a site sees about as many
 * adds per run as the coverage: no aggregation ahead of them); the reads counted and the adds made go to stats[0] / stats[1] once per block
 * (block_sums_to).  Every text position fetched lies in [0, n_fwd), every read base in [0, len), every site number below n_sites (the index was
 * built from this text).
 * Q, k_pile_q (`map -b / -Y`): with the base qualities - the rule is in include/bwbble_hip.h (bwb_hip_pileq_begin).  quals holds one byte per
 * base in FASTQ order, strided like the reads, and a base's byte is the one at the read base's own index (len - 1 - ri on the reverse strand),
 * loaded only when the base falls on a site and is no N.  Q = 0 below '!', else min(byte - 33, 93).  A base with Q < min_baseq is dropped: no
 * add, counted in `dropped`, which goes to stats[2].  err_cap != 0 (4..93, then qsum is a table like counts): the base also adds
 * min(max(Q, 4), err_cap) to qsum at the counter's index, the same kind of atomic.  Q is a template argument and the two kernels two entry
 * points, not a flag read at run time: k_pile keeps its registers (69 VGPRs, 7 waves per SIMD; k_pile_q 74 and 6). */
#define PILEQ_MAX_Q 93u
#define PILEQ_MIN_W 4u
template <bool Q> struct PileWalk {
	const uint4 *text; uint64_t cur; uint4 w; uint32_t mask;  /* the packed text, the word held and its site mask */
	const uint32_t *site_base; uint32_t *counts, *qsum;
	const uint8_t *seq, *qual; uint32_t len; bool reverse;
	uint32_t min_baseq, err_cap;                              /* (qsum, qual and these two: Q only) */
	uint32_t ri, adds, dropped; uint64_t tp;
	__device__ __forceinline__ void step(uint32_t op, uint32_t count) { /* op: 0 M, 1 I, 2 D, 4 S */
		if (op == 0u) {
			for (uint32_t k = 0; k < count; k++, ri++, tp++) {
				const uint64_t wi = tp >> 5;
				if (wi != cur) { w = text[wi]; cur = wi; mask = site_mask32(w); }
				const uint32_t at = (uint32_t)tp & 31u;
				if (!((mask >> at) & 1u)) continue;
				const uint32_t idx = reverse ? len - 1u - ri : ri;
				const uint32_t c = seq[idx];
				if (c > 3u) continue; /* a read N */
				uint32_t qv = 0;
				if constexpr (Q) {
					const uint32_t qc = qual[idx];
					qv = qc < 33u ? 0u : (qc - 33u > PILEQ_MAX_Q ? PILEQ_MAX_Q : qc - 33u);
					if (qv < min_baseq) { dropped++; continue; }
				}
				const uint32_t b = reverse ? 3u - c : c; /* A0 G1 C2 T3 as printed */
				const uint32_t col = (b == 1u || b == 2u) ? 3u - b : b; /* A C G T */
				const uint64_t site = (uint64_t)site_base[wi] + (uint32_t)__popc(mask & ((1u << at) - 1u));
				__hip_atomic_fetch_add(counts + site * 4u + col, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if constexpr (Q) {
					if (err_cap) {
						const uint32_t lo = qv < PILEQ_MIN_W ? PILEQ_MIN_W : qv;
						__hip_atomic_fetch_add(qsum + site * 4u + col, lo > err_cap ? err_cap : lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					}
				}
				adds++;
			}
		} else if (op == 2u) tp += count;
		else ri += count;
	}
};
template <bool Q> __device__ __forceinline__ void pile_body(const uint8_t *reads, const uint8_t *quals, const uint16_t *lens, uint32_t stride, const uint4 *places, uint32_t n_reads,
                                                            const uint8_t *lift_kind, const uint64_t *lift_off, const uint4 *lift_recs, const uint64_t *lstart, uint32_t n_seq,
                                                            const uint4 *text, uint64_t n_fwd, const uint8_t *mapq, uint32_t mapq_stride, uint32_t min_mapq, uint32_t min_baseq,
                                                            uint32_t err_cap, const uint32_t *site_base, uint32_t *counts, uint32_t *qsum, unsigned long long *stats) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	unsigned long long mine[Q ? 3 : 2] = {}; /* reads, adds, and with Q the bases dropped */
	for (uint32_t q = blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_reads; q += gstride) {
		const MdRead v = md_read(q, places, lift_kind, lift_off, lift_recs, lstart, n_seq);
		const uint32_t mq = mapq ? mapq[(size_t)q * mapq_stride] : (places[(size_t)q * 3 + 1].x >> 16) & 0xFFu;
		if (mq < min_mapq) continue;
		const uint32_t len = lens[q];
		if (md_gate(v, len, stride, n_fwd) != MD_OK) continue;
		PileWalk<Q> m;
		m.text = text; m.cur = ~0ull; m.w = make_uint4(0u, 0u, 0u, 0u); m.mask = 0u;
		m.site_base = site_base; m.counts = counts; m.qsum = qsum;
		m.seq = reads + (size_t)q * stride; m.qual = Q ? quals + (size_t)q * stride : nullptr; m.len = len; m.reverse = v.reverse;
		m.min_baseq = min_baseq; m.err_cap = err_cap;
		m.ri = 0; m.adds = 0; m.dropped = 0; m.tp = (uint64_t)v.start;
		md_walk(m, v);
		mine[0]++; mine[1] += m.adds;
		if constexpr (Q) mine[2] += m.dropped;
	}
	block_sums_to(mine, stats);
}
__global__ __launch_bounds__(BWB_BLOCK) void k_pile(const uint8_t *reads, const uint16_t *lens, uint32_t stride, const uint4 *places, uint32_t n_reads, const uint8_t *lift_kind,
                                                     const uint64_t *lift_off, const uint4 *lift_recs, const uint64_t *lstart, uint32_t n_seq, const uint4 *text, uint64_t n_fwd,
                                                     const uint8_t *mapq, uint32_t mapq_stride, uint32_t min_mapq, const uint32_t *site_base, uint32_t *counts,
                                                     unsigned long long *stats) {
	pile_body<false>(reads, nullptr, lens, stride, places, n_reads, lift_kind, lift_off, lift_recs, lstart, n_seq, text, n_fwd, mapq, mapq_stride, min_mapq, 0u, 0u, site_base, counts, nullptr,
	                 stats);
}
__global__ __launch_bounds__(BWB_BLOCK) void k_pile_q(const uint8_t *reads, const uint8_t *quals, const uint16_t *lens, uint32_t stride, const uint4 *places, uint32_t n_reads,
                                                       const uint8_t *lift_kind, const uint64_t *lift_off, const uint4 *lift_recs, const uint64_t *lstart, uint32_t n_seq,
                                                       const uint4 *text, uint64_t n_fwd, const uint8_t *mapq, uint32_t mapq_stride, uint32_t min_mapq, uint32_t min_baseq,
                                                       uint32_t err_cap, const uint32_t *site_base, uint32_t *counts, uint32_t *qsum, unsigned long long *stats) {
	pile_body<true>(reads, quals, lens, stride, places, n_reads, lift_kind, lift_off, lift_recs, lstart, n_seq, text, n_fwd, mapq, mapq_stride, min_mapq, min_baseq, err_cap, site_base, counts,
	                qsum, stats);
}

/* ---- ref / alt read support per indel bubble (`map -I`) --------------------------------------------------------------------------------
 * The rule is in include/bwbble_hip.h (bwb_hip_indel_begin).  k_indel: one lane per READ, grid-strided, over the placement records of k_place
 * and the locus records of k_locus.  A read's printed CIGAR is walked one text position at a time (lift_op_at: at most 8 gap runs compared per
 * position), once for the bases it consumes and its first and last M, then once per window it is classed against - that walk ends at the
 * window's hi.  A read on bubble b's record has one window (elig[b] says whether b is eligible).  A read on a chromosome record c bisects
 * tab[] - the eligible bubbles ascending by (c, lo, bubble), one 16-byte word lo | c | bubble each - for the first entry not below (c, its first
 * M), `trips` steps for every lane (2^trips > n_tab, a kernel argument: selects, no divergent while), and walks on while the entry's c is its
 * own and lo does not exceed its last M: the loop is bounded by the table alone.  An entry whose hi = C + w - 1 (from bub[]) lies behind the
 * last M is skipped.  The adds are relaxed, agent-scope atomics into counts[bubble * 4 + ref 0 | alt 1 | ref_gapped 2 | alt_gapped 3]; reads
 * counted, adds made and candidates examined go to stats[0..2] once per block (block_sums_to).  Every index is bounded: tab[] below n_tab, a
 * locus record's bubble below the table's size (bwb_hip_set_loci checked bubble_of), an entry's bubble likewise. */
struct IndelRead { int64_t pos1; bool reverse; uint32_t alen; uint4 runs; };
/* 0 not covering, 1 clean, 2 gapped (lo < hi: a window is at least two positions wide) */
__device__ __forceinline__ uint32_t indel_class(const IndelRead &v, int64_t lo, int64_t hi) {
	int64_t x = v.pos1;
	bool at_lo = false, at_hi = false, dirty = false;
	for (uint32_t t = 0; t < v.alen && x <= hi; t++) {
		const uint32_t op = lift_op_at(v.runs, v.alen, v.reverse, t);
		if (op == 1u) { dirty = dirty || at_lo; continue; } /* (the M at hi ends the walk: an I behind it is not seen) */
		if (x >= lo) {
			if (op == 0u) { at_lo = at_lo || x == lo; at_hi = at_hi || x == hi; }
			else dirty = true;
		}
		x++;
	}
	return at_lo && at_hi ? (dirty ? 2u : 1u) : 0u;
}
__global__ __launch_bounds__(BWB_BLOCK) void k_indel(const uint4 *places, const uint4 *loci, uint32_t n_reads, const uint16_t *lens, const uint8_t *mapq, uint32_t mapq_stride,
                                                      uint32_t min_mapq, const uint64_t *bub, const uint8_t *elig, uint32_t anchor, const uint4 *tab, uint32_t n_tab, uint32_t trips,
                                                      uint32_t *counts, unsigned long long *stats) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	unsigned long long my_reads = 0, my_adds = 0, my_cand = 0;
	for (uint32_t q = blockIdx.x * BWB_BLOCK + threadIdx.x; q < n_reads; q += gstride) {
		const uint4 p1 = places[(size_t)q * 3 + 1], l0 = loci[(size_t)q * 2];
		if (!((p1.x >> 24) & PLACE_F_MAPPED) || l0.x == 0xFFFFFFFFu) continue;
		const uint32_t mq = mapq ? mapq[(size_t)q * mapq_stride] : (p1.x >> 16) & 0xFFu;
		if (mq < min_mapq) continue;
		IndelRead v;
		v.pos1 = (int64_t)(int32_t)l0.y; v.reverse = ((p1.x >> 24) & PLACE_F_REVERSE) != 0; v.alen = p1.z & 0xFFFFu; v.runs = places[(size_t)q * 3 + 2];
		int64_t x = v.pos1, xf = 0, xl = -1;
		uint32_t on_read = 0;
		bool any = false;
		for (uint32_t t = 0; t < v.alen; t++) {
			const uint32_t op = lift_op_at(v.runs, v.alen, v.reverse, t);
			on_read += op != 2u;
			if (op == 1u) continue;
			if (op == 0u) { xf = any ? xf : x; any = true; xl = x; }
			x++;
		}
		if (lens && on_read != lens[q]) continue;
		my_reads++;
		const int32_t b = (int32_t)l0.z;
		if (b >= 0) {
			if (!elig[b]) continue;
			const uint64_t *e = bub + (size_t)b * 5;
			const int64_t Bm = (int64_t)e[1], alt = (int64_t)(int32_t)(uint32_t)(e[4] >> 32);
			my_cand++;
			const uint32_t cls = indel_class(v, Bm - (int64_t)anchor + 1, Bm + alt + (int64_t)anchor);
			if (cls) { __hip_atomic_fetch_add(counts + (size_t)b * 4 + (cls == 1u ? 1u : 3u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); my_adds++; }
			continue;
		}
		if (!any) continue;
		const int32_t c = (int32_t)l0.x;
		uint32_t at = 0; /* the entries below (c, xf) */
		for (uint32_t t = trips; t-- > 0;) {
			const uint32_t s = 1u << t;
			bool below = false;
			if (s <= n_tab - at) { /* (at <= n_tab throughout) */
				const uint4 k = tab[at + s - 1u];
				const int64_t klo = (int64_t)((uint64_t)k.x | ((uint64_t)k.y << 32));
				below = (int32_t)k.z < c || ((int32_t)k.z == c && klo < xf);
			}
			at = below ? at + s : at;
		}
		for (; at < n_tab; at++) {
			const uint4 k = tab[at];
			const int64_t klo = (int64_t)((uint64_t)k.x | ((uint64_t)k.y << 32));
			if ((int32_t)k.z != c || klo > xl) break;
			my_cand++;
			const int64_t khi = (int64_t)(bub[(size_t)k.w * 5 + 2] + (uint64_t)anchor - 1u);
			if (khi > xl) continue;
			const uint32_t cls = indel_class(v, klo, khi);
			if (cls) { __hip_atomic_fetch_add(counts + (size_t)k.w * 4 + (cls == 1u ? 0u : 2u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); my_adds++; }
		}
	}
	unsigned long long mine[3] = { my_reads, my_adds, my_cand };
	block_sums_to(mine, stats); /* (every thread of the block gets here: the loop has no barrier inside) */
}

/* ---- genotype calls at IUPAC sites and indel bubbles (`map -G`) ---------------------------------------------------------------------------
 * The rule is in include/bwbble_hip.h (bwb_hip_geno_begin); all of it is integer arithmetic.  geno_rule: the raw costs of the 3 (k == 2) or 6
 * genotypes in VCF order from the allele counts n0, n1, n2 and the depth, the first smallest, GQ and the saturated PLs.  Every array index is a
 * constant after unrolling: the costs live in registers, nothing in scratch. */
#define GENO_HET 3u /* the cost of a base under a heterozygous genotype that carries it: 10 log10 2, rounded */
#define GENO_MEMBERS 0x09D570B30AE60C00ull /* nibble c: the members of code c as columns, bit 0 A, 1 C, 2 G, 3 T (0: no site) */
static_assert(((GENO_MEMBERS >> 8) & 15u) == 12u && ((GENO_MEMBERS >> 32) & 15u) == 3u && ((GENO_MEMBERS >> 56) & 15u) == 9u, "K is G, T; M is A, C; W is A, T");
struct GenoCall { uint32_t gt, gq; uint32_t pl[6]; };
__device__ __forceinline__ GenoCall geno_rule(uint64_t n0, uint64_t n1, uint64_t n2, uint32_t k, uint64_t depth, uint64_t err) {
	uint64_t raw[6];
	raw[0] = err * (depth - n0);
	raw[1] = GENO_HET * (n0 + n1) + err * (depth - n0 - n1);
	raw[2] = err * (depth - n1);
	raw[3] = GENO_HET * (n0 + n2) + err * (depth - n0 - n2);
	raw[4] = GENO_HET * (n1 + n2) + err * (depth - n1 - n2);
	raw[5] = err * (depth - n2);
	const uint32_t ng = k == 3u ? 6u : 3u;
	uint32_t gt = 0;
	uint64_t best = raw[0];
#pragma unroll
	for (uint32_t j = 1; j < 6; j++) { const bool lower = j < ng && raw[j] < best; gt = lower ? j : gt; best = lower ? raw[j] : best; }
	uint64_t second = ~0ull;
#pragma unroll
	for (uint32_t j = 0; j < 6; j++) { const bool in = j < ng && j != gt && raw[j] - best < second; second = in ? raw[j] - best : second; }
	GenoCall g;
	g.gt = gt; g.gq = second > 99ull ? 99u : (uint32_t)second;
#pragma unroll
	for (uint32_t j = 0; j < 6; j++) { const uint64_t d = raw[j] - best; g.pl[j] = j < ng ? (d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d) : 0u; }
	return g;
}
/* the weighted rule (`map -Y`, bwb_hip_pileq_begin): s0, s1, s2 the alleles' qsum columns, S the sum of all four; GT, GQ and the PLs from the raw
 * costs as in geno_rule.  (The selection is repeated here, not shared: sharing it through a helper changed k_geno_emit's instructions, and
 * every kernel from before -Y stays as it was.) */
__device__ __forceinline__ GenoCall geno_rule_q(uint64_t n0, uint64_t n1, uint64_t n2, uint64_t s0, uint64_t s1, uint64_t s2, uint32_t k, uint64_t S) {
	uint64_t raw[6];
	raw[0] = S - s0;
	raw[1] = GENO_HET * (n0 + n1) + (S - s0 - s1);
	raw[2] = S - s1;
	raw[3] = GENO_HET * (n0 + n2) + (S - s0 - s2);
	raw[4] = GENO_HET * (n1 + n2) + (S - s1 - s2);
	raw[5] = S - s2;
	const uint32_t ng = k == 3u ? 6u : 3u;
	uint32_t gt = 0;
	uint64_t best = raw[0];
#pragma unroll
	for (uint32_t j = 1; j < 6; j++) { const bool lower = j < ng && raw[j] < best; gt = lower ? j : gt; best = lower ? raw[j] : best; }
	uint64_t second = ~0ull;
#pragma unroll
	for (uint32_t j = 0; j < 6; j++) { const bool in = j < ng && j != gt && raw[j] - best < second; second = in ? raw[j] - best : second; }
	GenoCall g;
	g.gt = gt; g.gq = second > 99ull ? 99u : (uint32_t)second;
#pragma unroll
	for (uint32_t j = 0; j < 6; j++) { const uint64_t d = raw[j] - best; g.pl[j] = j < ng ? (d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d) : 0u; }
	return g;
}
/* Site s (< n_sites, checked by the caller) -> its word: the last w with site_base[w] <= s, by `trips` halving steps for every lane (2^trips >=
 * n_words, a kernel argument: selects, no divergent while; site_base[] does not descend and site_base[0] = 0).  The lanes of a wave hold 64
 * consecutive sites, which lie in a handful of neighbouring words: all but the last few steps load the same address in every lane, one
 * request each, and the top of the tree stays in L2 for the whole grid.  Every index is bounded: site_base[] below n_words. */
__device__ __forceinline__ uint32_t geno_word(uint64_t s, const uint32_t *site_base, uint32_t n_words, uint32_t trips) {
	uint32_t w = 0;
	for (uint32_t t = trips; t-- > 0;) {
		const uint32_t step = 1u << t;
		bool go = false;
		if (step < n_words - w) go = (uint64_t)site_base[w + step] <= s; /* (w < n_words throughout) */
		w = go ? w + step : w;
	}
	return w;
}
/* the character of the r-th site of a word (r < 32: at most 31 bits cleared), or 32 when the word has no such site - impossible on the index
 * built from this text, and then nothing is called - and the code there */
__device__ __forceinline__ uint32_t geno_char(const uint4 tw, uint32_t r, uint32_t *code) {
	uint32_t m = site_mask32(tw);
	for (uint32_t i = 0; i < r && m; i++) m &= m - 1u;
	const uint32_t at = m && r < 32u ? (uint32_t)__ffs((int)m) - 1u : 32u;
	const uint32_t q = (at & 31u) >> 3, x = q == 0u ? tw.x : q == 1u ? tw.y : q == 2u ? tw.z : tw.w;
	*code = (x >> (4u * (at & 7u))) & 15u;
	return at;
}
/* k_geno_count: one lane per site of [first, first + n) (first + n <= n_sites, checked by the caller: counts[] below n_sites), grid-strided:
 * cnt[i] = 1 when site first + i is called - depth, the sum of its four counters in one 16-byte load, >= min_depth - and its word kept in word[i]
 * so that k_geno_emit does not bisect again.  The scan of k_place_alt (k_scan_blocks / k_scan_sums / k_scan_add) turns cnt[] into off[0 .. n],
 * off[n] = the called sites. */
__global__ __launch_bounds__(BWB_BLOCK) void k_geno_count(const uint4 *text, const uint32_t *site_base, uint32_t n_words, uint32_t trips, const uint4 *counts, uint64_t first, uint32_t n,
                                                           uint64_t min_depth, uint32_t *cnt, uint32_t *word) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	for (uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x; i < n; i += gstride) {
		const uint64_t s = first + i;
		const uint32_t w = geno_word(s, site_base, n_words, trips);
		uint32_t code;
		const uint64_t r = s - (uint64_t)site_base[w];
		const uint32_t at = geno_char(text[w], r < 32u ? (uint32_t)r : 32u, &code);
		const uint4 c = counts[s];
		word[i] = w;
		cnt[i] = at < 32u && (uint64_t)c.x + c.y + c.z + c.w >= min_depth ? 1u : 0u;
	}
}
/* k_geno_emit, k_geno_emit_q: the same lanes; a called site makes its call and writes its 64-byte bwb_geno_site record at out[off[i]] (off[i] <
 * off[n] <= n: the output holds n records) as four 16-byte vector stores back to back.  The called lanes of a wave write neighbouring records, so
 * the wave's stores fill the same run of whole 64-byte lines, which L2 combines: no transpose through LDS (1.05 M sites, 787 k records: 0.09 ms
 * for the count pass, the scan and this kernel together).
 * Q, k_geno_emit_q (`map -Y`): behind the same k_geno_count and scan, with the weighted rule - the site's four qsum words in one 16-byte load
 * beside its counters - and the 80-byte bwb_geno_site_q record (the output holds n records of 80 bytes): the 64 bytes of bwb_geno_site, then the
 * four qsum words, as five 16-byte stores. */
template <bool Q> __device__ __forceinline__ void geno_emit_body(const uint4 *text, const uint32_t *site_base, uint32_t n_words, const uint4 *counts, const uint4 *qsum, uint64_t first,
                                                                 uint32_t n, uint32_t err, const uint32_t *cnt, const uint32_t *word, const uint64_t *off, uint4 *out) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	for (uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x; i < n; i += gstride) {
		if (!cnt[i]) continue;
		const uint64_t s = first + i, o = off[i];
		const uint32_t w = word[i];
		if (w >= n_words || o >= (uint64_t)n) continue; /* (k_geno_count wrote both: never) */
		uint32_t code;
		const uint64_t r = s - (uint64_t)site_base[w];
		const uint32_t at = geno_char(text[w], r < 32u ? (uint32_t)r : 32u, &code) & 31u; /* (k_geno_count found it below 32) */
		const uint32_t mem = (uint32_t)(GENO_MEMBERS >> (4u * code)) & 15u;
		const uint4 c = counts[s];
		uint4 qs = make_uint4(0u, 0u, 0u, 0u);
		if constexpr (Q) qs = qsum[s];
		/* the members in column order: the counters (with Q: and the quality sums) of the set bits of mem, lowest first (two or three of them) */
		uint64_t a[3] = { 0, 0, 0 }, e[3] = { 0, 0, 0 };
		uint32_t k = 0;
#pragma unroll
		for (uint32_t col = 0; col < 4; col++) {
			const uint32_t v = col == 0u ? c.x : col == 1u ? c.y : col == 2u ? c.z : c.w;
			const bool in = (mem >> col) & 1u;
			a[0] = in && k == 0u ? v : a[0]; a[1] = in && k == 1u ? v : a[1]; a[2] = in && k == 2u ? v : a[2];
			if constexpr (Q) {
				const uint32_t u = col == 0u ? qs.x : col == 1u ? qs.y : col == 2u ? qs.z : qs.w;
				e[0] = in && k == 0u ? u : e[0]; e[1] = in && k == 1u ? u : e[1]; e[2] = in && k == 2u ? u : e[2];
			}
			k += in ? 1u : 0u;
		}
		GenoCall g;
		if constexpr (Q) g = geno_rule_q(a[0], a[1], a[2], e[0], e[1], e[2], k, (uint64_t)qs.x + qs.y + qs.z + qs.w);
		else g = geno_rule(a[0], a[1], a[2], k, (uint64_t)c.x + c.y + c.z + c.w, err);
		const uint64_t pos = (uint64_t)w * 32u + at;
		uint4 *dst = out + o * (Q ? 5u : 4u);
		dst[0] = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), (uint32_t)s, (uint32_t)(s >> 32));
		dst[1] = c;
		dst[2] = make_uint4(code | (k == 3u ? 6u : 3u) << 8 | g.gt << 16 | g.gq << 24, 0u, g.pl[0], g.pl[1]);
		dst[3] = make_uint4(g.pl[2], g.pl[3], g.pl[4], g.pl[5]);
		if constexpr (Q) dst[4] = qs;
	}
}
__global__ __launch_bounds__(BWB_BLOCK) void k_geno_emit(const uint4 *text, const uint32_t *site_base, uint32_t n_words, const uint4 *counts, uint64_t first, uint32_t n, uint64_t min_depth,
                                                          uint32_t err, const uint32_t *cnt, const uint32_t *word, const uint64_t *off, uint4 *out) {
	geno_emit_body<false>(text, site_base, n_words, counts, nullptr, first, n, err, cnt, word, off, out);
}
__global__ __launch_bounds__(BWB_BLOCK) void k_geno_emit_q(const uint4 *text, const uint32_t *site_base, uint32_t n_words, const uint4 *counts, const uint4 *qsum, uint64_t first, uint32_t n,
                                                            const uint32_t *cnt, const uint32_t *word, const uint64_t *off, uint4 *out) {
	geno_emit_body<true>(text, site_base, n_words, counts, qsum, first, n, 0u, cnt, word, off, out);
}
/* k_geno_bubbles: one lane per bubble of [first, first + n) (first + n <= n_bub, checked by the caller), grid-strided.  off NULL, the count pass:
 * cnt[i] = 1 when the bubble is eligible (elig[], one byte per bubble from bwb_hip_indel_begin) and depth = ref + alt + ref_gapped + alt_gapped >=
 * min_depth; the same scan; then with off[] the emit pass: the call over R / V with other = the two gapped counters, and the 48-byte
 * bwb_geno_bubble record at out[off[i]] (off[i] < n) as three 16-byte vector stores. */
__global__ __launch_bounds__(BWB_BLOCK) void k_geno_bubbles(const uint8_t *elig, const uint4 *counts, uint32_t first, uint32_t n, uint64_t min_depth, uint32_t err, uint32_t *cnt,
                                                             const uint64_t *off, uint4 *out) {
	const uint32_t gstride = gridDim.x * BWB_BLOCK;
	for (uint32_t i = blockIdx.x * BWB_BLOCK + threadIdx.x; i < n; i += gstride) {
		const uint32_t b = first + i;
		const uint4 c = counts[b];
		const uint64_t depth = (uint64_t)c.x + c.y + c.z + c.w;
		const bool called = elig[b] && depth >= min_depth;
		if (!off) { cnt[i] = called ? 1u : 0u; continue; }
		if (!called) continue;
		const uint64_t o = off[i];
		if (o >= (uint64_t)n) continue; /* (the scan of the same predicate: never) */
		const GenoCall g = geno_rule(c.x, c.y, 0ull, 2u, depth, err);
		uint4 *dst = out + o * 3u;
		dst[0] = make_uint4(b, c.x, c.y, c.z);
		dst[1] = make_uint4(c.w, g.gt | g.gq << 8, g.pl[0], g.pl[1]);
		dst[2] = make_uint4(g.pl[2], 0u, 0u, 0u);
	}
}
