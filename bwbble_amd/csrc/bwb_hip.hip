/*
 * bwb_hip.hip - C-ABI implementation of include/bwbble_hip.h (libbwbble_hip.so), MI355X / gfx950 only.
 *
 * Host orchestration (replaces the per-batch body of align_reads_inexact_parallel, mg-aligner/inexact_match.c:103-165).
 * A context keeps up to BWB_MAX_SLOTS batches of reads resident ("slots") and runs them as a stream:
 *
 *   slot_upload(s)  reads -> pinned staging -> HBM on the copy stream                        (overlaps the kernels)
 *   slot_submit(s)  kl_calc_d over the slot, then ONE SLICE of kl_search fed from the slot's cursor.  With more batches to
 *                   come the slice does not drain: when the cursor runs out, waves park the reads they are working on in
 *                   the lanes' save area (bwb_lane.h) and the next slot's slice resumes them, so the heavy tail of batch k
 *                   runs next to the bulk of batch k+1 instead of on a nearly empty GPU.
 *   slot_wait(s)    until every read of the slot is done (normally when the following slice ends; a draining launch
 *                   otherwise), then the rare reads that did not fit the class-0 per-read scratch are re-run - still on the
 *                   GPU - in class 1, then class 2 (fewer lanes, larger lists, the whole chunk pool after a draining launch)
 *   slot_result(s)  hit log -> host on the result stream, put into read order
 *
 * batch_upload / batch_run / batch_result are the same on slot 0 with a draining slice (one batch, nothing to overlap).
 * There is no CPU fallback anywhere in this file.
 */
#include <hip/hip_runtime.h>
#include <time.h>
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "../../include/bwbble_hip.h"
#include "bwb_kernels.h"
static double wall_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
#include "bwb_lane.h"

static thread_local std::string g_err;
static int fail(int code, const std::string &m) { g_err = m; return code; }
#define HIPCHK(x)                                                                                         \
	do {                                                                                                  \
		hipError_t e_ = (x);                                                                              \
		if (e_ != hipSuccess) return fail(BWB_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));  \
	} while (0)
/* the same for this file's own functions: BWB_OK, or the error code of a call that has set the message */
#define RC(x)                    \
	do {                         \
		const int rc_ = (x);     \
		if (rc_) return rc_;     \
	} while (0)

/* device / pinned-host allocations that free themselves: an early error return leaks nothing */
struct DevMem {
	void *p = nullptr;
	size_t bytes = 0;
	DevMem() = default;
	DevMem(const DevMem &) = delete;
	DevMem &operator=(const DevMem &) = delete;
	~DevMem() { release(); }
	void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
	hipError_t alloc(size_t n) { release(); hipError_t e = hipMalloc(&p, n ? n : 1); if (e == hipSuccess) bytes = n; else p = nullptr; return e; }
	/* contents are NOT kept; grows by half again at least, so that a stream of slightly larger batches does not reallocate (hipFree
	 * synchronises the whole device and would stall the queued slices) */
	hipError_t reserve(size_t n) {
		if (p && bytes >= n) return hipSuccess;
		if (p && alloc(std::max(n, bytes + bytes / 2)) == hipSuccess) return hipSuccess;
		return alloc(n); /* (exactly what is asked for, when half again as much does not fit) */
	}
	template <typename T> T *as() const { return (T *)p; }
};
struct PinMem {
	void *p = nullptr;
	size_t bytes = 0;
	PinMem() = default;
	PinMem(const PinMem &) = delete;
	PinMem &operator=(const PinMem &) = delete;
	~PinMem() { if (p) (void)hipHostFree(p); }
	hipError_t reserve(size_t n) {
		if (p && bytes >= n) return hipSuccess;
		if (p) (void)hipHostFree(p);
		p = nullptr; bytes = 0;
		hipError_t e = hipHostMalloc(&p, n ? n : 1, hipHostMallocDefault);
		if (e == hipSuccess) bytes = n; else p = nullptr;
		return e;
	}
	template <typename T> T *as() const { return (T *)p; }
};
struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(const Event &) = delete;
	Event &operator=(const Event &) = delete;
	~Event() { if (e) (void)hipEventDestroy(e); }
	hipError_t create() { return e ? hipSuccess : hipEventCreate(&e); }
};

/* the buffers of one place_alt call: items per read, their exclusive scan, the scan's block sums, the bwb_alt records; and what the host gets */
struct AltBufs {
	DevMem d_cnt, d_off, d_bsum, d_alts;
	PinMem h_off, h_alts;
};

/* the buffers of one lift call: the kind byte and record size of every placement, the sizes' exclusive scan and its block sums, the records; and
 * what the host gets */
struct LiftBufs {
	DevMem d_kind, d_cnt, d_off, d_bsum, d_recs;
	PinMem h_kind, h_off, h_recs;
};

/* the buffers of one md call: one bwb_md per read, the MD lengths, their exclusive scan and its block sums, the MD bytes; and what the host gets */
struct MdBufs {
	DevMem d_recs, d_cnt, d_off, d_bsum, d_text;
	PinMem h_recs, h_off, h_text;
};

/* a pile kernel's block of 64-bit sums (k_pile: reads, adds; k_pile_q: and the bases dropped), and the figures of its last call that launched */
struct PileFigures {
	DevMem d_stats; PinMem h_stats;
	double ms = 0; uint64_t reads = 0, adds = 0, dropped = 0;
	int begin(size_t bytes) { HIPCHK(d_stats.alloc(bytes)); HIPCHK(h_stats.reserve(bytes)); return BWB_OK; }
	void zero() { ms = 0; reads = adds = dropped = 0; }
};

/* per-lane scratch of one class (class 0 = every resident lane, classes 1/2 = fewer lanes with larger lists) */
struct ScratchClass {
	DevMem mem;
	LaneScratch sc{};
	uint32_t blocks = 0;
	bool ready = false;
};

/* Which records a slot's result-stream stages hold: the arguments each was launched with last (-1: none).  A stage re-launches when its key differs;
 * what else it reads is invalidated here, by name, and nowhere else:
 *   place        key max_mm                                reads the hit log and the SA
 *   alt          key max_alt                               reads the hit log and the SA
 *   locus        key max_mm                                reads place and the tables of set_loci
 *   join         key max_mm, max_alt                       reads place, alt, locus, the hit log and the table of set_bubble_chrom
 *   lift         key max_mm, max_alt                       reads place, locus, alt (max_alt > 0), the tables of set_loci and set_bubble_chrom
 *   md           key max_mm, lifted, max_alt when lifted   reads the slot's reads, place, lift (lifted) and the text
 *   pile, indel  once per submission */
struct StageCache {
	int place_mm = -1, alt_max = -1, locus_mm = -1, join_mm = -1, join_alt = -1, lift_mm = -1, lift_alt = -1, md_mm = -1, md_alt = -1, md_lifted = -1;
	bool piled = false, indeled = false;
	void reset() { *this = StageCache(); }                                /* new reads or a new hit log: slot_upload, submit */
	void loci_replaced() { locus_mm = join_mm = lift_mm = md_mm = -1; }   /* set_loci (md reads lift) */
	void chrom_replaced() { join_mm = lift_mm = md_mm = -1; }             /* set_bubble_chrom */
	void text_replaced() { md_mm = -1; }                                  /* set_text */
};

/* one resident batch */
struct Slot {
	bool uploaded = false, submitted = false, complete = false, fetched = false;
	uint32_t n_reads = 0, stride = 0, maxlen = 0, dstride = 0;
	DevMem d_reads, d_lens, d_dbuf, d_status, d_n, d_off, d_worklist, d_log, d_ctl, d_dbg_iters, d_src;
	uint32_t n_tot = 0;           /* n_reads, plus one when the carried read (the source of a leading short read's D_seed) rides along for kl_calc_d */
	bool inherit = false;         /* some read takes its D_seed from an earlier one (d_src) */
	std::vector<uint32_t> h_src;
	uint64_t log_cap = 0;
	PinMem h_reads, h_lens, h_cnt, h_off, h_log, h_ctl;
	DevMem d_place;               /* bwb_hip_slot_place: one bwb_place per read */
	PinMem h_place;
	AltBufs alt;                  /* bwb_hip_slot_place_alt: the items of the slot's reads */
	DevMem d_locus;               /* bwb_hip_slot_locus: one bwb_locus per read */
	PinMem h_locus;
	DevMem d_cls, d_join;         /* bwb_hip_slot_join: one class byte per item, one bwb_join per read */
	PinMem h_join;
	LiftBufs lift;                /* bwb_hip_slot_lift */
	MdBufs md;                    /* bwb_hip_slot_md */
	StageCache stage;             /* which arguments the records above were made for */
	std::vector<uint8_t> h_status;
	std::vector<uint64_t> h_aln_off;
	std::vector<bwb_aln> h_alns;
	Event ev_up;
	DevMem d_quals; PinMem h_quals; /* bwb_hip_slot_quals: one quality byte per base of the resident reads, strided like d_reads */
	Event ev_quals;
	uint32_t up_stride = 0;         /* the caller's stride at slot_upload (slot_quals takes the same) */
	bool quals_set = false;         /* this upload's qualities are there; cleared by slot_upload */
	bool calcd_queued = false;    /* kl_calc_d of this batch has been queued ahead of its submit, on the context's second kernel stream (calcd_ahead) */
	Event ev_calcd;
	uint64_t launch = 0;          /* sequence number of the slice that was fed from this slot */
	/* control words on the device (d_ctl, 64 bytes apart): the work cursor, the number of finished reads, the hit count */
	uint32_t *ctl_counter() const { return d_ctl.as<uint32_t>(); }
	unsigned int *ctl_done() const { return d_ctl.as<unsigned int>() + 16; }
	unsigned long long *ctl_count() const { return (unsigned long long *)(d_ctl.as<unsigned char>() + 128); }
	uint32_t *ctl_counter2() const { return d_ctl.as<uint32_t>() + 48; } /* cursor of the re-run launches */
};

struct PendingTime { hipEvent_t e0, e1; int kind; }; /* kind 0 = kl_calc_d, 1 = kl_search */

struct bwb_hip_ctx {
	int device = 0, num_cu = 0;
	hipStream_t stream = nullptr, cstream = nullptr, rstream = nullptr; /* kernels; uploads; results */
	hipStream_t dstream = nullptr;      /* kl_calc_d of the batches AHEAD of the one being searched (calcd_ahead > 0) */
	int calcd_ahead = 0;                /* BWB_CALCD_AHEAD: how many uploaded slots beyond the submitted one get their kl_calc_d queued on dstream at once */
	DevIndex ix{};
	DevMem d_buckets, d_SA, d_stats, d_descs, d_misc;
	uint64_t sa0_index = 0, num_sa = 0;
	bool pos32 = true;                  /* BWT rows fit 32-bit positions */
	bwb_params p{};
	KParams kp{};
	bool have_params = false;
	Slot slots[BWB_MAX_SLOTS];
	SlotDesc h_descs[BWB_MAX_SLOTS]{};
	ScratchClass cls[3];
	DevMem d_pool, d_pool_bump;         /* heap chunk pool, POOL_REGIONS equal regions (the re-run classes use it after a drain); bump counters (two sets) */
	uint32_t keep = 256;                /* chunks of a lane's private run */
	int bpc_search = LANE_WAVES_PER_SIMD, bpc_calcd = LANE_WAVES_PER_SIMD; /* blocks of four waves per CU = waves per SIMD */
	bool wide = false;                  /* 32-byte heap entries (max_gapo > 1: more than one gap run per path) */
	bool parked = false;                /* reads may be parked in the class-0 save area (the last class-0 launch was a non-draining slice) */
	uint64_t n_launches = 0;            /* class-0 search launches so far */
	std::vector<hipEvent_t> launch_ev;  /* launch_ev[k-1-ev_base]: recorded after class-0 search launch k */
	uint64_t ev_base = 0;               /* launches whose events have been recycled (no slot in flight can wait for them) */
	std::vector<PendingTime> pending;
	std::vector<hipEvent_t> free_events;
	uint32_t slice_iters = 0;           /* BWB_SLICE_ITERS: test knob, time-sliced launches */
	double locate_ms = 0; uint64_t locate_steps = 0, locate_rows = 0; /* the last bwb_hip_locate call */
	DevMem d_qtab;                      /* k_place: 256 bytes (int)(4.343 * log(n) + 0.5), then its step counter */
	double place_ms = 0; uint64_t place_steps = 0, place_reads = 0;   /* the last place call */
	DevMem d_altctl;                    /* k_place_alt: its step counter and its count of flagged items */
	AltBufs hits_alt;                   /* bwb_hip_place_hits_alt: the items of the caller's hit list */
	double alt_ms = 0; uint64_t alt_steps = 0, alt_items = 0;         /* the last place_alt call */
	DevMem d_lstart, d_lend, d_lbub, d_bubbles; /* k_locus: the .ann records' first and last positions, their bubble numbers; the bubble table */
	uint32_t loci_nseq = 0, loci_trips = 0;       /* records (0: bwb_hip_set_loci has not been called); steps of the search, ceil(log2(records)) */
	double locus_ms = 0; uint64_t locus_reads = 0; /* the last locus call */
	std::vector<int32_t> loci_bub_of;             /* set_loci's bubble_of (set_bubble_chrom checks its table against it) */
	uint32_t loci_nbub = 0;
	DevMem d_chrom; bool chrom_set = false;       /* k_join_items: the chromosome record of every bubble (bwb_hip_set_bubble_chrom) */
	double join_ms = 0; uint64_t join_items = 0, join_joined = 0; /* the last join call */
	std::string lift_refusal;                     /* set_loci: why the rule of bwb_lift refuses the bubble table (empty: it does not) */
	LiftBufs lift_rec;                            /* bwb_hip_lift_records */
	double lift_ms = 0; uint64_t lift_lifted = 0, lift_unliftable = 0; /* the last lift call */
	DevMem d_text; uint64_t text_n = 0;           /* k_md_count / k_md: the forward text at 4 bits per character (bwb_hip_set_text; 0: none) */
	MdBufs md_rec;                                /* bwb_hip_md_records */
	double md_ms = 0; uint64_t md_reads = 0, md_bytes = 0; /* the last md call */
	DevMem d_site_base, d_counts;                 /* k_pile: the sites below every 16-byte word of the text, the n_sites x 4 counters (bwb_hip_pile_begin) */
	bool pile_on = false; uint64_t pile_sites = 0; /* pile_begin has run on this text; its sites */
	DevMem d_qsum;                                /* k_pile_q: the n_sites x 4 quality sums (weighted only; bwb_hip_pileq_begin) */
	bool pileq_on = false, pileq_weighted = false; /* pileq_begin has run behind this pile_begin: the slots keep quality bytes; qsum exists */
	PileFigures pile_fig, pileq_fig;              /* the last plain pile call that launched (k_pile: 2 sums), the last pile_q call that launched (k_pile_q: 3) */
	std::vector<bwb_bubble> loci_bubbles; std::vector<int32_t> chrom_of; /* the host's copies of set_loci's bubble table and set_bubble_chrom's records (bwb_hip_indel_begin) */
	DevMem d_indel_tab, d_indel_elig, d_indel_counts, d_indel_stats; /* k_indel: the eligible bubbles sorted by (chrom_of, lo, bubble), one byte per bubble, the n_bub x 4 counters, three sums of one launch */
	PinMem h_indel_stats;
	bool indel_on = false; uint32_t indel_anchor = 0, indel_ntab = 0, indel_trips = 0; /* indel_begin has run on these tables */
	double indel_ms = 0; uint64_t indel_reads = 0, indel_adds = 0, indel_cands = 0; /* the last indel call that launched */
	DevMem d_geno_cnt, d_geno_word, d_geno_off, d_geno_bsum, d_geno_sites, d_geno_bubs; /* the geno kernels: per entry of a piece the called flag, the site's word and the scan; the called records */
	PinMem h_geno_sites, h_geno_bubs, h_geno_n;
	bool geno_q = false;                /* geno_begin came behind a weighted pileq_begin: the site records' buffers hold 80-byte bwb_geno_site_q */
	bool geno_on = false, geno_bub = false; uint32_t geno_piece = 0, geno_piece_bub = 0; /* geno_begin has run on this site index (and on this bubble table) */
	double geno_ms = 0; uint64_t geno_sites_called = 0, geno_bubs_called = 0; /* the last geno_sites / geno_bubbles call: its kernels' time; the entries each called last */
	bool force_slices = false;          /* BWB_FORCE_SLICES: the one-batch API parks and resumes too (tests) */
	bool dbg = false, dbg_iters = false;
	const char *launch_log = nullptr;   /* BWB_LAUNCH_LOG=<file>: one JSON line per class-0 kernel launch (synchronises after every launch: a profiling aid) */
	unsigned long long log_prev[16] = { 0 };
	bwb_stats stats{};
	double t_run0 = 0;
	/* the calculate_d table (bwb_lane.h: DTab): entries and interval lists of all 4^K K-mers, built at the first large batch */
	DevMem d_dtab_ent, d_dtab_pool;
	int dtab_K = 0;                     /* 0: no table */
	uint32_t dtab_nm1[4] = { 0, 0, 0, 0 }; /* the level-1 entries' summed widths (DTab::nm1) */
	int dtab_multiref = -1;             /* the alphabet it was built for (-S has its own children) */
	int dtab_mode = -1;                 /* BWB_DTAB: 0 never, 1 always, unset: when a batch has at least DTAB_MIN_READS reads */
	bool dtab_failed = false;           /* a build did not fit its buffers: not tried again */
	double dtab_seconds = 0;
	/* bwb_hip_ctx_create_async: the index upload runs on this thread; everything that launches a kernel joins it first (index_ready) */
	std::thread idx_thread;
	int idx_rc = BWB_OK;
	std::string idx_err;
	double idx_seconds = 0, pool_seconds = 0; /* index upload (context creation to the last bucket in HBM); the chunk pool's hipMalloc */
	~bwb_hip_ctx() {
		if (idx_thread.joinable()) idx_thread.join();
		for (auto &pt : pending) { (void)hipEventDestroy(pt.e0); (void)hipEventDestroy(pt.e1); }
		for (auto e : free_events) (void)hipEventDestroy(e);
		for (auto e : launch_ev) (void)hipEventDestroy(e);
		if (stream) (void)hipStreamDestroy(stream);
		if (cstream) (void)hipStreamDestroy(cstream);
		if (rstream) (void)hipStreamDestroy(rstream);
		if (dstream) (void)hipStreamDestroy(dstream);
	}
};

/* The run-time choices among a kernel's instantiations, so that a launch is written once: f(uint32_t{}) or f(uint64_t{}) by the context's
 * position width, f(std::true_type{}) or f(std::false_type{}) by a flag; f is a generic lambda that names decltype(p) / decltype(b)::value. */
template <typename F> static auto with_pos(const bwb_hip_ctx *c, F &&f) { return c->pos32 ? f(uint32_t{}) : f(uint64_t{}); }
template <typename F> static auto with_flag(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
/* grid of a kernel that works in octets of lanes, one item per octet (k_rank16, k_locate, k_place, k_place_alt) */
static unsigned oct_grid(const bwb_hip_ctx *c, size_t n) { return (unsigned)std::min<size_t>((n + BWB_OCTS_PER_BLOCK - 1) / BWB_OCTS_PER_BLOCK, (size_t)c->num_cu * 8); }

/* blocks that give every one of n items a lane; and the grid of a kernel whose lanes stride over the items, eight blocks per CU at the most (the
 * kernels behind k_place: a lane's walk is a chain of dependent loads, and the waves beside it are what hides their latency) */
static unsigned blocks_of(size_t n) { return (unsigned)((n + BWB_BLOCK - 1) / BWB_BLOCK); }
static unsigned lane_grid(const bwb_hip_ctx *c, size_t n) { return (unsigned)std::min<size_t>(blocks_of(n), (size_t)c->num_cu * 8); }
/* the steps of a bisection over n entries: ceil(log2(n)), 0 for n <= 1 */
static uint32_t ceil_log2(uint64_t n) { uint32_t t = 0; while (((uint64_t)1 << t) < n) t++; return t; }

extern "C" const char *bwb_hip_last_error(void) { return g_err.c_str(); }
static_assert(sizeof(bwb_aln) == 16 * ALN_U4, "bwb_aln is ALN_U4 16-byte words (bwb_lane.h)");
extern "C" int bwb_hip_abi_version(void) { return BWB_HIP_ABI_VERSION; }

/* NUMA node of the device's PCIe root (sysfs), -1 when the machine has one node or it cannot be told: `bwbble align` pins the host
 * thread that drives a GPU, and with it the pinned staging buffers that thread allocates, to that node */
extern "C" int bwb_hip_device_numa_node(int device) {
	char bus[64] = { 0 };
	if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return -1;
	for (char *q = bus; *q; q++) *q = (char)tolower((unsigned char)*q);
	const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
	FILE *f = fopen(path.c_str(), "r");
	if (!f) return -1;
	int node = -1;
	if (fscanf(f, "%d", &node) != 1) node = -1;
	fclose(f);
	return node;
}

extern "C" int bwb_hip_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" void bwb_default_params(bwb_params *p) { /* set_default_aln_params, align.c:22-38 */
	memset(p, 0, sizeof(*p));
	p->gape_score = 4; p->gapo_score = 11; p->mm_score = 3; p->max_diff = 0; p->max_gape = 6; p->max_gapo = 1;
	p->seed_length = 32; p->max_diff_seed = 2; p->max_entries = 3000000; p->use_precalc = 0; p->matched_Ncontig = 0;
	p->is_multiref = 1; p->max_best = 30; p->no_indel_length = 5; p->n_threads = 1;
}

/* D2H of a few bytes without touching the null stream (which would wait for every queued slice) */
static int fetch(bwb_hip_ctx *c, void *dst, const void *src, size_t n) {
	HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	return BWB_OK;
}

/* waits until the caller's loader has brought the first `need` 128-character blocks of the index into the host arrays */
static void wait_blocks(const volatile uint64_t *ready, uint64_t need) {
	if (!ready) return;
	while (__atomic_load_n(ready, __ATOMIC_ACQUIRE) < need) { struct timespec ts = { 0, 200000 }; nanosleep(&ts, nullptr); }
}

extern "C" int bwb_hip_ctx_create(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt,
                                  const uint64_t *O, bwb_hip_ctx **out) {
	return bwb_hip_ctx_create_streamed(device, hdr, C, bwt, O, nullptr, out);
}

#ifndef BWB_IDX_CHUNK_SHIFT
#define BWB_IDX_CHUNK_SHIFT 20          /* blocks per upload chunk = 2^20 (the test build `make testlib` uses 10, so that a few-M-row index is uploaded in
                                           dozens of chunks - both staging sets, a partial last chunk, superblock starts inside chunks - like a GRCh37-scale one) */
#endif
/* the upload: re-layout on the GPU, chunk by chunk behind the caller's loader (runs on the creating thread, or on the context's own
 * thread after bwb_hip_ctx_create_async) */
static int index_upload(bwb_hip_ctx *c, uint64_t num_words, uint64_t sa0, const uint64_t *C, const uint32_t *bwt, const uint64_t *O, const volatile uint64_t *blocks_ready) {
	const double t0 = wall_s();
	HIPCHK(hipSetDevice(c->device));
	const uint64_t nblk = c->ix.nblk;
	/* superblock base table (a superblock's row is filled in when the upload below reaches its first block: with a streamed index the
	 * host arrays are still being read) */
	std::vector<uint64_t> sbcount(BWB_NSB_MAX * 16, 0);
	/* 2^20 blocks (128 M characters) per chunk: reference arrays -> 128-character buckets in a staging
	 * buffer (k_relayout) -> the index's 64-character buckets (k_relayout64); the two staging sets alternate so that the copy
	 * of chunk k+1 overlaps the kernels of chunk k */
	const uint64_t CH = 1ull << BWB_IDX_CHUNK_SHIFT;
	DevMem d_bwt[2], d_O[2], d_b128[2], d_sbc;
	Event ev_k[2];
	for (int t = 0; t < 2; t++) {
		HIPCHK(d_bwt[t].alloc(std::min(CH, nblk) * 64));
		HIPCHK(d_O[t].alloc(std::min(CH, nblk) * 128));
		HIPCHK(d_b128[t].alloc(std::min(CH, nblk) * 128));
		HIPCHK(ev_k[t].create());
	}
	HIPCHK(d_sbc.alloc(sbcount.size() * 8));
	int t = 0;
	for (uint64_t b0 = 0; b0 < nblk; b0 += CH, t ^= 1) {
		const uint64_t nb = std::min(CH, nblk - b0);
		const uint64_t w0 = b0 * 16, nw = std::min(nb * 16, num_words - w0);
		wait_blocks(blocks_ready, b0 + nb); /* streamed: the loader has read this chunk of the .bwt file */
		for (uint64_t blk = b0; blk < b0 + nb; blk += (1ull << BWB_SB_SHIFT) - (blk & ((1ull << BWB_SB_SHIFT) - 1))) {
			if (blk & ((1ull << BWB_SB_SHIFT) - 1)) continue; /* (on to the next superblock start inside this chunk) */
			const uint64_t sb = blk >> BWB_SB_SHIFT;
			const uint32_t first = bwt[blk * 16] >> 28;
			for (int j = 0; j < 16; j++) {
				sbcount[sb * 16 + j] = O[blk * 16 + j] - ((first == (uint32_t)j && !(j == 0 && blk * 128 == sa0)) ? 1 : 0);
				c->ix.base[sb][j] = C[j] + sbcount[sb * 16 + j];
			}
			HIPCHK(hipStreamSynchronize(c->stream)); /* (the kernels queued so far read the table: a superblock is 16 chunks, this is rare) */
			HIPCHK(hipMemcpy(d_sbc.p, sbcount.data(), sbcount.size() * 8, hipMemcpyHostToDevice));
		}
		HIPCHK(hipEventSynchronize(ev_k[t].e)); /* the kernel that read this staging set two chunks ago */
		HIPCHK(hipMemcpyAsync(d_bwt[t].p, bwt + w0, nw * 4, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemcpyAsync(d_O[t].p, O + b0 * 16, nb * 128, hipMemcpyHostToDevice, c->stream));
		const uint64_t nthreads = nb * 8;
		hipLaunchKernelGGL(k_relayout, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, c->stream, d_bwt[t].as<uint32_t>(), d_O[t].as<uint64_t>(), b0, nb, nw,
		                   sa0, d_sbc.as<uint64_t>(), d_b128[t].as<uint4>());
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_relayout64, dim3((unsigned)((nb * 2 + 255) / 256)), dim3(256), 0, c->stream, d_b128[t].as<uint4>(), nb, c->d_buckets.as<uint4>() + b0 * 16);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev_k[t].e, c->stream));
	}
	HIPCHK(hipStreamSynchronize(c->stream));
	c->idx_seconds = wall_s() - t0;
	return BWB_OK;
}

/* joins the upload thread of an asynchronously created context; its error becomes this call's */
static int index_ready(bwb_hip_ctx *c) {
	if (c->idx_thread.joinable()) c->idx_thread.join();
	if (c->idx_rc) return fail(c->idx_rc, "index upload: " + c->idx_err);
	return BWB_OK;
}

static int ctx_create(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt, const uint64_t *O,
                      const volatile uint64_t *blocks_ready, bool async, bwb_hip_ctx **out) {
	if (!hdr || !C || !bwt || !O || !out) return fail(BWB_E_ARG, "ctx_create: null argument");
	const uint64_t length = hdr[0], num_words = hdr[1], num_occ = hdr[3];
	const uint64_t nblk = (length + 127) / 128;
	if (length < 2 || num_occ != nblk || num_words != (length + 7) / 8) return fail(BWB_E_ARG, "ctx_create: inconsistent .bwt header");
	const uint64_t nsb = (nblk + (1ull << BWB_SB_SHIFT) - 1) >> BWB_SB_SHIFT;
	if (nsb > BWB_NSB_MAX) return fail(BWB_E_ARG, "ctx_create: index larger than the superblock table covers (2^34 characters)");
	HIPCHK(hipSetDevice(device));
	std::unique_ptr<bwb_hip_ctx> c(new bwb_hip_ctx()); /* freed with everything it owns on any early return */
	c->device = device;
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, device));
	c->num_cu = prop.multiProcessorCount;
	HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
	HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
	HIPCHK(hipStreamCreateWithFlags(&c->rstream, hipStreamNonBlocking));
	HIPCHK(c->d_buckets.alloc(nblk * 256)); /* 64-character buckets: 2 bytes per BWT character */
	HIPCHK(c->d_stats.alloc(sizeof(unsigned long long) * STAT_WORDS));
	HIPCHK(c->d_descs.alloc(sizeof(SlotDesc) * BWB_MAX_SLOTS));
	HIPCHK(c->d_misc.alloc(256));
	HIPCHK(hipMemsetAsync(c->d_stats.p, 0, sizeof(unsigned long long) * STAT_WORDS, c->stream));
	c->dbg = getenv("BWB_DEBUG") != nullptr;
	c->dbg_iters = getenv("BWB_DEBUG_ITERS") != nullptr;
	if (getenv("BWB_DTAB") && *getenv("BWB_DTAB")) c->dtab_mode = atoi(getenv("BWB_DTAB")) ? 1 : 0;
	c->launch_log = getenv("BWB_LAUNCH_LOG");
	if (c->launch_log && !*c->launch_log) c->launch_log = nullptr;
	if (getenv("BWB_SLICE_ITERS")) c->slice_iters = (uint32_t)strtoul(getenv("BWB_SLICE_ITERS"), nullptr, 10);
	c->force_slices = getenv("BWB_FORCE_SLICES") != nullptr || c->slice_iters != 0;
	if (getenv("BWB_CALCD_AHEAD")) c->calcd_ahead = std::max(0, std::min(BWB_MAX_SLOTS - 1, atoi(getenv("BWB_CALCD_AHEAD"))));
	if (c->calcd_ahead > 0) {
		int lo = 0, hi = 0; /* (numerically lowest = highest priority) */
		(void)hipDeviceGetStreamPriorityRange(&lo, &hi);
		const char *pe = getenv("BWB_CALCD_PRIO");
		HIPCHK(hipStreamCreateWithPriority(&c->dstream, hipStreamNonBlocking, (pe && atoi(pe) > 0) ? hi : ((pe && atoi(pe) < 0) ? lo : 0)));
	}
	memset(&c->ix, 0, sizeof(c->ix));
	for (uint64_t sb = 0; sb < BWB_NSB_MAX; sb++)
		for (int j = 0; j < 16; j++) c->ix.base[sb][j] = C[j];
	for (int j = 0; j < 16; j++) { c->ix.base[BWB_ROW_NEG][j] = C[j]; c->ix.base[BWB_ROW_END][j] = C[j + 1]; }
	c->ix.buckets = c->d_buckets.as<uint4>();
	c->ix.length = length;
	c->ix.nblk = nblk;
	c->sa0_index = hdr[4];
	c->pos32 = length < 0xFFFFFFFFull && !getenv("BWB_FORCE_POS64");
	if (!async) {
		RC(index_upload(c.get(), num_words, hdr[4], C, bwt, O, blocks_ready));
	} else {
		bwb_hip_ctx *cp = c.get();
		const uint64_t sa0 = hdr[4];
		cp->idx_thread = std::thread([cp, num_words, sa0, C, bwt, O, blocks_ready]() {
			cp->idx_rc = index_upload(cp, num_words, sa0, C, bwt, O, blocks_ready);
			if (cp->idx_rc) cp->idx_err = g_err; /* (g_err is per thread: handed to whoever joins) */
		});
	}
	*out = c.release();
	return BWB_OK;
}

extern "C" int bwb_hip_ctx_create_streamed(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt,
                                           const uint64_t *O, const volatile uint64_t *blocks_ready, bwb_hip_ctx **out) {
	return ctx_create(device, hdr, C, bwt, O, blocks_ready, false, out);
}

extern "C" int bwb_hip_ctx_create_async(int device, const uint64_t hdr[5], const uint64_t C[17], const uint32_t *bwt,
                                        const uint64_t *O, const volatile uint64_t *blocks_ready, bwb_hip_ctx **out) {
	return ctx_create(device, hdr, C, bwt, O, blocks_ready, true, out);
}

extern "C" int bwb_hip_ctx_index_wait(bwb_hip_ctx *c, double *seconds) {
	if (!c) return fail(BWB_E_ARG, "ctx_index_wait: null context");
	RC(index_ready(c));
	if (seconds) *seconds = c->idx_seconds;
	return BWB_OK;
}

extern "C" int bwb_hip_dtab_info(bwb_hip_ctx *c, int *K, double *build_seconds, uint64_t *bytes) {
	if (!c) return fail(BWB_E_ARG, "dtab_info: null context");
	if (K) *K = c->dtab_K;
	if (build_seconds) *build_seconds = c->dtab_seconds;
	if (bytes) *bytes = c->dtab_K ? c->d_dtab_ent.bytes + c->d_dtab_pool.bytes : 0;
	return BWB_OK;
}

extern "C" int bwb_hip_setup_times(bwb_hip_ctx *c, double *index_seconds, double *pool_seconds, uint64_t *pool_bytes) {
	if (!c) return fail(BWB_E_ARG, "setup_times: null context");
	if (index_seconds) *index_seconds = c->idx_thread.joinable() ? -1.0 : c->idx_seconds; /* (-1: the upload is still running) */
	if (pool_seconds) *pool_seconds = c->pool_seconds;
	if (pool_bytes) *pool_bytes = c->d_pool.bytes;
	return BWB_OK;
}

extern "C" void bwb_hip_ctx_destroy(bwb_hip_ctx *c) {
	if (!c) return;
	(void)hipSetDevice(c->device);
	if (c->idx_thread.joinable()) c->idx_thread.join(); /* (the upload thread reads the caller's arrays: they are free once this returns) */
	(void)hipDeviceSynchronize();
	delete c;
}

static size_t lane_lds(const bwb_hip_ctx *c) {
	(void)c;
	return (size_t)LDS_WAVES_OFF + (size_t)(LANE_BLOCK / 64) * WAVE_LDS_BYTES + LDS_ALIGN_SLACK; /* base table + zero row + per wave: gather staging / children */
}
static size_t calcd_lds(void) { return (size_t)CALCD_LDS_BYTES; } /* kl_calc_d's own map: one base table, its own number of compacted U rows (bwb_lane.h) */

static uint32_t max_reads_resident(const bwb_hip_ctx *c) {
	uint32_t n = 1;
	for (const Slot &s : c->slots) n = std::max(n, s.n_reads);
	return n;
}

/* The class-0 heap chunk pool, sized for the batches at hand and grown when a larger batch or index needs more (it can be
 * replaced only while no read is parked).  hipMalloc costs about 27 ms per GB here, which a 600-read run should not pay. */
static int ensure_pool(bwb_hip_ctx *c) {
	size_t fr = 0, tot = 0;
	HIPCHK(hipMemGetInfo(&fr, &tot));
	fr += c->d_pool.bytes; /* what would be free without the current pool */
	/* Ceiling: what is free (the index, the class-0 scratch and the first slot are allocated by now) minus what is still to
	 * come - the scratch of the re-run classes and their pool, three more slots like the largest so far, some slack - and what
	 * the regions can name: a state word holds a 26-bit chunk index relative to the block's region. */
	const size_t isz = c->pos32 ? 8 : 16;
	const size_t cls1 = (size_t)std::max(1, c->num_cu / 2) * LANE_BLOCK * (2 * 8192 * isz + 1024 * sizeof(bwb_aln)), cls2 = (size_t)LANE_BLOCK * (2 * ((size_t)1 << 20) * isz + 65536 * sizeof(bwb_aln));
	size_t slot_bytes = 0;
	for (const Slot &s : c->slots) slot_bytes = std::max(slot_bytes, s.d_reads.bytes + s.d_quals.bytes + s.d_dbuf.bytes + s.d_log.bytes + (size_t)s.n_reads * sizeof(bwb_aln));
	/* (every slot still to come like the largest so far: a stream needs them all - the heaviest reads of a batch take several slices'
	 * time, DESIGN.md section 2.3 - and 8 x 3 GB is little next to the pool) */
	size_t more_slots = 0; /* slots that have no buffers yet (a caller that uploads every slot before the first submit - bench.py - has none left) */
	for (const Slot &s : c->slots) if (s.d_reads.bytes == 0) more_slots++;
	/* (the calculate_d table, when it is still to be built: 4^12 entries of 32 bytes and their lists - about sixty intervals each at GRCh37
	 * scale, never more intervals than one and a half times the BWT's rows plus one per K-mer; its BUILD borrows this pool as scratch) */
	const size_t dtab_res = (c->dtab_mode != 0 && !c->dtab_K && !c->dtab_failed)
	                            ? ((size_t)32 << 24) + std::min<size_t>((size_t)64 << 24, (size_t)(c->ix.length + c->ix.length / 2) + ((size_t)1 << 24)) * isz + ((size_t)1 << 28) : 0;
	const size_t reserve = cls1 + cls2 + more_slots * slot_bytes + ((size_t)4 << 30) + dtab_res;
	const size_t ceiling = std::min<size_t>(fr > reserve + ((size_t)1 << 30) ? fr - reserve : fr / 2, (size_t)POOL_REGIONS << 36);
	/* Need: per read in flight, the private run (keep chunks of 1 KB, 2 KB with 32-byte entries) plus a share of the
	 * common part that grows with the index: measured 37 KB per lane at 106 M rows, ~300 KB at 884 M, 870 KB at 6.85 G. */
	const size_t lanes = std::min<size_t>(max_reads_resident(c), (size_t)c->num_cu * (size_t)c->bpc_search * LANE_BLOCK);
	const size_t index_mb = (size_t)(c->ix.nblk >> 13) + 1;
	const size_t per_lane = ((size_t)c->keep << 10) + std::min<size_t>((size_t)1536 << 10, index_mb << 9);
	size_t want = std::max<size_t>((size_t)1 << 30, lanes * per_lane / 4 * 5 * (c->wide ? 2 : 1));
	/* (`-n 0`, the reference's default: a read's heap is its root entry - the search goes straight to the exact tail, :345 - so the pool is a
	 * few chunks per lane instead of 170 GB, whose hipMalloc and hipFree were a quarter of a 10 M-read `align -n 0` run: round 6) */
	if (c->kp.max_diff == 0) want = std::max<size_t>((size_t)256 << 20, lanes * (size_t)4096);
	if (want > ceiling) want = ceiling;
	if (getenv("BWB_POOL_GB") && *getenv("BWB_POOL_GB")) want = std::min<size_t>((size_t)atol(getenv("BWB_POOL_GB")) << 30, fr / 10 * 7);
	if (want < ((size_t)256 << 20)) want = (size_t)256 << 20; /* floor (also what BWB_POOL_GB=0 selects, to test the re-run path: class 2 must still fit a read) */
	want &= ~(size_t)(POOL_REGIONS * 4096 - 1);
	/* (a pool within 15 % of what would be asked for now is kept: `want` moves by a slot's size with every upload and by the table's reserve
	 * once that is built, and giving 170 GB back to the driver and taking them again costs five seconds - rounds 3-5 did that at every one of a
	 * stream's first uploads, round 6's profiles/r6_ab_steps.txt session 3) */
	if (c->d_pool.p && (c->d_pool.bytes >= want || (c->d_pool.bytes >= want / 20 * 17 && !getenv("BWB_POOL_GB")))) return BWB_OK;
	if (c->parked) return BWB_OK; /* parked reads hold chunks of the present pool: keep it (the admission control copes) */
	c->d_pool.release();
	if (want > fr) return fail(BWB_E_HIP, "not enough device memory for the heap chunk pool");
	{ const double t0 = wall_s(); HIPCHK(c->d_pool.alloc(want)); c->pool_seconds += wall_s() - t0; }
	if (c->dbg) fprintf(stderr, "[bwb] chunk pool: %.1f GB allocated in %.2f s\n", (double)want / (1u << 30), c->pool_seconds);
	if (!c->d_pool_bump.p) HIPCHK(c->d_pool_bump.alloc(2 * POOL_REGIONS * 64));
	return BWB_OK;
}

static int ensure_class(bwb_hip_ctx *c, int k) {
	ScratchClass &s = c->cls[k];
	uint32_t blocks, lcap, acap;
	if (k == 0) {
		/* Blocks (of four waves) per CU.  Both kernels are built for three (bwb_lane.h), and run three.  (Rounds 3-5 ran kl_search at two when
		 * the parameters allow more than three differences: every lane holds a read with its heap, and the stationary heaps of 196 608 reads
		 * with -n 5 on 150 bp reads overran the 200 GB chunk pool - reads were abandoned and re-run, 103 k reads/s against 224 k at two blocks,
		 * profiles/r5_bench_line_c5_three_blocks.json.)  The choice can change only while nothing is parked (the grid, and with it the pool
		 * geometry, is fixed for the life of a stream); BWB_BLOCKS_PER_CU overrides it. */
		if (!s.ready || !c->parked) {
			c->bpc_search = LANE_WAVES_PER_SIMD; /* (round 6: also beyond three differences - with the gap entries halved, see bwb_lane.h `combined group`,
			                                        the stationary heaps of 196 608 reads with -n 5 on 150 bp reads fill 60 % of the pool; rounds 3-5 ran two blocks there) */
			c->bpc_calcd = CALCD_WAVES_PER_SIMD;
			if (getenv("BWB_BLOCKS_PER_CU")) c->bpc_search = std::max(1, atoi(getenv("BWB_BLOCKS_PER_CU")));
			if (getenv("BWB_CALCD_BLOCKS_PER_CU")) c->bpc_calcd = std::max(1, atoi(getenv("BWB_CALCD_BLOCKS_PER_CU")));
			/* A slice's blocks must all be resident at once: a parked read only moves while its block runs, and a block that had to
			 * wait for another one to leave would find the cursor exhausted and park again at once.  So never more blocks per CU than
			 * the runtime says fit (registers, LDS) - and never more than the LDS really holds: the runtime's answer was 3 for a block
			 * size of which the hardware placed 2 (allocation in units of 1 280 bytes; profiles/r4_lds_probe.txt), which cost 13 % unnoticed. */
			int occ = 0;
			auto lds_fit = [&](const void *f, size_t dyn) {
				hipFuncAttributes fa;
				if (hipFuncGetAttributes(&fa, f) != hipSuccess) return LANE_WAVES_PER_SIMD;
				const size_t need = ((fa.sharedSizeBytes + dyn + LDS_GRANULE - 1) / LDS_GRANULE) * LDS_GRANULE;
				return (int)std::max<size_t>(1, LDS_CU_BYTES / need);
			};
			const void *kf = with_pos(c, [&](auto p) { /* (the -S instantiations need no more) */
				return with_flag(c->wide, [](auto w) { return (const void *)kl_search<decltype(p), decltype(w)::value, true>; });
			});
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kf, LANE_BLOCK, lane_lds(c)) == hipSuccess && occ >= 1) {
				if (c->dbg && !s.ready) fprintf(stderr, "[bwb] kl_search: %d block(s) of %d threads fit a CU\n", occ, LANE_BLOCK);
				c->bpc_search = std::min(c->bpc_search, std::min(occ, lds_fit(kf, lane_lds(c))));
				if (c->dbg && !s.ready && lds_fit(kf, lane_lds(c)) < occ) fprintf(stderr, "[bwb] kl_search: only %d block(s) per CU by LDS granules\n", lds_fit(kf, lane_lds(c)));
			}
			const void *kd = with_pos(c, [](auto p) { return (const void *)kl_calc_d<decltype(p)>; });
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kd, LANE_BLOCK, calcd_lds()) == hipSuccess && occ >= 1) {
				c->bpc_calcd = std::min(c->bpc_calcd, std::min(occ, lds_fit(kd, calcd_lds())));
				if (c->dbg && !s.ready) fprintf(stderr, "[bwb] kl_calc_d: %d block(s) per CU (occupancy query %d, LDS granules %d)\n", c->bpc_calcd, occ, lds_fit(kd, calcd_lds()));
			}
		}
		/* (the scratch is sized for the larger grid: the two kernels share it) */
		blocks = (uint32_t)(c->num_cu * std::max(LANE_WAVES_PER_SIMD, std::max(c->bpc_search, c->bpc_calcd))); lcap = 4096; acap = 256;
	} else if (k == 1) {
		blocks = (uint32_t)std::max(1, c->num_cu / 2); lcap = 8192; acap = 1024;
	} else {
		blocks = 1; lcap = 1u << 20; acap = 1u << 16;
	}
	const uint32_t nslots = blocks * LANE_BLOCK;
	const size_t isz = c->pos32 ? 8 : 16;
	auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const uint32_t brow = std::max<uint32_t>(BSTATE_ROW_MIN, ((uint32_t)c->kp.num_buckets + 63u) & ~63u);
	const size_t b_bstate = al((size_t)brow * nslots * 4), b_lists = al((size_t)nslots * 2 * lcap * isz), b_alns = al((size_t)nslots * acap * sizeof(bwb_aln)),
	             b_save = al((size_t)nslots * SAVE_U4 * 16), b_bsave = al((size_t)blocks * 16);
	/* class 0 runs kl_calc_d of the next batch while parked reads keep their lists: it gets a second set; the re-run classes
	 * are drained before anything else uses them */
	const size_t bytes = b_bstate + b_lists * (k == 0 ? 2 : 1) + b_alns + b_save + b_bsave;
	if (!(s.mem.p && s.mem.bytes >= bytes)) {
		if (k == 0 && c->parked) return fail(BWB_E_STATE, "the class-0 scratch cannot grow while reads are parked (flush first)");
		if (c->dstream) HIPCHK(hipStreamSynchronize(c->dstream)); /* (a kl_calc_d queued ahead works in this scratch) */
		s.mem.release();
		size_t fr = 0, tot = 0;
		HIPCHK(hipMemGetInfo(&fr, &tot));
		if (bytes + ((size_t)1 << 30) > fr) return fail(BWB_E_HIP, "not enough device memory for the per-lane scratch (class " + std::to_string(k) + ")");
		HIPCHK(s.mem.alloc(bytes));
		HIPCHK(hipMemsetAsync((unsigned char *)s.mem.p + bytes - b_save - b_bsave, 0, b_save + b_bsave, c->stream));
	}
	unsigned char *base = s.mem.as<unsigned char>();
	s.sc.bstate = (uint32_t *)base; base += b_bstate;
	s.sc.lists = (void *)base; base += b_lists;
	s.sc.lists_d = s.sc.lists;
	if (k == 0) { s.sc.lists_d = (void *)base; base += b_lists; }
	s.sc.alns = (uint4 *)base; base += b_alns;
	s.sc.save = (uint4 *)base; base += b_save;
	s.sc.blocksave = (uint32_t *)base;
	s.sc.nslots = nslots; s.sc.lcap = lcap; s.sc.acap = acap; s.sc.brow = brow;
	s.sc.keep = c->keep;
	s.blocks = blocks;
	s.ready = true;
	return ensure_pool(c); /* (after the scratch: the pool takes what is left over; the re-run classes use it too, after a drain) */
}

static hipEvent_t get_event(bwb_hip_ctx *c) {
	if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
	hipEvent_t e = nullptr;
	if (hipEventCreate(&e) != hipSuccess) return nullptr;
	return e;
}

/* One timed region of a stream: two events of the context's pool, recorded around it.  Both go back to the pool on every way out (one
 * alone too, when the other could not be created) - unless the span has been handed to c->pending, whose events resolve_times returns
 * once the launch has finished. */
struct Timed {
	bwb_hip_ctx *c;
	hipStream_t st;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	bool own = true;
	Timed(bwb_hip_ctx *c_, hipStream_t st_) : c(c_), st(st_) {}
	Timed(const Timed &) = delete;
	Timed &operator=(const Timed &) = delete;
	~Timed() { if (own && e0) c->free_events.push_back(e0); if (own && e1) c->free_events.push_back(e1); }
	int begin() {
		e0 = get_event(c); e1 = get_event(c);
		if (!e0 || !e1) return fail(BWB_E_HIP, "hipEventCreate failed");
		HIPCHK(hipEventRecord(e0, st));
		return BWB_OK;
	}
	int end() { HIPCHK(hipEventRecord(e1, st)); return BWB_OK; }
	int ms(float *out) const { HIPCHK(hipEventElapsedTime(out, e0, e1)); return BWB_OK; } /* (after the stream, or e1, has been waited for) */
	void defer(int kind) { c->pending.push_back(PendingTime{ e0, e1, kind }); own = false; } /* kind: PendingTime */
};

/* adds the HIP-event time of every finished launch to the statistics (all of them when `all`: the stream must be idle then) */
static int resolve_times(bwb_hip_ctx *c, bool all) {
	size_t w = 0;
	for (size_t i = 0; i < c->pending.size(); i++) {
		PendingTime &pt = c->pending[i];
		const bool ready = all || hipEventQuery(pt.e1) == hipSuccess;
		if (!ready) { c->pending[w++] = pt; continue; }
		if (all) HIPCHK(hipEventSynchronize(pt.e1));
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, pt.e0, pt.e1));
		if (pt.kind == 0) { c->stats.ms_calc_d += ms; c->stats.launches_calc_d++; }
		else { c->stats.ms_search += ms; c->stats.launches_search++; }
		c->free_events.push_back(pt.e0); c->free_events.push_back(pt.e1);
	}
	c->pending.resize(w);
	return BWB_OK;
}

static int check_params(const bwb_params *p, int *nb_out) {
	if (p->max_gapo < 0 || p->max_gapo > BWB_MAX_GAP_RUNS) return fail(BWB_E_ARG, "max_gapo (-o) must be in [0,8] on the GPU path (a heap entry and a hit record hold eight gap runs)");
	if (p->max_gape < 0 || p->max_gape > 100 || p->max_diff < 0 || p->max_diff > 100) return fail(BWB_E_ARG, "max_gape/max_diff out of the supported range [0,100]");
	if (p->seed_length < 0 || p->seed_length > 255) return fail(BWB_E_ARG, "seed_length must be in [0,255]");
	if (p->mm_score < 0 || p->gapo_score < 0 || p->gape_score < 0) return fail(BWB_E_ARG, "negative penalties are not supported");
	if (p->mm_score > 255 || p->gapo_score > 255 || p->gape_score > 255) return fail(BWB_E_ARG, "penalties (-M, -O, -E) above 255 are not supported on the GPU path");
	const int nb = (p->max_diff + 1) * p->mm_score + (p->max_gapo + 1) * p->gapo_score + (p->max_gape + 1) * p->gape_score; /* heap_init :513 */
	if (nb < 1 || nb > 1024) return fail(BWB_E_ARG, "score range (heap buckets = (n+1) M + (o+1) O + (e+1) E) must be in [1,1024]");
	if (p->max_entries < 1) return fail(BWB_E_ARG, "max_entries must be positive");
	*nb_out = nb;
	return BWB_OK;
}

static bool any_in_flight(const bwb_hip_ctx *c) {
	for (const Slot &s : c->slots) if (s.submitted && !s.complete) return true;
	return false;
}

static int slot_wait(bwb_hip_ctx *c, int si);

extern "C" int bwb_hip_flush(bwb_hip_ctx *c) {
	if (!c) return fail(BWB_E_ARG, "flush: null context");
	HIPCHK(hipSetDevice(c->device));
	for (int s = 0; s < BWB_MAX_SLOTS; s++)
		if (c->slots[s].submitted && !c->slots[s].complete) RC(slot_wait(c, s));
	HIPCHK(hipStreamSynchronize(c->stream));
	return resolve_times(c, true);
}

extern "C" int bwb_hip_slot_upload(bwb_hip_ctx *c, int si, const bwb_params *p, const uint8_t *reads_fwd, const uint16_t *lens,
                                   uint32_t n_reads, uint32_t stride, const uint8_t *carry_seq, uint32_t carry_len) {
	if (!c || !p || si < 0 || si >= BWB_MAX_SLOTS || (n_reads && (!reads_fwd || !lens)) || stride == 0) return fail(BWB_E_ARG, "slot_upload: bad argument");
	int nb = 0;
	RC(check_params(p, &nb));
	HIPCHK(hipSetDevice(c->device));
	Slot &s = c->slots[si];
	if (s.submitted && !s.complete) RC(slot_wait(c, si)); /* the slot is being reused */
	if (s.uploaded) HIPCHK(hipEventSynchronize(s.ev_up.e)); /* its previous H2D copy has left the pinned staging buffers */
	if (s.calcd_queued && !s.submitted) HIPCHK(hipStreamSynchronize(c->dstream)); /* (uploaded, its kl_calc_d queued ahead, never submitted: that kernel reads the buffers) */
	s.calcd_queued = false;
	/* every slot in flight runs under the same parameters (they are launch arguments) */
	if (c->have_params && memcmp(&c->p, p, sizeof(*p)) != 0 && (any_in_flight(c) || c->parked)) RC(bwb_hip_flush(c));
	/* 32-byte heap entries: more than one gap run per path - and penalties above 63, whose buckets can lie beyond the 64-bucket window of
	 * the non-empty buckets: only these kernels carry the code for that (LHeap::far) */
	const bool wide = p->max_gapo > 1 || p->mm_score > 63 || p->gapo_score > 63 || p->gape_score > 63;
	if (c->cls[0].ready && wide != c->wide && c->parked) RC(bwb_hip_flush(c));
	c->p = *p; c->have_params = true;
	c->kp = KParams{ p->max_diff, p->max_gapo, p->max_gape, p->max_entries, p->mm_score, p->gapo_score, p->gape_score,
	                 p->seed_length, p->max_diff_seed, p->max_best, p->no_indel_length, nb, p->use_precalc ? 1 : 0, p->is_multiref ? 1 : 0 };
	c->wide = wide;

	/* Reads the kernels cannot represent (longer than 255 bases: aln_entry_t.i is 8-bit, align.h:104; shorter than 12 with -P:
	 * read2index, align.c:174-186, reads before the buffer) get an empty record and a warning instead of failing the batch. */
	uint32_t maxlen = 0, n_bad = 0;
	/* D_seed of the reads that are not longer than the seed: that of the last longer read before them (k_dseed_inherit).
	 * `carry` = that read for the head of the batch, when the caller knows one from earlier in the file. */
	const uint32_t sl = (uint32_t)p->seed_length;
	auto is_source = [&](const uint8_t *seq, uint32_t len) { /* computes D_seed (inexact_match.c:62-64) and is not skipped by -P (:50-57) */
		if (!(sl && len > sl) || len > 255) return false;
		if (p->use_precalc) { if (len < PRECALC_LEN) return false; for (int k = 0; k < PRECALC_LEN; k++) if (seq[k] > 3) return false; }
		return true;
	};
	const bool ghost = carry_seq && is_source(carry_seq, carry_len) && n_reads;
	uint32_t last = ghost ? n_reads : NONE32;
	s.inherit = false;
	s.h_src.clear();
	for (uint32_t i = 0; i < n_reads; i++) {
		const bool bad = lens[i] > 255 || lens[i] > stride || (p->use_precalc && lens[i] < PRECALC_LEN);
		if (bad) { n_bad++; continue; }
		maxlen = std::max<uint32_t>(maxlen, lens[i]);
		if (is_source(reads_fwd + (size_t)i * stride, lens[i])) last = i;
		else if (sl && lens[i] <= sl && last != NONE32) {
			if (!s.inherit) { s.h_src.assign(n_reads, NONE32); s.inherit = true; }
			s.h_src[i] = last;
		}
	}
	const bool use_ghost = ghost && s.inherit; /* (the carried read only matters when a short read precedes the batch's first longer one) */
	if (s.inherit && !use_ghost) for (uint32_t i = 0; i < n_reads; i++) if (s.h_src[i] == n_reads) s.h_src[i] = NONE32;
	if (s.inherit) { bool any = false; for (uint32_t v : s.h_src) any |= v != NONE32; s.inherit = any; }
	if (use_ghost) maxlen = std::max<uint32_t>(maxlen, carry_len);
	s.n_tot = n_reads + (use_ghost && s.inherit ? 1u : 0u);
	if (n_bad) fprintf(stderr, "[bwbble_hip] warning: %u read(s) longer than 255 bases%s get an empty alignment record\n", n_bad, p->use_precalc ? " or shorter than 12 (-P)" : "");
	s.n_reads = n_reads; s.stride = std::min<uint32_t>(stride, std::max<uint32_t>(maxlen, 1)); s.maxlen = maxlen;
	s.dstride = REC_BYTES * rec_count(maxlen) + 16; /* per read: its records (bwb_kernels.h: rec_put), then 16 bytes (work, N count) */
	const size_t nr = s.n_tot ? s.n_tot : 1;
	HIPCHK(s.d_reads.reserve(nr * s.stride));
	HIPCHK(s.d_lens.reserve(nr * 2));
	if (c->pileq_on) HIPCHK(s.d_quals.reserve(nr * s.stride)); /* (here, so that ensure_pool counts it with the slot's other buffers) */
	s.up_stride = stride; s.quals_set = false;
	HIPCHK(s.d_dbuf.reserve(nr * s.dstride));
	HIPCHK(s.d_status.reserve(nr));
	HIPCHK(s.d_worklist.reserve(nr * 4));
	HIPCHK(s.d_n.reserve(nr * 4));
	HIPCHK(s.d_off.reserve(nr * 8));
	HIPCHK(s.d_ctl.reserve(256));
	HIPCHK(s.h_ctl.reserve(256));
	HIPCHK(s.ev_up.create());
	const uint64_t want = std::max<uint64_t>((uint64_t)nr * 8, 1u << 16); /* hit log: 8 records per read, grown on demand */
	if (s.log_cap < want) { HIPCHK(s.d_log.alloc(want * sizeof(bwb_aln))); s.log_cap = want; }
	if (c->dbg_iters) { HIPCHK(s.d_dbg_iters.reserve(nr * 4)); HIPCHK(hipMemsetAsync(s.d_dbg_iters.p, 0, nr * 4, c->cstream)); }
	/* staging: the caller's buffers are free again when this returns; the copy to HBM proceeds on the copy stream */
	HIPCHK(s.h_reads.reserve(nr * s.stride));
	HIPCHK(s.h_lens.reserve(nr * 2));
	uint8_t *hr = s.h_reads.as<uint8_t>();
	uint16_t *hl = s.h_lens.as<uint16_t>();
	if (s.stride == stride && !n_bad) { memcpy(hr, reads_fwd, (size_t)n_reads * stride); memcpy(hl, lens, (size_t)n_reads * 2); }
	else
		for (uint32_t i = 0; i < n_reads; i++) {
			const bool bad = lens[i] > 255 || lens[i] > stride || (p->use_precalc && lens[i] < PRECALC_LEN);
			hl[i] = bad ? (uint16_t)BAD_LEN : lens[i];
			memcpy(hr + (size_t)i * s.stride, reads_fwd + (size_t)i * stride, bad ? 0 : lens[i]);
		}
	if (s.n_tot > n_reads) { hl[n_reads] = (uint16_t)carry_len; memcpy(hr + (size_t)n_reads * s.stride, carry_seq, carry_len); }
	if (s.n_tot) {
		HIPCHK(hipMemcpyAsync(s.d_reads.p, hr, (size_t)s.n_tot * s.stride, hipMemcpyHostToDevice, c->cstream));
		HIPCHK(hipMemcpyAsync(s.d_lens.p, hl, (size_t)s.n_tot * 2, hipMemcpyHostToDevice, c->cstream));
	}
	if (s.inherit) {
		HIPCHK(s.d_src.reserve((size_t)n_reads * 4));
		HIPCHK(hipMemcpyAsync(s.d_src.p, s.h_src.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice, c->cstream));
		HIPCHK(hipStreamSynchronize(c->cstream)); /* (h_src is pageable) */
	}
	/* the slot's entry of the device table */
	SlotDesc &d = c->h_descs[si];
	d.b.reads = s.d_reads.as<uint8_t>(); d.b.lens = s.d_lens.as<uint16_t>(); d.b.n_reads = n_reads; d.b.stride = s.stride;
	d.b.dbuf = s.d_dbuf.as<uint8_t>(); d.b.dstride = s.dstride; d.b.status = s.d_status.as<uint8_t>(); d.b.dbg_iters = s.d_dbg_iters.as<uint32_t>();
	d.out.alns = s.d_log.as<uint4>(); d.out.count = s.ctl_count(); d.out.cap = s.log_cap; d.out.off = s.d_off.as<uint64_t>(); d.out.n = s.d_n.as<uint32_t>();
	d.done = s.ctl_done();
	/* (pageable source: the runtime stages it before returning, so h_descs may change again right away) */
	HIPCHK(hipMemcpyAsync(c->d_descs.as<SlotDesc>() + si, &d, sizeof(SlotDesc), hipMemcpyHostToDevice, c->cstream));
	HIPCHK(hipEventRecord(s.ev_up.e, c->cstream));
	s.uploaded = true; s.submitted = false; s.complete = false; s.fetched = false;
	s.stage.reset();
	return ensure_class(c, 0);
}

/* the table as the kernels see it (none: the table of another alphabet, or not built) */
template <typename P> static DTab<P> dtab_of(const bwb_hip_ctx *c) {
	DTab<P> t;
	const bool use = c->dtab_K > 0 && c->dtab_multiref == (c->kp.multiref ? 1 : 0);
	t.ent = use ? c->d_dtab_ent.as<uint4>() : nullptr;
	t.pool = c->d_dtab_pool.as<Intv<P>>();
	t.K = c->dtab_K;
	for (int j = 0; j < 4; j++) t.nm1[j] = c->dtab_nm1[j];
	return t;
}

/* Builds the calculate_d table (bwb_lane.h: DTab, k_dtab_level) for the current alphabet: K levels, each one step from the one before.  The
 * levels' interval lists ping-pong between the two halves of the heap chunk pool, which is idle - nothing is parked, no slot in flight -
 * when this runs (the first large batch of a context); the last level is copied into an allocation of its own size.  A build that does not
 * fit (pool halves, memory) leaves the context without a table: kl_calc_d then computes every step, as before. */
#define DTAB_MIN_READS 200000u
static bool any_in_flight(const bwb_hip_ctx *c);
template <typename P> static int build_dtab_t(bwb_hip_ctx *c, int K) {
	const double t0 = wall_s();
	ScratchClass &sc = c->cls[0];
	const size_t isz = sizeof(Intv<P>);
	/* scratch for the levels' lists: the two halves of the (idle) chunk pool when they are large enough for any index of this size - never more
	 * intervals than one and a half times the BWT's rows plus one per K-mer, 2^30 at most - else (`-n 0` runs keep a small pool) a temporary
	 * allocation of that size; when that fails, whatever the pool offers (a build that outgrows it leaves no table) */
	const size_t need_half = std::min<size_t>((size_t)64 << 24, (size_t)(c->ix.length + c->ix.length / 2) + ((size_t)1 << (2 * K))) * isz;
	DevMem tmp;
	unsigned char *pool0 = c->d_pool.as<unsigned char>();
	size_t half = (c->d_pool.bytes / 2) & ~(size_t)255;
	if (half < need_half) {
		if (tmp.alloc(2 * need_half) == hipSuccess) { pool0 = tmp.as<unsigned char>(); half = need_half; }
		else (void)hipGetLastError();
	}
	const unsigned long long cap = half / isz;
	DevMem entA, entB, bump;
	const size_t nK = (size_t)1 << (2 * K);
	HIPCHK(entA.alloc(nK * 32));
	HIPCHK(entB.alloc(std::max<size_t>(nK / 4, 1) * 32));
	HIPCHK(bump.alloc(8));
	unsigned char *pool1 = pool0 + half;
	/* level 0: the empty suffix - one interval, the whole index; no restart, no visit */
	const Intv<P> root{ (P)0, (P)(c->ix.length - 1) };
	const uint4 e0[2] = { make_uint4(0u, (1u << 15) | (1u << 16), 0u, 0u), make_uint4(0u, 0u, 0u, 0u) };
	/* levels alternate between the entry arrays so that level K lands in entA, and between the pool halves */
	DevMem *ent_of[2] = { (K & 1) ? &entB : &entA, (K & 1) ? &entA : &entB }; /* ent_of[k & 1] */
	unsigned char *pool_of[2] = { pool0, pool1 };
	HIPCHK(hipMemcpyAsync(ent_of[0]->p, e0, sizeof(e0), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(pool_of[0], &root, sizeof(root), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	const uint32_t grid = (uint32_t)(c->num_cu * c->bpc_calcd);
	unsigned long long total = 0;
	for (int k = 1; k <= K; k++) {
		HIPCHK(hipMemsetAsync(bump.p, 0, 8, c->stream));
		const uint64_t tasks = 1ull << (2 * k);
		const uint32_t g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(grid, (tasks + LANE_BLOCK - 1) / LANE_BLOCK));
		hipLaunchKernelGGL(k_dtab_level<P>, dim3(g), dim3(LANE_BLOCK), calcd_lds(), c->stream, c->ix, c->kp.multiref, k, ent_of[(k - 1) & 1]->template as<uint4>(),
		                   (const Intv<P> *)pool_of[(k - 1) & 1], ent_of[k & 1]->template as<uint4>(), (Intv<P> *)pool_of[k & 1], bump.as<unsigned long long>(), cap, sc.sc);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(c->stream)); /* (the level is complete: its interval count) */
		RC(fetch(c, &total, bump.p, 8));
		if (k == 1) { /* the first step's summed width by base: what a lookup after a restart compares the restart's width with */
			uint4 e1[8];
			RC(fetch(c, e1, ent_of[1]->p, sizeof(e1)));
			for (int j = 0; j < 4; j++) c->dtab_nm1[j] = e1[2 * j].z;
		}
		if (total > cap) {
			if (c->dbg) fprintf(stderr, "[bwb] calculate_d table: level %d needs %llu intervals, the scratch holds %llu: no table\n", k, total, cap);
			c->dtab_failed = true;
			return BWB_OK;
		}
	}
	/* the last level's lists into their own allocation (+ 64 bytes: kl_calc_d reads a list in groups of four intervals) */
	if (c->d_dtab_pool.alloc((size_t)total * isz + 64) != hipSuccess) { (void)hipGetLastError(); c->dtab_failed = true; return BWB_OK; }
	HIPCHK(hipMemcpyAsync(c->d_dtab_pool.p, pool_of[K & 1], (size_t)total * isz, hipMemcpyDeviceToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->d_dtab_ent.release();
	std::swap(c->d_dtab_ent.p, entA.p); std::swap(c->d_dtab_ent.bytes, entA.bytes);
	c->dtab_K = K; c->dtab_multiref = c->kp.multiref ? 1 : 0;
	c->dtab_seconds = wall_s() - t0;
	if (c->dbg) fprintf(stderr, "[bwb] calculate_d table: K = %d, %llu intervals (%.2f GB + %.2f GB of entries), built in %.3f s\n", K, total, (double)total * isz / (1u << 30),
	                    (double)nK * 32 / (1u << 30), c->dtab_seconds);
	return BWB_OK;
}
static int ensure_dtab(bwb_hip_ctx *c, uint32_t n_reads) {
	if (c->dtab_mode == 0 || c->dtab_failed) return BWB_OK;
	if (c->dtab_K && c->dtab_multiref == (c->kp.multiref ? 1 : 0)) return BWB_OK;
	if (c->dtab_mode < 0 && n_reads < DTAB_MIN_READS) return BWB_OK;
	if (c->parked || any_in_flight(c) || !c->d_pool.p || !c->cls[0].ready) return BWB_OK; /* (the pool and the list scratch must be idle: next chance at the next idle submit) */
	if (c->dstream) HIPCHK(hipStreamSynchronize(c->dstream));
	HIPCHK(hipStreamSynchronize(c->stream));
	int K = DTAB_KMAX;
	if (getenv("BWB_DTAB_K")) K = std::max(1, std::min(DTAB_KMAX, atoi(getenv("BWB_DTAB_K"))));
	if (c->dtab_K) { c->d_dtab_ent.release(); c->d_dtab_pool.release(); c->dtab_K = 0; } /* (another alphabet) */
	return with_pos(c, [&](auto p) { return build_dtab_t<decltype(p)>(c, K); });
}

/* BWB_LAUNCH_LOG: what ONE launch did - its HIP-event time and the counters it added (buckets fetched, heap entries stored / loaded, records
 * loaded) - so that per-dispatch PMC counters (tools/pmc_traffic.sh) can be priced launch by launch, slices and the draining launch apart */
static int log_launch(bwb_hip_ctx *c, const char *kernel, int k, int si, bool drains, const Timed &t) {
	HIPCHK(hipStreamSynchronize(t.st));
	float ms = 0;
	RC(t.ms(&ms));
	unsigned long long cur[16];
	RC(fetch(c, cur, c->d_stats.p, sizeof(cur)));
	if (FILE *f = fopen(c->launch_log, "a")) {
		auto d = [&](int i) { return cur[i] - c->log_prev[i]; };
		fprintf(f, "{\"kernel\": \"%s\", \"class\": %d, \"slot\": %d, \"drains\": %s, \"ms\": %.3f, \"buckets\": %llu, \"entries_stored\": %llu, \"entries_loaded\": %llu, \"records_loaded\": %llu}\n",
		        kernel, k, si, drains ? "true" : "false", ms, d(kernel[3] == 'c' ? STAT_BKT_CALCD : STAT_BKT_SEARCH), d(STAT_ENT_ST), d(STAT_ENT_LD), d(STAT_REC_LD));
		fclose(f);
	}
	memcpy(c->log_prev, cur, sizeof(cur));
	return BWB_OK;
}

static int launch_calc_d(bwb_hip_ctx *c, int k, int si, const uint32_t *wl, uint32_t n_work, uint32_t *counter, int32_t *dbgD, int32_t *dbgDs, hipStream_t st = nullptr) {
	ScratchClass &sc = c->cls[k];
	Slot &s = c->slots[si];
	if (!st) st = c->stream;
	Work wk{ wl, n_work, counter, (uint32_t)si, 0, 0, 0 };
	HIPCHK(hipMemsetAsync(counter, 0, 4, st));
	const uint32_t maxb = k == 0 ? (uint32_t)(c->num_cu * c->bpc_calcd) : sc.blocks;
	const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(maxb, (n_work + LANE_BLOCK - 1) / LANE_BLOCK));
	const size_t lds = calcd_lds();
	Timed t(c, st);
	RC(t.begin());
	with_pos(c, [&](auto p) {
		hipLaunchKernelGGL(kl_calc_d<decltype(p)>, dim3(grid), dim3(LANE_BLOCK), lds, st, c->ix, c->h_descs[si].b, wk, c->kp, sc.sc, dbgD, dbgDs,
		                   s.maxlen + 1, (uint32_t)c->kp.seed_length + 1, c->d_stats.as<unsigned long long>(), dtab_of<decltype(p)>(c));
	});
	HIPCHK(hipGetLastError());
	RC(t.end());
	t.defer(0);
	if (c->dbg) {
		HIPCHK(hipStreamSynchronize(st));
		float ms = 0;
		RC(t.ms(&ms));
		fprintf(stderr, "[bwb] kl_calc_d class %d slot %d: %u reads, grid %u, %.3f ms\n", k, si, n_work, grid, ms);
	}
	if (c->launch_log) return log_launch(c, "kl_calc_d", k, si, false, t);
	return BWB_OK;
}

/* reads not longer than the seed take the D_seed bounds of the last longer read before them (k_dseed_inherit) */
static int launch_inherit(bwb_hip_ctx *c, int si, hipStream_t st = nullptr) {
	Slot &s = c->slots[si];
	if (!s.inherit) return BWB_OK;
	hipLaunchKernelGGL(k_dseed_inherit, dim3((s.n_reads + 255) / 256), dim3(256), 0, st ? st : c->stream, c->h_descs[si].b, s.d_src.as<uint32_t>(), s.n_reads);
	HIPCHK(hipGetLastError());
	return BWB_OK;
}

/* one launch of kl_search in class k: new reads come from `wl`/`n_work` of slot si (n_work 0: only parked reads progress) */
static int launch_search(bwb_hip_ctx *c, int k, int si, const uint32_t *wl, uint32_t n_work, uint32_t *counter, bool suspend, bool reset_counter = true,
                         bool force_drain = false) {
	ScratchClass &s = c->cls[k];
	const bool resume = k == 0 && c->parked;
	if (k != 0 && c->parked) return fail(BWB_E_STATE, "a re-run class was launched while reads are parked");
	const uint32_t slice_iters = (k == 0 && !force_drain) ? c->slice_iters : 0; /* (force_drain: also the time-sliced test mode runs to the end) */
	Work wk{ wl, n_work, counter, (uint32_t)si, suspend ? 1u : 0u, slice_iters, resume ? 1u : 0u };
	const size_t lds = lane_lds(c);
	unsigned int *bump = c->d_pool_bump.as<unsigned int>() + (k == 0 ? 0 : POOL_REGIONS * 16);
	if (reset_counter) HIPCHK(hipMemsetAsync(counter, 0, 4, c->stream));
	if (!resume) HIPCHK(hipMemsetAsync(bump, 0, POOL_REGIONS * 64, c->stream)); /* nothing is parked: the launch starts with an empty chunk pool */
	/* class 0 always runs its full grid: every lane's save word is rewritten by every launch, and the pool geometry
	 * (regions, private runs) must not change while reads are parked */
	const uint32_t grid = k == 0 ? (uint32_t)(c->num_cu * c->bpc_search) : std::max<uint32_t>(1, std::min<uint32_t>(s.blocks, (n_work + LANE_BLOCK - 1) / LANE_BLOCK));
	DevMem &pool = c->d_pool;
	s.sc.pool = pool.as<uint4>(); s.sc.pool_bump = bump;
	/* one region per 8 blocks up to POOL_REGIONS, so that the few blocks of a small launch (class 2) are not confined to
	 * a fraction of the pool; a state word names 2^26 chunks of its region */
	s.sc.n_regions = std::max<uint32_t>(1, std::min<uint32_t>(POOL_REGIONS, grid / 8));
	s.sc.region_u4 = pool.bytes / s.sc.n_regions / 4096 * 256;
	s.sc.pool_cap = (uint32_t)std::min<size_t>(s.sc.region_u4 * 16 / (c->wide ? 2048 : 1024), (size_t)1 << 26);
	{ /* private runs take at most three quarters of a region */
		const uint32_t lanes = (grid + s.sc.n_regions - 1) / s.sc.n_regions * LANE_BLOCK;
		s.sc.keep = std::min<uint32_t>(c->keep, s.sc.pool_cap / 4 * 3 / lanes);
	}
	Timed t(c, c->stream);
	RC(t.begin());
	const SlotDesc *descs = c->d_descs.as<SlotDesc>();
	unsigned long long *st = c->d_stats.as<unsigned long long>();
	/* position width x 32-byte entries x the IUPAC alphabet: the one place that picks among the eight instantiations */
	with_pos(c, [&](auto p) { with_flag(c->wide, [&](auto w) { with_flag(c->kp.multiref != 0, [&](auto m) {
		hipLaunchKernelGGL((kl_search<decltype(p), decltype(w)::value, decltype(m)::value>), dim3(grid), dim3(LANE_BLOCK), lds, c->stream, c->ix, descs, wk, c->kp, s.sc, st);
	}); }); });
	HIPCHK(hipGetLastError());
	RC(t.end());
	t.defer(1);
	if (k == 0) {
		c->parked = suspend || slice_iters != 0;
		hipEvent_t le = get_event(c);
		if (!le) return fail(BWB_E_HIP, "hipEventCreate failed");
		HIPCHK(hipEventRecord(le, c->stream));
		c->launch_ev.push_back(le);
		c->n_launches++;
		/* slot_wait starts at the slot's own launch: events of launches before the oldest slot in flight are never needed again */
		uint64_t oldest = c->n_launches;
		for (const Slot &t : c->slots) if (t.submitted && !t.complete && t.launch) oldest = std::min(oldest, t.launch);
		size_t drop = 0;
		while (c->ev_base + drop + 1 < oldest && drop < c->launch_ev.size()) c->free_events.push_back(c->launch_ev[drop++]);
		if (drop) { c->launch_ev.erase(c->launch_ev.begin(), c->launch_ev.begin() + (long)drop); c->ev_base += drop; }
	}
	if (c->dbg) {
		HIPCHK(hipStreamSynchronize(c->stream));
		float ms = 0;
		RC(t.ms(&ms));
		unsigned int hb[POOL_REGIONS * 16], used_max = 0;
		unsigned long long used = 0;
		RC(fetch(c, hb, bump, sizeof(hb)));
		const uint32_t priv = (grid + s.sc.n_regions - 1) / s.sc.n_regions * LANE_BLOCK * s.sc.keep;
		for (uint32_t r = 0; r < s.sc.n_regions; r++) { used += std::min(priv + hb[r * 16], s.sc.pool_cap); used_max = std::max(used_max, priv + hb[r * 16]); }
		fprintf(stderr, "[bwb] kl_search class %d slot %d: %u new reads, grid %u, %s%s, %.3f ms, pool chunks used %llu of %d x %u (fullest region asked for %u; %u private per lane)\n",
		        k, si, n_work, grid, suspend ? "slice (parks)" : "drains", resume ? ", resumes parked reads" : "", ms, used, (int)s.sc.n_regions, s.sc.pool_cap, used_max, s.sc.keep);
	}
	if (c->launch_log) return log_launch(c, "kl_search", k, si, !(suspend || slice_iters != 0), t);
	return BWB_OK;
}

/* kl_calc_d (+ the D_seed inheritance) of an uploaded slot on the second kernel stream, ahead of the slot's submit */
static int queue_calc_d(bwb_hip_ctx *c, int si) {
	Slot &s = c->slots[si];
	HIPCHK(s.ev_calcd.create());
	HIPCHK(hipStreamWaitEvent(c->dstream, s.ev_up.e, 0));
	HIPCHK(hipMemsetAsync(s.d_status.p, 0, (size_t)s.n_tot, c->dstream));
	RC(launch_calc_d(c, 0, si, nullptr, s.n_tot, s.ctl_counter(), nullptr, nullptr, c->dstream));
	RC(launch_inherit(c, si, c->dstream));
	HIPCHK(hipEventRecord(s.ev_calcd.e, c->dstream));
	s.calcd_queued = true;
	return BWB_OK;
}

static int submit(bwb_hip_ctx *c, int si, bool suspend) {
	Slot &s = c->slots[si];
	if (!s.uploaded) return fail(BWB_E_STATE, "slot_submit: nothing uploaded into this slot");
	if (s.submitted && !s.complete) return fail(BWB_E_STATE, "slot_submit: the slot is still in flight");
	RC(index_ready(c)); /* (a context created with bwb_hip_ctx_create_async: its index upload may still be running) */
	RC(ensure_class(c, 0));
	RC(ensure_dtab(c, s.n_reads));
	HIPCHK(hipStreamWaitEvent(c->stream, s.ev_up.e, 0));
	const bool ahead = c->calcd_ahead > 0 && s.n_reads != 0;
	if (ahead) { /* kl_calc_d of this batch runs (or has run) on the second kernel stream: the search waits for it (the slot's cursor is its cursor too) */
		if (!s.calcd_queued) RC(queue_calc_d(c, si));
		HIPCHK(hipStreamWaitEvent(c->stream, s.ev_calcd.e, 0));
	}
	HIPCHK(hipMemsetAsync(s.d_ctl.p, 0, 256, c->stream));
	s.submitted = true; s.complete = false; s.fetched = false; s.launch = 0;
	s.stage.reset();
	if (s.n_reads == 0) { s.complete = true; s.launch = c->n_launches; return BWB_OK; }
	HIPCHK(hipMemsetAsync(s.d_n.p, 0, (size_t)s.n_reads * 4, c->stream));
	if (!ahead) {
		HIPCHK(hipMemsetAsync(s.d_status.p, 0, (size_t)s.n_tot, c->stream));
		RC(launch_calc_d(c, 0, si, nullptr, s.n_tot, s.ctl_counter(), nullptr, nullptr));
		RC(launch_inherit(c, si));
	}
	RC(launch_search(c, 0, si, nullptr, s.n_reads, s.ctl_counter(), suspend));
	s.launch = c->n_launches;
	/* the batches the caller has uploaded beyond this one (slots are used round-robin): their kl_calc_d is queued NOW, on the second
	 * stream, where it runs beside the search slices instead of in front of its own (the two calls are independent per read,
	 * inexact_match.c:140-144, and kl_calc_d has its own lists) */
	for (int k = 1; ahead && k <= c->calcd_ahead; k++) {
		const int sj = (si + k) % BWB_MAX_SLOTS;
		Slot &t = c->slots[sj];
		if (t.uploaded && !t.submitted && !t.calcd_queued && t.n_reads) RC(queue_calc_d(c, sj));
	}
	return BWB_OK;
}

extern "C" int bwb_hip_slot_submit(bwb_hip_ctx *c, int si) {
	if (!c || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_submit: bad argument");
	HIPCHK(hipSetDevice(c->device));
	return submit(c, si, true);
}

/* the first n status bytes of the slot -> s.h_status (n_reads, or n_tot: a carried read that rides along for its D_seed can overflow
 * calculate_d too; it is never searched) */
static int load_status(bwb_hip_ctx *c, Slot &s, uint32_t n) {
	s.h_status.resize(n);
	return fetch(c, s.h_status.data(), s.d_status.p, n);
}

/* ids -> the slot's device worklist; there when this returns */
static int put_worklist(bwb_hip_ctx *c, Slot &s, const std::vector<uint32_t> &ids) {
	HIPCHK(hipMemcpyAsync(s.d_worklist.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return BWB_OK;
}

/* reads of the slot whose status == want -> the slot's device worklist */
static int collect(bwb_hip_ctx *c, Slot &s, uint8_t want, std::vector<uint32_t> &ids) {
	RC(load_status(c, s, s.n_reads));
	ids.clear();
	for (uint32_t i = 0; i < s.n_reads; i++) if (s.h_status[i] == want) ids.push_back(i);
	return ids.empty() ? BWB_OK : put_worklist(c, s, ids);
}

/* grows the slot's hit log (keeping what is in it) */
static int grow_log(bwb_hip_ctx *c, int si) {
	Slot &s = c->slots[si];
	unsigned long long cnt = 0;
	RC(fetch(c, &cnt, s.ctl_count(), 8));
	const uint64_t valid = std::min<uint64_t>(cnt, s.log_cap);
	const uint64_t ncap = s.log_cap * 4;
	DevMem nl;
	HIPCHK(nl.alloc(ncap * sizeof(bwb_aln)));
	HIPCHK(hipMemcpyAsync(nl.p, s.d_log.p, valid * sizeof(bwb_aln), hipMemcpyDeviceToDevice, c->stream));
	cnt = valid;
	HIPCHK(hipMemcpyAsync(s.ctl_count(), &cnt, 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	std::swap(s.d_log.p, nl.p); std::swap(s.d_log.bytes, nl.bytes);
	s.log_cap = ncap;
	c->h_descs[si].out.alns = s.d_log.as<uint4>(); c->h_descs[si].out.cap = ncap;
	HIPCHK(hipMemcpyAsync(c->d_descs.as<SlotDesc>() + si, &c->h_descs[si], sizeof(SlotDesc), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return BWB_OK;
}

/* Re-runs, in the larger scratch classes, the reads of a finished slot that did not fit class 0: an SA-interval list or the
 * hit list overflowed, the chunk pool was empty when the read needed it, or the slot's hit log was full.  Draining launches
 * on the kernel stream (behind whatever slices are queued there). */
static int rerun_overflows(bwb_hip_ctx *c, int si) {
	Slot &s = c->slots[si];
	std::vector<uint32_t> todo, dids, list;
	/* The re-run classes take the whole chunk pool (a read that found it empty among 131 072 others gets, in class 1, four times
	 * its share and in class 2 a five-hundredth of the pool to itself).  So whatever is parked must finish first: one draining
	 * launch (fed from this slot's exhausted cursor) completes the parked reads of every slot. */
	if (c->parked) {
		RC(launch_search(c, 0, si, nullptr, s.n_reads, s.ctl_counter(), false, false, true));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	for (int k = 1; k <= 2; k++) {
		RC(load_status(c, s, s.n_tot));
		todo.clear(); dids.clear();
		for (uint32_t i = 0; i < s.n_tot; i++) {
			if (s.h_status[i] != ST_OK && i < s.n_reads) todo.push_back(i);
			if (s.h_status[i] == ST_D_OVF) dids.push_back(i);
		}
		if (todo.empty()) return BWB_OK;
		if (k == 1) c->stats.n_overflow_reads += todo.size(); /* (class 2 re-runs a subset of these) */
		RC(ensure_class(c, k));
		if (!dids.empty()) { /* calculate_d first: it leaves ST_OK, or ST_D_OVF again (then the next class tries); ST_D_WAIT reads only need the inheritance */
			RC(put_worklist(c, s, dids));
			RC(launch_calc_d(c, k, si, s.d_worklist.as<uint32_t>(), (uint32_t)dids.size(), s.ctl_counter2(), nullptr, nullptr));
			RC(launch_inherit(c, si)); /* sources that were late are there now (a read whose source still is not stays ST_D_WAIT) */
			HIPCHK(hipStreamSynchronize(c->stream));
			RC(load_status(c, s, s.n_tot));
		}
		list.clear();
		for (uint32_t i : todo) if (s.h_status[i] < ST_D_OVF) list.push_back(i);
		for (int guard = 0; !list.empty(); guard++) {
			if (guard == 40) return fail(BWB_E_OVERFLOW, "hit log kept overflowing");
			bool out_ovf = false;
			for (uint32_t i : list) out_ovf |= s.h_status[i] == ST_OUT_OVF;
			if (out_ovf) RC(grow_log(c, si));
			RC(put_worklist(c, s, list));
			RC(launch_search(c, k, si, s.d_worklist.as<uint32_t>(), (uint32_t)list.size(), s.ctl_counter2(), false));
			HIPCHK(hipStreamSynchronize(c->stream));
			RC(load_status(c, s, s.n_tot));
			/* only reads the hit log had no room for are repeated within a class (the log grows x4 each time) */
			std::vector<uint32_t> again;
			for (uint32_t i : list) if (s.h_status[i] == ST_OUT_OVF) again.push_back(i);
			list.swap(again);
		}
	}
	RC(load_status(c, s, s.n_tot));
	for (uint32_t i = 0; i < s.n_tot; i++)
		if (s.h_status[i] != ST_OK) return fail(BWB_E_OVERFLOW, "a read exceeded the largest per-read scratch class");
	return BWB_OK;
}

static int slot_wait(bwb_hip_ctx *c, int si) {
	Slot &s = c->slots[si];
	if (!s.submitted) return fail(BWB_E_STATE, "slot_wait: the slot has not been submitted");
	if (s.complete) return BWB_OK;
	/* A slice leaves the slot's unfinished reads parked; the slice after it resumes them and normally finishes them long
	 * before it ends.  So: wait for the slot's own slice; if reads are left, for the next queued one; and when nothing is
	 * queued any more, launch a draining slice. */
	uint64_t L = s.launch;
	for (;;) {
		HIPCHK(hipEventSynchronize(c->launch_ev[L - 1 - c->ev_base]));
		unsigned int done = 0;
		RC(fetch(c, &done, s.ctl_done(), 4));
		if (done >= s.n_reads) break;
		if (L < c->n_launches) { L++; continue; }
		/* (the slot's cursor is where the slices left it: normally exhausted, so only parked reads run) */
		RC(launch_search(c, 0, si, nullptr, s.n_reads, s.ctl_counter(), false, false));
		L = c->n_launches;
	}
	RC(resolve_times(c, false));
	/* anything that needs a larger scratch class?  (one byte per read; almost always all zero) */
	RC(load_status(c, s, s.n_tot));
	bool clean = true;
	for (uint32_t i = 0; i < s.n_tot && clean; i++) clean = s.h_status[i] == ST_OK;
	if (!clean) RC(rerun_overflows(c, si));
	s.complete = true;
	if (!any_in_flight(c)) c->parked = false; /* every read of every submitted slot is done: nothing can be parked any more */
	return BWB_OK;
}

extern "C" int bwb_hip_slot_wait(bwb_hip_ctx *c, int si) {
	if (!c || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_wait: bad argument");
	HIPCHK(hipSetDevice(c->device));
	return slot_wait(c, si);
}

extern "C" int bwb_hip_slot_result(bwb_hip_ctx *c, int si, bwb_result *out) {
	if (!c || !out || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_result: bad argument");
	HIPCHK(hipSetDevice(c->device));
	Slot &s = c->slots[si];
	if (!s.submitted) return fail(BWB_E_STATE, "slot_result: the slot has not been submitted");
	RC(slot_wait(c, si));
	const uint32_t n = s.n_reads;
	if (!s.fetched) {
		/* per-read counts and offsets into the hit log, and the log itself, on the result stream (the kernel stream keeps running) */
		unsigned long long cnt = 0;
		if (n) {
			HIPCHK(s.h_cnt.reserve((size_t)n * 4));
			HIPCHK(s.h_off.reserve((size_t)n * 8));
			HIPCHK(hipMemcpyAsync(s.h_cnt.p, s.d_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->rstream));
			HIPCHK(hipMemcpyAsync(s.h_off.p, s.d_off.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->rstream));
			HIPCHK(hipMemcpyAsync(s.h_ctl.p, s.ctl_count(), 8, hipMemcpyDeviceToHost, c->rstream));
			HIPCHK(hipStreamSynchronize(c->rstream));
			cnt = std::min<unsigned long long>(*s.h_ctl.as<unsigned long long>(), s.log_cap);
			if (cnt) {
				HIPCHK(s.h_log.reserve((size_t)cnt * sizeof(bwb_aln)));
				HIPCHK(hipMemcpyAsync(s.h_log.p, s.d_log.p, (size_t)cnt * sizeof(bwb_aln), hipMemcpyDeviceToHost, c->rstream));
				HIPCHK(hipStreamSynchronize(c->rstream));
			}
		}
		/* into read order (the log is in completion order; a read's hits are contiguous and in discovery order) */
		const uint32_t *hc = s.h_cnt.as<uint32_t>();
		const uint64_t *ho = s.h_off.as<uint64_t>();
		const bwb_aln *hl = s.h_log.as<bwb_aln>();
		s.h_aln_off.assign((size_t)n + 1, 0);
		for (uint32_t i = 0; i < n; i++) s.h_aln_off[i + 1] = s.h_aln_off[i] + hc[i];
		const uint64_t total = s.h_aln_off[n];
		s.h_alns.resize(total ? total : 1);
		for (uint32_t i = 0; i < n; i++) {
			if (!hc[i]) continue;
			if (ho[i] + hc[i] > cnt) return fail(BWB_E_STATE, "slot_result: a read's hits lie outside the hit log");
			memcpy(&s.h_alns[s.h_aln_off[i]], hl + ho[i], (size_t)hc[i] * sizeof(bwb_aln));
		}
		s.fetched = true;
	}
	out->n_reads = n;
	out->aln_off = s.h_aln_off.data();
	out->alns = s.h_alns.data();
	return BWB_OK;
}

/* ---- the one-batch interface: slot 0, one draining launch ------------------------------------------------------ */
extern "C" int bwb_hip_batch_upload(bwb_hip_ctx *c, const bwb_params *p, const uint8_t *reads_fwd, const uint16_t *lens,
                                    uint32_t n_reads, uint32_t stride) {
	if (!c) return fail(BWB_E_ARG, "batch_upload: null context");
	RC(bwb_hip_flush(c)); /* this interface owns the context: nothing else may be in flight */
	RC(bwb_hip_slot_upload(c, 0, p, reads_fwd, lens, n_reads, stride, nullptr, 0));
	HIPCHK(hipStreamSynchronize(c->cstream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return BWB_OK;
}

static int read_device_stats(bwb_hip_ctx *c) {
	unsigned long long st[STAT_WORDS];
	RC(fetch(c, st, c->d_stats.p, sizeof(st)));
	c->stats.visits_single = st[STAT_VIS_SINGLE]; c->stats.visits_alphabet = st[STAT_VIS_ALPHA]; c->stats.visits_calc_d = st[STAT_VIS_CALCD];
	c->stats.heap_pops = st[STAT_POPS]; c->stats.heap_pushes = st[STAT_PUSHES]; c->stats.n_alignments = st[STAT_ALNS];
	c->stats.bucket_loads_search = st[STAT_BKT_SEARCH]; c->stats.bucket_loads_calc_d = st[STAT_BKT_CALCD];
	c->stats.n_parked_reads = st[STAT_PARKED];
	c->stats.lane_iterations = st[STAT_N]; c->stats.wave_iterations = st[STAT_WAVE_ITERS];
	c->stats.heap_entries_stored = st[STAT_ENT_ST]; c->stats.heap_entries_loaded = st[STAT_ENT_LD]; c->stats.record_loads = st[STAT_REC_LD];
#ifdef BWB_HIST
	{
		static const char *hn[H_N] = { "iter", "pop", "pop_from_mirror", "pop_gapped", "pruned", "hit", "exact_start", "expand", "exact_step", "need_rank", "same_bkt", "two_bkt",
			"w1", "w2", "w3_4", "w5_8", "w9_32", "w33_128", "w_big", "ne0", "ne1", "ne2", "ne3_4", "ne5_8", "ne9+", "push_gap", "push_mis", "push_match",
			"del_ok", "mm_ok", "ins_ok", "top_reload", "wave_iters", "wave_gaploop_trips", "wave_misloop_trips", "wave_matchloop_trips", "wave_any_two_bkt", "wave_any_wide8",
			"wave_nreq_le16", "alpha", "exact_multi", "finish", "group_pops", "wave_any_exact", "wave_any_expand", "wave_all_exact", "exp_same_w1", "exp_same_w2_4", "count_only_gap", "count_only_mis", "count_only_pop", "expand_after_hit",
			"list_st_first", "list_st_second", "list_st_merge", "list_st_interior", "list_ld" };
		fprintf(stderr, "[bwb hist]");
		for (int k = 0; k < H_N; k++) fprintf(stderr, " %s=%llu", hn[k], st[STAT_HIST + k]);
		fprintf(stderr, "\n");
	}
#endif
#ifdef BWB_BBPROF
	if (const char *bo = getenv("BWB_BBPROF_OUT")) { /* tools/bbprof.py: the basic-block counters of the instrumented kernels, one JSON line per call */
		if (FILE *f = fopen(bo, "a")) {
			fprintf(f, "{\"wave_iterations_search\": %llu, \"wave_iterations_calc_d\": %llu, \"lane_iterations_search\": %llu, \"counters\": [", st[STAT_WAVE_ITERS], st[STAT_WAVE_ITERS_CALCD], st[STAT_N]);
			for (int k = 0; k < 2048; k++) fprintf(f, "%s%llu", k ? "," : "", st[STAT_BBPROF + k]);
			fprintf(f, "]}\n");
			fclose(f);
		}
	}
#endif
#ifdef BWB_STAMPS
	if (st[STAT_STAMPS + 3]) {
		double tot = 0; for (int k = 0; k < 16; k++) tot += (double)st[STAT_STAMPS + k];
		const char *nm[16] = { "top", "A(pop)", "B(issue)", "C(rank)", "D.tail", "E.top-reload", "E.exact-step", "F(finish,grab)", "D.prune/hit", "D.masks", "D.reserve", "D.templates", "D.gap", "D.mm/match", "C.gather(exchange,loads,wait)", "E.exact-done/hits" };
		fprintf(stderr, "[bwb] stamps (%% of lane cycles):");
		for (int k = 0; k < 16; k++) if (st[STAT_STAMPS + k]) fprintf(stderr, " %s %.1f |", nm[k], 100.0 * (double)st[STAT_STAMPS + k] / tot);
		fprintf(stderr, "\n");
	}
#endif
	if (c->dbg) {
		fprintf(stderr, "[bwb] search loop iterations: total %llu, wave iterations %llu (%.1f of 64 lanes busy), reads parked at slice ends %llu\n",
		        st[STAT_N], st[STAT_WAVE_ITERS], st[STAT_WAVE_ITERS] ? (double)st[STAT_N] / (double)st[STAT_WAVE_ITERS] : 0.0, st[STAT_PARKED]);
	}
	return BWB_OK;
}

extern "C" int bwb_hip_reset_stats(bwb_hip_ctx *c) {
	if (!c) return fail(BWB_E_ARG, "reset_stats: null context");
	HIPCHK(hipSetDevice(c->device));
	RC(resolve_times(c, false));
	memset(&c->stats, 0, sizeof(c->stats));
	memset(c->log_prev, 0, sizeof(c->log_prev));
	HIPCHK(hipMemsetAsync(c->d_stats.p, 0, sizeof(unsigned long long) * STAT_WORDS, c->stream));
	c->t_run0 = wall_s();
	return BWB_OK;
}

extern "C" int bwb_hip_batch_run(bwb_hip_ctx *c) {
	if (!c || !c->slots[0].uploaded) return fail(BWB_E_STATE, "batch_run: no batch uploaded");
	HIPCHK(hipSetDevice(c->device));
	RC(bwb_hip_flush(c));
	RC(bwb_hip_reset_stats(c));
	const double t0 = wall_s();
	RC(submit(c, 0, c->force_slices));
	RC(slot_wait(c, 0));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->stats.ms_total = (wall_s() - t0) * 1e3;
	RC(resolve_times(c, true));
	return read_device_stats(c);
}

/* totals since the last reset_stats / batch_run; kernel times cover the launches that have finished */
extern "C" int bwb_hip_get_stats(bwb_hip_ctx *c, bwb_stats *out) {
	if (!c || !out) return fail(BWB_E_ARG, "get_stats: null argument");
	HIPCHK(hipSetDevice(c->device));
	RC(resolve_times(c, false));
	RC(read_device_stats(c));
	*out = c->stats;
	return BWB_OK;
}

extern "C" int bwb_hip_batch_result(bwb_hip_ctx *c, bwb_result *out) {
	if (!c || !out) return fail(BWB_E_ARG, "batch_result: null argument");
	if (!c->slots[0].submitted || !c->slots[0].complete) return fail(BWB_E_STATE, "batch_result: batch_run has not completed");
	return bwb_hip_slot_result(c, 0, out);
}

extern "C" int bwb_hip_align_batch(bwb_hip_ctx *c, const bwb_params *p, const uint8_t *reads_fwd, const uint16_t *lens,
                                   uint32_t n_reads, uint32_t stride, bwb_result *out) {
	if (!c) return fail(BWB_E_ARG, "align_batch: null context");
	double t0 = wall_s();
	RC(bwb_hip_batch_upload(c, p, reads_fwd, lens, n_reads, stride));
	const double t1 = wall_s();
	RC(bwb_hip_batch_run(c));
	const double t2 = wall_s();
	const int rc = bwb_hip_batch_result(c, out);
	if (c->dbg) fprintf(stderr, "[bwb] align_batch: upload %.3f s, run %.3f s, result %.3f s\n", t1 - t0, t2 - t1, wall_s() - t2);
	return rc;
}

extern "C" int bwb_hip_calc_d(bwb_hip_ctx *c, int32_t *out_D, int32_t *out_Dseed) {
	if (!c || !out_D || !out_Dseed) return fail(BWB_E_ARG, "calc_d: null argument");
	Slot &s = c->slots[0];
	if (!s.uploaded) return fail(BWB_E_STATE, "calc_d: no batch uploaded");
	HIPCHK(hipSetDevice(c->device));
	RC(bwb_hip_flush(c));
	RC(index_ready(c));
	const size_t nD = (size_t)s.n_reads * (s.maxlen + 1) * 2, nS = (size_t)s.n_reads * (c->kp.seed_length + 1) * 2;
	DevMem dD, dS;
	HIPCHK(dD.alloc((nD ? nD : 1) * 4));
	HIPCHK(dS.alloc((nS ? nS : 1) * 4));
	HIPCHK(hipMemsetAsync(dD.p, 0, (nD ? nD : 1) * 4, c->stream));
	HIPCHK(hipMemsetAsync(dS.p, 0, (nS ? nS : 1) * 4, c->stream));
	RC(bwb_hip_reset_stats(c));
	if (s.n_reads) {
		HIPCHK(hipStreamWaitEvent(c->stream, s.ev_up.e, 0));
		HIPCHK(hipMemsetAsync(s.d_status.p, 0, s.n_reads, c->stream));
		RC(launch_calc_d(c, 0, 0, nullptr, s.n_reads, s.ctl_counter(), dD.as<int32_t>(), dS.as<int32_t>()));
		HIPCHK(hipStreamSynchronize(c->stream));
		std::vector<uint32_t> ids;
		for (int k = 1; k <= 2; k++) {
			RC(collect(c, s, ST_D_OVF, ids));
			if (ids.empty()) break;
			RC(ensure_class(c, k));
			RC(launch_calc_d(c, k, 0, s.d_worklist.as<uint32_t>(), (uint32_t)ids.size(), s.ctl_counter2(), dD.as<int32_t>(), dS.as<int32_t>()));
			HIPCHK(hipStreamSynchronize(c->stream));
		}
		RC(collect(c, s, ST_D_OVF, ids));
		if (!ids.empty()) return fail(BWB_E_OVERFLOW, "calculate_d: SA-interval list exceeded the largest scratch class");
	}
	HIPCHK(hipMemcpyAsync(out_D, dD.p, nD * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(out_Dseed, dS.p, nS * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	RC(resolve_times(c, true));
	return read_device_stats(c);
}

extern "C" int bwb_hip_rank16(bwb_hip_ctx *c, const uint64_t *pos, size_t n, int inc, int exact, uint64_t *out) {
	if (!c || (n && (!pos || !out))) return fail(BWB_E_ARG, "rank16: null argument");
	if (n == 0) return BWB_OK;
	for (size_t i = 0; i < n; i++)
		if (pos[i] != ~0ull && pos[i] >= c->ix.length) return fail(BWB_E_ARG, "rank16: position out of range");
	HIPCHK(hipSetDevice(c->device));
	RC(index_ready(c));
	DevMem dp, dout;
	HIPCHK(dp.alloc(n * 8));
	HIPCHK(dout.alloc(n * 128));
	HIPCHK(hipMemcpyAsync(dp.p, pos, n * 8, hipMemcpyHostToDevice, c->stream));
	const unsigned grid = oct_grid(c, n);
	hipLaunchKernelGGL(k_rank16, dim3(grid), dim3(BWB_BLOCK), 0, c->stream, c->ix, dp.as<uint64_t>(), (uint64_t)n, inc, exact, dout.as<uint64_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, dout.p, n * 128, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return BWB_OK;
}

/* wave_children by itself, for parity tests: pair q runs as lane q % 64 of wave q / 64 (kl_children, bwb_lane.h) */
extern "C" int bwb_hip_children(bwb_hip_ctx *c, const uint64_t *iL, const uint64_t *iU, const uint8_t *flags, size_t n, uint64_t *out_L, uint64_t *out_U, uint32_t *out_mask) {
	if (!c || (n && (!iL || !iU || !flags || !out_L || !out_U || !out_mask))) return fail(BWB_E_ARG, "children: null argument");
	if (n == 0) return BWB_OK;
	for (size_t i = 0; i < n; i++) /* iL - 1 and iU are positions: -1 (iL == 0) .. length - 1 */
		if (iL[i] > c->ix.length || iU[i] >= c->ix.length || (flags[i] & ~3u)) return fail(BWB_E_ARG, "children: interval out of range or unknown flag");
	HIPCHK(hipSetDevice(c->device));
	RC(index_ready(c));
	DevMem dL, dU, df, doL, doU, dm;
	HIPCHK(dL.alloc(n * 8)); HIPCHK(dU.alloc(n * 8)); HIPCHK(df.alloc(n));
	HIPCHK(doL.alloc(n * 15 * 8)); HIPCHK(doU.alloc(n * 15 * 8)); HIPCHK(dm.alloc(n * 4));
	HIPCHK(hipMemcpyAsync(dL.p, iL, n * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(dU.p, iU, n * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(df.p, flags, n, hipMemcpyHostToDevice, c->stream));
	const unsigned grid = (unsigned)std::min<size_t>((n + LANE_BLOCK - 1) / LANE_BLOCK, (size_t)c->num_cu * 8);
	with_pos(c, [&](auto p) {
		hipLaunchKernelGGL(kl_children<decltype(p)>, dim3(grid), dim3(LANE_BLOCK), 0, c->stream, c->ix, dL.as<uint64_t>(), dU.as<uint64_t>(), df.as<uint8_t>(), (uint64_t)n, doL.as<uint64_t>(), doU.as<uint64_t>(), dm.as<uint32_t>());
	});
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out_L, doL.p, n * 15 * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(out_U, doU.p, n * 15 * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(out_mask, dm.p, n * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return BWB_OK;
}

/* layout 0: octet-cooperative rank (k_rank_bench); 1: one query per lane, the layout of the alignment kernels */
static int rank_bench(bwb_hip_ctx *c, int layout, size_t n, int iters, uint64_t seed, double *ms_per_iter, uint64_t *checksum) {
	if (!c || n < 4 || iters < 1) return fail(BWB_E_ARG, "rank_bench: bad argument");
	n &= ~(size_t)3;
	HIPCHK(hipSetDevice(c->device));
	RC(index_ready(c));
	unsigned long long *cs = c->d_misc.as<unsigned long long>();
	HIPCHK(hipMemsetAsync(cs, 0, 8, c->stream));
	const unsigned grid = (unsigned)(c->num_cu * 8);
	auto launch = [&](uint64_t sd) {
		with_pos(c, [&](auto p) {
			if (layout == 0) hipLaunchKernelGGL(k_rank_bench<decltype(p)>, dim3(grid), dim3(BWB_BLOCK), 0, c->stream, c->ix, (uint64_t)n, sd, cs);
			else hipLaunchKernelGGL(k_rank_bench_lane<decltype(p)>, dim3(grid), dim3(LANE_BLOCK), 0, c->stream, c->ix, (uint64_t)n, sd, cs);
		});
	};
	Timed t(c, c->stream);
	launch(seed); /* warm-up */
	HIPCHK(hipMemsetAsync(cs, 0, 8, c->stream));
	RC(t.begin());
	for (int i = 0; i < iters; i++)
		launch(seed + i);
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms = 0;
	RC(t.ms(&ms));
	unsigned long long v = 0;
	RC(fetch(c, &v, cs, 8));
	if (ms_per_iter) *ms_per_iter = ms / iters;
	if (checksum) *checksum = v;
	return BWB_OK;
}
extern "C" int bwb_hip_rank_bench(bwb_hip_ctx *c, size_t n, int iters, uint64_t seed, double *ms_per_iter, uint64_t *checksum) {
	return rank_bench(c, 0, n, iters, seed, ms_per_iter, checksum);
}
extern "C" int bwb_hip_rank_bench_lane(bwb_hip_ctx *c, size_t n, int iters, uint64_t seed, double *ms_per_iter, uint64_t *checksum) {
	return rank_bench(c, 1, n, iters, seed, ms_per_iter, checksum);
}

extern "C" int bwb_hip_set_sa(bwb_hip_ctx *c, const uint64_t *SA, uint64_t num_sa) {
	if (!c || !SA || num_sa != (c->ix.length + 31) / 32) return fail(BWB_E_ARG, "set_sa: bad argument");
	HIPCHK(hipSetDevice(c->device));
	/* (on the result stream, which only the caller's thread uses: after ctx_create_async the context's upload thread is still queueing
	 * the index on the kernel stream, and neither waits for the other.  `bwbble map` calls this before its first slot_upload, so that
	 * the chunk pool is sized from what is free with the SA resident) */
	HIPCHK(c->d_SA.alloc(num_sa * 8));
	HIPCHK(hipMemcpyAsync(c->d_SA.p, SA, num_sa * 8, hipMemcpyHostToDevice, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	c->num_sa = num_sa;
	return BWB_OK;
}

extern "C" int bwb_hip_locate(bwb_hip_ctx *c, const uint64_t *rows, size_t n, uint64_t *out_pos) {
	if (!c || (n && (!rows || !out_pos))) return fail(BWB_E_ARG, "locate: null argument");
	if (!c->d_SA.p) return fail(BWB_E_STATE, "locate: sampled SA not uploaded (bwb_hip_set_sa)");
	if (n == 0) { c->locate_ms = 0; c->locate_steps = 0; c->locate_rows = 0; return BWB_OK; } /* (locate_stats reports THIS call) */
	for (size_t i = 0; i < n; i++) if (rows[i] >= c->ix.length) return fail(BWB_E_ARG, "locate: row out of range");
	HIPCHK(hipSetDevice(c->device));
	RC(index_ready(c));
	DevMem dr, dout;
	HIPCHK(dr.alloc(n * 8));
	HIPCHK(dout.alloc(n * 8));
	HIPCHK(hipMemcpyAsync(dr.p, rows, n * 8, hipMemcpyHostToDevice, c->stream));
	const unsigned grid = oct_grid(c, n);
	Timed t(c, c->stream);
	unsigned long long *steps = c->d_stats.as<unsigned long long>() + STAT_LOCATE_STEPS;
	HIPCHK(hipMemsetAsync(steps, 0, 8, c->stream));
	RC(t.begin());
	hipLaunchKernelGGL(k_locate, dim3(grid), dim3(BWB_BLOCK), 0, c->stream, c->ix, c->d_SA.as<uint64_t>(), c->sa0_index, dr.as<uint64_t>(), (uint64_t)n, dout.as<uint64_t>(), c->d_stats.as<unsigned long long>());
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipMemcpyAsync(out_pos, dout.p, n * 8, hipMemcpyDeviceToHost, c->stream));
	unsigned long long hsteps = 0;
	HIPCHK(hipMemcpyAsync(&hsteps, steps, 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	float ms = 0;
	RC(t.ms(&ms));
	c->locate_ms = ms; c->locate_steps = hsteps; c->locate_rows = n;
	return BWB_OK;
}

/* the last bwb_hip_locate call: rows, invPsi steps (= rank-block visits: one 128-byte bucket each) and the kernel's HIP-event time */
extern "C" int bwb_hip_locate_stats(bwb_hip_ctx *c, uint64_t *rows, uint64_t *steps, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "locate_stats: null context");
	if (rows) *rows = c->locate_rows;
	if (steps) *steps = c->locate_steps;
	if (kernel_ms) *kernel_ms = c->locate_ms;
	return BWB_OK;
}

/* ---- placement records: eval_aln + mapq on the GPU (k_place) ------------------------------------------------------ */
static_assert(sizeof(bwb_place) == 48, "bwb_place is three 16-byte words (k_place)");
static int ensure_qtab(bwb_hip_ctx *c) { /* mapq's table (k_place, k_join_reads), followed by k_place's step counter */
	if (c->d_qtab.p) return BWB_OK;
	uint8_t tab[256 + 8] = { 0 }; /* the only floating point of mapq (align.c:744), with the host's own expression */
	for (int k = 1; k < 256; k++) tab[k] = (uint8_t)(int)(4.343 * log((double)k) + 0.5);
	HIPCHK(c->d_qtab.alloc(sizeof(tab)));
	HIPCHK(hipMemcpyAsync(c->d_qtab.p, tab, sizeof(tab), hipMemcpyHostToDevice, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	return BWB_OK;
}
/* an array of the caller's (pageable memory) into a fresh allocation, on the result stream: the caller synchronises once, after its last one */
static int stage_in(bwb_hip_ctx *c, DevMem &d, const void *src, size_t bytes) {
	HIPCHK(d.alloc(bytes));
	if (bytes) HIPCHK(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, c->rstream));
	return BWB_OK;
}
/* the exclusive scan of cnt[0 .. n) into off[0 .. n], the total last, on the result stream; bsum holds blocks_of(n) block sums */
static void scan_offsets(bwb_hip_ctx *c, const uint32_t *d_cnt, uint32_t n, uint64_t *d_off, uint64_t *d_bsum) {
	const unsigned nblk = blocks_of(n);
	hipLaunchKernelGGL(k_scan_blocks, dim3(nblk), dim3(BWB_BLOCK), 0, c->rstream, d_cnt, n, d_off, d_bsum);
	hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(BWB_BLOCK), 0, c->rstream, d_bsum, (uint32_t)nblk, d_off + n);
	hipLaunchKernelGGL(k_scan_add, dim3(nblk), dim3(BWB_BLOCK), 0, c->rstream, d_off, n, d_bsum);
}
/* off[0 .. n] of a caller's records: starts at 0, ascends, and - max_per_read below NO_LIMIT - no read owns more */
static const uint64_t NO_LIMIT = ~0ull;
static int check_offsets(const char *who, const char *what, const uint64_t *off, uint32_t n, uint64_t max_per_read) {
	if (off[0] != 0) return fail(BWB_E_ARG, std::string(who) + ": " + what + "[0] must be 0");
	for (uint32_t r = 0; r < n; r++) {
		if (off[r + 1] >= off[r] && off[r + 1] - off[r] <= max_per_read) continue;
		if (max_per_read == NO_LIMIT) return fail(BWB_E_ARG, std::string(who) + ": " + what + " does not ascend at read " + std::to_string(r));
		return fail(BWB_E_ARG, std::string(who) + ": read " + std::to_string(r) + " does not own 0.." + std::to_string(max_per_read) + " items");
	}
	return BWB_OK;
}
/* what every bwb_hip_batch_* stage call asks before it forwards to slot 0 */
static int batch_ready(bwb_hip_ctx *c, const char *who) {
	if (!c->d_SA.p) return fail(BWB_E_STATE, std::string(who) + ": sampled SA not uploaded (bwb_hip_set_sa)");
	if (!c->slots[0].submitted || !c->slots[0].complete) return fail(BWB_E_STATE, std::string(who) + ": batch_run has not completed");
	return BWB_OK;
}
/* k_place over n reads whose hits are log[off[r] .. off[r] + cnt[r]) (all device memory, log_n hits in the log) -> n records in d_out, copied to
 * h_out; sets the context's place_ms / place_steps.  On the result stream.  Shared by slot_place (the slot's hit log) and place_hits (a hit
 * list of the caller's): the same kernel, the same launch. */
static int place_launch(bwb_hip_ctx *c, const char *who, const uint4 *d_log, uint64_t log_n, const uint64_t *d_off, const uint32_t *d_cnt, uint32_t n, int max_mm,
                        uint4 *d_out, bwb_place *h_out) {
	RC(ensure_qtab(c));
	c->place_ms = 0; c->place_steps = 0; c->place_reads = n;
	if (!n) return BWB_OK;
	Timed t(c, c->rstream);
	unsigned long long *steps = (unsigned long long *)(c->d_qtab.as<unsigned char>() + 256);
	HIPCHK(hipMemsetAsync(steps, 0, 8, c->rstream));
	const unsigned grid = oct_grid(c, n);
	RC(t.begin());
	hipLaunchKernelGGL(k_place, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->ix, c->d_SA.as<uint64_t>(), c->sa0_index, d_log, log_n,
	                   d_off, d_cnt, n, max_mm, c->d_qtab.as<uint8_t>(), d_out, steps);
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(bwb_place), hipMemcpyDeviceToHost, c->rstream));
	unsigned long long hsteps = 0;
	HIPCHK(hipMemcpyAsync(&hsteps, steps, 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	float ms = 0;
	RC(t.ms(&ms));
	c->place_ms = ms; c->place_steps = hsteps;
	for (uint32_t i = 0; i < n; i++)
		if (h_out[i].flags & PLACE_F_BAD) return fail(BWB_E_STATE, std::string(who) + ": a read's hits lie outside the hit log or the index");
	return BWB_OK;
}

/* How many hits the log of a finished slot holds.  On the result stream: the kernel stream may hold slices of later slots, seconds each,
 * and the place calls must not wait for them.  The slot's reads are done (slot_wait) and were published with a system-scope release; the
 * host reads the same memory on this stream in slot_result. */
static int slot_log_n(bwb_hip_ctx *c, Slot &s, uint64_t *log_n) {
	RC(fetch(c, s.h_ctl.p, s.ctl_count(), 8));
	*log_n = std::min<unsigned long long>(*s.h_ctl.as<unsigned long long>(), s.log_cap);
	return BWB_OK;
}

/* The chain behind the bwb_hip_slot_* calls.  ensure_X leaves stage X's records for these arguments in the slot, in device memory and in the pinned
 * buffers, and calls ensure_* on the stages X reads; it refuses, under the name slot_X, what bwb_hip_slot_X refuses.  A stage whose key matches
 * (StageCache) launches nothing and leaves the *_stats figures where the last launch put them; a slot of 0 reads always takes the launch path, which
 * reserves the buffers and returns.  Every chain begins with ensure_place: it selects the device and waits for the slot. */
static int ensure_place(bwb_hip_ctx *c, int si, int max_mm) {
	HIPCHK(hipSetDevice(c->device));
	Slot &s = c->slots[si];
	if (!c->d_SA.p) return fail(BWB_E_STATE, "slot_place: sampled SA not uploaded (bwb_hip_set_sa)");
	if (!s.submitted) return fail(BWB_E_STATE, "slot_place: the slot has not been submitted");
	RC(slot_wait(c, si));
	const uint32_t n = s.n_reads;
	if (s.stage.place_mm == max_mm && n) return BWB_OK;
	HIPCHK(s.h_place.reserve((size_t)n * sizeof(bwb_place)));
	uint64_t log_n = 0;
	if (n) {
		HIPCHK(s.d_place.reserve((size_t)n * sizeof(bwb_place)));
		RC(slot_log_n(c, s, &log_n));
	}
	RC(place_launch(c, "slot_place", s.d_log.as<uint4>(), log_n, s.d_off.as<uint64_t>(), s.d_n.as<uint32_t>(), n, max_mm, s.d_place.as<uint4>(), s.h_place.as<bwb_place>()));
	s.stage.place_mm = max_mm;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_place(bwb_hip_ctx *c, int si, int max_mm, const bwb_place **out, uint32_t *n_reads) {
	if (!c || !out || !n_reads || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_place: bad argument");
	RC(ensure_place(c, si, max_mm));
	*out = c->slots[si].h_place.as<bwb_place>();
	*n_reads = c->slots[si].n_reads;
	return BWB_OK;
}

/* k_place on a hit list of the caller's instead of a slot's hit log (for parity tests): read r owns alns[aln_off[r] .. aln_off[r + 1]) */
static int alt_launch(bwb_hip_ctx *c, const char *who, const uint4 *d_log, uint64_t log_n, const uint64_t *d_off, const uint32_t *d_cnt, uint32_t n, int max_alt, AltBufs &ab);
/* (max_alt 0: the placement records only; otherwise the items as well, into the context's hits_alt) */
static int place_hits_impl(bwb_hip_ctx *c, const std::string &who, const bwb_aln *alns, const uint64_t *aln_off, uint32_t n_reads, int max_mm, int max_alt, bwb_place *out) {
	if (!c->d_SA.p) return fail(BWB_E_STATE, who + ": sampled SA not uploaded (bwb_hip_set_sa)");
	const uint64_t base = aln_off[0], total = aln_off[n_reads] - base;
	std::vector<uint64_t> off(n_reads ? n_reads : 1);
	std::vector<uint32_t> cnt(n_reads ? n_reads : 1);
	for (uint32_t r = 0; r < n_reads; r++) {
		if (aln_off[r + 1] < aln_off[r] || aln_off[r + 1] - aln_off[r] > 0xFFFFFFFFull) return fail(BWB_E_ARG, who + ": aln_off is not ascending");
		off[r] = aln_off[r] - base; cnt[r] = (uint32_t)(aln_off[r + 1] - aln_off[r]);
	}
	if (total && !alns) return fail(BWB_E_ARG, who + ": null argument");
	HIPCHK(hipSetDevice(c->device));
	RC(index_ready(c));
	static_assert(sizeof(bwb_aln) == 48, "bwb_aln is the hit log's three 16-byte words");
	DevMem d_log, d_off, d_cnt, d_out;
	RC(stage_in(c, d_log, total ? alns + base : nullptr, (size_t)total * sizeof(bwb_aln)));
	RC(stage_in(c, d_off, off.data(), (size_t)n_reads * 8));
	RC(stage_in(c, d_cnt, cnt.data(), (size_t)n_reads * 4));
	HIPCHK(d_out.alloc((size_t)n_reads * sizeof(bwb_place)));
	if (n_reads) HIPCHK(hipStreamSynchronize(c->rstream));
	const int rc = place_launch(c, who.c_str(), d_log.as<uint4>(), total, d_off.as<uint64_t>(), d_cnt.as<uint32_t>(), n_reads, max_mm, d_out.as<uint4>(), out);
	if (rc || !max_alt) return rc;
	return alt_launch(c, who.c_str(), d_log.as<uint4>(), total, d_off.as<uint64_t>(), d_cnt.as<uint32_t>(), n_reads, max_alt, c->hits_alt);
}

extern "C" int bwb_hip_place_hits(bwb_hip_ctx *c, const bwb_aln *alns, const uint64_t *aln_off, uint32_t n_reads, int max_mm, bwb_place *out) {
	if (!c || !aln_off || (n_reads && !out)) return fail(BWB_E_ARG, "place_hits: null argument");
	return place_hits_impl(c, "place_hits", alns, aln_off, n_reads, max_mm, 0, out);
}

extern "C" int bwb_hip_place_hits_alt(bwb_hip_ctx *c, const bwb_aln *alns, const uint64_t *aln_off, uint32_t n_reads, int max_mm, int max_alt, bwb_place *out,
                                      const uint64_t **alt_off, const bwb_alt **alts) {
	if (!c || !aln_off || (n_reads && !out) || !alt_off || !alts) return fail(BWB_E_ARG, "place_hits_alt: null argument");
	if (max_alt < 1 || max_alt > 255) return fail(BWB_E_ARG, "place_hits_alt: max_alt must be 1..255");
	RC(place_hits_impl(c, "place_hits_alt", alns, aln_off, n_reads, max_mm, max_alt, out));
	*alt_off = c->hits_alt.h_off.as<uint64_t>();
	*alts = c->hits_alt.h_alts.as<bwb_alt>();
	return BWB_OK;
}

extern "C" int bwb_hip_batch_place(bwb_hip_ctx *c, int max_mm, const bwb_place **out, uint32_t *n_reads) {
	if (!c || !out || !n_reads) return fail(BWB_E_ARG, "batch_place: null argument");
	RC(batch_ready(c, "batch_place"));
	return bwb_hip_slot_place(c, 0, max_mm, out, n_reads);
}

/* the last place call: reads, invPsi steps and the kernel's HIP-event time */
extern "C" int bwb_hip_place_stats(bwb_hip_ctx *c, uint64_t *reads, uint64_t *steps, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "place_stats: null context");
	if (reads) *reads = c->place_reads;
	if (steps) *steps = c->place_steps;
	if (kernel_ms) *kernel_ms = c->place_ms;
	return BWB_OK;
}

/* ---- a read's other placements: bwb_alt records (k_alt_count, the scan, k_place_alt) ------------------------------------------ */
static_assert(sizeof(bwb_alt) == 32, "bwb_alt is two 16-byte words (k_place_alt)");
/* The three steps over n reads whose hits are log[off[r] .. off[r] + cnt[r]) -> ab.h_off[n + 1] and ab.h_alts[h_off[n]]; sets the context's
 * alt_ms / alt_steps / alt_items.  On the result stream, like place_launch.  The only host round trip is the read of the total, which sizes
 * the record buffers: they hold the items there are, never n * max_alt. */
static int alt_launch(bwb_hip_ctx *c, const char *who, const uint4 *d_log, uint64_t log_n, const uint64_t *d_off, const uint32_t *d_cnt, uint32_t n, int max_alt, AltBufs &ab) {
	c->alt_ms = 0; c->alt_steps = 0; c->alt_items = 0;
	HIPCHK(ab.h_off.reserve(((size_t)n + 1) * 8));
	ab.h_off.as<uint64_t>()[0] = 0;
	if (!n) return BWB_OK;
	const unsigned nblk = blocks_of(n);
	HIPCHK(ab.d_cnt.reserve((size_t)n * 4));
	HIPCHK(ab.d_off.reserve(((size_t)n + 1) * 8));
	HIPCHK(ab.d_bsum.reserve((size_t)nblk * 8));
	if (!c->d_altctl.p) HIPCHK(c->d_altctl.alloc(16));
	Timed t_count(c, c->rstream), t_place(c, c->rstream); /* k_alt_count and the scan; k_place_alt */
	unsigned long long *ctl = c->d_altctl.as<unsigned long long>();
	uint64_t *d_altoff = ab.d_off.as<uint64_t>();
	HIPCHK(hipMemsetAsync(ctl, 0, 16, c->rstream));
	RC(t_count.begin());
	hipLaunchKernelGGL(k_alt_count, dim3(nblk), dim3(BWB_BLOCK), 0, c->rstream, d_log, log_n, d_off, d_cnt, n, (uint32_t)max_alt, ab.d_cnt.as<uint32_t>());
	scan_offsets(c, ab.d_cnt.as<uint32_t>(), n, d_altoff, ab.d_bsum.as<uint64_t>());
	HIPCHK(hipGetLastError());
	RC(t_count.end());
	HIPCHK(hipMemcpyAsync(ab.h_off.p, d_altoff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	const uint64_t total = ab.h_off.as<uint64_t>()[n];
	float ms = 0, ms2 = 0;
	RC(t_count.ms(&ms));
	unsigned long long hctl[2] = { 0, 0 };
	if (total) {
		HIPCHK(ab.d_alts.reserve((size_t)total * sizeof(bwb_alt)));
		HIPCHK(ab.h_alts.reserve((size_t)total * sizeof(bwb_alt)));
		const unsigned grid = oct_grid(c, total);
		RC(t_place.begin());
		hipLaunchKernelGGL(k_place_alt, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->ix, c->d_SA.as<uint64_t>(), c->sa0_index, d_log, log_n, d_off, d_cnt, n,
		                   (const uint64_t *)d_altoff, total, ab.d_alts.as<uint4>(), ctl);
		HIPCHK(hipGetLastError());
		RC(t_place.end());
		HIPCHK(hipMemcpyAsync(ab.h_alts.p, ab.d_alts.p, (size_t)total * sizeof(bwb_alt), hipMemcpyDeviceToHost, c->rstream));
		HIPCHK(hipMemcpyAsync(hctl, ctl, 16, hipMemcpyDeviceToHost, c->rstream));
		HIPCHK(hipStreamSynchronize(c->rstream));
		RC(t_place.ms(&ms2));
	}
	c->alt_ms = (double)ms + ms2; c->alt_steps = hctl[0]; c->alt_items = total;
	if (hctl[1]) return fail(BWB_E_STATE, std::string(who) + ": an alternative's hit lies outside the hit log or its row outside the index");
	return BWB_OK;
}

static int ensure_alt(bwb_hip_ctx *c, int si, int max_mm, int max_alt) {
	RC(ensure_place(c, si, max_mm));
	Slot &s = c->slots[si];
	const uint32_t n = s.n_reads;
	if (s.stage.alt_max == max_alt && n) return BWB_OK;
	uint64_t log_n = 0;
	if (n) RC(slot_log_n(c, s, &log_n));
	RC(alt_launch(c, "slot_place_alt", s.d_log.as<uint4>(), log_n, s.d_off.as<uint64_t>(), s.d_n.as<uint32_t>(), n, max_alt, s.alt));
	s.stage.alt_max = max_alt;
	return BWB_OK;
}
/* how many items the slot's alt holds (max_alt 0: the caller has not asked for any) */
static uint64_t slot_items(const Slot &s, int max_alt) { return max_alt && s.n_reads ? s.alt.h_off.as<uint64_t>()[s.n_reads] : 0; }

extern "C" int bwb_hip_slot_place_alt(bwb_hip_ctx *c, int si, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off, const bwb_alt **alts, uint32_t *n_reads) {
	if (!c || !places || !alt_off || !alts || !n_reads || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_place_alt: bad argument");
	if (max_alt < 1 || max_alt > 255) return fail(BWB_E_ARG, "slot_place_alt: max_alt must be 1..255");
	RC(ensure_alt(c, si, max_mm, max_alt));
	const Slot &s = c->slots[si];
	*places = s.h_place.as<bwb_place>();
	*alt_off = s.alt.h_off.as<uint64_t>();
	*alts = s.alt.h_alts.as<bwb_alt>();
	*n_reads = s.n_reads;
	return BWB_OK;
}

extern "C" int bwb_hip_batch_place_alt(bwb_hip_ctx *c, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off, const bwb_alt **alts, uint32_t *n_reads) {
	if (!c || !places || !alt_off || !alts || !n_reads) return fail(BWB_E_ARG, "batch_place_alt: null argument");
	if (max_alt < 1 || max_alt > 255) return fail(BWB_E_ARG, "batch_place_alt: max_alt must be 1..255");
	RC(batch_ready(c, "batch_place_alt"));
	return bwb_hip_slot_place_alt(c, 0, max_mm, max_alt, places, alt_off, alts, n_reads);
}

/* the last place_alt call: items, invPsi steps and the HIP-event time of its kernels (count + scan + k_place_alt) */
extern "C" int bwb_hip_place_alt_stats(bwb_hip_ctx *c, uint64_t *items, uint64_t *steps, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "place_alt_stats: null context");
	if (items) *items = c->alt_items;
	if (steps) *steps = c->alt_steps;
	if (kernel_ms) *kernel_ms = c->alt_ms;
	return BWB_OK;
}

/* ---- bubble hits in reference coordinates: bwb_locus records (k_locus) ---------------------------------------------------------- */
static_assert(sizeof(bwb_locus) == 32, "bwb_locus is two 16-byte words (k_locus)");
static_assert(sizeof(bwb_bubble) == 40, "bwb_bubble is five 64-bit words (k_locus)");
/* empty, or the first bubble the rule of bwb_lift refuses and why (bwb_hip_slot_lift answers BWB_E_ARG with it; -B and -J take any table) */
static std::string lift_table_refusal(const bwb_bubble *bubbles, uint32_t n_bub) {
	for (uint32_t k = 0; k < n_bub; k++) {
		const bwb_bubble &b = bubbles[k];
		const __int128 gap = (__int128)b.C - (__int128)b.A - (__int128)b.B_minus_A;
		const char *why = b.B_minus_A < 0 ? "B_minus_A is negative" : b.D_minus_C < -1 ? "D_minus_C is below -1" : b.alt_len < 0 ? "alt_len is negative" :
		                  gap < 0 ? "its flanks overlap on the chromosome (C - A - B_minus_A is negative)" : gap >= ((__int128)1 << 28) ? "its flanks lie 2^28 positions or more apart" : nullptr;
		if (why) return "bubble " + std::to_string(k) + ": " + why;
	}
	return std::string();
}
extern "C" int bwb_hip_set_loci(bwb_hip_ctx *c, const uint64_t *start, const uint64_t *end, const int32_t *bubble_of, uint32_t n_seq, const bwb_bubble *bubbles, uint32_t n_bub) {
	if (!c || !start || !end || !bubble_of || (n_bub && !bubbles)) return fail(BWB_E_ARG, "set_loci: null argument");
	if (n_seq < 1 || n_seq > 0x7FFFFFFFu || n_bub > 0x7FFFFFFFu) return fail(BWB_E_ARG, "set_loci: the number of records must be 1 .. 2^31 - 1");
	for (uint32_t i = 0; i < n_seq; i++) {
		if (start[i] > end[i] || (i && start[i] <= end[i - 1])) return fail(BWB_E_ARG, "set_loci: the records are not ascending and disjoint (record " + std::to_string(i) + ")");
		if (bubble_of[i] < -1 || (int64_t)bubble_of[i] >= (int64_t)n_bub)
			return fail(BWB_E_ARG, "set_loci: bubble_of[" + std::to_string(i) + "] = " + std::to_string(bubble_of[i]) + " lies outside the table of " + std::to_string(n_bub) + " bubbles");
	}
	HIPCHK(hipSetDevice(c->device));
	c->loci_nseq = 0; /* (no tables until all four are resident) */
	c->chrom_set = false;
	for (auto &s : c->slots) s.stage.loci_replaced();
	c->indel_on = false; /* (the table and the counters were these bubbles') */
	c->lift_refusal = lift_table_refusal(bubbles, n_bub);
	HIPCHK(c->d_lstart.alloc((size_t)n_seq * 8));
	HIPCHK(c->d_lend.alloc((size_t)n_seq * 8));
	HIPCHK(c->d_lbub.alloc((size_t)n_seq * 4));
	HIPCHK(c->d_bubbles.alloc((size_t)n_bub * sizeof(bwb_bubble)));
	/* (on the result stream, like set_sa: the caller's thread alone uses it) */
	HIPCHK(hipMemcpyAsync(c->d_lstart.p, start, (size_t)n_seq * 8, hipMemcpyHostToDevice, c->rstream));
	HIPCHK(hipMemcpyAsync(c->d_lend.p, end, (size_t)n_seq * 8, hipMemcpyHostToDevice, c->rstream));
	HIPCHK(hipMemcpyAsync(c->d_lbub.p, bubble_of, (size_t)n_seq * 4, hipMemcpyHostToDevice, c->rstream));
	if (n_bub) HIPCHK(hipMemcpyAsync(c->d_bubbles.p, bubbles, (size_t)n_bub * sizeof(bwb_bubble), hipMemcpyHostToDevice, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	c->loci_trips = ceil_log2(n_seq);
	c->loci_bub_of.assign(bubble_of, bubble_of + n_seq);
	c->loci_bubbles.assign(bubbles, bubbles + n_bub);
	c->loci_nbub = n_bub;
	c->loci_nseq = n_seq;
	return BWB_OK;
}

/* k_locus over n placement records in device memory -> n records in d_out, copied to h_out; sets the context's locus_ms / locus_reads.  On the
 * result stream, behind the k_place that wrote the records.  Shared by slot_locus and locus_places. */
static int locus_launch(bwb_hip_ctx *c, const uint4 *d_places, uint32_t n, uint4 *d_out, bwb_locus *h_out) {
	c->locus_ms = 0; c->locus_reads = n;
	if (!n) return BWB_OK;
	Timed t(c, c->rstream);
	RC(t.begin());
	hipLaunchKernelGGL(k_locus, dim3(lane_grid(c, n)), dim3(BWB_BLOCK), 0, c->rstream, d_places, n, c->d_lstart.as<uint64_t>(), c->d_lend.as<uint64_t>(), c->d_lbub.as<int32_t>(),
	                   c->loci_nseq, c->loci_trips, c->d_bubbles.as<uint64_t>(), d_out);
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipMemcpyAsync(h_out, d_out, (size_t)n * sizeof(bwb_locus), hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	float ms = 0;
	RC(t.ms(&ms));
	c->locus_ms = ms;
	return BWB_OK;
}

static int ensure_locus(bwb_hip_ctx *c, int si, int max_mm) {
	if (!c->loci_nseq) return fail(BWB_E_STATE, "slot_locus: record and bubble tables not uploaded (bwb_hip_set_loci)");
	RC(ensure_place(c, si, max_mm));
	Slot &s = c->slots[si];
	const uint32_t n = s.n_reads;
	if (s.stage.locus_mm == max_mm && n) return BWB_OK;
	HIPCHK(s.h_locus.reserve((size_t)n * sizeof(bwb_locus)));
	if (n) HIPCHK(s.d_locus.reserve((size_t)n * sizeof(bwb_locus)));
	RC(locus_launch(c, s.d_place.as<uint4>(), n, s.d_locus.as<uint4>(), s.h_locus.as<bwb_locus>()));
	s.stage.locus_mm = max_mm;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_locus(bwb_hip_ctx *c, int si, int max_mm, const bwb_place **places, const bwb_locus **loci, uint32_t *n_reads) {
	if (!c || !places || !loci || !n_reads || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_locus: bad argument");
	RC(ensure_locus(c, si, max_mm));
	const Slot &s = c->slots[si];
	*places = s.h_place.as<bwb_place>();
	*loci = s.h_locus.as<bwb_locus>();
	*n_reads = s.n_reads;
	return BWB_OK;
}

extern "C" int bwb_hip_batch_locus(bwb_hip_ctx *c, int max_mm, const bwb_place **places, const bwb_locus **loci, uint32_t *n_reads) {
	if (!c || !places || !loci || !n_reads) return fail(BWB_E_ARG, "batch_locus: null argument");
	if (!c->loci_nseq) return fail(BWB_E_STATE, "batch_locus: record and bubble tables not uploaded (bwb_hip_set_loci)");
	RC(batch_ready(c, "batch_locus"));
	return bwb_hip_slot_locus(c, 0, max_mm, places, loci, n_reads);
}

/* k_locus on placement records of the caller's instead of a slot's (for parity tests) */
extern "C" int bwb_hip_locus_places(bwb_hip_ctx *c, const bwb_place *places, uint32_t n, bwb_locus *out) {
	if (!c || (n && (!places || !out)) || n > 0x7FFFFFFFu) return fail(BWB_E_ARG, "locus_places: bad argument");
	if (!c->loci_nseq) return fail(BWB_E_STATE, "locus_places: record and bubble tables not uploaded (bwb_hip_set_loci)");
	HIPCHK(hipSetDevice(c->device));
	DevMem d_in, d_out;
	RC(stage_in(c, d_in, places, (size_t)n * sizeof(bwb_place)));
	HIPCHK(d_out.alloc((size_t)n * sizeof(bwb_locus)));
	if (n) HIPCHK(hipStreamSynchronize(c->rstream));
	return locus_launch(c, d_in.as<uint4>(), n, d_out.as<uint4>(), out);
}

/* the last locus call: reads resolved and the kernel's HIP-event time */
extern "C" int bwb_hip_locus_stats(bwb_hip_ctx *c, uint64_t *reads, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "locus_stats: null context");
	if (reads) *reads = c->locus_reads;
	if (kernel_ms) *kernel_ms = c->locus_ms;
	return BWB_OK;
}

/* ---- a read's placements counted by locus: bwb_join records (k_join_items, k_join_reads) ---------------------------------------- */
static_assert(sizeof(bwb_join) == 16, "bwb_join is one 16-byte word (k_join_reads)");
extern "C" int bwb_hip_set_bubble_chrom(bwb_hip_ctx *c, const int32_t *chrom_of, uint32_t n_bub) {
	if (!c || (n_bub && !chrom_of)) return fail(BWB_E_ARG, "set_bubble_chrom: null argument");
	if (!c->loci_nseq) return fail(BWB_E_STATE, "set_bubble_chrom: record and bubble tables not uploaded (bwb_hip_set_loci)");
	if (n_bub != c->loci_nbub) return fail(BWB_E_ARG, "set_bubble_chrom: " + std::to_string(n_bub) + " bubbles, the table of set_loci has " + std::to_string(c->loci_nbub));
	for (uint32_t b = 0; b < n_bub; b++)
		if (chrom_of[b] < 0 || (uint32_t)chrom_of[b] >= c->loci_nseq || c->loci_bub_of[chrom_of[b]] != -1)
			return fail(BWB_E_ARG, "set_bubble_chrom: chrom_of[" + std::to_string(b) + "] = " + std::to_string(chrom_of[b]) + " is not a non-bubble record of the table of " +
			                           std::to_string(c->loci_nseq) + " records");
	HIPCHK(hipSetDevice(c->device));
	c->chrom_set = false;
	for (auto &s : c->slots) s.stage.chrom_replaced();
	c->indel_on = false;
	c->chrom_of.assign(chrom_of, chrom_of + n_bub);
	HIPCHK(c->d_chrom.alloc((size_t)n_bub * 4));
	if (n_bub) {
		HIPCHK(hipMemcpyAsync(c->d_chrom.p, chrom_of, (size_t)n_bub * 4, hipMemcpyHostToDevice, c->rstream));
		HIPCHK(hipStreamSynchronize(c->rstream));
	}
	c->chrom_set = true;
	return BWB_OK;
}

/* what the two kernels read, all device memory: n placement records, their locus records, alt_off[n + 1], n_items items, and for the suboptimal
 * bit either the hit log the items came from (log, log_n, off, cnt) or one byte per item (sub) */
struct JoinIn {
	const uint4 *places; uint32_t n; const uint4 *loci; const uint64_t *alt_off; const uint4 *alts; uint64_t n_items;
	const uint4 *log; uint64_t log_n; const uint64_t *off; const uint32_t *cnt; const uint8_t *sub;
};
/* k_join_items + k_join_reads -> n records in d_out, copied to h_out; sets the context's join_ms / join_items / join_joined.  On the result
 * stream, behind the kernels that wrote the records.  Shared by slot_join and join_records. */
static int join_launch(bwb_hip_ctx *c, const JoinIn &in, int max_mm, DevMem &d_cls, uint4 *d_out, bwb_join *h_out) {
	c->join_ms = 0; c->join_items = in.n_items; c->join_joined = 0;
	if (!in.n) return BWB_OK;
	RC(ensure_qtab(c));
	HIPCHK(d_cls.reserve((size_t)in.n_items));
	Timed t(c, c->rstream);
	RC(t.begin());
	if (in.n_items)
		hipLaunchKernelGGL(k_join_items, dim3(lane_grid(c, in.n_items)), dim3(BWB_BLOCK), 0, c->rstream,
		                   in.places, in.n, ceil_log2(in.n), in.alt_off, in.alts, in.n_items, in.loci, c->d_lstart.as<uint64_t>(), c->d_lend.as<uint64_t>(), c->d_lbub.as<int32_t>(),
		                   c->loci_nseq, c->loci_trips, c->d_bubbles.as<uint64_t>(), c->d_chrom.as<int32_t>(), in.log, in.log_n, in.off, in.cnt, in.sub, d_cls.as<uint8_t>());
	hipLaunchKernelGGL(k_join_reads, dim3(lane_grid(c, in.n)), dim3(BWB_BLOCK), 0, c->rstream,
	                   in.places, in.n, in.alt_off, d_cls.as<uint8_t>(), max_mm, c->d_qtab.as<uint8_t>(), d_out);
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipMemcpyAsync(h_out, d_out, (size_t)in.n * sizeof(bwb_join), hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	float ms = 0;
	RC(t.ms(&ms));
	c->join_ms = ms;
	for (uint32_t r = 0; r < in.n; r++) c->join_joined += h_out[r].joined;
	return BWB_OK;
}

static int join_ready(bwb_hip_ctx *c, const char *who, int max_alt) {
	if (max_alt < 1 || max_alt > 255) return fail(BWB_E_ARG, std::string(who) + ": max_alt must be 1..255");
	if (!c->loci_nseq) return fail(BWB_E_STATE, std::string(who) + ": record and bubble tables not uploaded (bwb_hip_set_loci)");
	if (!c->chrom_set) return fail(BWB_E_STATE, std::string(who) + ": the bubbles' chromosome records not uploaded (bwb_hip_set_bubble_chrom)");
	return BWB_OK;
}

static int ensure_join(bwb_hip_ctx *c, int si, int max_mm, int max_alt) {
	RC(join_ready(c, "slot_join", max_alt));
	RC(ensure_alt(c, si, max_mm, max_alt));
	RC(ensure_locus(c, si, max_mm));
	Slot &s = c->slots[si];
	const uint32_t n = s.n_reads;
	if (s.stage.join_mm == max_mm && s.stage.join_alt == max_alt && n) return BWB_OK;
	HIPCHK(s.h_join.reserve((size_t)n * sizeof(bwb_join)));
	uint64_t log_n = 0;
	if (n) {
		HIPCHK(s.d_join.reserve((size_t)n * sizeof(bwb_join)));
		RC(slot_log_n(c, s, &log_n));
	}
	const JoinIn in = { s.d_place.as<uint4>(), n, s.d_locus.as<uint4>(), s.alt.d_off.as<uint64_t>(), s.alt.d_alts.as<uint4>(), slot_items(s, max_alt),
	                    s.d_log.as<uint4>(), log_n, s.d_off.as<uint64_t>(), s.d_n.as<uint32_t>(), nullptr };
	RC(join_launch(c, in, max_mm, s.d_cls, s.d_join.as<uint4>(), s.h_join.as<bwb_join>()));
	s.stage.join_mm = max_mm; s.stage.join_alt = max_alt;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_join(bwb_hip_ctx *c, int si, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off, const bwb_alt **alts,
                                 const bwb_locus **loci, const bwb_join **joins, uint32_t *n_reads) {
	if (!c || !places || !alt_off || !alts || !loci || !joins || !n_reads || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_join: bad argument");
	RC(ensure_join(c, si, max_mm, max_alt));
	const Slot &s = c->slots[si];
	*places = s.h_place.as<bwb_place>();
	*alt_off = s.alt.h_off.as<uint64_t>();
	*alts = s.alt.h_alts.as<bwb_alt>();
	*loci = s.h_locus.as<bwb_locus>();
	*joins = s.h_join.as<bwb_join>();
	*n_reads = s.n_reads;
	return BWB_OK;
}

extern "C" int bwb_hip_batch_join(bwb_hip_ctx *c, int max_mm, int max_alt, const bwb_place **places, const uint64_t **alt_off, const bwb_alt **alts,
                                  const bwb_locus **loci, const bwb_join **joins, uint32_t *n_reads) {
	if (!c || !places || !alt_off || !alts || !loci || !joins || !n_reads) return fail(BWB_E_ARG, "batch_join: null argument");
	RC(join_ready(c, "batch_join", max_alt));
	RC(batch_ready(c, "batch_join"));
	return bwb_hip_slot_join(c, 0, max_mm, max_alt, places, alt_off, alts, loci, joins, n_reads);
}

/* the kernels on records of the caller's instead of a slot's (for parity tests): k_locus for the primaries' loci, then the two join kernels */
extern "C" int bwb_hip_join_records(bwb_hip_ctx *c, const bwb_place *places, uint32_t n, const uint64_t *alt_off, const bwb_alt *alts, const uint8_t *alt_sub, int max_mm,
                                    bwb_join *out) {
	if (!c || !alt_off || (n && (!places || !out)) || n > 0x7FFFFFFFu) return fail(BWB_E_ARG, "join_records: bad argument");
	RC(join_ready(c, "join_records", 1));
	RC(check_offsets("join_records", "alt_off", alt_off, n, 255));
	const uint64_t n_items = alt_off[n];
	if (n_items && (!alts || !alt_sub)) return fail(BWB_E_ARG, "join_records: null argument");
	HIPCHK(hipSetDevice(c->device));
	DevMem d_places, d_loci, d_off, d_alts, d_sub, d_cls, d_out;
	RC(stage_in(c, d_places, places, (size_t)n * sizeof(bwb_place)));
	RC(stage_in(c, d_off, alt_off, ((size_t)n + 1) * 8));
	RC(stage_in(c, d_alts, alts, (size_t)n_items * sizeof(bwb_alt)));
	RC(stage_in(c, d_sub, alt_sub, (size_t)n_items));
	HIPCHK(d_loci.alloc((size_t)n * sizeof(bwb_locus)));
	HIPCHK(d_out.alloc((size_t)n * sizeof(bwb_join)));
	HIPCHK(hipStreamSynchronize(c->rstream));
	std::vector<bwb_locus> h_loci(n ? n : 1);
	RC(locus_launch(c, d_places.as<uint4>(), n, d_loci.as<uint4>(), h_loci.data()));
	const JoinIn in = { d_places.as<uint4>(), n, d_loci.as<uint4>(), d_off.as<uint64_t>(), d_alts.as<uint4>(), n_items, nullptr, 0, nullptr, nullptr, d_sub.as<uint8_t>() };
	return join_launch(c, in, max_mm, d_cls, d_out.as<uint4>(), out);
}

/* the last join call: items compared, items joined and the two kernels' HIP-event time */
extern "C" int bwb_hip_join_stats(bwb_hip_ctx *c, uint64_t *items, uint64_t *joined, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "join_stats: null context");
	if (items) *items = c->join_items;
	if (joined) *joined = c->join_joined;
	if (kernel_ms) *kernel_ms = c->join_ms;
	return BWB_OK;
}

/* ---- placements on bubble records in chromosome coordinates: bwb_lift records (k_lift_count, k_lift) ---------------------------------- */
static_assert(sizeof(bwb_lift) == 16, "bwb_lift is one 16-byte word (k_lift)");
static int lift_ready(bwb_hip_ctx *c, const char *who, int max_alt) {
	if (max_alt < 0 || max_alt > 255) return fail(BWB_E_ARG, std::string(who) + ": max_alt must be 0..255");
	if (!c->loci_nseq) return fail(BWB_E_STATE, std::string(who) + ": record and bubble tables not uploaded (bwb_hip_set_loci)");
	if (!c->chrom_set) return fail(BWB_E_STATE, std::string(who) + ": the bubbles' chromosome records not uploaded (bwb_hip_set_bubble_chrom)");
	if (!c->lift_refusal.empty()) return fail(BWB_E_ARG, std::string(who) + ": " + c->lift_refusal);
	return BWB_OK;
}
/* k_lift_count, the scan and k_lift over n placement records, their locus records and n_items items (all device memory) -> lb.h_kind[n + n_items],
 * lb.h_off[n + n_items + 1] and lb.h_recs[h_off[last]]; sets the context's lift_ms / lift_lifted / lift_unliftable.  On the result stream, behind
 * the kernels that wrote the records.  The only host round trip is the read of the total, which sizes the record buffers: they hold the records
 * there are.  Shared by slot_lift and lift_records. */
static int lift_launch(bwb_hip_ctx *c, const char *who, const uint4 *d_places, uint32_t n, const uint4 *d_loci, const uint4 *d_alts, uint64_t n_items, LiftBufs &lb) {
	c->lift_ms = 0; c->lift_lifted = 0; c->lift_unliftable = 0;
	const uint64_t n_q = (uint64_t)n + n_items;
	if (n_q > 0x7FFFFFFFu) return fail(BWB_E_ARG, std::string(who) + ": more than 2^31 - 1 placements");
	HIPCHK(lb.h_off.reserve(((size_t)n_q + 1) * 8));
	HIPCHK(lb.h_kind.reserve((size_t)n_q));
	HIPCHK(lb.h_recs.reserve(sizeof(bwb_lift)));
	lb.h_off.as<uint64_t>()[0] = 0;
	if (!n_q) return BWB_OK;
	const unsigned grid = lane_grid(c, n_q);
	HIPCHK(lb.d_kind.reserve((size_t)n_q));
	HIPCHK(lb.d_cnt.reserve((size_t)n_q * 4));
	HIPCHK(lb.d_off.reserve(((size_t)n_q + 1) * 8));
	HIPCHK(lb.d_bsum.reserve((size_t)blocks_of(n_q) * 8));
	uint64_t *d_off = lb.d_off.as<uint64_t>();
	Timed t_count(c, c->rstream), t_lift(c, c->rstream); /* k_lift_count and the scan; k_lift */
	RC(t_count.begin());
	hipLaunchKernelGGL(k_lift_count, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, d_places, n, d_loci, d_alts, n_q, c->d_lstart.as<uint64_t>(), c->d_lend.as<uint64_t>(),
	                   c->d_lbub.as<int32_t>(), c->loci_nseq, c->loci_trips, c->d_bubbles.as<uint64_t>(), lb.d_kind.as<uint8_t>(), lb.d_cnt.as<uint32_t>());
	scan_offsets(c, lb.d_cnt.as<uint32_t>(), (uint32_t)n_q, d_off, lb.d_bsum.as<uint64_t>());
	HIPCHK(hipGetLastError());
	RC(t_count.end());
	HIPCHK(hipMemcpyAsync(lb.h_off.p, d_off, ((size_t)n_q + 1) * 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipMemcpyAsync(lb.h_kind.p, lb.d_kind.p, (size_t)n_q, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	const uint64_t total = lb.h_off.as<uint64_t>()[n_q];
	float ms = 0, ms2 = 0;
	RC(t_count.ms(&ms));
	if (total) {
		HIPCHK(lb.d_recs.reserve((size_t)total * sizeof(bwb_lift)));
		HIPCHK(lb.h_recs.reserve((size_t)total * sizeof(bwb_lift)));
		RC(t_lift.begin());
		hipLaunchKernelGGL(k_lift, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, d_places, n, d_loci, d_alts, n_q, c->d_lstart.as<uint64_t>(), c->d_lend.as<uint64_t>(),
		                   c->d_lbub.as<int32_t>(), c->loci_nseq, c->loci_trips, c->d_bubbles.as<uint64_t>(), c->d_chrom.as<int32_t>(), lb.d_kind.as<uint8_t>(), (const uint64_t *)d_off,
		                   lb.d_recs.as<uint4>());
		HIPCHK(hipGetLastError());
		RC(t_lift.end());
		HIPCHK(hipMemcpyAsync(lb.h_recs.p, lb.d_recs.p, (size_t)total * sizeof(bwb_lift), hipMemcpyDeviceToHost, c->rstream));
		HIPCHK(hipStreamSynchronize(c->rstream));
		RC(t_lift.ms(&ms2));
	}
	c->lift_ms = (double)ms + ms2;
	const uint8_t *kind = lb.h_kind.as<uint8_t>();
	for (uint64_t q = 0; q < n_q; q++) { c->lift_lifted += kind[q] == BWB_LIFT_LIFTED; c->lift_unliftable += kind[q] == BWB_LIFT_UNLIFTABLE; }
	return BWB_OK;
}

static int ensure_lift(bwb_hip_ctx *c, int si, int max_mm, int max_alt) {
	RC(lift_ready(c, "slot_lift", max_alt));
	if (max_alt) RC(ensure_alt(c, si, max_mm, max_alt));
	RC(ensure_locus(c, si, max_mm));
	Slot &s = c->slots[si];
	if (s.stage.lift_mm == max_mm && s.stage.lift_alt == max_alt && s.n_reads) return BWB_OK;
	RC(lift_launch(c, "slot_lift", s.d_place.as<uint4>(), s.n_reads, s.d_locus.as<uint4>(), s.alt.d_alts.as<uint4>(), slot_items(s, max_alt), s.lift));
	s.stage.lift_mm = max_mm; s.stage.lift_alt = max_alt;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_lift(bwb_hip_ctx *c, int si, int max_mm, int max_alt, const uint8_t **kinds, const uint64_t **lift_off, const bwb_lift **recs, uint64_t *n_placements) {
	if (!c || !kinds || !lift_off || !recs || !n_placements || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_lift: bad argument");
	RC(ensure_lift(c, si, max_mm, max_alt));
	const Slot &s = c->slots[si];
	*kinds = s.lift.h_kind.as<uint8_t>();
	*lift_off = s.lift.h_off.as<uint64_t>();
	*recs = s.lift.h_recs.as<bwb_lift>();
	*n_placements = (uint64_t)s.n_reads + slot_items(s, max_alt);
	return BWB_OK;
}

extern "C" int bwb_hip_batch_lift(bwb_hip_ctx *c, int max_mm, int max_alt, const uint8_t **kinds, const uint64_t **lift_off, const bwb_lift **recs, uint64_t *n_placements) {
	if (!c || !kinds || !lift_off || !recs || !n_placements) return fail(BWB_E_ARG, "batch_lift: null argument");
	RC(lift_ready(c, "batch_lift", max_alt));
	RC(batch_ready(c, "batch_lift"));
	return bwb_hip_slot_lift(c, 0, max_mm, max_alt, kinds, lift_off, recs, n_placements);
}

/* the kernels on records of the caller's instead of a slot's (for parity tests): k_locus for the primaries' loci, then the lift kernels */
extern "C" int bwb_hip_lift_records(bwb_hip_ctx *c, const bwb_place *places, uint32_t n, const uint64_t *alt_off, const bwb_alt *alts, const uint8_t **kinds,
                                    const uint64_t **lift_off, const bwb_lift **recs) {
	if (!c || !alt_off || !kinds || !lift_off || !recs || (n && !places) || n > 0x7FFFFFFFu) return fail(BWB_E_ARG, "lift_records: bad argument");
	RC(lift_ready(c, "lift_records", 1));
	RC(check_offsets("lift_records", "alt_off", alt_off, n, NO_LIMIT));
	const uint64_t n_items = alt_off[n];
	if (n_items && !alts) return fail(BWB_E_ARG, "lift_records: null argument");
	if ((uint64_t)n + n_items > 0x7FFFFFFFu) return fail(BWB_E_ARG, "lift_records: more than 2^31 - 1 placements");
	HIPCHK(hipSetDevice(c->device));
	DevMem d_places, d_loci, d_alts;
	RC(stage_in(c, d_places, places, (size_t)n * sizeof(bwb_place)));
	RC(stage_in(c, d_alts, alts, (size_t)n_items * sizeof(bwb_alt)));
	HIPCHK(d_loci.alloc((size_t)n * sizeof(bwb_locus)));
	HIPCHK(hipStreamSynchronize(c->rstream));
	std::vector<bwb_locus> h_loci(n ? n : 1);
	RC(locus_launch(c, d_places.as<uint4>(), n, d_loci.as<uint4>(), h_loci.data()));
	RC(lift_launch(c, "lift_records", d_places.as<uint4>(), n, d_loci.as<uint4>(), d_alts.as<uint4>(), n_items, c->lift_rec));
	*kinds = c->lift_rec.h_kind.as<uint8_t>();
	*lift_off = c->lift_rec.h_off.as<uint64_t>();
	*recs = c->lift_rec.h_recs.as<bwb_lift>();
	return BWB_OK;
}

/* the last lift call: placements lifted, placements on a bubble record that are not liftable, and the kernels' HIP-event time */
extern "C" int bwb_hip_lift_stats(bwb_hip_ctx *c, uint64_t *lifted, uint64_t *unliftable, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "lift_stats: null context");
	if (lifted) *lifted = c->lift_lifted;
	if (unliftable) *unliftable = c->lift_unliftable;
	if (kernel_ms) *kernel_ms = c->lift_ms;
	return BWB_OK;
}

/* ---- NM:i and MD:Z against the text: bwb_md records and the MD bytes (k_text_pack, k_md_count, k_md) ------------------------------------ */
static_assert(sizeof(bwb_md) == 8, "bwb_md is one 8-byte word (k_md_count)");
static_assert(BWB_MD_NONE == MD_NONE && BWB_MD_OK == MD_OK && BWB_MD_TOO_LONG == MD_TOO_LONG && BWB_MD_MAX_SPAN == MD_MAX_SPAN, "the kernels' kinds are the header's");
#ifndef BWB_TEXT_CHUNK_SHIFT
#define BWB_TEXT_CHUNK_SHIFT (BWB_IDX_CHUNK_SHIFT + 5) /* text characters per staged chunk of set_text = 2^25 (the test build: 2^15, so that a text of 40 000 characters takes two) */
#endif
extern "C" int bwb_hip_set_text(bwb_hip_ctx *c, const uint8_t *codes, uint64_t n_fwd) {
	if (!c || !codes || !n_fwd) return fail(BWB_E_ARG, "set_text: null argument or an empty text");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->rstream)); /* (a kernel of an earlier md call may still read the text that is replaced) */
	c->text_n = 0;
	for (auto &s : c->slots) s.stage.text_replaced();
	c->pile_on = false; c->pile_sites = 0; /* (the site index and the counters were this text's) */
	c->d_site_base.release(); c->d_counts.release();
	c->pileq_on = false; c->pileq_weighted = false; c->d_qsum.release();
	c->geno_on = false; c->geno_bub = false;
	const uint64_t CH = 1ull << BWB_TEXT_CHUNK_SHIFT, n_words = (n_fwd + 31) / 32;
	HIPCHK(c->d_text.alloc((size_t)n_words * 16));
	DevMem d_stage, d_bad;
	HIPCHK(d_stage.alloc((size_t)std::min<uint64_t>(CH, n_words * 32)));
	HIPCHK(d_bad.alloc(4));
	HIPCHK(hipMemsetAsync(d_bad.p, 0, 4, c->rstream));
	for (uint64_t c0 = 0; c0 < n_fwd; c0 += CH) { /* (CH is a multiple of 32: every chunk begins a 16-byte word of the packed text) */
		const uint64_t nc = std::min<uint64_t>(CH, n_fwd - c0), nw = (nc + 31) / 32;
		HIPCHK(hipMemcpyAsync(d_stage.p, codes + c0, (size_t)nc, hipMemcpyHostToDevice, c->rstream));
		hipLaunchKernelGGL(k_text_pack, dim3(lane_grid(c, nw)), dim3(BWB_BLOCK), 0, c->rstream, d_stage.as<uint8_t>(), nc, c->d_text.as<uint4>() + c0 / 32, d_bad.as<uint32_t>());
		HIPCHK(hipGetLastError());
	}
	uint32_t bad = 0;
	HIPCHK(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	if (bad) { c->d_text.release(); return fail(BWB_E_ARG, "set_text: the text holds a code above 15"); }
	c->text_n = n_fwd;
	return BWB_OK;
}

/* k_md_count, the scan and k_md over n reads (reads, lengths, placement records and - d_kind NULL: none - lift records, all device memory) ->
 * mb.h_recs[n], mb.h_off[n + 1] and mb.h_text[h_off[n]]; sets the context's md_ms / md_reads / md_bytes.  On the result stream, behind the kernels
 * that wrote the records.  The only host round trip is the read of the total, which sizes the text buffers: they hold the bytes there are.  Eight
 * blocks per CU, the grid of k_locus and the lift kernels: a lane's walk is a chain of dependent loads, and the waves beside it are what hides
 * their latency.  Shared by slot_md and md_records. */
static int md_launch(bwb_hip_ctx *c, const uint8_t *d_reads, const uint16_t *d_lens, uint32_t stride, const uint4 *d_places, uint32_t n, const uint8_t *d_kind, const uint64_t *d_loff,
                     const uint4 *d_lrecs, MdBufs &mb) {
	c->md_ms = 0; c->md_reads = 0; c->md_bytes = 0;
	HIPCHK(mb.h_off.reserve(((size_t)n + 1) * 8));
	HIPCHK(mb.h_recs.reserve((size_t)n * sizeof(bwb_md)));
	HIPCHK(mb.h_text.reserve(1));
	mb.h_off.as<uint64_t>()[0] = 0;
	if (!n) return BWB_OK;
	const unsigned grid = lane_grid(c, n);
	HIPCHK(mb.d_recs.reserve((size_t)n * sizeof(bwb_md)));
	HIPCHK(mb.d_cnt.reserve((size_t)n * 4));
	HIPCHK(mb.d_off.reserve(((size_t)n + 1) * 8));
	HIPCHK(mb.d_bsum.reserve((size_t)blocks_of(n) * 8));
	uint64_t *d_off = mb.d_off.as<uint64_t>();
	const uint32_t n_seq = d_kind ? c->loci_nseq : 0u;
	Timed t_count(c, c->rstream), t_md(c, c->rstream); /* k_md_count and the scan; k_md */
	RC(t_count.begin());
	hipLaunchKernelGGL(k_md_count, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, d_reads, d_lens, stride, d_places, n, d_kind, d_loff, d_lrecs, c->d_lstart.as<uint64_t>(), n_seq,
	                   c->d_text.as<uint4>(), c->text_n, mb.d_recs.as<uint2>(), mb.d_cnt.as<uint32_t>());
	scan_offsets(c, mb.d_cnt.as<uint32_t>(), n, d_off, mb.d_bsum.as<uint64_t>());
	HIPCHK(hipGetLastError());
	RC(t_count.end());
	HIPCHK(hipMemcpyAsync(mb.h_off.p, d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipMemcpyAsync(mb.h_recs.p, mb.d_recs.p, (size_t)n * sizeof(bwb_md), hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	const uint64_t total = mb.h_off.as<uint64_t>()[n];
	float ms = 0, ms2 = 0;
	RC(t_count.ms(&ms));
	if (total) {
		HIPCHK(mb.d_text.reserve((size_t)total));
		HIPCHK(mb.h_text.reserve((size_t)total));
		RC(t_md.begin());
		hipLaunchKernelGGL(k_md, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, d_reads, d_lens, stride, d_places, n, d_kind, d_loff, d_lrecs, c->d_lstart.as<uint64_t>(), n_seq,
		                   c->d_text.as<uint4>(), mb.d_recs.as<uint2>(), (const uint64_t *)d_off, mb.d_text.as<char>());
		HIPCHK(hipGetLastError());
		RC(t_md.end());
		HIPCHK(hipMemcpyAsync(mb.h_text.p, mb.d_text.p, (size_t)total, hipMemcpyDeviceToHost, c->rstream));
		HIPCHK(hipStreamSynchronize(c->rstream));
		RC(t_md.ms(&ms2));
	}
	c->md_ms = (double)ms + ms2;
	c->md_bytes = total;
	const bwb_md *recs = mb.h_recs.as<bwb_md>();
	for (uint32_t q = 0; q < n; q++) c->md_reads += recs[q].kind == BWB_MD_OK;
	return BWB_OK;
}

/* (a cached call leaves md_stats at the last launch's figures, whichever slot's: a caller that sums them - retire_map - asks every slot once) */
static int ensure_md(bwb_hip_ctx *c, int si, int max_mm, int max_alt, bool lifted) {
	RC(lifted ? ensure_lift(c, si, max_mm, max_alt) : ensure_place(c, si, max_mm));
	Slot &s = c->slots[si];
	const uint32_t n = s.n_reads; /* (not n_tot: a carried read that rides along behind the batch's reads has no record) */
	if (s.stage.md_mm == max_mm && s.stage.md_lifted == (int)lifted && (!lifted || s.stage.md_alt == max_alt) && n) return BWB_OK;
	HIPCHK(hipStreamWaitEvent(c->rstream, s.ev_up.e, 0)); /* (the slot's reads, uploaded on the copy stream) */
	/* (a slot whose every placement lies on no bubble record has no lift records at all: d_recs may be NULL, and no lane reads it) */
	RC(md_launch(c, s.d_reads.as<uint8_t>(), s.d_lens.as<uint16_t>(), s.stride, s.d_place.as<uint4>(), n, lifted ? s.lift.d_kind.as<uint8_t>() : nullptr,
	             s.lift.d_off.as<uint64_t>(), s.lift.d_recs.as<uint4>(), s.md));
	s.stage.md_mm = max_mm; s.stage.md_alt = max_alt; s.stage.md_lifted = (int)lifted;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_md(bwb_hip_ctx *c, int si, int max_mm, int max_alt, int lifted, const bwb_md **recs, const uint64_t **md_off, const char **md_text, uint32_t *n_reads) {
	if (!c || !recs || !md_off || !md_text || !n_reads || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_md: bad argument");
	if (!c->text_n) return fail(BWB_E_STATE, "slot_md: the text has not been uploaded (bwb_hip_set_text)");
	if (!c->d_SA.p) return fail(BWB_E_STATE, "slot_md: sampled SA not uploaded (bwb_hip_set_sa)");
	RC(ensure_md(c, si, max_mm, max_alt, lifted != 0));
	const Slot &s = c->slots[si];
	*recs = s.md.h_recs.as<bwb_md>();
	*md_off = s.md.h_off.as<uint64_t>();
	*md_text = s.md.h_text.as<char>();
	*n_reads = s.n_reads;
	return BWB_OK;
}

extern "C" int bwb_hip_batch_md(bwb_hip_ctx *c, int max_mm, int max_alt, int lifted, const bwb_md **recs, const uint64_t **md_off, const char **md_text, uint32_t *n_reads) {
	if (!c || !recs || !md_off || !md_text || !n_reads) return fail(BWB_E_ARG, "batch_md: null argument");
	if (!c->text_n) return fail(BWB_E_STATE, "batch_md: the text has not been uploaded (bwb_hip_set_text)");
	RC(batch_ready(c, "batch_md"));
	return bwb_hip_slot_md(c, 0, max_mm, max_alt, lifted, recs, md_off, md_text, n_reads);
}

/* what md_records and pile_records are given, in device memory: n reads, their lengths and placement records, and - kinds NULL: none, and kind, loff
 * and lrecs stay NULL - their lift records.  Checks the lift arrays under the caller's name; the caller synchronises (stage_in). */
struct StagedReads { DevMem reads, lens, places, kind, loff, lrecs; };
static int stage_reads(bwb_hip_ctx *c, const char *who, const uint8_t *reads_fwd, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n, const uint8_t *kinds,
                       const uint64_t *lift_off, const bwb_lift *lift_recs, StagedReads &in) {
	if (kinds && !c->loci_nseq) return fail(BWB_E_STATE, std::string(who) + ": lift records need the record table (bwb_hip_set_loci)");
	if (kinds) RC(check_offsets(who, "lift_off", lift_off, n, NO_LIMIT));
	const uint64_t words = kinds ? lift_off[n] : 0;
	if (words && !lift_recs) return fail(BWB_E_ARG, std::string(who) + ": null argument");
	HIPCHK(hipSetDevice(c->device));
	RC(stage_in(c, in.reads, reads_fwd, (size_t)n * stride));
	RC(stage_in(c, in.lens, lens, (size_t)n * 2));
	RC(stage_in(c, in.places, places, (size_t)n * sizeof(bwb_place)));
	if (!kinds) return BWB_OK;
	RC(stage_in(c, in.kind, kinds, (size_t)n));
	RC(stage_in(c, in.loff, lift_off, ((size_t)n + 1) * 8));
	return stage_in(c, in.lrecs, lift_recs, (size_t)words * sizeof(bwb_lift));
}

/* the kernels on reads and records of the caller's instead of a slot's (for parity tests) */
extern "C" int bwb_hip_md_records(bwb_hip_ctx *c, const uint8_t *reads_fwd, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n, const uint8_t *kinds,
                                  const uint64_t *lift_off, const bwb_lift *lift_recs, const bwb_md **recs, const uint64_t **md_off, const char **md_text) {
	if (!c || !recs || !md_off || !md_text || (n && (!reads_fwd || !lens || !places)) || n > 0x7FFFFFFFu || stride < 1 || stride > 255) return fail(BWB_E_ARG, "md_records: bad argument");
	if ((kinds != nullptr) != (lift_off != nullptr)) return fail(BWB_E_ARG, "md_records: the lift kinds and offsets come together");
	if (!c->text_n) return fail(BWB_E_STATE, "md_records: the text has not been uploaded (bwb_hip_set_text)");
	StagedReads in;
	RC(stage_reads(c, "md_records", reads_fwd, lens, stride, places, n, kinds, lift_off, lift_recs, in));
	HIPCHK(hipStreamSynchronize(c->rstream));
	RC(md_launch(c, in.reads.as<uint8_t>(), in.lens.as<uint16_t>(), stride, in.places.as<uint4>(), n, in.kind.as<uint8_t>(), in.loff.as<uint64_t>(), in.lrecs.as<uint4>(), c->md_rec));
	*recs = c->md_rec.h_recs.as<bwb_md>();
	*md_off = c->md_rec.h_off.as<uint64_t>();
	*md_text = c->md_rec.h_text.as<char>();
	return BWB_OK;
}

/* the last md call: reads that got their tags, MD bytes written, and the kernels' HIP-event time */
extern "C" int bwb_hip_md_stats(bwb_hip_ctx *c, uint64_t *reads, uint64_t *md_bytes, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "md_stats: null context");
	if (reads) *reads = c->md_reads;
	if (md_bytes) *md_bytes = c->md_bytes;
	if (kernel_ms) *kernel_ms = c->md_ms;
	return BWB_OK;
}

/* ---- allele counts at the text's IUPAC sites (k_site_count, k_site_add, k_pile, k_site_of) ---------------------------------------------- */
extern "C" int bwb_hip_pile_begin(bwb_hip_ctx *c, uint64_t *n_sites) {
	if (!c || !n_sites) return fail(BWB_E_ARG, "pile_begin: null argument");
	if (!c->text_n) return fail(BWB_E_STATE, "pile_begin: the text has not been uploaded (bwb_hip_set_text)");
	const uint64_t n_words = (c->text_n + 31) / 32;
	if (n_words > 0xFFFFFFFFull) return fail(BWB_E_ARG, "pile_begin: the text has more than 2^32 - 1 words of 32 characters");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->rstream)); /* (a pile kernel of an earlier call may still add to the counters that are replaced) */
	c->pile_on = false; c->pile_sites = 0;
	c->pileq_on = false; c->pileq_weighted = false; c->d_qsum.release(); /* (pileq_begin comes behind its pile_begin) */
	c->geno_on = false; c->geno_bub = false; /* (the calls were for this index and these counters) */
	const unsigned nblk = blocks_of(n_words);
	DevMem d_bsum, d_total;
	HIPCHK(c->d_site_base.alloc((size_t)n_words * 4));
	HIPCHK(d_bsum.alloc((size_t)nblk * 8));
	HIPCHK(d_total.alloc(8));
	hipLaunchKernelGGL(k_site_count, dim3(nblk), dim3(BWB_BLOCK), 0, c->rstream, c->d_text.as<uint4>(), (uint32_t)n_words, c->d_site_base.as<uint32_t>(), d_bsum.as<uint64_t>());
	hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(BWB_BLOCK), 0, c->rstream, d_bsum.as<uint64_t>(), (uint32_t)nblk, d_total.as<uint64_t>());
	hipLaunchKernelGGL(k_site_add, dim3(nblk), dim3(BWB_BLOCK), 0, c->rstream, c->d_site_base.as<uint32_t>(), (uint32_t)n_words, d_bsum.as<uint64_t>());
	HIPCHK(hipGetLastError());
	uint64_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, d_total.p, 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	if (total > 0xFFFFFFFFull) { c->d_site_base.release(); return fail(BWB_E_ARG, "pile_begin: the text has more than 2^32 - 1 sites"); }
	HIPCHK(c->d_counts.alloc((size_t)total * 16));
	if (total) HIPCHK(hipMemsetAsync(c->d_counts.p, 0, (size_t)total * 16, c->rstream));
	RC(c->pile_fig.begin(16));
	HIPCHK(hipStreamSynchronize(c->rstream));
	c->pile_on = true; c->pile_sites = total;
	c->pile_fig.zero();
	*n_sites = total;
	return BWB_OK;
}

/* the quality part of a pile call (k_pile_q); a null pointer to it is the plain form (k_pile) */
struct PileQuals { const uint8_t *d_quals; int min_baseq, err_cap; };

/* k_pile - with q, k_pile_q - over n reads (reads, lengths, placement records, - d_kind NULL: none - lift records and - d_mapq NULL: the placement's
 * own - one MAPQ byte every mapq_stride bytes, all device memory) into the context's counters; sets the figures of its form, pile_fig or pileq_fig.
 * On the result stream, behind the kernels that wrote the records; the grid of the md kernels, for their reason (a lane's walk is a chain of
 * dependent loads).  What comes back is the 16 bytes of the two sums, or the 24 of the three. */
static int pile_launch(bwb_hip_ctx *c, const uint8_t *d_reads, const uint16_t *d_lens, uint32_t stride, const uint4 *d_places, uint32_t n, const uint8_t *d_kind, const uint64_t *d_loff,
                       const uint4 *d_lrecs, const uint8_t *d_mapq, uint32_t mapq_stride, int min_mapq, const PileQuals *q) {
	if (!n) return BWB_OK; /* (nothing launched: the figures of the last launch stay) */
	PileFigures &f = q ? c->pileq_fig : c->pile_fig;
	const size_t bytes = q ? 24 : 16;
	const uint32_t n_seq = d_kind ? c->loci_nseq : 0u;
	HIPCHK(hipMemsetAsync(f.d_stats.p, 0, bytes, c->rstream));
	Timed t(c, c->rstream);
	RC(t.begin());
	if (q)
		hipLaunchKernelGGL(k_pile_q, dim3(lane_grid(c, n)), dim3(BWB_BLOCK), 0, c->rstream, d_reads, q->d_quals, d_lens, stride, d_places, n, d_kind, d_loff, d_lrecs, c->d_lstart.as<uint64_t>(), n_seq,
		                   c->d_text.as<uint4>(), c->text_n, d_mapq, mapq_stride, (uint32_t)min_mapq, (uint32_t)q->min_baseq, (uint32_t)q->err_cap, c->d_site_base.as<uint32_t>(),
		                   c->d_counts.as<uint32_t>(), c->d_qsum.as<uint32_t>(), f.d_stats.as<unsigned long long>());
	else
		hipLaunchKernelGGL(k_pile, dim3(lane_grid(c, n)), dim3(BWB_BLOCK), 0, c->rstream, d_reads, d_lens, stride, d_places, n, d_kind, d_loff, d_lrecs, c->d_lstart.as<uint64_t>(), n_seq,
		                   c->d_text.as<uint4>(), c->text_n, d_mapq, mapq_stride, (uint32_t)min_mapq, c->d_site_base.as<uint32_t>(), c->d_counts.as<uint32_t>(),
		                   f.d_stats.as<unsigned long long>());
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipMemcpyAsync(f.h_stats.p, f.d_stats.p, bytes, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	float ms = 0;
	RC(t.ms(&ms));
	f.ms = ms;
	f.reads = f.h_stats.as<uint64_t>()[0];
	f.adds = f.h_stats.as<uint64_t>()[1];
	f.dropped = q ? f.h_stats.as<uint64_t>()[2] : 0;
	return BWB_OK;
}

static int pile_ready(bwb_hip_ctx *c, const char *who, int max_alt, int lifted, int joined, int min_mapq) {
	if (min_mapq < 0 || min_mapq > 255) return fail(BWB_E_ARG, std::string(who) + ": min_mapq must be 0..255");
	if (max_alt < 0 || max_alt > 255) return fail(BWB_E_ARG, std::string(who) + ": max_alt must be 0..255");
	if (!c->pile_on) return fail(BWB_E_STATE, std::string(who) + ": no site index and counters (bwb_hip_pile_begin)");
	if (!c->d_SA.p) return fail(BWB_E_STATE, std::string(who) + ": sampled SA not uploaded (bwb_hip_set_sa)");
	if (lifted) RC(lift_ready(c, who, max_alt));
	if (joined) {
		if (!max_alt) return fail(BWB_E_STATE, std::string(who) + ": the joined MAPQ needs the items of max_alt 1..255");
		RC(join_ready(c, who, max_alt));
	}
	return BWB_OK;
}

static int pileq_args(bwb_hip_ctx *c, const char *who, int min_baseq, int err_cap) {
	if (min_baseq < 0 || min_baseq > 93) return fail(BWB_E_ARG, std::string(who) + ": min_baseq must be 0..93");
	if (err_cap != 0 && (err_cap < 4 || err_cap > 93)) return fail(BWB_E_ARG, std::string(who) + ": err_cap must be 0 or 4..93");
	if (!c->pile_on) return fail(BWB_E_STATE, std::string(who) + ": no site index and counters (bwb_hip_pile_begin)");
	if (!c->pileq_on) return fail(BWB_E_STATE, std::string(who) + ": no quality buffers (bwb_hip_pileq_begin)");
	if (err_cap && !c->pileq_weighted) return fail(BWB_E_STATE, std::string(who) + ": no quality sums (bwb_hip_pileq_begin with weighted != 0)");
	return BWB_OK;
}

/* bwb_hip_slot_pile and, with q (its d_quals is set here, to the slot's), bwb_hip_slot_pile_q */
static int slot_pile(bwb_hip_ctx *c, const char *who, int si, int max_mm, int max_alt, int lifted, int joined, int min_mapq, PileQuals *q, uint64_t *reads_counted) {
	if (!c || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, std::string(who) + ": bad argument");
	if (q) RC(pileq_args(c, who, q->min_baseq, q->err_cap));
	RC(pile_ready(c, who, max_alt, lifted, joined, min_mapq));
	if (reads_counted) *reads_counted = 0;
	RC(ensure_place(c, si, max_mm));
	Slot &s = c->slots[si];
	if (s.stage.piled) return BWB_OK; /* (a submission is counted once, by slot_pile or by slot_pile_q) */
	if (q && !s.quals_set) return fail(BWB_E_STATE, std::string(who) + ": the slot's upload has no qualities (bwb_hip_slot_quals)");
	if (lifted) RC(ensure_lift(c, si, max_mm, max_alt));
	if (joined) RC(ensure_join(c, si, max_mm, max_alt));
	const uint32_t n = s.n_reads; /* (not n_tot: a carried read that rides along behind the batch's reads has no record) */
	if (n) {
		HIPCHK(hipStreamWaitEvent(c->rstream, s.ev_up.e, 0)); /* (the slot's reads and, with q, its qualities, uploaded on the copy stream) */
		if (q) { HIPCHK(hipStreamWaitEvent(c->rstream, s.ev_quals.e, 0)); q->d_quals = s.d_quals.as<uint8_t>(); }
		RC(pile_launch(c, s.d_reads.as<uint8_t>(), s.d_lens.as<uint16_t>(), s.stride, s.d_place.as<uint4>(), n, lifted ? s.lift.d_kind.as<uint8_t>() : nullptr,
		               s.lift.d_off.as<uint64_t>(), s.lift.d_recs.as<uint4>(), joined ? s.d_join.as<uint8_t>() + offsetof(bwb_join, mapq) : nullptr, (uint32_t)sizeof(bwb_join), min_mapq, q));
		if (reads_counted) *reads_counted = (q ? c->pileq_fig : c->pile_fig).reads;
	}
	s.stage.piled = true;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_pile(bwb_hip_ctx *c, int si, int max_mm, int max_alt, int lifted, int joined, int min_mapq, uint64_t *reads_counted) {
	return slot_pile(c, "slot_pile", si, max_mm, max_alt, lifted, joined, min_mapq, nullptr, reads_counted);
}

extern "C" int bwb_hip_batch_pile(bwb_hip_ctx *c, int max_mm, int max_alt, int lifted, int joined, int min_mapq, uint64_t *reads_counted) {
	if (!c) return fail(BWB_E_ARG, "batch_pile: null context");
	RC(pile_ready(c, "batch_pile", max_alt, lifted, joined, min_mapq));
	RC(batch_ready(c, "batch_pile"));
	return bwb_hip_slot_pile(c, 0, max_mm, max_alt, lifted, joined, min_mapq, reads_counted);
}

/* the kernel on reads and records of the caller's instead of a slot's (for parity tests): bwb_hip_pile_records and, with q and the caller's quality
 * bytes (staged here: its d_quals is set to them; needs no slot_quals), bwb_hip_pile_records_q */
static int pile_records(bwb_hip_ctx *c, const char *who, const uint8_t *reads_fwd, const uint8_t *quals, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n,
                        const uint8_t *kinds, const uint64_t *lift_off, const bwb_lift *lift_recs, const uint8_t *mapq, int min_mapq, PileQuals *q) {
	if (!c || (n && (!reads_fwd || (q && !quals) || !lens || !places)) || n > 0x7FFFFFFFu || stride < 1 || stride > 255) return fail(BWB_E_ARG, std::string(who) + ": bad argument");
	if ((kinds != nullptr) != (lift_off != nullptr)) return fail(BWB_E_ARG, std::string(who) + ": the lift kinds and offsets come together");
	if (min_mapq < 0 || min_mapq > 255) return fail(BWB_E_ARG, std::string(who) + ": min_mapq must be 0..255");
	if (q) RC(pileq_args(c, who, q->min_baseq, q->err_cap));
	else if (!c->pile_on) return fail(BWB_E_STATE, std::string(who) + ": no site index and counters (bwb_hip_pile_begin)");
	StagedReads in;
	DevMem d_mapq, d_quals; /* (d_mapq stays NULL without a MAPQ array, and without reads) */
	RC(stage_reads(c, who, reads_fwd, lens, stride, places, n, kinds, lift_off, lift_recs, in));
	if (q) { RC(stage_in(c, d_quals, quals, (size_t)n * stride)); q->d_quals = d_quals.as<uint8_t>(); }
	if (mapq && n) RC(stage_in(c, d_mapq, mapq, (size_t)n));
	HIPCHK(hipStreamSynchronize(c->rstream));
	return pile_launch(c, in.reads.as<uint8_t>(), in.lens.as<uint16_t>(), stride, in.places.as<uint4>(), n, in.kind.as<uint8_t>(), in.loff.as<uint64_t>(), in.lrecs.as<uint4>(),
	                   d_mapq.as<uint8_t>(), 1u, min_mapq, q);
}

extern "C" int bwb_hip_pile_records(bwb_hip_ctx *c, const uint8_t *reads_fwd, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n, const uint8_t *kinds,
                                    const uint64_t *lift_off, const bwb_lift *lift_recs, const uint8_t *mapq, int min_mapq) {
	return pile_records(c, "pile_records", reads_fwd, nullptr, lens, stride, places, n, kinds, lift_off, lift_recs, mapq, min_mapq, nullptr);
}

/* The two counter tables, four 32-bit counters per entry: the sites' (pile_begin) and the bubbles' (indel_begin).  What the counts / put / reset calls
 * of either need: the buffer, its entries, whether its *_begin has run, and the words of the messages. */
struct CounterTable { const DevMem &buf; uint64_t entries; bool on; const char *missing, *unit; };
static CounterTable site_counters(const bwb_hip_ctx *c) { return { c->d_counts, c->pile_sites, c->pile_on, "no site index and counters (bwb_hip_pile_begin)", "sites" }; }
static CounterTable qsum_counters(const bwb_hip_ctx *c) { return { c->d_qsum, c->pile_sites, c->pile_on && c->pileq_weighted, "no quality sums (bwb_hip_pileq_begin with weighted != 0)", "sites" }; }
static CounterTable bubble_counters(const bwb_hip_ctx *c) { return { c->d_indel_counts, c->loci_nbub, c->indel_on, "no bubble table and counters (bwb_hip_indel_begin)", "bubbles" }; }
/* n entries from `first` on, device to host or host to device (pageable memory of the caller: waits for the copy) */
static int counters_copy(bwb_hip_ctx *c, const char *who, const CounterTable &t, uint64_t first, uint64_t n, const void *host, hipMemcpyKind kind) {
	if (n && !host) return fail(BWB_E_ARG, std::string(who) + ": null argument");
	if (!t.on) return fail(BWB_E_STATE, std::string(who) + ": " + t.missing);
	if (first > t.entries || n > t.entries - first) return fail(BWB_E_ARG, std::string(who) + ": the range leaves the " + std::to_string(t.entries) + " " + t.unit);
	HIPCHK(hipSetDevice(c->device));
	void *dev = t.buf.as<uint32_t>() + first * 4, *h = const_cast<void *>(host); /* (written device to host only: the counts calls' pointer is not const) */
	const bool put = kind == hipMemcpyHostToDevice;
	if (n) HIPCHK(hipMemcpyAsync(put ? dev : h, put ? h : dev, (size_t)n * 16, kind, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	return BWB_OK;
}
static int counters_reset(bwb_hip_ctx *c, const char *who, const CounterTable &t) {
	if (!t.on) return fail(BWB_E_STATE, std::string(who) + ": " + t.missing);
	HIPCHK(hipSetDevice(c->device));
	if (t.entries) HIPCHK(hipMemsetAsync(t.buf.p, 0, (size_t)t.entries * 16, c->rstream));
	return BWB_OK;
}

extern "C" int bwb_hip_pile_counts(bwb_hip_ctx *c, uint64_t first, uint64_t n, uint32_t *out) {
	if (!c) return fail(BWB_E_ARG, "pile_counts: null argument");
	return counters_copy(c, "pile_counts", site_counters(c), first, n, out, hipMemcpyDeviceToHost);
}

extern "C" int bwb_hip_pile_reset(bwb_hip_ctx *c) {
	if (!c) return fail(BWB_E_ARG, "pile_reset: null context");
	RC(counters_reset(c, "pile_reset", site_counters(c)));
	return c->pileq_weighted ? counters_reset(c, "pile_reset", qsum_counters(c)) : BWB_OK;
}

extern "C" int bwb_hip_pile_site_of(bwb_hip_ctx *c, const uint64_t *pos, size_t n, int64_t *site) {
	if (!c || (n && (!pos || !site))) return fail(BWB_E_ARG, "pile_site_of: null argument");
	if (!c->pile_on) return fail(BWB_E_STATE, "pile_site_of: no site index and counters (bwb_hip_pile_begin)");
	for (size_t i = 0; i < n; i++)
		if (pos[i] >= c->text_n) return fail(BWB_E_ARG, "pile_site_of: position outside the text");
	if (n == 0) return BWB_OK;
	HIPCHK(hipSetDevice(c->device));
	DevMem dp, dout;
	HIPCHK(dp.alloc(n * 8));
	HIPCHK(dout.alloc(n * 8));
	HIPCHK(hipMemcpyAsync(dp.p, pos, n * 8, hipMemcpyHostToDevice, c->rstream));
	hipLaunchKernelGGL(k_site_of, dim3(lane_grid(c, n)), dim3(BWB_BLOCK), 0, c->rstream, c->d_text.as<uint4>(), c->d_site_base.as<uint32_t>(), dp.as<uint64_t>(), (uint64_t)n, dout.as<int64_t>());
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(site, dout.p, n * 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	return BWB_OK;
}

/* the last pile call that launched: reads counted, adds made, and the kernel's HIP-event time */
extern "C" int bwb_hip_pile_stats(bwb_hip_ctx *c, uint64_t *reads, uint64_t *adds, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "pile_stats: null context");
	if (reads) *reads = c->pile_fig.reads;
	if (adds) *adds = c->pile_fig.adds;
	if (kernel_ms) *kernel_ms = c->pile_fig.ms;
	return BWB_OK;
}

/* ---- the pile with base qualities (k_pile_q): a minimum base quality, and the quality sums the weighted calls need ----------------------------- */
extern "C" int bwb_hip_pileq_begin(bwb_hip_ctx *c, int weighted) {
	if (!c) return fail(BWB_E_ARG, "pileq_begin: null context");
	if (!c->pile_on) return fail(BWB_E_STATE, "pileq_begin: no site index and counters (bwb_hip_pile_begin)");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->rstream)); /* (a kernel of an earlier call may still add to the sums that are replaced) */
	c->pileq_on = false; c->pileq_weighted = false;
	c->d_qsum.release();
	if (weighted) {
		HIPCHK(c->d_qsum.alloc((size_t)c->pile_sites * 16));
		if (c->pile_sites) HIPCHK(hipMemsetAsync(c->d_qsum.p, 0, (size_t)c->pile_sites * 16, c->rstream));
	}
	RC(c->pileq_fig.begin(24));
	HIPCHK(hipStreamSynchronize(c->rstream));
	c->pileq_on = true; c->pileq_weighted = weighted != 0;
	c->pileq_fig.zero();
	return BWB_OK;
}

extern "C" int bwb_hip_slot_quals(bwb_hip_ctx *c, int si, const uint8_t *quals, uint32_t stride) {
	if (!c || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_quals: bad argument");
	if (!c->pileq_on) return fail(BWB_E_STATE, "slot_quals: no quality buffers (bwb_hip_pileq_begin)");
	Slot &s = c->slots[si];
	if (!s.uploaded) return fail(BWB_E_STATE, "slot_quals: the slot has no upload");
	if (stride != s.up_stride) return fail(BWB_E_ARG, "slot_quals: the stride is " + std::to_string(stride) + ", the upload's " + std::to_string(s.up_stride));
	if (s.n_reads && !quals) return fail(BWB_E_ARG, "slot_quals: null argument");
	HIPCHK(hipSetDevice(c->device));
	const size_t bytes = (size_t)s.n_reads * s.stride;
	HIPCHK(s.ev_quals.create());
	HIPCHK(hipEventSynchronize(s.ev_quals.e)); /* (the slot's previous copy has left the staging buffer; an event never recorded is complete) */
	HIPCHK(s.d_quals.reserve(bytes)); /* (slot_upload sized it when pileq_begin came first) */
	HIPCHK(s.h_quals.reserve(bytes));
	uint8_t *hq = s.h_quals.as<uint8_t>();
	/* (the slot's stride is the upload's clamped to its longest read: the bytes behind it belong to no base) */
	if (s.stride == stride) memcpy(hq, quals, bytes);
	else for (uint32_t i = 0; i < s.n_reads; i++) memcpy(hq + (size_t)i * s.stride, quals + (size_t)i * stride, s.stride);
	if (bytes) HIPCHK(hipMemcpyAsync(s.d_quals.p, hq, bytes, hipMemcpyHostToDevice, c->cstream));
	HIPCHK(hipEventRecord(s.ev_quals.e, c->cstream));
	s.quals_set = true;
	return BWB_OK;
}

extern "C" int bwb_hip_slot_pile_q(bwb_hip_ctx *c, int si, int max_mm, int max_alt, int lifted, int joined, int min_mapq, int min_baseq, int err_cap, uint64_t *reads_counted) {
	PileQuals q = { nullptr, min_baseq, err_cap };
	return slot_pile(c, "slot_pile_q", si, max_mm, max_alt, lifted, joined, min_mapq, &q, reads_counted);
}

extern "C" int bwb_hip_batch_pile_q(bwb_hip_ctx *c, int max_mm, int max_alt, int lifted, int joined, int min_mapq, int min_baseq, int err_cap, uint64_t *reads_counted) {
	if (!c) return fail(BWB_E_ARG, "batch_pile_q: null context");
	RC(pileq_args(c, "batch_pile_q", min_baseq, err_cap));
	RC(pile_ready(c, "batch_pile_q", max_alt, lifted, joined, min_mapq));
	RC(batch_ready(c, "batch_pile_q"));
	return bwb_hip_slot_pile_q(c, 0, max_mm, max_alt, lifted, joined, min_mapq, min_baseq, err_cap, reads_counted);
}

extern "C" int bwb_hip_pile_records_q(bwb_hip_ctx *c, const uint8_t *reads_fwd, const uint8_t *quals, const uint16_t *lens, uint32_t stride, const bwb_place *places, uint32_t n,
                                      const uint8_t *kinds, const uint64_t *lift_off, const bwb_lift *lift_recs, const uint8_t *mapq, int min_mapq, int min_baseq, int err_cap) {
	PileQuals q = { nullptr, min_baseq, err_cap };
	return pile_records(c, "pile_records_q", reads_fwd, quals, lens, stride, places, n, kinds, lift_off, lift_recs, mapq, min_mapq, &q);
}

extern "C" int bwb_hip_pileq_sums(bwb_hip_ctx *c, uint64_t first, uint64_t n, uint32_t *out) {
	if (!c) return fail(BWB_E_ARG, "pileq_sums: null argument");
	return counters_copy(c, "pileq_sums", qsum_counters(c), first, n, out, hipMemcpyDeviceToHost);
}
extern "C" int bwb_hip_pileq_put(bwb_hip_ctx *c, uint64_t first, uint64_t n, const uint32_t *sums) {
	if (!c) return fail(BWB_E_ARG, "pileq_put: null argument");
	return counters_copy(c, "pileq_put", qsum_counters(c), first, n, sums, hipMemcpyHostToDevice);
}

/* the last pile_q call that launched: reads counted, adds made, bases dropped by min_baseq, and the kernel's HIP-event time */
extern "C" int bwb_hip_pileq_stats(bwb_hip_ctx *c, uint64_t *reads, uint64_t *adds, uint64_t *dropped, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "pileq_stats: null context");
	if (reads) *reads = c->pileq_fig.reads;
	if (adds) *adds = c->pileq_fig.adds;
	if (dropped) *dropped = c->pileq_fig.dropped;
	if (kernel_ms) *kernel_ms = c->pileq_fig.ms;
	return BWB_OK;
}

/* ---- ref / alt read support per indel bubble (k_indel) ------------------------------------------------------------------------------------ */
struct IndelEntry { int64_t lo; int32_t chrom; uint32_t bubble; }; /* one 16-byte word of k_indel's table */
static_assert(sizeof(IndelEntry) == 16, "an entry of the indel table is one 16-byte word (k_indel)");
/* the rule's eligibility (include/bwbble_hip.h), in the wrapping 64-bit arithmetic of the kernels */
static bool indel_eligible(const bwb_bubble &b, int64_t w) {
	const __int128 gap = (__int128)b.C - (__int128)b.A - (__int128)b.B_minus_A;
	if (b.B_minus_A < 0 || b.D_minus_C < -1 || b.alt_len < 0 || gap < 0 || gap >= ((__int128)1 << 28)) return false;
	return b.B_minus_A >= w && b.D_minus_C + 1 >= w && (int64_t)((uint64_t)b.A + (uint64_t)b.B_minus_A - (uint64_t)w) >= 1;
}
extern "C" int bwb_hip_indel_begin(bwb_hip_ctx *c, int anchor, uint64_t *n_eligible) {
	if (!c || !n_eligible) return fail(BWB_E_ARG, "indel_begin: null argument");
	if (anchor < 1 || anchor > 255) return fail(BWB_E_ARG, "indel_begin: the anchor must be 1..255");
	if (!c->loci_nseq) return fail(BWB_E_STATE, "indel_begin: record and bubble tables not uploaded (bwb_hip_set_loci)");
	if (!c->chrom_set) return fail(BWB_E_STATE, "indel_begin: the bubbles' chromosome records not uploaded (bwb_hip_set_bubble_chrom)");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->rstream)); /* (a kernel of an earlier call may still read the table and add to the counters that are replaced) */
	c->indel_on = false;
	c->geno_bub = false; /* (geno_begin sized its bubble output for the table that is replaced) */
	const uint32_t n_bub = c->loci_nbub;
	std::vector<IndelEntry> tab;
	std::vector<uint8_t> elig(n_bub ? n_bub : 1, 0);
	for (uint32_t b = 0; b < n_bub; b++) {
		const bwb_bubble &v = c->loci_bubbles[b];
		if (!indel_eligible(v, anchor)) continue;
		elig[b] = 1;
		tab.push_back(IndelEntry{ (int64_t)((uint64_t)v.A + (uint64_t)v.B_minus_A - (uint64_t)anchor), c->chrom_of[b], b });
	}
	std::sort(tab.begin(), tab.end(), [](const IndelEntry &x, const IndelEntry &y) {
		return x.chrom != y.chrom ? x.chrom < y.chrom : x.lo != y.lo ? x.lo < y.lo : x.bubble < y.bubble; });
	HIPCHK(c->d_indel_tab.alloc(tab.size() * sizeof(IndelEntry)));
	HIPCHK(c->d_indel_elig.alloc(elig.size()));
	HIPCHK(c->d_indel_counts.alloc((size_t)n_bub * 16));
	HIPCHK(c->d_indel_stats.alloc(24));
	HIPCHK(c->h_indel_stats.reserve(24));
	if (!tab.empty()) HIPCHK(hipMemcpyAsync(c->d_indel_tab.p, tab.data(), tab.size() * sizeof(IndelEntry), hipMemcpyHostToDevice, c->rstream));
	HIPCHK(hipMemcpyAsync(c->d_indel_elig.p, elig.data(), elig.size(), hipMemcpyHostToDevice, c->rstream));
	if (n_bub) HIPCHK(hipMemsetAsync(c->d_indel_counts.p, 0, (size_t)n_bub * 16, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream)); /* (pageable memory of this function) */
	/* (one step more than a bisection over the entries when their number is a power of two: the first power of two ABOVE it) */
	c->indel_anchor = (uint32_t)anchor; c->indel_ntab = (uint32_t)tab.size(); c->indel_trips = ceil_log2((uint64_t)tab.size() + 1);
	c->indel_ms = 0; c->indel_reads = 0; c->indel_adds = 0; c->indel_cands = 0;
	c->indel_on = true;
	*n_eligible = tab.size();
	return BWB_OK;
}

/* k_indel over n placement and locus records (device memory; d_lens NULL: no read lengths; d_mapq NULL: the placement's own MAPQ, else one byte
 * every mapq_stride bytes) into the context's counters; sets indel_ms / indel_reads / indel_adds / indel_cands.  On the result stream, behind the
 * kernels that wrote the records.  What comes back is the 24 bytes of the three sums. */
static int indel_launch(bwb_hip_ctx *c, const uint4 *d_places, const uint4 *d_loci, uint32_t n, const uint16_t *d_lens, const uint8_t *d_mapq, uint32_t mapq_stride, int min_mapq) {
	if (!n) return BWB_OK; /* (nothing launched: the figures of the last launch stay) */
	HIPCHK(hipMemsetAsync(c->d_indel_stats.p, 0, 24, c->rstream));
	Timed t(c, c->rstream);
	RC(t.begin());
	hipLaunchKernelGGL(k_indel, dim3(lane_grid(c, n)), dim3(BWB_BLOCK), 0, c->rstream, d_places, d_loci, n, d_lens, d_mapq, mapq_stride, (uint32_t)min_mapq, c->d_bubbles.as<uint64_t>(),
	                   c->d_indel_elig.as<uint8_t>(), c->indel_anchor, c->d_indel_tab.as<uint4>(), c->indel_ntab, c->indel_trips, c->d_indel_counts.as<uint32_t>(),
	                   c->d_indel_stats.as<unsigned long long>());
	HIPCHK(hipGetLastError());
	RC(t.end());
	HIPCHK(hipMemcpyAsync(c->h_indel_stats.p, c->d_indel_stats.p, 24, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	float ms = 0;
	RC(t.ms(&ms));
	c->indel_ms = ms;
	c->indel_reads = c->h_indel_stats.as<uint64_t>()[0];
	c->indel_adds = c->h_indel_stats.as<uint64_t>()[1];
	c->indel_cands = c->h_indel_stats.as<uint64_t>()[2];
	return BWB_OK;
}

static int indel_ready(bwb_hip_ctx *c, const char *who, int max_alt, int joined, int min_mapq) {
	if (min_mapq < 0 || min_mapq > 255) return fail(BWB_E_ARG, std::string(who) + ": min_mapq must be 0..255");
	if (max_alt < 0 || max_alt > 255) return fail(BWB_E_ARG, std::string(who) + ": max_alt must be 0..255");
	if (!c->indel_on) return fail(BWB_E_STATE, std::string(who) + ": no bubble table and counters (bwb_hip_indel_begin)");
	if (!c->d_SA.p) return fail(BWB_E_STATE, std::string(who) + ": sampled SA not uploaded (bwb_hip_set_sa)");
	if (joined) {
		if (!max_alt) return fail(BWB_E_STATE, std::string(who) + ": the joined MAPQ needs the items of max_alt 1..255");
		RC(join_ready(c, who, max_alt));
	}
	return BWB_OK;
}

extern "C" int bwb_hip_slot_indel(bwb_hip_ctx *c, int si, int max_mm, int max_alt, int joined, int min_mapq, uint64_t *reads_counted) {
	if (!c || si < 0 || si >= BWB_MAX_SLOTS) return fail(BWB_E_ARG, "slot_indel: bad argument");
	RC(indel_ready(c, "slot_indel", max_alt, joined, min_mapq));
	if (reads_counted) *reads_counted = 0;
	RC(ensure_locus(c, si, max_mm));
	Slot &s = c->slots[si];
	if (s.stage.indeled) return BWB_OK; /* (a submission is counted once) */
	if (joined) RC(ensure_join(c, si, max_mm, max_alt));
	const uint32_t n = s.n_reads; /* (not n_tot: a carried read that rides along behind the batch's reads has no record) */
	if (n) {
		HIPCHK(hipStreamWaitEvent(c->rstream, s.ev_up.e, 0)); /* (the slot's read lengths, uploaded on the copy stream) */
		RC(indel_launch(c, s.d_place.as<uint4>(), s.d_locus.as<uint4>(), n, s.d_lens.as<uint16_t>(), joined ? s.d_join.as<uint8_t>() + offsetof(bwb_join, mapq) : nullptr,
		                (uint32_t)sizeof(bwb_join), min_mapq));
		if (reads_counted) *reads_counted = c->indel_reads;
	}
	s.stage.indeled = true;
	return BWB_OK;
}

extern "C" int bwb_hip_batch_indel(bwb_hip_ctx *c, int max_mm, int max_alt, int joined, int min_mapq, uint64_t *reads_counted) {
	if (!c) return fail(BWB_E_ARG, "batch_indel: null context");
	RC(indel_ready(c, "batch_indel", max_alt, joined, min_mapq));
	RC(batch_ready(c, "batch_indel"));
	return bwb_hip_slot_indel(c, 0, max_mm, max_alt, joined, min_mapq, reads_counted);
}

/* the kernel on placement records of the caller's instead of a slot's (for parity tests): k_locus for their loci, then k_indel */
extern "C" int bwb_hip_indel_records(bwb_hip_ctx *c, const bwb_place *places, uint32_t n, const uint8_t *mapq, int min_mapq) {
	if (!c || (n && !places) || n > 0x7FFFFFFFu) return fail(BWB_E_ARG, "indel_records: bad argument");
	if (min_mapq < 0 || min_mapq > 255) return fail(BWB_E_ARG, "indel_records: min_mapq must be 0..255");
	if (!c->indel_on) return fail(BWB_E_STATE, "indel_records: no bubble table and counters (bwb_hip_indel_begin)");
	if (!n) return BWB_OK;
	HIPCHK(hipSetDevice(c->device));
	DevMem d_places, d_loci, d_mapq;
	RC(stage_in(c, d_places, places, (size_t)n * sizeof(bwb_place)));
	if (mapq) RC(stage_in(c, d_mapq, mapq, (size_t)n));
	HIPCHK(d_loci.alloc((size_t)n * sizeof(bwb_locus)));
	HIPCHK(hipStreamSynchronize(c->rstream));
	std::vector<bwb_locus> h_loci(n);
	RC(locus_launch(c, d_places.as<uint4>(), n, d_loci.as<uint4>(), h_loci.data()));
	return indel_launch(c, d_places.as<uint4>(), d_loci.as<uint4>(), n, nullptr, d_mapq.as<uint8_t>(), 1u, min_mapq);
}

extern "C" int bwb_hip_indel_counts(bwb_hip_ctx *c, uint64_t first, uint64_t n, uint32_t *out) {
	if (!c) return fail(BWB_E_ARG, "indel_counts: null argument");
	return counters_copy(c, "indel_counts", bubble_counters(c), first, n, out, hipMemcpyDeviceToHost);
}

extern "C" int bwb_hip_indel_reset(bwb_hip_ctx *c) {
	if (!c) return fail(BWB_E_ARG, "indel_reset: null context");
	return counters_reset(c, "indel_reset", bubble_counters(c));
}

/* the last indel call that launched: reads counted, adds made, candidates examined, and the kernel's HIP-event time */
extern "C" int bwb_hip_indel_stats(bwb_hip_ctx *c, uint64_t *reads, uint64_t *adds, uint64_t *candidates, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "indel_stats: null context");
	if (reads) *reads = c->indel_reads;
	if (adds) *adds = c->indel_adds;
	if (candidates) *candidates = c->indel_cands;
	if (kernel_ms) *kernel_ms = c->indel_ms;
	return BWB_OK;
}

/* ---- genotype calls at IUPAC sites and indel bubbles (k_geno_count, k_geno_emit, k_geno_bubbles) ------------------------------------------- */
static_assert(sizeof(bwb_geno_site) == 64 && offsetof(bwb_geno_site, n) == 16 && offsetof(bwb_geno_site, code) == 32 && offsetof(bwb_geno_site, pl) == 40, "k_geno_emit writes this layout");
static_assert(sizeof(bwb_geno_bubble) == 48 && offsetof(bwb_geno_bubble, gt) == 20 && offsetof(bwb_geno_bubble, pl) == 24, "k_geno_bubbles writes this layout");
static_assert(sizeof(bwb_geno_site_q) == 80 && offsetof(bwb_geno_site_q, qs) == 64, "k_geno_emit_q writes this layout");
extern "C" int bwb_hip_geno_begin(bwb_hip_ctx *c, uint32_t piece) {
	if (!c) return fail(BWB_E_ARG, "geno_begin: null context");
	if (piece < 1 || piece > (1u << 24)) return fail(BWB_E_ARG, "geno_begin: the piece must be 1..2^24");
	if (!c->pile_on) return fail(BWB_E_STATE, "geno_begin: no site index and counters (bwb_hip_pile_begin)");
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->rstream)); /* (a geno kernel of an earlier call may still use the buffers that are replaced) */
	c->geno_on = false; c->geno_bub = false;
	HIPCHK(c->d_geno_cnt.alloc((size_t)piece * 4));
	HIPCHK(c->d_geno_word.alloc((size_t)piece * 4));
	HIPCHK(c->d_geno_off.alloc(((size_t)piece + 1) * 8));
	HIPCHK(c->d_geno_bsum.alloc((size_t)blocks_of(piece) * 8));
	c->geno_q = c->pileq_on && c->pileq_weighted;
	const size_t site_rec = c->geno_q ? sizeof(bwb_geno_site_q) : sizeof(bwb_geno_site);
	HIPCHK(c->d_geno_sites.alloc((size_t)piece * site_rec));
	HIPCHK(c->h_geno_sites.reserve((size_t)piece * site_rec));
	HIPCHK(c->h_geno_n.reserve(8));
	c->geno_piece = piece;
	if (c->indel_on) {
		const uint32_t pb = std::min(piece, std::max(c->loci_nbub, 1u));
		HIPCHK(c->d_geno_bubs.alloc((size_t)pb * sizeof(bwb_geno_bubble)));
		HIPCHK(c->h_geno_bubs.reserve((size_t)pb * sizeof(bwb_geno_bubble)));
		c->geno_piece_bub = pb; c->geno_bub = true;
	}
	c->geno_ms = 0; c->geno_sites_called = 0; c->geno_bubs_called = 0;
	c->geno_on = true;
	return BWB_OK;
}

/* the mirrors of pile_counts / indel_counts: overwrite the counters of a range (several workers' sums meet on one device; tests inject counts) */
extern "C" int bwb_hip_pile_put(bwb_hip_ctx *c, uint64_t first, uint64_t n, const uint32_t *counts) {
	if (!c) return fail(BWB_E_ARG, "pile_put: null argument");
	return counters_copy(c, "pile_put", site_counters(c), first, n, counts, hipMemcpyHostToDevice);
}
extern "C" int bwb_hip_indel_put(bwb_hip_ctx *c, uint64_t first, uint64_t n, const uint32_t *counts) {
	if (!c) return fail(BWB_E_ARG, "indel_put: null argument");
	return counters_copy(c, "indel_put", bubble_counters(c), first, n, counts, hipMemcpyHostToDevice);
}

static int geno_args(bwb_hip_ctx *c, const char *who, uint64_t first, uint64_t n, int err, int64_t min_depth, uint64_t table, uint32_t piece) {
	if (err < 4 || err > 93) return fail(BWB_E_ARG, std::string(who) + ": the error phred must be 4..93");
	if (min_depth < 1 || min_depth > 0x7FFFFFFFll) return fail(BWB_E_ARG, std::string(who) + ": the minimum depth must be 1..2^31 - 1");
	if (first > table || n > table - first) return fail(BWB_E_ARG, std::string(who) + ": the range leaves the table of " + std::to_string(table));
	if (n > piece) return fail(BWB_E_ARG, std::string(who) + ": more than the piece of " + std::to_string(piece) + " (bwb_hip_geno_begin)");
	(void)c;
	return BWB_OK;
}
/* the scan of cnt[0 .. n) and the read-back of what the emit kernel wrote: the total first (8 bytes), then that many records */
static void geno_scan(bwb_hip_ctx *c, uint32_t n) { scan_offsets(c, c->d_geno_cnt.as<uint32_t>(), n, c->d_geno_off.as<uint64_t>(), c->d_geno_bsum.as<uint64_t>()); }
static int geno_fetch(bwb_hip_ctx *c, Timed &t, uint32_t n, const void *d_recs, void *h_recs, size_t rec_bytes, uint64_t *n_out) {
	HIPCHK(hipMemcpyAsync(c->h_geno_n.p, c->d_geno_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	const uint64_t called = c->h_geno_n.as<uint64_t>()[0];
	if (called > n) return fail(BWB_E_HIP, "geno: the scan counts more called entries than the range has");
	if (called) HIPCHK(hipMemcpyAsync(h_recs, d_recs, (size_t)called * rec_bytes, hipMemcpyDeviceToHost, c->rstream));
	HIPCHK(hipStreamSynchronize(c->rstream));
	float ms = 0;
	RC(t.ms(&ms));
	c->geno_ms = ms;
	*n_out = called;
	return BWB_OK;
}

/* the sites' calls, by the existing rule (64-byte records) or - weighted - by the quality sums (80-byte records), into h_geno_sites */
static int geno_sites_run(bwb_hip_ctx *c, const char *who, bool weighted, uint64_t first, uint64_t n, int err, int64_t min_depth, uint64_t *n_out) {
	if (!c->geno_on || !c->pile_on) return fail(BWB_E_STATE, std::string(who) + ": no scratch and output (bwb_hip_geno_begin)");
	if (weighted && !(c->pileq_on && c->pileq_weighted && c->geno_q)) return fail(BWB_E_STATE, std::string(who) + ": no quality sums before geno_begin (bwb_hip_pileq_begin with weighted != 0)");
	RC(geno_args(c, who, first, n, err, min_depth, c->pile_sites, c->geno_piece));
	*n_out = 0;
	if (!n) return BWB_OK; /* (nothing launched: the figures of the last launch stay) */
	HIPCHK(hipSetDevice(c->device));
	const uint64_t n_words64 = (c->text_n + 31) / 32;
	const uint32_t n_words = (uint32_t)n_words64, nn = (uint32_t)n;
	const unsigned grid = lane_grid(c, nn);
	Timed t(c, c->rstream);
	RC(t.begin());
	hipLaunchKernelGGL(k_geno_count, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->d_text.as<uint4>(), c->d_site_base.as<uint32_t>(), n_words, ceil_log2(n_words64), c->d_counts.as<uint4>(), first, nn,
	                   (uint64_t)min_depth, c->d_geno_cnt.as<uint32_t>(), c->d_geno_word.as<uint32_t>());
	geno_scan(c, nn);
	if (weighted)
		hipLaunchKernelGGL(k_geno_emit_q, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->d_text.as<uint4>(), c->d_site_base.as<uint32_t>(), n_words, c->d_counts.as<uint4>(), c->d_qsum.as<uint4>(),
		                   first, nn, c->d_geno_cnt.as<uint32_t>(), c->d_geno_word.as<uint32_t>(), c->d_geno_off.as<uint64_t>(), c->d_geno_sites.as<uint4>());
	else
		hipLaunchKernelGGL(k_geno_emit, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->d_text.as<uint4>(), c->d_site_base.as<uint32_t>(), n_words, c->d_counts.as<uint4>(), first, nn,
		                   (uint64_t)min_depth, (uint32_t)err, c->d_geno_cnt.as<uint32_t>(), c->d_geno_word.as<uint32_t>(), c->d_geno_off.as<uint64_t>(), c->d_geno_sites.as<uint4>());
	HIPCHK(hipGetLastError());
	RC(t.end());
	RC(geno_fetch(c, t, nn, c->d_geno_sites.p, c->h_geno_sites.p, weighted ? sizeof(bwb_geno_site_q) : sizeof(bwb_geno_site), n_out));
	c->geno_sites_called = *n_out;
	return BWB_OK;
}

extern "C" int bwb_hip_geno_sites(bwb_hip_ctx *c, uint64_t first, uint64_t n, int err, int64_t min_depth, const bwb_geno_site **out, uint64_t *n_out) {
	if (!c || !out || !n_out) return fail(BWB_E_ARG, "geno_sites: null argument");
	RC(geno_sites_run(c, "geno_sites", false, first, n, err, min_depth, n_out));
	*out = c->h_geno_sites.as<bwb_geno_site>();
	return BWB_OK;
}

/* the weighted calls: err is checked like geno_sites' (the sums were capped by the pile's err_cap; the rule itself no longer needs E) */
extern "C" int bwb_hip_geno_sites_q(bwb_hip_ctx *c, uint64_t first, uint64_t n, int err, int64_t min_depth, const bwb_geno_site_q **out, uint64_t *n_out) {
	if (!c || !out || !n_out) return fail(BWB_E_ARG, "geno_sites_q: null argument");
	RC(geno_sites_run(c, "geno_sites_q", true, first, n, err, min_depth, n_out));
	*out = c->h_geno_sites.as<bwb_geno_site_q>();
	return BWB_OK;
}

extern "C" int bwb_hip_geno_bubbles(bwb_hip_ctx *c, uint64_t first, uint64_t n, int err, int64_t min_depth, const bwb_geno_bubble **out, uint64_t *n_out) {
	if (!c || !out || !n_out) return fail(BWB_E_ARG, "geno_bubbles: null argument");
	if (!c->geno_on) return fail(BWB_E_STATE, "geno_bubbles: no scratch and output (bwb_hip_geno_begin)");
	if (!c->indel_on || !c->geno_bub) return fail(BWB_E_STATE, "geno_bubbles: no bubble table and counters before geno_begin (bwb_hip_indel_begin)");
	RC(geno_args(c, "geno_bubbles", first, n, err, min_depth, c->loci_nbub, c->geno_piece_bub));
	*out = c->h_geno_bubs.as<bwb_geno_bubble>(); *n_out = 0;
	if (!n) return BWB_OK;
	HIPCHK(hipSetDevice(c->device));
	const uint32_t nn = (uint32_t)n;
	const unsigned grid = lane_grid(c, nn);
	Timed t(c, c->rstream);
	RC(t.begin());
	hipLaunchKernelGGL(k_geno_bubbles, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->d_indel_elig.as<uint8_t>(), c->d_indel_counts.as<uint4>(), (uint32_t)first, nn, (uint64_t)min_depth,
	                   (uint32_t)err, c->d_geno_cnt.as<uint32_t>(), (const uint64_t *)nullptr, (uint4 *)nullptr);
	geno_scan(c, nn);
	hipLaunchKernelGGL(k_geno_bubbles, dim3(grid), dim3(BWB_BLOCK), 0, c->rstream, c->d_indel_elig.as<uint8_t>(), c->d_indel_counts.as<uint4>(), (uint32_t)first, nn, (uint64_t)min_depth,
	                   (uint32_t)err, c->d_geno_cnt.as<uint32_t>(), (const uint64_t *)c->d_geno_off.as<uint64_t>(), c->d_geno_bubs.as<uint4>());
	HIPCHK(hipGetLastError());
	RC(t.end());
	RC(geno_fetch(c, t, nn, c->d_geno_bubs.p, c->h_geno_bubs.p, sizeof(bwb_geno_bubble), n_out));
	c->geno_bubs_called = *n_out;
	return BWB_OK;
}

/* the entries the last geno_sites and the last geno_bubbles call called, and the HIP-event time of the kernels of whichever came last */
extern "C" int bwb_hip_geno_stats(bwb_hip_ctx *c, uint64_t *sites_called, uint64_t *bubbles_called, double *kernel_ms) {
	if (!c) return fail(BWB_E_ARG, "geno_stats: null context");
	if (sites_called) *sites_called = c->geno_sites_called;
	if (bubbles_called) *bubbles_called = c->geno_bubs_called;
	if (kernel_ms) *kernel_ms = c->geno_ms;
	return BWB_OK;
}

/* developer aid (not in include/bwbble_hip.h): per-read loop iteration counts of slot 0 when BWB_DEBUG_ITERS is set */
extern "C" int bwb_hip_debug_iters(bwb_hip_ctx *c, uint32_t *out) {
	if (!c || !c->slots[0].d_dbg_iters.p) return fail(BWB_E_STATE, "debug iteration counts are off (set BWB_DEBUG_ITERS)");
	return fetch(c, out, c->slots[0].d_dbg_iters.p, (size_t)c->slots[0].n_reads * 4);
}

/* developer aid: kl_calc_d visits per read of slot 0 */
extern "C" int bwb_hip_debug_calcd_work(bwb_hip_ctx *c, uint32_t *out) {
	if (!c || !c->slots[0].uploaded) return fail(BWB_E_STATE, "no batch");
	Slot &s = c->slots[0];
	std::vector<uint8_t> h((size_t)s.n_reads * s.dstride);
	RC(fetch(c, h.data(), s.d_dbuf.p, h.size()));
	for (uint32_t i = 0; i < s.n_reads; i++) memcpy(&out[i], &h[(size_t)i * s.dstride + s.dstride - 8], 4);
	return BWB_OK;
}
