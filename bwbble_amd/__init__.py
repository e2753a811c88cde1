"""bwbble_amd - host-side Python mirror of the C-ABI in include/bwbble_hip.h (ctypes, no torch types).

The product is libbwbble_hip.so (hand-written HIP for gfx950) plus the C host tools in
bwbble_amd/host; this module only binds the library for tests and bench.py.  It fails loudly when
the library is missing or no GPU is present: there is no CPU path here.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BWB_LIB") or os.path.join(HERE, "libbwbble_hip.so")  # BWB_LIB: tests load the `make testlib` build
TEST_LIB_PATH = os.path.join(HERE, "libbwbble_hip_test.so")
HOST_BIN = os.path.join(HERE, "bin", "bwbble")
SYNTH_BIN = os.path.join(HERE, "bin", "bwb_synth")

EXPORTS = [
    "bwb_hip_device_count", "bwb_hip_last_error", "bwb_default_params", "bwb_hip_ctx_create", "bwb_hip_ctx_destroy",
    "bwb_hip_align_batch", "bwb_hip_batch_upload", "bwb_hip_batch_run", "bwb_hip_batch_result", "bwb_hip_get_stats",
    "bwb_hip_calc_d", "bwb_hip_rank16", "bwb_hip_children", "bwb_hip_rank_bench", "bwb_hip_rank_bench_lane", "bwb_hip_set_sa", "bwb_hip_locate", "bwb_hip_locate_stats",
    "bwb_hip_reset_stats", "bwb_hip_slot_upload", "bwb_hip_slot_submit", "bwb_hip_slot_wait", "bwb_hip_slot_result", "bwb_hip_flush", "bwb_hip_abi_version", "bwb_hip_ctx_create_streamed", "bwb_hip_device_numa_node",
    "bwb_hip_ctx_create_async", "bwb_hip_ctx_index_wait", "bwb_hip_setup_times", "bwb_hip_dtab_info",
    "bwb_hip_slot_place", "bwb_hip_batch_place", "bwb_hip_place_stats", "bwb_hip_place_hits",
    "bwb_hip_slot_place_alt", "bwb_hip_batch_place_alt", "bwb_hip_place_alt_stats", "bwb_hip_place_hits_alt",
    "bwb_hip_set_loci", "bwb_hip_slot_locus", "bwb_hip_batch_locus", "bwb_hip_locus_places", "bwb_hip_locus_stats",
    "bwb_hip_set_bubble_chrom", "bwb_hip_slot_join", "bwb_hip_batch_join", "bwb_hip_join_records", "bwb_hip_join_stats",
    "bwb_hip_slot_lift", "bwb_hip_batch_lift", "bwb_hip_lift_records", "bwb_hip_lift_stats",
    "bwb_hip_set_text", "bwb_hip_slot_md", "bwb_hip_batch_md", "bwb_hip_md_records", "bwb_hip_md_stats",
    "bwb_hip_pile_begin", "bwb_hip_slot_pile", "bwb_hip_batch_pile", "bwb_hip_pile_records", "bwb_hip_pile_counts", "bwb_hip_pile_reset", "bwb_hip_pile_site_of", "bwb_hip_pile_stats",
    "bwb_hip_indel_begin", "bwb_hip_slot_indel", "bwb_hip_batch_indel", "bwb_hip_indel_records", "bwb_hip_indel_counts", "bwb_hip_indel_reset", "bwb_hip_indel_stats",
    "bwb_hip_geno_begin", "bwb_hip_pile_put", "bwb_hip_indel_put", "bwb_hip_geno_sites", "bwb_hip_geno_bubbles", "bwb_hip_geno_stats",
    "bwb_hip_pileq_begin", "bwb_hip_slot_quals", "bwb_hip_slot_pile_q", "bwb_hip_batch_pile_q", "bwb_hip_pile_records_q", "bwb_hip_pileq_sums", "bwb_hip_pileq_put", "bwb_hip_pileq_stats",
    "bwb_hip_geno_sites_q",
]
ABI_VERSION = 3  # BWB_HIP_ABI_VERSION (include/bwbble_hip.h)
MAX_SLOTS = 8  # BWB_MAX_SLOTS


class Params(C.Structure):
    """bwb_params == aln_params_t (mg-aligner/align.h:48-79)."""
    _fields_ = [(n, C.c_int32) for n in (
        "max_diff", "max_gapo", "max_gape", "max_entries", "mm_score", "gapo_score", "gape_score",
        "seed_length", "max_diff_seed", "max_best", "no_indel_length", "matched_Ncontig", "use_precalc",
        "is_multiref", "n_threads")]


class Result(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("aln_off", C.POINTER(C.c_uint64)), ("alns", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("visits_single", C.c_uint64), ("visits_calc_d", C.c_uint64), ("visits_alphabet", C.c_uint64), ("heap_pops", C.c_uint64),
                ("heap_pushes", C.c_uint64), ("n_alignments", C.c_uint64), ("n_overflow_reads", C.c_uint64), ("n_parked_reads", C.c_uint64),
                ("bucket_loads_search", C.c_uint64), ("bucket_loads_calc_d", C.c_uint64), ("lane_iterations", C.c_uint64), ("wave_iterations", C.c_uint64),
                ("heap_entries_stored", C.c_uint64), ("heap_entries_loaded", C.c_uint64), ("record_loads", C.c_uint64),
                ("ms_calc_d", C.c_double), ("ms_search", C.c_double), ("ms_total", C.c_double),
                ("launches_calc_d", C.c_uint32), ("launches_search", C.c_uint32)]


ALN_DTYPE = np.dtype([("L", "<u8"), ("U", "<u8"), ("score", "<u2"), ("num_mm", "u1"), ("num_gapo", "u1"),
                      ("num_gape", "u1"), ("reserved", "u1"), ("aln_length", "<u2"), ("gap_run", "<u2", (8,)), ("reserved2", "<u8")])
assert ALN_DTYPE.itemsize == 48
# bwb_place: what eval_aln + mapq make of one read's hits (kernel k_place); flags bit 0 = mapped, bit 1 = reverse strand
PLACE_DTYPE = np.dtype([("pos", "<u8"), ("top1", "<i4"), ("top2", "<i4"), ("score", "<u2"), ("mapq", "u1"), ("flags", "u1"),
                        ("num_mm", "u1"), ("num_gapo", "u1"), ("num_gape", "u1"), ("reserved", "u1"), ("aln_length", "<u2"),
                        ("ref_len", "<u2"), ("reserved2", "<u4"), ("gap_run", "<u2", (8,))])
assert PLACE_DTYPE.itemsize == 48
PLACE_MAPPED, PLACE_REVERSE = 1, 2
# bwb_alt: one of a read's other placements (kernel k_place_alt); flags as in bwb_place
ALT_DTYPE = np.dtype([("pos", "<u8"), ("flags", "u1"), ("hit", "u1"), ("num_mm", "u1"), ("num_gapo", "u1"), ("num_gape", "u1"),
                      ("reserved", "u1"), ("aln_length", "<u2"), ("gap_run", "<u2", (8,))])
assert ALT_DTYPE.itemsize == 32
# bwb_bubble: one bubble of bubble.data (mg-ref/comb.cpp:245-253); bwb_locus: where a placement lies in reference coordinates (kernel k_locus)
BUBBLE_DTYPE = np.dtype([("A", "<i8"), ("B_minus_A", "<i8"), ("C", "<i8"), ("D_minus_C", "<i8"), ("ref_len", "<i4"), ("alt_len", "<i4")])
assert BUBBLE_DTYPE.itemsize == 40
LOCUS_DTYPE = np.dtype([("seqid", "<i4"), ("pos1", "<i4"), ("bubble", "<i4"), ("kind", "u1"), ("reserved", "u1", (3,)), ("ref_lo", "<i8"), ("ref_hi", "<i8")])
assert LOCUS_DTYPE.itemsize == 32
LOCUS_POINT, LOCUS_RANGE = 1, 2
# bwb_join: a read's counts and MAPQ once the placements that lie where its primary lies are counted as one (kernels k_join_items / k_join_reads)
JOIN_DTYPE = np.dtype([("top1", "<i4"), ("top2", "<i4"), ("mapq", "u1"), ("joined", "u1"), ("reserved", "<u2"), ("reserved2", "<u4")])
assert JOIN_DTYPE.itemsize == 16
# bwb_lift: the header of a lifted placement's record (kernels k_lift_count / k_lift); n_ops ops follow as uint32 = len << 4 | op, zero-padded to four
LIFT_DTYPE = np.dtype([("pos", "<i8"), ("seqid", "<i4"), ("n_ops", "u1"), ("reserved", "u1", (3,))])
assert LIFT_DTYPE.itemsize == 16
LIFT_M, LIFT_I, LIFT_D, LIFT_S, LIFT_MAX_OPS = 0, 1, 2, 4, 20
LIFT_NONE, LIFT_LIFTED, LIFT_UNLIFTABLE = 0, 1, 2
# bwb_md: a read's NM and the length of its MD text against the index's text (kernels k_md_count / k_md)
# bwb_geno_site / bwb_geno_bubble (include/bwbble_hip.h): the called sites' and bubbles' records of the geno family
GENO_SITE_DTYPE = np.dtype([("pos", "<u8"), ("site", "<u8"), ("n", "<u4", (4,)), ("code", "u1"), ("n_geno", "u1"), ("gt", "u1"), ("gq", "u1"), ("reserved", "<u4"), ("pl", "<u4", (6,))])
GENO_BUBBLE_DTYPE = np.dtype([("bubble", "<u4"), ("n", "<u4", (4,)), ("gt", "u1"), ("gq", "u1"), ("reserved", "<u2"), ("pl", "<u4", (3,)), ("pad", "<u4", (3,))])
# bwb_geno_site_q: the site's record by the weighted rule (-Y), then its four quality sums
GENO_SITE_Q_DTYPE = np.dtype(GENO_SITE_DTYPE.descr + [("qs", "<u4", (4,))])
assert GENO_SITE_DTYPE.itemsize == 64 and GENO_BUBBLE_DTYPE.itemsize == 48 and GENO_SITE_Q_DTYPE.itemsize == 80 and GENO_SITE_Q_DTYPE.fields["qs"][1] == 64
MD_DTYPE = np.dtype([("nm", "<u4"), ("md_len", "<u2"), ("kind", "u1"), ("reserved", "u1")])
assert MD_DTYPE.itemsize == 8
MD_NONE, MD_OK, MD_TOO_LONG, MD_MAX_SPAN = 0, 1, 2, 4096

_FLAG = {"-M": "mm_score", "-O": "gapo_score", "-E": "gape_score", "-n": "max_diff", "-k": "max_diff_seed",
         "-o": "max_gapo", "-e": "max_gape", "-l": "seed_length", "-m": "max_entries", "-t": "n_threads"}
NO_FLAG = ("max_best", "no_indel_length")  # fields of aln_params_t without a flag: keyword arguments of params()

_lib = None


class BwbError(RuntimeError):
    pass


def build(testlib=False):
    """Compiles the HIP library and the host tools in-tree (hipcc --offload-arch=gfx950); testlib: the test build as well."""
    subprocess.run(["make", "-s", "-C", HERE] + (["all", "testlib"] if testlib else []), check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BwbError(f"{LIB_PATH} is missing: run `make -C bwbble_amd` (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        if not hasattr(L, "bwb_hip_abi_version") or L.bwb_hip_abi_version() != ABI_VERSION:
            raise BwbError(f"{LIB_PATH} implements another version of the C-ABI than this mirror (want {ABI_VERSION}): rebuild it")
        L.bwb_hip_last_error.restype = C.c_char_p
        L.bwb_hip_ctx_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.bwb_hip_ctx_destroy.argtypes = [C.c_void_p]
        L.bwb_hip_batch_upload.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.bwb_hip_batch_run.argtypes = [C.c_void_p]
        L.bwb_hip_batch_result.argtypes = [C.c_void_p, C.POINTER(Result)]
        L.bwb_hip_align_batch.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Result)]
        L.bwb_hip_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.bwb_hip_calc_d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bwb_hip_rank16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        L.bwb_hip_children.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bwb_hip_rank_bench.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.bwb_hip_rank_bench_lane.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.bwb_hip_reset_stats.argtypes = [C.c_void_p]
        L.bwb_hip_slot_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        L.bwb_hip_slot_submit.argtypes = [C.c_void_p, C.c_int]
        L.bwb_hip_slot_wait.argtypes = [C.c_void_p, C.c_int]
        L.bwb_hip_slot_result.argtypes = [C.c_void_p, C.c_int, C.POINTER(Result)]
        L.bwb_hip_flush.argtypes = [C.c_void_p]
        L.bwb_hip_set_sa.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.bwb_hip_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.bwb_hip_dtab_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.bwb_hip_setup_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.bwb_hip_locate_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_slot_place.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.bwb_hip_batch_place.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.bwb_hip_place_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_place_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.bwb_hip_slot_place_alt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.bwb_hip_batch_place_alt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.bwb_hip_place_alt_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_place_hits_alt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.bwb_hip_set_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.bwb_hip_slot_locus.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.bwb_hip_batch_locus.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
        L.bwb_hip_locus_places.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.bwb_hip_locus_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_set_bubble_chrom.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.bwb_hip_slot_join.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_uint32)]
        L.bwb_hip_batch_join.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_uint32)]
        L.bwb_hip_join_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.bwb_hip_join_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_slot_lift.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint64)]
        L.bwb_hip_batch_lift.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint64)]
        L.bwb_hip_lift_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
        L.bwb_hip_lift_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_set_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.bwb_hip_slot_md.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint32)]
        L.bwb_hip_batch_md.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint32)]
        L.bwb_hip_md_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
        L.bwb_hip_md_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_pile_begin.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.bwb_hip_slot_pile.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_batch_pile.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_pile_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.bwb_hip_pile_counts.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bwb_hip_pile_reset.argtypes = [C.c_void_p]
        L.bwb_hip_pile_site_of.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.bwb_hip_pile_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_indel_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_slot_indel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_batch_indel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_indel_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
        L.bwb_hip_indel_counts.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bwb_hip_indel_reset.argtypes = [C.c_void_p]
        L.bwb_hip_indel_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_geno_begin.argtypes = [C.c_void_p, C.c_uint32]
        L.bwb_hip_pile_put.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bwb_hip_indel_put.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bwb_hip_geno_sites.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.bwb_hip_geno_bubbles.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.bwb_hip_geno_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_pileq_begin.argtypes = [C.c_void_p, C.c_int]
        L.bwb_hip_slot_quals.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
        L.bwb_hip_slot_pile_q.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_batch_pile_q.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.bwb_hip_pile_records_q.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.bwb_hip_pileq_sums.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bwb_hip_pileq_put.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bwb_hip_pileq_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.bwb_hip_geno_sites_q.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise BwbError(f"bwbble_hip error {rc}: {lib().bwb_hip_last_error().decode()}")


def _read_arrays(seqs, lens):
    """the read codes and lengths as the C-ABI takes them: (n_reads, stride) uint8 rows, one uint16 length per row"""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    if seqs.ndim != 2 or len(lens) != seqs.shape[0]:
        raise ValueError("seqs must be (n_reads, stride) uint8 with one length per row")
    return seqs, lens


def _hit_arrays(aln_off, alns):
    """a caller's hit list as the C-ABI takes it: n_reads + 1 uint64 offsets into ALN_DTYPE records"""
    aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
    alns = np.ascontiguousarray(alns, dtype=ALN_DTYPE)
    if len(aln_off) < 1 or (len(aln_off) > 1 and int(aln_off.max()) > len(alns)):
        raise ValueError("aln_off must hold n_reads + 1 offsets into alns")
    return aln_off, alns


def device_count():
    return lib().bwb_hip_device_count()


def params(flags=(), **fields):
    """Defaults of set_default_aln_params (align.c:22-38) + `bwbble align` style flags (main.c:100-117) + the fields of aln_params_t
    that the CLI has no flag for and a caller of the C-ABI may still set: max_best=, no_indel_length=."""
    p = Params()
    lib().bwb_default_params(C.byref(p))
    flags = list(flags)
    i = 0
    while i < len(flags):
        if flags[i] == "-S":
            p.is_multiref = 0
            i += 1
        elif flags[i] == "-P":
            p.use_precalc = 1
            i += 1
        else:
            setattr(p, _FLAG[flags[i]], int(flags[i + 1]))
            i += 2
    for name, v in fields.items():
        if name not in NO_FLAG:
            raise TypeError(f"params() takes no field {name!r}")
        setattr(p, name, int(v))
    return p


class BwtFile:
    """In-memory bwt_t (bwt.h:19-40) read from a reference-format .bwt file (bwt.c:66-82)."""

    def __init__(self, path, load_sa=False):
        hdr = np.fromfile(path, dtype="<u8", count=22)
        self.hdr = hdr[:5].copy()
        self.length, self.num_words, self.num_sa, self.num_occ, self.sa0_index = (int(v) for v in hdr[:5])
        self.C = hdr[5:22].copy()
        off = 22 * 8
        # memory-mapped: a GRCh37-scale file is 12 GB, and the ranks of a multi-GPU run share its pages
        self.bwt = np.memmap(path, dtype="<u4", mode="r", offset=off, shape=(self.num_words,))
        off += 4 * self.num_words
        self.O = np.memmap(path, dtype="<u8", mode="r", offset=off, shape=(self.num_occ * 16,))
        off += 8 * self.num_occ * 16
        self.SA = np.memmap(path, dtype="<u8", mode="r", offset=off, shape=(self.num_sa,)) if load_sa else None


class Context:
    """One GPU context (bwb_hip_ctx): device-resident FM-index + batch state."""

    def __init__(self, bwt, device=0):
        if isinstance(bwt, str):
            bwt = BwtFile(bwt)
        if device_count() < 1:
            raise BwbError("no HIP device visible: the alignment path has no CPU fallback")
        self.bwt = bwt
        self._h = C.c_void_p()
        _chk(lib().bwb_hip_ctx_create(device, bwt.hdr.ctypes.data, bwt.C.ctypes.data, bwt.bwt.ctypes.data,
                                      bwt.O.ctypes.data, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().bwb_hip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batch API ------------------------------------------------------------------------------
    def upload(self, p, seqs, lens):
        seqs, lens = _read_arrays(seqs, lens)
        self._keep = (seqs, lens)
        _chk(lib().bwb_hip_batch_upload(self._h, C.byref(p), seqs.ctypes.data, lens.ctypes.data, seqs.shape[0], max(seqs.shape[1], 1)))

    def run(self):
        _chk(lib().bwb_hip_batch_run(self._h))

    # -- streaming API: up to MAX_SLOTS batches resident, slices that park instead of draining ---------------------
    def slot_upload(self, slot, p, seqs, lens, carry=None):
        """carry: codes of the last read longer than the seed that precedes this batch in the file (D_seed of leading short reads)"""
        seqs, lens = _read_arrays(seqs, lens)
        carry = None if carry is None else np.ascontiguousarray(carry, dtype=np.uint8)
        _chk(lib().bwb_hip_slot_upload(self._h, slot, C.byref(p), seqs.ctypes.data, lens.ctypes.data, seqs.shape[0], max(seqs.shape[1], 1),
                                       None if carry is None else carry.ctypes.data, 0 if carry is None else len(carry)))

    def slot_submit(self, slot):
        _chk(lib().bwb_hip_slot_submit(self._h, slot))

    def slot_wait(self, slot):
        _chk(lib().bwb_hip_slot_wait(self._h, slot))

    def slot_result(self, slot):
        r = Result()
        _chk(lib().bwb_hip_slot_result(self._h, slot, C.byref(r)))
        return self._unpack(r)

    def flush(self):
        _chk(lib().bwb_hip_flush(self._h))

    def reset_stats(self):
        _chk(lib().bwb_hip_reset_stats(self._h))

    def result(self):
        r = Result()
        _chk(lib().bwb_hip_batch_result(self._h, C.byref(r)))
        return self._unpack(r)

    @staticmethod
    def _unpack(r):
        n = r.n_reads
        off = np.ctypeslib.as_array(r.aln_off, shape=(n + 1,)).copy()
        total = int(off[n])
        alns = np.frombuffer(C.string_at(r.alns, total * ALN_DTYPE.itemsize), dtype=ALN_DTYPE) if total else np.zeros(0, dtype=ALN_DTYPE)
        return off, alns

    def align(self, p, seqs, lens):
        self.upload(p, seqs, lens)
        self.run()
        return self.result()

    def stats(self):
        s = Stats()
        _chk(lib().bwb_hip_get_stats(self._h, C.byref(s)))
        return s

    def calc_d(self, p, seqs, lens):
        """D / D_seed of every read as (n, maxlen+1, 2) and (n, seed_length+1, 2) int32 (num_diff, sa_intv_width)."""
        self.upload(p, seqs, lens)
        n, maxlen = len(lens), int(max(lens)) if len(lens) else 0
        D = np.zeros((n, maxlen + 1, 2), dtype=np.int32)
        Ds = np.zeros((n, p.seed_length + 1, 2), dtype=np.int32)
        _chk(lib().bwb_hip_calc_d(self._h, D.ctypes.data, Ds.ctypes.data))
        return D, Ds

    # -- rank -----------------------------------------------------------------------------------
    def rank16(self, pos, inc=0, exact=False):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.zeros((len(pos), 16), dtype=np.uint64)
        _chk(lib().bwb_hip_rank16(self._h, pos.ctypes.data, len(pos), inc, int(exact), out.ctypes.data))
        return out

    def children(self, iL, iU, need=True, alpha=False):
        """wave_children by itself: (L, U) as (n, 16) uint64 with column j = child j (column 0 is zero) and the non-empty mask (n,) uint32.
        Pair q runs as lane q % 64 of wave q / 64: the order of the pairs composes the waves."""
        iL = np.ascontiguousarray(iL, dtype=np.uint64)
        iU = np.ascontiguousarray(iU, dtype=np.uint64)
        n = len(iL)
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(need, dtype=bool), (n,)).astype(np.uint8)
                                     | (np.broadcast_to(np.asarray(alpha, dtype=bool), (n,)).astype(np.uint8) << 1))
        if len(iU) != n:
            raise ValueError("iL and iU must have one entry per pair")
        oL, oU, mask = np.zeros((n, 15), dtype=np.uint64), np.zeros((n, 15), dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        _chk(lib().bwb_hip_children(self._h, iL.ctypes.data, iU.ctypes.data, flags.ctypes.data, n, oL.ctypes.data, oU.ctypes.data, mask.ctypes.data))
        z = np.zeros((n, 1), dtype=np.uint64)
        return np.hstack([z, oL]), np.hstack([z, oU]), mask

    def rank_bench(self, n, iters=5, seed=1, lane=False):
        """Random Occ16 micro-benchmark: octet layout (8 lanes share a bucket) or the alignment kernels' lane layout."""
        ms, cs = C.c_double(), C.c_uint64()
        f = lib().bwb_hip_rank_bench_lane if lane else lib().bwb_hip_rank_bench
        _chk(f(self._h, n, iters, seed, C.byref(ms), C.byref(cs)))
        return ms.value, cs.value

    def set_sa(self, SA):
        SA = np.ascontiguousarray(SA, dtype=np.uint64)
        _chk(lib().bwb_hip_set_sa(self._h, SA.ctypes.data, len(SA)))

    def locate(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(len(rows), dtype=np.uint64)
        _chk(lib().bwb_hip_locate(self._h, rows.ctypes.data, len(rows), out.ctypes.data))
        return out

    def _count_steps_ms(self, getter):
        """(count, steps, kernel ms) of the last call of one kind: locate_stats, place_stats, place_alt_stats"""
        n, st, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        _chk(getter(self._h, C.byref(n), C.byref(st), C.byref(ms)))
        return n.value, st.value, ms.value

    # -- placement records: eval_aln + mapq on the GPU (needs set_sa) ----------------------------------------------
    @staticmethod
    def _places(ptr, n):
        return np.frombuffer(C.string_at(ptr, n * PLACE_DTYPE.itemsize), dtype=PLACE_DTYPE).copy() if n else np.zeros(0, dtype=PLACE_DTYPE)

    def slot_place(self, slot, max_mm=6):
        """one PLACE_DTYPE record per read of the slot, in read order (max_mm: mapq's, aln2sam's -n)"""
        ptr, n = C.c_void_p(), C.c_uint32()
        _chk(lib().bwb_hip_slot_place(self._h, slot, max_mm, C.byref(ptr), C.byref(n)))
        return self._places(ptr, n.value)

    def place(self, max_mm=6):
        """the same for the one-batch interface (after run() / align())"""
        ptr, n = C.c_void_p(), C.c_uint32()
        _chk(lib().bwb_hip_batch_place(self._h, max_mm, C.byref(ptr), C.byref(n)))
        return self._places(ptr, n.value)

    def place_hits(self, aln_off, alns, max_mm=6):
        """the same kernel on a hit list of the caller's: read r owns alns[aln_off[r]:aln_off[r + 1]] (ALN_DTYPE, discovery order)"""
        aln_off, alns = _hit_arrays(aln_off, alns)
        out = np.zeros(len(aln_off) - 1, dtype=PLACE_DTYPE)
        _chk(lib().bwb_hip_place_hits(self._h, alns.ctypes.data, aln_off.ctypes.data, len(aln_off) - 1, max_mm, out.ctypes.data))
        return out

    def place_stats(self):
        """(reads, invPsi steps = rank-block visits, kernel ms) of the last place call"""
        return self._count_steps_ms(lib().bwb_hip_place_stats)

    # -- a read's other placements (X0 / X1 / XA): the placement records, and one ALT_DTYPE record per item -------------------
    @staticmethod
    def _alts(n, off_ptr, alt_ptr):
        off = np.frombuffer(C.string_at(off_ptr, (n + 1) * 8), dtype="<u8").copy()
        total = int(off[n])
        alts = np.frombuffer(C.string_at(alt_ptr, total * ALT_DTYPE.itemsize), dtype=ALT_DTYPE).copy() if total else np.zeros(0, dtype=ALT_DTYPE)
        return off, alts

    def slot_place_alt(self, slot, max_mm=6, max_alt=5):
        """(places, alt_off, alts): slot_place's records, and read r's items alts[alt_off[r]:alt_off[r + 1]] (max_alt: map's -X, 1..255)"""
        pp, po, pa, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        _chk(lib().bwb_hip_slot_place_alt(self._h, slot, max_mm, max_alt, C.byref(pp), C.byref(po), C.byref(pa), C.byref(n)))
        return (self._places(pp, n.value),) + self._alts(n.value, po, pa)

    def place_alt(self, max_mm=6, max_alt=5):
        """the same for the one-batch interface (after run() / align())"""
        pp, po, pa, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        _chk(lib().bwb_hip_batch_place_alt(self._h, max_mm, max_alt, C.byref(pp), C.byref(po), C.byref(pa), C.byref(n)))
        return (self._places(pp, n.value),) + self._alts(n.value, po, pa)

    def place_hits_alt(self, aln_off, alns, max_mm=6, max_alt=5):
        """the same kernels on a hit list of the caller's (see place_hits)"""
        aln_off, alns = _hit_arrays(aln_off, alns)
        n = len(aln_off) - 1
        out = np.zeros(n, dtype=PLACE_DTYPE)
        po, pa = C.c_void_p(), C.c_void_p()
        _chk(lib().bwb_hip_place_hits_alt(self._h, alns.ctypes.data, aln_off.ctypes.data, n, max_mm, max_alt, out.ctypes.data, C.byref(po), C.byref(pa)))
        return (out,) + self._alts(n, po, pa)

    def place_alt_stats(self):
        """(items, invPsi steps = rank-block visits, kernel ms) of the last place_alt call"""
        return self._count_steps_ms(lib().bwb_hip_place_alt_stats)

    # -- bubble hits in reference coordinates (bC / bP): one LOCUS_DTYPE record per read (needs set_loci; the slot forms need set_sa) -----------
    def set_loci(self, start, end, bubble_of, bubbles):
        """the tables of kernel k_locus: the .ann records' first and last text positions (ascending, disjoint), the bubble number of every
        record (-1: not a bubble record; see bubble_of()) and the bubble table (BUBBLE_DTYPE, see read_bubble_data())"""
        start = np.ascontiguousarray(start, dtype=np.uint64)
        end = np.ascontiguousarray(end, dtype=np.uint64)
        bubble_of = np.ascontiguousarray(bubble_of, dtype=np.int32)
        bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
        if not len(start) == len(end) == len(bubble_of):
            raise ValueError("start, end and bubble_of must have one entry per record")
        _chk(lib().bwb_hip_set_loci(self._h, start.ctypes.data, end.ctypes.data, bubble_of.ctypes.data, len(start), bubbles.ctypes.data, len(bubbles)))

    @staticmethod
    def _loci(ptr, n):
        return np.frombuffer(C.string_at(ptr, n * LOCUS_DTYPE.itemsize), dtype=LOCUS_DTYPE).copy() if n else np.zeros(0, dtype=LOCUS_DTYPE)

    def slot_locus(self, slot, max_mm=6):
        """(places, loci): slot_place's records and one LOCUS_DTYPE record per read of the slot, in read order"""
        pp, pl, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _chk(lib().bwb_hip_slot_locus(self._h, slot, max_mm, C.byref(pp), C.byref(pl), C.byref(n)))
        return self._places(pp, n.value), self._loci(pl, n.value)

    def locus(self, max_mm=6):
        """the same for the one-batch interface (after run() / align())"""
        pp, pl, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _chk(lib().bwb_hip_batch_locus(self._h, max_mm, C.byref(pp), C.byref(pl), C.byref(n)))
        return self._places(pp, n.value), self._loci(pl, n.value)

    def locus_places(self, places):
        """the same kernel on placement records of the caller's (PLACE_DTYPE)"""
        places = np.ascontiguousarray(places, dtype=PLACE_DTYPE)
        out = np.zeros(len(places), dtype=LOCUS_DTYPE)
        _chk(lib().bwb_hip_locus_places(self._h, places.ctypes.data, len(places), out.ctypes.data))
        return out

    def locus_stats(self):
        """(reads, kernel ms) of the last locus call"""
        n, ms = C.c_uint64(), C.c_double()
        _chk(lib().bwb_hip_locus_stats(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    # -- a read's placements counted by locus (-J): one JOIN_DTYPE record per read (needs set_loci and set_bubble_chrom; the slot forms set_sa) --
    def set_bubble_chrom(self, chrom_of):
        """after set_loci: the .ann record of the chromosome every bubble lies on (see bubble_chrom_of()); for join() and lift()"""
        chrom_of = np.ascontiguousarray(chrom_of, dtype=np.int32)
        _chk(lib().bwb_hip_set_bubble_chrom(self._h, chrom_of.ctypes.data, len(chrom_of)))

    def _joined(self, call, *args):
        p = [C.c_void_p() for _ in range(5)]
        n = C.c_uint32()
        _chk(call(self._h, *args, *[C.byref(x) for x in p], C.byref(n)))
        n = n.value
        joins = np.frombuffer(C.string_at(p[4], n * JOIN_DTYPE.itemsize), dtype=JOIN_DTYPE).copy() if n else np.zeros(0, dtype=JOIN_DTYPE)
        return (self._places(p[0], n),) + self._alts(n, p[1], p[2]) + (self._loci(p[3], n), joins)

    def slot_join(self, slot, max_mm=6, max_alt=5):
        """(places, alt_off, alts, loci, joins): slot_place_alt's and slot_locus's records and one JOIN_DTYPE record per read of the slot"""
        return self._joined(lib().bwb_hip_slot_join, slot, max_mm, max_alt)

    def join(self, max_mm=6, max_alt=5):
        """the same for the one-batch interface (after run() / align())"""
        return self._joined(lib().bwb_hip_batch_join, max_mm, max_alt)

    def join_records(self, places, alt_off, alts, alt_sub, max_mm=6):
        """the same kernels on records of the caller's: read r owns alts[alt_off[r]:alt_off[r + 1]], alt_sub[q] != 0: item q is suboptimal"""
        places = np.ascontiguousarray(places, dtype=PLACE_DTYPE)
        alt_off = np.ascontiguousarray(alt_off, dtype=np.uint64)
        alts = np.ascontiguousarray(alts, dtype=ALT_DTYPE)
        alt_sub = np.ascontiguousarray(alt_sub, dtype=np.uint8)
        if len(alt_off) != len(places) + 1 or not len(alts) == len(alt_sub) == int(alt_off[-1]):
            raise ValueError("alt_off must have one entry per read and one more, alts and alt_sub one per item")
        out = np.zeros(len(places), dtype=JOIN_DTYPE)
        _chk(lib().bwb_hip_join_records(self._h, places.ctypes.data, len(places), alt_off.ctypes.data, alts.ctypes.data, alt_sub.ctypes.data, max_mm, out.ctypes.data))
        return out

    def join_stats(self):
        """(items, joined items, kernel ms) of the last join call"""
        return self._count_steps_ms(lib().bwb_hip_join_stats)

    # -- placements on bubble records in chromosome coordinates (-R): per placement a kind byte, and for a lifted one a record (needs set_loci and
    #    set_bubble_chrom; the slot forms set_sa).  Placement q < n_reads is read q's primary, n_reads + j is item j --
    @staticmethod
    def _lifted(p, nq):
        kinds = np.frombuffer(C.string_at(p[0], nq), dtype=np.uint8).copy() if nq else np.zeros(0, dtype=np.uint8)
        off = np.frombuffer(C.string_at(p[1], (nq + 1) * 8), dtype=np.uint64).copy()
        words = int(off[-1])
        recs = np.frombuffer(C.string_at(p[2], words * 16), dtype=np.uint32).copy() if words else np.zeros(0, dtype=np.uint32)
        return kinds, off, recs.reshape(-1, 4)

    def slot_lift(self, slot, max_mm=6, max_alt=5):
        """(kinds, lift_off, words): the kind byte of every placement of the slot, and the 16-byte words of the lifted ones' records as rows of
        four uint32 - see lift_record().  max_alt 0: the primaries alone"""
        p = [C.c_void_p() for _ in range(3)]
        nq = C.c_uint64()
        _chk(lib().bwb_hip_slot_lift(self._h, slot, max_mm, max_alt, *[C.byref(x) for x in p], C.byref(nq)))
        return self._lifted(p, nq.value)

    def lift(self, max_mm=6, max_alt=5):
        """the same for the one-batch interface (after run() / align())"""
        p = [C.c_void_p() for _ in range(3)]
        nq = C.c_uint64()
        _chk(lib().bwb_hip_batch_lift(self._h, max_mm, max_alt, *[C.byref(x) for x in p], C.byref(nq)))
        return self._lifted(p, nq.value)

    def lift_records(self, places, alt_off, alts):
        """the same kernels on records of the caller's: read r owns alts[alt_off[r]:alt_off[r + 1]]"""
        places = np.ascontiguousarray(places, dtype=PLACE_DTYPE)
        alt_off = np.ascontiguousarray(alt_off, dtype=np.uint64)
        alts = np.ascontiguousarray(alts, dtype=ALT_DTYPE)
        if len(alt_off) != len(places) + 1 or len(alts) != int(alt_off[-1]):
            raise ValueError("alt_off must have one entry per read and one more, alts one per item")
        p = [C.c_void_p() for _ in range(3)]
        _chk(lib().bwb_hip_lift_records(self._h, places.ctypes.data, len(places), alt_off.ctypes.data, alts.ctypes.data, *[C.byref(x) for x in p]))
        return self._lifted(p, len(places) + len(alts))

    def lift_stats(self):
        """(placements lifted, placements not liftable, kernel ms) of the last lift call"""
        return self._count_steps_ms(lib().bwb_hip_lift_stats)

    # -- NM:i and MD:Z against the index's text (-D): per read an MD_DTYPE record and, for kind MD_OK, its MD bytes (needs set_text; the slot forms
    #    set_sa, and with lifted set_loci and set_bubble_chrom) --
    def set_text(self, codes):
        """the forward text, one code 0..15 per character (see read_ref()): packed to 4 bits per character on the device.  Before the first upload"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        _chk(lib().bwb_hip_set_text(self._h, codes.ctypes.data, len(codes)))

    @staticmethod
    def _md(p, n):
        recs = np.frombuffer(C.string_at(p[0], n * MD_DTYPE.itemsize), dtype=MD_DTYPE).copy() if n else np.zeros(0, dtype=MD_DTYPE)
        off = np.frombuffer(C.string_at(p[1], (n + 1) * 8), dtype=np.uint64).copy()
        return recs, off, C.string_at(p[2], int(off[-1])) if int(off[-1]) else b""

    def slot_md(self, slot, max_mm=6, max_alt=5, lifted=False):
        """(recs, md_off, text): read r's MD text is text[md_off[r]:md_off[r + 1]].  lifted: the primaries slot_lift(max_mm, max_alt) lifts are
        walked by their lift records"""
        p = [C.c_void_p() for _ in range(3)]
        n = C.c_uint32()
        _chk(lib().bwb_hip_slot_md(self._h, slot, max_mm, max_alt, int(bool(lifted)), *[C.byref(x) for x in p], C.byref(n)))
        return self._md(p, n.value)

    def batch_md(self, max_mm=6, max_alt=5, lifted=False):
        """the same for the one-batch interface (after run() / align())"""
        p = [C.c_void_p() for _ in range(3)]
        n = C.c_uint32()
        _chk(lib().bwb_hip_batch_md(self._h, max_mm, max_alt, int(bool(lifted)), *[C.byref(x) for x in p], C.byref(n)))
        return self._md(p, n.value)

    @staticmethod
    def _record_arrays(seqs, lens, places, kinds, lift_off, words, mapq):
        """the arrays and pointers of the *_records calls (md_records: mapq None), checked"""
        seqs, lens = _read_arrays(seqs, lens)
        places = np.ascontiguousarray(places, dtype=PLACE_DTYPE)
        if len(places) != len(lens):
            raise ValueError("one placement record per read")
        lift = [None, None, None]
        if kinds is not None:
            kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
            lift_off = np.ascontiguousarray(lift_off, dtype=np.uint64)
            words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 4)
            if len(kinds) != len(lens) or len(lift_off) != len(lens) + 1 or len(words) != int(lift_off[-1]):
                raise ValueError("kinds must have one entry per read, lift_off one more, words one row per 16-byte word")
            lift = [kinds.ctypes.data, lift_off.ctypes.data, words.ctypes.data]
        if mapq is not None:
            mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
            if len(mapq) != len(lens):
                raise ValueError("one MAPQ per read")
        return seqs, lens, places, lift, mapq, (kinds, lift_off, words)  # (the last: kept alive behind the pointers in `lift`)

    def md_records(self, seqs, lens, places, kinds=None, lift_off=None, words=None):
        """the same kernels on reads and placement records of the caller's; kinds / lift_off / words: every read's lift kind and the 16-byte words
        of the lifted ones' records, laid out as slot_lift() returns them for its primaries"""
        seqs, lens, places, lift, _mapq, _keep = self._record_arrays(seqs, lens, places, kinds, lift_off, words, None)
        p = [C.c_void_p() for _ in range(3)]
        _chk(lib().bwb_hip_md_records(self._h, seqs.ctypes.data, lens.ctypes.data, seqs.shape[1], places.ctypes.data, len(lens), *lift, *[C.byref(x) for x in p]))
        return self._md(p, len(lens))

    def md_stats(self):
        """(reads of kind MD_OK, MD bytes, kernel ms) of the last md call"""
        return self._count_steps_ms(lib().bwb_hip_md_stats)

    # -- allele counts at the text's IUPAC sites (-A): device-resident counters, n_sites x (A, C, G, T), summed over every pile call (needs set_text
    #    and pile_begin; the slot forms set_sa, with lifted / joined set_loci and set_bubble_chrom) --
    def pile_begin(self):
        """builds the site index over the text and zeroed counters -> the number of sites.  After set_text, before the first upload"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_pile_begin(self._h, C.byref(n)))
        return n.value

    def slot_pile(self, slot, max_mm=6, max_alt=5, lifted=False, joined=False, min_mapq=0):
        """counts the slot's reads -> the reads counted; a second call on the same submission counts nothing and returns 0"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_slot_pile(self._h, slot, max_mm, max_alt, int(bool(lifted)), int(bool(joined)), min_mapq, C.byref(n)))
        return n.value

    def batch_pile(self, max_mm=6, max_alt=5, lifted=False, joined=False, min_mapq=0):
        """the same for the one-batch interface (after run() / align())"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_batch_pile(self._h, max_mm, max_alt, int(bool(lifted)), int(bool(joined)), min_mapq, C.byref(n)))
        return n.value

    def pile_records(self, seqs, lens, places, kinds=None, lift_off=None, words=None, mapq=None, min_mapq=0):
        """the same kernel on reads and records of the caller's, laid out as for md_records; mapq: one value per read in place of the records' own"""
        seqs, lens, places, lift, mapq, _keep = self._record_arrays(seqs, lens, places, kinds, lift_off, words, mapq)
        _chk(lib().bwb_hip_pile_records(self._h, seqs.ctypes.data, lens.ctypes.data, seqs.shape[1], places.ctypes.data, len(lens), *lift,
                                        mapq.ctypes.data if mapq is not None else None, min_mapq))

    def pile_counts(self, first=0, n=None, n_sites=None):
        """the counters of the sites first .. first + n - 1 as an (n, 4) uint32 array: A, C, G, T (n None: up to n_sites, which pile_begin returned)"""
        if n is None:
            n = n_sites - first
        out = np.zeros((n, 4), dtype=np.uint32)
        _chk(lib().bwb_hip_pile_counts(self._h, first, n, out.ctypes.data))
        return out

    def pile_reset(self):
        _chk(lib().bwb_hip_pile_reset(self._h))

    def pile_site_of(self, pos):
        """the site number of every text position, -1 where it is no site"""
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.zeros(len(pos), dtype=np.int64)
        _chk(lib().bwb_hip_pile_site_of(self._h, pos.ctypes.data, len(pos), out.ctypes.data))
        return out

    def pile_stats(self):
        """(reads counted, adds, kernel ms) of the last pile call that launched"""
        return self._count_steps_ms(lib().bwb_hip_pile_stats)

    # -- base qualities in the pile (-b / -Y): a minimum base quality, and device-resident quality sums beside the counters (needs pile_begin and
    #    pileq_begin; the slot forms slot_quals behind the slot's upload) --
    def pileq_begin(self, weighted=False):
        """the slots keep quality bytes from now on; weighted: zeroed quality sums, n_sites x (A, C, G, T).  After pile_begin, before the first upload"""
        _chk(lib().bwb_hip_pileq_begin(self._h, int(bool(weighted))))

    def slot_quals(self, slot, quals, stride=None):
        """the quality bytes of the slot's reads, (n_reads, stride) uint8 laid out like the upload's seqs (stride None: the array's)"""
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        if quals.ndim != 2:
            raise ValueError("quals must be (n_reads, stride) uint8")
        _chk(lib().bwb_hip_slot_quals(self._h, slot, quals.ctypes.data, max(quals.shape[1], 1) if stride is None else stride))

    def slot_pile_q(self, slot, max_mm=6, max_alt=5, lifted=False, joined=False, min_mapq=0, min_baseq=0, err_cap=0):
        """slot_pile with the slot's qualities: bases below min_baseq are dropped; err_cap 4..93 also adds min(max(Q, 4), err_cap) to the sums"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_slot_pile_q(self._h, slot, max_mm, max_alt, int(bool(lifted)), int(bool(joined)), min_mapq, min_baseq, err_cap, C.byref(n)))
        return n.value

    def batch_pile_q(self, max_mm=6, max_alt=5, lifted=False, joined=False, min_mapq=0, min_baseq=0, err_cap=0):
        """the same for the one-batch interface (after run() / align(); slot_quals(0, ...) behind the upload)"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_batch_pile_q(self._h, max_mm, max_alt, int(bool(lifted)), int(bool(joined)), min_mapq, min_baseq, err_cap, C.byref(n)))
        return n.value

    def pile_records_q(self, seqs, quals, lens, places, kinds=None, lift_off=None, words=None, mapq=None, min_mapq=0, min_baseq=0, err_cap=0):
        """pile_records with the reads' quality bytes, laid out like seqs"""
        seqs, lens, places, lift, mapq, _keep = self._record_arrays(seqs, lens, places, kinds, lift_off, words, mapq)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        if quals.shape != seqs.shape:
            raise ValueError("quals must have the shape of seqs")
        _chk(lib().bwb_hip_pile_records_q(self._h, seqs.ctypes.data, quals.ctypes.data, lens.ctypes.data, seqs.shape[1], places.ctypes.data, len(lens), *lift,
                                          mapq.ctypes.data if mapq is not None else None, min_mapq, min_baseq, err_cap))

    def pileq_sums(self, first=0, n=None, n_sites=None):
        """the quality sums of the sites first .. first + n - 1 as an (n, 4) uint32 array: A, C, G, T (n None: up to n_sites)"""
        if n is None:
            n = n_sites - first
        out = np.zeros((n, 4), dtype=np.uint32)
        _chk(lib().bwb_hip_pileq_sums(self._h, first, n, out.ctypes.data))
        return out

    def pileq_put(self, first, sums):
        """overwrites the quality sums of the sites first .. with an (n, 4) uint32 array: A, C, G, T"""
        sums = np.ascontiguousarray(sums, dtype=np.uint32).reshape(-1, 4)
        _chk(lib().bwb_hip_pileq_put(self._h, first, len(sums), sums.ctypes.data))

    def pileq_stats(self):
        """(reads counted, adds, bases dropped by min_baseq, kernel ms) of the last pile_q call that launched"""
        r, a, d, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _chk(lib().bwb_hip_pileq_stats(self._h, C.byref(r), C.byref(a), C.byref(d), C.byref(ms)))
        return r.value, a.value, d.value, ms.value

    # -- ref / alt read support per indel bubble (-I): device-resident counters, n_bub x (ref, alt, ref_gapped, alt_gapped), summed over every
    #    indel call (needs set_loci, set_bubble_chrom and indel_begin; the slot forms set_sa) --
    def indel_begin(self, anchor=1):
        """builds the sorted table of the bubbles eligible at this anchor and zeroed counters -> their number.  Before the first upload"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_indel_begin(self._h, anchor, C.byref(n)))
        return n.value

    def slot_indel(self, slot, max_mm=6, max_alt=5, joined=False, min_mapq=0):
        """counts the slot's reads -> the reads counted; a second call on the same submission counts nothing and returns 0"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_slot_indel(self._h, slot, max_mm, max_alt, int(bool(joined)), min_mapq, C.byref(n)))
        return n.value

    def batch_indel(self, max_mm=6, max_alt=5, joined=False, min_mapq=0):
        """the same for the one-batch interface (after run() / align())"""
        n = C.c_uint64()
        _chk(lib().bwb_hip_batch_indel(self._h, max_mm, max_alt, int(bool(joined)), min_mapq, C.byref(n)))
        return n.value

    def indel_records(self, places, mapq=None, min_mapq=0):
        """the same kernel on placement records of the caller's; mapq: one value per read in place of the records' own"""
        places = np.ascontiguousarray(places, dtype=PLACE_DTYPE)
        if mapq is not None:
            mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
            if len(mapq) != len(places):
                raise ValueError("one MAPQ per read")
        _chk(lib().bwb_hip_indel_records(self._h, places.ctypes.data, len(places), mapq.ctypes.data if mapq is not None else None, min_mapq))

    def indel_counts(self, first=0, n=None, n_bub=None):
        """the counters of the bubbles first .. first + n - 1 as an (n, 4) uint32 array: ref, alt, ref_gapped, alt_gapped (n None: up to n_bub)"""
        if n is None:
            n = n_bub - first
        out = np.zeros((n, 4), dtype=np.uint32)
        _chk(lib().bwb_hip_indel_counts(self._h, first, n, out.ctypes.data))
        return out

    def indel_reset(self):
        _chk(lib().bwb_hip_indel_reset(self._h))

    def indel_stats(self):
        """(reads counted, adds, candidates examined, kernel ms) of the last indel call that launched"""
        r, a, k, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _chk(lib().bwb_hip_indel_stats(self._h, C.byref(r), C.byref(a), C.byref(k), C.byref(ms)))
        return r.value, a.value, k.value, ms.value

    # -- genotype calls at the IUPAC sites and the indel bubbles (-G): from the pile and indel counters that live on the device (needs pile_begin,
    #    for bubbles indel_begin, then geno_begin) --
    def geno_begin(self, piece):
        """scratch and pinned output for `piece` sites (and, after indel_begin, min(piece, n_bub) bubbles).  Before the first upload"""
        _chk(lib().bwb_hip_geno_begin(self._h, piece))

    def pile_put(self, first, counts):
        """overwrites the counters of the sites first .. with an (n, 4) uint32 array: A, C, G, T"""
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 4)
        _chk(lib().bwb_hip_pile_put(self._h, first, len(counts), counts.ctypes.data))

    def indel_put(self, first, counts):
        """overwrites the counters of the bubbles first .. with an (n, 4) uint32 array: ref, alt, ref_gapped, alt_gapped"""
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 4)
        _chk(lib().bwb_hip_indel_put(self._h, first, len(counts), counts.ctypes.data))

    def _geno(self, fn, dtype, first, n, err, min_depth):
        out, k = C.c_void_p(), C.c_uint64()
        _chk(fn(self._h, first, n, err, min_depth, C.byref(out), C.byref(k)))
        if not k.value:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(out.value, k.value * dtype.itemsize), dtype=dtype).copy()

    def geno_sites(self, first, n, err=20, min_depth=1):
        """the records (GENO_SITE_DTYPE, a copy) of the called sites among first .. first + n - 1, in site order"""
        return self._geno(lib().bwb_hip_geno_sites, GENO_SITE_DTYPE, first, n, err, min_depth)

    def geno_sites_q(self, first, n, err=20, min_depth=1):
        """the same by the weighted rule, from the counters and the quality sums (GENO_SITE_Q_DTYPE; needs pileq_begin(weighted) before geno_begin)"""
        return self._geno(lib().bwb_hip_geno_sites_q, GENO_SITE_Q_DTYPE, first, n, err, min_depth)

    def geno_bubbles(self, first, n, err=20, min_depth=1):
        """the records (GENO_BUBBLE_DTYPE, a copy) of the called bubbles among first .. first + n - 1, in bubble order"""
        return self._geno(lib().bwb_hip_geno_bubbles, GENO_BUBBLE_DTYPE, first, n, err, min_depth)

    def geno_stats(self):
        """(sites the last geno_sites called, bubbles the last geno_bubbles called, kernel ms of whichever launched last)"""
        return self._count_steps_ms(lib().bwb_hip_geno_stats)

    def dtab_info(self):
        """the context's calculate_d table: {K (0: none), build seconds, bytes}"""
        k, sec, nb = C.c_int(), C.c_double(), C.c_uint64()
        _chk(lib().bwb_hip_dtab_info(self._h, C.byref(k), C.byref(sec), C.byref(nb)))
        return {"K": k.value, "build_s": round(sec.value, 3), "GB": round(nb.value / 1e9, 2)}

    def locate_stats(self):
        """(rows, invPsi steps = rank-block visits, kernel ms) of the last locate()"""
        return self._count_steps_ms(lib().bwb_hip_locate_stats)


# -- formats ------------------------------------------------------------------------------------


def read_ann(path):
    """.ann of `bwbble index` (io.c:324-349) -> (names, first text positions, last text positions: uint64)"""
    with open(path) as f:
        n = int(f.readline().split("\t")[1])
        rows = [f.readline().rstrip("\n").split("\t") for _ in range(n)]
    return ([r[0] for r in rows], np.array([int(r[1]) for r in rows], dtype=np.uint64), np.array([int(r[2]) for r in rows], dtype=np.uint64))


def read_ref(path_fa):
    """the forward text of <fasta>.ref (`bwbble index` / `fasta2ref`): one code per byte, n_fwd = the first number of <fasta>.ann"""
    with open(str(path_fa) + ".ann") as f:
        n_fwd = int(f.readline().split("\t")[0])
    if os.path.getsize(str(path_fa) + ".ref") != 2 * n_fwd:
        raise ValueError(f"{path_fa}.ref: not 2 x {n_fwd} bytes (bwbble fasta2ref writes it)")
    return np.fromfile(str(path_fa) + ".ref", dtype=np.uint8, count=n_fwd)


def read_bubble_data(path):
    """bubble.data of the reference's `comb` (mg-ref/comb.cpp:245-253) -> (chromosome headers, BUBBLE_DTYPE records): two lines per bubble,
    the header and `A  B-A  C  D-C  ref_len  alt_len`.  Half a pair or a numbers line without six integers is an error, as in the host tools."""
    lines = open(path).read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) % 2:
        raise ValueError(f"{path} has an odd number of lines")
    anns, recs = lines[0::2], np.zeros(len(lines) // 2, dtype=BUBBLE_DTYPE)
    for k, ln in enumerate(lines[1::2]):
        v = ln.split()
        if len(v) < 6:
            raise ValueError(f"{path} line {2 * k + 2}: expected six integers")
        recs[k] = tuple(int(x) for x in v[:6])
    return anns, recs


def bubble_of(names, n_bubbles):
    """the bubble number of every .ann record as the reference's sam_pad reads it from the name (mg-ref/sam_pad.cpp:67-72): -1 unless the name
    starts with `bubble`, else the leading decimal number (0 without one) of its first word after the word's first six characters"""
    import re
    out = np.full(len(names), -1, dtype=np.int32)
    for i, name in enumerate(names):
        if name.startswith("bubble"):
            m = re.match(r"[+-]?[0-9]+", name.split()[0][6:])
            w = int(m.group()) if m else 0
            if not 0 <= w < n_bubbles:
                raise ValueError(f"record {i} ({name!r}) names a bubble outside the table of {n_bubbles}")
            out[i] = w
    return out


def bubble_chrom_of(names, anns):
    """the .ann record of the chromosome every bubble lies on (-J, -R): the one record whose name's first word is the first word of the bubble's
    header line in bubble.data (anns, see read_bubble_data()); none, several, or a bubble record is an error, as in the host tools"""
    word = lambda t: t.split()[0] if t.split() else ""
    by_word = {}
    for i, n in enumerate(names):
        by_word.setdefault(word(n), []).append(i)
    out = np.zeros(len(anns), dtype=np.int32)
    for b, a in enumerate(anns):
        w = word(a)
        hits = by_word.get(w, [])
        if len(hits) != 1 or names[hits[0]].startswith("bubble"):
            raise ValueError(f"bubble {b} ({a!r}): {len(hits)} records are named {w!r}" if len(hits) != 1 else f"bubble {b} ({a!r}): record {hits[0]} is itself a bubble record")
        out[b] = hits[0]
    return out


def lift_record(words, off):
    """(pos, seqid, [(len, op), ...]) of the record that starts at 16-byte word `off` of slot_lift's words"""
    hdr = words[int(off)].view(LIFT_DTYPE)[0]
    ops = words[int(off) + 1:int(off) + 1 + (int(hdr["n_ops"]) + 3) // 4].reshape(-1)[:int(hdr["n_ops"])]
    return int(hdr["pos"]), int(hdr["seqid"]), [(int(v) >> 4, int(v) & 15) for v in ops]


_BASE_LUT = np.full(256, 4, dtype=np.uint8)  # ASCII -> read->seq code (io.h:112-130): A0 G1 C2 T3 in either case, anything else 4
_BASE_LUT[np.frombuffer(b"AGCTagct", dtype=np.uint8)] = np.arange(8) % 4


def encode_reads(ascii_reads):
    """read->seq codes of fastq2reads (io.c:467; io.h:112-130): A0 G1 C2 T3, anything else 4."""
    lens = np.array([len(r) for r in ascii_reads], dtype=np.uint16)
    stride = int(lens.max()) if len(lens) else 1
    seqs = np.full((len(ascii_reads), max(stride, 1)), 4, dtype=np.uint8)
    for i, r in enumerate(ascii_reads):
        seqs[i, :len(r)] = _BASE_LUT[np.frombuffer(r.encode(), dtype=np.uint8)]
    return seqs, lens


def load_fastq_codes(path, max_reads=0, chunk=500000):
    """FASTQ -> (codes (n, stride) uint8, lens uint16) without a Python loop per read (same encoding as encode_reads);
    the gather runs over `chunk` reads at a time so that a 10 M-read file does not need tens of GB of index temporaries."""
    data = np.fromfile(path, dtype=np.uint8)
    nl = np.flatnonzero(data == 10)
    if len(data) and data[-1] != 10:
        nl = np.append(nl, len(data))
    n = len(nl) // 4
    if max_reads:
        n = min(n, max_reads)
    if n == 0:
        return np.full((0, 1), 4, dtype=np.uint8), np.zeros(0, dtype=np.uint16)
    e0 = nl[1:4 * n:4]
    s0 = nl[0:4 * n:4] + 1
    lens = (e0 - s0).astype(np.uint16)
    stride = int(lens.max())
    seqs = np.empty((n, stride), dtype=np.uint8)
    cols = np.arange(stride)[None, :]
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        idx = s0[a:b, None] + cols
        valid = cols < lens[a:b, None]
        seqs[a:b] = np.where(valid, _BASE_LUT[data[np.minimum(idx, len(data) - 1)]], 4)
    return seqs, lens


def read_fastq(path, max_reads=0):
    """Sequence lines of a 4-line FASTQ (the subset of fastq2reads, io.c:410-515, that align needs)."""
    out = []
    with open(path) as f:
        while True:
            name = f.readline()
            if not name:
                break
            if not name.startswith("@"):
                continue
            seq = f.readline().rstrip("\n")
            f.readline()
            f.readline()
            out.append(seq)
            if max_reads and len(out) >= max_reads:
                break
    return out


def aln_path(rec):
    """Edit path bytes (index 0 = first backward-search step) of one hit from its gap runs."""
    alen = int(rec["aln_length"])
    path = np.zeros(256 + 8, dtype=np.uint8)
    for run in rec["gap_run"]:
        run = int(run)
        if run == 0xFFFF:
            continue
        start, ln, is_del = run & 0xFF, (run >> 8) & 0x7F, run >> 15
        path[start:start + ln] = 2 if is_del else 1
    return path[:alen]


def aln_bytes(aln_off, alns):
    """Serialises hits exactly like alns2alnf_bin (align.c:345-382): the bytes of a .aln file."""
    out = bytearray()
    i32 = lambda v: int(v).to_bytes(4, "little", signed=True)
    for r in range(len(aln_off) - 1):
        lo, hi = int(aln_off[r]), int(aln_off[r + 1])
        out += i32(hi - lo)
        for rec in alns[lo:hi]:
            out += i32(rec["score"]) + int(rec["L"]).to_bytes(8, "little") + int(rec["U"]).to_bytes(8, "little")
            out += i32(rec["num_mm"]) + i32(rec["num_gapo"]) + i32(rec["num_gape"]) + i32(rec["aln_length"])
            path = aln_path(rec)
            if len(path) == 0:
                out += i32(0)
                continue
            pairs = []
            state, count = int(path[-1]), 1
            for s in path[-2::-1]:
                if int(s) == state:
                    count += 1
                else:
                    pairs.append(state | (count << 2))
                    state, count = int(s), 1
            pairs.append(state | (count << 2))
            out += i32(len(pairs))
            for v in pairs:
                out += i32(v)
    return bytes(out)
