"""ctypes binding of libc3hip.so (C ABI: include/c3hip.h).

The reference binds its native code with cffi in API mode (build.py:38-85 -> ``libclair3.lib.<fn>``); cffi is
not installed in this image, so the binding below uses ctypes against the same C ABI -- INTEGRATION.md
shows the equivalent cffi ``cdef``.  There is NO fallback: if the HIP library is missing or cannot be
loaded, importing a model fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("C3HIP_LIB", os.path.join(_HERE, "lib", "libc3hip.so"))

KIND_PILEUP = 0
KIND_FULL_ALIGNMENT = 1
DTYPE_I8, DTYPE_I32, DTYPE_F32, DTYPE_I64 = 0, 1, 2, 3
# status of a candidate (C3_CAND_* in include/c3hip.h)
CAND_NO_WINDOW, CAND_MAIN, CAND_EMPTY_COLUMN, CAND_HEAD, CAND_TAIL = 0, 1, 2, 3, 4

# every symbol include/c3hip.h declares (tests/test_abi.py checks the header against this list)
EXPORTS = (
    "c3_version", "c3_last_error", "c3_device_count", "c3_mem_info", "c3_device_pci_bus_id", "c3_model_create", "c3_model_set_geometry",
    "c3_model_load", "c3_model_output_size", "c3_model_row_size", "c3_model_set_decode_columns", "c3_model_window_bytes", "c3_predict", "c3_predict_submit", "c3_predict_submit_dev",
    "c3_predict_wait", "c3_comm_unique_id", "c3_comm_create", "c3_comm_destroy", "c3_gather_rows", "c3_comm_count", "c3_comm_abort", "c3_stream_wait", "c3_model_describe", "c3_model_set_sharing", "c3_predict_device", "c3_predict_device_checked", "c3_model_range_status", "c3_predict_pileup_region", "c3_outcome_maxima", "c3_decode_columns", "c3_vcf_rows", "c3_model_synchronize", "c3_model_destroy", "c3_debug_fetch",
    "c3_debug_keep_activations", "c3_debug_tap", "c3_debug_tap_fetch", "c3_profile_enable", "c3_profile_reset", "c3_profile_read",
    "c3_model_set_max_depth", "c3_predict_depth", "c3_predict_submit_depth", "c3_predict_pileup_region_depth", "c3_predict_submit_region",
    "c3_predict_submit_candidates", "c3_predict_pileup_candidates",
    "c3_predict_submit_rows", "c3_predict_rows", "c3_pack_rows",
    "c3_model_set_verify", "c3_model_verify_stats", "c3_model_verify_reset",
    "c3_model_set_verify_layers", "c3_model_verify_layers",
    "c3_model_set_layer_precision", "c3_model_layer_precision", "c3_layer_precision_check",
    "c3_model_calibrate", "c3_model_calibrate_reset", "c3_model_calibration_census", "c3_model_calibration_solve",
    "c3_model_set_channel_lowering", "c3_model_set_calibration_origin", "c3_model_channel_exps", "c3_calibration_rule",
    "c3_model_set_exact", "c3_predict_exact", "c3_exact_fetch",
    "c3_model_set_answer", "c3_model_set_verify_reference", "c3_model_verify_extra",
    "c3_model_set_range_policy", "c3_range_policy_check", "c3_model_range_stats",
    "c3_predict_submit_parts", "c3_predict_parts",
    "c3_model_set_score", "c3_score_submit", "c3_score_wait", "c3_score", "c3_score_rows",
    "c3_model_set_score_census", "c3_score_census_read", "c3_score_census_reset",
    "c3_model_set_refine", "c3_model_refine_stats", "c3_model_refine_reset", "c3_refine_select",
    "c3_jackknife_rows", "c3_jackknife", "c3_jackknife_reduce",
    "c3_subsample_rows", "c3_subsample", "c3_subsample_reduce",
    "c3_occlude", "c3_occlude_rows", "c3_occlude_reduce",
    "c3_gvcf_site", "c3_gvcf_site_table", "c3_gvcf_blocks_host", "c3_gvcf_create", "c3_gvcf_destroy", "c3_gvcf_blocks_counts",
    "c3_gvcf_blocks_region", "c3_gvcf_text", "c3_gvcf_tile_sites", "c3_gvcf_top_span", "c3_gvcf_table_depth",
    "c3_pileup_create", "c3_pileup_destroy", "c3_pileup_reads", "c3_pileup_reads_host", "c3_pileup_sizes", "c3_pileup_result", "c3_pileup_stats",
    "c3_pileup_tile_sites",
    "c3_predict_submit_pileup", "c3_predict_pileup_reads",
    "c3_fa_reads_create", "c3_fa_reads_destroy", "c3_fa_reads", "c3_fa_reads_host", "c3_fa_reads_sizes", "c3_fa_reads_result", "c3_fa_reads_stats",
    "c3_fa_lds_reads",
    "c3_predict_submit_fa_reads", "c3_predict_fa_reads",
    "c3_fa_haplotag", "c3_fa_haplotag_host", "c3_fa_haplotag_sizes", "c3_fa_haplotag_result", "c3_fa_haplotag_stats", "c3_fa_haplotag_shape",
    "c3_fa_reads_phased", "c3_fa_reads_phased_host",
    "c3_fa_reads_dwell", "c3_fa_reads_dwell_host", "c3_fa_reads_channels", "c3_fa_dwell_cum_host", "c3_fa_dwell_table", "c3_fa_dwell_step",
)
# layout of a leave-one-read-out variant (C3_JACKKNIFE_* in include/c3hip.h)
JACKKNIFE_LAYOUT = {"recentre": 0, "in_place": 1}
MAX_PARTS = 64  # C3_MAX_PARTS (include/c3hip.h)
# policy of verify mode (C3_VERIFY_* in include/c3hip.h)
VERIFY_REPORT, VERIFY_ESCALATE, VERIFY_REPLACE = 0, 1, 2
VERIFY_POLICY = {VERIFY_REPORT: "report", VERIFY_ESCALATE: "escalate", VERIFY_REPLACE: "replace"}
# what verify mode compares with (C3_VERIFY_REF_*) and what answers a batch of the ring (C3_ANSWER_*)
VERIFY_REF = {"fp32": 0, "exact": 1}
ANSWER = {"product": 0, "exact": 1}
# policy of the range guard (C3_RANGE_* in include/c3hip.h)
RANGE_STICKY, RANGE_RECALIBRATE = 0, 1
# status of a layer of verify mode's layer records (C3_VERIFY_LAYER_* in include/c3hip.h)
VERIFY_LAYER_STATUS = {0: "none", 1: "compared", 2: "fused"}


class RowsConfig(C.Structure):
    """c3_rows_config (include/c3hip.h)"""
    _fields_ = [("width", C.c_int32), ("flank", C.c_int32), ("show_reference", C.c_int32), ("keep_iupac", C.c_int32),
                ("has_qs_pass", C.c_int32), ("pileup", C.c_int32), ("max_len", C.c_int32), ("infer", C.c_int32),
                ("f32_arith", C.c_int32), ("walk", C.c_int32), ("gvcf", C.c_int32), ("haploid", C.c_int32),
                ("long_indel", C.c_int32), ("long_infer", C.c_int32), ("qs_pass", C.c_double), ("phred_trans", C.c_double), ("long_prop", C.c_double),
                ("gt", (C.c_char * 8) * 4)]


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("dtype", C.c_int32), ("ndim", C.c_int32), ("shape", C.c_int64 * 4),
                ("data", C.c_void_p)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("mfma_flops", C.c_double), ("mfma_peak_tflops", C.c_double)]


class VerifyStats(C.Structure):
    """c3_verify_stats (include/c3hip.h)"""
    _fields_ = [("batches_submitted", C.c_int64), ("batches_checked", C.c_int64), ("batches_skipped", C.c_int64),
                ("windows_checked", C.c_int64), ("worst_batch", C.c_int64), ("worst_row", C.c_int64), ("rows_over_tol", C.c_int64),
                ("label_diffs", C.c_int64 * 4), ("near_ties", C.c_int64 * 4), ("escalations", C.c_int64),
                ("max_abs_diff", C.c_float), ("head_max_abs_diff", C.c_float * 4), ("tol", C.c_float), ("near_tie", C.c_float),
                ("every", C.c_int32), ("policy", C.c_int32)]


class VerifyExtra(C.Structure):
    """c3_verify_extra (include/c3hip.h)"""
    _fields_ = [("reference", C.c_int32), ("reserved", C.c_int32), ("rows_replaced", C.c_int64), ("batches_with_replacements", C.c_int64),
                ("max_abs_diff_f64", C.c_double)]


class VerifyLayer(C.Structure):
    """c3_verify_layer (include/c3hip.h)"""
    _fields_ = [("name", C.c_char * 16), ("status", C.c_int32), ("reserved", C.c_int32), ("batches", C.c_int64), ("windows", C.c_int64),
                ("worst_batch", C.c_int64), ("worst_window", C.c_int64), ("worst_index", C.c_int64), ("max_abs_diff", C.c_float),
                ("ref_max_abs", C.c_float), ("test_max_abs", C.c_float), ("reserved2", C.c_float)]


class RangeStats(C.Structure):
    """c3_range_stats (include/c3hip.h)"""
    _fields_ = [("trips", C.c_int64), ("recalibrations", C.c_int64), ("reruns", C.c_int64), ("census_windows", C.c_int64),
                ("channels_lowered", C.c_int32), ("cap_log2", C.c_int32), ("policy", C.c_int32), ("max_recalibrations", C.c_int32),
                ("fell_back", C.c_int32), ("reason", C.c_char * 96)]


class ScoreResult(C.Structure):
    """c3_score_result (include/c3hip.h)"""
    _fields_ = [("windows", C.c_int64), ("tasks", C.c_int32), ("reserved", C.c_int32), ("loss_sum", C.c_double * 4),
                ("correct", C.c_int64 * 4), ("nonfinite", C.c_int64)]


class ScoreCensus(C.Structure):
    """c3_score_census (include/c3hip.h)"""
    _fields_ = [("windows", C.c_int64), ("tasks", C.c_int32), ("reserved", C.c_int32), ("confusion", C.c_int64 * 2628),
                ("rel_windows", (C.c_int64 * 20) * 4), ("rel_correct", (C.c_int64 * 20) * 4), ("rel_conf_q32", (C.c_int64 * 20) * 4),
                ("rel_skipped", C.c_int64 * 4), ("gap_below", (C.c_int64 * 6) * 4)]


class RefineStats(C.Structure):
    """c3_refine_stats (include/c3hip.h)"""
    _fields_ = [("batches", C.c_int64), ("batches_refined", C.c_int64), ("batches_skipped", C.c_int64), ("windows", C.c_int64),
                ("windows_selected", C.c_int64), ("windows_changed", C.c_int64), ("head_selected", C.c_int64 * 4),
                ("decoder_selected", C.c_int64), ("min_gap", C.c_float * 4), ("max_abs_diff", C.c_float), ("gap", C.c_float)]


class JackknifeWindow(C.Structure):
    """c3_jackknife_window (include/c3hip.h); synthetic.JACKKNIFE_DTYPE is the same record as a numpy dtype"""
    _fields_ = [("reads", C.c_int32), ("nonfinite", C.c_int32), ("flips", C.c_int32 * 4), ("decision_flips", C.c_int32 * 4),
                ("lean_read", C.c_int32 * 4), ("lean_drop", C.c_float * 4), ("max_delta", C.c_float), ("reserved", C.c_int32)]


class JackknifeInfo(C.Structure):
    """c3_jackknife_info (include/c3hip.h)"""
    _fields_ = [("windows", C.c_int64), ("variants", C.c_int64), ("passes", C.c_int64), ("bytes_staged", C.c_int64),
                ("on_fp32", C.c_int32), ("reserved", C.c_int32), ("expand_us", C.c_float), ("reduce_us", C.c_float)]


class SubsampleLevel(C.Structure):
    """c3_subsample_level (include/c3hip.h); synthetic.SUBSAMPLE_LEVEL_DTYPE is the same record as a numpy dtype"""
    _fields_ = [("keep", C.c_int32), ("run", C.c_int32), ("nonfinite", C.c_int32), ("decision_flips", C.c_int32), ("flips", C.c_int32 * 4),
                ("min_kept", C.c_float * 4)]


class SubsampleWindow(C.Structure):
    """c3_subsample_window (include/c3hip.h); synthetic.SUBSAMPLE_WINDOW_DTYPE is the same record as a numpy dtype"""
    _fields_ = [("reads", C.c_int32), ("levels_run", C.c_int32), ("hold_level", C.c_int32 * 4), ("hold_decision", C.c_int32), ("reserved", C.c_int32)]


class SubsampleInfo(C.Structure):
    """c3_subsample_info (include/c3hip.h)"""
    _fields_ = [("windows", C.c_int64), ("variants", C.c_int64), ("passes", C.c_int64), ("bytes_staged", C.c_int64),
                ("on_fp32", C.c_int32), ("reserved", C.c_int32), ("expand_us", C.c_float), ("reduce_us", C.c_float)]


# what occlusion mode sets to zero (C3_OCCLUDE_* in include/c3hip.h)
OCCLUDE_WHAT = {"channels": 1, "bands": 2, "both": 3}


class OccludeWindow(C.Structure):
    """c3_occlude_window (include/c3hip.h); synthetic.OCCLUDE_DTYPE is the same record as a numpy dtype"""
    _fields_ = [("variants", C.c_int32), ("nonfinite", C.c_int32), ("flips", C.c_int32 * 4 * 2), ("decision_flips", C.c_int32 * 4 * 2),
                ("lean", C.c_int32 * 4 * 2), ("lean_drop", C.c_float * 4 * 2), ("max_delta", C.c_float), ("reserved", C.c_int32)]


class OccludeInfo(C.Structure):
    """c3_occlude_info (include/c3hip.h)"""
    _fields_ = [("windows", C.c_int64), ("variants", C.c_int64), ("passes", C.c_int64), ("bytes_staged", C.c_int64),
                ("on_fp32", C.c_int32), ("reserved", C.c_int32), ("expand_us", C.c_float), ("reduce_us", C.c_float)]


GVCF_MORE = 2  # C3_GVCF_MORE (include/c3hip.h)


class GvcfConfig(C.Structure):
    """c3_gvcf_config (include/c3hip.h)"""
    _fields_ = [("base_err", C.c_double), ("gq_bin_size", C.c_int32), ("bp_resolution", C.c_int32)]


class GvcfBlock(C.Structure):
    """c3_gvcf_block (include/c3hip.h); gvcf.BLOCK_DTYPE is the same record as a numpy dtype"""
    _fields_ = [("pos", C.c_int64), ("end", C.c_int64), ("min_dp", C.c_int32), ("max_dp", C.c_int32), ("gq", C.c_int32), ("pl", C.c_int32 * 3),
                ("ref", C.c_uint8), ("gt", C.c_uint8), ("per_site", C.c_uint8), ("first_n", C.c_uint8), ("reserved", C.c_int32)]


class ReadSetC(C.Structure):
    """c3_read_set (include/c3hip.h)"""
    _fields_ = [("n_reads", C.c_int64), ("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p), ("cigar_first", C.c_void_p),
                ("cigar", C.c_void_p), ("seq_first", C.c_void_p), ("seq", C.c_void_p)]


class PileupConfig(C.Structure):
    """c3_pileup_config (include/c3hip.h)"""
    _fields_ = [("min_depth", C.c_int64), ("min_snp_af", C.c_float), ("min_indel_af", C.c_float), ("min_mq", C.c_int32),
                ("max_indel_length", C.c_int32), ("call_snp_only", C.c_int32), ("gvcf", C.c_int32), ("call_ht", C.c_int32), ("reserved", C.c_int32),
                ("hash_mask", C.c_uint64)]


class ReadExtrasC(C.Structure):
    """c3_read_extras (include/c3hip.h)"""
    _fields_ = [("qual_first", C.c_void_p), ("qual", C.c_void_p), ("haplotype", C.c_void_p), ("name_key", C.c_void_p)]


class ReadMovesC(C.Structure):
    """c3_read_moves (include/c3hip.h)"""
    _fields_ = [("mv_first", C.c_void_p), ("mv", C.c_void_p)]


class FaConfig(C.Structure):
    """c3_fa_config (include/c3hip.h)"""
    _fields_ = [("min_mq", C.c_int32), ("max_indel_length", C.c_int32), ("matrix_depth", C.c_int32), ("lds_reads", C.c_int32), ("seed", C.c_uint64)]


class FaCounters(C.Structure):
    """c3_fa_counters (include/c3hip.h)"""
    _fields_ = [("reads_kept", C.c_int64), ("reads_dropped", C.c_int64), ("rows", C.c_int64), ("deep_windows", C.c_int64),
                ("fell_back", C.c_int32), ("on_host", C.c_int32), ("kernel_ms", C.c_float * 8)]


class PhasedVariantsC(C.Structure):
    """c3_phased_variants (include/c3hip.h)"""
    _fields_ = [("n", C.c_int64), ("pos", C.c_void_p), ("alt_base", C.c_void_p), ("genotype", C.c_void_p), ("phase_set", C.c_void_p)]


class HaplotagConfig(C.Structure):
    """c3_haplotag_config (include/c3hip.h)"""
    _fields_ = [("min_haplotag_mq", C.c_int32), ("reserved", C.c_int32)]


class HaplotagCounters(C.Structure):
    """c3_haplotag_counters (include/c3hip.h)"""
    _fields_ = [("reads_hap", C.c_int64 * 3), ("reads_low_mapq", C.c_int64), ("pairs_realigned", C.c_int64), ("pairs_allele0", C.c_int64),
                ("on_host", C.c_int32), ("reserved", C.c_int32), ("kernel_ms", C.c_float * 8)]


class PileupCounters(C.Structure):
    """c3_pileup_counters (include/c3hip.h)"""
    _fields_ = [("reads_kept", C.c_int64), ("reads_dropped", C.c_int64), ("events", C.c_int64), ("collisions", C.c_int64),
                ("fell_back", C.c_int32), ("on_host", C.c_int32), ("kernel_ms", C.c_float * 8)]


class C3Error(RuntimeError):
    pass


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7, found through $ORIGIN) while libc3hip.so's RUNPATH points at /opt/rocm.  If libc3hip is
    loaded first, a later ``import torch`` brings a SECOND copy of the runtime whose HSA initialisation fails
    ("No HIP GPUs are available").  Pre-loading torch's copy (without importing torch) makes libc3hip's
    NEEDED libamdhip64.so.7 resolve to it, so both share one runtime whatever the import order.  Without
    torch installed nothing happens and /opt/rocm's runtime is used."""
    import importlib.machinery
    import sys
    from . import lazy_torch
    if "torch" in sys.modules and not lazy_torch.standing_in():
        return
    # (PathFinder, not importlib.util.find_spec: with lazy_torch's stand-in in sys.modules the latter looks at ITS __spec__; the package
    # may still be imported later in this process, and must then find the runtime it expects)
    try:
        spec = importlib.machinery.PathFinder.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load libc3hip.so once; raise if it is not there (no CPU fallback by design)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise C3Error(f"{LIB_PATH} not found: build it with `python -m clair3_amd.build` "
                      "(hipcc --offload-arch=gfx950); clair3_amd has no CPU fallback")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    L.c3_version.restype = C.c_char_p
    L.c3_last_error.restype = C.c_char_p
    L.c3_device_count.restype = C.c_int
    L.c3_mem_info.argtypes = [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.c3_vcf_rows.argtypes = [C.POINTER(RowsConfig), C.c_int64, C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                              C.c_void_p, C.c_void_p]
    L.c3_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.c3_model_create.restype = C.c_void_p
    L.c3_model_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.c3_model_set_geometry.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.c3_model_load.argtypes = [C.c_void_p, C.POINTER(TensorDesc), C.c_int]
    L.c3_model_output_size.argtypes = [C.c_void_p]
    L.c3_model_row_size.argtypes = [C.c_void_p]
    L.c3_model_set_decode_columns.argtypes = [C.c_void_p, C.c_int]
    L.c3_model_window_bytes.restype = C.c_int64
    L.c3_model_window_bytes.argtypes = [C.c_void_p, C.c_int]
    L.c3_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    L.c3_predict_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int]
    L.c3_predict_submit_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int]
    L.c3_predict_wait.argtypes = [C.c_void_p, C.c_int]
    L.c3_predict_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    L.c3_comm_unique_id.argtypes = [C.c_void_p]
    L.c3_comm_create.restype = C.c_void_p
    L.c3_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.c3_comm_destroy.argtypes = [C.c_void_p]
    L.c3_gather_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_void_p]
    L.c3_comm_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.c3_comm_abort.argtypes = [C.c_void_p]
    L.c3_stream_wait.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.c3_model_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.c3_model_set_sharing.argtypes = [C.c_void_p, C.c_int]
    L.c3_predict_device_checked.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    L.c3_model_range_status.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.c3_predict_pileup_region.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    L.c3_model_set_max_depth.argtypes = [C.c_void_p, C.c_int]
    L.c3_predict_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    L.c3_predict_submit_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.c3_predict_pileup_region_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.c3_predict_submit_region.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.c3_predict_submit_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]
    L.c3_predict_pileup_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.c3_predict_submit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
    L.c3_predict_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.c3_predict_submit_parts.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int]
    L.c3_predict_parts.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.c3_pack_rows.restype = C.c_int64
    L.c3_pack_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.c3_model_set_verify.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int]
    L.c3_model_verify_stats.argtypes = [C.c_void_p, C.POINTER(VerifyStats)]
    L.c3_model_verify_reset.argtypes = [C.c_void_p]
    L.c3_model_set_verify_layers.argtypes = [C.c_void_p, C.c_int]
    L.c3_model_set_layer_precision.argtypes = [C.c_void_p, C.c_char_p]
    L.c3_model_layer_precision.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.c3_layer_precision_check.argtypes = [C.c_int, C.c_char_p]
    L.c3_model_verify_layers.argtypes = [C.c_void_p, C.POINTER(VerifyLayer), C.c_int]
    L.c3_model_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    L.c3_model_calibrate_reset.argtypes = [C.c_void_p]
    L.c3_model_calibration_census.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.c3_model_calibration_solve.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.c3_model_set_channel_lowering.argtypes = [C.c_void_p, C.c_void_p]
    L.c3_model_set_calibration_origin.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    L.c3_model_channel_exps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.c3_calibration_rule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.c3_model_set_exact.argtypes = [C.c_void_p, C.c_int]
    L.c3_predict_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    L.c3_exact_fetch.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    L.c3_model_set_answer.argtypes = [C.c_void_p, C.c_int]
    L.c3_model_set_verify_reference.argtypes = [C.c_void_p, C.c_int]
    L.c3_model_verify_extra.argtypes = [C.c_void_p, C.POINTER(VerifyExtra)]
    L.c3_model_set_range_policy.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.c3_range_policy_check.argtypes = [C.c_char_p]
    L.c3_model_range_stats.argtypes = [C.c_void_p, C.POINTER(RangeStats)]
    L.c3_model_set_score.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    L.c3_score_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.c3_score_wait.argtypes = [C.c_void_p, C.c_int, C.POINTER(ScoreResult)]
    L.c3_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ScoreResult)]
    L.c3_score_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.POINTER(ScoreResult), C.c_void_p]
    L.c3_model_set_score_census.argtypes = [C.c_void_p, C.c_int]
    L.c3_score_census_read.argtypes = [C.c_void_p, C.POINTER(ScoreCensus)]
    L.c3_score_census_reset.argtypes = [C.c_void_p]
    L.c3_model_set_refine.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.c3_model_refine_stats.argtypes = [C.c_void_p, C.POINTER(RefineStats)]
    L.c3_model_refine_reset.argtypes = [C.c_void_p]
    L.c3_refine_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    L.c3_jackknife_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(JackknifeInfo)]
    L.c3_jackknife.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(JackknifeInfo)]
    L.c3_jackknife_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.c3_subsample_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SubsampleInfo)]
    L.c3_subsample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SubsampleInfo)]
    L.c3_occlude.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(OccludeInfo)]
    L.c3_occlude_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(OccludeInfo)]
    L.c3_occlude_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    L.c3_subsample_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]
    L.c3_gvcf_site.argtypes = [C.POINTER(GvcfConfig), C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    L.c3_gvcf_site_table.argtypes = [C.POINTER(GvcfConfig), C.c_int, C.c_void_p]
    L.c3_gvcf_blocks_host.argtypes = [C.POINTER(GvcfConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                      C.POINTER(C.c_int64)]
    L.c3_gvcf_create.restype = C.c_void_p
    L.c3_gvcf_create.argtypes = [C.c_int, C.POINTER(GvcfConfig)]
    L.c3_gvcf_destroy.argtypes = [C.c_void_p]
    L.c3_gvcf_blocks_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int64)]
    L.c3_gvcf_blocks_region.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_int64, C.POINTER(C.c_int64)]
    L.c3_gvcf_text.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.c3_gvcf_top_span.restype = C.c_int64
    L.c3_pileup_create.restype = C.c_void_p
    L.c3_pileup_create.argtypes = [C.c_int]
    L.c3_pileup_destroy.argtypes = [C.c_void_p]
    for fn in (L.c3_pileup_reads, L.c3_pileup_reads_host):
        fn.argtypes = [C.c_void_p, C.POINTER(ReadSetC), C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(PileupConfig)]
    L.c3_pileup_sizes.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 4
    L.c3_pileup_result.argtypes = [C.c_void_p] * 8
    L.c3_pileup_stats.argtypes = [C.c_void_p, C.POINTER(PileupCounters)]
    L.c3_predict_submit_pileup.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]
    L.c3_predict_pileup_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.c3_fa_reads_create.restype = C.c_void_p
    L.c3_fa_reads_create.argtypes = [C.c_int]
    L.c3_fa_reads_destroy.argtypes = [C.c_void_p]
    for fn in (L.c3_fa_reads, L.c3_fa_reads_host):
        fn.argtypes = [C.c_void_p, C.POINTER(ReadSetC), C.POINTER(ReadExtrasC), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                       C.POINTER(FaConfig)]
    L.c3_fa_reads_sizes.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3 + [C.POINTER(C.c_int32)]
    L.c3_fa_reads_result.argtypes = [C.c_void_p] * 5
    L.c3_fa_reads_stats.argtypes = [C.c_void_p, C.POINTER(FaCounters)]
    L.c3_predict_submit_fa_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]
    L.c3_predict_fa_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    for fn in (L.c3_fa_haplotag, L.c3_fa_haplotag_host):
        fn.argtypes = [C.c_void_p, C.POINTER(ReadSetC), C.POINTER(PhasedVariantsC), C.c_void_p, C.c_int64, C.c_int64, C.POINTER(HaplotagConfig)]
    L.c3_fa_haplotag_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.c3_fa_haplotag_result.argtypes = [C.c_void_p] * 4
    L.c3_fa_haplotag_stats.argtypes = [C.c_void_p, C.POINTER(HaplotagCounters)]
    L.c3_fa_haplotag_shape.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    for fn in (L.c3_fa_reads_phased, L.c3_fa_reads_phased_host):
        fn.argtypes = [C.c_void_p, C.POINTER(ReadSetC), C.POINTER(ReadExtrasC), C.POINTER(PhasedVariantsC), C.c_void_p, C.c_int64, C.c_void_p,
                       C.c_int64, C.c_int64, C.POINTER(FaConfig), C.POINTER(HaplotagConfig)]
    for fn in (L.c3_fa_reads_dwell, L.c3_fa_reads_dwell_host):
        fn.argtypes = [C.c_void_p, C.POINTER(ReadSetC), C.POINTER(ReadExtrasC), C.POINTER(ReadMovesC), C.POINTER(PhasedVariantsC), C.c_void_p,
                       C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(FaConfig), C.POINTER(HaplotagConfig)]
    L.c3_fa_reads_channels.argtypes = [C.c_void_p]
    L.c3_fa_dwell_cum_host.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    L.c3_fa_dwell_table.restype = C.c_int64
    L.c3_fa_dwell_table.argtypes = [C.c_void_p, C.c_void_p]
    L.c3_outcome_maxima.argtypes =[C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.c3_decode_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.c3_model_synchronize.argtypes = [C.c_void_p]
    L.c3_model_destroy.argtypes = [C.c_void_p]
    L.c3_debug_fetch.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]
    L.c3_debug_keep_activations.argtypes = [C.c_void_p, C.c_int]
    L.c3_debug_tap.argtypes = [C.c_void_p, C.c_char_p]
    L.c3_debug_tap_fetch.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    L.c3_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.c3_profile_reset.argtypes = [C.c_void_p]
    L.c3_profile_read.argtypes = [C.c_void_p, C.POINTER(KernelStat), C.c_int]
    for name in EXPORTS:
        getattr(L, name)  # AttributeError here = the .so is older than the header
    _lib = L
    return L


def last_error():
    return lib().c3_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise C3Error(f"{what}: {last_error()}")


def device_count():
    n = lib().c3_device_count()
    if n < 0:
        raise C3Error(f"c3_device_count: {last_error()}")
    return n


def pci_bus_id(device=0):
    """PCI address of a visible device as sysfs spells it (c3_device_pci_bus_id)."""
    buf = C.create_string_buffer(32)
    check(lib().c3_device_pci_bus_id(int(device), buf, 32), "c3_device_pci_bus_id")
    return buf.value.decode()


def mem_info(device=0):
    """(free_bytes, total_bytes) of a device -- the ROCm replacement for the reference's nvidia-smi probe
    (clair3/CallVariantsFromCffiGPU.py:13-19)."""
    f, t = C.c_size_t(0), C.c_size_t(0)
    check(lib().c3_mem_info(device, C.byref(f), C.byref(t)), "c3_mem_info")
    return f.value, t.value
