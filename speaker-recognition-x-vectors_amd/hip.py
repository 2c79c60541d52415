"""ctypes binding of libxvec_hip.so (C ABI: include/xvec_hip.h).

The library is the product; there is no CPU or eager-PyTorch fallback.  If the shared
object has not been built (python -c "import __graft_entry__ as g; g.build()") or cannot
be loaded, importing this module raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os

# torch first: it ships its own HIP runtime, and libxvec_hip.so must bind to THAT copy.  Loading the
# library before torch pulls in the system's libamdhip64 as a second runtime in the process, and the
# later one reports "no ROCm-capable device" (seen with build() followed by smoke() in one process).
import torch  # noqa: F401

from ._device import checker as _checker

_HERE = os.path.dirname(os.path.abspath(__file__))
# XVEC_LIB: development override (A/B runs of two builds on one GPU box; diagnostic builds under build/).  It must
# be an absolute path and is announced on stderr, so a stray library can never be picked up silently; the
# default -- and the only thing that ships -- is the in-tree build.
_override = os.environ.get("XVEC_LIB")
if _override:
    import sys
    if not os.path.isabs(_override):
        raise ImportError(f"XVEC_LIB={_override!r} must be an absolute path (unset it to load the in-tree library)")
    print(f"[xvector_amd] XVEC_LIB override: loading {_override}", file=sys.stderr)
LIB_PATH = _override or os.path.join(_HERE, "libxvec_hip.so")

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_WORKSPACE, ERR_TOO_LARGE = 0, 1, 2, 3, 4, 5
F32, BF16, BF16X3 = 0, 1, 2
PLDA_X_F32, PLDA_X_F64 = 0, 1                                   # XVEC_PLDA_X_*
LDA_X_F32, LDA_X_F64 = 0, 1                                     # XVEC_LDA_X_*
IDENT_X_F32, IDENT_X_F64 = 0, 1                                 # XVEC_IDENT_X_*
EMBED_MAX_DIM, EMBED_ROW_GROUP = 65536, 64                      # XVEC_EMBED_*
AUG_POOL_F32, AUG_POOL_I16 = 0, 1                               # XVEC_AUG_POOL_*
TSNE_X_F32, TSNE_X_F64 = 0, 1                                   # XVEC_TSNE_X_*
GMM_X_F32, GMM_X_F64 = 0, 1                                     # XVEC_GMM_X_*
MODE_LOGITS, MODE_POOLED, MODE_XVEC6, MODE_XVEC7 = 0, 5, 6, 7
SEG6, SEG7, OUTPUT = 6, 7, 8
KERNEL_NAMES = {0: None, 1: "tile128", 2: "pp", 3: "first"}      # XVEC_KERNEL_*
FORM_NAMES = {0: "direct", 1: "winograd_f23", 2: "bf16_split3"}     # XVEC_FORM_*
OPERAND_NAMES = {0: "fp32", 1: "bf16", 2: "bf16x3", 3: "bf16_split3"}     # XVEC_OPERANDS_*
AFFINE_FORM_NAMES = {0: None, 1: "tile16", 2: "tile16_elementwise", 3: "splitk", 4: "splitk_bf16x3", 5: "direct",
                     6: "direct_bf16x3"}                                     # XVEC_AFFINE_*
TIMING_NAMES = ("tdnn1", "tdnn2", "tdnn3", "tdnn4", "tdnn5_pool", "pool_finalize",
                "segment6", "segment7", "output", "pack")


class XvecError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"xvec_hip error {code}: {msg}")
        self.code = code


class MfccCfg(C.Structure):
    _fields_ = [("samplerate", C.c_int32), ("winlen", C.c_float), ("winstep", C.c_float), ("numcep", C.c_int32),
                ("nfilt", C.c_int32), ("nfft", C.c_int32), ("lowfreq", C.c_float), ("highfreq", C.c_float),
                ("preemph", C.c_float), ("ceplifter", C.c_int32), ("append_energy", C.c_int32),
                ("device", C.c_int32)]


class WsLayout(C.Structure):
    _fields_ = [("act_a", C.c_size_t), ("act_b", C.c_size_t), ("part", C.c_size_t), ("part_cnt", C.c_size_t),
                ("pooled", C.c_size_t), ("bytes", C.c_size_t), ("rows_alloc", C.c_int64), ("part_slots", C.c_int64),
                ("pool_n_pad", C.c_int32), ("hidden_n_pad", C.c_int32), ("num_cu", C.c_int32)]


class Cfg(C.Structure):
    _fields_ = [("input_size", C.c_int32), ("hidden_size", C.c_int32), ("num_classes", C.c_int32),
                ("x_vector_size", C.c_int32), ("batch_norm", C.c_int32), ("device", C.c_int32)]


class VadOptions(C.Structure):                                  # xvec_vad_options
    _fields_ = [("energy_threshold", C.c_double), ("energy_mean_scale", C.c_double), ("proportion_threshold", C.c_double),
                ("frames_context", C.c_int32), ("energy_col", C.c_int32)]


class VbxOptions(C.Structure):                                  # xvec_vbx_options
    _fields_ = [("loop_prob", C.c_double), ("Fa", C.c_double), ("Fb", C.c_double), ("epsilon", C.c_double),
                ("max_iter", C.c_int32), ("reserved", C.c_int32)]


class CmvnOptions(C.Structure):                                 # xvec_cmvn_options
    _fields_ = [("cmn_window", C.c_int32), ("min_window", C.c_int32), ("center", C.c_int32), ("norm_vars", C.c_int32)]


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build the HIP library first "
        "(python -c 'import __graft_entry__ as g; g.build()' or make -C "
        f"{os.path.join(_HERE, 'csrc')}). There is no CPU fallback.")

lib = C.CDLL(LIB_PATH)

_vp, _i32, _i64, _f32p = C.c_void_p, C.c_int32, C.c_int64, C.c_void_p


class _wsb(C.c_size_t):
    """size_t workspace_bytes of include/xvec_calib.h: C.c_size_t under a name of its own.  tests/test_workspace_refusals.py lists
    every (void*, C.c_size_t) pair of the table below against answers recorded once; the calibration unit's answers are held by
    tests/test_calibrate.py instead."""


class _wsb_report(_wsb):
    """size_t workspace_bytes of include/xvec_report.h: `_wsb` again, under one more name.  tests/test_calibrate.py lists every
    (void*, _wsb) pair of the table below as the calibration unit's own; the report unit's answers are held by
    tests/test_report.py."""


class _wsb_vbx(_wsb_report):
    """size_t workspace_bytes of include/xvec_vbx.h: one more name.  tests/test_report.py lists every (void*, _wsb_report) pair
    of the table below as the report unit's own; the VBx unit's answers are held by tests/test_vbx.py."""


class _wsb_der(_wsb_vbx):
    """size_t workspace_bytes of include/xvec_der.h: one more name.  tests/test_vbx.py lists every (void*, _wsb_vbx) pair of the
    table below as the VBx unit's own; the DER unit's answers are held by tests/test_der.py."""


class _wsb_fuse(_wsb_der):
    """size_t workspace_bytes of include/xvec_fuse.h: one more name.  tests/test_der.py lists every (void*, _wsb_der) pair of the
    table below as the DER unit's own; the fusion unit's answers are held by tests/test_fuse.py."""


class _wsb_boot(_wsb_fuse):
    """size_t workspace_bytes of include/xvec_boot.h and of xvec_eval_sorted_order (include/xvec_eval.h), whose sort the bootstrap
    unit compiles: one more name.  tests/test_fuse.py lists every (void*, _wsb_fuse) pair of the table below as the fusion unit's
    own; the answers of these are held by tests/test_bootstrap.py."""


class _wsb_analyze(_wsb_boot):
    """size_t workspace_bytes of include/xvec_analyze.h: one more name.  tests/test_bootstrap.py lists every (void*, _wsb_boot)
    pair of the table below as the bootstrap unit's own; the analysis unit's answers are held by tests/test_analyze.py."""


class _wsb_gmm(_wsb_analyze):
    """size_t workspace_bytes of include/xvec_gmm.h: one more name.  tests/test_analyze.py lists every (void*, _wsb_analyze)
    pair of the table below as the analysis unit's own; the GMM unit's answers are held by tests/test_gmm.py."""


class GmmFrames(C.Structure):                                   # xvec_gmm_frames (utt_first / utt_count are HOST arrays)
    _fields_ = [("x", C.c_void_p), ("x_type", C.c_int32), ("reserved", C.c_int32), ("rows", C.c_int64), ("ldx", C.c_int64),
                ("utt_first", C.POINTER(C.c_int64)), ("utt_count", C.POINTER(C.c_int64)), ("n_utts", C.c_int64)]


class GmmMstepOptions(C.Structure):                             # xvec_gmm_mstep_options
    _fields_ = [("reg_covar", C.c_double), ("var_floor", C.c_double), ("min_count", C.c_double)]


class AnalyzeBins(C.Structure):                                 # xvec_analyze_bins
    _fields_ = [("width", C.c_double), ("first", C.c_int64), ("n_bins", C.c_int32), ("rounding", C.c_int32),
                ("hist_copies", C.c_int32), ("reserved", C.c_int32)]


class AnalyzeSelect(C.Structure):                               # xvec_analyze_select
    _fields_ = [("k", C.c_int32), ("cand_cap", C.c_int32)]


class BootParams(C.Structure):                                  # xvec_boot_params
    _fields_ = [("row_group", C.c_void_p), ("col_group", C.c_void_p), ("n_row_groups", C.c_int32), ("n_col_groups", C.c_int32),
                ("joint", C.c_int32), ("n_boot", C.c_int32), ("seed", C.c_uint64), ("c_miss", C.c_double), ("c_fa", C.c_double),
                ("p_target", C.c_double)]


_SIGS = {
    "xvec_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(_vp)]),
    "xvec_destroy": (None, [_vp]),
    "xvec_last_error": (C.c_char_p, []),
    "xvec_version": (C.c_char_p, []),
    "xvec_load_tdnn": (C.c_int, [_vp, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, _vp]),
    "xvec_load_affine": (C.c_int, [_vp, C.c_int, _f32p, _f32p, _vp]),
    "xvec_workspace_bytes": (C.c_size_t, [_vp, _i64, _i32]),
    "xvec_workspace_layout": (C.c_int, [_vp, _i64, _i32, C.POINTER(WsLayout)]),
    "xvec_forward": (C.c_int, [_vp, _f32p, C.POINTER(_i32), _i32, _i32, C.c_int, C.c_int, _f32p, _vp,
                               C.c_size_t, _vp]),
    "xvec_forward_packed": (C.c_int, [_vp, _f32p, C.POINTER(_i64), _i32, C.c_int, C.c_int, _f32p, _vp,
                                      C.c_size_t, _vp]),
    "xvec_segments_workspace_bytes": (C.c_size_t, [_vp, _i64, _i32, _i64]),
    "xvec_forward_segments": (C.c_int, [_vp, _f32p, C.POINTER(_i64), _i32, _vp, _vp, _vp, _i64, C.c_int, C.c_int, _f32p, _vp,
                                        C.c_size_t, _vp]),
    "xvec_stat_pool_segments": (C.c_int, [_vp, C.c_int, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _f32p, _vp]),
    "xvec_stat_pool_segments_vector": (C.c_int, [_vp, C.c_int, _i32, _i32]),
    "xvec_tdnn_layer": (C.c_int, [_vp, C.c_int, _f32p, _i32, _i32, C.c_int, _f32p, _vp, C.c_size_t, _vp]),
    "xvec_tdnn_pool_layer": (C.c_int, [_vp, _f32p, _i32, _i32, C.c_int, _f32p, _vp, C.c_size_t, _vp]),
    "xvec_stat_pool": (C.c_int, [_f32p, _vp, _i32, _i32, _i32, _f32p, _vp]),
    "xvec_affine": (C.c_int, [_vp, C.c_int, _f32p, _i32, C.c_int, _f32p, _vp]),
    "xvec_segment_layer": (C.c_int, [_vp, C.c_int, _f32p, _i32, C.c_int, C.c_int, _f32p, _vp, C.c_size_t, _vp]),
    "xvec_set_profiling": (C.c_int, [_vp, C.c_int]),
    "xvec_get_timings": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "xvec_get_dispatch": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xvec_get_tdnn_launch": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xvec_get_tdnn_form": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xvec_get_tdnn_operands": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xvec_get_affine_dispatch": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xvec_mfcc_create": (C.c_int, [C.POINTER(MfccCfg), C.POINTER(_vp)]),
    "xvec_mfcc_destroy": (None, [_vp]),
    "xvec_mfcc_last_error": (C.c_char_p, []),
    "xvec_mfcc_frames": (C.c_int32, [_vp, _i64]),
    "xvec_mfcc_kernel_form": (C.c_int32, [_vp]),
    "xvec_mfcc": (C.c_int, [_vp, _f32p, _i32, _i64, _f32p, _vp]),
    "xvec_mfcc_i16": (C.c_int, [_vp, _vp, C.c_float, _i32, _i64, _f32p, _vp]),
    # include/xvec_score.h
    "xvec_score_last_error": (C.c_char_p, []),
    "xvec_gemm_nt_f64": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, C.c_double, C.c_double, _vp,
                                   _i64, _vp]),
    "xvec_score_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32]),
    "xvec_plda_score": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp,
                                  C.c_size_t, _vp]),
    "xvec_plda_score_lowrank": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, C.c_double, C.c_double, _vp,
                                          _vp, C.c_size_t, _vp]),
    "xvec_cosine_score": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, C.c_size_t, _vp]),
    # include/xvec_plda.h
    "xvec_plda_last_error": (C.c_char_p, []),
    "xvec_plda_stats_workspace_bytes": (C.c_size_t, [_i64, _i32, _i32]),
    "xvec_plda_stats": (C.c_int, [_vp, _i32, _i64, _i32, _vp, C.POINTER(_i64), _i32, C.c_double, _vp, _vp, _vp, _vp,
                                  _vp, _vp, C.c_size_t, _vp]),
    "xvec_plda_em_workspace_bytes": (C.c_size_t, [_i32, _i32]),
    "xvec_plda_em_products": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, C.c_size_t, _vp]),
    # include/xvec_eval.h
    "xvec_eval_last_error": (C.c_char_p, []),
    "xvec_eval_workspace_bytes": (C.c_size_t, [_i64]),
    "xvec_eval_trials": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                   C.c_size_t, _vp]),
    "xvec_eval_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                      C.c_size_t, _vp]),
    "xvec_eval_sorted_keys": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_eval_sorted_order_workspace_bytes": (C.c_size_t, [_i64]),
    "xvec_eval_sorted_order": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _wsb_boot, _vp]),
    "xvec_eval_sorted_order_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _wsb_boot, _vp]),
    # include/xvec_boot.h  (the workspace size is spelt _wsb_boot: see the class above; `params` is a HOST xvec_boot_params)
    "xvec_boot_last_error": (C.c_char_p, []),
    "xvec_boot_workspace_bytes": (C.c_size_t, [_i64, _i32, _i32, _i32]),
    "xvec_boot_batch": (C.c_int32, [_i64, _i32]),
    "xvec_boot_batches": (C.c_int32, [_i64, _i32]),
    "xvec_boot_trials": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.POINTER(BootParams), _vp, _vp, _vp, _wsb_boot, _vp]),
    "xvec_boot_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, C.POINTER(BootParams), _vp, _vp, _vp, _wsb_boot, _vp]),
    "xvec_boot_counts_host": (C.c_int, [C.c_uint64, _i32, _i32, _i32, C.POINTER(C.c_uint16)]),
    "xvec_boot_poisson_host": (C.c_int, [C.c_uint64, _i32, _i64, C.POINTER(C.c_int32)]),
    # include/xvec_analyze.h  (`bins` and `select` are HOST structs; bins may be null)
    "xvec_analyze_last_error": (C.c_char_p, []),
    "xvec_analyze_plan_host": (C.c_int, [_i64, _i32, C.POINTER(C.c_int64)]),
    "xvec_analyze_summary_workspace_bytes": (C.c_size_t, [_i64, _i32]),
    "xvec_analyze_hardest_workspace_bytes": (C.c_size_t, [_i64, _i32, _i32]),
    "xvec_analyze_summary": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.POINTER(AnalyzeBins), _vp, _vp, _vp,
                                       _wsb_analyze, _vp]),
    "xvec_analyze_summary_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, _i32, C.POINTER(AnalyzeBins), _vp, _vp, _vp,
                                                 _wsb_analyze, _vp]),
    "xvec_analyze_hardest": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.POINTER(AnalyzeSelect), _vp, _vp, _vp, _vp,
                                       _wsb_analyze, _vp]),
    "xvec_analyze_hardest_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, _i32, C.POINTER(AnalyzeSelect), _vp, _vp, _vp,
                                                 _vp, _wsb_analyze, _vp]),
    # include/xvec_gmm.h  (`frames` and `options` are HOST structs)
    "xvec_gmm_last_error": (C.c_char_p, []),
    "xvec_gmm_plan_host": (C.c_int, [_i64, _i64, _i32, _i32, _i32, _i32, C.POINTER(C.c_int64)]),
    "xvec_gmm_loglik_workspace_bytes": (C.c_size_t, [_i64, _i32, _i32]),
    "xvec_gmm_accumulate_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "xvec_gmm_em_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32, _i32, _i32]),
    "xvec_gmm_linear_scores_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32, _i32]),
    "xvec_gmm_prepare": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "xvec_gmm_loglik": (C.c_int, [C.POINTER(GmmFrames), _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _wsb_gmm, _vp]),
    "xvec_gmm_accumulate": (C.c_int, [C.POINTER(GmmFrames), _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _wsb_gmm, _vp]),
    "xvec_gmm_mstep": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(GmmMstepOptions), _vp, _vp, _vp, _vp]),
    "xvec_gmm_em": (C.c_int, [C.POINTER(GmmFrames), _i32, _i32, _i32, C.c_double, C.POINTER(GmmMstepOptions), _i32, _vp, _vp, _vp,
                              _vp, _vp, _vp, _vp, _wsb_gmm, _vp]),
    "xvec_gmm_map_means": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, C.c_double, _vp, _vp]),
    "xvec_gmm_linear_scores": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _wsb_gmm, _vp]),
    # include/xvec_snorm.h
    "xvec_snorm_last_error": (C.c_char_p, []),
    "xvec_snorm_workspace_bytes": (C.c_size_t, [_i64, _i64]),
    "xvec_snorm_row_stats": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_snorm_apply": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    # include/xvec_ident.h
    "xvec_ident_last_error": (C.c_char_p, []),
    "xvec_model_mean_workspace_bytes": (C.c_size_t, [_i32]),
    "xvec_model_mean": (C.c_int, [_vp, _i32, _i64, _i32, _i64, _vp, C.POINTER(_i64), _i32, _vp, _vp, C.c_size_t, _vp]),
    "xvec_ident_workspace_bytes": (C.c_size_t, [_i64, _i64, _i32]),
    "xvec_open_set_scores": (C.c_int, [_vp, _i64, _i64, _i64, C.c_double, _vp, _i64, _vp, C.c_size_t, _vp]),
    "xvec_identify_topk": (C.c_int, [_vp, _i64, _i64, _i64, _i32, C.c_double, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    # include/xvec_diar.h
    "xvec_diar_last_error": (C.c_char_p, []),
    "xvec_ahc_workspace_bytes": (C.c_size_t, [C.POINTER(_i64), _i32]),
    "xvec_ahc_cluster": (C.c_int, [_vp, _i64, C.POINTER(_i64), _i32, C.c_double, _i32, C.POINTER(_i32), _vp, _vp, _vp, _vp, _vp,
                                   _vp, C.c_size_t, _vp]),
    # include/xvec_lda.h
    "xvec_lda_last_error": (C.c_char_p, []),
    "xvec_lda_stats_workspace_bytes": (C.c_size_t, [_i64, _i32, _i32]),
    "xvec_lda_stats": (C.c_int, [_vp, _i32, _i64, _i32, _vp, C.POINTER(_i64), _i32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_embed_transform_workspace_bytes": (C.c_size_t, [_i64, _i32, _i32]),
    "xvec_embed_transform": (C.c_int, [_vp, _i32, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _i64, _vp, C.c_size_t, _vp]),
    # include/xvec_augment.h
    "xvec_aug_last_error": (C.c_char_p, []),
    "xvec_aug_mix_workspace_bytes": (C.c_size_t, [_i32, _i64, _i64]),
    "xvec_aug_mix": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i32, _i32, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                               C.c_size_t, _vp]),
    "xvec_aug_reverb_workspace_bytes": (C.c_size_t, [_i32, _i64, _i64]),
    "xvec_aug_reverb": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i32, _i64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_aug_normalize": (C.c_int, [_vp, _i64, _i32, _i64, _vp]),
    # include/xvec_resample.h
    "xvec_resample_last_error": (C.c_char_p, []),
    "xvec_resample_out_len": (_i64, [_i64, C.c_double]),
    "xvec_resample_tile_span": (_i64, [C.c_double, _i64, _i32]),
    "xvec_resample_workspace_bytes": (C.c_size_t, [_i32, _i32]),
    "xvec_resample": (C.c_int, [_vp, _i32, _i64, _i32, _i64, _vp, _i32, C.POINTER(C.c_double), _i32, _vp, _i64, _i32, _i32, _vp,
                                _i32, _i64, _i64, _vp, _vp, C.c_size_t, _vp]),
    # include/xvec_vad.h
    "xvec_vad_last_error": (C.c_char_p, []),
    "xvec_vad_workspace_bytes": (C.c_size_t, [_i32, _i32]),
    "xvec_vad_energy": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, C.POINTER(VadOptions), _vp, _i64, _vp, _vp, _vp]),
    "xvec_cmvn_sliding": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, C.POINTER(CmvnOptions), _vp, _i64, _vp, _i64, _i64,
                                    _vp, _vp, C.c_size_t, _vp]),
    "xvec_vad_cmvn": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, C.POINTER(VadOptions), C.POINTER(CmvnOptions), _i32, _vp,
                                _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, C.c_size_t, _vp]),
    # include/xvec_tsne.h
    "xvec_tsne_last_error": (C.c_char_p, []),
    "xvec_tsne_workspace_bytes": (C.c_size_t, [_i32, _i32]),
    "xvec_tsne_plan": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "xvec_tsne_sqdist": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i32, _vp, _i64, _vp, C.c_size_t, _vp]),
    "xvec_tsne_affinities": (C.c_int, [_vp, _i64, _i32, C.c_double, _vp, _i64, _vp, _vp, C.c_size_t, _vp]),
    "xvec_tsne_steps": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _i32, C.c_double, C.c_double, C.c_double,
                                  C.c_double, _vp, _vp, _vp, C.c_size_t, _vp]),
    # include/xvec_calib.h  (the workspace size is spelt _wsb, not C.c_size_t: see the class above)
    "xvec_calib_last_error": (C.c_char_p, []),
    "xvec_calib_workspace_bytes": (C.c_size_t, [_i64]),
    "xvec_calib_fit": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.c_double, _i32, _vp, _vp, _wsb, _vp]),
    "xvec_calib_fit_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, C.c_double, _i32, _vp, _vp, _wsb, _vp]),
    "xvec_calib_apply": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]),
    "xvec_calib_cllr": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                  _wsb, _vp]),
    "xvec_calib_cllr_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                            _wsb, _vp]),
    "xvec_calib_min_cllr": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _wsb,
                                      _vp]),
    # include/xvec_fuse.h  (the workspace size is spelt _wsb_fuse: see the class above; `terms` is a HOST array of xvec_fuse_term)
    "xvec_fuse_last_error": (C.c_char_p, []),
    "xvec_fuse_workspace_bytes": (C.c_size_t, [_i64, _i32]),
    "xvec_fuse_fit": (C.c_int, [_vp, _i32, _i64, _i64, _vp, _vp, _vp, _i64, C.c_double, C.c_double, _i32, _vp, _vp, _wsb_fuse, _vp]),
    "xvec_fuse_fit_all_pairs": (C.c_int, [_vp, _i32, _i64, _i64, _vp, _vp, _i32, C.c_double, C.c_double, _i32, _vp, _vp, _wsb_fuse,
                                          _vp]),
    "xvec_fuse_apply": (C.c_int, [_vp, _i32, _i64, _i64, _vp, _vp, _i64, _vp]),
    # include/xvec_report.h  (the workspace size is spelt _wsb_report: see the class above)
    "xvec_report_last_error": (C.c_char_p, []),
    "xvec_report_trial_map": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "xvec_report_range_workspace_bytes": (C.c_size_t, []),
    "xvec_report_range": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _wsb_report, _vp]),
    "xvec_report_images": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, C.c_double, C.c_double, C.c_uint32, _i32, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp]),
    "xvec_report_det_workspace_bytes": (C.c_size_t, [_i64]),
    "xvec_report_det": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _wsb_report,
                                  _vp]),
    "xvec_report_det_all_pairs": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _i64, _vp,
                                            _wsb_report, _vp]),
    # include/xvec_vbx.h  (the workspace size is spelt _wsb_vbx: see the class above)
    "xvec_vbx_last_error": (C.c_char_p, []),
    "xvec_vbx_workspace_bytes": (C.c_size_t, [C.POINTER(_i64), _i32, _i32, _i32]),
    "xvec_vbx_init": (C.c_int, [_vp, C.POINTER(_i64), _i32, _i32, C.c_double, _vp, _i64, _vp, _vp]),
    "xvec_vbx_run": (C.c_int, [_vp, _i64, _i32, _vp, C.POINTER(_i64), _i32, _i32, C.POINTER(VbxOptions), _vp, _i64, _vp, _vp, _vp,
                               _vp, _vp, _vp, _wsb_vbx, _vp]),
    # include/xvec_der.h  (the workspace size is spelt _wsb_der: see the class above)
    "xvec_der_last_error": (C.c_char_p, []),
    "xvec_der_workspace_bytes": (C.c_size_t, [C.POINTER(_i64), _i32, _i64, _i64]),
    "xvec_der_cooccurrence": (C.c_int, [_vp, _i64, _vp, _i64, C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _wsb_der, _vp]),
    "xvec_der_assign": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "xvec_der_score": (C.c_int, [_vp, _i64, _vp, _i64, C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _wsb_der,
                                 _vp]),
    # include/xvec_train.h
    "xvec_train_last_error": (C.c_char_p, []),
    "xvec_tdnn_train_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, C.POINTER(_i32), _i32]),
    "xvec_tdnn_train_forward": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp, C.c_float,
                                          _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_tdnn_train_backward": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp,
                                           C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_train_tail_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "xvec_train_tail_forward": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_train_tail_backward": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xvec_tdnn_train_forward_ragged": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp,
                                                 C.c_float, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "xvec_tdnn_train_backward_ragged": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp,
                                                  _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "xvec_train_tail_forward_ragged": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                                 _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "xvec_train_tail_backward_ragged": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "xvec_tdnn_train_forward_dropout": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp,
                                                  C.c_float, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_float,
                                                  C.c_uint64, C.c_uint64]),
    "xvec_tdnn_train_backward_dropout": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp,
                                                   _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                                                   C.c_float]),
    "xvec_dropout_keep_host": (C.c_int, [_vp, _i64, _i32, C.c_float, C.c_uint64, C.c_uint64]),
    "xvec_adam_step": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i64), _i32,
                                 C.c_double, C.c_double, C.c_double, C.c_double, _i64, _vp]),
}
EXPORTS = tuple(_SIGS)
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)      # AttributeError here = header/library mismatch
    _fn.restype = _res
    _fn.argtypes = _args


def last_error() -> str:
    return lib.xvec_last_error().decode()


check = _checker(lib.xvec_last_error)


def version() -> str:
    return lib.xvec_version().decode()


def affine_dispatch(handle) -> list:
    """[(form name, K ranges)] of the last launch of segment_layer6 / segment_layer7 / output on `handle`
    (xvec_get_affine_dispatch; test introspection, nothing in the product calls it)."""
    forms, ranges, n = (C.c_int * 3)(), (C.c_int * 3)(), C.c_int(0)
    check(lib.xvec_get_affine_dispatch(handle, forms, ranges, C.byref(n)))
    return [(AFFINE_FORM_NAMES[int(forms[i])], int(ranges[i])) for i in range(n.value)]
