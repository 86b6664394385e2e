"""MI355X-native ML-GGD DNN trainer: Python host-side binding of the C-ABI (include/mlggd.h).

`BPGpu` mirrors the reference's device-engine class `BP_GPU`
(Train_code_ML_GGD/BP_GPU.h:45-70: train / CrossValid / CrossValiddB / CrossValid2 /
returnWeights) over libmlggd.so.  There is NO CPU fallback: if the HIP library is missing
or no GPU is present, construction raises.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_CSRC, "libmlggd.so")
MAXLAYER = 10
UNIQUE_ID_BYTES = 128

_fp = C.POINTER(C.c_float)
_fpp = C.POINTER(_fp)


class MlggdError(RuntimeError):
    pass


class _ConfigSlots(C.Union):
    """the five reserved slots of mlggd_config, and the names of those that have taken a meaning (include/mlggd.h)"""
    _fields_ = [("mask_bins", C.c_int32), ("reserved", C.c_int32 * 5)]  # mask_bins = reserved[0]


class _Config(C.Structure):
    _anonymous_ = ("_slots",)
    _fields_ = [
        ("struct_size", C.c_int32), ("random_seed", C.c_int32), ("device", C.c_int32),
        ("numlayers", C.c_int32), ("layersizes", C.c_int32 * MAXLAYER), ("bunchsize", C.c_int32),
        ("lrate", C.c_float), ("momentum", C.c_float), ("weightcost", C.c_float),
        ("shapefactor", C.c_float), ("MLflag", C.c_int32), ("dropoutflag", C.c_int32),
        ("visible_omit", C.c_float), ("hid_omit", C.c_float), ("max_cache_frames", C.c_int32),
        ("activation", C.c_int32), ("nat_frames", C.c_int32), ("_slots", _ConfigSlots),
    ]


ACTIVATIONS = ("sigmoid", "relu")  # MLGGD_ACT_SIGMOID = 0, MLGGD_ACT_RELU = 1 (include/mlggd.h)


def activation_code(activation):
    """"sigmoid" | "relu" | 0 | 1 -> the MLGGD_ACT_* value of mlggd_config.activation; anything else is a ValueError."""
    if isinstance(activation, str) and activation in ACTIVATIONS:
        return ACTIVATIONS.index(activation)
    if isinstance(activation, (int, np.integer)) and not isinstance(activation, bool) and 0 <= activation < len(ACTIVATIONS):
        return int(activation)
    raise ValueError("activation %r: must be one of %s or 0 / 1" % (activation, " / ".join(map(repr, ACTIVATIONS))))


# every symbol include/mlggd.h declares (tests check the library exports all of them)
EXPORTS = [
    "mlggd_create", "mlggd_destroy", "mlggd_last_error", "mlggd_device_count", "mlggd_train_chunk",
    "mlggd_load_chunk", "mlggd_train_resident", "mlggd_sync", "mlggd_cv_sqerr", "mlggd_cv_abserr",
    "mlggd_cv_loglik", "mlggd_cv_all", "mlggd_forward", "mlggd_get_weights", "mlggd_set_weights",
    "mlggd_get_scalefactor", "mlggd_set_scalefactor", "mlggd_set_lrate", "mlggd_gamma",
    "mlggd_get_activation",
    "mlggd_debug_tensor", "mlggd_comm_unique_id", "mlggd_comm_init", "mlggd_last_train_ms",
    "mlggd_profile_select", "mlggd_profile_stride", "mlggd_profile_read", "mlggd_profile_overhead",
    "mlggd_kernel_work", "mlggd_dw_launches_per_step", "mlggd_dp_mode", "mlggd_debug_fake_world",
    "mlggd_debug_stamp_select", "mlggd_debug_stamp_read",
    "mlggd_load_frames", "mlggd_train_frames", "mlggd_train_frames_async", "mlggd_cv_all_frames", "mlggd_forward_frames",
    "mlggd_alloc_pinned", "mlggd_alloc_pinned_on", "mlggd_free_pinned", "mlggd_set_cv_device_reduce",
    "mlggd_comm_info", "mlggd_debug_plan_count", "mlggd_debug_buffers", "mlggd_debug_math", "mlggd_debug_out_slabs", "mlggd_debug_gemm_plan",
    "mlggd_debug_keep_ranks", "mlggd_debug_rank_tensor",
    "mlggd_wave_to_lps", "mlggd_lps_to_wave", "mlggd_enhance_wave",
    "mlggd_enhance_waves_layout", "mlggd_enhance_waves",
    "mlggd_score_waves", "mlggd_enhance_waves_scored",
    "mlggd_stoi_layout", "mlggd_stoi_waves", "mlggd_enhance_waves_scored_stoi",
    "mlggd_live_layout", "mlggd_live_open", "mlggd_live_push", "mlggd_live_received", "mlggd_live_close",
    "mlggd_error_stats", "mlggd_error_stats_frames", "mlggd_ggd_fit",
    "mlggd_set_shapefactors", "mlggd_get_shapefactors", "mlggd_read_shapefactors",
    "mlggd_output_stats", "mlggd_output_stats_frames", "mlggd_gv_fit", "mlggd_set_gv", "mlggd_get_gv", "mlggd_read_gv",
    "mlggd_wave_samples", "mlggd_mix_waves", "mlggd_lps_stats", "mlggd_norm_from_stats",
    "mlggd_load_waves", "mlggd_cv_all_waves", "mlggd_set_noise", "mlggd_train_waves",
    "mlggd_load_frames_nat", "mlggd_train_frames_nat", "mlggd_cv_all_frames_nat", "mlggd_forward_frames_nat",
    "mlggd_nat_estimate", "mlggd_nat_rows", "mlggd_get_nat_frames",
    "mlggd_set_mask", "mlggd_get_mask", "mlggd_get_mask_bins", "mlggd_mask_targets", "mlggd_mask_select",
    "mlggd_set_asymmetry", "mlggd_get_asymmetry", "mlggd_error_stats_signed", "mlggd_error_stats_signed_frames",
    "mlggd_asym_fit", "mlggd_read_asymmetry",
    "mlggd_set_scale_mode", "mlggd_get_scale_mode", "mlggd_get_scale_state", "mlggd_set_scale_state",
    "mlggd_read_scale_state", "mlggd_write_scale_state",
    "mlggd_set_optimizer", "mlggd_get_optimizer", "mlggd_get_optimizer_state", "mlggd_set_optimizer_state", "mlggd_adam_apply",
    "mlggd_write_optimizer_state", "mlggd_read_optimizer_header", "mlggd_read_optimizer_state",
    "mlggd_rbm_open", "mlggd_rbm_set_rates", "mlggd_rbm_train_chunk", "mlggd_rbm_train_frames", "mlggd_rbm_visible_bias",
    "mlggd_rbm_debug_tensor", "mlggd_rbm_close", "mlggd_rbm_draws",
]
MAX_BETAS = 32

_lib = None


def build(force=False):
    """Compile libmlggd.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in ("engine.hip", "kernels.hip.h", "kernels64.hip.h", "spectral.hip.h", "score.hip.h", "live.hip.h",
                                             "live_rule.h", "stoi.hip.h", "stoi_rule.h", "colstats.hip.h", "gv_rule.h", "mask_rule.h", "mask.hip.h", "mix.hip.h",
                                             "mix_rule.h", "nat_rule.h", "rbm_rule.h", "rbm.hip.h", "asym_rule.h", "scale_rule.h", "adam_rule.h", "devbuf.h", "devbuf_rule.h")]
    srcs.append(os.path.join(_HERE, "..", "include", "mlggd.h"))
    srcs.append(os.path.join(_HERE, "host", "errmodel.h"))
    srcs.append(os.path.join(_HERE, "host", "gvfile.h"))
    srcs.append(os.path.join(_HERE, "host", "asymfile.h"))
    srcs.append(os.path.join(_HERE, "host", "scalefile.h"))
    srcs.append(os.path.join(_HERE, "host", "optfile.h"))
    srcs.append(os.path.join(_HERE, "host", "binfile.h"))
    stale = not os.path.exists(LIB_PATH) or any(
        os.path.getmtime(LIB_PATH) < os.path.getmtime(s) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _CSRC, "-s"])
    return LIB_PATH


def load():
    """Load libmlggd.so (never builds implicitly; raises if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MlggdError("HIP extension %s is missing: run __graft_entry__.build() "
                         "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.mlggd_last_error.restype = C.c_char_p
    L.mlggd_gamma.restype = C.c_float
    L.mlggd_gamma.argtypes = [C.c_float]
    L.mlggd_create.argtypes = [C.POINTER(_Config), _fpp, _fpp, C.POINTER(C.c_void_p)]
    L.mlggd_destroy.argtypes = [C.c_void_p]
    L.mlggd_device_count.argtypes = [C.POINTER(C.c_int)]
    L.mlggd_train_chunk.argtypes = [C.c_void_p, C.c_int, _fp, _fp, C.POINTER(C.c_int)]
    L.mlggd_load_chunk.argtypes = [C.c_void_p, C.c_int, _fp, _fp]
    L.mlggd_train_resident.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mlggd_sync.argtypes = [C.c_void_p]
    for f in (L.mlggd_cv_sqerr, L.mlggd_cv_abserr, L.mlggd_cv_loglik):
        f.argtypes = [C.c_void_p, C.c_int, _fp, _fp, _fp]
    L.mlggd_cv_all.argtypes = [C.c_void_p, C.c_int, _fp, _fp, _fp, _fp, _fp]
    L.mlggd_forward.argtypes = [C.c_void_p, C.c_int, _fp, _fp]
    L.mlggd_get_weights.argtypes = [C.c_void_p, _fpp, _fpp]
    L.mlggd_set_weights.argtypes = [C.c_void_p, _fpp, _fpp]
    L.mlggd_get_scalefactor.argtypes = [C.c_void_p, _fp]
    L.mlggd_set_scalefactor.argtypes = [C.c_void_p, _fp]
    L.mlggd_set_lrate.argtypes = [C.c_void_p, C.c_float]
    L.mlggd_get_activation.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_set_cv_device_reduce.argtypes = [C.c_void_p, C.c_int]
    L.mlggd_alloc_pinned_on.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.mlggd_debug_tensor.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _fp, C.c_size_t]
    L.mlggd_comm_unique_id.argtypes = [C.c_void_p]
    L.mlggd_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.mlggd_last_train_ms.argtypes = [C.c_void_p, _fp, C.POINTER(C.c_int)]
    L.mlggd_profile_select.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L.mlggd_profile_stride.argtypes = [C.c_void_p, C.c_int]
    L.mlggd_profile_read.argtypes = [C.c_void_p, _fp, C.POINTER(C.c_int)]
    L.mlggd_profile_overhead.argtypes = [C.c_void_p, _fp]
    L.mlggd_kernel_work.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]
    L.mlggd_dw_launches_per_step.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_dp_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_debug_fake_world.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.mlggd_debug_keep_ranks.argtypes = [C.c_void_p, C.c_int]
    L.mlggd_debug_rank_tensor.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, _fp, C.c_size_t]
    L.mlggd_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mlggd_debug_plan_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_debug_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.mlggd_debug_out_slabs.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_debug_gemm_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mlggd_debug_math.argtypes = [C.c_void_p, C.c_char_p, _fp, C.c_float, _fp, C.c_size_t]
    L.mlggd_debug_stamp_select.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.mlggd_debug_stamp_read.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_int)]
    _ip = C.POINTER(C.c_int32)
    L.mlggd_load_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int]
    L.mlggd_train_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int, C.POINTER(C.c_int)]
    L.mlggd_train_frames_async.argtypes = L.mlggd_train_frames.argtypes
    L.mlggd_cv_all_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int, _fp, _fp, _fp]
    L.mlggd_forward_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, C.c_int, _ip, _fp]
    L.mlggd_alloc_pinned.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.mlggd_free_pinned.argtypes = [C.c_void_p]
    _sp = C.POINTER(C.c_int16)
    L.mlggd_wave_to_lps.argtypes = [C.c_int, C.c_int, C.c_int, _sp, C.POINTER(C.c_int), _fp]
    L.mlggd_lps_to_wave.argtypes = [C.c_int, C.c_int, C.c_int, _sp, C.c_int, _fp, _sp, _fp]
    L.mlggd_enhance_wave.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _sp, _sp, _fp, C.POINTER(C.c_int)]
    _lp = C.POINTER(C.c_int64)
    L.mlggd_enhance_waves_layout.argtypes = [C.c_int, C.c_int, _lp, C.POINTER(C.c_int32), _lp]
    L.mlggd_enhance_waves.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _sp, _lp, _sp, _fp, _fp]
    L.mlggd_score_waves.argtypes = [C.c_int, C.c_int, C.c_int, _sp, _sp, _lp, _fp, _ip, _fp, _fp]
    L.mlggd_enhance_waves_scored.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _sp, _sp, _lp, _ip, _sp,
                                             _fp, _fp, _fp, _fp]
    L.mlggd_stoi_layout.argtypes = [C.c_int, C.c_int64, _lp, _lp, _lp]
    L.mlggd_stoi_waves.argtypes = [C.c_int, C.c_int, C.c_int, _sp, _sp, _lp, _lp, _fp, _ip]
    L.mlggd_enhance_waves_scored_stoi.argtypes = L.mlggd_enhance_waves_scored.argtypes + [_lp, _fp, _ip]
    _bp = C.POINTER(C.c_uint8)
    L.mlggd_live_layout.argtypes = [C.c_int, C.c_int, C.c_int, _lp, _lp, _bp, _lp]
    L.mlggd_live_open.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, C.POINTER(C.c_void_p)]
    L.mlggd_live_push.argtypes = [C.c_void_p, _sp, _lp, _bp, _sp, _fp, C.c_int64, _lp]
    L.mlggd_live_received.argtypes = [C.c_void_p, _lp]
    L.mlggd_live_close.argtypes = [C.c_void_p]
    _dp = C.POINTER(C.c_double)
    L.mlggd_error_stats.argtypes = [C.c_void_p, C.c_int, _fp, _fp, C.c_int, _fp, _dp]
    L.mlggd_error_stats_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int, C.c_int, _fp, _dp]
    L.mlggd_ggd_fit.argtypes = [C.c_int, C.c_int64, C.c_int, _fp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _ip]
    L.mlggd_set_shapefactors.argtypes = [C.c_void_p, _fp]
    L.mlggd_get_shapefactors.argtypes = [C.c_void_p, _fp]
    L.mlggd_read_shapefactors.argtypes = [C.c_char_p, C.c_int, C.c_float, _fp]
    L.mlggd_set_asymmetry.argtypes = [C.c_void_p, _fp]
    L.mlggd_get_asymmetry.argtypes = [C.c_void_p, _fp]
    L.mlggd_error_stats_signed.argtypes = [C.c_void_p, C.c_int, _fp, _fp, C.c_int, _fp, _dp]
    L.mlggd_error_stats_signed_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int, C.c_int, _fp, _dp]
    L.mlggd_asym_fit.argtypes = [C.c_int, C.c_int64, C.c_int, _fp, _dp, _dp, _dp, _dp, _ip, _dp, _ip]
    L.mlggd_read_asymmetry.argtypes = [C.c_char_p, C.c_int, C.c_float, _fp]
    L.mlggd_set_scale_mode.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    L.mlggd_get_scale_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int), _fp, _fp, _fp, C.POINTER(C.c_int64)]
    L.mlggd_get_scale_state.argtypes = [C.c_void_p, _fp, _fp]
    L.mlggd_set_scale_state.argtypes = [C.c_void_p, _fp, _fp]
    L.mlggd_read_scale_state.argtypes = [C.c_char_p, C.c_int, _fp, _fp]
    L.mlggd_write_scale_state.argtypes = [C.c_char_p, C.c_int, _fp, _fp, C.c_float, C.c_float, C.c_float, C.c_int64]
    _i64p = C.POINTER(C.c_int64)
    L.mlggd_set_optimizer.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    L.mlggd_get_optimizer.argtypes = [C.c_void_p, C.POINTER(C.c_int), _fp, _fp, _fp, _i64p]
    L.mlggd_get_optimizer_state.argtypes = [C.c_void_p, _fpp, _fpp, _fpp, _fpp]
    L.mlggd_set_optimizer_state.argtypes = [C.c_void_p, _fpp, _fpp, _fpp, _fpp, C.c_int64]
    L.mlggd_adam_apply.argtypes = [_fp, _fp, _fp, _fp, C.c_int64] + [C.c_float] * 6 + [C.c_int64]
    L.mlggd_write_optimizer_state.argtypes = [C.c_char_p, C.c_int, _ip, _fpp, _fpp, _fpp, _fpp, C.c_float, C.c_float, C.c_float, C.c_int64]
    L.mlggd_read_optimizer_header.argtypes = [C.c_char_p, _ip, _ip, _fp, _fp, _fp, _i64p]
    L.mlggd_read_optimizer_state.argtypes = [C.c_char_p, C.c_int, _ip, _fpp, _fpp, _fpp, _fpp, _fp, _fp, _fp, _i64p]
    L.mlggd_output_stats.argtypes = [C.c_void_p, C.c_int, _fp, _fp, _dp]
    L.mlggd_output_stats_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _ip, C.c_int, _dp]
    L.mlggd_gv_fit.argtypes = [C.c_int, C.c_int64, _dp, _dp, _dp, _fp, _bp, _dp, _dp, _fp, _ip]
    L.mlggd_set_gv.argtypes = [C.c_void_p, _fp]
    L.mlggd_get_gv.argtypes = [C.c_void_p, _fp]
    L.mlggd_read_gv.argtypes = [C.c_char_p, C.c_int, C.c_int, _fp]
    L.mlggd_wave_samples.argtypes = [C.c_int, C.c_int, C.c_int, _lp, _ip, _lp]
    L.mlggd_mix_waves.argtypes = [C.c_int, C.c_int, _sp, _lp, _sp, C.c_int64, _lp, _lp, _lp, _dp, _sp, _dp, _ip]
    L.mlggd_lps_stats.argtypes = [C.c_int, C.c_int, C.c_int, _sp, _lp, _dp, _lp]
    L.mlggd_norm_from_stats.argtypes = [C.c_int, C.c_int64, _dp, _fp, _fp]
    L.mlggd_load_waves.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _sp, _sp, _lp, C.c_int, _ip, C.c_int]
    L.mlggd_cv_all_waves.argtypes = L.mlggd_load_waves.argtypes + [_fp, _fp, _fp]
    L.mlggd_set_noise.argtypes = [C.c_void_p, C.c_int64, _sp]
    L.mlggd_train_waves.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp, C.c_int, _sp, _lp, _lp, _lp, _lp, _dp, C.c_int,
                                    _ip, C.c_int, _sp, _dp, _ip, C.POINTER(C.c_int)]
    L.mlggd_load_frames_nat.argtypes = L.mlggd_load_frames.argtypes + [C.c_int, _fp, _ip]
    L.mlggd_train_frames_nat.argtypes = L.mlggd_load_frames_nat.argtypes + [C.POINTER(C.c_int)]
    L.mlggd_cv_all_frames_nat.argtypes = L.mlggd_load_frames_nat.argtypes + [_fp, _fp, _fp]
    L.mlggd_forward_frames_nat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, C.c_int, _ip, C.c_int, _fp, _ip, _fp]
    L.mlggd_nat_estimate.argtypes = [C.c_int, C.c_int, _ip, _fp, C.c_int, _fp]
    L.mlggd_nat_rows.argtypes = [C.c_int, _ip, C.c_int, _ip, _ip]
    L.mlggd_get_nat_frames.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_set_mask.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    L.mlggd_get_mask.argtypes = [C.c_void_p, C.POINTER(C.c_int), _fp, _fp, _fp]
    L.mlggd_get_mask_bins.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mlggd_mask_targets.argtypes = [C.c_int, C.c_int, C.c_int64, _fp, _fp, C.c_float, _fp]
    L.mlggd_mask_select.argtypes = [C.c_int, C.c_int64, _fp, _fp, _fp, C.c_float, C.c_float, _fp]
    L.mlggd_rbm_open.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_uint32, C.POINTER(C.c_void_p)]
    L.mlggd_rbm_set_rates.argtypes = [C.c_void_p, C.c_float, C.c_float]
    L.mlggd_rbm_train_chunk.argtypes = [C.c_void_p, C.c_int, _fp, C.POINTER(C.c_int), _dp]
    L.mlggd_rbm_train_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, C.c_int, _ip, C.POINTER(C.c_int), _dp]
    L.mlggd_rbm_visible_bias.argtypes = [C.c_void_p, _fp]
    L.mlggd_rbm_debug_tensor.argtypes = [C.c_void_p, C.c_char_p, _fp, C.c_size_t]
    L.mlggd_rbm_close.argtypes = [C.c_void_p]
    L.mlggd_rbm_draws.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, _fp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise MlggdError("mlggd error %d: %s" % (rc, load().mlggd_last_error().decode()))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
    return a


def _p(a):
    return a.ctypes.data_as(_fp)


def _ptr_array(arrs):
    """float*[numlayers] with slot 0 unused, like BP_GPU's float** arguments."""
    pa = (_fp * (len(arrs) + 1))()
    for i, a in enumerate(arrs):
        pa[i + 1] = _p(a)
    return pa


def device_count():
    n = C.c_int(0)
    _check(load().mlggd_device_count(C.byref(n)))
    return n.value


def gamma(x):
    return float(load().mlggd_gamma(float(x)))


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _frame_off(frame_off):
    fo = np.ascontiguousarray(frame_off, dtype=np.int32)
    if fo.ndim != 1 or fo.size < 1:
        raise ValueError("frame_off is a 1-D table of n_utts + 1 frame indices")
    return fo


def nat_estimate(rows, frame_off, nat_frames):
    """The noise rows [n_utts][D] float32 of noise-aware training (csrc/nat_rule.h, mlggd_nat_estimate): utterance u
    holds the NORMALISED rows rows[frame_off[u]:frame_off[u+1]]; its row is the mean of its first min(nat_frames, F_u)
    rows, added from left to right in fp32 and divided once; zeros for an utterance without frames.  A host call: needs
    no device."""
    rows = _f32(rows)
    fo = _frame_off(frame_off)
    if rows.ndim != 2 or rows.shape[0] < int(fo[-1]):
        raise ValueError("rows must be [frame_off[-1]][D]")
    out = np.zeros((fo.size - 1, rows.shape[1]), np.float32)
    _check(load().mlggd_nat_estimate(rows.shape[1], fo.size - 1, _i32p(fo), _p(rows), int(nat_frames), _p(out)))
    return out


def nat_rows(frame_off, first_frame):
    """nat_row [n_samples] int32: the utterance that holds each sample's first frame (mlggd_nat_rows); utterances
    without frames are stepped over.  A host call: needs no device."""
    fo = _frame_off(frame_off)
    first = np.ascontiguousarray(first_frame, dtype=np.int32)
    if first.ndim != 1:
        raise ValueError("first_frame is a 1-D table of frame indices")
    out = np.zeros(first.size, np.int32)
    _check(load().mlggd_nat_rows(fo.size - 1, _i32p(fo), first.size, _i32p(first), _i32p(out)))
    return out


# frame length L, hop S and FFT length N of the spectral front end per sampling rate in kHz (Wav2LogSpec_be.c)
SPECTRAL_PARAMS = {8: (256, 128, 256), 11: (256, 110, 256), 16: (512, 256, 512)}


def _wave(a):
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype != np.int16:
        raise ValueError("a wave is a 1-D int16 array")
    return np.ascontiguousarray(a)


def _sp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


def wave_to_lps(wave, fs_khz=16, device=0):
    """Log-power spectra [F][N/2+1] float32 of an int16 wave (the original project's Wav2LPS_be)."""
    wave = _wave(wave)
    F = C.c_int(0)
    _check(load().mlggd_wave_to_lps(int(device), int(fs_khz), wave.size, _sp(wave), C.byref(F), None))
    L, S, N = SPECTRAL_PARAMS[int(fs_khz)]
    lps = np.empty((F.value, N // 2 + 1), np.float32)
    if F.value:
        _check(load().mlggd_wave_to_lps(int(device), int(fs_khz), wave.size, _sp(wave), C.byref(F), _p(lps)))
    return lps


def lps_to_wave(noisy, lps, fs_khz=16, device=0, return_float=False):
    """int16 wave of F*S + L - S samples from LPS rows and the noisy wave's phase (the original project's LPS2Wav_be);
    return_float: (int16 wave, float32 wave before the cast)."""
    noisy = _wave(noisy)
    lps = _f32(lps)
    if lps.ndim != 2:
        raise ValueError("lps must be [n_frames][N/2+1]")
    L, S, N = SPECTRAL_PARAMS[int(fs_khz)]
    n_out = lps.shape[0] * S + L - S
    out = np.empty(n_out, np.int16)
    outf = np.empty(n_out, np.float32) if return_float else None
    _check(load().mlggd_lps_to_wave(int(device), int(fs_khz), noisy.size, _sp(noisy), lps.shape[0], _p(lps), _sp(out),
                                    _p(outf) if return_float else None))
    return (out, outf) if return_float else out


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=off[1:])
    return off


def enhance_waves_layout(lengths, fs_khz=16):
    """(frames, frame_off, out_off) of a packed batch of utterances of `lengths` samples (BPGpu.enhance_waves):
    frames [n] per utterance, frame_off [n+1] int32 into the packed frames, out_off [n+1] int64 into the packed
    output.  A host call: needs no device."""
    off = _offsets(lengths)
    n = off.size - 1
    frame_off = np.zeros(n + 1, np.int32)
    out_off = np.zeros(n + 1, np.int64)
    _lp = C.POINTER(C.c_int64)
    _check(load().mlggd_enhance_waves_layout(int(fs_khz), n, off.ctypes.data_as(_lp),
                                             frame_off.ctypes.data_as(C.POINTER(C.c_int32)),
                                             out_off.ctypes.data_as(_lp)))
    return np.diff(frame_off), frame_off, out_off


def _end_flags(end, n):
    if end is None:
        return None
    e = np.ascontiguousarray(np.asarray(end) != 0, dtype=np.uint8)
    if e.shape != (n,):
        raise ValueError("end must hold one flag per session")
    return e


def _bp(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None


def live_layout(had, add, end=None, fs_khz=16, fea_context=7):
    """out_off [n+1] int64 of the live push (BPGpu.live) that adds add[u] samples to a session that has received
    had[u], ending it where end[u]: session u emits out_off[u+1] - out_off[u] samples.  A host call: needs no
    device (mlggd_live_layout)."""
    had = np.ascontiguousarray(had, dtype=np.int64)
    add = np.ascontiguousarray(add, dtype=np.int64)
    if had.ndim != 1 or had.shape != add.shape:
        raise ValueError("had and add must hold one count per session")
    e = _end_flags(end, had.size)
    out_off = np.zeros(had.size + 1, np.int64)
    _lp = C.POINTER(C.c_int64)
    _check(load().mlggd_live_layout(int(fs_khz), int(fea_context), had.size, had.ctypes.data_as(_lp),
                                    add.ctypes.data_as(_lp), _bp(e), out_off.ctypes.data_as(_lp)))
    return out_off


class LiveGroup:
    """n_sessions audio sessions decoded block by block on one engine (BPGpu.live, mlggd_live_*): what a session
    emits from its first sample to its end, concatenated, equals enhance_wave of the whole recording bit for bit."""

    def __init__(self, eng, mean, inv_std, n_sessions, fs_khz, fea_context):
        self._s = None
        L, S, N = SPECTRAL_PARAMS.get(int(fs_khz), (0, 0, 0))
        D = N // 2 + 1
        if fea_context is None:
            fea_context = eng.K0 // D
        self.n_sessions, self.fs_khz, self.fea_context = int(n_sessions), int(fs_khz), int(fea_context)
        mean = _f32(mean, (D,)) if N else _f32(mean)
        inv = _f32(inv_std, (D,)) if N else _f32(inv_std)
        s = C.c_void_p()
        _check(load().mlggd_live_open(eng._h, self.fs_khz, self.fea_context, _p(mean), _p(inv), self.n_sessions,
                                      C.byref(s)))
        self._s = s
        self._eng = eng
        eng._lives.append(self)

    def received(self):
        """samples each session has received since it began, [n_sessions] int64"""
        had = np.zeros(self.n_sessions, np.int64)
        _check(load().mlggd_live_received(self._s, had.ctypes.data_as(C.POINTER(C.c_int64))))
        return had

    def push(self, blocks, end=None, return_f32=False):
        """blocks: n_sessions int16 arrays (possibly empty), the next samples of every session; end[u]: session u is
        finished after them.  Returns the list of int16 arrays that became final in this push (with return_f32 a
        tuple of two lists, the float32 samples before the cast second)."""
        if len(blocks) != self.n_sessions:
            raise ValueError("one block per session")
        blocks = [_wave(b) for b in blocks]
        n = self.n_sessions
        e = _end_flags(end, n)
        off = _offsets([b.size for b in blocks])
        total = live_layout(self.received(), np.diff(off), e, self.fs_khz, self.fea_context)[-1]
        packed = np.concatenate(blocks) if n else np.zeros(0, np.int16)
        out = np.empty(int(total), np.int16)
        outf = np.empty(out.size, np.float32) if return_f32 else None
        out_off = np.zeros(n + 1, np.int64)
        _lp = C.POINTER(C.c_int64)
        _check(load().mlggd_live_push(self._s, _sp(packed), off.ctypes.data_as(_lp), _bp(e), _sp(out),
                                      _p(outf) if return_f32 else None, out.size, out_off.ctypes.data_as(_lp)))
        res = [out[out_off[u]:out_off[u + 1]] for u in range(n)]
        if return_f32:
            return res, [outf[out_off[u]:out_off[u + 1]] for u in range(n)]
        return res

    def close(self):
        if self._s:
            load().mlggd_live_close(self._s)
            self._s = None
            if self in self._eng._lives:
                self._eng._lives.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _score_frames(score_frames, n):
    if score_frames is None:
        return None
    sf = np.ascontiguousarray(score_frames, dtype=np.int32)
    if sf.shape != (n,):
        raise ValueError("score_frames must hold one count per utterance")
    return sf


def _clean_like(cleans, noisys):
    """the clean waves packed with the noisy waves' offsets: each one cut or zero-padded to its noisy wave's length"""
    if len(cleans) != len(noisys):
        raise ValueError("one clean wave per noisy wave")
    packed = np.zeros(sum(w.size for w in noisys), np.int16)
    at = 0
    for c, w in zip(cleans, noisys):
        c = _wave(c)
        m = min(c.size, w.size)
        packed[at:at + m] = c[:m]
        at += w.size
    return packed


def score_waves(cleans, noisys, lps_list, fs_khz=16, device=0, score_frames=None):
    """(segsnr [n], lsd [n]) float32: the quality report of the original project's LPS2Wav_be for a list of utterances
    in one pass over the device (mlggd_score_waves) -- enhanced LPS rows lps_list[u] [F_u][N/2+1] of the noisy wave
    noisys[u] against the clean wave cleans[u].  score_frames[u] (None: all F_u) = the leading frames that are scored;
    0: the utterance is not scored and both numbers are 0.  A clean wave shorter than its noisy wave is zero-padded:
    pass its own frame count in score_frames."""
    noisys = [_wave(w) for w in noisys]
    n = len(noisys)
    _, frame_off, _ = enhance_waves_layout([w.size for w in noisys], fs_khz)
    D = SPECTRAL_PARAMS[int(fs_khz)][2] // 2 + 1
    if len(lps_list) != n:
        raise ValueError("one LPS matrix per noisy wave")
    rows = [_f32(l, (int(frame_off[u + 1] - frame_off[u]), D)) for u, l in enumerate(lps_list)]
    lps = np.concatenate(rows) if n else np.zeros((0, D), np.float32)
    clean = _clean_like(cleans, noisys)
    packed = np.concatenate(noisys) if n else np.zeros(0, np.int16)
    off = _offsets([w.size for w in noisys])
    sf = _score_frames(score_frames, n)
    segsnr, lsd = np.zeros(n, np.float32), np.zeros(n, np.float32)
    _check(load().mlggd_score_waves(int(device), int(fs_khz), n, _sp(clean), _sp(packed),
                                    off.ctypes.data_as(C.POINTER(C.c_int64)), _p(lps),
                                    sf.ctypes.data_as(C.POINTER(C.c_int32)) if sf is not None else None,
                                    _p(segsnr), _p(lsd)))
    return segsnr, lsd


def stoi_layout(n_samples, fs_khz=16):
    """(len10, frames, min_segments_if_all_kept) of an utterance of n_samples for STOI (stoi_waves): its samples at
    10 kHz, its frames of 256 at hop 128, and the 30-frame segments it has when no frame is removed as silent.  A host
    call: needs no device (mlggd_stoi_layout)."""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _check(load().mlggd_stoi_layout(int(fs_khz), int(n_samples), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def _stoi_samples(stoi_samples, n):
    if stoi_samples is None:
        return None
    ss = np.ascontiguousarray(stoi_samples, dtype=np.int64)
    if ss.shape != (n,):
        raise ValueError("stoi_samples must hold one count per utterance")
    return ss


def stoi_waves(cleans, procs, fs_khz=16, device=0, stoi_samples=None, return_segments=False):
    """STOI [n] float32 (Taal et al. 2011) of the processed int16 waves procs[u] against the clean int16 waves
    cleans[u], in one pass over the device (mlggd_stoi_waves).  stoi_samples[u] = the leading samples that are scored
    (None: as many as both waves have).  NaN where the utterance has no value: fewer than 30 frames after the silent
    ones are removed, or a processed band of exact zeros over a whole segment (segments still counted).
    return_segments: (stoi, segments [n] int32), the 30-frame segments behind each value."""
    procs = [_wave(w) for w in procs]
    n = len(procs)
    clean = _clean_like(cleans, procs)
    ss = _stoi_samples(stoi_samples, n)
    if ss is None:
        ss = np.array([min(_wave(c).size, w.size) for c, w in zip(cleans, procs)], np.int64).reshape(n)
    packed = np.concatenate(procs) if n else np.zeros(0, np.int16)
    off = _offsets([w.size for w in procs])
    _lp = C.POINTER(C.c_int64)
    stoi, seg = np.zeros(n, np.float32), np.zeros(n, np.int32)
    _check(load().mlggd_stoi_waves(int(device), int(fs_khz), n, _sp(clean), _sp(packed), off.ctypes.data_as(_lp),
                                   ss.ctypes.data_as(_lp), _p(stoi), seg.ctypes.data_as(C.POINTER(C.c_int32))))
    return (stoi, seg) if return_segments else stoi


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def wave_samples(lengths, fea_context, fs_khz=16):
    """first_frame [n] int32: every window of fea_context frames that lies inside one utterance of a packed batch of
    utterances of `lengths` samples, in utterance and frame order, as indices into the packed frame stream -- the sample
    table of BPGpu.load_waves / train_waves.  Shuffling is the caller's: permute it.  A host call: needs no device
    (mlggd_wave_samples)."""
    off = _offsets(lengths)
    n = C.c_int64(0)
    _check(load().mlggd_wave_samples(int(fs_khz), int(fea_context), off.size - 1, _i64p(off), None, C.byref(n)))
    first = np.zeros(n.value, np.int32)
    _check(load().mlggd_wave_samples(int(fs_khz), int(fea_context), off.size - 1, _i64p(off),
                                     first.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)))
    return first


def _mix_args(n, n_noise, snr_db, noise_start, noise_seg):
    """snr_db, noise_start [n] and the segments [(lo, len)] (None: the whole noise for every utterance)"""
    snr = np.ascontiguousarray(np.broadcast_to(np.asarray(snr_db, np.float64), (n,)))
    start = np.ascontiguousarray(np.broadcast_to(np.asarray(noise_start, np.int64), (n,)))
    if noise_seg is None:
        lo, ln = np.zeros(n, np.int64), np.full(n, n_noise, np.int64)
    else:
        seg = np.asarray(noise_seg, np.int64).reshape(-1, 2)
        if seg.shape != (n, 2):
            raise ValueError("noise_seg must hold one (lo, len) per utterance")
        lo, ln = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
    return snr, start, lo, ln


def mix_waves(cleans, noise, snr_db, noise_start, noise_seg=None, device=0, return_info=False):
    """Noisy int16 waves: cleans[u] plus `noise` scaled to snr_db[u] dB (mlggd_mix_waves; the rule is csrc/mix_rule.h).
    Utterance u takes the noise segment noise_seg[u] = (lo, len) (None: the whole noise) from noise_start[u] inside it
    on, wrapping at the segment's end.  return_info: (waves, gain [n] float64, clipped [n] int32)."""
    cleans = [_wave(w) for w in cleans]
    noise = _wave(noise)
    n = len(cleans)
    snr, start, lo, ln = _mix_args(n, noise.size, snr_db, noise_start, noise_seg)
    off = _offsets([w.size for w in cleans])
    packed = np.concatenate(cleans) if n else np.zeros(0, np.int16)
    out = np.zeros(packed.size, np.int16)
    gain, clipped = np.zeros(n, np.float64), np.zeros(n, np.int32)
    _check(load().mlggd_mix_waves(int(device), n, _sp(packed), _i64p(off), _sp(noise), noise.size, _i64p(lo), _i64p(ln),
                                  _i64p(start), snr.ctypes.data_as(C.POINTER(C.c_double)), _sp(out),
                                  gain.ctypes.data_as(C.POINTER(C.c_double)),
                                  clipped.ctypes.data_as(C.POINTER(C.c_int32))))
    waves = [out[off[u]:off[u + 1]] for u in range(n)]
    return (waves, gain, clipped) if return_info else waves


def lps_stats(waves, fs_khz=16, device=0):
    """(n_frames, sums [2][D] float64): per bin the sum and the sum of squares of the LPS rows of all the waves, formed
    on the device (mlggd_lps_stats).  Additive over calls; norm_from_stats turns them into the norm vectors."""
    waves = [_wave(w) for w in waves]
    D = SPECTRAL_PARAMS.get(int(fs_khz), (0, 0, 512))[2] // 2 + 1
    off = _offsets([w.size for w in waves])
    packed = np.concatenate(waves) if waves else np.zeros(0, np.int16)
    sums = np.zeros((2, D), np.float64)
    n = C.c_int64(0)
    _check(load().mlggd_lps_stats(int(device), int(fs_khz), len(waves), _sp(packed), _i64p(off),
                                  sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
    return n.value, sums


def norm_from_stats(n, sums):
    """(mean [D], inv_std [D]) float32 from the sums of lps_stats over n frames: mean = S1/n, inv_std = 1 / sqrt(S2/n -
    mean^2), the population variance, in double (mlggd_norm_from_stats).  A host call: needs no device."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != 2:
        raise ValueError("sums must be [2][D]")
    D = s.shape[1]
    mean, inv = np.zeros(D, np.float32), np.zeros(D, np.float32)
    _check(load().mlggd_norm_from_stats(D, int(n), s.ctypes.data_as(C.POINTER(C.c_double)), _p(mean), _p(inv)))
    return mean, inv


GgdFit = collections.namedtuple("GgdFit", "mean var kurt alpha loglik best loglik_shared best_shared")


def _betas(betas):
    b = np.ascontiguousarray(betas, dtype=np.float32)
    if b.ndim != 1:
        raise ValueError("betas is a 1-D grid of shapes")
    return b


def ggd_fit(n, sums, betas):
    """Fit of the GGD error model to the [4 + K][D] sums of BPGpu.error_stats over n samples (added over the chunks
    by the caller): a GgdFit of mean, var, kurt [D], alpha, loglik [K][D] (ML scale and profile log-likelihood per
    grid shape), best [D] (grid index per bin, -1 where the bin has no fit), loglik_shared [K] and best_shared, the
    grid index to put into `shapefactor`.  A host call: needs no device (mlggd_ggd_fit)."""
    b = _betas(betas)
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != 4 + b.size:
        raise ValueError("sums must be [4 + len(betas)][D]")
    K, D = b.size, s.shape[1]
    _dp, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    mean, var, kurt = np.zeros(D), np.zeros(D), np.zeros(D)
    alpha, loglik = np.zeros((K, D)), np.zeros((K, D))
    best, shared, bs = np.zeros(D, np.int32), np.zeros(K), C.c_int32(0)
    d = lambda a: a.ctypes.data_as(_dp)
    _check(load().mlggd_ggd_fit(D, int(n), K, _p(b), d(s), d(mean), d(var), d(kurt), d(alpha), d(loglik),
                                best.ctypes.data_as(_i32), d(shared), C.byref(bs)))
    return GgdFit(mean, var, kurt, alpha, loglik, best, shared, bs.value)


def read_shapefactors(path, D, fallback):
    """[D] float32 shapes from a plain list of D numbers or from the file MLGGD_ERRMODEL writes (its best_beta column;
    a bin without a fit takes the file's shared beta, else `fallback`).  A host call: needs no device
    (mlggd_read_shapefactors); a malformed file raises MlggdError naming the line."""
    b = np.empty(int(D), np.float32)
    _check(load().mlggd_read_shapefactors(None if path is None else os.fsencode(path), int(D), float(fallback), _p(b)))
    return b


AsymFit = collections.namedtuple("AsymFit", "kappa alpha loglik best loglik_shared best_shared")


def asym_fit(n, signed, betas):
    """Fit of the asymmetric GGD error model to the [2 K][D] sums of BPGpu.error_stats_signed over n samples (added
    over the chunks by the caller): an AsymFit of kappa, alpha, loglik [K][D] (the closed-form ML skew and scale and
    the profile log-likelihood per grid shape; NaN / 0 / NaN where a bin has no fit), best [D] (grid index per bin, -1
    without a fit), loglik_shared [K] and best_shared.  A host call: needs no device (mlggd_asym_fit)."""
    b = _betas(betas)
    s = np.ascontiguousarray(signed, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != 2 * b.size:
        raise ValueError("signed must be [2 * len(betas)][D]")
    K, D = b.size, s.shape[1]
    _dp, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    kappa, alpha, loglik = np.zeros((K, D)), np.zeros((K, D)), np.zeros((K, D))
    best, shared, bs = np.zeros(D, np.int32), np.zeros(K), C.c_int32(0)
    d = lambda a: a.ctypes.data_as(_dp)
    _check(load().mlggd_asym_fit(D, int(n), K, _p(b), d(s), d(kappa), d(alpha), d(loglik), best.ctypes.data_as(_i32),
                                 d(shared), C.byref(bs)))
    return AsymFit(kappa, alpha, loglik, best, shared, bs.value)


def read_asymmetry(path, D, fallback=1.0):
    """[D] float32 skews from a plain list of D numbers or from the file MLGGD_ASYMMODEL writes (its best_kappa column;
    a bin without a fit takes `fallback`).  A host call: needs no device (mlggd_read_asymmetry); a malformed file
    raises MlggdError naming the line."""
    k = np.empty(int(D), np.float32)
    _check(load().mlggd_read_asymmetry(None if path is None else os.fsencode(path), int(D), float(fallback), _p(k)))
    return k


SCALE_MODES = ("alternating", "learned")  # MLGGD_SCALE_ALTERNATING = 0, MLGGD_SCALE_LEARNED = 1 (include/mlggd.h)
ScaleMode = collections.namedtuple("ScaleMode", "mode lrate momentum vmax steps")


def scale_mode_code(mode):
    if mode not in SCALE_MODES:
        raise ValueError("scale mode %r: must be one of %s" % (mode, ", ".join(SCALE_MODES)))
    return SCALE_MODES.index(mode)


def read_scale_state(path, D):
    """(alpha, velocity), [D] float32 each, from the file write_scale_state or the trainer's MLGGD_SCALE_FILE writes.  A
    host call: needs no device (mlggd_read_scale_state); a malformed file raises MlggdError naming the line."""
    a, v = np.empty(int(D), np.float32), np.empty(int(D), np.float32)
    _check(load().mlggd_read_scale_state(None if path is None else os.fsencode(path), int(D), _p(a), _p(v)))
    return a, v


def write_scale_state(path, alpha, velocity=None, lrate=0.05, momentum=0.5, vmax=1.0, steps=0):
    """The learned scale's state as text, every number in %.9g: a round trip through read_scale_state keeps every bit.
    velocity None: zeros.  A host call: needs no device (mlggd_write_scale_state)."""
    a = np.ascontiguousarray(alpha, dtype=np.float32).ravel()
    v = None if velocity is None else _f32(velocity, (a.size,))
    _check(load().mlggd_write_scale_state(None if path is None else os.fsencode(path), a.size, _p(a), None if v is None else _p(v),
                                          float(lrate), float(momentum), float(vmax), int(steps)))


OPTIMIZERS = ("sgd", "adam")  # MLGGD_OPT_SGD = 0, MLGGD_OPT_ADAM = 1 (include/mlggd.h)
Optimizer = collections.namedtuple("Optimizer", "name beta1 beta2 eps steps")
OptimizerState = collections.namedtuple("OptimizerState", "m_w v_w m_b v_b steps")
OptimizerFile = collections.namedtuple("OptimizerFile", "layersizes beta1 beta2 eps steps m_w v_w m_b v_b")


def optimizer_code(name):
    if name not in OPTIMIZERS:
        raise ValueError("optimizer %r: must be one of %s" % (name, ", ".join(OPTIMIZERS)))
    return OPTIMIZERS.index(name)


def adam_apply(w, m, v, G, nf, weightcost, lrate, beta1=0.9, beta2=0.999, eps=1e-8, steps=0):
    """One Adam update of the arrays (w, m, v) from the summed gradient G of a minibatch of nf frames, `steps` updates
    having been taken before: the rule of csrc/adam_rule.h compiled for the host (mlggd_adam_apply), the statements the
    device launch runs.  Returns new (w, m, v), float32 in w's shape; the inputs are not written.  Needs no device."""
    w, m, v, G = (np.array(a, dtype=np.float32, order="C") for a in (w, m, v, G))
    if not (w.shape == m.shape == v.shape == G.shape):
        raise ValueError("w, m, v and G must have one shape")
    _check(load().mlggd_adam_apply(_p(w), _p(m), _p(v), _p(G), w.size, float(nf), float(weightcost), float(lrate), float(beta1),
                                   float(beta2), float(eps), int(steps)))
    return w, m, v


def _moment_arrays(layersizes):
    L = len(layersizes)
    return ([np.empty((layersizes[l], layersizes[l + 1]), np.float32) for l in range(L - 1)],
            [np.empty(layersizes[l + 1], np.float32) for l in range(L - 1)])


def write_optimizer_state(path, layersizes, m_w, v_w, m_b, v_b, beta1=0.9, beta2=0.999, eps=1e-8, steps=0):
    """The Adam state as the binary file the trainer's MLGGD_OPT_FILE holds (host/optfile.h): the moments of every layer,
    unpadded, in returnWeights' shapes, behind a header with the layer sizes, the betas, eps and steps.  A host call:
    needs no device (mlggd_write_optimizer_state)."""
    ls = [int(x) for x in layersizes]
    L = len(ls)
    arrs = []
    for name, group, wide in (("m_w", m_w, True), ("v_w", v_w, True), ("m_b", m_b, False), ("v_b", v_b, False)):
        if len(group) != max(L - 1, 0):
            raise ValueError("%s: %d arrays for %d layers" % (name, len(group), L))
        arrs.append([_f32(a, (ls[l], ls[l + 1]) if wide else (ls[l + 1],)) for l, a in enumerate(group)])
    lsa = (C.c_int32 * max(L, 1))(*ls)
    _check(load().mlggd_write_optimizer_state(None if path is None else os.fsencode(path), L, lsa, *[_ptr_array(a) for a in arrs],
                                              float(beta1), float(beta2), float(eps), int(steps)))


def read_optimizer_state(path):
    """OptimizerFile(layersizes, beta1, beta2, eps, steps, m_w, v_w, m_b, v_b) from the file write_optimizer_state or
    the trainer's MLGGD_OPT_FILE writes.  A host call: needs no device; a file that is cut, of another version or not
    such a file raises MlggdError naming what is wrong."""
    fn = None if path is None else os.fsencode(path)
    n, lsa = C.c_int32(0), (C.c_int32 * MAXLAYER)()
    _check(load().mlggd_read_optimizer_header(fn, C.byref(n), lsa, None, None, None, None))
    ls = [int(lsa[i]) for i in range(n.value)]
    (m_w, m_b), (v_w, v_b) = _moment_arrays(ls), _moment_arrays(ls)
    b1, b2, eps, st = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int64(0)
    _check(load().mlggd_read_optimizer_state(fn, len(ls), lsa, _ptr_array(m_w), _ptr_array(v_w), _ptr_array(m_b), _ptr_array(v_b),
                                             C.byref(b1), C.byref(b2), C.byref(eps), C.byref(st)))
    return OptimizerFile(ls, b1.value, b2.value, eps.value, st.value, m_w, v_w, m_b, v_b)


GvFit = collections.namedtuple("GvFit","gv_est gv_ref eta fitted gv_est_shared gv_ref_shared eta_shared fitted_shared")


def gv_fit(n, sums):
    """Fit of the global variance equalisation factors to the [4][D] sums of BPGpu.output_stats over n samples (added
    over the chunks by the caller): a GvFit of gv_est, gv_ref [D] float64 (variances of the normalised outputs and
    targets), eta [D] float32 = sqrt(gv_ref / gv_est), fitted [D] bool (False where a variance is not positive: eta 1
    there), and the same four for the factor shared by all bins.  A host call: needs no device (mlggd_gv_fit)."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != 4:
        raise ValueError("sums must be [4][D]")
    D = s.shape[1]
    _dp = C.POINTER(C.c_double)
    est, ref, eta, fitted = np.zeros(D), np.zeros(D), np.ones(D, np.float32), np.zeros(D, np.uint8)
    est_s, ref_s, eta_s, fit_s = C.c_double(0), C.c_double(0), C.c_float(1), C.c_int32(0)
    d = lambda a: a.ctypes.data_as(_dp)
    _check(load().mlggd_gv_fit(D, int(n), d(s), d(est), d(ref), _p(eta), fitted.ctypes.data_as(C.POINTER(C.c_uint8)),
                               C.byref(est_s), C.byref(ref_s), C.byref(eta_s), C.byref(fit_s)))
    return GvFit(est, ref, eta, fitted.astype(bool), est_s.value, ref_s.value, np.float32(eta_s.value), bool(fit_s.value))


def read_gv(path, D, shared=False):
    """[D] float32 equalisation factors from a plain list of D numbers or from the file MLGGD_GVFILE writes (its eta
    column; a bin without a fit takes 1; shared=True: the file's shared factor in every bin).  A host call: needs no
    device (mlggd_read_gv); a malformed file raises MlggdError naming the line."""
    e = np.empty(int(D), np.float32)
    _check(load().mlggd_read_gv(None if path is None else os.fsencode(path), int(D), 1 if shared else 0, _p(e)))
    return e


MASK_MODES = ("off", "select")  # MLGGD_MASK_OFF = 0, MLGGD_MASK_SELECT = 1 (include/mlggd.h)
Mask = collections.namedtuple("Mask", "mode lo hi scale")


def mask_mode_code(mode):
    if mode not in MASK_MODES:
        raise ValueError("mask mode %r: must be one of %s" % (mode, ", ".join(MASK_MODES)))
    return MASK_MODES.index(mode)


def mask_targets(noisy_lps, clean_lps, scale=1.0, device=0):
    """The mask half of a mask engine's target rows (csrc/mask_rule.h) from UN-normalised LPS rows [n][D]:
    scale * min(1, exp_det(0.5 * (clean - noisy))) in float32, the arithmetic train_waves runs, on the device
    (mlggd_mask_targets)."""
    n, c = _f32(noisy_lps), _f32(clean_lps)
    if n.ndim != 2 or n.shape != c.shape or n.shape[1] < 1:
        raise ValueError("noisy_lps and clean_lps must both be [n][D]")
    out = np.empty(n.shape, np.float32)
    _check(load().mlggd_mask_targets(int(device), n.shape[1], n.shape[0], _p(n), _p(c), float(scale), _p(out)))
    return out


def mask_select(noisy_lps, lps, mask, lo, hi):
    """The mask post-filter on rows [n][D]: mask > hi takes the noisy LPS, lo <= mask <= hi the mean of the noisy LPS and
    the estimate lps, else (a NaN included) the estimate.  A host call: needs no device (mlggd_mask_select), the float32
    statement of csrc/mask_rule.h."""
    n, x, m = _f32(noisy_lps), _f32(lps), _f32(mask)
    if n.ndim != 2 or n.shape != x.shape or n.shape != m.shape or n.shape[1] < 1:
        raise ValueError("noisy_lps, lps and mask must all be [n][D]")
    out = np.empty(n.shape, np.float32)
    _check(load().mlggd_mask_select(n.shape[1], n.shape[0], _p(n), _p(x), _p(m), float(lo), float(hi), _p(out)))
    return out


RBM_VISIBLE = ("gaussian", "bernoulli")  # MLGGD_RBM_GAUSSIAN = 0, MLGGD_RBM_BERNOULLI = 1 (include/mlggd.h)


def rbm_draws(seed, step, B, N):
    """r [B][N] in [0, 1): the uniform draws of step `step` of an RBM session opened with `seed`, h0s = (r < h0p)
    (csrc/rbm_rule.h).  A host call: needs no device (mlggd_rbm_draws)."""
    out = np.empty((int(B), int(N)), np.float32)
    _check(load().mlggd_rbm_draws(int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, int(B), int(N), _p(out)))
    return out


class Rbm:
    """CD-1 pre-training of one hidden layer of a sigmoid engine (csrc/rbm_rule.h, mlggd_rbm_*): made by BPGpu.rbm().
    It trains the engine's own weights and bias of that layer in place; the visible bias and the momentum are its own."""

    def __init__(self, eng, layer, visible, lrate, momentum, weightcost, seed):
        self._h = None
        self._eng = eng
        self.layer = int(layer)
        if isinstance(visible, str):
            if visible not in RBM_VISIBLE:
                raise ValueError("visible %r: must be one of %s" % (visible, " / ".join(map(repr, RBM_VISIBLE))))
            visible = RBM_VISIBLE.index(visible)
        h = C.c_void_p()
        _check(load().mlggd_rbm_open(eng._h, self.layer, int(visible), float(lrate), float(momentum), float(weightcost),
                                     int(seed) & 0xFFFFFFFF, C.byref(h)))
        self._h = h
        self.K, self.N = eng.layersizes[self.layer - 1], eng.layersizes[self.layer]
        eng._rbms.append(self)

    def set_rates(self, lrate, momentum):
        _check(load().mlggd_rbm_set_rates(self._h, float(lrate), float(momentum)))

    def train(self, inp):
        """One CD-1 step on every full bunch of inp [n][layersizes[0]]: (bunches, recon_sqerr)."""
        inp = _f32(inp)
        if inp.ndim != 2 or inp.shape[1] != self._eng.K0:
            raise ValueError("in must be [n][%d]" % self._eng.K0)
        steps, sq = C.c_int(0), C.c_double(0.0)
        _check(load().mlggd_rbm_train_chunk(self._h, inp.shape[0], _p(inp), C.byref(steps), C.byref(sq)))
        return steps.value, sq.value

    def train_frames(self, feat, first_frame, fea_context):
        """The same on a frame stream [n_frames][layersizes[0] / fea_context] and the first frame of every sample."""
        feat, _, first = self._eng._frames_args(feat, None, first_frame, fea_context)
        steps, sq = C.c_int(0), C.c_double(0.0)
        _check(load().mlggd_rbm_train_frames(self._h, feat.shape[0], int(fea_context), _p(feat), first.size,
                                             first.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(steps), C.byref(sq)))
        return steps.value, sq.value

    def visible_bias(self):
        out = np.empty(self.K, np.float32)
        _check(load().mlggd_rbm_visible_bias(self._h, _p(out)))
        return out

    def tensor(self, name):
        """A tensor of the last step: "v0", "v1" [B][K]; "h0p", "h0s", "h1p" [B][N]; "delta_w" [K][N]; "delta_b" [N];
        "delta_c", "vbias" [K]."""
        B = self._eng.bunchsize
        shape = {"v0": (B, self.K), "v1": (B, self.K), "h0p": (B, self.N), "h0s": (B, self.N), "h1p": (B, self.N),
                 "delta_w": (self.K, self.N), "delta_b": (self.N,), "delta_c": (self.K,), "vbias": (self.K,)}.get(name)
        if shape is None:
            raise ValueError("unknown RBM tensor %r" % (name,))
        out = np.empty(shape, np.float32)
        _check(load().mlggd_rbm_debug_tensor(self._h, name.encode(), _p(out), out.size))
        return out

    def close(self):
        if self._h:
            load().mlggd_rbm_close(self._h)
            self._h = None
            if self in self._eng._rbms:
                self._eng._rbms.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def comm_unique_id():
    buf = (C.c_char * UNIQUE_ID_BYTES)()
    _check(load().mlggd_comm_unique_id(buf))
    return bytes(buf)


class BPGpu:
    """Same constructor arguments and methods as the reference's BP_GPU (BP_GPU.h:48-59)."""

    def __init__(self, random_seed, gpu, layersizes, bunchsize, lrate, momentum, weightcost, weights, bias,
                 shapefactor, MLflag, dropoutflag=0, visible_omit=0.0, hid_omit=0.0, max_cache_frames=0, activation="sigmoid",
                 nat_frames=0, mask_bins=0):
        self._h = None
        act = activation_code(activation)  # hidden units: "sigmoid" (the reference's BPtrain_Sigmoid) or "relu"
        self._lives = []
        self._rbms = []
        self._n_noise = 0
        self._nat = int(nat_frames) > 0
        self.layersizes = [int(x) for x in layersizes]
        self.numlayers = len(self.layersizes)
        if not 2 <= self.numlayers <= MAXLAYER:
            raise ValueError("numlayers must be 2..%d" % MAXLAYER)
        self.bunchsize = int(bunchsize)
        self.D = self.layersizes[-1]
        self.K0 = self.layersizes[0]
        ws = [_f32(w, (self.layersizes[l], self.layersizes[l + 1])) for l, w in enumerate(weights)]
        bs = [_f32(b, (self.layersizes[l + 1],)) for l, b in enumerate(bias)]
        if len(ws) != self.numlayers - 1 or len(bs) != self.numlayers - 1:
            raise ValueError("need numlayers-1 weight matrices and bias vectors")
        cfg = _Config()
        cfg.struct_size = C.sizeof(_Config)
        cfg.random_seed = int(random_seed)
        cfg.device = int(gpu)
        cfg.numlayers = self.numlayers
        for i, v in enumerate(self.layersizes):
            cfg.layersizes[i] = v
        cfg.bunchsize = self.bunchsize
        cfg.lrate, cfg.momentum, cfg.weightcost = lrate, momentum, weightcost
        cfg.shapefactor, cfg.MLflag = shapefactor, int(MLflag)
        cfg.dropoutflag, cfg.visible_omit, cfg.hid_omit = int(dropoutflag), visible_omit, hid_omit
        cfg.max_cache_frames = int(max_cache_frames)
        cfg.activation = act
        cfg.nat_frames = int(nat_frames)  # noise-aware training: every input row ends in its utterance's noise row
        cfg.mask_bins = int(mask_bins)  # multi-objective net: 2 * mask_bins outputs, the clean LPS and a ratio mask
        h = C.c_void_p()
        rc = load().mlggd_create(C.byref(cfg), _ptr_array(ws), _ptr_array(bs), C.byref(h))
        if rc != 0:
            msg = load().mlggd_last_error().decode()
            if h:
                load().mlggd_destroy(h)
            raise MlggdError("mlggd_create failed (%d): %s" % (rc, msg))
        self._h = h

    @property
    def activation(self):
        """"sigmoid" or "relu": what the engine's hidden layers apply (mlggd_get_activation)."""
        a = C.c_int()
        _check(load().mlggd_get_activation(self._h, C.byref(a)))
        return ACTIVATIONS[a.value]

    @property
    def nat_frames(self):
        """0, or the T of noise-aware training the engine was created with (mlggd_get_nat_frames)."""
        n = C.c_int()
        _check(load().mlggd_get_nat_frames(self._h, C.byref(n)))
        return n.value

    @property
    def mask_bins(self):
        """0, or the M of a multi-objective net: 2 M outputs, the clean LPS and a ratio mask (mlggd_get_mask_bins)."""
        n = C.c_int()
        _check(load().mlggd_get_mask_bins(self._h, C.byref(n)))
        return n.value

    def set_mask(self, mode="select", lo=0.25, hi=0.75, scale=1.0):
        """The mask post-filter of a mask engine's decoders and the scale of its mask targets (csrc/mask_rule.h,
        mlggd_set_mask): "select" lets mask / scale choose per bin between the noisy LPS (> hi), the mean of noisy
        LPS and estimate (lo .. hi) and the estimate; "off" decodes the LPS half alone.  The defaults are a choice,
        not a measured optimum."""
        _check(load().mlggd_set_mask(self._h, mask_mode_code(mode), float(lo), float(hi), float(scale)))

    def mask(self):
        """Mask(mode, lo, hi, scale) in effect (mlggd_get_mask)."""
        m, lo, hi, s = C.c_int(), C.c_float(), C.c_float(), C.c_float()
        _check(load().mlggd_get_mask(self._h, C.byref(m), C.byref(lo), C.byref(hi), C.byref(s)))
        return Mask(MASK_MODES[m.value], lo.value, hi.value, s.value)

    # -- lifetime
    def close(self):
        if self._h:
            for g in list(self._lives):  # an engine with an open live group cannot be destroyed
                g.close()
            for r in list(self._rbms):  # ... nor one with an open RBM session
                r.close()
            load().mlggd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- BP_GPU::train
    def train(self, inp, targ):
        inp = _f32(inp)
        targ = _f32(targ)
        n = inp.shape[0]
        if inp.shape != (n, self.K0) or targ.shape != (n, self.D):
            raise ValueError("in must be [n][%d] and targ [n][%d]" % (self.K0, self.D))
        trained = C.c_int(0)
        _check(load().mlggd_train_chunk(self._h, n, _p(inp), _p(targ), C.byref(trained)))
        return trained.value

    def load_chunk(self, inp, targ):
        inp = _f32(inp)
        targ = _f32(targ)
        n = inp.shape[0]
        if inp.shape != (n, self.K0) or targ.shape != (n, self.D):
            raise ValueError("in must be [n][%d] and targ [n][%d]" % (self.K0, self.D))
        _check(load().mlggd_load_chunk(self._h, n, _p(inp), _p(targ)))

    def train_resident(self, first_frame, n_frames):
        trained = C.c_int(0)
        _check(load().mlggd_train_resident(self._h, int(first_frame), int(n_frames), C.byref(trained)))
        return trained.value

    # -- frame-stream chunks (input pipeline on the device)
    def _frames_args(self, feat, targ, first_frame, fea_context):
        feat = _f32(feat)
        first = np.ascontiguousarray(first_frame, dtype=np.int32)
        if feat.ndim != 2 or feat.shape[1] * fea_context != self.K0:
            raise ValueError("feat must be [n_frames][%d/fea_context]" % self.K0)
        if targ is not None:
            targ = _f32(targ, (feat.shape[0], self.D))
        return feat, targ, first

    def load_frames(self, feat, targ, first_frame, fea_context, targ_offset):
        feat, targ, first = self._frames_args(feat, targ, first_frame, fea_context)
        _check(load().mlggd_load_frames(self._h, feat.shape[0], int(fea_context), _p(feat),
                                        _p(targ) if targ is not None else None, first.size,
                                        first.ctypes.data_as(C.POINTER(C.c_int32)), int(targ_offset)))

    def train_frames(self, feat, targ, first_frame, fea_context, targ_offset, wait=True):
        """wait=False: mlggd_train_frames_async -- returns once the chunk is on the device and its steps are
        enqueued (the arrays may be reused at once); sync() waits."""
        feat, targ, first = self._frames_args(feat, targ, first_frame, fea_context)
        trained = C.c_int(0)
        fn = load().mlggd_train_frames if wait else load().mlggd_train_frames_async
        _check(fn(self._h, feat.shape[0], int(fea_context), _p(feat), _p(targ), first.size,
                  first.ctypes.data_as(C.POINTER(C.c_int32)), int(targ_offset), C.byref(trained)))
        return trained.value

    def cv_all_frames(self, feat, targ, first_frame, fea_context, targ_offset):
        feat, targ, first = self._frames_args(feat, targ, first_frame, fea_context)
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(load().mlggd_cv_all_frames(self._h, feat.shape[0], int(fea_context), _p(feat), _p(targ), first.size,
                                          first.ctypes.data_as(C.POINTER(C.c_int32)), int(targ_offset), C.byref(a),
                                          C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # -- the column statistics of a CV chunk, both chunk forms: fn one of the six C entries, rows(K) the rows of its
    # sums for a grid of K shapes, betas None where the entry has no grid
    def _col_stats(self, fn, rows, inp, targ, betas=None):
        inp, targ = _f32(inp), _f32(targ)
        b = None if betas is None else _betas(betas)
        grid = () if b is None else (b.size, _p(b))
        n = inp.shape[0]
        if inp.shape != (n, self.K0) or targ.shape != (n, self.D):
            raise ValueError("in must be [n][%d] and targ [n][%d]" % (self.K0, self.D))
        sums = np.zeros((rows(0 if b is None else b.size), self.D), np.float64)
        _check(fn(self._h, n, _p(inp), _p(targ), *grid,
                  sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    def _col_stats_frames(self, fn, rows, feat, targ, first_frame, fea_context, targ_offset, betas=None):
        feat, targ, first = self._frames_args(feat, targ, first_frame, fea_context)
        b = None if betas is None else _betas(betas)
        grid = () if b is None else (b.size, _p(b))
        sums = np.zeros((rows(0 if b is None else b.size), self.D), np.float64)
        _check(fn(self._h, feat.shape[0], int(fea_context), _p(feat), _p(targ), first.size,
                  first.ctypes.data_as(C.POINTER(C.c_int32)), int(targ_offset),
                  *grid, sums.ctypes.data_as(C.POINTER(C.c_double))))
        return sums

    # -- the GGD error model: per-bin sums of e^1..4 and |e|^beta over a CV chunk, formed on the device (ggd_fit fits them)
    def error_stats(self, inp, targ, betas):
        """[4 + K][D] float64: sum e, e^2, e^3, e^4 and sum |e|^betas[k] per output bin over the rows of inp / targ,
        e = forward(inp) - targ (mlggd_error_stats).  Additive over chunks."""
        return self._col_stats(load().mlggd_error_stats, lambda K: 4 + K, inp, targ, betas)

    def error_stats_frames(self, feat, targ, first_frame, fea_context, targ_offset, betas):
        """The same over a frame-stream chunk (mlggd_error_stats_frames): the same bits for the same rows."""
        return self._col_stats_frames(load().mlggd_error_stats_frames, lambda K: 4 + K, feat, targ, first_frame, fea_context,
                                      targ_offset, betas)

    # -- the asymmetric error model: the power sums split by the sign of e (asym_fit fits them), and the skew per bin
    def error_stats_signed(self, inp, targ, betas):
        """[2 K][D] float64: rows 0..K-1 sum_{e>0} e^betas[k], rows K..2K-1 sum_{e<0} (-e)^betas[k] per output bin over
        the rows of inp / targ, e = forward(inp) - targ (mlggd_error_stats_signed).  Additive over chunks."""
        return self._col_stats(load().mlggd_error_stats_signed, lambda K: 2 * K, inp, targ, betas)

    def error_stats_signed_frames(self, feat, targ, first_frame, fea_context, targ_offset, betas):
        """The same over a frame-stream chunk (mlggd_error_stats_signed_frames): the same bits for the same rows."""
        return self._col_stats_frames(load().mlggd_error_stats_signed_frames, lambda K: 2 * K, feat, targ, first_frame,
                                      fea_context, targ_offset, betas)

    def asymmetry(self):
        """The D skews in effect: the vector of set_asymmetry, else ones."""
        k = np.empty(self.D, np.float32)
        _check(load().mlggd_get_asymmetry(self._h, _p(k)))
        return k

    def set_asymmetry(self, kappas):
        """One skew per output bin from the next step or CV call on (MLflag 1 only); None: off.  Weights, momentum,
        the current scalefactor and the shape vector stay (mlggd_set_asymmetry)."""
        if kappas is None:
            _check(load().mlggd_set_asymmetry(self._h, None))
            return
        k = _f32(kappas, (self.D,))
        _check(load().mlggd_set_asymmetry(self._h, _p(k)))

    # -- global variance equalisation: per-bin sums of y, y^2, t, t^2 over a CV chunk, formed on the device (gv_fit fits them)
    def output_stats(self, inp, targ):
        """[4][D] float64: sum y, y^2, t, t^2 per output bin over the rows of inp / targ, y = forward(inp)
        (mlggd_output_stats).  Additive over chunks."""
        return self._col_stats(load().mlggd_output_stats, lambda K: 4, inp, targ)

    def output_stats_frames(self, feat, targ, first_frame, fea_context, targ_offset):
        """The same over a frame-stream chunk (mlggd_output_stats_frames): the same bits for the same rows."""
        return self._col_stats_frames(load().mlggd_output_stats_frames, lambda K: 4, feat, targ, first_frame, fea_context,
                                      targ_offset)

    def forward_frames(self, feat, first_frame, fea_context):
        feat, _, first = self._frames_args(feat, None, first_frame, fea_context)
        out = np.empty((first.size, self.D), np.float32)
        _check(load().mlggd_forward_frames(self._h, feat.shape[0], int(fea_context), _p(feat), first.size,
                                           first.ctypes.data_as(C.POINTER(C.c_int32)), _p(out)))
        return out

    # -- the same on a NAT engine: a stream row is K0 / (fea_context + 1) wide, nat [n_nat][that] is the noise table and
    # nat_row[i] the noise row of sample i (mlggd_*_frames_nat)
    def _frames_nat_args(self, feat, targ, first_frame, fea_context, nat, nat_row):
        feat = _f32(feat)
        first = np.ascontiguousarray(first_frame, dtype=np.int32)
        if feat.ndim != 2 or feat.shape[1] * (fea_context + 1) != self.K0:
            raise ValueError("feat must be [n_frames][%d/(fea_context+1)]" % self.K0)
        if targ is not None:
            targ = _f32(targ, (feat.shape[0], self.D))
        nat = _f32(nat)
        rows = np.ascontiguousarray(nat_row, dtype=np.int32)
        if nat.ndim != 2 or nat.shape[1] != feat.shape[1]:
            raise ValueError("nat must be [n_nat][%d]" % feat.shape[1])
        if rows.shape != first.shape or first.ndim != 1:
            raise ValueError("nat_row holds one index per sample of first_frame")
        return feat, targ, first, nat, rows

    def load_frames_nat(self, feat, targ, first_frame, fea_context, targ_offset, nat, nat_row):
        feat, targ, first, nat, rows = self._frames_nat_args(feat, targ, first_frame, fea_context, nat, nat_row)
        _check(load().mlggd_load_frames_nat(self._h, feat.shape[0], int(fea_context), _p(feat),
                                            _p(targ) if targ is not None else None, first.size, _i32p(first),
                                            int(targ_offset), nat.shape[0], _p(nat), _i32p(rows)))

    def train_frames_nat(self, feat, targ, first_frame, fea_context, targ_offset, nat, nat_row):
        feat, targ, first, nat, rows = self._frames_nat_args(feat, targ, first_frame, fea_context, nat, nat_row)
        trained = C.c_int(0)
        _check(load().mlggd_train_frames_nat(self._h, feat.shape[0], int(fea_context), _p(feat), _p(targ), first.size,
                                             _i32p(first), int(targ_offset), nat.shape[0], _p(nat), _i32p(rows),
                                             C.byref(trained)))
        return trained.value

    def cv_all_frames_nat(self, feat, targ, first_frame, fea_context, targ_offset, nat, nat_row):
        feat, targ, first, nat, rows = self._frames_nat_args(feat, targ, first_frame, fea_context, nat, nat_row)
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(load().mlggd_cv_all_frames_nat(self._h, feat.shape[0], int(fea_context), _p(feat), _p(targ), first.size,
                                              _i32p(first), int(targ_offset), nat.shape[0], _p(nat), _i32p(rows),
                                              C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def forward_frames_nat(self, feat, first_frame, fea_context, nat, nat_row):
        feat, _, first, nat, rows = self._frames_nat_args(feat, None, first_frame, fea_context, nat, nat_row)
        out = np.empty((first.size, self.D), np.float32)
        _check(load().mlggd_forward_frames_nat(self._h, feat.shape[0], int(fea_context), _p(feat), first.size,
                                               _i32p(first), nat.shape[0], _p(nat), _i32p(rows), _p(out)))
        return out

    def sync(self):
        _check(load().mlggd_sync(self._h))

    # -- training data from waves: the wave pair (or the clean wave and the noise bank) is analysed, normalised and
    # handed to the training loop on the device (mlggd_load_waves, mlggd_cv_all_waves, mlggd_train_waves)
    def _waves_args(self, cleans, mean, inv_std, first_frame, fea_context, fs_khz):
        cleans = [_wave(w) for w in cleans]
        D = SPECTRAL_PARAMS.get(int(fs_khz), (0, 0, 2 * self.D - 2))[2] // 2 + 1
        if fea_context is None:
            fea_context = self.K0 // D - (1 if self._nat else 0)  # a NAT engine's last D inputs are the noise row
        first = np.ascontiguousarray(first_frame, dtype=np.int32)
        if first.ndim != 1:
            raise ValueError("first_frame is a 1-D table of frame indices")
        packed = np.concatenate(cleans) if cleans else np.zeros(0, np.int16)
        return (packed, _offsets([w.size for w in cleans]), _f32(mean, (D,)), _f32(inv_std, (D,)), first,
                int(fea_context))

    def _pair_args(self, noisys, cleans, mean, inv_std, first_frame, targ_offset, fea_context, fs_khz):
        clean, off, mean, inv, first, ctx = self._waves_args(cleans, mean, inv_std, first_frame, fea_context, fs_khz)
        noisys = [_wave(w) for w in noisys]
        if [w.size for w in noisys] != list(np.diff(off)):
            raise ValueError("one noisy wave per clean wave, of the same length")
        noisy = np.concatenate(noisys) if noisys else np.zeros(0, np.int16)
        return (self._h, int(fs_khz), ctx, _p(mean), _p(inv), off.size - 1, _sp(noisy), _sp(clean), _i64p(off),
                first.size, first.ctypes.data_as(C.POINTER(C.c_int32)), int(targ_offset))

    def load_waves(self, noisys, cleans, mean, inv_std, first_frame, targ_offset, fea_context=None, fs_khz=16):
        """load_frames from a wave pair: afterwards train_resident indexes the samples of first_frame (a table of
        wave_samples, permuted as the caller likes).  fea_context None: layersizes[0] / bins."""
        _check(load().mlggd_load_waves(*self._pair_args(noisys, cleans, mean, inv_std, first_frame, targ_offset,
                                                        fea_context, fs_khz)))

    def cv_all_waves(self, noisys, cleans, mean, inv_std, first_frame, targ_offset, fea_context=None, fs_khz=16):
        """cv_all_frames from a wave pair: (sqerr, abserr, loglik), the same bits as on the rows built on the host."""
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(load().mlggd_cv_all_waves(*self._pair_args(noisys, cleans, mean, inv_std, first_frame, targ_offset,
                                                          fea_context, fs_khz), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_noise(self, noise):
        """The noise bank of train_waves, kept on the device between calls; None frees it (mlggd_set_noise)."""
        if noise is None:
            _check(load().mlggd_set_noise(self._h, 0, None))
            self._n_noise = 0
            return
        noise = _wave(noise)
        _check(load().mlggd_set_noise(self._h, noise.size, _sp(noise)))
        self._n_noise = noise.size

    def train_waves(self, cleans, snr_db, noise_start, mean, inv_std, first_frame, targ_offset, noise_seg=None,
                    fea_context=None, fs_khz=16, return_noisy=False):
        """Mix cleans[u] with the noise bank at snr_db[u] (mix_waves' arguments and rule), analyse both waves, load and
        train in one pass on the device (mlggd_train_waves).  Returns the number of bunches trained; with return_noisy
        (bunches, noisy waves, gain, clipped) -- mix_waves' bytes."""
        clean, off, mean, inv, first, ctx = self._waves_args(cleans, mean, inv_std, first_frame, fea_context, fs_khz)
        n = off.size - 1
        snr, start, lo, ln = _mix_args(n, self._n_noise, snr_db, noise_start, noise_seg)
        out = np.zeros(clean.size, np.int16) if return_noisy else None
        gain, clipped = np.zeros(n, np.float64), np.zeros(n, np.int32)
        trained = C.c_int(0)
        _check(load().mlggd_train_waves(self._h, int(fs_khz), ctx, _p(mean), _p(inv), n, _sp(clean), _i64p(off),
                                        _i64p(lo), _i64p(ln), _i64p(start), snr.ctypes.data_as(C.POINTER(C.c_double)),
                                        first.size, first.ctypes.data_as(C.POINTER(C.c_int32)), int(targ_offset),
                                        _sp(out) if return_noisy else None,
                                        gain.ctypes.data_as(C.POINTER(C.c_double)) if return_noisy else None,
                                        clipped.ctypes.data_as(C.POINTER(C.c_int32)) if return_noisy else None,
                                        C.byref(trained)))
        if return_noisy:
            return trained.value, [out[off[u]:off[u + 1]] for u in range(n)], gain, clipped
        return trained.value

    # -- Test_code/decode.m on the device: noisy wave -> LPS -> normalise -> context -> forward -> de-normalise -> wave
    def enhance_wave(self, noisy, mean, inv_std, fea_context=7, fs_khz=16, return_float=False):
        noisy = _wave(noisy)
        L, S, N = SPECTRAL_PARAMS[int(fs_khz)]
        mean = _f32(mean, (N // 2 + 1,))
        inv = _f32(inv_std, (N // 2 + 1,))
        F = max(0, (noisy.size - (L - S)) // S)
        out = np.empty(F * S + L - S, np.int16)
        outf = np.empty(out.size, np.float32) if return_float else None
        n = C.c_int(0)
        _check(load().mlggd_enhance_wave(self._h, int(fs_khz), int(fea_context), _p(mean), _p(inv), noisy.size,
                                         _sp(noisy), _sp(out), _p(outf) if return_float else None, C.byref(n)))
        return (out, outf) if return_float else out

    def enhance_waves(self, waves, mean, inv_std, fs_khz=16, fea_context=None, return_f32=False, return_lps=False,
                      cleans=None, score_frames=None, stoi=False, stoi_samples=None):
        """enhance_wave over a list of int16 waves in one pass over the device (mlggd_enhance_waves): a list of int16
        arrays, each bit-equal to enhance_wave on that wave alone; with return_f32 / return_lps a tuple of lists, the
        float32 waves before the cast and the de-normalised network outputs [F_u][D] added in that order.
        fea_context None: layersizes[0] / bins.  With cleans (one clean wave per utterance, cut or zero-padded to the
        noisy wave's length) the quality report of the same pass (mlggd_enhance_waves_scored) is added at the end of
        the tuple: segsnr [n] and lsd [n] float32, over the leading score_frames[u] frames of each utterance (None:
        all; 0: not scored, both 0).  With stoi=True (needs cleans) stoi [n] float32 follows them: the STOI of the
        pass's own int16 output against the clean wave (mlggd_enhance_waves_scored_stoi; stoi_waves on the same waves
        bit for bit), over the leading stoi_samples[u] samples (None: as many as the clean and the noisy wave both
        have); NaN where the utterance has no value."""
        if stoi and cleans is None:
            raise ValueError("stoi=True needs the clean waves")
        waves = [_wave(w) for w in waves]
        L, S, N = SPECTRAL_PARAMS[int(fs_khz)]
        D = N // 2 + 1
        mean = _f32(mean, (D,))
        inv = _f32(inv_std, (D,))
        if fea_context is None:
            fea_context = self.K0 // D - (1 if self._nat else 0)  # a NAT engine's last D inputs are the noise row
        frames, frame_off, out_off = enhance_waves_layout([w.size for w in waves], fs_khz)
        n = len(waves)
        packed = np.concatenate(waves) if n else np.zeros(0, np.int16)
        off = _offsets([w.size for w in waves])
        out = np.empty(int(out_off[-1]), np.int16)
        outf = np.empty(out.size, np.float32) if return_f32 else None
        lps = np.empty((int(frame_off[-1]), D), np.float32) if return_lps else None
        if cleans is None:
            _check(load().mlggd_enhance_waves(self._h, int(fs_khz), int(fea_context), _p(mean), _p(inv), n, _sp(packed),
                                              off.ctypes.data_as(C.POINTER(C.c_int64)), _sp(out),
                                              _p(outf) if return_f32 else None, _p(lps) if return_lps else None))
        else:
            clean = _clean_like(cleans, waves)
            sf = _score_frames(score_frames, n)
            segsnr, lsd = np.zeros(n, np.float32), np.zeros(n, np.float32)
            args = (self._h, int(fs_khz), int(fea_context), _p(mean), _p(inv), n, _sp(packed), _sp(clean),
                    off.ctypes.data_as(C.POINTER(C.c_int64)),
                    sf.ctypes.data_as(C.POINTER(C.c_int32)) if sf is not None else None, _sp(out),
                    _p(outf) if return_f32 else None, _p(lps) if return_lps else None, _p(segsnr), _p(lsd))
            if stoi:
                ss = _stoi_samples(stoi_samples, n)
                if ss is None:
                    ss = np.array([min(_wave(c).size, w.size) for c, w in zip(cleans, waves)], np.int64).reshape(n)
                stoi_v = np.zeros(n, np.float32)
                _check(load().mlggd_enhance_waves_scored_stoi(*args, ss.ctypes.data_as(C.POINTER(C.c_int64)),
                                                              _p(stoi_v), None))
            else:
                _check(load().mlggd_enhance_waves_scored(*args))
        res = [[out[out_off[u]:out_off[u + 1]] for u in range(n)]]
        if return_f32:
            res.append([outf[out_off[u]:out_off[u + 1]] for u in range(n)])
        if return_lps:
            res.append([lps[frame_off[u]:frame_off[u + 1]] for u in range(n)])
        if cleans is not None:
            res += [segsnr, lsd]
            if stoi:
                res.append(stoi_v)
        return res[0] if len(res) == 1 else tuple(res)

    def live(self, mean, inv_std, n_sessions, fs_khz=16, fea_context=None):
        """A live group of n_sessions sessions on this engine (mlggd_live_open): push(blocks, end=None,
        return_f32=False), received(), close(); BPGpu.close() closes it too.  fea_context None: layersizes[0] / bins."""
        return LiveGroup(self, mean, inv_std, n_sessions, fs_khz, fea_context)

    def rbm(self, layer, visible="gaussian", lrate=0.001, momentum=0.5, weightcost=0.0002, seed=1):
        """Open a CD-1 pre-training session (Rbm, a context manager) on hidden layer `layer` = 1 .. numlayers - 2:
        "gaussian" visibles for layer 1 on z-normalised input, "bernoulli" above.  The default rates are a choice of this
        project, not a measured optimum.  One session per engine at a time; dropout flags are ignored."""
        return Rbm(self, layer, visible, lrate, momentum, weightcost, seed)

    def last_train_ms(self):
        ms, steps = C.c_float(0), C.c_int(0)
        _check(load().mlggd_last_train_ms(self._h, C.byref(ms), C.byref(steps)))
        return ms.value, steps.value

    # -- BP_GPU::CrossValid / CrossValiddB / CrossValid2 / cv_bunch_single
    def _cv(self, fn, inp, targ):
        inp = _f32(inp)
        targ = _f32(targ)
        out = C.c_float(0)
        _check(fn(self._h, inp.shape[0], _p(inp), _p(targ), C.byref(out)))
        return out.value

    def CrossValid(self, inp, targ):
        return self._cv(load().mlggd_cv_sqerr, inp, targ)

    def CrossValiddB(self, inp, targ):
        return self._cv(load().mlggd_cv_abserr, inp, targ)

    def CrossValid2(self, inp, targ):
        return self._cv(load().mlggd_cv_loglik, inp, targ)

    def cv_all(self, inp, targ):
        inp = _f32(inp)
        targ = _f32(targ)
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(load().mlggd_cv_all(self._h, inp.shape[0], _p(inp), _p(targ), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def forward(self, inp):
        inp = _f32(inp)
        out = np.empty((inp.shape[0], self.D), np.float32)
        _check(load().mlggd_forward(self._h, inp.shape[0], _p(inp), _p(out)))
        return out

    # -- BP_GPU::returnWeights and friends
    def returnWeights(self):
        ws = [np.empty((self.layersizes[l], self.layersizes[l + 1]), np.float32) for l in range(self.numlayers - 1)]
        bs = [np.empty(self.layersizes[l + 1], np.float32) for l in range(self.numlayers - 1)]
        _check(load().mlggd_get_weights(self._h, _ptr_array(ws), _ptr_array(bs)))
        return ws, bs

    def set_weights(self, weights, bias):
        ws = [_f32(w, (self.layersizes[l], self.layersizes[l + 1])) for l, w in enumerate(weights)]
        bs = [_f32(b, (self.layersizes[l + 1],)) for l, b in enumerate(bias)]
        _check(load().mlggd_set_weights(self._h, _ptr_array(ws), _ptr_array(bs)))

    def scalefactor(self):
        a = np.empty(self.D, np.float32)
        _check(load().mlggd_get_scalefactor(self._h, _p(a)))
        return a

    def set_scalefactor(self, alpha):
        a = _f32(alpha, (self.D,))
        _check(load().mlggd_set_scalefactor(self._h, _p(a)))

    def set_scale_mode(self, mode="learned", lrate=0.05, momentum=0.5, vmax=1.0):
        """How the GGD scale alpha_d is found (MLflag 1 only; csrc/scale_rule.h, mlggd_set_scale_mode).  "alternating",
        the default of every engine: the closed form of each minibatch.  "learned": alpha_d is a state that lives across
        minibatches and ln alpha_d moves by SGD with momentum beside the weights, v' = momentum v - lrate (1 - beta S /
        alpha^beta) clamped to [-vmax, vmax], alpha' = alpha exp(v'); entering it takes alpha from the current
        scalefactor (0: the bin seeds from its first minibatch) and v = 0.  lrate = momentum = 0 trains under a fixed
        scale.  The default rates are a choice, not a measured optimum."""
        _check(load().mlggd_set_scale_mode(self._h, scale_mode_code(mode), float(lrate), float(momentum), float(vmax)))

    def scale_mode(self):
        """ScaleMode(mode, lrate, momentum, vmax, steps) in effect (mlggd_get_scale_mode); steps counts the learned steps
        since the mode was entered."""
        m, st = C.c_int(0), C.c_int64(0)
        lr, mo, vm = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(load().mlggd_get_scale_mode(self._h, C.byref(m), C.byref(lr), C.byref(mo), C.byref(vm), C.byref(st)))
        return ScaleMode(SCALE_MODES[m.value], lr.value, mo.value, vm.value, st.value)

    def scale_state(self):
        """(alpha, velocity), [D] float32 each: the learned scale's state the next step reads (mlggd_get_scale_state)."""
        a, v = np.empty(self.D, np.float32), np.empty(self.D, np.float32)
        _check(load().mlggd_get_scale_state(self._h, _p(a), _p(v)))
        return a, v

    def set_scale_state(self, alpha, velocity=None):
        """Set the learned scale's state; velocity None: zeros.  alpha must be finite and not negative, 0 meaning "seed
        from the next minibatch" (mlggd_set_scale_state)."""
        a = _f32(alpha, (self.D,))
        v = None if velocity is None else _f32(velocity, (self.D,))
        _check(load().mlggd_set_scale_state(self._h, _p(a), None if v is None else _p(v)))

    def set_optimizer(self, name="adam", beta1=0.9, beta2=0.999, eps=1e-8):
        """The weight rule of the steps to come (csrc/adam_rule.h, mlggd_set_optimizer).  "sgd", the default of every
        engine: the reference's SGD with momentum and L2.  "adam": two moments per weight and bias on the device, g = G / n
        + weightcost w, m' = beta1 m + (1 - beta1) g, v' = beta2 v + (1 - beta2) g g, w' = w - a_t m' / (sqrt(v') + eps)
        with the bias correction in a_t; lrate (and set_lrate) is the Adam rate, momentum is ignored.  Entering "adam"
        -- also from "adam" -- zeroes the moments and the step count; the SGD momentum buffers are left alone, so "sgd"
        continues from the deltas it had.  Single device only.  No default here has been evaluated on speech."""
        _check(load().mlggd_set_optimizer(self._h, optimizer_code(name), float(beta1), float(beta2), float(eps)))

    def optimizer(self):
        """Optimizer(name, beta1, beta2, eps, steps) in effect (mlggd_get_optimizer); steps counts the Adam updates."""
        k, st = C.c_int(0), C.c_int64(0)
        b1, b2, ep = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(load().mlggd_get_optimizer(self._h, C.byref(k), C.byref(b1), C.byref(b2), C.byref(ep), C.byref(st)))
        return Optimizer(OPTIMIZERS[k.value], b1.value, b2.value, ep.value, st.value)

    def optimizer_state(self):
        """OptimizerState(m_w, v_w, m_b, v_b, steps): the Adam moments of every layer, unpadded, in returnWeights' shapes
        (mlggd_get_optimizer_state)."""
        ls = self.layersizes[:self.numlayers]
        (m_w, m_b), (v_w, v_b) = _moment_arrays(ls), _moment_arrays(ls)
        _check(load().mlggd_get_optimizer_state(self._h, _ptr_array(m_w), _ptr_array(v_w), _ptr_array(m_b), _ptr_array(v_b)))
        return OptimizerState(m_w, v_w, m_b, v_b, self.optimizer().steps)

    def set_optimizer_state(self, m_w, v_w, m_b, v_b, steps):
        """Set the Adam moments and the number of updates they stand for (mlggd_set_optimizer_state): with the weights,
        what a run needs to continue as if it had not been interrupted."""
        n = self.numlayers - 1
        ws = lambda g: [_f32(a, (self.layersizes[l], self.layersizes[l + 1])) for l, a in enumerate(g)]
        bs = lambda g: [_f32(a, (self.layersizes[l + 1],)) for l, a in enumerate(g)]
        if not (len(m_w) == len(v_w) == len(m_b) == len(v_b) == n):
            raise ValueError("expected %d arrays of each kind" % n)
        mw, vw, mb, vb = ws(m_w), ws(v_w), bs(m_b), bs(v_b)
        _check(load().mlggd_set_optimizer_state(self._h, _ptr_array(mw), _ptr_array(vw), _ptr_array(mb), _ptr_array(vb), int(steps)))

    def shapefactors(self):
        """The D shapes in effect: the vector of set_shapefactors, else `shapefactor` D times."""
        b = np.empty(self.D, np.float32)
        _check(load().mlggd_get_shapefactors(self._h, _p(b)))
        return b

    def set_shapefactors(self, betas):
        """One shape per output bin from the next step or CV call on (MLflag 1 only); None: back to `shapefactor`.
        Weights, momentum and the current scalefactor stay (mlggd_set_shapefactors)."""
        if betas is None:
            _check(load().mlggd_set_shapefactors(self._h, None))
            return
        b = _f32(betas, (self.D,))
        _check(load().mlggd_set_shapefactors(self._h, _p(b)))

    def gv(self):
        """The D equalisation factors in effect: the vector of set_gv, else ones."""
        e = np.empty(self.D, np.float32)
        _check(load().mlggd_get_gv(self._h, _p(e)))
        return e

    def set_gv(self, eta):
        """One global variance equalisation factor per output bin, applied by every wave decoder and live push from
        the next call on: v = ((y * eta) / inv_std) + mean.  None: off.  Weights, momentum, scalefactor and shape
        factors stay (mlggd_set_gv)."""
        if eta is None:
            _check(load().mlggd_set_gv(self._h, None))
            return
        e = _f32(eta, (self.D,))
        _check(load().mlggd_set_gv(self._h, _p(e)))

    def set_lrate(self, lrate):
        _check(load().mlggd_set_lrate(self._h, float(lrate)))

    def debug_tensor(self, name, layer=0):
        if name == "scalefactor":
            shape = (self.D,)
        elif name == "out":
            shape = (self.bunchsize, self.D)
        elif name in ("y", "dedx", "yt", "dedxt"):
            shape = (self.bunchsize, self.layersizes[layer])
        elif name in ("weights", "delta_w", "grad_w"):
            shape = (self.layersizes[layer - 1], self.layersizes[layer])
        elif name in ("bias", "delta_b", "grad_b"):
            shape = (self.layersizes[layer],)
        elif name == "adam_pads":  # counts of pad entries that are not zero: W, m_w, v_w, bias, m_b, v_b
            shape = (6,)
        else:
            raise KeyError(name)
        a = np.empty(shape, np.float32)
        _check(load().mlggd_debug_tensor(self._h, name.encode(), int(layer), _p(a), a.size))
        return a

    # -- data parallel
    def comm_init(self, unique_id, world_size, rank):
        buf = (C.c_char * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        _check(load().mlggd_comm_init(self._h, buf, int(world_size), int(rank)))

    # -- kernel-class timing
    def profile_select(self, kernel_class, layer=0, max_launches=4096, stride=1):
        kc = kernel_class.encode() if kernel_class else None
        _check(load().mlggd_profile_select(self._h, kc, int(layer), int(max_launches)))
        _check(load().mlggd_profile_stride(self._h, int(stride)))

    def profile_read(self):
        us, n = C.c_float(0), C.c_int(0)
        _check(load().mlggd_profile_read(self._h, C.byref(us), C.byref(n)))
        return us.value, n.value

    def profile_overhead(self):
        us = C.c_float(0)
        _check(load().mlggd_profile_overhead(self._h, C.byref(us)))
        return us.value

    def kernel_work(self, kernel_class, layer=0):
        f, b = C.c_double(0), C.c_double(0)
        _check(load().mlggd_kernel_work(self._h, kernel_class.encode(), int(layer), C.byref(f), C.byref(b)))
        return f.value, b.value

    def dw_launches_per_step(self):
        n = C.c_int(0)
        _check(load().mlggd_dw_launches_per_step(self._h, C.byref(n)))
        return n.value

    def dp_mode(self):
        """0 single device, 1 all-reduce of gradients, 2 all-gather of the gradient factors, 3 = 2 + sharded update,
        4 = 3 with the activations exchanged by all-to-all (each rank receives only its block's units)"""
        n = C.c_int(0)
        _check(load().mlggd_dp_mode(self._h, C.byref(n)))
        return n.value

    def out_slabs(self):
        """split-K slabs of the output-layer forward GEMM (the oracle's MFMA-order twin restates the same split)"""
        n = C.c_int(0)
        _check(load().mlggd_debug_out_slabs(self._h, C.byref(n)))
        return n.value

    def gemm_plan(self):
        """[(fwd_waves, dx_waves)] per layer 1..L-1: 4 = the 32 x 32-tile kernels (reduction over 4 waves), 1 = the
        64 x 64-tile kernels (one chain per output element)"""
        out = []
        for l in range(1, len(self.layersizes)):
            f, d = C.c_int(0), C.c_int(0)
            _check(load().mlggd_debug_gemm_plan(self._h, l, C.byref(f), C.byref(d)))
            out.append((f.value, d.value))
        return out

    def comm_info(self):
        """(ranks, rank) of the engine's RCCL communicator as RCCL reports them; (0, -1) without one."""
        n, r = C.c_int(0), C.c_int(-1)
        _check(load().mlggd_comm_info(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def debug_math(self, fn, x, y=0.0):
        """fn(x, y) elementwise on the device with the kernels' own libm ("powf" "expf" "sigmoid" "div")."""
        x = _f32(x).ravel()
        out = np.empty_like(x)
        _check(load().mlggd_debug_math(self._h, fn.encode(), _p(x), float(y), _p(out), x.size))
        return out

    def plan_count(self):
        n = C.c_int(0)
        _check(load().mlggd_debug_plan_count(self._h, C.byref(n)))
        return n.value

    def buffer_stats(self):
        """(allocations, bytes) of the engine's growable device buffers and of its open live groups: device allocations
        made since creation (never falls) and bytes held now.  A call that exceeds no capacity adds no allocation."""
        n, b = C.c_int64(0), C.c_int64(0)
        _check(load().mlggd_debug_buffers(self._h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def set_cv_device_reduce(self, on=True):
        """CV sums formed on the device (no n x D copy back) instead of the reference-order host loop."""
        _check(load().mlggd_set_cv_device_reduce(self._h, 1 if on else 0))

    def fake_world(self, world_size, sharded=False, allreduce=False, a2a=False):
        """Emulate world_size ranks on this GPU: every step consumes world_size*bunchsize rows, rank r owns
        rows [r*bunchsize,(r+1)*bunchsize) of them (test hook, mlggd_debug_fake_world)."""
        _check(load().mlggd_debug_fake_world(self._h, int(world_size), 3 if a2a else 2 if allreduce else 1 if sharded else 0))

    def keep_ranks(self, on=True):
        """From the next step on, keep what every emulated rank computed (test hook, mlggd_debug_keep_ranks)."""
        _check(load().mlggd_debug_keep_ranks(self._h, 1 if on else 0))

    def rank_tensor(self, name, layer=0, rank=0):
        """Rank `rank`'s "x" (input rows after input dropout), "y", "dedx" or "out" of the last step, [bunchsize][units]
        (test hook, mlggd_debug_rank_tensor)."""
        units = {"x": self.K0, "out": self.D}.get(name)
        if units is None:
            if name not in ("y", "dedx"):
                raise KeyError(name)
            units = self.layersizes[layer]
        a = np.empty((self.bunchsize, units), np.float32)
        _check(load().mlggd_debug_rank_tensor(self._h, name.encode(), int(layer), int(rank), _p(a), a.size))
        return a

    def stamp_select(self, kernel_class, layer):
        _check(load().mlggd_debug_stamp_select(self._h, kernel_class.encode(), int(layer)))

    def stamp_read(self, cap_blocks=8192):
        buf = np.zeros((cap_blocks, 8), np.int64)
        n = C.c_int(0)
        _check(load().mlggd_debug_stamp_read(self._h, buf.ctypes.data_as(C.POINTER(C.c_longlong)), cap_blocks,
                                             C.byref(n)))
        return buf[:n.value]


def shard_rows(global_frames, world_size, rank):
    """Row range [lo, hi) of a global minibatch that `rank` trains (SURVEY.md 8e partition)."""
    if global_frames % world_size:
        raise ValueError("global minibatch %d not divisible by world size %d" % (global_frames, world_size))
    per = global_frames // world_size
    return rank * per, (rank + 1) * per


def weight_row_block(in_units, world_size, rank):
    """Rows [lo, hi) of a layer's weight matrix W [in][out] that `rank` owns in the sharded updates (the `shard`,
    `shard_a2a` and `allreduce` exchanges; engine.hip shard_alloc): the ceil32-padded input width is cut into 64-row tile
    rows, ceil(tile rows / world) of them per rank; hi is clipped to the true width, so late ranks may own fewer rows or
    none.  Also the block of UNITS of the layer below that rank receives in the all-to-all form."""
    kp = (int(in_units) + 31) // 32 * 32
    tile_rows = (kp + 63) // 64
    per = (tile_rows + world_size - 1) // world_size
    lo = min(rank * per * 64, int(in_units))
    hi = min((rank + 1) * per * 64, int(in_units))
    return lo, hi
