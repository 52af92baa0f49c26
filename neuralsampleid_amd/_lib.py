"""ctypes binding of libnsid_hip.so (C ABI: include/nsid.h).

The product path has no CPU fallback: if the library is missing this module raises, and every op raises
RuntimeError on a non-zero return code."""
import ctypes
import os

import torch  # noqa: F401  -- must come first: torch bundles its own libamdhip64; loading the kernel library before it
#                              would bind the system HIP runtime and leave two runtimes in one process

_PKG = os.path.dirname(os.path.abspath(__file__))
# NSID_LIB: path of an alternative BUILD of the same library (one-box kernel A/B, tools/build_variant.sh). It selects which .so is
# loaded, nothing inside the library reads the environment; bench.py records an override in its JSON line (config.lib).
LIB_PATH = os.environ.get("NSID_LIB") or os.path.join(_PKG, "libnsid_hip.so")

# signature letters: p = device pointer, i = int, l = long, z = size_t, f = float, d = double, s = stream (void*)
SIGNATURES = {
    "nsid_set_gemm_precision": "i",
    "nsid_linear_fwd": "pipippiiiiippiipiis",
    "nsid_linear_fwd_res": "pipippipiiiiippiis",
    "nsid_linear_bwd_data": "pipipipiiiiiis",
    "nsid_linear_bwd_data_bn": "pipipipiiiiiipppppips",
    "nsid_linear_bwd_weight": "pipipiiiippiis",
    "nsid_linear_bwd_weight_grouped": "piiis",
    "nsid_colsum_acc": "piiipis",
    "nsid_bn_finalize": "piiipppppffpppps",
    "nsid_bn_finalize_deferred": "piiippfppppps",
    "nsid_bn_running_update": "ippppppppfs",
    "nsid_bn_eval_affine": "ppppfipps",
    "nsid_bn_apply": "pppippiiis",
    "nsid_bn_bwd_reduce": "ppiippppipis",
    "nsid_bn_bwd_finalize": "piiippps",
    "nsid_bn_bwd_apply": "ppiippppippis",
    "nsid_bn_bwd_finalize_fused": "piiipppppppps",
    "nsid_knn_graph": "pippiiiiipis",
    "nsid_mr_aggregate_fwd": "pipppiiiippis",
    "nsid_mr_aggregate_bwd": "pppiiiipis",
    "nsid_im2col3_fwd": "piiipis",
    "nsid_im2col3_bwd": "piiipis",
    "nsid_pack_ds_weight": "piips",
    "nsid_dsact_fwd": "piiippipppipppiis",
    "nsid_dsact_bwd_weight": "ppppipiiiiis",
    "nsid_dsact_bwd_data": "pppiiiipppppipis",
    "nsid_pack_ds_weight_bwd": "piips",
    "nsid_downsample3_fwd": "piiipippipis",
    "nsid_downsample3_bwd_weight": "pppiiiiis",
    "nsid_downsample3_bwd_data": "pppipiiiiis",
    "nsid_unpack_ds_wgrad": "piips",
    "nsid_ds_prepack": "ipppppps",
    "nsid_peak_patchify_fwd": "pppiiiiiipipis",
    "nsid_peak_patchify_bwd": "ppppiiiiiiippis",
    "nsid_peak_patchify_bwd_ws": "ppppiiiiiiipppis",
    "nsid_node_mean_fwd": "piiipis",
    "nsid_node_mean_bwd": "piiipis",
    "nsid_elu_bwd": "pplps",
    "nsid_l2norm_fwd": "piifpps",
    "nsid_l2norm_bwd": "pppiifps",
    "nsid_ntxent_fwd_bwd": "ppiifiipppps",
    "nsid_pair_ce_fwd_bwd": "ppiipppps",
    "nsid_triplet_fwd_bwd": "ppiidppps",
    "nsid_baseline_objective_fwd_bwd": "ppiidddpppps",
    "nsid_baseline_objective_rows_fwd_bwd": "ppiiiidddpppps",
    "nsid_sumsq_partial": "plps",
    "nsid_adam_step": "pppplpppips",
    "nsid_f32_to_bf16": "ppls",
    "nsid_reflect_pad": "plips",
    "nsid_power_mel_db": "plippiips",
    "nsid_unfold_segments": "piiiiips",
    "nsid_logmel_fft": "pliliippppiplls",
    "nsid_cqt": "pliliiipiplpplls",
    "nsid_logmel_fft_ragged": "ppillliippppipls",
    "nsid_cqt_ragged": "ppillliiipiplppls",
    "nsid_unfold_segments_ragged": "pliiplips",
    "nsid_aug_stft": "plplilpppps",
    "nsid_aug_vocoder": "pilpffpls",
    "nsid_aug_istft": "plilpffpppls",
    "nsid_aug_finish": "plilppffppls",
    "nsid_aug_compress": "plilpppls",
    "nsid_aug_biquad": "plilppippls",
    "nsid_aug_frames": "plplpilpppipls",
    "nsid_resample_sinc": "pliliiippiipls",
    "nsid_stem_pairs_gate": "plppipppppillfppps",
    "nsid_stem_pairs_build": "plppippppppilliiplplps",
    "nsid_bcn_to_rows": "piiipiis",
    "nsid_rows_to_bcn": "piiiipis",
    "nsid_batched_index_select_fwd": "ppiiiiips",
    "nsid_batched_index_select_bwd": "ppiiiiips",
    "nsid_fill_zero": "pzs",
    "nsid_scale_f32": "pplps",
    "nsid_row_sqnorm": "piiips",
    "nsid_flat_l2_topk": "piipiippiipppzs",
    "nsid_seq_scores": "pipiiipippipis",
    "nsid_clf_node_rows": "piiipps",
    "nsid_clf_pair_scores": "pipiipppiipppls",
    "nsid_clf_pair_scores_c": "pipiiipppiipppls",
    "nsid_clf_node_rows_n": "piiipps",
    "nsid_clf_pair_scores_n": "pipiiipppiipppls",
    "nsid_song_vote": "pipippipiipippps",
    "nsid_song_vote_clf": "pipppppipiipfippps",
    "nsid_vote_candidates": "pliips",
    "nsid_clf_mine_hard_negatives": "pipiiips",
    "nsid_clf_attn_fwd": "pipiippippps",
    "nsid_clf_head_fwd": "ppppips",
    "nsid_clf_head_bwd": "pppppipppps",
    "nsid_clf_attn_bwd": "pppipiippipps",
    "nsid_clf_seg_reduce": "ppppppiiiipps",
    "nsid_clf_attn_fwd_c": "pipiiippippps",
    "nsid_clf_attn_bwd_c": "pppipiiippipps",
    "nsid_clf_seg_reduce_c": "ppppppiiiiipps",
    "nsid_conv2d_fwd": "piiiipipppiiiiis",
    "nsid_ibn_relu_fwd": "piiippfpppis",
    "nsid_stem7_pool_fwd": "piiipppis",
    "nsid_gem_pool_fwd": "piiipfpis",
    "nsid_gem_pool_bwd": "ppiiipfpppis",
    "nsid_conv2d_bwd_data": "piiiipippiiiis",
    "nsid_conv2d_bwd_weight": "ppiiiippiiiis",
    "nsid_col_stat": "piiipis",
    "nsid_ibn_relu_bwd": "ppiiippfppppppppppis",
    "nsid_bn_add_relu_fwd": "pppppppiiis",
    "nsid_relu_bwd": "ppplis",
    "nsid_stem7_stat": "piiipps",
    "nsid_stem7_pool_train_fwd": "piiipppppis",
    "nsid_stem7_bwd": "pipiiipppppppppps",
}

class WgradProblem(ctypes.Structure):
    """include/nsid.h nsid_wgrad_problem: one layer's weight gradient over up to two row segments (the two views)"""
    _fields_ = [("dout", ctypes.c_void_p * 2), ("x", ctypes.c_void_p * 2), ("in_scale", ctypes.c_void_p * 2),
                ("in_shift", ctypes.c_void_p * 2), ("dw", ctypes.c_void_p), ("ldd", ctypes.c_int), ("ldx", ctypes.c_int),
                ("M", ctypes.c_int), ("Nout", ctypes.c_int), ("K", ctypes.c_int), ("groups", ctypes.c_int), ("act_in", ctypes.c_int),
                ("ds_out_nodes", ctypes.c_int)]


_CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "d": ctypes.c_double, "s": ctypes.c_void_p,
       "z": ctypes.c_size_t}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m neuralsampleid_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, sig in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = [_CT[c] for c in sig]
        fn.restype = ctypes.c_int
    lib.nsid_version.restype = ctypes.c_int
    if lib.nsid_version() < 0:      # (builds of rounds 3-4 with result-changing timing switches reported a negative version)
        raise ImportError(f"{LIB_PATH} reports a negative version: not a product build of this tree; rebuild with "
                          "`python -m neuralsampleid_amd.build --force`")
    lib.nsid_debug_gemm_trace.argtypes = [ctypes.c_void_p]
    lib.nsid_debug_gemm_trace.restype = ctypes.c_int
    lib.nsid_debug_knn_trace.argtypes = [ctypes.c_void_p]
    lib.nsid_debug_knn_trace.restype = ctypes.c_int
    lib.nsid_get_gemm_precision.restype = ctypes.c_int
    lib.nsid_gemm_g256_launches.argtypes = []
    lib.nsid_gemm_g256_launches.restype = ctypes.c_long
    lib.nsid_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_long]
    lib.nsid_set_tuning.restype = ctypes.c_int
    lib.nsid_get_tuning.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]
    lib.nsid_get_tuning.restype = ctypes.c_int
    lib.nsid_reset_tuning.argtypes = []
    lib.nsid_reset_tuning.restype = ctypes.c_int
    lib.nsid_workspace_bytes.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_long]
    lib.nsid_workspace_bytes.restype = ctypes.c_long
    lib.nsid_tuning_count.argtypes = []
    lib.nsid_tuning_count.restype = ctypes.c_int
    lib.nsid_tuning_key.argtypes = [ctypes.c_int]
    lib.nsid_tuning_key.restype = ctypes.c_char_p
    lib.nsid_debug_counter.argtypes = [ctypes.c_char_p]
    lib.nsid_debug_counter.restype = ctypes.c_long
    lib.nsid_debug_counters_reset.argtypes = []
    lib.nsid_debug_counters_reset.restype = ctypes.c_int
    lib.nsid_debug_counter_count.argtypes = []
    lib.nsid_debug_counter_count.restype = ctypes.c_int
    lib.nsid_debug_counter_key.argtypes = [ctypes.c_int]
    lib.nsid_debug_counter_key.restype = ctypes.c_char_p
    # returns 1 (nothing launched) for shapes outside the fused form: bound directly, not through call()
    lib.nsid_linear_bwd_data_bnapply.argtypes = [_CT[c] for c in "pppippipipiiiiiipppppips"]
    lib.nsid_linear_bwd_data_bnapply.restype = ctypes.c_int
    lib.nsid_mr_aggregate_bwd_bn.argtypes = [_CT[c] for c in "pppiiiippippppipis"]     # declines with NSID_EINVAL outside its form: the caller falls back
    lib.nsid_mr_aggregate_bwd_bn.restype = ctypes.c_int
    lib.nsid_ffn_fused_fwd.argtypes = [_CT[c] for c in "ppppppiiis"]
    lib.nsid_ffn_fused_fwd.restype = ctypes.c_int
    lib.nsid_mrconv_fused_fwd.argtypes = [_CT[c] for c in "ppiiiippps"]
    lib.nsid_mrconv_fused_fwd.restype = ctypes.c_int
    lib.nsid_row_tiles.argtypes = [ctypes.c_int]
    lib.nsid_row_tiles.restype = ctypes.c_int
    lib.nsid_dsact_part_rows.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.nsid_dsact_part_rows.restype = ctypes.c_int
    lib.nsid_sumsq_blocks.argtypes = [ctypes.c_long]
    lib.nsid_sumsq_blocks.restype = ctypes.c_int
    lib.nsid_ntxent_ws_floats.argtypes = [ctypes.c_int]
    lib.nsid_ntxent_ws_floats.restype = ctypes.c_size_t
    lib.nsid_baseline_loss_ws_floats.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.nsid_baseline_loss_ws_floats.restype = ctypes.c_size_t
    lib.nsid_baseline_loss_rows_ws_floats.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.nsid_baseline_loss_rows_ws_floats.restype = ctypes.c_size_t
    lib.nsid_conv2d_wgrad_splits.argtypes = [ctypes.c_long, ctypes.c_long]
    lib.nsid_conv2d_wgrad_splits.restype = ctypes.c_int
    lib.nsid_stem7_partials.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_int]
    lib.nsid_stem7_partials.restype = ctypes.c_long
    lib.nsid_stem7_bwd_set_floats.argtypes = []
    lib.nsid_stem7_bwd_set_floats.restype = ctypes.c_long
    return lib


lib = _load()
EXPORTS = list(SIGNATURES) + ["nsid_version", "nsid_debug_gemm_trace", "nsid_debug_knn_trace", "nsid_get_gemm_precision", "nsid_gemm_g256_launches", "nsid_linear_bwd_data_bnapply", "nsid_mr_aggregate_bwd_bn", "nsid_ffn_fused_fwd", "nsid_mrconv_fused_fwd", "nsid_debug_counter", "nsid_debug_counters_reset", "nsid_debug_counter_count", "nsid_debug_counter_key", "nsid_set_tuning", "nsid_get_tuning", "nsid_reset_tuning", "nsid_tuning_count", "nsid_tuning_key", "nsid_row_tiles", "nsid_dsact_part_rows", "nsid_sumsq_blocks", "nsid_ntxent_ws_floats", "nsid_baseline_loss_ws_floats", "nsid_baseline_loss_rows_ws_floats", "nsid_conv2d_wgrad_splits", "nsid_stem7_partials", "nsid_stem7_bwd_set_floats", "nsid_workspace_bytes"]

_ERR = {-1: "NSID_EINVAL (unsupported shape, misaligned pointer or bad argument)",
        -2: "NSID_ELAUNCH (HIP runtime refused the launch)"}


def call(name, *args):
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {_ERR.get(rc, rc)}")


def set_tuning(key: str, value: int) -> None:
    """one launch-heuristic constant of the kernel library (include/nsid.h nsid_set_tuning; keys: tuning_keys())"""
    if lib.nsid_set_tuning(key.encode(), int(value)) != 0:
        raise KeyError(f"unknown tuning key {key!r}; known: {', '.join(tuning_keys())}")


def get_tuning(key: str) -> int:
    v = ctypes.c_long()
    if lib.nsid_get_tuning(key.encode(), ctypes.byref(v)) != 0:
        raise KeyError(f"unknown tuning key {key!r}")
    return int(v.value)


def reset_tuning() -> None:
    lib.nsid_reset_tuning()


def launch_counters(reset: bool = False) -> dict:
    """launches per kernel variant since the last reset (include/nsid.h nsid_debug_counter)"""
    out = {}
    for i in range(lib.nsid_debug_counter_count()):
        k = lib.nsid_debug_counter_key(i)
        out[k.decode()] = int(lib.nsid_debug_counter(k))
    if reset:
        lib.nsid_debug_counters_reset()
    return out


def tuning_keys():
    return [lib.nsid_tuning_key(i).decode() for i in range(lib.nsid_tuning_count())]
