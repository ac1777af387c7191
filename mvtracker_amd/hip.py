"""ctypes binding of libmvtracker_hip.so (C ABI in include/mvtracker_hip.h).

The library is the product: there is NO eager / CPU fallback.  Importing this module loads the
shared object and raises ``RuntimeError`` if it is missing (build it with
``python -m mvtracker_amd.build``); every wrapper raises on a non-zero return code.  PyTorch only
provides device memory and the current HIP stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVT_LIB") or os.path.join(_HERE, "lib", "libmvtracker_hip.so")  # MVT_LIB: A/B builds of the same ABI

if not os.path.exists(LIB_PATH):
    raise RuntimeError(
        f"{LIB_PATH} not found: the HIP library is required (no fallback path exists). "
        "Build it with `python -m mvtracker_amd.build`.")
_lib = C.CDLL(LIB_PATH)

P, I, LL, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float

# name -> argument types (all return int unless listed in _RET)
SIGNATURES = {
    "mvt_abi_version": [],
    "mvt_build_arch": [],
    "mvt_gemm": [P, I, P, I, P, P, I, P, I, I, I, I, I, P],
    "mvt_conv2d": [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P],
    "mvt_split_bf16": [P, P, P, LL, P],
    "mvt_gemm_bf16": [P, I, P, P, I, P, P, I, P, I, I, I, I, I, I, P],
    "mvt_conv2d_stat_slots": [I, I, I, I, I, I, I, I],
    "mvt_conv2d_bf16": [P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, P, P],
    "mvt_conv3x3s2_down_bf16": [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, P],
    "mvt_instnorm_finish_slots": [P, I, P, I, LL, I, P],
    "mvt_ln_gemm_bf16": [P, I, P, P, F, P, P, I, P, P, I, P, I, I, I, I, I, P],
    "mvt_pack_frag_bf16": [P, I, I, I, P, P],
    "mvt_block_fused_bf16": [P, I, P, I, I, I, P, I, P, P, I, P, P, I, P, I, P, I, LL, I, P, P],
    "mvt_mlp_fused_bf16": [P, I, P, I, P, P, I, P, LL, I, I, F, P],
    "mvt_rgb_to_nhwc4": [P, P, I, I, I, I, I, I, P],
    "mvt_rgb_u8_to_nhwc4": [P, P, I, I, I, I, I, I, P],
    "mvt_rgb_images_to_nhwc4": [P, I, P, I, I, I, I, LL, I, P],
    "mvt_resize_nearest": [P, P, LL, I, I, I, I, P],
    "mvt_instnorm_stats": [P, I, P, P, I, LL, I, I, P],
    "mvt_instnorm_apply": [P, P, P, P, P, I, LL, I, I, P],
    "mvt_resize_bilinear_ac": [P, P, I, I, I, I, I, I, I, I, I, P],
    "mvt_concat_resize_bilinear_ac": [I, P, P, P, P, P, I, I, I, I, I, P],
    "mvt_invert_cameras": [P, P, P, P, I, P],
    "mvt_depth_subsample": [P, P, I, I, I, I, I, P],
    "mvt_avgpool2": [P, P, LL, I, I, I, I, P],
    "mvt_unproject": [P, P, P, P, I, I, I, I, I, I, P],
    "mvt_tile_aabb": [P, LL, I, I, I, P, P],
    "mvt_knn_scan": [P, LL, P, I, I, I, I, I, I, I, I, I, I, P, P, I, I, I, I, I, P, I, I, P],
    "mvt_knn_merge": [P, I, I, I, I, LL, P, P],
    "mvt_ln_proj_bf16": [P, I, P, I, LL, I, P],
    "mvt_input_proj_bf16": [P, I, I, LL, P, P, P, I, P, I, P, I, LL, I, P],
    "mvt_adapter_best_view": [P, P, P, P, I, I, I, I, I, P, P, P],
    "mvt_knn_scan_levels": [I, P, P, I, I, I, I, I, I, I, I, I, I, P],
    "mvt_knn_search_levels": [I, P, P, I, I, I, I, I, I, I, I, I, I, P],
    "mvt_knn_search": [P, LL, P, I, I, I, I, I, I, I, I, I, P, I, I, I, I, I, P, P, I, I, P, P],
    "mvt_tile_group_aabb": [P, LL, I, P, P],
    "mvt_knn_merge_levels": [I, P, I, I, I, P],
    "mvt_corr_gather_dot": [I, P, P, I, P, P, I, P, P, I, I, I, I, I, I, I, I, I, P, I, I, P],
    "mvt_corr_gather_dot_opts": [I, P, P, I, P, P, I, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P, I, I, P],
    "mvt_knn1_gather": [P, I, LL, I, P, I, I, I, I, I, I, I, P, P, P],
    "mvt_window_corr": [P, P, P, P, I, I, I, I, I, I, I, I, I, P],
    "mvt_window_corr_levels": [I, P, I, P, P, P, P, P, I, I, I, I, I, I, P],
    "mvt_pos_embed": [P, I, I, I, I, P, P, P],
    "mvt_token_assemble": [P, P, I, P, I, P, P, P, I, I, I, P, I, P],
    "mvt_delta_split": [P, I, P, P, P, P, LL, I, P, P],
    "mvt_rowdot": [P, I, P, P, P, LL, I, P],
    "mvt_layernorm": [P, I, P, P, P, I, LL, I, F, P],
    "mvt_attention": [P, I, LL, LL, P, P, I, LL, LL, P, I, I, I, I, I, I, P],
    "mvt_attention_bf16": [P, I, LL, LL, P, P, I, LL, LL, P, I, I, I, I, I, I, I, P, P],
    "mvt_broadcast_rows": [P, P, I, I, I, I, P],
    "mvt_attention_segmented": [P, I, LL, LL, P, P, I, LL, LL, P, I, I, I, I, I, P, P, P, P, P],
    "mvt_attention_bf16_segmented": [P, I, LL, LL, P, P, I, LL, LL, P, I, I, I, I, I, I, P, P, P, P, P, LL, P],
    "mvt_broadcast_rows_repeat": [P, P, I, I, I, I, I, P],
    "mvt_updateformer_grouped_workspace_bytes": [I, I, I],
    "mvt_updateformer_forward_grouped": [P, P, I, I, I, P, P, I, P, P, P, P, LL, P],
    "mvt_updateformer_forward_tokens_grouped": [P, P, I, I, P, P, I, P, P, P, P, LL, P],
    "mvt_attn_block_fused_bf16": [P, I, P, P, P, P, P, P, P, I, P, I, LL, I, P, P],
    "mvt_window_prepare": [P, P, P, P, P, P, I, I, I, I, I, I, I, P, P, P, P],
    "mvt_window_store": [P, P, P, P, I, I, I, I, I, I, I, I, P, P, P, P],
    "mvt_track_metrics": [P, P, P, P, P, I, I, I, P, I, F, P, I, P],
    "mvt_encoder_workspace_bytes": [I, I, I, I],
    "mvt_encoder_forward": [P, P, I, I, I, P, I, I, P, LL, P],
    "mvt_encoder_forward_rgb": [P, P, I, I, I, LL, I, I, I, P, I, I, P, LL, P],
    "mvt_updateformer_workspace_bytes": [I, I],
    "mvt_updateformer_forward": [P, P, I, I, P, I, P, P, P, P, LL, P],
    "mvt_updateformer_forward_tokens": [P, P, I, P, I, P, P, P, P, LL, P],
    "mvt_token_input_proj_bf16": [P, P, I, P, I, P, P, P, I, I, I, P, P, P, P, I, P, I, LL, I, P],
    "mvt_update_head_bf16": [P, I, P, P, P, P, P, P, P, P, P, P, P, P, P, I, LL, I, I, P, P],
    "mvt_query_pool": [P, P, P, P, I, I, I, I, I, F, F, F, F, F, F, I, P, P, P, P],
    "mvt_kmeans_stats": [P, LL, F, P, P, P],
    "mvt_kmeans_seed": [P, LL, I, LL, P, P, P, P, P],
    "mvt_kmeans_assign": [P, LL, P, I, P, P, P, I, I, P],
    "mvt_kmeans_update": [P, I, P, P, I, I, P],
    "mvt_kmeans_iterate": [P, LL, P, I, P, P, P, I, I, P],
    "mvt_select_kth": [P, LL, LL, P, P, P],
    "mvt_scene_stats": [P, P, P, P, I, I, I, I, I, F, I, F, F, P, P, P, P, P],
    "mvt_scene_apply": [P, P, LL, P, P, I, P, P, LL, P, P],
    "mvt_scene_tracks": [P, P, LL, P, P],
    "mvt_clean_points": [P, P, P, P, I, I, I, I, I, I, F, P, P, P],
    "mvt_clean_search": [P, I, LL, I, I, I, I, F, I, P, P, P, P, P],
    "mvt_clean_mask": [P, P, I, LL, I, F, I, P, P, P],
    "mvt_align_normals": [P, I, I, I, F, P, P],
    "mvt_align_transform": [P, P, LL, P, P],
    "mvt_align_queries": [LL, I, I, I, P],
    "mvt_align_correspond": [P, LL, I, I, I, I, P, F, P, I, P, P, P, P, P],
    "mvt_align_solve": [P, LL, P, I, I, P, P, P, P, P, P],
    "mvt_normals_estimate": [P, I, LL, I, I, I, F, P, P, P, P, P, P, P, P],
    "mvt_voxel_bounds": [P, LL, C.c_double, P, P, P],
    "mvt_voxel_insert": [P, LL, P, P, LL, P],
    "mvt_voxel_emit": [P, LL, P, P, LL, P, P, P, P, P, P, P],
    "mvt_reproject_clear": [P, LL, P],
    "mvt_reproject_splat_depths": [P, P, P, P, I, I, I, I, I, F, P, I, P, P, I, F, I, P, P],
    "mvt_reproject_splat_points": [P, LL, I, P, P, I, I, F, I, P, P],
    "mvt_reproject_resolve": [P, I, I, I, P, I, I, I, I, P, LL, LL, P, P, P, P],
    "mvt_photometric_blocks": [I, I],
    "mvt_photometric_score": [P, I, P, I, P, P, P, I, I, I, F, P, P, P],
    "mvt_cluster_crop": [P, I, LL, P, P, P],
    "mvt_cluster_count": [P, I, LL, I, I, F, I, P, P, P, P],
    "mvt_cluster_link": [P, I, LL, I, I, F, P, P, P, P, P, P],
    "mvt_cluster_border": [P, I, LL, I, I, F, P, P, P, P, P, P],
    "mvt_cluster_finish": [P, I, LL, I, P, P, P, P, P, P, P],
    "mvt_motion_blocks": [I, I],
    "mvt_motion_tiles": [I, I],
    "mvt_motion_temporal": [P, I, I, I, I, I, I, P, P, P],
    "mvt_motion_mask": [P, I, I, I, I, I, I, F, P, P, P],
    "mvt_motion_report": [P, P, I, I, I, I, I, P, P],
    "mvt_overlay_project": [P, P, P, I, I, I, P, P, I, I, F, P, I, P, I, I, P, P],
    "mvt_overlay_draw": [P, P, P, P, P, I, I, I, I, I, I, I, P, P, P],
    "mvt_overlay_compose": [P, I, I, I, I, I, I, I, P, I, P, P, P],
    "mvt_mask_stats": [P, P, P, P, P, I, I, I, I, F, F, F, P, P],
    "mvt_mask_centroids": [P, I, I, I, P, P],
    "mvt_mask_match": [P, I, I, I, C.c_double, I, P, P, P, P, P],
    "mvt_mask_relabel": [P, P, I, I, I, I, P, P],
    "mvt_mask_pool": [P, P, P, P, P, I, I, I, I, I, F, F, F, P, I, I, P, P, P, P, P],
    "mvt_rigid_members": [P, P, I, I, I, P, P, P, P, P],
    "mvt_rigid_fit": [P, P, P, P, P, P, P, I, I, I, C.c_double, I, I, I, C.c_double, I, P, P, P, P, P, P, P, P],
    "mvt_rigid_compose": [P, P, I, I, I, P, P],
    "mvt_rigid_move": [P, P, P, I, I, I, P, P],
    "mvt_rigid_fill": [P, P, P, P, P, P, P, P, I, I, I, I, I, P, P, P],
}
_RET = {"mvt_build_arch": C.c_char_p, "mvt_encoder_workspace_bytes": C.c_longlong, "mvt_updateformer_workspace_bytes": C.c_longlong,
        "mvt_updateformer_grouped_workspace_bytes": C.c_longlong}

for _name, _args in SIGNATURES.items():
    _fn = getattr(_lib, _name)  # AttributeError here = header / library mismatch
    _fn.argtypes = _args
    _fn.restype = _RET.get(_name, C.c_int)

ACT_NONE, ACT_RELU, ACT_GELU_TANH, ACT_GELU_ERF = 0, 1, 2, 3
IN_SLABS = 64


class HipError(RuntimeError):
    pass


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise HipError("libmvtracker_hip needs device tensors (got a CPU tensor); there is no CPU path")
    return t.data_ptr()


def require_device(t):
    """The product path has no CPU implementation: refuse host tensors loudly; and the tensors' device must be the current
    one (the launch stream is the current device's) -- entry points get there through ``device_guard``."""
    if not t.is_cuda:
        raise HipError("the MI355X tracker needs device tensors (got a CPU tensor); there is no CPU path")
    if t.device.index != torch.cuda.current_device():
        raise HipError(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                       "launches go to the current device's stream (wrap the call in hip.device_guard(tensor))")


def _stream():
    """The launch stream: torch's current stream of the CURRENT device.  Every public entry point of the package runs
    under ``device_guard`` of its tensors, so this is the stream of the device the pointers live on."""
    return torch.cuda.current_stream().cuda_stream


def device_guard(t):
    """Context manager that makes ``t``'s device the current one (no-op for host tensors, which only the CPU host-logic
    tests pass).  A model on cuda:1 called while cuda:0 is current would otherwise launch on device 0's stream with
    device-1 pointers."""
    if t is not None and t.is_cuda:
        return torch.cuda.device(t.device)
    return contextlib.nullcontext()


def guarded(fn):
    """Decorator for entry points whose first tensor argument fixes the device of the call."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t = next((a for a in list(args) + list(kwargs.values()) if isinstance(a, torch.Tensor)), None)
        if t is None:  # e.g. (store dict, ...) first: look one level into dicts / lists
            for a in list(args) + list(kwargs.values()):
                if isinstance(a, dict):
                    a = list(a.values())
                if isinstance(a, (list, tuple)):
                    t = next((x for x in a if isinstance(x, torch.Tensor)), None) or next(
                        (y for x in a if isinstance(x, (list, tuple)) for y in x if isinstance(y, torch.Tensor)), None)
                    if t is not None:
                        break
        with device_guard(t):
            return fn(*args, **kwargs)
    return wrapper


def _call(name, *args):
    rc = getattr(_lib, name)(*args)
    if rc != 0:
        raise HipError(f"{name} failed with code {rc}" + (" (arguments rejected)" if rc == 1 else " (HIP launch error)"))


IO_IN_BF16, IO_OUT_BF16, IO_SHORT_WG = 1, 2, 4


def _io(t_in, t_out=None):
    """MVT_IO_* flags from the element types of the activation tensors (fp32 or bf16)."""
    for t in (t_in, t_out):
        assert t is None or t.dtype in (torch.float32, torch.bfloat16), t.dtype
    return (IO_IN_BF16 if t_in is not None and t_in.dtype == torch.bfloat16 else 0) | \
           (IO_OUT_BF16 if t_out is not None and t_out.dtype == torch.bfloat16 else 0)


def _f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


def abi_version() -> int:
    return _lib.mvt_abi_version()


def build_arch() -> str:
    return _lib.mvt_build_arch().decode()


# ------------------------------------------------------------------ thin typed wrappers
def gemm(A, lda, Wt, ldw, bias, R, ldr, Cm, ldc, M, N, K, act=ACT_NONE):
    _call("mvt_gemm", _ptr(A), lda, _ptr(Wt), ldw, _ptr(bias), _ptr(R), ldr, _ptr(Cm), ldc, M, N, K, act, _stream())


def conv2d(x, wt, bias, out, n, H, W, Cin, Cout, KH, KW, stride, pad, ldo, act=ACT_NONE):
    _call("mvt_conv2d", _ptr(x), _ptr(wt), _ptr(bias), _ptr(out), n, H, W, Cin, Cout, KH, KW, stride, pad, ldo, act, _stream())


def split_bf16(src, hi, lo, n):
    _call("mvt_split_bf16", _ptr(src), _ptr(hi), _ptr(lo), n, _stream())


def gemm_bf16(A, lda, Whi, Wlo, ldw, bias, R, ldr, Cm, ldc, M, N, K, act=ACT_NONE):
    _call("mvt_gemm_bf16", _ptr(A), lda, _ptr(Whi), _ptr(Wlo), ldw, _ptr(bias), _ptr(R), ldr, _ptr(Cm), ldc, M, N, K, act,
          _io(None, Cm), _stream())


def conv2d_stat_slots(H, W, Cin, KH, KW, stride, pad, split=False) -> int:
    """split: the weights carry a bf16 lo part (bf16x3 mode) -- the two 3x3 kernels cut the image differently."""
    return _lib.mvt_conv2d_stat_slots(H, W, Cin, KH, KW, stride, pad, int(split))


def conv2d_bf16(x, wt_hi, wt_lo, bias, out, n, H, W, Cin, Cout, KH, KW, stride, pad, ldo, act=ACT_NONE, in_stats=None,
                out_partial=None, short_wg=False):
    """``short_wg`` (MVT_IO_SHORT_WG): the launch shares the GPU with other streams -- keep every workgroup short-lived (the wide
    3x3 layers then run on the 64-channel row tiles instead of one 512-thread workgroup per CU; identical results)."""
    _call("mvt_conv2d_bf16", _ptr(x), _ptr(wt_hi), _ptr(wt_lo), _ptr(bias), _ptr(out), n, H, W, Cin, Cout, KH, KW, stride, pad,
          ldo, act, _io(x, out) | (IO_SHORT_WG if short_wg else 0), _ptr(in_stats), _ptr(out_partial), _stream())


def conv3x3s2_down_bf16(x, w3, b3, wd, bd, out3, outd, n, H, W, Cin, Cout, ldo, part3=None, partd=None):
    """conv1 (3x3 / stride 2) and downsample[0] (1x1 / stride 2) of a strided ResidualBlock in one launch (bf16 tensors)."""
    assert x.dtype == torch.bfloat16 and out3.dtype == torch.bfloat16 and outd.dtype == torch.bfloat16
    _call("mvt_conv3x3s2_down_bf16", _ptr(x), _ptr(w3), _ptr(b3), _ptr(wd), _ptr(bd), _ptr(out3), _ptr(outd), n, H, W, Cin, Cout, ldo,
          _ptr(part3), _ptr(partd), _stream())


def instnorm_finish_slots(partial, slots, mean_rstd, n, HW, Cc):
    _call("mvt_instnorm_finish_slots", _ptr(partial), slots, _ptr(mean_rstd), n, HW, Cc, _stream())


def ln_gemm_bf16(A, lda, ln_w, ln_b, eps, Whi, Wlo, ldw, bias, R, ldr, Cm, ldc, M, N, K, act=ACT_NONE):
    _call("mvt_ln_gemm_bf16", _ptr(A), lda, _ptr(ln_w), _ptr(ln_b), eps, _ptr(Whi), _ptr(Wlo), ldw, _ptr(bias), _ptr(R), ldr,
          _ptr(Cm), ldc, M, N, K, act, _stream())


def pack_frag_bf16(w, ld, N, K, out):
    _call("mvt_pack_frag_bf16", _ptr(w), ld, N, K, _ptr(out), _stream())


class BlockNext(C.Structure):
    """mvt_block_next of include/mvtracker_hip.h."""
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("lnw", C.c_void_p), ("lnb", C.c_void_p), ("y", C.c_void_p),
                ("ldw", C.c_int), ("N", C.c_int), ("ldy", C.c_int), ("eps", C.c_float), ("row_lo", C.c_longlong),
                ("row_hi", C.c_longlong), ("y_bf16", C.c_int)]


BLOCK_MAX_NEXT = 3


def _next_array(nexts):
    """The mvt_block_next array of a list of follow-up projections (the dicts of ``block_fused_bf16``); never zero-sized."""
    arr = (BlockNext * max(1, len(nexts)))()
    for i, nx in enumerate(nexts):
        arr[i] = BlockNext(_ptr(nx["w"]), _ptr(nx["b"]), _ptr(nx.get("lnw")), _ptr(nx.get("lnb")), _ptr(nx["y"]), nx["ldw"], nx["N"],
                           nx["ldy"], nx["eps"], *nx.get("rows", (0, 0)), 1 if nx["y"].dtype == torch.bfloat16 else 0)
    return arr


def block_fused_bf16(x, ldx, att, ldatt, Ko, wo, ldwo, bo, w1, ldw1, b1, w2, ldw2, b2, H, nexts, M, Cc, ws=None):
    """nexts: list of dicts(w, ldw, b, N, lnw, lnb, eps, y, ldy[, rows=(lo, hi)]) -- at most BLOCK_MAX_NEXT follow-up
    projections; ``rows`` restricts one to a row range (y is always indexed by the global row).  ``ws``: optional fp32
    workspace of (H/256 + 1) * M * Cc elements that lets M <= 2048 run cut over 4x more workgroups."""
    assert ws is None or (ws.dtype == torch.float32 and ws.numel() >= (H // 256 + 1) * M * Cc)
    arr = _next_array(nexts)
    _call("mvt_block_fused_bf16", _ptr(x), ldx, _ptr(att), 1 if (att is not None and att.dtype == torch.bfloat16) else 0, ldatt, Ko, _ptr(wo), ldwo, _ptr(bo), _ptr(w1), ldw1, _ptr(b1), _ptr(w2),
          ldw2, _ptr(b2), H, C.cast(arr, C.c_void_p), len(nexts), M, Cc, _ptr(ws), _stream())


def ln_proj_bf16(x, ldx, nexts, M, Cc):
    """LayerNorm + projections of ``nexts`` (same dicts as ``block_fused_bf16``); x is only read."""
    arr = _next_array(nexts)
    _call("mvt_ln_proj_bf16", _ptr(x), ldx, C.cast(arr, C.c_void_p), len(nexts), M, Cc, _stream())


def input_proj_bf16(tokens, ldtok, token_dim, Mp, win, bin_, virtual_tokens, S, x, ldx, nexts, M, Cc):
    """x = [tokens . Win^T + b ; virtual tokens] written, then the LayerNorm + projections of ``nexts`` (one launch)."""
    arr = _next_array(nexts)
    _call("mvt_input_proj_bf16", _ptr(_f32c(tokens)), ldtok, token_dim, Mp, _ptr(win), _ptr(bin_), _ptr(virtual_tokens), S, _ptr(x), ldx,
          C.cast(arr, C.c_void_p), len(nexts), M, Cc, _stream())


def mlp_fused_bf16(x, ldx, w1, ldw1, b1, w2, ldw2, b2, M, Cc, H, eps):
    _call("mvt_mlp_fused_bf16", _ptr(x), ldx, _ptr(w1), ldw1, _ptr(b1), _ptr(w2), ldw2, _ptr(b2), M, Cc, H, eps, _stream())


def rgb_to_nhwc4(rgbs, out, V, T, H, W, t0, nt):
    if rgbs.dtype == torch.uint8:
        assert rgbs.is_contiguous()
        _call("mvt_rgb_u8_to_nhwc4", _ptr(rgbs), _ptr(out), V, T, H, W, t0, nt, _stream())
    else:
        _call("mvt_rgb_to_nhwc4", _ptr(_f32c(rgbs)), _ptr(out), V, T, H, W, t0, nt, _stream())


def rgb_images_to_nhwc4(rgbs, out, V, T, H, W, img0, nimg):
    """Images img0 .. img0+nimg-1 in frame-major numbering (t * V + v) of rgbs (V,T,3,H,W) fp32 or uint8 -> out (nimg,H,W,4)."""
    assert rgbs.is_contiguous() and rgbs.dtype in (torch.uint8, torch.float32)
    _call("mvt_rgb_images_to_nhwc4", _ptr(rgbs), 1 if rgbs.dtype == torch.uint8 else 0, _ptr(out), V, T, H, W, img0, nimg, _stream())


def resize_nearest(x, out, planes, Hi, Wi, Ho, Wo):
    _call("mvt_resize_nearest", _ptr(_f32c(x)), _ptr(out), planes, Hi, Wi, Ho, Wo, _stream())


def instnorm_stats(x, ldx, partial, mean_rstd, n, HW, Cc):
    _call("mvt_instnorm_stats", _ptr(x), ldx, _ptr(partial), _ptr(mean_rstd), n, HW, Cc, _io(x), _stream())


def instnorm_apply(x, mean_rstd, skip, skip_stats, y, n, HW, Cc, skip_relu=False):
    assert y.dtype == x.dtype and (skip is None or skip.dtype == x.dtype)
    _call("mvt_instnorm_apply", _ptr(x), _ptr(mean_rstd), _ptr(skip), _ptr(skip_stats), _ptr(y), n, HW, Cc,
          _io(x, y) | (4 if skip_relu else 0), _stream())


def resize_bilinear_ac(src, dst, n, Hs, Ws, Cc, Hd, Wd, ldd, c_off):
    assert src.dtype == dst.dtype
    _call("mvt_resize_bilinear_ac", _ptr(src), _ptr(dst), n, Hs, Ws, Cc, Hd, Wd, ldd, c_off, _io(src, dst), _stream())


def concat_resize_bilinear_ac(srcs, dims, dst, n, Hd, Wd, ldd):
    """srcs: device tensors (n, Hs_k, Ws_k, C_k) of one element type; dims: [(Hs_k, Ws_k, C_k)]; one launch for the whole concat."""
    k = len(srcs)
    assert all(t.dtype == dst.dtype for t in srcs)
    ia = lambda j: (C.c_int * k)(*[d[j] for d in dims])
    _call("mvt_concat_resize_bilinear_ac", k, (C.c_void_p * k)(*[_ptr(t) for t in srcs]), ia(0), ia(1), ia(2), _ptr(dst), n, Hd, Wd, ldd,
          _io(srcs[0], dst), _stream())


def invert_cameras(intrs, extrs, kinv, einv, n):
    _call("mvt_invert_cameras", _ptr(_f32c(intrs)), _ptr(_f32c(extrs)), _ptr(kinv), _ptr(einv), n, _stream())


def depth_subsample(depths, out, V, T, H, W, s):
    _call("mvt_depth_subsample", _ptr(_f32c(depths)), _ptr(out), V, T, H, W, s, _stream())


def avgpool2(x, out, n, h, w, Cc):
    assert x.dtype == out.dtype
    _call("mvt_avgpool2", _ptr(x), _ptr(out), n, h, w, Cc, _io(x, out), _stream())


def unproject(depth_s, kinv, einv, xyz, V, T, hs, ws, stride, level):
    _call("mvt_unproject", _ptr(depth_s), _ptr(kinv), _ptr(einv), _ptr(xyz), V, T, hs, ws, stride, level, _stream())


def tile_aabb(xyz, Pn, T, box, grid=(0, 0)):
    """box (T, ceil(Pn/64), 8) <- bounding boxes of the 64-point tiles; grid = per-view (w, h) for 8x8 patch tiles."""
    _call("mvt_tile_aabb", _ptr(xyz), Pn, T, grid[0], grid[1], _ptr(box), _stream())


def _frames(T):
    """The frame rule of include/mvtracker_hip.h, (base, R, lo, hi), from what the slot-mapped wrappers take where ``T`` stands: an
    int is a linear store of T frames, (0, T, 0, T-1); a ring store's (base, R, lo, hi) passes through (the store tensors hold R
    frame slots, frame f in slot (f - base) mod R, frames [lo, hi] resident, a window slot reads clamp(frame0 + s * frame_step, lo, hi))."""
    if isinstance(T, int):
        return (0, T, 0, T - 1)
    if isinstance(T, (tuple, list)) and len(T) == 4:
        return tuple(T)
    raise HipError(f"frames must be a frame count T or (base, R, lo, hi), got {T!r}")


def knn_scan(xyz, Pn, coords, N, S, frame0, frame_step, T, K, nseg, keys, seed_idx=None, seed_k=0, seed_dims=(0, 0, 0, 0), box=None,
             grid=(0, 0)):
    """T: the store's frames (``_frames``), here and in every wrapper below that takes it.  seed_dims = (coarse_w, coarse_h, fine_w, fine_h) per-view grids when the seed comes from the coarser level;
    box / grid: tile bounding boxes from ``tile_aabb`` (same grid) for culling."""
    _call("mvt_knn_scan", _ptr(xyz), Pn, _ptr(coords), N, S, frame0, frame_step, *_frames(T), K, nseg, _ptr(keys), _ptr(seed_idx),
          seed_k, *seed_dims, _ptr(box), grid[0], grid[1], _stream())


class KnnLevel(C.Structure):
    """mvt_knn_level of include/mvtracker_hip.h."""
    _fields_ = [("xyz", C.c_void_p), ("P", C.c_longlong), ("keys", C.c_void_p), ("seed_idx", C.c_void_p), ("tile_box", C.c_void_p),
                ("nseg", C.c_int), ("grid_w", C.c_int), ("grid_h", C.c_int), ("idx_out", C.c_void_p), ("group_box", C.c_void_p)]


def _knn_levels(levels):
    arr = (KnnLevel * len(levels))()
    for i, lv in enumerate(levels):
        g = lv.get("grid", (0, 0))
        arr[i] = KnnLevel(_ptr(lv["xyz"]), lv["P"], _ptr(lv["keys"]), _ptr(lv.get("seed_idx")), _ptr(lv.get("box")), lv["nseg"], g[0], g[1],
                          _ptr(lv.get("idx_out")), _ptr(lv.get("gbox")))
    return arr


def knn_scan_levels(levels, coords, N, S, frame0, frame_step, T, K, seed_k=0):
    """levels: list of dicts(xyz, P, keys, nseg[, seed_idx, box, grid, idx_out]); one launch for all of them."""
    arr = _knn_levels(levels)
    _call("mvt_knn_scan_levels", len(levels), C.cast(arr, C.c_void_p), _ptr(coords), N, S, frame0, frame_step, *_frames(T), K, seed_k,
          _stream())


def tile_group_aabb(box, Pn, T, group_box):
    """group_box [T][ceil(ntiles/64)][8]: union boxes of 64 consecutive tiles (coarse culling level of the searches)."""
    _call("mvt_tile_group_aabb", _ptr(box), Pn, T, _ptr(group_box), _stream())


def cloud_boxes(xyz, n_clouds, n_points, grid):
    """The boxes that every cloud search walks, of clouds xyz (n_clouds, n_points, 4): ``tile_aabb`` then ``tile_group_aabb``.
    Returns (box (n_clouds, tiles, 8), gbox (n_clouds, ceil(tiles / 64), 8))."""
    nt = (n_points + 63) // 64
    box = torch.empty(n_clouds, nt, 8, device=xyz.device)
    gbox = torch.empty(n_clouds, (nt + 63) // 64, 8, device=xyz.device)
    tile_aabb(xyz, n_points, n_clouds, box, grid)
    tile_group_aabb(box, n_points, n_clouds, gbox)
    return box, gbox


def knn_search(xyz, Pn, coords, N, S, frame0, frame_step, T, K, idx_out, box, grid=(0, 0), gbox=None, seed_idx=None, seed_k=0,
               seed_dims=(0, 0, 0, 0)):
    """``knn_scan`` (one segment) + ``knn_merge`` in one launch: neighbour indices straight to idx_out (N,S,K) int32."""
    _call("mvt_knn_search", _ptr(xyz), Pn, _ptr(coords), N, S, frame0, frame_step, *_frames(T), K, _ptr(seed_idx), seed_k, *seed_dims,
          _ptr(box), _ptr(gbox), grid[0], grid[1], _ptr(idx_out), _stream())


def knn_search_levels(levels, coords, N, S, frame0, frame_step, T, K, seed_k):
    """Seeded scan + merge in one launch: levels of dicts(xyz, P, seed_idx, box, grid, idx_out[, gbox]); idx_out may alias seed_idx."""
    arr = _knn_levels([dict(lv, keys=None, nseg=1) for lv in levels])
    _call("mvt_knn_search_levels", len(levels), C.cast(arr, C.c_void_p), _ptr(coords), N, S, frame0, frame_step, *_frames(T), K, seed_k,
          _stream())


def knn_merge_levels(levels, N, S, K):
    arr = _knn_levels(levels)
    _call("mvt_knn_merge_levels", len(levels), C.cast(arr, C.c_void_p), N, S, K, _stream())


def adapter_best_view(depths, intrs, extrs, query_points, V, T, H, W, N, view_out, xyz_out=None):
    _call("mvt_adapter_best_view", _ptr(_f32c(depths)), _ptr(_f32c(intrs)), _ptr(_f32c(extrs)), _ptr(_f32c(query_points)), V, T, H, W, N,
          _ptr(view_out), _ptr(xyz_out), _stream())


def knn_merge(keys, N, S, K, nseg, Pn, idx_out):
    _call("mvt_knn_merge", _ptr(keys), N, S, K, nseg, Pn, _ptr(idx_out), _stream())


def _corr_levels(xyz_l, fvec_l, P_l, idx_l):
    """The leading arguments of the two gather-dot entries: level count, per-level pointer arrays, the feature rows' type."""
    n = len(xyz_l)
    pa = (C.c_void_p * n)
    bf = fvec_l[0].dtype == torch.bfloat16
    assert all((t.dtype == torch.bfloat16) == bf for t in fvec_l)
    return (n, pa(*[_ptr(t) for t in xyz_l]), pa(*[_ptr(t) for t in fvec_l]), 1 if bf else 0, (C.c_longlong * n)(*P_l),
            pa(*[_ptr(t) for t in idx_l]))


def corr_gather_dot(xyz_l, fvec_l, P_l, idx_l, Cc, targets, coords, N, S, frame0, frame_step, T, K, out, ldo, o_off):
    """xyz_l / fvec_l / idx_l: lists of per-level device tensors; P_l: list of point counts."""
    _call("mvt_corr_gather_dot", *_corr_levels(xyz_l, fvec_l, P_l, idx_l), Cc, _ptr(targets), _ptr(coords), N, S, frame0, frame_step,
          *_frames(T), K, _ptr(out), ldo, o_off, _stream())


def corr_gather_dot_opts(xyz_l, fvec_l, P_l, idx_l, Cc, targets, coords, N, S, frame0, frame_step, T, K, groups, add_offset, add_xyz, out, ldo,
                         o_off):
    """``corr_gather_dot`` with the non-default correlation options: groups + 3 add_offset + 3 add_xyz values per neighbour."""
    _call("mvt_corr_gather_dot_opts", *_corr_levels(xyz_l, fvec_l, P_l, idx_l), Cc, _ptr(targets), _ptr(coords), N, S, frame0, frame_step,
          *_frames(T), K, groups, 1 if add_offset else 0, 1 if add_xyz else 0, _ptr(out), ldo, o_off, _stream())


def knn1_gather(fvec, Pn, Cc, keys, n, nseg, frame, feat_out, idx_out=None, frames=None):
    """frames: the store's frames (``_frames``); None = ``frame`` is the slot itself (a linear store that holds it)."""
    _call("mvt_knn1_gather", _ptr(fvec), 1 if fvec.dtype == torch.bfloat16 else 0, Pn, Cc, _ptr(keys), n, nseg, frame,
          *((0, frame + 1, 0, frame) if frames is None else _frames(frames)), _ptr(feat_out), _ptr(idx_out), _stream())


# The names under which the tracker reads a ring store (streaming), and under which the host tests put their stand-ins for it:
# the wrappers above, with ``ring`` = (base, R, lo, hi) in T's place.
knn_scan_ring, knn_search_ring, knn_scan_levels_ring, knn_search_levels_ring = knn_scan, knn_search, knn_scan_levels, knn_search_levels
corr_gather_dot_ring, corr_gather_dot_opts_ring = corr_gather_dot, corr_gather_dot_opts


def knn1_gather_ring(fvec, Pn, Cc, keys, n, nseg, frame, ring, feat_out, idx_out=None):
    knn1_gather(fvec, Pn, Cc, keys, n, nseg, frame, feat_out, idx_out, frames=ring)


def window_corr(fmap, targets, coords, out, BS, N, Cc, h, w, level, radius, ldo, o_off):
    _call("mvt_window_corr", _ptr(fmap), _ptr(targets), _ptr(coords), _ptr(out), BS, N, Cc, h, w, level, radius, ldo, o_off,
          _stream())


def window_corr_levels(fmaps, targets, coords, out, BS, N, Cc, radius, ldo, o_off=0):
    """CorrBlock.corr_sample for all levels in one launch; fmaps: list of channels-last (BS,h,w,C) device tensors, fp32 or bf16."""
    n = len(fmaps)
    bf = fmaps[0].dtype == torch.bfloat16
    assert all((f.dtype == torch.bfloat16) == bf and f.is_contiguous() and f.shape[0] == BS and f.shape[3] == Cc for f in fmaps)
    _call("mvt_window_corr_levels", n, (C.c_void_p * n)(*[_ptr(f) for f in fmaps]), 1 if bf else 0, (C.c_int * n)(*[f.shape[1] for f in fmaps]),
          (C.c_int * n)(*[f.shape[2] for f in fmaps]), _ptr(_f32c(targets)), _ptr(_f32c(coords)), _ptr(out), BS, N, Cc, radius, ldo, o_off, _stream())


def pos_embed(coords, N, S, D, dim_padded, pos, omega=None):
    """omega: optional device fp64 table of dim_padded // 6 frequencies (the reference's numpy values)."""
    assert omega is None or (omega.dtype == torch.float64 and omega.numel() >= dim_padded // 6)
    _call("mvt_pos_embed", _ptr(coords), N, S, D, dim_padded, _ptr(omega), _ptr(pos), _stream())


def token_assemble(coords, fcorr, Fc, ffeats, Cc, mask_vis, pos, time_embed, N, S, E, x, ldx):
    _call("mvt_token_assemble", _ptr(coords), _ptr(fcorr), Fc, _ptr(ffeats), Cc, _ptr(mask_vis), _ptr(pos), _ptr(time_embed),
          N, S, E, _ptr(x), ldx, _stream())


def delta_split(delta, ldd, gw, gb, coords, dn, rows, Cc, nan_flag=None):
    _call("mvt_delta_split", _ptr(delta), ldd, _ptr(gw), _ptr(gb), _ptr(coords), _ptr(dn), rows, Cc, _ptr(nan_flag), _stream())


def rowdot(x, ldx, w, b, out, rows, Cc):
    _call("mvt_rowdot", _ptr(x), ldx, _ptr(w), _ptr(b), _ptr(out), rows, Cc, _stream())


def layernorm(x, ldx, w, b, y, ldy, rows, Cc, eps):
    _call("mvt_layernorm", _ptr(x), ldx, _ptr(w), _ptr(b), _ptr(y), ldy, rows, Cc, eps, _stream())


def attention(q, ldq, q_gs, q_is, k, v, ldkv, k_gs, k_is, o, ldo, groups, nq, nk, heads, dh):
    _call("mvt_attention", _ptr(q), ldq, q_gs, q_is, _ptr(k), _ptr(v), ldkv, k_gs, k_is, _ptr(o), ldo, groups, nq, nk, heads,
          dh, _stream())


def attention_ws_floats(groups, nq, heads):
    """Workspace size (fp32 elements) of the key-split path of ``attention_bf16``."""
    return 4 * groups * heads * ((nq + 63) // 64) * 64 * 68


ATTN_PARTIALS_ONLY = 8  # MVT_ATTN_PARTIALS_ONLY
ATTN_NSPLIT = 4         # MVT_ATTN_NSPLIT


def attention_bf16(q, ldq, q_gs, q_is, k, v, ldkv, k_gs, k_is, o, ldo, groups, nq, nk, heads, dh, ws=None, partials_only=False):
    """``partials_only``: stop after the key-split partials in ``ws`` (MVT_ATTN_PARTIALS_ONLY; ``o`` is not written) -- the
    library refuses it unless the key-split form is the one this call takes."""
    assert q.dtype == k.dtype == v.dtype
    assert ws is None or (ws.dtype == torch.float32 and ws.numel() >= attention_ws_floats(groups, nq, heads))
    _call("mvt_attention_bf16", _ptr(q), ldq, q_gs, q_is, _ptr(k), _ptr(v), ldkv, k_gs, k_is, _ptr(o), ldo, groups, nq, nk, heads,
          dh, _io(q, o) | (ATTN_PARTIALS_ONLY if partials_only else 0), _ptr(ws), _stream())


def _segments(q_row0, nq, k_row0, nk):
    n = len(nq)
    assert n > 0 and len(q_row0) == len(k_row0) == len(nk) == n
    return (n, (C.c_longlong * n)(*map(int, q_row0)), (C.c_int * n)(*map(int, nq)), (C.c_longlong * n)(*map(int, k_row0)),
            (C.c_int * n)(*map(int, nk)))


def attention_segmented(q, ldq, q_gs, q_is, k, v, ldkv, k_gs, k_is, o, ldo, groups, heads, dh, q_row0, nq, k_row0, nk):
    """``attention`` on independent segments in one launch per kernel form: segment s has nq[s] queries per group from row
    q_row0[s] of q / o and nk[s] keys from row k_row0[s] of k / v (host lists); each segment's output equals ``attention`` on it."""
    _call("mvt_attention_segmented", _ptr(q), ldq, q_gs, q_is, _ptr(k), _ptr(v), ldkv, k_gs, k_is, _ptr(o), ldo, groups, heads, dh,
          *_segments(q_row0, nq, k_row0, nk), _stream())


def attention_segmented_ws_floats(groups, nq, heads):
    """Workspace of ``attention_bf16_segmented`` that lets every segment (queries per group ``nq``: a list) take its key split."""
    return sum(attention_ws_floats(groups, n, heads) for n in nq)


def attention_bf16_segmented(q, ldq, q_gs, q_is, k, v, ldkv, k_gs, k_is, o, ldo, groups, heads, dh, q_row0, nq, k_row0, nk, ws=None):
    assert q.dtype == k.dtype == v.dtype
    assert ws is None or (ws.dtype == torch.float32 and ws.is_contiguous())
    _call("mvt_attention_bf16_segmented", _ptr(q), ldq, q_gs, q_is, _ptr(k), _ptr(v), ldkv, k_gs, k_is, _ptr(o), ldo, groups, heads, dh,
          _io(q, o), *_segments(q_row0, nq, k_row0, nk), _ptr(ws), ws.numel() if ws is not None else 0, _stream())


def broadcast_rows_repeat(v, x, ld, n, S, Cc, reps):
    _call("mvt_broadcast_rows_repeat", _ptr(v), _ptr(x), ld, n, S, Cc, reps, _stream())


def window_prepare(qxyz, qt, feat_init, prev_coords, prev_vis, n, p0, S, Cc, frame0, T, coords, mask_vis, ffeats, frame_step=1, carry_src=None):
    """Track state of the window whose slot s is clip frame frame0 + frame_step * s (-1: the time-reversed pass; ``qt`` holds the query
    frames themselves either way).  The first ``p0`` rows continue from their own rows of ``prev_*``, or, with ``carry_src`` (int32,
    then p0 = 0), row i from row carry_src[i] >= 0, -1 for a track that enters here."""
    assert qt.dtype == torch.int32
    assert carry_src is None or (carry_src.dtype == torch.int32 and carry_src.numel() >= n)
    _call("mvt_window_prepare", _ptr(_f32c(qxyz)), _ptr(qt), _ptr(_f32c(feat_init)), _ptr(prev_coords), _ptr(prev_vis), _ptr(carry_src),
          n, p0, S, Cc, frame0, frame_step, T, _ptr(coords), _ptr(mask_vis), _ptr(ffeats), _stream())


def window_store(coords, vis, order, n, S, frame0, T, N, traj, vis_logit, vis_prob, frame_step=1, before=None, frames=None):
    """The window's slots into traj (f1-f0, N, 3) / vis_* (f1-f0, N), which hold frames ``frames`` = (f0, f1) of a clip of T frames (as
    far as known, f1 <= T; None: the whole clip).  Slots outside the range are dropped, and with ``before`` (int32 per row: the
    reversed pass's query frames) a row's slots at or past its bound."""
    f0, f1 = (0, T) if frames is None else frames
    assert order.dtype == torch.int64 and traj.shape[0] == f1 - f0 and traj.shape[1] == N
    assert before is None or before.dtype == torch.int32
    _call("mvt_window_store", _ptr(coords), _ptr(vis), _ptr(order), _ptr(before), n, S, frame0, frame_step, T, f0, f1, N, _ptr(traj),
          _ptr(vis_logit), _ptr(vis_prob), _stream())


def broadcast_rows(v, x, ld, n, S, Cc):
    _call("mvt_broadcast_rows", _ptr(v), _ptr(x), ld, n, S, Cc, _stream())


# ------------------------------------------------------------------ composite entry points
class LinFrag(C.Structure):
    """mvt_lin_frag of include/mvtracker_hip.h."""
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("N", C.c_int), ("K", C.c_int)]


class LinRows(C.Structure):
    """mvt_lin_rows."""
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("N", C.c_int), ("K", C.c_int), ("ldw", C.c_int)]


class UpdaterBlock(C.Structure):
    """mvt_updater_block."""
    _fields_ = [("qkv", LinFrag), ("q", LinFrag), ("kv", LinFrag), ("ctx_ln_w", C.c_void_p), ("ctx_ln_b", C.c_void_p),
                ("out", LinFrag), ("fc1", LinFrag), ("fc2", LinFrag)]


UPDATER_MAX_DEPTH = 8
COMPOSITE = True  # (the CPU host-logic tests, which replace the kernels one by one, switch the composite calls off)


class UpdaterWeights(C.Structure):
    """mvt_updater_weights: host struct of device pointers (the tensors must outlive it: keep them referenced)."""
    _fields_ = [("depth", C.c_int), ("hidden", C.c_int), ("heads", C.c_int), ("dim_head", C.c_int), ("n_virtual", C.c_int),
                ("S", C.c_int), ("token_dim", C.c_int), ("out_dim", C.c_int), ("fuse_attention", C.c_int), ("virtual_tokens", C.c_void_p),
                ("input_transform", LinRows), ("flow0", LinRows), ("flow2", LinRows), ("flow4", LinRows),
                ("time_blk", UpdaterBlock * UPDATER_MAX_DEPTH), ("v2p", UpdaterBlock * UPDATER_MAX_DEPTH),
                ("vself", UpdaterBlock * UPDATER_MAX_DEPTH), ("p2v", UpdaterBlock * UPDATER_MAX_DEPTH),
                ("flow0_frag", LinFrag), ("flow2_frag", LinFrag), ("flow4_frag", LinFrag), ("ffeats_updater", LinFrag),
                ("input_frag", LinFrag),
                ("ffeats_norm_w", C.c_void_p), ("ffeats_norm_b", C.c_void_p)]


def lin_frag(frag, bias, N, K):
    return LinFrag(_ptr(frag), _ptr(bias), N, K)


def lin_rows(w_hi, bias, N, K):
    return LinRows(_ptr(w_hi), _ptr(bias), N, K, w_hi.shape[1])


def updateformer_workspace_bytes(n, S) -> int:
    return int(_lib.mvt_updateformer_workspace_bytes(n, S))


def updateformer_forward(weights: UpdaterWeights, x, ldx, n, delta, ldd, workspace, coords=None, ffeats=None, nan_flag=None):
    """EfficientUpdateFormer.forward as one library call (bf16 mode, shipped geometry); workspace: uint8 device tensor.
    With ``coords`` / ``ffeats`` the track and feature update runs inside the flow-head kernel (``delta`` may then be None)."""
    _call("mvt_updateformer_forward", C.addressof(weights), _ptr(_f32c(x)), ldx, n, _ptr(delta), ldd, _ptr(coords), _ptr(ffeats),
          _ptr(nan_flag), _ptr(workspace), workspace.numel(), _stream())


def update_head_bf16(tok, ldt, w0, b0, w2, b2, w4, b4, gn_w, gn_b, wu, bu, coords, ffeats, delta, ldd, rows, hidden, out_dim, nan_flag=None):
    _call("mvt_update_head_bf16", _ptr(tok), ldt, _ptr(w0), _ptr(b0), _ptr(w2), _ptr(b2), _ptr(w4), _ptr(b4), _ptr(gn_w), _ptr(gn_b), _ptr(wu),
          _ptr(bu), _ptr(coords), _ptr(ffeats), _ptr(delta), ldd, rows, hidden, out_dim, _ptr(nan_flag), _stream())


ATTN_TIME, ATTN_FRAME, ATTN_PARTIALS = 1, 2, 3


class BlockAttn(C.Structure):
    """mvt_block_attn."""
    _fields_ = [("kind", C.c_int), ("S", C.c_int), ("n_keys", C.c_int), ("heads", C.c_int), ("dim_head", C.c_int), ("ldq", C.c_int),
                ("ldkv", C.c_int), ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("partials", C.c_void_p), ("n_splits", C.c_int),
                ("defer_pass2", C.c_int), ("ctx", C.c_void_p)]  # (the context form is only driven by the composite updater call)


def attn_block_fused_bf16(x, ldx, kind, S, q, ldq, k, v, ldkv, n_keys, wo, bo, w1, b1, w2, b2, H, nexts, M, Cc, ws=None, partials=None,
                          n_splits=0, defer_pass2=False):
    """``block_fused_bf16`` with the preceding attention inside the kernel (bf16 q / k / v; 6 heads x 48).
    ``ATTN_PARTIALS``: q / k / v are None and ``partials`` is the workspace that ``attention_bf16(..., partials_only=True)``
    left (``n_splits`` = ATTN_NSPLIT states per chunk).  ``defer_pass2``: split-path forms launch pass 1 only."""
    assert kind == ATTN_PARTIALS or q.dtype == k.dtype == v.dtype == torch.bfloat16
    assert partials is None or partials.dtype == torch.float32
    at = BlockAttn(kind, S, n_keys, 6, 48, ldq, ldkv, _ptr(q), _ptr(k), _ptr(v), _ptr(partials), n_splits, 1 if defer_pass2 else 0, None)
    arr = _next_array(nexts)
    _call("mvt_attn_block_fused_bf16", _ptr(x), ldx, C.addressof(at), _ptr(wo), _ptr(bo), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), H,
          C.cast(arr, C.c_void_p), len(nexts), M, Cc, _ptr(ws), _stream())


def track_metrics(gt_tracks, pred_tracks, gt_visible, pred_occluded, query_frame, T, N, D, thresholds, survival_threshold, out):
    """Per-track evaluation metrics; gt_visible / pred_occluded uint8 (T,N), query_frame int32 (N), out (N, 11 + 2K) fp32."""
    assert gt_visible.dtype == torch.uint8 and pred_occluded.dtype == torch.uint8 and query_frame.dtype == torch.int32
    K = len(thresholds)
    th = (C.c_float * K)(*[float(t) for t in thresholds])
    _call("mvt_track_metrics", _ptr(_f32c(gt_tracks)), _ptr(_f32c(pred_tracks)), _ptr(gt_visible), _ptr(pred_occluded), _ptr(query_frame),
          T, N, D, C.cast(th, C.c_void_p), K, float(survival_threshold), _ptr(out), out.shape[1], _stream())


class TokenInputs(C.Structure):
    """mvt_token_inputs."""
    _fields_ = [("coords", C.c_void_p), ("fcorr", C.c_void_p), ("ffeats", C.c_void_p), ("mask_vis", C.c_void_p), ("pos", C.c_void_p),
                ("time_embed", C.c_void_p), ("Fc", C.c_int), ("Cf", C.c_int), ("E", C.c_int)]


def updateformer_forward_tokens(weights: UpdaterWeights, coords, fcorr, Fc, ffeats, Cf, mask_vis, pos, time_embed, E, n, delta, ldd, workspace,
                                upd_coords=None, upd_ffeats=None, nan_flag=None):
    """``updateformer_forward`` with the token rows assembled inside its first kernel (no token matrix)."""
    ti = TokenInputs(_ptr(_f32c(coords)), _ptr(_f32c(fcorr)), _ptr(_f32c(ffeats)), _ptr(_f32c(mask_vis)), _ptr(_f32c(pos)), _ptr(_f32c(time_embed)),
                     Fc, Cf, E)
    _call("mvt_updateformer_forward_tokens", C.addressof(weights), C.addressof(ti), n, _ptr(delta), ldd, _ptr(upd_coords), _ptr(upd_ffeats),
          _ptr(nan_flag), _ptr(workspace), workspace.numel(), _stream())


ENCODER_CONVS = 23


class ConvWeights(C.Structure):
    """mvt_conv_weights."""
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p)]


class EncoderWeights(C.Structure):
    """mvt_encoder_weights (host struct of device pointers; keep the tensors referenced)."""
    _fields_ = [("latent_dim", C.c_int), ("short_workgroups", C.c_int), ("conv", ConvWeights * ENCODER_CONVS)]


def encoder_workspace_bytes(n, H, W, Cc) -> int:
    return int(_lib.mvt_encoder_workspace_bytes(n, H, W, Cc))


def encoder_forward_rgb(weights: EncoderWeights, rgbs, V, T, img0, n, H, W, out_rows, ldo, workspace):
    """``encoder_forward`` reading images img0 .. img0+n-1 (frame-major) of the planar clip rgbs (V,T,3,H,W) fp32 / uint8 directly."""
    assert rgbs.is_contiguous() and rgbs.dtype in (torch.uint8, torch.float32) and tuple(rgbs.shape) == (V, T, 3, H, W)
    _call("mvt_encoder_forward_rgb", C.addressof(weights), _ptr(rgbs), 1 if rgbs.dtype == torch.uint8 else 0, V, T, img0, n, H, W,
          _ptr(out_rows), ldo, 1 if out_rows.dtype == torch.bfloat16 else 0, _ptr(workspace), workspace.numel(), _stream())


def encoder_forward(weights: EncoderWeights, x4, n, H, W, out_rows, ldo, workspace):
    """BasicEncoder.forward as one library call (bf16 mode): x4 (n,H,W,4) fp32 -> out_rows (n,H/4,W/4,ldo) fp32 or bf16."""
    _call("mvt_encoder_forward", C.addressof(weights), _ptr(_f32c(x4)), n, H, W, _ptr(out_rows), ldo,
          1 if out_rows.dtype == torch.bfloat16 else 0, _ptr(workspace), workspace.numel(), _stream())


def _group_n(group_n):
    return len(group_n), (C.c_int * len(group_n))(*map(int, group_n))


def updateformer_grouped_workspace_bytes(n, S, G) -> int:
    return int(_lib.mvt_updateformer_grouped_workspace_bytes(n, S, G))


def updateformer_forward_grouped(weights: UpdaterWeights, x, ldx, group_n, delta, ldd, workspace, coords=None, ffeats=None, nan_flag=None):
    """``updateformer_forward`` on independent query sets of group_n[g] tracks each (host list), laid out back to back."""
    _call("mvt_updateformer_forward_grouped", C.addressof(weights), _ptr(_f32c(x)), ldx, sum(group_n), *_group_n(group_n), _ptr(delta), ldd,
          _ptr(coords), _ptr(ffeats), _ptr(nan_flag), _ptr(workspace), workspace.numel(), _stream())


def updateformer_forward_tokens_grouped(weights: UpdaterWeights, coords, fcorr, Fc, ffeats, Cf, mask_vis, pos, time_embed, E, group_n, delta,
                                        ldd, workspace, upd_coords=None, upd_ffeats=None, nan_flag=None):
    """``updateformer_forward_tokens`` on independent query sets of group_n[g] tracks each (host list)."""
    ti = TokenInputs(_ptr(_f32c(coords)), _ptr(_f32c(fcorr)), _ptr(_f32c(ffeats)), _ptr(_f32c(mask_vis)), _ptr(_f32c(pos)), _ptr(_f32c(time_embed)),
                     Fc, Cf, E)
    _call("mvt_updateformer_forward_tokens_grouped", C.addressof(weights), C.addressof(ti), sum(group_n), *_group_n(group_n), _ptr(delta), ldd,
          _ptr(upd_coords), _ptr(upd_ffeats), _ptr(nan_flag), _ptr(workspace), workspace.numel(), _stream())


# ------------------------------------------------------------------ query sampling (mvtracker_amd/queries.py drives these)
POOL_RADIUS_INCLUSIVE = 1  # MVT_POOL_RADIUS_INCLUSIVE
KMEANS_MAX_K, KMEANS_MAX_CAND, KMEANS_SEED_BLOCKS, KMEANS_STAT_BLOCKS = 4096, 10, 4096, 1024
KM_LO, KM_HI, KM_SCALE, KM_SCALE2, KM_TOL, KM_ITER, KM_CONVERGED, KM_EMPTY, KM_INERTIA, KM_SHIFT, KM_POT, KM_WORDS = 0, 3, 6, 7, 8, 9, 10, 11, 12, 14, 15, 32
KM_INERTIA_ACC, KM_CAND = 13, 16  # the running fixed-point inertia; KMEANS_MAX_CAND candidate indices of the running seeding step


def query_pool(depths, conf, kinv, einv, V, T, t, H, W, conf_threshold, x0, y0, radius_sq, z_min, z_max, pool, count, block_counts,
               radius_inclusive=False, flags=None):
    """Candidate pool of frame t of the clip depths (V,T,1,H,W) [conf: the same layout or None] -> pool (V*H*W,3), count (1,) int32.
    ``flags``: the raw MVT_POOL_* word in place of ``radius_inclusive``."""
    assert depths.is_contiguous() and depths.dtype == torch.float32 and depths.numel() == V * T * H * W
    assert conf is None or (conf.is_contiguous() and conf.dtype == torch.float32 and conf.numel() == V * T * H * W)
    assert pool.dtype == torch.float32 and pool.numel() >= V * H * W * 3 and count.dtype == torch.int32
    assert block_counts.dtype == torch.int32 and block_counts.numel() >= (V * H * W + 255) // 256
    _call("mvt_query_pool", _ptr(depths), _ptr(conf), _ptr(_f32c(kinv)), _ptr(_f32c(einv)), V, T, t, H, W, conf_threshold, x0, y0, radius_sq,
          z_min, z_max, (POOL_RADIUS_INCLUSIVE if radius_inclusive else 0) if flags is None else int(flags), _ptr(pool), _ptr(count), _ptr(block_counts), _stream())


def _km_check(pts, M, state):
    assert pts.dtype == torch.float32 and pts.is_contiguous() and pts.numel() == M * 3
    assert state.dtype == torch.int64 and state.numel() >= KM_WORDS


def kmeans_stats(pts, M, tol, partial, state):
    _km_check(pts, M, state)
    assert partial.dtype == torch.float64 and partial.numel() >= KMEANS_STAT_BLOCKS * 6
    _call("mvt_kmeans_stats", _ptr(pts), M, tol, _ptr(partial), _ptr(state), _stream())


def kmeans_seed(pts, M, k, seed, min_d2, partials, centres, state):
    _km_check(pts, M, state)
    assert min_d2.dtype == torch.float32 and min_d2.numel() >= M and centres.dtype == torch.float32 and centres.numel() >= k * 3
    assert partials.dtype == torch.int64 and partials.numel() >= KMEANS_MAX_CAND * KMEANS_SEED_BLOCKS
    _call("mvt_kmeans_seed", _ptr(pts), M, k, seed, _ptr(min_d2), _ptr(partials), _ptr(centres), _ptr(state), _stream())


def _km_check_acc(centres, k, labels, M, acc):
    assert centres.dtype == torch.float32 and centres.is_contiguous() and centres.numel() >= k * 3
    assert labels is None or (labels.dtype == torch.int32 and labels.numel() >= M)
    assert acc.dtype == torch.int64 and acc.numel() >= k * 4


def kmeans_assign(pts, M, centres, k, labels, acc, state, max_iter=300, final_pass=False):
    """labels (M,) int32 <- nearest centre; acc (k,4) int64 += fixed-point coordinate sums and counts (zero it before the first call)."""
    _km_check(pts, M, state)
    _km_check_acc(centres, k, labels, M, acc)
    _call("mvt_kmeans_assign", _ptr(pts), M, _ptr(centres), k, _ptr(labels), _ptr(acc), _ptr(state), max_iter, int(final_pass), _stream())


def kmeans_update(centres, k, acc, state, max_iter=300, final_pass=False):
    _km_check_acc(centres, k, None, 0, acc)
    assert state.dtype == torch.int64 and state.numel() >= KM_WORDS
    _call("mvt_kmeans_update", _ptr(centres), k, _ptr(acc), _ptr(state), max_iter, int(final_pass), _stream())


def kmeans_iterate(pts, M, centres, k, labels, acc, state, n_iters, max_iter):
    _km_check(pts, M, state)
    _km_check_acc(centres, k, labels, M, acc)
    _call("mvt_kmeans_iterate", _ptr(pts), M, _ptr(centres), k, _ptr(labels), _ptr(acc), _ptr(state), n_iters, max_iter, _stream())


# ------------------------------------------------------------------ scene normalisation (mvtracker_amd/scene.py drives these)
SELECT_WS_WORDS, SCENE_BLOCKS = 264, 1024  # MVT_SELECT_WS_WORDS, MVT_SCENE_BLOCKS
(SN_M, SN_CENTROID, SN_Z_QUANTILE, SN_FLOOR, SN_Z_LO, SN_Z_HI, SN_Z_RANK, SN_R_QUANTILE, SN_R_LO, SN_R_HI, SN_R_RANK, SN_NONFINITE,
 SN_Z_WEIGHT, SN_R_WEIGHT, SN_WORDS) = 0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16


def select_kth(values, n, k, out, workspace):
    """out[0] <- the k-th smallest (0-based) of the first n fp32 values, exactly (radix select; the caller refuses NaN)."""
    assert values.dtype == torch.float32 and values.is_contiguous() and values.numel() >= n
    assert out.dtype == torch.float32 and out.numel() >= 1
    assert workspace.dtype == torch.int32 and workspace.numel() >= SELECT_WS_WORDS
    _call("mvt_select_kth", _ptr(values), n, k, _ptr(out), _ptr(workspace), _stream())


def scene_stats(depths, conf, kinv, einv, V, T, t, H, W, conf_thresh, min_points, q_floor, q_radius, keys, partial, iws, state):
    """Pool statistics of frame t of depths (V,T,1,H,W) [conf: the same layout or None] -> state (SN_WORDS int64 words, doubles and
    integers as SN_* name them).  q_radius None: no radius quantile."""
    assert depths.is_contiguous() and depths.dtype == torch.float32 and depths.numel() == V * T * H * W
    assert conf is None or (conf.is_contiguous() and conf.dtype == torch.float32 and conf.numel() == V * T * H * W)
    assert keys.dtype == torch.int32 and keys.numel() >= V * H * W
    assert partial.dtype == torch.float64 and partial.numel() >= SCENE_BLOCKS * 3
    assert iws.dtype == torch.int32 and iws.numel() >= SELECT_WS_WORDS + V
    assert state.dtype == torch.int64 and state.numel() >= SN_WORDS
    _call("mvt_scene_stats", _ptr(depths), _ptr(conf), _ptr(_f32c(kinv)), _ptr(_f32c(einv)), V, T, t, H, W, conf_thresh, min_points, q_floor,
          -1.0 if q_radius is None else q_radius, _ptr(keys), _ptr(partial), _ptr(iws), _ptr(state), _stream())


def _xf(params):
    assert len(params) == 13, len(params)
    return (C.c_double * 13)(*[float(p) for p in params])


def scene_apply(params, depths=None, depths_out=None, extrs=None, extrs_out=None, queries=None, queries_out=None):
    """X' = t + R (s X) with params = (s, R row-major, t), 13 host floats: depths * s, extrinsics [n][3][4] right-multiplied by the
    rigid inverse, query rows (N,4) with the frame column kept.  Each part: a contiguous fp32 tensor and its output of the same size."""
    for a, b in ((depths, depths_out), (extrs, extrs_out), (queries, queries_out)):
        assert (a is None) == (b is None)
        assert a is None or (a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel())
    assert extrs is None or extrs.numel() % 12 == 0
    assert queries is None or queries.numel() % 4 == 0
    n = lambda t_, d: 0 if t_ is None else t_.numel() // d
    _call("mvt_scene_apply", _ptr(depths), _ptr(depths_out), n(depths, 1), _ptr(extrs), _ptr(extrs_out), n(extrs, 12), _ptr(queries),
          _ptr(queries_out), n(queries, 4), _xf(params), _stream())


def scene_tracks(params, tracks, out):
    """The same map on rows of three floats (…,3)."""
    assert tracks.dtype == out.dtype == torch.float32 and tracks.is_contiguous() and out.is_contiguous()
    assert tracks.numel() == out.numel() and tracks.numel() % 3 == 0 and tracks.numel() > 0
    _call("mvt_scene_tracks", _ptr(tracks), _ptr(out), tracks.numel() // 3, _xf(params), _stream())


# ------------------------------------------------------------------ depth cleaning (mvtracker_amd/clean.py drives these)
CLEAN_STATISTICAL, CLEAN_RADIUS, CLEAN_MAX_K = 0, 1, 64  # MVT_CLEAN_*


def clean_points(depths, conf, kinv, einv, V, T, t0, nt, H, W, conf_thresh, sphere, xyz):
    """Cloud points of frames [t0, t0 + nt) of depths (V,T,1,H,W) [conf: the same layout or None] -> xyz (V*nt, Hp*Wp, 4) on the grid
    padded to multiples of 8, NaN where the pixel is not valid.  sphere: None or (cx, cy, cz, radius) host numbers."""
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    assert depths.is_contiguous() and depths.dtype == torch.float32 and depths.numel() == V * T * H * W
    assert conf is None or (conf.is_contiguous() and conf.dtype == torch.float32 and conf.numel() == V * T * H * W)
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.numel() >= V * nt * Hp * Wp * 4
    sp = None if sphere is None else (C.c_float * 4)(*[float(v) for v in sphere])
    _call("mvt_clean_points", _ptr(depths), _ptr(conf), _ptr(_f32c(kinv)), _ptr(_f32c(einv)), V, T, t0, nt, H, W,
          0.0 if conf_thresh is None else conf_thresh, sp, _ptr(xyz), _stream())


def clean_search(xyz, Cn, Pn, grid, mode, K, radius, min_points, box, gbox, a_out=None, c_out=None):
    """Self-search of Cn clouds xyz (Cn, Pn, 4): a_out (Cn, Pn) fp32 mean distance to the K nearest (CLEAN_STATISTICAL) or c_out
    (Cn, Pn) int32 neighbours within radius, stopped at min_points + 1 (CLEAN_RADIUS).  box / gbox from tile_aabb / tile_group_aabb."""
    nt = (Pn + 63) // 64
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.numel() >= Cn * Pn * 4
    assert box.dtype == torch.float32 and box.numel() >= Cn * nt * 8 and gbox.dtype == torch.float32 and gbox.numel() >= Cn * ((nt + 63) // 64) * 8
    out = a_out if mode == CLEAN_STATISTICAL else c_out
    assert out is not None and out.dtype == (torch.float32 if mode == CLEAN_STATISTICAL else torch.int32) and out.numel() >= Cn * Pn
    _call("mvt_clean_search", _ptr(xyz), Cn, Pn, grid[0], grid[1], mode, K, radius, min_points, _ptr(box), _ptr(gbox), _ptr(a_out), _ptr(c_out),
          _stream())


def clean_mask(a, c, Cn, Pn, mode, std_ratio, min_points, state, keep):
    """state (Cn, 4) fp64 = (M, mu, sigma, thr) and keep (Cn, Pn) uint8 from the search's a (CLEAN_STATISTICAL) or c (CLEAN_RADIUS)."""
    src = a if mode == CLEAN_STATISTICAL else c
    assert src is not None and src.numel() >= Cn * Pn and src.dtype == (torch.float32 if mode == CLEAN_STATISTICAL else torch.int32)
    assert state.dtype == torch.float64 and state.numel() >= Cn * 4 and keep.dtype == torch.uint8 and keep.numel() >= Cn * Pn
    _call("mvt_clean_mask", _ptr(a), _ptr(c), Cn, Pn, mode, std_ratio, min_points, _ptr(state), _ptr(keep), _stream())


# ------------------------------------------------------------------ camera alignment (mvtracker_amd/align.py drives these)
ALIGN_MAX_TARGETS, ALIGN_ROW, ALIGN_HIST = 8, 30, 10  # MVT_ALIGN_*
ALIGN_I_DONE, ALIGN_I_ITERATIONS, ALIGN_I_STATUS, ALIGN_I_EVALS = 0, 1, 2, 3
ALIGN_FEW, ALIGN_SINGULAR = 1, 2


class AlignCloud(C.Structure):
    """mvt_align_cloud of include/mvtracker_hip.h."""
    _fields_ = [("xyz", C.c_void_p), ("nrm", C.c_void_p), ("tile_box", C.c_void_p), ("group_box", C.c_void_p), ("P", C.c_longlong),
                ("grid_w", C.c_int), ("grid_h", C.c_int)]


def align_normals(xyz, Cn, grid, max_edge, nrm):
    """nrm (Cn, h*w, 4) <- normals of the Cn organised clouds xyz (Cn, h*w, 4), grid = (w, h); NaN rows where there is none."""
    n = Cn * grid[0] * grid[1] * 4
    assert xyz.dtype == nrm.dtype == torch.float32 and xyz.is_contiguous() and nrm.is_contiguous() and xyz.numel() >= n and nrm.numel() >= n
    _call("mvt_align_normals", _ptr(xyz), Cn, grid[0], grid[1], max_edge, _ptr(nrm), _stream())


def align_transform(xyz0, D, n, xyz):
    """xyz[:n] = D xyz0[:n] (rows of 4 floats); D: 12 doubles on the device."""
    assert xyz0.dtype == xyz.dtype == torch.float32 and xyz0.is_contiguous() and xyz.is_contiguous()
    assert xyz0.numel() >= n * 4 and xyz.numel() >= n * 4 and D.dtype == torch.float64 and D.is_contiguous() and D.numel() >= 12
    _call("mvt_align_transform", _ptr(xyz0), _ptr(D), n, _ptr(xyz), _stream())


def align_queries(Pn, grid=(0, 0), sample_stride=1):
    """(query tiles per frame, tiles per row) of a source cloud; raises for a cloud the search refuses."""
    tpr = C.c_int(0)
    n = _lib.mvt_align_queries(Pn, grid[0], grid[1], sample_stride, C.cast(C.pointer(tpr), C.c_void_p))
    if n <= 0:
        raise HipError(f"mvt_align_queries refused P {Pn} grid {grid} sample_stride {sample_stride}")
    return n, tpr.value


def align_correspond(src0, Pn, grid, sample_stride, frames, D, cap2, targets, istate, partial, q_idx=None, q_d2=None):
    """targets: list of dicts(xyz, nrm, box, gbox, P, grid) of (frames, P, 4) clouds; partial (frames, tiles, ALIGN_ROW) fp64;
    q_idx / q_d2 (frames, tiles * 64) int32 / fp32 or None."""
    ntq = align_queries(Pn, grid, sample_stride)[0]
    assert src0.dtype == torch.float32 and src0.is_contiguous() and src0.numel() >= frames * Pn * 4
    assert D.dtype == torch.float64 and D.is_contiguous() and D.numel() >= 12 and istate.dtype == torch.int32 and istate.numel() >= 4
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.numel() >= frames * ntq * ALIGN_ROW
    assert (q_idx is None) == (q_d2 is None)
    assert q_idx is None or (q_idx.dtype == torch.int32 and q_d2.dtype == torch.float32 and min(q_idx.numel(), q_d2.numel()) >= frames * ntq * 64)
    arr = (AlignCloud * max(1, len(targets)))()
    for i, t in enumerate(targets):
        nt = (t["P"] + 63) // 64
        for k in ("xyz", "nrm"):
            assert t[k].dtype == torch.float32 and t[k].is_contiguous() and t[k].numel() >= frames * t["P"] * 4
        assert t["box"].dtype == torch.float32 and t["box"].is_contiguous() and t["box"].numel() >= frames * nt * 8
        assert t["gbox"].dtype == torch.float32 and t["gbox"].is_contiguous() and t["gbox"].numel() >= frames * ((nt + 63) // 64) * 8
        arr[i] = AlignCloud(_ptr(t["xyz"]), _ptr(t["nrm"]), _ptr(t["box"]), _ptr(t["gbox"]), t["P"], t["grid"][0], t["grid"][1])
    _call("mvt_align_correspond", _ptr(src0), Pn, grid[0], grid[1], sample_stride, frames, _ptr(D), cap2, C.cast(arr, C.c_void_p), len(targets),
          _ptr(istate), _ptr(partial), _ptr(q_idx), _ptr(q_d2), _stream())


def align_solve(partial, n_rows, n_queries, final_call, D, istate, hist, result, sums=None):
    """One evaluation of the ICP loop: hist (max_hist, ALIGN_HIST) fp64, result (4,) fp64, sums (ALIGN_ROW,) fp64 or None."""
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.numel() >= n_rows * ALIGN_ROW
    assert n_queries.dtype == torch.float64 and n_queries.numel() >= 1 and D.dtype == torch.float64 and D.is_contiguous() and D.numel() >= 12
    assert istate.dtype == torch.int32 and istate.numel() >= 4 and hist.dtype == torch.float64 and hist.is_contiguous()
    assert result.dtype == torch.float64 and result.is_contiguous() and result.numel() >= 4
    assert sums is None or (sums.dtype == torch.float64 and sums.numel() >= ALIGN_ROW)
    _call("mvt_align_solve", _ptr(partial), n_rows, _ptr(n_queries), int(final_call), hist.numel() // ALIGN_HIST, _ptr(D), _ptr(istate), _ptr(hist),
          _ptr(sums), _ptr(result), _stream())


# ------------------------------------------------------------------ cloud preparation (mvtracker_amd/cloud.py drives these)
NORMALS_MAX_NN = 64  # MVT_NORMALS_MAX_NN
VOXEL_RANGE, VOXEL_FULL = 1, 2  # MVT_VOXEL_* status bits
VOXEL_ORIGIN, VOXEL_SIZE, VOXEL_STATUS, VOXEL_POINTS, VOXEL_STATE_WORDS, VOXEL_BOUND_BLOCKS, VOXEL_SLOT_WORDS = 0, 3, 4, 5, 8, 1024, 6


def normals_estimate(xyz, Cn, Pn, grid, max_nn, radius, box, gbox, nrm, viewpoint=None, nbr_idx=None, nbr_cnt=None, cov=None):
    """nrm (Cn, Pn, 4) <- PCA normals of the Cn clouds xyz (Cn, Pn, 4) over the max_nn nearest points within radius (NaN rows where
    there is none).  box / gbox from tile_aabb / tile_group_aabb; viewpoint (Cn, 3) fp32 or None; optional nbr_idx (Cn, Pn, max_nn)
    int32, nbr_cnt (Cn, Pn) int32, cov (Cn, Pn, 6) fp64."""
    nt = (Pn + 63) // 64
    assert xyz.dtype == nrm.dtype == torch.float32 and xyz.is_contiguous() and nrm.is_contiguous()
    assert xyz.numel() >= Cn * Pn * 4 and nrm.numel() >= Cn * Pn * 4
    assert box.dtype == torch.float32 and box.numel() >= Cn * nt * 8 and gbox.dtype == torch.float32 and gbox.numel() >= Cn * ((nt + 63) // 64) * 8
    assert viewpoint is None or (viewpoint.dtype == torch.float32 and viewpoint.is_contiguous() and viewpoint.numel() >= Cn * 3)
    assert nbr_idx is None or (nbr_idx.dtype == torch.int32 and nbr_idx.is_contiguous() and nbr_idx.numel() >= Cn * Pn * max_nn)
    assert nbr_cnt is None or (nbr_cnt.dtype == torch.int32 and nbr_cnt.numel() >= Cn * Pn)
    assert cov is None or (cov.dtype == torch.float64 and cov.is_contiguous() and cov.numel() >= Cn * Pn * 6)
    _call("mvt_normals_estimate", _ptr(xyz), Cn, Pn, grid[0], grid[1], max_nn, radius, _ptr(box), _ptr(gbox), _ptr(viewpoint), _ptr(nrm),
          _ptr(nbr_idx), _ptr(nbr_cnt), _ptr(cov), _stream())


def voxel_capacity(Pn):
    """Slots of the hash table of a cloud of Pn points: the power of two >= 2 Pn."""
    return 1 << max(1, (2 * Pn - 1).bit_length())


def _voxel_check(xyz, Pn, state, table=None, capacity=0):
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.numel() >= Pn * 4
    assert state.dtype == torch.int64 and state.numel() >= VOXEL_STATE_WORDS
    assert table is None or (table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= capacity * VOXEL_SLOT_WORDS)


def voxel_bounds(xyz, Pn, voxel, partial, state):
    """state <- origin = (minimum of the points taking part) - voxel / 2, the voxel size, a clear status, the points taking part."""
    _voxel_check(xyz, Pn, state)
    assert partial.dtype == torch.float64 and partial.numel() >= VOXEL_BOUND_BLOCKS * 4
    _call("mvt_voxel_bounds", _ptr(xyz), Pn, float(voxel), _ptr(partial), _ptr(state), _stream())


def voxel_insert(xyz, Pn, state, table, capacity):
    """table (capacity * VOXEL_SLOT_WORDS int64 words) <- per cell the count, the first index and the fixed-point offset sums."""
    _voxel_check(xyz, Pn, state, table, capacity)
    _call("mvt_voxel_insert", _ptr(xyz), Pn, _ptr(state), _ptr(table), capacity, _stream())


def voxel_emit(xyz, Pn, state, table, capacity, block_counts, points, counts, first, n_out, labels=None):
    """points (>= Mv, 4) fp32, counts / first (>= Mv) int32, n_out (1,) int32 = Mv, labels (Pn,) int32 or None."""
    _voxel_check(xyz, Pn, state, table, capacity)
    assert block_counts.dtype == torch.int32 and block_counts.numel() >= (Pn + 255) // 256
    assert points.dtype == torch.float32 and points.is_contiguous() and counts.dtype == first.dtype == n_out.dtype == torch.int32
    assert labels is None or (labels.dtype == torch.int32 and labels.numel() >= Pn)
    _call("mvt_voxel_emit", _ptr(xyz), Pn, _ptr(state), _ptr(table), capacity, _ptr(block_counts), _ptr(points), _ptr(counts), _ptr(first),
          _ptr(labels), _ptr(n_out), _stream())


# ------------------------------------------------------------------ reprojection check (mvtracker_amd/reproject.py drives these)
REPROJECT_MAX_TARGETS, SCORE_WORDS = 16, 16  # MVT_REPROJECT_MAX_TARGETS, MVT_SCORE_WORDS
(SCORE_N, SCORE_COVERED, SCORE_SSE, SCORE_SAE, SCORE_SSE_COV, SCORE_SAE_COV, SCORE_SSIM, SCORE_SSIM_COV, SCORE_N_DEPTH, SCORE_N_CLOSE,
 SCORE_DEPTH_SAE, SCORE_DEPTH_SAE_CLOSE) = range(12)  # MVT_SCORE_*
SCORE_DOUBLES = (SCORE_SSIM, SCORE_SSIM_COV, SCORE_DEPTH_SAE, SCORE_DEPTH_SAE_CLOSE)


def _cams_check(intrs, extrs, n):
    assert intrs.dtype == extrs.dtype == torch.float32 and intrs.is_contiguous() and extrs.is_contiguous()
    assert intrs.numel() >= n * 9 and extrs.numel() >= n * 12


def reproject_clear(keys, n):
    """keys[:n] = ~0: the empty z-buffer (int64 words, a memset on the stream)."""
    assert keys.dtype == torch.int64 and keys.is_contiguous() and keys.numel() >= n
    _call("mvt_reproject_clear", _ptr(keys), n, _stream())


def reproject_splat_depths(depths, conf, kinv, einv, V, T, t, H, W, conf_thresh, target_views, intrs, extrs, exclude_self, min_depth, splat,
                           keys):
    """Frame t of depths (V,T,1,H,W) [conf: the same layout or None] into the cameras intrs (n, 9) / extrs (n, 12) of the views
    ``target_views`` (host integers): keys (n, H*W) int64 words take the minimum."""
    n = len(target_views)
    assert depths.is_contiguous() and depths.dtype == torch.float32 and depths.numel() == V * T * H * W
    assert conf is None or (conf.is_contiguous() and conf.dtype == torch.float32 and conf.numel() == V * T * H * W)
    assert keys.dtype == torch.int64 and keys.is_contiguous() and keys.numel() >= n * H * W
    _cams_check(intrs, extrs, n)
    tv = (C.c_int * max(1, n))(*[int(v) for v in target_views])
    _call("mvt_reproject_splat_depths", _ptr(depths), _ptr(conf), _ptr(_f32c(kinv)), _ptr(_f32c(einv)), V, T, t, H, W,
          0.0 if conf_thresh is None else conf_thresh, C.cast(tv, C.c_void_p), n, _ptr(intrs), _ptr(extrs), int(exclude_self), min_depth, splat,
          _ptr(keys), _stream())


def reproject_splat_points(points, M, n_targets, intrs, extrs, H, W, min_depth, splat, keys):
    """points (M, 3) fp32 into n_targets cameras: keys (n_targets, H*W) int64 words take the minimum; the index is the row."""
    assert points.dtype == torch.float32 and points.is_contiguous() and points.numel() >= M * 3
    assert keys.dtype == torch.int64 and keys.is_contiguous() and keys.numel() >= n_targets * H * W
    _cams_check(intrs, extrs, n_targets)
    _call("mvt_reproject_splat_points", _ptr(points), M, n_targets, _ptr(intrs), _ptr(extrs), H, W, min_depth, splat, _ptr(keys), _stream())


def reproject_resolve(keys, n_targets, H, W, index, depth, color, target_stride=1, rgbs=None, V=0, T=0, t=0, colors=None):
    """keys -> index (int32), depth (fp32), color (uint8, planar), target k at image k * target_stride of each; the colour from frame t
    of rgbs (V,T,3,H,W) uint8 / fp32 (clip form) or from colors (M, 3) uint8 (list form)."""
    need = ((n_targets - 1) * target_stride + 1) * H * W
    assert keys.dtype == torch.int64 and keys.is_contiguous() and keys.numel() >= n_targets * H * W
    assert index.dtype == torch.int32 and depth.dtype == torch.float32 and color.dtype == torch.uint8
    assert index.is_contiguous() and depth.is_contiguous() and color.is_contiguous()
    assert index.numel() >= need and depth.numel() >= need and color.numel() >= 3 * need
    assert (rgbs is None) != (colors is None)
    M = 0
    if colors is not None:
        assert colors.dtype == torch.uint8 and colors.is_contiguous() and colors.dim() == 2 and colors.shape[1] == 3
        M = colors.shape[0]
    else:
        assert rgbs.dtype in (torch.uint8, torch.float32) and rgbs.is_contiguous() and rgbs.numel() == V * T * 3 * H * W
    _call("mvt_reproject_resolve", _ptr(keys), n_targets, H, W, _ptr(rgbs), int(rgbs is not None and rgbs.dtype == torch.uint8), V, T, t,
          _ptr(colors), M, target_stride, _ptr(index), _ptr(depth), _ptr(color), _stream())


def photometric_blocks(H, W):
    """Workspace records per image of ``photometric_score``; raises for a size it refuses (H, W >= 6)."""
    n = _lib.mvt_photometric_blocks(H, W)
    if n <= 0:
        raise HipError(f"mvt_photometric_blocks refused {H} x {W} (the SSIM window needs H, W >= 6)")
    return n


def photometric_score(a, b, index, depth, target_depth, n, H, W, depth_tol, scores, partial=None):
    """scores (n, SCORE_WORDS) int64 words (the SCORE_DOUBLES are doubles: ``scores.view(torch.float64)``) of the renders a against
    the frames b, both (n, 3, H, W) uint8 / fp32, with the renders' index / depth (n, H, W) and the targets' depth maps."""
    for img in (a, b):
        assert img.dtype in (torch.uint8, torch.float32) and img.is_contiguous() and img.numel() >= n * 3 * H * W
    assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() >= n * H * W
    assert depth.dtype == target_depth.dtype == torch.float32 and depth.is_contiguous() and target_depth.is_contiguous()
    assert depth.numel() >= n * H * W and target_depth.numel() >= n * H * W
    assert scores.dtype == torch.int64 and scores.is_contiguous() and scores.numel() >= n * SCORE_WORDS
    if partial is None:
        partial = torch.empty(n * photometric_blocks(H, W) * SCORE_WORDS, dtype=torch.int64, device=scores.device)
    assert partial.dtype == torch.int64 and partial.is_contiguous() and partial.numel() >= n * max(1, _lib.mvt_photometric_blocks(H, W)) * SCORE_WORDS
    _call("mvt_photometric_score", _ptr(a), int(a.dtype == torch.uint8), _ptr(b), int(b.dtype == torch.uint8), _ptr(index), _ptr(depth),
          _ptr(target_depth), n, H, W, depth_tol, _ptr(partial), _ptr(scores), _stream())


# ------------------------------------------------------------------ region clustering (mvtracker_amd/cluster.py drives these)
CLUSTER_CANDIDATES, CLUSTER_CORE, CLUSTER_CLUSTERS, CLUSTER_CHOSEN, CLUSTER_CHOSEN_SIZE, CLUSTER_NOISE, CLUSTER_FALLBACK, CLUSTER_STATUS = range(8)
CLUSTER_STATE_WORDS = 8  # MVT_CLUSTER_*
CLUSTER_FEW, CLUSTER_NONE, CLUSTER_EMPTY = 1, 2, 3


def _cluster_check(xyz, Cn, Pn, box, gbox, core):
    nt = (Pn + 63) // 64
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.numel() >= Cn * Pn * 4
    assert box.dtype == torch.float32 and box.numel() >= Cn * nt * 8 and gbox.dtype == torch.float32 and gbox.numel() >= Cn * ((nt + 63) // 64) * 8
    assert core.dtype == torch.uint8 and core.is_contiguous() and core.numel() >= Cn * Pn


def cluster_crop(xyz, Cn, Pn, region_T_world, bounds):
    """In place: points of the Cn clouds xyz (Cn, Pn, 4) that are not strictly inside ``bounds`` = (xlo, xhi, ylo, yhi, zlo, zhi)
    in the frame region_T_world (Cn, 3, 4) fp32 become NaN rows."""
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.numel() >= Cn * Pn * 4
    assert region_T_world.dtype == torch.float32 and region_T_world.is_contiguous() and region_T_world.numel() >= Cn * 12
    b = (C.c_float * 6)(*[float(v) for v in bounds])
    _call("mvt_cluster_crop", _ptr(xyz), Cn, Pn, _ptr(region_T_world), b, _stream())


def cluster_count(xyz, Cn, Pn, grid, r2, min_samples, box, gbox, core):
    """core (Cn, Pn) uint8 <- 1 where a point of xyz (Cn, Pn, 4) has at least min_samples points (itself included) with d2 <= r2."""
    _cluster_check(xyz, Cn, Pn, box, gbox, core)
    _call("mvt_cluster_count", _ptr(xyz), Cn, Pn, grid[0], grid[1], r2, min_samples, _ptr(box), _ptr(gbox), _ptr(core), _stream())


def cluster_link(xyz, Cn, Pn, grid, r2, box, gbox, core, parent, state):
    """parent (Cn, Pn) int32 <- for core points the lowest core index of their component; state (Cn, CLUSTER_STATE_WORDS) int64 is
    cleared and its status word written."""
    _cluster_check(xyz, Cn, Pn, box, gbox, core)
    assert parent.dtype == torch.int32 and parent.is_contiguous() and parent.numel() >= Cn * Pn
    assert state.dtype == torch.int64 and state.is_contiguous() and state.numel() >= Cn * CLUSTER_STATE_WORDS
    _call("mvt_cluster_link", _ptr(xyz), Cn, Pn, grid[0], grid[1], r2, _ptr(box), _ptr(gbox), _ptr(core), _ptr(parent), _ptr(state), _stream())


def cluster_border(xyz, Cn, Pn, grid, r2, box, gbox, core, parent, root):
    """root (Cn, Pn) int32 <- parent for core points, the lowest parent among the core neighbours for the others, -1 without one."""
    _cluster_check(xyz, Cn, Pn, box, gbox, core)
    for t in (parent, root):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= Cn * Pn
    _call("mvt_cluster_border", _ptr(xyz), Cn, Pn, grid[0], grid[1], r2, _ptr(box), _ptr(gbox), _ptr(core), _ptr(parent), _ptr(root), _stream())


def cluster_finish(xyz, Cn, Pn, min_samples, core, root, sizes, labels, select, state):
    """labels (Cn, Pn) int32, select (Cn, Pn) uint8 and words 0..6 of state; sizes (Cn, Pn) int32 is workspace."""
    assert xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.numel() >= Cn * Pn * 4
    assert core.dtype == torch.uint8 and core.numel() >= Cn * Pn and select.dtype == torch.uint8 and select.numel() >= Cn * Pn
    for t in (root, sizes, labels):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= Cn * Pn
    assert state.dtype == torch.int64 and state.is_contiguous() and state.numel() >= Cn * CLUSTER_STATE_WORDS
    _call("mvt_cluster_finish", _ptr(xyz), Cn, Pn, min_samples, _ptr(core), _ptr(root), _ptr(sizes), _ptr(labels), _ptr(select), _ptr(state),
          _stream())


# ------------------------------------------------------------------ motion masks (mvtracker_amd/motion.py drives these)
MOTION_MAX_RADIUS = 15  # MVT_MOTION_MAX_RADIUS


def motion_blocks(H, W):
    """Rows per view of ``motion_temporal``'s partial sums; raises for a size it refuses."""
    n = _lib.mvt_motion_blocks(H, W)
    if n <= 0:
        raise HipError(f"mvt_motion_blocks refused {H} x {W}")
    return n


def motion_tiles(H, W):
    """Counts per image of ``motion_mask``; raises for a size it refuses."""
    n = _lib.mvt_motion_tiles(H, W)
    if n <= 0:
        raise HipError(f"mvt_motion_tiles refused {H} x {W}")
    return n


def motion_temporal(rgbs, V, T, H, W, all_mode, out, partial):
    """One pass over rgbs (V, T, 3, H, W) uint8 / fp32: out (V, H, W) <- the largest boundary diff (``all_mode``) or out
    (V, T-1, H, W) <- every boundary's diff; partial (V * motion_blocks(H, W), T-1) fp64 <- the workgroups' sums of |dc0|+|dc1|+|dc2|."""
    assert rgbs.dtype in (torch.uint8, torch.float32) and rgbs.is_contiguous() and rgbs.numel() == V * T * 3 * H * W
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= V * (1 if all_mode else T - 1) * H * W
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.numel() >= V * motion_blocks(H, W) * (T - 1)
    _call("mvt_motion_temporal", _ptr(rgbs), int(rgbs.dtype == torch.uint8), V, T, H, W, int(bool(all_mode)), _ptr(out), _ptr(partial), _stream())


def motion_mask(src, V, T, H, W, win, r, thresh, mask, counts):
    """mask (V, T, H, W) bool <- static pixels.  win >= 1: src is ``motion_temporal``'s (V, T-1, H, W); win == 0: its all_mode
    (V, H, W), pooled once and written to every frame.  counts (V * T or V, motion_tiles(H, W)) int32 <- static pixels per tile."""
    assert src.dtype == torch.float32 and src.is_contiguous() and src.numel() >= V * (T - 1 if win > 0 else 1) * H * W
    assert mask.dtype == torch.bool and mask.is_contiguous() and mask.numel() == V * T * H * W
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= V * (T if win > 0 else 1) * motion_tiles(H, W)
    _call("mvt_motion_mask", _ptr(src), V, T, H, W, win, r, thresh, _ptr(mask), _ptr(counts), _stream())


def motion_report(partial, counts, V, T, H, W, all_mode, report):
    """report (T-1 + V*T) fp64 <- the boundary sums, then the static pixels of every (view, frame), added in a fixed order."""
    assert partial.dtype == torch.float64 and partial.is_contiguous() and partial.numel() >= V * motion_blocks(H, W) * (T - 1)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= V * (1 if all_mode else T) * motion_tiles(H, W)
    assert report.dtype == torch.float64 and report.is_contiguous() and report.numel() >= T - 1 + V * T
    _call("mvt_motion_report", _ptr(partial), _ptr(counts), V, T, H, W, int(bool(all_mode)), _ptr(report), _stream())


# ------------------------------------------------------------------ track overlays (mvtracker_amd/overlay.py drives these)
OVERLAY_MAX_LINEWIDTH, OVERLAY_MAX_PAD, OVERLAY_MAX_SIDE, OVERLAY_MAX_INDEX = 8, 64, 8192, 1 << 20  # MVT_OVERLAY_*


def overlay_project(tracks, intrs, extrs, V, T, N, xyz=None, points=None, pad=0, min_depth=None, query_frames=None, frame0=0, lut=None,
                    color_view=0, Hp=0, colors=None):
    """tracks (T, N, 3), intrs (V, T, 3, 3), extrs (V, T, 3, 4) fp32 -> any of xyz (V, T, N, 3) fp32 <- (px, py, camera z); points
    (T, V, N, 4) int32 <- (x, y, valid, 0); with ``lut`` (256, 3) uint8, colors (N, 3) uint8 rows of the tracks whose query frame is
    one of frame0 .. frame0 + T - 1."""
    for a, shape in ((tracks, (T, N, 3)), (intrs, (V, T, 3, 3)), (extrs, (V, T, 3, 4))):
        assert tuple(_f32c(a).shape) == shape, (tuple(a.shape), shape)
    assert xyz is None or (tuple(_f32c(xyz).shape) == (V, T, N, 3))
    assert points is None or (points.dtype == torch.int32 and points.is_contiguous() and tuple(points.shape) == (T, V, N, 4))
    if lut is not None:
        assert lut.dtype == torch.uint8 and lut.is_contiguous() and tuple(lut.shape) == (256, 3)
        assert colors.dtype == torch.uint8 and colors.is_contiguous() and tuple(colors.shape) == (N, 3)
        assert query_frames.dtype == torch.int32 and query_frames.is_contiguous() and query_frames.numel() == N
    _call("mvt_overlay_project", _ptr(tracks), _ptr(intrs), _ptr(extrs), V, T, N, _ptr(xyz), _ptr(points), pad, int(min_depth is not None),
          0.0 if min_depth is None else float(min_depth), _ptr(query_frames) if lut is not None else None, frame0, _ptr(lut), color_view, Hp,
          _ptr(colors) if lut is not None else None, _stream())


def overlay_draw(prev, cur, visibility, query_frames, colors, V, N, M, t, linewidth, Hp, Wp, line_keys, marker_keys):
    """The markers of frame t (cur (V, N, 4) int32) into marker_keys and, with prev (frame t-1) and line_keys, the segments t-1 -> t
    into line_keys, both (V, Hp, Wp) int64 holding unsigned keys.  visibility (N) bool of frame t or None."""
    for p in (prev, cur):
        assert p is None or (p.dtype == torch.int32 and p.is_contiguous() and tuple(p.shape) == (V, N, 4))
    assert visibility is None or (visibility.dtype in (torch.bool, torch.uint8) and visibility.is_contiguous() and visibility.numel() == N)
    assert query_frames.dtype == torch.int32 and query_frames.is_contiguous() and query_frames.numel() == N
    assert colors.dtype == torch.uint8 and colors.is_contiguous() and tuple(colors.shape) == (N, 3)
    for k in (line_keys, marker_keys):
        assert k is None or (k.dtype == torch.int64 and k.is_contiguous() and tuple(k.shape) == (V, Hp, Wp))
    _call("mvt_overlay_draw", _ptr(prev), _ptr(cur), _ptr(visibility), _ptr(query_frames), _ptr(colors), V, N, M, t, linewidth, Hp, Wp,
          _ptr(line_keys), _ptr(marker_keys), _stream())


def overlay_compose(frames, V, T, t_local, H, W, pad, line_keys, first_segment, marker_keys, out):
    """out[:, t_local] of (V, T, 3, H + 2 pad, W + 2 pad) uint8 <- markers over the lines of segments >= first_segment over
    frames[:, t_local] of (V, T, 3, H, W) uint8 or fp32 over the white border; marker_keys is zero again afterwards."""
    Hp, Wp = H + 2 * pad, W + 2 * pad
    assert frames.dtype in (torch.uint8, torch.float32) and frames.is_contiguous() and tuple(frames.shape) == (V, T, 3, H, W)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (V, T, 3, Hp, Wp)
    for k in (line_keys, marker_keys):
        assert k is None or (k.dtype == torch.int64 and k.is_contiguous() and tuple(k.shape) == (V, Hp, Wp))
    _call("mvt_overlay_compose", _ptr(frames), int(frames.dtype == torch.uint8), V, T, t_local, H, W, pad, _ptr(line_keys), first_segment,
          _ptr(marker_keys), _ptr(out), _stream())


# ------------------------------------------------------------------ mask queries (mvtracker_amd/masks.py drives these)
MASK_LABELS, MASK_MAX_LABEL, MASK_MAX_VIEWS, MASK_FRAC_BITS, MASK_RANGE_BITS = 256, 255, 64, 20, 18  # MVT_MASK_*
MASK_STAT_WORDS, MASK_PIXELS, MASK_COUNT, MASK_SUM, MASK_OUT_OF_RANGE = 6, 0, 1, 2, 5


def _mask_clip_check(labels, depths, conf, kinv, einv, V, T, H, W):
    assert labels.dtype == torch.uint8 and labels.is_contiguous() and tuple(labels.shape) == (V, T, H, W)
    assert depths.dtype == torch.float32 and depths.is_contiguous() and depths.numel() == V * T * H * W
    assert conf is None or (conf.dtype == torch.float32 and conf.is_contiguous() and conf.numel() == V * T * H * W)
    assert _f32c(kinv).numel() == V * T * 9 and _f32c(einv).numel() == V * T * 12


def mask_stats(labels, depths, conf, kinv, einv, V, T, H, W, min_depth, max_depth, conf_thresh, stats):
    """stats (V, T, 256, MASK_STAT_WORDS) int64 <- per (view, frame, label): labelled pixels, valid pixels in range, their
    fixed-point coordinate sums, valid pixels out of range.  labels (V, T, H, W) uint8; conf_thresh is read only with ``conf``."""
    _mask_clip_check(labels, depths, conf, kinv, einv, V, T, H, W)
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() == V * T * MASK_LABELS * MASK_STAT_WORDS
    _call("mvt_mask_stats", _ptr(labels), _ptr(depths), _ptr(conf), _ptr(kinv), _ptr(einv), V, T, H, W, min_depth, max_depth,
          0.0 if conf is None else conf_thresh, _ptr(stats), _stream())


def mask_centroids(stats, V, T, min_pixels, centroid):
    """centroid (V, T, 256, 3) fp64 <- sum / count * 2^-20 where count >= min_pixels, NaN elsewhere."""
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() == V * T * MASK_LABELS * MASK_STAT_WORDS
    assert centroid.dtype == torch.float64 and centroid.is_contiguous() and centroid.numel() == V * T * MASK_LABELS * 3
    _call("mvt_mask_centroids", _ptr(stats), V, T, min_pixels, _ptr(centroid), _stream())


def mask_match(centroid, V, T, min_common_frames, distance_threshold, match, ids, global_id, distance, state):
    """global_id (V, 256) int32, distance (V, 256) fp64, state (2,) int32 = (objects, present ids) <- the greedy matching of the
    centroids (V, T, 256, 3); ids: workspace (V * 256,) int32."""
    assert centroid.dtype == torch.float64 and centroid.is_contiguous() and centroid.numel() == V * T * MASK_LABELS * 3
    for a, n in ((ids, V * MASK_LABELS), (global_id, V * MASK_LABELS), (state, 2)):
        assert a.dtype == torch.int32 and a.is_contiguous() and a.numel() == n
    assert distance.dtype == torch.float64 and distance.is_contiguous() and distance.numel() == V * MASK_LABELS
    _call("mvt_mask_match", _ptr(centroid), V, T, min_common_frames, distance_threshold, int(bool(match)), _ptr(ids), _ptr(global_id),
          _ptr(distance), _ptr(state), _stream())


def mask_relabel(labels, table, V, T, H, W, out):
    """out (V, T, H, W) int32 <- table[v][label], -1 for background; table (V, 256) int32."""
    assert labels.dtype == torch.uint8 and labels.is_contiguous() and tuple(labels.shape) == (V, T, H, W)
    assert table.dtype == torch.int32 and table.is_contiguous() and table.numel() == V * MASK_LABELS
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (V, T, H, W)
    _call("mvt_mask_relabel", _ptr(labels), _ptr(table), V, T, H, W, _ptr(out), _stream())


def mask_pool(labels, depths, conf, kinv, einv, V, T, t, H, W, min_depth, max_depth, conf_thresh, table, obj, pool, pixel, count, block_counts):
    """The pool of (object ``obj``, frame t): pool (capacity, 3) fp32 <- world points, pixel (capacity,) int32 <- raster indices, in
    raster order; count (1,) int32 <- the pool's size.  Nothing is written past ``capacity = len(pixel)`` rows."""
    _mask_clip_check(labels, depths, conf, kinv, einv, V, T, H, W)
    assert table.dtype == torch.int32 and table.is_contiguous() and table.numel() == V * MASK_LABELS
    capacity = pixel.numel()
    assert pool.dtype == torch.float32 and pool.is_contiguous() and pool.numel() == capacity * 3
    assert pixel.dtype == torch.int32 and pixel.is_contiguous() and count.dtype == torch.int32 and count.numel() >= 1
    assert block_counts.dtype == torch.int32 and block_counts.numel() >= (V * H * W + 255) // 256
    _call("mvt_mask_pool", _ptr(labels), _ptr(depths), _ptr(conf), _ptr(kinv), _ptr(einv), V, T, t, H, W, min_depth, max_depth,
          0.0 if conf is None else conf_thresh, _ptr(table), obj, capacity, _ptr(pool) if capacity else None, _ptr(pixel) if capacity else None,
          _ptr(count), _ptr(block_counts), _stream())


# ------------------------------------------------------------------ rigid object motion (mvtracker_amd/rigid.py drives these)
RIGID_MAX_OBJECTS, RIGID_MAX_ITERATIONS, RIGID_MAX_FRAMES = 65535, 64, 65535  # MVT_RIGID_*
RIGID_OK, RIGID_TOO_FEW, RIGID_DEGENERATE = 0, 1, 2
RIGID_FILL_OCCLUDED, RIGID_FILL_OUTLIERS = 1, 2


def _i32(t, n):
    assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n, (t.dtype, tuple(t.shape), n)
    return t


def _u8(t, n):
    """(bool and uint8 tensors are both one byte of 0 / 1 per element)"""
    assert t.dtype in (torch.bool, torch.uint8) and t.is_contiguous() and t.numel() == n, (t.dtype, tuple(t.shape), n)
    return t


def _rigid_dims(T, N, G):
    assert 1 <= T <= RIGID_MAX_FRAMES and 1 <= N <= 1 << 30 and 1 <= G <= RIGID_MAX_OBJECTS, (T, N, G)


def rigid_members(object_ids, query_frames, N, G, T, counts, offsets, members, reference_frames):
    """counts (G), offsets (G + 1), members (N), reference_frames (G) int32 <- the member lists of the objects 0..G-1 in ascending
    track order and every object's largest query frame (clamped to the clip; -1 without members)."""
    _rigid_dims(T, N, G)
    _i32(object_ids, N), _i32(query_frames, N), _i32(counts, G), _i32(offsets, G + 1), _i32(members, N), _i32(reference_frames, G)
    _call("mvt_rigid_members", _ptr(object_ids), _ptr(query_frames), N, G, T, _ptr(counts), _ptr(offsets), _ptr(members), _ptr(reference_frames),
          _stream())


def rigid_fit(tracks, visibility, query_frames, object_ids, offsets, members, reference_frames, T, N, G, inlier_threshold, iterations, min_points,
              use_visibility, min_spread, live_before_query, poses, residual, inliers, used, inlier_count, rmse, status):
    """poses (G, T, 4, 4) fp32, residual (T, N) fp32, inliers (T, N) bool, used / inlier_count / status (G, T) int32, rmse (G, T) fp32
    <- the weighted Kabsch fit of every (object, frame) with its inlier refits; tracks (T, N, 3) fp32, visibility (T, N) bool."""
    _rigid_dims(T, N, G)
    assert _f32c(tracks).numel() == T * N * 3 and _f32c(poses).numel() == G * T * 16 and _f32c(residual).numel() == T * N
    assert _f32c(rmse).numel() == G * T
    _u8(visibility, T * N), _u8(inliers, T * N)
    _i32(query_frames, N), _i32(object_ids, N), _i32(offsets, G + 1), _i32(members, N), _i32(reference_frames, G)
    _i32(used, G * T), _i32(inlier_count, G * T), _i32(status, G * T)
    assert 1 <= iterations <= RIGID_MAX_ITERATIONS and min_points >= 3 and inlier_threshold >= 0 and min_spread >= 0
    _call("mvt_rigid_fit", _ptr(tracks), _ptr(visibility), _ptr(query_frames), _ptr(object_ids), _ptr(offsets), _ptr(members),
          _ptr(reference_frames), T, N, G, float(inlier_threshold), iterations, min_points, int(bool(use_visibility)), float(min_spread),
          int(bool(live_before_query)), _ptr(poses), _ptr(residual), _ptr(inliers), _ptr(used), _ptr(inlier_count), _ptr(rmse), _ptr(status),
          _stream())


def rigid_compose(poses, status, G, T, frame, xf):
    """xf (G, T, 3, 4) fp64 <- rows 0..2 of pose[g, t] (frame None) or of pose[g, t] pose[g, frame]^-1, NaN where a status it needs is
    not 0."""
    _rigid_dims(T, 1, G)
    assert _f32c(poses).numel() == G * T * 16 and xf.dtype == torch.float64 and xf.is_contiguous() and xf.numel() == G * T * 12
    _i32(status, G * T)
    frame = -1 if frame is None else int(frame)
    assert -1 <= frame < T, frame
    _call("mvt_rigid_compose", _ptr(poses), _ptr(status), G, T, frame, _ptr(xf), _stream())


def rigid_move(points, point_objects, xf, M, T, G, out):
    """out (T, M, 3) fp32 <- xf[point_objects[m], t] applied to points[m]; NaN for ids outside [0, G)."""
    _rigid_dims(T, M, G)
    assert _f32c(points).numel() == M * 3 and _f32c(out).numel() == T * M * 3
    assert xf.dtype == torch.float64 and xf.is_contiguous() and xf.numel() == G * T * 12
    _i32(point_objects, M)
    _call("mvt_rigid_move", _ptr(points), _ptr(point_objects), _ptr(xf), M, T, G, _ptr(out), _stream())


def rigid_fill(tracks, visibility, inliers, query_frames, object_ids, reference_frames, poses, status, T, N, G, replace, live_before_query, out,
               filled):
    """out (T, N, 3) fp32 <- tracks with the occluded (replace & 1) and / or outlying (replace & 2) points of live members under a
    status-0 pose replaced by pose * (the member's reference point); filled (T, N) bool <- where."""
    _rigid_dims(T, N, G)
    assert _f32c(tracks).numel() == T * N * 3 and _f32c(out).numel() == T * N * 3 and out.data_ptr() != tracks.data_ptr()
    assert _f32c(poses).numel() == G * T * 16 and 0 <= replace <= 3
    _u8(visibility, T * N), _u8(inliers, T * N), _u8(filled, T * N)
    _i32(query_frames, N), _i32(object_ids, N), _i32(reference_frames, G), _i32(status, G * T)
    _call("mvt_rigid_fill", _ptr(tracks), _ptr(visibility), _ptr(inliers), _ptr(query_frames), _ptr(object_ids), _ptr(reference_frames),
          _ptr(poses), _ptr(status), T, N, G, replace, int(bool(live_before_query)), _ptr(out), _ptr(filled), _stream())
