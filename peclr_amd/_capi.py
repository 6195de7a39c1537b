"""ctypes binding of libpeclr_hip.so (include/peclr_hip.h) for torch device tensors.

This is the ONLY place the product touches the native library, and there is no fallback:
if the library is missing, or a tensor is not a contiguous fp32 HIP tensor, the call raises.
PyTorch is plumbing here (device memory + the current hipStream_t); every function below is a
thin argument marshaller around one C entry point.
"""
from __future__ import annotations

import ctypes
import os
import struct
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p
from typing import Optional

import torch  # must be imported BEFORE the CDLL: the .so binds to torch's libamdhip64.so.7

# (PECLR_HIP_LIB: another build of the same library, for same-box A/B runs of a kernel change)
_LIB_PATH = os.environ.get("PECLR_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpeclr_hip.so")
_LIB = None

GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
DTYPE_F32, DTYPE_BF16, DTYPE_F16, DTYPE_F64 = 0, 1, 2, 3   # PECLR_DTYPE_*: the element type of an activation tensor
ALIGN_CROP, ALIGN_ROTATE, ALIGN_SINGLE_NORM = 1, 2, 4
OPT_CHUNK = 4096

# name -> (restype, argtypes); mirrors include/peclr_hip.h one to one
_P = c_void_p
SIGNATURES = {
    "peclr_version": (c_int, []),
    "peclr_error_string": (c_char_p, [c_int]),
    "peclr_stream_capture_id": (c_int, [_P, _P]),
    "peclr_gemm_f32": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P, _P]),
    "peclr_gemm_add_f32": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P]),
    "peclr_gemm_add_bf16": (c_int, [c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P]),
    "peclr_gemm_add_f16": (c_int, [c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P]),
    "peclr_gemm_pick_split_k": (c_int, [c_int, c_int, c_int]),
    "peclr_slab_reduce_f32": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    "peclr_bn_relu_fwd_f32": (c_int, [_P, c_int, _P, c_int, c_int, _P, _P, c_float, c_float, c_int, _P, _P,
                                      _P, _P, _P, _P, _P, _P]),
    "peclr_bn_relu_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "peclr_align_fwd_f32": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_float, c_float,
                                    _P, _P, _P, _P, _P, _P, _P]),
    "peclr_align_bwd_f32": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "peclr_ntxent_jsplit": (c_int, [c_int, c_int, c_int]),
    "peclr_ntxent_fwd_f32": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, _P, _P, _P, c_int, _P]),
    "peclr_ntxent_finalize_f32": (c_int, [_P, c_int, _P, c_int, c_float, _P, _P, c_int, _P, _P]),
    "peclr_ntxent_bwd_f32": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_float, _P, _P, c_float, _P,
                                     c_int, _P]),
    "peclr_stem_pack_bytes": (c_int, [c_int]),
    "peclr_stem_pack": (c_int, [_P, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _P, c_int, _P]),
    "peclr_stem_workgroups": (c_int, [c_int, c_int, c_int]),
    "peclr_stem_conv7x7_s2": (c_int, [_P, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    "peclr_stem_wgrad_slabs": (c_int, [c_int, c_int, c_int, c_int]),
    "peclr_stem_wgrad": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, c_int, _P]),
    "peclr_bn2d_n_split": (c_int, [c_int, c_int, c_int]),
    "peclr_bn2d_stats": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_int, _P]),
    "peclr_bn2d_combine_f64": (c_int, [_P, c_int, c_int, _P, _P]),
    "peclr_bn2d_finalize_totals_f32": (c_int, [_P, _P, c_int, c_float, c_float, _P, _P, _P, _P, _P, _P, _P, _P,
                                               _P]),
    "peclr_bn2d_bwd_finalize_totals_f32": (c_int, [_P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "peclr_bn2d_finalize_f32": (c_int, [_P, c_int, c_int, c_int, c_int, c_float, c_float, _P, _P, _P, _P, _P, _P,
                                        _P, _P, _P]),
    "peclr_bn2d_apply": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    "peclr_bn2d_apply_res_bn": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    "peclr_bn2d_bwd_reduce": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P]),
    "peclr_bn2d_bwd_finalize_f32": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "peclr_bn2d_bwd_apply": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_bn2d_bwd_apply_res_bn": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_bn2d_apply_avgpool": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "peclr_bn2d_bwd_reduce_avgpool": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P]),
    "peclr_bn2d_bwd_apply_avgpool": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_bn2d_pool_n_split": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "peclr_bn2d_pool_apply": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "peclr_bn2d_pool_bwd_reduce": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P]),
    "peclr_bn2d_pool_bwd_apply": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "peclr_augment_warp_crop_u8": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "peclr_augment_resize_color_norm": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, c_int, _P, _P, c_int, _P,
                                                _P]),
    "peclr_augment_pre_u8": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P]),
    "peclr_augment_resize_color_norm_ext": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, c_uint64,
                                                    c_uint32, c_int, c_int, _P, _P, c_int, _P, _P]),
    "peclr_augment_pre_ragged_u8": (c_int, [_P, c_int, c_int, _P, c_int64, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P]),
    "peclr_augment_warp_crop_ragged_u8": (c_int, [_P, c_int, c_int, _P, _P, _P, c_int, c_int, _P, _P]),
    "peclr_augment_resize_color_norm_ragged": (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, _P, _P, c_int, _P, _P]),
    "peclr_augment_warp_crop_mirror_u8": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "peclr_augment_pre_mirror_u8": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P, _P]),
    "peclr_augment_pre_ragged_mirror_u8": (c_int, [_P, c_int, c_int, _P, c_int64, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P,
                                                   _P]),
    "peclr_augment_warp_crop_ragged_mirror_u8": (c_int, [_P, c_int, c_int, _P, _P, _P, c_int, c_int, _P, _P, _P]),
    "peclr_augment_resize_color_norm_ragged_ext": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, c_int, c_uint64, c_uint32,
                                                           c_int, c_int, _P, _P, c_int, _P, _P]),
    "peclr_augment_draw_views": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_uint64, _P, _P, _P, _P, _P,
                                         _P, _P]),
    "peclr_gemm_x6_f32": (c_int, [c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P, c_int, _P]),
    "peclr_gemm_x6_tn_slabs": (c_int, [c_int, c_int, c_int]),
    "peclr_gemm_x6_tn_f32": (c_int, [c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P]),
    "peclr_x6_pack_bytes": (c_int64, [c_int, c_int]),
    "peclr_x6_pack_f32": (c_int, [_P, c_int, c_int, _P]),
    "peclr_x6_pack_pair_bytes": (c_int64, [c_int, c_int]),
    "peclr_x6_absmax_f32": (c_int, [_P, c_int, c_int, _P, _P]),
    "peclr_x6_pack_pair_f32": (c_int, [_P, c_int, c_int, _P, _P, _P]),
    "peclr_gemm_x6p_tile_rows": (c_int, [c_int, c_int, c_int]),
    "peclr_gemm_x6p_f32": (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "peclr_conv3x3_s2_dgrad_x6p_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, _P]),
    "peclr_gemm_x6p_s2add_f32": (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "peclr_gemm_x6p_maskadd_f32": (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, c_int, _P, c_int, _P, _P, _P]),
    "peclr_gemm_x6t_slabs": (c_int, [c_int, c_int, c_int, c_int]),
    "peclr_gemm_x6t_f32": (c_int, [c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "peclr_conv_s2_x6p_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, _P]),
    "peclr_conv3x3_x6p_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "peclr_h_pack_bytes": (c_int64, [c_int, c_int]),
    "peclr_h_pack": (c_int, [_P, c_int, c_int, _P]),
    "peclr_conv_h_tile_rows": (c_int, [c_int, c_int]),
    "peclr_conv_h_row_blocks": (c_int, [c_int] * 7),
    "peclr_gemm_h": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    "peclr_conv_h": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    "peclr_gemm_h_bnact": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_int, _P, c_int, _P, c_int, c_int, _P]),
    "peclr_conv_h_bnact": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, c_int, _P]),
    "peclr_bn2d_eval_tables": (c_int, [_P, c_int, c_int, _P]),
    "peclr_conv3x3_s2_dgrad_h": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P]),
    "peclr_wgrad3_h_slabs": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "peclr_wgrad3_h": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P]),
    "peclr_wgrad3w_h_slabs": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "peclr_wgrad3w_h": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P]),
    "peclr_wgrad3s2_h_slabs": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "peclr_wgrad3s2_h": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P]),
    "peclr_wgrad_h_slabs": (c_int, [c_int, c_int, c_int]),
    "peclr_wgrad_h": (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "peclr_lars_sumsq_f32": (c_int, [_P, _P, c_int, _P, _P, c_int, _P, _P]),
    "peclr_lars_adam_update_f32": (c_int, [_P, _P, c_int, _P, _P, _P, _P, c_int, _P, _P, _P, _P, c_int, c_float,
                                           c_float, c_float, c_float, c_float, c_int, c_float, c_float, c_int,
                                           _P]),
    "peclr_lars_sumsq_amp_f32": (c_int, [_P, _P, c_int, _P, _P, c_int, _P, _P, _P]),
    "peclr_lars_adam_update_amp_f32": (c_int, [_P, _P, c_int, _P, _P, _P, _P, c_int, _P, _P, _P, _P, c_int, c_double,
                                               c_double, c_float, c_int, c_float, c_float, c_int, _P, _P]),
    "peclr_amp_update": (c_int, [_P, c_float, c_float, c_int, _P]),
    "peclr_pose_crop_u8": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P]),
    "peclr_pose_head_f32": (c_int, [_P, c_int, c_int, _P, _P, _P, c_float, c_float, _P, c_int, c_float, _P, _P, _P, _P, c_int,
                                    _P, _P, _P, _P]),
    "peclr_pose_crop_ragged_u8": (c_int, [_P, c_int64, c_int, _P, _P, _P, _P, c_int, _P, _P, _P]),
    "peclr_pose_unmap": (c_int, [_P, _P, _P, _P, _P, c_int, _P, _P, _P, _P]),
    "peclr_pose_head_train_fwd_f32": (c_int, [_P, c_int, c_int, _P, _P, _P, c_float, c_float, c_float, c_float, _P, _P, _P, c_int,
                                              c_float, _P, _P, _P, _P, _P]),
    "peclr_pose_head_train_bwd_f32": (c_int, [_P, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_pose_head_train_launches": (c_int, [c_int, c_int]),
    "peclr_pose_eval": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, c_int, _P]),
    "peclr_joints3d_to_25d": (c_int, [_P, _P, c_int, _P, _P, _P]),
    "peclr_joints25d_to_3d": (c_int, [_P, _P, _P, _P, c_int, _P, _P, _P]),
    "peclr_supervised_labels": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_supervised_labels_mirror": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_pose_loss": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "peclr_pose_loss_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
    "peclr_pose_step_metrics_f32": (c_int, [_P, _P, _P, _P, c_int, _P, _P, _P]),
}


class PeclrHipError(RuntimeError):
    pass


def library_path() -> str:
    return _LIB_PATH


def lib() -> ctypes.CDLL:
    """Load libpeclr_hip.so (once).  Raises if it has not been built -- there is no fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise PeclrHipError(
                f"{_LIB_PATH} is missing: build it with `make -C peclr_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "peclr_amd has no CPU or PyTorch fallback for its HIP kernels.")
        handle = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().peclr_error_string(rc).decode()
        raise PeclrHipError(f"{what} failed: {msg} (code {rc})")


def _ptr(t: Optional[torch.Tensor], dtype=torch.float32, what: str = "tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise PeclrHipError(f"{what}: expected a HIP device tensor, got device={t.device} "
                            "(peclr_amd has no CPU path)")
    if t.dtype != dtype:
        raise PeclrHipError(f"{what}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise PeclrHipError(f"{what}: tensor must be contiguous")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-kernel HIP-event timing (bench.py): one entry point = one launch, so an event
# pair recorded on the launch stream around a call times exactly that kernel.
EVENT_LOG = None  # None = off; dict name -> list[(start, end)] when bench.py turns it on
WEIGHTS_EPOCH = 0    # bumped by every fused optimiser launch (it updates the parameters through raw pointers)
TAG_BOUND_SUFFIX = False   # bench.py: launches of the six-product GEMMs whose OWN roof is HBM (layer1 / layer2's 1x1 shapes: 4 B/elem
#                            x (K + N) columns take longer at 8 TB/s than 2 K N flops at 417 TFLOP/s) log as "<tag>~hbm", so that a tag's
#                            average is never a mix of MFMA-bound and HBM-bound launches priced against one roof
LAUNCH_ORDER = None  # None = off; list of names in launch order (one entry per launch) while EVENT_LOG is on:
#                      lets tools/pmc_mfma.py align a rocprofv3 dispatch table with the bench's kernel names


class _timed:
    """`nbytes` / `flops`: the launch's ALGORITHMIC work when it is shape-dependent (summed per name); `kernel`: the
    kernel family that runs under this name when the entry point has more than one (bench.py prices a launch against
    the roof of the kernel that actually ran)."""
    __slots__ = ("name", "s", "e", "nbytes", "flops", "kernel")

    def __init__(self, name, nbytes=0, flops=0, kernel=None):
        # (the kernel's own matrix-core roof: dense bf16 / fp16 peak over six products, or over three in pair arithmetic)
        if (TAG_BOUND_SUFFIX and flops and nbytes and kernel and kernel.startswith("gemm_x6")
                and nbytes / 8e12 > flops / (833.3e12 if "<pair>" in kernel else 416.7e12)):
            name += "~hbm"
        self.name, self.nbytes, self.flops, self.kernel = name, nbytes, flops, kernel

    def __enter__(self):
        if EVENT_LOG is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()  # current stream == the stream the kernel is launched on
            if LAUNCH_ORDER is not None:
                LAUNCH_ORDER.append(self.name)

    def __exit__(self, *exc):
        if EVENT_LOG is not None:
            self.e.record()
            EVENT_LOG.setdefault(self.name, []).append((self.s, self.e, self.nbytes, self.flops, self.kernel))
        return False


def _call(name: str, *args):
    """Call the status-returning entry point `name` (a SIGNATURES key) with `args` as the header orders them -- the stream
    last, spelled out by the caller -- and raise under that same name if it refuses."""
    _check(getattr(lib(), name)(*args), name)


def _launch(tag: str, name: str, *args, nbytes=0, flops=0, kernel=None):
    """`_call` for an entry point that is one kernel launch, timed under `tag` (see `_timed`)."""
    with _timed(tag, nbytes, flops, kernel):
        rc = getattr(lib(), name)(*args)
    _check(rc, name)


def capture_id() -> int:
    """Identity of the hipGraph capture the current stream is in; 0 when it is not capturing."""
    if not torch.cuda.is_current_stream_capturing():
        return 0
    out = ctypes.c_ulonglong(0)
    _call("peclr_stream_capture_id", _stream(), ctypes.addressof(out))
    return int(out.value) or 1


# ------------------------------------------------------------------ GEMM
def pick_split_k(m: int, n: int, k: int) -> int:
    return lib().peclr_gemm_pick_split_k(m, n, k)


def gemm(layout: int, a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None,
         split_k: int = 1, tag: Optional[str] = None) -> torch.Tensor:
    """Returns C [M,N] (split_k == 1) or slabs [split_k, M, N]."""
    if layout == GEMM_NT:
        (m, k), (n, k2) = a.shape, b.shape
    elif layout == GEMM_NN:
        (m, k), (k2, n) = a.shape, b.shape
    else:
        (k, m), (k2, n) = a.shape, b.shape
    if k != k2:
        raise PeclrHipError(f"gemm: contraction mismatch {tuple(a.shape)} x {tuple(b.shape)} layout {layout}")
    if split_k == 1:
        out = torch.empty((m, n), device=a.device, dtype=torch.float32)
        c_ptr, slab_ptr = out.data_ptr(), None
    else:
        out = torch.empty((split_k, m, n), device=a.device, dtype=torch.float32)
        c_ptr, slab_ptr = None, out.data_ptr()
    _launch(tag or f"gemm_{('nt', 'nn', 'tn')[layout]}_{m}x{n}x{k}", "peclr_gemm_f32",
            layout, m, n, k, _ptr(a, what="gemm A"), a.stride(0), _ptr(b, what="gemm B"), b.stride(0), c_ptr, n,
            _ptr(bias, what="gemm bias"), split_k, slab_ptr, _stream())
    return out


def slab_reduce(slabs: torch.Tensor, bias: Optional[torch.Tensor] = None, tag: str = "slab_reduce") -> torch.Tensor:
    s, rows, cols = slabs.shape
    out = torch.empty((rows, cols), device=slabs.device, dtype=torch.float32)
    _launch(tag, "peclr_slab_reduce_f32", _ptr(slabs), s, rows, cols, _ptr(bias), out.data_ptr(), _stream(),
            nbytes=4 * (s + 1) * rows * cols, kernel="slab_reduce_kernel")
    return out


def _sum_slabs(slabs: torch.Tensor, tag: str = "slab_reduce") -> torch.Tensor:
    """The tail of every split-K wrapper: the only slab as it is, several summed in their fixed order."""
    return slabs[0] if slabs.shape[0] == 1 else slab_reduce(slabs, tag=tag)


# ------------------------------------------------------------------ BN + ReLU
def bn_relu_fwd(a_slabs, bias, gamma, beta, eps, momentum, training, running_mean, running_var,
                num_batches_tracked):
    s, m, h = a_slabs.shape
    dev = a_slabs.device
    a_pre = torch.empty((m, h), device=dev, dtype=torch.float32)
    a_out = torch.empty((m, h), device=dev, dtype=torch.float32)
    save = torch.empty((2, h), device=dev, dtype=torch.float32)
    _launch("bn_relu_fwd", "peclr_bn_relu_fwd_f32",
            _ptr(a_slabs), s, _ptr(bias), m, h, _ptr(gamma), _ptr(beta), eps, momentum, int(training),
            _ptr(running_mean), _ptr(running_var),
            _ptr(num_batches_tracked, torch.int64, "num_batches_tracked"), a_pre.data_ptr(), a_out.data_ptr(),
            save[0].data_ptr(), save[1].data_ptr(), _stream())
    return a_pre, a_out, save


def bn_relu_bwd(d_a_out, a_pre, save, gamma, beta, training=True):
    m, h = a_pre.shape
    d_a_pre = torch.empty_like(a_pre)
    dparams = torch.empty((3, h), device=a_pre.device, dtype=torch.float32)  # dgamma, dbeta, dbias
    _launch("bn_relu_bwd", "peclr_bn_relu_bwd_f32",
            _ptr(d_a_out), _ptr(a_pre), save[0].data_ptr(), save[1].data_ptr(), _ptr(gamma), _ptr(beta), m, h,
            int(training), d_a_pre.data_ptr(), dparams[0].data_ptr(), dparams[1].data_ptr(), dparams[2].data_ptr(),
            _stream())
    return d_a_pre, dparams[0], dparams[1], dparams[2]


# ------------------------------------------------------------------ align
def align_fwd(p_slabs, n_pairs, flags, jitter, extents, angles, want_stats=True):
    """jitter = (jx1, jx2, jy1, jy2) int64 tensors or None; angles = (a1, a2) float64 or None."""
    s, m, d = p_slabs.shape
    dev = p_slabs.device
    p = torch.empty((m, d), device=dev, dtype=torch.float32)
    z = torch.empty((m, d), device=dev, dtype=torch.float32)
    norms = torch.empty((2, m), device=dev, dtype=torch.float32)
    row_stats = torch.empty((m, 8), device=dev, dtype=torch.float32) if want_stats else None
    j = [_ptr(t, torch.int64, "jitter") for t in jitter] if jitter is not None else [None] * 4
    a = [_ptr(t, torch.float64, "angle") for t in angles] if angles is not None else [None] * 2
    _launch("align_fwd", "peclr_align_fwd_f32",
            _ptr(p_slabs), s, m, d, n_pairs, flags, j[0], j[1], j[2], j[3], float(extents[0]), float(extents[1]),
            a[0], a[1], p.data_ptr(), z.data_ptr(), norms.data_ptr(), _ptr(row_stats), _stream())
    return p, z, norms, row_stats


def align_bwd(dz, p, z, norms, n_pairs, flags, angles):
    m, d = p.shape
    dp = torch.empty_like(p)
    a = [_ptr(t, torch.float64, "angle") for t in angles] if angles is not None else [None] * 2
    _launch("align_bwd", "peclr_align_bwd_f32",
            _ptr(dz, what="dz"), _ptr(p), _ptr(z), _ptr(norms), m, d, n_pairs, flags, a[0], a[1], dp.data_ptr(), _stream())
    return dp


# ------------------------------------------------------------------ NT-Xent
def ntxent_jsplit(mr: int, mg: int, backward: bool) -> int:
    js = lib().peclr_ntxent_jsplit(mr, mg, int(backward))
    if js < 1:
        raise PeclrHipError(f"peclr_ntxent_jsplit: unsupported shape Mr={mr} Mg={mg}")
    return js


def ntxent_fwd(z_rows, row_offset, z_all, n_half, inv_tau, loss_scale, row_stats=None, n_pairs_stats=0,
               want_sim=False):
    """Main kernel + finalize kernel.  Returns (out17, row_lse, sim)."""
    mr, d = z_rows.shape
    mg = z_all.shape[0]
    dev = z_rows.device
    js = ntxent_jsplit(mr, mg, False)
    partial = torch.empty((js, mr), device=dev, dtype=torch.float32)
    pos = torch.empty(mr, device=dev, dtype=torch.float32)
    row_lse = torch.empty(mr, device=dev, dtype=torch.float32)
    out17 = torch.zeros(17, device=dev, dtype=torch.float32)
    sim = torch.empty((mr, mg), device=dev, dtype=torch.float32) if want_sim else None
    _launch("ntxent_fwd", "peclr_ntxent_fwd_f32",
            _ptr(z_rows, what="z_rows"), mr, row_offset, _ptr(z_all, what="z_all"), mg, d, n_half, inv_tau, _ptr(sim),
            partial.data_ptr(), pos.data_ptr(), js, _stream())
    _launch("ntxent_finalize", "peclr_ntxent_finalize_f32",
            partial.data_ptr(), js, pos.data_ptr(), mr, loss_scale, row_lse.data_ptr(), _ptr(row_stats), n_pairs_stats,
            out17.data_ptr(), _stream())
    return out17, row_lse, sim


def ntxent_bwd(z_rows, row_offset, z_all, n_half, inv_tau, lse_all, dloss, grad_scale):
    mr, d = z_rows.shape
    mg = z_all.shape[0]
    js = ntxent_jsplit(mr, mg, True)
    slabs = torch.empty((js, mr, d), device=z_rows.device, dtype=torch.float32)
    _launch("ntxent_bwd", "peclr_ntxent_bwd_f32",
            _ptr(z_rows, what="z_rows"), mr, row_offset, _ptr(z_all, what="z_all"), mg, d, n_half, inv_tau,
            _ptr(lse_all, what="lse_all"), _ptr(dloss, what="dloss"), grad_scale, slabs.data_ptr(), js, _stream())
    return _sum_slabs(slabs)


# ------------------------------------------------------------------ optimiser
def lars_adam_step(ptrs, sizes, n_tensors, chunk_tensor, chunk_offset, tensor_chunk_begin, tensor_group, n_chunks,
                   norms_ws, group_lr, group_wd, beta1, beta2, adam_eps, bias_corr1, bias_corr2, use_lars,
                   lars_eta, lars_eps, lars_clip, device_hyper=None, amp=None):
    """group_lr / group_wd: Python float lists, one entry per parameter group (host arrays).
    device_hyper: optional device float[18] that overrides lr / wd / bias corrections (graph replay).
    amp: optional (state int32[4] device tensor = peclr_amp_state, growth_factor, backoff_factor, growth_interval):
    the gradients hold scale*g; inf/nan check + unscale + skip + scale update on the device (three launches)."""
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1
    p = _ptr(ptrs, torch.int64, "ptrs")
    sz = _ptr(sizes, torch.int64, "sizes")
    ct = _ptr(chunk_tensor, torch.int32, "chunk_tensor")
    co = _ptr(chunk_offset, torch.int64, "chunk_offset")
    ng = len(group_lr)
    lr_arr = (c_float * ng)(*group_lr)
    wd_arr = (c_float * ng)(*group_wd)
    if amp is not None:
        state, growth, backoff, interval = amp
        st = _ptr(state, torch.int32, "amp state")
        if state.numel() != 4:
            raise PeclrHipError("amp state: expected 4 x 32-bit words (peclr_amp_state)")
        _launch("lars_sumsq", "peclr_lars_sumsq_amp_f32", p, sz, n_tensors, ct, co, n_chunks, _ptr(norms_ws), st, _stream())
        _launch("lars_adam_update", "peclr_lars_adam_update_amp_f32",
                p, sz, n_tensors, ct, co, _ptr(tensor_chunk_begin, torch.int32, "tensor_chunk_begin"),
                _ptr(tensor_group, torch.int32, "tensor_group"), n_chunks, _ptr(norms_ws), _ptr(device_hyper),
                ctypes.cast(lr_arr, c_void_p), ctypes.cast(wd_arr, c_void_p), ng, beta1, beta2, adam_eps,
                int(use_lars), lars_eta, lars_eps, int(lars_clip), st, _stream())
        _launch("amp_update", "peclr_amp_update", st, growth, backoff, int(interval), _stream(), nbytes=16)
        return
    if use_lars:
        _launch("lars_sumsq", "peclr_lars_sumsq_f32", p, sz, n_tensors, ct, co, n_chunks, _ptr(norms_ws), _stream())
    _launch("lars_adam_update", "peclr_lars_adam_update_f32",
            p, sz, n_tensors, ct, co, _ptr(tensor_chunk_begin, torch.int32, "tensor_chunk_begin"),
            _ptr(tensor_group, torch.int32, "tensor_group"), n_chunks, _ptr(norms_ws), _ptr(device_hyper),
            ctypes.cast(lr_arr, c_void_p), ctypes.cast(wd_arr, c_void_p), ng, beta1, beta2, adam_eps, bias_corr1,
            bias_corr2, int(use_lars), lars_eta, lars_eps, int(lars_clip), _stream())


def gemm_add(layout: int, a: torch.Tensor, b: torch.Tensor, addend: torch.Tensor, tag: str = "gemm_add") -> torch.Tensor:
    """C = op(A) op(B) + addend, all fp32 row-major contiguous 2-D HIP tensors."""
    if layout == GEMM_NT:
        (m, k), (n, k2) = a.shape, b.shape
    elif layout == GEMM_NN:
        (m, k), (k2, n) = a.shape, b.shape
    else:
        (k, m), (k2, n) = a.shape, b.shape
    if k != k2 or tuple(addend.shape) != (m, n):
        raise PeclrHipError(f"gemm_add: shapes {tuple(a.shape)} x {tuple(b.shape)} + {tuple(addend.shape)} (layout {layout})")
    out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    _launch(tag, "peclr_gemm_add_f32", layout, m, n, k, _ptr(a), a.shape[1], _ptr(b), b.shape[1], out.data_ptr(), n,
            _ptr(addend), n, _stream(),
            nbytes=4 * (m * k + k * n + 2 * m * n), flops=2 * m * n * k, kernel="gemm_f32 (v_mfma_f32)")
    return out


def gemm_x6(a: torch.Tensor, b_t: torch.Tensor, addend: Optional[torch.Tensor] = None, tag: str = "gemm_x6",
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C (fp32) = A[M,K] . B_t[N,K]^T (+ addend), fp32 row-major contiguous 2-D HIP tensors, computed on the bf16
    matrix cores at fp32 accuracy (exact three-way bf16 split of both operands, six products: peclr_gemm_x6_f32)."""
    (m, k), (n, k2) = a.shape, b_t.shape
    if k != k2 or (addend is not None and tuple(addend.shape) != (m, n)):
        raise PeclrHipError(f"gemm_x6: shapes {tuple(a.shape)} x {tuple(b_t.shape)}^T")
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    _launch(tag, "peclr_gemm_x6_f32", m, n, k, _ptr(a), k, _ptr(b_t), k, _ptr(out), n, _ptr(addend), n, _stream(),
            nbytes=4 * (m * k + k * n + (2 if addend is not None else 1) * m * n), flops=2 * m * n * k, kernel="gemm_x6_nt128_kernel")
    return out


_X6P_TILE_ROWS = int(os.environ.get("PECLR_X6P_TILE_ROWS", "0"))   # experiments: force 128- or 256-row tiles for the 1x1 GEMMs


class _BnBwdFuse(ctypes.Structure):
    """peclr_bn_bwd_fuse (include/peclr_hip.h)."""
    _fields_ = [("x", c_void_p), ("mean", c_void_p), ("invstd", c_void_p), ("scale_shift", c_void_p), ("relu_mask", c_void_p),
                ("relu", c_int), ("partial", c_void_p)]


def _byref(struct):
    return ctypes.byref(struct) if struct is not None else None


def _epilogue(who: str, m: int, n: int, tile_rows: int, stat_shift, bn_bwd, device, groups: int = 1, dtype=torch.float32,
              row_blocks: int = 0, pick_rows=None):
    """The fused epilogue of a packed-operand GEMM / convolution `who` whose [m, n] output is computed in blocks of `tile_rows` rows
    -> (tile_rows, partial, n_split, fuse).  tile_rows: as given, or -- 0 and an epilogue asked for -- what `pick_rows()` says the
    library will choose.  n_split: `row_blocks` where the kernel reports its own count, else the row blocks of each of `groups`
    equal row sets.
    stat_shift (fp32 [n]): the output's BatchNorm statistics -- partial [2 n_split + 1, n] in peclr_bn2d_stats' layout (the shift in
    the last row), fuse None;
    else bn_bwd = (x, save [2, n], ss [2, n], mask or None, relu) of the BatchNorm layer whose incoming gradient the output is (x:
    that layer's input, m * n elements of `dtype`) -- partial [2 n_split, n] in peclr_bn2d_bwd_reduce's layout, fuse the
    peclr_bn_bwd_fuse to pass by reference (`_byref`);
    neither: (tile_rows, None, 0, None)."""
    if stat_shift is None and bn_bwd is None:
        return tile_rows, None, 0, None
    if pick_rows is not None:
        tile_rows = tile_rows or pick_rows()
    ns = row_blocks or groups * ((m // groups + tile_rows - 1) // tile_rows)
    if stat_shift is not None:
        if stat_shift.numel() != n:
            raise PeclrHipError(f"{who}: stat_shift has {stat_shift.numel()} entries for {n} columns")
        return tile_rows, torch.empty((2 * ns + 1, n), device=device, dtype=torch.float32), ns, None
    x, save, ss, mask, relu = bn_bwd
    if x.dtype != dtype or x.numel() != m * n or not x.is_cuda:
        raise PeclrHipError(f"bn backward fusion: layer input of {x.numel()} {x.dtype} elements for a {dtype} [{m}, {n}] gradient")
    partial = torch.empty((2 * ns, n), device=device, dtype=torch.float32)
    return tile_rows, partial, ns, _BnBwdFuse(x.data_ptr(), save[0].data_ptr(), save[1].data_ptr(), _ptr(ss),
                                              _ptr(mask, torch.int32, "relu mask"), int(relu), partial.data_ptr())


def _with_partial(out, partial, ns):
    """What a wrapper with a fused epilogue returns: the output alone, or (output, partial, n_split) when `_epilogue` made one."""
    return out if partial is None else (out, partial, ns)


def _check_addend_modes(who: str, m: int, n: int, addend, stat_shift, addend_s2, addend_mask):
    """The compact (addend_s2) and the masked (addend_mask) addend of the packed-operand GEMM `who` with an [m, n] output."""
    if addend_s2 is not None and (addend is None or stat_shift is not None or addend_mask is not None):
        raise PeclrHipError(f"{who}: addend_s2 needs the compact addend (and has no statistics output / mask)")
    if addend_mask is not None and (addend is None or stat_shift is not None or n % 32 or addend_mask.dtype != torch.int32
                                    or addend_mask.numel() != m * (n // 32) or not addend_mask.is_contiguous()):
        raise PeclrHipError(f"{who}: addend_mask is the int32 [M, n / 32] bit mask of a dense addend (no statistics output)")


class _WeightPlanes:
    """What X6Planes and HPlanes share: one plane buffer per matrix, and the int64 device table [count, 8] the pack kernels walk
    (weight pointer, plane pointer, n, k, row stride, transposed, first chunk, format).  `who` names the class in messages,
    `what` the weights in `_ptr`'s; `pack_bytes`: the entry point that sizes one matrix's planes; `k_step`: the k extent of a chunk."""

    def __init__(self, who: str, what: str, specs, pack_bytes: str, k_step: int, fmt: int):
        dev = specs[0][0].device
        rows, self.planes, self.shapes, chunk = [], [], [], 0
        for w, transposed in specs:
            _ptr(w, what=what)
            if w.dim() != 2:
                raise PeclrHipError(f"{who}: 2-D weight matrices expected")
            t = int(transposed)                     # 0 plain, 1 transposed, T > 1: T-tap filter [Cout * T, Cin] for its input gradient
            n, k = (w.shape[1], w.shape[0]) if t else (w.shape[0], w.shape[1])
            nbytes = getattr(lib(), pack_bytes)(n, k)
            if nbytes <= 0:
                raise PeclrHipError(f"{who}: B_t[{n}, {k}] needs n % 64 == 0 and k % {k_step} == 0")
            planes = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            rows.append([w.data_ptr(), planes.data_ptr(), n, k, w.stride(0), t, chunk, fmt])
            chunk += ((n + 127) // 128) * (k // k_step)
            self.planes.append(planes)
            self.shapes.append((n, k))
        self._sources = [w for w, _ in specs]          # keep the storage alive
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.count, self.chunks = len(rows), chunk
        self.nbytes = sum(p.numel() for p in self.planes) + 4 * sum(w.numel() for w in self._sources)


class X6Planes(_WeightPlanes):
    """Weight matrices split once into fragment-ordered bf16 planes (peclr_x6_pack_f32) for peclr_gemm_x6p_f32.
    `specs`: list of (fp32 2-D HIP tensor W, transposed) -- B_t = W ([N, K]) or W^T (W is [K, N]).  The device table is
    built once (the tensors' storage must stay where it is: parameters do); `pack()` is ONE launch that re-splits every
    matrix from its current values -- call it after the weights changed (once per optimiser step)."""

    def __init__(self, specs, pair: bool = False):
        """pair: the fp16-pair format of peclr_x6_pack_pair_f32 (two planes, one power of two per matrix: `scale(i)`) instead of
        the three bf16 planes."""
        if not specs:
            raise PeclrHipError("X6Planes: nothing to pack")
        self.pair = bool(pair)
        super().__init__("X6Planes", "x6 weight", specs, "peclr_x6_pack_pair_bytes" if self.pair else "peclr_x6_pack_bytes", 16, 0)
        if self.pair:
            dev = self.table.device
            self.wbytes = 4 * sum(w.numel() for w in self._sources)       # (the maxima's pass reads the weights once more)
            self.absmax = torch.zeros(self.count, device=dev, dtype=torch.float32)
            self.scales = torch.ones(self.count, device=dev, dtype=torch.float32)

    def scale(self, i: int) -> torch.Tensor:
        """The device float holding the power of two matrix i was multiplied by (pair format)."""
        return self.scales[i:i + 1]

    def pack(self):
        if self.pair:
            _launch("x6_absmax", "peclr_x6_absmax_f32", self.table.data_ptr(), self.count, self.chunks, self.absmax.data_ptr(), _stream(),
                    nbytes=self.wbytes, kernel="x6_pair_kernel")
            _launch("x6_pack", "peclr_x6_pack_pair_f32", self.table.data_ptr(), self.count, self.chunks, self.absmax.data_ptr(),
                    self.scales.data_ptr(), _stream(), nbytes=self.nbytes, kernel="x6_pair_kernel")
            return self
        _launch("x6_pack", "peclr_x6_pack_f32", self.table.data_ptr(), self.count, self.chunks, _stream(),
                nbytes=self.nbytes, kernel="x6_pack_kernel")
        return self


class _X6Pair(ctypes.Structure):
    _fields_ = [("a_absmax", ctypes.c_void_p), ("w_scale", ctypes.c_void_p)]


def _pair_arg(pair, who: str):
    """pair = None (six-product arithmetic on bf16-triple planes) or (a_absmax, w_scale): one-element fp32 HIP tensors -- the
    maximum of |A| over the whole activation tensor (written by the pass that produced it) and the weight planes' power of two
    (`X6Planes(pair=True).scale(i)`).  Returns (struct or None to pass, bytes per weight element of the planes)."""
    if pair is None:
        return None, 6
    a_absmax, w_scale = pair
    for t, name in ((a_absmax, "a_absmax"), (w_scale, "w_scale")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
            raise PeclrHipError(f"{who}: pair.{name} is a one-element fp32 HIP tensor")
    return _X6Pair(a_absmax.data_ptr(), w_scale.data_ptr()), 4


def gemm_x6p(a: torch.Tensor, planes: torch.Tensor, n: int, addend: Optional[torch.Tensor] = None, tag: str = "gemm_x6p",
             tile_rows: int = 0, stat_shift: Optional[torch.Tensor] = None, bn_bwd=None, addend_s2=None,
             addend_mask: Optional[torch.Tensor] = None, pair=None):
    """C (fp32) [M, n] = A[M, K] . B_t^T (+ addend) with B_t given as packed planes (X6Planes): fp32 accuracy on the
    bf16 matrix cores, the weight operand split once per step (peclr_gemm_x6p_f32).
    stat_shift (fp32 [n]): also return the training-mode BatchNorm statistics of C as `(partial, n_split)` in the layout
    of peclr_bn2d_stats (sums of (C - shift) and its square per row block; the shift in the last row) -> (C, partial, n_split).
    bn_bwd (see `_epilogue`): C is the gradient arriving at that BatchNorm layer; also return its backward reduction
    `(partial, n_split)` in peclr_bn2d_bwd_reduce's layout -> (C, partial, n_split).
    addend_s2 = (H, W): the rows are the pixels of H x W images and `addend` [M / 4, n] holds every second pixel only (the
    compact input gradient of a 1x1 / stride-2 convolution): added at the even (h, w) rows (peclr_gemm_x6p_s2add_f32).
    addend_mask (int32 [M, n / 32], the 1-bit ReLU mask of peclr_bn2d_apply): addend elements whose bit is clear count as
    zero (peclr_gemm_x6p_maskadd_f32).
    pair (see `_pair_arg`): fp16-pair arithmetic, `planes` of `X6Planes(pair=True)`."""
    m, k = a.shape
    add_rows = m if addend_s2 is None else m // 4
    pst, wb = _pair_arg(pair, "gemm_x6p")
    if planes.dtype != torch.uint8 or planes.numel() != wb * ((n + 127) // 128 * 128) * k or (addend is not None and tuple(addend.shape) != (add_rows, n)):
        raise PeclrHipError(f"gemm_x6p: A {tuple(a.shape)}, planes of {planes.numel()} bytes for B_t[{n}, {k}]")
    _check_addend_modes("gemm_x6p", m, n, addend, stat_shift, addend_s2, addend_mask)
    out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    tile_rows, partial, ns, fuse = _epilogue("gemm_x6p", m, n, tile_rows or _X6P_TILE_ROWS, stat_shift, bn_bwd, a.device,
                                             pick_rows=lambda: lib().peclr_gemm_x6p_tile_rows(m, n, k))
    add_elems = 0 if addend is None else addend.numel() + (0 if addend_mask is None else addend_mask.numel())
    head = (m, n, k, _ptr(a), k, _ptr(planes, torch.uint8), out.data_ptr(), n, _ptr(addend), n)
    if addend_mask is not None:
        name, args = "peclr_gemm_x6p_maskadd_f32", (_ptr(addend_mask, torch.int32), tile_rows)
    elif addend_s2 is not None:
        name, args = "peclr_gemm_x6p_s2add_f32", (int(addend_s2[0]), int(addend_s2[1]), tile_rows)
    else:
        name, args = "peclr_gemm_x6p_f32", (tile_rows, _ptr(stat_shift), partial.data_ptr() if stat_shift is not None else None)
    _launch(tag, name, *head, *args, _byref(fuse), _byref(pst), _stream(),
            nbytes=4 * (m * k + m * n + add_elems + (m * n if fuse is not None else 0)) + wb * k * n, flops=2 * m * n * k,
            kernel="gemm_x6p_kernel" if pst is None else "gemm_x6p_kernel<pair>")
    return _with_partial(out, partial, ns)


_CONV3X3_VARIANT = int(os.environ.get("PECLR_CONV3X3_HALO", "1"))   # A/B: 1 = one split per 16-channel chunk and workgroup (halo patch in LDS)
_ZEROS = {}


def _zeros(device):
    z = _ZEROS.get(device)
    if z is None:
        z = _ZEROS[device] = torch.zeros(64, device=device, dtype=torch.float32)
    return z


def conv3x3_x6p(x: torch.Tensor, planes: torch.Tensor, cout: int, flip: bool = False, addend: Optional[torch.Tensor] = None,
                tag: str = "conv3x3_x6p", tile_rows: int = 0, stat_shift: Optional[torch.Tensor] = None, bn_bwd=None, variant: Optional[int] = None,
                pair=None):
    """3x3 / stride-1 / padding-1 convolution of an NHWC (channels_last) fp32 tensor x [N, Cin, H, W] as an implicit GEMM on
    the bf16 matrix cores at fp32 accuracy (peclr_conv3x3_x6p_f32); `planes` = X6Planes of W seen as [Cout, 9 * Cin]
    (flip=False) or, for the input gradient (flip=True, x = dY), of [Cout_w * 9, Cin_w] packed with transposed = 9.
    Returns y [N, cout, H, W] channels_last (and (partial, n_split) when stat_shift or bn_bwd is given, as in gemm_x6p)."""
    nb, cin, h, w = x.shape
    xp = _nhwc_ptr(x, "conv3x3 x", torch.float32)
    pst, wb = _pair_arg(pair, "conv3x3_x6p")
    if planes.dtype != torch.uint8 or planes.numel() != wb * ((cout + 127) // 128 * 128) * 9 * cin:
        raise PeclrHipError(f"conv3x3_x6p: planes of {planes.numel()} bytes for [{cout}, 9 * {cin}]")
    y = torch.empty((nb, cout, h, w), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)
    m = nb * h * w
    tile_rows, partial, ns, fuse = _epilogue("conv3x3_x6p", m, cout, tile_rows, stat_shift, bn_bwd, x.device,
                                             pick_rows=lambda: lib().peclr_gemm_x6p_tile_rows(m, cout, 9 * cin))
    ap = _nhwc_ptr(addend, "conv3x3 addend", torch.float32) if addend is not None else None
    _launch(tag, "peclr_conv3x3_x6p_f32", nb, h, w, cin, cout, xp, _ptr(planes, torch.uint8), y.data_ptr(), ap, int(flip), tile_rows,
            _CONV3X3_VARIANT if variant is None else int(variant), _zeros(x.device).data_ptr(), _ptr(stat_shift),
            partial.data_ptr() if stat_shift is not None else None, _byref(fuse), _byref(pst), _stream(),
            nbytes=4 * (m * cin + (2 if addend is not None else 1) * m * cout + (m * cout if fuse is not None else 0)) + 9 * wb * cin * cout,
            flops=18 * m * cin * cout, kernel="gemm_x6p_kernel (3x3)" if pst is None else "gemm_x6p_kernel<pair> (3x3)")
    return _with_partial(y, partial, ns)


def conv3x3_s2_dgrad_x6p(gy: torch.Tensor, planes: torch.Tensor, cin: int, tag: str = "conv3x3_s2_dgrad", tile_rows: int = 0, bn_bwd=None,
                         pair=None):
    """Input gradient of a 3x3 / padding-1 / stride-2 convolution: gy [N, Cout, Ho, Wo] channels_last fp32 -> dx
    [N, cin, 2 Ho, 2 Wo], one implicit GEMM per parity class of input pixels (1, 2, 2 and 4 of the nine taps:
    peclr_conv3x3_s2_dgrad_x6p_f32); `planes` as for the stride-1 input gradient ([Cout * 9, Cin] packed with
    transposed = 9).  bn_bwd: as in gemm_x6p (the BatchNorm layer dx arrives at) -> (dx, partial, n_split)."""
    nb, cout, ho, wo = gy.shape
    gp = _nhwc_ptr(gy, "conv_s2 dgrad gy", torch.float32)
    pst, wb = _pair_arg(pair, "conv3x3_s2_dgrad_x6p")
    if planes.dtype != torch.uint8 or planes.numel() != wb * ((cin + 127) // 128 * 128) * 9 * cout:
        raise PeclrHipError(f"conv3x3_s2_dgrad_x6p: planes of {planes.numel()} bytes for [{cin}, 9 * {cout}]")
    dx = torch.empty((nb, cin, 2 * ho, 2 * wo), device=gy.device, dtype=torch.float32, memory_format=torch.channels_last)
    mc = nb * ho * wo
    tile_rows, partial, ns, fuse = _epilogue("conv3x3_s2_dgrad_x6p", 4 * mc, cin, tile_rows, None, bn_bwd, gy.device, groups=4,
                                             pick_rows=lambda: lib().peclr_gemm_x6p_tile_rows(mc, cin, 4 * cout))
    _launch(tag, "peclr_conv3x3_s2_dgrad_x6p_f32", nb, ho, wo, cout, cin, gp, _ptr(planes, torch.uint8), dx.data_ptr(), tile_rows,
            _zeros(gy.device).data_ptr(), _byref(fuse), _byref(pst), _stream(),
            nbytes=4 * (mc * cout + 4 * mc * cin * (2 if fuse is not None else 1)) + 9 * wb * cin * cout, flops=18 * mc * cin * cout,
            kernel="gemm_x6p_kernel (3x3)" if pst is None else "gemm_x6p_kernel<pair> (3x3)")
    return _with_partial(dx, partial, ns)


def conv_s2_x6p(x: torch.Tensor, planes: torch.Tensor, cout: int, taps: int, tag: str = "conv_s2_x6p", tile_rows: int = 0,
                stat_shift: Optional[torch.Tensor] = None, pair=None):
    """Forward of a stride-2 convolution (taps = 9: 3x3 / padding 1; taps = 1: 1x1) of an NHWC fp32 tensor x [N, Cin, H, W]
    (H, W even) on the six-product kernel (peclr_conv_s2_x6p_f32) -> y [N, cout, H/2, W/2] channels_last (and
    (partial, n_split) of the output's BatchNorm statistics when stat_shift is given)."""
    nb, cin, h, w = x.shape
    xp = _nhwc_ptr(x, "conv_s2 x", torch.float32)
    pst, wb = _pair_arg(pair, "conv_s2_x6p")
    if planes.dtype != torch.uint8 or planes.numel() != wb * ((cout + 127) // 128 * 128) * taps * cin or h % 2 or w % 2:
        raise PeclrHipError(f"conv_s2_x6p: planes of {planes.numel()} bytes for [{cout}, {taps} * {cin}], input {h} x {w}")
    y = torch.empty((nb, cout, h // 2, w // 2), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)
    m = nb * (h // 2) * (w // 2)
    tile_rows, partial, ns, _ = _epilogue("conv_s2_x6p", m, cout, tile_rows, stat_shift, None, x.device,
                                          pick_rows=lambda: lib().peclr_gemm_x6p_tile_rows(m, cout, taps * cin))
    _launch(tag, "peclr_conv_s2_x6p_f32", nb, h, w, cin, cout, taps, xp, _ptr(planes, torch.uint8), y.data_ptr(), tile_rows,
            _zeros(x.device).data_ptr(), _ptr(stat_shift), _ptr(partial), _byref(pst), _stream(),
            nbytes=4 * (nb * h * w * cin + m * cout) + wb * taps * cin * cout, flops=2 * m * taps * cin * cout,
            kernel="gemm_x6p_kernel (stride 2)" if pst is None else "gemm_x6p_kernel<pair> (stride 2)")
    return _with_partial(y, partial, ns)


def gemm_x6_tn(a: torch.Tensor, b: torch.Tensor, tag: str = "gemm_x6_tn") -> torch.Tensor:
    """C[M,N] (fp32) = A[K,M]^T . B[K,N], fp32 row-major contiguous 2-D HIP tensors whose ROWS are the contraction
    index (the 1x1 weight gradient dW = dY^T X on NHWC storage), on the bf16 matrix cores at fp32 accuracy; split-K
    slabs summed in a fixed order (peclr_gemm_x6_tn_f32 + peclr_slab_reduce_f32): deterministic."""
    (k, m), (k2, n) = a.shape, b.shape
    if k != k2:
        raise PeclrHipError(f"gemm_x6_tn: shapes {tuple(a.shape)}^T x {tuple(b.shape)}")
    ns = lib().peclr_gemm_x6_tn_slabs(m, n, k)
    if ns < 1:
        raise PeclrHipError(f"gemm_x6_tn: unsupported shape M={m} N={n} K={k}")
    slabs = torch.empty((ns, m, n), device=a.device, dtype=torch.float32)
    _launch(tag, "peclr_gemm_x6_tn_f32", m, n, k, _ptr(a), m, _ptr(b), n, slabs.data_ptr(), ns, _stream(),
            nbytes=4 * (k * m + k * n + ns * m * n), flops=2 * m * n * k, kernel="gemm_x6_tn128_kernel")
    return _sum_slabs(slabs, "wgrad_slab_reduce")


def gemm_x6t(a: torch.Tensor, b: torch.Tensor, taps: int = 1, hw=None, stride: int = 1, tag: str = "gemm_x6t") -> torch.Tensor:
    """C[M, taps * N] (fp32) = sum over rows of A[K, M]^T . B[K (shifted by the tap), N] -- the weight gradient of a 1x1
    (taps = 1) or 3x3 / padding-1 (taps = 9, hw = (H, W) of the images A's rows are the pixels of) convolution on NHWC
    storage, on the bf16 matrix cores at fp32 accuracy (peclr_gemm_x6t_f32 + peclr_slab_reduce_f32: fixed-order split-K,
    deterministic).  stride = 2: A = dY over the H x W output pixels, B = X over the 2H x 2W input pixels (4 K rows).
    (Weight gradients stay on six products: in pair arithmetic they were 21 - 29 % faster and, on real layer tensors, 3 - 46 % less
    accurate than this kernel -- tools/exp/pair_wgrad.patch)"""
    (k, m), (k2, n) = a.shape, b.shape
    if k * stride * stride != k2 or taps not in (1, 9) or stride not in (1, 2) or ((taps == 9 or stride == 2) and hw is None):
        raise PeclrHipError(f"gemm_x6t: shapes {tuple(a.shape)}^T x {tuple(b.shape)}, taps {taps}, stride {stride}")
    h, w = hw if hw is not None else (1, 1)
    ns = lib().peclr_gemm_x6t_slabs(m, n, k, taps)
    if ns < 1:
        raise PeclrHipError(f"gemm_x6t: unsupported shape M={m} N={n} K={k}")
    slabs = torch.empty((ns, m, taps * n), device=a.device, dtype=torch.float32)
    _launch(tag, "peclr_gemm_x6t_f32", m, n, k, _ptr(a), a.stride(0), _ptr(b), b.stride(0), slabs.data_ptr(), ns, taps, h, w, stride,
            _zeros(a.device).data_ptr(), _stream(),
            nbytes=4 * (k * m + k2 * n // (stride * stride) * (1 if taps == 1 else stride * stride) + ns * m * n * taps),
            flops=2 * m * n * k * taps, kernel="gemm_x6w2_kernel | gemm_x6w_kernel" if taps == 9 else "gemm_x6t2_kernel | gemm_x6t_kernel")
    return _sum_slabs(slabs, "wgrad_slab_reduce")


def gemm_add_half(a: torch.Tensor, b_t: torch.Tensor, addend: Optional[torch.Tensor], tag: str = "gemm_add") -> torch.Tensor:
    """C (16-bit) = A[M,K] . B_t[N,K]^T + addend, row-major contiguous 2-D HIP tensors that are ALL bf16 or ALL
    fp16, fp32 accumulate (peclr_gemm_add_bf16 / peclr_gemm_add_f16)."""
    (m, k), (n, k2) = a.shape, b_t.shape
    half = a.dtype
    if half not in (torch.bfloat16, torch.float16):
        raise PeclrHipError(f"gemm_add_half: bf16 or fp16 tensors expected, got {half}")
    for t in (a, b_t) + ((addend,) if addend is not None else ()):
        if not t.is_cuda or t.dtype != half or not t.is_contiguous():
            raise PeclrHipError(f"gemm_add_half: contiguous {half} HIP tensors expected (peclr_amd has no CPU path)")
    if k != k2 or (addend is not None and tuple(addend.shape) != (m, n)):
        raise PeclrHipError(f"gemm_add_half: shapes {tuple(a.shape)} x {tuple(b_t.shape)}^T")
    out = torch.empty((m, n), device=a.device, dtype=half)
    _launch(tag, "peclr_gemm_add_bf16" if half == torch.bfloat16 else "peclr_gemm_add_f16",
            m, n, k, a.data_ptr(), k, b_t.data_ptr(), k, out.data_ptr(), n, addend.data_ptr() if addend is not None else None, n, _stream(),
            nbytes=2 * (m * k + k * n + 2 * m * n), flops=2 * m * n * k)
    return out


# ------------------------------------------------------------------ 16-bit convolutions (csrc/conv_h.hip)
_HALF_IO = {torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16}
_HZEROS = {}


def _hzeros(device, dtype):
    z = _HZEROS.get((device, dtype))
    if z is None:
        z = _HZEROS[(device, dtype)] = torch.zeros(64, device=device, dtype=dtype)
    return z


def _half_io(t: torch.Tensor, what: str) -> int:
    if t.dtype not in _HALF_IO or not t.is_cuda:
        raise PeclrHipError(f"{what}: a bf16 / fp16 HIP tensor expected, got {t.dtype} on {t.device} (peclr_amd has no CPU path)")
    return _HALF_IO[t.dtype]


class HPlanes(_WeightPlanes):
    """Weight matrices packed once per optimiser step from the fp32 MASTER weights into 16-bit MFMA-fragment order
    (peclr_h_pack) for peclr_gemm_h / peclr_conv_h -- the cast autocast performs per forward rides in that launch.
    `specs`: list of (fp32 2-D HIP tensor W, transposed) exactly as X6Planes; dtype: torch.bfloat16 or torch.float16."""

    def __init__(self, specs, dtype):
        if not specs:
            raise PeclrHipError("HPlanes: nothing to pack")
        if dtype not in _HALF_IO:
            raise PeclrHipError(f"HPlanes: bf16 or fp16, got {dtype}")
        self.dtype = dtype
        super().__init__("HPlanes", "16-bit pack: fp32 master weight", specs, "peclr_h_pack_bytes", 32, _HALF_IO[dtype])

    def pack(self):
        _launch("h_pack", "peclr_h_pack", self.table.data_ptr(), self.count, self.chunks, _stream(), nbytes=self.nbytes, kernel="h_pack_kernel")
        return self


def _h_planes_ok(planes, n, k, what):
    if planes.dtype != torch.uint8 or planes.numel() != 2 * ((n + 127) // 128 * 128) * k:
        raise PeclrHipError(f"{what}: planes of {planes.numel()} bytes for B_t[{n}, {k}]")


def gemm_h(a: torch.Tensor, planes: torch.Tensor, n: int, addend: Optional[torch.Tensor] = None, tag: str = "gemm_h",
           tile_rows: int = 0, stat_shift: Optional[torch.Tensor] = None, bn_bwd=None, addend_s2=None,
           addend_mask: Optional[torch.Tensor] = None):
    """C (16-bit) [M, n] = A[M, K] . B_t^T (+ addend), A / C / addend bf16 or fp16, B_t packed by HPlanes, fp32 accumulation
    (peclr_gemm_h).  Arguments and returns as `gemm_x6p` (statistics / backward-reduction partials are fp32, in the same
    layouts; they are sums over the ROUNDED 16-bit outputs)."""
    m, k = a.shape
    io = _half_io(a, "gemm_h A")
    _h_planes_ok(planes, n, k, "gemm_h")
    add_rows = m if addend_s2 is None else m // 4
    if not a.is_contiguous() or (addend is not None and (tuple(addend.shape) != (add_rows, n) or addend.dtype != a.dtype or not addend.is_contiguous())):
        raise PeclrHipError(f"gemm_h: contiguous {a.dtype} A {tuple(a.shape)} / addend expected")
    _check_addend_modes("gemm_h", m, n, addend, stat_shift, addend_s2, addend_mask)
    out = torch.empty((m, n), device=a.device, dtype=a.dtype)
    tile_rows, partial, ns, fuse = _epilogue("gemm_h", m, n, tile_rows, stat_shift, bn_bwd, a.device, dtype=a.dtype,
                                             pick_rows=lambda: lib().peclr_conv_h_tile_rows(m, n))
    add_elems = 0 if addend is None else addend.numel()
    mask_bytes = 0 if addend_mask is None else 4 * addend_mask.numel()
    _launch(tag, "peclr_gemm_h", io, m, n, k, a.data_ptr(), k, _ptr(planes, torch.uint8), out.data_ptr(), n,
            addend.data_ptr() if addend is not None else None, n,
            int(addend_s2[0]) if addend_s2 is not None else 0, int(addend_s2[1]) if addend_s2 is not None else 0,
            _ptr(addend_mask, torch.int32), tile_rows, _ptr(stat_shift),
            partial.data_ptr() if stat_shift is not None else None, _byref(fuse), _stream(),
            nbytes=2 * (m * k + m * n + add_elems + (m * n if fuse is not None else 0) + k * n) + mask_bytes, flops=2 * m * n * k,
            kernel="conv_h_kernel")
    return _with_partial(out, partial, ns)


def conv_h(x: torch.Tensor, planes: torch.Tensor, cout: int, taps: int = 9, stride: int = 1, flip: bool = False,
           tag: str = "conv_h", tile_rows: int = 0, stat_shift: Optional[torch.Tensor] = None, bn_bwd=None):
    """3x3 / padding-1 (taps = 9) or 1x1 (taps = 1, stride 2) convolution of an NHWC bf16 / fp16 tensor x [N, Cin, H, W]
    (peclr_conv_h): forward, or -- flip=True, stride 1 -- the input gradient with x = dY and planes packed with
    transposed = 9.  Returns y [N, cout, H / stride, W / stride] channels_last (+ (partial, n_split) as gemm_h)."""
    nb, cin, h, w = x.shape
    io = _half_io(x, "conv_h x")
    xp = _nhwc_ptr(x, "conv_h x", x.dtype)
    _h_planes_ok(planes, cout, taps * cin, "conv_h")
    if h % stride or w % stride:
        raise PeclrHipError(f"conv_h: {h} x {w} input with stride {stride}")
    ho, wo = h // stride, w // stride
    y = torch.empty((nb, cout, ho, wo), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    m = nb * ho * wo
    ns = 0
    if stat_shift is not None or bn_bwd is not None:
        ns = lib().peclr_conv_h_row_blocks(nb, h, w, cout, taps, stride, tile_rows)     # (tile_rows 0: the library's choice)
        if ns <= 0:
            raise PeclrHipError(f"conv_h: no launch for tile_rows = {tile_rows} at {h} x {w}, taps {taps}, stride {stride}")
    tile_rows, partial, ns, fuse = _epilogue("conv_h", m, cout, tile_rows, stat_shift, bn_bwd, x.device, dtype=x.dtype, row_blocks=ns)
    _launch(tag, "peclr_conv_h", io, nb, h, w, cin, cout, taps, stride, xp, _ptr(planes, torch.uint8), y.data_ptr(), int(flip), tile_rows,
            _hzeros(x.device, x.dtype).data_ptr(), _ptr(stat_shift),
            partial.data_ptr() if stat_shift is not None else None, _byref(fuse), _stream(),
            nbytes=2 * (nb * h * w * cin + m * cout * (2 if fuse is not None else 1) + taps * cin * cout), flops=2 * m * taps * cin * cout,
            kernel="conv_h_kernel (3x3)" if taps == 9 else "conv_h_kernel (stride 2)")
    return _with_partial(y, partial, ns)


def _fold_table(scale_shift, n: int, device, who: str):
    """The fp32 [2, n] scale / shift table of the BatchNorm2d folded into `who`'s epilogue (None -> the library's null code)."""
    if scale_shift is None:
        return None
    if scale_shift.dtype != torch.float32 or scale_shift.numel() != 2 * n or not scale_shift.is_contiguous() or scale_shift.device != device:
        raise PeclrHipError(f"{who}: scale_shift is the contiguous fp32 [2, {n}] table of the folded BatchNorm2d on {device}")
    return scale_shift.data_ptr()


def gemm_h_bnact(a: torch.Tensor, planes: torch.Tensor, n: int, scale_shift: Optional[torch.Tensor], relu: bool = True,
                 addend: Optional[torch.Tensor] = None, tag: str = "conv1x1_bnact", tile_rows: int = 0) -> torch.Tensor:
    """`gemm_h` with the eval-mode BatchNorm2d (+ dense addend) (+ ReLU) behind it in the epilogue (peclr_gemm_h_bnact):
    C = round(relu(fmaf(A . B_t^T, scale, shift) + addend)), one rounding; scale_shift: that layer's fp32 [2, n] table."""
    m, k = a.shape
    io = _half_io(a, "gemm_h_bnact A")
    _h_planes_ok(planes, n, k, "gemm_h_bnact")
    if not a.is_contiguous() or (addend is not None and (tuple(addend.shape) != (m, n) or addend.dtype != a.dtype or not addend.is_contiguous())):
        raise PeclrHipError(f"gemm_h_bnact: contiguous {a.dtype} A {tuple(a.shape)} / addend [{m}, {n}] expected")
    out = torch.empty((m, n), device=a.device, dtype=a.dtype)
    _launch(tag, "peclr_gemm_h_bnact", io, m, n, k, a.data_ptr(), k, _ptr(planes, torch.uint8), out.data_ptr(), n,
            addend.data_ptr() if addend is not None else None, n, _fold_table(scale_shift, n, a.device, "gemm_h_bnact"), int(relu),
            tile_rows, _stream(), nbytes=2 * (m * k + m * n + (m * n if addend is not None else 0) + k * n) + 8 * n,
            flops=2 * m * n * k, kernel="conv_h_kernel")
    return out


def conv_h_bnact(x: torch.Tensor, planes: torch.Tensor, cout: int, scale_shift: Optional[torch.Tensor], relu: bool = True, taps: int = 9,
                 stride: int = 1, tag: Optional[str] = None, tile_rows: int = 0) -> torch.Tensor:
    """`conv_h` (forward) with the eval-mode BatchNorm2d (+ ReLU) behind it in the epilogue (peclr_conv_h_bnact)."""
    nb, cin, h, w = x.shape
    io = _half_io(x, "conv_h_bnact x")
    xp = _nhwc_ptr(x, "conv_h_bnact x", x.dtype)
    _h_planes_ok(planes, cout, taps * cin, "conv_h_bnact")
    if h % stride or w % stride:
        raise PeclrHipError(f"conv_h_bnact: {h} x {w} input with stride {stride}")
    ho, wo = h // stride, w // stride
    y = torch.empty((nb, cout, ho, wo), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    m = nb * ho * wo
    _launch(tag or ("conv3x3_bnact" if stride == 1 else "conv_s2_bnact"), "peclr_conv_h_bnact", io, nb, h, w, cin, cout, taps, stride, xp,
            _ptr(planes, torch.uint8), y.data_ptr(), tile_rows, _hzeros(x.device, x.dtype).data_ptr(),
            _fold_table(scale_shift, cout, x.device, "conv_h_bnact"), int(relu), _stream(),
            nbytes=2 * (nb * h * w * cin + m * cout + taps * cin * cout) + 8 * cout, flops=2 * m * taps * cin * cout,
            kernel="conv_h_kernel (3x3)" if taps == 9 else "conv_h_kernel (stride 2)")
    return y


WGRAD3_MAX_W, WGRAD3W_MAX_W = 62, 512      # widest row of peclr_wgrad3_h (one ring) and of peclr_wgrad3w_h (column segments)


def wgrad_h_ok(gy: torch.Tensor, x: torch.Tensor, taps: int, stride: int) -> bool:
    """Does peclr_wgrad_h take this weight gradient?  (1x1 convolutions, stride 1 or 2, channel counts multiples of 32.)"""
    cout, cin = gy.shape[1], x.shape[1]
    if taps == 9:       # 3x3 / padding 1 / stride 1 (peclr_wgrad3_h, rows wider than 62 pixels: peclr_wgrad3w_h); the stride-2 ones
        #                 stay on MIOpen (faster there)
        return (stride == 1 and cout % 64 == 0 and cin % 64 == 0 and gy.dtype in _HALF_IO and x.dtype == gy.dtype
                and x.shape[2] == stride * gy.shape[2] and x.shape[3] == stride * gy.shape[3] and gy.shape[3] <= WGRAD3W_MAX_W
                and gy.shape[0] * gy.shape[2] * gy.shape[3] >= 512)
    return (taps == 1 and stride in (1, 2) and cout % 32 == 0 and cin % 32 == 0 and gy.dtype in _HALF_IO and x.dtype == gy.dtype
            and gy.shape[0] * gy.shape[2] * gy.shape[3] >= 32
            and (stride == 1 or (x.shape[2] == 2 * gy.shape[2] and x.shape[3] == 2 * gy.shape[3])))


def wgrad_h(gy: torch.Tensor, x: torch.Tensor, taps: int = 1, stride: int = 1, tag: str = "conv1x1_wgrad") -> torch.Tensor:
    """dW [Cout, taps * Cin] (fp32) of a 1x1 (taps = 1) or 3x3 / padding-1 (taps = 9) convolution, stride 1 or 2, from 16-bit NHWC
    activations gy [N, Cout, Ho, Wo], x [N, Cin, H, W] (peclr_wgrad_h / peclr_wgrad3_h / peclr_wgrad3w_h +
    peclr_slab_reduce_f32: fixed-order split-K, deterministic)."""
    if not wgrad_h_ok(gy, x, taps, stride):
        raise PeclrHipError(f"wgrad_h: unsupported problem gy {tuple(gy.shape)} x {tuple(x.shape)} taps {taps} stride {stride}")
    io = _half_io(gy, "wgrad_h gy")
    nb, cout, ho, wo = gy.shape
    cin = x.shape[1]
    gp, xp = _nhwc_ptr(gy, "wgrad_h gy", gy.dtype), _nhwc_ptr(x, "wgrad_h x", gy.dtype)
    k = nb * ho * wo
    if taps == 9:
        if wo <= WGRAD3_MAX_W:
            entry, kernel, ns = "peclr_wgrad3_h", "wgrad3_h_kernel", lib().peclr_wgrad3_h_slabs(cout, cin, nb, ho, wo)
        else:
            entry, kernel, ns = "peclr_wgrad3w_h", "wgrad3_h_kernel (segments)", lib().peclr_wgrad3w_h_slabs(cout, cin, nb, ho, wo)
        if ns < 1:
            raise PeclrHipError(f"wgrad_h: unsupported 3x3 shape M={cout} N={cin} {nb} x {ho} x {wo}")
        slabs = torch.empty((ns, cout, 9 * cin), device=gy.device, dtype=torch.float32)
        _launch("conv3x3_wgrad" if tag == "conv1x1_wgrad" else tag, entry,
                io, cout, cin, nb, ho, wo, gp, xp, slabs.data_ptr(), ns, _hzeros(gy.device, gy.dtype).data_ptr(), _stream(),
                nbytes=2 * k * (cout + cin) + 4 * ns * cout * 9 * cin, flops=18 * cout * cin * k, kernel=kernel)
    else:
        ns = lib().peclr_wgrad_h_slabs(cout, cin, k)
        if ns < 1:
            raise PeclrHipError(f"wgrad_h: unsupported shape M={cout} N={cin} K={k}")
        slabs = torch.empty((ns, cout, cin), device=gy.device, dtype=torch.float32)
        _launch(tag, "peclr_wgrad_h", io, cout, cin, k, gp, cout, xp, cin, slabs.data_ptr(), ns, stride, ho, wo,
                _hzeros(gy.device, gy.dtype).data_ptr(), _stream(),
                nbytes=2 * k * (cout + cin) + 4 * ns * cout * cin, flops=2 * cout * cin * k, kernel="wgrad_h_kernel")
    return _sum_slabs(slabs, "wgrad_slab_reduce")


WGRAD3_S2_MAX_WO = 62                      # widest OUTPUT row of peclr_wgrad3s2_h (the lead of its 192-slot rings)


def wgrad3_s2_h_ok(gy: torch.Tensor, x: torch.Tensor) -> bool:
    """Does peclr_wgrad3s2_h take this 3x3 / padding-1 / stride-2 weight gradient?  (16-bit channels_last operands of one format,
    channel counts multiples of 64, even input sizes, output rows of up to 62 pixels -- and at least 512 output pixels, the
    minimum of the stride-1 3x3 route: not a tuning knob, nothing widens it.)"""
    if gy.dim() != 4 or x.dim() != 4:
        return False
    nb, cout, ho, wo = gy.shape
    return (gy.dtype in _HALF_IO and x.dtype == gy.dtype and x.shape[0] == nb and cout % 64 == 0 and x.shape[1] % 64 == 0
            and cout > 0 and x.shape[1] > 0 and ho >= 1 and 1 <= wo <= WGRAD3_S2_MAX_WO and x.shape[2] == 2 * ho and x.shape[3] == 2 * wo
            and nb * ho * wo >= 512 and nb * (ho + 1) * (wo + 1) <= 0x7FFFFFFF // 2
            and gy.is_contiguous(memory_format=torch.channels_last) and x.is_contiguous(memory_format=torch.channels_last))


def wgrad3_s2_h(gy: torch.Tensor, x: torch.Tensor, tag: str = "conv3x3_wgrad") -> torch.Tensor:
    """dW [Cout, 9 * Cin] (fp32) of a 3x3 / padding-1 / stride-2 convolution from 16-bit NHWC activations gy [N, Cout, Ho, Wo],
    x [N, Cin, 2 Ho, 2 Wo] (peclr_wgrad3s2_h: the four parity planes of x through LDS rings, all nine taps in one workgroup +
    peclr_slab_reduce_f32: fixed-order split-K, deterministic)."""
    if not wgrad3_s2_h_ok(gy, x):
        raise PeclrHipError(f"wgrad3_s2_h: unsupported problem gy {gy.dtype} {tuple(gy.shape)} x {x.dtype} {tuple(x.shape)}")
    io = _half_io(gy, "wgrad3_s2_h gy")
    nb, cout, ho, wo = gy.shape
    cin = x.shape[1]
    gp, xp = _nhwc_ptr(gy, "wgrad3_s2_h gy", gy.dtype), _nhwc_ptr(x, "wgrad3_s2_h x", gy.dtype)
    ns = lib().peclr_wgrad3s2_h_slabs(cout, cin, nb, ho, wo)
    if ns < 1:
        raise PeclrHipError(f"wgrad3_s2_h: unsupported shape M={cout} N={cin} {nb} x {ho} x {wo}")
    k = nb * ho * wo
    slabs = torch.empty((ns, cout, 9 * cin), device=gy.device, dtype=torch.float32)
    _launch(tag, "peclr_wgrad3s2_h", io, cout, cin, nb, ho, wo, gp, xp, slabs.data_ptr(), ns, _hzeros(gy.device, gy.dtype).data_ptr(),
            _stream(), nbytes=2 * k * (cout + 4 * cin) + 4 * ns * cout * 9 * cin, flops=18 * cout * cin * k, kernel="wgrad3_h_s2_kernel")
    return _sum_slabs(slabs, "wgrad_slab_reduce")


def conv3x3_s2_dgrad_h(gy: torch.Tensor, planes: torch.Tensor, cin: int, tag: str = "conv3x3_s2_dgrad", tile_rows: int = 0, bn_bwd=None):
    """Input gradient of a 3x3 / padding-1 / stride-2 convolution, 16-bit: gy [N, Cout, Ho, Wo] channels_last -> dx
    [N, cin, 2 Ho, 2 Wo] (peclr_conv3x3_s2_dgrad_h: one implicit GEMM per parity class of input pixels)."""
    nb, cout, ho, wo = gy.shape
    io = _half_io(gy, "conv3x3_s2_dgrad_h gy")
    gp = _nhwc_ptr(gy, "conv3x3_s2_dgrad_h gy", gy.dtype)
    _h_planes_ok(planes, cin, 9 * cout, "conv3x3_s2_dgrad_h")
    dx = torch.empty((nb, cin, 2 * ho, 2 * wo), device=gy.device, dtype=gy.dtype, memory_format=torch.channels_last)
    mc = nb * ho * wo
    tile_rows, partial, ns, fuse = _epilogue("conv3x3_s2_dgrad_h", 4 * mc, cin, tile_rows, None, bn_bwd, gy.device, groups=4, dtype=gy.dtype,
                                             pick_rows=lambda: lib().peclr_conv_h_tile_rows(mc, cin))
    _launch(tag, "peclr_conv3x3_s2_dgrad_h", io, nb, ho, wo, cout, cin, gp, _ptr(planes, torch.uint8), dx.data_ptr(), tile_rows,
            _hzeros(gy.device, gy.dtype).data_ptr(), _byref(fuse), _stream(),
            nbytes=2 * (mc * cout + 4 * mc * cin * (2 if fuse is not None else 1) + 9 * cin * cout), flops=18 * mc * cin * cout,
            kernel="conv_h_kernel (3x3)")
    return _with_partial(dx, partial, ns)


# ------------------------------------------------------------------ stem (csrc/stem.hip)
STEM_FMT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}      # output / arithmetic of peclr_stem_conv7x7_s2


class StemPlanes:
    """The 7x7 stem filter [64, 3, 7, 7] (any strides) in the fragment order of peclr_stem_conv7x7_s2: three bf16 planes for
    fp32 runs (six products), one bf16 / fp16 plane for autocast runs.  `pack()` is one launch; call it after the weight changed."""

    def __init__(self, weight: torch.Tensor, dtype=torch.float32):
        if tuple(weight.shape) != (64, 3, 7, 7) or weight.dtype != torch.float32 or not weight.is_cuda:
            raise PeclrHipError(f"StemPlanes: an fp32 HIP [64, 3, 7, 7] filter expected, got {weight.dtype} {tuple(weight.shape)} on {weight.device}")
        self.fmt = STEM_FMT[dtype]
        self.weight = weight
        self.planes = torch.empty(lib().peclr_stem_pack_bytes(self.fmt), device=weight.device, dtype=torch.uint8)

    def pack(self):
        w = self.weight
        _launch("stem_pack", "peclr_stem_pack", w.data_ptr(), *w.stride(), self.planes.data_ptr(), self.fmt, _stream(),
                nbytes=4 * w.numel() + self.planes.numel(), kernel="stem_pack_kernel")
        return self


def stem_conv(x: torch.Tensor, planes: "StemPlanes", stat_shift: Optional[torch.Tensor] = None, tag: str = "stem_fwd"):
    """y [N, 64, H/2, W/2] channels_last = conv2d(x, W, stride 2, padding 3) for fp32 channels_last images x [N, 3, H, W]
    (peclr_stem_conv7x7_s2); y is fp32 (fp32 accuracy: six bf16 products) or bf16 / fp16 (one product of the rounded operands:
    autocast) as `planes` was packed.  stat_shift (fp32 [64]): also the training statistics of y as (partial, n_split) in the
    layout of peclr_bn2d_stats -> (y, partial, n_split)."""
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous(memory_format=torch.channels_last):
        raise PeclrHipError(f"stem_conv: fp32 channels_last HIP images [N, 3, H, W] expected, got {x.dtype} {tuple(x.shape)} on {x.device} "
                            "(peclr_amd has no CPU path)")
    n, _, h, w = x.shape
    ns = lib().peclr_stem_workgroups(n, h, w)
    if ns < 1:
        raise PeclrHipError(f"stem_conv: unsupported image size {h} x {w}")
    out_dtype = {v: k for k, v in STEM_FMT.items()}[planes.fmt]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, 64, ho, wo), device=x.device, dtype=out_dtype, memory_format=torch.channels_last)
    _, partial, ns, _ = _epilogue("stem_conv", n * ho * wo, 64, 0, stat_shift, None, x.device, row_blocks=ns)     # (one block per workgroup)
    _launch(tag, "peclr_stem_conv7x7_s2", x.data_ptr(), n, h, w, planes.planes.data_ptr(), planes.fmt, y.data_ptr(), _ptr(stat_shift),
            partial.data_ptr() if partial is not None else None, _stream(),
            nbytes=4 * x.numel() + y.element_size() * y.numel() + planes.planes.numel(), flops=2 * n * ho * wo * 64 * 147,
            kernel="stem_fwd_kernel")
    return _with_partial(y, partial, ns)


def stem_wgrad(gy: torch.Tensor, x: torch.Tensor, tag: str = "stem_wgrad") -> torch.Tensor:
    """dW [64, 3, 7, 7] (fp32; a view of a [64, 7, 8, 4] buffer: the layout the kernel accumulates in) of the stem convolution
    for channels_last gy [N, 64, H/2, W/2] (fp32, or bf16 / fp16 under autocast) and the fp32 channels_last images x [N, 3, H, W]
    (peclr_stem_wgrad + peclr_slab_reduce_f32: fixed-order slabs, deterministic)."""
    if (x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous(memory_format=torch.channels_last)
            or gy.dtype not in STEM_FMT or gy.dim() != 4 or gy.shape[1] != 64 or not gy.is_contiguous(memory_format=torch.channels_last)):
        raise PeclrHipError(f"stem_wgrad: fp32 channels_last images and a channels_last [N, 64, H/2, W/2] gradient expected, got "
                            f"{x.dtype} {tuple(x.shape)}, {gy.dtype} {tuple(gy.shape)} (peclr_amd has no CPU path)")
    n, _, h, w = x.shape
    if tuple(gy.shape) != (n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1):
        raise PeclrHipError(f"stem_wgrad: gradient {tuple(gy.shape)} for images {tuple(x.shape)}")
    fmt = STEM_FMT[gy.dtype]
    ns = lib().peclr_stem_wgrad_slabs(n, h, w, fmt)
    if ns < 1:
        raise PeclrHipError(f"stem_wgrad: unsupported image size {h} x {w}")
    slabs = torch.empty((ns, 64, 224), device=x.device, dtype=torch.float32)
    _launch(tag, "peclr_stem_wgrad", x.data_ptr(), gy.data_ptr(), n, h, w, fmt, slabs.data_ptr(), ns, _stream(),
            nbytes=4 * x.numel() + gy.element_size() * gy.numel() + 4 * slabs.numel(), flops=2 * gy.numel() * 147, kernel="stem_wgrad_kernel")
    dw = _sum_slabs(slabs, "wgrad_slab_reduce")
    return dw.view(64, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2)          # [n][kh][kw][c] -> [n][c][kh][kw]


# ------------------------------------------------------------------ backbone glue: BN2d (+add) (+ReLU), NHWC
_IO = {torch.float32: (DTYPE_F32, 4), torch.bfloat16: (DTYPE_BF16, 2), torch.float16: (DTYPE_F16, 2)}


def _nhwc_ptr(t: torch.Tensor, what: str, dtype=None):
    if not t.is_cuda:
        raise PeclrHipError(f"{what}: expected a HIP device tensor (peclr_amd has no CPU path)")
    if t.dtype not in _IO or t.dim() != 4 or (dtype is not None and t.dtype != dtype):
        raise PeclrHipError(f"{what}: expected a 4-D {dtype or 'fp32/bf16/fp16'} tensor, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous(memory_format=torch.channels_last):
        raise PeclrHipError(f"{what}: tensor must be channels_last (NHWC) contiguous")
    return t.data_ptr()


def bn2d_n_split(r: int, c: int, io: int) -> int:
    n = lib().peclr_bn2d_n_split(r, c, io)
    if n < 1:
        raise PeclrHipError(f"fused BatchNorm2d: unsupported shape R={r} C={c} (C must be a ResNet width)")
    return n


def _sync_totals(partial, ns, c, rows, group):
    """Synchronised BatchNorm: combine this rank's slice partials into double [2][C] totals, append the
    row count and SUM-all-reduce over `group`.  Returns (local totals, global totals, global rows)."""
    import torch.distributed as td

    local = torch.empty(2 * c + 1, device=partial.device, dtype=torch.float64)
    _launch("bn2d_combine", "peclr_bn2d_combine_f64", partial.data_ptr(), ns, c, local.data_ptr(), _stream(), nbytes=8 * ns * c)
    local[2 * c] = float(rows)
    total = local.clone()
    td.all_reduce(total, op=td.ReduceOp.SUM, group=group)
    return local, total


def _bn2d_scale_shift(x, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, sync_group=None, sync_shift=None,
                      pre=None):
    """stats -> finalize: (save [mean, invstd], scale_shift) for x [N,C,H,W] NHWC; updates the running
    statistics in training mode."""
    n, c, h, w = x.shape
    r = n * h * w
    dev = x.device
    xp = _nhwc_ptr(x, "bn2d x")
    io, e = _IO[x.dtype]
    save = torch.empty((2, c), device=dev, dtype=torch.float32)
    ss = torch.empty((2, c), device=dev, dtype=torch.float32)
    part_ptr, ns = None, 0
    sync = sync_group is not None
    if training and pre is not None:
        # the producer of x (a GEMM epilogue) already summed the statistics per row block: `pre` = (partial, n_split,
        # shift it used) in peclr_bn2d_stats' layout; nothing re-reads x here
        partial, ns, shift = pre
        if tuple(partial.shape) != (2 * ns + 1, c):
            raise PeclrHipError(f"bn2d: precomputed statistics of shape {tuple(partial.shape)} for C = {c}, n_split = {ns}")
        part_ptr = _ptr(partial, what="bn2d partial statistics")
    elif training:
        ns = bn2d_n_split(r, c, io)
        partial = torch.empty((2 * ns + 1, c), device=dev, dtype=torch.float32)
        part_ptr = partial.data_ptr()
        if sync and running_mean is None and sync_shift is None:
            raise PeclrHipError("synchronised BatchNorm needs running statistics (their mean is the common shift)")
        # synchronised: every rank must subtract the SAME shift before summing -> the (replicated) running mean, or the
        # copy of it the caller kept (re-run of a checkpointed block: the running statistics have moved since)
        shift = (sync_shift if sync_shift is not None else running_mean.detach().clone()) if sync else None
        _launch("bn2d_stats", "peclr_bn2d_stats", xp, io, r, c, _ptr(shift), part_ptr, ns, _stream(), nbytes=e * r * c)
    if training and sync:
        _, total = _sync_totals(partial, ns, c, r, sync_group)
        _launch("bn2d_finalize", "peclr_bn2d_finalize_totals_f32", total.data_ptr(), shift.data_ptr(), c, eps, momentum,
                _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(nbt, torch.int64, "num_batches_tracked"),
                save[0].data_ptr(), save[1].data_ptr(), ss.data_ptr(), _stream(), nbytes=16 * c)
    else:
        _launch("bn2d_finalize", "peclr_bn2d_finalize_f32", part_ptr, ns, r, c, int(training), eps, momentum, _ptr(gamma), _ptr(beta),
                _ptr(running_mean), _ptr(running_var), _ptr(nbt, torch.int64, "num_batches_tracked") if training else None,
                save[0].data_ptr(), save[1].data_ptr(), ss.data_ptr(), _stream(), nbytes=8 * ns * c)
    return save, ss


class BnEvalTables:
    """The eval-mode scale / shift tables of a list of BatchNorm2d layers, written by ONE launch (peclr_bn2d_eval_tables) into
    one flat fp32 buffer; `table(i)` is layer i's [2, C] view of it.  `layers`: (gamma, beta, running_mean, running_var, eps)
    per layer, fp32 HIP tensors.  The descriptor table is built and uploaded here, once; `stale(layers)` says whether a tensor
    has moved since (then build a new object -- not while a hipGraph is being captured: the upload is a host-to-device copy)."""

    def __init__(self, layers):
        if not layers:
            raise PeclrHipError("BnEvalTables: no layers")
        dev = layers[0][0].device
        rows, self.offsets, chan = [], [], 0
        for gamma, beta, rm, rv, eps in layers:
            c = gamma.numel()
            for t in (gamma, beta, rm, rv):
                _ptr(t, what="BnEvalTables: BatchNorm2d parameter / running statistic")
                if t.numel() != c or t.device != dev:
                    raise PeclrHipError("BnEvalTables: gamma, beta, running_mean, running_var of one layer are [C] tensors on one device")
            self.offsets.append((2 * chan, c))
            rows.append([gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0,
                         c | (int.from_bytes(struct.pack("<f", float(eps)), "little") << 32), 2 * chan, chan])
            chan += c
        self.flat = torch.empty(2 * chan, device=dev, dtype=torch.float32)
        for r in rows:
            r[4] = self.flat.data_ptr()
        self.ptrs = self._ptrs(layers)
        self._keep = [t for layer in layers for t in layer[:4]]
        self.table_dev = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.count, self.channels = len(rows), chan
        self.views = [self.flat[off:off + 2 * c].view(2, c) for off, c in self.offsets]

    @staticmethod
    def _ptrs(layers):
        return [(g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), float(eps)) for g, b, rm, rv, eps in layers]

    def stale(self, layers) -> bool:
        return self._ptrs(layers) != self.ptrs

    def launch(self):
        _launch("bn2d_eval_tables", "peclr_bn2d_eval_tables", self.table_dev.data_ptr(), self.count, self.channels, _stream(),
                nbytes=24 * self.channels, kernel="bn2d_eval_tables_kernel")
        return self

    def table(self, i: int) -> torch.Tensor:
        return self.views[i]


def bn2d_eval_tables(layers) -> "BnEvalTables":
    """One launch for the eval-mode tables of `layers` (see `BnEvalTables`); a caller that runs this every forward keeps the object
    and calls its `launch()`."""
    return BnEvalTables(layers).launch()


_ABSMAX_SLABS: dict = {}


def absmax_slot(device) -> torch.Tensor:
    """A zeroed one-element fp32 tensor for a pass's `absmax_out` (the "pair" GEMMs' peclr_x6_pair.a_absmax).  Slots are views of a
    256-float slab that ONE fill launch zeroes; a new slab is taken when the current one is used up -- and whenever a stream capture
    begins, so that the fill is part of the captured graph and every replay starts from zeros."""
    key = (device, capture_id())
    slab = _ABSMAX_SLABS.get(key)
    if slab is None or slab[1] >= slab[0].numel():
        for k in [k for k in _ABSMAX_SLABS if k[0] == device and k != key]:
            del _ABSMAX_SLABS[k]                       # (slots handed out stay alive through their views)
        slab = _ABSMAX_SLABS[key] = [torch.zeros(256, device=device, dtype=torch.float32), 0]
    i = slab[1]
    slab[1] += 1
    return slab[0][i:i + 1]


def _absmax_ptr(absmax, x):
    if absmax is None:
        return None
    if x.dtype != torch.float32 or not (absmax.is_cuda and absmax.dtype == torch.float32 and absmax.numel() == 1):
        raise PeclrHipError("absmax: a zeroed one-element fp32 HIP tensor, for fp32 passes")
    return absmax.data_ptr()


def bn2d_apply(x, ss, relu: bool = True, absmax=None):
    """y = (relu)(fmaf(x, scale, shift)) from a finished scale / shift table: the apply pass of `bn2d_fwd` on its own (the
    fallback of a layer whose apply was left to its consumer, `bn2d_fwd(..., apply=False)`)."""
    n, c, h, w = x.shape
    r = n * h * w
    io, e = _IO[x.dtype]
    y = torch.empty_like(x, memory_format=torch.channels_last)
    _launch("bn2d_apply", "peclr_bn2d_apply", _nhwc_ptr(x, "bn2d x"), None, io, r, c, ss.data_ptr(), int(relu), y.data_ptr(), None,
            _absmax_ptr(absmax, x), _stream(), nbytes=2 * e * r * c)
    return y


def bn2d_fwd(x, residual, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, relu,
             want_mask=False, sync_group=None, sync_shift=None, pre=None, apply=True, residual_bn=None, absmax=None):
    """want_mask: also write the 1-bit ReLU mask ([R, C/32] int32) the backward reads instead of y.
    absmax: a zeroed one-element fp32 tensor (`absmax_slot`) that receives max |y|.
    residual_bn = (x_s, scale_shift_s) instead of `residual`: the residual is the output of the shortcut's BatchNorm2d, which
    was not written -- this pass computes it from that layer's input and table (peclr_bn2d_apply_res_bn).
    sync_group: a process group -> training statistics are those of the rows of ALL its ranks
    (mean/var of the global batch, as one device holding the concatenated batch would compute)."""
    n, c, h, w = x.shape
    r = n * h * w
    dev = x.device
    xp = _nhwc_ptr(x, "bn2d x")
    io, e = _IO[x.dtype]
    save, ss = _bn2d_scale_shift(x, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, sync_group, sync_shift, pre)
    if not apply:                        # statistics and the table only: the consumer applies them in its operand path
        if residual is not None or want_mask:
            raise PeclrHipError("bn2d_fwd(apply=False): plain BatchNorm (+ ReLU) layers only")
        return None, save, ss, None
    y = torch.empty_like(x, memory_format=torch.channels_last)
    mask = torch.empty((r, c // 32), device=dev, dtype=torch.int32) if (want_mask and relu and c % 32 == 0) else None
    mask_bytes = r * c // 8 if mask is not None else 0
    tail = (io, r, c, ss.data_ptr(), int(relu), y.data_ptr(), mask.data_ptr() if mask is not None else None)
    if residual_bn is not None:
        xs, ss_s = residual_bn
        if residual is not None or tuple(xs.shape) != tuple(x.shape) or ss_s.numel() != 2 * c or ss_s.dtype != torch.float32:
            raise PeclrHipError("bn2d_fwd: residual_bn = (input of the shortcut's BatchNorm, its fp32 [2, C] table), no residual tensor")
        _launch("bn2d_apply", "peclr_bn2d_apply_res_bn", xp, _nhwc_ptr(xs, "bn2d shortcut x", x.dtype), ss_s.data_ptr(), *tail,
                _absmax_ptr(absmax, x), _stream(), nbytes=3 * e * r * c + mask_bytes)
    else:
        _launch("bn2d_apply", "peclr_bn2d_apply", xp, _nhwc_ptr(residual, "bn2d residual", x.dtype) if residual is not None else None, *tail,
                _absmax_ptr(absmax, x), _stream(), nbytes=(3 if residual is not None else 2) * e * r * c + mask_bytes)
    return y, save, ss, mask


def _bn2d_bwd_finalize(partial, ns, r, c, ss, training, sync_group):
    """The middle launch of every BatchNorm2d backward: the reduction's partials [2 n_split, C] -> (dparams [dgamma, dbeta], coef
    [2, C] for the apply pass).  Synchronised (training with a `sync_group`): dgamma / dbeta from this rank's totals, coef from
    the group's."""
    dparams = torch.empty((2, c), device=partial.device, dtype=torch.float32)
    coef = torch.empty((2, c), device=partial.device, dtype=torch.float32)
    out = (ss.data_ptr(), dparams[0].data_ptr(), dparams[1].data_ptr(), coef.data_ptr(), _stream())
    if training and sync_group is not None:
        local, total = _sync_totals(partial, ns, c, r, sync_group)
        _launch("bn2d_bwd_finalize", "peclr_bn2d_bwd_finalize_totals_f32", local.data_ptr(), total.data_ptr(), c, 1, *out, nbytes=32 * c)
    else:
        _launch("bn2d_bwd_finalize", "peclr_bn2d_bwd_finalize_f32", partial.data_ptr(), ns, r, c, int(training), *out, nbytes=8 * ns * c)
    return dparams, coef


def bn2d_bwd(dy, x, y, mask, save, ss, training, relu, want_dres, sync_group=None, pre=None, absmax=None):
    """ReLU mask source: `mask` (bit mask from the forward) > `y` (forward output) > recomputed from x.
    sync_group: as in bn2d_fwd; dgamma/dbeta stay this rank's local sums (the gradient all-reduce sums
    them later), dx uses the global sums."""
    n, c, h, w = x.shape
    r = n * h * w
    dev = x.device
    io, e = _IO[x.dtype]
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    dres = torch.empty_like(x, memory_format=torch.channels_last) if want_dres else None
    dyp, xp = _nhwc_ptr(dy, "bn2d dy", x.dtype), _nhwc_ptr(x, "bn2d x")
    yp = _nhwc_ptr(y, "bn2d y", x.dtype) if (y is not None and mask is None) else None
    mp = _ptr(mask, torch.int32, "relu mask")
    extra = (r * c // 8) if mask is not None else (e * r * c if yp is not None else 0)
    head = (dyp, xp, yp, mp, io, r, c, int(relu), save[0].data_ptr(), save[1].data_ptr(), ss.data_ptr())
    if pre is not None:
        # the GEMM that produced dy already reduced it against this layer's x in its epilogue (peclr_bn_bwd_fuse)
        partial, ns = pre
        if tuple(partial.shape) != (2 * ns, c):
            raise PeclrHipError(f"bn2d backward: precomputed reduction of shape {tuple(partial.shape)} for C = {c}, n_split = {ns}")
    else:
        ns = bn2d_n_split(r, c, io)
        partial = torch.empty((2 * ns, c), device=dev, dtype=torch.float32)
        _launch("bn2d_bwd_reduce", "peclr_bn2d_bwd_reduce", *head, partial.data_ptr(), ns, _stream(), nbytes=2 * e * r * c + extra)
    dparams, coef = _bn2d_bwd_finalize(partial, ns, r, c, ss, training, sync_group)
    _launch("bn2d_bwd_apply", "peclr_bn2d_bwd_apply", *head, coef.data_ptr(), dx.data_ptr(), dres.data_ptr() if dres is not None else None,
            _absmax_ptr(absmax, x), _stream(), nbytes=(3 + (1 if want_dres else 0)) * e * r * c + extra)
    return dx, dparams[0], dparams[1], dres


def bn2d_bwd_res_bn(dy, x, mask, save, ss, training, xs, save_s, ss_s, training_s, pre=None, absmax=None, absmax_s=None):
    """Backward of `bn2d_fwd(..., relu=True, residual_bn=(xs, ss_s))`, both BatchNorm layers at once: (dx, dgamma, dbeta, dxs,
    dgamma_s, dbeta_s).  The gradient that reaches the shortcut's layer is mask . dy; it is not written out: that layer's reduction
    reads (dy, mask) against xs (the partial table `bn2d_bwd` would sum from the written tensor, n_split included), and ONE apply
    pass writes dx and dxs (peclr_bn2d_bwd_apply_res_bn) -- bit-identical to `bn2d_bwd(want_dres=True)` followed by the shortcut
    layer's own `bn2d_bwd`.  pre: as in `bn2d_bwd` (the sums of THIS layer); per-rank statistics only."""
    n, c, h, w = x.shape
    r = n * h * w
    dev = x.device
    io, e = _IO[x.dtype]
    if mask is None or c % 32 or tuple(xs.shape) != tuple(x.shape):
        raise PeclrHipError("bn2d_bwd_res_bn: needs the forward's 1-bit ReLU mask (C % 32 == 0) and a shortcut input of x's shape")
    dyp, xp, xsp = _nhwc_ptr(dy, "bn2d dy", x.dtype), _nhwc_ptr(x, "bn2d x"), _nhwc_ptr(xs, "bn2d shortcut x", x.dtype)
    mp = _ptr(mask, torch.int32, "relu mask")
    mask_bytes = r * c // 8
    ns = bn2d_n_split(r, c, io)
    partial_s = torch.empty((2 * ns, c), device=dev, dtype=torch.float32)
    _launch("bn2d_bwd_reduce", "peclr_bn2d_bwd_reduce", dyp, xsp, None, mp, io, r, c, 1, save_s[0].data_ptr(), save_s[1].data_ptr(),
            ss_s.data_ptr(), partial_s.data_ptr(), ns, _stream(), nbytes=2 * e * r * c + mask_bytes)
    dparams_s, coef_s = _bn2d_bwd_finalize(partial_s, ns, r, c, ss_s, training_s, None)
    if pre is not None:
        partial, ns = pre
        if tuple(partial.shape) != (2 * ns, c):
            raise PeclrHipError(f"bn2d backward: precomputed reduction of shape {tuple(partial.shape)} for C = {c}, n_split = {ns}")
    else:
        partial = torch.empty((2 * ns, c), device=dev, dtype=torch.float32)
        _launch("bn2d_bwd_reduce", "peclr_bn2d_bwd_reduce", dyp, xp, None, mp, io, r, c, 1, save[0].data_ptr(), save[1].data_ptr(),
                ss.data_ptr(), partial.data_ptr(), ns, _stream(), nbytes=2 * e * r * c + mask_bytes)
    dparams, coef = _bn2d_bwd_finalize(partial, ns, r, c, ss, training, None)
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    dxs = torch.empty_like(x, memory_format=torch.channels_last)
    _launch("bn2d_bwd_apply", "peclr_bn2d_bwd_apply_res_bn", dyp, mp, xp, xsp, io, r, c, save[0].data_ptr(), save[1].data_ptr(),
            ss.data_ptr(), coef.data_ptr(), save_s[0].data_ptr(), save_s[1].data_ptr(), ss_s.data_ptr(), coef_s.data_ptr(),
            dx.data_ptr(), dxs.data_ptr(), _absmax_ptr(absmax, x), _absmax_ptr(absmax_s, x), _stream(),
            nbytes=5 * e * r * c + mask_bytes)
    return dx, dparams[0], dparams[1], dxs, dparams_s[0], dparams_s[1]


def bn2d_avgpool_fwd(x, residual, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, sync_group=None,
                     sync_shift=None, pre=None):
    """Encoder tail: mean over H x W of relu(bn(x) + residual) as fp32 [N, C]; the activation itself is not
    written.  Returns (pooled, relu mask, save, scale_shift)."""
    n, c, h, w = x.shape
    r = n * h * w
    if c % 32 or residual is None:
        raise PeclrHipError("fused BN + add + ReLU + average pool needs a residual and C % 32 == 0")
    io, e = _IO[x.dtype]
    save, ss = _bn2d_scale_shift(x, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, sync_group, sync_shift, pre)
    pooled = torch.empty((n, c), device=x.device, dtype=torch.float32)
    mask = torch.empty((r, c // 32), device=x.device, dtype=torch.int32)
    _launch("bn2d_apply_avgpool", "peclr_bn2d_apply_avgpool", _nhwc_ptr(x, "bn2d x"), _nhwc_ptr(residual, "bn2d residual", x.dtype), io, n,
            h * w, c, ss.data_ptr(), pooled.data_ptr(), mask.data_ptr(), _stream(), nbytes=2 * e * r * c + r * c // 8 + 4 * n * c)
    return pooled, mask, save, ss


def bn2d_avgpool_bwd(d_pooled, x, mask, save, ss, training, sync_group=None, absmax=None):
    """Backward of bn2d_avgpool_fwd from the fp32 [N, C] gradient of the pooled output: (dx, dgamma, dbeta,
    d_residual)."""
    n, c, h, w = x.shape
    r = n * h * w
    io, e = _IO[x.dtype]
    ns = bn2d_n_split(r, c, io)
    partial = torch.empty((2 * ns, c), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    dres = torch.empty_like(x, memory_format=torch.channels_last)
    head = (_ptr(d_pooled, what="d_pooled"), _nhwc_ptr(x, "bn2d x"), _ptr(mask, torch.int32, "relu mask"), io, n, h * w, c,
            save[0].data_ptr(), save[1].data_ptr(), ss.data_ptr())
    _launch("bn2d_bwd_reduce_avgpool", "peclr_bn2d_bwd_reduce_avgpool", *head, partial.data_ptr(), ns, _stream(),
            nbytes=e * r * c + r * c // 8 + 4 * n * c)
    dparams, coef = _bn2d_bwd_finalize(partial, ns, r, c, ss, training, sync_group)
    _launch("bn2d_bwd_apply_avgpool", "peclr_bn2d_bwd_apply_avgpool", *head, coef.data_ptr(), dx.data_ptr(), dres.data_ptr(),
            _absmax_ptr(absmax, x), _stream(), nbytes=3 * e * r * c + r * c // 8 + 4 * n * c)
    return dx, dparams[0], dparams[1], dres


def bn2d_pool_fwd(x, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, sync_group=None, sync_shift=None,
                  pre=None, absmax=None):
    """Stem: y = maxpool3x3/2(relu(bn(x))) in one pass; returns (y, tap codes, save, scale_shift).
    pre: (partial, n_split, shift) -- the statistics the stem convolution summed in its epilogue (no pass over x then)."""
    n, c, h, w = x.shape
    io, e = _IO[x.dtype]
    save, ss = _bn2d_scale_shift(x, gamma, beta, running_mean, running_var, nbt, training, eps, momentum, sync_group, sync_shift, pre)
    ph, pw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, c, ph, pw), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    x_at_max = torch.empty_like(y)
    code = torch.empty((n, ph, pw, c), device=x.device, dtype=torch.uint8)
    _launch("bn2d_pool_apply", "peclr_bn2d_pool_apply", _nhwc_ptr(x, "bn2d x"), io, n, h, w, c, ss.data_ptr(), y.data_ptr(),
            x_at_max.data_ptr(), code.data_ptr(), _absmax_ptr(absmax, x), _stream(),
            nbytes=e * n * c * (h * w + 2 * ph * pw) + n * c * ph * pw)
    return y, x_at_max, code, save, ss


def bn2d_pool_bwd(dy, x, x_at_max, code, save, ss, training, sync_group=None):
    n, c, h, w = x.shape
    r = n * h * w
    ph, pw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    io, e = _IO[x.dtype]
    ns = lib().peclr_bn2d_pool_n_split(n, h, w, c, io)
    if ns < 1:
        raise PeclrHipError(f"fused stem BN+ReLU+max-pool: unsupported shape {tuple(x.shape)}")
    partial = torch.empty((2 * ns, c), device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    dyp, xp = _nhwc_ptr(dy, "pooled dy", x.dtype), _nhwc_ptr(x, "bn2d x")
    pooled = n * c * ph * pw
    _launch("bn2d_pool_bwd_reduce", "peclr_bn2d_pool_bwd_reduce", dyp, _nhwc_ptr(x_at_max, "x at the maximum", x.dtype), io, n, h, w, c,
            save[0].data_ptr(), save[1].data_ptr(), ss.data_ptr(), partial.data_ptr(), ns, _stream(), nbytes=2 * e * pooled)
    dparams, coef = _bn2d_bwd_finalize(partial, ns, r, c, ss, training, sync_group)
    _launch("bn2d_pool_bwd_apply", "peclr_bn2d_pool_bwd_apply", dyp, xp, code.data_ptr(), io, n, h, w, c, save[0].data_ptr(),
            save[1].data_ptr(), ss.data_ptr(), coef.data_ptr(), dx.data_ptr(), _stream(), nbytes=(e + 1) * pooled + 2 * e * r * c)
    return dx, dparams[0], dparams[1]


# ------------------------------------------------------------------ two-view augmentation (pixel side)
AUG_PARAM_DOUBLES = 16
AUG_EXT_INTS = 8
AUG_EXT_BLUR = 4
AUG_EXT_PRE, AUG_EXT_POST = 1 | 2 | 4, 8 | 16  # sobel, cut-out, blur | noise, colour drop


def _aug_params(params: torch.Tensor, b: int) -> int:
    """params [V,B,16] float64 (HIP) for a batch of b -> V."""
    if (params.dtype != torch.float64 or params.dim() != 3 or params.shape[1] != b
            or params.shape[2] != AUG_PARAM_DOUBLES or not params.is_cuda or not params.is_contiguous()):
        raise PeclrHipError(f"augment: params must be a contiguous [V,{b},{AUG_PARAM_DOUBLES}] float64 HIP tensor")
    return params.shape[0]


def _aug_uniform_args(images: torch.Tensor, params: torch.Tensor):
    """images [B,H,W,3] uint8 (HIP) and their params -> (b, v)."""
    if not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise PeclrHipError(f"augment: images must be a [B,H,W,3] uint8 HIP tensor, got {images.dtype} "
                            f"{tuple(images.shape)} on {images.device} (peclr_amd has no CPU path)")
    if not images.is_contiguous():
        raise PeclrHipError("augment: images must be contiguous")
    return images.shape[0], _aug_params(params, images.shape[0])


class _AugExt:
    """The checked arguments of the other five augmentations: ext [V,B,8] int32 records, coefs int32 Q8 blur taps, noise_table
    int32 storage of n_table uint32 thresholds, the Philox key and call index, and `ops`, the OR of all records' bits."""

    def __init__(self, v, b, ext, coefs, noise_table, n_table, noise_seed, call, ops):
        if ext.dtype != torch.int32 or tuple(ext.shape) != (v, b, AUG_EXT_INTS) or not ext.is_cuda or not ext.is_contiguous():
            raise PeclrHipError(f"augment: ext must be a contiguous [{v},{b},{AUG_EXT_INTS}] int32 HIP tensor")
        for name, t in (("coefs", coefs), ("noise_table", noise_table)):
            if t.dtype != torch.int32 or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
                raise PeclrHipError(f"augment: {name} must be a contiguous 1-D int32 HIP tensor")
        if not 0 <= n_table <= noise_table.numel():
            raise PeclrHipError(f"augment: n_table {n_table} exceeds the table's {noise_table.numel()} entries")
        self.ext, self.coefs, self.ops = ext.data_ptr(), coefs.data_ptr(), ops
        self.noise = (ext.data_ptr(), noise_table.data_ptr(), n_table, noise_seed & (2 ** 64 - 1), call & 0xFFFFFFFF)


def _aug_mirror(mirror, b: int):
    """The per-sample left-hand table (None, or int32 [B] on the device, non-zero = the image is read mirrored) -> its pointer."""
    if mirror is None:
        return None
    if (not isinstance(mirror, torch.Tensor) or mirror.dtype != torch.int32 or tuple(mirror.shape) != (b,) or not mirror.is_cuda
            or not mirror.is_contiguous()):
        raise PeclrHipError(f"augment: mirror must be a contiguous [{b}] int32 HIP tensor")
    return mirror.data_ptr()


def _aug_out(v, b, out_hw, mean, std, channels_last, device):
    """The float32 [V*B,3,oh,ow] output and the tail of both resize entry points' arguments that writes it."""
    oh, ow = out_hw
    out = torch.empty((v * b, 3, oh, ow), device=device, dtype=torch.float32,
                      memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    mean_arr, std_arr = (c_float * 3)(*mean), (c_float * 3)(*std)
    return out, (oh, ow, ctypes.cast(mean_arr, c_void_p), ctypes.cast(std_arr, c_void_p), int(channels_last), out.data_ptr())


def _augment_uniform(images, params, b, v, aug, ksize, out_hw, mean, std, channels_last, mirror=None):
    """Both stages for same-size images -> (out, srcs or None, crops).  aug: `_AugExt` or None.  Stage 0 (sobel / cut-out /
    blur), when `aug.ops` names it, writes per-view sources and the warp then runs once per view on them.  mirror: the
    left-hand table's pointer or None; it goes to the ONE stage that reads `images` (stage 0 when it runs, else the warp),
    whose log entry then names the mirrored kernel."""
    _, h, w, _ = images.shape
    dev, stream = images.device, _stream()
    crops = torch.empty((v, b, h, w, 3), device=dev, dtype=torch.uint8)
    out, out_args = _aug_out(v, b, out_hw, mean, std, channels_last, dev)
    ops = aug.ops if aug is not None else 0
    srcs = None
    if ops & AUG_EXT_PRE:
        kx, ky = ksize
        srcs = torch.empty((v, b, h, w, 3), device=dev, dtype=torch.uint8)
        tmp = torch.empty((v, b, h, w, 3), device=dev, dtype=torch.int16) if ops & AUG_EXT_BLUR else None
        blur_bytes = (kx + ky) * 3 if tmp is not None else 0
        pre_tail = (srcs.data_ptr(), None if tmp is None else tmp.data_ptr(), stream)
        pre_work = dict(nbytes=v * b * h * w * (3 + 3 + 4 * (3 if tmp is not None else 0)), flops=v * b * h * w * blur_bytes)
        if mirror is None:
            _launch("augment_pre", "peclr_augment_pre_u8", images.data_ptr(), b, h, w, v, aug.ext, aug.coefs, kx, ky, *pre_tail,
                    **pre_work)
        else:
            _launch("augment_pre", "peclr_augment_pre_mirror_u8", images.data_ptr(), b, h, w, v, aug.ext, aug.coefs, kx, ky, mirror,
                    *pre_tail, kernel="pre_rows_kernel<Mirrored>", **pre_work)
        for i in range(v):
            _launch("augment_warp_crop", "peclr_augment_warp_crop_u8", srcs[i].data_ptr(), b, h, w, 1, params[i].data_ptr(),
                    crops[i].data_ptr(), stream, nbytes=2 * b * h * w * 3)
    elif mirror is None:
        _launch("augment_warp_crop", "peclr_augment_warp_crop_u8", images.data_ptr(), b, h, w, v, params.data_ptr(), crops.data_ptr(),
                stream, nbytes=2 * v * b * h * w * 3)
    else:
        _launch("augment_warp_crop", "peclr_augment_warp_crop_mirror_u8", images.data_ptr(), b, h, w, v, params.data_ptr(), mirror,
                crops.data_ptr(), stream, nbytes=2 * v * b * h * w * 3, kernel="warp_crop_kernel<Mirrored>")
    head = (crops.data_ptr(), b, h, w, v, params.data_ptr())
    nbytes = v * b * (h * w * 3 + out_hw[0] * out_hw[1] * 12)
    if ops & AUG_EXT_POST:
        _launch("augment_resize_color_norm_ext", "peclr_augment_resize_color_norm_ext", *head, *aug.noise, *out_args, stream, nbytes=nbytes)
    else:
        _launch("augment_resize_color_norm", "peclr_augment_resize_color_norm", *head, *out_args, stream, nbytes=nbytes)
    return out, srcs, crops


def augment_views(images: torch.Tensor, params: torch.Tensor, out_hw, mean, std, channels_last: bool = True,
                  mirror: Optional[torch.Tensor] = None):
    """images [B,H,W,3] uint8 (HIP), params [V,B,16] float64 (HIP) -> float32 [V*B,3,out_h,out_w]
    (channels_last storage if asked).  Two launches: rotate+crop window, then resize+colour+normalise.
    mirror: None, or int32 [B] (HIP), non-zero = that sample's image is read mirrored (a left hand; include/peclr_hip.h) --
    the same two launches, the warp through its `_mirror` entry point."""
    b, v = _aug_uniform_args(images, params)
    out, _, crops = _augment_uniform(images, params, b, v, None, None, out_hw, mean, std, channels_last, _aug_mirror(mirror, b))
    return out, crops


def augment_views_ext(images: torch.Tensor, params: torch.Tensor, ext: torch.Tensor, coefs: torch.Tensor, ksize,
                      noise_table: torch.Tensor, n_table: int, noise_seed: int, call: int, ops: int, out_hw, mean, std,
                      channels_last: bool = True, mirror: Optional[torch.Tensor] = None):
    """augment_views plus the reference's other five augmentations (peclr_amd/augment.py builds the inputs):
    ext [V,B,8] int32 records, coefs int32 Q8 blur taps, ksize (horizontal, vertical) blur lengths of the batch,
    noise_table int32 storage of n_table uint32 thresholds, the Philox key and call index, and `ops`, the OR of
    all records' bits (the stages it names are the only ones launched).  Stage 0 (sobel / cut-out / blur) writes
    per-view sources, the warp then runs once per view on them.  mirror: as augment_views; stage 0 mirrors when it runs
    (srcs then hold the mirrored images and the warp reads them as they are), the warp otherwise.
    Returns (out, srcs or None, crops)."""
    b, v = _aug_uniform_args(images, params)
    aug = _AugExt(v, b, ext, coefs, noise_table, n_table, noise_seed, call, ops)
    return _augment_uniform(images, params, b, v, aug, ksize, out_hw, mean, std, channels_last, _aug_mirror(mirror, b))


# ---- the same for a batch whose images differ in size (include/peclr_hip.h: the geometry tables)
AUG_GEOM_INT64S, AUG_WIN_INT64S = 5, 4


def ragged_image(buf: torch.Tensor, geom: torch.Tensor, i: int) -> torch.Tensor:
    """Sample i's [H,W,3] image in one view of a packed buffer (the source, or srcs[v] of augment_views_ragged_ext)."""
    off, h, w = (int(t) for t in geom[i, :3])
    return buf[off:off + h * w * 3].view(h, w, 3)


def ragged_window(crops: torch.Tensor, wins: torch.Tensor, v: int, i: int) -> torch.Tensor:
    """The [ch,cw,3] crop window of (view v, sample i) in the scratch the ragged calls return."""
    off, stride, cw, ch = (int(t) for t in wins[v, i])
    return crops[off:off + ch * stride * 3].view(ch, stride, 3)[:, :cw]


def _ragged_args(packed, geom, wins, params):
    if not packed.is_cuda or packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise PeclrHipError(f"augment: the packed images must be a contiguous 1-D uint8 HIP tensor, got {packed.dtype} "
                            f"{tuple(packed.shape)} on {packed.device} (peclr_amd has no CPU path)")
    if geom.is_cuda or geom.dtype != torch.int64 or geom.dim() != 2 or geom.shape[1] != AUG_GEOM_INT64S or geom.shape[0] < 1:
        raise PeclrHipError(f"augment: geom must be a host [B,{AUG_GEOM_INT64S}] int64 tensor")
    b = geom.shape[0]
    v = _aug_params(params, b)
    if wins.is_cuda or wins.dtype != torch.int64 or tuple(wins.shape) != (v, b, AUG_WIN_INT64S):
        raise PeclrHipError(f"augment: wins must be a host [{v},{b},{AUG_WIN_INT64S}] int64 tensor")
    ends = geom[:, 0] + geom[:, 1] * geom[:, 2] * 3
    if int(geom[:, :3].min()) < 0 or int(geom[:, 1:3].min()) < 1 or int(ends.max()) > packed.numel():
        raise PeclrHipError(f"augment: geom names bytes outside the packed buffer of {packed.numel()}")
    if int(wins.min()) < 0 or int(wins[..., 2:].min()) < 1 or bool((wins[..., 1] < wins[..., 2]).any()):
        raise PeclrHipError("augment: wins needs offsets >= 0, windows of at least one pixel and row strides >= their width")
    # the scratch ends where the last window row does
    scratch = int((wins[..., 0] + ((wins[..., 3] - 1) * wins[..., 1] + wins[..., 2]) * 3).max())
    return b, v, scratch


def _augment_ragged(packed, geom, wins, params, b, v, scratch, aug, out_hw, mean, std, channels_last, mirror=None):
    """`_augment_uniform` for a packed batch (`_ragged_args` checked it) -> (out, srcs or None, crops)."""
    dev, stream = packed.device, _stream()
    total = packed.numel()
    geom_d, wins_d = geom.contiguous().to(dev, non_blocking=True), wins.contiguous().to(dev, non_blocking=True)
    crops = torch.empty(scratch, device=dev, dtype=torch.uint8)
    out, out_args = _aug_out(v, b, out_hw, mean, std, channels_last, dev)
    win_bytes = int((wins[..., 2] * wins[..., 3]).sum()) * 3
    max_cw, max_ch = int(wins[..., 2].max()), int(wins[..., 3].max())
    ops = aug.ops if aug is not None else 0
    srcs = None
    if ops & AUG_EXT_PRE:
        srcs = torch.empty((v, total), device=dev, dtype=torch.uint8)
        tmp = torch.empty((v, total), device=dev, dtype=torch.int16) if ops & AUG_EXT_BLUR else None
        # (without the blur stage the lengths are not read: nothing to check)
        kx, ky = (int(geom[:, 3].max()), int(geom[:, 4].max())) if tmp is not None else (1, 1)
        blur_work = int(((geom[:, 3] + geom[:, 4]) * geom[:, 1] * geom[:, 2]).sum()) * 3 if tmp is not None else 0
        pre_head = (packed.data_ptr(), b, v, geom_d.data_ptr(), total, int(geom[:, 1].max()), int(geom[:, 2].max()), aug.ext, aug.coefs,
                    kx, ky)
        pre_tail = (srcs.data_ptr(), None if tmp is None else tmp.data_ptr(), stream)
        pre_work = dict(nbytes=v * total * (1 + 1 + (4 if tmp is not None else 0)), flops=v * blur_work)
        if mirror is None:
            _launch("augment_pre", "peclr_augment_pre_ragged_u8", *pre_head, *pre_tail, **pre_work)
        else:
            _launch("augment_pre", "peclr_augment_pre_ragged_mirror_u8", *pre_head, mirror, *pre_tail,
                    kernel="pre_rows_kernel<Mirrored>", **pre_work)
        for i in range(v):
            _launch("augment_warp_crop", "peclr_augment_warp_crop_ragged_u8", srcs[i].data_ptr(), b, 1, geom_d.data_ptr(), params[i].data_ptr(),
                    wins_d[i].data_ptr(), max_cw, max_ch, crops.data_ptr(), stream, nbytes=2 * int((wins[i, :, 2] * wins[i, :, 3]).sum()) * 3)
    elif mirror is None:
        _launch("augment_warp_crop", "peclr_augment_warp_crop_ragged_u8", packed.data_ptr(), b, v, geom_d.data_ptr(), params.data_ptr(),
                wins_d.data_ptr(), max_cw, max_ch, crops.data_ptr(), stream, nbytes=2 * win_bytes)
    else:
        _launch("augment_warp_crop", "peclr_augment_warp_crop_ragged_mirror_u8", packed.data_ptr(), b, v, geom_d.data_ptr(),
                params.data_ptr(), wins_d.data_ptr(), max_cw, max_ch, mirror, crops.data_ptr(), stream, nbytes=2 * win_bytes,
                kernel="warp_crop_kernel<Mirrored>")
    head = (crops.data_ptr(), b, v, wins_d.data_ptr(), params.data_ptr())
    nbytes = win_bytes + v * b * out_hw[0] * out_hw[1] * 12
    if ops & AUG_EXT_POST:
        _launch("augment_resize_color_norm_ext", "peclr_augment_resize_color_norm_ragged_ext", *head, *aug.noise, *out_args, stream, nbytes=nbytes)
    else:
        _launch("augment_resize_color_norm", "peclr_augment_resize_color_norm_ragged", *head, *out_args, stream, nbytes=nbytes)
    return out, srcs, crops


def augment_views_ragged(packed: torch.Tensor, geom: torch.Tensor, wins: torch.Tensor, params: torch.Tensor, out_hw, mean,
                         std, channels_last: bool = True, mirror: Optional[torch.Tensor] = None):
    """augment_views for images of different sizes: `packed` the 1-D uint8 HIP buffer of the images back to back,
    geom [B,5] / wins [V,B,4] the HOST int64 tables of include/peclr_hip.h (peclr_amd/augment.py builds them; they are
    uploaded here), params [V,B,16] float64 (HIP).  The same two launches.  mirror: as augment_views.
    Returns (out, crops, wins): crops the packed scratch, `ragged_window(crops, wins, v, i)` a window of it."""
    b, v, scratch = _ragged_args(packed, geom, wins, params)
    out, _, crops = _augment_ragged(packed, geom, wins, params, b, v, scratch, None, out_hw, mean, std, channels_last,
                                    _aug_mirror(mirror, b))
    return out, crops, wins


def augment_views_ragged_ext(packed: torch.Tensor, geom: torch.Tensor, wins: torch.Tensor, params: torch.Tensor,
                             ext: torch.Tensor, coefs: torch.Tensor, noise_table: torch.Tensor, n_table: int, noise_seed: int,
                             call: int, ops: int, out_hw, mean, std, channels_last: bool = True,
                             mirror: Optional[torch.Tensor] = None):
    """augment_views_ext for images of different sizes (arguments as augment_views_ragged and augment_views_ext; the
    blur lengths are geom's, per sample).  Stage 0's per-view sources come back as srcs [V, total bytes] in the packed
    layout (`ragged_image(srcs[v], geom, i)`).  mirror: as augment_views_ext.  Returns (out, srcs or None, crops, wins)."""
    b, v, scratch = _ragged_args(packed, geom, wins, params)
    aug = _AugExt(v, b, ext, coefs, noise_table, n_table, noise_seed, call, ops)
    return (*_augment_ragged(packed, geom, wins, params, b, v, scratch, aug, out_hw, mean, std, channels_last,
                             _aug_mirror(mirror, b)), wins)


# ---- the parameter side on the device (include/peclr_hip.h: peclr_augment_draw_views)
AUG_DRAW_ROTATE, AUG_DRAW_CROP, AUG_DRAW_RANDOM_CROP, AUG_DRAW_RESIZE, AUG_DRAW_COLOR_JITTER = 1, 2, 4, 8, 16
AUG_DRAW_RANGES, AUG_DRAW_SCALARS, AUG_DRAW_UNIFORMS = 14, 6, 8


def augment_draw_state(device):
    """The device state of one stream of draws: (call, counters) -- call int64 [1] (the uint64 call counter's storage), counters
    int32 [2] (cumulative empty windows, ticket).  Both zero; two fill launches, so allocate it OUTSIDE a graph capture."""
    return torch.zeros(1, device=device, dtype=torch.int64), torch.zeros(2, device=device, dtype=torch.int32)


def augment_draw_views(joints: torch.Tensor, image_hw, geom: Optional[torch.Tensor], mirror: Optional[torch.Tensor], flags: int,
                       ranges, seed: int, call: torch.Tensor, counters: torch.Tensor, n_views: int = 2,
                       return_uniforms: bool = False):
    """joints [B,21,3] float32 / float64 (HIP); image_hw = (H, W) of every sample, or None with geom, the DEVICE [B,5] int64 table
    of a mixed-size batch; mirror: None or int32 [B] (HIP), non-zero = a left hand; flags: AUG_DRAW_* bits; ranges: the 14
    doubles of include/peclr_hip.h; seed: the Philox key; call / counters: `augment_draw_state`, advanced by the launch.
    ONE launch, no host synchronisation.  Returns (params [V,B,16] float64, scalars [V,6,B] float64 -- angle, crop margin, h, s,
    a, b --, jitter [V,2,B] int64, uniforms [V,B,8] float64 or None)."""
    if (not isinstance(joints, torch.Tensor) or joints.dim() != 3 or tuple(joints.shape[1:]) != (21, 3)
            or joints.dtype not in (torch.float32, torch.float64)):
        raise PeclrHipError("augment_draw: joints must be a [B,21,3] float32 or float64 HIP tensor")
    b, dev = joints.shape[0], joints.device
    joints_ptr = _ptr(joints, joints.dtype, "augment_draw: joints")
    if geom is None:
        h, w = (int(x) for x in image_hw)
        geom_ptr = None
    else:
        if tuple(geom.shape) != (b, AUG_GEOM_INT64S):
            raise PeclrHipError(f"augment_draw: geom must be a device [{b},{AUG_GEOM_INT64S}] int64 tensor")
        h, w, geom_ptr = 0, 0, _ptr(geom, torch.int64, "augment_draw: geom")
    if len(ranges) != AUG_DRAW_RANGES:
        raise PeclrHipError(f"augment_draw: ranges must hold {AUG_DRAW_RANGES} numbers")
    if tuple(call.shape) != (1,) or tuple(counters.shape) != (2,):
        raise PeclrHipError("augment_draw: call must be int64 [1] and counters int32 [2] (augment_draw_state)")
    ranges_arr = (c_double * AUG_DRAW_RANGES)(*(float(x) for x in ranges))
    params = torch.empty((n_views, b, AUG_PARAM_DOUBLES), device=dev, dtype=torch.float64)
    scalars = torch.empty((n_views, AUG_DRAW_SCALARS, b), device=dev, dtype=torch.float64)
    jitter = torch.empty((n_views, 2, b), device=dev, dtype=torch.int64)
    uniforms = torch.empty((n_views, b, AUG_DRAW_UNIFORMS), device=dev, dtype=torch.float64) if return_uniforms else None
    _launch("augment_draw", "peclr_augment_draw_views", joints_ptr, DTYPE_F32 if joints.dtype == torch.float32 else DTYPE_F64, b,
            n_views, h, w, geom_ptr, _aug_mirror(mirror, b), int(flags), ctypes.cast(ranges_arr, c_void_p), int(seed) & (2 ** 64 - 1),
            _ptr(call, torch.int64, "augment_draw: call"), _ptr(counters, torch.int32, "augment_draw: counters"), params.data_ptr(),
            scalars.data_ptr(), jitter.data_ptr(), None if uniforms is None else uniforms.data_ptr(), _stream(),
            nbytes=n_views * b * 8 * (AUG_PARAM_DOUBLES + AUG_DRAW_SCALARS + 2) + b * 63 * joints.element_size())
    return params, scalars, jitter, uniforms


# ------------------------------------------------------------------ 2.5D hand-pose model at evaluation time (peclr_amd/pose.py)
POSE_MLP_TENSORS = 14
POSE_STATUS_NO_BBOX, POSE_STATUS_NAN = 1, 2


def _mat_ptr(t, b, dtype, what, broadcast=False):
    if t is None:
        return None
    ok = t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.dim() == 3 and tuple(t.shape[1:]) == (3, 3)
    if not ok or not (t.shape[0] == b or (broadcast and t.shape[0] == 1)):
        raise PeclrHipError(f"pose: {what} must be a contiguous [{b},3,3] {dtype} HIP tensor, got {t.dtype} {tuple(t.shape)} "
                            f"on {t.device} (peclr_amd has no CPU path)")
    return t.data_ptr()


def pose_crop(images: torch.Tensor, T: torch.Tensor, K: Optional[torch.Tensor], table: torch.Tensor, size: int):
    """images [B,H,W,3] uint8, T [B,3,3] float64 forward matrices, K [B,3,3] float64 or None, table [3,256] float32 ->
    (float32 [B,3,size,size] channels_last, float32 K' = T @ K [B,3,3] or None).  One launch."""
    if not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise PeclrHipError(f"pose_crop: images must be a contiguous [B,H,W,3] uint8 HIP tensor, got {images.dtype} "
                            f"{tuple(images.shape)} on {images.device} (peclr_amd has no CPU path)")
    b, h, w, _ = images.shape
    tp, kp = _mat_ptr(T, b, torch.float64, "T"), _mat_ptr(K, b, torch.float64, "K")
    if tuple(table.shape) != (3, 256):
        raise PeclrHipError("pose_crop: table must be [3,256] float32")
    out = torch.empty((b, 3, size, size), device=images.device, dtype=torch.float32, memory_format=torch.channels_last)
    k_out = torch.empty((b, 3, 3), device=images.device, dtype=torch.float32) if K is not None else None
    _launch("pose_crop", "peclr_pose_crop_u8", images.data_ptr(), b, h, w, tp, kp, _ptr(table, what="pose_crop table"), size,
            out.data_ptr(), k_out.data_ptr() if k_out is not None else None, _stream(), nbytes=b * h * w * 3 + b * size * size * 12)
    return out, k_out


def pose_head(feat: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, mlp, bn_eps, K: torch.Tensor, eps: float,
              T1: Optional[torch.Tensor] = None, size: int = 0, scale: Optional[torch.Tensor] = None,
              status: Optional[torch.Tensor] = None):
    """Pooled features [B,2048] -> (out64 [B,64], kp3d [B,21,3], T2 [B,3,3] float64 or None, fh [B,21,3] float64 or None,
    status [B] int32).  mlp: the 14 tensors of zroot_ref.zroot_ref in the order of include/peclr_hip.h; K [B or 1,3,3]
    float32.  Pass 1: T1 given (T2 out, status written); pass 2: scale [B] float64 given (fh out, NaN bit OR-ed into
    `status`, zeros when not given).  One launch."""
    if feat.dim() != 2:
        raise PeclrHipError(f"pose_head: features must be [B,2048], got {tuple(feat.shape)}")
    b, nf = feat.shape
    fp = _ptr(feat, what="pose_head features")
    kp = _mat_ptr(K, b, torch.float32, "K", broadcast=True)
    if len(mlp) != POSE_MLP_TENSORS:
        raise PeclrHipError(f"pose_head: {POSE_MLP_TENSORS} MLP tensors expected, got {len(mlp)}")
    mlp_arr = (c_void_p * POSE_MLP_TENSORS)(*[_ptr(t, what="pose_head MLP tensor") for t in mlp])
    dev = feat.device
    out64 = torch.empty((b, 64), device=dev, dtype=torch.float32)
    kp3d = torch.empty((b, 21, 3), device=dev, dtype=torch.float32)
    T2 = torch.empty((b, 3, 3), device=dev, dtype=torch.float64) if T1 is not None else None
    fh = torch.empty((b, 21, 3), device=dev, dtype=torch.float64) if scale is not None else None
    if status is None:
        status = torch.zeros((b,), device=dev, dtype=torch.int32)
    if scale is not None and (tuple(scale.shape) != (b,)):
        raise PeclrHipError(f"pose_head: scale must be [{b}] float64")
    if tuple(status.shape) != (b,):
        raise PeclrHipError(f"pose_head: status must be [{b}] int32")
    _launch("pose_head", "peclr_pose_head_f32", fp, b, nf, _ptr(fc_w, what="pose_head fc weight"), _ptr(fc_b, what="pose_head fc bias"),
            ctypes.cast(mlp_arr, c_void_p), float(bn_eps[0]), float(bn_eps[1]), kp,
            int(K.shape[0] != 1 or b == 1), float(eps), out64.data_ptr(), kp3d.data_ptr(),
            _mat_ptr(T1, b, torch.float64, "T1"), T2.data_ptr() if T2 is not None else None, int(size),
            _ptr(scale, torch.float64, "pose_head scale"), fh.data_ptr() if fh is not None else None,
            _ptr(status, torch.int32, "pose_head status"), _stream(), nbytes=4 * b * (nf + 64 + 63 + 64) + 4 * 64 * nf)
    return out64, kp3d, T2, fh, status


# ------------------------------------------------------------------ the same prediction for images of any size (peclr_amd/predict.py)
POSE_GEOM_COLS = 4   # a row of the device table: byte offset into the packed buffer, H, W, flip


def _pose_geom_ptr(geom, what):
    if (not geom.is_cuda or geom.dtype != torch.int64 or geom.dim() != 2 or geom.shape[1] != POSE_GEOM_COLS or geom.shape[0] < 1
            or not geom.is_contiguous()):
        raise PeclrHipError(f"{what}: geom must be a contiguous [B,{POSE_GEOM_COLS}] int64 HIP tensor (offset, H, W, flip), got "
                            f"{geom.dtype} {tuple(geom.shape)} on {geom.device} (peclr_amd has no CPU path)")
    return geom.data_ptr(), int(geom.shape[0])


def pose_crop_ragged(data: torch.Tensor, geom: torch.Tensor, T: torch.Tensor, K: Optional[torch.Tensor], table: torch.Tensor,
                     size: int):
    """`pose_crop` for a packed batch: data 1-D uint8 (the images back to back), geom [B,4] int64 ON THE DEVICE = (byte offset, H,
    W, flip) per sample -> (float32 [B,3,size,size] channels_last, float32 K' [B,3,3] or None).  flip: the crop of
    img[:, ::-1] and K' = T @ Kf (include/peclr_hip.h).  That every row lies inside `data` is the caller's to check (the table
    is on the device); the kernel reads nothing through a row that does not.  One launch."""
    if not data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1 or data.numel() < 1 or not data.is_contiguous():
        raise PeclrHipError(f"pose_crop_ragged: data must be a contiguous 1-D uint8 HIP tensor, got {data.dtype} "
                            f"{tuple(data.shape)} on {data.device} (peclr_amd has no CPU path)")
    gp, b = _pose_geom_ptr(geom, "pose_crop_ragged")
    tp, kp = _mat_ptr(T, b, torch.float64, "T"), _mat_ptr(K, b, torch.float64, "K")
    if tuple(table.shape) != (3, 256):
        raise PeclrHipError("pose_crop_ragged: table must be [3,256] float32")
    out = torch.empty((b, 3, size, size), device=data.device, dtype=torch.float32, memory_format=torch.channels_last)
    k_out = torch.empty((b, 3, 3), device=data.device, dtype=torch.float32) if K is not None else None
    _launch("pose_crop_ragged", "peclr_pose_crop_ragged_u8", data.data_ptr(), data.numel(), b, gp, tp, kp,
            _ptr(table, what="pose_crop_ragged table"), size, out.data_ptr(), k_out.data_ptr() if k_out is not None else None,
            _stream(), nbytes=data.numel() + b * size * size * 12)
    return out, k_out


def pose_unmap(out64: torch.Tensor, T2: torch.Tensor, geom: torch.Tensor, kp3d: torch.Tensor, fh: torch.Tensor):
    """The pass-2 outputs back into the sample's own frame: out64 [B,64] float32, T2 [B,3,3] float64, geom as `pose_crop_ragged`,
    kp3d [B,21,3] float32, fh [B,21,3] float64 -> (kp2d_src [B,21,2] float64 in source pixels, kp3d, xyz: copies with X negated
    for flip).  The inputs are not written.  One launch."""
    gp, b = _pose_geom_ptr(geom, "pose_unmap")
    for t, shape, what in ((out64, (b, 64), "out64"), (kp3d, (b, 21, 3), "kp3d"), (fh, (b, 21, 3), "fh")):
        if tuple(t.shape) != shape:
            raise PeclrHipError(f"pose_unmap: {what} must be {list(shape)}, got {tuple(t.shape)}")
    dev = out64.device
    kp2d_src = torch.empty((b, 21, 2), device=dev, dtype=torch.float64)
    kp3d_out = torch.empty((b, 21, 3), device=dev, dtype=torch.float32)
    xyz = torch.empty((b, 21, 3), device=dev, dtype=torch.float64)
    _launch("pose_unmap", "peclr_pose_unmap", _ptr(out64, what="pose_unmap out64"), _mat_ptr(T2, b, torch.float64, "T2"), gp,
            _ptr(kp3d, what="pose_unmap kp3d"), _ptr(fh, torch.float64, "pose_unmap fh"), b, kp2d_src.data_ptr(),
            kp3d_out.data_ptr(), xyz.data_ptr(), _stream(), nbytes=b * (64 * 4 + 72 + 63 * 24 + 42 * 8))
    return kp2d_src, kp3d_out, xyz


# ------------------------------------------------------------------ the same head in train mode, with its backward
POSE_TRAIN_MAX_BATCH = 1024
POSE_MLP_GRADS = 10   # zroot_ref.zroot_ref.{0.weight, 0.bias, 1.weight, 1.bias, 3.weight, 3.bias, 4.weight, 4.bias, 6.weight, 6.bias}
_POSE_MLP_GRAD_OF = (0, 1, 2, 3, 6, 7, 8, 9, 12, 13)    # their positions among the 14 MLP tensors


def pose_head_train_launches(backward: bool, want_d_feat: bool = True) -> int:
    return lib().peclr_pose_head_train_launches(int(bool(backward)), int(bool(want_d_feat)))


def _pose_train_args(what, feat, K, mlp):
    if feat.dim() != 2:
        raise PeclrHipError(f"{what}: features must be [B,2048], got {tuple(feat.shape)}")
    b, nf = feat.shape
    if b == 1:
        raise ValueError(f"{what}: expected more than 1 value per channel when training, got input size {tuple(feat.shape)}")
    if b > POSE_TRAIN_MAX_BATCH:
        raise PeclrHipError(f"{what}: at most {POSE_TRAIN_MAX_BATCH} samples per call, got {b}")
    if len(mlp) != POSE_MLP_TENSORS:
        raise PeclrHipError(f"{what}: {POSE_MLP_TENSORS} MLP tensors expected, got {len(mlp)}")
    fp = _ptr(feat, what=f"{what} features")
    kp = _mat_ptr(K, b, torch.float32, "K", broadcast=True)
    mlp_arr = (c_void_p * POSE_MLP_TENSORS)(*[_ptr(t, what=f"{what} MLP tensor") for t in mlp])
    return b, nf, fp, kp, int(K.shape[0] != 1), mlp_arr


def pose_head_train_fwd(feat: torch.Tensor, fc_w: torch.Tensor, fc_b: torch.Tensor, mlp, bn_eps, momentum, nbt, K: torch.Tensor,
                        eps: float):
    """The head in train mode: pooled features [B,2048], 2 <= B <= 1024 -> (out64 [B,64], kp3d [B,21,3], zroot [B], save: the
    float32 workspace `pose_head_train_bwd` reads).  mlp, K, eps as `pose_head`; the running statistics among `mlp` and the
    two int64 `nbt` (num_batches_tracked) are updated in place with `momentum` (one per BatchNorm1d).  Four launches, logged
    as one EVENT_LOG entry whose `kernel` field says so."""
    b, nf, fp, kp, per_sample, mlp_arr = _pose_train_args("pose_head_train_fwd", feat, K, mlp)
    dev = feat.device
    out64 = torch.empty((b, 64), device=dev, dtype=torch.float32)
    kp3d = torch.empty((b, 21, 3), device=dev, dtype=torch.float32)
    zroot = torch.empty((b,), device=dev, dtype=torch.float32)
    save = torch.empty((b * 639 + 1024,), device=dev, dtype=torch.float32)
    n = pose_head_train_launches(False)
    _launch("pose_head_train_fwd", "peclr_pose_head_train_fwd_f32", fp, b, nf, _ptr(fc_w, what="pose_head_train_fwd fc weight"),
            _ptr(fc_b, what="pose_head_train_fwd fc bias"), ctypes.cast(mlp_arr, c_void_p), float(bn_eps[0]), float(bn_eps[1]),
            float(momentum[0]), float(momentum[1]), _ptr(nbt[0], torch.int64, "pose_head_train_fwd num_batches_tracked"),
            _ptr(nbt[1], torch.int64, "pose_head_train_fwd num_batches_tracked"), kp, per_sample, float(eps), out64.data_ptr(),
            kp3d.data_ptr(), zroot.data_ptr(), save.data_ptr(), _stream(), nbytes=4 * b * (nf + 64 + 63 + 1 + 2 * 639) + 4 * 64 * nf,
            kernel=f"{n} launches")
    return out64, kp3d, zroot, save


def pose_head_train_bwd(feat: torch.Tensor, fc_w: torch.Tensor, mlp, K: torch.Tensor, out64: torch.Tensor, zroot: torch.Tensor,
                        save: torch.Tensor, g_kp3d: Optional[torch.Tensor] = None, g_out64: Optional[torch.Tensor] = None,
                        g_zroot: Optional[torch.Tensor] = None, want_d_feat: bool = True):
    """Backward of `pose_head_train_fwd` from its inputs and outputs: upstream gradients g_kp3d [B,21,3], g_out64 [B,64],
    g_zroot [B] (None = zeros) -> (d_feat [B,2048] or None, d_fc_w [64,2048], d_fc_b [64], the POSE_MLP_GRADS parameter
    gradients in state_dict order, d_out [B,64]: the gradient at the fc output).  Six launches, five without d_feat, logged
    as one EVENT_LOG entry whose `kernel` field says so."""
    b, nf, fp, kp, per_sample, mlp_arr = _pose_train_args("pose_head_train_bwd", feat, K, mlp)
    dev = feat.device
    if tuple(save.shape) != (b * 639 + 1024,):
        raise PeclrHipError(f"pose_head_train_bwd: save must be what pose_head_train_fwd returned for {b} samples")
    z = dict(device=dev, dtype=torch.float32)
    ws = torch.empty((b * 321,), **z)
    d_feat = torch.empty((b, nf), **z) if want_d_feat else None
    d_fc_w, d_fc_b = torch.empty((64, nf), **z), torch.empty((64,), **z)
    d_mlp = [torch.empty_like(mlp[i]) for i in _POSE_MLP_GRAD_OF]
    d_arr = (c_void_p * POSE_MLP_GRADS)(*[t.data_ptr() for t in d_mlp])
    n = pose_head_train_launches(True, want_d_feat)
    _launch("pose_head_train_bwd", "peclr_pose_head_train_bwd_f32", fp, b, nf, _ptr(fc_w, what="pose_head_train_bwd fc weight"),
            ctypes.cast(mlp_arr, c_void_p), kp, per_sample, _label_ptr(out64, (b, 64), "pose_head_train_bwd out64"),
            _label_ptr(zroot, (b,), "pose_head_train_bwd zroot"), _ptr(save, what="pose_head_train_bwd save"),
            _label_ptr(g_kp3d, (b, 21, 3), "pose_head_train_bwd g_kp3d"), _label_ptr(g_out64, (b, 64), "pose_head_train_bwd g_out64"),
            _label_ptr(g_zroot, (b,), "pose_head_train_bwd g_zroot"), ws.data_ptr(), None if d_feat is None else d_feat.data_ptr(),
            d_fc_w.data_ptr(), d_fc_b.data_ptr(), ctypes.cast(d_arr, c_void_p), _stream(),
            nbytes=4 * b * (nf * (2 if want_d_feat else 1) + 639 + 2 * 321 + 3 * 64) + 4 * 64 * nf * (3 if want_d_feat else 2),
            kernel=f"{n} launches")
    return d_feat, d_fc_w, d_fc_b, d_mlp, ws[b * 256:b * 320].view(b, 64)


# ------------------------------------------------------------------ scoring pose predictions (peclr_amd/pose_eval.py)
POSE_EVAL_DEGENERATE = 4
_EVAL_DTYPES = {torch.float32: DTYPE_F32, torch.float64: DTYPE_F64}


def pose_eval(pred: torch.Tensor, gt: torch.Tensor, dim: int = 3, procrustes: bool = True, thr: Optional[torch.Tensor] = None,
              counts: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, dist: Optional[torch.Tensor] = None,
              dist_aligned: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None, want_transform: bool = True):
    """pred, gt [B,21,3], both float32 or both float64 -> dict(dist [B,21], status [B] int32 and, with `procrustes`,
    dist_aligned [B,21], aligned [B,21,3], rot [B,3,3], scale [B], trans [B,3] (the last four only with `want_transform`)).
    thr [T] of the same dtype with counts [2,21,T] int64: PCK counts are ADDED to `counts`.  status is OR-ed into (zeros when
    not given).  Streaming: cursor = int32 [2] device tensor {rows filled, 0}, dist / dist_aligned / status then are
    [capacity, ...] buffers filled from row cursor[0], which the launch advances by B.  One launch."""
    for t, what in ((pred, "pred"), (gt, "gt")):
        if not t.is_cuda or t.dtype not in _EVAL_DTYPES or t.dim() != 3 or tuple(t.shape[1:]) != (21, 3) or not t.is_contiguous():
            raise PeclrHipError(f"pose_eval: {what} must be a contiguous [B,21,3] float32 / float64 HIP tensor, got {t.dtype} "
                                f"{tuple(t.shape)} on {t.device} (peclr_amd has no CPU path)")
    if pred.dtype != gt.dtype or pred.shape != gt.shape:
        raise PeclrHipError(f"pose_eval: pred {pred.dtype} {tuple(pred.shape)} and gt {gt.dtype} {tuple(gt.shape)} differ")
    if dim == 2 and procrustes:
        raise PeclrHipError("pose_eval: the Procrustes alignment needs dim = 3")
    b, dt, dev = pred.shape[0], pred.dtype, pred.device
    rows = b
    if cursor is not None:
        if dist is None or status is None or (procrustes and dist_aligned is None):
            raise PeclrHipError("pose_eval: the streaming form needs the dist / dist_aligned / status buffers")
        rows = dist.shape[0]
        _ptr(cursor, torch.int32, "pose_eval cursor")
        if tuple(cursor.shape) != (2,):
            raise PeclrHipError("pose_eval: cursor must be int32 [2]")
    if dist is None:
        dist = torch.empty((rows, 21), device=dev, dtype=dt)
    if status is None:
        status = torch.zeros((rows,), device=dev, dtype=torch.int32)
    if procrustes and dist_aligned is None:
        dist_aligned = torch.empty((rows, 21), device=dev, dtype=dt)
    for t, what in ((dist, "dist"), (dist_aligned, "dist_aligned")):
        if t is not None and tuple(t.shape) != (rows, 21):
            raise PeclrHipError(f"pose_eval: {what} must be [{rows},21], got {tuple(t.shape)}")
    if tuple(status.shape) != (rows,):
        raise PeclrHipError(f"pose_eval: status must be [{rows}] int32, got {tuple(status.shape)}")
    n_thr = 0
    if thr is not None:
        n_thr = thr.numel()
        if counts is None or tuple(counts.shape) != (2, 21, n_thr) or thr.dim() != 1:
            raise PeclrHipError(f"pose_eval: counts must be int64 [2,21,{n_thr}] next to thr [{n_thr}]")
    aligned = rot = scale = trans = None
    if procrustes and want_transform:
        aligned = torch.empty((b, 21, 3), device=dev, dtype=dt)
        rot = torch.empty((b, 3, 3), device=dev, dtype=dt)
        scale = torch.empty((b,), device=dev, dtype=dt)
        trans = torch.empty((b, 3), device=dev, dtype=dt)
    _launch("pose_eval", "peclr_pose_eval", pred.data_ptr(), gt.data_ptr(), b, _EVAL_DTYPES[dt], int(dim), _ptr(dist, dt, "pose_eval dist"),
            _ptr(aligned, dt), _ptr(rot, dt), _ptr(scale, dt), _ptr(trans, dt),
            _ptr(dist_aligned if procrustes else None, dt, "pose_eval dist_aligned"),
            _ptr(thr, dt, "pose_eval thresholds") if n_thr else None, n_thr,
            _ptr(counts, torch.int64, "pose_eval counts") if n_thr else None,
            _ptr(status, torch.int32, "pose_eval status"),
            cursor.data_ptr() if cursor is not None else None, rows if cursor is not None else 0, _stream(),
            nbytes=2 * pred.numel() * pred.element_size())
    return {"dist": dist, "dist_aligned": dist_aligned if procrustes else None, "aligned": aligned, "rot": rot, "scale": scale,
            "trans": trans, "status": status}


# ------------------------------------------------------------------ labels of a supervised sample (peclr_amd/supervised.py)
def _label_ptr(t, shape, what, dtype=torch.float32):
    """Pointer of a contiguous HIP tensor of exactly `shape` and `dtype` (None stays None)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise PeclrHipError(f"{what}: expected a HIP device tensor, got {where} (peclr_amd has no CPU path)")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise PeclrHipError(f"{what}: must be a contiguous {list(shape)} {dtype} tensor, got {t.dtype} {tuple(t.shape)}")
    return t.data_ptr()


def _label_batch(joints, what):
    if not isinstance(joints, torch.Tensor) or not joints.is_cuda:
        where = joints.device if isinstance(joints, torch.Tensor) else type(joints).__name__
        raise PeclrHipError(f"{what}: expected a HIP device tensor, got {where} (peclr_amd has no CPU path)")
    if joints.dim() != 3 or tuple(joints.shape[1:]) != (21, 3) or joints.shape[0] < 1:
        raise PeclrHipError(f"{what}: joints must be [B,21,3] with B >= 1, got {tuple(joints.shape)}")
    return joints.shape[0]


def joints3d_to_25d(K: torch.Tensor, joints3d: torch.Tensor, out: Optional[torch.Tensor] = None,
                    scale: Optional[torch.Tensor] = None):
    """K [B,3,3], joints3d [B,21,3] float32 -> (joints25d [B,21,3], scale [B]) float32: the batched convert_to_2_5D.  One launch."""
    b = _label_batch(joints3d, "joints3d_to_25d")
    kp, jp = _label_ptr(K, (b, 3, 3), "joints3d_to_25d K"), _label_ptr(joints3d, (b, 21, 3), "joints3d_to_25d joints3d")
    out = torch.empty((b, 21, 3), device=joints3d.device, dtype=torch.float32) if out is None else out
    scale = torch.empty((b,), device=joints3d.device, dtype=torch.float32) if scale is None else scale
    _launch("joints3d_to_25d", "peclr_joints3d_to_25d", kp, jp, b, _label_ptr(out, (b, 21, 3), "joints3d_to_25d out"),
            _label_ptr(scale, (b,), "joints3d_to_25d scale"), _stream(), nbytes=4 * b * (9 + 63 + 63 + 1))
    return out, scale


def joints25d_to_3d(joints25d: torch.Tensor, scale: torch.Tensor, K: torch.Tensor, z_root_calc: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, z_root: Optional[torch.Tensor] = None):
    """joints25d [B,21,3], scale [B], K [B,3,3] float32 (z_root_calc [B]: a root depth to use instead of the quadratic's) ->
    (joints3d [B,21,3], z_root [B]: the quadratic's root depth) float32: the batched convert_2_5D_to_3D.  One launch; `out`
    and `z_root` may be buffers the caller owns."""
    b = _label_batch(joints25d, "joints25d_to_3d")
    jp, sp = _label_ptr(joints25d, (b, 21, 3), "joints25d_to_3d joints25d"), _label_ptr(scale, (b,), "joints25d_to_3d scale")
    kp, zp = _label_ptr(K, (b, 3, 3), "joints25d_to_3d K"), _label_ptr(z_root_calc, (b,), "joints25d_to_3d z_root_calc")
    out = torch.empty((b, 21, 3), device=joints25d.device, dtype=torch.float32) if out is None else out
    z_root = torch.empty((b,), device=joints25d.device, dtype=torch.float32) if z_root is None else z_root
    _launch("joints25d_to_3d", "peclr_joints25d_to_3d", jp, sp, kp, zp, b, _label_ptr(out, (b, 21, 3), "joints25d_to_3d out"),
            _label_ptr(z_root, (b,), "joints25d_to_3d z_root"), _stream(), nbytes=4 * b * (63 + 1 + 9 + 63 + 1))
    return out, z_root


def supervised_labels(K: torch.Tensor, joints3d: torch.Tensor, T: torch.Tensor, use_palm: bool = False,
                      joints_raw: Optional[torch.Tensor] = None, mirror_w: Optional[torch.Tensor] = None):
    """K [B,3,3], joints3d [B,21,3] float32, T [B,3,3] float64 forward matrices, joints_raw [B,21,3] float32 or None -> dict of
    float32 tensors: joints, K (= fl32(T) @ K), scale, joints3D, joints3D_recreated, joints_raw, T.  One launch.
    mirror_w: None, or int32 [B] (HIP): 0 = the sample as stored, W > 0 = a left hand in an image of width W, labelled as the
    right hand of the mirrored image (K <- fl32(F K M), X of joints3d / joints_raw negated; include/peclr_hip.h)."""
    b = _label_batch(joints3d, "supervised_labels")
    kp, jp = _label_ptr(K, (b, 3, 3), "supervised_labels K"), _label_ptr(joints3d, (b, 21, 3), "supervised_labels joints3d")
    tp = _label_ptr(T, (b, 3, 3), "supervised_labels T", torch.float64)
    rp = _label_ptr(joints_raw, (b, 21, 3), "supervised_labels joints_raw")
    mp = _label_ptr(mirror_w, (b,), "supervised_labels mirror_w", torch.int32)
    z = dict(device=joints3d.device, dtype=torch.float32)
    out = {"joints": torch.empty((b, 21, 3), **z), "K": torch.empty((b, 3, 3), **z), "scale": torch.empty((b,), **z),
           "joints3D": torch.empty((b, 21, 3), **z), "joints3D_recreated": torch.empty((b, 21, 3), **z),
           "joints_raw": torch.empty((b, 21, 3), **z), "T": torch.empty((b, 3, 3), **z)}
    outs = tuple(out[k].data_ptr() for k in ("joints", "K", "scale", "joints3D", "joints3D_recreated", "joints_raw", "T"))
    nbytes = 4 * b * (9 + 63 + 18 + 4 * 63 + 1 + 18)
    if mirror_w is None:
        _launch("supervised_labels", "peclr_supervised_labels", kp, jp, tp, rp, b, int(bool(use_palm)), *outs, _stream(), nbytes=nbytes)
    else:
        _launch("supervised_labels", "peclr_supervised_labels_mirror", kp, jp, tp, rp, mp, b, int(bool(use_palm)), *outs, _stream(),
                nbytes=nbytes + 4 * b, kernel="supervised_labels_kernel<mirror>")
    return out


# ------------------------------------------------------------------ supervised pose losses (peclr_amd/pose_loss.py)
def pose_loss(pred: torch.Tensor, joints: Optional[torch.Tensor], joints3d: Optional[torch.Tensor], scale: torch.Tensor,
              K: Optional[torch.Tensor], joints_valid: Optional[torch.Tensor] = None, z_root_calc: Optional[torch.Tensor] = None):
    """pred, joints, joints3d [B,21,3], scale [B], K [B,3,3] float32 (joints_valid [B,21,1] or None for ones; z_root_calc [B]
    or None for the closed-form root depth) -> (losses [4] float32: loss_2d, loss_z, loss_z_unscaled, loss_3d; the float64
    workspaces `pose_loss_bwd` reads: g_l1, g_3d [B,21,3], g_zroot [B] or None, inv_valid [1]).  The forward launch pair.
    joints = None leaves the three L1 losses out (they are 0), joints3d = K = None the 3D loss."""
    b = _label_batch(pred, "pose_loss")
    if (joints is None and joints3d is None) or (joints3d is None) != (K is None) or (joints3d is None and z_root_calc is not None):
        raise PeclrHipError("pose_loss: needs joints, or joints3d with K (z_root_calc only with them)")
    pp, jp = _label_ptr(pred, (b, 21, 3), "pose_loss pred"), _label_ptr(joints, (b, 21, 3), "pose_loss joints")
    j3p, sp = _label_ptr(joints3d, (b, 21, 3), "pose_loss joints3d"), _label_ptr(scale, (b,), "pose_loss scale")
    kp, vp = _label_ptr(K, (b, 3, 3), "pose_loss K"), _label_ptr(joints_valid, (b, 21, 1), "pose_loss joints_valid")
    zp = _label_ptr(z_root_calc, (b,), "pose_loss z_root_calc")
    z = dict(device=pred.device, dtype=torch.float64)
    partials, g_l1, g_3d = torch.empty((b, 5), **z), torch.empty((b, 21, 3), **z), torch.empty((b, 21, 3), **z)
    g_zroot = torch.empty((b,), **z) if z_root_calc is not None else None
    inv_valid = torch.empty((1,), **z)
    losses = torch.empty((4,), device=pred.device, dtype=torch.float32)
    _launch("pose_loss", "peclr_pose_loss", pp, jp, j3p, sp, kp, vp, zp, b, partials.data_ptr(), g_l1.data_ptr(), g_3d.data_ptr(),
            None if g_zroot is None else g_zroot.data_ptr(), losses.data_ptr(), inv_valid.data_ptr(), _stream(),
            nbytes=4 * b * (3 * 63 + 1 + 9 + 21 + 1) + 8 * b * (2 * 5 + 2 * 63 + 1))
    return losses, g_l1, g_3d, g_zroot, inv_valid


def pose_loss_bwd(grad_losses: torch.Tensor, g_l1: torch.Tensor, g_3d: torch.Tensor, g_zroot: Optional[torch.Tensor],
                  scale: torch.Tensor, inv_valid: torch.Tensor, want_z_root: bool = False):
    """grad_losses [4] float32 on the device and what `pose_loss` left -> (grad_pred [B,21,3] float32, grad_z_root_calc [B]
    float32 or None).  One launch, no host read."""
    b = _label_batch(g_l1, "pose_loss_bwd")
    up = _label_ptr(grad_losses, (4,), "pose_loss_bwd grad_losses")
    lp = _label_ptr(g_l1, (b, 21, 3), "pose_loss_bwd g_l1", torch.float64)
    tp = _label_ptr(g_3d, (b, 21, 3), "pose_loss_bwd g_3d", torch.float64)
    zp = _label_ptr(g_zroot, (b,), "pose_loss_bwd g_zroot", torch.float64)
    sp = _label_ptr(scale, (b,), "pose_loss_bwd scale")
    ip = _label_ptr(inv_valid, (1,), "pose_loss_bwd inv_valid", torch.float64)
    if want_z_root and g_zroot is None:
        raise PeclrHipError("pose_loss_bwd: the gradient of z_root_calc needs the forward's g_zroot")
    grad_pred = torch.empty((b, 21, 3), device=g_l1.device, dtype=torch.float32)
    grad_z = torch.empty((b,), device=g_l1.device, dtype=torch.float32) if want_z_root else None
    _launch("pose_loss_bwd", "peclr_pose_loss_bwd", up, lp, tp, zp, sp, ip, b, grad_pred.data_ptr(),
            None if grad_z is None else grad_z.data_ptr(), _stream(), nbytes=4 * b * (63 + 2) + 8 * b * (2 * 63 + 1))
    return grad_pred, grad_z


# ------------------------------------------------------------------ metrics of a supervised step (peclr_amd/pose_metrics.py)
POSE_METRICS_MAX_BATCH = 1024


def pose_step_metrics(pred: torch.Tensor, truth: torch.Tensor, pred2: Optional[torch.Tensor] = None,
                      truth2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pred, truth [B,21,3] float32, 1 <= B <= 1024 (pred2, truth2: an optional second pair of the same shape) -> out [4]
    float32: the mean and torch's lower median of the per-joint Euclidean distances of the first pair, then of the second
    (out[2:4] is left as it is without one).  `workspace`: int32 [2 * 21 * B] (half without the second pair), from torch's
    allocator when not given.  One launch, logged as one EVENT_LOG entry whose `kernel` field says so; no host read."""
    b = _label_batch(pred, "pose_step_metrics")
    if b > POSE_METRICS_MAX_BATCH:
        raise PeclrHipError(f"pose_step_metrics: at most {POSE_METRICS_MAX_BATCH} samples per call, got {b}")
    if (pred2 is None) != (truth2 is None):
        raise PeclrHipError("pose_step_metrics: the second pair needs both its prediction and its truth")
    pairs = 1 if pred2 is None else 2
    pp, tp = _label_ptr(pred, (b, 21, 3), "pose_step_metrics pred"), _label_ptr(truth, (b, 21, 3), "pose_step_metrics truth")
    p2, t2 = _label_ptr(pred2, (b, 21, 3), "pose_step_metrics pred2"), _label_ptr(truth2, (b, 21, 3), "pose_step_metrics truth2")
    out = torch.empty((4,), device=pred.device, dtype=torch.float32) if out is None else out
    if workspace is None:
        workspace = torch.empty((pairs * 21 * b,), device=pred.device, dtype=torch.int32)
    elif not workspace.is_cuda or workspace.dtype != torch.int32 or not workspace.is_contiguous() or workspace.numel() < pairs * 21 * b:
        raise PeclrHipError(f"pose_step_metrics workspace: a contiguous int32 HIP tensor of at least {pairs * 21 * b} elements")
    _launch("pose_step_metrics", "peclr_pose_step_metrics_f32", pp, tp, p2, t2, b, workspace.data_ptr(),
            _label_ptr(out, (4,), "pose_step_metrics out"), _stream(), nbytes=pairs * 21 * b * (6 * 4 + 5 * 2 * 4) + 8 * pairs,
            kernel="1 launch")
    return out
