"""ctypes binding of liblci.so (the C-ABI declared in include/lci.h).

There is no fallback: if the library is missing, or a tensor is not on a ROCm device, the op raises.
`import torch` happens first so that liblci's libamdhip64.so.7 dependency binds to the HIP runtime torch
already loaded (one runtime, one set of streams).
"""
from __future__ import annotations

import ctypes
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "liblci.so")
LIB_PATH = os.environ.get("LCI_LIB_PATH", DEFAULT_LIB)   # override: kernel-variant A/B runs (no staleness check)
ABI_VERSION = 39  # include/lci.h LCI_ABI_VERSION

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_L = ctypes.c_longlong
_D = ctypes.c_double

# name -> argtypes (all return int status)
SIGNATURES = {
    "lci_attn_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_attn_fwd_variant": [_I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_attn_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_attn_bwd_stage": [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_attn_bwd_variant": [_I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_attn_gen_fwd": [_I, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_attn_gen_bwd": [_I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "lci_patch_embed_fwd": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P],
    "lci_patch_embed_bwd": [_P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P],
    "lci_selective_scan_fwd": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
    "lci_selective_scan_bwd": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I,
                               _I, _P, _P, _P, _P, _P],
    "lci_window_bias": [_P, _P, _P, _P, _P, _P],
    "lci_window_attn_fwd": [_P, _P, _P, _I, _P, _P, _P, _F, _P],
    "lci_window_attn_bwd": [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _P],
    "lci_window_index_map": [_P, _P, _P, _P, _P, _P],
    "lci_fft_twiddles": [_P, _I, _P],
    "lci_fftconv_spectrum": [_P, _P, _P, _P, _P, _I, _I, _P],
    "lci_fftconv_fwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lci_fftconv_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lci_hyena_pre_fwd": [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lci_hyena_post_fwd": [_I, _P, _P, _P, _I, _I, _I, _P],
    "lci_hyena_post_bwd": [_I, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "lci_hyena_pre_bwd": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "lci_dwconv_silu_fwd": [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_conv3_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_conv3_fwd_split": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_conv3_pack_weight": [_P, _P, _I, _I, _I, _I, _I, _P],
    "lci_convup_interleave": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_conv3_wgrad": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_inorm_reduce": [_P, _P, _P, _P, _L, _I, _I, _I, _F, _P],
    "lci_inorm_finalize": [_P, _P, _L, _I, _I, _I, _F, _P],
    "lci_bn_relu_fwd": [_P, _P, _P, _P, _P, _L, _I, _P],
    "lci_bn_relu_bwd_reduce": [_P, _P, _I, _P, _P, _P, _P, _L, _I, _P],
    "lci_bn_relu_bwd_apply": [_P, _P, _I, _P, _P, _P, _P, _P, _L, _I, _P],
    "lci_inorm_apply": [_P, _P, _P, _P, _P, _L, _I, _I, _I, _F, _P],
    "lci_inorm_apply_res": [_P, _P, _P, _P, _P, _L, _I, _I, _F, _P],
    "lci_layernorm_fwd": [_P, _P, _P, _P, _I, _P, _P, _L, _I, _F, _P],
    "lci_layernorm_add_fwd": [_P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _L, _I, _F, _P],
    "lci_layernorm_bwd": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P],
    "lci_dwconv_silu_bwd": [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_linear_wgrad": [_P, _L, _P, _L, _L, _I, _I, _P, _P, _P],
    "lci_gemm_bt": [_P, _L, _P, _P, _P, _L, _L, _I, _I, _P],
    "lci_gemm_bt_acc": [_P, _L, _P, _P, _L, _L, _I, _I, _P],
    "lci_gemm_bt_small": [_P, _L, _P, _P, _P, _L, _L, _I, _I, _P],
    "lci_gemm_bt_small_acc": [_P, _L, _P, _P, _L, _L, _I, _I, _P],
    "lci_linear_small_fwd": [_P, _L, _P, _P, _P, _L, _I, _I, _P],
    "lci_linear_small_bwd": [_P, _L, _P, _P, _P, _P, _L, _I, _I, _P],
    "lci_gelu_fwd": [_P, _P, _L, _P],
    "lci_gelu_bwd": [_P, _P, _P, _L, _P],
    "lci_upsample2x_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "lci_upsample2x_bwd": [_P, _P, _I, _I, _I, _I, _P],
    "lci_upsample2x_nhwc_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "lci_upsample2x_nhwc_bwd": [_P, _P, _I, _I, _I, _I, _P],
    "lci_upsample3d_cl_fwd": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_resample1d_adj": [_P, _I, _P, _L, _I, _I, _L, _P],
    "lci_resample1d_adj_ac": [_P, _I, _P, _L, _I, _I, _L, _I, _P],
    "lci_resample_cl_fwd": [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "lci_direct_conv_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "lci_window_gather": [_P, _P, _I, _P, _I, _P],
    "lci_mamba_proj_dims": [_I, _I, _I, _P],
    "lci_mamba_proj_fwd": [_P, _L, _P, _P, _P, _P, _L, _P, _P, _I, _L, _I, _I, _I, _P],
    "lci_mamba_proj_bwd": [_P, _L, _P, _P, _P, _P, _L, _P, _L, _P, _I, _L, _I, _I, _I, _P],
    "lci_direct_conv_dk": [_P, _P, _P, _I, _I, _I, _P],
    "lci_hyena_filter_prep": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P],
    "lci_hyena_filter_fwd": [_P, _P, _P, _P, _I, _I, _F, _P, _P],
    "lci_adam_step": [_P, _P, _P, _P, _P, _P, _I, _D, _D, _D, _D, _D, _I, _I, _P],
    "lci_adam_step_ex": [_P, _P, _P, _P, _P, _P, _I, _D, _D, _D, _D, _D, _I, _I, _P, _P, _P, _P],
    "lci_onecycle_eval": [_P, _I, _P, _P, _P],
    "lci_grad_sumsq": [_P, _P, _I, _P, _P],
    "lci_grad_clip_coef": [_P, _L, _D, _P, _P],
    "lci_hyena_filter_bwd": [_P, _P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "lci_enhance_loss": [_P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "lci_enhance_metrics": [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "lci_seg_f1": [_P, _I, _P, _P, _P, _P, _I, _I, _L, _P],
    "lci_class_append": [_P, _I, _P, _P, _P, _P, _L, _I, _I, _P],
    "lci_class_score": [_P, _P, _P, _P, _L, _I, _P],
    "lci_class_metrics": [_P, _I, _P, _P, _P, _P, _I, _I, _P],
}

_lib = None


class LciError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load liblci.so and bind every symbol in SIGNATURES (raises if missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise LciError(f"{path} not found: build it with `python -m long_context_biomedical_imaging_amd.build_lib`"
                       " (the HIP path has no CPU fallback)")
    lib = ctypes.CDLL(path)
    lib.lci_last_error.restype = ctypes.c_char_p
    lib.lci_abi_version.restype = ctypes.c_int
    lib.lci_build_hash.restype = ctypes.c_char_p
    if lib.lci_abi_version() != ABI_VERSION:
        raise LciError(f"{path}: ABI version {lib.lci_abi_version()} != {ABI_VERSION} expected by this binding; "
                       "rebuild with `python -m long_context_biomedical_imaging_amd.build_lib`")
    if path == DEFAULT_LIB and os.path.isdir(os.path.join(HERE, "csrc")):
        from . import build_lib
        want, got = build_lib.source_hash(), lib.lci_build_hash().decode()
        if want != got:
            raise LciError(f"{path} is stale: built from sources {got}, the sources beside it hash to {want}; "
                           "rebuild with `python -m long_context_biomedical_imaging_amd.build_lib`")
    lib.lci_window_dS_elems.restype = ctypes.c_longlong
    lib.lci_window_dS_elems.argtypes = [_P]
    lib.lci_window_pad_ws_elems.restype = ctypes.c_longlong
    lib.lci_window_pad_ws_elems.argtypes = [_P]
    lib.lci_window_bwd_needs_plain.restype = ctypes.c_int
    lib.lci_window_bwd_needs_plain.argtypes = [_P]
    lib.lci_selective_scan_bwd_plain_dbc.restype = ctypes.c_int
    lib.lci_selective_scan_bwd_plain_dbc.argtypes = [_I, _I, _I]
    lib.lci_window_bias_elems.restype = ctypes.c_longlong
    lib.lci_window_bias_elems.argtypes = [_P, _I]
    lib.lci_attn_bwd_ws_bytes.restype = ctypes.c_longlong
    lib.lci_attn_bwd_ws_bytes.argtypes = [_I, _I, _I]
    lib.lci_attn_fwd_ws_bytes.restype = ctypes.c_longlong
    lib.lci_attn_fwd_ws_bytes.argtypes = [_I, _I, _I]
    lib.lci_attn_fwd_pick.restype = ctypes.c_int
    lib.lci_attn_fwd_pick.argtypes = [_I, _I, _I, _I]
    lib.lci_attn_bwd_dq_pick.restype = ctypes.c_int
    lib.lci_attn_bwd_dq_pick.argtypes = [_I, _I, _I, _I]
    lib.lci_conv3_fwd_splits.restype = ctypes.c_int
    lib.lci_conv3_fwd_splits.argtypes = [ctypes.c_longlong, _I, _I, _I]
    lib.lci_conv3_wgrad_splits.restype = ctypes.c_longlong
    lib.lci_conv3_wgrad_splits.argtypes = [ctypes.c_longlong, _I, _I, _I]
    lib.lci_linear_wgrad_splits.restype = ctypes.c_longlong
    lib.lci_linear_wgrad_splits.argtypes = [ctypes.c_longlong, _I, _I]
    lib.lci_gemm_bt_supported.restype = ctypes.c_int
    lib.lci_gemm_bt_supported.argtypes = [_I, _I]
    lib.lci_gemm_bt_small_supported.restype = ctypes.c_int
    lib.lci_gemm_bt_small_supported.argtypes = [_I, _I]
    lib.lci_linear_small_threads.restype = ctypes.c_int
    lib.lci_linear_small_threads.argtypes = []
    lib.lci_inorm_chunks.restype = ctypes.c_int
    lib.lci_inorm_chunks.argtypes = [ctypes.c_longlong, _I]
    lib.lci_layernorm_bwd_blocks.restype = ctypes.c_int
    lib.lci_layernorm_bwd_blocks.argtypes = [ctypes.c_longlong]
    lib.lci_hyena_filter_img_elems.restype = ctypes.c_longlong
    lib.lci_hyena_filter_img_elems.argtypes = []
    lib.lci_hyena_filter_partials.restype = ctypes.c_longlong
    lib.lci_hyena_filter_partials.argtypes = [_I, _I]
    lib.lci_fft_size.restype = ctypes.c_longlong
    lib.lci_fft_size.argtypes = [_I]
    lib.lci_dwconv_silu_bwd_part_rows.restype = ctypes.c_longlong
    lib.lci_dwconv_silu_bwd_part_rows.argtypes = [_I, _I]
    lib.lci_adam_max_tensors.restype = ctypes.c_int
    lib.lci_adam_max_tensors.argtypes = []
    lib.lci_grad_sumsq_parts.restype = ctypes.c_longlong
    lib.lci_grad_sumsq_parts.argtypes = [_P, _I]
    lib.lci_direct_conv_max_len.restype = ctypes.c_int
    lib.lci_direct_conv_max_len.argtypes = []
    lib.lci_direct_conv_dk_splits.restype = ctypes.c_int
    lib.lci_direct_conv_dk_splits.argtypes = [_I, _I, _I]
    lib.lci_enhance_loss_ws_bytes.restype = ctypes.c_longlong
    lib.lci_enhance_loss_ws_bytes.argtypes = [_I, _I, _I, _I]
    lib.lci_enhance_metrics_ws_bytes.restype = ctypes.c_longlong
    lib.lci_enhance_metrics_ws_bytes.argtypes = [_I, _I, _I, _I, _I]
    lib.lci_seg_f1_ws_bytes.restype = ctypes.c_longlong
    lib.lci_seg_f1_ws_bytes.argtypes = [_I, _I, _L]
    lib.lci_ssim_tile.restype = ctypes.c_int
    lib.lci_ssim_tile.argtypes = [_I]
    lib.lci_class_tile.restype = ctypes.c_int
    lib.lci_class_tile.argtypes = [_I]
    lib.lci_class_metrics_ws_bytes.restype = ctypes.c_longlong
    lib.lci_class_metrics_ws_bytes.argtypes = [_I, _I]
    for name, argt in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = ctypes.c_int
    _lib = lib
    return lib


def call(name: str, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise LciError(f"{name} failed (rc={rc}): {lib.lci_last_error().decode()}")


def plain_tensors():
    """Context for building a cached constant tensor. Under torch.inference_mode() (trainer.EvalStep) it leaves that
    mode, so the tensor is a plain one that a later training step may save for its backward; anywhere else it does
    nothing at all (torch.inference_mode(False) would also switch grad mode on inside a no_grad region)."""
    import contextlib
    return torch.inference_mode(False) if torch.is_inference_mode_enabled() else contextlib.nullcontext()


def stream_of(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def require_gpu(*ts: torch.Tensor):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise LciError("liblci ops run on the GPU only (tensor on %s); there is no CPU path" % t.device)
        if not t.is_contiguous():
            raise LciError("liblci ops need contiguous tensors")
