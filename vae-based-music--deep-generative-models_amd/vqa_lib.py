"""ctypes binding of libvqa.so (the C-ABI in include/vqa.h).

There is no CPU or PyTorch fallback: if libvqa.so is missing, `lib()` raises ImportError, and every op
raises VQAError with the library's own message when a call fails. Tensors are passed as raw device
pointers on torch's current HIP stream (so the calls are captured by torch.cuda.graph).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# VQA_LIB_PATH: another build of the same sources (A/B and diagnosis tools only; the product loads libvqa.so)
LIB_PATH = os.environ.get("VQA_LIB_PATH") or os.path.join(HERE, "libvqa.so")

F32, BF16 = 0, 1
PRE_RELU, ADD_RESIDUAL, POST_MASK, X_F32, Y_F32 = 1, 2, 4, 8, 16

ABI_VERSION = 2  # include/vqa.h VQA_ABI_VERSION this binding is written against

EXPORTED = [
    "vqa_get_last_error", "vqa_version", "vqa_abi_version", "vqa_same_pad_left", "vqa_same_out_len",
    "vqa_conv1d_fwd", "vqa_conv1d_bwd_data", "vqa_conv1d_bwd_weight", "vqa_conv1d_bwd_weight_workspace",
    "vqa_conv1d_transpose_fwd", "vqa_conv1d_transpose_bwd_data", "vqa_conv1d_transpose_bwd_weight",
    "vqa_conv1d_transpose_bwd_weight_workspace",
    "vqa_vq_sqnorm", "vqa_vq_argmin", "vqa_vq_quantize", "vqa_vq_quantize_workspace", "vqa_vq_backward",
    "vqa_vq_reset_rows", "vqa_vq_ema_apply", "vqa_vq_ema_apply_derived", "vqa_reset_perm_index",
    "vqa_mse_loss", "vqa_mse_loss_workspace", "vqa_adam_keras", "vqa_lr_schedule", "vqa_counter_add",
    "vqa_conv1d_bwd_weight_partials", "vqa_conv1d_transpose_bwd_weight_partials", "vqa_reduce_partials",
    "vqa_conv1d_bwd_data_weight", "vqa_conv1d_bwd_data_weight_workspace", "vqa_conv1d_route",
    "vqa_spectral_loss", "vqa_spectral_loss_workspace", "vqa_stft_magnitude",
    "vqa_vq_argmin_split", "vqa_vq_split_bf16x3",
    "vqa_resblock_supported", "vqa_resblock_fwd", "vqa_resblock_bwd", "vqa_resblock_bwd_workspace",
    "vqa_resblock_plan",
    "vqa_spectral_target_workspace", "vqa_spectral_target", "vqa_spectral_loss_target_workspace",
    "vqa_spectral_loss_target", "vqa_dtail_supported", "vqa_dtail_workspace", "vqa_dtail_fwd", "vqa_dtail_bwd",
    "vqa_step_metrics", "vqa_synthetic_batch",
    "vqa_embedding_fwd", "vqa_embedding_bwd", "vqa_embedding_bwd_workspace", "vqa_layernorm_fwd",
    "vqa_layernorm_bwd", "vqa_layernorm_bwd_workspace",
    "vqa_seqlin_fwd", "vqa_seqlin_prep", "vqa_seqlin_fwd_prepped", "vqa_seqlin_fwd_ln_prepped", "vqa_seqlin_wgrad_workspace", "vqa_seqlin_wgrad", "vqa_prior_embed_fwd", "vqa_colsum",
    "vqa_seqlin_route", "vqa_seqlin_wgrad_plan", "vqa_head_bwd_plan",
    "vqa_axpy", "vqa_dropout", "vqa_scale_f32", "vqa_tf_mix", "vqa_attn_fwd", "vqa_attn_bwd", "vqa_head_wt",
    "vqa_head_fwd", "vqa_head_bwd_workspace", "vqa_head_bwd", "vqa_rowsum_workspace", "vqa_rowsum", "vqa_prior_decode_cache_bytes",
    "vqa_prior_decode", "vqa_prior_decode_primed", "vqa_prior_decode_filtered", "vqa_prior_decode_scored",
    "vqa_corpus_steps_per_epoch", "vqa_corpus_batch", "vqa_pcm_encode", "vqa_pcm_splice", "vqa_code_batch",
    "vqa_resample", "vqa_resample_route",
    "vqa_attn_weights_elems", "vqa_attn_weights",
    "vqa_grad_norm", "vqa_grad_norm_workspace", "vqa_adam_keras_clipped",
    "vqa_adam_keras_ema", "vqa_adam_keras_clipped_ema", "vqa_swap_f32",
    "vqa_grad_finite", "vqa_adam_keras_guarded", "vqa_counter_add_if", "vqa_step_metrics_if",
    "vqa_vq_ema_apply_guarded",
]


class VQAError(RuntimeError):
    pass


class PartialsDesc(ctypes.Structure):
    """vqa_partials_desc (include/vqa.h)."""
    _fields_ = [("partials", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("db", ctypes.c_void_p),
                ("nparts", ctypes.c_int), ("n", ctypes.c_int), ("n_w", ctypes.c_int), ("reserved", ctypes.c_int)]


_P, _I, _L, _S, _F, _U = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float,
                          ctypes.c_uint64)
_CONV = [_I] * 11  # B T_in T_out C_in C_out K stride dilation pad flags dtype
_CONVT = [_I] * 10  # B T_in T_out C_in C_out K stride pad flags dtype

_SIGS = {
    "vqa_get_last_error": (ctypes.c_char_p, []),
    "vqa_version": (ctypes.c_char_p, []),
    "vqa_abi_version": (_I, []),
    "vqa_same_pad_left": (_I, [_I, _I, _I, _I]),
    "vqa_same_out_len": (_I, [_I, _I]),
    "vqa_conv1d_fwd": (_I, [_P, _P, _P, _P, _P] + _CONV + [_P]),
    "vqa_conv1d_bwd_data": (_I, [_P, _P, _P, _P, _P] + _CONV + [_P]),
    "vqa_conv1d_bwd_weight": (_I, [_P, _P, _P, _P] + _CONV + [_P, _S, _P]),
    "vqa_conv1d_bwd_weight_workspace": (_S, _CONV),
    "vqa_conv1d_transpose_fwd": (_I, [_P, _P, _P, _P, _P] + _CONVT + [_P]),
    "vqa_conv1d_transpose_bwd_data": (_I, [_P, _P, _P, _P, _P] + _CONVT + [_P]),
    "vqa_conv1d_transpose_bwd_weight": (_I, [_P, _P, _P, _P] + _CONVT + [_P, _S, _P]),
    "vqa_conv1d_transpose_bwd_weight_workspace": (_S, _CONVT),
    "vqa_vq_sqnorm": (_I, [_P, _P, _I, _I, _P]),
    "vqa_vq_argmin": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _P]),
    "vqa_vq_quantize": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _F, _I, _P, _S, _P]),
    "vqa_vq_quantize_workspace": (_S, [_L, _I, _I, _I]),
    "vqa_vq_backward": (_I, [_P, _P, _P, _P, _P, _F, _L, _I, _I, _P]),
    "vqa_vq_reset_rows": (_I, [_P, _P, _L, _L, _L, _I, _I, _U, _P, _I, _I, _P]),
    "vqa_vq_ema_apply": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _P, _I, _I, _P]),
    "vqa_vq_ema_apply_derived": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _P, _P, _P, _I, _I, _P]),
    "vqa_reset_perm_index": (_L, [_U, _L, _I, _L, _L]),
    "vqa_mse_loss": (_I, [_P, _P, _P, _P, _P, _L, _P, _S, _P]),
    "vqa_mse_loss_workspace": (_S, [_L]),
    "vqa_adam_keras": (_I, [_P, _P, _P, _P, _L, _P, _F, _P, _F, _F, _F, _F, _P]),
    "vqa_grad_norm": (_I, [_P, _L, _P, _P, _I, _F, _I, _F, _F, _F, _P, _P, _P, _S, _P]),
    "vqa_grad_norm_workspace": (_S, [_L, _I]),
    "vqa_adam_keras_clipped": (_I, [_P, _P, _P, _P, _L, _P, _F, _P, _F, _F, _F, _F, _P, _P, _I, _I, _F, _F, _F, _P,
                                    _P, _P]),
    "vqa_adam_keras_ema": (_I, [_P, _P, _P, _P, _L, _P, _F, _P, _F, _F, _F, _F, _P, _F, _L, _I, _P]),
    "vqa_adam_keras_clipped_ema": (_I, [_P, _P, _P, _P, _L, _P, _F, _P, _F, _F, _F, _F, _P, _P, _I, _I, _F, _F, _F, _P,
                                        _P, _P, _F, _L, _I, _P]),
    "vqa_swap_f32": (_I, [_P, _P, _L, _P]),
    "vqa_grad_finite": (_I, [_P, _L, _P, _P]),
    "vqa_adam_keras_guarded": (_I, [_P, _P, _P, _P, _L, _P, _F, _P, _F, _F, _F, _F, _P, _P, _I, _I, _F, _F, _F, _P,
                                    _P, _P, _F, _L, _I, _P, _P, _P]),
    "vqa_counter_add_if": (_I, [_P, _L, _P, _P]),
    "vqa_step_metrics_if": (_I, [_P, _P, _P, _I, _F, _P, _P]),
    "vqa_vq_ema_apply_guarded": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _P, _P, _P, _P, _I, _I, _P, _P]),
    "vqa_lr_schedule": (_I, [_P, _P, _I, _F, _F, _F, _F, _P]),
    "vqa_counter_add": (_I, [_P, _L, _P]),
    "vqa_step_metrics": (_I, [_P, _P, _P, _I, _F, _P]),
    "vqa_synthetic_batch": (_I, [_P, _I, _L, _U, _I, _F, _P]),
    "vqa_embedding_fwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P]),
    "vqa_embedding_bwd": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _S, _P]),
    "vqa_embedding_bwd_workspace": (_S, [_L, _I, _I]),
    "vqa_layernorm_fwd": (_I, [_P, _P, _P, _P, _L, _I, _F, _I, _P]),
    "vqa_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _F, _I, _P, _S, _P, _P]),
    "vqa_layernorm_bwd_workspace": (_S, [_L, _I]),
    "vqa_conv1d_bwd_weight_partials": (_I, [_P, _P, _P, _P] + _CONV + [_P, _S, _P, _P]),
    "vqa_conv1d_transpose_bwd_weight_partials": (_I, [_P, _P, _P, _P] + _CONVT + [_P, _S, _P, _P]),
    "vqa_reduce_partials": (_I, [_P, _I, _P]),
    "vqa_conv1d_bwd_data_weight": (_I, [_P, _P, _P, _P, _P, _P, _P] + _CONV + [_P, _S, _P, _P]),
    "vqa_conv1d_bwd_data_weight_workspace": (_S, _CONV),
    "vqa_conv1d_route": (_I, [_I] + _CONV + [_P]),
    "vqa_spectral_loss": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P, _S, _P]),
    "vqa_spectral_loss_workspace": (_S, [_I, _I, _P, _P, _P, _I, _I]),
    "vqa_stft_magnitude": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "vqa_vq_argmin_split": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P]),
    "vqa_vq_split_bf16x3": (_I, [_P, _P, _I, _I, _P]),
    "vqa_resblock_supported": (_I, [_I, _I, _I]),
    "vqa_resblock_fwd": (_I, [_P] * 7 + [_I] * 5 + [_P]),
    "vqa_resblock_bwd": (_I, [_P] * 11 + [_I] * 5 + [_P, _S, _P, _P]),
    "vqa_resblock_bwd_workspace": (_S, [_I] * 5),
    "vqa_resblock_plan": (_I, [_I] * 6 + [_P]),
    "vqa_dtail_supported": (_I, [_I] * 7),
    "vqa_dtail_workspace": (_S, [_I] * 5),
    "vqa_dtail_fwd": (_I, [_P] * 6 + [_I] * 5 + [_P, _S, _P]),
    "vqa_dtail_bwd": (_I, [_P] * 11 + [_I] * 5 + [_P, _S, _P]),
    "vqa_spectral_target_workspace": (_S, [_I, _I, _P, _P, _P, _I]),
    "vqa_spectral_target": (_I, [_P, _P, _S, _I, _I, _P, _P, _P, _I, _P]),
    "vqa_spectral_loss_target_workspace": (_S, [_I, _I, _P, _P, _P, _I, _I]),
    "vqa_spectral_loss_target": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _P, _S, _P]),
    # factorized-attention prior
    "vqa_seqlin_fwd": (_I, [_P, _L, _P, _P, _P, _L, _P, _L] + [_I] * 9 + [_P]),
    "vqa_seqlin_prep": (_I, [_P, _I, _I, _P]),
    "vqa_seqlin_fwd_prepped": (_I, [_P, _L, _P, _P, _P, _L, _P, _L] + [_I] * 8 + [_P]),
    "vqa_seqlin_fwd_ln_prepped": (_I, [_P, _L, _P, _P, ctypes.c_float, _P, _P, _P, _L, _P, _L] + [_I] * 7 + [_P]),
    "vqa_seqlin_route": (_I, [_P, _L, _P, _P, _P, _P, _L, _P, _L] + [_I] * 10 + [_P]),
    "vqa_seqlin_wgrad_plan": (_I, [_I] * 6 + [_P, _P, _P]),
    "vqa_head_bwd_plan": (_I, [_L, _I, _I, _P, _P]),
    "vqa_seqlin_wgrad_workspace": (_S, [_I] * 5),
    "vqa_seqlin_wgrad": (_I, [_P, _L, _P, _L, _P, _P] + [_I] * 6 + [_P, _S, _P, _P]),
    "vqa_prior_embed_fwd": (_I, [_P] * 6 + [_I] * 4 + [_F, _F, _U, _L, _P, _I, _P]),
    "vqa_colsum": (_I, [_P, _P, _I, _L, _L, _I, _I, _P]),
    "vqa_axpy": (_I, [_P, _P, _P, _L, _I, _P]),
    "vqa_dropout": (_I, [_P, _L, _F, _U, _U, _L, _P, _I, _P]),
    "vqa_scale_f32": (_I, [_P, _L, _F, _P]),
    "vqa_tf_mix": (_I, [_P, _P, _P, _P, _I, _I, _L, _F, _U, _U, _L, _P, _P]),
    "vqa_attn_fwd": (_I, [_P] * 6 + [_I] * 6 + [_F, _I, _P]),
    "vqa_attn_bwd": (_I, [_P] * 10 + [_I] * 6 + [_F, _I, _P]),
    "vqa_attn_weights_elems": (_S, [_I] * 5),
    "vqa_attn_weights": (_I, [_P] * 4 + [_S] + [_I] * 6 + [_F, _I, _P]),
    "vqa_head_wt": (_I, [_P, _P, _I, _I, _I, _P]),
    "vqa_head_fwd": (_I, [_P] * 8 + [_L, _I, _I, _I, _P]),
    "vqa_head_bwd_workspace": (_S, [_L, _I, _I]),
    "vqa_head_bwd": (_I, [_P] * 5 + [_F, _P, _P, _P, _L, _I, _I, _I, _P, _S, _P, _P]),
    "vqa_rowsum_workspace": (_S, [_L, _L]),
    "vqa_rowsum": (_I, [_P, _L, _L, _F, _P, _P, _S, _P]),
    "vqa_prior_decode_cache_bytes": (_S, [_I, _I, _I]),
    "vqa_prior_decode": (_I, [_P, _I] + [_P] * 10 + [_S] + [_I] * 8 + [_L, _U, _P]),
    "vqa_prior_decode_primed": (_I, [_P, _I] + [_P] * 10 + [_S] + [_I] * 8 + [_L, _U, _P, _I, _F, _I, _P]),
    "vqa_prior_decode_filtered": (_I, [_P, _I] + [_P] * 10 + [_S] + [_I] * 8 + [_L, _U, _P, _I, _F, _I, _F, _P, _P]),
    "vqa_prior_decode_scored": (_I, [_P, _I] + [_P] * 10 + [_S] + [_I] * 8 + [_L, _U, _P, _I, _F, _I, _F, _P, _P, _P,
                                                                                _P]),
    # device-resident corpus feed
    "vqa_corpus_steps_per_epoch": (_L, [_L, _I, _I]),
    "vqa_corpus_batch": (_I, [_P, _L, _I, _P, _P, _L, _P, _P, _P, _I, _L, _U, _P, _L, _I, _I, _I, _P]),
    "vqa_code_batch": (_I, [_P, _L, _P, _L, _I, _I, _P, _P, _L, _P, _P, _P, _P, _I, _L, _U, _P, _L, _I, _I, _I, _P]),
    # waveform -> int16 PCM
    "vqa_pcm_encode": (_I, [_P, _L, _P, _L, _I, _L, _L, _L, _F, _P, _P]),
    "vqa_pcm_splice": (_I, [_P, _L, _P, _L, _P, _L, _I, _L, _L, _L, _L, _L, _F, _P, _P]),
    # polyphase sample-rate conversion
    "vqa_resample": (_I, [_P, _I, _L, _L, _L, _L, _P, _L, _L, _L, _I, _I, _I, _P, _I, _P]),
    "vqa_resample_route": (_I, [_I, _I, _I, _P, _P]),
}

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load libvqa.so once. Raises ImportError if it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libvqa.so not found at {LIB_PATH}; build it with `python -c "
                              f"'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        abi = L.vqa_abi_version() if hasattr(L, "vqa_abi_version") else 1
        if abi != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} implements C-ABI revision {abi}, this binding needs {ABI_VERSION}: "
                              f"rebuild the library (argument lists differ between revisions)")
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return lib().vqa_get_last_error().decode()


def _check(rc: int, what: str):
    if rc != 0:
        raise VQAError(f"{what} failed ({rc}): {last_error()}")


def ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise VQAError("libvqa ops take device tensors only (got a CPU tensor)")
    if not t.is_contiguous():
        raise VQAError(f"libvqa ops take contiguous (N, T, C) tensors (got strides {t.stride()})")
    return ctypes.c_void_p(t.data_ptr())


# Test hook (tests/test_gpu_race.py, tools/cotenant.py inject): a callable run right before every libvqa launch is
# queued, on the launching thread with the launch's stream current — the race tests use it to put random spin
# delays in front of launches, so every cross-stream ordering the step relies on is exercised. None in the product.
launch_hook = None


def stream():
    if launch_hook is not None:
        launch_hook()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float32:
        return F32
    raise VQAError(f"unsupported activation dtype {dt}")


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ---- host-only helpers (callable without a GPU) --------------------------------------------------
def same_pad_left(T_in: int, K: int, stride: int, dilation: int = 1) -> int:
    return lib().vqa_same_pad_left(T_in, K, stride, dilation)


def same_out_len(T_in: int, stride: int) -> int:
    return lib().vqa_same_out_len(T_in, stride)


def reset_perm_index(seed: int, counter: int, level: int, M: int, k: int) -> int:
    return lib().vqa_reset_perm_index(seed, counter, level, M, k)


# which kernel a conv call runs (vqa_conv1d_route): ops, kernel families, and the names of the detail entries
OP_FWD, OP_BWD_DATA, OP_BWD_WEIGHT, OP_BWD_DATA_WEIGHT, OP_T_FWD, OP_T_BWD_DATA, OP_T_BWD_WEIGHT = range(7)
ROUTE_FAMILIES = ("co1", "conv32", "gather_mfma", "ci1", "thinO", "thin", "direct", "wgrad_mfma", "wgrad_thin",
                  "wgrad_direct", "two_call")
_ROUTE_DETAIL = {
    "co1": ("C",), "conv32": ("O", "PVX", "NEP", "FW"), "gather_mfma": ("C", "O", "PV", "TM", "NEP"),
    "ci1": ("O", "KT"), "thinO": ("C",), "thin": ("OV",), "direct": ("C", "O"), "wgrad_mfma": ("C", "O", "TT"),
    "wgrad_thin": ("C", "O", "wide_x"), "wgrad_direct": ("C", "O", "TT"), "two_call": ("data", "weight"),
}
ROUTE_DETAIL = 8


def conv1d_route(op, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype):
    """(family, detail) of the kernel the conv call `op` with these arguments runs: the family's name and a dict of
    its template parameters (for "two_call" the families of its two calls). Host-only: needs no GPU. Raises
    VQAError where the call itself would be refused."""
    d = (ctypes.c_int * ROUTE_DETAIL)()
    rc = lib().vqa_conv1d_route(op, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype, d)
    if rc < 0:
        _check(rc, "vqa_conv1d_route")
    fam = ROUTE_FAMILIES[rc]
    det = dict(zip(_ROUTE_DETAIL[fam], list(d)))
    if fam == "two_call":
        det = {k: ROUTE_FAMILIES[v] for k, v in det.items()}
    return fam, det


# ---- device ops ------------------------------------------------------------------------------------
def conv1d_fwd(x, w, b, residual, y, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype):
    _check(lib().vqa_conv1d_fwd(ptr(x), ptr(w), ptr(b), ptr(residual), ptr(y), B, T_in, T_out, C_in, C_out, K,
                                stride, dilation, pad, flags, dtype, stream()), "vqa_conv1d_fwd")


def conv1d_bwd_data(dy, w, mask, residual, dx, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype):
    _check(lib().vqa_conv1d_bwd_data(ptr(dy), ptr(w), ptr(mask), ptr(residual), ptr(dx), B, T_in, T_out, C_in,
                                     C_out, K, stride, dilation, pad, flags, dtype, stream()), "vqa_conv1d_bwd_data")


def conv1d_bwd_weight(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype):
    n = lib().vqa_conv1d_bwd_weight_workspace(B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype)
    ws = workspace(n, x.device)
    _check(lib().vqa_conv1d_bwd_weight(ptr(x), ptr(dy), ptr(dw), ptr(db), B, T_in, T_out, C_in, C_out, K, stride,
                                       dilation, pad, flags, dtype, ptr(ws), ws.numel(), stream()),
           "vqa_conv1d_bwd_weight")


class Deferred:
    """Collects deferred weight-gradient partials; flush() reduces them all in one launch."""

    def __init__(self):
        self.descs, self.keep = [], []

    def add(self, desc, ws):
        descs = desc if isinstance(desc, (list, tuple)) else [desc]
        self.descs.extend(descs)
        self.keep.append(ws)  # the partials must outlive the reduce launch

    def flush(self):
        if self.descs:
            arr = (PartialsDesc * len(self.descs))(*self.descs)
            _check(lib().vqa_reduce_partials(arr, len(self.descs), stream()), "vqa_reduce_partials")
        self.descs, self.keep = [], []


def conv1d_bwd_weight_deferred(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype,
                               deferred):
    n = lib().vqa_conv1d_bwd_weight_workspace(B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype)
    ws = workspace(n, x.device)
    d = PartialsDesc()
    _check(lib().vqa_conv1d_bwd_weight_partials(ptr(x), ptr(dy), ptr(dw), ptr(db), B, T_in, T_out, C_in, C_out, K,
                                                stride, dilation, pad, flags, dtype, ptr(ws), ws.numel(),
                                                ctypes.byref(d), stream()), "vqa_conv1d_bwd_weight_partials")
    deferred.add(d, ws)


def conv1d_bwd_data_weight(dy, w, x, residual, dx, dw, db, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad,
                           flags, dtype, deferred=None):
    """dx and (dw, db) of one Conv1D in one pass (vqa_conv1d_bwd_data_weight); `x` is the conv input (its
    ReLU' mask with VQA_PRE_RELU). With `deferred` the weight-gradient reduction joins its batch."""
    n = lib().vqa_conv1d_bwd_data_weight_workspace(B, T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags,
                                                    dtype)
    ws = workspace(n, x.device)
    d = PartialsDesc() if deferred is not None else None
    _check(lib().vqa_conv1d_bwd_data_weight(ptr(dy), ptr(w), ptr(x), ptr(residual), ptr(dx), ptr(dw), ptr(db), B,
                                            T_in, T_out, C_in, C_out, K, stride, dilation, pad, flags, dtype,
                                            ptr(ws), ws.numel(), ctypes.byref(d) if d is not None else None,
                                            stream()), "vqa_conv1d_bwd_data_weight")
    if deferred is not None:
        deferred.add(d, ws)


def dtail_supported(C, Cu, K_up, stride_up, K_out, C_out, dtype) -> bool:
    return bool(lib().vqa_dtail_supported(C, Cu, K_up, stride_up, K_out, C_out, dtype))


def dtail_fwd(h, w_up, b_up, w_out, b_out, y):
    """encdec.py:67-68 (last Conv1DTranspose) + :148 (output Conv1D) composed: h (B, T, 32) -> y (B, 2T, 1)
    fp32 (vqa_dtail_fwd)."""
    B, T, C = h.shape
    dt = dtype_code(h.dtype)
    Cu = w_up.shape[1]
    ws = workspace(lib().vqa_dtail_workspace(B, T, C, Cu, dt), h.device)
    _check(lib().vqa_dtail_fwd(ptr(h), ptr(w_up), ptr(b_up), ptr(w_out), ptr(b_out), ptr(y), B, T, C, Cu, dt, ptr(ws),
                               ws.numel(), stream()), "vqa_dtail_fwd")


def dtail_bwd(dy, h, w_up, b_up, w_out, b_out, dh, dw_up, db_up, dw_out, db_out):
    """Backward of dtail_fwd: dh and the gradients of both layers' kernels and biases (written)."""
    B, T, C = h.shape
    dt = dtype_code(h.dtype)
    Cu = w_up.shape[1]
    ws = workspace(lib().vqa_dtail_workspace(B, T, C, Cu, dt), h.device)
    _check(lib().vqa_dtail_bwd(ptr(dy), ptr(h), ptr(w_up), ptr(b_up), ptr(w_out), ptr(b_out), ptr(dh), ptr(dw_up),
                               ptr(db_up), ptr(dw_out), ptr(db_out), B, T, C, Cu, dt, ptr(ws), ws.numel(), stream()),
           "vqa_dtail_bwd")


def resblock_supported(C, dilation, dtype) -> bool:
    return bool(lib().vqa_resblock_supported(C, dilation, dtype))


class ResblockPlanInfo(ctypes.Structure):
    """vqa_resblock_plan_info (include/vqa.h)."""
    _fields_ = [("tile_rows", ctypes.c_int), ("compiled_dilation", ctypes.c_int), ("tiles_per_item", ctypes.c_int),
                ("tiles", ctypes.c_int), ("workgroups", ctypes.c_int), ("tiles_per_workgroup", ctypes.c_int),
                ("extra_tile_workgroups", ctypes.c_int), ("partial_rows", ctypes.c_int),
                ("lds_bytes", ctypes.c_int64)]

    def __repr__(self):
        return "ResblockPlan(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"

    def run(self, w):
        """[first, end) tiles of workgroup w"""
        first = w * self.tiles_per_workgroup + min(w, self.extra_tile_workgroups)
        return first, first + self.tiles_per_workgroup + (w < self.extra_tile_workgroups)


def resblock_plan(B, T, C, dilation, dtype, backward):
    """vqa_resblock_plan: the ResblockPlanInfo a resblock_fwd / resblock_bwd call of these sizes follows (dtype a
    torch dtype). Host-only, nothing is launched."""
    r = ResblockPlanInfo()
    _check(lib().vqa_resblock_plan(B, T, C, dilation, dtype_code(dtype), int(bool(backward)), ctypes.byref(r)),
           "vqa_resblock_plan")
    return r


def resblock_fwd(x, wa, ba, wb, bb, y, dilation, h_out=None):
    """resnet.py:7-29 forward, fused (vqa_resblock_fwd); x, y, h_out (B, T, 32) in the compute dtype."""
    B, T, C = x.shape
    _check(lib().vqa_resblock_fwd(ptr(x), ptr(wa), ptr(ba), ptr(wb), ptr(bb), ptr(y), ptr(h_out), B, T, C, dilation,
                                  dtype_code(x.dtype), stream()), "vqa_resblock_fwd")


def resblock_bwd(dy, x, wa, ba, wb, bb, dx, dwa, dba, dwb, dbb, dilation, deferred=None):
    """Backward of the fused block (h recomputed from x): dx and the four weight gradients."""
    B, T, C = x.shape
    dt = dtype_code(x.dtype)
    ws = workspace(lib().vqa_resblock_bwd_workspace(B, T, C, dilation, dt), x.device)
    descs = (PartialsDesc * 2)() if deferred is not None else None
    _check(lib().vqa_resblock_bwd(ptr(dy), ptr(x), ptr(wa), ptr(ba), ptr(wb), ptr(bb), ptr(dx), ptr(dwa), ptr(dba),
                                  ptr(dwb), ptr(dbb), B, T, C, dilation, dt, ptr(ws), ws.numel(), descs, stream()),
           "vqa_resblock_bwd")
    if deferred is not None:
        deferred.add([descs[0], descs[1]], ws)


def conv1d_transpose_bwd_weight_deferred(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, pad, flags, dtype,
                                         deferred):
    n = lib().vqa_conv1d_transpose_bwd_weight_workspace(B, T_in, T_out, C_in, C_out, K, stride, pad, flags, dtype)
    ws = workspace(n, x.device)
    d = PartialsDesc()
    _check(lib().vqa_conv1d_transpose_bwd_weight_partials(ptr(x), ptr(dy), ptr(dw), ptr(db), B, T_in, T_out, C_in,
                                                          C_out, K, stride, pad, flags, dtype, ptr(ws), ws.numel(),
                                                          ctypes.byref(d), stream()),
           "vqa_conv1d_transpose_bwd_weight_partials")
    deferred.add(d, ws)


def conv1d_transpose_fwd(x, w, b, residual, y, B, T_in, T_out, C_in, C_out, K, stride, pad, flags, dtype):
    _check(lib().vqa_conv1d_transpose_fwd(ptr(x), ptr(w), ptr(b), ptr(residual), ptr(y), B, T_in, T_out, C_in,
                                          C_out, K, stride, pad, flags, dtype, stream()), "vqa_conv1d_transpose_fwd")


def conv1d_transpose_bwd_data(dy, w, mask, residual, dx, B, T_in, T_out, C_in, C_out, K, stride, pad, flags, dtype):
    _check(lib().vqa_conv1d_transpose_bwd_data(ptr(dy), ptr(w), ptr(mask), ptr(residual), ptr(dx), B, T_in, T_out,
                                               C_in, C_out, K, stride, pad, flags, dtype, stream()),
           "vqa_conv1d_transpose_bwd_data")


def conv1d_transpose_bwd_weight(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, pad, flags, dtype):
    n = lib().vqa_conv1d_transpose_bwd_weight_workspace(B, T_in, T_out, C_in, C_out, K, stride, pad, flags, dtype)
    ws = workspace(n, x.device)
    _check(lib().vqa_conv1d_transpose_bwd_weight(ptr(x), ptr(dy), ptr(dw), ptr(db), B, T_in, T_out, C_in, C_out, K,
                                                 stride, pad, flags, dtype, ptr(ws), ws.numel(), stream()),
           "vqa_conv1d_transpose_bwd_weight")


def vq_sqnorm(E, esq):
    D, K = E.shape
    _check(lib().vqa_vq_sqnorm(ptr(E), ptr(esq), D, K, stream()), "vqa_vq_sqnorm")


def vq_argmin(z, E, esq, idx, min_dist=None):
    N, D = z.shape
    K = E.shape[1]
    _check(lib().vqa_vq_argmin(ptr(z), ptr(E), ptr(esq), ptr(idx), ptr(min_dist), N, D, K, dtype_code(z.dtype),
                               stream()), "vqa_vq_argmin")


def vq_split_bf16x3(E, E3):
    D, K = E.shape
    if tuple(E3.shape) != (K, 3, D) or E3.dtype != torch.bfloat16:
        raise VQAError(f"vq_split_bf16x3: E3 must be ({K}, 3, {D}) bf16")
    _check(lib().vqa_vq_split_bf16x3(ptr(E), ptr(E3), D, K, stream()), "vqa_vq_split_bf16x3")


def vq_argmin_split(z, E3, esq, idx, min_dist=None):
    N, D = z.shape
    K = E3.shape[0]
    if z.dtype != torch.bfloat16:
        raise VQAError("vq_argmin_split takes bf16 z")
    _check(lib().vqa_vq_argmin_split(ptr(z), ptr(E3), ptr(esq), ptr(idx), ptr(min_dist), N, D, K, stream()),
           "vqa_vq_argmin_split")


def vq_quantize(z, ET, idx, q_st, commit_out, m_sumT, n_sum, beta):
    N, D = z.shape
    K = ET.shape[0]
    dt = dtype_code(z.dtype)
    ws = workspace(lib().vqa_vq_quantize_workspace(N, D, K, dt), z.device)
    _check(lib().vqa_vq_quantize(ptr(z), ptr(ET), ptr(idx), ptr(q_st), ptr(commit_out), ptr(m_sumT), ptr(n_sum), N,
                                 D, K, beta, dt, ptr(ws), ws.numel(), stream()), "vqa_vq_quantize")


def vq_backward(dq, z, ET, idx, dz, scale):
    N, D = z.shape
    _check(lib().vqa_vq_backward(ptr(dq), ptr(z), ptr(ET), ptr(idx), ptr(dz), scale, N, D, dtype_code(z.dtype),
                                 stream()), "vqa_vq_backward")


def vq_reset_rows(z, RT, row_offset, N_global, seed, counter, level):
    N, D = z.shape
    K = RT.shape[0]
    _check(lib().vqa_vq_reset_rows(ptr(z), ptr(RT), N, row_offset, N_global, D, K, seed, ptr(counter), level,
                                   dtype_code(z.dtype), stream()), "vqa_vq_reset_rows")


def vq_ema_apply(E, ET, m_t, N_t, m_sumT, n_sum, RT, gamma, omg, thresh, metrics, counter, esq=None, E3=None,
                 ok=None):
    """EMA + dead-code reset; with esq / E3 also |e|^2 and the bf16 planes of the new codebook (same pass). With
    `ok` (an int32 device flag, grad_finite's) the guarded form: nothing is written unless ok[0] == 1."""
    D, K = E.shape
    if E3 is not None and (E3.dtype != torch.bfloat16 or tuple(E3.shape) != (K, 3, D)):
        raise VQAError(f"vq_ema_apply: E3 must be ({K}, 3, {D}) bf16")
    if ok is not None:
        _check(lib().vqa_vq_ema_apply_guarded(ptr(E), ptr(ET), ptr(m_t), ptr(N_t), ptr(m_sumT), ptr(n_sum), ptr(RT),
                                              gamma, omg, thresh, ptr(metrics), ptr(counter), ptr(esq), ptr(E3), D, K,
                                              _flag(ok), stream()), "vqa_vq_ema_apply_guarded")
        return
    _check(lib().vqa_vq_ema_apply_derived(ptr(E), ptr(ET), ptr(m_t), ptr(N_t), ptr(m_sumT), ptr(n_sum), ptr(RT), gamma,
                                          omg, thresh, ptr(metrics), ptr(counter), ptr(esq), ptr(E3), D, K, stream()),
           "vqa_vq_ema_apply_derived")


def mse_loss(x, r, extra, dr, loss_out):
    n = x.numel()
    ws = workspace(lib().vqa_mse_loss_workspace(n), x.device)
    _check(lib().vqa_mse_loss(ptr(x), ptr(r), ptr(extra), ptr(dr), ptr(loss_out), n, ptr(ws), ws.numel(), stream()),
           "vqa_mse_loss")


def adam_keras(w, g, m, v, step, lr, beta1, beta2, eps, grad_scale, lr_dev=None):
    _check(lib().vqa_adam_keras(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), ptr(step), float(lr), ptr(lr_dev), beta1,
                                beta2, eps, grad_scale, stream()), "vqa_adam_keras")


# gradient clipping (include/vqa.h): mode bits, floats per workgroup of the variable table, floats in `stats`
CLIP_VALUE, CLIP_NORM, CLIP_GLOBAL_NORM = 1, 2, 4
CLIP_BLOCK = 4096
CLIP_STATS = 8


def grad_norm_workspace(n: int, nseg: int) -> int:
    return lib().vqa_grad_norm_workspace(n, nseg)


def grad_norm(g, seg_start, block_seg, grad_scale, modes, clipvalue, clipnorm, global_clipnorm, seg_norm, stats,
              ws):
    """The norm pass of a clipped step (vqa_grad_norm): per-variable norms and the statistics of grad_scale * g."""
    _check(lib().vqa_grad_norm(ptr(g), g.numel(), ptr(seg_start), ptr(block_seg), seg_start.numel(), grad_scale,
                               int(modes), clipvalue, clipnorm, global_clipnorm, ptr(seg_norm), ptr(stats), ptr(ws),
                               ws.numel(), stream()), "vqa_grad_norm")


def adam_keras_clipped(w, g, m, v, step, lr, beta1, beta2, eps, grad_scale, seg_start, block_seg, modes, clipvalue,
                       clipnorm, global_clipnorm, seg_norm, stats, lr_dev=None):
    _check(lib().vqa_adam_keras_clipped(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), ptr(step), float(lr), ptr(lr_dev),
                                        beta1, beta2, eps, grad_scale, ptr(seg_start), ptr(block_seg),
                                        seg_start.numel(), int(modes), clipvalue, clipnorm, global_clipnorm,
                                        ptr(seg_norm), ptr(stats), stream()), "vqa_adam_keras_clipped")


def adam_keras_ema(w, g, m, v, step, lr, beta1, beta2, eps, grad_scale, ema, average_decay, start_step=0,
                   dynamic=False, lr_dev=None):
    """adam_keras with the weights' moving average `ema` updated in the same launch (vqa_adam_keras_ema)."""
    _check(lib().vqa_adam_keras_ema(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), ptr(step), float(lr), ptr(lr_dev),
                                    beta1, beta2, eps, grad_scale, ptr(ema), float(average_decay), int(start_step),
                                    int(bool(dynamic)), stream()), "vqa_adam_keras_ema")


def adam_keras_clipped_ema(w, g, m, v, step, lr, beta1, beta2, eps, grad_scale, seg_start, block_seg, modes,
                           clipvalue, clipnorm, global_clipnorm, seg_norm, stats, ema, average_decay, start_step=0,
                           dynamic=False, lr_dev=None):
    """adam_keras_clipped with the weights' moving average in the same launch (vqa_adam_keras_clipped_ema)."""
    _check(lib().vqa_adam_keras_clipped_ema(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), ptr(step), float(lr),
                                            ptr(lr_dev), beta1, beta2, eps, grad_scale, ptr(seg_start),
                                            ptr(block_seg), seg_start.numel(), int(modes), clipvalue, clipnorm,
                                            global_clipnorm, ptr(seg_norm), ptr(stats), ptr(ema),
                                            float(average_decay), int(start_step), int(bool(dynamic)), stream()),
           "vqa_adam_keras_clipped_ema")


def swap_f32(a, b):
    """Exchange the contents of two fp32 buffers of equal size in place, exactly (vqa_swap_f32)."""
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel():
        raise VQAError("swap_f32: two float32 buffers of equal size")
    _check(lib().vqa_swap_f32(ptr(a), ptr(b), a.numel(), stream()), "vqa_swap_f32")


FINITE_MAX_BLOCKS = 4096  # VQA_FINITE_MAX_BLOCKS: vqa_grad_finite's grid cap (workgroups of 256)


def _flag(ok):
    if ok.dtype != torch.int32:
        raise VQAError("the step guard's flag is an int32 device tensor")
    return ptr(ok)


def grad_finite(g, ok):
    """ok[0] = 1 if every float of g is finite, else 0 (vqa_grad_finite; ok: int32 device tensor)."""
    if g.dtype != torch.float32:
        raise VQAError("grad_finite: a float32 buffer")
    flag = _flag(ok)
    _check(lib().vqa_grad_finite(ptr(g), g.numel(), flag, stream()), "vqa_grad_finite")


def adam_keras_guarded(w, g, m, v, step, lr, beta1, beta2, eps, grad_scale, ok, skip_counters, clip=None, ema=None,
                       lr_dev=None):
    """The Adam update behind grad_finite's flag (vqa_adam_keras_guarded). clip: None or (seg_start, block_seg,
    modes, clipvalue, clipnorm, global_clipnorm, seg_norm, stats); ema: None or (average, average_decay, start_step,
    dynamic). skip_counters: int64[2] device tensor (skipped in all, skipped in a row)."""
    seg_start, block_seg, modes, cv, cn, gcn, seg_norm, stats = clip or (None, None, 0, 0.0, 0.0, 0.0, None, None)
    average, decay, start, dynamic = ema or (None, 0.0, 0, False)
    if skip_counters.dtype != torch.int64 or skip_counters.numel() != 2:
        raise VQAError("adam_keras_guarded: skip_counters is an int64 device tensor of 2")
    _check(lib().vqa_adam_keras_guarded(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), ptr(step), float(lr), ptr(lr_dev),
                                        beta1, beta2, eps, grad_scale, ptr(seg_start), ptr(block_seg),
                                        0 if seg_start is None else seg_start.numel(), int(modes), cv, cn, gcn,
                                        ptr(seg_norm), ptr(stats), ptr(average), float(decay), int(start),
                                        int(bool(dynamic)), _flag(ok), ptr(skip_counters), stream()),
           "vqa_adam_keras_guarded")


def lr_schedule(step, lr_out, kind, p):
    p = list(p) + [0.0] * (4 - len(p))
    _check(lib().vqa_lr_schedule(ptr(step), ptr(lr_out), int(kind), *[float(v) for v in p[:4]], stream()),
           "vqa_lr_schedule")


def step_metrics(loss_slots, vq_metrics, macc, levels, scale):
    _check(lib().vqa_step_metrics(ptr(loss_slots), ptr(vq_metrics), ptr(macc), levels, scale, stream()),
           "vqa_step_metrics")


def step_metrics_if(loss_slots, vq_metrics, macc, levels, scale, ok):
    _check(lib().vqa_step_metrics_if(ptr(loss_slots), ptr(vq_metrics), ptr(macc), levels, scale, _flag(ok), stream()),
           "vqa_step_metrics_if")


def synthetic_batch(x, seed, rank=0, sample_rate=44100.0):
    """x: (B, T) or (B, T, 1) fp32 device tensor, filled in place (vqa_synthetic_batch)."""
    B, T = x.shape[0], x.numel() // x.shape[0]
    if x.dtype != torch.float32:
        raise VQAError("synthetic_batch fills an fp32 tensor")
    _check(lib().vqa_synthetic_batch(ptr(x), B, T, seed, rank, sample_rate, stream()), "vqa_synthetic_batch")


def embedding_fwd(table, idx, out):
    """src/conditioner/conditioners.py:64 layers.Embedding: out (..., D) = table[idx] (vqa_embedding_fwd)."""
    K, D = table.shape
    N = idx.numel()
    if idx.dtype != torch.int64 or out.shape[-1] != D or out.numel() != N * D:
        raise VQAError("embedding_fwd: idx int64 (...), out (..., D)")
    _check(lib().vqa_embedding_fwd(ptr(table), ptr(idx), ptr(out), N, D, K, dtype_code(out.dtype), stream()),
           "vqa_embedding_fwd")


def embedding_bwd(dy, idx, dtable):
    """dtable[k] += sum of dy rows with idx == k, fixed order (vqa_embedding_bwd)."""
    K, D = dtable.shape
    N = idx.numel()
    ws = workspace(lib().vqa_embedding_bwd_workspace(N, D, K), dy.device)
    _check(lib().vqa_embedding_bwd(ptr(dy), ptr(idx), ptr(dtable), N, D, K, dtype_code(dy.dtype), ptr(ws), ws.numel(),
                                   stream()), "vqa_embedding_bwd")


def layernorm_fwd(x, gamma, beta, y, eps):
    C = x.shape[-1]
    _check(lib().vqa_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), x.numel() // C, C, eps, dtype_code(x.dtype),
                                   stream()), "vqa_layernorm_fwd")


def layernorm_bwd(x, dy, gamma, dx, dgamma, dbeta, eps, deferred=None):
    C = x.shape[-1]
    rows = x.numel() // C
    ws = workspace(lib().vqa_layernorm_bwd_workspace(rows, C), x.device)
    d = PartialsDesc() if deferred is not None else None
    _check(lib().vqa_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(dx), ptr(dgamma), ptr(dbeta), rows, C, eps,
                                   dtype_code(x.dtype), ptr(ws), ws.numel(), ctypes.byref(d) if d is not None else None,
                                   stream()), "vqa_layernorm_bwd")
    if deferred is not None:
        deferred.add(d, ws)


def counter_add(counter, delta=1):
    _check(lib().vqa_counter_add(ptr(counter), delta, stream()), "vqa_counter_add")


def counter_add_if(counter, ok, delta=1):
    """counter += delta if ok[0] == 1 (vqa_counter_add_if)."""
    _check(lib().vqa_counter_add_if(ptr(counter), delta, _flag(ok), stream()), "vqa_counter_add_if")


PCM_I16, PCM_F32 = 0, 1  # VQA_PCM_*
FEED_PERM_LEVEL = 0x46454544  # VQA_FEED_PERM_LEVEL: the `level` of the feed's shuffle key


def corpus_steps_per_epoch(M: int, B: int, world: int = 1) -> int:
    """Full steps in one epoch of M windows, M // (B*world) (vqa_corpus_steps_per_epoch; host only)."""
    return int(lib().vqa_corpus_steps_per_epoch(int(M), int(B), int(world)))


def _feed_checks(op, int64_names, int64, stores, unit, starts, labels, labels_out, index_out, B) -> int:
    """The checks corpus_batch and code_batch share -> M. int64: the tensors that must be int64 (int64_names in the
    message); stores: (tensor or None, its length, its name, the length's name), each allocated up to its length
    rounded up to 16 bytes (the kernels' memory contract)."""
    if any(t is not None and t.dtype != torch.int64 for t in int64):
        raise VQAError(f"{op}: {int64_names} are int64")
    for t, n, what, length in stores:
        if t is not None and (n * t.element_size() + 15) // 16 * 16 > t.numel() * t.element_size():
            raise VQAError(f"{op}: the {what} tensor ({t.numel()} {unit}) does not cover {length} {n} "
                           f"rounded up to 16 bytes")
    M = starts.numel()
    if labels is not None and labels.numel() != M:
        raise VQAError(f"{op}: {labels.numel()} labels for {M} windows")
    for t in (labels_out, index_out):
        if t is not None and t.numel() != B:
            raise VQAError(f"{op}: labels_out / index_out hold {B} entries")
    return M


def corpus_batch(corpus, corpus_len, starts, labels, x, labels_out=None, index_out=None, seed=0, counter=None,
                 step=0, rank=0, world=1, shuffle=True):
    """One step's batch of a device-resident corpus (vqa_corpus_batch, include/vqa.h): corpus is the 1-D int16 or
    fp32 sample tensor (allocated up to a multiple of 16 bytes past corpus_len samples), starts / labels the (M,)
    int64 window table, x the (B, T) or (B, T, 1) fp32 batch; labels_out / index_out (B,) int64."""
    if corpus.dtype == torch.int16:
        pcm = PCM_I16
    elif corpus.dtype == torch.float32:
        pcm = PCM_F32
    else:
        raise VQAError(f"corpus_batch: the corpus is int16 or float32 (got {corpus.dtype})")
    if x.dtype != torch.float32:
        raise VQAError("corpus_batch fills an fp32 tensor")
    corpus_len = int(corpus_len)
    B, T = x.shape[0], x.numel() // x.shape[0]
    M = _feed_checks("corpus_batch", "starts, labels, labels_out, index_out and counter",
                     (starts, labels, labels_out, index_out, counter), [(corpus, corpus_len, "corpus", "corpus_len")],
                     "samples", starts, labels, labels_out, index_out, B)
    _check(lib().vqa_corpus_batch(ptr(corpus), corpus_len, pcm, ptr(starts), ptr(labels), M, ptr(x), ptr(labels_out),
                                  ptr(index_out), B, T, int(seed), ptr(counter), int(step), int(rank), int(world),
                                  int(bool(shuffle)), stream()), "vqa_corpus_batch")


CODE_I16, CODE_I32 = 0, 1  # VQA_CODE_*


def code_batch(codes, codes_len, starts, labels, z, upper=None, upper_len=0, rate=1, z_upper=None, labels_out=None,
               index_out=None, seed=0, counter=None, step=0, rank=0, world=1, shuffle=True):
    """One step's batch of a device-resident code corpus (vqa_code_batch, include/vqa.h): codes (and upper, the level
    above's codes of the same tracks) are 1-D int16 or int32 tensors allocated up to a multiple of 16 bytes past
    codes_len (upper_len) codes, starts / labels the (M,) int64 window table, z the (B, T) int64 batch, z_upper the
    (B, T / rate) int64 windows of the level above; labels_out / index_out (B,) int64."""
    if codes.dtype == torch.int16:
        width = CODE_I16
    elif codes.dtype == torch.int32:
        width = CODE_I32
    else:
        raise VQAError(f"code_batch: the codes are int16 or int32 (got {codes.dtype})")
    if upper is not None and upper.dtype != codes.dtype:
        raise VQAError(f"code_batch: upper is {upper.dtype}, codes {codes.dtype}")
    codes_len, upper_len, rate = int(codes_len), int(upper_len), int(rate)
    B, T = z.shape[0], z.numel() // z.shape[0]
    M = _feed_checks("code_batch", "starts, labels, z, z_upper, labels_out, index_out and counter",
                     (starts, z, z_upper, labels, labels_out, index_out, counter),
                     [(codes, codes_len, "codes", "its length"), (upper, upper_len, "upper", "its length")], "codes",
                     starts, labels, labels_out, index_out, B)
    if z_upper is not None and rate >= 1 and z_upper.numel() != B * (T // rate):
        raise VQAError(f"code_batch: z_upper holds {z_upper.numel()} codes, not {B} x {T // rate}")
    _check(lib().vqa_code_batch(ptr(codes), codes_len, ptr(upper), upper_len, rate, width, ptr(starts), ptr(labels), M,
                                ptr(z), ptr(z_upper), ptr(labels_out), ptr(index_out), B, T, int(seed), ptr(counter),
                                int(step), int(rank), int(world), int(bool(shuffle)), stream()), "vqa_code_batch")


def pcm_encode(x, out, x0=0, o0=0, n=None, gain=1.0, clipped=None):
    """fp32 waveform -> int16 PCM with crop and placement (vqa_pcm_encode, include/vqa.h): x is the (B, ldx) or
    (B, ldx, 1) fp32 source (1-D: one row), out the (B, ldo) int16 destination; samples [x0, x0 + n) of every row of
    x go to [o0, o0 + n) of the same row of out as clamp(round_half_even(x * gain * 32768)), NaN as 0. n defaults to
    the rest of x's rows. clipped (B,) int32 is added to, never zeroed: the samples that were clamped or NaN."""
    if x.dtype != torch.float32 or out.dtype != torch.int16:
        raise VQAError(f"pcm_encode: x is float32 and out int16 (got {x.dtype}, {out.dtype})")
    B = x.shape[0] if x.dim() > 1 else 1
    ldx = x.numel() // max(B, 1)
    Bo = out.shape[0] if out.dim() > 1 else 1
    ldo = out.numel() // max(Bo, 1)
    if Bo != B:
        raise VQAError(f"pcm_encode: x has {B} rows, out {Bo}")
    if clipped is not None and (clipped.dtype != torch.int32 or clipped.numel() != B):
        raise VQAError(f"pcm_encode: clipped holds {B} int32 entries")
    n = ldx - int(x0) if n is None else int(n)
    _check(lib().vqa_pcm_encode(ptr(x), ldx, ptr(out), ldo, B, int(x0), int(o0), n, float(gain), ptr(clipped),
                                stream()), "vqa_pcm_encode")


def pcm_splice(x, p, out, seam, fade=0, x0=0, o0=0, n=None, gain=1.0, clipped=None):
    """pcm_encode with a second source and a seam (vqa_pcm_splice, include/vqa.h): p is the (B, ldp) or (B, ldp, 1)
    fp32 prompt audio, indexed by absolute position as out is. The samples of out at [o0, o0 + n) are p before
    seam - fade, x from seam on and, over the `fade` samples between, p + (x - p) * (i + 1) / (fade + 1); then
    pcm_encode's gain, rounding, clamp and clipped count."""
    if x.dtype != torch.float32 or p.dtype != torch.float32 or out.dtype != torch.int16:
        raise VQAError(f"pcm_splice: x and p are float32 and out int16 (got {x.dtype}, {p.dtype}, {out.dtype})")
    B = x.shape[0] if x.dim() > 1 else 1
    ldx = x.numel() // max(B, 1)
    Bp = p.shape[0] if p.dim() > 1 else 1
    ldp = p.numel() // max(Bp, 1)
    Bo = out.shape[0] if out.dim() > 1 else 1
    ldo = out.numel() // max(Bo, 1)
    if Bo != B or Bp != B:
        raise VQAError(f"pcm_splice: x has {B} rows, p {Bp}, out {Bo}")
    if clipped is not None and (clipped.dtype != torch.int32 or clipped.numel() != B):
        raise VQAError(f"pcm_splice: clipped holds {B} int32 entries")
    n = ldx - int(x0) if n is None else int(n)
    _check(lib().vqa_pcm_splice(ptr(x), ldx, ptr(p), ldp, ptr(out), ldo, B, int(x0), int(o0), n, int(seam), int(fade),
                                float(gain), ptr(clipped), stream()), "vqa_pcm_splice")


RESAMPLE_F32, RESAMPLE_I16 = 0, 1  # x_dtype of vqa_resample


def _rows(t, what):
    """(pointer, rows, samples per row, samples between rows) of a device tensor (n,) or (B, n) whose rows are
    dense; the rows may be a slice of wider ones (a view: stride(0) is what the kernel steps by)."""
    if not t.is_cuda:
        raise VQAError(f"resample: {what} is a device tensor (got a CPU tensor)")
    if t.dim() not in (1, 2) or t.numel() == 0 or t.stride(-1) != 1:
        raise VQAError(f"resample: {what} is (n,) or (B, n) with dense rows (got shape {tuple(t.shape)}, strides "
                       f"{t.stride()})")
    B = t.shape[0] if t.dim() == 2 else 1
    ld = t.stride(0) if t.dim() == 2 and B > 1 else t.shape[-1]
    if ld < t.shape[-1]:
        raise VQAError(f"resample: the rows of {what} overlap (strides {t.stride()})")
    return ctypes.c_void_p(t.data_ptr()), B, t.shape[-1], ld


def resample(x, out, taps, up, down, *, in0=0, m0=0, track_len=None):
    """Polyphase sample-rate conversion (vqa_resample, include/vqa.h): x (n_in,) or (B, n_in), fp32 or int16 (read as
    x * 2^-15), holds samples [in0, in0 + n_in) of tracks of track_len samples (default: in0 + n_in); out (n_out,) or
    (B, n_out) fp32 receives outputs [m0, m0 + n_out); taps is the contiguous (up, P) fp32 table. x and out may be
    column slices of wider tensors."""
    if x.dtype == torch.float32:
        code = RESAMPLE_F32
    elif x.dtype == torch.int16:
        code = RESAMPLE_I16
    else:
        raise VQAError(f"resample: x is float32 or int16 (got {x.dtype})")
    if out.dtype != torch.float32 or taps.dtype != torch.float32:
        raise VQAError(f"resample: out and taps are float32 (got {out.dtype}, {taps.dtype})")
    px, B, n_in, ldx = _rows(x, "x")
    po, Bo, n_out, ldo = _rows(out, "out")
    if Bo != B:
        raise VQAError(f"resample: x has {B} rows, out {Bo}")
    if taps.dim() != 2 or taps.shape[0] != int(up):
        raise VQAError(f"resample: taps is (up, taps_per_phase) = ({int(up)}, P) (got shape {tuple(taps.shape)})")
    track_len = int(in0) + n_in if track_len is None else int(track_len)
    _check(lib().vqa_resample(px, code, ldx, int(in0), n_in, track_len, po, ldo, int(m0), n_out, B, int(up),
                              int(down), ptr(taps), taps.shape[1], stream()), "vqa_resample")


def resample_route(up, down, taps_per_phase):
    """(table_in_lds, tile_outputs) of a vqa_resample call with these rates and taps: whether the tap table is
    staged in LDS (else it is read from global memory) and the outputs a workgroup computes. Host-only."""
    lds, tile = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().vqa_resample_route(int(up), int(down), int(taps_per_phase), ctypes.byref(lds), ctypes.byref(tile)),
           "vqa_resample_route")
    return bool(lds.value), tile.value


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def spectral_loss_workspace(B, T, n_fft, hop, win, with_grad=True) -> int:
    n = lib().vqa_spectral_loss_workspace(B, T, _int_array(n_fft), _int_array(hop), _int_array(win), len(n_fft),
                                          1 if with_grad else 0)
    if n == 0:
        raise VQAError(f"spectral_loss: bad shape B={B} T={T} n_fft={n_fft} hop={hop} win={win}")
    return n


def spectral_loss(x, r, loss_out, dr, item_loss, n_fft, hop, win, ws=None):
    """x, r, dr: (B, T) fp32 device tensors; loss_out: 1-element fp32. dr / item_loss may be None."""
    B, T = x.shape[0], x.numel() // x.shape[0]
    nres = len(n_fft)
    if ws is None:
        ws = workspace(spectral_loss_workspace(B, T, n_fft, hop, win, dr is not None), x.device)
    _check(lib().vqa_spectral_loss(ptr(x), ptr(r), ptr(loss_out), ptr(dr), ptr(item_loss), B, T, _int_array(n_fft),
                                   _int_array(hop), _int_array(win), nres, ptr(ws), ws.numel(), stream()),
           "vqa_spectral_loss")


def spectral_target(x, n_fft, hop, win):
    """Tables + |S_x| of every resolution for a (B, T) fp32 target -> a uint8 device buffer."""
    B, T = x.shape[0], x.numel() // x.shape[0]
    a = (_int_array(n_fft), _int_array(hop), _int_array(win))
    n = lib().vqa_spectral_target_workspace(B, T, *a, len(n_fft))
    if n == 0:
        raise VQAError(f"spectral_target: bad shape B={B} T={T} n_fft={n_fft} hop={hop} win={win}")
    tg = workspace(n, x.device)
    _check(lib().vqa_spectral_target(ptr(x), ptr(tg), tg.numel(), B, T, *a, len(n_fft), stream()),
           "vqa_spectral_target")
    return tg


def spectral_loss_target_workspace(B, T, n_fft, hop, win, with_grad=True) -> int:
    n = lib().vqa_spectral_loss_target_workspace(B, T, _int_array(n_fft), _int_array(hop), _int_array(win),
                                                 len(n_fft), 1 if with_grad else 0)
    if n == 0:
        raise VQAError(f"spectral_loss_target: bad shape B={B} T={T} n_fft={n_fft} hop={hop} win={win}")
    return n


def spectral_loss_target(target, r, loss_out, dr, item_loss, n_fft, hop, win, ws=None):
    """The spectral loss of r (B, T) against a spectral_target buffer; dr / item_loss may be None."""
    B, T = r.shape[0], r.numel() // r.shape[0]
    a = (_int_array(n_fft), _int_array(hop), _int_array(win))
    if ws is None:
        ws = workspace(spectral_loss_target_workspace(B, T, n_fft, hop, win, dr is not None), r.device)
    _check(lib().vqa_spectral_loss_target(ptr(target), ptr(r), ptr(loss_out), ptr(dr), ptr(item_loss), B, T, *a,
                                          len(n_fft), ptr(ws), ws.numel(), stream()), "vqa_spectral_loss_target")


def stft_magnitude(x, mag, n_fft, hop, win):
    B, T = x.shape[0], x.numel() // x.shape[0]
    _check(lib().vqa_stft_magnitude(ptr(x), ptr(mag), B, T, n_fft, hop, win, stream()), "vqa_stft_magnitude")


# ---- factorized-attention prior (vqa_prior*.hip) ----------------------------------------------------
def rptr(t: torch.Tensor):
    """(pointer, row stride) of a row-strided view (last dim contiguous, uniform row stride): column slices
    such as qkv[..., 0:32] of a (N, T, 96) tensor."""
    if not t.is_cuda:
        raise VQAError("libvqa ops take device tensors only (got a CPU tensor)")
    if t.stride(-1) != 1:
        raise VQAError("row-strided view needs a contiguous last dimension")
    ld = t.stride(-2) if t.dim() >= 2 else t.shape[-1]
    for d in range(t.dim() - 2):
        if t.stride(d) != t.stride(d + 1) * t.shape[d + 1]:
            raise VQAError(f"view with strides {t.stride()} is not row-strided")
    return ctypes.c_void_p(t.data_ptr()), ld


def seqlin_fwd(x, w, b, y, T, taps=1, dir=-1, wtrans=False, residual=None, accumulate=False):
    """vqa_seqlin_fwd on (nseq*T, K) rows -> (nseq*T, N) rows. w: (taps, K, N) (wtrans: (taps, N, K)) or (K, N)."""
    px, ldx = rptr(x)
    py, ldy = rptr(y)
    pr, ldr = rptr(residual) if residual is not None else (None, 0)
    K, N = x.shape[-1], y.shape[-1]
    rows = x.numel() // K
    _check(lib().vqa_seqlin_fwd(px, ldx, ptr(w), ptr(b), pr, ldr, py, ldy, rows // T, T, K, N, taps, dir,
                                int(bool(wtrans)), int(bool(accumulate)), dtype_code(x.dtype), stream()),
           "vqa_seqlin_fwd")


class SeqlinPrepDesc(ctypes.Structure):
    """vqa_seqlin_prep_desc (include/vqa.h)."""
    _fields_ = [("w", ctypes.c_void_p), ("out", ctypes.c_void_p), ("taps", ctypes.c_int), ("K", ctypes.c_int),
                ("N", ctypes.c_int), ("wtrans", ctypes.c_int)]


def seqlin_prep(descs, dtype):
    """One launch converting a list of (w fp32 tensor, out tensor, taps, K, N, wtrans) to [taps][N][K] images."""
    arr = (SeqlinPrepDesc * len(descs))(*[SeqlinPrepDesc(ptr(w).value, ptr(o).value, t, k, n, int(bool(tr)))
                                         for (w, o, t, k, n, tr) in descs])
    _check(lib().vqa_seqlin_prep(arr, len(descs), dtype_code(dtype), stream()), "vqa_seqlin_prep")


def seqlin_fwd_prepped(x, wp, b, y, T, taps=1, dir=-1, residual=None, accumulate=False):
    """vqa_seqlin_fwd_prepped: wp = (taps, N, K) image in the activation dtype (seqlin_prep)."""
    px, ldx = rptr(x)
    py, ldy = rptr(y)
    pr, ldr = rptr(residual) if residual is not None else (None, 0)
    K, N = x.shape[-1], y.shape[-1]
    rows = x.numel() // K
    _check(lib().vqa_seqlin_fwd_prepped(px, ldx, ptr(wp), ptr(b), pr, ldr, py, ldy, rows // T, T, K, N, taps, dir,
                                        int(bool(accumulate)), dtype_code(x.dtype), stream()),
           "vqa_seqlin_fwd_prepped")


def seqlin_fused_ln_ok(x, K):
    """vqa_seqlin_fwd_ln_prepped's domain: bf16 activations with K = 128 channels."""
    return x.dtype == torch.bfloat16 and K == 128


def seqlin_fwd_ln_prepped(x, gamma, beta, eps, wp, b, y, T, taps=1, dir=-1, residual=None):
    """vqa_seqlin_fwd_ln_prepped: seqlin_fwd_prepped(LayerNorm(x)) in one launch (bf16, K = 128)."""
    px, ldx = rptr(x)
    py, ldy = rptr(y)
    pr, ldr = rptr(residual) if residual is not None else (None, 0)
    K, N = x.shape[-1], y.shape[-1]
    rows = x.numel() // K
    _check(lib().vqa_seqlin_fwd_ln_prepped(px, ldx, ptr(gamma), ptr(beta), float(eps), ptr(wp), ptr(b), pr, ldr, py,
                                           ldy, rows // T, T, K, N, taps, dir, dtype_code(x.dtype), stream()),
           "vqa_seqlin_fwd_ln_prepped")


class SeqlinRouteInfo(ctypes.Structure):
    """vqa_seqlin_route_info (include/vqa.h)."""
    _fields_ = [("direct", ctypes.c_int), ("waves", ctypes.c_int), ("tile_rows", ctypes.c_int),
                ("workgroups", ctypes.c_int), ("tiles", ctypes.c_int), ("out_tiles", ctypes.c_int),
                ("lds_bytes", ctypes.c_int64)]

    def __repr__(self):
        return "SeqlinRoute(" + ", ".join(f"{n}={getattr(self, n)}" for n, _ in self._fields_) + ")"


def seqlin_route(x, y, T, w=None, wp=None, b=None, taps=1, dir=-1, wtrans=False, residual=None, accumulate=False,
                 layernorm=False):
    """vqa_seqlin_route for the seqlin_fwd (w) / seqlin_fwd_prepped (wp) / seqlin_fwd_ln_prepped (wp, layernorm)
    call with these tensors: the SeqlinRouteInfo the launch would follow. Host-only, nothing is launched."""
    px, ldx = rptr(x)
    py, ldy = rptr(y)
    pr, ldr = rptr(residual) if residual is not None else (None, 0)
    K, N = x.shape[-1], y.shape[-1]
    rows = x.numel() // K
    r = SeqlinRouteInfo()
    _check(lib().vqa_seqlin_route(px, ldx, ptr(w), ptr(wp), ptr(b), pr, ldr, py, ldy, rows // T, T, K, N, taps, dir,
                                  int(bool(wtrans)), int(bool(accumulate)), dtype_code(x.dtype),
                                  int(bool(layernorm)), ctypes.byref(r)), "vqa_seqlin_route")
    return r


def seqlin_wgrad_plan(nseq, T, K, N, taps, dtype):
    """(seg_rows, segs, pairs_per_wave) of a vqa_seqlin_wgrad call. Host-only."""
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().vqa_seqlin_wgrad_plan(nseq, T, K, N, taps, dtype_code(dtype), ctypes.byref(a), ctypes.byref(b),
                                       ctypes.byref(c)), "vqa_seqlin_wgrad_plan")
    return a.value, b.value, c.value


def head_bwd_plan(M, K, V):
    """(segs, seg_rows) of vqa_head_bwd's weight-gradient kernel. Host-only."""
    a, b = ctypes.c_int(0), ctypes.c_int64(0)
    _check(lib().vqa_head_bwd_plan(int(M), int(K), int(V), ctypes.byref(a), ctypes.byref(b)), "vqa_head_bwd_plan")
    return a.value, b.value


def seqlin_wgrad(x, dy, dw, db, T, taps=1, deferred=None):
    px, ldx = rptr(x)
    pd, ldd = rptr(dy)
    K, N = x.shape[-1], dy.shape[-1]
    nseq = (x.numel() // K) // T
    ws = workspace(lib().vqa_seqlin_wgrad_workspace(nseq, T, K, N, taps), x.device)
    d = PartialsDesc() if deferred is not None else None
    _check(lib().vqa_seqlin_wgrad(px, ldx, pd, ldd, ptr(dw), ptr(db), nseq, T, K, N, taps, dtype_code(x.dtype),
                                  ptr(ws), ws.numel(), ctypes.byref(d) if d is not None else None, stream()),
           "vqa_seqlin_wgrad")
    if deferred is not None:
        deferred.add(d, ws)


def prior_embed_fwd(table, pos, tokens, out, scale, ycond=None, xcond=None, rate=0.0, seed=0, counter=None,
                    elem_offset=0):
    N, T = tokens.shape
    bins, W = table.shape
    _check(lib().vqa_prior_embed_fwd(ptr(table), ptr(pos), ptr(tokens), ptr(ycond), ptr(xcond), ptr(out), N, T, W,
                                     bins, scale, rate, seed, int(elem_offset), ptr(counter), dtype_code(out.dtype),
                                     stream()),
           "vqa_prior_embed_fwd")


def colsum(x, out, nout, ostride, inner, accumulate=False):
    _check(lib().vqa_colsum(ptr(x), ptr(out), nout, ostride, inner, int(bool(accumulate)), dtype_code(x.dtype),
                            stream()), "vqa_colsum")


def axpy(x, y, z):
    _check(lib().vqa_axpy(ptr(x), ptr(y), ptr(z), x.numel(), dtype_code(x.dtype), stream()), "vqa_axpy")


EMB_DROPOUT_SALT = 0x454D42  # VQA_EMB_DROPOUT_SALT: vqa_prior_embed_fwd's dropout mask is vqa_dropout's with this salt


def dropout_(x, rate, seed, salt, counter=None, elem_offset=0):
    """keras Dropout in place; elem_offset = the global flat index of x[0] (data parallel: rank * x.numel())."""
    _check(lib().vqa_dropout(ptr(x), x.numel(), rate, seed, salt, int(elem_offset), ptr(counter), dtype_code(x.dtype),
                             stream()),
           "vqa_dropout")


def scale_f32_(x, s):
    _check(lib().vqa_scale_f32(ptr(x), x.numel(), s, stream()), "vqa_scale_f32")


def tf_mix(codes, amax, mask, out, start, rate=0.0, seed=0, step=0, counter=None, row_offset=0):
    N, T = codes.shape
    _check(lib().vqa_tf_mix(ptr(codes), ptr(amax), ptr(mask), ptr(out), N, T, start, rate, seed, step, row_offset,
                            ptr(counter), stream()), "vqa_tf_mix")


def attn_fwd(q, k, v, o, lse, mode, l, heads, scale, vbias=None):
    N, T, C = q.shape
    _check(lib().vqa_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(vbias), N, T, heads, C // heads, l, mode,
                              scale, dtype_code(q.dtype), stream()), "vqa_attn_fwd")


def attn_bwd(q, k, v, o, lse, dout, dsum, dq, dk, dv, mode, l, heads, scale):
    N, T, C = q.shape
    _check(lib().vqa_attn_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(dout), ptr(dsum), ptr(dq), ptr(dk),
                              ptr(dv), N, T, heads, C // heads, l, mode, scale, dtype_code(q.dtype), stream()),
           "vqa_attn_bwd")


def attn_weights_shape(N, T, H, l, mode):
    """The shape of vqa_attn_weights' output (include/vqa.h): (N*nb, H, l, l) for row (0) and previous-row (2)
    layers, (N*l, H, nb, nb) for column (1) layers, nb = T / l. Host-only."""
    N, T, H, l, mode = int(N), int(T), int(H), int(l), int(mode)
    if not (N > 0 and T > 0 and H > 0 and l > 0 and T % l == 0 and mode in (0, 1, 2)):
        raise VQAError(f"attn_weights: bad shape (N {N}, T {T}, H {H}, l {l}, mode {mode})")
    nb = T // l
    return (N * l, H, nb, nb) if mode == 1 else (N * nb, H, l, l)


def attn_weights(q, k, lse, mode, l, heads, scale, out=None):
    """Attention probabilities of attn_fwd on the same q, k (N, T, H*16) and the lse (N, T, H) it saved
    (vqa_attn_weights, include/vqa.h): an fp32 tensor of attn_weights_shape(N, T, H, l, mode), allocated here or the
    `out` given. Everything is checked on the host before the call."""
    if q.dtype not in (torch.float32, torch.bfloat16) or k.dtype != q.dtype:
        raise VQAError(f"attn_weights: q and k are both float32 or both bfloat16 (got {q.dtype}, {k.dtype})")
    if lse.dtype != torch.float32:
        raise VQAError(f"attn_weights: lse is float32 (got {lse.dtype})")
    heads = int(heads)
    if q.dim() != 3 or k.shape != q.shape or heads <= 0 or q.shape[2] % heads:
        raise VQAError(f"attn_weights: q and k are (N, T, H*head_dim) (got {tuple(q.shape)}, {tuple(k.shape)}, "
                       f"{heads} heads)")
    N, T, C = q.shape
    if tuple(lse.shape) != (N, T, heads):
        raise VQAError(f"attn_weights: lse is ({N}, {T}, {heads}) (got {tuple(lse.shape)})")
    shape = attn_weights_shape(N, T, heads, l, mode)
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != shape):
        raise VQAError(f"attn_weights: out is float32 {shape} (got {out.dtype} {tuple(out.shape)})")
    for name, t in (("q", q), ("k", k), ("lse", lse)) + ((("out", out),) if out is not None else ()):
        if not t.is_cuda:
            raise VQAError(f"attn_weights: {name} is a CPU tensor (device tensors only)")
        if not t.is_contiguous():
            raise VQAError(f"attn_weights: {name} is not contiguous (strides {t.stride()})")
        if t.device != q.device:
            raise VQAError(f"attn_weights: {name} is on {t.device}, q on {q.device}")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=q.device)
    _check(lib().vqa_attn_weights(ptr(q), ptr(k), ptr(lse), ptr(out), out.numel(), N, T, heads, C // heads, int(l),
                                  int(mode), float(scale), dtype_code(q.dtype), stream()), "vqa_attn_weights")
    return out


def head_wt(w, wt):
    K, V = w.shape
    _check(lib().vqa_head_wt(ptr(w), ptr(wt), K, V, dtype_code(wt.dtype), stream()), "vqa_head_wt")


def head_fwd(x, wt, bias, lse, amax=None, targets=None, loss_row=None, correct=None):
    K = x.shape[-1]
    M = x.numel() // K
    _check(lib().vqa_head_fwd(ptr(x), ptr(wt), ptr(bias), ptr(targets), ptr(lse), ptr(amax), ptr(loss_row),
                              ptr(correct), M, K, wt.shape[0], dtype_code(x.dtype), stream()), "vqa_head_fwd")


def head_bwd(x, wt, bias, targets, lse, inv_count, dx, dw, db, deferred=None):
    K = x.shape[-1]
    M = x.numel() // K
    V = wt.shape[0]
    ws = workspace(lib().vqa_head_bwd_workspace(M, K, V), x.device)
    d = PartialsDesc() if deferred is not None else None
    _check(lib().vqa_head_bwd(ptr(x), ptr(wt), ptr(bias), ptr(targets), ptr(lse), inv_count, ptr(dx), ptr(dw),
                              ptr(db), M, K, V, dtype_code(x.dtype), ptr(ws), ws.numel(),
                              ctypes.byref(d) if d is not None else None, stream()), "vqa_head_bwd")
    if deferred is not None:
        deferred.add(d, ws)


def rowsum(x, rows, n, scale, out):
    ws = workspace(lib().vqa_rowsum_workspace(rows, n), x.device)
    _check(lib().vqa_rowsum(ptr(x), rows, n, scale, ptr(out), ptr(ws), ws.numel(), stream()), "vqa_rowsum")


class PriorLayerDesc(ctypes.Structure):
    """vqa_prior_layer (include/vqa.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "ln1_gamma", "ln1_beta", "qkv_kernel", "qkv_bias", "query_kernel", "query_bias", "key_kernel", "key_bias",
        "value_kernel", "value_bias", "out_kernel", "out_bias", "proj_kernel", "proj_bias", "ln2_gamma", "ln2_beta",
        "mlp_kernel", "mlp_bias")] + [("attn_type", ctypes.c_int)]


# vqa_prior_decode's softmax scratch (VQA_DECODE_SCORE_FLOATS, include/vqa.h): `heads` rows of max(block length,
# blocks) floats must fit it, and a block is at most DECODE_MAX_BLOCK_LEN tokens
DECODE_SCORE_FLOATS = 4096
DECODE_MAX_BLOCK_LEN = 2048
# the decode kernel's compile-time shape (kDecW, kDecAW, kDecMaxLayers, vqa_prior_decode.hip): the entry point is told
# the model width and the depth, but not the attention width its layer descriptors describe
DECODE_WIDTH = 128
DECODE_ATTN_WIDTH = 32
DECODE_MAX_LAYERS = 8


def decode_shape_error(ctx, heads, blocks, width=DECODE_WIDTH, attn_width=DECODE_ATTN_WIDTH, depth=1) -> Optional[str]:
    """None if vqa_prior_decode accepts a model of this shape, else the rule it breaks (include/vqa.h). width: the
    model width; attn_width: int(width * m_attn), the width of the q / k / v heads that the layers' kernels hold —
    the kernel strides them as 32 columns whatever they are, so only this check can refuse another one."""
    if width != DECODE_WIDTH:
        return f"decode supports a model width of {DECODE_WIDTH} (got {width})"
    if attn_width != DECODE_ATTN_WIDTH:
        return (f"decode supports an attention width of {DECODE_ATTN_WIDTH} (width * m_attn; got {attn_width}): the "
                f"kernel reads every layer's q / k / v kernels as {DECODE_ATTN_WIDTH} columns")
    if not 1 <= depth <= DECODE_MAX_LAYERS:
        return f"decode supports a depth of 1 to {DECODE_MAX_LAYERS} layers (got {depth})"
    l = ctx // blocks
    if heads not in (1, 2, 4):
        return f"decode supports 1, 2 or 4 heads (got {heads})"
    if l > DECODE_MAX_BLOCK_LEN:
        return f"decode supports blocks of at most {DECODE_MAX_BLOCK_LEN} tokens (got {l})"
    if heads * max(l, blocks) > DECODE_SCORE_FLOATS:
        return (f"decode needs heads * max(block length, blocks) <= {DECODE_SCORE_FLOATS} "
                f"(got {heads} * max({l}, {blocks}))")
    return None


def prior_decode(layers, emb, pos, out_w, out_b, tokens, cache, steps, ctx, heads, blocks, start, seed, ycond=None,
                 xcond=None, forced=None, logits=None, bins=None, prime=None, temperature=1.0, top_k=0, top_p=1.0,
                 kept=None, logp_model=None, logp_draw=None):
    """out_w (width, ld) / out_b (ld,) with ld a multiple of 4 >= bins (zero-padded columns are never sampled).
    prime (N, P) int64: the first P next-input tokens (vqa_prior_decode_primed, include/vqa.h); temperature and
    top_k as there. The defaults run the unfiltered kernel. top_p < 1 (nucleus sampling) or kept ((N, steps) int32
    output: the bins that took part in each draw) go through vqa_prior_decode_filtered; without them the call is
    vqa_prior_decode_primed's, as before. logp_model / logp_draw ((N, steps) fp32 outputs: the log-probability of
    every written token under the model and under the distribution it was drawn from) go through
    vqa_prior_decode_scored."""
    N = tokens.shape[0]
    bins = out_w.shape[1] if bins is None else int(bins)
    arr = (PriorLayerDesc * len(layers))(*layers)
    prime_len = 0
    if prime is not None:
        if prime.dtype != torch.int64 or prime.dim() != 2 or prime.shape[0] != N:
            raise VQAError(f"prime must be ({N}, P) int64 (got {tuple(prime.shape)} {prime.dtype})")
        prime_len = int(prime.shape[1])
        if prime_len == 0:
            prime = None
    if kept is not None and (kept.dtype != torch.int32 or tuple(kept.shape) != (N, steps)
                             or not kept.is_contiguous()):
        raise VQAError(f"kept must be a contiguous ({N}, {steps}) int32 tensor "
                       f"(got {tuple(kept.shape)} {kept.dtype})")
    if logp_model is not None or logp_draw is not None:
        for name, t in (("logp_model", logp_model), ("logp_draw", logp_draw)):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (N, steps) or not t.is_contiguous()):
                raise VQAError(f"{name} must be a contiguous ({N}, {steps}) float32 tensor "
                               f"(got {tuple(t.shape)} {t.dtype})")
        _check(lib().vqa_prior_decode_scored(arr, len(layers), ptr(emb), ptr(pos), ptr(out_w), ptr(out_b),
                                             ptr(ycond), ptr(xcond), ptr(forced), ptr(logits), ptr(tokens),
                                             ptr(cache), cache.numel(), N, steps, ctx, emb.shape[1], heads, blocks,
                                             bins, out_w.shape[1], start, seed, ptr(prime), prime_len,
                                             float(temperature), int(top_k), float(top_p), ptr(kept),
                                             ptr(logp_model), ptr(logp_draw), stream()),
               "vqa_prior_decode_scored")
        return
    if float(top_p) != 1.0 or kept is not None:
        _check(lib().vqa_prior_decode_filtered(arr, len(layers), ptr(emb), ptr(pos), ptr(out_w), ptr(out_b),
                                               ptr(ycond), ptr(xcond), ptr(forced), ptr(logits), ptr(tokens),
                                               ptr(cache), cache.numel(), N, steps, ctx, emb.shape[1], heads, blocks,
                                               bins, out_w.shape[1], start, seed, ptr(prime), prime_len,
                                               float(temperature), int(top_k), float(top_p), ptr(kept), stream()),
               "vqa_prior_decode_filtered")
        return
    _check(lib().vqa_prior_decode_primed(arr, len(layers), ptr(emb), ptr(pos), ptr(out_w), ptr(out_b), ptr(ycond),
                                         ptr(xcond), ptr(forced), ptr(logits), ptr(tokens), ptr(cache),
                                         cache.numel(), N, steps, ctx, emb.shape[1], heads, blocks, bins,
                                         out_w.shape[1], start, seed, ptr(prime), prime_len, float(temperature),
                                         int(top_k), stream()),
           "vqa_prior_decode_primed")
