"""Conv kernel parity: libvqa (through the C-ABI) vs the CPU oracle's TF-semantics convs (fp64).

Covers every conv shape of the model (encdec.py:33,38,60,67-68,148; resnet.py:13,17) in all three
directions (forward, data-gradient, weight-gradient), with the fused ReLU / residual / ReLU'-mask flags,
fp32 (tolerance 2e-5 relative to the max magnitude) and bf16 (2e-2), plus ragged and tiny lengths.

Which kernel a conv runs is decided on the host (channel counts, taps, stride, dilation, dtype, epilogue
flags). The cases past the model's own shapes (width 64, dilation > 27) are there for the kernel they reach:
each states its routes in ROUTES, and every call asserts the route vqa_conv1d_route reports before it launches,
so a change to a dispatch threshold fails here instead of silently moving a case onto another kernel.
test_route_coverage (no GPU) holds the list of kernel variants the table has to reach.
"""
import numpy as np
import pytest
import torch

import vqa_lib as V
from oracle.vqvae_ref import conv1d as ref_conv, conv1d_transpose as ref_convT, same_pad

gpu = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2.5e-2}


_errors = []  # every error a test measured, in order (printed by the test; pytest -s shows it)


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    _errors.append(float((a - b).abs().max() / max(b.abs().max(), 1e-12)))
    return _errors[-1]


def _q(t, dt):
    """round to the activation dtype (what the kernel sees), back to fp64 for the reference"""
    return t.to(dt).double()


CONV_CASES = [
    # (C_in, C_out, K, stride, dilation, B, T)
    (1, 32, 4, 2, 1, 2, 1024),     # first encoder down conv (generic path, fp32 waveform in)
    (1, 32, 4, 2, 1, 1, 1537),     # ... ragged: last row block partial, SAME pad on both ends
    (1, 64, 3, 1, 3, 2, 700),      # one-input-channel kernel with 64 outputs, dilated
    (32, 32, 4, 2, 1, 2, 1000),    # down conv, ragged length
    (32, 32, 4, 2, 1, 1, 513),     # odd length: SAME pads (1, 2)
    (64, 32, 4, 2, 1, 3, 512),     # level>=1 first down conv
    (32, 32, 3, 1, 1, 2, 777),     # residual conv_b
    (32, 32, 3, 1, 3, 2, 1024),
    (32, 32, 3, 1, 9, 1, 300),
    (32, 32, 3, 1, 27, 2, 2048),
    (32, 32, 3, 1, 27, 1, 40),     # dilation halo wider than the signal
    (32, 64, 3, 1, 1, 2, 515),     # encoder projection
    (64, 32, 3, 1, 1, 2, 512),     # decoder pre-conv
    (64, 1, 3, 1, 1, 2, 1024),     # decoder output conv (row-dot kernels, fp32 out)
    (64, 1, 3, 1, 1, 3, 65536),    # ... at the cfg2 chunk length
    (32, 1, 3, 1, 1, 2, 700),      # ragged tile, 32 channels
    (64, 1, 3, 1, 3, 1, 300),      # dilated taps
    (64, 1, 2, 1, 1, 2, 513),      # even kernel: SAME pads (0, 1)
    (8, 32, 3, 1, 3, 2, 256),      # generic small widths
    (32, 8, 3, 1, 1, 2, 256),
    (128, 32, 3, 1, 1, 2, 64),     # ConditionerNet pre conv (embed width 128 -> residual width 32)
    (32, 128, 3, 1, 1, 2, 300),    # 128-channel output
    # ---- beyond the default architecture: width 64 and dilation > 27, one kernel variant each (ROUTES)
    (64, 64, 3, 1, 1, 2, 300),     # ragged last tile for 64- and 128-row tiles
    (64, 64, 3, 1, 3, 2, 515),
    (64, 64, 3, 1, 27, 1, 200),
    (64, 64, 3, 1, 27, 1, 40),     # halo wider than the signal
    (64, 64, 3, 1, 81, 2, 300),
    (64, 64, 3, 1, 243, 1, 700),
    (64, 64, 3, 1, 243, 1, 300),   # T < 2d: both outer taps out of range for a band of rows
    (64, 64, 4, 2, 1, 2, 513),     # width-64 down conv, odd length, pads (1, 2)
    (32, 32, 3, 1, 33, 2, 300),    # both ends of the bf16 range of the 5-chunk 32-channel kernel
    (32, 32, 3, 1, 96, 1, 515),
    (32, 32, 3, 1, 97, 1, 515),    # ... and the first dilation past it
    (32, 32, 3, 1, 81, 2, 1000),
    (32, 32, 3, 1, 243, 1, 700),
    (32, 64, 3, 1, 81, 1, 300),
    (64, 32, 3, 1, 81, 1, 300),
    # variants the route sweep of test_route_coverage finds reachable and the cases above do not reach
    (64, 32, 3, 1, 27, 1, 200),    # fp32 data gradient: 32-channel kernel, 64 outputs, 6 chunks
    (64, 32, 3, 1, 40, 1, 300),    # ... 9 chunks
    (32, 64, 3, 1, 100, 1, 300),   # bf16 forward past the 32-channel kernel: MFMA 32 -> 64 with 5 chunks
    (32, 64, 4, 2, 22, 1, 300),    # ... with 4 chunks: only a dilated stride-2 conv gets there (no data gradient)
    (32, 64, 1, 1, 1, 2, 300),     # 1x1 conv: bf16 data gradient is MFMA 64 -> 32 with exactly 4 chunks
]

DT_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def route_str(fam, det):
    """One kernel variant as a short string: the family and the template parameters that vary."""
    if fam == "conv32":
        return f"conv32 O{det['O']} PVX{det['PVX']} NEP{det['NEP']}" + (" FW" if det["FW"] else "")
    if fam == "gather_mfma":
        return f"gather_mfma C{det['C']} O{det['O']} PV{det['PV']}"
    if fam in ("wgrad_mfma", "wgrad_direct"):
        return f"{fam} C{det['C']} O{det['O']} TT{det['TT']}"
    if fam == "direct":
        return f"direct C{det['C']} O{det['O']}"
    if fam == "two_call":
        return f"two_call {det['data']}+{det['weight']}"
    return fam


def conv_calls(case, dt):
    """The library calls test_conv1d_fwd_bwd issues for `case`, as (tag, op, conv arguments): the tag names the
    op and its epilogue flags (m: ReLU' mask, r: residual). The ReLU on the input does not enter the dispatch."""
    Cin, Cout, K, s, d, B, T = case
    To, pl, _ = same_pad(T, K, s, d)
    fxy = 0
    if dt != torch.float32:
        fxy = (V.X_F32 if Cin == 1 else 0) | (V.Y_F32 if Cout == 1 else 0)
    args = (B, T, To, Cin, Cout, K, s, d, pl)
    calls = [("fwd_r" if (Cin == Cout and s == 1) else "fwd", V.OP_FWD, fxy | (V.ADD_RESIDUAL if Cin == Cout and s == 1 else 0))]
    if Cin > 1:
        calls += [("dgrad_mr", V.OP_BWD_DATA, fxy | V.POST_MASK | V.ADD_RESIDUAL), ("dgrad", V.OP_BWD_DATA, fxy),
                  ("dgrad_m", V.OP_BWD_DATA, fxy | V.POST_MASK)]
    calls.append(("wgrad", V.OP_BWD_WEIGHT, fxy))
    if Cin > 1:
        calls += [("fused_mr", V.OP_BWD_DATA_WEIGHT, fxy | V.PRE_RELU | V.ADD_RESIDUAL),
                  ("fused_m", V.OP_BWD_DATA_WEIGHT, fxy | V.PRE_RELU), ("fused", V.OP_BWD_DATA_WEIGHT, fxy)]
    return [(tag, op, args + (fl, V.dtype_code(dt))) for tag, op, fl in calls]


def convt_calls(case, dt):
    Cin, Cout, B, T = case
    args = (B, T, 2 * T, Cin, Cout, 4, 2, 1, 1)
    return [(tag, op, args + (fl, V.dtype_code(dt))) for tag, op, fl in
            (("t_fwd", V.OP_T_FWD, 0), ("t_dgrad_m", V.OP_T_BWD_DATA, V.POST_MASK), ("t_wgrad", V.OP_T_BWD_WEIGHT, 0))]


def route_of(op, args):
    try:
        return route_str(*V.conv1d_route(op, *args))
    except V.VQAError:  # the call itself is refused with the same code before anything is launched
        return "unsupported"


def routes_of(calls):
    return {tag: route_of(op, args) for tag, op, args in calls}


# The kernel variant every call of the cases past the model's own shapes reaches: {case: {dtype: {tag: route}}},
# tags as in conv_calls / convt_calls. test_conv1d_fwd_bwd / test_conv1d_transpose assert it before launching.
ROUTES = {
    (64, 64, 3, 1, 1, 2, 300): {
        "fp32": {"fwd_r": "gather_mfma C64 O64 PV12", "dgrad_mr": "direct C64 O64",
                 "dgrad": "gather_mfma C64 O64 PV5", "dgrad_m": "gather_mfma C64 O64 PV12",
                 "wgrad": "wgrad_mfma C64 O64 TT64", "fused_mr": "two_call direct+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C64 O64 PV5", "dgrad_mr": "gather_mfma C64 O64 PV8",
                 "dgrad": "gather_mfma C64 O64 PV3", "dgrad_m": "gather_mfma C64 O64 PV5",
                 "wgrad": "wgrad_mfma C64 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 64, 3, 1, 3, 2, 515): {
        "fp32": {"fwd_r": "gather_mfma C64 O64 PV12", "dgrad_mr": "direct C64 O64",
                 "dgrad": "gather_mfma C64 O64 PV5", "dgrad_m": "gather_mfma C64 O64 PV12",
                 "wgrad": "wgrad_mfma C64 O64 TT64", "fused_mr": "two_call direct+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C64 O64 PV5", "dgrad_mr": "gather_mfma C64 O64 PV8",
                 "dgrad": "gather_mfma C64 O64 PV3", "dgrad_m": "gather_mfma C64 O64 PV5",
                 "wgrad": "wgrad_mfma C64 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 64, 3, 1, 27, 1, 200): {
        "fp32": {"fwd_r": "gather_mfma C64 O64 PV12", "dgrad_mr": "direct C64 O64",
                 "dgrad": "gather_mfma C64 O64 PV8", "dgrad_m": "gather_mfma C64 O64 PV12",
                 "wgrad": "wgrad_mfma C64 O64 TT64", "fused_mr": "two_call direct+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C64 O64 PV8", "dgrad_mr": "gather_mfma C64 O64 PV8",
                 "dgrad": "gather_mfma C64 O64 PV4", "dgrad_m": "gather_mfma C64 O64 PV8",
                 "wgrad": "wgrad_mfma C64 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 64, 3, 1, 27, 1, 40): {
        "fp32": {"fwd_r": "gather_mfma C64 O64 PV12", "dgrad_mr": "direct C64 O64",
                 "dgrad": "gather_mfma C64 O64 PV8", "dgrad_m": "gather_mfma C64 O64 PV12",
                 "wgrad": "wgrad_mfma C64 O64 TT64", "fused_mr": "two_call direct+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C64 O64 PV8", "dgrad_mr": "gather_mfma C64 O64 PV8",
                 "dgrad": "gather_mfma C64 O64 PV4", "dgrad_m": "gather_mfma C64 O64 PV8",
                 "wgrad": "wgrad_mfma C64 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 64, 3, 1, 81, 2, 300): {
        "fp32": {"fwd_r": "direct C64 O64", "dgrad_mr": "direct C64 O64", "dgrad": "direct C64 O64",
                 "dgrad_m": "direct C64 O64", "wgrad": "wgrad_mfma C64 O64 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C64 O64 PV12", "dgrad_mr": "gather_mfma C64 O64 PV12",
                 "dgrad": "gather_mfma C64 O64 PV8", "dgrad_m": "gather_mfma C64 O64 PV12",
                 "wgrad": "wgrad_mfma C64 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 64, 3, 1, 243, 1, 700): {
        "fp32": {"fwd_r": "direct C64 O64", "dgrad_mr": "direct C64 O64", "dgrad": "direct C64 O64",
                 "dgrad_m": "direct C64 O64", "wgrad": "unsupported", "fused_mr": "unsupported",
                 "fused_m": "unsupported", "fused": "unsupported"},
        "bf16": {"fwd_r": "direct C64 O64", "dgrad_mr": "direct C64 O64", "dgrad": "direct C64 O64",
                 "dgrad_m": "direct C64 O64", "wgrad": "wgrad_mfma C64 O64 TT128",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
    },
    (64, 64, 3, 1, 243, 1, 300): {
        "fp32": {"fwd_r": "direct C64 O64", "dgrad_mr": "direct C64 O64", "dgrad": "direct C64 O64",
                 "dgrad_m": "direct C64 O64", "wgrad": "unsupported", "fused_mr": "unsupported",
                 "fused_m": "unsupported", "fused": "unsupported"},
        "bf16": {"fwd_r": "direct C64 O64", "dgrad_mr": "direct C64 O64", "dgrad": "direct C64 O64",
                 "dgrad_m": "direct C64 O64", "wgrad": "wgrad_mfma C64 O64 TT128",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
    },
    (64, 64, 4, 2, 1, 2, 513): {
        "fp32": {"fwd": "gather_mfma C64 O64 PV12", "dgrad_mr": "direct C64 O128", "dgrad": "direct C64 O128",
                 "dgrad_m": "direct C64 O128", "wgrad": "wgrad_mfma C64 O64 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
        "bf16": {"fwd": "gather_mfma C64 O64 PV5", "dgrad_mr": "gather_mfma C64 O128 PV12",
                 "dgrad": "gather_mfma C64 O128 PV3", "dgrad_m": "gather_mfma C64 O128 PV8",
                 "wgrad": "wgrad_mfma C64 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (32, 32, 3, 1, 33, 2, 300): {
        "fp32": {"fwd_r": "conv32 O32 PVX9 NEP1", "dgrad_mr": "conv32 O32 PVX9 NEP2", "dgrad": "conv32 O32 PVX9 NEP0",
                 "dgrad_m": "conv32 O32 PVX9 NEP1", "wgrad": "wgrad_mfma C32 O32 TT64",
                 "fused_mr": "conv32 O32 PVX9 NEP2 FW", "fused_m": "conv32 O32 PVX9 NEP1 FW",
                 "fused": "conv32 O32 PVX9 NEP1 FW"},
        "bf16": {"fwd_r": "conv32 O32 PVX5 NEP1", "dgrad_mr": "conv32 O32 PVX5 NEP2", "dgrad": "conv32 O32 PVX5 NEP0",
                 "dgrad_m": "conv32 O32 PVX5 NEP1", "wgrad": "wgrad_mfma C32 O32 TT128",
                 "fused_mr": "conv32 O32 PVX5 NEP2 FW", "fused_m": "conv32 O32 PVX5 NEP1 FW",
                 "fused": "conv32 O32 PVX5 NEP1 FW"},
    },
    (32, 32, 3, 1, 96, 1, 515): {
        "fp32": {"fwd_r": "direct C32 O32", "dgrad_mr": "direct C32 O32", "dgrad": "gather_mfma C32 O32 PV12",
                 "dgrad_m": "direct C32 O32", "wgrad": "wgrad_mfma C32 O32 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "conv32 O32 PVX5 NEP1", "dgrad_mr": "conv32 O32 PVX5 NEP2", "dgrad": "conv32 O32 PVX5 NEP0",
                 "dgrad_m": "conv32 O32 PVX5 NEP1", "wgrad": "wgrad_mfma C32 O32 TT128",
                 "fused_mr": "conv32 O32 PVX5 NEP2 FW", "fused_m": "conv32 O32 PVX5 NEP1 FW",
                 "fused": "conv32 O32 PVX5 NEP1 FW"},
    },
    (32, 32, 3, 1, 97, 1, 515): {
        "fp32": {"fwd_r": "direct C32 O32", "dgrad_mr": "direct C32 O32", "dgrad": "gather_mfma C32 O32 PV12",
                 "dgrad_m": "direct C32 O32", "wgrad": "wgrad_mfma C32 O32 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C32 O32 PV8", "dgrad_mr": "gather_mfma C32 O32 PV12",
                 "dgrad": "gather_mfma C32 O32 PV8", "dgrad_m": "gather_mfma C32 O32 PV8",
                 "wgrad": "wgrad_mfma C32 O32 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (32, 32, 3, 1, 81, 2, 1000): {
        "fp32": {"fwd_r": "direct C32 O32", "dgrad_mr": "direct C32 O32", "dgrad": "gather_mfma C32 O32 PV12",
                 "dgrad_m": "direct C32 O32", "wgrad": "wgrad_mfma C32 O32 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd_r": "conv32 O32 PVX5 NEP1", "dgrad_mr": "conv32 O32 PVX5 NEP2", "dgrad": "conv32 O32 PVX5 NEP0",
                 "dgrad_m": "conv32 O32 PVX5 NEP1", "wgrad": "wgrad_mfma C32 O32 TT128",
                 "fused_mr": "conv32 O32 PVX5 NEP2 FW", "fused_m": "conv32 O32 PVX5 NEP1 FW",
                 "fused": "conv32 O32 PVX5 NEP1 FW"},
    },
    (32, 32, 3, 1, 243, 1, 700): {
        "fp32": {"fwd_r": "direct C32 O32", "dgrad_mr": "direct C32 O32", "dgrad": "direct C32 O32",
                 "dgrad_m": "direct C32 O32", "wgrad": "wgrad_mfma C32 O32 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
        "bf16": {"fwd_r": "gather_mfma C32 O32 PV12", "dgrad_mr": "direct C32 O32",
                 "dgrad": "gather_mfma C32 O32 PV12", "dgrad_m": "gather_mfma C32 O32 PV12",
                 "wgrad": "wgrad_mfma C32 O32 TT128", "fused_mr": "two_call direct+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (32, 64, 3, 1, 81, 1, 300): {
        "fp32": {"fwd": "gather_mfma C32 O64 PV8", "dgrad_mr": "direct C64 O32", "dgrad": "direct C64 O32",
                 "dgrad_m": "direct C64 O32", "wgrad": "wgrad_mfma C32 O64 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
        "bf16": {"fwd": "conv32 O64 PVX5 NEP0", "dgrad_mr": "direct C64 O32", "dgrad": "gather_mfma C64 O32 PV12",
                 "dgrad_m": "gather_mfma C64 O32 PV12", "wgrad": "wgrad_mfma C32 O64 TT128",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call gather_mfma+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 32, 3, 1, 81, 1, 300): {
        "fp32": {"fwd": "direct C64 O32", "dgrad_mr": "direct C32 O64", "dgrad": "gather_mfma C32 O64 PV8",
                 "dgrad_m": "gather_mfma C32 O64 PV12", "wgrad": "wgrad_mfma C64 O32 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call gather_mfma+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd": "gather_mfma C64 O32 PV12", "dgrad_mr": "conv32 O64 PVX5 NEP2",
                 "dgrad": "conv32 O64 PVX5 NEP0", "dgrad_m": "conv32 O64 PVX5 NEP1",
                 "wgrad": "wgrad_mfma C64 O32 TT128", "fused_mr": "two_call conv32+wgrad_mfma",
                 "fused_m": "two_call conv32+wgrad_mfma", "fused": "two_call conv32+wgrad_mfma"},
    },
    (64, 32, 3, 1, 27, 1, 200): {
        "fp32": {"fwd": "gather_mfma C64 O32 PV12", "dgrad_mr": "conv32 O64 PVX6 NEP2",
                 "dgrad": "conv32 O64 PVX6 NEP0", "dgrad_m": "conv32 O64 PVX6 NEP1",
                 "wgrad": "wgrad_mfma C64 O32 TT64", "fused_mr": "two_call conv32+wgrad_mfma",
                 "fused_m": "two_call conv32+wgrad_mfma", "fused": "two_call conv32+wgrad_mfma"},
        "bf16": {"fwd": "gather_mfma C64 O32 PV8", "dgrad_mr": "conv32 O64 PVX3 NEP2",
                 "dgrad": "conv32 O64 PVX3 NEP0", "dgrad_m": "conv32 O64 PVX3 NEP1",
                 "wgrad": "wgrad_mfma C64 O32 TT128", "fused_mr": "two_call conv32+wgrad_mfma",
                 "fused_m": "two_call conv32+wgrad_mfma", "fused": "two_call conv32+wgrad_mfma"},
    },
    (64, 32, 3, 1, 40, 1, 300): {
        "fp32": {"fwd": "direct C64 O32", "dgrad_mr": "conv32 O64 PVX9 NEP2", "dgrad": "conv32 O64 PVX9 NEP0",
                 "dgrad_m": "conv32 O64 PVX9 NEP1", "wgrad": "wgrad_mfma C64 O32 TT64",
                 "fused_mr": "two_call conv32+wgrad_mfma", "fused_m": "two_call conv32+wgrad_mfma",
                 "fused": "two_call conv32+wgrad_mfma"},
        "bf16": {"fwd": "gather_mfma C64 O32 PV8", "dgrad_mr": "conv32 O64 PVX5 NEP2",
                 "dgrad": "conv32 O64 PVX5 NEP0", "dgrad_m": "conv32 O64 PVX5 NEP1",
                 "wgrad": "wgrad_mfma C64 O32 TT128", "fused_mr": "two_call conv32+wgrad_mfma",
                 "fused_m": "two_call conv32+wgrad_mfma", "fused": "two_call conv32+wgrad_mfma"},
    },
    (32, 64, 3, 1, 100, 1, 300): {
        "fp32": {"fwd": "gather_mfma C32 O64 PV12", "dgrad_mr": "direct C64 O32", "dgrad": "direct C64 O32",
                 "dgrad_m": "direct C64 O32", "wgrad": "wgrad_mfma C32 O64 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call direct+wgrad_mfma"},
        "bf16": {"fwd": "gather_mfma C32 O64 PV5", "dgrad_mr": "direct C64 O32", "dgrad": "gather_mfma C64 O32 PV12",
                 "dgrad_m": "direct C64 O32", "wgrad": "wgrad_mfma C32 O64 TT128",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call direct+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (32, 64, 4, 2, 22, 1, 300): {
        "fp32": {"fwd": "gather_mfma C32 O64 PV8", "dgrad_mr": "unsupported", "dgrad": "unsupported",
                 "dgrad_m": "unsupported", "wgrad": "wgrad_mfma C32 O64 TT64", "fused_mr": "unsupported",
                 "fused_m": "unsupported", "fused": "unsupported"},
        "bf16": {"fwd": "gather_mfma C32 O64 PV4", "dgrad_mr": "unsupported", "dgrad": "unsupported",
                 "dgrad_m": "unsupported", "wgrad": "wgrad_mfma C32 O64 TT128", "fused_mr": "unsupported",
                 "fused_m": "unsupported", "fused": "unsupported"},
    },
    (32, 64, 1, 1, 1, 2, 300): {
        "fp32": {"fwd": "conv32 O64 PVX5 NEP0", "dgrad_mr": "direct C64 O32", "dgrad": "gather_mfma C64 O32 PV8",
                 "dgrad_m": "gather_mfma C64 O32 PV12", "wgrad": "wgrad_mfma C32 O64 TT64",
                 "fused_mr": "two_call direct+wgrad_mfma", "fused_m": "two_call gather_mfma+wgrad_mfma",
                 "fused": "two_call gather_mfma+wgrad_mfma"},
        "bf16": {"fwd": "conv32 O64 PVX3 NEP0", "dgrad_mr": "gather_mfma C64 O32 PV8",
                 "dgrad": "gather_mfma C64 O32 PV4", "dgrad_m": "gather_mfma C64 O32 PV8",
                 "wgrad": "wgrad_mfma C32 O64 TT128", "fused_mr": "two_call gather_mfma+wgrad_mfma",
                 "fused_m": "two_call gather_mfma+wgrad_mfma", "fused": "two_call gather_mfma+wgrad_mfma"},
    },
    (64, 64, 2, 300): {
        "fp32": {"t_fwd": "direct C64 O128", "t_dgrad_m": "direct C64 O64", "t_wgrad": "wgrad_mfma C64 O64 TT64"},
        "bf16": {"t_fwd": "gather_mfma C64 O128 PV3", "t_dgrad_m": "gather_mfma C64 O64 PV8",
                 "t_wgrad": "wgrad_mfma C64 O64 TT128"},
    },
    (64, 64, 1, 37): {
        "fp32": {"t_fwd": "direct C64 O128", "t_dgrad_m": "direct C64 O64", "t_wgrad": "wgrad_mfma C64 O64 TT64"},
        "bf16": {"t_fwd": "gather_mfma C64 O128 PV3", "t_dgrad_m": "gather_mfma C64 O64 PV8",
                 "t_wgrad": "wgrad_mfma C64 O64 TT128"},
    },
}


def check_routes(case, dt, calls):
    """The routes of this case's calls; equal to the ones ROUTES pins for it."""
    got = routes_of(calls)
    if case in ROUTES:
        assert got == ROUTES[case][DT_NAME[dt]], f"{case} {DT_NAME[dt]}: the dispatch moved this case to another kernel"
    return got


@gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv1d_fwd_bwd(cuda, case, dt):
    Cin, Cout, K, s, d, B, T = case
    routes = check_routes(case, dt, conv_calls(case, dt))
    del _errors[:]
    g = torch.Generator().manual_seed(hash(case) % 2**31)
    x = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    W = torch.randn(K, Cin, Cout, generator=g, dtype=torch.float64) / np.sqrt(K * Cin)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    To, pl, _ = same_pad(T, K, s, d)
    dy = torch.randn(B, To, Cout, generator=g, dtype=torch.float64)
    xdt = torch.float32 if Cin == 1 else dt   # waveform side is fp32
    ydt = torch.float32 if Cout == 1 else dt
    flags_x = V.X_F32 if (xdt == torch.float32 and dt != torch.float32) else 0
    flags_y = V.Y_F32 if (ydt == torch.float32 and dt != torch.float32) else 0
    cd = V.dtype_code(dt)
    xq, dyq = _q(x, xdt), _q(dy, ydt)
    Wq = W.float().double()
    bq = b.float().double()
    Wd, bd = W.float().to(cuda), b.float().to(cuda)
    xd, dyd = x.to(xdt).to(cuda), dy.to(ydt).to(cuda)
    tol = TOL[dt]

    for pre_relu in (False, True):
        # forward, optional residual when shapes allow
        use_res = (Cin == Cout and s == 1)
        res = torch.randn(B, To, Cout, generator=g, dtype=torch.float64) if use_res else None
        y = torch.empty(B, To, Cout, dtype=ydt, device=cuda)
        fl = flags_x | flags_y | (V.PRE_RELU if pre_relu else 0) | (V.ADD_RESIDUAL if use_res else 0)
        V.conv1d_fwd(xd, Wd, bd, res.to(ydt).to(cuda) if use_res else None, y, B, T, To, Cin, Cout, K, s, d, pl,
                     fl, cd)
        xin = torch.relu(xq) if pre_relu else xq
        ref = ref_conv(xin, Wq, bq, s, d)
        if use_res:
            ref = _q(res, ydt) + ref
        assert _rel(y, ref) < tol, f"fwd pre_relu={pre_relu}"

    # a call the library refuses (VQA_E_UNSUPPORTED before any launch; the route query says which) must raise
    def refused(fn, *a):
        with pytest.raises(V.VQAError, match=r"\(-2\)"):
            fn(*a)

    # data gradient (with ReLU' mask = x and a residual)
    if Cin > 1 and routes["dgrad"] == "unsupported":
        assert routes["dgrad_mr"] == routes["dgrad_m"] == "unsupported"
        refused(V.conv1d_bwd_data, dyd, Wd, None, None, torch.empty(B, T, Cin, dtype=xdt, device=cuda), B, T, To, Cin,
                Cout, K, s, d, pl, flags_x | flags_y, cd)
    elif Cin > 1:
        xv = xq.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((ref_conv(xv, Wq, bq, s, d) * dyq).sum(), xv)
        resid = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
        dx = torch.empty(B, T, Cin, dtype=xdt, device=cuda)
        V.conv1d_bwd_data(dyd, Wd, xd, resid.to(xdt).to(cuda), dx, B, T, To, Cin, Cout, K, s, d, pl,
                          flags_x | flags_y | V.POST_MASK | V.ADD_RESIDUAL, cd)
        ref = _q(resid, xdt) + torch.where(xq > 0, gx, torch.zeros_like(gx))
        assert _rel(dx, ref) < tol, "bwd_data"
        dx2 = torch.empty(B, T, Cin, dtype=xdt, device=cuda)
        V.conv1d_bwd_data(dyd, Wd, None, None, dx2, B, T, To, Cin, Cout, K, s, d, pl, flags_x | flags_y, cd)
        assert _rel(dx2, gx) < tol, "bwd_data plain"

    # weight gradient (pre-ReLU on x)
    for pre_relu in (False, True):
        Wv = Wq.clone().requires_grad_(True)
        bv = bq.clone().requires_grad_(True)
        xin = torch.relu(xq) if pre_relu else xq
        gW, gb = torch.autograd.grad((ref_conv(xin, Wv, bv, s, d) * dyq).sum(), (Wv, bv))
        dW = torch.empty(K, Cin, Cout, dtype=torch.float32, device=cuda)
        db = torch.empty(Cout, dtype=torch.float32, device=cuda)
        if routes["wgrad"] == "unsupported":
            refused(V.conv1d_bwd_weight, xd, dyd, dW, db, B, T, To, Cin, Cout, K, s, d, pl,
                    flags_x | flags_y | (V.PRE_RELU if pre_relu else 0), cd)
            continue
        V.conv1d_bwd_weight(xd, dyd, dW, db, B, T, To, Cin, Cout, K, s, d, pl,
                            flags_x | flags_y | (V.PRE_RELU if pre_relu else 0), cd)
        assert _rel(dW, gW) < tol * 2, f"bwd_weight dW pre_relu={pre_relu}"
        assert _rel(db, gb) < tol * 2, "bwd_weight db"

    # fused data + weight gradient (vqa_conv1d_bwd_data_weight): one kernel for the stride-1 32-channel
    # convs, the two-call fallback elsewhere; dx must equal the plain data-gradient call bit for bit
    if Cin > 1:
        for pre_relu, use_res, deferred in ((True, True, False), (True, False, True), (False, False, False)):
            Wv = Wq.clone().requires_grad_(True)
            bv = bq.clone().requires_grad_(True)
            xv = xq.clone().requires_grad_(True)
            xin = torch.relu(xv) if pre_relu else xv
            gx, gW, gb = torch.autograd.grad((ref_conv(xin, Wv, bv, s, d) * dyq).sum(), (xv, Wv, bv))
            resid = torch.randn(B, T, Cin, generator=g, dtype=torch.float64) if use_res else None
            rd = resid.to(xdt).to(cuda) if use_res else None
            dx = torch.empty(B, T, Cin, dtype=xdt, device=cuda)
            dW = torch.full((K, Cin, Cout), float("nan"), dtype=torch.float32, device=cuda)
            db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=cuda)
            fl = flags_x | flags_y | (V.PRE_RELU if pre_relu else 0) | (V.ADD_RESIDUAL if use_res else 0)
            dfr = V.Deferred() if deferred else None
            if routes["fused_mr" if use_res else ("fused_m" if pre_relu else "fused")] == "unsupported":
                refused(V.conv1d_bwd_data_weight, dyd, Wd, xd, rd, dx, dW, db, B, T, To, Cin, Cout, K, s, d, pl, fl, cd,
                        dfr)
                continue
            V.conv1d_bwd_data_weight(dyd, Wd, xd, rd, dx, dW, db, B, T, To, Cin, Cout, K, s, d, pl, fl, cd, dfr)
            if dfr is not None:
                dfr.flush()
            ref = gx + (_q(resid, xdt) if use_res else 0)
            tag = f"fused pre_relu={pre_relu} res={use_res} deferred={deferred}"
            assert _rel(dx, ref) < tol, f"{tag}: dx"
            assert _rel(dW, gW) < tol * 2, f"{tag}: dW"
            assert _rel(db, gb) < tol * 2, f"{tag}: db"
            dx_plain = torch.empty_like(dx)
            V.conv1d_bwd_data(dyd, Wd, xd if pre_relu else None, rd, dx_plain, B, T, To, Cin, Cout, K, s, d, pl,
                              flags_x | flags_y | (V.POST_MASK if pre_relu else 0) | (V.ADD_RESIDUAL if use_res else 0),
                              cd)
            assert torch.equal(dx, dx_plain), f"{tag}: dx differs from vqa_conv1d_bwd_data"
    print(f"conv {case} {DT_NAME[dt]}: worst error {max(_errors):.2e} over {len(_errors)} checks "
          f"(bound {tol:.1e}; dW, db {2 * tol:.1e})")


CONVT_CASES = [
    # (C_in, C_out, B, T_in)
    (32, 32, 2, 512),
    (32, 64, 2, 300),   # last up conv maps to latent width
    (32, 32, 1, 37),
    (32, 8, 2, 128),    # generic path
    (64, 32, 2, 256),
    (32, 128, 2, 64),   # ConditionerNet last up conv (residual width 32 -> embed width 128)
    (64, 64, 2, 300),   # width-64 up conv: the PAIR layout with 128 gather outputs
    (64, 64, 1, 37),
]


@gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONVT_CASES)
def test_conv1d_transpose(cuda, case, dt):
    Cin, Cout, B, T = case
    check_routes(case, dt, convt_calls(case, dt))
    del _errors[:]
    K, s = 4, 2
    g = torch.Generator().manual_seed(1000 + hash(case) % 2**31)
    x = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    W = torch.randn(K, Cout, Cin, generator=g, dtype=torch.float64) / np.sqrt(K * Cin)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    To = s * T
    _, pl, _ = same_pad(To, K, s, 1)
    assert pl == 1
    dy = torch.randn(B, To, Cout, generator=g, dtype=torch.float64)
    cd = V.dtype_code(dt)
    xq, dyq, Wq, bq = _q(x, dt), _q(dy, dt), W.float().double(), b.float().double()
    xd, dyd, Wd, bd = x.to(dt).to(cuda), dy.to(dt).to(cuda), W.float().to(cuda), b.float().to(cuda)
    tol = TOL[dt]

    y = torch.empty(B, To, Cout, dtype=dt, device=cuda)
    V.conv1d_transpose_fwd(xd, Wd, bd, None, y, B, T, To, Cin, Cout, K, s, pl, 0, cd)
    assert _rel(y, ref_convT(xq, Wq, bq, s)) < tol, "convT fwd"

    xv = xq.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad((ref_convT(xv, Wq, bq, s) * dyq).sum(), xv)
    dx = torch.empty(B, T, Cin, dtype=dt, device=cuda)
    V.conv1d_transpose_bwd_data(dyd, Wd, xd, None, dx, B, T, To, Cin, Cout, K, s, pl, V.POST_MASK, cd)
    assert _rel(dx, torch.where(xq > 0, gx, torch.zeros_like(gx))) < tol, "convT bwd_data"

    Wv, bv = Wq.clone().requires_grad_(True), bq.clone().requires_grad_(True)
    gW, gb = torch.autograd.grad((ref_convT(xq, Wv, bv, s) * dyq).sum(), (Wv, bv))
    dW = torch.empty(K, Cout, Cin, dtype=torch.float32, device=cuda)
    db = torch.empty(Cout, dtype=torch.float32, device=cuda)
    V.conv1d_transpose_bwd_weight(xd, dyd, dW, db, B, T, To, Cin, Cout, K, s, pl, 0, cd)
    assert _rel(dW, gW) < tol * 2, "convT dW"
    assert _rel(db, gb) < tol * 2, "convT db"
    print(f"convT {case} {DT_NAME[dt]}: worst error {max(_errors):.2e} over {len(_errors)} checks "
          f"(bound {tol:.1e}; dW, db {2 * tol:.1e})")


@gpu
def test_conv_rejects_bad_args(cuda):
    x = torch.zeros(1, 16, 32, device=cuda)
    W = torch.zeros(3, 32, 32, device=cuda)
    y = torch.zeros(1, 16, 32, device=cuda)
    with pytest.raises(V.VQAError, match="T_out"):
        V.conv1d_fwd(x, W, None, None, y, 1, 16, 15, 32, 32, 3, 1, 1, 1, 0, V.F32)
    with pytest.raises(V.VQAError, match="mask"):
        V.conv1d_bwd_data(y, W, None, None, x, 1, 16, 16, 32, 32, 3, 1, 1, 1, V.POST_MASK, V.F32)
    with pytest.raises(V.VQAError, match="stride 2"):
        V.conv1d_transpose_fwd(x, W, None, None, y, 1, 16, 48, 32, 32, 3, 3, 1, 0, V.F32)


# Every variant of the two MFMA conv kernels the dispatch can reach from a conv or transposed conv with 32 or 64
# channels on either side, K <= 4, stride <= 2, dilation <= 243, any epilogue flags, fp32 or bf16 (conv32: output
# channels, x chunks per thread, epilogue tensors, fused weight gradient; gather_mfma: gather input / output channels
# (128: the PAIR layout), chunks per thread), as test_route_coverage's sweep of the route query finds them.
REACHABLE = [
    "conv32 O32 PVX3 NEP0", "conv32 O32 PVX3 NEP1", "conv32 O32 PVX3 NEP1 FW", "conv32 O32 PVX3 NEP2",
    "conv32 O32 PVX3 NEP2 FW", "conv32 O32 PVX5 NEP0", "conv32 O32 PVX5 NEP1", "conv32 O32 PVX5 NEP1 FW",
    "conv32 O32 PVX5 NEP2", "conv32 O32 PVX5 NEP2 FW", "conv32 O32 PVX6 NEP0", "conv32 O32 PVX6 NEP1",
    "conv32 O32 PVX6 NEP1 FW", "conv32 O32 PVX6 NEP2", "conv32 O32 PVX6 NEP2 FW", "conv32 O32 PVX9 NEP0",
    "conv32 O32 PVX9 NEP1", "conv32 O32 PVX9 NEP1 FW", "conv32 O32 PVX9 NEP2", "conv32 O32 PVX9 NEP2 FW",
    "conv32 O64 PVX3 NEP0", "conv32 O64 PVX3 NEP1", "conv32 O64 PVX3 NEP2", "conv32 O64 PVX5 NEP0",
    "conv32 O64 PVX5 NEP1", "conv32 O64 PVX5 NEP2", "conv32 O64 PVX6 NEP0", "conv32 O64 PVX6 NEP1",
    "conv32 O64 PVX6 NEP2", "conv32 O64 PVX9 NEP0", "conv32 O64 PVX9 NEP1", "conv32 O64 PVX9 NEP2",
    "gather_mfma C32 O128 PV12", "gather_mfma C32 O128 PV3", "gather_mfma C32 O128 PV8", "gather_mfma C32 O32 PV12",
    "gather_mfma C32 O32 PV8", "gather_mfma C32 O64 PV12", "gather_mfma C32 O64 PV4", "gather_mfma C32 O64 PV5",
    "gather_mfma C32 O64 PV8", "gather_mfma C64 O128 PV12", "gather_mfma C64 O128 PV3", "gather_mfma C64 O128 PV8",
    "gather_mfma C64 O32 PV12", "gather_mfma C64 O32 PV4", "gather_mfma C64 O32 PV5", "gather_mfma C64 O32 PV8",
    "gather_mfma C64 O64 PV12", "gather_mfma C64 O64 PV3", "gather_mfma C64 O64 PV4", "gather_mfma C64 O64 PV5",
    "gather_mfma C64 O64 PV8",
]


def _sweep_reachable():
    found = set()
    T = 300
    for cd in (V.F32, V.BF16):
        for Cin in (32, 64):
            for Cout in (32, 64):
                for K in (1, 2, 3, 4):
                    for s in (1, 2):
                        for d in range(1, 244):
                            a = (1, T, V.same_out_len(T, s), Cin, Cout, K, s, d, V.same_pad_left(T, K, s, d))
                            for fl in (0, V.ADD_RESIDUAL):
                                found.add(route_of(V.OP_FWD, a + (fl, cd)))
                                found.add(route_of(V.OP_BWD_DATA, a + (fl, cd)))
                                found.add(route_of(V.OP_BWD_DATA, a + (fl | V.POST_MASK, cd)))
                                found.add(route_of(V.OP_BWD_DATA_WEIGHT, a + (fl, cd)))
                                found.add(route_of(V.OP_BWD_DATA_WEIGHT, a + (fl | V.PRE_RELU, cd)))
                a = (1, T, 2 * T, Cin, Cout, 4, 2, 1, 1)
                for fl in (0, V.ADD_RESIDUAL):
                    found.add(route_of(V.OP_T_FWD, a + (fl, cd)))
                    found.add(route_of(V.OP_T_BWD_DATA, a + (fl, cd)))
                    found.add(route_of(V.OP_T_BWD_DATA, a + (fl | V.POST_MASK, cd)))
    return found


def test_route_coverage():
    """The case tables reach every variant of the MFMA conv kernels the dispatch can produce (no GPU needed).

    REACHABLE is what a sweep of vqa_conv1d_route over the whole range finds; the sweep is repeated here, so a
    dispatch change that adds or removes a variant fails until the list (and a case for it) follows. The routes of
    every call test_conv1d_fwd_bwd / test_conv1d_transpose issue over CONV_CASES / CONVT_CASES must include all of
    it, the generic VALU kernel reached from 32- and 64-channel convs, and the two-call form of the fused gradient
    (with an MFMA, a 32-channel-kernel and a generic data gradient).

    Variants the launchers hold and no shape in the range reaches (absent from REACHABLE): conv32 with O = 64 and
    the fused weight gradient does not exist (static_assert). gather_mfma PV 3 / 4 / 5 for C = O = 32, PV 3 for
    32 -> 64 and for 64 -> 32, PV 4 / 5 for the 128-output PAIR tiles: every tile that small is taken by conv32
    first, or (PAIR, 3 taps at dilation 1) has one size without and one with epilogue tensors and nothing between.
    fp32 64 -> 128 (PAIR: the width-64 transposed conv and stride-2 data gradient) does not fit the LDS and runs the
    generic kernel. fp32 64 -> 64 at dilation 243 has no weight gradient (the staged input span exceeds the LDS): the
    library
    refuses it before launching, which test_conv1d_fwd_bwd asserts."""
    reach = {r for r in _sweep_reachable() if r.startswith(("conv32", "gather_mfma"))}
    assert reach == set(REACHABLE), (sorted(reach - set(REACHABLE)), sorted(set(REACHABLE) - reach))
    covered = set()
    for dt in (torch.float32, torch.bfloat16):
        for case in CONV_CASES:
            covered |= set(routes_of(conv_calls(case, dt)).values())
        for case in CONVT_CASES:
            covered |= set(routes_of(convt_calls(case, dt)).values())
    want = set(REACHABLE) | {"direct C32 O32", "direct C64 O64", "direct C64 O32", "direct C32 O64", "direct C64 O128",
                             "two_call gather_mfma+wgrad_mfma", "two_call conv32+wgrad_mfma",
                             "two_call direct+wgrad_mfma", "wgrad_mfma C64 O64 TT64", "wgrad_mfma C64 O64 TT128"}
    assert want <= covered, sorted(want - covered)
    # every case past the model's own shapes pins its routes
    first_new = CONV_CASES.index((64, 64, 3, 1, 1, 2, 300))
    assert set(CONV_CASES[first_new:]) | {c for c in CONVT_CASES if c[:2] == (64, 64)} == set(ROUTES)


CROSS_CASES = [
    # convs whose data gradient changes kernel family with the epilogue flags (C_in, C_out, K, s, d, B, T)
    (32, 32, 3, 1, 243, 1, 700),   # bf16: MFMA plain and with the mask, generic with mask + residual
    (32, 32, 3, 1, 96, 1, 515),    # fp32: MFMA plain, generic with any epilogue tensor
    (32, 64, 3, 1, 81, 1, 300),    # bf16: MFMA 64 -> 32 plain / mask, generic with both
    (64, 64, 3, 1, 27, 1, 200),    # fp32: MFMA 8 and 12 chunks, generic with both
    (64, 64, 4, 2, 1, 2, 513),     # stride 2 (PAIR layout): bf16 MFMA 3 / 8 / 12 chunks; fp32 generic throughout
]


@gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CROSS_CASES)
def test_data_gradient_across_routes(cuda, case, dt):
    """The data gradient with no epilogue, with the ReLU' mask, with the residual and with both — up to three
    different kernels for one conv — each against fp64, and against each other:
    dx(mask + residual) = where(mask > 0, dx(plain), 0) + residual.
    Bound of the identity, per element: both sides were rounded to the activation dtype once (round to nearest,
    unit roundoff u = 2^-p for p significant bits: 2^-8 bf16, 2^-24 fp32, relative to the value rounded — the
    stored dx(plain) and the result), and the two kernels' fp32 accumulations each stay within the fp32 bound of
    this file (2e-5 of the largest gradient)."""
    Cin, Cout, K, s, d, B, T = case
    calls = {tag: (op, args) for tag, op, args in conv_calls(case, dt)}
    fams = {tag: route_of(*calls[tag]).split()[0] for tag in ("dgrad", "dgrad_m", "dgrad_mr")}
    g = torch.Generator().manual_seed(77 + hash(case) % 2**31)
    x = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    W = (torch.randn(K, Cin, Cout, generator=g, dtype=torch.float64) / np.sqrt(K * Cin)).float()
    To, pl, _ = same_pad(T, K, s, d)
    dy = torch.randn(B, To, Cout, generator=g, dtype=torch.float64)
    resid = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    cd = V.dtype_code(dt)
    xq, dyq, rq = _q(x, dt), _q(dy, dt), _q(resid, dt)
    xv = xq.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad((ref_conv(xv, W.double(), torch.zeros(Cout, dtype=torch.float64), s, d) * dyq).sum(), xv)
    Wd, xd, dyd, rd = W.to(cuda), x.to(dt).to(cuda), dy.to(dt).to(cuda), resid.to(dt).to(cuda)
    out = {}
    for tag, mask, res in (("plain", False, False), ("m", True, False), ("r", False, True), ("mr", True, True)):
        dx = torch.empty(B, T, Cin, dtype=dt, device=cuda)
        V.conv1d_bwd_data(dyd, Wd, xd if mask else None, rd if res else None, dx, B, T, To, Cin, Cout, K, s, d, pl,
                          (V.POST_MASK if mask else 0) | (V.ADD_RESIDUAL if res else 0), cd)
        ref = torch.where(xq > 0, gx, torch.zeros_like(gx)) if mask else gx
        ref = ref + rq if res else ref
        err = _rel(dx, ref)
        print(f"{case} {DT_NAME[dt]} dx({tag}): {err:.3e} (bound {TOL[dt]:.1e})")
        assert err < TOL[dt], f"dx({tag})"
        out[tag] = dx.double().cpu()
    u = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -24
    noise = 2 * TOL[torch.float32] * float(gx.abs().max())
    for tag, mask, res in (("m", True, False), ("r", False, True), ("mr", True, True)):
        want = torch.where(xq > 0, out["plain"], torch.zeros_like(gx)) if mask else out["plain"]
        want = want + rq if res else want
        bound = u * (out["plain"].abs() + want.abs()) + noise
        over = ((out[tag] - want).abs() - bound).max()
        print(f"{case} {DT_NAME[dt]} dx({tag}) against dx(plain): worst |difference| - bound = {float(over):.3e}")
        assert over <= 0, f"dx({tag}) against dx(plain): {float(over):.3e} over the bound ({fams})"
    if DT_NAME[dt] in CROSS_FAMILIES[case]:
        assert len(set(fams.values())) > 1, f"{fams}: the epilogue flags no longer change the kernel family"


# the dtypes at which the flags of a CROSS_CASES conv change its data gradient's kernel family
CROSS_FAMILIES = {
    (32, 32, 3, 1, 243, 1, 700): ("bf16",),
    (32, 32, 3, 1, 96, 1, 515): ("fp32",),
    (32, 64, 3, 1, 81, 1, 300): ("bf16",),
    (64, 64, 3, 1, 27, 1, 200): ("fp32",),
    (64, 64, 4, 2, 1, 2, 513): (),
}
