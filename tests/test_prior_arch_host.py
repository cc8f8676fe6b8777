"""CPU-only side of tests/test_gpu_prior_arch.py: the host guards of the prior's architecture matrix (what sample()
and the constructor refuse before a pointer reaches the device, and what the sequence-linear entry points accept of
an attention width of 16), the power of the GPU cases to tell architectures apart, and the sinusoid table."""
import ctypes
import math

import numpy as np
import pytest
import torch

import vqa_lib as V
from oracle import prior_ref as P
from prior import FMHABasedAutoregressiveModel, positional_encoding
from test_gpu_prior import DECODE_SHAPES

PTR = ctypes.c_void_p(0x1000)
F32, BF16 = 0, 1


# ------------------------------------------------------------------ decode_shape_error
def test_decode_shape_error_names_every_rule():
    ok = (256, 2, 4)
    assert V.decode_shape_error(*ok) is None
    assert V.decode_shape_error(*ok, 128, 32, 1) is None and V.decode_shape_error(*ok, 128, 32, 8) is None
    assert V.decode_shape_error(*ok, width=128, attn_width=32, depth=3) is None
    for width in (64, 256):
        assert V.decode_shape_error(*ok, width, 32, 3) == f"decode supports a model width of 128 (got {width})"
    for aw in (16, 64):
        why = V.decode_shape_error(*ok, 128, aw, 3)
        assert why.startswith(f"decode supports an attention width of 32 (width * m_attn; got {aw})")
    for depth in (0, 9, -1):
        assert V.decode_shape_error(*ok, 128, 32, depth) == f"decode supports a depth of 1 to 8 layers (got {depth})"
    # the rules of the score scratch keep their texts, with the new parameters given or not
    assert V.decode_shape_error(64, 8, 1) == "decode supports 1, 2 or 4 heads (got 8)"
    assert V.decode_shape_error(64, 8, 1, 128, 32, 8) == "decode supports 1, 2 or 4 heads (got 8)"
    assert V.decode_shape_error(2049, 1, 1) == "decode supports blocks of at most 2048 tokens (got 2049)"
    assert V.decode_shape_error(1025, 4, 1, depth=2) == ("decode needs heads * max(block length, blocks) <= 4096 "
                                                         "(got 4 * max(1025, 1))")
    assert (V.DECODE_WIDTH, V.DECODE_ATTN_WIDTH, V.DECODE_MAX_LAYERS) == (128, 32, 8)


def test_decode_shapes_of_the_gpu_suite_pass_the_positional_form():
    for ctx, blocks, heads, _, _ in DECODE_SHAPES:
        assert V.decode_shape_error(ctx, heads, blocks) is None
        assert V.decode_shape_error(ctx, heads, blocks, 128, 32, 3) is None
        assert V.decode_shape_error(ctx, heads, blocks, 128, 16, 3) is not None


def test_sinusoid_table_shorter_than_the_context_is_refused_at_construction():
    """Raised before the constructor touches the device, so it is checked here too (8192 is the headline context)."""
    kw = dict(heads=2, attn_stacks=1, drop_out_rate=0.0, levels=1, level=0)
    with pytest.raises(ValueError, match="context length 8192 exceeds the sinusoid table of .*5000 rows"):
        FMHABasedAutoregressiveModel(64, 128, 1, 4, context_length=(8192,), pos_emb=False, **kw)
    with pytest.raises(ValueError, match="context length 5004 exceeds"):
        FMHABasedAutoregressiveModel(64, 128, 1, 4, context_length=(5004,), pos_emb=False, **kw)
    with pytest.raises(ValueError, match="context length 256 exceeds the sinusoid table of .*128 rows"):
        FMHABasedAutoregressiveModel(64, 128, 1, 4, context_length=(256,), pos_emb=False, maximum_pos_encoding=128, **kw)


# ------------------------------------------------------------------ what the training kernels accept of other widths
def _route(K, N, taps, dt, ldx=None, ldy=None, dir=-1):
    info = V.SeqlinRouteInfo()
    rc = V.lib().vqa_seqlin_route(PTR, ldx or K, None, PTR, None, None, 0, PTR, ldy or N, 2, 256, K, N, taps, dir, 0, 0,
                                  dt, 0, ctypes.byref(info))
    return rc, info


def test_attention_width_16_routes_in_fp32():
    """m_attn 0.125, one head (attention width 16): every prepared-image launch of a train step has a route in fp32
    — the q/k/v conv and the data gradients into it on the direct kernels, the 16-wide maps (no direct instantiation
    for K = 16 or 48) on the staged kernel — and every weight gradient a plan. Nothing is launched."""
    w, d = 16, 128
    fwd = {(d, 3 * w, 3, d, 3 * w): 1,       # qkv conv
           (w, w, 1, 3 * w, w): 0,           # query / key / value on column slices of qkv (row stride 48)
           (w, w, 1, w, w): 0,               # out
           (w, d, 1, w, d): 0,               # proj
           (d, d, 1, d, d): 1,               # mlp and its transpose
           (d, w, 1, d, w): 1,               # proj transposed
           (w, w, 1, w, 3 * w): 0}           # q / k / v transposed into column slices of dqkv
    for (K, N, taps, ldx, ldy), direct in fwd.items():
        rc, info = _route(K, N, taps, F32, ldx, ldy)
        assert rc == 0, V.last_error()
        assert info.direct == direct, (K, N, taps, info)
    rc, info = _route(3 * w, d, 3, F32, dir=1)   # qkv transposed (the conv's data gradient)
    assert rc == 0 and info.direct == 0
    for K, N, taps in ((d, 3 * w, 3), (w, w, 1), (w, d, 1), (d, w, 1), (d, d, 1)):
        seg_rows, segs, ppw = V.seqlin_wgrad_plan(2, 256, K, N, taps, torch.float32)
        assert seg_rows % 64 == 0 and segs >= 1 and ppw in (1, 2, 6)


@pytest.mark.parametrize("dt,K,N,taps,msg", [
    (BF16, 16, 16, 1, "seqlin_fwd: K=16 N=16 unsupported"),      # bf16 at attention width 16: K % 32
    (F32, 128, 192, 3, "seqlin_fwd: K=128 N=192 unsupported"),   # m_attn 0.5: the q/k/v conv is 192 wide
    (BF16, 128, 192, 3, "seqlin_fwd: K=128 N=192 unsupported")])
def test_other_widths_are_refused_by_the_entry_check(dt, K, N, taps, msg):
    rc, _ = _route(K, N, taps, dt)
    assert rc == -2 and V.last_error() == msg, V.last_error()


# ------------------------------------------------------------------ the GPU cases tell architectures apart
CFG = dict(bins=64, ctx=256, width=128, heads=2, blocks=4)


def _gap(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_gpu_cases_tell_architectures_apart():
    """With one set of parameter values (their shapes do not depend on attn_stacks) the fp64 oracle's logits differ by
    far more than the GPU bound of 2e-5 of max |logit| between the architectures the GPU suite claims to separate.
    Required: 1e-2 (500x the bound). Measured at seed 3: attn_stacks 0 vs 1 at depth 4: 1.8e-1; depth 4 vs its first
    3 layers: 4.0e-1; sinusoid table vs a zero table (depth 3): 1.2 (seed 5: 1.2e-1, 4.3e-1, 1.0)."""
    c1 = P.PriorConfig(depth=4, attn_stacks=1, **CFG)
    c0 = P.PriorConfig(depth=4, attn_stacks=0, **CFG)
    c3 = P.PriorConfig(depth=3, attn_stacks=1, **CFG)
    assert [c0.attn_func(i) for i in range(4)] == [0, 1, 0, 1] and [c1.attn_func(i) for i in range(4)] == [0, 1, 2, 0]
    p = P.to_torch(P.init_params(c1, 3))
    tok = torch.randint(0, 64, (2, 256), generator=torch.Generator().manual_seed(1))
    l1 = P.model_forward(p, c1, tok)
    gaps = {"attn_stacks 0 vs 1": _gap(P.model_forward(p, c0, tok), l1),
            "depth 4 vs first 3 layers": _gap(P.model_forward(p, c3, tok), l1)}
    sin, zero = dict(p), dict(p)
    sin["prior/pos_embedding/embeddings"] = torch.from_numpy(positional_encoding(5000, 128)[0, :256]).double()
    zero["prior/pos_embedding/embeddings"] = torch.zeros(256, 128, dtype=torch.float64)
    gaps["sinusoid vs zero table"] = _gap(P.model_forward(zero, c3, tok), P.model_forward(sin, c3, tok))
    print(gaps)
    for what, gap in gaps.items():
        assert gap >= 1e-2, (what, gap)


# ------------------------------------------------------------------ the sinusoid table
def test_positional_encoding_matches_a_direct_evaluation():
    """multi_head_attention.py:33-59 term by term in fp64: angle = pos * 1 / 10000^(2 (i // 2) / d), sine on the even
    columns, cosine on the odd ones, cast to fp32 at the end. The product's table is that to fp32 rounding: half an
    ulp of a value in [-1, 1] (2^-24), plus the fp64 error of an angle of up to 5000 radians (1e-12)."""
    table = positional_encoding(5000, 128)
    assert table.shape == (1, 5000, 128) and table.dtype == np.float32
    want = np.empty((5000, 128), np.float64)
    for i in range(128):
        rate = 1.0 / math.pow(10000.0, (2 * (i // 2)) / 128.0)
        f = math.sin if i % 2 == 0 else math.cos
        for pos in range(5000):
            want[pos, i] = f(pos * rate)
    err = np.abs(table[0].astype(np.float64) - want).max()
    assert err <= 2.0 ** -24 + 1e-12, err
    assert table[0, 0, 0] == 0.0 and table[0, 0, 1] == 1.0
    # not degenerate: the slowest column pair still moves over the table, and no two of the rows a test uses agree
    assert abs(float(table[0, 4999, 126])) > 0.5
    assert len(np.unique(table[0, :256].round(6), axis=0)) == 256
