"""Fused residual block (vqa_resblock.hip, resnet.py:7-29 ResnetConv1DBlock) vs the unfused conv kernels and
fp64 autograd of the oracle's TF-semantics convs.

Forward: y (and relu(h)) bit-identical to the two-call unfused path (same MFMA order, same bf16 rounding of
h). Backward (h recomputed from x): dx and the four weight gradients against fp64 autograd with the ReLU
masks of the GPU's own h — relative L2 1e-5 in fp32; in bf16 against the unfused backward within 2e-2.
Ragged lengths, T shorter than a tile, every dilation of the model (1, 3, 9, 27) and the largest supported.

Per-element parity (tests/resblock_parity_ref.py): the backward, fp32 and bf16, at the smallest shape of every tile
plan (asserted through vqa_resblock_plan), against the fp64 reference with its own ReLU masks, dx element by element
and the weight gradients to the fp32 bound; a workgroup's run crossing from one item's ragged last tile into the next
item; the persistent loops' steady state (>= 4 tiles per workgroup with extras, one checked item replicated, so no
large reference); the forward looping above 3 workgroups per CU; ba = NULL; exact zeros in x. Inputs and dx sit
between NaN guard bands and the gradient buffers start as NaN.
"""
import numpy as np
import pytest
import torch

import resblock_parity_ref as R
import vqa_lib as V
from oracle.vqvae_ref import conv1d as ref_conv

pytestmark = pytest.mark.gpu

C = 32


def _l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(b.norm(), 1e-30))


def _block(B, T, d, seed, dt, cuda):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g)
    wa = torch.randn(3, C, C, generator=g) / np.sqrt(3 * C)
    wb = torch.randn(3, C, C, generator=g) / np.sqrt(3 * C)
    ba = 0.1 * torch.randn(C, generator=g)
    bb = 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B, T, C, generator=g)
    to = lambda t, tdt=torch.float32: t.to(tdt).to(cuda).contiguous()  # noqa: E731
    return dict(x=to(x, dt), dy=to(dy, dt), wa=to(wa), wb=to(wb), ba=to(ba), bb=to(bb))


def _unfused_fwd(p, d):
    x = p["x"]
    B, T, _ = x.shape
    cd = V.dtype_code(x.dtype)
    h = torch.empty_like(x)
    y = torch.empty_like(x)
    V.conv1d_fwd(x, p["wa"], p["ba"], None, h, B, T, T, C, C, 3, 1, d, d, V.PRE_RELU, cd)
    V.conv1d_fwd(h, p["wb"], p["bb"], x, y, B, T, T, C, C, 3, 1, 1, 1, V.PRE_RELU | V.ADD_RESIDUAL, cd)
    return h, y


def _fused_fwd(p, d):
    x = p["x"]
    y, h = torch.empty_like(x), torch.empty_like(x)
    V.resblock_fwd(x, p["wa"], p["ba"], p["wb"], p["bb"], y, d, h_out=h)
    return h, y


def _fused_bwd(p, d, deferred=False):
    x = p["x"]
    dx = torch.empty_like(x)
    g = {k: torch.full(s, float("nan"), device=x.device) for k, s in
         (("wa", (3, C, C)), ("ba", (C,)), ("wb", (3, C, C)), ("bb", (C,)))}
    dfr = V.Deferred() if deferred else None
    V.resblock_bwd(p["dy"], x, p["wa"], p["ba"], p["wb"], p["bb"], dx, g["wa"], g["ba"], g["wb"], g["bb"], d, dfr)
    if dfr is not None:
        dfr.flush()
    return dx, g


CASES = [(2, 1000, 1), (2, 1000, 3), (1, 777, 9), (2, 2048, 27), (1, 40, 27), (3, 129, 32), (1, 300, 2)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,d", CASES)
def test_forward_bitwise_vs_unfused(cuda, B, T, d, dt):
    p = _block(B, T, d, seed=B * 1000 + T + d, dt=dt, cuda=cuda)
    h0, y0 = _unfused_fwd(p, d)
    h1, y1 = _fused_fwd(p, d)
    assert torch.equal(y1, y0)
    assert torch.equal(h1, torch.relu(h0))


@pytest.mark.parametrize("B,T,d", CASES)
def test_backward_fp32_vs_autograd(cuda, B, T, d):
    p = _block(B, T, d, seed=7 * T + d, dt=torch.float32, cuda=cuda)
    h, _ = _fused_fwd(p, d)  # relu(h) exactly as the backward recomputes it: its masks
    dx, g = _fused_bwd(p, d)
    cpu = {k: v.double().cpu() for k, v in p.items()}
    W = {k: cpu[k].clone().requires_grad_(True) for k in ("wa", "ba", "wb", "bb")}
    xv = cpu["x"].clone().requires_grad_(True)
    hh = ref_conv(xv * (cpu["x"] > 0), W["wa"], W["ba"], 1, d)
    y = xv + ref_conv(hh * (h.double().cpu() > 0), W["wb"], W["bb"], 1, 1)
    grads = torch.autograd.grad((y * cpu["dy"]).sum(), [xv] + [W[k] for k in ("wa", "ba", "wb", "bb")])
    assert _l2(dx, grads[0]) < 1e-5
    for k, gr in zip(("wa", "ba", "wb", "bb"), grads[1:]):
        assert _l2(g[k], gr) < 1e-5, k


@pytest.mark.parametrize("B,T,d", [(2, 1000, 1), (2, 2048, 27), (1, 40, 27), (4, 4096, 9)])
def test_backward_bf16_vs_unfused(cuda, B, T, d):
    p = _block(B, T, d, seed=3 * T + d, dt=torch.bfloat16, cuda=cuda)
    x, dy = p["x"], p["dy"]
    cd = V.BF16
    h, _ = _unfused_fwd(p, d)
    dh = torch.empty_like(x)
    dx0 = torch.empty_like(x)
    ref = {k: torch.empty(s, device=cuda) for k, s in (("wa", (3, C, C)), ("ba", (C,)), ("wb", (3, C, C)), ("bb", (C,)))}
    V.conv1d_bwd_data_weight(dy, p["wb"], h, None, dh, ref["wb"], ref["bb"], B, T, T, C, C, 3, 1, 1, 1, V.PRE_RELU, cd)
    V.conv1d_bwd_data_weight(dh, p["wa"], x, dy, dx0, ref["wa"], ref["ba"], B, T, T, C, C, 3, 1, d, d,
                             V.PRE_RELU | V.ADD_RESIDUAL, cd)
    dx, g = _fused_bwd(p, d)
    assert _l2(dx, dx0) < 2e-2
    for k in ref:
        assert _l2(g[k], ref[k]) < 2e-2, k


def test_backward_deterministic_and_deferred(cuda):
    p = _block(4, 3000, 9, seed=5, dt=torch.bfloat16, cuda=cuda)
    dx1, g1 = _fused_bwd(p, 9)
    dx2, g2 = _fused_bwd(p, 9, deferred=True)
    assert torch.equal(dx1, dx2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def _unfused_bwd(p, d, h):
    x, dy = p["x"], p["dy"]
    B, T, _ = x.shape
    cd = V.dtype_code(x.dtype)
    dh, dx0 = torch.empty_like(x), torch.empty_like(x)
    ref = {k: torch.empty(s, device=x.device) for k, s in (("wa", (3, C, C)), ("ba", (C,)), ("wb", (3, C, C)),
                                                              ("bb", (C,)))}
    V.conv1d_bwd_data_weight(dy, p["wb"], h, None, dh, ref["wb"], ref["bb"], B, T, T, C, C, 3, 1, 1, 1, V.PRE_RELU, cd)
    V.conv1d_bwd_data_weight(dh, p["wa"], x, dy, dx0, ref["wa"], ref["ba"], B, T, T, C, C, 3, 1, d, d,
                             V.PRE_RELU | V.ADD_RESIDUAL, cd)
    return dx0, ref


def block_grads_fp64(x, dy, h_gpu, W, d):
    """fp64 autograd of resnet.py:7-29 on the GPU's own bf16 inputs, with the ReLU' masks of the GPU's relu(h)
    (the weights as the kernels use them: bf16-rounded kernels, fp32 biases). -> (dx, dW_a, db_a, dW_b, db_b)."""
    x, dy = x.double().cpu(), dy.double().cpu()
    Wv = {k: W[k].double().cpu().clone().requires_grad_(True) for k in ("wa", "ba", "wb", "bb")}
    xv = x.clone().requires_grad_(True)
    hh = ref_conv(xv * (x > 0), Wv["wa"], Wv["ba"], 1, d)
    y = xv + ref_conv(hh * (h_gpu.double().cpu() > 0), Wv["wb"], Wv["bb"], 1, 1)
    return torch.autograd.grad((y * dy).sum(), [xv] + [Wv[k] for k in ("wa", "ba", "wb", "bb")])


def bf16_weights(p):
    """the kernels stage the fp32 conv kernels as bf16 MFMA operands; biases stay fp32"""
    return {"wa": p["wa"].to(torch.bfloat16), "ba": p["ba"], "wb": p["wb"].to(torch.bfloat16), "bb": p["bb"]}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("T,d", [(32768, 27), (32768, 1), (8192, 9), (512, 3)])
def test_full_size_cfg2(cuda, T, d):
    """cfg2 shapes (B = 32, bf16; T = 32768 is level 0's first stack, 512 level 2's last): forward
    bit-identical to the unfused path; backward (dx and all four weight gradients, through the persistent
    grid and the partial-row reduction at full size) against fp64 autograd of the block on the same bf16 inputs
    (the GPU's relu(h) masks; bf16 kernels) within 1e-2 relative L2 — the bf16 roundings of dh and dx — and
    against the unfused HIP backward within the bf16 bound."""
    B = 32
    p = _block(B, T, d, seed=11 + d, dt=torch.bfloat16, cuda=cuda)
    h0, y0 = _unfused_fwd(p, d)
    h1, y1 = _fused_fwd(p, d)
    assert torch.equal(y1, y0)
    dx, g = _fused_bwd(p, d)
    want = block_grads_fp64(p["x"], p["dy"], h1, bf16_weights(p), d)
    errs = {"dx": _l2(dx, want[0])}
    errs.update({k: _l2(g[k], gr) for k, gr in zip(("wa", "ba", "wb", "bb"), want[1:])})
    print(f"T={T} d={d} fp64 relative L2: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < 1e-2, f"{k} vs fp64: {e:.3e}"
    dx0, ref = _unfused_bwd(p, d, h0)
    assert _l2(dx, dx0) < 2e-2
    for k in ref:
        assert _l2(g[k], ref[k]) < 2e-2, k


def test_unsupported(cuda):
    assert not V.resblock_supported(64, 1, V.BF16)
    assert not V.resblock_supported(32, 33, V.BF16)
    assert V.resblock_supported(32, 27, V.BF16) and V.resblock_supported(32, 27, V.F32)


# ------------------------------------------------------------------ per-element parity on every tile plan
GUARD = 4096   # NaN elements on either side of x, dy and dx
DTS = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]


def _guarded(t, cuda):
    """a device copy of t between two NaN bands -> (the copy, the whole buffer)"""
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=t.dtype, device=cuda)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _bands_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _dev(p, cuda):
    q = {k: (None if v is None else v.to(cuda).contiguous()) for k, v in p.items()}
    q["x"], q["x_buf"] = _guarded(p["x"], cuda)
    q["dy"], q["dy_buf"] = _guarded(p["dy"], cuda)
    return q


def _bwd_guarded(q, d, deferred=False):
    """the fused backward with dx between NaN bands and NaN-filled gradient buffers -> (dx, grads)"""
    x = q["x"]
    dx, dx_buf = _guarded(torch.zeros(x.shape, dtype=x.dtype), x.device)
    dx.fill_(float("nan"))
    g = {k: torch.full(s, float("nan"), device=x.device) for k, s in
         (("wa", (3, C, C)), ("ba", (C,)), ("wb", (3, C, C)), ("bb", (C,)))}
    dfr = V.Deferred() if deferred else None
    V.resblock_bwd(q["dy"], x, q["wa"], q["ba"], q["wb"], q["bb"], dx, g["wa"], g["ba"], g["wb"], g["bb"], d, dfr)
    if dfr is not None:
        dfr.flush()
    torch.cuda.synchronize()
    assert _bands_intact(dx_buf) and not bool(torch.isnan(dx).any())
    assert _bands_intact(q["x_buf"]) and _bands_intact(q["dy_buf"])
    return dx, g


def _assert_parity(name, ref, dx, g):
    """every output against the reference's per-element tolerance; the figures go to the table first"""
    ratios = {}
    for k, got in [("dx", dx)] + [(k, g[k]) for k in R.GRADS]:
        ratios[k] = ref.ratio(k, got)
        R.record(k, name, ref.e32[k], ref.c[k], ref.err(k, got), ratios[k])
    assert ref.s_share <= R.S_MAX
    for k, r in ratios.items():
        assert r <= 1.0, f"{name} {k}: err / tolerance = {r:.3f}"


def _name(B, T, d, dt, tag=""):
    return f"B={B} T={T} d={d} {R.dt_name(dt)}{tag}"


# (tile rows, compiled dilation) of every backward plan case
WANT_PLAN = {(1, 8269, 1): (160, 1), (1, 8269, 3): (160, 3), (1, 8269, 9): (160, 9), (1, 8191, 9): (128, 9),
             (1, 8192, 9): (160, 9), (2, 2049, 27): (128, 27), (3, 129, 32): (128, 0), (1, 300, 2): (128, 0),
             (1, 1, 27): (128, 27), (1, 5, 27): (128, 27), (1, 27, 27): (128, 27), (1, 1, 1): (128, 1)}


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("B,T,d", R.PLAN_CASES)
def test_backward_per_element_on_every_plan(cuda, B, T, d, dt):
    pl = V.resblock_plan(B, T, C, d, dt, True)
    assert (pl.tile_rows, pl.compiled_dilation) == WANT_PLAN[(B, T, d)], pl
    assert pl.tiles_per_item == -(-T // pl.tile_rows) and pl.tiles == B * pl.tiles_per_item
    assert pl.partial_rows == pl.workgroups
    if (B, T, d) == (2, 2049, 27):
        assert T - (pl.tiles_per_item - 1) * pl.tile_rows == 1      # a last tile of one row
    p, ref = R.case(B, T, d, dt, pl.tile_rows)
    dx, g = _bwd_guarded(_dev(p, cuda), d)
    _assert_parity(_name(B, T, d, dt), ref, dx, g)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("B,T,d", R.CROSS_CASES)
def test_backward_run_crosses_into_the_next_item(cuda, B, T, d, dt):
    """9 tiles on 4 workgroups, one of them with an extra tile: a run goes from item 1's ragged last tile (44 rows)
    into item 2's first, prefetching across the boundary."""
    pl = V.resblock_plan(B, T, C, d, dt, True)
    assert (pl.tile_rows, pl.tiles_per_item, pl.tiles) == (128, 3, 9), pl
    assert (pl.workgroups, pl.tiles_per_workgroup, pl.extra_tile_workgroups) == (4, 2, 1), pl
    runs = [pl.run(w) for w in range(pl.workgroups)]
    assert runs[-1][1] == pl.tiles
    assert any(a // pl.tiles_per_item != (b - 1) // pl.tiles_per_item for a, b in runs)
    p, ref = R.case(B, T, d, dt, pl.tile_rows)
    dx, g = _bwd_guarded(_dev(p, cuda), d)
    _assert_parity(_name(B, T, d, dt, " cross"), ref, dx, g)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T,d", R.STEADY_CASES)
def test_backward_steady_state_replicated_item(cuda, T, d, dt):
    """One checked item replicated B times, B the smallest for which the plan gives every workgroup at least 4
    tiles and some of them one more: every item's dx is bitwise the single-item launch's (a tile's arithmetic does
    not depend on its slot), the weight gradients are B times the single item's fp64 reference within the bound (its
    e32 taken over the fp32 running sum of B copies), and the deferred reduction gives the same bits."""
    one = V.resblock_plan(1, T, C, d, dt, True)
    assert one.tile_rows == (160 if d == 9 else 128)
    B = next(b for b in range(2, 4096) if (lambda q: q.tiles_per_workgroup >= 4 and q.extra_tile_workgroups >= 1)(
        V.resblock_plan(b, T, C, d, dt, True)))
    pl = V.resblock_plan(B, T, C, d, dt, True)
    assert pl.tile_rows == one.tile_rows and pl.tiles_per_workgroup >= 4 and pl.extra_tile_workgroups >= 1, pl
    p, ref = R.case(1, T, d, dt, one.tile_rows)
    dx1, g1 = _bwd_guarded(_dev(p, cuda), d)
    _assert_parity(_name(1, T, d, dt, " single"), ref, dx1, g1)
    rep = dict(p, x=p["x"].expand(B, T, C).contiguous(), dy=p["dy"].expand(B, T, C).contiguous())
    q = _dev(rep, cuda)
    dxB, gB = _bwd_guarded(q, d)
    assert torch.equal(dxB, dx1.expand(B, T, C))
    dxD, gD = _bwd_guarded(q, d, deferred=True)
    assert torch.equal(dxD, dxB)
    for k in R.GRADS:
        assert torch.equal(gD[k], gB[k]), k
        want, allow = B * ref.r[k], B * ref.allow[k]
        run = torch.zeros_like(ref.lo[k])
        for _ in range(B):
            run = run + ref.lo[k]                      # the fp32 running sum of B item sums
        scale = float(want.abs().max())
        e32 = float(((run.double() - want).abs() - allow).clamp_min(0).max()) / scale
        c = max(R.WGRAD_TOL, 8.0 * e32)
        ratio = ref.ratio(k, gB[k], want, c * scale + allow)
        R.record(k, _name(B, T, d, dt, " steady"), e32, c, ref.err(k, gB[k], want), ratio)
        assert ratio <= 1.0, f"{k}: err / tolerance = {ratio:.3f}"


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("T,d", [(2 * 176 + 5, 3), (300, 2)])
def test_forward_loops_above_three_workgroups_per_cu(cuda, T, d, dt):
    """B sized from the plan so that every forward workgroup loops over 2 tiles and some over 3 (the prefetch two
    ahead), runs crossing items: bit-identical to the unfused path."""
    B = next(b for b in range(1, 1 << 16) if (lambda q: q.tiles_per_workgroup >= 2 and q.extra_tile_workgroups >= 1)(
        V.resblock_plan(b, T, C, d, dt, False)))
    pl = V.resblock_plan(B, T, C, d, dt, False)
    assert (pl.tile_rows, pl.compiled_dilation, pl.tiles_per_item) == ((176, 3, 3) if d == 3 else (128, 0, 3)), pl
    assert pl.tiles_per_workgroup >= 2 and pl.extra_tile_workgroups >= 1 and pl.partial_rows == 0
    p = _block(B, T, d, seed=T + d, dt=dt, cuda=cuda)
    h0, y0 = _unfused_fwd(p, d)
    h1, y1 = _fused_fwd(p, d)
    assert torch.equal(y1, y0)
    assert torch.equal(h1, torch.relu(h0))


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_no_bias_a(cuda, dt):
    """ba = NULL on both entry points: the bits of a zero bias, and the backward within the per-element bound of the
    reference without b_a."""
    B, T, d = 2, 300, 3
    pl = V.resblock_plan(B, T, C, d, dt, True)
    p, ref = R.case(B, T, d, dt, pl.tile_rows, 0, False)
    q = _dev(p, cuda)
    z = dict(q, ba=torch.zeros(C, device=cuda))
    h0, y0 = _fused_fwd(z, d)
    h1, y1 = _fused_fwd(q, d)
    assert torch.equal(y1, y0) and torch.equal(h1, h0)
    hu, yu = _unfused_fwd(z, d)
    assert torch.equal(y1, yu) and torch.equal(h1, torch.relu(hu))
    want_y = ref.r["y"]
    assert float((y1.double().cpu() - want_y).abs().max()) <= (2.0 ** -7 if dt == torch.bfloat16 else 1e-5) * float(
        want_y.abs().max())
    dx0, g0 = _bwd_guarded(z, d)
    dx1, g1 = _bwd_guarded(q, d)
    assert torch.equal(dx1, dx0)
    for k in R.GRADS:
        assert torch.equal(g1[k], g0[k]), k
    _assert_parity(_name(B, T, d, dt, " ba=None"), ref, dx1, g1)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_exact_zeros_in_x(cuda, dt):
    """x > 0, not x >= 0: at a planted zero (of either sign) dx is dy itself."""
    B, T, d = 3, 300, 27
    pl = V.resblock_plan(B, T, C, d, dt, True)
    p, ref = R.case(B, T, d, dt, pl.tile_rows, 600, True)
    zero = p["x"] == 0
    assert int(zero.sum()) == 600 and bool(torch.signbit(p["x"][zero]).any())
    dx, g = _bwd_guarded(_dev(p, cuda), d)
    assert torch.equal(dx.cpu()[zero], p["dy"][zero])
    _assert_parity(_name(B, T, d, dt, " zeros"), ref, dx, g)
