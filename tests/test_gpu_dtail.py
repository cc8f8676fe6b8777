"""Decoder-tail kernels (vqa_dtail.hip) vs the CPU oracle in fp64.

The tail is encdec.py:67-68 (the last Conv1DTranspose, K=4, stride 2, 32 -> 64 channels) followed by
encdec.py:148 (the decoder's output Conv1D, K=3, 64 -> 1), composed into one thin convolution. The oracle
runs the two layers separately (oracle/vqvae_ref.conv1d_transpose, conv1d) in fp64 and differentiates them
with autograd. Tolerances: fp32 activations 2e-5 of the output's max-abs (the composite only re-associates
the sums); bf16 activations (h rounded to bf16 on input; dh rounded on output) 1e-2 for dh and 2e-5 for y and
the parameter gradients (both are fp32 sums of the same bf16 inputs).

test_plan_case and below: every launch plan of the forward (grid-stride passes, clamped gx), of the backward's
partial-row reduction (single stage below and above 64 rows, the smallest and a deep two-stage plan), every Cu route
of the compose and chain kernels, NULL biases, and the rows at the wave and pass boundaries. Each case asserts the
plan it is there for (tests/dtail_parity_ref.py restates the launch code's constants), writes y and dh into the
middle of NaN-filled guarded buffers, and holds y, fp32 dh and the parameter gradients to 2e-5 of the reference's
max-abs, or, where the fp32 sums are much longer than that figure was set on (Cu >= 130; the parameter gradients of
a batch of hundreds), to max(2e-5, 4 x the float32 two-layer oracle's own measured error). bf16 dh is held per
element: |got - ref| <= 2^-8 |ref| + (that fp32 bound) max|ref|.
"""
import functools

import pytest
import torch

import dtail_parity_ref as D
import vqa_lib as V
from oracle import vqvae_ref as R

pytestmark = pytest.mark.gpu


def _params(Cu, seed):
    g = torch.Generator().manual_seed(seed)
    w_up = torch.randn(4, Cu, 32, generator=g) * 0.1
    b_up = torch.randn(Cu, generator=g) * 0.1
    w_out = torch.randn(3, Cu, 1, generator=g) * 0.1
    b_out = torch.randn(1, generator=g) * 0.1
    return w_up, b_up, w_out, b_out


def _oracle(h, dy, w_up, b_up, w_out, b_out):
    hd = h.double().clone().requires_grad_(True)
    ps = [p.double().clone().requires_grad_(True) for p in (w_up, b_up, w_out, b_out)]
    u = R.conv1d_transpose(hd, ps[0], ps[1], 2)
    y = R.conv1d(u, ps[2], ps[3])
    (y * dy.double()).sum().backward()
    return y.detach(), hd.grad, [p.grad for p in ps]


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("B,T,Cu,dt", [(2, 64, 64, torch.float32), (3, 37, 64, torch.float32), (1, 1, 64, torch.float32),
                                       (2, 300, 48, torch.float32), (2, 64, 64, torch.bfloat16),
                                       (4, 1000, 64, torch.bfloat16),
                                       (2, 70001, 64, torch.bfloat16)])  # several backward passes, ragged last
def test_forward_backward(cuda, B, T, Cu, dt):
    g = torch.Generator().manual_seed(B * 1000 + T)
    h = torch.randn(B, T, 32, generator=g).to(dt)
    dy = torch.randn(B, 2 * T, 1, generator=g)
    w_up, b_up, w_out, b_out = _params(Cu, T)
    y_ref, dh_ref, (dwu_ref, dbu_ref, dwo_ref, dbo_ref) = _oracle(h.float(), dy, w_up, b_up, w_out, b_out)

    hd = h.to(cuda)
    p = [t.to(cuda).contiguous() for t in (w_up, b_up, w_out, b_out)]
    y = torch.empty(B, 2 * T, 1, device=cuda)
    V.dtail_fwd(hd, *p, y)
    assert _rel(y.cpu(), y_ref) < 2e-5

    dh = torch.empty_like(hd)
    grads = [torch.full_like(t, float("nan")) for t in p]  # written, not accumulated
    V.dtail_bwd(dy.to(cuda), hd, *p, dh, *grads)
    assert _rel(dh.cpu().float(), dh_ref) < (1e-2 if dt == torch.bfloat16 else 2e-5)
    for got, ref in zip(grads, (dwu_ref, dbu_ref, dwo_ref, dbo_ref)):
        assert _rel(got.cpu(), ref) < 2e-5


def test_deterministic(cuda):
    B, T = 8, 4096
    g = torch.Generator().manual_seed(5)
    h = torch.randn(B, T, 32, generator=g).to(torch.bfloat16).to(cuda)
    dy = torch.randn(B, 2 * T, 1, generator=g).to(cuda)
    p = [t.to(cuda) for t in _params(64, 9)]
    outs = []
    for _ in range(2):
        dh = torch.empty_like(h)
        grads = [torch.empty_like(t) for t in p]
        V.dtail_bwd(dy, h, *p, dh, *grads)
        outs.append([dh] + grads)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_supported():
    assert V.dtail_supported(32, 64, 4, 2, 3, 1, V.BF16)
    assert not V.dtail_supported(64, 64, 4, 2, 3, 1, V.BF16)
    assert not V.dtail_supported(32, 64, 3, 2, 3, 1, V.BF16)
    assert not V.dtail_supported(32, 64, 4, 2, 3, 2, V.F32)


# ------------------------------------------------------------------ every launch plan, guarded, per-element bf16
class _Guarded:
    """An output tensor as the middle of a NaN-filled buffer with one item of guard before and after."""

    def __init__(self, N, shape, dtype):
        self.big = torch.full((N + 2, *shape), float("nan"), dtype=dtype, device="cuda")
        self.t = self.big[1:N + 1]
        assert self.t.is_contiguous()
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        self.before = self.big.view(self.bits)[[0, N + 1]].clone()

    def check(self, name):
        N = self.t.shape[0]
        assert torch.equal(self.big.view(self.bits)[[0, N + 1]], self.before), f"{name}: guard items written"
        assert not bool(torch.isnan(self.t).any()), f"{name}: NaN left in the output"


@functools.lru_cache(maxsize=2)
def _reference(B, T, Cu, dt, bias):
    """inputs, the fp64 two-layer oracle on h rounded to dt, and the bound of every output (computed once per case)"""
    h, dy = D.inputs(B, T, dt)
    w_up, b_up, w_out, b_out = D.params(Cu, T)
    if not bias:
        b_up = b_out = None
    args = (h.float(), dy, w_up, b_up, w_out, b_out)
    ref = D.oracle(*args)
    names = D.long_sums(B, Cu)
    measured = D.fp32_oracle_error(ref, *args, names) if names else {}
    return h, dy, (w_up, b_up, w_out, b_out), ref, measured


def _run(B, T, Cu, dt, bias=True, grads=(True, True)):
    """forward and backward in guarded buffers -> {name: tensor on the CPU}"""
    h, dy, prm, _, _ = _reference(B, T, Cu, dt, bias)
    hd = h.cuda()
    p = [None if t is None else t.cuda().contiguous() for t in prm]
    y = _Guarded(B, (2 * T, 1), torch.float32)
    V.dtail_fwd(hd, *p, y.t)
    dh = _Guarded(B, (T, D.C), dt)
    nan = lambda t: torch.full_like(t, float("nan"))  # noqa: E731  (written, not accumulated)
    g = [nan(p[0]), torch.full((Cu,), float("nan"), device="cuda") if grads[0] else None, nan(p[2]),
         torch.full((1,), float("nan"), device="cuda") if grads[1] else None]
    V.dtail_bwd(dy.cuda(), hd, *p, dh.t, *g)
    torch.cuda.synchronize()
    y.check("y")
    dh.check("dh")
    out = {"y": y.t.cpu(), "dh": dh.t.cpu(), "dw_up": g[0].cpu(), "dw_out": g[2].cpu()}
    if grads[0]:
        out["db_up"] = g[1].cpu()
    if grads[1]:
        out["db_out"] = g[3].cpu()
    return out


def _check(tag, B, T, Cu, dt, bias=True):
    _, _, _, ref, measured = _reference(B, T, Cu, dt, bias)
    got = _run(B, T, Cu, dt, bias)
    name = "bf16" if dt == torch.bfloat16 else "fp32"
    fails = []
    for k in D.NAMES:
        assert got[k].shape == ref[k].shape and not bool(torch.isnan(got[k]).any()), k
        bd = D.bound(measured.get(k))
        src = f"max(2e-5, 4 x fp32 oracle {measured[k]:.2e})" if k in measured else "project 2e-5"
        if k == "dh" and dt == torch.bfloat16:
            err = D.bf16_dh_excess(got[k], ref[k], bd)
            line = f"excess over 2^-8|ref| + {bd:.1e} max|ref| {err:.3f} (<= 1)"
            ok = err <= 1.0
        else:
            err = D.rel(got[k], ref[k])
            line = f"bound {bd:.2e} [{src}] kernel {err:.2e}"
            ok = err < bd
        print(f"PARITY dtail {tag} B={B} T={T} Cu={Cu} {name} {k:6s} {line}")
        if not ok:
            fails.append((k, err, bd))
    assert not fails, fails


DTS = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("B,T", list(D.FWD_CASES))
def test_forward_passes(cuda, B, T, dt):
    """the grid-stride loop: second and third passes, the carried prefetch, halo rows at the pass boundary, the
    prefetch past the item; 768 // B == 0 clamps gx to 1"""
    gx, passes = D.fwd_plan(B, T)
    assert (gx, passes) == D.FWD_CASES[(B, T)] and passes >= 2, (gx, passes)
    _check(f"fwd gx={gx} passes={passes}", B, T, 64, dt)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("B,T", list(D.BWD_CASES))
def test_backward_plans(cuda, B, T, dt):
    """P partial rows: single stage at P >= 64 (P % 16 != 0), the smallest two-stage plan, a deep one over three passes"""
    plan = D.bwd_plan(B, T)
    assert plan == D.BWD_CASES[(B, T)], plan
    assert plan[1] >= 64 and (plan[2] > 0) == (plan[1] % D.GROUPS == 0)
    _check(f"bwd P={plan[1]} R={plan[2]} passes={plan[3]}", B, T, 64, dt)


@pytest.mark.parametrize("Cu,dt", [(c, torch.float32) for c in D.CU_CASES] + [(130, torch.bfloat16)])
def test_channel_counts(cuda, Cu, dt):
    """Cu = 1, 33: the lane clamp and the ragged last chain workgroup; 65, 130, 1024: the compose kernel's loop"""
    assert V.dtail_supported(32, Cu, 4, 2, 3, 1, V.BF16 if dt == torch.bfloat16 else V.F32)
    _check("Cu", 2, 70, Cu, dt)


@pytest.mark.parametrize("T", D.EDGE_T)
def test_edge_rows(cuda, T):
    """T = 1: both edge corrections on one row; 63..65: the wave boundary; 255..257: the pass boundary"""
    _check("edge", 2, T, 64, torch.float32)


def test_null_biases(cuda):
    """b_up = b_out = NULL is the oracle with zero biases; db_up = db_out = NULL leaves the other outputs' bits alone"""
    _check("null b_up b_out", 2, 70, 64, torch.float32, bias=False)
    full = _run(2, 70, 64, torch.float32)
    for grads in ((False, False), (False, True), (True, False)):
        part = _run(2, 70, 64, torch.float32, grads=grads)
        for k, v in part.items():
            assert torch.equal(v.view(torch.int32), full[k].view(torch.int32)), (grads, k)
