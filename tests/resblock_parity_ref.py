"""Plain reference and per-element bounds of the fused residual block (csrc/vqa_resblock.hip), shared by
tests/test_gpu_resblock.py and the CPU-only tests/test_resblock_parity_host.py.

The block (resnet.py:7-29) and its backward are written out as shifted matmuls, generic in the dtype:
    h = conv_a(relu x) + b_a          y  = x + conv_b(relu h) + b_b
    dh = conv_b^T(dy) * (h > 0)       dx = dy + conv_a^T(dh) * (x > 0)
    dW_b = relu(h)^T dy, db_b = sum dy, dW_a = relu(x)^T dh, db_a = sum dh          (shifted per tap)
Evaluated in fp64 on the rounded inputs (x, dy and the conv kernels in the activation dtype, biases fp32) it is the
reference. In bf16 it mirrors the kernel's two roundings: relu(h) is rounded to bf16 (what dW_b reads) and dh is rounded
to bf16 before conv_a^T and before dW_a / db_a. dx is left unrounded: the kernel's last rounding is the u_out term.

Discrete decisions. The kernel recomputes h and dh in fp32 in its own MFMA order, so a decision that hangs on the sign
or on the last bf16 bit of such a value may fall either way when the value lies within fp32 error of the threshold.
Both outcomes are accepted, and what the other outcome would add is put on the tolerance of exactly the outputs the
element reaches:
    S    elements with |h64| <= MARGIN * sum |terms of h|: either ReLU mask. dh there may be 0 or conv_b^T(dy); relu(h)
         moves by at most |h64| + margin. The masks are the reference's own, never the GPU's.
    F    (bf16 only) elements of relu(h) / dh within MARGIN * sum |terms| of a bf16 rounding boundary: either neighbour,
         one bf16 ulp apart.
MARGIN = 64 * 2^-24; the fp32 run of this reference stays far inside it (tests/test_resblock_parity_host.py asserts that
its masks differ from the fp64 ones only inside S). S must stay below S_MAX = 1e-4 of the elements of every case.

Bounds. None is taken from a kernel's error.
    dx, per element:   |err_i| <= u_out |dx_i| + c (|W_a|^T applied to |dh|)_i (x_i > 0) + allowance_i
                       u_out = 2^-8 in bf16, 0 in fp32; where x_i <= 0 the kernel must return dy_i itself.
    dW, db:            |err| <= c max |ref| + allowance, per element of the gradient; the fp32 bound in bf16 too (fp32
                       sums of exact products of rounded operands).
    c = max(2e-6, 8 e32): e32 is this reference run in fp32 against fp64 on the same rounded inputs, net of the
    allowance and relative to the same scale — the project's rule for a sum taken in another order (prior_parity_ref).
The inputs put the weight of dy on the rows next to a tile edge and on each item's last row (edge gains), so a tile's
edge row or a one-row last tile is a visible share of every weight-gradient sum.
"""
import functools
import os

import numpy as np
import torch

from prior_parity_ref import shift_rows

C = 32
MARGIN = 64 * 2.0 ** -24
S_MAX = 1e-4
DX_TOL = 2e-6
WGRAD_TOL = 2e-6
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}
GRADS = ("wa", "ba", "wb", "bb")
REPORT = os.environ.get("VQA_PARITY_REPORT")  # a file to append every case's figures to (unset: no table)
EDGE_GAIN = 8.0


def conv(x, w, b, d):
    """y[t] = sum_k x[t + (k - 1) d] @ w[k] (+ b): Keras kernel (3, in, out), SAME padding."""
    y = sum(shift_rows(x, (k - 1) * d) @ w[k] for k in range(3))
    return y if b is None else y + b


def conv_t(dy, w, d):
    """the data gradient of conv: dx[t] = sum_k dy[t - (k - 1) d] @ w[k]^T"""
    return sum(shift_rows(dy, -(k - 1) * d) @ w[k].t() for k in range(3))


def wgrad(x, dy, d):
    """dW[k] = sum_t x[t + (k - 1) d]^T dy[t], db = sum_t dy[t]"""
    n = dy.shape[-1]
    dw = torch.stack([shift_rows(x, (k - 1) * d).reshape(-1, x.shape[-1]).t() @ dy.reshape(-1, n) for k in range(3)])
    return dw, dy.reshape(-1, n).sum(0)


def _round_to(t, act):
    return t if act in (None, torch.float32) else t.to(act).to(t.dtype)


def block(x, dy, wa, ba, wb, bb, d, act=None):
    """The block and its backward in the dtype of the arguments (fp64: the reference, fp32: its e32 run); act = the
    activation dtype whose roundings of relu(h) and dh are mirrored. Returns every intermediate by name."""
    xpos = x > 0
    rx = torch.relu(x)
    h = conv(rx, wa, ba, d)
    hpos = h > 0
    rh = _round_to(torch.relu(h), act)
    y = x + conv(rh, wb, bb, 1)
    dhf = conv_t(dy, wb, 1)
    dh = _round_to(dhf * hpos, act)
    dx = dy + conv_t(dh, wa, d) * xpos
    dwb, dbb = wgrad(rh, dy, 1)
    dwa, dba = wgrad(rx, dh, d)
    return dict(xpos=xpos, rx=rx, h=h, hpos=hpos, rh=rh, y=y, dhf=dhf, dh=dh, dx=dx, wa=dwa, ba=dba, wb=dwb, bb=dbb)


def bf16_ulp(v):
    """spacing of the bf16 numbers around |v| (8 significant bits)"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


def near_bf16_boundary(v, margin):
    """|v| within margin of the midpoint of two neighbouring bf16 numbers: it may round either way"""
    ulp = bf16_ulp(v)
    q = v.abs() / torch.where(ulp > 0, ulp, torch.ones_like(ulp))
    return (ulp > 0) & (((q - q.floor()) - 0.5).abs() * ulp <= margin)


def edge_gains(T, tile_rows, gain=EDGE_GAIN):
    """per-row gains of dy: the first and last row of every tile and the item's last row"""
    t = torch.arange(T)
    m = (t % tile_rows == 0) | (t % tile_rows == tile_rows - 1) | (t == T - 1)
    return torch.where(m, torch.tensor(gain), torch.tensor(1.0))


def make_inputs(B, T, d, dt, seed, tile_rows, zeros=0, bias_a=True):
    """CPU tensors of one case, drawn as tests/test_gpu_resblock.py's _block draws them (x and dy in dt, weights fp32),
    dy with the edge gains; zeros > 0 plants that many exact zeros (every other one a negative zero) in x."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g)
    wa = torch.randn(3, C, C, generator=g) / np.sqrt(3 * C)
    wb = torch.randn(3, C, C, generator=g) / np.sqrt(3 * C)
    ba = 0.1 * torch.randn(C, generator=g)
    bb = 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B, T, C, generator=g) * edge_gains(T, tile_rows)[None, :, None]
    if zeros:
        idx = torch.randperm(x.numel(), generator=g)[:zeros]
        x.view(-1)[idx] = 0.0
        x.view(-1)[idx[::2]] = -0.0
    return dict(x=x.to(dt), dy=dy.to(dt), wa=wa, wb=wb, ba=ba if bias_a else None, bb=bb)


def rounded(p, dt, to=torch.float64):
    """the operands as the kernels read them (conv kernels staged in the activation dtype, biases fp32), widened"""
    ba = p["ba"] if p["ba"] is not None else torch.zeros(C)
    return dict(x=p["x"].to(to), dy=p["dy"].to(to), wa=p["wa"].to(dt).to(to), wb=p["wb"].to(dt).to(to),
                ba=ba.to(to), bb=p["bb"].to(to))


class Reference:
    """fp64 reference of one case with its ambiguous sets, allowances, scales, e32 figures and tolerances."""

    def __init__(self, p, d, dt):
        self.d, self.dt = d, dt
        a = rounded(p, dt)
        self.a = a
        r = self.r = block(**a, d=d, act=dt)
        bf = dt == torch.bfloat16
        m_h = MARGIN * conv(r["rx"], a["wa"].abs(), a["ba"].abs(), d)
        m_dh = MARGIN * conv_t(a["dy"].abs(), a["wb"].abs(), 1)
        self.m_h = m_h
        self.S = r["h"].abs() <= m_h
        self.s_share = float(self.S.double().mean())
        zero = torch.zeros_like(r["h"])
        # how far the kernel's relu(h) and dh may lie from the reference's by a decision falling the other way
        e_h = torch.where(self.S, r["h"].abs() + m_h, zero)
        e_dh = torch.where(self.S, r["dhf"].abs() + m_dh, zero)
        if bf:
            e_h = e_h + torch.where(self.S | (r["hpos"] & near_bf16_boundary(r["h"], m_h)), bf16_ulp(r["h"]), zero)
            e_dh = e_dh + torch.where(self.S | (r["hpos"] & near_bf16_boundary(r["dhf"], m_dh)), bf16_ulp(r["dhf"]),
                                      zero)
        self.f_share = float((e_dh > 0).double().mean())
        wa_abs = a["wa"].abs()
        self.allow = {"dx": conv_t(e_dh, wa_abs, d) * r["xpos"], "bb": torch.zeros(C, dtype=torch.float64)}
        self.allow["wa"], self.allow["ba"] = wgrad(r["rx"], e_dh, d)
        self.allow["wb"] = wgrad(e_h, a["dy"].abs(), 1)[0]
        self.scale = {"dx": conv_t(r["dh"].abs(), wa_abs, d) * r["xpos"]}
        for k in GRADS:
            self.scale[k] = torch.full_like(r[k], float(r[k].abs().max()))
        lo = self.lo = block(**rounded(p, dt, torch.float32), d=d, act=dt)
        self.e32, self.c, self.tol = {}, {}, {}
        for k in ("dx",) + GRADS:
            net = ((lo[k].double() - r[k]).abs() - self.allow[k]).clamp_min(0)
            live = self.scale[k] > 0
            assert float(net[~live].max() if (~live).any() else 0.0) == 0.0, k   # dx = dy exactly where x <= 0
            self.e32[k] = float((net[live] / self.scale[k][live]).max()) if live.any() else 0.0
            self.c[k] = max(DX_TOL if k == "dx" else WGRAD_TOL, 8.0 * self.e32[k])
            self.tol[k] = self.c[k] * self.scale[k] + self.allow[k]
        self.tol["dx"] = self.tol["dx"] + U_OUT[dt] * r["dx"].abs()

    def ratio(self, k, got, ref=None, tol=None):
        """max |got - ref| / tolerance over the elements of output k (inf where a zero tolerance is missed)"""
        ref = self.r[k] if ref is None else ref
        tol = self.tol[k] if tol is None else tol
        err = (torch.as_tensor(got).detach().double().cpu().reshape(ref.shape) - ref).abs()
        if bool(torch.isnan(err).any()):
            return float("inf")
        bad = (tol == 0) & (err > 0)
        if bool(bad.any()):
            return float("inf")
        live = tol > 0
        return float((err[live] / tol[live]).max()) if bool(live.any()) else 0.0

    def err(self, k, got, ref=None):
        """max |got - ref| relative to max |ref| (for the table)"""
        ref = self.r[k] if ref is None else ref
        e = (torch.as_tensor(got).detach().double().cpu().reshape(ref.shape) - ref).abs().max()
        return float(e / max(float(ref.abs().max()), 1e-300))


def l2(a, b):
    """the old metric: relative L2"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def dt_name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


def record(group, case, e32, bnd, err, ratio):
    """One line per case into the measured table (profiles/resblock_parity.txt is a copy of one run's): e32 and the
    accumulation bound c of the group, the largest error relative to max |ref|, and the largest err / tolerance."""
    line = f"{group:6s} {case:44s} e32 {e32:9.3e} bound {bnd:9.3e} err {err:9.3e} ratio {ratio:6.3f}"
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


# The backward cases of tests/test_gpu_resblock.py: (B, T, d), with the seed of each chosen so that the reference's
# own S stays below S_MAX (tests/test_resblock_parity_host.py asserts it in both dtypes).
PLAN_CASES = [(1, 8192 + 77, 1), (1, 8192 + 77, 3), (1, 8192 + 77, 9), (1, 8191, 9), (1, 8192, 9), (2, 2048 + 1, 27),
              (3, 129, 32), (1, 300, 2), (1, 1, 27), (1, 5, 27), (1, 27, 27), (1, 1, 1)]
CROSS_CASES = [(3, 300, 1), (3, 300, 27)]
STEADY_CASES = [(4097, 27), (8192 + 77, 9)]     # (T, d) of the replicated item: a 128-row and the 160-row plan
SEEDS = {}


def seed_of(B, T, d):
    return SEEDS.get((B, T, d), 1000 * B + 7 * T + d)


@functools.lru_cache(maxsize=None)
def case(B, T, d, dt, tile_rows, zeros=0, bias_a=True):
    """(inputs, Reference) of a case, computed once per process and left unchanged"""
    p = make_inputs(B, T, d, dt, seed_of(B, T, d), tile_rows, zeros, bias_a)
    return p, Reference(p, d, dt)
