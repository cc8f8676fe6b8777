"""Plain references shared by the VQ-VAE side's kernel-level parity suites (tests/test_gpu_vq.py, test_gpu_losses.py,
test_gpu_adam.py, test_gpu_cond.py) and their CPU-only checks (tests/test_vqvae_parity_host.py).

Two kinds of reference:
  restatements in the kernels' fp32 operation order (vq_quantize's straight-through value, vq_backward's dz, the MSE
  gradient, Adam's m and v). The kernels build with -ffp-contract=off, torch's CPU ops are separate multiplies and
  adds, and every constant is rounded to float32 the way the kernel's host side rounds it, so torch-CPU fp32 gives
  the kernel's bits: these are compared with torch.equal;
  a layer norm generic in the dtype: evaluated in fp64 it is the reference, evaluated in fp32 on the same rounded
  inputs its error e32 sizes the bound, max(project bound, 8 * e32) (prior_parity_ref.bound).
Project bounds (relative to max |ref|): layer norm 1e-5 fp32 / 1e-2 bf16 (tests/test_gpu_cond.py); dgamma and dbeta are
fp32 sums in both dtypes and take the fp32 figure (a bf16 figure would hide a lost row).
"""
import numpy as np
import torch

from prior_parity_ref import bound, e32_of, edge_weights, gen, record, rel  # noqa: F401  (re-exported)

LN_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
LN_WGRAD_TOL = 1e-5
NAN = float("nan")


def f32(c):
    """A host double as the kernel receives it: rounded to float32 at the C ABI."""
    return torch.tensor(float(c), dtype=torch.float32)


# ---- guarded outputs: a view cut from a filled buffer, and the check that nothing outside the view was written
def guarded(shape, dtype, device, shift=0):
    """(buffer, view): `view` has `shape`, cut from a buffer filled with NaN (-7 for integers). The guard in front
    is one row rounded up to 8 elements, so the view keeps the allocation's 16-byte alignment; shift = 1 starts it
    one element later (off every vector boundary)."""
    n = int(np.prod(shape))
    pad = 8 * -(-int(shape[-1]) // 8)
    off = pad + shift
    buf = torch.full((off + n + pad,), NAN if dtype.is_floating_point else -7, dtype=dtype, device=device)
    return buf, buf[off:off + n].view(shape)


def guards_intact(buf, view):
    off = view.storage_offset()
    head, tail = buf[:off], buf[off + view.numel():]
    if buf.dtype.is_floating_point:
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == -7).all()) and bool((tail == -7).all())


# ---- quantizer (vqa_vq.hip)
def quantize_st(z, ET, idx):
    """vq_quantize's straight-through output: z + (q - z) in fp32, one rounding to z's dtype."""
    zf = z.float()
    return (zf + (ET[idx] - zf)).to(z.dtype)


def commit_ref(z, ET, idx, beta):
    """beta * mean((q - z)^2) in fp64."""
    return beta * float(((ET[idx].double() - z.double()) ** 2).mean())


def backward_dz(dq, z, ET, idx, scale, commit=1.0):
    """vq_backward: dq + scale32 * (z - q) in fp32, one rounding. commit = 0 drops the commitment term, -1 negates
    it (the wrong kernels of tests/test_vqvae_parity_host.py)."""
    zf = z.float()
    term = f32(scale) * (zf - ET[idx])
    if commit == 0:
        return dq.float().to(z.dtype)
    return (dq.float() + (term if commit > 0 else -term)).to(z.dtype)


def planted_codes(D, K, N, dt, seed=None, noise=1e-3):
    """A codebook E ~ N(0, 1) (D, K) fp32 and rows that sit on its codes in turn: row r = E[:, r % K] +
    noise * N(0, 1), rounded to dt, so every code (the last ones of a ragged chunk, the first of a split's span) is
    some row's answer. E stays as generated for bf16 too (the split path takes fp32 E). Returns z, E, the fp64
    distances' argmin, the fp64 top-2 margin and the fp64 minimum distance."""
    g = gen(D * 1000 + K + N if seed is None else seed)
    E = torch.randn(D, K, generator=g)
    z = (E.t()[torch.arange(N) % K] + noise * torch.randn(N, D, generator=g)).to(dt)
    d = ref_dist(z, E)
    top2 = torch.topk(d, 2, dim=1, largest=False).values
    return z, E, d.argmin(1), top2[:, 1] - top2[:, 0], top2[:, 0]


ARGMIN_SHAPES = [(32, 129, 300), (32, 70, 129), (64, 100, 257), (8, 130, 513), (4, 16, 129)]      # (D, K, N)
SPLIT_SHAPES = [(32, 70, 300), (64, 129, 257), (64, 2048, 2100), (32, 64, 300)]


def split_spans(N, K):
    """(nsplit, kspan) of vqa_vq_argmin_split (vqa_vq.hip): row blocks of 256; small batches also split the
    codebook in spans of whole 64-code chunks so that about 512 workgroups run. nsplit > 1 is the packed path
    (atomicMin on keys, then the unpack kernel), nsplit == 1 writes idx directly."""
    rb = -(-N // 256)
    nsplit = min(max(1, 512 // rb), -(-K // 64))
    per = -(-K // nsplit)
    kspan = -(-per // 64) * 64
    return -(-K // kspan), kspan


def ref_dist(z, E):
    z, E = z.double(), E.double()
    return (z * z).sum(1, keepdim=True) + (E * E).sum(0) - 2 * z @ E


def clear_margin(margin, dmin):
    """a row counts when its top-2 margin exceeds 1e-5 |d_min|."""
    return margin > 1e-5 * dmin.abs().clamp(min=1e-12)


# ---- MSE loss (vqa_runtime.hip)
def mse_grad(x, r, extra=None):
    """gscale32 * (r - x) (+ extra) in fp32, gscale32 = float32(2 / n)."""
    g = f32(2.0 / x.numel()) * (r - x)
    return g + extra if extra is not None else g


def mse_grad64(x, r, extra=None):
    g = (2.0 / x.numel()) * (r.double() - x.double())
    return g + extra.double() if extra is not None else g


# ---- Adam (vqa_optim.hip AdamStep)
def adam_mv(g, m, v, b1, b2, gs):
    """m += (g gs - m)(1 - b1), v += ((g gs)^2 - v)(1 - b2), every constant and operation in fp32."""
    gi = g * f32(gs)
    omb1, omb2 = f32(1.0) - f32(b1), f32(1.0) - f32(b2)
    return m + (gi - m) * omb1, v + (gi * gi - v) * omb2


def adam_mv64(g, m, v, b1, b2, gs):
    gi = g.double() * gs
    return m.double() + (gi - m.double()) * (1 - b1), v.double() + (gi * gi - v.double()) * (1 - b2)


# ---- layer norm (vqa_cond.hip), generic in the dtype
def ln_fwd(x, gamma, beta, eps=1e-6):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    inv = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * inv * gamma + beta


def ln_bwd(x, dy, gamma, eps=1e-6):
    """(dx, dgamma, dbeta): dx = inv (g - mean(g) - xhat mean(g xhat)), g = dy gamma."""
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    inv = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xhat = xc * inv
    g = dy * gamma
    dx = inv * ((g - g.mean(-1, keepdim=True)) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0)


def ln_inputs(C, rows, dt, seed=None):
    """x = 3 randn + 1 with row 0 constant (variance 0) and row 1 = 1000 + 1e-2 randn (mean >> spread); dy's rows
    weighted by edge_weights(rows, 64): the rows next to a 64-row edge carry the weight of dgamma / dbeta."""
    g = gen(C * 7 + rows if seed is None else seed)
    x = torch.randn(rows, C, generator=g) * 3 + 1
    x[0] = 2.5
    if rows > 1:
        x[1] = 1000 + 1e-2 * torch.randn(C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g) * edge_weights(rows, 64).float()[:, None]
    return x.to(dt), gamma, beta, dy.to(dt)
