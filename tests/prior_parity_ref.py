"""Plain references and bounds shared by the prior's kernel-level parity suites (tests/test_gpu_seqlin.py,
tests/test_gpu_head.py, tests/test_gpu_prior_glue.py) and their CPU-only checks (tests/test_prior_parity_host.py).

The sequence-linear layer is written out as a per-tap shifted matmul, generic in the dtype: evaluated in fp64 it is
the reference, evaluated in fp32 on the same rounded inputs its error e32 against fp64 sizes the bound of a long sum:
bound = max(project bound, 8 * e32). The factor 8 covers a different, chunked accumulation order (MFMA K blocks,
per-segment partials, a second-stage reduction); it is never taken from a kernel's own error.
Project bounds (relative to max |ref|): seqlin 2e-6 fp32 / 2e-2 bf16, head 1e-5 / 3e-2.
"""
import os

import torch

SEQLIN_TOL = {torch.float32: 2e-6, torch.bfloat16: 2e-2}
HEAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 3e-2}
# Weight gradients (seqlin dW / db, head db) are fp32 sums of products of the rounded inputs; a bf16 x bf16 product is
# exact in fp32 and the kernels accumulate in fp32, so these outputs obey the fp32 bound in bf16 too. (The project's
# bf16 figure would hide one lost row of a 600-row sum: tests/test_prior_parity_host.py.)
WGRAD_TOL = 2e-6
HEAD_DB_TOL = 2e-5
REPORT = os.environ.get("VQA_PARITY_REPORT")  # a file to append every case's figures to (unset: no table)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def shift_rows(x, s):
    """z[:, t] = x[:, t + s] inside [0, T), zero outside."""
    T = x.shape[1]
    z = torch.zeros_like(x)
    if s == 0:
        return x
    if abs(s) >= T:
        return z
    if s < 0:
        z[:, -s:] = x[:, :T + s]
    else:
        z[:, :T - s] = x[:, s:]
    return z


def seqlin_ref(x, w, b=None, dir=-1, r=None, y0=None):
    """y[t] = sum_tap x[t + dir * (taps - 1 - tap)] @ w[tap] (+ b) (+ r) (+ y0); x (nseq, T, K), w (taps, K, N)."""
    taps = w.shape[0]
    y = None
    for tap in range(taps):
        term = shift_rows(x, dir * (taps - 1 - tap)) @ w[tap]
        y = term if y is None else y + term
    if b is not None:
        y = y + b
    if r is not None:
        y = y + r
    if y0 is not None:
        y = y + y0
    return y


def seqlin_wgrad_ref(x, dy, taps):
    """dW[tap] = sum_t x[t - (taps - 1 - tap)]^T dy[t], db = sum_t dy[t] (the forward direction dir = -1)."""
    K, N = x.shape[-1], dy.shape[-1]
    dw = torch.stack([shift_rows(x, -(taps - 1 - tap)).reshape(-1, K).t() @ dy.reshape(-1, N) for tap in range(taps)])
    return dw, dy.reshape(-1, N).sum(0)


def e32_of(fn, *tensors):
    """Error of fn evaluated in fp32 against fn in fp64 on the same (already rounded) inputs, relative to
    max |fp64 result|; fn returns a tensor or a tuple of tensors (one figure each)."""
    hi = fn(*[t.double() if t is not None else None for t in tensors])
    lo = fn(*[t.float() if t is not None else None for t in tensors])
    if isinstance(hi, tuple):
        return tuple(rel(a, b) for a, b in zip(lo, hi))
    return rel(lo, hi)


def bound(project, e32):
    return max(project, 8.0 * e32)


def record(group, case, e32, bnd, err):
    """One line per case into the measured table (profiles/prior_kernel_parity.txt is a copy of one run's)."""
    line = f"{group:14s} {case:58s} e32 {e32:9.3e} bound {bnd:9.3e} err {err:9.3e} ratio {err / bnd:6.3f}"
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


def edge_weights(T, chunk=64, gain=8.0):
    """Per-row gains that put the weight of a sum on the rows next to a chunk edge (t % chunk in {0, chunk - 1}):
    a kernel that loses an edge row of a tile or chunk then misses a visible share of the sum."""
    t = torch.arange(T)
    m = (t % chunk == 0) | (t % chunk == chunk - 1)
    return torch.where(m, torch.tensor(gain), torch.tensor(1.0)).double()


def head_inputs(M, Vb, dt, seed=None):
    """(x in dt, W fp32, bias, targets) of a head case. The rows next to a 64-row chunk edge (every segment edge is
    one) and the last row carry 4x the weight: V > M leaves most vocabulary columns one target row, so max |dW| is
    about one row's contribution, and with unit rows one lost row moves dW by 0.4 of it, inside 10x the bf16 bound
    (6e-2); with these gains a lost edge row moves it by 0.7 (tests/test_prior_parity_host.py)."""
    g = gen(M + Vb if seed is None else seed)
    ew = edge_weights(M, 64, 4.0).float()
    ew[-1] = 4.0
    x = (torch.randn(M, 128, generator=g) * ew[:, None]).to(dt)
    w = torch.randn(128, Vb, generator=g) / 8
    b = torch.randn(Vb, generator=g)
    tgt = torch.randint(0, Vb, (M,), generator=g)
    tgt[0] = Vb - 1
    tgt[-1] = 0 if M > 1 else Vb - 1
    if M > 2:
        tgt[1] = 0
    return x, w, b, tgt
