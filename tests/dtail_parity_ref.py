"""Shared by the decoder-tail and spectral-loss parity tests (tests/test_gpu_dtail.py, test_dtail_parity_host.py,
test_gpu_spectral.py, test_spectral_parity_host.py): the launch plans restated from the launch code's constants, the
bounds, the two-layer oracle, and a plain fp64 restatement of the composed decoder tail that can be told to go wrong
the way a kernel does.

The composite (csrc/vqa_dtail.hip, header comment), h (B, T, 32), dy (B, 2T):
    u[s] = b_up + sum_{kb, j: s = 2j + kb - 1} W_up[kb] h[j]          y[t] = b_out + sum_k W_out[k] . u[t + k - 1]
 => y[2j + p] = bias + sum_{a = -1..1} sum_c V[a][c][p] h[j + a][c]   V[a][c][p] = sum_k sum_o W_out[k][o] W_up[p + k - 2a][o][c]
minus, at t = 0, tap k = 0 (edge vector e0[c] = sum_o W_out[0][o] W_up[0][o][c] and bias term b0 = W_out[0] . b_up) and,
at t = 2T - 1, tap k = 2 (e1 from W_out[2], W_up[3]; b2). The parameter gradients follow from dV = sum h (x) dy, the
edge sums Eh, Et and the dy sums S, F, L through the bilinear composition.
"""
import torch

from oracle import vqvae_ref as R

C = 32
F32, BF16 = torch.float32, torch.bfloat16

# ---- launch plans (csrc/vqa_dtail.hip: kDtU, kDtFwdWgs, kDtBwdWgs, kDtGroups, dt_gx, dt_part_row)
FWD_ROWS = 4 * 16 * 4      # 4 waves x 16 quads x kDtU rows per workgroup and pass
BWD_ROWS = 4 * 16 * 2
FWD_WGS, BWD_WGS, GROUPS = 768, 512, 16


def _gx(B, T, rows, total):
    return max(1, min(total // B, -(-T // rows)))


def fwd_plan(B, T):
    """(gx, passes of the busiest workgroup)"""
    gx = _gx(B, T, FWD_ROWS, FWD_WGS)
    return gx, -(-T // (gx * FWD_ROWS))


def bwd_plan(B, T):
    """(gx, P partial rows, stage-1 depth R of the two-stage reduction or 0 for the single stage, passes)"""
    gx = _gx(B, T, BWD_ROWS, BWD_WGS)
    P = gx * B
    two = P >= 4 * GROUPS and P % GROUPS == 0
    return gx, P, (P // GROUPS if two else 0), -(-T // (gx * BWD_ROWS))


def part_rows(B, T, p):
    """(item, [row ranges]) that workgroup p of the backward sums into its partial row"""
    gx, _, _, passes = bwd_plan(B, T)
    n, bx = divmod(p, gx)
    return n, [(j0, min(T, j0 + BWD_ROWS)) for j0 in range(bx * BWD_ROWS, T, gx * BWD_ROWS)]


# ---- the cases of tests/test_gpu_dtail.py: (B, T, Cu), with the plan each one is there for
FWD_CASES = {(768, 257): (1, 2), (768, 512): (1, 2), (384, 1300): (2, 3), (1000, 300): (1, 2)}       # -> (gx, passes)
BWD_CASES = {(4, 2048): (16, 64, 4, 1), (3, 3000): (24, 72, 0, 1), (65, 100): (1, 65, 0, 1),
             (512, 300): (1, 512, 32, 3)}                                                             # -> bwd_plan
CU_CASES = [1, 33, 65, 130, 1024]
EDGE_T = [1, 2, 3, 63, 64, 65, 255, 256, 257]
CHUNK = 64          # items per oracle call: u is (B, 2T, Cu) fp64

# ---- bounds
PROJECT = 2e-5      # of the reference's max-abs: y, fp32 dh, parameter gradients (the composite re-associates the sums)
BF16_REL = 2.0 ** -8  # one bf16 rounding of the stored dh: half an ulp of 2^-7, reached just above a power of two


def long_sums(B, Cu):
    """which outputs sum far more fp32 terms than the project's figure was set on: all of them for Cu >= 130, the
    parameter gradients for a batch the oracle has to take in chunks"""
    if Cu >= 130:
        return ("y", "dh", "dw_up", "db_up", "dw_out", "db_out")
    return ("dw_up", "db_up", "dw_out", "db_out") if B > CHUNK else ()


def bound(measured=None):
    """the project's figure, or 4 x the fp32 two-layer oracle's own error where that is larger (the factor 4: the
    composite associates the sums differently)"""
    return PROJECT if measured is None else max(PROJECT, 4.0 * measured)


def rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def bf16_dh_excess(got, ref, frac=PROJECT):
    """max over the elements of |got - ref| / (2^-8 |ref| + frac max|ref|): inside the bound when <= 1"""
    ref = ref.double()
    lim = BF16_REL * ref.abs() + frac * ref.abs().max()
    return float(((got.double() - ref).abs() / lim).max())


def params(Cu, seed):
    g = torch.Generator().manual_seed(seed)
    w_up = torch.randn(4, Cu, 32, generator=g) * 0.1
    b_up = torch.randn(Cu, generator=g) * 0.1
    w_out = torch.randn(3, Cu, 1, generator=g) * 0.1
    b_out = torch.randn(1, generator=g) * 0.1
    return w_up, b_up, w_out, b_out


def inputs(B, T, dt, seed=None):
    g = torch.Generator().manual_seed(B * 1000 + T if seed is None else seed)
    h = torch.randn(B, T, C, generator=g).to(dt)
    dy = torch.randn(B, 2 * T, 1, generator=g)
    return h, dy


NAMES = ("y", "dh", "dw_up", "db_up", "dw_out", "db_out")


def oracle(h, dy, w_up, b_up, w_out, b_out, dtype=torch.float64):
    """The two layers (oracle.vqvae_ref.conv1d_transpose, conv1d) and autograd, in chunks of CHUNK items; the
    parameter gradients of the chunks are summed in `dtype`. b_up / b_out None = zero. -> dict of NAMES"""
    Cu = w_up.shape[1]
    b_up = torch.zeros(Cu) if b_up is None else b_up
    b_out = torch.zeros(1) if b_out is None else b_out
    ys, dhs, acc = [], [], None
    for n0 in range(0, h.shape[0], CHUNK):
        hd = h[n0:n0 + CHUNK].to(dtype).clone().requires_grad_(True)
        ps = [p.to(dtype).clone().requires_grad_(True) for p in (w_up, b_up, w_out, b_out)]
        y = R.conv1d(R.conv1d_transpose(hd, ps[0], ps[1], 2), ps[2], ps[3])
        (y * dy[n0:n0 + CHUNK].to(dtype)).sum().backward()
        ys.append(y.detach())
        dhs.append(hd.grad)
        acc = [p.grad for p in ps] if acc is None else [a + p.grad for a, p in zip(acc, ps)]
    return dict(zip(NAMES, [torch.cat(ys), torch.cat(dhs)] + acc))


def fp32_oracle_error(ref, h, dy, w_up, b_up, w_out, b_out, names):
    """the same two-layer oracle in float32 on the CPU against its fp64 run: {name: error / max-abs}"""
    lo = oracle(h, dy, w_up, b_up, w_out, b_out, torch.float32)
    return {k: rel(lo[k], ref[k]) for k in names}


# ---- the composite, restated
DEFECTS = ("halo row dropped at the pass boundary", "halo row dropped at a wave boundary", "t = 0 edge omitted",
           "t = 2T - 1 edge omitted", "phases swapped on one row", "partial row lost", "partial row counted twice",
           "b_up dropped from dW_out")


def _kb(p, k, a):
    kb = p + k - 2 * a
    return kb if 0 <= kb <= 3 else None


def composite(h, dy, w_up, b_up, w_out, b_out, defect=None):
    """fp64, one defect planted at most. h (B, T, 32), dy (B, 2T, 1) -> dict of NAMES (shapes as the oracle's)."""
    assert defect is None or defect in DEFECTS
    h, dy = h.double(), dy.double().reshape(h.shape[0], -1)
    wu, wo = w_up.double(), w_out.double()[:, :, 0]                  # (4, Cu, 32), (3, Cu)
    Cu = wu.shape[1]
    bu = torch.zeros(Cu, dtype=torch.float64) if b_up is None else b_up.double()
    bo = 0.0 if b_out is None else float(b_out.double())
    B, T, _ = h.shape
    # Vk[k][a + 1][c][p]: tap k's share of V
    Vk = torch.zeros(3, 3, C, 2, dtype=torch.float64)
    for k in range(3):
        for a in (-1, 0, 1):
            for p in range(2):
                if _kb(p, k, a) is not None:
                    Vk[k, a + 1, :, p] = wo[k] @ wu[_kb(p, k, a)]
    V = Vk.sum(0)
    e0, e1 = wo[0] @ wu[0], wo[2] @ wu[3]
    bk = wo @ bu
    bias = bo + float(bk.sum())

    hp = torch.zeros(B, T + 2, C, dtype=torch.float64)
    hp[:, 1:T + 1] = h
    # A[a + 1][n, j, p] = sum_c V[a][c][p] h[j + a][c]
    A = [torch.einsum("njc,cp->njp", hp[:, 1 + a:1 + a + T], V[a + 1]) for a in (-1, 0, 1)]
    for name, row in (("halo row dropped at the pass boundary", FWD_ROWS), ("halo row dropped at a wave boundary", 64)):
        if defect == name:
            assert T > row
            A[0][:, row] = 0.0                                       # row's tap a = -1 comes from the halo row - 1
    y = bias + A[0] + A[1] + A[2]                                    # (B, T, 2)
    if defect != "t = 0 edge omitted":
        y[:, 0, 0] -= h[:, 0] @ e0
    y[:, 0, 0] -= bk[0]
    if defect != "t = 2T - 1 edge omitted":
        y[:, T - 1, 1] -= h[:, T - 1] @ e1
    y[:, T - 1, 1] -= bk[2]
    if defect == "phases swapped on one row":
        j = T // 2
        y[:, j] = y[:, j].flip(-1)
    y = y.reshape(B, 2 * T, 1)

    # dh[j][c] = sum_{a, p} V[a][c][p] dy[2 (j - a) + p]
    d2 = torch.zeros(B, T + 2, 2, dtype=torch.float64)
    d2[:, 1:T + 1] = dy.reshape(B, T, 2)
    win = [d2[:, 1 - a:1 - a + T] for a in (-1, 0, 1)]               # win[a + 1][n, j, p] = dy[2 (j - a) + p]
    dh = sum(torch.einsum("njp,cp->njc", win[a + 1], V[a + 1]) for a in (-1, 0, 1))
    dh[:, 0] -= dy[:, :1] * e0
    dh[:, T - 1] -= dy[:, 2 * T - 1:] * e1

    # the sums over the rows, each row weighted by how often its workgroup's partial row is counted
    wrow = torch.ones(B, T, dtype=torch.float64)
    if defect in ("partial row lost", "partial row counted twice"):
        P = bwd_plan(B, T)[1]
        n, spans = part_rows(B, T, P - 1 if P > 1 else 0)
        for j0, j1 in spans:
            wrow[n, j0:j1] = 0.0 if defect == "partial row lost" else 2.0
    hw = h * wrow[:, :, None]
    dV = torch.stack([torch.einsum("njc,njp->cp", hw, win[a + 1]) for a in (-1, 0, 1)])     # (3, C, 2)
    Eh = (hw[:, 0] * dy[:, :1]).sum(0)
    Et = (hw[:, T - 1] * dy[:, 2 * T - 1:]).sum(0)
    S = float((d2[:, 1:T + 1].sum(-1) * wrow).sum())
    Fs, L = float((dy[:, 0] * wrow[:, 0]).sum()), float((dy[:, 2 * T - 1] * wrow[:, T - 1]).sum())

    def dvk(k, a, p):
        x = dV[a + 1, :, p].clone()
        if k == 0 and a == 0 and p == 0:
            x -= Eh
        if k == 2 and a == 0 and p == 1:
            x -= Et
        return x

    sk = [S - Fs, S, S - L]
    dw_up = torch.zeros(4, Cu, C, dtype=torch.float64)
    dw_out = torch.zeros(3, Cu, dtype=torch.float64)
    for k in range(3):
        for a in (-1, 0, 1):
            for p in range(2):
                kb = _kb(p, k, a)
                if kb is not None:
                    dw_out[k] += wu[kb] @ dvk(k, a, p)
                    dw_up[kb] += wo[k][:, None] * dvk(k, a, p)[None, :]
        if defect != "b_up dropped from dW_out":
            dw_out[k] += bu * sk[k]
    db_up = sum(wo[k] * sk[k] for k in range(3))
    return {"y": y, "dh": dh, "dw_up": dw_up, "db_up": db_up, "dw_out": dw_out[:, :, None],
            "db_out": torch.tensor([S], dtype=torch.float64)}


# ---- spectral loss (tests/test_gpu_spectral.py, test_spectral_parity_host.py)
SPEC_MAG, SPEC_LOSS, SPEC_GRAD = 2e-6, 1e-5, 1e-4   # of the spectrum's max; relative; of the gradient's max-abs


def white_signals(B, T, seed):
    """x and r independent white noise at 0.3: no bin and no sample dominates, so bounds relative to a maximum bind on
    every bin and every sample"""
    g = torch.Generator().manual_seed(seed)
    return 0.3 * torch.randn(B, T, generator=g), 0.3 * torch.randn(B, T, generator=g)


def spectral_oracle(x, r, n_fft, hop, win, copies=1):
    """one resolution, fp64, item by item (the items are independent): magnitudes of x (B, F, n_fft/2 + 1), per-item
    loss, batch-mean loss, d(batch-mean loss)/dr. `copies` equal resolutions average to the same loss."""
    B = x.shape[0]
    mags, items, grads = [], [], []
    for b in range(B):
        rd = r[b].double().clone().requires_grad_(True)
        sx = R.spectral(x[b].double(), n_fft, hop, win)
        item = R.norm(sx - R.spectral(rd, n_fft, hop, win)) / R.norm(sx)
        (g,) = torch.autograd.grad(item / B, rd)
        mags.append(sx)
        items.append(item.detach())
        grads.append(g)
    items = torch.stack(items)
    return torch.stack(mags), items, float(items.mean()), torch.stack(grads)


def uncovered(T, hop, win):
    """bool (T,): samples no frame covers (between frames when hop > win, and past the last frame)"""
    F = 1 + (T - win) // hop
    m = torch.ones(T, dtype=torch.bool)
    for f in range(F):
        m[f * hop:f * hop + win] = False
    return m


def pair_walk(n_fft, cus):
    """(waves per workgroup, LDS bytes per workgroup, upper limit on resident workgroups per CU) of the frame-pair
    kernel for n_fft: launch_pairs (Stockham, kSpecWaves = 4; csrc/vqa_spectral_stockham.hip) / launch_pairs4
    (four-step, kSpec4Waves = 8; csrc/vqa_spectral_fourstep.hip); the limit is the smaller of 160 KiB / LDS and 32 wave
    slots / waves"""
    N = n_fft
    if N == 2048:
        waves, Pn = 8, N // 64
        lds = (Pn * (64 + 64 // Pn) + 64) * 8 + N * 4 + waves * (N + 64) * 8
    else:
        waves = 4
        lds = N * 8 + N * 4 + waves * (N + N // 8) * 8
    return waves, lds, min(160 * 1024 // lds, 32 // waves)
