"""Spectral-loss kernel parity (vqa_spectral*.hip) vs the CPU oracle in fp64.

Follows data_utils.py:25-40 (spectral / norm) and vqvae.py:309-326 (_multispectral_loss); the oracle's
gradient is torch autograd through rfft/abs (abs'(0) = 0, as TF). Tolerances (fp32 FFT vs fp64):
magnitudes 2e-6 of the spectrum's max, loss 1e-5 relative, gradient 1e-4 of its max-abs.

test_single_resolution and below use white noise (tests/dtail_parity_ref.white_signals: no bin and no sample
dominates, so the same three bounds bind on every bin and every sample) and take one resolution at a time, so each
of the two FFT implementations (the Stockham pair kernel for 256 / 512 / 1024, the four-step pair kernel for 2048) is
held to the bounds alone in each of its modes, at every frame geometry the layout accepts, with either gather kernel,
down to one frame per item, and on every item of a persistent walk of three pairs per wave. stft_magnitude is the pair
kernels' self-table mode (magnitude mode with the tables evaluated in the kernel): the bits of the target buffer.
"""
import numpy as np
import pytest
import torch

import dtail_parity_ref as D
import vqa_lib as V
from data_utils import STFT_ARGS, SpectralTarget, multispectral_loss_and_grad, spectral
from oracle import vqvae_ref as R

pytestmark = pytest.mark.gpu

RES = list(zip(*STFT_ARGS))  # (n_fft, hop, win) per resolution


def _signals(B, T, seed, recon_scale=0.3):
    x = torch.from_numpy(R.synthetic_batch(B, T, seed=seed))
    g = torch.Generator().manual_seed(seed + 1)
    r = recon_scale * torch.randn(B, T, 1, generator=g) + 0.5 * x
    return x, r


def _oracle(x, r):
    rd = r.double().clone().requires_grad_(True)
    per_item = R.multispectral_loss(x.double(), rd)
    loss = per_item.mean()
    (g,) = torch.autograd.grad(loss, rd)
    return float(loss.detach()), per_item.detach(), g


@pytest.mark.parametrize("n_fft,hop,win", RES + [(256, 64, 256), (512, 100, 300), (1024, 1, 7)])
def test_stft_magnitude(cuda, n_fft, hop, win):
    x, _ = _signals(3, 4096 + 37, seed=n_fft + win)
    got = spectral(x.squeeze(-1).to(cuda), n_fft, hop, win).cpu().double()
    ref = R.spectral(x.squeeze(-1).double(), n_fft, hop, win)
    assert got.shape == ref.shape
    err = (got - ref).abs().max() / ref.abs().max()
    assert err < 2e-6, err


@pytest.mark.parametrize("B,T", [(2, 8192), (3, 4096 + 113), (1, 1200), (4, 2048)])
def test_loss_and_grad(cuda, B, T):
    x, r = _signals(B, T, seed=B * 1000 + T)
    loss_ref, item_ref, g_ref = _oracle(x, r)
    tgt = SpectralTarget(x.to(cuda))
    loss, dr = multispectral_loss_and_grad(tgt, r.to(cuda))
    assert abs(float(loss) - loss_ref) / loss_ref < 1e-5
    g = dr.cpu().double()
    assert g.shape == g_ref.shape
    err = (g - g_ref).abs().max() / g_ref.abs().max()
    assert err < 1e-4, err
    # per-item losses through the C-ABI's item_loss output
    item = torch.empty(B, device=cuda)
    out = torch.empty(1, device=cuda)
    V.spectral_loss(tgt.x, r.to(cuda).reshape(B, T).contiguous(), out, None, item, *STFT_ARGS)
    assert torch.allclose(item.cpu().double(), item_ref, rtol=1e-5)
    assert float(out) == float(loss)  # loss-only mode = the same reduction


def test_full_size_deterministic(cuda):
    """cfg2 chunk length: bit-identical repeat, and loss/grad vs the oracle on 2 of the 32 items."""
    B, T = 32, 65536
    x, r = _signals(B, T, seed=7)
    tgt = SpectralTarget(x.to(cuda))
    rd = r.to(cuda)
    l1, g1 = multispectral_loss_and_grad(tgt, rd)
    l2, g2 = multispectral_loss_and_grad(tgt, rd)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    # items are independent: the batch-mean gradient of item b is (1/B) x its single-item gradient
    sub = [0, 31]
    loss_ref, item_ref, g_ref = _oracle(x[sub], r[sub])
    item = torch.empty(B, device=cuda)
    V.spectral_loss(tgt.x, rd.reshape(B, T), torch.empty(1, device=cuda), None, item, *STFT_ARGS)
    assert torch.allclose(item.cpu().double()[sub], item_ref, rtol=1e-5)
    g = g1.cpu().double()[sub] * (B / len(sub))
    err = (g - g_ref).abs().max() / g_ref.abs().max()
    assert err < 1e-4, err


def test_zero_bins_gradient(cuda):
    """abs'(0) = 0: a reconstruction that is exactly zero has zero spectral gradient (no NaN)."""
    B, T = 2, 4096
    x, _ = _signals(B, T, seed=3)
    r = torch.zeros(B, T, 1)
    loss, dr = multispectral_loss_and_grad(SpectralTarget(x.to(cuda)), r.to(cuda))
    assert abs(float(loss) - 1.0) < 1e-6  # ||S_x - 0|| / ||S_x||
    assert torch.count_nonzero(dr).item() == 0


def test_bad_shapes(cuda):
    x = torch.zeros(2, 1000, device=cuda)
    with pytest.raises(V.VQAError):
        V.spectral_loss_workspace(2, 1000, *STFT_ARGS)  # 1000 < win 1200
    with pytest.raises(V.VQAError):
        V.stft_magnitude(x, torch.empty(1, device=cuda), 4096, 10, 100)  # n_fft unsupported


@pytest.mark.parametrize("B,T", [(3, 4096 + 113), (2, 65536)])
def test_shared_target(cuda, B, T):
    """One vqa_spectral_target buffer serves several reconstructions (the levels of a train step) and gives
    the same bits as the one-call vqa_spectral_loss; odd frame counts exercise the unpaired last frame."""
    x, r = _signals(B, T, seed=11 + T)
    tgt = SpectralTarget(x.to(cuda))
    for k, scale in enumerate((0.3, 0.05)):
        rr = (scale * torch.randn(B, T, 1, generator=torch.Generator().manual_seed(k)) + 0.5 * x).to(cuda)
        l1, g1 = multispectral_loss_and_grad(tgt, rr)
        l0 = torch.empty(1, device=cuda)
        g0 = torch.empty(B, T, device=cuda)
        V.spectral_loss(tgt.x, rr.reshape(B, T), l0, g0, None, *STFT_ARGS)
        assert torch.equal(l0, l1) and torch.equal(g0, g1.reshape(B, T))
        l2, _ = multispectral_loss_and_grad(tgt, rr, need_grad=False)
        assert torch.equal(l1, l2)
    if T < 10000:
        loss_ref, _, g_ref = _oracle(x, rr.cpu())
        assert abs(float(l1) - loss_ref) / loss_ref < 1e-5
        err = (g1.cpu().double() - g_ref).abs().max() / g_ref.abs().max()
        assert err < 1e-4, err


@pytest.mark.parametrize("args", [
    [(512, 256), (20, 64), (300, 256)],                 # 15 frames over a sample: the general overlap-add
    [(2048, 1024, 512, 256, 512), (240, 120, 50, 64, 100), (1200, 600, 240, 256, 300)],  # 5 resolutions
    [(256,), (1,), (7,)],                                # hop 1
    [tuple(a) for a in STFT_ARGS],                       # the model's: the 8-frame gather
])
def test_gradient_overlap_add_forms(cuda, args):
    """The frame-gradient overlap-add runs as spec_gather8_kernel (<= 4 resolutions, <= 8 frames over a
    sample) or spec_gather_kernel (otherwise); both against the fp64 autograd oracle for these resolutions."""
    n_fft, hop, win = (list(a) for a in args)
    B, T = 2, 4096 + 77
    x, r = _signals(B, T, seed=len(n_fft) * 31 + hop[0])
    rd = r.double().squeeze(-1).clone().requires_grad_(True)
    xd = x.double().squeeze(-1)
    per = torch.stack([R.norm(R.spectral(xd, n, h, w) - R.spectral(rd, n, h, w)) / R.norm(R.spectral(xd, n, h, w))
                       for n, h, w in zip(n_fft, hop, win)], dim=-1).mean(dim=-1)
    (g_ref,) = torch.autograd.grad(per.mean(), rd)
    out = torch.empty(1, device=cuda)
    dr = torch.empty(B, T, device=cuda)
    V.spectral_loss(x.squeeze(-1).to(cuda).contiguous(), r.squeeze(-1).to(cuda).contiguous(), out, dr, None,
                    n_fft, hop, win)
    assert abs(float(out) - float(per.mean())) / float(per.mean()) < 1e-5
    err = (dr.cpu().double() - g_ref).abs().max() / g_ref.abs().max()
    assert err < 1e-4, err


@pytest.mark.parametrize("B,T", [(3, 4096 + 113), (1, 1200), (2, 8192 + 1)])
def test_pair_magnitudes_vs_oracle(cuda, B, T):
    """The target spectrograms as vqa_spectral_target writes them (the frame-pair kernel in its magnitude mode, both
    frames of a pair from one complex FFT; an odd frame count leaves the last frame unpaired), read out of the
    target buffer by its layout (per resolution: twiddles 2N | window | |S_x| (B*F, N/2 + 1), each 64-float
    aligned), against the oracle's |tf.signal.stft| at 2e-6 of the spectrum's max."""
    x, _ = _signals(B, T, seed=5 + T)
    tgt = SpectralTarget(x.to(cuda))
    buf = tgt.mags.view(torch.float32).cpu() if tgt.mags.dtype != torch.float32 else tgt.mags.cpu()
    al = lambda n: (n + 63) // 64 * 64  # noqa: E731
    o = 0
    for n_fft, hop, win in RES:
        F = 1 + (T - win) // hop
        o += al(2 * n_fft) + al(win)
        got = buf[o:o + B * F * (n_fft // 2 + 1)].double().reshape(B, F, n_fft // 2 + 1)
        o += al(B * F * (n_fft // 2 + 1))
        ref = R.spectral(x.squeeze(-1).double(), n_fft, hop, win)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        err = (got - ref).abs().max() / ref.abs().max()
        assert err < 2e-6, (n_fft, float(err))


# ------------------------------------------------------------------ one resolution at a time, white noise
def _target_mags(xd, B, T, n_fft, hop, win):
    """|S_x| as vqa_spectral_target leaves it (the pair kernel's magnitude mode), read by the buffer's layout"""
    buf = V.spectral_target(xd, [n_fft], [hop], [win]).view(torch.float32).cpu()
    al = lambda n: (n + 63) // 64 * 64  # noqa: E731
    F, KB = 1 + (T - win) // hop, n_fft // 2 + 1
    o = al(2 * n_fft) + al(win)
    return buf[o:o + B * F * KB].double().reshape(B, F, KB)


def _loss_grad(xd, rd, res, copies, grad=True):
    B, T = xd.shape
    a = [[v] * copies for v in res]
    out, item = torch.full((1,), float("nan"), device=xd.device), torch.full((B,), float("nan"), device=xd.device)
    dr = torch.full((B + 2, T), float("nan"), device=xd.device) if grad else None     # one guard item either side
    ws = V.workspace(V.spectral_loss_workspace(B, T, *a, with_grad=grad), xd.device)
    V.spectral_loss(xd, rd, out, dr[1:B + 1] if grad else None, item, *a, ws=ws)
    torch.cuda.synchronize()
    if grad:
        assert bool(torch.isnan(dr[[0, B + 1]]).all()), "gradient written outside its items"
        dr = dr[1:B + 1].cpu()
    return out.cpu(), item.cpu(), dr


def _single(cuda, B, T, n_fft, hop, win, tag):
    """every mode of one resolution against the fp64 oracle; returns the figures"""
    x, r = D.white_signals(B, T, seed=n_fft + 7 * hop + win + B)
    m_ref, item_ref, loss_ref, g_ref = D.spectral_oracle(x, r, n_fft, hop, win)
    xd, rd = x.to(cuda).contiguous(), r.to(cuda).contiguous()
    F, KB = 1 + (T - win) // hop, n_fft // 2 + 1
    smax = m_ref.abs().max()
    # magnitude mode of the pair kernel, and its self-table mode (vqa_stft_magnitude; "frame" in the figures): the
    # same table formulas and the same instructions after the prologue, so the same bits, and stores by frame
    # (one guard frame either side of the output stays NaN)
    tm = _target_mags(xd, B, T, n_fft, hop, win)
    e_pair = float((tm - m_ref).abs().max() / smax)
    guard = torch.full((B * F + 2, KB), float("nan"), device=cuda)
    fm = guard[1:B * F + 1].view(B, F, KB)
    V.stft_magnitude(xd, fm, n_fft, hop, win)
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard[[0, B * F + 1]]).all()), "magnitudes written outside their frames"
    e_frame = float((fm.cpu().double() - m_ref).abs().max() / smax)
    same_bits = torch.equal(fm.cpu().view(torch.int32), tm.float().view(torch.int32))
    # gradient mode (the 8-frame gather while <= 8 frames cover a sample) and loss-only mode
    loss, item, g = _loss_grad(xd, rd, (n_fft, hop, win), 1)
    e_loss = abs(float(loss) - loss_ref) / loss_ref
    e_item = float(((item.double() - item_ref).abs() / item_ref).max())
    e_grad = float((g.double() - g_ref).abs().max() / g_ref.abs().max())
    loss0, item0, _ = _loss_grad(xd, rd, (n_fft, hop, win), 1, grad=False)
    print(f"PARITY spectral {tag} n_fft={n_fft} hop={hop} win={win} B={B} T={T} F={F} magnitudes pair {e_pair:.2e} "
          f"frame {e_frame:.2e} (bound {D.SPEC_MAG:.0e}) loss {e_loss:.2e} item {e_item:.2e} (bound {D.SPEC_LOSS:.0e}) "
          f"gradient {e_grad:.2e} (bound {D.SPEC_GRAD:.0e})")
    assert e_pair < D.SPEC_MAG and e_frame < D.SPEC_MAG, (e_pair, e_frame)
    assert same_bits, "vqa_stft_magnitude differs from the target buffer's magnitudes"
    assert e_loss < D.SPEC_LOSS and e_item < D.SPEC_LOSS, (e_loss, e_item)
    assert e_grad < D.SPEC_GRAD, e_grad
    assert torch.equal(loss0.view(torch.int32), loss.view(torch.int32)) and torch.equal(item0, item)
    # samples no frame covers (between frames when hop > win; past the last frame): an exact zero
    gap = D.uncovered(T, hop, win)
    assert (hop > win) == bool(gap[:(F - 1) * hop + win].any())
    assert torch.count_nonzero(g[:, gap]).item() == 0
    return xd, rd, g, loss_ref, g_ref


def _five_copies(xd, rd, res, g, loss_ref, g_ref):
    """the same resolution five times: more than kGatherMaxRes = 4 forces spec_gather_kernel, and the five equal
    terms average to the same loss. Both gathers sum a sample's frames in the same order, so the sums agree to the
    bit; the scale they are multiplied by does not (1 / (5 B) for 1 / B, rounded once each, and five products
    added), which is worth at most 12 roundings of 2^-24 with no cancellation (five equal terms): every element
    within 16 x 2^-24 of its own size, zeros exact."""
    loss5, _, g5 = _loss_grad(xd, rd, res, 5)
    assert abs(float(loss5) - loss_ref) / loss_ref < D.SPEC_LOSS
    assert float((g5.double() - g_ref).abs().max() / g_ref.abs().max()) < D.SPEC_GRAD
    assert bool(((g5.double() - g.double()).abs() <= 16 * 2.0 ** -24 * g.double().abs()).all())
    assert torch.equal(g5 == 0, g == 0)


def _geometries(n_fft):
    win = (n_fft * 5 // 8) | 1                       # odd, < n_fft: 161, 321, 641, 1281
    return [(n_fft // 4, n_fft), (win // 5 + 1, win), (win, win), (win + 13, win)]


@pytest.mark.parametrize("n_fft,hop,win", [(n, h, w) for n in (256, 512, 1024, 2048) for h, w in _geometries(n)])
def test_single_resolution(cuda, n_fft, hop, win):
    """full window without zero padding; an odd window; hop == win; hop > win (gaps between the frames)"""
    B, T = 3, 3 * n_fft + 37
    assert (win + hop - 1) // hop <= 8                # alone: spec_gather8_kernel (kGatherMaxF)
    xd, rd, g, loss_ref, g_ref = _single(cuda, B, T, n_fft, hop, win, "single")
    _five_copies(xd, rd, (n_fft, hop, win), g, loss_ref, g_ref)


@pytest.mark.parametrize("B,T,F", [(1, 300, 1), (4, 300, 1), (3, 400, 2), (2, 500, 3)])
def test_frame_count_edges(cuda, B, T, F):
    """F = 1 with B = 1: a lone half pair; F = 1 with B = 4: every pair straddles two items; F = 2; F = 3"""
    n_fft, hop, win = 512, 100, 300
    assert 1 + (T - win) // hop == F
    xd, rd, g, loss_ref, g_ref = _single(cuda, B, T, n_fft, hop, win, "frames")
    _five_copies(xd, rd, (n_fft, hop, win), g, loss_ref, g_ref)


@pytest.mark.parametrize("n_fft,hop,win", [(256, 8, 64), (2048, 16, 256)])
def test_persistent_walk_every_item(cuda, n_fft, hop, win):
    """grid = min(groups, CUs x resident): sized so that every wave of the pair kernel (Stockham at 256, four-step at
    2048) takes at least three pairs whatever the occupancy query answers, and every item's magnitudes, loss and
    gradient are compared with the oracle."""
    B = 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves, lds, limit = D.pair_walk(n_fft, cus)
    need = 3 * cus * limit * waves
    F = -(-2 * need // B)
    T = win + (F - 1) * hop
    pairs = (B * F + 1) // 2
    assert pairs >= need and pairs // (cus * limit * waves) >= 3 and T < 400000
    print(f"PARITY spectral walk n_fft={n_fft} CUs={cus} waves/workgroup={waves} LDS={lds} resident limit={limit} "
          f"pairs={pairs} >= 3 x {cus * limit * waves} waves; B={B} T={T} F={F}")
    _single(cuda, B, T, n_fft, hop, win, "walk")
