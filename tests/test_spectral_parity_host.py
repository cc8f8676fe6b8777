"""CPU-only side of the spectral loss's parity suite: a numpy fp64 restatement of what csrc/vqa_spectral.hip computes
(two real frames through one complex FFT and the split of its bins, the per-item loss, the Hermitian extension and
the inverse transform of the pair, the overlap-add gather with its f_lo / f_hi rule) against oracle.vqvae_ref.spectral
and autograd at 1e-12, and the sensitivity of the bounds of tests/test_gpu_spectral.py (magnitudes 2e-6 of the
spectrum's max, loss 1e-5 relative, gradient 1e-4 of its max-abs): the restatement damaged the way a kernel goes wrong
must break them on the white-noise family. The same defects on the older family (a 0.5 sine plus 0.05 noise, at the
model's three resolutions) are measured beside it: what that family lets through is why the white one was added.
"""
import numpy as np
import pytest
import torch

import dtail_parity_ref as D
from oracle import vqvae_ref as R

DEFECTS = ("Nyquist bin of the second frame from the first", "conjugate lost in the split",
           "unpaired last frame skipped", "straddling pair's second frame credited to the first's item",
           "f_lo one too high at t == win", "frame j = 8 dropped from the gather")


def _hann(win):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)


def _frames(x, N, hop, win):
    B, T = x.shape
    F = 1 + (T - win) // hop
    idx = hop * np.arange(F)[:, None] + np.arange(win)[None, :]
    fr = np.zeros((B * F, N))
    fr[:, :win] = (x[:, idx] * _hann(win)).reshape(B * F, win)
    return fr, F


def _pair_spectra(fr, N, defect):
    """rfft of every frame, two frames per complex FFT: z = a + i b, A[k] = (Z[k] + conj Z[N - k]) / 2,
    B[k] = (Z[k] - conj Z[N - k]) / 2i. The frame count is made even with a copy of the last frame."""
    n = fr.shape[0]
    if n % 2:
        fr = np.concatenate([fr, fr[-1:]])
    Z = np.fft.fft(fr[0::2] + 1j * fr[1::2], axis=-1)
    KB = N // 2 + 1
    Zk, Zm = Z[:, :KB], Z[:, (N - np.arange(KB)) % N]
    if defect != "conjugate lost in the split":
        Zm = np.conj(Zm)
    A, Bq = 0.5 * (Zk + Zm), (Zk - Zm) / 2j
    if defect == "Nyquist bin of the second frame from the first":
        Bq[:, N // 2] = A[:, N // 2]
    S = np.empty((2 * A.shape[0], KB), dtype=complex)
    S[0::2], S[1::2] = A, Bq
    return S[:n]


def restate(x, r, N, hop, win, nres=1, defect=None):
    """one resolution -> (|S_x| (B, F, N/2 + 1), per-item loss (B,), d(mean_b loss / nres)/dr (B, T))"""
    B, T = x.shape
    fx, F = _frames(x, N, hop, win)
    fr, _ = _frames(r, N, hop, win)
    n = B * F
    Sx, Sr = _pair_spectra(fx, N, defect), _pair_spectra(fr, N, defect)
    mx, mr = np.abs(Sx), np.abs(Sr)
    live = np.ones(n, dtype=bool)
    if defect == "unpaired last frame skipped" and n % 2:
        live[-1] = False
        mx[-1] = 0.0
    item = np.arange(n) // F
    if defect == "straddling pair's second frame credited to the first's item":
        odd = np.arange(1, n, 2)
        item[odd] = item[odd - 1]
    sd = np.zeros(B)
    sx = np.zeros(B)
    np.add.at(sd, item, ((mx - mr) ** 2).sum(-1) * live)
    np.add.at(sx, item, (mx ** 2).sum(-1) * live)
    with np.errstate(invalid="ignore", divide="ignore"):   # a defect may leave an item without frames: NaN, as on the device
        loss = np.sqrt(sd) / np.sqrt(sx)
        scale = 1.0 / (nres * B) / (np.sqrt(sd) * np.sqrt(sx))
    # dL/dS_r per bin, Hermitian extension (G / 2 inside, G at k = 0 and N / 2), pair H_a + i H_b through one inverse
    G = np.where(mr > 0, (mr - mx) / np.where(mr > 0, mr, 1.0), 0.0) * Sr * live[:, None]
    H = np.zeros((n + n % 2, N), dtype=complex)
    H[:n, 0], H[:n, N // 2] = G[:, 0].real, G[:, N // 2].real
    H[:n, 1:N // 2] = 0.5 * G[:, 1:N // 2]
    H[:n, N // 2 + 1:] = 0.5 * np.conj(G[:, 1:N // 2][:, ::-1])
    hh = np.fft.ifft(H[0::2] + 1j * H[1::2], axis=-1) * N
    g = np.empty((n + n % 2, N))
    g[0::2], g[1::2] = hh.real, hh.imag
    fg = (g[:n, :win] * _hann(win) * scale[item][:, None]).reshape(-1)       # frame gradients, (B F, win) flat
    # overlap-add: sample t gathers frames f_lo .. f_hi
    t = np.arange(T)
    f_hi = np.minimum(F - 1, t // hop)
    f_lo = np.where(t >= win, (t - win) // hop + 1, 0)
    if defect == "f_lo one too high at t == win":
        f_lo[t == win] += 1
    dr = np.zeros((B, T))
    for j in range(int((f_hi - f_lo).max()) + 1):
        if j == 8 and defect == "frame j = 8 dropped from the gather":
            continue
        f = f_lo + j
        ok = f <= f_hi
        fc = np.minimum(f, f_hi)
        off = np.clip(t - fc * hop, 0, win - 1)
        for b in range(B):
            dr[b] += np.where(ok, fg[(b * F + fc) * win + off], 0.0)
    return mx.reshape(B, F, -1), loss, dr


def restate_mix(x, r, res, defect=None):
    out = [restate(x, r, n, h, w, len(res), defect) for n, h, w in res]
    return [o[0] for o in out], sum(o[1] for o in out) / len(res), sum(o[2] for o in out)


def oracle_mix(x, r, res):
    xd = torch.from_numpy(x)
    rd = torch.from_numpy(r).clone().requires_grad_(True)
    mags = [R.spectral(xd, n, h, w) for n, h, w in res]
    per = torch.stack([R.norm(m - R.spectral(rd, n, h, w)) / R.norm(m) for m, (n, h, w) in zip(mags, res)], -1).mean(-1)
    (g,) = torch.autograd.grad(per.mean(), rd)
    return [m.numpy() for m in mags], per.detach().numpy(), g.numpy()


def excess(got, ref):
    """error / bound of the three figures tests/test_gpu_spectral.py checks: (magnitudes, loss, gradient)"""
    (gm, gl, gg), (rm, rl, rg) = got, ref
    mag = max(float(np.abs(a - b).max() / b.max()) for a, b in zip(gm, rm)) / D.SPEC_MAG
    loss = abs(float(gl.mean()) - float(rl.mean())) / float(rl.mean()) / D.SPEC_LOSS
    grad = float(np.abs(gg - rg).max() / np.abs(rg).max()) / D.SPEC_GRAD
    return tuple(e if np.isfinite(e) else float("inf") for e in (mag, loss, grad))   # a NaN fails every comparison


def _white(B, T, seed):
    x, r = D.white_signals(B, T, seed)
    return x.double().numpy(), r.double().numpy()


def _sine(B, T, seed):
    """the older family of tests/test_gpu_spectral.py (_signals)"""
    x = torch.from_numpy(R.synthetic_batch(B, T, seed=seed))
    r = 0.3 * torch.randn(B, T, 1, generator=torch.Generator().manual_seed(seed + 1)) + 0.5 * x
    return x.squeeze(-1).double().numpy(), r.squeeze(-1).double().numpy()


# odd B F (an unpaired last frame), odd F with B > 1 (pairs straddle items), 16 frames over a sample (j = 8 exists)
WHITE = [(3, 805, [(256, 64, 256)]), (3, 1573, [(512, 61, 301)]), (2, 1000, [(2048, 16, 256)]),
         (3, 1100, [(1024, 300, 300)]), (3, 700, [(256, 113, 100)]), (4, 300, [(512, 100, 300)])]
MODEL = [tuple(a) for a in R.STFT_ARGS]


@pytest.mark.parametrize("B,T,res", WHITE + [(3, 4096 + 113, MODEL), (1, 300, [(512, 100, 300)])])
def test_restatement_matches_the_oracle(B, T, res):
    x, r = _white(B, T, seed=B + T)
    got, ref = restate_mix(x, r, res), oracle_mix(x, r, res)
    for a, b in zip(got[0], ref[0]):
        assert a.shape == b.shape and np.abs(a - b).max() / b.max() < 1e-12
    assert np.abs(got[1] - ref[1]).max() / ref[1].max() < 1e-12
    assert np.abs(got[2] - ref[2]).max() / np.abs(ref[2]).max() < 1e-12
    # samples no frame covers: an exact zero
    for n, h, w in res[:1] if len(res) == 1 else []:
        assert np.count_nonzero(got[2][:, D.uncovered(T, h, w).numpy()]) == 0


def test_bounds_see_every_planted_defect_on_white_noise(capsys):
    worst = {d: 0.0 for d in DEFECTS}
    for B, T, res in WHITE:
        x, r = _white(B, T, seed=B + T)
        ref = restate_mix(x, r, res)
        for d in DEFECTS:
            e = excess(restate_mix(x, r, res, d), ref)
            worst[d] = max(worst[d], *e)
            with capsys.disabled():
                print(f"PARITY spectral defect white B={B} T={T} {res[0]} {d:60s} error / bound: magnitudes {e[0]:9.3g} "
                      f"loss {e[1]:9.3g} gradient {e[2]:9.3g}")
    for d, w in worst.items():
        assert w > 1.0, (d, w)


def test_what_the_sine_family_at_the_model_resolutions_lets_through(capsys):
    """The older inputs (one spectral line two orders above the rest) at the model's three resolutions, B = 3,
    T = 4096 + 113 (13, 31 and 80 frames per item: odd B F and straddling pairs in the first two). Measured in fp64:
    the gather never has a frame j = 8 there (5 frames over a sample), so that defect is invisible to any input at
    these resolutions. The other two of the last three ARE caught by the old family in fp64 (straddling pair: loss
    20 x, gradient 420 x the bound; f_lo: gradient 87 x), so no claim is made that its bounds let them through: what
    the old tests lacked for them was coverage (one resolution alone, every item of a persistent walk, F = 1), not a
    sharper input. The figures are printed and kept in profiles/dtail_spectral_parity.txt."""
    B, T = 3, 4096 + 113
    x, r = _sine(B, T, seed=B * 1000 + T)
    ref = restate_mix(x, r, MODEL)
    seen = {}
    for d in DEFECTS:
        e = excess(restate_mix(x, r, MODEL, d), ref)
        seen[d] = e
        with capsys.disabled():
            print(f"PARITY spectral defect sine  B={B} T={T} model resolutions {d:60s} error / bound: magnitudes "
                  f"{e[0]:9.3g} loss {e[1]:9.3g} gradient {e[2]:9.3g} -> {'caught' if max(e) > 1 else 'PASSES'}")
    assert max(seen["frame j = 8 dropped from the gather"]) == 0.0
