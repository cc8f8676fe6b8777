"""Codes -> audio on the GPU: VQVAE.decode_chunked / render against the whole-sequence decode and the fp64 oracle,
the refusal of codes outside the codebook, and VQVAESampler.sample_audio end to end with the WAV writer.

Models: 2 levels, down_depth [3, 2], residual depth 3, dilation 3 — width 32 (the fused residual block and the fused
decoder tail) and width 8 (the gather route) — B = 2, 300 codes. The halos are 30 (level 0) and 34 (level 1) codes,
so chunks of 128, 100 and 37 codes give interior chunks, a short last one, and inputs clamped at both ends; 1000 is
one chunk. Every model's whole-sequence decodes and the oracle's are computed once and shared.

Measured on an MI355X (relative L2 per item, the worst item; a run with -s prints every figure):
  fp32 whole vs fp64 oracle 3.0e-7 .. 5.3e-7 (bound 1e-4); bf16 whole vs fp32 whole 6.2e-3 .. 1.1e-2;
  chunked vs whole exactly 0 at every chunk size, level and width, in fp32 and in bf16 (the kernels' arithmetic does
  not depend on where a sample lies in its tensor), so render differs from the quantised whole decode by 0 LSB and
  the clip counts equal numpy's.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]

from oracle import vqvae_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, CODES, K, D = 2, 300, 64, 16
CHUNKS = (1000, 128, 100, 37)
FORWARD_BOUND = 1e-4  # tests/test_gpu_train.py's bound of a forward against the oracle
_CASES = {}


def _cfg(width):
    return R.RefConfig(input_len=2048, levels=2, latent_dim=D, down_depth=[3, 2], strides=[2, 2], num_embeddings=K,
                       residual_width=width, residual_depth=3, dilation_factor=3)


def _state(width):
    cfg = _cfg(width)
    params, vq = R.init_params(cfg, 31), R.init_vq_state(cfg, 32)
    rng = np.random.default_rng(33)
    for n in params:  # zero biases would make a padded edge look more like an interior than it does in a trained model
        if n.endswith("/bias"):
            params[n] = rng.uniform(-0.1, 0.1, size=params[n].shape).astype(np.float32)
    for st in vq:     # codebook entries of the size of trained latents
        st["embeddings"] = (st["embeddings"] * 20.0).astype(np.float32)
    return cfg, params, vq


def _model(width, dtype):
    from vqvae import VQVAE
    cfg, params, vq = _state(width)
    m = VQVAE((cfg.input_len, 1), cfg.levels, cfg.latent_dim, cfg.down_depth, cfg.strides, num_embeddings=K,
              residual_width=width, residual_depth=3, dilation_factor=3, dtype=dtype, device="cuda:0")
    m.set_weights(params)
    m.set_vq_state(vq)
    return m


def _codes():
    return torch.from_numpy(np.random.default_rng(34).integers(0, K, size=(2, B, CODES)))  # [level]


def _case(width):
    """(fp32 model, bf16 model, codes per level on the device, per level: oracle decode, fp32 whole, bf16 whole)."""
    if width not in _CASES:
        cfg, params, vq = _state(width)
        ref = R.RefVQVAE(cfg, params, vq, dtype=torch.float64)
        codes = _codes()
        m32, m16 = _model(width, "fp32"), _model(width, "bf16")
        dev = [codes[l].cuda() for l in range(2)]
        per = []
        for l in range(2):
            per.append(dict(oracle=ref.decode(codes[l], l).numpy(), whole32=m32.decode(dev[l], l).cpu().numpy(),
                            whole16=m16.decode(dev[l], l).cpu().numpy()))
        _CASES[width] = (m32, m16, dev, per)
    return _CASES[width]


def _item_l2(a, b):
    """Relative L2 error of a against b per item, the worst item."""
    a, b = np.asarray(a, np.float64).reshape(B, -1), np.asarray(b, np.float64).reshape(B, -1)
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)))


def test_halo_and_hops_of_the_test_models(cuda):
    m32 = _case(32)[0]
    assert [m32.decode_halo(l) for l in range(2)] == [30, 34]
    assert m32.decode_hops == [8, 32] == list(m32.hops)
    assert _case(8)[0].decode_halo(0) == 30  # the halo does not depend on the width


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("width", [32, 8])
def test_chunked_decode_equals_whole_fp32(cuda, width, level):
    m32, _, dev, per = _case(width)
    p = per[level]
    hop = m32.decode_hops[level]
    assert p["whole32"].shape == (B, CODES * hop, 1)
    err_oracle = _item_l2(p["whole32"], p["oracle"])
    print(f"width {width} level {level}: fp32 whole vs oracle {err_oracle:.3e}")
    assert 0.0 < err_oracle < FORWARD_BOUND
    for chunk in CHUNKS:
        y = m32.decode_chunked(dev[level], level, chunk_codes=chunk)
        assert y.shape == (B, CODES * hop, 1) and y.dtype == torch.float32
        err = _item_l2(y.cpu().numpy(), p["whole32"])
        print(f"  chunk {chunk}: chunked vs whole {err:.3e}")
        assert err <= err_oracle, (chunk, err, err_oracle)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("width", [32, 8])
def test_chunked_decode_equals_whole_bf16(cuda, width, level):
    _, m16, dev, per = _case(width)
    p = per[level]
    bound = _item_l2(p["whole16"], p["whole32"])  # what bf16 activations cost this model
    print(f"width {width} level {level}: bf16 whole vs fp32 whole {bound:.3e}")
    assert 0.0 < bound < 0.1
    for chunk in CHUNKS:
        y = m16.decode_chunked(dev[level], level, chunk_codes=chunk)
        err = _item_l2(y.cpu().numpy(), p["whole16"])
        print(f"  chunk {chunk}: chunked vs whole {err:.3e}")
        assert err <= bound, (chunk, err, bound)


def _restate(x, gain=1.0):
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(x, np.float32) * np.float32(gain)) * np.float32(32768.0)
        r = np.rint(v)
        bad = np.isnan(v) | (r > 32767) | (r < -32768)
        return np.where(np.isnan(v), np.float32(0), np.clip(r, -32768, 32767)).astype(np.int16), bad.sum(axis=-1)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("peak", [0.9, 1.5])
def test_render_matches_the_quantised_decode(cuda, peak, level):
    """The output conv's kernel and bias rescaled (the decoder is linear in them) so that the peak of decode(zq) is
    0.9 (nothing clips) or 1.5 (it clips)."""
    m = _model(32, "fp32")
    zq = _codes()[level].cuda()
    scale = peak / float(m.decode(zq, level).abs().max())
    w = m.get_weights()
    m.set_weights({n: w[n] * np.float32(scale) for n in (f"dec{level}/out/kernel", f"dec{level}/out/bias")})
    whole = m.decode(zq, level)
    assert abs(float(whole.abs().max()) - peak) < 1e-3
    chunk = 100
    fdiff = float((m.decode_chunked(zq, level, chunk_codes=chunk) - whole).abs().max())
    lsb = int(np.ceil(fdiff * 32768.0)) + 1
    want, count = _restate(whole.cpu().numpy()[:, :, 0])
    pcm, clipped = m.render(zq, level, chunk_codes=chunk)
    assert pcm.shape == whole.shape[:2] and pcm.dtype == torch.int16 and pcm.is_cuda
    assert clipped.shape == (B,) and clipped.dtype == torch.int32
    got = pcm.cpu().numpy()
    worst = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max())
    print(f"peak {peak} level {level}: float diff {fdiff:.3e} -> bound {lsb} LSB, worst {worst} LSB, "
          f"clipped {clipped.tolist()} (numpy {count.tolist()})")
    assert worst <= lsb
    pcm2, clipped2 = m.render(zq, level, chunk_codes=chunk)
    assert torch.equal(pcm, pcm2) and torch.equal(clipped, clipped2)  # bitwise run to run
    if peak < 1.0:
        assert int(clipped.sum()) == 0 and int(count.sum()) == 0
        half, _ = m.render(zq, level, chunk_codes=chunk, gain=0.5)
        assert int(np.abs(half.cpu().numpy().astype(np.int32) * 2 - got).max()) <= 2 * lsb + 1
    else:
        assert int(clipped.sum()) > 0 and int(count.sum()) > 0
        assert (got == 32767).any() or (got == -32768).any()
    one, clipped1 = m.render(zq, level, chunk_codes=1000)  # one chunk: the same samples
    assert int(np.abs(one.cpu().numpy().astype(np.int32) - want).max()) <= lsb


def test_bad_codes_raise_before_any_launch(cuda):
    m = _case(32)[0]
    good = _codes()[0].cuda()
    token, negative = good.clone(), good.clone()
    token[1, 17] = K
    negative[0, 3] = -1
    as_int32 = good.to(torch.int32)
    flat = good.reshape(-1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for fn in (m.render, m.decode_chunked):
        with pytest.raises(ValueError, match=f"code {K} outside.*start token"):
            fn(token, 0)
        with pytest.raises(ValueError, match="code -1 outside"):
            fn(negative, 0)
        with pytest.raises(ValueError, match="int64"):
            fn(as_int32, 0)
        with pytest.raises(ValueError, match=r"\(B, T\)"):
            fn(flat, 0)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before  # no output, no activation: nothing was launched
    with pytest.raises(ValueError):
        m.render(good, 0, chunk_codes=0)
    with pytest.raises(ValueError):
        m.render(good, 0, gain=-1.0)


def test_sample_audio_end_to_end(cuda, tmp_path):
    import data_utils as DU
    from sampler import VQVAESampler
    n, total = 2, 24
    m = _case(32)[0]
    s = VQVAESampler([3, 2], [2, 2], [64, 16], codebook_size=K, dtype="fp32", device="cuda", seed=4)
    pcm, clipped, zs = s.sample_audio(n, m, seed=9, total_length=total)
    hop_top = int(s.hop_lengths[-1])
    assert hop_top == 32 and pcm.shape == (n, total * hop_top) and pcm.dtype == torch.int16
    assert clipped.shape == (n,) and clipped.dtype == torch.int32
    again = s.sample(n, seed=9, total_length=total)
    assert [tuple(z.shape) for z in zs] == [(n, 96), (n, 24)]
    for a, b in zip(zs, again):
        assert torch.equal(a, b)
    want, want_clipped = m.render(zs[0])
    assert torch.equal(pcm, want) and torch.equal(clipped, want_clipped)
    top, _, _ = s.sample_audio(n, m, seed=9, level=1, chunk_codes=8, total_length=total)
    assert top.shape == pcm.shape and torch.equal(top, m.render(zs[1], 1)[0])

    paths = DU.save_wavs(pcm, tmp_path / "wavs", 3000, labels=[1, 4])
    assert [os.path.basename(p) for p in paths] == ["sample_0_disco.wav", "sample_1_jazz.wav"]
    for i, p in enumerate(paths):
        back, bits, rate = DU.read_wav_pcm(p, sr=3000)
        assert bits == 16 and np.array_equal(back[:, 0], pcm[i].cpu().numpy())

    # a prior with bins = num_embeddings + 1 can emit the start token K: the codes are passed in directly
    class EmitsStartToken(VQVAESampler):
        def sample(self, n_samples, **kw):
            out = [z.clone() for z in zs]
            out[0][0, 5] = K
            return out

    bad = EmitsStartToken([3, 2], [2, 2], [64, 16], codebook_size=K + 1, priors=s.priors)
    with pytest.raises(ValueError, match="start token"):
        bad.sample_audio(n, m, seed=9, total_length=total)
    with pytest.raises(ValueError, match="start token"):
        m.render(bad.sample(n)[0])
    torch.cuda.synchronize()  # nothing faulted: the device still answers
    assert torch.equal(m.render(zs[0])[0], pcm)

    # a VQ-VAE of other levels or hops is refused before anything is drawn
    from vqvae import VQVAE
    other = VQVAE((1024, 1), 1, D, [3], [2], num_embeddings=K, residual_width=32, residual_depth=1, dtype="fp32",
                  device="cuda:0")
    with pytest.raises(ValueError, match="levels"):
        s.sample_audio(n, other, seed=9)
