"""Bounded-memory tokenization on the GPU: VQVAE.encode_chunked must give exactly the codes of encode_level (the
kernels' arithmetic for a position does not depend on where it lies in its tensor, and the halo of
Encoder.receptive_reach covers every cut), and CodeCorpus.from_audio must store exactly those codes per track.

Model: 2 levels, down_depth [3, 2], strides [2, 2] (hops 8 and 32), residual depth 2, dilation factor 3, 256 codes;
residual width 32 (the fused residual-block route) and 8 (the gather route), fp32 and bf16. T is the smallest
multiple of 32 at which a 512-sample core of level 1 has both of its cuts in the interior."""
import numpy as np
import pytest
import torch

from audio_feed import AudioCorpus
from code_feed import CodeCorpus
from vqvae import VQVAE, encode_plan

pytestmark = pytest.mark.gpu

KW = dict(num_embeddings=256, residual_depth=2, dilation_factor=3)


def _model(T, width, dtype, like=None):
    m = VQVAE((T, 1), 2, 64, [3, 2], [2, 2], residual_width=width, dtype=dtype, device="cuda:0", **KW)
    if like is not None:       # the same weights and codebooks at another input length
        m.set_weights(like.get_weights())
        m.set_vq_state(like.get_vq_state())
    return m


def _length(m):
    """The smallest multiple of 32 for which the second 512-sample core of level 1 has in_lo > 0 and in_hi < T."""
    halo, hop = m.encoders[1].receptive_reach()
    assert hop == 32 and m.encode_hops == [8, 32]
    k = halo * hop // 512 + 1              # the first core whose widened input starts past sample 0
    T = 512 * (k + 1) + halo * hop + 32    # and the first length its widened input ends before
    plan = encode_plan(T, 512, halo, hop)
    assert any(lo > 0 and hi < T for lo, hi, _, _ in plan)
    assert not any(lo > 0 and hi < T - 32 for lo, hi, _, _ in encode_plan(T - 32, 512, halo, hop))
    return T


@pytest.fixture(scope="module", params=[(32, "fp32"), (32, "bf16"), (8, "fp32"), (8, "bf16")],
                ids=lambda p: f"w{p[0]}-{p[1]}")
def case(request, cuda):
    width, dtype = request.param
    T = _length(_model(64, width, dtype))
    m = _model(T, width, dtype)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, T, 1, generator=g) * 2 - 1).to(cuda)
    whole = [m.encode_level(x, l) for l in range(2)]
    return m, x, whole


def test_halo_and_hops_match_the_host_walk(case):
    from vqvae import encode_halo_for
    m, _, _ = case
    for l in range(2):
        assert m.encode_halo(l) == encode_halo_for(l, [3, 2], [2, 2], residual_width=m.encoders[l].blocks[0].embed_width,
                                                   residual_depth=2, dilation_factor=3)


@pytest.mark.parametrize("level", [0, 1])
def test_encode_chunked_equals_encode_level(case, level):
    m, x, whole = case
    T = x.shape[1]
    hop = m.encode_hops[level]
    assert whole[level].shape == (2, T // hop) and whole[level].dtype == torch.int64
    assert len(torch.unique(whole[level])) > 8                       # not a degenerate encode
    odd = next(c for c in range(544, T, 32) if T % c)               # a multiple of both hops that does not divide T
    for chunk in (512, odd, T, T + 4096):
        got = m.encode_chunked(x, level, chunk_samples=chunk)
        assert got.dtype == torch.int64 and got.shape == whole[level].shape
        assert torch.equal(got, whole[level]), (level, chunk, int((got != whole[level]).sum()))
    again = m.encode_chunked(x, level, chunk_samples=512)
    assert torch.equal(again, m.encode_chunked(x, level, chunk_samples=512))   # bitwise run to run


def test_encode_chunked_rejects_bad_lengths(case):
    m, x, _ = case
    with pytest.raises(ValueError):
        m.encode_chunked(x[:, :1000], 1)        # not a multiple of the level's hop
    with pytest.raises(ValueError):
        m.encode_chunked(x[:, :, 0][:, :, None, None], 0)
    with pytest.raises(ValueError):
        m.encode_chunked(x, 0, chunk_samples=0)


def test_from_audio_stores_each_tracks_codes(cuda):
    """Three short int16 tracks whose lengths are not multiples of the top hop (32), and one shorter than a top-level
    code: each kept track's stored codes equal encode_level of that track cut to a multiple of 32."""
    m = _model(64, 32, "fp32")
    rng = np.random.default_rng(8)
    lengths = (1301, 20, 777, 2085)
    tracks = [rng.integers(-20000, 20000, n).astype(np.int16) for n in lengths]
    audio = AudioCorpus.from_arrays(tracks, (4, 9, 1, 4), window=64, device=cuda)
    corpus = CodeCorpus.from_audio(audio, m, chunk_samples=512)
    cut = [n // 32 * 32 for n in lengths if n >= 32]
    assert corpus.track_labels.tolist() == [4, 1, 4] and corpus.hops == [8, 32] and corpus.num_embeddings == 256
    assert corpus.lengths[0].tolist() == [n // 8 for n in cut] and corpus.lengths[1].tolist() == [n // 32 for n in cut]
    assert np.array_equal(corpus.offsets[0], 4 * corpus.offsets[1]) and corpus.rate(0) == 4
    assert corpus.codes[0].dtype == torch.int16 and corpus.codes[0].numel() % 8 == 0
    kept = [t for t in tracks if len(t) >= 32]
    for j, (t, n) in enumerate(zip(kept, cut)):
        x = torch.from_numpy(t[:n].astype(np.float32) / np.float32(32768.0)).to(cuda).view(1, n, 1)
        mj = _model(n, 32, "fp32", like=m)
        for l in range(2):
            want = mj.encode_level(x, l).view(-1)
            assert torch.equal(corpus.track_codes(l, j).long(), want), (j, l)
    for l in range(2):
        assert not corpus.codes[l][corpus.code_lens[l]:].any()
