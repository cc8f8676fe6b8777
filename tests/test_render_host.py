"""Host-side parts of the codes -> audio path, no GPU: the chunk plan of the bounded-memory decode (decode_plan), the
decoder's halo against the fp64 oracle (a chunked decode of the oracle's own decoder must reproduce its whole
decode: the arithmetic is identical, so only a halo that is too short can miss the bound), and the WAV writer
against the reader."""
import json
import os

import numpy as np
import pytest
import torch

import data_utils as DU
from oracle import vqvae_ref as R
from vqvae import decode_halo_for, decode_plan

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- decode_plan -----------------------------------------------------------------------------------------
def _check_plan(total, chunk, halo):
    plan = decode_plan(total, chunk, halo)
    covered = np.zeros(total, np.int64)
    prev = 0
    for in_lo, in_hi, core_lo, core_hi in plan:
        assert core_lo == prev and core_lo < core_hi <= total and core_hi - core_lo <= chunk
        prev = core_hi
        covered[core_lo:core_hi] += 1
        assert in_lo == max(0, core_lo - halo) and in_hi == min(total, core_hi + halo)  # widened, then clamped
        assert 0 <= in_lo <= core_lo and core_hi <= in_hi <= total
    assert prev == total and np.array_equal(covered, np.ones(total, np.int64))  # the cores tile exactly once
    assert len(plan) == -(-total // chunk)
    assert plan[0][0] == 0 and plan[-1][1] == total  # the ends are reached by the chunks themselves
    return plan


@pytest.mark.parametrize("total,chunk,halo", [
    (5, 16, 3),        # total < chunk: one chunk, nothing to widen
    (96, 16, 11),      # a multiple of the chunk
    (100, 16, 11),     # not a multiple: a short last core
    (97, 16, 40),      # halo wider than a chunk
    (7, 1, 2),         # chunk = 1
    (50, 8, 0),        # halo = 0: input = core
    (1, 1, 0),
    (300, 37, 13),
])
def test_decode_plan_tiles_once_and_clamps(total, chunk, halo):
    _check_plan(total, chunk, halo)


def test_decode_plan_cases_by_hand():
    assert decode_plan(5, 16, 3) == [(0, 5, 0, 5)]
    assert decode_plan(10, 4, 1) == [(0, 5, 0, 4), (3, 9, 4, 8), (7, 10, 8, 10)]
    assert decode_plan(3, 1, 0) == [(0, 1, 0, 1), (1, 2, 1, 2), (2, 3, 2, 3)]


@pytest.mark.parametrize("total,chunk,halo", [(0, 4, 1), (-3, 4, 1), (10, 0, 1), (10, -2, 1), (10, 4, -1)])
def test_decode_plan_rejects_bad_sizes(total, chunk, halo):
    with pytest.raises(ValueError):
        decode_plan(total, chunk, halo)


# ---- decode_halo against the fp64 oracle -----------------------------------------------------------------
def _micro_cfg():
    meta = json.load(open(os.path.join(HERE, "golden", "micro.json")))
    return R.RefConfig(**meta["config"])


ONE_LEVEL = R.RefConfig(input_len=768, levels=1, latent_dim=4, down_depth=[3], strides=[2], num_embeddings=32,
                        residual_width=8, residual_depth=3, dilation_factor=3)
CONFIGS = {"micro": _micro_cfg(), "one_level_d3": ONE_LEVEL}


def _halo(cfg, level):
    return decode_halo_for(level, cfg.down_depth, cfg.strides, residual_width=cfg.residual_width,
                           residual_depth=cfg.residual_depth, dilation_factor=cfg.dilation_factor,
                           latent_dim=cfg.latent_dim)


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def oracle_case(request):
    cfg = CONFIGS[request.param]
    ref = R.RefVQVAE(cfg, R.init_params(cfg, 5), R.init_vq_state(cfg, 6), dtype=torch.float64)
    # biases are zero at init: random ones, so that a padded edge differs from a true interior
    rng = np.random.default_rng(11)
    for n in ref.p:
        if n.endswith("/bias"):
            ref.p[n] = torch.tensor(rng.uniform(-0.1, 0.1, size=tuple(ref.p[n].shape)), dtype=torch.float64)
    codes = torch.from_numpy(rng.integers(0, cfg.num_embeddings, size=(2, 96)))
    return cfg, ref, codes


def _chunked_max_diff(cfg, ref, codes, level, halo, chunk=16):
    hop = int(np.prod([s ** d for s, d in zip(cfg.strides[:level + 1], cfg.down_depth[:level + 1])]))
    with torch.no_grad():
        q = ref.vq[level]["embeddings"].T[codes]                    # (B, 96, D)
        whole = ref.decoder(q, level)
        assert whole.shape == (codes.shape[0], codes.shape[1] * hop, 1)
        assert torch.equal(whole, ref.decode(codes, level))
        worst = 0.0
        for in_lo, in_hi, core_lo, core_hi in decode_plan(codes.shape[1], chunk, halo):
            part = ref.decoder(q[:, in_lo:in_hi], level)
            core = part[:, (core_lo - in_lo) * hop:(core_hi - in_lo) * hop]
            worst = max(worst, float((core - whole[:, core_lo * hop:core_hi * hop]).abs().max()))
    return worst


def test_decode_halo_covers_the_oracle_decoder(oracle_case):
    cfg, ref, codes = oracle_case
    for level in range(cfg.levels):
        halo = _halo(cfg, level)
        assert 0 < halo < 96
        diff = _chunked_max_diff(cfg, ref, codes, level, halo)
        print(f"level {level}: halo {halo} codes, chunked vs whole max |diff| {diff:.3e}")
        assert diff <= 1e-12, (level, halo, diff)


def test_the_oracle_check_sees_a_short_halo(oracle_case):
    """The check above has teeth: with no halo at all the chunked oracle decode differs from the whole one."""
    cfg, ref, codes = oracle_case
    assert _chunked_max_diff(cfg, ref, codes, 0, 0) > 1e-6


def test_decode_halo_values_by_hand():
    """micro level 0 (down_depth 2, residual depth 2, dilations reversed [3, 1]): pre 1; block (3 + 1) + (1 + 1) = 6
    -> 7; up 2*7 + 1 = 15; block -> 21; up -> 43; out -> 44 samples at hop 4 = 11 codes."""
    cfg = CONFIGS["micro"]
    assert _halo(cfg, 0) == 11
    # no dilation, depth 1, one stride-2 step: pre 1, block 2 -> 3, up 7, out 8 samples at hop 2 = 4 codes
    assert decode_halo_for(0, [1], [2], residual_width=8, residual_depth=1, dilation_factor=1, latent_dim=4) == 4


# ---- write_wav / save_wavs ---------------------------------------------------------------------------------
def _pcm(n, C, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, size=(n, C)).astype(np.int16)
    a[0, 0], a[1, 0], a[2, 0] = -32768, 32767, 0
    return a


@pytest.mark.parametrize("C,sr", [(1, 3000), (2, 44100)])
def test_write_wav_round_trips_through_read_wav_pcm(tmp_path, C, sr):
    a = _pcm(1001, C, 3)
    f = tmp_path / "a.wav"
    DU.write_wav(f, a, sr)
    back, bits, rate = DU.read_wav_pcm(f)
    assert bits == 16 and rate == sr and back.dtype == np.int16
    assert np.array_equal(back, a)
    assert back.min() == -32768 and back.max() == 32767


def test_write_wav_takes_1d_and_tensors_and_refuses_other_types(tmp_path):
    a = _pcm(257, 1, 4)[:, 0]
    DU.write_wav(tmp_path / "m.wav", a, 8000)
    DU.write_wav(tmp_path / "t.wav", torch.from_numpy(a.copy()), 8000)
    for name in ("m.wav", "t.wav"):
        back, bits, rate = DU.read_wav_pcm(tmp_path / name, sr=8000)
        assert np.array_equal(back[:, 0], a) and back.shape == (257, 1)
    with pytest.raises(ValueError):
        DU.write_wav(tmp_path / "f.wav", a.astype(np.float32), 8000)
    with pytest.raises(ValueError):
        DU.write_wav(tmp_path / "f.wav", a.astype(np.int32), 8000)
    with pytest.raises(ValueError):
        DU.write_wav(tmp_path / "f.wav", np.zeros((2, 3, 4), np.int16), 8000)


def test_save_wavs_names_and_contents(tmp_path):
    pcm = _pcm(64, 3, 5).T.copy()  # (3 rows, 64 samples)
    paths = DU.save_wavs(pcm, tmp_path / "out", 3000)
    assert [os.path.basename(p) for p in paths] == ["sample_0.wav", "sample_1.wav", "sample_2.wav"]
    paths = DU.save_wavs(torch.from_numpy(pcm), tmp_path / "out", 3000, labels=[2, 0, 9], prefix="gen")
    assert [os.path.basename(p) for p in paths] == ["gen_0_classical.wav", "gen_1_metal.wav", "gen_2_hiphop.wav"]
    for i, p in enumerate(paths):
        back, bits, rate = DU.read_wav_pcm(p, sr=3000)
        assert np.array_equal(back[:, 0], pcm[i])
    with pytest.raises(ValueError):
        DU.save_wavs(pcm, tmp_path / "out", 3000, labels=[1, 2])
