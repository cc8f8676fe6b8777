"""The resampling filter on the host (resample.py), no GPU: the design's sizes and table, the fp64 restatement
`resample_reference` against scipy's upfirdn, an analytic sine and impulses, and data_utils.load_audio(resample=)."""
import math
import wave

import numpy as np
import pytest

import data_utils as D
import resample as RS

# (sr_in, sr_out, quality) -> (L, M, W, P): the sizes table of the design
SIZES = {
    (22050, 3000, "best"): (20, 147, 249, 498),
    (22050, 3000, "fast"): (20, 147, 139, 278),
    (3000, 22050, "best"): (147, 20, 34, 68),
    (44100, 22050, "best"): (1, 2, 68, 136),
    (48000, 44100, "best"): (147, 160, 37, 74),
}


@pytest.mark.parametrize("key", sorted(SIZES))
def test_design_sizes_and_table(key):
    plan = RS.design(*key)
    L, M, W, P = SIZES[key]
    assert (plan.up, plan.down, plan.W, plan.P) == (L, M, W, P)
    assert plan.table.dtype == np.float32 and plan.table.shape == (L, P)
    assert np.isfinite(plan.table).all()
    assert RS.design(*key) is plan  # cached per (rates, quality)


@pytest.mark.parametrize("key", sorted(SIZES))
def test_rows_of_the_fp64_table_sum_to_one(key):
    plan = RS.design(*key)
    _, t64 = RS.design_table(plan.up, plan.down, plan.quality)
    worst = float(np.abs(t64.sum(axis=1) - 1.0).max())
    print(f"{key}: worst |row sum - 1| = {worst:.3g}")
    assert worst <= (1e-6 if plan.quality == "best" else 2e-5)


def test_unknown_quality_is_refused():
    with pytest.raises(ValueError, match="quality"):
        RS.design(22050, 3000, "medium")


@pytest.mark.parametrize("key", [(22050, 3000, "best"), (22050, 3000, "fast"), (3000, 22050, "best"),
                                 (44100, 22050, "best"), (48000, 44100, "best"), (2, 3, "best")])
def test_reference_equals_upfirdn_of_the_prototype_filter(key):
    sig = pytest.importorskip("scipy.signal")
    plan = RS.design(*key)
    L, M, W, P = plan.up, plan.down, plan.W, plan.P
    h = np.zeros(P * L)
    for r in range(L):
        j = np.arange(P) - W + 1
        h[W * L - (j * L - r)] = plan.table[r].astype(np.float64)
    x = np.random.default_rng(3).uniform(-1, 1, 1531)
    full = sig.upfirdn(h, x, L, 1)
    m = np.arange(plan.output_length(len(x)))
    want = full[W * L + m * M]
    got = RS.resample_reference(x, plan)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("quality,bound", [("best", 1e-6), ("fast", 1e-4)])
def test_sine_below_the_new_nyquist_comes_out_as_the_analytic_sine(quality, bound):
    plan = RS.design(22050, 3000, quality)
    f = 0.4 * 1500.0
    n = 22050
    x = np.sin(2 * np.pi * f * np.arange(n) / 22050.0)
    y = RS.resample_reference(x, plan)
    edge = math.ceil(plan.W * plan.up / plan.down) + 1
    m = np.arange(len(y))[edge:len(y) - edge]
    err = float(np.abs(y[m] - np.sin(2 * np.pi * f * m / 3000.0)).max())
    print(f"{quality}: sine error {err:.3g}")
    assert len(m) > 2000 and err <= bound


@pytest.mark.parametrize("key", [(22050, 3000, "best"), (3000, 22050, "best"), (2, 3, "fast")])
def test_impulse_reads_the_table(key):
    plan = RS.design(*key)
    L, M, W, P = plan.up, plan.down, plan.W, plan.P
    n = 611
    for p in (0, n // 2, n - 1):
        x = np.zeros(n)
        x[p] = 1.0
        y = RS.resample_reference(x, plan)
        m = np.arange(len(y))
        k0, r = np.divmod(m * M, L)
        i = p - k0 + W - 1
        inside = (i >= 0) & (i < P)
        want = np.where(inside, plan.table[r, np.clip(i, 0, P - 1)].astype(np.float64), 0.0)
        assert inside.any() and np.array_equal(y, want)


def test_output_lengths():
    plan = RS.design(22050, 3000, "best")
    for n in (1, 5, plan.W - 1, 4099):
        want = math.ceil(n * plan.up / plan.down)
        assert RS.output_length(n, plan.up, plan.down) == plan.output_length(n) == want
        assert RS.resample_reference(np.ones(n), plan).shape == (want,)
    assert RS.resample_reference(np.ones((2, 3, 5)), plan).shape == (2, 3, 1)


def test_equal_rates_return_the_input():
    plan = RS.design(3000, 3000, "best")
    x = np.random.default_rng(0).uniform(-1, 1, (2, 77))
    assert plan.identity and np.array_equal(RS.resample_reference(x, plan), x)


def _write_wav(path, frames, rate, width=2):
    a = np.asarray(frames)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes((a.astype(np.uint8) if width == 1 else a.astype("<i2")).tobytes())


@pytest.mark.parametrize("quality", ["best", "fast"])
def test_load_audio_resamples_each_channel_before_mono(tmp_path, quality):
    rng = np.random.default_rng(11)
    n = 2205
    pcm = rng.integers(-20000, 20000, (n, 2)).astype(np.int16)
    f = tmp_path / "stereo.wav"
    _write_wav(f, pcm, 22050)
    plan = RS.design(22050, 3000, quality)
    want = RS.resample_reference(pcm.T.astype(np.float64) / 32768.0, plan)
    got = D.load_audio(f, sr=3000, resample=quality)
    assert got.dtype == np.float32 and got.shape == (2, math.ceil(n * 20 / 147))
    assert np.array_equal(got, want.astype(np.float32))
    mono = D.load_audio(f, sr=3000, mono=True, resample=quality)
    assert mono.shape == (1, got.shape[1]) and np.array_equal(mono, want.mean(axis=0, keepdims=True).astype(np.float32))
    # offset and duration are seconds of the file
    part = D.load_audio(f, sr=3000, offset=0.02, duration=0.05, resample=quality)
    cut = pcm[int(0.02 * 22050):int(0.02 * 22050) + int(0.05 * 22050)]
    assert np.array_equal(part, RS.resample_reference(cut.T / 32768.0, plan).astype(np.float32))


def test_load_audio_leaves_a_file_at_the_requested_rate_alone(tmp_path):
    pcm = np.random.default_rng(5).integers(-30000, 30000, 300).astype(np.int16)
    f = tmp_path / "at_rate.wav"
    _write_wav(f, pcm, 3000)
    assert np.array_equal(D.load_audio(f, sr=3000, resample="best"), D.load_audio(f, sr=3000))


def test_load_audio_without_resample_still_refuses_another_rate(tmp_path):
    f = tmp_path / "other.wav"
    _write_wav(f, np.zeros(100, np.int16), 22050)
    with pytest.raises(ValueError, match="files are not resampled"):
        D.load_audio(f, sr=3000)
    with pytest.raises(ValueError, match="files are not resampled"):
        D.split_convert([str(f)], [0], sample_rate=3000)
    with pytest.raises(ValueError, match="quality"):
        D.load_audio(f, sr=3000, resample="medium")


def test_split_convert_passes_resample_through(tmp_path):
    pcm = np.random.default_rng(8).integers(-20000, 20000, 22050).astype(np.int16)
    f = tmp_path / "song.wav"
    _write_wav(f, pcm, 22050)
    waves, genres, names = D.split_convert([str(f)], [4], sample_rate=3000, duration=30, split_window=0.25,
                                           resample="fast")
    assert waves.shape == (4, 1, 750) and list(genres) == [4] * 4 and list(names) == ["song.wav"] * 4
    want = D.load_audio(f, sr=3000, resample="fast")
    assert np.array_equal(waves[1, 0], want[0, 750:1500])
