"""vqa_resample on the GPU against resample.resample_reference (numpy fp64 from the same fp32 table), on both routes
(tap table in LDS / in global memory), whole and chunked, and through AudioCorpus.from_files(resample=).

The parity bound is derived, not measured: an output is a sum of P products accumulated in fp32, each step rounding
a partial sum of magnitude at most A = max_r sum_i |T[r][i]| * max|x| with relative error 2^-24, whether the step is
a fused multiply-add (one rounding) or a multiply and an add (two, the product's bounded the same way); the
reference's own fp64 error is far below one such step. So |y - ref| <= (P + 2) * 2^-24 * A, in any order."""
import math
import wave

import numpy as np
import pytest
import torch

import resample as RS
import vqa_lib as V
from audio_feed import AudioCorpus, AudioFeed

pytestmark = pytest.mark.gpu

# (sr_in, sr_out, quality, table in LDS)
CASES = [(22050, 3000, "best", True), (22050, 3000, "fast", True), (3000, 22050, "best", True),
         (44100, 22050, "best", True), (48000, 44100, "best", True), (22050, 16001, "best", False),
         (2, 3, "best", True)]
LENGTHS = [4099, 611, 5, 1]
B = 3
SENTINEL = 12345.0
_REF = {}


def bound(plan, xmax=1.0):
    return (plan.P + 2) * 2.0 ** -24 * plan.abs_row_sum() * xmax


def _input(n, kind):
    """(B, n) seeded noise in [-1, 1] as the kernel gets it, and its fp64 value."""
    rng = np.random.default_rng(1000 + n)
    if kind == "int16":
        a = rng.integers(-32768, 32768, (B, n)).astype(np.int16)
        return a, a.astype(np.float64) / 32768.0
    a = rng.uniform(-1.0, 1.0, (B, n)).astype(np.float32)
    return a, a.astype(np.float64)


def _reference(case, n, kind):
    key = (case[:3], n, kind)
    if key not in _REF:
        ref = RS.resample_reference(_input(n, kind)[1], RS.design(*case[:3]))
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


@pytest.mark.parametrize("kind", ["int16", "fp32"])
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_parity_with_the_fp64_reference(cuda, case, n, kind):
    plan = RS.design(*case[:3])
    assert V.resample_route(plan.up, plan.down, plan.P)[0] is case[3]
    a, _ = _input(n, kind)
    ref = _reference(case, n, kind)
    n_out = plan.output_length(n)
    assert ref.shape == (B, n_out)
    # rows wider than the data on both sides: the padding of x holds values that would wreck the result if read,
    # the padding of out a sentinel that must survive
    xb = torch.full((B, n + 3), 32767 if kind == "int16" else 1e30, dtype=torch.from_numpy(a).dtype, device=cuda)
    xb[:, :n] = torch.from_numpy(a).to(cuda)
    ob = torch.full((B, n_out + 5), SENTINEL, dtype=torch.float32, device=cuda)
    V.resample(xb[:, :n], ob[:, :n_out], plan.device_table(cuda), plan.up, plan.down)
    got = ob.cpu().numpy()
    assert (got[:, n_out:] == SENTINEL).all()
    err = float(np.abs(got[:, :n_out].astype(np.float64) - ref).max())
    print(f"{case[:3]} n={n} {kind}: err {err:.3g} bound {bound(plan):.3g} ratio {err / bound(plan):.3f}")
    assert err <= bound(plan)


@pytest.mark.parametrize("kind,amp", [("fp32", 1.0), ("int16", 16384)])
@pytest.mark.parametrize("case", [CASES[0], CASES[5], CASES[2]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_impulse_gives_the_table_entries_exactly(cuda, case, kind, amp):
    plan = RS.design(*case[:3])
    assert V.resample_route(plan.up, plan.down, plan.P)[0] is case[3]
    L, M, W, P = plan.up, plan.down, plan.W, plan.P
    n = 611
    ps = [0, n // 2, n - 1]
    x = np.zeros((len(ps), n), np.int16 if kind == "int16" else np.float32)
    for row, p in enumerate(ps):
        x[row, p] = amp
    got = RS.Resampler(*case[:3], device=cuda)(torch.from_numpy(x).to(cuda)).cpu().numpy()
    m = np.arange(got.shape[1])
    k0, r = np.divmod(m * M, L)
    scale = np.float32(1.0 if kind == "fp32" else 0.5)  # 16384 * 2^-15
    for row, p in enumerate(ps):
        i = p - k0 + W - 1
        inside = (i >= 0) & (i < P)
        want = np.where(inside, plan.table[r, np.clip(i, 0, P - 1)] * scale, np.float32(0.0))
        assert inside.any() and np.array_equal(got[row], want), (case, p)


@pytest.mark.parametrize("kind", ["int16", "fp32"])
@pytest.mark.parametrize("case,n", [(CASES[0], 4099), (CASES[5], 611), (CASES[2], 150)],
                         ids=["lds-down", "global", "lds-up"])
def test_chunked_equals_whole_bitwise(cuda, case, n, kind):
    rs = RS.Resampler(*case[:3], device=cuda)
    lds, tile = rs.route()
    assert lds is case[3]
    x = torch.from_numpy(_input(n, kind)[0][:2].copy()).to(cuda)
    whole = rs(x)
    n_out = whole.shape[1]
    assert n_out > tile + 1
    assert torch.equal(rs(x), whole)  # two runs give the same bits
    for c in (1, 7, tile - 1, tile + 1, n_out):
        assert torch.equal(rs.chunked(x, c), whole), c
    assert torch.equal(rs.chunked(x[0], 7), whole[0])  # one row, 1-D


def test_equal_rates_return_the_values_without_a_launch(cuda):
    rs = RS.Resampler(3000, 3000, "best", device=cuda)
    a, v = _input(611, "fp32")
    i16, v16 = _input(611, "int16")
    calls = []
    V.launch_hook = lambda: calls.append(1)
    try:
        x = torch.from_numpy(a).to(cuda)
        assert rs(x) is x and rs.chunked(x, 7) is x
        got16 = rs(torch.from_numpy(i16).to(cuda))
    finally:
        V.launch_hook = None
    assert not calls
    assert got16.dtype == torch.float32 and np.array_equal(got16.cpu().numpy(), v16.astype(np.float32))


def _write_wav(path, frames, rate, width=2):
    a = np.asarray(frames)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes((a.astype(np.uint8) if width == 1 else a.astype("<i2")).tobytes())


def test_corpus_from_files_of_mixed_rates(cuda, tmp_path):
    rng = np.random.default_rng(21)
    mono = rng.integers(-32768, 32768, 2205).astype(np.int16)
    stereo = rng.integers(-32768, 32768, (1500, 2)).astype(np.int16)
    eight = rng.integers(0, 256, 1201).astype(np.uint8)
    at_rate = rng.integers(-32768, 32768, 900).astype(np.int16)
    files = [tmp_path / f"{k}.wav" for k in ("mono", "stereo", "eight", "at_rate")]
    _write_wav(files[0], mono, 22050)
    _write_wav(files[1], stereo, 22050)
    _write_wav(files[2], eight, 22050, width=1)
    _write_wav(files[3], at_rate, 3000)
    labels = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="files are not resampled"):
        AudioCorpus.from_files(files, labels, sr=3000, window=64, device=cuda)

    corpus = AudioCorpus.from_files(files, labels, sr=3000, window=64, device=cuda, resample="best")
    plan = RS.design(22050, 3000, "best")
    sources = [mono.astype(np.float64) / 32768.0,
               (stereo.astype(np.float64) / 32768.0).mean(axis=1).astype(np.float32).astype(np.float64),
               ((eight.astype(np.float64) - 128.0) / 128.0).astype(np.float32).astype(np.float64)]
    want_len = [math.ceil(len(s) * 20 / 147) for s in sources] + [900]
    assert corpus.dtype == torch.float32 and list(corpus.track_lengths) == want_len
    assert corpus.corpus_len == sum(want_len)
    flat = corpus.samples[:corpus.corpus_len].cpu().numpy()
    for s, off, n in zip(sources, corpus.track_offsets, want_len):
        err = float(np.abs(flat[off:off + n].astype(np.float64) - RS.resample_reference(s, plan)).max())
        assert err <= bound(plan), err
    off = int(corpus.track_offsets[3])
    assert np.array_equal(flat[off:off + 900], at_rate.astype(np.float32) / np.float32(32768.0))
    # the window table, the labels and the feed work on the result as on any corpus
    assert len(corpus) == sum(n // 64 for n in want_len)
    assert set(corpus.labels_host.tolist()) == {0, 1, 2, 3}
    feed = AudioFeed(corpus, batch_size=4, seed=1, rank=0, world=1)
    x, y = feed.next()
    assert np.array_equal(x.cpu().numpy(), feed.host_batch(0))
    assert y.cpu().tolist() == corpus.labels_host[feed.slots(0)].tolist()
    train, test = corpus.split(0.5, seed=3)
    assert len(train) + len(test) == len(corpus)

    # every file already at the rate: nothing is converted and the corpus stays int16
    same = AudioCorpus.from_files([files[3]], [3], sr=3000, window=64, device=cuda, resample="best")
    assert same.dtype == torch.int16 and same.corpus_len == 900


def test_corpus_from_arrays_with_rates(cuda):
    a16, v16 = _input(611, "int16")
    af, vf = _input(4099, "fp32")
    with pytest.raises(ValueError, match="tracks are not resampled"):
        AudioCorpus.from_arrays([a16[0], af[0]], [0, 1], window=32, device=cuda, rates=[22050, 48000], sr=3000)
    c = AudioCorpus.from_arrays([a16[0], af[0], af[1][:300]], [0, 1, 2], window=32, device=cuda,
                                rates=[22050, 48000, 3000], sr=3000, resample="fast")
    plans = [RS.design(22050, 3000, "fast"), RS.design(48000, 3000, "fast")]
    want = [RS.resample_reference(v16[0], plans[0]), RS.resample_reference(vf[0], plans[1]), vf[1][:300]]
    assert list(c.track_lengths) == [len(w) for w in want]
    flat = c.samples[:c.corpus_len].cpu().numpy().astype(np.float64)
    for w, off, b in zip(want, c.track_offsets, [bound(plans[0]), bound(plans[1]), 0.0]):
        assert np.abs(flat[off:off + len(w)] - w).max() <= b
