"""The host loaders of data_utils (load_audio, split_convert, read_data, generate_genre_samples) and the window
table of the device corpus, without a GPU. The WAVs are written with the standard library into tmp_path.

Exactness: a sample of b bits is int / 2^(b-1), a dyadic rational with at most 24 significant bits for b <= 24, so
float32 holds it exactly and the comparisons below are equalities."""
import os
import struct
import wave

import numpy as np
import pytest

import data_utils as D
from audio_feed import AudioCorpus, window_starts

SR = 8000


def _write_wav(path, frames, bits, rate=SR):
    """frames: (n, C) integers in the signed range of `bits` (8-bit is stored unsigned with the 128 offset)."""
    frames = np.asarray(frames)
    n, C = frames.shape
    if bits == 8:
        raw = (frames + 128).astype(np.uint8).tobytes()
    elif bits == 16:
        raw = frames.astype("<i2").tobytes()
    elif bits == 24:
        raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in frames.reshape(-1))
    else:
        raw = frames.astype("<i4").tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(C)
        w.setsampwidth(bits // 8)
        w.setframerate(rate)
        w.writeframes(raw)


def _ints(n, C, bits, seed):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    a = np.random.default_rng(seed).integers(lo, hi + 1, size=(n, C), dtype=np.int64)
    a[0, 0], a[1, 0] = lo, hi  # the extreme values
    return a


@pytest.mark.parametrize("bits,C", [(16, 1), (16, 2), (8, 1), (24, 1), (24, 2)])
def test_load_audio_values_exact(tmp_path, bits, C):
    a = _ints(1000, C, bits, seed=bits + C)
    f = tmp_path / f"a{bits}_{C}.wav"
    _write_wav(f, a, bits)
    x = D.load_audio(str(f), sr=SR)
    assert x.dtype == np.float32 and x.shape == (C, 1000)
    want = (a.astype(np.float64) / float(1 << (bits - 1))).T
    assert np.array_equal(x.astype(np.float64), want)
    if bits == 16:
        assert x[0, 0] == -1.0 and x[0, 1] == np.float32(32767 / 32768)


def test_load_audio_32_bit(tmp_path):
    a = _ints(64, 1, 32, seed=5)
    f = tmp_path / "a32.wav"
    _write_wav(f, a, 32)
    x = D.load_audio(str(f), sr=SR)
    assert np.array_equal(x, (a.astype(np.float64) / 2.0 ** 31).T.astype(np.float32))


def test_load_audio_offset_duration_mono(tmp_path):
    a = _ints(SR * 2, 2, 16, seed=9)
    f = tmp_path / "s.wav"
    _write_wav(f, a, 16)
    full = D.load_audio(str(f), sr=SR)
    part = D.load_audio(str(f), sr=SR, offset=0.5, duration=0.25)
    assert part.shape == (2, SR // 4)
    assert np.array_equal(part, full[:, SR // 2:SR // 2 + SR // 4])
    assert D.load_audio(str(f), sr=SR, offset=1.5).shape == (2, SR // 2)          # to the end
    assert D.load_audio(str(f), sr=SR, offset=1.5, duration=3.0).shape == (2, SR // 2)  # clipped at the end
    mono = D.load_audio(str(f), sr=SR, mono=True)
    assert mono.shape == (1, 2 * SR)
    want = ((a[:, 0].astype(np.float64) + a[:, 1]) / 2.0 / 32768.0).astype(np.float32)
    assert np.array_equal(mono[0], want)


def test_load_audio_rate_mismatch_names_both_rates(tmp_path):
    f = tmp_path / "r.wav"
    _write_wav(f, _ints(10, 1, 16, 1), 16, rate=11025)
    with pytest.raises(ValueError) as e:
        D.load_audio(str(f), sr=22050)
    assert "11025" in str(e.value) and "22050" in str(e.value)


def test_load_audio_rejects_float_wav(tmp_path):
    # a hand-written RIFF header with format tag 3 (IEEE float)
    data = np.zeros(16, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, SR, SR * 4, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    f = tmp_path / "f.wav"
    f.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    with pytest.raises(ValueError):
        D.load_audio(str(f), sr=SR)


# ---- read_data / split_convert / generate_genre_samples --------------------------------------------------
GENRES = {"rock": 0, "jazz": 1}
N_SAMPLES = 1200  # per file


@pytest.fixture()
def tree(tmp_path):
    # created in an order that is not the sorted one
    for g, _ in GENRES.items():
        os.makedirs(tmp_path / g)
        for i in (3, 0, 4, 1, 2):
            _write_wav(tmp_path / g / f"{g}.{i:05d}.wav", _ints(N_SAMPLES, 1, 16, seed=10 * GENRES[g] + i), 16)
    return str(tmp_path) + "/"


def test_read_data_split_shapes_and_determinism(tree):
    kw = dict(test_data_percentage=0.4, sample_rate=SR, duration=30, split_window=0.25, split_overlap=0.5,
              max_signal_len=1000)
    out = D.read_data(tree, GENRES, **kw)
    Xtr, ytr, ftr, Xte, yte, fte = out
    # 1000 samples per file after the cut; chunks of 250 hopping 125: 7 per file, (n, 1, chunk) as the reference
    assert Xtr.shape == (6 * 7, 1, 250) and Xte.shape == (4 * 7, 1, 250)
    assert Xtr.dtype == np.float32
    assert ytr.shape == (42,) and ftr.shape == (42,) and yte.shape == (28,) and fte.shape == (28,)
    assert set(ftr).isdisjoint(set(fte)) and len(set(ftr)) == 6 and len(set(fte)) == 4
    for g in GENRES.values():  # stratified: 3 train and 2 test files of each genre
        assert len(set(ftr[ytr == g])) == 3 and len(set(fte[yte == g])) == 2
    # every chunk is the file's own samples
    first = str(fte[0])
    genre = first.split(".")[0]
    sig = D.load_audio(os.path.join(tree, genre, first), sr=SR)[:, :1000]
    assert np.array_equal(Xte[0], sig[:, :250]) and np.array_equal(Xte[1], sig[:, 125:375])
    again = D.read_data(tree, GENRES, **kw)
    for a, b in zip(out, again):
        assert np.array_equal(a, b)
    # another seed gives another (still stratified) partition for some seed
    others = [set(D.read_data(tree, GENRES, random_state=s, **kw)[5]) for s in range(1, 6)]
    assert any(o != set(fte) for o in others)


def test_read_data_shuffle_after_split_stratifies_by_file(tree):
    Xtr, ytr, ftr, Xte, yte, fte = D.read_data(tree, GENRES, test_data_percentage=0.25, sample_rate=SR,
                                               split_window=0.125, split_overlap=0.0, max_signal_len=1200,
                                               shuffle_after_split=True)
    # 8 chunks of 150 per file: 6 train and 2 test chunks of every file
    assert Xtr.shape == (60, 1, 150) and Xte.shape == (20, 1, 150)
    for name in set(ftr) | set(fte):
        assert int((ftr == name).sum()) == 6 and int((fte == name).sum()) == 2


def test_list_genre_files_sorted_and_capped(tree):
    fn, lab = D.list_genre_files(tree, GENRES, max_files_per_genre=3)
    assert [os.path.basename(f) for f in fn] == [f"{g}.{i:05d}.wav" for g in GENRES for i in range(3)]
    assert lab == [0, 0, 0, 1, 1, 1]


def test_generate_genre_samples():
    X = np.arange(6 * 4, dtype=np.float32).reshape(6, 4)
    y = np.array([1, 0, 1, 2, 0, 2])
    s, g = D.generate_genre_samples(X, y, return_genre=True)
    assert np.array_equal(s, X[[1, 0, 3]]) and np.array_equal(g, [0, 1, 2])
    assert np.array_equal(D.generate_genre_samples(X, y), s)


def test_stratified_split_counts():
    y = np.array([0] * 10 + [1] * 5 + [2])
    tr, te = D.stratified_split(y, 0.2, seed=3)
    assert sorted(np.concatenate([tr, te]).tolist()) == list(range(16))
    assert [(y[te] == c).sum() for c in (0, 1, 2)] == [2, 1, 0]
    tr2, te2 = D.stratified_split(y, 0.2, seed=3)
    assert np.array_equal(te, te2) and np.array_equal(tr, tr2)


# ---- the window table against splitsongs ---------------------------------------------------------------
def _splitsongs_starts(n, window, overlap, chunk):
    """Window starts splitsongs cuts from a track of n samples: the track is a ramp, so a piece's first value is its
    start. `chunk` is the chunk length the fraction must give."""
    pieces, _ = D.splitsongs(np.arange(n, dtype=np.int64), 0, window=window, overlap=overlap)
    if len(pieces) == 0:
        return []
    assert pieces.shape[1] == chunk
    assert np.array_equal(pieces, pieces[:, :1] + np.arange(chunk))
    return pieces[:, 0].tolist()


def test_window_table_matches_splitsongs():
    W = 1025
    # a track of exactly `window` samples: one window
    s, t = window_starts([W], W, hop=512)
    assert s.tolist() == _splitsongs_starts(W, 1.0, 0.5, W) == [0]
    # window - 1 samples: none (1024 * (1025 / 1024) is exactly 1025 in floating point)
    s, t = window_starts([W - 1], W, hop=512)
    assert s.tolist() == _splitsongs_starts(W - 1, W / (W - 1), 0.5, W) == []
    # several windows, the last one dropped where it would leave the track; the second track starts after the first
    s, t = window_starts([4096 + 100, 2048], 512, hop=256)
    a = _splitsongs_starts(4096 + 100, 512 / 4196, 0.5, 512)
    b = _splitsongs_starts(2048, 0.25, 0.5, 512)
    assert len(a) == 15 and len(b) == 7
    assert s.tolist() == a + [4196 + v for v in b]
    assert t.tolist() == [0] * 15 + [1] * 7
    # a max_signal_len cut: the windows of the first 2048 samples only, offsets still into the full tracks
    s, t = window_starts([3000, 3000], 512, hop=256, max_signal_len=2048)
    assert s.tolist() == b + [3000 + v for v in b]


def test_corpus_table_on_host(tmp_path):
    """AudioCorpus on the CPU device: int16 kept for 16-bit mono files, labels per window, the split by track."""
    files, labels = [], []
    for i, n in enumerate([1000, 299, 300, 650, 700, 900]):
        f = tmp_path / f"t{i}.wav"
        _write_wav(f, _ints(n, 1, 16, seed=i), 16)
        files.append(str(f))
        labels.append(i % 2)
    c = AudioCorpus.from_files(files, labels, sr=SR, window=300, hop=100, max_signal_len=800, device="cpu")
    assert c.dtype.is_floating_point is False and c.samples.numel() % 8 == 0 and c.corpus_len == 3849
    per_track = [6, 0, 1, 4, 5, 6]  # 800 usable samples of the first and the last track
    assert len(c) == sum(per_track)
    assert np.bincount(c.track_host, minlength=6).tolist() == per_track
    assert np.array_equal(c.labels_host, np.asarray(labels)[c.track_host])
    flat = c.samples[:c.corpus_len].numpy()
    a0 = _ints(1000, 1, 16, seed=0)[:, 0]
    assert np.array_equal(flat[c.starts_host[1]:c.starts_host[1] + 300], a0[100:400])
    tr, te = c.split(0.34, seed=1)
    assert tr.samples.data_ptr() == te.samples.data_ptr() == c.samples.data_ptr()
    assert set(tr.track_host).isdisjoint(set(te.track_host))
    assert len(tr) + len(te) == len(c)
    _, te_tracks = D.stratified_split(c.track_labels, 0.34, seed=1)  # one track of each label on the test side
    assert sorted(c.track_labels[te_tracks].tolist()) == [0, 1]
    assert set(te.track_host) <= set(te_tracks.tolist())
    # a stereo or 24-bit file makes the corpus float32 with the same values
    _write_wav(tmp_path / "st.wav", _ints(400, 2, 16, seed=7), 16)
    cf = AudioCorpus.from_files(files[:1] + [str(tmp_path / "st.wav")], sr=SR, window=300, device="cpu")
    assert cf.dtype.is_floating_point and cf.labels is None
    assert np.array_equal(cf.samples[:1000].numpy(), a0.astype(np.float32) / np.float32(32768))
    with pytest.raises(ValueError):
        AudioCorpus(c.samples, c.corpus_len, 300, np.array([c.corpus_len - 299]), None, np.array([0]),
                    c.track_lengths, None)
