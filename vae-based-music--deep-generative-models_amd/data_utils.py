"""Spectral-loss helpers, the audio loaders and the synthetic device feed of the reference data_utils.py.

data_utils.py:19-22  STFT_ARGS (n_fft, hop_length, window_size) per resolution
data_utils.py:25-30  spectral = |tf.signal.stft(x, frame_length=win, frame_step=hop, fft_length=n_fft)|
data_utils.py:33-40  norm = tf.norm(x, 'fro', axis=[-2, -1])
vqvae.py:309-326     _multispectral_loss = mean_res ||S_x - S_r||_F / ||S_x||_F
The STFT, the loss and its gradient run in libvqa's spectral kernels (csrc/vqa_spectral*.hip: one wave per frame
pair, a Stockham or four-step FFT in registers and LDS, with TF framing — no centering, frame t = x[t*hop : t*hop+win] times a periodic Hann window, rfft
zero-padded at the end to n_fft).

data_utils.py:43-238  load_audio, splitsongs, split_convert, read_data, generate_genre_samples: a folder of
genre-labelled WAVs turned into training windows and labels, with the reference's names, arguments and result
shapes. Files are integer-PCM WAV read with the standard library (no librosa: by default nothing is resampled and a
file whose rate is not the requested one is an error; resample="best" / "fast" converts it with the polyphase filter
of resample.py) and the stratified split is a deterministic one of our own (no sklearn).
These build host arrays, as the reference does; training itself reads a device-resident corpus through
audio_feed.AudioCorpus / AudioFeed (one gather kernel per step inside the step's graph).

`synthetic_batch_device` generates synthetic chunks in HBM with a HIP kernel; `synthetic_batch` is
the numpy restatement the tests and the oracle use.
"""
from __future__ import annotations

import os
import wave

import numpy as np
import torch

import vqa_lib as V
from resample import design, resample_reference

STFT_ARGS = [(2048, 1024, 512),  # n_fft
             (240, 120, 50),  # hop_length
             (1200, 600, 240)]  # window_size


def spectral(x: torch.Tensor, n_fft: int, hop_length: int, window_length: int) -> torch.Tensor:
    """data_utils.py:25-30 |tf.signal.stft(x, window_length, hop_length, n_fft)| on the HIP FFT kernel:
    x (..., T) fp32 device tensor -> (..., F, n_fft//2 + 1) fp32."""
    lead, T = tuple(x.shape[:-1]), x.shape[-1]
    xf = x.detach().reshape(-1, T).float().contiguous()
    if window_length > T:
        raise ValueError(f"spectral: signal of {T} samples is shorter than the {window_length}-sample window")
    F = 1 + (T - window_length) // hop_length
    mag = torch.empty(xf.shape[0], F, n_fft // 2 + 1, dtype=torch.float32, device=x.device)
    V.stft_magnitude(xf, mag, n_fft, hop_length, window_length)
    return mag.reshape(*lead, F, n_fft // 2 + 1)


def norm(x: torch.Tensor) -> torch.Tensor:
    """data_utils.py:33-40 tf.norm(x, 'fro', axis=[-2, -1])."""
    return torch.sqrt((x * x).sum(dim=(-2, -1)))


class SpectralTarget:
    """The target waveform of one batch, (B, T) fp32 on the device, and its spectrograms |S_x| for every
    resolution (computed once by vqa_spectral_target and shared by the loss of every level)."""

    def __init__(self, x: torch.Tensor):
        self.x = x.reshape(x.shape[0], -1).float().contiguous()
        self.B, self.T = self.x.shape
        self.mags = V.spectral_target(self.x, *STFT_ARGS)
        self._ws = {}
        # the spectrograms are complete when this event (on the producing stream) has fired: a loss on another
        # stream waits for it (the levels' streams only need the target at their losses, not at their start)
        self.ready = None
        if self.x.is_cuda:
            self._stream = torch.cuda.current_stream(self.x.device)
            self.ready = torch.cuda.Event()
            self.ready.record(self._stream)

    def wait(self):
        """Order the current stream after the spectrograms (no-op on the producing stream)."""
        if self.ready is not None:
            cur = torch.cuda.current_stream(self.x.device)
            if cur != self._stream:
                cur.wait_event(self.ready)

    def workspace(self, grad: bool) -> torch.Tensor:
        """Loss scratch, one per stream (levels on concurrent streams never share it)."""
        key = (grad, torch.cuda.current_stream(self.x.device).cuda_stream if self.x.is_cuda else 0)
        if key not in self._ws:
            n = V.spectral_loss_target_workspace(self.B, self.T, *STFT_ARGS, with_grad=grad)
            self._ws[key] = V.workspace(n, self.x.device)
        return self._ws[key]


def multispectral_loss_and_grad(target: SpectralTarget, recon: torch.Tensor, loss_out=None, need_grad=True):
    """vqvae.py:309-326 _multispectral_loss (mean over the batch of the per-item mean over resolutions) and
    its gradient d loss / d recon, (B, T, 1) fp32 — one vqa_spectral_loss_target call against the shared
    target spectrograms. Returns (loss (1,), grad)."""
    r = recon.reshape(recon.shape[0], -1)
    if r.dtype != torch.float32:
        raise ValueError("the multispectral loss takes the fp32 reconstruction")
    if r.shape != target.x.shape:
        raise ValueError(f"reconstruction {tuple(r.shape)} vs target {tuple(target.x.shape)}")
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=r.device)
    dr = torch.empty_like(r) if need_grad else None
    target.wait()
    V.spectral_loss_target(target.mags, r.contiguous(), loss, dr, None, *STFT_ARGS, ws=target.workspace(need_grad))
    return loss, (dr.reshape(recon.shape) if need_grad else None)


def splitsongs(X, y, window=0.05, overlap=0.5):
    """data_utils.py:65-91: a song cut into overlapping chunks of int(T * window) samples, hopping by
    int(chunk * (1 - overlap)); a chunk that would run past the end is dropped. X is (T,) or (C, T); returns
    ((n, chunk) or (n, C, chunk), (n,) copies of the label) — channels first, as the reference's callers then
    transpose to (B, T, C). Host numpy, like the reference. The device feed cuts its windows by the same rule
    (audio_feed.window_starts) but keeps only their start offsets: the samples stay in one device tensor and a
    step's windows are gathered by vqa_corpus_batch."""
    X = np.asarray(X)
    T = X.shape[-1]
    chunk = int(T * window)
    hop = int(chunk * (1.0 - overlap))
    pieces = [X[..., s:s + chunk] for s in range(0, T - chunk + hop, hop)]
    pieces = [p for p in pieces if p.shape[-1] == chunk]
    return np.array(pieces), np.array([y] * len(pieces))


SAMPLE_RATE = 3000

# the GTZAN genre folders in the reference's label order (data_utils.py:13-16)
IDX_TO_GENRES = dict(enumerate(("metal", "disco", "classical", "rock", "jazz", "country", "pop", "blues", "reggae",
                                "hiphop")))
GENRES = {name: idx for idx, name in IDX_TO_GENRES.items()}

# data_utils.py:161: the one GTZAN file that does not decode
SKIP_FILES = ("jazz/jazz.00054.wav",)

SPLIT_PERM_LEVEL = 0x53504C54  # the `level` of the permutation key of stratified_split


def read_wav_pcm(file, sr=None, offset=0.0, duration=None):
    """Integer-PCM WAV -> (frames (n, C) integers as stored, bits per sample, sample rate). 8-bit samples are
    returned with their 128 offset removed (int16), 16-bit as int16, 24- and 32-bit as int32. `offset` and
    `duration` are seconds, cut to whole frames as int(seconds * rate). Raises ValueError for a WAV that is not
    integer PCM (float, compressed) and, with `sr`, for a file of another rate: nothing is resampled."""
    try:
        w = wave.open(str(file), "rb")
    except wave.Error as e:
        raise ValueError(f"{file}: not an integer-PCM WAV ({e})") from None
    with w:
        rate, C, width, total = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        if w.getcomptype() != "NONE" or width not in (1, 2, 3, 4):
            raise ValueError(f"{file}: not an integer-PCM WAV (compression {w.getcomptype()}, {8 * width} bit)")
        if sr is not None and int(sr) != rate:
            raise ValueError(f"{file}: sample rate {rate} Hz, requested {int(sr)} Hz (files are not resampled)")
        first = min(total, max(0, int(offset * rate)))
        n = total - first if duration is None else min(total - first, max(0, int(duration * rate)))
        w.setpos(first)
        raw = w.readframes(n)
    n = len(raw) // (width * C)  # a truncated file gives the frames it has
    raw = raw[:n * width * C]
    if width == 1:
        a = np.frombuffer(raw, np.uint8).astype(np.int16) - 128
    elif width == 2:
        a = np.frombuffer(raw, "<i2")
    elif width == 4:
        a = np.frombuffer(raw, "<i4")
    else:  # 24 bit: three little-endian bytes into the top of an int32, shifted down with the sign
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.uint32)
        a = ((b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)).view(np.int32) >> 8
    return a.reshape(n, C), 8 * width, rate


def write_wav(file, pcm, sr):
    """The inverse of read_wav_pcm for 16-bit data: pcm, int16 (n,) or (n, C) frames — a numpy array or a tensor
    (a device tensor is copied to the host once) — written as an integer-PCM WAV of rate `sr` through the standard
    library's `wave`. Anything but int16 is a ValueError: nothing is scaled or rounded here (VQVAE.render and
    vqa_pcm_encode do that on the device)."""
    a = pcm.detach().cpu().numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    if a.dtype != np.int16:
        raise ValueError(f"write_wav: 16-bit PCM is int16 (got {a.dtype})")
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] < 1):
        raise ValueError(f"write_wav: frames are (n,) or (n, C) (got shape {a.shape})")
    if int(sr) <= 0:
        raise ValueError(f"write_wav: sample rate {sr}")
    with wave.open(str(file), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(np.ascontiguousarray(a, dtype="<i2").tobytes())


def save_wavs(pcm, directory, sr, labels=None, prefix="sample"):
    """One mono WAV per row of pcm, int16 (B, n) (VQVAE.render's / VQVAESampler.sample_audio's result; a device
    tensor is copied once): directory/prefix_{i}.wav, or with labels directory/prefix_{i}_{genre}.wav, genre =
    IDX_TO_GENRES[labels[i]] (utils/tf_utils.py:196-226 generate_and_save_waves names its files by genre too).
    The directory is created. Returns the paths."""
    a = pcm.detach().cpu().numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
    if a.ndim != 2:
        raise ValueError(f"save_wavs: pcm is (B, n) (got shape {a.shape})")
    if labels is not None:
        labels = [int(v) for v in (labels.tolist() if hasattr(labels, "tolist") else labels)]
        if len(labels) != a.shape[0]:
            raise ValueError(f"save_wavs: {len(labels)} labels for {a.shape[0]} rows")
    os.makedirs(directory, exist_ok=True)
    paths = []
    for i in range(a.shape[0]):
        name = f"{prefix}_{i}.wav" if labels is None else f"{prefix}_{i}_{IDX_TO_GENRES[labels[i]]}.wav"
        paths.append(os.path.join(directory, name))
        write_wav(paths[-1], a[i], sr)
    return paths


def load_audio(file, sr=22050, offset=0.0, duration=None, mono=False, resample=None):
    """data_utils.py:43-48 (librosa.load there): -> (C, n) float32, a sample being int / 2^(bits-1) (8-bit data is
    unsigned with a 128 offset), exactly for up to 24 bits. Integer-PCM WAV of 8, 16, 24 or 32 bits through the
    standard library's `wave`; `mono` averages the channels; `offset` / `duration` are seconds. By default there is
    no resampling: a file whose rate is not `sr` raises ValueError (naming both rates), as does a non-PCM WAV.
    resample="best" / "fast" reads the file at its own rate (`offset` / `duration` stay seconds of the file) and
    converts every channel to `sr` on the host (resample.resample_reference, fp64) before `mono`:
    -> (C, ceil(n * L / M)); a file already at `sr` is returned as without it."""
    a, bits, rate = read_wav_pcm(file, sr=sr if resample is None else None, offset=offset, duration=duration)
    x = (a.astype(np.float64) / float(1 << (bits - 1))).T  # (C, n)
    if resample is not None:
        x = resample_reference(x, design(rate, sr, resample))
    if mono:
        x = x.mean(axis=0, keepdims=True)
    return np.ascontiguousarray(x, dtype=np.float32)


def stratified_split(labels, test_fraction, seed=42):
    """Deterministic stratified split -> (train indices, test indices), both ascending. Every class gives
    floor(n_c * test_fraction + 0.5) of its n_c members to the test side (at least one and at most n_c - 1 when
    n_c >= 2 and the fraction is positive; a class of one stays in train). The members picked are the first of the
    class under the library's keyed permutation (vqa_reset_perm_index with key (seed, class rank,
    SPLIT_PERM_LEVEL)). This is NOT sklearn's train_test_split partition: the reference's split depends on numpy's
    global generator, ours only on the arguments."""
    labels = np.asarray(labels)
    classes, inv = np.unique(labels, return_inverse=True)
    test = []
    for c in range(len(classes)):
        members = np.nonzero(inv == c)[0]
        n = len(members)
        k = 0
        if test_fraction > 0 and n >= 2:
            k = min(max(int(np.floor(n * float(test_fraction) + 0.5)), 1), n - 1)
        test.extend(int(members[V.reset_perm_index(int(seed), c, SPLIT_PERM_LEVEL, n, j)]) for j in range(k))
    test = np.array(sorted(test), dtype=np.int64)
    train = np.setdiff1d(np.arange(len(labels), dtype=np.int64), test)
    return train, test


def split_convert(X, y, sample_rate=3000, duration=30, max_signal_len=660000, split_window=1.0, split_overlap=0.0,
                  resample=None):
    """data_utils.py:100-136: every file of X loaded (load_audio, `duration` seconds, cut to max_signal_len
    samples) and cut by splitsongs -> (waves (n, C, chunk) float32, genres (n,), file labels (n,) — the file's
    base name repeated for each of its chunks). `resample` is load_audio's."""
    arr_waves, arr_genres, arr_file_label = [], [], []
    for fn, genre in zip(X, y):
        file_label = str(fn).split('/')[-1]
        signal = load_audio(fn, sr=sample_rate, duration=duration, resample=resample)[:, :max_signal_len]
        signals, ys = splitsongs(signal, genre, window=split_window, overlap=split_overlap)
        arr_waves.extend(signals)
        arr_genres.extend(ys)
        arr_file_label.extend([file_label] * len(ys))
    return np.array(arr_waves), np.array(arr_genres), np.array(arr_file_label)


def list_genre_files(src_dir, genres, max_files_per_genre=1000):
    """The file walk of read_data (data_utils.py:152-168): for every genre of `genres` (a name -> label dict) the
    files under src_dir/<genre>, in sorted order so that the result does not depend on the file system, at most
    max_files_per_genre per folder, without SKIP_FILES -> (file names, labels)."""
    arr_fn, arr_genres = [], []
    for name, label in genres.items():
        folder = os.path.join(src_dir, name)
        for root, subdirs, files in sorted(os.walk(folder)):
            for file in sorted(files)[:max_files_per_genre]:
                file_name = os.path.join(root, file).replace(os.sep, "/")
                if any(file_name.endswith(s) for s in SKIP_FILES):
                    continue
                arr_fn.append(file_name)
                arr_genres.append(label)
    return arr_fn, arr_genres


def read_data(src_dir, genres, test_data_percentage=0.1, sample_rate=22050, duration=30, split_window=1.0,
              split_overlap=0.0, max_signal_len=660000, shuffle_after_split=False, max_files_per_genre=1000,
              random_state=42, resample=None):
    """data_utils.py:146-206 -> (X_train, y_train, y_file_train, X_test, y_test, y_file_test), X (n, C, chunk)
    float32. The files are split into train and test stratified by genre and each side is then loaded and cut
    (split_convert); with shuffle_after_split all files are cut first and the chunks are split stratified by file.
    The split is stratified_split with `random_state` as its seed (the reference's 42): deterministic, but not
    sklearn's partition. `resample` is load_audio's (None: files of another rate are an error)."""
    arr_fn, arr_genres = list_genre_files(src_dir, genres, max_files_per_genre)
    kw = dict(sample_rate=sample_rate, duration=duration, max_signal_len=max_signal_len, split_window=split_window,
              split_overlap=split_overlap, resample=resample)
    if shuffle_after_split:
        X, y, y_file = split_convert(arr_fn, arr_genres, **kw)
        tr, te = stratified_split(y_file, test_data_percentage, random_state)
        return X[tr], y[tr], y_file[tr], X[te], y[te], y_file[te]
    tr, te = stratified_split(arr_genres, test_data_percentage, random_state)
    X_test, y_test, y_file_test = split_convert([arr_fn[i] for i in te], [arr_genres[i] for i in te], **kw)
    X_train, y_train, y_file_train = split_convert([arr_fn[i] for i in tr], [arr_genres[i] for i in tr], **kw)
    return X_train, y_train, y_file_train, X_test, y_test, y_file_test


def generate_genre_samples(X, y, return_genre=False):
    """data_utils.py:209-238: one sample per genre, the first of X carrying each label 0 .. n_classes-1, stacked
    -> (n_classes, ...); with return_genre also the labels (n_classes,)."""
    y = np.asarray(y)
    n_classes = len(np.unique(y))
    first = []
    for i in range(n_classes):
        hits = np.where(y == i)[0]
        if len(hits) == 0:
            raise ValueError(f"labels must be 0 .. {n_classes - 1}: none is {i}")
        first.append(int(hits[0]))
    train_samples = np.stack([X[j] for j in first], axis=0)
    if return_genre:
        return train_samples, np.arange(n_classes)
    return train_samples


def synthetic_batch(B: int, T: int, sr: int = 44100, seed: int = 1234) -> np.ndarray:
    """clip(0.5 sin(2 pi f t / sr + phi) + 0.05 N(0,1), -1, 1), f ~ U[55, 2000] Hz,
    phi ~ U[0, 2 pi). Shape (B, T, 1) fp32, never silent (the spectral loss has no epsilon)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(55.0, 2000.0, size=(B, 1))
    ph = rng.uniform(0.0, 2 * np.pi, size=(B, 1))
    t = np.arange(T)[None, :]
    x = 0.5 * np.sin(2 * np.pi * f * t / sr + ph) + 0.05 * rng.standard_normal((B, T))
    return np.clip(x, -1.0, 1.0).astype(np.float32)[:, :, None]


def synthetic_batch_device(B: int, T: int, seed: int = 1234, rank: int = 0, sr: float = 44100.0,
                           device="cuda", out: torch.Tensor = None) -> torch.Tensor:
    """The same distribution generated on the GPU (vqa_synthetic_batch: counter-based draws keyed by seed,
    rank, item and sample), (B, T, 1) fp32 resident in HBM — the device feed of the train step; no host
    staging. Deterministic per (seed, rank); ranks draw disjoint streams."""
    x = out if out is not None else torch.empty(B, T, 1, dtype=torch.float32, device=device)
    V.synthetic_batch(x, seed, rank, sr)
    return x
