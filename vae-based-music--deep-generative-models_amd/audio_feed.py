"""Device-resident audio corpus and its graph-capturable training feed.

Replaces the host chunk feed of the reference (data_utils.py:65-206: splitsongs / split_convert / read_data building
numpy arrays that a shuffled tf.data pipeline batches): the samples of every track stay in ONE device tensor (int16
when every track is mono 16-bit PCM, float32 otherwise), the windows are a table of start offsets (and labels), and a
step's batch is gathered and converted by one HIP kernel (vqa_corpus_batch, include/vqa.h) from a step counter that
lives on the device. The launch is therefore the same every step: `VQVAE.capture_train_step(feed)` records it inside
the step's hipGraph and an epoch of training is nothing but graph replays, with no host batch and no copy.

  corpus = AudioCorpus.from_files(files, labels, sr=22050, window=65536)     # or from_arrays(tracks, labels, ...)
  corpus = AudioCorpus.from_files(files, labels, sr=3000, window=8192, resample="best")  # files of any rate, converted
                                                                             # to sr on the device (resample.Resampler)
  train, val = corpus.split(0.1, seed=42)
  feed = AudioFeed(train, batch_size=32, seed=1)
  model.capture_train_step(feed); model.fit(feed, epochs=10); model.evaluate(AudioFeed(val, 32, shuffle=False))
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

import vqa_dp
import vqa_lib as V
from data_utils import read_wav_pcm, stratified_split
from resample import Resampler, design


def window_starts(track_lengths: Sequence[int], window: int, hop: Optional[int] = None,
                  max_signal_len: Optional[int] = None):
    """The window table of tracks laid back to back (host rule, no device): track j of track_lengths[j] samples
    (cut to max_signal_len when given) contributes the windows splitsongs would cut from it with a chunk of
    `window` samples — starts 0, hop, 2*hop, ... while the window lies wholly inside the track; a track shorter
    than `window` contributes none. hop defaults to window (no overlap).
    -> (starts (M,) int64 offsets into the concatenation of the FULL tracks, track (M,) int64 index of each
    window's track)."""
    window = int(window)
    hop = window if hop is None else int(hop)
    if window < 1 or hop < 1:
        raise ValueError(f"window {window} and hop {hop} must be positive")
    starts, track = [], []
    base = 0
    for j, n in enumerate(track_lengths):
        n = int(n)
        usable = n if max_signal_len is None else min(n, int(max_signal_len))
        if usable >= window:
            s = np.arange(0, usable - window + 1, hop, dtype=np.int64)
            starts.append(base + s)
            track.append(np.full(len(s), j, dtype=np.int64))
        base += n
    if not starts:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(starts), np.concatenate(track)


def padded_len(n: int, itemsize: int) -> int:
    """Samples to allocate so that n samples rounded up to 16 bytes are readable (vqa_corpus_batch's contract)."""
    per = 16 // itemsize
    return max(per, (n + per - 1) // per * per)


class AudioCorpus:
    """Tracks concatenated into one 1-D device tensor plus the window table (starts, labels: int64 on the device).

    samples     (padded,) int16 or float32 device tensor; `corpus_len` real samples, zero padded to 16 bytes
    starts      (M,) int64 device: first sample of each window;  labels (M,) int64 device or None
    starts_host / labels_host / track_host: the same table (and each window's track) as numpy arrays
    track_offsets / track_lengths / track_labels: where each track lies in `samples`
    """

    def __init__(self, samples: torch.Tensor, corpus_len: int, window: int, starts: np.ndarray,
                 labels: Optional[np.ndarray], track: np.ndarray, track_lengths: np.ndarray,
                 track_labels: Optional[np.ndarray]):
        self.samples, self.corpus_len, self.window = samples, int(corpus_len), int(window)
        self.device = samples.device
        self.starts_host = np.ascontiguousarray(starts, np.int64)
        self.labels_host = None if labels is None else np.ascontiguousarray(labels, np.int64)
        self.track_host = np.ascontiguousarray(track, np.int64)
        self.track_lengths = np.asarray(track_lengths, np.int64)
        self.track_offsets = np.concatenate([[0], np.cumsum(self.track_lengths)[:-1]]).astype(np.int64)
        self.track_labels = None if track_labels is None else np.asarray(track_labels, np.int64)
        # every window start is checked on the host before the table is uploaded
        if len(self.starts_host) and (self.starts_host.min() < 0
                                      or self.starts_host.max() + self.window > self.corpus_len):
            raise ValueError("a window of the table leaves the corpus")
        if padded_len(self.corpus_len, samples.element_size()) > samples.numel():
            raise ValueError("the sample tensor is not padded to 16 bytes past corpus_len")
        self.starts = torch.from_numpy(self.starts_host).to(self.device)
        self.labels = None if self.labels_host is None else torch.from_numpy(self.labels_host).to(self.device)

    def __len__(self) -> int:
        return len(self.starts_host)

    @property
    def dtype(self) -> torch.dtype:
        return self.samples.dtype

    @classmethod
    def from_arrays(cls, tracks, labels=None, window: int = 65536, hop: Optional[int] = None, device="cuda",
                    max_signal_len: Optional[int] = None, rates: Optional[Sequence[int]] = None,
                    sr: Optional[int] = None, resample: Optional[str] = None) -> "AudioCorpus":
        """tracks: a list of 1-D arrays (or (1, n) / (n, 1): one channel), one per track; labels: one class per
        track. Tracks that are ALL int16 are stored as int16 (the kernel scales by 2^-15); otherwise the whole corpus
        is float32 (an int16 track among them scaled by 2^-15, so both forms feed the same values).
        rates (one per track) with sr: the tracks' own sample rates and the corpus's. By default a track of another
        rate is a ValueError; resample="best" / "fast" converts it to sr on the device (resample.Resampler: an int16
        track is uploaded as int16, the result written straight into the corpus), tracks already at sr are not
        touched, and the corpus is float32 as soon as one track is converted. window, hop and max_signal_len count
        samples at sr."""
        arrs = []
        for t in tracks:
            a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
            if a.ndim == 2 and 1 in a.shape:
                a = a.reshape(-1)
            if a.ndim != 1:
                raise ValueError(f"a track is one channel of samples (got shape {a.shape}); average the channels first")
            arrs.append(a)
        if not arrs:
            raise ValueError("no tracks")
        if labels is not None and len(labels) != len(arrs):
            raise ValueError(f"{len(labels)} labels for {len(arrs)} tracks")
        if rates is not None:
            if sr is None or len(rates) != len(arrs):
                raise ValueError(f"rates needs sr and one rate per track ({len(rates)} rates, {len(arrs)} tracks)")
            other = [j for j, r in enumerate(rates) if int(r) != int(sr)]
            if other and resample is None:
                raise ValueError(f"track {other[0]}: sample rate {int(rates[other[0]])} Hz, requested {int(sr)} Hz "
                                 f"(tracks are not resampled)")
            if other:
                return cls._from_arrays_resampled(arrs, [int(r) for r in rates], int(sr), resample, labels, window,
                                                  hop, device, max_signal_len)
        if all(a.dtype == np.int16 for a in arrs):
            dt = np.int16
        else:
            dt = np.float32
            arrs = [a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a.astype(np.float32) for a in arrs]
        lengths = np.array([len(a) for a in arrs], np.int64)
        n = int(lengths.sum())
        host = np.zeros(padded_len(n, np.dtype(dt).itemsize), dt)
        host[:n] = np.concatenate(arrs)
        starts, track = window_starts(lengths, window, hop, max_signal_len)
        tl = None if labels is None else np.asarray(labels, np.int64)
        return cls(torch.from_numpy(host).to(device), n, window, starts, None if tl is None else tl[track], track,
                   lengths, tl)

    @classmethod
    def _from_arrays_resampled(cls, arrs, rates, sr, quality, labels, window, hop, device, max_signal_len):
        """from_arrays when a track has another rate than sr: the float32 corpus is assembled on the device, every
        track of another rate converted by the resampling kernel into its place."""
        design(rates[0], sr, quality)  # an unknown quality is refused before anything is uploaded
        lengths = np.array([len(a) if r == sr else design(r, sr, quality).output_length(len(a))
                            for a, r in zip(arrs, rates)], np.int64)
        n = int(lengths.sum())
        samples = torch.zeros(padded_len(n, 4), dtype=torch.float32, device=device)
        off = 0
        for a, r, m in zip(arrs, rates, lengths):
            m = int(m)
            if r == sr:
                h = a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a.astype(np.float32)
                samples[off:off + m] = torch.from_numpy(np.array(h)).to(device)  # a copy: a file's frames are read-only
            elif m:
                h = a if a.dtype == np.int16 else a.astype(np.float32)
                Resampler(r, sr, quality, device)(torch.from_numpy(np.array(h)).to(device), out=samples[off:off + m])
            off += m
        starts, track = window_starts(lengths, window, hop, max_signal_len)
        tl = None if labels is None else np.asarray(labels, np.int64)
        return cls(samples, n, window, starts, None if tl is None else tl[track], track, lengths, tl)

    @classmethod
    def from_files(cls, files, labels=None, sr: int = 22050, window: int = 65536, hop: Optional[int] = None,
                   duration: Optional[float] = None, max_signal_len: Optional[int] = None,
                   device="cuda", resample: Optional[str] = None) -> "AudioCorpus":
        """Integer-PCM WAV files of rate `sr` (data_utils.read_wav_pcm; by default no resampling), `duration`
        seconds of each at most, as split_convert loads them. 16-bit mono files stay int16 end to end (never through
        float); a file with more channels is averaged to mono and, like any other bit depth, makes the corpus
        float32. resample="best" / "fast" reads every file at its own rate (`duration` stays seconds of the file)
        and converts those of another rate to sr on the device (from_arrays with rates): a 16-bit mono file is
        uploaded as int16, the others as their fp32 mono average."""
        tracks, rates = [], []
        for f in files:
            a, bits, rate = read_wav_pcm(f, sr=sr if resample is None else None, duration=duration)
            rates.append(rate)
            if bits == 16 and a.shape[1] == 1:
                tracks.append(a[:, 0])
            else:
                tracks.append((a.astype(np.float64) / float(1 << (bits - 1))).mean(axis=1).astype(np.float32))
        if resample is None:
            return cls.from_arrays(tracks, labels, window=window, hop=hop, device=device,
                                   max_signal_len=max_signal_len)
        return cls.from_arrays(tracks, labels, window=window, hop=hop, device=device, max_signal_len=max_signal_len,
                               rates=rates, sr=sr, resample=resample)

    def subset(self, tracks: Sequence[int]) -> "AudioCorpus":
        """The corpus of the windows of the given tracks; the sample tensor is shared, not copied."""
        keep = np.isin(self.track_host, np.asarray(list(tracks), np.int64))
        return AudioCorpus(self.samples, self.corpus_len, self.window, self.starts_host[keep],
                           None if self.labels_host is None else self.labels_host[keep], self.track_host[keep],
                           self.track_lengths, self.track_labels)

    def split(self, test_fraction: float, seed: int = 42):
        """-> (train corpus, test corpus) sharing the sample tensor. The split is by TRACK, stratified by the
        tracks' labels (data_utils.stratified_split), so no track has windows on both sides."""
        tl = self.track_labels if self.track_labels is not None else np.zeros(len(self.track_lengths), np.int64)
        train, test = stratified_split(tl, test_fraction, seed)
        return self.subset(train), self.subset(test)


class DeviceFeed:
    """What the device feeds of one rank share (AudioFeed here, code_feed.CodeFeed): the slot rule over a table of M
    windows and the step counter on the device. Step g of the run draws slot k = ((g % S)*world + rank)*B + b of
    epoch g // S's permutation (S = steps_per_epoch): within an epoch every window is used at most once over all
    ranks. A subclass owns its batch buffers and next(), which launches the gather and then advances the counter
    (vqa_counter_add), both on the current stream, so the pair can be captured in a hipGraph and replayed."""

    def __init__(self, M: int, batch_size: int, seed: int, shuffle: bool, device, rank: Optional[int],
                 world: Optional[int], process_group):
        self.M, self.B, self.seed, self.shuffle = int(M), int(batch_size), int(seed), bool(shuffle)
        self.rank = vqa_dp.rank(process_group) if rank is None else int(rank)
        self.world = vqa_dp.world_size(process_group) if world is None else int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {self.rank} outside [0, {self.world})")
        self.steps_per_epoch = V.corpus_steps_per_epoch(self.M, self.B, self.world)
        if self.steps_per_epoch < 1:
            raise ValueError(f"{self.M} windows give no full step of {self.B} x {self.world} ranks")
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.index = torch.zeros(self.B, dtype=torch.int64, device=device)

    def __next__(self):
        return self.next()

    def __len__(self) -> int:
        return self.steps_per_epoch

    @property
    def step(self) -> int:
        """The device step counter (a synchronising read)."""
        return int(self.counter.item())

    def slots(self, step: int, rank: Optional[int] = None) -> List[int]:
        """The window numbers step `step` draws for `rank` (default: this feed's), computed on the host by the same
        rule (vqa_reset_perm_index with the feed's level)."""
        rank = self.rank if rank is None else int(rank)
        epoch, pos = divmod(int(step), self.steps_per_epoch)
        ks = [(pos * self.world + rank) * self.B + b for b in range(self.B)]
        if not self.shuffle:
            return ks
        return [V.reset_perm_index(self.seed, epoch, V.FEED_PERM_LEVEL, self.M, k) for k in ks]

    def state_dict(self):
        return {"counter": self.step, "seed": self.seed}

    def load_state_dict(self, sd):
        """Resume: the same seed and step counter draw the same batches. A train step captured with this feed keeps
        the seed it was captured with: after a change of seed the model runs eagerly until it is captured again."""
        self.seed = int(sd["seed"])
        self.counter.fill_(int(sd["counter"]))


class AudioFeed(DeviceFeed):
    """The VQ-VAE's device feed: every next() launches vqa_corpus_batch and advances the step (DeviceFeed).

    x (B, T, 1) fp32, y (B,) int64 labels (when the corpus has labels) and index (B,) int64 window numbers are the
    feed's own buffers, overwritten by each next()."""

    def __init__(self, corpus: AudioCorpus, batch_size: int, seed: int = 0, shuffle: bool = True,
                 rank: Optional[int] = None, world: Optional[int] = None, process_group=None):
        super().__init__(len(corpus), batch_size, seed, shuffle, corpus.device, rank, world, process_group)
        self.corpus = corpus
        self.x = torch.zeros(self.B, corpus.window, 1, dtype=torch.float32, device=corpus.device)
        self.y = torch.zeros(self.B, dtype=torch.int64, device=corpus.device) if corpus.labels is not None else None

    def next(self):
        """Draw this rank's batch of the current step and advance the step -> x, or (x, y) with labels."""
        c = self.corpus
        V.corpus_batch(c.samples, c.corpus_len, c.starts, c.labels, self.x, self.y, self.index, seed=self.seed,
                       counter=self.counter, step=0, rank=self.rank, world=self.world, shuffle=self.shuffle)
        V.counter_add(self.counter, 1)
        return self.x if self.y is None else (self.x, self.y)

    def __iter__(self):
        """One epoch: steps_per_epoch batches from the current step on."""
        for _ in range(self.steps_per_epoch):
            yield self.next()

    def host_batch(self, step: int, rank: Optional[int] = None) -> np.ndarray:
        """The (B, T, 1) float32 batch of `step` gathered on the host from a copy of the corpus (tests, debugging)."""
        c = self.corpus
        flat = c.samples[:c.corpus_len].cpu().numpy()
        T = c.window
        rows = [flat[s:s + T] for s in c.starts_host[self.slots(step, rank)]]
        out = np.stack(rows).astype(np.float32)
        if flat.dtype == np.int16:
            out = out / np.float32(32768.0)
        return out[:, :, None]
