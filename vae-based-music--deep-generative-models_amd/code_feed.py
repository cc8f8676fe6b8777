"""Device-resident code corpus and the prior's graph-capturable training feed.

The prior trains on the VQ-VAE's codes, and the frozen encoder gives the same codes for the same audio every time:
instead of re-running it on every step (prior.py:257-260, `Prior._codes` on raw audio), the corpus is tokenized ONCE
(`VQVAE.encode_chunked`, bounded memory), the codes of every level stay in device memory — track after track, one
1-D tensor per level — and a step's batch is gathered by one HIP kernel (vqa_code_batch, include/vqa.h) from a step
counter that lives on the device: the window of this level, the window of the level above that lies over it (the
upsampler's conditioning) and the genre label. `Prior.capture_train_step(feed)` records that launch inside the
step's hipGraph, so an epoch of prior training is nothing but graph replays, as it is for the VQ-VAE with
audio_feed.AudioFeed.

  codes = CodeCorpus.from_audio(audio_corpus, vqvae)           # or from_codes(...) / CodeCorpus.load(path)
  train, val = codes.split(0.1, seed=42)
  feed = CodeFeed(train, level=1, n_ctx=8192, batch_size=8, seed=1)
  prior.capture_train_step(feed); prior.fit(feed, epochs=10)
  prior.evaluate(CodeFeed(val, 1, 8192, 8, shuffle=False))
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

import vqa_lib as V
from audio_feed import DeviceFeed, padded_len, window_starts
from data_utils import stratified_split


def code_dtype(num_embeddings: int):
    """The storage of a code below num_embeddings: int16 up to 32768 entries, int32 above."""
    return np.int16 if int(num_embeddings) <= 32768 else np.int32


class CodeCorpus:
    """The codes of every track at every level, track after track; each level is one 1-D device tensor.

    codes[l]        (padded,) int16 (num_embeddings <= 32768) or int32 device tensor, zero padded to 16 bytes past
                    code_lens[l] codes (vqa_code_batch's contract)
    lengths[l][j]   codes of track j at level l;  offsets[l][j] where they start in codes[l]
    track_labels    (tracks,) int64 or None;  hops[l] audio samples per code of level l
    tracks          the tracks this corpus draws windows from (all of them, or the subset of subset / split)
    Every track holds a whole number of top-level codes, so lengths[l][j] * hops[l] is the same at every level and
    offsets[l][j] = rate * offsets[l + 1][j] with rate = hops[l + 1] / hops[l]: code t of level l lies under code
    t / rate of level l + 1, at the same place in both tensors."""

    def __init__(self, codes: Sequence[torch.Tensor], lengths, track_labels, hops, num_embeddings: int,
                 tracks: Optional[Sequence[int]] = None):
        self.codes = list(codes)
        self.levels = len(self.codes)
        self.hops = [int(h) for h in hops]
        self.num_embeddings = int(num_embeddings)
        self.lengths = [np.asarray(n, np.int64).reshape(-1) for n in lengths]
        if not (self.levels == len(self.hops) == len(self.lengths)) or self.levels < 1:
            raise ValueError("one code tensor, one length array and one hop per level")
        self.device = self.codes[0].device
        n_tracks = len(self.lengths[0])
        self.track_labels = None if track_labels is None else np.asarray(track_labels, np.int64).reshape(-1)
        if self.track_labels is not None and len(self.track_labels) != n_tracks:
            raise ValueError(f"{len(self.track_labels)} labels for {n_tracks} tracks")
        for l in range(self.levels):
            if self.hops[l] < 1 or (l and self.hops[l] % self.hops[l - 1]):
                raise ValueError(f"hops {self.hops}: each level's hop is a positive multiple of the level below's")
            if len(self.lengths[l]) != n_tracks or np.any(self.lengths[l] * self.hops[l]
                                                          != self.lengths[-1] * self.hops[-1]):
                raise ValueError(f"level {l}: the tracks' code lengths do not agree with the hops {self.hops} "
                                 f"(every level covers the same samples of a track)")
            t = self.codes[l]
            if t.dim() != 1 or t.dtype != torch.from_numpy(np.zeros(0, code_dtype(self.num_embeddings))).dtype:
                raise ValueError(f"level {l}: codes are a 1-D {code_dtype(self.num_embeddings).__name__} tensor")
            if padded_len(int(self.lengths[l].sum()), t.element_size()) > t.numel():
                raise ValueError(f"level {l}: the code tensor is not padded to 16 bytes past its length")
        self.code_lens = [int(n.sum()) for n in self.lengths]
        self.offsets = [np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) for n in self.lengths]
        self.tracks = (np.arange(n_tracks, dtype=np.int64) if tracks is None
                       else np.unique(np.asarray(list(tracks), np.int64)))
        if len(self.tracks) and (self.tracks.min() < 0 or self.tracks.max() >= n_tracks):
            raise ValueError(f"tracks outside [0, {n_tracks})")

    def __len__(self) -> int:
        return len(self.tracks)

    def rate(self, level: int) -> int:
        """Codes of `level` per code of the level above."""
        return self.hops[level + 1] // self.hops[level]

    def track_codes(self, level: int, track: int) -> torch.Tensor:
        """The stored codes of one track (a view of the level's tensor)."""
        o, n = int(self.offsets[level][track]), int(self.lengths[level][track])
        return self.codes[level][o:o + n]

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_codes(cls, tracks_per_level, labels, hops, num_embeddings, device="cuda") -> "CodeCorpus":
        """tracks_per_level[l][j]: the 1-D integer codes of track j at level l (arrays or tensors). Checked here:
        the levels' track lengths agree with the hops, and every code lies in [0, num_embeddings)."""
        dt = code_dtype(num_embeddings)
        if len(tracks_per_level) != len(hops) or not len(hops):
            raise ValueError(f"{len(tracks_per_level)} levels of tracks for {len(hops)} hops")
        stores, lengths = [], []
        for l, tracks in enumerate(tracks_per_level):
            arrs = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in tracks]
            if not arrs:
                raise ValueError("no tracks")
            for j, a in enumerate(arrs):
                if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"level {l} track {j}: codes are a 1-D integer array (got {a.dtype}, {a.shape})")
                if len(a) and (int(a.min()) < 0 or int(a.max()) >= int(num_embeddings)):
                    raise ValueError(f"level {l} track {j}: a code outside [0, {int(num_embeddings)})")
            n = int(sum(len(a) for a in arrs))
            host = np.zeros(padded_len(n, np.dtype(dt).itemsize), dt)
            host[:n] = np.concatenate(arrs).astype(dt)
            stores.append(torch.from_numpy(host).to(device))
            lengths.append([len(a) for a in arrs])
        return cls(stores, lengths, labels, hops, num_embeddings)

    @classmethod
    def from_audio(cls, audio_corpus, vqvae, chunk_samples: int = 1 << 18) -> "CodeCorpus":
        """Tokenize every track of an audio_feed.AudioCorpus with `vqvae`, at every level, once. A track's samples
        are taken from the corpus' device tensor (int16 scaled by 2^-15, exact: the values the audio feed
        produces), cut to a multiple of the top level's hop (the tail shorter than one top-level code is dropped, a
        track shorter than that is dropped with its label) and encoded by VQVAE.encode_chunked, so memory is
        bounded by one chunk whatever the track's length."""
        hops = vqvae.encode_hops
        top = hops[-1]
        dt = torch.from_numpy(np.zeros(0, code_dtype(vqvae.num_embeddings))).dtype
        per_level = [[] for _ in hops]
        keep = []
        for j, (off, n) in enumerate(zip(audio_corpus.track_offsets, audio_corpus.track_lengths)):
            n = int(n) // top * top
            if n < top:
                continue
            keep.append(j)
            x = audio_corpus.samples[int(off):int(off) + n]
            x = (x.to(torch.float32) * (1.0 / 32768.0) if x.dtype == torch.int16 else x.to(torch.float32))
            x = x.to(vqvae.device).view(1, n, 1)
            for l in range(len(hops)):
                per_level[l].append(vqvae.encode_chunked(x, l, chunk_samples=chunk_samples).view(-1).to(dt))
        if not keep:
            raise ValueError(f"no track holds one top-level code ({top} samples)")
        stores, lengths = [], []
        for l, tracks in enumerate(per_level):
            n = sum(t.numel() for t in tracks)
            store = torch.zeros(padded_len(n, tracks[0].element_size()), dtype=dt, device=vqvae.device)
            store[:n] = torch.cat(tracks)
            stores.append(store)
            lengths.append([t.numel() for t in tracks])
        tl = audio_corpus.track_labels
        return cls(stores, lengths, None if tl is None else np.asarray(tl)[keep], hops, vqvae.num_embeddings)

    # ------------------------------------------------------------------ subsets
    def subset(self, tracks: Sequence[int]) -> "CodeCorpus":
        """The corpus of the given tracks; the code tensors are shared, not copied."""
        return CodeCorpus(self.codes, self.lengths, self.track_labels, self.hops, self.num_embeddings, tracks)

    def split(self, test_fraction: float, seed: int = 42):
        """-> (train corpus, test corpus) sharing the code tensors. The split is by TRACK, stratified by the
        tracks' labels (data_utils.stratified_split), so no track has windows on both sides."""
        tl = (self.track_labels[self.tracks] if self.track_labels is not None
              else np.zeros(len(self.tracks), np.int64))
        train, test = stratified_split(tl, test_fraction, seed)
        return self.subset(self.tracks[train]), self.subset(self.tracks[test])

    # ------------------------------------------------------------------ disk
    def save(self, path):
        """An .npz of arrays only: codes{l} (this corpus' tracks back to back, unpadded), lengths (levels, tracks),
        labels ((tracks,), or empty when the corpus has none), hops and num_embeddings."""
        out = {"hops": np.asarray(self.hops, np.int64), "num_embeddings": np.asarray(self.num_embeddings, np.int64),
               "lengths": np.stack([n[self.tracks] for n in self.lengths]),
               "labels": (np.zeros(0, np.int64) if self.track_labels is None else self.track_labels[self.tracks])}
        for l in range(self.levels):
            parts = [self.track_codes(l, int(j)).cpu().numpy() for j in self.tracks]
            out[f"codes{l}"] = np.concatenate(parts) if parts else np.zeros(0, code_dtype(self.num_embeddings))
        with open(path, "wb") as f:
            np.savez(f, **out)

    @classmethod
    def load(cls, path, device="cuda") -> "CodeCorpus":
        """Read a `save` file (numpy arrays only, nothing in it is executed); every check of the constructor and of
        the code range runs again."""
        with np.load(path, allow_pickle=False) as f:
            hops, K, lengths = f["hops"].tolist(), int(f["num_embeddings"]), f["lengths"]
            labels = f["labels"] if f["labels"].size else None
            tracks = []
            for l in range(len(hops)):
                flat = f[f"codes{l}"]
                if len(flat) != int(lengths[l].sum()):
                    raise ValueError(f"{path}: level {l} holds {len(flat)} codes, its track lengths {lengths[l].sum()}")
                tracks.append(np.split(flat, np.cumsum(lengths[l])[:-1]))
        return cls.from_codes(tracks, labels, hops, K, device=device)


class CodeFeed(DeviceFeed):
    """The device feed of one rank for the prior of `level`: every next() launches vqa_code_batch and advances the
    step (audio_feed.DeviceFeed: the slot rule, and the permutation key, of audio_feed.AudioFeed). The window table
    is built here on the host: within each track starts 0, hop, 2 hop, ... while the window of n_ctx codes lies
    inside the track (hop defaults to n_ctx).

    conditioned (default: every level but the top): the windows of the level above come with the batch; n_ctx and
    hop, and so every start, must then be multiples of rate = hops[level + 1] / hops[level].

    codes (B, n_ctx) int64, upper (B, n_ctx / rate) int64 or None, y (B,) int64 labels or None and index (B,) int64
    window numbers are the feed's own buffers, overwritten by each next()."""

    def __init__(self, corpus: CodeCorpus, level: int, n_ctx: int, batch_size: int, hop: Optional[int] = None,
                 seed: int = 0, shuffle: bool = True, conditioned: Optional[bool] = None, rank: Optional[int] = None,
                 world: Optional[int] = None, process_group=None):
        self.corpus, self.level, self.n_ctx, self.B = corpus, int(level), int(n_ctx), int(batch_size)
        if not 0 <= self.level < corpus.levels:
            raise ValueError(f"level {self.level} outside [0, {corpus.levels})")
        self.hop = self.n_ctx if hop is None else int(hop)
        if self.n_ctx < 1 or self.hop < 1 or self.B < 1:
            raise ValueError(f"n_ctx {self.n_ctx}, hop {self.hop} and batch_size {self.B} must be positive")
        top = self.level == corpus.levels - 1
        self.conditioned = (not top) if conditioned is None else bool(conditioned)
        if self.conditioned and top:
            raise ValueError(f"level {self.level} is the top level: there is no level above to condition on")
        self.rate = corpus.rate(self.level) if self.conditioned else 1
        if self.n_ctx % self.rate or self.hop % self.rate:
            raise ValueError(f"a conditioned feed needs n_ctx {self.n_ctx} and hop {self.hop} to be multiples of "
                             f"rate {self.rate} (the codes of level {self.level} under one code of the level above)")
        # the table: window_starts over ALL tracks (offsets into the level's tensor), then the corpus' own tracks
        starts, track = window_starts(corpus.lengths[self.level], self.n_ctx, self.hop)
        keep = np.isin(track, corpus.tracks)
        self.starts_host, self.track_host = starts[keep], track[keep]
        self.labels_host = None if corpus.track_labels is None else corpus.track_labels[self.track_host]
        if len(self.starts_host) and (self.starts_host.min() < 0 or self.starts_host.max() + self.n_ctx
                                      > corpus.code_lens[self.level] or np.any(self.starts_host % self.rate)):
            raise ValueError("a window of the table leaves the corpus or is not a multiple of rate")
        dev = corpus.device
        super().__init__(len(self.starts_host), self.B, seed, shuffle, dev, rank, world, process_group)
        self.starts = torch.from_numpy(self.starts_host).to(dev)
        self.labels = None if self.labels_host is None else torch.from_numpy(self.labels_host).to(dev)
        self.codes = torch.zeros(self.B, self.n_ctx, dtype=torch.int64, device=dev)
        self.upper = (torch.zeros(self.B, self.n_ctx // self.rate, dtype=torch.int64, device=dev)
                      if self.conditioned else None)
        self.y = torch.zeros(self.B, dtype=torch.int64, device=dev) if self.labels is not None else None

    def next(self):
        """Draw this rank's batch of the current step and advance the step -> (codes, upper or None, y or None)."""
        c, l = self.corpus, self.level
        V.code_batch(c.codes[l], c.code_lens[l], self.starts, self.labels, self.codes,
                     upper=c.codes[l + 1] if self.conditioned else None,
                     upper_len=c.code_lens[l + 1] if self.conditioned else 0, rate=self.rate, z_upper=self.upper,
                     labels_out=self.y, index_out=self.index, seed=self.seed, counter=self.counter, step=0,
                     rank=self.rank, world=self.world, shuffle=self.shuffle)
        V.counter_add(self.counter, 1)
        return self.codes, self.upper, self.y

    def batch(self):
        """The feed's buffers as the tuple Prior.train_step / test_step take: (codes[, upper][, y])."""
        return tuple(t for t in (self.codes, self.upper, self.y) if t is not None)

    def __iter__(self):
        """One epoch: steps_per_epoch batches from the current step on (each the tuple of `batch`)."""
        for _ in range(self.steps_per_epoch):
            self.next()
            yield self.batch()

    def host_batch(self, step: int, rank: Optional[int] = None):
        """(codes (B, n_ctx), upper (B, n_ctx / rate) or None, y (B,) or None) int64 numpy arrays of `step`, gathered
        on the host from a copy of the corpus (tests, debugging)."""
        c, l = self.corpus, self.level
        idx = self.slots(step, rank)
        flat = c.codes[l][:c.code_lens[l]].cpu().numpy()
        codes = np.stack([flat[s:s + self.n_ctx] for s in self.starts_host[idx]]).astype(np.int64)
        upper = None
        if self.conditioned:
            up, n = c.codes[l + 1][:c.code_lens[l + 1]].cpu().numpy(), self.n_ctx // self.rate
            upper = np.stack([up[s // self.rate:s // self.rate + n] for s in self.starts_host[idx]]).astype(np.int64)
        return codes, upper, None if self.labels_host is None else self.labels_host[idx]
