"""VQVAESampler — drop-in for the reference's Sampler.py:10-136 (BASELINE config 5's ancestral decode).

Top-down sampling over the VQ-VAE's levels: the top prior samples one window of codes; every lower prior (an
upsampler, conditioned through its ConditionerNet on the level above) samples its window conditioned on the codes
just drawn above it. Each window is ONE persistent decode launch (Prior.sample -> vqa_prior_decode): the KV-cache
kernel walks the positions on the device, so the whole multi-level draw is `levels` launches plus the
conditioners' up-sampling — no per-token host round trip and no per-token graph replay.

Long-form sampling (sample(total_length=...)): a level's codes are drawn in overlapping windows (window_starts);
every window after the first is primed with the codes it shares with the windows before it
(vqa_prior_decode_primed) and is still one launch.

return_logprobs=True also returns, for every code, the log-probability the window that drew it gave it
(vqa_prior_decode_scored); best_of=K draws K top-level candidates per sample and keeps the one the model finds most
likely.

prompt=[codes or None per level] continues given codes: the windows, seeds and conditioning stay those of the
unprompted call, a window wholly inside the known codes launches nothing and every other is primed with the known
codes it covers (prompt_windows). continue_audio goes from a recording to its continuation: encode, sample with the
codes as the prompt, render with the recording's own samples in front (VQVAE.render(prompt_audio=...)).

averaged=True draws every level from the moving average of its prior's weights (Prior.averaged_weights; the
optimizer's average_decay), and sample_audio also renders through the VQ-VAE's averaged weights.
"""
from __future__ import annotations

from contextlib import nullcontext
from typing import List, Optional

import numpy as np
import torch

from prior import Prior


class VQVAESampler:
    """Sampler.py:10-63. n_ctxs[l]: the context (window) length of level l's prior, in that level's codes."""

    def __init__(self, down_depth, strides, n_ctxs, codebook_size=513, priors: Optional[List[Prior]] = None,
                 num_genres=None, dtype="fp32", device="cuda", seed=1, **kwargs):
        self.downsamples = [stride ** down for stride, down in zip(strides, down_depth)]
        self.hop_lengths = np.cumprod(self.downsamples)
        self.levels = len(down_depth)
        self.bins = codebook_size
        # Sampler.py:24-25
        self.x_cond_kwargs = dict(dilation_factor=3, dilation_cycle=4, residual_width=32, residual_depth=8)
        self.prior_kwargs = dict(width=128, depth=6, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.0)
        self.priors: List[Prior] = []
        if priors is not None:
            assert len(priors) == self.levels
            self.priors = list(priors)
            return

        def rescale(level, cur_level):  # Sampler.py:21-22
            return (n_ctxs[cur_level] * int(self.hop_lengths[cur_level]) // int(self.hop_lengths[level]),)

        for l in range(self.levels):
            zs_shapes = [rescale(l_, l) for l_ in range(self.levels)]
            assert zs_shapes[l][0] == n_ctxs[l]
            x_cond_kwargs = self.x_cond_kwargs if l != self.levels - 1 else None
            self.priors.append(Prior(level=l, z_shapes=zs_shapes, bins=self.bins, down_depth=down_depth,
                                     strides=strides, vqvae_model=None, prior_kwargs=self.prior_kwargs,
                                     x_cond_kwargs=x_cond_kwargs, genre_classes=num_genres, dtype=dtype,
                                     device=device, seed=seed + l))

    def sample(self, n_samples, y_genre=None, seed=0, *, total_length=None, hop_lengths=None, temperature=1.0,
               top_k=0, top_p=1.0, return_logprobs=False, best_of=1, averaged=False, prompt=None):
        """Sampler.py:65-114: from the top level down; returns [zs_0, ..., zs_{L-1}], (n_samples, codes_l) int64
        codes without the start token.

        total_length=None: one window per level (codes_l = n_ctx_l), level l drawing its Gumbel noise with
        seed + l. Otherwise long-form sampling: total_length counts top-level codes (at least the top n_ctx) and
        level l gets total_length * hop_top / hop_l codes, drawn in windows of n_ctx_l codes that start every
        hop_lengths[l] codes (default n_ctx_l // 2; window_starts). Each window is one primed decode launch, see
        sample_level. temperature / top_k / top_p: as FMHABasedAutoregressiveModel.sample, for every window.

        return_logprobs: returns (zs, logps) with logps[l] = (logp_model, logp_draw), two (n_samples, codes_l) fp32
        tensors: for every code the log-probability under the model and under the distribution it was drawn from,
        taken from the window that drew it (never from a primed position), sliced as the codes are.
        best_of=K (an integer >= 1; 1 is the plain path): the top level draws n_samples * K candidates, sample s owning
        the batch rows s K .. s K + K - 1 (y_genre repeated K times each, the seeds unchanged over all windows); the
        candidate with the highest sum of logp_model over its whole top-level sequence wins, ties to the lowest row,
        picked on the device without a read-back. The lower levels are drawn for the n_samples winners, whose
        log-probabilities are the ones returned.
        averaged=True: every level is drawn under its prior's averaged_weights(); a prior whose optimizer keeps no
        average is a ValueError before anything is drawn.
        prompt: the piece continues given codes. A list with one entry per level, (n_samples, P_l) int64 codes (the
        level's first P_l, 1 <= P_l < codes_l, none of them the prior's start token) or None: that level is drawn
        from scratch, conditioned on the level above (upsampling given the top codes). Two prompted levels' lengths
        are in the ratio of their hops. The returned codes start with the prompt; the windows, their seeds and their
        conditioning are those of the unprompted call, a window wholly inside the prompt launches nothing and every
        other is primed with the known codes it covers (prompt_windows), so the prompt cut from a draw of the same
        seed gives that draw back bit for bit. With return_logprobs the prompt positions hold 0 in both tensors, as
        primed positions do; with best_of=K the top level's prompt rows are repeated K times each, as y_genre is.
        A bad prompt is a ValueError before anything is drawn."""
        if averaged:
            self._check_averaged(self.priors)
        if isinstance(best_of, bool) or not isinstance(best_of, (int, np.integer)) or best_of < 1:
            raise ValueError(f"best_of {best_of!r} must be an integer >= 1")
        K = int(best_of)
        dev = self.priors[0].device
        zs = [torch.zeros(n_samples, 0, dtype=torch.int64, device=dev) for _ in range(self.levels)]
        totals, hops = self._plan(total_length, hop_lengths)
        prompt = self._checked_prompts(prompt, n_samples, totals)
        logps = [None] * self.levels
        for level in reversed(range(self.levels)):
            kw = dict(seed=seed, total_length=totals[level], hop_length=hops[level], temperature=temperature,
                      top_k=top_k, top_p=top_p, averaged=averaged, prompt=prompt[level])
            if K > 1 and level == self.levels - 1:
                zs[level] = torch.zeros(n_samples * K, 0, dtype=torch.int64, device=dev)
                yk = None
                if y_genre is not None:
                    yk = torch.as_tensor(y_genre, device=dev).long().reshape(-1).repeat_interleave(K)
                if prompt[level] is not None:
                    kw["prompt"] = prompt[level].repeat_interleave(K, dim=0)
                zs, lp = self.sample_level(zs, level, y_genre=yk, return_logprobs=True, **kw)
                rows = best_rows(lp[0], K)
                zs[level] = zs[level][rows]
                logps[level] = (lp[0][rows], lp[1][rows])
            elif return_logprobs:
                zs, logps[level] = self.sample_level(zs, level, y_genre=y_genre, return_logprobs=True, **kw)
            else:
                zs = self.sample_level(zs, level, y_genre=y_genre, **kw)
        return (zs, logps) if return_logprobs else zs

    def sample_audio(self, n_samples, vqvae, y_genre=None, seed=0, *, level=0, chunk_codes=4096, gain=1.0,
                     averaged=False, **sample_kwargs):
        """sample() followed by the VQ-VAE's decoder, as the reference does after every sampling run
        (utils/tf_utils.py:196-226 generate_and_save_waves: model.decode(codes, level)): draws the codes of every
        level (sample_kwargs: total_length, hop_lengths, temperature, top_k, top_p, best_of, prompt — the draw is
        sample()'s, seeds included), then renders level `level`'s codes to 16-bit PCM in chunks of chunk_codes codes
        (VQVAE.render: with a prompt, the prompt's reconstruction; continue_audio keeps the recording itself).
        Returns (pcm (n_samples, codes * hop) int16, clipped (n_samples,) int32, zs). The sampler and the VQ-VAE
        must have the same levels and hop lengths; codes outside the codebook — the start token of a prior whose
        bins exceed num_embeddings — raise VQVAE.render's ValueError. averaged=True: sample(averaged=True), and the
        render runs under the VQ-VAE's averaged_weights(); a prior or a VQ-VAE without an average is a ValueError
        before anything is drawn."""
        self._check_vqvae(vqvae, level, sample_kwargs, "sample_audio")
        if averaged:
            self._check_averaged(self.priors + [vqvae])
        zs = self.sample(n_samples, y_genre=y_genre, seed=seed, averaged=averaged, **sample_kwargs)
        with vqvae.averaged_weights() if averaged else nullcontext():
            pcm, clipped = vqvae.render(zs[level], level, chunk_codes=chunk_codes, gain=gain)
        return pcm, clipped, zs

    def _check_vqvae(self, vqvae, level, sample_kwargs, what):
        """The checks sample_audio and continue_audio make before anything is drawn."""
        if vqvae.levels != self.levels:
            raise ValueError(f"{what}: the VQ-VAE has {vqvae.levels} levels, the sampler {self.levels}")
        hops = [int(h) for h in vqvae.decode_hops]
        if hops != [int(h) for h in self.hop_lengths]:
            raise ValueError(f"{what}: the VQ-VAE's hop lengths {hops} differ from the sampler's "
                             f"{[int(h) for h in self.hop_lengths]}")
        if not 0 <= int(level) < self.levels:
            raise ValueError(f"{what}: level {level} outside [0, {self.levels})")
        if sample_kwargs.get("return_logprobs"):
            raise ValueError(f"{what} returns no log-probabilities: call sample(return_logprobs=True)")

    @staticmethod
    def _check_averaged(models):
        for m in models:
            if m.optimizer is None or not m.optimizer.averaging:
                what = f"the level {m.level} prior" if isinstance(m, Prior) else "the VQ-VAE"
                raise ValueError(f"averaged=True: {what}'s optimizer keeps no average of the weights "
                                 "(vqa_optim.Adam(average_decay=...))")

    def _start_token(self, level) -> int:
        return int(self.priors[level].prior.start_token)

    def _checked_prompts(self, prompt, n_samples, totals):
        """sample()'s prompt as a list of one checked (n_samples, P_l) int64 tensor or None per level, or ValueError."""
        if prompt is None:
            return [None] * self.levels
        if not isinstance(prompt, (list, tuple)) or len(prompt) != self.levels:
            raise ValueError(f"prompt: a list of {self.levels} entries, one per level (codes or None)")
        out = [None if z is None else self._checked_prompt(z, l, n_samples, totals[l]) for l, z in enumerate(prompt)]
        given = [l for l in range(self.levels) if out[l] is not None]
        for l in given[1:]:
            a = given[0]
            if out[a].shape[1] * int(self.hop_lengths[a]) != out[l].shape[1] * int(self.hop_lengths[l]):
                raise ValueError(f"prompt: levels {a} and {l} hold {out[a].shape[1]} and {out[l].shape[1]} codes, not "
                                 f"in the ratio of their hops {int(self.hop_lengths[a])} and "
                                 f"{int(self.hop_lengths[l])}")
        return out

    def continue_audio(self, audio, vqvae, y_genre=None, seed=0, *, total_length, level=0, fade_samples=0,
                       chunk_samples=1 << 18, chunk_codes=4096, gain=1.0, averaged=False, **sample_kwargs):
        """Go on from a recording: encode it, sample with its codes as the prompt, render with the recording itself
        in front. audio: (n, T) fp32 at the training rate, on the device or the host (loading and resampling are
        data_utils' and resample's); it is cut to a multiple of the top level's hop, the tail dropped. Its codes at
        every level (VQVAE.encode_chunked, cores of chunk_samples samples) are sample()'s prompt (sample_kwargs:
        hop_lengths, temperature, top_k, top_p, best_of; total_length counts top-level codes, the prompt included),
        and level `level`'s codes are rendered by VQVAE.render(prompt_audio=the cut audio, fade_samples=...): the
        piece is the recording's own samples up to the seam at prompt_samples, the decode after it, and a linear
        cross-fade over the fade_samples samples in front of the seam (default 0: a hard cut).
        Returns (pcm (n, total_length * hop_top) int16, clipped (n,) int32, zs, prompt_samples); the dropped tail is
        audio.shape[1] - prompt_samples. sample_audio's checks on levels and hops apply; an audio shorter than one
        top-level code and a prompt not shorter than the piece are ValueErrors, all before anything is drawn.
        averaged=True: the encode, the draw and the render run under the averaged weights."""
        self._check_vqvae(vqvae, level, sample_kwargs, "continue_audio")
        if "prompt" in sample_kwargs:
            raise ValueError("continue_audio makes the prompt from the audio: call sample(prompt=...) for codes")
        audio = torch.as_tensor(audio)
        if audio.dim() == 3 and audio.shape[-1] == 1:
            audio = audio[:, :, 0]
        if audio.dim() != 2 or audio.dtype != torch.float32:
            raise ValueError(f"continue_audio: audio must be (n, T) float32 (got {audio.dtype}, shape "
                             f"{tuple(audio.shape)})")
        hop_top = int(self.hop_lengths[-1])
        n, T = audio.shape
        prompt_samples = T // hop_top * hop_top
        if prompt_samples < hop_top:
            raise ValueError(f"continue_audio: {T} samples are shorter than one top-level code of {hop_top}")
        if prompt_samples // hop_top >= int(total_length):
            raise ValueError(f"continue_audio: the prompt's {prompt_samples // hop_top} top-level codes are not "
                             f"shorter than the piece's {int(total_length)}")
        if averaged:
            self._check_averaged(self.priors + [vqvae])
        cut = audio[:, :prompt_samples].to(vqvae.device).contiguous()
        with vqvae.averaged_weights() if averaged else nullcontext():
            prompt = [vqvae.encode_chunked(cut, l, chunk_samples=chunk_samples) for l in range(self.levels)]
        zs = self.sample(n, y_genre=y_genre, seed=seed, total_length=total_length, averaged=averaged, prompt=prompt,
                         **sample_kwargs)
        with vqvae.averaged_weights() if averaged else nullcontext():
            pcm, clipped = vqvae.render(zs[level], level, chunk_codes=chunk_codes, gain=gain, prompt_audio=cut,
                                        fade_samples=fade_samples)
        return pcm, clipped, zs, prompt_samples

    def _plan(self, total_length, hop_lengths):
        """(codes per level, hop per level) of a sample() call, checked before anything is drawn: every window
        start and end of a conditioned level must fall on a code of the level above (Prior.get_cond)."""
        n_ctxs = [pr.context_length for pr in self.priors]
        if total_length is None:
            if hop_lengths is not None:
                raise ValueError("hop_lengths needs total_length")
            return list(n_ctxs), list(n_ctxs)
        top = self.levels - 1
        total_length = int(total_length)
        if total_length < n_ctxs[top]:
            raise ValueError(f"total_length {total_length} is shorter than the top window of {n_ctxs[top]}")
        hops = [max(1, c // 2) for c in n_ctxs] if hop_lengths is None else [int(h) for h in hop_lengths]
        if len(hops) != self.levels:
            raise ValueError(f"hop_lengths has {len(hops)} entries for {self.levels} levels")
        totals = []
        for l in range(self.levels):
            # hop_lengths are cumulative products: the top level's is a multiple of every other
            totals.append(total_length * int(self.hop_lengths[top]) // int(self.hop_lengths[l]))
            self._check_windows(l, totals[l], hops[l])
        return totals, hops

    def _check_windows(self, level, total, hop):
        n_ctx = self.priors[level].context_length
        starts = window_starts(total, n_ctx, hop)  # raises ValueError for a bad total or hop
        r = self.priors[level].prior.cond_downsample_rate
        if level != self.levels - 1 and r:
            bad = [v for v in [hop, n_ctx] + starts if v % r]
            if bad:
                raise ValueError(f"level {level}: hop {hop}, window {n_ctx} and every window start must be multiples "
                                 f"of the conditioning rate {r} (got {bad[0]})")
        return starts

    def sample_level(self, zs, level, y_genre=None, seed=0, total_length=None, hop_length=None, temperature=1.0,
                     top_k=0, top_p=1.0, return_logprobs=False, averaged=False, prompt=None):
        """Sampler.py:116-124 (a stub in the reference): draw level `level` given the levels above it in zs and
        return zs with that level filled. total_length: this level's codes (default one window), hop_length: the
        distance of its window starts (default n_ctx // 2).

        Window w at start s (window_starts) is one persistent decode launch: primed with the codes already drawn
        in [s, s + n_ctx), conditioned on get_cond(zs, s, s + n_ctx), the label embedding at its position 0 as in
        a training window, its noise seeded seed + level + levels * w (window 0 keeps the one-window seed). Only
        the codes past the prime are appended. A failed launch raises; no later window is queued.
        return_logprobs: returns (zs, (logp_model, logp_draw)), (n_samples, total) fp32 each, sliced from every
        window's log-probabilities exactly as its codes are (Prior.sample; start token and prime removed).
        averaged=True: the windows are drawn under this prior's averaged_weights() (the conditioner, part of the
        prior's store, included).
        prompt: this level's first codes, (n_samples, P) int64 with 1 <= P < total_length, or None. The windows are
        prompt_windows': one that lies wholly inside the known codes launches nothing, the others are primed with the
        known codes they cover and keep their index and seed; the log-probabilities of the prompt's positions are 0."""
        pr = self.priors[level]
        with pr.averaged_weights() if averaged else nullcontext():
            return self._sample_level(pr, zs, level, y_genre, seed, total_length, hop_length, temperature, top_k,
                                      top_p, return_logprobs, prompt)

    def _sample_level(self, pr, zs, level, y_genre, seed, total_length, hop_length, temperature, top_k, top_p,
                      return_logprobs, prompt=None):
        n_ctx = pr.context_length
        total = n_ctx if total_length is None else int(total_length)
        hop = max(1, n_ctx // 2) if hop_length is None else int(hop_length)
        self._check_windows(level, total, hop)
        n_samples = zs[level].shape[0]
        if prompt is None:
            z = zs[level][:, :0]
        else:
            z = self._checked_prompt(prompt, level, n_samples, total).to(zs[level].device)
        zs = list(zs)
        lpm = lpd = None
        if return_logprobs and z.shape[1]:  # prompt positions hold 0, as primed positions do
            lpm = torch.zeros(z.shape, dtype=torch.float32, device=z.device)
            lpd = torch.zeros_like(lpm)
        for w, s, have in prompt_windows(total, n_ctx, hop, z.shape[1]):
            prime = z[:, s:s + have] if have else None
            x_cond = pr.get_cond(zs, s, s + n_ctx)
            seq = pr.sample(n_samples=n_samples, z_cond=x_cond, y=y_genre, seed=seed + level + self.levels * w,
                            prime=prime, temperature=temperature, top_k=top_k, top_p=top_p,
                            return_logprobs=return_logprobs)
            if return_logprobs:
                # position j of a window's log-probabilities scores its token j + 1: the same slice less the start
                seq, (wm, wd) = seq
                wm, wd = wm[:, have:], wd[:, have:]
                lpm = wm if lpm is None else torch.cat([lpm, wm], dim=-1)
                lpd = wd if lpd is None else torch.cat([lpd, wd], dim=-1)
            z = torch.cat([z, seq[:, 1 + have:]], dim=-1)  # start token and prime removed
        zs[level] = z
        return (zs, (lpm, lpd)) if return_logprobs else zs

    def _checked_prompt(self, prompt, level, n_samples, total) -> torch.Tensor:
        """A level's prompt as (n_samples, P) int64 with 1 <= P < total and every code one the level's prior can
        draw (not negative, below its start token), or ValueError. One read-back for the minimum and maximum."""
        z = prompt if isinstance(prompt, torch.Tensor) else torch.as_tensor(np.asarray(prompt))
        if z.dtype != torch.int64 or z.dim() != 2:
            raise ValueError(f"prompt: level {level}'s codes must be (n_samples, P) int64 (got {z.dtype}, shape "
                             f"{tuple(z.shape)})")
        if z.shape[0] != n_samples:
            raise ValueError(f"prompt: level {level} has {z.shape[0]} rows for {n_samples} samples")
        if not 1 <= z.shape[1] < total:
            raise ValueError(f"prompt: level {level}'s length {z.shape[1]} outside [1, {total}): at least one code "
                             "is drawn on every prompted level")
        lo, hi = (int(v) for v in torch.aminmax(z))
        start = self._start_token(level)
        if lo < 0 or hi >= start:
            raise ValueError(f"prompt: level {level} holds code {lo if lo < 0 else hi} outside [0, {start}), the "
                             "codes its prior can draw")
        return z.contiguous()


def best_rows(logp_model, K) -> torch.Tensor:
    """(n K, codes) log-probabilities, sample s owning rows s K .. s K + K - 1 -> (n,) int64 row of every sample's
    winner: the highest sum over the sequence, ties to the lowest row (a NaN sum ranks last). Device ops only."""
    inf = float("inf")
    sums = torch.nan_to_num(logp_model.sum(dim=1), nan=-inf, posinf=inf, neginf=-inf).reshape(-1, K)
    k = torch.arange(K, device=sums.device).expand_as(sums)
    win = torch.where(sums == sums.max(dim=1, keepdim=True).values, k, K).min(dim=1).values
    return torch.arange(sums.shape[0], device=sums.device) * K + win


def window_starts(total_length, n_ctx, hop_length) -> List[int]:
    """Starts of the windows of n_ctx codes that cover total_length codes of one level (the window rule of
    long-form sampling): 0, hop, 2 hop, ... while the window ends before total_length, then a last window that
    ends exactly there (total_length - n_ctx; every earlier start is below it, so no start repeats). Each window
    after the first shares n_ctx - hop codes (more for the last) with the windows before it."""
    if total_length < n_ctx:
        raise ValueError(f"total_length {total_length} is shorter than one window of {n_ctx}")
    if not 1 <= hop_length <= n_ctx:
        raise ValueError(f"hop_length {hop_length} outside [1, {n_ctx}]")
    starts, start = [], 0
    while start + n_ctx < total_length:
        starts.append(start)
        start += hop_length
    starts.append(total_length - n_ctx)
    return starts


def prompt_windows(total_length, n_ctx, hop_length, prompt_length=0):
    """The windows of window_starts that a level with its first prompt_length codes given (0 <= prompt_length <
    total_length) still draws: [(w, start, prime_len)], w the window's index in window_starts — it keeps its index,
    and with it its seed, whether or not the windows before it ran. `known` codes are there when a window's turn
    comes: the prompt, then everything up to the end of the last window that ran. A window with start + n_ctx <=
    known lies wholly inside them and launches nothing; every other window is primed with its prime_len =
    min(known, start + n_ctx) - start known codes (0: an unprimed window) and draws [start + prime_len,
    start + n_ctx). The drawn ranges tile [prompt_length, total_length) exactly once."""
    starts = window_starts(total_length, n_ctx, hop_length)
    if not 0 <= prompt_length < total_length:
        raise ValueError(f"prompt_length {prompt_length} outside [0, {total_length})")
    out, known = [], prompt_length
    for w, start in enumerate(starts):
        if start + n_ctx <= known:
            continue
        out.append((w, start, known - start))  # hop <= n_ctx: no window starts past what is known
        known = start + n_ctx
    return out
