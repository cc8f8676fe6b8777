"""numpy restatement of include/vqa.h's vqa_pcm_splice rule, shared by the splice and continue_audio tests. Every fp32
operation of the rule is rounded on its own, and numpy's float32 arithmetic rounds every operation on its own too, so
the restatement is exact: the kernel is compared with it bitwise."""
import numpy as np


def mix(x, p, t0, seam, fade):
    """The mixed fp32 samples s at absolute positions t0 .. t0 + n: x (..., n) fp32 is b of the rule (the decode at
    those positions), p (..., >= min(seam, t0 + n)) fp32 the prompt indexed by absolute position."""
    x = np.asarray(x, np.float32)
    n = x.shape[-1]
    t = np.arange(t0, t0 + n, dtype=np.int64)
    a = np.zeros_like(x)
    before = t < seam
    a[..., before] = np.asarray(p, np.float32)[..., t[before]]
    i = t - (seam - fade)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (i + 1).astype(np.float32) / np.float32(fade + 1)
        d = x - a
        m = d * w
        s = a + m
    assert w.dtype == d.dtype == m.dtype == s.dtype == np.float32
    return np.where(t >= seam, x, np.where(t < seam - fade, a, s)).astype(np.float32)


def quantise(s, gain=1.0):
    """(pcm int16, per-row count of clamped or NaN samples) of s (..., n) fp32: vqa_pcm_encode's rule."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(s, np.float32) * np.float32(gain)) * np.float32(32768.0)
        assert v.dtype == np.float32
        r = np.rint(v)
        bad = np.isnan(v) | (r > 32767) | (r < -32768)
        pcm = np.where(np.isnan(v), np.float32(0), np.clip(r, -32768, 32767)).astype(np.int16)
    return pcm, bad.sum(axis=-1).astype(np.int32)


def splice(x, p, t0, seam, fade, gain=1.0):
    """(pcm int16 (..., n), clipped (...,) int32) of one vqa_pcm_splice launch that writes [t0, t0 + n)."""
    return quantise(mix(x, p, t0, seam, fade), gain)
