"""Sample-rate conversion: the filter design, its fp64 restatement and the device resampler.

The reference loads every file through librosa.load(file, sr=sample_rate) (data_utils.py:43-48), which resamples it
to the training rate. Here that step is a polyphase windowed-sinc filter pinned by three numbers — zero crossings Z,
rolloff rho and Kaiser beta, the public "kaiser_best" / "kaiser_fast" designs — so that host and device compute the
same thing and a test can state it exactly:

  g = gcd(sr_in, sr_out), L = sr_out / g (up), M = sr_in / g (down)
  s = rho * min(1, L / M), Wf = Z / s, W = ceil(Wf), P = 2 W taps per phase
  T[r][i] = fp32( s * sinc(s t) * kaiser(t / Wf) ),  t = (i - W + 1) - r / L,  r in [0, L), i in [0, P)
            kaiser(u) = I0(beta sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0     (fp64, rounded once)
  y[m]    = sum_i x[k0 + i - W + 1] * T[r][i],  k0, r = divmod(m M, L),  x zero outside the track,
            m in [0, ceil(n L / M)): output m sits at input time m M / L exactly, no delay

`resample_reference` evaluates that sum in numpy fp64 from the fp32 table (the oracle of the tests and the host path
of data_utils.load_audio); `Resampler` runs it on the device (vqa_resample, csrc/vqa_resample.hip), whole or in
chunks with bitwise equal results. Parity is to this stated design, not to librosa bit for bit.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

import vqa_lib as V

# quality -> (zero crossings, rolloff, Kaiser beta)
QUALITIES = {
    "best": (32, 0.9475937167399596, 14.769656459379492),
    "fast": (16, 0.85, 8.555504641634386),
}


def output_length(n: int, up: int, down: int) -> int:
    """ceil(n * up / down): the outputs of a track of n samples."""
    return -((-int(n) * int(up)) // int(down))


def design_table(up: int, down: int, quality: str = "best") -> Tuple[int, np.ndarray]:
    """(W, the fp64 table (up, 2 W)) of the design above, before the rounding to fp32."""
    if quality not in QUALITIES:
        raise ValueError(f"resample quality {quality!r} is not one of {sorted(QUALITIES)}")
    Z, rho, beta = QUALITIES[quality]
    s = rho * min(1.0, up / down)
    Wf = Z / s
    W = int(math.ceil(Wf))
    j = np.arange(2 * W, dtype=np.float64) - W + 1
    t = j[None, :] - (np.arange(up, dtype=np.float64) / up)[:, None]
    u = t / Wf
    inside = np.abs(u) < 1.0
    win = np.where(inside, np.i0(beta * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(beta), 0.0)
    return W, s * np.sinc(s * t) * win


class ResamplePlan:
    """One conversion: up = L, down = M, W, P = 2 W, `table` the (L, P) fp32 taps; device_table(device) is its
    device copy, uploaded once per device."""

    def __init__(self, sr_in: int, sr_out: int, quality: str):
        self.sr_in, self.sr_out, self.quality = int(sr_in), int(sr_out), quality
        if self.sr_in < 1 or self.sr_out < 1:
            raise ValueError(f"sample rates {sr_in} and {sr_out} must be positive")
        g = math.gcd(self.sr_in, self.sr_out)
        self.up, self.down = self.sr_out // g, self.sr_in // g
        self.W, t64 = design_table(self.up, self.down, quality)
        self.P = 2 * self.W
        self.table = np.ascontiguousarray(t64, dtype=np.float32)
        self._device: Dict[str, torch.Tensor] = {}

    @property
    def identity(self) -> bool:
        return self.up == self.down  # both 1: equal rates

    def device_table(self, device) -> torch.Tensor:
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.table).to(device)
        return self._device[key]

    def output_length(self, n: int) -> int:
        return output_length(n, self.up, self.down)

    def input_span(self, m0: int, n_out: int, track_len: int) -> Tuple[int, int]:
        """[lo, hi): the samples of a track of track_len that outputs [m0, m0 + n_out) read (vqa_resample's rule)."""
        lo = max(m0 * self.down // self.up - self.W + 1, 0)
        hi = min((m0 + n_out - 1) * self.down // self.up + self.W, track_len - 1)
        return lo, hi + 1

    def abs_row_sum(self) -> float:
        """max_r sum_i |T[r][i]|: the gain of the worst phase, which scales every rounding-error bound."""
        return float(np.abs(self.table.astype(np.float64)).sum(axis=1).max())


_PLANS: Dict[Tuple[int, int, str], ResamplePlan] = {}


def design(sr_in: int, sr_out: int, quality: str = "best") -> ResamplePlan:
    """The plan of sr_in -> sr_out, cached per (rates, quality); its device copies are cached per device."""
    key = (int(sr_in), int(sr_out), quality)
    if key not in _PLANS:
        _PLANS[key] = ResamplePlan(sr_in, sr_out, quality)
    return _PLANS[key]


def resample_reference(x, plan: ResamplePlan, block: int = 8192) -> np.ndarray:
    """The sum above in fp64 from the fp32 table: x (..., n) real samples -> (..., ceil(n L / M)) float64. Equal
    rates return the input (as float64)."""
    x = np.asarray(x, dtype=np.float64)
    if plan.identity:
        return x
    n = x.shape[-1]
    L, M, W, P = plan.up, plan.down, plan.W, plan.P
    n_out = plan.output_length(n)
    T = plan.table.astype(np.float64)
    pad = [(0, 0)] * (x.ndim - 1) + [(W - 1, W + 1)]
    xp = np.pad(x, pad)  # xp[k + W - 1] = x[k]
    y = np.empty(x.shape[:-1] + (n_out,), np.float64)
    taps = np.arange(P, dtype=np.int64)
    for a in range(0, n_out, block):
        m = np.arange(a, min(a + block, n_out), dtype=np.int64)
        k0, r = np.divmod(m * M, L)
        idx = k0[:, None] + taps[None, :]  # into xp: (k0 + i - W + 1) + (W - 1)
        y[..., a:a + len(m)] = np.einsum("...mp,mp->...m", xp[..., idx], T[r])
    return y


class Resampler:
    """sr_in -> sr_out on the device. __call__(x): x (n,) or (B, n), int16 (read as x * 2^-15) or fp32 device tensor
    -> fp32 of ceil(n L / M) samples per row (`out`: write there instead of allocating). Equal rates launch nothing:
    fp32 comes back as it is, int16 scaled."""

    def __init__(self, sr_in: int, sr_out: int, quality: str = "best", device="cuda"):
        self.plan = design(sr_in, sr_out, quality)
        self.device = torch.device(device)
        self.taps = None if self.plan.identity else self.plan.device_table(self.device)

    def route(self):
        """(table_in_lds, tile_outputs) of this conversion's launches (vqa_resample_route)."""
        return V.resample_route(self.plan.up, self.plan.down, self.plan.P)

    def _unchanged(self, x):
        return x if x.dtype == torch.float32 else x.to(torch.float32) * (1.0 / 32768.0)

    def _out(self, x, out):
        n_out = self.plan.output_length(x.shape[-1])
        if out is None:
            out = torch.empty(x.shape[:-1] + (n_out,), dtype=torch.float32, device=x.device)
        elif out.shape != x.shape[:-1] + (n_out,):
            raise ValueError(f"out is {tuple(out.shape)}, the result {tuple(x.shape[:-1]) + (n_out,)}")
        return out

    def __call__(self, x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        if self.plan.identity:
            return self._unchanged(x)
        out = self._out(x, out)
        V.resample(x, out, self.taps, self.plan.up, self.plan.down)
        return out

    def chunked(self, x: torch.Tensor, chunk_outputs: int, out: torch.Tensor = None) -> torch.Tensor:
        """The same result, bit for bit, through calls of at most chunk_outputs outputs, each given only the slice
        of x its outputs read (vqa_resample's m0 / in0 form: what a streamed track would pass)."""
        if self.plan.identity:
            return self._unchanged(x)
        chunk_outputs = int(chunk_outputs)
        if chunk_outputs < 1:
            raise ValueError(f"chunk_outputs {chunk_outputs} must be positive")
        out = self._out(x, out)
        n, n_out = x.shape[-1], out.shape[-1]
        for m0 in range(0, n_out, chunk_outputs):
            c = min(chunk_outputs, n_out - m0)
            lo, hi = self.plan.input_span(m0, c, n)
            V.resample(x[..., lo:hi], out[..., m0:m0 + c], self.taps, self.plan.up, self.plan.down, in0=lo, m0=m0,
                       track_len=n)
        return out
