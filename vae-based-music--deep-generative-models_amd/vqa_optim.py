"""keras.optimizers.Adam (TF 2.7 defaults) over a ParamStore: one libvqa launch per step.

Keras' Adam hands each variable to TF's ApplyAdam with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) and eps = 1e-7
applied after the bias correction (not PyTorch's form). `iterations` lives on the device so a captured
train step replays with the right t. `learning_rate` is a float or a keras LearningRateSchedule
(schedules.CustomSchedule — src/transformer/multi_head_attention.py:82-101 — or ExponentialDecay): a schedule
is evaluated on the device from `iterations` (vqa_lr_schedule) right before the update, so graph replay stays
valid.

Gradient clipping is OptimizerV2's: `clipvalue`, `clipnorm` (per variable) and `global_clipnorm`, applied in
that order to the aggregated gradient grad_scale * g (after the data-parallel exchange, as Keras clips after
aggregation). The norms, the scale and the clipped update are kernels on the step's stream (vqa_grad_norm,
vqa_adam_keras_clipped), so a captured step replays them; nothing is read back. The gradient buffer is not
rewritten. Deviation from Keras: a threshold of 0 (which Keras accepts and which zeroes every gradient) is
refused, as is any value that is not finite and > 0. The thresholds are configuration, not state: checkpoints
hold nothing of them.

Weight averaging is tensorflow_addons' MovingAverage wrapper folded into the step: with `average_decay` set, the
Adam launch also updates `average`, an exponential moving average of the flat parameter buffer (DESIGN.md states the
rule), keyed by the same device step count as a learning-rate schedule, so a captured step replays it.
`average_start_step` and `dynamic_average_decay` are tfa's start_step and dynamic_decay. assign_average_vars and
swap_weights carry tfa's names; swap_weights exchanges contents exactly (vqa_swap_f32). The three settings are
configuration like the thresholds; the average itself is state and travels in checkpoints.

Skipping non-finite steps is Keras' LossScaleOptimizer rule without the loss scale: with `skip_nonfinite=True` a step
whose aggregated gradient holds a NaN or an inf is not applied. vqa_grad_finite writes a device flag from the gradient
(after the data-parallel exchange, so every rank reads the same bits and decides alike), the update and the increment
of `iterations` run behind it (vqa_adam_keras_guarded, vqa_counter_add_if), and two device counters keep the skipped
steps in all and in a row. A skipped step writes no byte of the weights, the moments or the average and leaves
`iterations`, hence the bias correction, a schedule's rate and the average's start step and dynamic decay, where they
were. Nothing is read back; a captured step replays the decision. The setting is configuration; the two counters are
state and travel in checkpoints.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import vqa_lib as V
from schedules import LearningRateSchedule

# Adam.grad_stats() keys, in the order of vqa_grad_norm's `stats`
GRAD_STATS = ("global_norm", "clipped_global_norm", "global_scale", "clipnorm_variables", "clipvalue_elements")
# Adam.skip_stats() keys
SKIP_STATS = ("skipped_steps", "consecutive_skipped", "last_step_ok")


def _threshold(name, value):
    if value is None:
        return None
    try:
        c = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: a finite number > 0 or None (got {value!r})") from None
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"{name}: a finite number > 0 or None (got {value!r}; Keras' 0 is refused)")
    return c


def _average_settings(decay, start_step, dynamic):
    """(decay or None, start step, dynamic) checked as the constructor's arguments."""
    if decay is None:
        if start_step != 0 or dynamic:
            raise ValueError("average_start_step and dynamic_average_decay need average_decay "
                             f"(got average_start_step={start_step!r}, dynamic_average_decay={dynamic!r})")
        return None, 0, False
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"average_decay: a finite number in [0, 1) or None (got {decay!r})") from None
    if isinstance(decay, bool) or not (math.isfinite(d) and 0.0 <= d < 1.0):
        raise ValueError(f"average_decay: a finite number in [0, 1) or None (got {decay!r})")
    if isinstance(start_step, bool) or not isinstance(start_step, (int, np.integer)) or start_step < 0:
        raise ValueError(f"average_start_step: an integer >= 0 (got {start_step!r})")
    return d, int(start_step), bool(dynamic)


def clip_tables(offsets, size: int):
    """The variable table of vqa_grad_norm / vqa_adam_keras_clipped for a ParamStore layout (host, numpy):
    seg_start (int64, one ascending offset per variable) and block_seg (int32, per block of V.CLIP_BLOCK floats the
    variable that holds the block's first element)."""
    seg = np.array(sorted(int(o) for o, _ in offsets.values()), np.int64)
    if seg.size == 0 or seg[0] != 0 or np.any(seg % 4) or np.any(np.diff(seg) <= 0) or seg[-1] >= size:
        raise ValueError("clip_tables: offsets must start at 0, ascend and be multiples of 4 floats")
    nblk = -(-size // V.CLIP_BLOCK)
    first = np.arange(nblk, dtype=np.int64) * V.CLIP_BLOCK
    block_seg = (np.searchsorted(seg, first, side="right") - 1).astype(np.int32)
    return seg, block_seg


class Adam:
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, *, clipvalue=None,
                 clipnorm=None, global_clipnorm=None, average_decay=None, average_start_step=0,
                 dynamic_average_decay=False, skip_nonfinite=False, **kwargs):
        if callable(learning_rate) and not isinstance(learning_rate, LearningRateSchedule):
            # a host callable cannot be evaluated inside a replayed hipGraph
            raise TypeError("learning_rate: a float or a schedules.LearningRateSchedule (device-evaluated)")
        if clipnorm is not None and global_clipnorm is not None:
            raise ValueError(f"Cannot accept both `clipnorm` and `global_clipnorm`, received: clipnorm={clipnorm}, "
                             f"global_clipnorm={global_clipnorm}")
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon
        self.clipvalue = _threshold("clipvalue", clipvalue)
        self.clipnorm = _threshold("clipnorm", clipnorm)
        self.global_clipnorm = _threshold("global_clipnorm", global_clipnorm)
        self.average_decay, self.average_start_step, self.dynamic_average_decay = _average_settings(
            average_decay, average_start_step, dynamic_average_decay)
        if not isinstance(skip_nonfinite, (bool, np.bool_)):
            raise ValueError(f"skip_nonfinite: True or False (got {skip_nonfinite!r})")
        self.skip_nonfinite = bool(skip_nonfinite)
        self.iterations = None
        self.m = self.v = None
        self.average = None  # the weights' moving average, a flat buffer like store.flat (build)
        self._lr_dev = None
        self._clip = None  # device tables, norms, statistics and workspace of the clipped path (build)
        self.step_ok = None  # the guard's flag (int32[1]) and counters (int64[2]: skipped in all, in a row) (build)
        self.skipped = None

    @property
    def scheduled(self) -> bool:
        return isinstance(self.learning_rate, LearningRateSchedule)

    @property
    def clip_modes(self) -> int:
        return ((V.CLIP_VALUE if self.clipvalue is not None else 0) | (V.CLIP_NORM if self.clipnorm is not None else 0)
                | (V.CLIP_GLOBAL_NORM if self.global_clipnorm is not None else 0))

    @property
    def averaging(self) -> bool:
        return self.average_decay is not None

    def build(self, store):
        dev = store.flat.device
        self.m = torch.zeros_like(store.flat)
        self.v = torch.zeros_like(store.flat)
        self.iterations = torch.zeros(1, dtype=torch.int64, device=dev)
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=dev) if self.scheduled else None
        # allocated once (a captured step keeps the pointer); starts as the weights, as tfa's slot does
        self.average = store.flat.detach().clone() if self.averaging else None
        if self.skip_nonfinite:
            # allocated once: a captured step keeps these pointers
            self.step_ok = torch.ones(1, dtype=torch.int32, device=dev)
            self.skipped = torch.zeros(2, dtype=torch.int64, device=dev)
        if self.clip_modes:
            # allocated once: a captured step keeps these pointers
            seg, block_seg = clip_tables(store.offsets, store.size)
            self._clip = dict(
                seg_start=torch.from_numpy(seg).to(dev), block_seg=torch.from_numpy(block_seg).to(dev),
                seg_norm=torch.zeros(seg.size, dtype=torch.float32, device=dev),
                stats=torch.zeros(V.CLIP_STATS, dtype=torch.float32, device=dev),
                ws=V.workspace(V.grad_norm_workspace(store.size, seg.size), dev))

    def current_learning_rate(self) -> float:
        """The rate the next apply() uses (host evaluation of the schedule at the device step count)."""
        if not self.scheduled:
            return float(self.learning_rate)
        return self.learning_rate(int(self.iterations.item()))

    def grad_stats(self):
        """The last clipped step's statistics as 0-dim device tensors (views of one buffer the step writes; no
        host sync): the global norm of grad_scale * g before any clipping, the global norm after `clipvalue` (what
        the norm modes see), the factor `global_clipnorm` applied (1 when off), the number of variables whose norm
        exceeded `clipnorm`, the number of elements `clipvalue` clamped."""
        if self._clip is None:
            raise RuntimeError("grad_stats: no clipping configured, or the optimizer is not built yet")
        return {k: self._clip["stats"][i] for i, k in enumerate(GRAD_STATS)}

    def variable_grad_norms(self) -> torch.Tensor:
        """Per-variable norms of the last clipped step's gradient (after `clipvalue`), in offset order."""
        if self._clip is None:
            raise RuntimeError("variable_grad_norms: no clipping configured, or the optimizer is not built yet")
        return self._clip["seg_norm"]

    def skip_stats(self):
        """The step guard's state as 0-dim device tensors (views of the buffers the step writes; no host sync): the
        steps skipped in all, the steps skipped in a row up to and including the last one (0 after an applied step),
        and the last step's flag (1 applied, 0 skipped)."""
        if self.skipped is None:
            raise RuntimeError("skip_stats: skip_nonfinite is off, or the optimizer is not built yet")
        return dict(zip(SKIP_STATS, (self.skipped[0], self.skipped[1], self.step_ok[0])))

    def apply(self, store, grad_scale: float = 1.0):
        if self.m is None:
            self.build(store)
        g = store.grad[:store.size]
        if self.skip_nonfinite:  # the flag from the aggregated gradient; the update and the increment run behind it
            V.grad_finite(g, self.step_ok)
        lr = 0.0
        if self.scheduled:
            kind, p = self.learning_rate.device_spec()
            V.lr_schedule(self.iterations, self._lr_dev, kind, p)
        else:
            lr = self.learning_rate
        clip = ema = None
        if self.clip_modes:
            c = self._clip
            thr = (self.clipvalue or 0.0, self.clipnorm or 0.0, self.global_clipnorm or 0.0)
            V.grad_norm(g, c["seg_start"], c["block_seg"], grad_scale, self.clip_modes, *thr, c["seg_norm"],
                        c["stats"], c["ws"])
            clip = (c["seg_start"], c["block_seg"], self.clip_modes, *thr, c["seg_norm"], c["stats"])
        if self.averaging:
            ema = (self.average, self.average_decay, self.average_start_step, self.dynamic_average_decay)
        adam = (store.flat, g, self.m, self.v, self.iterations, lr, self.beta_1, self.beta_2, self.epsilon, grad_scale)
        if self.skip_nonfinite:
            V.adam_keras_guarded(*adam, self.step_ok, self.skipped, clip=clip, ema=ema, lr_dev=self._lr_dev)
        elif clip and ema:
            V.adam_keras_clipped_ema(*adam, *clip, *ema, lr_dev=self._lr_dev)
        elif clip:
            V.adam_keras_clipped(*adam, *clip, lr_dev=self._lr_dev)
        elif ema:
            V.adam_keras_ema(*adam, *ema, lr_dev=self._lr_dev)
        else:
            V.adam_keras(*adam, lr_dev=self._lr_dev)
        if self.skip_nonfinite:  # `iterations` advances only when the step was applied
            V.counter_add_if(self.iterations, self.step_ok)
        else:
            V.counter_add(self.iterations, 1)

    def _averaged(self, what, store):
        if not self.averaging:
            raise ValueError(f"{what}: the optimizer keeps no average (average_decay=None)")
        if self.average is None:
            self.build(store)
        return self.average

    def assign_average_vars(self, store):
        """tfa's assign_average_vars: the weights become a copy of their average (the average stays)."""
        average = self._averaged("assign_average_vars", store)
        store.flat.copy_(average)

    def swap_weights(self, store):
        """tfa's swap_weights: the weights and their average change places, exactly (vqa_swap_f32; no temporary).
        A second call restores both bitwise."""
        average = self._averaged("swap_weights", store)
        V.swap_f32(store.flat, average)
