"""GPU checks of the weight-averaging kernels (vqa_adam_keras_ema, vqa_adam_keras_clipped_ema, vqa_swap_f32).

Sizes: 1 (a single element), 3 (a pure scalar tail), 4095 / 4096 / 4097 (one VQA_CLIP_BLOCK and one either side of it)
and 1048576 + 3 (one element more than 4096 workgroups of 256 lanes cover in a sweep, plus a tail: vqa_adam_keras'
grid-stride loop, which the bitwise comparison runs, goes round a second time). Two more cases send the averaging
kernel itself round twice: the same size on buffers that are only 4-byte aligned (its element-by-element form), and
4 * 1048576 + 7 on aligned ones (its 16-byte form).

The clipped path runs on a variable table whose boundaries are multiples of 4 floats and never of a block: three
variables from 4095 floats up, five at the largest size (fewer where n leaves no room: one at 1 and 3).

w, m and v are compared bitwise with what the entry points without the average leave from the same inputs. The
average is compared, step by step, with tests/ema_ref.py evaluated from the device's own state before the step and its
own new weights, so nothing compounds; the bound is derived there (ema_ref.bound): 4 * 2^-24 * (|a| + |w_new|) per
element. Where d == 0 the average must be the new weights bitwise.
"""
import numpy as np
import pytest
import torch

import ema_ref as E
import vqa_lib as V
from schedules import ExponentialDecay
from vqa_layers import ParamStore
from vqa_optim import Adam, clip_tables

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4095, 4096, 4097, 1048576 + 3]
LR, B1, B2, EPS, GS = 1e-2, 0.9, 0.999, 1e-7, 0.5
BOUNDARIES = (0, 516, 2052, 4100, 70004)  # multiples of 4, none of 4096
CLIPS = {"plain": {}, "value+global": dict(clipvalue=0.8, global_clipnorm=20.0), "clipnorm": dict(clipnorm=5.0)}


def _inputs(n, seed=0):
    """Host fp32 w, g, m, v, a: weights of the size of their updates (so the average sees the step), an average
    that is not the weights."""
    rng = np.random.default_rng(1000 + seed)
    f = lambda s: (rng.standard_normal(n) * s).astype(np.float32)
    return dict(w=f(0.05), g=f(2.0), m=f(0.5), v=np.abs(f(1.0)), a=f(0.05))


class _Dev:
    """One set of device buffers and, for a clipped mode, its variable table and norm pass."""

    def __init__(self, cuda, host, clip, shift=0):
        n = host["w"].size
        self.n, self.clip = n, clip
        for k, x in host.items():
            buf = torch.zeros(n + shift, dtype=torch.float32, device=cuda)
            buf[shift:].copy_(torch.from_numpy(x))
            setattr(self, k, buf[shift:])
        self.step = torch.zeros(1, dtype=torch.int64, device=cuda)
        self.modes = ((V.CLIP_VALUE if "clipvalue" in clip else 0) | (V.CLIP_NORM if "clipnorm" in clip else 0)
                      | (V.CLIP_GLOBAL_NORM if "global_clipnorm" in clip else 0))
        self.thr = (clip.get("clipvalue", 0.0), clip.get("clipnorm", 0.0), clip.get("global_clipnorm", 0.0))
        if self.modes:
            offsets = {str(o): (o, (1,)) for o in BOUNDARIES if o < n}
            seg, block_seg = clip_tables(offsets, n)
            assert len(seg) >= 3 or n < 4095
            self.seg, self.block_seg = torch.from_numpy(seg).to(cuda), torch.from_numpy(block_seg).to(cuda)
            self.seg_norm = torch.zeros(len(seg), dtype=torch.float32, device=cuda)
            self.stats = torch.zeros(V.CLIP_STATS, dtype=torch.float32, device=cuda)
            self.ws = V.workspace(V.grad_norm_workspace(n, len(seg)), cuda)

    def apply(self, avg=None, lr_dev=None):
        """One optimizer step; avg = (decay, start_step, dynamic) takes the averaging entry point."""
        head = (self.w, self.g, self.m, self.v, self.step, LR, B1, B2, EPS, GS)
        if not self.modes:
            if avg is None:
                V.adam_keras(*head, lr_dev=lr_dev)
            else:
                V.adam_keras_ema(*head, self.a, *avg, lr_dev=lr_dev)
        else:
            V.grad_norm(self.g, self.seg, self.block_seg, GS, self.modes, *self.thr, self.seg_norm, self.stats, self.ws)
            tail = (self.seg, self.block_seg, self.modes, *self.thr, self.seg_norm, self.stats)
            if avg is None:
                V.adam_keras_clipped(*head, *tail, lr_dev=lr_dev)
            else:
                V.adam_keras_clipped_ema(*head, *tail, self.a, *avg, lr_dev=lr_dev)
        V.counter_add(self.step, 1)

    def host(self, *names):
        torch.cuda.synchronize()
        return [getattr(self, k).cpu().numpy().copy() for k in names]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check_average(a_dev, a_before, w_new, t, avg, what):
    d, _ = E.decay(t, *avg)
    if d == 0:
        assert np.array_equal(_bits(a_dev), _bits(w_new)), f"{what}: at d == 0 the average is the weights bitwise"
        return
    ref = E.average_step(a_before, w_new, t, *avg)
    err = np.abs(a_dev.astype(np.float64) - ref)
    bound = E.bound(a_before, w_new)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what} step {t}: d {float(d):.6f}, worst error / bound {worst:.3f}")
    assert np.all(err <= bound), (what, t, worst)
    # the check is not blind: the average moved, and it is neither the old average nor the weights
    assert not np.array_equal(a_dev, a_before) and not np.array_equal(a_dev, w_new)


def _run_steps(cuda, n, clip, avg, steps=1, what="", shift=0, sched=None):
    """`steps` steps on the averaging entry point, each checked against the plain entry point (w, m, v bitwise, from
    the same state) and against the reference (the average)."""
    host = _inputs(n)
    dev = _Dev(cuda, host, clip, shift)
    twin = _Dev(cuda, host, clip, shift)
    rng = np.random.default_rng(5)
    lr_dev = torch.zeros(1, dtype=torch.float32, device=cuda) if sched is not None else None
    for t in range(steps):
        if t:
            g = torch.from_numpy((rng.standard_normal(n) * 2.0).astype(np.float32)).to(cuda)
            dev.g.copy_(g)
            twin.g.copy_(g)
        (a_before,) = dev.host("a")
        if sched is not None:
            kind, p = sched.device_spec()
            V.lr_schedule(dev.step, lr_dev, kind, p)
        dev.apply(avg, lr_dev=lr_dev)
        twin.apply(None, lr_dev=lr_dev)
        w, m, v, a = dev.host("w", "m", "v", "a")
        for name, x, y in zip("wmv", (w, m, v), twin.host("w", "m", "v")):
            assert np.array_equal(_bits(x), _bits(y)), f"{what} step {t}: {name} differs from the path without average"
        assert np.array_equal(dev.host("g")[0], twin.host("g")[0])
        _check_average(a, a_before, w, t, avg, what)
    assert int(dev.step.item()) == steps
    return dev


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", list(CLIPS))
def test_w_m_v_bitwise_as_without_average_and_fixed_decay(cuda, n, mode):
    _run_steps(cuda, n, CLIPS[mode], (0.875, 0, False), steps=2, what=f"{mode} n={n}")


@pytest.mark.parametrize("n", [4097, 1048576 + 3])
@pytest.mark.parametrize("mode", ["plain", "clipnorm"])
def test_start_step_tracks_the_weights_then_averages(cuda, n, mode):
    """start_step 2 over steps 0..4: a bitwise copy at steps 0 and 1 (asserted in _check_average), the rule after."""
    avg = (0.99, 2, False)
    assert [float(E.decay(t, *avg)[0]) for t in range(5)] == [0.0, 0.0] + [float(np.float32(0.99))] * 3
    _run_steps(cuda, n, CLIPS[mode], avg, steps=5, what=f"start_step {mode} n={n}")


@pytest.mark.parametrize("n", [4097, 1048576 + 3])
@pytest.mark.parametrize("mode", ["plain", "value+global"])
def test_dynamic_decay(cuda, n, mode):
    """Steps 0..4 with the cap 0.3 reached at step 3: d = 1/10, 2/11, 3/12, then 0.3 twice."""
    avg = (0.3, 0, True)
    ds = [float(E.decay(t, *avg)[0]) for t in range(5)]
    assert ds[0] < ds[1] < ds[2] < ds[3] == ds[4] == float(np.float32(0.3))
    _run_steps(cuda, n, CLIPS[mode], avg, steps=5, what=f"dynamic {mode} n={n}")
    # and started late: n counts from start_step
    _run_steps(cuda, n, CLIPS[mode], (0.3, 1, True), steps=3, what=f"dynamic from 1 {mode} n={n}")


@pytest.mark.parametrize("mode", ["plain", "clipnorm"])
def test_scheduled_learning_rate(cuda, mode):
    """lr_dev: the schedule's device value drives both entry points alike."""
    dev = _run_steps(cuda, 4097, CLIPS[mode], (0.9, 0, False), steps=3, what=f"lr_dev {mode}",
                     sched=ExponentialDecay(0.05, 2, 0.5))
    fixed = _run_steps(cuda, 4097, CLIPS[mode], (0.9, 0, False), steps=3, what=f"fixed {mode}")
    assert not np.array_equal(dev.host("w")[0], fixed.host("w")[0]), "the schedule must have been used"


def test_element_by_element_form_on_unaligned_buffers(cuda):
    """Buffers one float past a 16-byte boundary take the plain averaging kernel's scalar loop, here round twice."""
    dev = _run_steps(cuda, 1048576 + 3, {}, (0.875, 0, False), steps=1, what="unaligned", shift=1)
    assert dev.w.data_ptr() % 16 == 4 and dev.a.data_ptr() % 16 == 4


def test_sixteen_byte_form_goes_round_twice(cuda):
    """More groups of four than 4096 workgroups of 256 lanes hold, and a tail of 3."""
    _run_steps(cuda, 4 * 1048576 + 7, {}, (0.875, 0, False), steps=1, what="two sweeps")


@pytest.mark.parametrize("mode", list(CLIPS))
def test_the_same_step_twice_gives_the_same_bits(cuda, mode):
    outs = []
    for _ in range(2):
        dev = _Dev(cuda, _inputs(1048576 + 3), CLIPS[mode])
        dev.apply((0.3, 0, True))
        dev.apply((0.3, 0, True))
        outs.append(dev.host("w", "m", "v", "a"))
    for x, y in zip(*outs):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_two_swaps_restore_both_buffers(cuda, n, shift):
    rng = np.random.default_rng(n)
    # every bit pattern travels unchanged, NaNs and denormals included
    a0 = torch.from_numpy(rng.integers(0, 2 ** 32, n + shift, dtype=np.uint32).view(np.float32).copy()).to(cuda)
    b0 = torch.from_numpy(rng.integers(0, 2 ** 32, n + shift, dtype=np.uint32).view(np.float32).copy()).to(cuda)
    a, b = a0.clone(), b0.clone()
    av, bv = a[shift:], b[shift:]
    eq = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    V.swap_f32(av, bv)
    assert eq(av, b0[shift:]) and eq(bv, a0[shift:])
    assert eq(a[:shift], a0[:shift]) and eq(b[:shift], b0[:shift])  # nothing before the views
    V.swap_f32(av, bv)
    assert eq(a, a0) and eq(b, b0)


# ---- through vqa_optim.Adam, on tests/test_gpu_clip.py's layout (alignment gaps behind five of its variables)
SHAPES = [("a", (1,)), ("b", (513,)), ("c", (3, 32, 32)), ("d", (5,)), ("e", (70001,)), ("f", (4,)),
          ("g", (2049, 7)), ("h", (2051,))]


def _store(cuda, w0):
    st = ParamStore()
    for name, s in SHAPES:
        st.add(name, s, "zeros")
    st.materialize(cuda)
    st.flat.copy_(torch.from_numpy(w0))
    return st


@pytest.mark.parametrize("mode", list(CLIPS))
def test_adam_with_average_is_adam_without_it_plus_the_average(cuda, mode):
    probe = _store(cuda, np.zeros(90003, np.float32))
    gaps = np.ones(probe.size, bool)
    for o, s in probe.offsets.values():
        gaps[o:o + int(np.prod(s))] = False
    assert probe.size == 90003 and gaps.sum() == 13
    rng = np.random.default_rng(77)
    w0 = np.where(gaps, 0, rng.standard_normal(probe.size) * 0.05).astype(np.float32)
    plain, avgd = _store(cuda, w0), _store(cuda, w0)
    a = Adam(LR, B1, B2, EPS, **CLIPS[mode])
    b = Adam(LR, B1, B2, EPS, **CLIPS[mode], average_decay=0.9, average_start_step=1)
    a.build(plain)
    b.build(avgd)
    assert a.average is None and torch.equal(b.average, avgd.flat) and b.average.data_ptr() != avgd.flat.data_ptr()
    ptr = b.average.data_ptr()
    for t in range(3):
        g = torch.from_numpy(np.where(gaps, 0, rng.standard_normal(probe.size) * 2.0).astype(np.float32)).to(cuda)
        for st, opt in ((plain, a), (avgd, b)):
            st.grad[:st.size].copy_(g)
            opt.apply(st, grad_scale=GS)
        torch.cuda.synchronize()
        assert torch.equal(plain.flat, avgd.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert torch.equal(a.iterations, b.iterations)
        if t == 0:
            assert torch.equal(b.average, avgd.flat)        # below start_step
        else:
            assert not torch.equal(b.average, avgd.flat)
        assert not np.any(b.average.cpu().numpy()[gaps]), "the alignment gaps of the average stay zero"
    assert b.average.data_ptr() == ptr
    # tfa's two methods
    w, avg = avgd.flat.clone(), b.average.clone()
    b.swap_weights(avgd)
    assert torch.equal(avgd.flat, avg) and torch.equal(b.average, w)
    b.swap_weights(avgd)
    assert torch.equal(avgd.flat, w) and torch.equal(b.average, avg)
    b.assign_average_vars(avgd)
    assert torch.equal(avgd.flat, avg) and torch.equal(b.average, avg)
    with pytest.raises(ValueError, match="no average"):
        a.swap_weights(plain)
