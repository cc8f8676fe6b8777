"""GPU parity of gradient clipping in Adam (vqa_grad_norm + vqa_adam_keras_clipped through vqa_optim.Adam) against
the fp64 NumPy restatement of TF 2.7's formulas (tests/clip_ref.py).

One synthetic ParamStore, 90,003 floats, holds every layout edge at once: a 1-element variable, a 513-element one
that leaves an alignment gap, a 3x32x32 kernel, 5- and 4-element variables, 70,001 elements (17 blocks of 4096 and
an odd tail), a 2049x7 matrix, and a last variable that ends at `size`, which is no multiple of 4. Gradients are
seeded normal draws, fresh for each of three steps; the 3x32x32 variable is scaled by 100, so per-variable and
global clipping differ.

Bounds: SURVEY.md §8c's fp32 criterion, 1e-5 relative to the largest reference magnitude, for the norms, the scale,
m, v and w. m and v are linear and quadratic in the clipped gradient (w after one Adam step is nearly blind to its
scale: three steps, and small weights, so that the updates are a sizeable part of w). Counts are exact; where a
threshold is set AT a norm, the one variable whose fp64 norm lies within 1e-5 of the threshold may count either
way, because the device's fp32 norm may land on either side of it.
"""
import numpy as np
import pytest
import torch

import clip_ref as C
import vqa_lib as V
from schedules import ExponentialDecay
from vqa_layers import ParamStore
from vqa_optim import Adam

pytestmark = pytest.mark.gpu

SHAPES = [("a", (1,)), ("b", (513,)), ("c", (3, 32, 32)), ("d", (5,)), ("e", (70001,)), ("f", (4,)),
          ("g", (2049, 7)), ("h", (2051,))]
SIZE = 90003
STEPS = 3
TOL = 1e-5
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7


def _layout():
    st = ParamStore()
    for n, s in SHAPES:
        st.add(n, s, "zeros")
    assert st.size == SIZE and SIZE % 4 == 3
    return st


def _flat(rng, scale, boost=None):
    """A flat host buffer in the store's layout: normal draws in the variables, zeros in the gaps."""
    st = _layout()
    out = np.zeros(SIZE, np.float32)
    for n, (o, s) in st.offsets.items():
        k = int(np.prod(s))
        sc = scale * (boost if boost and n == "c" else 1.0)
        out[o:o + k] = rng.standard_normal(k).astype(np.float32) * np.float32(sc)
    return out


_RNG = np.random.default_rng(20261020)
W0 = _flat(_RNG, 0.01)
GRADS = [_flat(_RNG, 1.0, boost=100.0) for _ in range(STEPS)]
SEG = sorted(o for o, _ in _layout().offsets.values())
GAPS = np.ones(SIZE, bool)
for _o, _s in _layout().offsets.values():
    GAPS[_o:_o + int(np.prod(_s))] = False
assert GAPS.sum() == 3 + 3 + 3 + 3 + 1  # behind a, b, d, e and g


def _f32(x):
    return float(np.float32(x))


def _norms0(gs=1.0, clipvalue=None):
    """fp64 per-variable norms and statistics of the first step's gradient."""
    _, norms, st = C.transform_flat(GRADS[0], SEG, grad_scale=gs, clipvalue=clipvalue)
    return norms, st


def _reference(clip, gs=1.0, lrs=None, dtype=np.float64):
    dt = np.dtype(dtype)
    w, m, v = W0.astype(dt), np.zeros(SIZE, dt), np.zeros(SIZE, dt)
    per_step = []
    for t in range(STEPS):
        u, norms, st = C.transform_flat(GRADS[t], SEG, grad_scale=gs, dtype=dt, **clip)
        w, m, v = C.adam_step(w, m, v, u, t + 1, lr=LR if lrs is None else lrs[t], beta_1=B1, beta_2=B2, epsilon=EPS)
        per_step.append((norms, st))
    return w, m, v, per_step


def _device(cuda, clip, gs=1.0, learning_rate=LR):
    st = _layout()
    st.materialize(cuda)
    st.flat.copy_(torch.from_numpy(W0))
    opt = Adam(learning_rate, B1, B2, EPS, **clip)
    opt.build(st)
    per_step = []
    for t in range(STEPS):
        g = torch.from_numpy(GRADS[t]).to(cuda)
        st.grad[:SIZE].copy_(g)
        opt.apply(st, grad_scale=gs)
        assert torch.equal(st.grad[:SIZE], g), "a clipped apply() must leave the gradient buffer as it is"
        if opt.clip_modes:
            per_step.append((opt.variable_grad_norms().cpu().numpy().copy(),
                             {k: float(x) for k, x in opt.grad_stats().items()}))
    torch.cuda.synchronize()
    assert int(opt.iterations.item()) == STEPS
    return st.flat.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy(), per_step


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(float(np.max(np.abs(b))), 1e-30))


def _check(got, ref, clip, what):
    gw, gm, gv, gsteps = got
    rw, rm, rv, rsteps = ref
    for t, ((gn, gst), (rn, rst)) in enumerate(zip(gsteps, rsteps)):
        e = _rel(gn, rn)
        print(f"{what} step {t}: variable norms rel {e:.2e}; stats {gst}")
        assert e < TOL, (what, t, e)
        for k in ("global_norm", "clipped_global_norm", "global_scale"):
            assert abs(gst[k] - rst[k]) <= TOL * abs(rst[k]), (what, t, k, gst[k], rst[k])
        assert gst["clipvalue_elements"] == rst["clipvalue_elements"], (what, t, gst, rst)
        c = clip.get("clipnorm")
        if c is None:
            assert gst["clipnorm_variables"] == 0
        else:
            sure = int(np.count_nonzero(rn > c * (1 + TOL)))
            maybe = int(np.count_nonzero(rn > c * (1 - TOL)))
            assert sure <= gst["clipnorm_variables"] <= maybe, (what, t, gst, sure, maybe)
    for name, g, r in (("m", gm, rm), ("v", gv, rv), ("w", gw, rw)):
        e = _rel(g, r)
        print(f"{what}: {name} rel {e:.2e}")
        assert e < TOL, (what, name, e)
    for name, g in (("w", gw), ("m", gm), ("v", gv)):
        assert not np.any(g[GAPS]), f"{what}: the alignment gaps of {name} must stay zero"


def _thresholds():
    """Per mode: below, at and above the norm the mode looks at (first step's gradient, fp64, rounded to fp32)."""
    norms, st = _norms0()
    gmax = float(np.max(np.abs(GRADS[0])))
    _, st_cv = _norms0(clipvalue=0.5)
    e_norm = norms[SEG.index(_layout().offsets["e"][0])]
    cases = []
    for tag, c in (("below", 0.5), ("at", _f32(gmax)), ("above", 1000.0)):
        cases.append((f"clipvalue-{tag}", dict(clipvalue=c)))
    for tag, c in (("below", 10.0), ("at", _f32(e_norm)), ("above", 1e5)):
        cases.append((f"clipnorm-{tag}", dict(clipnorm=c)))
    for tag, c in (("below", 100.0), ("at", _f32(st["global_norm"])), ("above", 1e5)):
        cases.append((f"global-{tag}", dict(global_clipnorm=c)))
    for tag, c in (("below", 10.0), ("at", _f32(st_cv["clipped_global_norm"])), ("above", 1e4)):
        cases.append((f"value+global-{tag}", dict(clipvalue=0.5, global_clipnorm=c)))
    return cases


CASES = _thresholds()


@pytest.mark.parametrize("what,clip", CASES, ids=[c[0] for c in CASES])
def test_clipped_adam_matches_reference(cuda, what, clip):
    ref = _reference(clip)
    if what.endswith("below"):  # the case is about a clip that bites
        st = ref[3][0][1]
        assert st["clipvalue_elements"] > 0 or st["clipnorm_variables"] > 0 or st["global_scale"] < 0.5
    _check(_device(cuda, clip), ref, clip, what)


def test_clipping_changes_the_moments(cuda):
    """The check above is not blind: the unclipped moments are far from the clipped reference."""
    plain = _device(cuda, {})
    rw, rm, rv, _ = _reference(dict(global_clipnorm=100.0))
    assert _rel(plain[1], rm) > 1.0 and _rel(plain[2], rv) > 1.0


@pytest.mark.parametrize("clip", [dict(clipvalue=0.4), dict(clipnorm=100.0), dict(global_clipnorm=3000.0),
                                  dict(clipvalue=0.4, global_clipnorm=60.0)], ids=["value", "norm", "global", "both"])
def test_threshold_applies_to_the_scaled_gradient(cuda, clip):
    """grad_scale 0.5 (a two-rank sum): every threshold meets 0.5 * g. The global threshold 3000 lies between the
    norm of 0.5 * g (about 2770) and the norm of g, so it must not bite."""
    ref = _reference(clip, gs=0.5)
    if clip == dict(global_clipnorm=3000.0):
        assert ref[3][0][1]["global_norm"] < 3000.0 < 2 * ref[3][0][1]["global_norm"]
    _check(_device(cuda, clip, gs=0.5), ref, clip, f"grad_scale 0.5 {clip}")


def test_scheduled_learning_rate(cuda):
    """lr_dev on the clipped path: a clip that never bites (clipvalue 1e30: u keeps its bits) is bitwise the plain
    path under the same schedule, and a clip that bites matches the reference run at the schedule's rates."""
    sched = ExponentialDecay(0.01, 2, 0.5)
    plain = _device(cuda, {}, learning_rate=sched)
    idle = _device(cuda, dict(clipvalue=1e30), learning_rate=sched)
    for a, b in zip(plain[:3], idle[:3]):
        assert np.array_equal(a, b)
    clip = dict(clipnorm=10.0)
    ref = _reference(clip, lrs=[sched(t) for t in range(STEPS)])
    _check(_device(cuda, clip, learning_rate=sched), ref, clip, "ExponentialDecay + clipnorm")


def test_all_off_is_the_plain_launch_bitwise(cuda):
    st = _layout()
    st.materialize(cuda)
    st.flat.copy_(torch.from_numpy(W0))
    opt = Adam(LR, B1, B2, EPS)
    opt.build(st)
    assert opt.clip_modes == 0 and opt._clip is None
    w, m, v = st.flat.clone(), torch.zeros_like(st.flat), torch.zeros_like(st.flat)
    it = torch.zeros(1, dtype=torch.int64, device=cuda)
    for t in range(STEPS):
        g = torch.from_numpy(GRADS[t]).to(cuda)
        st.grad[:SIZE].copy_(g)
        opt.apply(st, grad_scale=0.5)
        V.adam_keras(w, g.clone(), m, v, it, LR, B1, B2, EPS, 0.5)
        V.counter_add(it, 1)
    torch.cuda.synchronize()
    assert torch.equal(st.flat, w) and torch.equal(opt.m, m) and torch.equal(opt.v, v)
    assert torch.equal(opt.iterations, it)


@pytest.mark.parametrize("clip", [dict(clipvalue=0.5), dict(clipnorm=10.0), dict(global_clipnorm=100.0),
                                  dict(clipvalue=0.5, global_clipnorm=10.0)], ids=["value", "norm", "global", "both"])
def test_two_runs_are_bitwise_identical(cuda, clip):
    a, b = _device(cuda, clip), _device(cuda, clip)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for (na, sa), (nb, sb) in zip(a[3], b[3]):
        assert np.array_equal(na, nb) and sa == sb


def test_nan_element(cuda):
    """clipvalue keeps a NaN a NaN (comparisons, not fminf / fmaxf) and touches nothing else; a non-finite global
    norm gives a NaN scale."""
    st = _layout()
    st.materialize(cuda)
    g = GRADS[0].copy()
    at = st.offsets["e"][0] + 12345
    g[at] = np.nan
    st.grad[:SIZE].copy_(torch.from_numpy(g))
    opt = Adam(LR, B1, B2, EPS, clipvalue=0.5)
    opt.apply(st)
    m = opt.m.cpu().numpy()
    stats = {k: float(x) for k, x in opt.grad_stats().items()}
    assert np.isnan(m[at]) and np.count_nonzero(np.isnan(m)) == 1
    _, _, rst = C.transform_flat(g, SEG, clipvalue=0.5)
    assert stats["clipvalue_elements"] == rst["clipvalue_elements"]
    assert np.isnan(stats["global_norm"]) and np.isnan(stats["clipped_global_norm"])
    opt = Adam(LR, B1, B2, EPS, global_clipnorm=1.0)
    opt.apply(st)
    assert np.isnan(float(opt.grad_stats()["global_scale"]))
    inside = ~GAPS
    assert np.all(np.isnan(opt.m.cpu().numpy()[inside]))
