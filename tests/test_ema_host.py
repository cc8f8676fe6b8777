"""Host checks of weight averaging that need no GPU: the NumPy restatement of the rule (tests/ema_ref.py) against
hand-computed answers, and the Adam constructor's rules."""
import math

import numpy as np
import pytest

import ema_ref as E
import vqa_lib as V
from vqa_optim import Adam

F = np.float32


# ---- the reference itself
def test_zero_decay_copies_the_weights_bitwise():
    rng = np.random.default_rng(1)
    a, w = rng.standard_normal(100).astype(F), rng.standard_normal(100).astype(F)
    for kw in (dict(average_decay=0.0), dict(average_decay=0.99, start_step=5)):
        out = E.average_step(a, w, 3, **kw)
        assert out.dtype == np.float64 and np.array_equal(out.astype(F).view(np.uint32), w.view(np.uint32))


def test_fixed_decay_by_hand():
    d, omd = E.decay(7, 0.75)
    assert (d, omd) == (F(0.75), F(0.25)) and d.dtype == F and omd.dtype == F
    assert np.array_equal(E.average_step([4.0, -2.0], [0.0, 2.0], 7, 0.75), [3.0, -1.0])
    # 1 - d is the float32 difference, not the float64 one
    d, omd = E.decay(0, 0.999)
    assert omd == F(1) - F(0.999) and float(omd) != 1.0 - 0.999


def test_dynamic_decay_values_and_cap():
    for n, want in ((0, F(1) / F(10)), (1, F(2) / F(11)), (10, F(11) / F(20))):
        assert E.decay(n, 0.999, dynamic=True)[0] == want
        assert E.decay(n + 4, 0.999, start_step=4, dynamic=True)[0] == want
    assert E.decay(0, 0.999, dynamic=True)[0] == F(0.1)
    assert abs(float(E.decay(1, 0.999, dynamic=True)[0]) - 2 / 11) < 1e-7
    assert E.decay(10, 0.999, dynamic=True)[0] == F(0.55)
    # capped by average_decay: (1 + 10) / (10 + 10) = 0.55 > 0.5, and far out the cap always holds
    assert E.decay(10, 0.5, dynamic=True)[0] == F(0.5)
    assert E.decay(10 ** 6, 0.999, dynamic=True)[0] == F(0.999)
    assert E.decay(3, 0.05, dynamic=True)[0] == F(0.05)


def test_steps_below_start_step_track_the_weights():
    rng = np.random.default_rng(2)
    a = rng.standard_normal(16)
    for t in range(5):
        w = rng.standard_normal(16)
        new = E.average_step(a, w, t, 0.9, start_step=3)
        if t < 3:
            assert E.decay(t, 0.9, start_step=3)[0] == 0 and np.array_equal(new, w)
        else:
            assert E.decay(t, 0.9, start_step=3)[0] == F(0.9) and not np.array_equal(new, w)
            assert np.allclose(new, 0.9 * a + 0.1 * w, rtol=0, atol=1e-6)  # float32(0.9) is 2.4e-8 off 0.9
        a = new


def test_adam_average_step_is_clip_refs_adam_plus_the_average():
    rng = np.random.default_rng(3)
    w, m, v, a, u = (rng.standard_normal(8) for _ in range(5))
    v = np.abs(v)
    w1, m1, v1, a1 = E.adam_average_step(w, m, v, a, u, 2, 0.9, lr=1e-2)
    rw, rm, rv = E.adam_step(w, m, v, u, 3, lr=1e-2)
    assert np.array_equal(w1, rw) and np.array_equal(m1, rm) and np.array_equal(v1, rv)
    assert np.array_equal(a1, E.average_step(a, rw, 2, 0.9))


def test_bound_is_four_half_ulps():
    assert np.array_equal(E.bound([1.0, -2.0], [3.0, 0.5]), 4 * 2.0 ** -24 * np.array([4.0, 2.5]))


# ---- Adam constructor
def test_averaging_is_off_by_default():
    before = Adam().clip_modes, Adam(clipvalue=0.5, global_clipnorm=1.0).clip_modes
    a = Adam(average_decay=None)
    assert not a.averaging and a.average is None and a.average_decay is None
    assert (a.clip_modes, Adam(clipvalue=0.5, global_clipnorm=1.0, average_decay=None).clip_modes) == before
    assert before == (0, V.CLIP_VALUE | V.CLIP_GLOBAL_NORM)


def test_settings_are_kept():
    a = Adam(average_decay=0.999, average_start_step=100, dynamic_average_decay=True)
    assert a.averaging and (a.average_decay, a.average_start_step, a.dynamic_average_decay) == (0.999, 100, True)
    assert a.average is None  # allocated by build()
    b = Adam(average_decay=0, clipnorm=1.0)
    assert b.averaging and b.average_decay == 0.0 and b.average_start_step == 0 and not b.dynamic_average_decay
    assert b.clip_modes == V.CLIP_NORM


@pytest.mark.parametrize("bad", [1, 1.0, 1.5, -0.1, math.inf, -math.inf, math.nan, "x", True])
def test_average_decay_must_be_finite_and_in_range(bad):
    with pytest.raises(ValueError, match="average_decay"):
        Adam(average_decay=bad)


@pytest.mark.parametrize("bad", [-1, 1.5, 2.0, "3", None, True])
def test_average_start_step_must_be_a_non_negative_integer(bad):
    with pytest.raises(ValueError, match="average_start_step"):
        Adam(average_decay=0.9, average_start_step=bad)


@pytest.mark.parametrize("kw", [dict(average_start_step=3), dict(dynamic_average_decay=True),
                                dict(average_start_step=3, dynamic_average_decay=True)])
def test_start_step_or_dynamic_without_a_decay_is_refused(kw):
    with pytest.raises(ValueError, match="need average_decay"):
        Adam(**kw)


def test_a_model_without_an_average_refuses_the_tfa_methods():
    a = Adam()
    for call in (a.assign_average_vars, a.swap_weights):
        with pytest.raises(ValueError, match="no average"):
            call(None)
