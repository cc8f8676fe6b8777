"""Host checks of gradient clipping that need no GPU: the Adam constructor's rules, the variable table, and the
NumPy restatement (tests/clip_ref.py) against hand-computed answers."""
import math

import numpy as np
import pytest

import clip_ref as C
import vqa_lib as V
from vqa_optim import GRAD_STATS, Adam, clip_tables


# ---- Adam constructor
def test_defaults_are_off():
    a = Adam()
    assert a.clipvalue is None and a.clipnorm is None and a.global_clipnorm is None
    assert a.clip_modes == 0


def test_modes():
    assert Adam(clipvalue=0.5).clip_modes == V.CLIP_VALUE
    assert Adam(clipnorm=2).clip_modes == V.CLIP_NORM
    assert Adam(global_clipnorm=1.0).clip_modes == V.CLIP_GLOBAL_NORM
    a = Adam(1e-4, clipvalue=0.5, global_clipnorm=3.0)
    assert a.clip_modes == V.CLIP_VALUE | V.CLIP_GLOBAL_NORM and (a.clipvalue, a.global_clipnorm) == (0.5, 3.0)
    assert Adam(clipvalue=0.5, clipnorm=1.0).clip_modes == V.CLIP_VALUE | V.CLIP_NORM


def test_clipnorm_and_global_clipnorm_together_are_refused():
    with pytest.raises(ValueError, match="both"):
        Adam(clipnorm=1.0, global_clipnorm=1.0)


@pytest.mark.parametrize("name", ["clipvalue", "clipnorm", "global_clipnorm"])
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, math.inf, -math.inf, math.nan, "x"])
def test_threshold_must_be_finite_and_positive(name, bad):
    with pytest.raises(ValueError, match=name):
        Adam(**{name: bad})


def test_unknown_kwargs_are_still_accepted():
    a = Adam(learning_rate=0.01, amsgrad=False, name="Adam", decay=0.0, global_clipnorm=1.0)
    assert a.learning_rate == 0.01 and a.global_clipnorm == 1.0


def test_grad_stats_before_build_or_without_clipping_raises():
    with pytest.raises(RuntimeError):
        Adam().grad_stats()
    assert GRAD_STATS == C.STATS


# ---- the variable table
def test_clip_tables():
    B = V.CLIP_BLOCK
    offs = {"a": (0, (1,)), "b": (4, (513,)), "c": (520, (3, 32, 32)), "d": (3592, (2 * B,)), "e": (3592 + 2 * B, (4,))}
    size = 3592 + 2 * B + 4
    seg, blk = clip_tables(offs, size)
    assert seg.dtype == np.int64 and blk.dtype == np.int32
    assert seg.tolist() == [0, 4, 520, 3592, 3592 + 2 * B]
    assert blk.tolist() == [0, 3, 3]  # element 0 in a, B and 2B in d
    for b, s in enumerate(blk):
        end = seg[s + 1] if s + 1 < len(seg) else size
        assert seg[s] <= b * B < end
    # a variable that starts exactly on a block boundary owns that block
    seg, blk = clip_tables({"a": (0, (B,)), "b": (B, (5,))}, B + 5)
    assert blk.tolist() == [0, 1]


@pytest.mark.parametrize("offs,size", [
    ({}, 10), ({"a": (4, (3,))}, 7), ({"a": (0, (3,)), "b": (3, (3,))}, 6), ({"a": (0, (4,)), "b": (8, (1,))}, 8)])
def test_clip_tables_refuses_a_bad_layout(offs, size):
    with pytest.raises(ValueError):
        clip_tables(offs, size)


# ---- clip_ref against known answers
def test_ref_variable_of_norm_exactly_c():
    u = np.array([3.0, 4.0])  # norm 5
    out, norms, st = C.transform([u], clipnorm=5.0)
    assert norms[0] == 5.0 and st["clipnorm_variables"] == 0
    np.testing.assert_array_equal(out[0], (u * 5.0) / 5.0)
    np.testing.assert_array_equal(out[0], u)
    out, _, st = C.transform([u], clipnorm=2.5)
    np.testing.assert_array_equal(out[0], [1.5, 2.0])
    assert st["clipnorm_variables"] == 1
    out, _, st = C.transform([u], clipnorm=10.0)  # below the threshold: (u * 10) / 10
    np.testing.assert_array_equal(out[0], u)


def test_ref_all_zero_variable_takes_the_norm_0_branch():
    out, norms, st = C.transform([np.zeros(7), np.array([0.0, 2.0])], clipnorm=1.0)
    assert norms.tolist() == [0.0, 2.0]
    np.testing.assert_array_equal(out[0], np.zeros(7))  # (0 * c) / max(0, c): no 0 / 0
    np.testing.assert_array_equal(out[1], [0.0, 1.0])
    assert st["clipnorm_variables"] == 1
    # global: a zero gradient has scale c * min(inf, 1 / c)
    out, _, st = C.transform([np.zeros(3)], global_clipnorm=4.0)
    assert st["global_scale"] == 4.0 * (1.0 / 4.0) and not np.any(out[0])


def test_ref_global_norm_and_scale():
    g = [np.array([3.0]), np.array([0.0, 4.0]), np.array([12.0])]  # global norm 13
    out, norms, st = C.transform(g, global_clipnorm=6.5)
    assert st["global_norm"] == 13.0 and st["clipped_global_norm"] == 13.0
    assert st["global_scale"] == 6.5 * (1.0 / 13.0)
    np.testing.assert_allclose(np.concatenate(out), [1.5, 0.0, 2.0, 6.0], rtol=1e-15)
    assert norms.tolist() == [3.0, 4.0, 12.0]
    out, _, st = C.transform(g, global_clipnorm=26.0)  # below the threshold: c * (1 / c), TF's arithmetic
    assert st["global_scale"] == 26.0 * (1.0 / 26.0)
    # grad_scale applies before the threshold
    _, _, st = C.transform(g, grad_scale=0.5, global_clipnorm=6.5)
    assert st["global_norm"] == 6.5 and st["global_scale"] == 6.5 * (1.0 / 6.5)


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_ref_non_finite_global_norm_gives_nan(bad):
    out, _, st = C.transform([np.array([1.0, bad]), np.array([2.0])], global_clipnorm=1.0)
    assert np.isnan(st["global_scale"])
    assert all(np.all(np.isnan(o)) for o in out)


def test_ref_clipvalue_keeps_a_nan_and_counts_clamped_elements():
    u = np.array([-3.0, -0.5, np.nan, 0.5, 0.25, 7.0, np.inf])
    out, norms, st = C.transform([u], clipvalue=0.5)
    np.testing.assert_array_equal(out[0], [-0.5, -0.5, np.nan, 0.5, 0.25, 0.5, 0.5])
    assert st["clipvalue_elements"] == 3  # -3, 7 and inf; a value equal to the threshold is not clamped
    assert np.isnan(norms[0]) and np.isnan(st["clipped_global_norm"])


def test_ref_order_is_value_then_norm():
    u = [np.array([10.0, 0.0, 0.0, 0.0]), np.array([0.3, 0.4])]
    out, norms, st = C.transform(u, clipvalue=1.0, global_clipnorm=0.5)
    assert st["global_norm"] == math.sqrt(100.25) and st["clipped_global_norm"] == math.sqrt(1.25)
    assert norms.tolist() == [1.0, 0.5] and st["clipvalue_elements"] == 1
    s = 0.5 * (1.0 / math.sqrt(1.25))
    np.testing.assert_array_equal(out[0], np.array([1.0, 0, 0, 0]) * s)
    with pytest.raises(ValueError):
        C.transform(u, clipnorm=1.0, global_clipnorm=1.0)


def test_ref_flat_counts_the_gap_with_the_variable_in_front():
    flat = np.array([3.0, 0, 0, 0, 4.0, 1.0])  # variables at 0 (1 value + gap) and 4
    u, norms, _ = C.transform_flat(flat, [0, 4], clipnorm=1.0)
    assert norms.tolist() == [3.0, math.sqrt(17.0)]
    assert u[:4].tolist() == [1.0, 0, 0, 0]


def test_ref_adam_first_step():
    z = np.zeros(2)
    w, m, v = C.adam_step(np.ones(2), z, z, np.array([0.5, -2.0]), 1, lr=0.1)
    # the betas arrive as float32: 1 - float32(0.9) = 0.10000002, 1 - float32(0.999) = 0.00099998713
    np.testing.assert_allclose(m, (1 - C.hyper(0.9)) * np.array([0.5, -2.0]), rtol=1e-12)
    np.testing.assert_allclose(v, (1 - C.hyper(0.999)) * np.array([0.25, 4.0]), rtol=1e-12)
    np.testing.assert_allclose(m, [0.05, -0.2], rtol=1e-6)
    np.testing.assert_allclose(v, [0.00025, 0.004], rtol=2e-5)
    np.testing.assert_allclose(w, [0.9, 1.1], rtol=1e-5)  # lr * sign(g) up to epsilon
