"""The fp64 reference of the decode's log-probabilities (tests/logprob_ref.py) on hand-made rows. No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from logprob_ref import MAX_EXPONENT, TOL, exponent, kept_set, logprob_fp64  # noqa: E402


def test_tol_is_within_what_the_check_allows():
    assert 8.9e-6 <= TOL <= 1e-4 and MAX_EXPONENT == 32.0


@pytest.mark.parametrize("bins", [64, 513])
@pytest.mark.parametrize("T", [1.0, 0.7, 2.0])
def test_uniform_row(bins, T):
    """Every bin equal: -log bins under the model and, with every bin kept, under the draw at any temperature."""
    row = np.full(bins, -1.25, np.float32)
    lm, ld = logprob_fp64(row, 7, T, bins)
    assert abs(lm + math.log(bins)) < 1e-12 and abs(ld + math.log(bins)) < 1e-12
    # any smaller count still keeps the whole tie
    assert logprob_fp64(row, 7, T, 1) == (lm, ld)


def test_kept_set_of_one_bin():
    """Only the top bin took part: the draw was certain, the model's value is unchanged by the filter."""
    row = np.log(np.array([0.1, 0.6, 0.2, 0.1])).astype(np.float32)
    lm, ld = logprob_fp64(row, 1, 0.7, 1)
    assert ld == 0.0
    assert abs(lm - math.log(0.6)) < 1e-7  # the row is fp32
    assert logprob_fp64(row, 1, 0.7, 4)[0] == lm


def test_token_outside_the_set():
    row = np.log(np.array([0.1, 0.6, 0.2, 0.1])).astype(np.float32)
    lm, ld = logprob_fp64(row, 2, 1.0, 1)
    assert ld == -np.inf and abs(lm - math.log(0.2)) < 1e-7


def test_ties_stay_together():
    """Masses .4, .2, .2, .1, .1: a count of 2 or 3 is the same set of three bins (the tie at .2 stays whole), a
    count of 4 or 5 all five."""
    row = np.log(np.array([0.4, 0.2, 0.2, 0.1, 0.1])).astype(np.float32)
    assert kept_set(row, 2).tolist() == kept_set(row, 3).tolist() == [True, True, True, False, False]
    assert kept_set(row, 4).all() and kept_set(row, 5).all()
    for k in (2, 3):
        lm, ld = logprob_fp64(row, 2, 1.0, k)
        assert abs(ld - math.log(0.2 / 0.8)) < 1e-7 and abs(lm - math.log(0.2)) < 1e-7
    assert logprob_fp64(row, 4, 1.0, 3)[1] == -np.inf
    lm, ld = logprob_fp64(row, 4, 1.0, 5)
    assert abs(ld - lm) < 1e-15


def test_temperature_sharpens_the_draw_only():
    """T = 0.5 squares the masses: .5, .25, .25 -> 4/6, 1/6, 1/6; the model's value does not move."""
    row = np.log(np.array([0.5, 0.25, 0.25])).astype(np.float32)
    lm, ld = logprob_fp64(row, 0, 0.5, 3)
    assert abs(lm - math.log(0.5)) < 1e-7 and abs(ld - math.log(4.0 / 6.0)) < 1e-6
    assert logprob_fp64(row, 0, 1.0, 3)[0] == lm


def test_filters_off_is_the_models_value():
    rng = np.random.default_rng(3)
    row = rng.normal(size=513).astype(np.float32)
    lm, ld = logprob_fp64(row, 100, 1.0, 513)
    assert lm == ld
    assert abs(lm - (float(row[100]) - math.log(np.exp(row.astype(np.float64)).sum()))) < 1e-12


def test_large_logits_do_not_overflow():
    row = np.array([1000.0, 999.0, -1000.0], np.float32)
    lm, ld = logprob_fp64(row, 1, 1.0, 3)
    assert abs(lm - (-1.0 - math.log1p(math.exp(-1.0)))) < 1e-12 and lm == ld
    assert exponent(row, 1, 0.5) == 2.0 and exponent(row, 2, 1.0) == 2000.0


def test_bad_count_is_refused():
    with pytest.raises(ValueError):
        kept_set(np.zeros(4, np.float32), 0)
    with pytest.raises(ValueError):
        kept_set(np.zeros(4, np.float32), 5)
