"""NumPy restatement of the weights' moving average that the Adam step keeps (not collected by pytest).

tensorflow_addons is not installed; the rule is DESIGN.md's (tfa MovingAverage: TF's assign_moving_average without
zero-debias, start_step and dynamic_decay as in tfa). For one optimizer step, t the optimizer's `iterations` before
the step's increment and w_new the weights the Adam update leaves:

  d = 0                                              if t < start_step
    = min(average_decay, (1 + n) / (10 + n))         if dynamic, n = t - start_step
    = average_decay                                  otherwise
  a = w_new                                          if d == 0 (a copy)
    = a - (a - w_new) * (1 - d)                      otherwise

d and 1 - d are float32, as the kernel forms them: the division and min are correctly rounded, so they reproduce bit
for bit. The update itself is float64. The Adam / clipping half is tests/clip_ref.py's.
"""
import numpy as np

from clip_ref import adam_step, hyper, transform_flat  # noqa: F401  (the Adam and clipping reference, reused)

F = np.float32


def decay(t, average_decay, start_step=0, dynamic=False):
    """(d, 1 - d) of step t, both float32."""
    t, start_step = int(t), int(start_step)
    d = F(average_decay)
    if t < start_step:
        d = F(0)
    elif dynamic:
        n = F(t - start_step)
        d = min(d, (F(1) + n) / (F(10) + n))
    d = F(d)
    return d, F(F(1) - d)


def average_step(a, w_new, t, average_decay, start_step=0, dynamic=False):
    """The average after step t, float64; where d == 0 exactly w_new's values."""
    d, omd = decay(t, average_decay, start_step, dynamic)
    w64 = np.asarray(w_new, np.float64)
    if d == 0:
        return w64.copy()
    a64 = np.asarray(a, np.float64)
    return a64 - (a64 - w64) * np.float64(omd)


def adam_average_step(w, m, v, a, u, t, average_decay, start_step=0, dynamic=False, **adam):
    """One whole step in u's precision for w, m, v (clip_ref.adam_step; t counts from 0 here, as `iterations` does)
    and the average of the new weights."""
    w, m, v = adam_step(w, m, v, u, t + 1, **adam)
    return w, m, v, average_step(a, w, t, average_decay, start_step, dynamic)


def bound(a, w_new):
    """|a_device - a_reference| allowed per element: the update is at most three fp32 roundings (subtract, multiply,
    subtract) and a fourth from the rounded 1 - d, each at most half an ulp, 2^-24 relative, of a quantity bounded
    by |a| + |w_new|."""
    return 4.0 * 2.0 ** -24 * (np.abs(np.asarray(a, np.float64)) + np.abs(np.asarray(w_new, np.float64)))
