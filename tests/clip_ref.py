"""NumPy restatement of Keras 2.7 OptimizerV2's gradient clipping and of Keras Adam (not collected by pytest).

TensorFlow is not installed; the formulas are restated from its source, unpinned, like the rest of the oracle.
They act on the aggregated gradient u = grad_scale * g in OptimizerV2._transform_gradients' order:

  clipvalue c         u <- min(max(u, -c), c); tf.minimum / tf.maximum propagate a NaN
  clipnorm c          per variable (tf.clip_by_norm): s2 = sum u^2; norm = sqrt(s2) where s2 > 0, else s2 (0, or
                      the NaN); u <- (u * c) / max(norm, c)
  global_clipnorm c   (tf.clip_by_global_norm) norm = sqrt(sum over variables of sum u^2);
                      scale = c * min(1 / norm, 1 / c) where norm is finite, else NaN; u <- u * scale

`dtype` is the arithmetic's precision: float64 is the reference, float32 measures what the formulas themselves
lose in the kernels' number format.
"""
import numpy as np

STATS = ("global_norm", "clipped_global_norm", "global_scale", "clipnorm_variables", "clipvalue_elements")


def _maximum(a, b):
    return np.maximum(a, b)  # NaN-propagating, like tf.maximum


def clip_by_value(u, c):
    return np.minimum(np.maximum(u, -c), c)


def variable_norm(u):
    s2 = np.sum(u * u, dtype=u.dtype)
    return np.sqrt(s2) if s2 > 0 else s2


def clip_by_norm(u, c):
    c = u.dtype.type(c)
    return (u * c) / _maximum(variable_norm(u), c)


def global_norm(us):
    dt = us[0].dtype
    tot = dt.type(0)
    for u in us:
        tot = tot + np.sum(u * u, dtype=dt)
    return np.sqrt(tot)


def global_scale(norm, c):
    c = type(norm)(c)
    if not np.isfinite(norm):
        return type(norm)(np.nan)
    with np.errstate(divide="ignore"):
        return c * min(type(norm)(1) / norm, type(norm)(1) / c)


def transform(grads, grad_scale=1.0, clipvalue=None, clipnorm=None, global_clipnorm=None, dtype=np.float64):
    """grads: one array per variable. Returns (clipped u per variable, per-variable norms after clipvalue,
    statistics dict with the keys of STATS)."""
    if clipnorm is not None and global_clipnorm is not None:
        raise ValueError("clipnorm and global_clipnorm exclude each other")
    dt = np.dtype(dtype)
    us = [np.asarray(g, dt).reshape(-1) * dt.type(grad_scale) for g in grads]
    stats = {"global_norm": global_norm(us), "global_scale": dt.type(1), "clipnorm_variables": 0,
             "clipvalue_elements": 0}
    if clipvalue is not None:
        c = dt.type(clipvalue)
        stats["clipvalue_elements"] = int(sum(np.count_nonzero((u < -c) | (u > c)) for u in us))
        us = [clip_by_value(u, c) for u in us]
    norms = np.array([variable_norm(u) for u in us], dt)
    stats["clipped_global_norm"] = global_norm(us)
    if clipnorm is not None:
        stats["clipnorm_variables"] = int(np.count_nonzero(norms > dt.type(clipnorm)))
        us = [clip_by_norm(u, clipnorm) for u in us]
    if global_clipnorm is not None:
        s = global_scale(stats["clipped_global_norm"], global_clipnorm)
        stats["global_scale"] = s
        us = [u * s for u in us]
    return us, norms, stats


def split(flat, seg_start, n):
    """The variables of a flat buffer: [seg_start[s], seg_start[s + 1]), the last one ending at n (an alignment
    gap, zero in a gradient, counts with the variable in front of it)."""
    ends = list(seg_start[1:]) + [n]
    return [np.asarray(flat[a:e]) for a, e in zip(seg_start, ends)]


def transform_flat(flat_grad, seg_start, grad_scale=1.0, dtype=np.float64, **clip):
    us, norms, stats = transform(split(flat_grad, seg_start, len(flat_grad)), grad_scale, dtype=dtype, **clip)
    return np.concatenate(us), norms, stats


def hyper(x):
    """A hyperparameter as the update receives it: Keras hands ApplyAdam float32 scalars, so 0.999 arrives as
    float32(0.999) and 1 - beta_2 is 0.00099998713, 1.3e-5 away from 0.001. The rounding is part of the input,
    not of the arithmetic under test."""
    return float(np.float32(x))


def adam_step(w, m, v, u, t, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """Keras Adam (TF ApplyAdam) step number t (1-based) on the clipped gradient u, in u's precision; the
    hyperparameters are the float32 values the update receives (hyper)."""
    dt = u.dtype
    one = dt.type(1)
    lr, beta_1, beta_2, epsilon = (dt.type(hyper(x)) for x in (lr, beta_1, beta_2, epsilon))
    alpha = lr * np.sqrt(one - beta_2 ** dt.type(t)) / (one - beta_1 ** dt.type(t))
    m = m + (u - m) * (one - beta_1)
    v = v + (u * u - v) * (one - beta_2)
    w = w - (m * alpha) / (np.sqrt(v) + epsilon)
    return w, m, v
