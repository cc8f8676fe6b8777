"""fp64 reference of the nucleus (top-p) filter of vqa_prior_decode_filtered (include/vqa.h), shared by
tests/test_gpu_decode_top_p.py and tests/test_top_p_rows_host.py.

DELTA, the margin inside which a row's kept set is not decided between the device and fp64 (a bin v with
|A(lg[v]) - p Z| <= DELTA * Z), follows from the arithmetic written above dec_nucleus_threshold (vqa_prior_decode.hip),
with the same fp32 logits, temperature and p on both sides:
  * the exponent a = (lg - max) / T is one fp32 subtraction and one division: relative error <= 2^-23, so the
    weight exp(a) is off by a factor within 1 +- |a| 2^-23; expf adds at most 1 ulp (2^-23);
  * a weight counts only above 2^-36 (|a| < 24.96), so a counted weight is off by at most (24.96 + 1) 2^-23
    = 3.1e-6 relative; truncation to 36 fractional bits and the weights dropped below 2^-36 add at most
    2^-36 each, 2048 * 2^-36 = 3e-8 in all, relative to Z >= 1 (the top bin weighs exactly 1);
  * the integer sums and the comparison with ceil(p Zq) are exact.
So |A_dev - A| <= 3.2e-6 Z and |p Z_dev - p Z| <= 3.2e-6 Z: the two sides of the comparison move by at most
6.4e-6 Z against each other. DELTA = 1e-5 covers it (and is below the 1e-4 the check allows)."""
import numpy as np

DELTA = 1e-5
UNCLEAR_CAP = 0.05  # at most this share of a case's rows may be undecided
# (bins, top_p, top_k) of the model-logit cases, at this temperature
TEMPERATURE = 0.7
CASES = [(bins, p, k) for bins in (64, 513) for p in (0.5, 0.9) for k in (0, 5)]


def nucleus_fp64(row, temperature, top_k, top_p):
    """One row of fp32 logits -> (keep mask, margin): the bins that take part in the draw by the rule of
    include/vqa.h in fp64 (temperature and top_p rounded to fp32 first, as the device receives them), and
    min over the top-k survivors of |A(lg[v]) - p Z| / Z."""
    lg = np.asarray(row, np.float32).astype(np.float64)
    T, p = float(np.float32(temperature)), float(np.float32(top_p))
    bins = lg.shape[0]
    S = lg >= np.sort(lg)[-top_k] if 0 < top_k < bins else np.ones(bins, bool)
    w = np.where(S, np.exp((lg - lg.max()) / T), 0.0)
    Z = w.sum()
    order = np.argsort(-lg, kind="stable")
    ls, ws = lg[order], w[order]
    csum = np.concatenate([[0.0], np.cumsum(ws)])
    # A(lg[v]): the mass of the bins with a strictly larger logit = csum at the first position holding lg[v]
    first = np.searchsorted(-ls, -lg, side="left")
    A = csum[first]
    keep = S & (A < p * Z)
    margin = float(np.min(np.abs(A[S] - p * Z)) / Z)
    return keep, margin
