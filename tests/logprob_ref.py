"""fp64 restatement of the two log-probabilities of vqa_prior_decode_scored (include/vqa.h), shared by
tests/test_logprob_ref_host.py, tests/test_gpu_decode_logprob.py and tests/test_gpu_sampler_logprob.py.

For a row of fp32 logits lg, the written token tok, the temperature T and the kept count k:
  logp_model = lg[tok] - log sum_v exp(lg[v])
  logp_draw  = lg[tok] / T - log sum_{v in K} exp(lg[v] / T),   -inf when tok is not in K
with K the k largest logits of the row. Bins with equal logits stay in or go out together on the device, so the
count fixes the set: K = {v: lg[v] >= the k-th largest logit}, and no row is undecided. k = 0 (a primed step whose
head was skipped) is not a row of logits at all: both values are 0.0 by convention and the caller checks that.

TOL, the absolute tolerance between the device and this file on the same fp32 logits and the same fp32 T, follows
from the arithmetic written above dec_score_max (vqa_prior_decode.hip): fp32, the row maximum m subtracted first,
plain expf / logf, a correctly rounded division, sums in a fixed order. With a = (lg[tok] - m) / T and |a| <= 32
(the tests assert it of their rows):
  * the exponent of tok: one subtraction and one division, relative 2^-24 each: |a| 2^-23 <= 3.8e-6;
  * the weights: w_v = expf(a_v) is off by at most (|a_v| + 2) 2^-23 relative (its exponent as above, expf within
    2 ulp), so the sum by (E|a_v| + 2) 2^-23 relative with E the mean under the softmax itself; E|a_v| = H - log Z
    <= log bins <= log 2048 = 7.6 (Z >= 1: the top bin weighs exactly 1): <= 1.2e-6 in the logarithm;
  * the additions: at most 8 per thread and 8 levels of the tree, 2^-24 relative each on positive terms: <= 1.0e-6;
    logf within 2 ulp of a result <= log 2048: <= 1.0e-6;
  * the final subtraction rounds a value below 64 once: <= 1.9e-6.
Derived bound: 8.9e-6. TOL = 1e-5 covers it (and is below the 1e-4 the check allows)."""
import numpy as np

TOL = 1e-5
MAX_EXPONENT = 32.0  # the |(lg[tok] - max) / T| up to which TOL holds


def kept_set(row, k):
    """The k largest logits of the row, ties with the k-th included (a boolean mask)."""
    lg = np.asarray(row, np.float32)
    k = int(k)
    if not 1 <= k <= lg.shape[0]:
        raise ValueError(f"kept count {k} outside [1, {lg.shape[0]}]")
    return lg >= np.sort(lg)[-k]


def logprob_fp64(row, tok, temperature, k):
    """One row of fp32 logits -> (logp_model, logp_draw) in fp64, the temperature rounded to fp32 first, as the
    device receives it."""
    lg = np.asarray(row, np.float32).astype(np.float64)
    T = float(np.float32(temperature))
    tok = int(tok)
    m = lg.max()
    logp_model = (lg[tok] - m) - np.log(np.exp(lg - m).sum())
    K = kept_set(row, k)
    if not K[tok]:
        return float(logp_model), -np.inf
    logp_draw = (lg[tok] - m) / T - np.log(np.exp((lg[K] - m) / T).sum())
    return float(logp_model), float(logp_draw)


def exponent(row, tok, temperature):
    """max(|lg[tok] - max|, |lg[tok] - max| / T): the size of the written token's exponent in the two formulas."""
    lg = np.asarray(row, np.float32).astype(np.float64)
    d = abs(lg[int(tok)] - lg.max())
    return float(max(d, d / float(np.float32(temperature))))
