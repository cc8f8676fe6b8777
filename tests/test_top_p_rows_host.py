"""The model-logit cases of tests/test_gpu_decode_top_p.py leave almost every row decided: on teacher-forced fp64
logits of the oracle (oracle/prior_ref.py) for the same weights, the share of rows with a bin inside the margin
DELTA of the nucleus boundary stays under the cap. Needs no GPU; the fp64 rule itself is checked on rows worked
out by hand."""
import numpy as np
import pytest
import torch

from oracle import prior_ref as P
from top_p_ref import CASES, DELTA, TEMPERATURE, UNCLEAR_CAP, nucleus_fp64

N, CTX, W = 3, 64, 128
_LOGITS = {}


def _logits(bins):
    if bins not in _LOGITS:
        cfg = P.PriorConfig(bins=bins, ctx=CTX, width=W, depth=6, heads=2, blocks=4, attn_stacks=1)
        p = P.to_torch(P.init_params(cfg, 3), torch.float64)
        tok = torch.randint(0, bins, (N, CTX), generator=torch.Generator().manual_seed(17))
        with torch.no_grad():
            _LOGITS[bins] = P.model_forward(p, cfg, tok).numpy().astype(np.float32).reshape(N * CTX, bins)
    return _LOGITS[bins]


def test_delta_is_inside_the_allowed_bound():
    assert 0 < DELTA <= 1e-4


@pytest.mark.parametrize("bins,top_p,top_k", CASES)
def test_unclear_share_of_the_model_logit_cases(bins, top_p, top_k):
    margins = np.array([nucleus_fp64(r, TEMPERATURE, top_k, top_p)[1] for r in _logits(bins)])
    share = float((margins <= DELTA).mean())
    print(f"bins {bins} top_p {top_p} top_k {top_k}: unclear share {share:.4f}, smallest margin {margins.min():.3e}")
    assert share <= UNCLEAR_CAP


def test_the_fp64_rule_on_rows_worked_out_by_hand():
    geo = np.log(0.5 ** np.arange(1, 65)).astype(np.float32)
    assert nucleus_fp64(geo, 1.0, 0, 0.6)[0].sum() == 2
    assert nucleus_fp64(geo, 1.0, 0, 0.8)[0].sum() == 3
    assert nucleus_fp64(geo, 2.0, 0, 0.6)[0].sum() == 3
    assert nucleus_fp64(geo, 1.0, 3, 0.8)[0].sum() == 2
    tie = np.full(64, -80.0, np.float32)
    tie[[5, 9, 20, 33, 40]] = np.log([0.4, 0.2, 0.2, 0.1, 0.1])
    keep = nucleus_fp64(tie, 1.0, 0, 0.5)[0]
    assert sorted(np.flatnonzero(keep)) == [5, 9, 20]
    assert nucleus_fp64(np.full(64, -1.0, np.float32), 1.0, 0, 0.01)[0].all()
