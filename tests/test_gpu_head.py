"""Kernel-level parity of the prior's fused head + cross entropy (vqa_prior_head.hip head_fwd_kernel, head_bwd_dx_kernel,
head_bwd_dw_kernel) past the shapes of tests/test_gpu_prior.py: weight-gradient segments of several 64-row chunks
with a ragged last one (M from vqa_head_bwd_plan), M = 1, the vocabulary edges V = 64 and 65, targets at 0 and V - 1,
head_fwd without targets, NaN guard bands on dx, lse and amax.

Bounds: 1e-5 (fp32) / 3e-2 (bf16) of max |ref| (x2 for the loss and the gradients, as test_gpu_prior.py); dW / db over
M rows max(that, 8 * e32) with e32 the fp32 evaluation of the same reference (prior_parity_ref), db at the fp32 figure
in both dtypes (an fp32 sum: prior_parity_ref.HEAD_DB_TOL). Worst observed err / bound (MI355X,
profiles/prior_kernel_parity.txt): 0.15. Inputs: prior_parity_ref.head_inputs (edge rows weighted so that the bf16
bound sees one lost row).
"""
import pytest
import torch

import prior_parity_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
G = 3  # guard rows


def _head_ref(x, w, b, tgt, inv):
    """(lse, row loss, dx, dW, db) of loss = inv * sum(lse - logit[target]) in x's dtype (fp64: the reference)."""
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    logits = x @ w + b
    lse = torch.logsumexp(logits, -1)
    ce = lse - logits.gather(1, tgt[:, None])[:, 0]
    (ce.sum() * inv).backward()
    return lse.detach(), ce.detach(), x.grad, w.grad, b.grad, logits.detach()


def _plan_M(Vb):
    """Smallest M past 1000 whose weight-gradient segments hold >= 2 chunks with a ragged last segment."""
    import vqa_lib as V
    for M in range(1001, 200000, 37):
        segs, seg_rows = V.head_bwd_plan(M, 128, Vb)
        if seg_rows >= 128 and M % seg_rows and M % 64:
            return M, segs, seg_rows
    raise AssertionError("no M found")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,Vb", [(0, 2048), (1, 64), (1, 65), (130, 64), (130, 65), (67, 2048)])
def test_head_edges(cuda, dt, M, Vb):
    import vqa_lib as V
    long_sum = M == 0
    if long_sum:
        M, segs, seg_rows = _plan_M(Vb)
        assert seg_rows >= 128 and segs >= 2
    else:
        assert V.head_bwd_plan(M, 128, Vb) == (-(-M // 64), 64)
    tol = R.HEAD_TOL[dt]
    x, w, b, tgt = R.head_inputs(M, Vb, dt)
    xd = x.cuda()
    wt = torch.empty(Vb, 128, dtype=dt, device="cuda")
    V.head_wt(w.cuda(), wt)
    assert torch.equal(wt.cpu(), w.t().contiguous().to(dt))  # the head computes with W rounded to the dtype
    wr = wt.cpu().t().contiguous()
    inv = 1.0 / M
    lse_r, ce_r, dx_r, dw_r, db_r, logits = _head_ref(x.double(), wr.double(), b.double(), tgt, inv)

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
        return buf, buf[G:G + n]

    lb, lse = guarded(M, torch.float32, NAN)
    ab, amax = guarded(M, torch.int64, -7)
    lr, cr = torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")
    tg, bd = tgt.cuda(), b.cuda()
    V.head_fwd(xd, wt, bd, lse, amax=amax, targets=tg, loss_row=lr, correct=cr)
    lb2, lse2 = guarded(M, torch.float32, NAN)
    ab2, amax2 = guarded(M, torch.int64, -7)
    V.head_fwd(xd, wt, bd, lse2, amax=amax2)   # no targets: the same lse and argmax, no loss
    torch.cuda.synchronize()
    for buf in (lb, lb2):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + M:]).all())
    for buf in (ab, ab2):
        assert bool((buf[:G] == -7).all()) and bool((buf[G + M:] == -7).all())
    assert torch.equal(lse, lse2) and torch.equal(amax, amax2)
    assert R.rel(lse, lse_r) < tol
    top2 = torch.topk(logits, 2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > (1e-3 if dt == torch.float32 else 1e-1)
    assert torch.equal(amax.cpu()[clear], logits.argmax(-1)[clear])
    assert R.rel(lr, ce_r) < 2 * tol
    assert torch.equal(cr.cpu()[clear], (logits.argmax(-1) == tgt).float()[clear])
    # backward
    db_, dx = torch.full(((M + 2 * G), 128), NAN, dtype=dt, device="cuda"), None
    dx = db_[G:G + M]
    dw = torch.full((128, Vb), NAN, device="cuda")
    db = torch.full((Vb,), NAN, device="cuda")
    V.head_bwd(xd, wt, bd, tg, lse, inv, dx, dw, db)
    torch.cuda.synchronize()
    assert bool(torch.isnan(db_[:G]).all()) and bool(torch.isnan(db_[G + M:]).all())
    assert R.rel(dx, dx_r) < 2 * tol
    tw, tb = 2 * tol, R.HEAD_DB_TOL
    ew = eb = 0.0
    if long_sum:
        lo = _head_ref(x.float(), wr.float(), b, tgt, inv)
        ew, eb = R.rel(lo[3], dw_r), R.rel(lo[4], db_r)
        tw, tb = R.bound(tw, ew), R.bound(tb, eb)
    name = f"{str(dt)[6:]} M{M} V{Vb} plan{V.head_bwd_plan(M, 128, Vb)}"
    gw, gb = R.rel(dw, dw_r), R.rel(db, db_r)
    R.record("head", name + " dW", ew, tw, gw)
    R.record("head", name + " db", eb, tb, gb)
    assert gw < tw and gb < tb, (name, gw, tw, gb, tb)
