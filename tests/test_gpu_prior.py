"""GPU parity of the factorized-attention prior (vqa_prior*.hip through the C-ABI) against oracle/prior_ref.py.

Kernel level: the sequence-linear layer (causal 3-tap conv and Dense, data and weight gradients), the three
attention factorizations (forward and backward vs fp64 autograd), the fused head + cross entropy. Model level:
logits of FMHABasedAutoregressiveModel, Prior.train_step (two teacher-forcing passes, gradients, Keras Adam),
the persistent decode kernel (teacher-forced logits and free Gumbel-max sampling vs the reference's full
recompute sampler), bf16 loss agreement and graph replay.
Tolerances: fp32 1e-5 (kernels, relative to max |ref|), 2e-4 end to end; bf16 2e-2.
Every route, tile count and edge of the sequence-linear family, the head and the glue kernels is checked at kernel
level in tests/test_gpu_seqlin.py, tests/test_gpu_head.py and tests/test_gpu_prior_glue.py (host side:
tests/test_prior_parity_host.py).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]

from oracle import prior_ref as P  # noqa: E402
from oracle.vqvae_ref import keras_adam  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = P.PriorConfig(bins=64, ctx=256, width=128, depth=3, heads=2, blocks=4, attn_stacks=1)


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ sequence-linear
@pytest.mark.parametrize("dt,tol", [(torch.float32, 2e-6), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("K,N,taps,T", [(128, 96, 3, 200), (32, 32, 1, 256), (32, 128, 1, 130), (128, 128, 1, 64)])
def test_seqlin_fwd_bwd(cuda, dt, tol, K, N, taps, T):
    import vqa_lib as V
    nseq = 3
    g = _gen(K + N + taps + T)
    x = torch.randn(nseq, T, K, generator=g, dtype=torch.float64)
    w = torch.randn(taps, K, N, generator=g, dtype=torch.float64) / math.sqrt(K * taps)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    r = torch.randn(nseq, T, N, generator=g, dtype=torch.float64)
    xd = x.to(dt).cuda()
    wd, bd = w.float().cuda(), b.float().cuda()
    xr = xd.double().cpu()  # reference on the rounded inputs
    ref = (P.causal_conv(xr, w, b) if taps == 3 else xr @ w[0] + b) + r.to(dt).double()
    y = torch.empty(nseq, T, N, dtype=dt, device="cuda")
    V.seqlin_fwd(xd, wd if taps == 3 else wd[0], bd, y, T, taps=taps, dir=-1, residual=r.to(dt).cuda())
    torch.cuda.synchronize()
    assert _rel(y, ref) < tol
    # data gradient (transposed weights, +shift) and weight gradient vs autograd
    xa = xr.clone().requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    ba = b.clone().requires_grad_(True)
    ya = P.causal_conv(xa, wa, ba) if taps == 3 else xa @ wa[0] + ba
    dy = torch.randn(nseq, T, N, generator=g, dtype=torch.float64).to(dt)
    ya.backward(dy.double())
    dyd = dy.cuda()
    dx = torch.empty(nseq, T, K, dtype=dt, device="cuda")
    V.seqlin_fwd(dyd, wd if taps == 3 else wd[0], None, dx, T, taps=taps, dir=1, wtrans=True)
    dw = torch.empty(taps, K, N, device="cuda")
    db = torch.empty(N, device="cuda")
    V.seqlin_wgrad(xd, dyd, dw if taps == 3 else dw[0], db, T, taps=taps)
    torch.cuda.synchronize()
    assert _rel(dx, xa.grad) < tol
    assert _rel(dw, wa.grad) < tol and _rel(db, ba.grad) < tol


def test_seqlin_column_slices(cuda):
    """q/k/v dense on column slices of the qkv tensor (row stride 96) and outputs into column slices."""
    import vqa_lib as V
    g = _gen(5)
    qkv = torch.randn(2, 128, 96, generator=g).cuda()
    w = (torch.randn(32, 32, generator=g) / 6).cuda()
    out = torch.zeros(2, 128, 96, device="cuda")
    V.seqlin_fwd(qkv[..., 32:64], w, None, out[..., 64:96], 128)
    torch.cuda.synchronize()
    ref = qkv[..., 32:64].double().cpu() @ w.double().cpu()
    assert _rel(out[..., 64:96], ref) < 2e-6 and float(out[..., :64].abs().max()) == 0.0


@pytest.mark.parametrize("K,N,taps,dir,T,res", [(128, 96, 3, -1, 200, False), (96, 128, 3, 1, 200, False),
                                                (32, 32, 1, -1, 136, False), (32, 128, 1, -1, 130, True),
                                                (128, 128, 1, -1, 130, True), (128, 32, 1, -1, 64, False)])
def test_seqlin_prepped_and_fused_layernorm(cuda, K, N, taps, dir, T, res):
    """Prepared-weight form (seqlin_d: 1-tap LDS epilogue, 8-wave launches for N >= 96) on ragged T vs fp64, and
    the LayerNorm-fused form (vqa_seqlin_fwd_ln_prepped, K = 128) BIT-identical to layernorm_fwd + the prepped
    launch; fp32 activations are refused by the fused form."""
    import vqa_lib as V
    dt, nseq = torch.bfloat16, 3
    g = _gen(K * N + taps + T)
    x = (torch.randn(nseq, T, K, generator=g) * 1.5 + 0.3).to(dt).cuda()
    w = (torch.randn(taps, K, N, generator=g) / math.sqrt(K * taps)).cuda()
    b = torch.randn(N, generator=g).cuda()
    r = torch.randn(nseq, T, N, generator=g).to(dt).cuda() if res else None
    wp = torch.empty(taps, N, K, dtype=dt, device="cuda")
    V.seqlin_prep([(w, wp, taps, K, N, False)], dt)
    y = torch.empty(nseq, T, N, dtype=dt, device="cuda")
    V.seqlin_fwd_prepped(x, wp, b, y, T, taps=taps, dir=dir, residual=r)
    torch.cuda.synchronize()
    xr, wr = x.double().cpu(), w.double().cpu()
    if taps == 3:
        # dir -1: rows t-2, t-1, t (causal conv); dir +1: rows t+2, t+1, t with the same tap weights
        ref = P.causal_conv(xr, wr, b.double().cpu()) if dir == -1 else \
            P.causal_conv(xr.flip(1), wr, b.double().cpu()).flip(1)
    else:
        ref = xr @ wr[0] + b.double().cpu()
    if res:
        ref = ref + r.double().cpu()
    assert _rel(y, ref) < 2e-2
    if K != 128:
        return
    gm = (1.0 + 0.2 * torch.randn(K, generator=g)).cuda()
    bt = (0.1 * torch.randn(K, generator=g)).cuda()
    a = torch.empty_like(x)
    V.layernorm_fwd(x, gm, bt, a, 1e-6)
    y0 = torch.empty_like(y)
    V.seqlin_fwd_prepped(a, wp, b, y0, T, taps=taps, dir=dir, residual=r)
    y1 = torch.full_like(y, float("nan"))
    V.seqlin_fwd_ln_prepped(x, gm, bt, 1e-6, wp, b, y1, T, taps=taps, dir=dir, residual=r)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    with pytest.raises(Exception):
        V.seqlin_fwd_ln_prepped(x.float(), gm, bt, 1e-6, wp, b, y1.float(), T, taps=taps, dir=dir)


# ------------------------------------------------------------------ attention
def _attn_ref(q, k, v, mode, l, H, vbias):
    """Core of keras MultiHeadAttention on projected heads (N, T, H*16), by the oracle's factorizations with
    identity projections."""
    N, T, C = q.shape
    hd = C // H
    p = {}
    pre = "m"
    for n in ("query", "key", "value"):
        p[f"{pre}/{n}/kernel"] = torch.eye(C, dtype=q.dtype).reshape(C, H, hd)
        p[f"{pre}/{n}/bias"] = torch.zeros(H, hd, dtype=q.dtype)
    p[f"{pre}/out/kernel"] = torch.eye(C, dtype=q.dtype).reshape(H, hd, C)
    p[f"{pre}/out/bias"] = torch.zeros(C, dtype=q.dtype)
    if mode == 2:
        # the zero block's keys/values are the dense biases of a zero input (key bias 0, value bias vbias):
        # block 0's output is vbias; real rows carry no bias under identity projections
        o = P.ATTN[2](p, pre, q, k, v, l)
        o[:, :l] = vbias.to(q.dtype)
        return o
    return P.ATTN[mode](p, pre, q, k, v, l)


@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-5), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_attention_fwd_bwd(cuda, dt, tol, mode):
    import vqa_lib as V
    N, T, H, l = 2, 256, 2, 64
    g = _gen(11 + mode)
    q, k, v = (torch.randn(N, T, 32, generator=g, dtype=torch.float64) for _ in range(3))
    vb = torch.randn(32, generator=g, dtype=torch.float64)
    qd, kd, vd = (t.to(dt).cuda() for t in (q, k, v))
    qr, kr, vr = (t.double().cpu().requires_grad_(True) for t in (qd, kd, vd))
    ref = _attn_ref(qr, kr, vr, mode, l, H, vb)
    o = torch.empty_like(qd)
    lse = torch.empty(N, T, H, device="cuda")
    V.attn_fwd(qd, kd, vd, o, lse, mode, l, H, 0.25, vbias=vb.float().cuda())
    torch.cuda.synchronize()
    assert _rel(o, ref) < tol
    do = torch.randn(N, T, 32, generator=g, dtype=torch.float64).to(dt)
    ref.backward(do.double())
    dq, dk, dv = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(qd)
    dsum = torch.empty(N, T, H, device="cuda")
    V.attn_bwd(qd, kd, vd, o, lse, do.cuda(), dsum, dq, dk, dv, mode, l, H, 0.25)
    torch.cuda.synchronize()
    assert _rel(dq, qr.grad) < tol * 4
    assert _rel(dk, kr.grad) < tol * 4
    assert _rel(dv, vr.grad) < tol * 4


# ------------------------------------------------------------------ head + cross entropy
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-5), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("M,Vb", [(300, 64), (256, 2048), (130, 17)])
def test_head_fused_cross_entropy(cuda, dt, tol, M, Vb):
    import vqa_lib as V
    g = _gen(M + Vb)
    x = torch.randn(M, 128, generator=g, dtype=torch.float64)
    w = torch.randn(128, Vb, generator=g, dtype=torch.float64) / 8
    b = torch.randn(Vb, generator=g, dtype=torch.float64)
    tgt = torch.randint(0, Vb, (M,), generator=g)
    xd = x.to(dt).cuda()
    xr = xd.double().cpu().requires_grad_(True)
    wt = torch.empty(Vb, 128, dtype=dt, device="cuda")
    V.head_wt(w.float().cuda(), wt)
    # the head computes with W rounded to the activation dtype
    wr = wt.double().cpu().t().contiguous().requires_grad_(True)
    br = b.float().double().requires_grad_(True)
    logits = xr @ wr + br
    lse = torch.empty(M, device="cuda")
    amax = torch.empty(M, dtype=torch.int64, device="cuda")
    lr, cr = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    tg = tgt.cuda()
    V.head_fwd(xd, wt, b.float().cuda(), lse, amax=amax, targets=tg, loss_row=lr, correct=cr)
    torch.cuda.synchronize()
    ref_lse = torch.logsumexp(logits.detach(), -1)
    assert _rel(lse, ref_lse) < tol
    top2 = torch.topk(logits.detach(), 2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(amax.cpu()[clear], logits.detach().argmax(-1)[clear])
    ce = ref_lse - logits.detach().gather(1, tgt[:, None])[:, 0]
    assert _rel(lr, ce) < tol * 2
    loss = (torch.logsumexp(logits, -1) - logits.gather(1, tgt[:, None])[:, 0]).mean()
    loss.backward()
    dx = torch.empty_like(xd)
    dw = torch.empty(128, Vb, device="cuda")
    db = torch.empty(Vb, device="cuda")
    V.head_bwd(xd, wt, b.float().cuda(), tg, lse, 1.0 / M, dx, dw, db)
    torch.cuda.synchronize()
    assert _rel(dx, xr.grad) < tol * 2
    assert _rel(dw, wr.grad) < tol * 2 and _rel(db, br.grad) < tol * 2


# ------------------------------------------------------------------ model level
def _model(cfg, dtype="fp32", seed=3, rate=0.0):
    from prior import FMHABasedAutoregressiveModel
    m = FMHABasedAutoregressiveModel(cfg.bins, cfg.width, cfg.depth, cfg.blocks, heads=cfg.heads,
                                     attn_stacks=cfg.attn_stacks, drop_out_rate=rate, context_length=(cfg.ctx,),
                                     levels=1, level=0, dtype=dtype, device="cuda", seed=seed)
    vals = P.init_params(cfg, seed)
    m.store.set_values(vals)
    return m, P.to_torch(vals)


def test_model_logits_match_oracle(cuda):
    m, p = _model(CFG)
    tok = torch.randint(0, CFG.bins, (2, CFG.ctx), generator=_gen(1))
    logits, _ = m(tok)
    torch.cuda.synchronize()
    ref = P.model_forward(p, CFG, tok)
    assert _rel(logits, ref) < 2e-5


def _prior(cfg, dtype="fp32", seed=3):
    from prior import Prior
    pr = Prior(0, [(cfg.ctx,)], cfg.bins, [3], [2], None,
               dict(width=cfg.width, depth=cfg.depth, heads=cfg.heads, blocks=cfg.blocks, attn_stacks=cfg.attn_stacks,
                    drop_out_rate=0.0), None, dtype=dtype, device="cuda", seed=seed)
    vals = P.init_params(cfg, seed)
    pr.prior.store.set_values(vals)
    return pr, vals


def test_train_step_matches_oracle(cuda):
    pr, vals = _prior(CFG)
    g = _gen(7)
    codes = torch.randint(0, CFG.bins - 1, (2, CFG.ctx), generator=g)
    mask = torch.rand(2, CFG.ctx, generator=g) < 0.2
    p = P.to_torch(vals)
    loss, acc, grads, bi = P.train_step_grads(p, CFG, codes, mask)
    res = pr.train_step(codes.cuda(), tf_mask=mask.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pr._last_batch_input.cpu(), bi)  # pass-1 argmax + mixing (exact)
    assert abs(float(res["loss"]) - loss) <= 1e-5 * abs(loss)
    assert abs(float(res["accuracy"]) - acc) <= 1.0 / codes.numel() + 1e-7
    got = pr.prior.store.grads()
    # the key biases' gradients are analytically zero (softmax is shift-invariant per query): errors are
    # measured against max(|grad of that tensor|, 1e-4 * the largest gradient of the model)
    gmax = max(float(g.abs().max()) for g in grads.values())
    errs = {k: float((torch.from_numpy(got[k]).double() - grads[k].double()).abs().max()) /
            max(float(grads[k].abs().max()), 1e-4 * gmax) for k in grads}
    worst = max(errs, key=errs.get)
    assert errs[worst] < 2e-4, (worst, errs[worst])
    # Keras Adam on the product's own gradients
    for k in ("prior/layer0/qkv/kernel", "prior/out/kernel", "prior/x_embedding/embeddings"):
        w1 = keras_adam(torch.from_numpy(vals[k]).double(), torch.from_numpy(got[k]).double(),
                        torch.zeros(vals[k].shape, dtype=torch.float64), torch.zeros(vals[k].shape, dtype=torch.float64),
                        1)[0]
        assert _rel(pr.prior.store.values()[k], w1) < 1e-6
    assert abs(float(res["perplexity(per word)"]) - math.exp(float(res["loss"]))) < 1e-4


def test_train_step_bf16_tracks_oracle(cuda):
    pr, vals = _prior(CFG, dtype="bf16")
    codes = torch.randint(0, CFG.bins - 1, (2, CFG.ctx), generator=_gen(9))
    mask = torch.zeros(2, CFG.ctx, dtype=torch.bool)
    loss, acc, _, _ = P.train_step_grads(P.to_torch(vals), CFG, codes, mask)
    res = pr.train_step(codes.cuda(), tf_mask=mask.cuda())
    assert abs(float(res["loss"]) - loss) <= 2e-2 * abs(loss)


def test_train_step_graph_replay_matches_eager(cuda):
    a, vals = _prior(CFG)
    b, _ = _prior(CFG)
    codes = torch.randint(0, CFG.bins - 1, (2, CFG.ctx), generator=_gen(4)).cuda()
    for _ in range(3):
        a.train_step(codes)
    b.capture_train_step(codes, warmup=1)
    b.train_step(codes)
    b.train_step(codes)
    torch.cuda.synchronize()
    assert torch.equal(a.prior.store.flat, b.prior.store.flat)
    assert float(a.results()["loss"]) == float(b.results()["loss"])
    # a teacher-forcing rate other than the captured one (a schedule) runs eagerly, with that rate
    a.train_step(codes, teacher_force_rate=0.7)
    b.train_step(codes, teacher_force_rate=0.7)
    torch.cuda.synchronize()
    assert torch.equal(a.prior.store.flat, b.prior.store.flat)
    assert torch.equal(a._last_batch_input, b._last_batch_input)


def test_decode_teacher_forced_logits_match_oracle(cuda):
    m, p = _model(CFG)
    L = 150  # crosses two block boundaries (l = 64)
    tok = torch.randint(0, CFG.bins, (2, L + 1), generator=_gen(12))
    tok[:, 0] = CFG.bins - 1
    out, logits = m.sample(2, max_length=L, forced=tok.cuda(), return_logits=True, seed=5)
    torch.cuda.synchronize()
    ref = P.model_forward(p, CFG, tok[:, :L])
    assert _rel(logits, ref) < 2e-5


def test_decode_sampling_matches_reference_sampler(cuda):
    """Free Gumbel-max sampling: the KV-cache decode reproduces the reference's full-recompute sampler token
    for token while the top-2 margin of logits + G stays clear of fp32 rounding."""
    m, p = _model(CFG)
    L, seed = 40, 21
    out = m.sample(2, max_length=L, seed=seed).cpu()
    ref, margins = P.sample_full_recompute(p, CFG, 2, L, seed)
    for n in range(2):
        for i in range(L):
            if margins[n, i] < 1e-3:
                break  # past a near tie the sequences may legitimately diverge
            assert int(out[n, i + 1]) == int(ref[n, i + 1]), (n, i)
    assert (out[:, 0] == CFG.bins - 1).all()


def test_prior_test_step_and_metrics(cuda):
    """prior.py:337-372: test_step feeds the batch's loss / accuracy into the trackers and returns their running
    means (a keras evaluate loop over several batches reports the mean of the batches)."""
    pr, vals = _prior(CFG)
    g = _gen(2)
    batches = [torch.randint(0, CFG.bins - 1, (2, CFG.ctx), generator=g) for _ in range(2)]
    want = [P.train_step_grads(P.to_torch(vals), CFG, c, torch.zeros(2, CFG.ctx, dtype=torch.bool))[:2] for c in batches]
    r1 = {k: float(v) for k, v in pr.test_step(batches[0].cuda()).items()}
    r2 = {k: float(v) for k, v in pr.test_step(batches[1].cuda()).items()}
    assert abs(r1["loss"] - want[0][0]) <= 1e-5 * want[0][0] and abs(r1["accuracy"] - want[0][1]) <= 1e-6
    mean_loss = (want[0][0] + want[1][0]) / 2
    assert abs(r2["loss"] - mean_loss) <= 1e-5 * mean_loss
    assert abs(r2["accuracy"] - (want[0][1] + want[1][1]) / 2) <= 1e-6
    assert abs(r2["perplexity(per word)"] - math.exp(r2["loss"])) <= 1e-4 * math.exp(r2["loss"])
    for t in pr.metrics:
        t.reset_state()
    codes = batches[0].cuda()
    pr.train_step(codes)
    names = [t.name for t in pr.metrics]
    assert names == ["train_loss", "train_accuracy"]
    for t in pr.metrics:
        t.reset_state()
    assert float(pr.train_loss_tracker.result()) == 0.0


def test_prior_evaluate_keras_semantics(cuda):
    """Prior.evaluate (keras Model.evaluate, as src/callback/monitors.py:81 calls it on the validation dataset):
    the trackers are reset, test_step runs on every batch (prior.py:337-372), and the running means over the
    batches come back — as a dict, or flattened in keras order (tracker names first; these keys are not tracker
    names, so sorted: accuracy, loss, perplexity)."""
    pr, vals = _prior(CFG)
    g = _gen(31)
    batches = [torch.randint(0, CFG.bins - 1, (2, CFG.ctx), generator=g) for _ in range(3)]
    want = [P.train_step_grads(P.to_torch(vals), CFG, c, torch.zeros(2, CFG.ctx, dtype=torch.bool))[:2] for c in batches]
    pr.test_step(batches[2].cuda())  # stale tracker state that evaluate must reset
    logs = pr.evaluate([b.cuda() for b in batches[:2]], return_dict=True)
    mean_loss, mean_acc = (want[0][0] + want[1][0]) / 2, (want[0][1] + want[1][1]) / 2
    assert abs(logs["loss"] - mean_loss) <= 1e-5 * mean_loss and abs(logs["accuracy"] - mean_acc) <= 1e-6
    flat = pr.evaluate(torch.cat([b for b in batches[:2]]).cuda(), batch_size=2)
    assert flat == [logs["accuracy"], logs["loss"], logs["perplexity(per word)"]]
    one = pr.evaluate([b.cuda() for b in batches], steps=1, return_dict=True)
    assert abs(one["loss"] - want[0][0]) <= 1e-5 * want[0][0]


# ------------------------------------------------------------------ dropout, conditioning
def test_dropout_mask_statistics_and_determinism(cuda):
    """keras Dropout(rate): kept elements scaled by 1/(1-rate), drop fraction = rate; counter-based mask:
    the same (seed, salt, counter) gives the same mask, another counter a different one."""
    import vqa_lib as V
    rate = 0.1
    x = torch.ones(1 << 20, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    a = x.clone()
    V.dropout_(a, rate, 7, 3, ctr)
    b = x.clone()
    V.dropout_(b, rate, 7, 3, ctr)
    ctr += 1
    c = x.clone()
    V.dropout_(c, rate, 7, 3, ctr)
    torch.cuda.synchronize()
    frac = float((a == 0).float().mean())
    assert abs(frac - rate) < 3e-3
    assert torch.equal(a[a != 0], torch.full_like(a[a != 0], 1.0 / (1.0 - rate)))
    assert torch.equal(a, b) and not torch.equal(a, c)
    # data parallel: a shard dropped with its global element offset is that slice of the full tensor's mask
    h = x.numel() // 2
    shard = x[h:].clone()
    V.dropout_(shard, rate, 7, 3, ctr, elem_offset=h)
    torch.cuda.synchronize()
    assert torch.equal(shard, c[h:])
    # the embedding's dropout: same statistics on (table row * scale + pos), and the same offset rule
    tok = torch.zeros(4, 4096, dtype=torch.int64, device="cuda")
    table = torch.ones(8, 128, device="cuda")
    pos = torch.zeros(4096, 128, device="cuda")
    out = torch.empty(4, 4096, 128, device="cuda")
    V.prior_embed_fwd(table, pos, tok, out, 1.0, rate=rate, seed=5)
    out2 = torch.empty(2, 4096, 128, device="cuda")
    V.prior_embed_fwd(table, pos, tok[2:].contiguous(), out2, 1.0, rate=rate, seed=5, elem_offset=2 * 4096 * 128)
    torch.cuda.synchronize()
    assert abs(float((out == 0).float().mean()) - rate) < 3e-3
    assert torch.equal(out2, out[2:])


def test_conditioning_shapes_are_checked(cuda):
    """autoregressive_fmha.py:145-148 asserts x_cond is [n_samples, max_length, d_model]: the wrappers refuse any
    x_cond / y_cond / forced that the kernels would read past (batch mismatch, too few positions, wrong width)
    with ValueError before a pointer reaches the device."""
    m, _ = _model(CFG)
    tok = torch.randint(0, CFG.bins, (2, CFG.ctx), generator=_gen(3))
    W = CFG.width
    bad_x = [torch.zeros(3, CFG.ctx, W), torch.zeros(2, CFG.ctx - 1, W), torch.zeros(2, CFG.ctx, W // 2)]
    for xc in bad_x:
        with pytest.raises(ValueError):
            m(tok, x_cond=xc.cuda())
    for yc in (torch.zeros(3, W), torch.zeros(2, W + 1)):
        with pytest.raises(ValueError):
            m(tok, y_cond=yc.cuda())
    L = 40
    for xc in (torch.zeros(3, CFG.ctx, W), torch.zeros(2, L - 1, W), torch.zeros(2, CFG.ctx, W - 4)):
        with pytest.raises(ValueError):
            m.sample(2, max_length=L, x_cond=xc.cuda())
    with pytest.raises(ValueError):
        m.sample(2, max_length=L, y_cond=torch.zeros(1, W).cuda())
    for forced in (torch.zeros(2, L, dtype=torch.int64), torch.zeros(1, L + 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            m.sample(2, max_length=L, forced=forced.cuda())
    with pytest.raises(ValueError):
        m.sample(2, max_length=CFG.ctx + 1)
    # the accepted forms still run: x_cond longer than the window is cut to it
    m.sample(2, max_length=L, x_cond=torch.zeros(2, CFG.ctx, W).cuda(), y_cond=torch.zeros(2, 1, W).cuda())
    m(tok, x_cond=torch.zeros(2, CFG.ctx, W).cuda())
    torch.cuda.synchronize()


def test_conditioned_logits_and_decode_match_oracle(cuda):
    """x_cond (an up-sampled upper level, autoregressive_fmha.py:142-151) and y_cond (a label embedding that
    replaces position 0, :120-129): the model's logits and the decode kernel's teacher-forced logits vs the
    oracle."""
    m, p = _model(CFG)
    g = _gen(31)
    tok = torch.randint(0, CFG.bins, (2, CFG.ctx), generator=g)
    tok[:, 0] = CFG.bins - 1
    xc = torch.randn(2, CFG.ctx, CFG.width, generator=g) * 0.5
    yc = torch.randn(2, CFG.width, generator=g) * 0.05
    logits, _ = m(tok, x_cond=xc.cuda(), y_cond=yc.cuda())
    ref = P.model_forward(p, CFG, tok, y_cond=yc.double()[:, None, :], x_cond=xc.double())
    assert _rel(logits, ref) < 2e-5
    L = 100
    _, dl = m.sample(2, max_length=L, x_cond=xc.cuda(), y_cond=yc.cuda(), forced=tok[:, :L + 1].cuda(),
                     return_logits=True, seed=1)
    torch.cuda.synchronize()
    ref = P.model_forward(p, CFG, tok[:, :L], y_cond=yc.double()[:, None, :], x_cond=xc.double())
    assert _rel(dl, ref) < 2e-5


def test_upsampler_train_step_with_conditioner_matches_oracle(cuda):
    """The upsampler prior (level 0 of 2, ConditionerNet on the level-1 codes, Sampler.py:25): one train step
    vs the oracle (conditioner_ref + prior_ref, fp64 autograd through both)."""
    from oracle import conditioner_ref as C
    from prior import Prior
    cfg = P.PriorConfig(bins=64, ctx=256, width=128, depth=3, heads=2, blocks=4, attn_stacks=1)
    ck = dict(dilation_factor=3, dilation_cycle=4, residual_width=32, residual_depth=8)
    pr = Prior(0, [(cfg.ctx,), (cfg.ctx // 4,)], cfg.bins, [3, 2], [2, 2], None,
               dict(width=128, depth=3, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.0), ck, dtype="fp32",
               device="cuda", seed=5)
    vals = pr.prior.store.values()
    g = _gen(8)
    codes = torch.randint(0, cfg.bins - 1, (2, cfg.ctx), generator=g)
    upper = torch.randint(0, cfg.bins - 1, (2, cfg.ctx // 4), generator=g)
    mask = torch.rand(2, cfg.ctx, generator=g) < 0.2
    pt = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in vals.items()}

    def xcond():
        return C.conditioner_forward(pt, upper, "prior/conditioner", 2, 2, 8, 3, dilation_cycle=4)

    start = cfg.bins - 1
    latent = P.shift_right(codes, start)
    with torch.no_grad():
        pred = P.shift_right(P.argmax_lowest(P.model_forward(pt, cfg, latent, x_cond=xcond())), start)
    bi = torch.where(mask, pred, latent)
    loss = P.ce_loss(codes, P.model_forward(pt, cfg, bi, x_cond=xcond()))
    loss.backward()
    res = pr.train_step((codes.cuda(), upper.cuda()), tf_mask=mask.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pr._last_batch_input.cpu(), bi)
    loss = float(loss.detach())
    assert abs(float(res["loss"]) - loss) <= 1e-5 * abs(loss)
    got = pr.prior.store.grads()
    gmax = max(float(t.grad.abs().max()) for t in pt.values() if t.grad is not None)
    for k, t in pt.items():
        ref = t.grad if t.grad is not None else torch.zeros_like(t)
        err = float((torch.from_numpy(got[k]).double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax)
        assert err < 5e-4, (k, err)


# ------------------------------------------------------------------ dropout and label conditioning in training
def _dropout_masks(pr, N, T, seed_pass, ctr):
    """The product's dropout multipliers for one pass (embedding: salt VQA_EMB_DROPOUT_SALT over (N, T, W); layer i:
    salt 1000 + i over the attention output), read back by dropping out a tensor of ones."""
    import vqa_lib as V
    m = pr.prior
    out = {}
    ones = torch.ones(N, T, m.d_model, device="cuda")
    e = ones.clone()
    V.dropout_(e, m.rate, seed_pass, V.EMB_DROPOUT_SALT, ctr)
    out["emb"] = e.double().cpu()
    for i in range(m.depth):
        t = ones.clone()
        V.dropout_(t, m.rate, seed_pass, 1000 + i, ctr)
        out[f"layer{i}"] = t.double().cpu()
    return out


def _grad_errs(got, grads):
    gmax = max(float(g.abs().max()) for g in grads.values())
    errs = {k: float((torch.from_numpy(got[k]).double() - grads[k].double()).abs().max()) /
            max(float(grads[k].abs().max()), 1e-4 * gmax) for k in grads}
    worst = max(errs, key=errs.get)
    return worst, errs[worst]


@pytest.mark.parametrize("labels", [False, True])
def test_train_step_dropout_and_labels_match_oracle(cuda, labels):
    """drop_out_rate 0.1 in both teacher-forcing passes (embedding and attention-output dropout, the masks read back
    from the product's counter-based RNG) and, with labels, the LabelConditioner: genre rows replace position 0
    (autoregressive_fmha.py:120-129) and the genre table is trained with the prior (prior.py:268-271,299). Loss,
    accuracy, pass-1 mixing and every gradient (the genre table's included) vs fp64 autograd."""
    from prior import Prior
    cfg = CFG
    pk = dict(width=cfg.width, depth=cfg.depth, heads=cfg.heads, blocks=cfg.blocks, attn_stacks=cfg.attn_stacks,
              drop_out_rate=0.1)
    pr = Prior(0, [(cfg.ctx,)], cfg.bins, [3], [2], None, pk, None, genre_classes=10 if labels else None,
               dtype="fp32", device="cuda", seed=11)
    vals = pr.prior.store.values()
    g = _gen(17)
    N = 2
    codes = torch.randint(0, cfg.bins - 1, (N, cfg.ctx), generator=g)
    mask = torch.rand(N, cfg.ctx, generator=g) < 0.2
    y = torch.tensor([3, 7])
    ctr = pr.optimizer.iterations.clone()
    seed = pr.teacher_seed
    d1 = _dropout_masks(pr, N, cfg.ctx, seed * 7919 + 1, ctr)
    d2 = _dropout_masks(pr, N, cfg.ctx, seed * 7919 + 2, ctr)
    lab = ("label_conditioner/genre_embedding/embeddings", y) if labels else None
    loss, acc, grads, bi = P.train_step_grads(P.to_torch(vals), cfg, codes, mask, labels=lab, drop1=d1, drop2=d2)
    x = (codes.cuda(), y.cuda()) if labels else codes.cuda()
    res = pr.train_step(x, tf_mask=mask.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pr._last_batch_input.cpu(), bi)
    assert abs(float(res["loss"]) - loss) <= 1e-5 * abs(loss)
    assert abs(float(res["accuracy"]) - acc) <= 1.0 / codes.numel() + 1e-7
    got = pr.prior.store.grads()
    if labels:
        gl = grads[lab[0]]
        assert float(gl[3].abs().max()) > 0 and float(gl[0].abs().max()) == 0  # only the rows of the labels
    worst, err = _grad_errs(got, grads)
    assert err < 2e-4, (worst, err)


def test_conditioned_labelled_graph_replay_matches_eager(cuda):
    """The upsampler (ConditionerNet on the level above) with genre labels and dropout 0.1, captured as one hipGraph:
    replays (the teacher-forcing draw and the dropout masks advancing on the device counter) end bitwise where the
    same steps run eagerly end."""
    from prior import Prior
    ck = dict(dilation_factor=3, dilation_cycle=4, residual_width=32, residual_depth=8)
    pk = dict(width=128, depth=3, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.1)

    def make():
        return Prior(0, [(256,), (64,)], 64, [3, 2], [2, 2], None, pk, ck, genre_classes=10, dtype="fp32",
                     device="cuda", seed=5)

    a, b = make(), make()
    g = _gen(23)
    codes = torch.randint(0, 63, (2, 256), generator=g).cuda()
    upper = torch.randint(0, 63, (2, 64), generator=g).cuda()
    y = torch.tensor([1, 8]).cuda()
    for _ in range(3):
        a.train_step((codes, upper, y))
    b.capture_train_step((codes, upper, y), warmup=1)
    b.train_step((codes, upper, y))
    b.train_step((codes, upper, y))
    torch.cuda.synchronize()
    assert torch.equal(a.prior.store.flat, b.prior.store.flat)
    assert float(a.results()["loss"]) == float(b.results()["loss"])
    # the genre rows of the labels moved, the others did not
    lc = a.label_conditioner
    w = a.prior.store.view(lc.name)
    w0 = make().prior.store.view(lc.name)
    assert not torch.equal(w[1], w0[1]) and torch.equal(w[0], w0[0])


def test_prior_checkpoint_resume_bitwise(cuda, tmp_path):
    """Prior.save / load (weights-only torch checkpoint): 2 steps, save, 2 more steps; a fresh prior loaded from
    the checkpoint runs the same 2 steps and ends bitwise where the uninterrupted run ended (teacher forcing and
    dropout follow the restored step counter)."""
    from prior import Prior
    ck = dict(dilation_factor=3, dilation_cycle=4, residual_width=32, residual_depth=8)
    pk = dict(width=128, depth=3, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.1)

    def make(seed):
        return Prior(0, [(256,), (64,)], 64, [3, 2], [2, 2], None, pk, ck, genre_classes=10, dtype="fp32",
                     device="cuda", seed=seed)

    g = _gen(29)
    batches = [(torch.randint(0, 63, (2, 256), generator=g).cuda(), torch.randint(0, 63, (2, 64), generator=g).cuda(),
                torch.randint(0, 10, (2,), generator=g).cuda()) for _ in range(4)]
    a = make(5)
    for bt in batches[:2]:
        a.train_step(bt)
    path = str(tmp_path / "prior.pt")
    a.save(path)
    for bt in batches[2:]:
        a.train_step(bt)
    b = make(6)  # different init: everything must come from the checkpoint
    b.load(path)
    for bt in batches[2:]:
        b.train_step(bt)
    torch.cuda.synchronize()
    assert torch.equal(a.prior.store.flat, b.prior.store.flat)
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v)
    assert float(a.results()["loss"]) == float(b.results()["loss"])
    raw = torch.load(path, weights_only=True)
    assert raw["format"] == "vqa-prior/2" and raw["iterations"] == 2
    # a format-/1 file of the packed layout (the first releases) loads by name into the aligned layout
    st = a.prior.store
    pack = lambda flat: torch.cat([flat[o:o + int(np.prod(sh))] for _, (o, sh) in st.offsets.items()])  # noqa: E731
    old = {k: v for k, v in raw.items() if k != "layout"}
    old.update(format="vqa-prior/1", weights=pack(raw["weights"]), adam_m=pack(raw["adam_m"]), adam_v=pack(raw["adam_v"]))
    assert old["weights"].numel() == st.count <= st.size
    torch.save(old, str(tmp_path / "prior_v1.pt"))
    c = make(7)
    c.load(str(tmp_path / "prior_v1.pt"))
    d = make(8)
    d.load(path)
    assert torch.equal(c.prior.store.flat, d.prior.store.flat) and torch.equal(c.optimizer.v, d.optimizer.v)


def test_train_step_small_prior_full_size(cuda):
    """The headline prior configuration (BASELINE config 4, SMALL_PRIOR: width 128, depth 6, 2 heads, 4 blocks,
    ctx 8192, 2048 bins; prior.py:414) on one full-length sequence: fp32 step vs the fp64 oracle (pass-1 mixing
    exact, loss 1e-5, every gradient 2e-4 of its tensor's max), then the bf16 model's loss within 2e-2 (SURVEY.md
    §8c) on the same input."""
    full = P.PriorConfig(bins=2048, ctx=8192, width=128, depth=6, heads=2, blocks=4, attn_stacks=1)
    pr, vals = _prior(full, seed=13)
    g = _gen(41)
    codes = torch.randint(0, full.bins - 1, (1, full.ctx), generator=g)
    mask = torch.rand(1, full.ctx, generator=g) < 0.2
    loss, acc, grads, bi = P.train_step_grads(P.to_torch(vals), full, codes, mask)
    res = pr.train_step(codes.cuda(), tf_mask=mask.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pr._last_batch_input.cpu(), bi)
    assert abs(float(res["loss"]) - loss) <= 1e-5 * abs(loss)
    assert abs(float(res["accuracy"]) - acc) <= 1.0 / codes.numel() + 1e-7
    worst, err = _grad_errs(pr.prior.store.grads(), grads)
    assert err < 2e-4, (worst, err)
    pb, _ = _prior(full, dtype="bf16", seed=13)
    rb = pb.train_step(codes.cuda(), tf_mask=torch.zeros_like(mask).cuda())
    l0, _, _, _ = P.train_step_grads(P.to_torch(vals), full, codes, torch.zeros_like(mask))
    assert abs(float(rb["loss"]) - l0) <= 2e-2 * abs(l0)


def test_decode_full_context_teacher_forced(cuda):
    """The decode kernel at the SMALL_UPSAMPLER shape (ctx 8192, 2048 bins, depth 6; BASELINE config 5) with an
    up-sampled x_cond: teacher-forced logits over 2100 positions (past the first 2048-block boundary, so the
    prev-row layers attend a real block) vs the fp64 oracle forward, 2e-5 of max |logit|."""
    full = P.PriorConfig(bins=2048, ctx=8192, width=128, depth=6, heads=2, blocks=4, attn_stacks=1)
    m, p = _model(full, seed=17)
    g = _gen(43)
    L = 2100
    tok = torch.randint(0, full.bins, (2, L + 1), generator=g)
    tok[:, 0] = full.bins - 1
    xc = torch.randn(2, full.ctx, full.width, generator=g) * 0.5
    _, dl = m.sample(2, max_length=L, x_cond=xc.cuda(), forced=tok.cuda(), return_logits=True, seed=3)
    torch.cuda.synchronize()
    ref = P.model_forward(p, full, tok[:, :L], x_cond=xc.double())
    assert _rel(dl, ref) < 2e-5


def test_random_sample_search_matches_oracle_scores(cuda):
    """autoregressive_fmha.py:242-302 random search: the product's per-sequence losses equal the fp64 oracle's
    mean cross entropy of the same samples (1e-5), and the returned sample is the lowest-loss one of all rounds
    among those passing the token-frequency rule (recomputed on the host from the same seeded samples)."""
    m, p = _model(CFG)
    L, iters, bpi, freq, seed = 60, 3, 4, 0.5, 11
    best, best_loss = m.random_sample(seq_length=L, iterations=iters, batch_per_iter=bpi, token_freq=freq, seed=seed)
    cands = []
    for i in range(iters):
        out = m.sample(bpi, max_length=L, seed=seed + i).cpu()
        got = m.sequence_loss(out[:, :-1], out[:, 1:]).cpu().double()
        logits = P.model_forward(p, CFG, out[:, :-1])
        ref = (torch.logsumexp(logits, -1) - torch.gather(logits, -1, out[:, 1:, None]).squeeze(-1)).mean(dim=1)
        assert _rel(got, ref) < 1e-5
        for k in range(bpi):
            _, counts = torch.unique(out[k], return_counts=True)
            if int(counts.max()) < int(L * freq):
                cands.append((float(got[k]), out[k]))
    want = min(cands, key=lambda c: c[0])
    assert abs(best_loss - want[0]) < 1e-6 and torch.equal(best.cpu(), want[1])


# ------------------------------------------------------------------ other block lengths, block counts and heads
def _cfg3(ctx, blocks, heads):
    cfg = P.PriorConfig(bins=64, ctx=ctx, width=128, depth=3, heads=heads, blocks=blocks, attn_stacks=1)
    assert sorted(cfg.attn_func(i) for i in range(cfg.depth)) == [0, 1, 2]  # row, column and previous row
    return cfg


@pytest.mark.parametrize("ctx,blocks", [(128, 2), (512, 8), (192, 1), (384, 2)])
def test_model_logits_match_oracle_shapes(cuda, ctx, blocks):
    """Logits at 2, 8 and 1 blocks of one key tile and at blocks of three tiles (l = 192)."""
    cfg = _cfg3(ctx, blocks, 2)
    m, p = _model(cfg, seed=5)
    tok = torch.randint(0, cfg.bins, (2, cfg.ctx), generator=_gen(ctx + blocks))
    logits, _ = m(tok)
    torch.cuda.synchronize()
    assert _rel(logits, P.model_forward(p, cfg, tok)) < 2e-5


def test_train_step_multi_tile_blocks_matches_oracle(cuda):
    """One fp32 train step at ctx 384 in 2 blocks (l = 192: three key tiles per block): the glue around the
    attention kernels, the value-bias gradient from block 0 of the previous-row layer included."""
    cfg = _cfg3(384, 2, 2)
    pr, vals = _prior(cfg, seed=19)
    g = _gen(37)
    codes = torch.randint(0, cfg.bins - 1, (2, cfg.ctx), generator=g)
    mask = torch.rand(2, cfg.ctx, generator=g) < 0.2
    loss, acc, grads, bi = P.train_step_grads(P.to_torch(vals), cfg, codes, mask)
    res = pr.train_step(codes.cuda(), tf_mask=mask.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pr._last_batch_input.cpu(), bi)
    assert abs(float(res["loss"]) - loss) <= 1e-5 * abs(loss)
    worst, err = _grad_errs(pr.prior.store.grads(), grads)
    assert err < 2e-4, (worst, err)
    vb = "prior/layer2/mha/value/bias"
    assert float(grads[vb].abs().max()) > 0  # the previous-row layer's value bias does receive a gradient


# (ctx, blocks, heads, L, N). l = 12: the decode has no multiple-of-64 rule, L = ctx runs the last position; one
# block: previous row is always the value bias, a column is one key; head dim 32 with more than 256 row keys (the
# idx += 256 loop wraps); 4 heads (head dim 8); and the two ends of the score scratch's rule heads * max(l, blocks)
# <= 4096: 4 heads of 1024-token blocks, 2 heads over 2048 one-token blocks (columns of up to 2048 keys)
DECODE_SHAPES = [(96, 8, 2, 96, 2), (192, 1, 2, 192, 2), (640, 2, 1, 640, 2), (96, 8, 4, 96, 2),
                 (1024, 1, 4, 1024, 2), (2048, 2048, 2, 2048, 1)]


@pytest.mark.parametrize("ctx,blocks,heads,L,N", DECODE_SHAPES)
def test_decode_teacher_forced_logits_shapes(cuda, ctx, blocks, heads, L, N):
    cfg = _cfg3(ctx, blocks, heads)
    m, p = _model(cfg, seed=23)
    tok = torch.randint(0, cfg.bins, (N, L + 1), generator=_gen(ctx + heads))
    tok[:, 0] = cfg.bins - 1
    _, logits = m.sample(N, max_length=L, forced=tok.cuda(), return_logits=True, seed=5)
    torch.cuda.synchronize()
    ref = P.model_forward(p, cfg, tok[:, :L])
    assert _rel(logits, ref) < 2e-5


@pytest.mark.parametrize("ctx,blocks,heads,msg", [
    (1025, 1, 4, r"heads 4 x max\(block length 1025, blocks 1\) exceeds the 4096-float score scratch"),
    (2049, 2049, 2, r"heads 2 x max\(block length 1, blocks 2049\) exceeds the 4096-float score scratch"),
    (4097, 4097, 1, r"heads 1 x max\(block length 1, blocks 4097\) exceeds the 4096-float score scratch"),
    (2049, 1, 1, r"heads 1 block 2049 unsupported"),
    (64, 1, 8, r"heads 8 block 64 unsupported")])
def test_decode_rejects_shapes_past_the_score_scratch(cuda, ctx, blocks, heads, msg):
    """Just past what the decode kernel's score scratch holds (include/vqa.h): sample() raises ValueError and the
    entry point itself returns VQA_E_UNSUPPORTED (-2); nothing is launched."""
    import vqa_lib as V
    cfg = P.PriorConfig(bins=64, ctx=ctx, width=128, depth=3, heads=heads, blocks=blocks, attn_stacks=1)
    m, _ = _model(cfg)
    assert V.decode_shape_error(ctx, heads, blocks) is not None
    with pytest.raises(ValueError, match="decode"):
        m.sample(1, max_length=1)
    layers = [ly.layer_desc() for ly in m.transformer.layers]
    tokens = torch.zeros(1, 2, dtype=torch.int64, device="cuda")
    with pytest.raises(V.VQAError, match=r"\(-2\): prior_decode: .*" + msg):
        V.prior_decode(layers, m.store.view(m.emb_name), m._pos().contiguous(), m.store.view(m.out_kernel),
                       m.store.view(m.out_bias), tokens, m.decode_cache(1), 1, ctx, heads, blocks, m.start_token, 0)
    for c, b, h, *_ in DECODE_SHAPES:
        assert V.decode_shape_error(c, h, b) is None
