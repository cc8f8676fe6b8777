"""The prior off the one architecture every other GPU test builds (width 128, 2 heads, m_attn 0.25, attn_stacks 1, depth
3 or 6, learned positions), against oracle/prior_ref.py in fp64.

Architectures (ARCHS): attn_stacks 0 (row / column alternation: no previous-row layer, so no value-bias post-add, and
only the column layers read the decode cache across a block boundary) at depths 2 and 4; attn_stacks 1 at depths 1, 4,
5 (the stack ends on a row, a row and a column layer instead of a previous-row one) and 8 (kDecMaxLayers: fills the
decode kernel's layer array and its ring of conv inputs; 112 weight images = three vqa_seqlin_prep batches); and
m_attn 0.125 with one head (attention width 16, head dim 16: trains in fp32, the decode kernel is compiled for 32).
Model level only: the kernel families have their own per-element suites.

Shapes: bins 64, ctx 256 in 4 blocks (l = 64: one key tile, the smallest block the flash kernels take, and every layer
type attends real keys), N = 2, fp32. Bounds are the project's (tests/test_gpu_prior.py): logits and teacher-forced
decode logits 2e-5 of max |logit|, loss 1e-5, every gradient 2e-4 of max(|its tensor|, 1e-4 of the largest gradient),
sampling token for token while the top-2 margin of logits + G is above 1e-3. Measured figures:
profiles/prior_arch_parity.txt. tests/test_prior_arch_host.py shows on the CPU that these cases tell the architectures
apart by at least 500x the logit bound.

The guards at the end are host checks: nothing may be launched (vqa_lib.launch_hook counts), except for the three
configurations that the training kernels themselves refuse with VQA_E_UNSUPPORTED (-2) in the first forward.
"""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]

from oracle import prior_ref as P  # noqa: E402
from test_gpu_prior import _grad_errs, _rel  # noqa: E402

pytestmark = pytest.mark.gpu

# id -> (attn_stacks, depth, heads, m_attn, seed of the parameters)
ARCHS = {"s0d2": (0, 2, 2, 0.25, 31), "s0d4": (0, 4, 2, 0.25, 32), "s1d1": (1, 1, 2, 0.25, 33),
         "s1d4": (1, 4, 2, 0.25, 34), "s1d5": (1, 5, 2, 0.25, 35), "s1d8": (1, 8, 2, 0.25, 36),
         "aw16": (1, 3, 1, 0.125, 37)}
DECODABLE = [a for a in ARCHS if ARCHS[a][3] == 0.25]  # attention width 32
LOGIT_TOL = DECODE_TOL = 2e-5
LOSS_TOL, GRAD_TOL, MARGIN = 1e-5, 2e-4, 1e-3
N, L_DECODE = 2, 150  # 150 positions cross two block boundaries


def _cfg(arch):
    stacks, depth, heads, m_attn, _ = ARCHS[arch]
    return P.PriorConfig(bins=64, ctx=256, width=128, depth=depth, heads=heads, blocks=4, attn_stacks=stacks,
                         m_attn=m_attn)


@functools.lru_cache(maxsize=None)
def _params(arch):
    """(numpy values, fp64 torch values) of an architecture: made once, never written to."""
    vals = P.init_params(_cfg(arch), ARCHS[arch][4])
    return vals, P.to_torch(vals)


@functools.lru_cache(maxsize=None)
def _tokens():
    tok = torch.randint(0, 64, (N, 256), generator=torch.Generator().manual_seed(101))
    tok[:, 0] = 63  # the start token, as a decode begins
    return tok


@functools.lru_cache(maxsize=None)
def _ref_logits(arch):
    """The oracle's logits on _tokens(): the model-forward case checks all 256 positions, the teacher-forced decode
    its first L_DECODE (every factorization is causal, so they are the logits of the 150-token prefix as well)."""
    return P.model_forward(_params(arch)[1], _cfg(arch), _tokens())


def _model(cfg, vals, dtype="fp32", depth=None, **kw):
    from prior import FMHABasedAutoregressiveModel
    m = FMHABasedAutoregressiveModel(cfg.bins, cfg.width, depth or cfg.depth, cfg.blocks, m_attn=cfg.m_attn,
                                     heads=cfg.heads, attn_stacks=cfg.attn_stacks, drop_out_rate=0.0,
                                     context_length=(cfg.ctx,), levels=1, level=0, dtype=dtype, device="cuda", seed=3,
                                     **kw)
    if vals is not None:
        m.store.set_values(vals)
    return m


def _report(case, what, got, bound):
    print(f"ARCH-PARITY {case:<24} {what:<28} {got:.3e}  bound {bound:.1e}")


def _decode_logits(m, tok, L):
    _, logits = m.sample(tok.shape[0], max_length=L, forced=tok[:, :L + 1].cuda(), return_logits=True, seed=5)
    torch.cuda.synchronize()
    return logits


# ------------------------------------------------------------------ logits
@pytest.mark.parametrize("arch", list(ARCHS))
def test_logits_match_oracle(cuda, arch):
    cfg = _cfg(arch)
    m = _model(cfg, _params(arch)[0])
    assert [ly.attn_func for ly in m.transformer.layers] == [cfg.attn_func(i) for i in range(cfg.depth)]
    logits, _ = m(_tokens())
    torch.cuda.synchronize()
    err = _rel(logits, _ref_logits(arch))
    _report(arch, "logits", err, LOGIT_TOL)
    assert err < LOGIT_TOL


# ------------------------------------------------------------------ one train step
@pytest.mark.parametrize("arch", ["s0d2", "s0d4", "s1d5", "s1d8", "aw16"])
def test_train_step_matches_oracle(cuda, arch):
    """Loss, pass-1 mixing and every gradient of one step with a 20 % teacher-forcing mask. The value-bias post-adds
    queued by the backward are counted: one per previous-row layer, none with attn_stacks 0 — where the value
    biases' gradients come from the weight-gradient kernels alone and must still match."""
    from prior import Prior, ResidualAttnBlock
    cfg = _cfg(arch)
    vals, p = _params(arch)
    pr = Prior(0, [(cfg.ctx,)], cfg.bins, [3], [2], None,
               dict(width=cfg.width, depth=cfg.depth, heads=cfg.heads, blocks=cfg.blocks, attn_stacks=cfg.attn_stacks,
                    m_attn=cfg.m_attn, drop_out_rate=0.0), None, dtype="fp32", device="cuda", seed=3)
    assert pr.prior.transformer.attn_width == cfg.attn_width
    pr.prior.store.set_values(vals)
    g = torch.Generator().manual_seed(107)
    codes = torch.randint(0, cfg.bins - 1, (N, cfg.ctx), generator=g)
    mask = torch.rand(N, cfg.ctx, generator=g) < 0.2
    loss, acc, grads, bi = P.train_step_grads(p, cfg, codes, mask)
    queued = []
    inner = ResidualAttnBlock.backward

    def backward(self, dout, T, deferred, post_adds):
        queued.append(post_adds)
        return inner(self, dout, T, deferred, post_adds)

    ResidualAttnBlock.backward = backward
    try:
        res = pr.train_step(codes.cuda(), tf_mask=mask.cuda())
        torch.cuda.synchronize()
    finally:
        ResidualAttnBlock.backward = inner
    assert len(queued) == cfg.depth and all(q is queued[0] for q in queued)
    prev_rows = [i for i in range(cfg.depth) if cfg.attn_func(i) == 2]
    assert len(queued[0]) == len(prev_rows)
    assert cfg.attn_stacks == 1 or not prev_rows
    assert torch.equal(pr._last_batch_input.cpu(), bi)  # pass-1 argmax + mixing (exact)
    lerr = abs(float(res["loss"]) - loss) / abs(loss)
    _report(arch, "train loss", lerr, LOSS_TOL)
    assert lerr <= LOSS_TOL
    assert abs(float(res["accuracy"]) - acc) <= 1.0 / codes.numel() + 1e-7
    got = pr.prior.store.grads()
    worst, err = _grad_errs(got, grads)
    _report(arch, f"grad {worst[6:]}", err, GRAD_TOL)
    assert err < GRAD_TOL, (worst, err)
    # the key biases' gradients are analytically zero and are measured against the floor: the worst real one too
    real = {k: v for k, v in grads.items() if not k.endswith("key/bias")}
    worst, err = _grad_errs(got, real)
    _report(arch, f"grad {worst[6:]}", err, GRAD_TOL)
    gmax = max(float(t.abs().max()) for t in grads.values())
    by_name = [k for k in grads if k.endswith("mha/value/bias")]
    assert len(by_name) == cfg.depth
    if arch == "s1d5":  # the stack ends on a column layer: every tensor of that layer, by name
        last = [k for k in grads if k.startswith("prior/layer4/")]
        assert len(last) == 18 and cfg.attn_func(4) == 1
        by_name += last
    for k in by_name:
        ref = grads[k].double()
        # every tensor named here receives a real gradient, but for the key bias (softmax is shift-invariant)
        assert k.endswith("key/bias") or float(ref.abs().max()) > 1e-4 * gmax, k
        e = float((torch.from_numpy(got[k]).double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-4 * gmax)
        assert e < GRAD_TOL, (k, e)


# ------------------------------------------------------------------ the decode kernel
@pytest.mark.parametrize("arch", DECODABLE)
def test_decode_teacher_forced_logits_match_oracle(cuda, arch):
    m = _model(_cfg(arch), _params(arch)[0])
    logits = _decode_logits(m, _tokens(), L_DECODE)
    err = _rel(logits, _ref_logits(arch)[:, :L_DECODE])
    _report(arch, "decode logits", err, DECODE_TOL)
    assert err < DECODE_TOL


@pytest.mark.parametrize("arch", ["s0d4", "s1d8"])
def test_decode_sampling_matches_reference_sampler(cuda, arch):
    """Free Gumbel-max sampling over 70 positions (past the first block boundary) reproduces the reference's
    full-recompute sampler token for token while the top-2 margin of logits + G stays clear of fp32 rounding."""
    cfg = _cfg(arch)
    m = _model(cfg, _params(arch)[0])
    L, seed = 70, 21
    out = m.sample(N, max_length=L, seed=seed).cpu()
    ref, margins = P.sample_full_recompute(_params(arch)[1], cfg, N, L, seed)
    checked = 0
    for n in range(N):
        for i in range(L):
            if margins[n, i] < MARGIN:
                break  # past a near tie the sequences may legitimately diverge
            assert int(out[n, i + 1]) == int(ref[n, i + 1]), (n, i)
            checked += 1
    _report(arch, "sampled tokens compared", checked, N * L)
    assert checked > N * L // 2  # the comparison did not end at an early near tie
    assert (out[:, 0] == cfg.bins - 1).all()


def test_decode_continuation_without_previous_row_layers(cuda):
    """attn_stacks 0, depth 4: a decode primed with its own first 65 tokens (one past the block boundary) gives the
    unprimed decode's tokens and logits bit for bit; only the column layers read the cache across the boundary."""
    arch = "s0d4"
    m = _model(_cfg(arch), _params(arch)[0])
    L, seed = 150, 9
    out, logits = m.sample(N, max_length=L, seed=seed, return_logits=True)
    out2, logits2 = m.sample(N, max_length=L, seed=seed, prime=out[:, 1:66].contiguous(), return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(logits, logits2)
    out3 = m.sample(N, max_length=L, seed=seed, prime=out[:, 1:66].contiguous())  # the heads of primed steps skipped
    assert torch.equal(out, out3)
    assert len(torch.unique(out[:, 66:])) > 8  # a real draw, not a constant sequence


# ------------------------------------------------------------------ the sinusoid table (pos_emb=False)
def test_sinusoid_positions_logits_and_decode_match_oracle(cuda):
    """pos_emb=False (autoregressive_fmha.py:136-137): the fixed table positional_encoding(5000, 128) instead of a
    learned embedding; the oracle takes its first 256 rows in the learned table's slot."""
    from prior import positional_encoding
    cfg = P.PriorConfig(bins=64, ctx=256, width=128, depth=3, heads=2, blocks=4, attn_stacks=1)
    vals = P.init_params(cfg, 38)
    m = _model(cfg, vals, pos_emb=False)
    assert not any("pos_embedding" in name for name in m.store.offsets)
    assert m.pos_name is None and tuple(m._pos().shape) == (5000, 128)
    p = P.to_torch(vals)
    p["prior/pos_embedding/embeddings"] = torch.from_numpy(positional_encoding(5000, 128)[0, :256]).double()
    tok = _tokens()
    ref = P.model_forward(p, cfg, tok)
    logits, _ = m(tok)
    torch.cuda.synchronize()
    err = _rel(logits, ref)
    _report("sinusoid s1d3", "logits", err, LOGIT_TOL)
    assert err < LOGIT_TOL
    err = _rel(_decode_logits(m, tok, L_DECODE), ref[:, :L_DECODE])
    _report("sinusoid s1d3", "decode logits", err, DECODE_TOL)
    assert err < DECODE_TOL


# ------------------------------------------------------------------ guards
class _Launches:
    """Counts libvqa launches (vqa_lib.launch_hook runs before every one is queued) inside a with block."""

    def __enter__(self):
        import vqa_lib as V
        self.n = 0
        assert V.launch_hook is None
        V.launch_hook = self._hit
        return self

    def _hit(self):
        self.n += 1

    def __exit__(self, *exc):
        import vqa_lib as V
        V.launch_hook = None
        return False


def test_sample_refuses_what_the_decode_kernel_is_not_compiled_for(cuda):
    """Attention width 16 (the kernel would stride the 48-column qkv kernel as 96 columns) and depth 9 (past
    kDecMaxLayers): ValueError from sample() with nothing launched."""
    cfg = _cfg("aw16")
    m = _model(cfg, _params("aw16")[0])
    deep = _model(_cfg("s1d8"), None, depth=9)
    with _Launches() as count:
        with pytest.raises(ValueError, match=r"sample\(\): .*attention width of 32 .*got 16"):
            m.sample(N, max_length=8)
        with pytest.raises(ValueError, match=r"sample\(\): .*attention width"):
            m.sample(N, max_length=8, forced=torch.zeros(N, 9, dtype=torch.int64), return_logits=True)
        with pytest.raises(ValueError, match=r"sample\(\): .*depth of 1 to 8 layers \(got 9\)"):
            deep.sample(N, max_length=8)
        assert count.n == 0
    m.sequence_loss(_tokens()[:, :-1], _tokens()[:, 1:])  # the model itself runs; the hook does count
    with _Launches() as count:
        m.sequence_loss(_tokens()[:, :-1], _tokens()[:, 1:])
    torch.cuda.synchronize()
    assert count.n > 0


def test_sinusoid_table_shorter_than_the_sequence_is_refused(cuda):
    """pos_emb=False with the headline context of 8192 against the 5000-row table: ValueError at construction.
    hidden() with more positions than the table holds (sinusoid or learned): ValueError before the first launch."""
    cfg = P.PriorConfig(bins=64, ctx=256, width=128, depth=1, heads=2, blocks=4, attn_stacks=1)
    long = P.PriorConfig(bins=64, ctx=8192, width=128, depth=1, heads=2, blocks=4, attn_stacks=1)
    short = _model(cfg, None, pos_emb=False, maximum_pos_encoding=300)
    learned = _model(cfg, None)
    with _Launches() as count:
        with pytest.raises(ValueError, match="context length 8192 exceeds the sinusoid table of .*5000 rows"):
            _model(long, None, pos_emb=False)
        tok = torch.zeros(1, 320, dtype=torch.int64, device="cuda")  # five whole blocks, 20 rows past the table
        with pytest.raises(ValueError, match="sequence of 320 > the 300 rows"):
            short.hidden(tok)
        with pytest.raises(ValueError, match="sequence of 320 > the 300 rows"):
            short(tok)
        with pytest.raises(ValueError, match="sequence of 320 > the 256 rows"):
            learned.hidden(tok)
        assert count.n == 0
    _model(long, None, pos_emb=False, maximum_pos_encoding=8192)  # a table as long as the context is accepted
    logits, _ = short(torch.zeros(1, 256, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("dtype,m_attn,heads,msg", [
    ("bf16", 0.125, 1, r"seqlin_fwd: K=16 N=16 unsupported"),    # attention width 16 breaks bf16's K % 32
    ("fp32", 0.5, 4, r"seqlin_fwd: K=128 N=192 unsupported"),    # the fused q/k/v conv is 192 wide, N <= 128
    ("fp32", 0.25, 1, r"attn: head_dim 32 unsupported \(16\)"),  # head dim 32
])
def test_training_kernels_refuse_other_widths_loudly(cuda, dtype, m_attn, heads, msg):
    """Configurations the constructors accept and the training kernels do not: VQAError (-2, VQA_E_UNSUPPORTED) from
    the first forward, raised by the entry point's own host check — never a wrong result."""
    import vqa_lib as V
    cfg = P.PriorConfig(bins=64, ctx=256, width=128, depth=1, heads=heads, blocks=4, attn_stacks=1, m_attn=m_attn)
    m = _model(cfg, None, dtype=dtype)
    with pytest.raises(V.VQAError, match=r"failed \(-2\): " + msg):
        m(_tokens())
    torch.cuda.synchronize()
