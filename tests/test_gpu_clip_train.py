"""Gradient clipping through the models' train steps (VQVAE and Prior): eager, captured and data parallel.

A clipped step is teacher-forced from the device's own raw gradients: after one step from zero moments, the store
still holds the raw summed gradient (a clipped apply() does not rewrite it), so m = (1 - beta_1) u and
v = (1 - beta_2) u^2 with u = tests/clip_ref.py's clipping of grad_scale * g in fp64. The thresholds come from a
first run whose clip cannot bite (global_clipnorm 1e30) and are half of what it reports, so clipping is certainly
active. Bounds: SURVEY.md §8c's fp32 criterion, 1e-5 relative to the largest reference magnitude. Captured replays
equal eager steps bitwise. Two gloo ranks on the one GPU end bitwise equal to each other and match the single
process on the concatenated batch within tests/test_gpu_dp.py's step-1 bounds (gradient 2e-6, moments and
weights 1e-5, all max-norm relative).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import clip_ref as C  # noqa: E402
import clip_dp_worker as CW  # noqa: E402
import dp_worker as W  # noqa: E402
from oracle import prior_ref as P  # noqa: E402
from oracle import vqvae_ref as R  # noqa: E402
from vqa_optim import Adam  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
# the survey's `tiny` config as tests/test_gpu_train.py runs it
TINY = R.RefConfig(input_len=2048, levels=2, latent_dim=8, down_depth=[2, 1], strides=[2, 2], num_embeddings=1024,
                   residual_width=32, residual_depth=2, dilation_factor=3)
TINY_B = 1
# the smallest prior tests/test_gpu_prior.py trains
PCFG = P.PriorConfig(bins=64, ctx=256, width=128, depth=3, heads=2, blocks=4, attn_stacks=1)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def _vqvae(clip):
    from vqvae import VQVAE
    cfg = TINY
    m = VQVAE((cfg.input_len, 1), cfg.levels, cfg.latent_dim, cfg.down_depth, cfg.strides,
              num_embeddings=cfg.num_embeddings, residual_width=cfg.residual_width,
              residual_depth=cfg.residual_depth, dilation_factor=cfg.dilation_factor, dtype="fp32", device="cuda:0")
    m.set_weights(R.init_params(cfg, 1))
    m.set_vq_state(R.init_vq_state(cfg, 2))
    m.compile(Adam(**clip))
    return m


def _prior(clip):
    from prior import Prior
    cfg = PCFG
    pr = Prior(0, [(cfg.ctx,)], cfg.bins, [3], [2], None,
               dict(width=cfg.width, depth=cfg.depth, heads=cfg.heads, blocks=cfg.blocks, attn_stacks=cfg.attn_stacks,
                    drop_out_rate=0.0), None, dtype="fp32", device="cuda", seed=3)
    pr.prior.store.set_values(P.init_params(cfg, 3))
    pr.compile(Adam(**clip))
    return pr


def _vq_batches(n):
    return [R.synthetic_batch(TINY_B, TINY.input_len, seed=40 + i) for i in range(n)]


def _codes(n):
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, PCFG.bins - 1, (2, PCFG.ctx), generator=g).cuda() for _ in range(n)]


class _Side:
    """What the checks read of either model: its store, optimizer and one train step."""

    def __init__(self, kind, clip):
        self.kind = kind
        self.model = _vqvae(clip) if kind == "vqvae" else _prior(clip)
        self.store = self.model.store if kind == "vqvae" else self.model.prior.store
        self.opt = self.model.optimizer

    def batches(self, n):
        return _vq_batches(n) if self.kind == "vqvae" else _codes(n)

    def state(self):
        torch.cuda.synchronize()
        return (self.store.flat.clone(), self.opt.m.clone(), self.opt.v.clone(), self.opt._clip["stats"].clone(),
                self.opt.variable_grad_norms().clone())


_PROBE = {}


def _probe(kind):
    """One step whose clip cannot bite: the gradient's global norm, per-variable norms and largest magnitude."""
    if kind not in _PROBE:
        s = _Side(kind, dict(global_clipnorm=1e30))
        s.model.train_step(s.batches(1)[0])
        torch.cuda.synchronize()
        st = {k: float(v) for k, v in s.opt.grad_stats().items()}
        assert st["global_norm"] > 0 and np.isfinite(st["global_norm"])
        assert st["clipped_global_norm"] == st["global_norm"] and st["clipnorm_variables"] == 0
        _PROBE[kind] = dict(norm=st["global_norm"], var_norms=s.opt.variable_grad_norms().cpu().numpy().copy(),
                            gmax=float(s.store.grad[:s.store.size].abs().max()))
        del s
        torch.cuda.empty_cache()
    return _PROBE[kind]


def _clip_for(kind, mode):
    p = _probe(kind)
    if mode == "global_clipnorm":
        return {mode: 0.5 * p["norm"]}
    if mode == "clipnorm":
        return {mode: 0.5 * float(p["var_norms"].max())}
    return {mode: 0.5 * p["gmax"]}


@pytest.mark.parametrize("mode", ["global_clipnorm", "clipnorm", "clipvalue"])
@pytest.mark.parametrize("kind", ["vqvae", "prior"])
def test_clipped_step_from_the_devices_own_gradient(cuda, kind, mode):
    clip = _clip_for(kind, mode)
    s = _Side(kind, clip)
    res = s.model.train_step(s.batches(1)[0])
    torch.cuda.synchronize()
    assert not any("norm" in k or "clip" in k for k in res), "grad statistics stay out of the step's result dict"
    n = s.store.size
    g = s.store.grad[:n].cpu().numpy()
    seg = sorted(int(o) for o, _ in s.store.offsets.values())
    u, norms, rst = C.transform_flat(g, seg, **clip)
    st = {k: float(v) for k, v in s.opt.grad_stats().items()}
    print(kind, clip, st)
    # clipping is active
    if mode == "global_clipnorm":
        assert 0.49 < st["global_scale"] < 0.51
    elif mode == "clipnorm":
        assert st["clipnorm_variables"] >= 1
    else:
        assert st["clipvalue_elements"] >= 1 and st["clipped_global_norm"] < st["global_norm"]
    for k in ("global_norm", "clipped_global_norm", "global_scale"):
        assert abs(st[k] - rst[k]) <= TOL * abs(rst[k]), (k, st[k], rst[k])
    assert st["clipvalue_elements"] == rst["clipvalue_elements"]
    assert _rel(s.opt.variable_grad_norms().cpu().numpy(), norms) < TOL
    omb1, omb2 = 1 - C.hyper(s.opt.beta_1), 1 - C.hyper(s.opt.beta_2)  # the float32 betas the kernel receives
    m_ref, v_ref = omb1 * u, omb2 * u * u
    em, ev = _rel(s.opt.m.cpu().numpy(), m_ref), _rel(s.opt.v.cpu().numpy(), v_ref)
    print(f"{kind} {mode}: m rel {em:.2e}, v rel {ev:.2e}")
    assert em < TOL and ev < TOL
    # and the unclipped moments would not pass
    assert _rel(omb1 * g.astype(np.float64), m_ref) > 0.1


@pytest.mark.parametrize("kind,mode", [("vqvae", "global_clipnorm"), ("vqvae", "clipnorm"), ("prior", "global_clipnorm"),
                                       ("prior", "clipvalue")])
def test_three_replays_equal_three_eager_steps_bitwise(cuda, kind, mode):
    clip = _clip_for(kind, mode)
    a, b = _Side(kind, clip), _Side(kind, clip)
    xs = a.batches(4)
    for x in xs:                        # eager: the warm-up batch, then three more
        a.model.train_step(x)
    b.model.capture_train_step(xs[0], warmup=1)
    for x in xs[1:]:                    # three replays
        b.model.train_step(x)
    assert b.model._graph is not None
    assert int(a.opt.iterations.item()) == int(b.opt.iterations.item()) == 4
    for name, x, y in zip(("weights", "m", "v", "stats", "variable norms"), a.state(), b.state()):
        assert torch.equal(x, y), name


# ---- data parallel: two gloo ranks on the one GPU
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(tmp_path, mode, thr, overlap, world=2):
    port, procs, outs = _port(), [], []
    for r in range(world):
        out = str(tmp_path / f"clip_{mode}_{int(overlap)}_rank{r}.pt")
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VQA_DP_BATCH=str(W.B_LOCAL), VQA_DP_OVERLAP="1" if overlap else "0")
        # each rank under its own time limit
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable,
                                       os.path.join(HERE, "clip_dp_worker.py"), out, mode, repr(thr)], env=env))
        outs.append(out)
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0] * world, codes
    return [torch.load(o, weights_only=True) for o in outs]


_SINGLE = {}


def _single(mode, thr):
    """The single process on the concatenated batch; thr None: the probe run whose clip cannot bite."""
    key = (mode, thr)
    if key not in _SINGLE:
        m = CW.build(W.B_LOCAL * 2, {mode: thr} if thr is not None else dict(global_clipnorm=1e30))
        _SINGLE[key] = CW.run(m, W.batches(2))
        del m
        torch.cuda.empty_cache()
    return _SINGLE[key]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode,overlap", [("global_clipnorm", False), ("clipnorm", False), ("global_clipnorm", True)],
                         ids=["global", "clipnorm", "global-overlapped"])
def test_dp2_clipped_step(cuda, tmp_path, mode, overlap):
    probe = _single("probe", None)
    thr = 0.5 * float(probe["stats"][0]) if mode == "global_clipnorm" else 0.5 * float(probe["var_norms"].max())
    s = _single(mode, thr)
    r0, r1 = _run_ranks(tmp_path, mode, thr, overlap)
    for k in ("weights", "adam_m", "adam_v", "stats", "var_norms", "grads"):
        assert torch.equal(r0[k], r1[k]), f"ranks differ in {k}"
    # the clip bit, on the averaged gradient: the summed one has twice the norm
    if mode == "global_clipnorm":
        assert 0.49 < float(r0["stats"][2]) < 0.51
    else:
        assert float(r0["stats"][3]) >= 1
    e = _rel(r0["grads"].numpy() / 2, s["grads"].numpy())
    assert e < 2e-6, f"exchanged gradient rel {e:.2e}"
    for k in ("adam_m", "adam_v", "weights", "var_norms"):
        e = _rel(r0[k].numpy(), s[k].numpy())
        print(f"dp2 {mode} overlap={overlap}: {k} rel {e:.2e}")
        assert e < 1e-5, (k, e)
    assert _rel(r0["stats"][:3].numpy(), s["stats"][:3].numpy()) < 1e-5
    assert torch.equal(r0["stats"][3:], s["stats"][3:])
    # the clipped moments are not the unclipped ones
    assert _rel(r0["adam_m"].numpy(), probe["adam_m"].numpy()) > 0.1
