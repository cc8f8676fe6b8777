"""Weight averaging through the models (VQVAE, Prior, VQVAESampler): captured steps, the averaged_weights() context,
the sampler's averaged=True, checkpoints and two data-parallel ranks.

Models: the smallest VQ-VAE and prior of tests/test_gpu_clip_train.py. Everything is compared bitwise except the two
ranks against the single process, which uses tests/test_gpu_clip_train.py's bound for the weights (1e-5, max-norm
relative). The optimizers start averaging at step 1 (average_start_step=1), so after the first step the average
still equals the weights and after the later ones it does not.
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

import dp_worker as W  # noqa: E402
import ema_dp_worker as EW  # noqa: E402
from oracle import prior_ref as P  # noqa: E402
from oracle import vqvae_ref as R  # noqa: E402
from vqa_optim import Adam  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = R.RefConfig(input_len=2048, levels=2, latent_dim=8, down_depth=[2, 1], strides=[2, 2], num_embeddings=1024,
                   residual_width=32, residual_depth=2, dilation_factor=3)
PCFG = P.PriorConfig(bins=64, ctx=256, width=128, depth=3, heads=2, blocks=4, attn_stacks=1)
AVG = dict(average_decay=0.9, average_start_step=1)


def _vqvae(opt):
    from vqvae import VQVAE
    cfg = TINY
    m = VQVAE((cfg.input_len, 1), cfg.levels, cfg.latent_dim, cfg.down_depth, cfg.strides,
              num_embeddings=cfg.num_embeddings, residual_width=cfg.residual_width,
              residual_depth=cfg.residual_depth, dilation_factor=cfg.dilation_factor, dtype="fp32", device="cuda:0")
    m.set_weights(R.init_params(cfg, 1))
    m.set_vq_state(R.init_vq_state(cfg, 2))
    m.compile(Adam(**opt))
    return m


def _prior(opt):
    from prior import Prior
    cfg = PCFG
    pr = Prior(0, [(cfg.ctx,)], cfg.bins, [3], [2], None,
               dict(width=cfg.width, depth=cfg.depth, heads=cfg.heads, blocks=cfg.blocks, attn_stacks=cfg.attn_stacks,
                    drop_out_rate=0.0), None, dtype="fp32", device="cuda", seed=3)
    pr.prior.store.set_values(P.init_params(cfg, 3))
    pr.compile(Adam(**opt))
    return pr


def _vq_batches(n):
    return [R.synthetic_batch(1, TINY.input_len, seed=40 + i) for i in range(n)]


def _codes(n):
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, PCFG.bins - 1, (2, PCFG.ctx), generator=g).cuda() for _ in range(n)]


class _Side:
    """What the checks read of either model: its store, optimizer and batches."""

    def __init__(self, kind, opt=AVG):
        self.kind = kind
        self.model = _vqvae(opt) if kind == "vqvae" else _prior(opt)
        self.store = self.model.store if kind == "vqvae" else self.model.prior.store
        self.opt = self.model.optimizer

    def batches(self, n):
        return _vq_batches(n) if self.kind == "vqvae" else _codes(n)

    def state(self):
        torch.cuda.synchronize()
        out = {"weights": self.store.flat.clone(), "m": self.opt.m.clone(), "v": self.opt.v.clone(),
               "iterations": self.opt.iterations.clone()}
        if self.opt.average is not None:
            out["average"] = self.opt.average.clone()
        return out

    def look(self, x):
        """A forward pass that changes no state (VQVAE.test_step would run the codebook EMA)."""
        if self.kind == "vqvae":
            return self.model(x, training=False)
        return self.model.evaluate([x], return_dict=True)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- replay equals eager
@pytest.mark.parametrize("kind,opt", [("vqvae", AVG), ("prior", dict(AVG, global_clipnorm=1.0)),
                                      ("prior", dict(average_decay=0.5, dynamic_average_decay=True))],
                         ids=["vqvae", "prior-clipped", "prior-dynamic"])
def test_three_replays_equal_three_eager_steps_bitwise(cuda, kind, opt):
    a, b = _Side(kind, opt), _Side(kind, opt)
    xs = a.batches(4)
    for x in xs:                        # eager: the warm-up batch, then three more
        a.model.train_step(x)
    b.model.capture_train_step(xs[0], warmup=1)
    for x in xs[1:]:                    # three replays
        b.model.train_step(x)
    assert b.model._graph is not None
    sa, sb = a.state(), b.state()
    assert int(sa["iterations"].item()) == 4 and not torch.equal(sa["average"], sa["weights"])
    _same(sa, sb)


def test_three_feed_replays_equal_three_eager_feed_steps_bitwise(cuda):
    """The corpus feed's gather at the head of the graph, the averaging Adam at its end."""
    from audio_feed import AudioCorpus, AudioFeed
    T = TINY.input_len
    rng = np.random.default_rng(7)
    tracks = []
    for n, f in ((3 * T + 100, 220.0), (2 * T, 523.0)):
        x = 0.5 * np.sin(2 * np.pi * f * np.arange(n) / 22050.0) + 0.05 * rng.standard_normal(n)
        tracks.append(np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))
    corpus = AudioCorpus.from_arrays(tracks, (1, 2), window=T, hop=T // 2, device=cuda)
    a, b = _Side("vqvae"), _Side("vqvae")
    fa, fb = AudioFeed(corpus, 1, seed=13), AudioFeed(corpus, 1, seed=13)
    for _ in range(4):
        a.model.train_step(fa)
    b.model.capture_train_step(fb, warmup=1)
    for _ in range(3):
        b.model.train_step(fb)
    assert b.model._graph_feed is fb and fa.step == fb.step == 4
    sa = a.state()
    assert not torch.equal(sa["average"], sa["weights"])
    _same(sa, b.state())


# ---- the context manager
@pytest.mark.parametrize("kind", ["vqvae", "prior"])
def test_averaged_weights_context(cuda, tmp_path, kind):
    s = _Side(kind)
    xs = s.batches(3)
    s.model.train_step(xs[0])
    torch.cuda.synchronize()
    assert torch.equal(s.opt.average, s.store.flat)          # step 0 lies below average_start_step
    for x in xs[1:]:
        s.model.train_step(x)
    before = s.state()
    assert not torch.equal(before["average"], before["weights"])
    outside = s.look(xs[0])

    def names(flat):
        host = flat.cpu().numpy()
        return {n: host[o:o + int(np.prod(sh))].reshape(sh) for n, (o, sh) in s.store.offsets.items()}

    with s.model.averaged_weights() as inside:
        assert inside is s.model
        got = s.model.get_weights()
        want = names(before["average"])
        assert got.keys() == want.keys() and all(np.array_equal(got[n], want[n]) for n in want)
        assert torch.equal(s.opt.average, before["weights"])  # contents exchanged, not copied
        seen = s.look(xs[0])
        for what, call in (("train_step", lambda: s.model.train_step(xs[0])),
                           ("capture_train_step", lambda: s.model.capture_train_step(xs[0])),
                           ("save", lambda: s.model.save(str(tmp_path / "inside.pt"))),
                           ("already inside", lambda: s.model.averaged_weights().__enter__())):
            with pytest.raises(RuntimeError, match=what):
                call()
        assert not (tmp_path / "inside.pt").exists()
    _same(before, s.state())                                  # nothing was trained, nothing stayed swapped
    if kind == "prior":
        assert seen["loss"] != outside["loss"], "the evaluation inside must have seen other weights"
    else:
        assert not torch.equal(seen[0][0], outside[0][0])     # level 0's reconstruction

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with s.model.averaged_weights():
            raise Boom()
    _same(before, s.state())
    with s.model.averaged_weights():                          # and the context can be entered again
        pass
    _same(before, s.state())
    s.model.train_step(xs[0])                                 # training goes on afterwards
    assert int(s.opt.iterations.item()) == 4


@pytest.mark.parametrize("kind", ["vqvae", "prior"])
def test_a_model_without_an_average_refuses_the_context(cuda, kind):
    s = _Side(kind, {})
    w = s.store.flat.clone()
    with pytest.raises(ValueError, match="no average"):
        with s.model.averaged_weights():
            pass
    assert torch.equal(s.store.flat, w) and s.opt.average is None


# ---- a captured step survives a swap
@pytest.mark.parametrize("kind", ["vqvae", "prior"])
def test_captured_step_survives_a_swap(cuda, kind):
    k = 2
    a, b = _Side(kind), _Side(kind)
    xs = a.batches(1 + 2 * k)
    a.model.capture_train_step(xs[0], warmup=1)
    for x in xs[1:]:
        a.model.train_step(x)                                 # 2k replays, uninterrupted
    b.model.capture_train_step(xs[0], warmup=1)
    for x in xs[1:1 + k]:
        b.model.train_step(x)
    with b.model.averaged_weights():
        b.look(xs[0])
    for x in xs[1 + k:]:
        b.model.train_step(x)                                 # the same graph, after the swaps
    assert a.model._graph is not None and b.model._graph is not None
    _same(a.state(), b.state())


# ---- the sampler
def test_sampler_averaged(cuda):
    from sampler import VQVAESampler
    from vqvae import VQVAE
    K, n, total = 64, 2, 24
    cfg = R.RefConfig(input_len=2048, levels=2, latent_dim=16, down_depth=[3, 2], strides=[2, 2], num_embeddings=K,
                      residual_width=32, residual_depth=3, dilation_factor=3)
    vq = VQVAE((cfg.input_len, 1), cfg.levels, cfg.latent_dim, cfg.down_depth, cfg.strides, num_embeddings=K,
               residual_width=32, residual_depth=3, dilation_factor=3, dtype="fp32", device="cuda:0")
    vq.set_weights(R.init_params(cfg, 31))
    vq.set_vq_state(R.init_vq_state(cfg, 32))
    s = VQVAESampler([3, 2], [2, 2], [64, 16], codebook_size=K, dtype="fp32", device="cuda", seed=4)
    with pytest.raises(ValueError, match="no average"):       # the priors' default optimizer keeps none
        s.sample(n, seed=9, averaged=True)
    # averages that are not the weights, without training three models: compiled in, then set by hand
    gen = torch.Generator(device="cuda").manual_seed(5)
    for m, store in [(pr, pr.prior.store) for pr in s.priors]:
        m.compile(Adam(average_decay=0.9))
        noise = torch.randn(store.flat.shape, generator=gen, device="cuda")
        m.optimizer.average.copy_(store.flat * (1.0 + 0.5 * noise))
    with pytest.raises(ValueError, match="VQ-VAE"):           # the priors average now, the VQ-VAE does not
        s.sample_audio(n, vq, seed=9, total_length=total, averaged=True)
    vq.compile(Adam(average_decay=0.9))
    vq.optimizer.average.copy_(vq.store.flat * 0.75)
    models = [(pr, pr.prior.store) for pr in s.priors] + [(vq, vq.store)]
    before = [(st.flat.clone(), m.optimizer.average.clone()) for m, st in models]

    plain = s.sample(n, seed=9, total_length=total)
    got = s.sample(n, seed=9, total_length=total, averaged=True)
    pcm, clipped, zs = s.sample_audio(n, vq, seed=9, total_length=total, averaged=True)
    torch.cuda.synchronize()
    for (m, st), (w, avg) in zip(models, before):             # every model is left as it was
        assert torch.equal(st.flat, w) and torch.equal(m.optimizer.average, avg)

    for m, st in models:
        m.optimizer.swap_weights(st)
    want = s.sample(n, seed=9, total_length=total)
    want_pcm, want_clipped = vq.render(want[0])
    for m, st in models:
        m.optimizer.swap_weights(st)
    for a, b, c, p in zip(got, want, zs, plain):
        assert torch.equal(a, b) and torch.equal(c, b)
    assert any(not torch.equal(a, p) for a, p in zip(got, plain)), "the averaged draw must differ from the plain one"
    assert torch.equal(pcm, want_pcm) and torch.equal(clipped, want_clipped)
    assert not torch.equal(pcm, vq.render(want[0])[0]), "the render must have used the averaged decoder"
    # one level on its own
    one = s.sample_level([torch.zeros(n, 0, dtype=torch.int64, device="cuda")] * 2, 1, seed=9, averaged=True)
    assert torch.equal(one[1], s.sample(n, seed=9, averaged=True)[1])


# ---- checkpoints
@pytest.mark.parametrize("kind", ["vqvae", "prior"])
def test_resume_reproduces_the_uninterrupted_run_average_included(cuda, tmp_path, kind):
    k = 2
    a, b, c = _Side(kind), _Side(kind), _Side(kind)
    xs = a.batches(2 * k)
    for x in xs:
        a.model.train_step(x)
    for x in xs[:k]:
        b.model.train_step(x)
    path = str(tmp_path / f"{kind}.pt")
    b.model.save(path)
    ck = torch.load(path, weights_only=True)
    assert ck["format"].endswith("/2") and torch.equal(ck["adam_ema"].cuda(), b.opt.average)
    c.model.load(path)
    _same(b.state(), c.state())
    for x in xs[k:]:
        c.model.train_step(x)
    sa = a.state()
    assert not torch.equal(sa["average"], sa["weights"])
    _same(sa, c.state())


@pytest.mark.parametrize("kind", ["vqvae", "prior"])
def test_checkpoints_cross_between_averaging_and_plain_models(cuda, tmp_path, kind):
    plain, avgd = _Side(kind, {}), _Side(kind)
    xs = plain.batches(3)
    for x in xs:
        plain.model.train_step(x)
        avgd.model.train_step(x)
    p_plain, p_avgd = str(tmp_path / "plain.pt"), str(tmp_path / "avgd.pt")
    plain.model.save(p_plain)
    avgd.model.save(p_avgd)
    assert "adam_ema" not in torch.load(p_plain, weights_only=True)
    # a file without an average into an averaging model: the average starts from the loaded weights
    into_avgd = _Side(kind)
    into_avgd.model.train_step(xs[0])
    into_avgd.model.load(p_plain)
    st = into_avgd.state()
    assert torch.equal(st["average"], st["weights"]) and torch.equal(st["weights"], plain.state()["weights"])
    into_avgd.model.train_step(xs[0])
    assert int(into_avgd.opt.iterations.item()) == 4
    # a file with an average into a plain model: ignored; it loads and trains as the plain run does
    into_plain = _Side(kind, {})
    into_plain.model.load(p_avgd)
    assert into_plain.opt.average is None
    _same(plain.state(), into_plain.state())                  # averaging never changed w, m, v
    into_plain.model.train_step(xs[0])
    plain.model.train_step(xs[0])
    _same(plain.state(), into_plain.state())


# ---- data parallel: two gloo ranks on the one GPU
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


@pytest.mark.timeout(600)
def test_dp2_averages_agree(cuda, tmp_path):
    world, port, procs, outs = 2, _port(), [], []
    for r in range(world):
        out = str(tmp_path / f"ema_rank{r}.pt")
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VQA_DP_BATCH=str(W.B_LOCAL), VQA_DP_OVERLAP="0")
        # each rank a fresh child process under its own time limit
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable,
                                       os.path.join(HERE, "ema_dp_worker.py"), out], env=env))
        outs.append(out)
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0] * world, codes
    r0, r1 = (torch.load(o, weights_only=True) for o in outs)
    assert r0["iterations"] == r1["iterations"] == EW.STEPS == 3
    for k in ("weights", "adam_m", "adam_v", "average"):
        assert torch.equal(r0[k], r1[k]), f"ranks differ in {k}"
    assert not torch.equal(r0["average"], r0["weights"])
    m = EW.build(W.B_LOCAL * world)
    single = EW.run(m, W.batches(world))
    for k in ("weights", "average"):
        e = _rel(r0[k].numpy(), single[k].numpy())
        print(f"dp2 against the single process: {k} rel {e:.2e}")
        assert e < 1e-5, (k, e)
