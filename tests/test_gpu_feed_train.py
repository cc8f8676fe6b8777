"""The device feed inside the models: VQVAE.train_step / capture_train_step / fit / evaluate with an AudioFeed and
Prior.train_step on the feed's (audio, labels) batch.

Everything is compared bitwise: a feed step runs the kernels of a host-batch step on the same values (the feed's
fp32 batch is exactly the int16 sample times 2^-15, which the host builds too), and a replayed graph runs the
kernels of the eager step in the same order."""
import numpy as np
import pytest
import torch

from audio_feed import AudioCorpus, AudioFeed
from oracle import vqvae_ref as R
from vqvae import VQVAE

pytestmark = pytest.mark.gpu

T, B = 4096, 2
CFG = R.RefConfig(input_len=T, levels=2, latent_dim=64, down_depth=[3, 2], strides=[2, 2], num_embeddings=256,
                  residual_width=32, residual_depth=2, dilation_factor=3)
LABELS = (4, 9, 0)


def _tracks():
    """Three int16 tracks of tones plus noise (never silent: the spectral loss has no epsilon)."""
    rng = np.random.default_rng(7)
    out = []
    for n, f in ((3 * T + 100, 220.0), (2 * T, 523.0), (T + T // 2 + 1, 1300.0)):
        t = np.arange(n)
        x = 0.5 * np.sin(2 * np.pi * f * t / 22050.0 + rng.uniform(0, 6.28)) + 0.05 * rng.standard_normal(n)
        out.append(np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))
    return out


@pytest.fixture(scope="module")
def corpus(cuda):
    c = AudioCorpus.from_arrays(_tracks(), LABELS, window=T, hop=T // 2, device=cuda)
    assert len(c) == 5 + 3 + 2
    return c


@pytest.fixture(scope="module")
def init():
    return R.init_params(CFG, 1), R.init_vq_state(CFG, 2)


def _model(init):
    m = VQVAE((T, 1), CFG.levels, CFG.latent_dim, CFG.down_depth, CFG.strides, num_embeddings=CFG.num_embeddings,
              residual_width=CFG.residual_width, residual_depth=CFG.residual_depth,
              dilation_factor=CFG.dilation_factor, dtype="bf16", device="cuda:0")
    m.set_weights(init[0])
    m.set_vq_state(init[1])
    m.compile()
    return m


def _restart(m, init):
    """The state of a fresh model, as tests/test_gpu_train.py::test_graph_replay_matches_eager restores it."""
    m.set_weights(init[0])
    m.set_vq_state(init[1])
    m.load_state_dict({**m.state_dict(), "adam_m": torch.zeros_like(m.optimizer.m).cpu(),
                       "adam_v": torch.zeros_like(m.optimizer.v).cpu(), "iterations": 0})


def _same_state(a, b):
    torch.cuda.synchronize()
    assert torch.equal(a.store.flat, b.store.flat)
    assert torch.equal(a.optimizer.m, b.optimizer.m) and torch.equal(a.optimizer.v, b.optimizer.v)
    for sa, sb in zip(a.get_vq_state(), b.get_vq_state()):
        assert sa["calls"] == sb["calls"]
        for k in ("embeddings", "m_t", "N_t"):
            assert np.array_equal(sa[k], sb[k]), k


def _host_batch(corpus, slots):
    flat = corpus.samples[:corpus.corpus_len].cpu().numpy()
    rows = np.stack([flat[s:s + T] for s in corpus.starts_host[slots]])
    return (rows.astype(np.float32) * np.float32(2.0 ** -15))[:, :, None]


@pytest.fixture(scope="module")
def eager4(corpus, init):
    """The reference run shared by the tests: 4 eager train_step(feed) calls from the initial state."""
    m = _model(init)
    feed = AudioFeed(corpus, B, seed=13)
    for _ in range(4):
        m.train_step(feed)
    assert feed.step == 4
    return m


def test_feed_steps_equal_host_batch_steps(corpus, init, eager4):
    feed = AudioFeed(corpus, B, seed=13)   # only for its slot rule: nothing is drawn from it
    assert feed.steps_per_epoch == 5
    m = _model(init)
    for i in range(4):
        m.train_step(_host_batch(corpus, feed.slots(i)))
    _same_state(eager4, m)


def test_captured_feed_step_equals_eager(corpus, init, eager4):
    m = _model(init)
    feed = AudioFeed(corpus, B, seed=13)
    m.capture_train_step(feed, warmup=1)     # one real eager step on the feed's step 0; the capture draws nothing
    assert feed.step == 1 and m._graph_x.data_ptr() == feed.x.data_ptr()
    for _ in range(3):
        m.train_step(feed)                   # replays: steps 1, 2, 3
    assert feed.step == 4
    _same_state(eager4, m)
    # from the restored state and step 0 the graph alone runs the same four steps
    _restart(m, init)
    feed.load_state_dict({"counter": 0, "seed": 13})
    for _ in range(4):
        m.train_step(feed)
    assert feed.step == 4
    _same_state(eager4, m)
    # another feed object is drawn eagerly (its own counter moves, the captured feed's does not); so is other data
    other = AudioFeed(corpus, B, seed=13)
    other.load_state_dict({"counter": 4, "seed": 13})
    m.train_step(other)
    assert other.step == 5 and feed.step == 4
    ref = _model(init)
    ref.load_state_dict(eager4.state_dict())
    ref.set_vq_state(eager4.get_vq_state())
    ref.train_step(_host_batch(corpus, other.slots(4)))
    torch.cuda.synchronize()
    assert torch.equal(ref.store.flat, m.store.flat)
    m.train_step(_host_batch(corpus, other.slots(5)))
    assert feed.step == 4


def test_fit_and_evaluate_run_whole_epochs(corpus, init):
    m = _model(init)
    feed = AudioFeed(corpus, B, seed=2)
    hist = m.fit(feed, epochs=2)
    assert len(hist) == 2 and all(np.isfinite(h["loss"]) for h in hist)
    assert feed.step == 2 * feed.steps_per_epoch == 10
    val = AudioFeed(corpus, B, shuffle=False)
    logs = m.evaluate(val, return_dict=True)
    assert val.step == val.steps_per_epoch and np.isfinite(logs["loss"])
    m.test_step(val)
    assert val.step == val.steps_per_epoch + 1


def test_prior_trains_on_the_feeds_labelled_batch(cuda):
    """Prior.train_step((audio, y)) as the reference's prior takes it (prior.py:251-254), with the feed's device
    tensors: the labels reach the step as the feed's own buffer (no host round trip) and equal the host's table."""
    from prior import Prior
    Tp = 2048
    vq = VQVAE((Tp, 1), 1, 64, [3], [2], num_embeddings=32, residual_width=32, residual_depth=2, dilation_factor=3,
               dtype="fp32", device="cuda:0")
    tracks = [t[:n] for t, n in zip(_tracks(), (3 * Tp, 2 * Tp, Tp))]
    c = AudioCorpus.from_arrays(tracks, LABELS, window=Tp, device=cuda)
    feed = AudioFeed(c, 2, seed=4)
    pk = dict(width=128, depth=3, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.0)
    pr = Prior(0, [(Tp // 8,)], 64, [3], [2], vq, pk, None, genre_classes=10, dtype="fp32", device="cuda:0", seed=11)
    batch = feed.next()
    codes, upper, y = pr._codes(batch)
    assert y.data_ptr() == feed.y.data_ptr() and upper is None
    assert codes.shape == (2, Tp // 8) and codes.is_cuda and int(codes.max()) < 32
    want = c.labels_host[feed.slots(0)]
    assert np.array_equal(feed.y.cpu().numpy(), want) and set(want.tolist()) <= set(LABELS)
    w0 = pr.prior.store.view(pr.label_conditioner.name).clone()
    res = pr.train_step(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(res["loss"]))
    w = pr.prior.store.view(pr.label_conditioner.name)
    moved = [k for k in range(10) if not torch.equal(w[k], w0[k])]
    assert sorted(moved) == sorted(set(want.tolist()))  # only the genre rows of the batch's labels were trained
