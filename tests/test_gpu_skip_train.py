"""The step guard through the models (VQVAE, Prior): eager and captured steps, fit's max_consecutive_skips,
checkpoints and two data-parallel ranks. Everything is compared bitwise.

Models: tests/dp_worker.py's cfg1 VQ-VAE and tests/prior_dp_worker.py's short prior. Non-finite values come from a
NaN sample in a batch or a corpus track and from an inf written into the prior's output bias; no kernel faults on
them (a NaN row quantises to code 0, an inf logit is the head's argmax).

test_the_bad_batch_poisons_a_model_without_the_guard is the check that fails without the feature: Adam swallows an
unknown skip_nonfinite, so there the "guarded" model's weights turn NaN as well.
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
import prior_dp_worker as PW  # noqa: E402
import skip_dp_worker as SW  # noqa: E402
from oracle import vqvae_ref as R  # noqa: E402
from vqa_optim import Adam  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2
T = W.CONFIGS["cfg1"]["input_len"]
GUARD = dict(skip_nonfinite=True, average_decay=0.9)
PLAIN = dict(average_decay=0.9)


def _vqvae(opt, dtype="fp32"):
    m = W.build(B, dtype=dtype)
    m.compile(Adam(**opt))
    return m


@pytest.fixture(scope="module")
def xs():
    """Five clean batches and the fourth with a single NaN sample (shared, never written)."""
    clean = [torch.as_tensor(R.synthetic_batch(B, T, seed=70 + i)) for i in range(5)]
    return clean, SW.poisoned(clean[3])


def _same(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k not in skip:
            assert torch.equal(a[k], b[k]), k


def _results(m):
    return {k: v.clone() for k, v in m.results().items()}


def _three_steps(m, xs, mode):
    """Three train steps on xs[0..2]: eager, or a capture whose one warm-up step is the first, then two replays."""
    if mode == "eager":
        m.train_step(xs[0])
    else:
        m.capture_train_step(xs[0], warmup=1)
    for x in xs[1:3]:
        m.train_step(x)
    assert (m._graph is not None) == (mode == "captured")


# ---- VQ-VAE
@pytest.mark.parametrize("mode", ["eager", "captured"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_vqvae_skips_a_nan_batch_and_goes_on_as_if_it_had_not_been_drawn(cuda, xs, dtype, mode):
    clean, bad = xs
    g, p = _vqvae(GUARD, dtype), _vqvae(PLAIN, dtype)
    assert g._guarded and not p._guarded
    _three_steps(g, clean, mode)
    _three_steps(p, clean, mode)
    # three clean steps: the guard changes nothing
    sg = SW.state(g)
    _same(sg, SW.state(p))
    assert int(sg["iterations"]) == 3
    rg, rp = _results(g), _results(p)
    assert set(rg) - set(rp) == {"skipped_steps"} and int(rg["skipped_steps"]) == 0
    for k in rp:
        assert torch.equal(rg[k], rp[k]), k
    # the NaN batch: nothing moves
    res = g.train_step(bad)
    _same(sg, SW.state(g))
    assert int(res["skipped_steps"]) == 1
    assert {k: int(v) for k, v in g.optimizer.skip_stats().items()} == dict(
        skipped_steps=1, consecutive_skipped=1, last_step_ok=0)
    for k in rp:
        assert torch.equal(_results(g)[k], rg[k]), k
    for a, b in zip(g.get_vq_state(), p.get_vq_state()):
        assert a["calls"] == b["calls"] and all(np.array_equal(a[k], b[k]) for k in ("embeddings", "m_t", "N_t"))
    # a clean step then equals the same step of the model that never saw the bad batch
    g.train_step(clean[4])
    p.train_step(clean[4])
    s = SW.state(g)
    _same(s, SW.state(p))
    assert int(s["iterations"]) == 4 and all(bool(torch.isfinite(v.float()).all()) for v in s.values())
    assert {k: int(v) for k, v in g.optimizer.skip_stats().items()} == dict(
        skipped_steps=1, consecutive_skipped=0, last_step_ok=1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_bad_batch_poisons_a_model_without_the_guard(cuda, xs, dtype):
    clean, bad = xs
    g, p = _vqvae(GUARD, dtype), _vqvae(PLAIN, dtype)
    for m in (g, p):
        m.train_step(clean[0])
        m.train_step(bad)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(p.store.flat).all()), "the unguarded step must have applied the NaN gradient"
    assert not bool(torch.isfinite(p.optimizer.average).all())
    assert bool(torch.isfinite(g.store.flat).all()) and bool(torch.isfinite(g.optimizer.average).all())
    assert int(g.optimizer.iterations.item()) == 1 and int(p.optimizer.iterations.item()) == 2


def test_test_step_is_not_guarded(cuda, xs):
    """test_step and evaluate stay as they were: the trackers and the codebook take every batch."""
    clean, _ = xs
    g, p = _vqvae(GUARD), _vqvae(PLAIN)
    for m in (g, p):
        m.train_step(clean[0])
        m.test_step(clean[1])
    _same(SW.state(g), SW.state(p))
    assert float(g._macc[0, 1]) == 2.0


# ---- fit
def _corpus(cuda, nan_track):
    from audio_feed import AudioCorpus
    rng = np.random.default_rng(3)
    one = lambda n: (0.3 * np.sin(2 * np.pi * 330.0 * np.arange(n) / 22050.0)
                     + 0.05 * rng.standard_normal(n)).astype(np.float32)
    tracks = [one(T), one(5 * T)]
    if nan_track:
        tracks[1][::T // 2] = np.nan      # every window of the second track holds a NaN: no batch of two is clean
    return AudioCorpus.from_arrays(tracks, (1, 2), window=T, hop=T, device=cuda)


def test_fit_raises_at_the_first_epoch_end_on_a_corpus_with_a_nan_track(cuda):
    from audio_feed import AudioFeed
    m = _vqvae(GUARD)
    feed = AudioFeed(_corpus(cuda, True), B, seed=5)
    assert feed.steps_per_epoch == 3
    w = m.store.flat.clone()
    with pytest.raises(FloatingPointError) as e:
        m.fit(feed, epochs=3, max_consecutive_skips=2)
    msg = str(e.value)
    assert "epoch 1" in msg and "3 train steps in a row" in msg and "3 steps skipped in all" in msg
    assert feed.step == 3                                  # the feed counts attempted steps; one epoch ran
    assert torch.equal(m.store.flat, w) and int(m.optimizer.iterations.item()) == 0


def test_fit_on_a_clean_corpus_reports_no_skips(cuda):
    from audio_feed import AudioFeed
    m = _vqvae(GUARD)
    hist = m.fit(AudioFeed(_corpus(cuda, False), B, seed=5), epochs=2, max_consecutive_skips=2)
    assert len(hist) == 2 and all(h["skipped_steps"] == 0 for h in hist)
    assert int(m.optimizer.iterations.item()) == 6 and np.isfinite(hist[-1]["loss"])


def test_a_skip_limit_without_the_guard_is_refused_before_any_launch(cuda):
    from audio_feed import AudioFeed
    m = _vqvae(PLAIN)
    feed = AudioFeed(_corpus(cuda, False), B, seed=5)
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        m.fit(feed, epochs=1, max_consecutive_skips=2)
    assert feed.step == 0 and int(m.optimizer.iterations.item()) == 0
    pr = _prior(PLAIN)
    with pytest.raises(ValueError, match="max_consecutive_skips"):
        pr.fit(None, max_consecutive_skips=2)


# ---- checkpoints
def test_resume_reproduces_the_uninterrupted_run_counters_included(cuda, xs, tmp_path):
    clean, bad = xs
    a, b, c = _vqvae(GUARD), _vqvae(GUARD), _vqvae(GUARD)
    for x in (clean[0], bad, clean[1], clean[2]):
        a.train_step(x)
    for x in (clean[0], bad):
        b.train_step(x)
    path = str(tmp_path / "skip.pt")
    b.save(path)
    assert torch.load(path, weights_only=True)["adam_skipped"] == [1, 1]
    c.load(path)
    want = {k: int(v) for k, v in b.optimizer.skip_stats().items()}
    assert want == dict(skipped_steps=1, consecutive_skipped=1, last_step_ok=0)
    assert {k: int(v) for k, v in c.optimizer.skip_stats().items()} == want
    _same(SW.state(b), SW.state(c), skip=("trackers",))       # the VQ-VAE's trackers are not checkpoint state
    for x in (clean[1], clean[2]):
        c.train_step(x)
    _same(SW.state(a), SW.state(c), skip=("trackers",))
    assert {k: int(v) for k, v in c.optimizer.skip_stats().items()} == {
        k: int(v) for k, v in a.optimizer.skip_stats().items()} == dict(
        skipped_steps=1, consecutive_skipped=0, last_step_ok=1)
    # the file loads into a model without the guard, which ignores the counters
    plain = _vqvae(PLAIN)
    plain.load(path)
    assert plain.optimizer.skipped is None and torch.equal(plain.store.flat, b.store.flat)


# ---- the prior
def _prior(opt):
    pr = PW.build()
    pr.compile(Adam(**opt))
    return pr


def _prior_state(pr):
    torch.cuda.synchronize()
    opt = pr.optimizer
    return {"weights": pr.prior.store.flat.clone(), "m": opt.m.clone(), "v": opt.v.clone(),
            "iterations": opt.iterations.clone(), "loss": pr.train_loss_tracker._acc.clone(),
            "accuracy": pr.train_accuracy_tracker._acc.clone()}


@pytest.mark.parametrize("mode", ["eager", "replayed"])
def test_prior_skips_steps_while_an_output_bias_is_inf(cuda, mode):
    codes = [PW.to_dev(c) for c in PW.batches(2)]
    g, t = _prior(dict(skip_nonfinite=True)), _prior(dict(skip_nonfinite=True))
    for pr in (g, t):                                      # one clean step each (the capture's warm-up step)
        if mode == "eager":
            pr.train_step(codes[0])
        else:
            pr.capture_train_step(codes[0], warmup=1)
    _same(_prior_state(g), _prior_state(t))
    before = _prior_state(g)
    bias = g.prior.store.view(g.prior.out_bias)
    keep = bias[5].clone()
    bias[5] = float("inf")
    hole = (bias[5:6].data_ptr() - g.prior.store.flat.data_ptr()) // 4
    for i in range(2):
        res = g.train_step(codes[1])
        assert int(res["skipped_steps"]) == i + 1
    assert (g._captured is not None) == (mode == "replayed")
    after = _prior_state(g)
    assert float(after["weights"][hole]) == float("inf")
    after["weights"][hole] = before["weights"][hole]
    _same(before, after)                                   # every other weight, m, v, iterations, both trackers
    assert {k: int(v) for k, v in g.optimizer.skip_stats().items()} == dict(
        skipped_steps=2, consecutive_skipped=2, last_step_ok=0)
    assert g._step == t._step + 2                          # the host count is of attempted steps
    # the element restored: the next step is the twin's, given the same host step
    bias[5] = keep
    t._step = g._step
    res = g.train_step(codes[1])
    t.train_step(codes[1])
    _same(_prior_state(g), _prior_state(t))
    assert int(res["skipped_steps"]) == 2 and int(g.optimizer.skip_stats()["consecutive_skipped"]) == 0
    assert int(g.optimizer.iterations.item()) == 2 and bool(torch.isfinite(g.prior.store.flat).all())
    assert "skipped_steps" not in _prior(dict()).results()


# ---- data parallel: two gloo ranks on the one GPU
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(600)
def test_dp2_both_ranks_skip_when_one_rank_draws_a_nan(cuda, tmp_path):
    world, port, procs, outs = 2, _port(), [], []
    for r in range(world):
        out = str(tmp_path / f"skip_rank{r}.pt")
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VQA_DP_BATCH=str(W.B_LOCAL), VQA_DP_OVERLAP="0")
        # each rank a fresh child process under its own time limit
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable,
                                       os.path.join(HERE, "skip_dp_worker.py"), out], env=env))
        outs.append(out)
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0] * world, codes
    r0, r1 = (torch.load(o, weights_only=True) for o in outs)
    assert r0["local_input_finite"] and not r1["local_input_finite"]   # only rank 1 drew the NaN
    for r in (r0, r1):
        assert r["skips"] == dict(skipped_steps=1, consecutive_skipped=1, last_step_ok=0)
        assert int(r["before"]["iterations"]) == 1
        _same(r["before"], r["after"])
    _same(r0["after"], r1["after"], skip=("trackers",))
    assert bool(torch.isfinite(r0["after"]["weights"]).all())
