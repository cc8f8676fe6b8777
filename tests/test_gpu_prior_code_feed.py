"""The prior trained from a CodeFeed: feed steps equal tensor steps on the same batches, a step captured with the
feed (its gather launch and counter increment inside the hipGraph) equals the eager steps, fit / evaluate walk the
feed's epochs, and a feed that does not fit the prior is refused before anything is launched. Everything is compared
bitwise: the step's reductions run in a fixed order."""
import numpy as np
import pytest
import torch

from code_feed import CodeCorpus, CodeFeed
from prior import Prior

pytestmark = pytest.mark.gpu

K, RATE = 64, 4
UPPER = (80, 64, 72, 96)          # upper-level codes per track; the lower level holds four times as many
LABELS = (3, 0, 2, 3)
# one block of 64: the row attention takes blocks of a multiple of 64 codes, and head_dim = 128 / 4 / 2 = 16
PK = dict(width=128, depth=2, heads=2, blocks=1, attn_stacks=1, drop_out_rate=0.1)
CK = dict(dilation_factor=3, dilation_cycle=4, residual_width=32, residual_depth=4)


@pytest.fixture(scope="module")
def corpus(cuda):
    rng = np.random.default_rng(17)
    lo = [rng.integers(0, K, RATE * n) for n in UPPER]
    up = [rng.integers(0, K, n) for n in UPPER]
    return CodeCorpus.from_codes([lo, up], LABELS, [8, 32], K, device=cuda)


def _prior(seed=5, **kw):
    """Level 0 of two, 64 codes of context, conditioned on the 16 codes above them, 4 genres."""
    kw = {"genre_classes": 4, **kw}
    return Prior(0, [(64,), (16,)], K, [3, 2], [2, 2], None, PK, CK, dtype="fp32", device="cuda:0", seed=seed, **kw)


def _feed(corpus, seed=7, **kw):
    return CodeFeed(corpus, 0, n_ctx=64, batch_size=2, hop=32, seed=seed, **kw)


def _state(p):
    return [t.clone() for t in (p.prior.store.flat, p.optimizer.m, p.optimizer.v, p.optimizer.iterations)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def eager(corpus):
    """Three eager train_step(feed) calls from a fresh prior -> (state after them, loss)."""
    p, feed = _prior(), _feed(corpus)
    assert feed.steps_per_epoch >= 3 and feed.upper.shape == (2, 16) and feed.y is not None
    for _ in range(3):
        res = p.train_step(feed)
    torch.cuda.synchronize()
    assert feed.step == 3 and np.isfinite(float(res["loss"]))
    return _state(p), float(res["loss"])


def test_feed_steps_equal_tensor_steps(corpus, eager):
    p, feed = _prior(), _feed(corpus)
    for i in range(3):
        codes, upper, y = (torch.from_numpy(a).cuda() for a in feed.host_batch(i))
        res = p.train_step((codes, upper, y))
    torch.cuda.synchronize()
    assert _same(_state(p), eager[0]) and float(res["loss"]) == eager[1]
    assert feed.step == 0                                   # host_batch draws nothing


def test_the_feeds_buffers_are_the_steps_inputs(corpus):
    p, feed = _prior(), _feed(corpus)
    codes, upper, y = p._codes(feed)
    assert codes.data_ptr() == feed.codes.data_ptr() and upper.data_ptr() == feed.upper.data_ptr()
    assert y.data_ptr() == feed.y.data_ptr() and feed.step == 1
    want = feed.host_batch(0)
    assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip((codes, upper, y), want))


def test_captured_feed_step_equals_eager(corpus, eager):
    p, feed = _prior(), _feed(corpus)
    start = _state(p)
    trackers = [t._acc.clone() for t in p.metrics]
    p.capture_train_step(feed, warmup=1)                    # a real step on the feed's first batch
    assert feed.step == 1 and p._graph_feed is feed
    p.train_step(feed)
    res = p.train_step(feed)
    torch.cuda.synchronize()
    assert feed.step == 3
    assert _same(_state(p), eager[0]) and float(res["loss"]) == eager[1]
    # the initial state put back and the counter at 0: three replays walk the same three batches
    for dst, src in zip((p.prior.store.flat, p.optimizer.m, p.optimizer.v, p.optimizer.iterations), start):
        dst.copy_(src)
    for t, acc in zip(p.metrics, trackers):
        t._acc.copy_(acc)
    feed.load_state_dict({"counter": 0, "seed": feed.seed})
    for _ in range(3):
        res = p.train_step(feed)
    torch.cuda.synchronize()
    assert feed.step == 3 and torch.equal(feed.index.cpu(), torch.tensor(feed.slots(2)))
    assert _same(_state(p), eager[0]) and float(res["loss"]) == eager[1]
    # a second feed object runs eagerly and leaves the captured feed's counter alone
    other = _feed(corpus)
    before = _state(p)
    p.train_step(other)
    torch.cuda.synchronize()
    assert other.step == 1 and feed.step == 3 and not _same(_state(p), before)
    # tensors run eagerly too: a replay would overwrite them with the feed's next batch
    it = int(p.optimizer.iterations.item())
    p.train_step(tuple(torch.from_numpy(a).cuda() for a in feed.host_batch(0)))
    torch.cuda.synchronize()
    assert feed.step == 3 and int(p.optimizer.iterations.item()) == it + 1
    # and the captured feed still replays
    p.train_step(feed)
    assert feed.step == 4


@pytest.mark.parametrize("source", ["tensors", "feed"])
def test_capture_warmup_and_the_host_step_counter(corpus, source):
    """Prior._step (the checkpoint's "step") counts a warm-up step of capture_train_step only when the capture
    draws from a feed; the optimizer counts every warm-up step either way, and a replay counts once. The feed's
    device counter stands at 2 after the capture — the draw recorded into the graph is not executed, as
    test_captured_feed_step_equals_eager has it for warmup=1 — and at 3 after the first replay."""
    p, feed = _prior(), _feed(corpus)
    example = feed if source == "feed" else tuple(torch.from_numpy(a).cuda() for a in feed.host_batch(0))
    p.capture_train_step(example, warmup=2)
    assert int(p.optimizer.iterations.item()) == 2
    if source == "feed":
        assert p._step == 2 and feed.step == 2
    else:
        assert p._step == 0 and feed.step == 0
    before = p._step
    p.train_step(example)                                   # a replay
    torch.cuda.synchronize()
    assert p._step == before + 1 and int(p.optimizer.iterations.item()) == 3
    assert feed.step == (3 if source == "feed" else 0)


def test_unconditioned_top_level_fit_and_evaluate(corpus):
    """The top level of two with 64 codes of context (its tracks hold 80, 64, 72 and 96)."""
    p = Prior(1, [(256,), (64,)], K, [3, 2], [2, 2], None, PK, None, dtype="fp32", device="cuda:0", seed=3)
    train, val = corpus.split(0.25, seed=1)
    assert len(train) == 3 and len(val) == 1
    feed = CodeFeed(train, 1, n_ctx=64, batch_size=2, hop=4, seed=2)
    assert not feed.conditioned and feed.upper is None and feed.y is not None
    with pytest.raises(ValueError):
        p.fit(feed)                                         # labels, and the prior has no genre_classes
    p = Prior(1, [(256,), (64,)], K, [3, 2], [2, 2], None, PK, None, genre_classes=4, dtype="fp32", device="cuda:0",
              seed=3)
    hist = p.fit(feed, epochs=2)
    assert len(hist) == 2 and all(np.isfinite(h["loss"]) and np.isfinite(h["accuracy"]) for h in hist)
    assert feed.step == 2 * feed.steps_per_epoch
    vfeed = CodeFeed(val, 1, n_ctx=64, batch_size=2, hop=4, shuffle=False)
    w = p.prior.store.flat.clone()
    logs = p.evaluate(vfeed, return_dict=True)
    assert vfeed.step == vfeed.steps_per_epoch and np.isfinite(logs["loss"])
    p.test_step(vfeed)
    assert vfeed.step == vfeed.steps_per_epoch + 1
    assert torch.equal(w, p.prior.store.flat)               # evaluation trains nothing


def test_a_feed_that_does_not_fit_is_refused_before_any_launch(corpus):
    p = _prior()
    cases = {
        "no upper": _feed(corpus, conditioned=False),
        "n_ctx": CodeFeed(corpus, 0, n_ctx=32, batch_size=2, hop=32),
    }
    for what, feed in cases.items():
        for call in (p.train_step, p.test_step, p.capture_train_step, p.fit):
            with pytest.raises(ValueError):
                call(feed)
        assert feed.step == 0, what                         # nothing was drawn
    nolabel = _prior(genre_classes=None)
    feed = _feed(corpus)
    for call in (nolabel.train_step, nolabel.test_step, nolabel.capture_train_step, nolabel.fit):
        with pytest.raises(ValueError):
            call(feed)
    assert feed.step == 0 and int(nolabel.optimizer.iterations.item()) == 0
    assert int(p.optimizer.iterations.item()) == 0 and p._graph is None
    with pytest.raises(ValueError):
        p.fit(torch.zeros(2, 64, dtype=torch.int64))        # fit trains from a CodeFeed
