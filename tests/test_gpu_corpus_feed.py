"""vqa_corpus_batch on the GPU against a numpy restatement of include/vqa.h's rule, bitwise (the kernel only moves
samples and scales int16 by 2^-15, which is exact in fp32, so there is no tolerance).

The smallest shapes at which the kernel can still go wrong: int16 tracks of 9003, 4099 and 4098 samples holding
+-full scale, windows of T = 4099 samples (odd: row b starts b*T floats into x, so its 16-byte alignment changes
from row to row and every head length 0..3 occurs) hopping by 613 (odd: the window starts 613*j cover all eight
residues of a 16-byte chunk of int16, and the second track starts at the odd offset 9003). That gives M = 10
windows — 9 from the first track (8*613 + 4099 = 9003, the shortest track with nine), 1 from the second, none from
the third, which is one sample short — so B = 5 gives S = 2 steps per epoch on one rank and S = 1 on two.
T = 4099 is two grid columns of the int16 kernel (2048 samples each) and four of the fp32 one."""
import numpy as np
import pytest
import torch

import vqa_lib as V
from audio_feed import AudioCorpus, AudioFeed
from oracle import reset_perm

pytestmark = pytest.mark.gpu

LENGTHS, T, HOP, B = (9003, 4099, 4098), 4099, 613, 5
LABELS = (3, 7, 1)
LEVEL = 0x46454544


def _tracks(dtype):
    rng = np.random.default_rng(2024)
    out = []
    for j, n in enumerate(LENGTHS):
        a = rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
        a[0], a[n // 2], a[-1], a[1] = -32768, 32767, -32768, 32767
        if dtype == "f32":  # values that are not multiples of 2^-15 either
            a = (a.astype(np.float32) / np.float32(32768)) + rng.standard_normal(n).astype(np.float32) * np.float32(1e-3)
        out.append(a)
    return out


@pytest.fixture(scope="module", params=["i16", "f32"])
def corpus(request, cuda):
    return AudioCorpus.from_arrays(_tracks(request.param), LABELS, window=T, hop=HOP, device=cuda)


def _ref(flat, starts, labels, T, B, seed, g, rank, world, shuffle):
    """x, labels_out, index_out of global step g by the rule in include/vqa.h."""
    M = len(starts)
    S = M // (B * world)
    epoch, pos = divmod(g, S)
    ks = np.array([(pos * world + rank) * B + b for b in range(B)])
    idx = reset_perm.perm_indices(reset_perm.perm_key(seed, epoch, LEVEL), M, ks) if shuffle else ks
    x = np.stack([flat[s:s + T] for s in starts[idx]])
    x = x.astype(np.float32) * np.float32(2.0 ** -15) if flat.dtype == np.int16 else x.astype(np.float32)
    return x, (None if labels is None else labels[idx]), idx.astype(np.int64)


def _host(c):
    return c.samples[:c.corpus_len].cpu().numpy(), c.starts_host, c.labels_host


def _check(feed, got, g, what=""):
    c = feed.corpus
    x, y, idx = _ref(*_host(c), c.window, feed.B, feed.seed, g, feed.rank, feed.world, feed.shuffle)
    gx, gy = got if isinstance(got, tuple) else (got, None)
    assert gx.shape == (feed.B, c.window, 1) and gx.dtype == torch.float32
    assert np.array_equal(feed.index.cpu().numpy(), idx), f"{what} step {g}: index"
    assert np.array_equal(gx.cpu().numpy()[:, :, 0].view(np.uint32), x.view(np.uint32)), f"{what} step {g}: x"
    if y is not None:
        assert np.array_equal(gy.cpu().numpy(), y), f"{what} step {g}: labels"
    return idx


def test_table(corpus):
    assert len(corpus) == 10
    assert np.bincount(corpus.track_host, minlength=3).tolist() == [9, 1, 0]
    assert sorted(set((corpus.starts_host % 8).tolist())) == list(range(8)) or corpus.dtype == torch.float32
    assert corpus.starts_host[9] == 9003 and corpus.corpus_len == sum(LENGTHS)
    assert corpus.samples.numel() * corpus.samples.element_size() % 16 == 0


def test_world1_crosses_two_epoch_boundaries(corpus):
    feed = AudioFeed(corpus, B, seed=11)
    assert feed.steps_per_epoch == 2
    seen = []
    for g in range(5):
        seen.append(_check(feed, feed.next(), g, "world 1"))
        assert seen[-1].tolist() == feed.slots(g)
    assert feed.step == 5
    for e in (0, 1):  # an epoch uses every window once; the epochs are permuted differently
        assert sorted(np.concatenate(seen[2 * e:2 * e + 2]).tolist()) == list(range(10))
    assert np.concatenate(seen[0:2]).tolist() != np.concatenate(seen[2:4]).tolist()


def test_world2_both_ranks(corpus):
    feeds = [AudioFeed(corpus, B, seed=11, rank=r, world=2) for r in (0, 1)]
    assert all(f.steps_per_epoch == 1 for f in feeds)
    for g in range(3):
        idx = [_check(f, f.next(), g, f"rank {f.rank}") for f in feeds]
        assert sorted(np.concatenate(idx).tolist()) == list(range(10))  # the ranks share the epoch's windows


def test_negative_counter_folds_into_the_table(corpus):
    """S = 2: g = -3 is pos 1 of epoch -2 (divmod floors, as the kernel's fold does), ..., g = 0 pos 0 of epoch 0."""
    feed = AudioFeed(corpus, B, seed=17)
    feed.counter.fill_(-3)
    for g in (-3, -2, -1, 0):
        idx = _check(feed, feed.next(), g, "negative")
        assert idx.min() >= 0 and idx.max() < 10
    assert feed.step == 1


def test_sequential_without_shuffle(corpus):
    feed = AudioFeed(corpus, B, shuffle=False)
    for g in range(3):
        idx = _check(feed, feed.next(), g, "sequential")
        assert idx.tolist() == [(g % 2) * B + b for b in range(B)]


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_fully_aligned_windows(cuda, dtype):
    """T = 4096, hop = 2048: every source chunk and every row of x is 16-byte aligned (no head, no tail)."""
    tr = [t[:n] for t, n in zip(_tracks(dtype), (8192, 4096, 4095))]
    c = AudioCorpus.from_arrays(tr, LABELS, window=4096, hop=2048, device=cuda)
    assert len(c) == 4
    feed = AudioFeed(c, 2, seed=5)
    for g in range(3):
        _check(feed, feed.next(), g, "aligned")


@pytest.mark.parametrize("pad", [4, 3])
def test_canaries_around_x(corpus, pad):
    """x inside a larger buffer, at a 16-byte aligned offset and at a 12-byte one: nothing before or after it is
    written, and the batch does not depend on x's alignment."""
    canary = float(np.float32(-12345.678))
    buf = torch.full((pad + B * T + 5,), canary, dtype=torch.float32, device=corpus.device)
    x = buf[pad:pad + B * T]
    index = torch.full((B,), -7, dtype=torch.int64, device=corpus.device)
    V.corpus_batch(corpus.samples, corpus.corpus_len, corpus.starts, corpus.labels, x.view(B, T), None, index,
                   seed=3, counter=None, step=3, rank=0, world=1, shuffle=True)
    want, _, idx = _ref(*_host(corpus), T, B, 3, 3, 0, 1, True)
    got = buf.cpu().numpy()
    assert np.all(got[:pad] == np.float32(canary)) and np.all(got[pad + B * T:] == np.float32(canary))
    assert np.array_equal(got[pad:pad + B * T].reshape(B, T).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(index.cpu().numpy(), idx)


@pytest.mark.parametrize("dtype", ["i16", "f32"])
def test_window_shorter_than_one_aligned_group(cuda, dtype):
    """T = 2, hop 1 over one track of 12 samples (M = 11), x one float into a canary buffer: row b starts 1 + 2 b
    floats in, so the heads up to the first 16-byte aligned output would be 3, 1, 3, 1, 3 samples and are clipped to
    T = 2; no row holds an aligned group, and the tail is what the head leaves (0, 1, 0, 1, 0 samples). Window 2 is
    made invalid (start -1): the zero fill at these sizes."""
    T2 = 2
    c = AudioCorpus.from_arrays([_tracks(dtype)[0][:12]], window=T2, hop=1, device=cuda)
    assert len(c) == 11
    canary = float(np.float32(-12345.678))
    buf = torch.full((1 + B * T2 + 5,), canary, dtype=torch.float32, device=cuda)
    x = buf[1:1 + B * T2]
    assert x.data_ptr() % 16 == 4
    starts = c.starts.clone()
    starts[2] = -1
    index = torch.full((B,), -7, dtype=torch.int64, device=cuda)
    V.corpus_batch(c.samples, c.corpus_len, starts, None, x.view(B, T2), None, index, seed=0, counter=None, step=0,
                   rank=0, world=1, shuffle=False)
    want, _, _ = _ref(*_host(c), T2, B, 0, 0, 0, 1, False)
    want[2] = 0
    got = buf.cpu().numpy()
    assert np.all(got[:1] == np.float32(canary)) and np.all(got[1 + B * T2:] == np.float32(canary))
    assert np.array_equal(got[1:1 + B * T2].reshape(B, T2).view(np.uint32), want.view(np.uint32))
    assert index.cpu().tolist() == [0, 1, -1, 3, 4]


def test_window_outside_the_corpus_is_zeroed_not_read(corpus):
    """Table entries corrupted to corpus_len - T + 1 (one sample past the last legal start) and to -1: their rows
    are zeros with index -1, the other rows are untouched by it."""
    starts = corpus.starts.clone()
    starts[1] = corpus.corpus_len - T + 1
    starts[3] = -1
    x = torch.full((B, T), 9.0, dtype=torch.float32, device=corpus.device)
    index = torch.zeros(B, dtype=torch.int64, device=corpus.device)
    y = torch.zeros(B, dtype=torch.int64, device=corpus.device)
    V.corpus_batch(corpus.samples, corpus.corpus_len, starts, corpus.labels, x, y, index, seed=0, counter=None,
                   step=0, rank=0, world=1, shuffle=False)
    want, labels, idx = _ref(*_host(corpus), T, B, 0, 0, 0, 1, False)
    got = x.cpu().numpy()
    assert index.cpu().tolist() == [0, -1, 2, -1, 4]
    assert np.array_equal(y.cpu().numpy(), labels)
    for b in range(B):
        if b in (1, 3):
            assert not got[b].any()
        else:
            assert np.array_equal(got[b].view(np.uint32), want[b].view(np.uint32))


def test_graph_replays_equal_eager_steps(corpus):
    eager = AudioFeed(corpus, B, seed=21)
    want = []
    for g in range(4):
        out = eager.next()
        want.append((out[0].clone(), out[1].clone(), eager.index.clone()))
    feed = AudioFeed(corpus, B, seed=21)
    feed.next()                                         # the kernels are loaded before the capture
    feed.load_state_dict({"counter": 0, "seed": 21})    # and the step is put back
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        feed.next()
    assert feed.step == 0                               # a capture runs nothing
    for g in range(4):
        graph.replay()
        assert torch.equal(feed.x, want[g][0]) and torch.equal(feed.y, want[g][1])
        assert torch.equal(feed.index, want[g][2])
        _check(feed, (feed.x, feed.y), g, "replay")
    assert feed.step == 4


def test_state_dict_resume(corpus):
    a = AudioFeed(corpus, B, seed=31)
    for _ in range(3):
        a.next()
    sd = a.state_dict()
    assert sd == {"counter": 3, "seed": 31}
    xa, ya = a.next()
    b = AudioFeed(corpus, B, seed=0)
    b.load_state_dict(sd)
    xb, yb = b.next()
    assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(a.index, b.index)
    _check(b, (xb, yb), 3, "resumed")
