"""vqa_code_batch on the GPU against a numpy restatement of include/vqa.h's rule built from V.reset_perm_index,
bit-exact (the kernel only moves codes and widens them to int64).

The smallest shapes at which the kernel can still go wrong. Unconditioned: tracks of 148, 84 and 36 codes, windows
of n_ctx = 19 codes hopping by 3 — the starts 3 j cover every residue of a 16-byte chunk of int16 (8) and of int32
(4), row b of z starts 19 b int64 in, so rows alternate between a head of one code and none, and 19 - head is no
multiple of 8 or 4: non-empty tails. M = 44 + 22 + 6 = 72 windows, B = 3: S = 24 steps per epoch on one rank, 12 on
two. Conditioned: rate 4, upper tracks of 37, 21 and 9 codes under lower tracks of four times that, n_ctx = 20,
hop = 8, labels; M = 17 + 9 + 3 = 29. Sentinels surround every output buffer."""
import numpy as np
import pytest
import torch

import vqa_lib as V
from code_feed import CodeCorpus, CodeFeed

pytestmark = pytest.mark.gpu

SENT = -0x5A5A5A5A5A5A5A5A
PAD = 3                       # int64 before each buffer: rows start 8-byte but not 16-byte aligned


def _codes(K, lengths, seed):
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, K, n) for n in lengths]
    for a in out:
        a[0], a[-1] = K - 1, 0
    return out


@pytest.fixture(scope="module", params=[64, 40000], ids=["i16", "i32"])
def flat(request, cuda):
    K = request.param
    return CodeCorpus.from_codes([_codes(K, (148, 84, 36), 1)], None, [8], K, device=cuda)


@pytest.fixture(scope="module", params=[32768, 32769], ids=["i16", "i32"])
def cond(request, cuda):
    K = request.param
    up = (37, 21, 9)
    return CodeCorpus.from_codes([_codes(K, [4 * n for n in up], 2), _codes(K, up, 3)], (3, 0, 2), [8, 32], K,
                                 device=cuda)


class Guarded:
    """An int64 buffer with sentinels before and after it, at an 8-byte (not 16-byte) aligned offset."""

    def __init__(self, shape, device, pad=PAD):
        n = int(np.prod(shape))
        self.buf = torch.full((pad + n + 5,), SENT, dtype=torch.int64, device=device)
        self.t = self.buf[pad:pad + n].view(*shape)
        self.pad, self.n = pad, n

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.pad] == SENT) and np.all(b[self.pad + self.n:] == SENT))


def _guard(feed):
    """Swap the feed's buffers for guarded ones -> the guards."""
    dev = feed.codes.device
    g = {"codes": Guarded(feed.codes.shape, dev), "index": Guarded(feed.index.shape, dev, pad=1)}
    if feed.upper is not None:
        g["upper"] = Guarded(feed.upper.shape, dev, pad=1)
    if feed.y is not None:
        g["y"] = Guarded(feed.y.shape, dev)
    for k, v in g.items():
        setattr(feed, k, v.t)
    return g


def _ref(feed, g, rank=None):
    """codes, upper, labels, index of global step g by the rule in include/vqa.h."""
    c, l = feed.corpus, feed.level
    rank = feed.rank if rank is None else rank
    M, S = len(feed.starts_host), feed.steps_per_epoch
    epoch, pos = divmod(g, S)              # floor division: a negative g folds into [0, S) of epoch -1, -2, ...
    ks = [(pos * feed.world + rank) * feed.B + b for b in range(feed.B)]
    idx = [V.reset_perm_index(feed.seed, epoch, V.FEED_PERM_LEVEL, M, k) for k in ks] if feed.shuffle else ks
    lo = c.codes[l][:c.code_lens[l]].cpu().numpy().astype(np.int64)
    z = np.stack([lo[s:s + feed.n_ctx] for s in feed.starts_host[idx]])
    zu = None
    if feed.conditioned:
        up = c.codes[l + 1][:c.code_lens[l + 1]].cpu().numpy().astype(np.int64)
        n = feed.n_ctx // feed.rate
        zu = np.stack([up[s // feed.rate:s // feed.rate + n] for s in feed.starts_host[idx]])
    y = None if feed.labels_host is None else feed.labels_host[idx]
    return z, zu, y, np.asarray(idx, np.int64)


def _check(feed, guards, g, what=""):
    z, zu, y, idx = _ref(feed, g)
    assert feed.codes.dtype == torch.int64 and feed.codes.shape == (feed.B, feed.n_ctx)
    assert np.array_equal(feed.index.cpu().numpy(), idx), f"{what} step {g}: index"
    assert np.array_equal(feed.codes.cpu().numpy(), z), f"{what} step {g}: codes"
    if zu is not None:
        assert np.array_equal(feed.upper.cpu().numpy(), zu), f"{what} step {g}: upper"
    if y is not None:
        assert np.array_equal(feed.y.cpu().numpy(), y), f"{what} step {g}: labels"
    assert all(v.intact() for v in guards.values()), f"{what} step {g}: a sentinel was overwritten"
    return idx


# ---- unconditioned ---------------------------------------------------------------------------------------
def test_table_covers_every_residue(flat):
    f = CodeFeed(flat, 0, 19, 3, hop=3)
    assert len(f.starts_host) == 72 and f.steps_per_epoch == 24 and not f.conditioned
    assert sorted(set((f.starts_host % 8).tolist())) == list(range(8))
    assert flat.codes[0].dtype == (torch.int16 if flat.num_embeddings <= 32768 else torch.int32)


@pytest.mark.parametrize("shuffle", [True, False])
def test_unconditioned_steps_across_an_epoch_boundary(flat, shuffle):
    feed = CodeFeed(flat, 0, 19, 3, hop=3, seed=11, shuffle=shuffle)
    guards = _guard(feed)
    feed.counter.fill_(22)                                   # the counter carried over the boundary at 24
    seen = []
    for g in range(22, 27):
        out = feed.next()
        assert out[0] is feed.codes and out[1] is None and out[2] is None
        seen.append(_check(feed, guards, g, f"shuffle {shuffle}"))
        assert seen[-1].tolist() == feed.slots(g)
    assert feed.step == 27
    if not shuffle:
        assert seen[0].tolist() == [66, 67, 68] and seen[2].tolist() == [0, 1, 2]
    else:
        assert seen[2].tolist() != [0, 1, 2] or seen[3].tolist() != [3, 4, 5]


def test_a_whole_epoch_uses_every_window_once(flat):
    feed = CodeFeed(flat, 0, 19, 3, hop=3, seed=5)
    guards = _guard(feed)
    idx = np.concatenate([(feed.next(), _check(feed, guards, g))[1] for g in range(24)])
    assert sorted(idx.tolist()) == list(range(72))


def test_world2_ranks_draw_disjoint_slots(flat):
    feeds = [CodeFeed(flat, 0, 19, 3, hop=3, seed=11, rank=r, world=2) for r in (0, 1)]
    guards = [_guard(f) for f in feeds]
    assert all(f.steps_per_epoch == 12 for f in feeds)
    epoch = []
    for g in range(12):
        for f, gd in zip(feeds, guards):
            f.next()
            epoch.append(_check(f, gd, g, f"rank {f.rank}"))
    assert sorted(np.concatenate(epoch).tolist()) == list(range(72))   # disjoint within the epoch, all used
    for f, gd in zip(feeds, guards):                                    # and the next epoch is another permutation
        f.next()
        _check(f, gd, 12, f"rank {f.rank}")


@pytest.mark.parametrize("shuffle", [True, False])
def test_negative_counter_folds_into_the_table(flat, shuffle):
    feed = CodeFeed(flat, 0, 19, 3, hop=3, seed=2, shuffle=shuffle)
    guards = _guard(feed)
    feed.counter.fill_(-2)
    for g in (-2, -1, 0):
        feed.next()
        idx = _check(feed, guards, g, "negative")
        assert idx.min() >= 0 and idx.max() < 72
    assert feed.step == 1


def test_window_shorter_than_one_aligned_group(flat):
    """n_ctx = 1, hop 1: row b of z starts PAD + b int64 in (PAD odd), so the head is the whole row (1 = T) on rows 0
    and 2 and empty on row 1, whose code is the tail; no row holds an aligned group. Then, through the raw binding,
    window 1 of the unshuffled step 0 is made invalid (start -1): a zero and index -1 between two exact rows."""
    feed = CodeFeed(flat, 0, 1, 3, hop=1, seed=4)
    guards = _guard(feed)
    assert len(feed.starts_host) == 268 and feed.codes.data_ptr() % 16 == 8
    for g in range(3):
        feed.next()
        _check(feed, guards, g, "short")
    starts = feed.starts.clone()
    starts[1] = -1
    feed.codes.fill_(7)
    V.code_batch(flat.codes[0], flat.code_lens[0], starts, None, feed.codes, index_out=feed.index, seed=0,
                 counter=None, step=0, rank=0, world=1, shuffle=False)
    lo = flat.codes[0][:3].cpu().numpy().astype(np.int64)
    assert feed.index.cpu().tolist() == [0, -1, 2]
    assert feed.codes.cpu().numpy()[:, 0].tolist() == [lo[0], 0, lo[2]] and lo[0] == flat.num_embeddings - 1
    assert all(v.intact() for v in guards.values())


# ---- conditioned -----------------------------------------------------------------------------------------
def test_conditioned_rows_labels_and_index(cond):
    feed = CodeFeed(cond, 0, 20, 3, hop=8, seed=9)
    assert len(feed.starts_host) == 29 and feed.rate == 4 and feed.upper.shape == (3, 5)
    guards = _guard(feed)
    for g in range(11):                                      # S = 9: one boundary
        out = feed.next()
        assert out[1] is feed.upper and out[2] is feed.y
        _check(feed, guards, g, "conditioned")
    host = feed.host_batch(4)
    z, zu, y, _ = _ref(feed, 4)
    assert np.array_equal(host[0], z) and np.array_equal(host[1], zu) and np.array_equal(host[2], y)
    assert int(feed.codes.max()) < cond.num_embeddings and int(feed.codes.min()) >= 0


def test_bad_table_entries_are_zero_rows_and_never_read(cond):
    """Through the raw binding, unshuffled step 0 (windows 0..4): start 1 made misaligned (not a multiple of rate),
    start 3 leaving the lower corpus, start 4 negative — zero rows in z and z_upper, index -1, the other rows
    exact, nothing else written."""
    feed = CodeFeed(cond, 0, 20, 5, hop=8, shuffle=False)
    guards = _guard(feed)
    z, zu, y, _ = _ref(feed, 0)
    starts = feed.starts.clone()
    starts[1] += 2
    starts[3] = cond.code_lens[0] - 20 + 4
    starts[4] = -4
    feed.codes.fill_(7)
    feed.upper.fill_(7)
    V.code_batch(cond.codes[0], cond.code_lens[0], starts, feed.labels, feed.codes, upper=cond.codes[1],
                 upper_len=cond.code_lens[1], rate=4, z_upper=feed.upper, labels_out=feed.y, index_out=feed.index,
                 seed=0, counter=None, step=0, rank=0, world=1, shuffle=False)
    assert feed.index.cpu().tolist() == [0, -1, 2, -1, -1]
    got, gotu = feed.codes.cpu().numpy(), feed.upper.cpu().numpy()
    for b in range(5):
        if b in (1, 3, 4):
            assert not got[b].any() and not gotu[b].any()
        else:
            assert np.array_equal(got[b], z[b]) and np.array_equal(gotu[b], zu[b])
    assert np.array_equal(feed.y.cpu().numpy(), y)
    assert got.min() >= 0 and gotu.min() >= 0
    assert all(v.intact() for v in guards.values())
    # a window that fits the lower corpus but whose upper window leaves the upper corpus is invalid too
    V.code_batch(cond.codes[0], cond.code_lens[0], feed.starts, feed.labels, feed.codes, upper=cond.codes[1],
                 upper_len=4, rate=4, z_upper=feed.upper, labels_out=None, index_out=feed.index,
                 seed=0, counter=None, step=0, rank=0, world=1, shuffle=False)
    assert feed.index.cpu().tolist() == [-1] * 5 and not feed.codes.any() and not feed.upper.any()
    assert all(v.intact() for v in guards.values())


# ---- determinism, capture --------------------------------------------------------------------------------
def test_two_launches_from_the_same_counter_are_equal(cond):
    feed = CodeFeed(cond, 0, 20, 3, hop=8, seed=13)
    feed.counter.fill_(5)
    feed.next()
    first = [t.clone() for t in (feed.codes, feed.upper, feed.y, feed.index)]
    for t in (feed.codes, feed.upper, feed.y, feed.index):
        t.fill_(-1)
    feed.load_state_dict({"counter": 5, "seed": 13})
    feed.next()
    assert all(torch.equal(a, b) for a, b in zip(first, (feed.codes, feed.upper, feed.y, feed.index)))
    assert feed.state_dict() == {"counter": 6, "seed": 13}


def test_graph_replays_equal_eager_steps(cond):
    eager = CodeFeed(cond, 0, 20, 3, hop=8, seed=21)
    want = []
    for g in range(4):
        eager.next()
        want.append([t.clone() for t in (eager.codes, eager.upper, eager.y, eager.index)])
    feed = CodeFeed(cond, 0, 20, 3, hop=8, seed=21)
    feed.next()                                              # the kernels are loaded before the capture
    feed.load_state_dict({"counter": 0, "seed": 21})
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        feed.next()
    assert feed.step == 0                                    # a capture runs nothing
    for g in range(4):
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(want[g], (feed.codes, feed.upper, feed.y, feed.index)))
    assert feed.step == 4
