"""GPU checks of the step guard's kernels: vqa_grad_finite, vqa_adam_keras_guarded with vqa_counter_add_if, and
vqa_vq_ema_apply_guarded. Everything is compared bitwise: the flag with numpy.isfinite(...).all(), an applied step
with the unguarded entry point's result from identical inputs, a skipped step with the buffers as they were.

vqa_grad_finite's sizes: 1, 3 (a tail only), 4 (one group of four), 5, 1023, 1024 * 4 * 2 + 1 (several workgroups and
a tail) and CAP + 1 with CAP = VQA_FINITE_MAX_BLOCKS * 256 * 4, one float more than one sweep of the capped grid
covers, so the grid-stride loop goes round again. Each on a 16-byte aligned buffer and on one offset by one float.
The loop runs over units, first the groups of four behind the head, then the head's and the tail's single floats
(_second_trip restates that to find the element the second trip starts with).
"""
import numpy as np
import pytest
import torch

import vqa_lib as V
from vqa_optim import clip_tables

pytestmark = pytest.mark.gpu

SWEEP = V.FINITE_MAX_BLOCKS * 256       # units one sweep of the capped grid covers
CAP = SWEEP * 4
SIZES = [1, 3, 4, 5, 1023, 1024 * 4 * 2 + 1, CAP + 1]
BAD = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def _layout(n, shift):
    """(head, n4, tail0) of a buffer whose first float sits `shift` floats behind a 16-byte boundary."""
    head = min((4 - shift) % 4, n)
    n4 = (n - head) // 4
    return head, n4, head + 4 * n4


def _second_trip(n, shift):
    """The element that unit SWEEP, the first of the second grid-stride trip, reads first (None: one trip)."""
    head, n4, tail0 = _layout(n, shift)
    if n4 + head + (n - tail0) <= SWEEP:
        return None
    if SWEEP < n4:
        return head + 4 * SWEEP
    j = SWEEP - n4
    return j if j < head else tail0 + (j - head)


def _positions(n, shift):
    """Where the bad value goes: the first element, the last, the scalar tail's first, the second trip's first."""
    head, n4, tail0 = _layout(n, shift)
    pos = {"first": 0, "last": n - 1}
    if tail0 < n:
        pos["tail"] = tail0
    if _second_trip(n, shift) is not None:
        pos["second-trip"] = _second_trip(n, shift)
    return pos


def test_the_largest_size_takes_a_second_trip_on_both_alignments():
    for shift in (0, 1):
        assert _second_trip(CAP + 1, shift) is not None and _second_trip(1024 * 4 * 2 + 1, shift) is None
        assert "tail" in _positions(CAP + 1, shift)


@pytest.fixture(scope="module")
def clean(cuda):
    """One finite buffer for every size and alignment (never written except for one element, put back)."""
    g = torch.Generator().manual_seed(5)
    return (torch.rand(CAP + 8, generator=g) - 0.5).to(cuda)


def _flag(buf, ok):
    V.grad_finite(buf, ok)
    torch.cuda.synchronize()
    return int(ok.item())


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_finite_equals_numpy_isfinite(cuda, clean, n, shift):
    buf = clean[shift:shift + n]
    assert buf.data_ptr() % 16 == 4 * shift
    ok = torch.full((1,), 7, dtype=torch.int32, device=cuda)
    assert _flag(buf, ok) == 1 == int(np.isfinite(buf.cpu().numpy()).all())
    for where, i in _positions(n, shift).items():
        for name, bad in BAD.items():
            keep = buf[i].clone()
            buf[i] = bad
            want = int(np.isfinite(buf.cpu().numpy()).all())
            got = _flag(buf, ok)
            buf[i] = keep
            assert got == want == 0, (n, shift, where, i, name)
        # the flag keeps nothing: a clean call after a 0 gives 1
        assert _flag(buf, ok) == 1, (n, shift, where)
    # the neighbours of the buffer do not count
    if shift:
        keep = clean[shift - 1].clone()
        clean[shift - 1] = float("nan")
        got = _flag(buf, ok)
        clean[shift - 1] = keep
        assert got == 1
    keep = clean[shift + n].clone()
    clean[shift + n] = float("inf")
    got = _flag(buf, ok)
    clean[shift + n] = keep
    assert got == 1


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset1"])
def test_large_finite_values_denormals_and_negative_zero_are_finite(cuda, shift):
    vals = np.array([3.4e38, -3.4e38, 1e-45, -1e-40, -0.0, 0.0, 1.0, np.finfo(np.float32).max,
                     np.finfo(np.float32).tiny, 2.0, -7.5], np.float32)
    assert np.isfinite(vals).all() and np.signbit(vals[4]) and 0 < vals[2] < np.finfo(np.float32).tiny
    store = torch.zeros(vals.size + shift, device=cuda)
    buf = store[shift:]
    buf.copy_(torch.from_numpy(vals))
    ok = torch.zeros(1, dtype=torch.int32, device=cuda)
    assert _flag(buf, ok) == 1
    buf[0] = float("inf")
    assert _flag(buf, ok) == 0
    buf[0] = 3.4e38
    assert _flag(buf, ok) == 1


# ---- the guarded update
LR, B1, B2, EPS, GS = 1e-2, 0.9, 0.999, 1e-7, 0.5
AVG = (0.9, 0, False)
COMBOS = ["plain", "ema", "clipped", "clipped_ema"]


class _Opt:
    """Device buffers of one optimizer at size n, identical for equal (n, seed); step() takes one update through the
    unguarded entry point of the combination or through the guarded one."""

    def __init__(self, cuda, n, combo, seed=0):
        rng = np.random.default_rng(300 + seed)
        f = lambda s: torch.from_numpy((rng.standard_normal(n) * s).astype(np.float32)).to(cuda)
        self.w, self.g, self.m, self.v, self.a = f(0.05), f(2.0), f(0.5), f(1.0).abs(), f(0.05)
        self.step_count = torch.full((1,), 3, dtype=torch.int64, device=cuda)
        self.ok = torch.ones(1, dtype=torch.int32, device=cuda)
        self.skips = torch.zeros(2, dtype=torch.int64, device=cuda)
        self.ema = AVG if "ema" in combo else None
        self.clip = None
        if "clipped" in combo:
            offsets = {str(o): (o, (1,)) for o in (0, 516, 2052) if o < n}
            seg, block_seg = clip_tables(offsets, n)
            self.seg, self.block_seg = torch.from_numpy(seg).to(cuda), torch.from_numpy(block_seg).to(cuda)
            self.seg_norm = torch.zeros(len(seg), device=cuda)
            self.stats = torch.zeros(V.CLIP_STATS, device=cuda)
            self.ws = V.workspace(V.grad_norm_workspace(n, len(seg)), cuda)
            self.modes, self.thr = V.CLIP_VALUE | V.CLIP_NORM, (0.8, 5.0, 0.0)
            self.clip = (self.seg, self.block_seg, self.modes, *self.thr, self.seg_norm, self.stats)

    def step(self, guarded):
        head = (self.w, self.g, self.m, self.v, self.step_count, LR, B1, B2, EPS, GS)
        if self.clip:
            V.grad_norm(self.g, self.seg, self.block_seg, GS, self.modes, *self.thr, self.seg_norm, self.stats, self.ws)
        if guarded:
            V.adam_keras_guarded(*head, self.ok, self.skips, clip=self.clip,
                                 ema=(self.a, *self.ema) if self.ema else None)
            V.counter_add_if(self.step_count, self.ok)
            return
        if self.clip and self.ema:
            V.adam_keras_clipped_ema(*head, *self.clip, self.a, *self.ema)
        elif self.clip:
            V.adam_keras_clipped(*head, *self.clip)
        elif self.ema:
            V.adam_keras_ema(*head, self.a, *self.ema)
        else:
            V.adam_keras(*head)
        V.counter_add(self.step_count, 1)

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).clone() for k in ("w", "m", "v", "a", "step_count")}


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [5, 4 * 256 * 4 + 3])
@pytest.mark.parametrize("combo", COMBOS)
def test_an_applied_step_equals_the_unguarded_entry_point_bitwise(cuda, combo, n):
    ref, dev = _Opt(cuda, n, combo), _Opt(cuda, n, combo)
    _same(ref.state(), dev.state())
    dev.skips.copy_(torch.tensor([6, 2]))
    for _ in range(2):
        ref.step(False)
        dev.step(True)
        sr, sd = ref.state(), dev.state()
        _same(sr, sd)
        assert dev.skips.tolist() == [6, 0]           # the total unchanged, the run of skips ended
    assert int(sd["step_count"]) == 5 and not torch.equal(sd["w"], _Opt(cuda, n, combo).w)
    if "ema" not in combo:
        assert torch.equal(sd["a"], _Opt(cuda, n, combo).a)   # no average: the buffer is not touched


@pytest.mark.parametrize("n", [5, 4 * 256 * 4 + 3])
@pytest.mark.parametrize("combo", COMBOS)
def test_a_skipped_step_writes_nothing_and_counts(cuda, combo, n):
    ref, dev = _Opt(cuda, n, combo), _Opt(cuda, n, combo)
    before = dev.state()
    dev.g[n // 2] = float("nan")
    V.grad_finite(dev.g, dev.ok)
    dev.step(True)
    _same(before, dev.state())
    assert dev.skips.tolist() == [1, 1] and int(dev.ok.item()) == 0
    dev.g[0] = float("-inf")
    dev.step(True)                                    # the flag is still 0
    _same(before, dev.state())
    assert dev.skips.tolist() == [2, 2] and int(dev.step_count.item()) == 3
    # a good step after two skips: the very step the unguarded entry point takes from the untouched state
    dev.g.copy_(ref.g)
    V.grad_finite(dev.g, dev.ok)
    dev.step(True)
    ref.step(False)
    _same(ref.state(), dev.state())
    assert dev.skips.tolist() == [2, 0] and int(dev.ok.item()) == 1 and int(dev.step_count.item()) == 4


def test_any_flag_value_but_one_skips(cuda):
    dev = _Opt(cuda, 37, "plain")
    before = dev.state()
    for i, val in enumerate((0, 2, -1)):
        dev.ok.fill_(val)
        dev.step(True)
        _same(before, dev.state())
        assert dev.skips.tolist() == [i + 1, i + 1]


# ---- the guarded codebook update
def _codebook(cuda, D, K, seed):
    g = torch.Generator().manual_seed(seed)
    E = (torch.rand(D, K, generator=g) - 0.5) * 0.1
    n_sum = torch.zeros(K)
    n_sum[: max(K // 3, 1)] = torch.randint(1, 50, (max(K // 3, 1),), generator=g).float()
    stats = torch.cat([(torch.randn(K, D, generator=g) * n_sum[:, None]).reshape(-1), n_sum,
                       torch.randn(K * D, generator=g)]).to(cuda)
    st = dict(E=E.to(cuda), ET=E.t().contiguous().to(cuda), m_t=E.clone().to(cuda), N_t=torch.ones(K, device=cuda),
              metrics=torch.full((3,), 0.25, device=cuda), calls=torch.full((1,), 4, dtype=torch.int64, device=cuda),
              esq=torch.full((K,), 0.5, device=cuda), E3=torch.ones(K, 3, D, dtype=torch.bfloat16, device=cuda))
    return st, stats


def _apply(st, stats, D, K, ok=None):
    V.vq_ema_apply(st["E"], st["ET"], st["m_t"], st["N_t"], stats[:K * D].view(K, D), stats[K * D:K * D + K],
                   stats[K * D + K:].view(K, D), float(np.float32(0.99)), float(np.float32(1 - 0.99)), 1.0,
                   st["metrics"], st["calls"], esq=st["esq"], E3=st["E3"], ok=ok)
    torch.cuda.synchronize()


# D = K = 1: the smallest codebook the kernel takes; (32, 70): 18 workgroups of four codes, the last one partial;
# (64, 2048): the benched codebook
@pytest.mark.parametrize("D,K", [(1, 1), (32, 70), (64, 2048)])
def test_guarded_codebook_update(cuda, D, K):
    ok = torch.zeros(1, dtype=torch.int32, device=cuda)
    region = lambda stats: stats[:K * D + K]          # m_sumT | n_sum: what the rule reads (not the reset rows)
    # clean statistics: bitwise vqa_vq_ema_apply's outputs
    ref, stats = _codebook(cuda, D, K, 3)
    dev, _ = _codebook(cuda, D, K, 3)
    _apply(ref, stats, D, K)
    V.grad_finite(region(stats), ok)
    _apply(dev, stats, D, K, ok=ok)
    assert int(ok.item()) == 1 and int(dev["calls"].item()) == 5
    for k in ref:
        assert torch.equal(ref[k], dev[k]), k
    assert not torch.equal(dev["E"], _codebook(cuda, D, K, 3)[0]["E"])
    # a NaN in n_sum only, an inf in one m_sumT element only: every output as it was, `calls` included
    for where, bad in ((K * D + K - 1, float("nan")), ((K * D) // 2, float("inf"))):
        dev, stats = _codebook(cuda, D, K, 3)
        before = {k: v.clone() for k, v in dev.items()}
        stats[where] = bad
        V.grad_finite(region(stats), ok)
        _apply(dev, stats, D, K, ok=ok)
        assert int(ok.item()) == 0
        for k in before:
            assert torch.equal(before[k], dev[k]), (where, k)
    # a non-finite reset row is not part of the rule: the update runs
    dev, stats = _codebook(cuda, D, K, 3)
    stats[-1] = float("nan")
    V.grad_finite(region(stats), ok)
    _apply(dev, stats, D, K, ok=ok)
    assert int(ok.item()) == 1 and int(dev["calls"].item()) == 5
