"""C-ABI checks of the corpus feed that need no GPU: vqa_corpus_batch settles its arguments on the host, so a bad
call returns VQA_E_INVALID_ARG with a "corpus_batch:" message before anything is launched (fake device pointers, as
tests/test_decode_primed_abi.py does), and the slot rule of include/vqa.h is checked through the host's
vqa_reset_perm_index against the oracle's restatement of the permutation."""
import ctypes

import numpy as np
import pytest
import torch

import vqa_lib as V
from audio_feed import AudioCorpus, AudioFeed
from code_feed import CodeCorpus, CodeFeed
from oracle import reset_perm

P = ctypes.c_void_p(0x1000)      # 16-byte aligned fake device pointer
ODD = ctypes.c_void_p(0x1008)    # 8-byte aligned only
GOOD = dict(corpus=P, corpus_len=1 << 20, pcm=0, starts=P, labels=P, M=64, x=P, labels_out=P, index_out=P, B=4,
            T=4096, seed=1, counter=P, step=0, rank=0, world=2, shuffle=1)
ORDER = ["corpus", "corpus_len", "pcm", "starts", "labels", "M", "x", "labels_out", "index_out", "B", "T", "seed",
         "counter", "step", "rank", "world", "shuffle"]


def _call(**kw):
    a = {**GOOD, **kw}
    return V.lib().vqa_corpus_batch(*[a[k] for k in ORDER], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(corpus=None), "null"),
    (dict(starts=None), "null"),
    (dict(x=None), "null"),
    (dict(B=0), "positive"),
    (dict(B=-3), "positive"),
    (dict(T=0), "positive"),
    (dict(M=0), "positive"),
    (dict(M=-1), "positive"),
    (dict(world=0), "world 0"),
    (dict(rank=-1), "rank -1 outside"),
    (dict(rank=2), "rank 2 outside"),
    (dict(M=7), "M 7 windows < B*world = 8"),
    (dict(pcm=2), "pcm 2"),
    (dict(pcm=-1), "pcm -1"),
    (dict(corpus=ODD), "16-byte aligned"),
    (dict(labels=None), "labels_out given without labels"),
])
def test_corpus_batch_rejects_bad_arguments_before_launch(kw, msg):
    rc = _call(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("corpus_batch:") and msg in err, err


def test_symbols_exported_and_steps_per_epoch():
    lib = V.lib()
    for s in ("vqa_corpus_batch", "vqa_corpus_steps_per_epoch"):
        assert s in V.EXPORTED and hasattr(lib, s)
    assert V.corpus_steps_per_epoch(11, 2, 2) == 2
    assert V.corpus_steps_per_epoch(12, 2, 2) == 3
    assert V.corpus_steps_per_epoch(3, 2, 2) == 0
    assert V.corpus_steps_per_epoch(1000, 32, 1) == 31
    assert V.corpus_steps_per_epoch(1 << 40, 32, 8) == (1 << 40) // 256
    assert V.corpus_steps_per_epoch(10, 0, 1) == 0 and V.corpus_steps_per_epoch(10, 2, 0) == 0
    assert V.FEED_PERM_LEVEL == 0x46454544 and (V.PCM_I16, V.PCM_F32) == (0, 1)


def _feeds(shuffle, seed=77):
    """M = 11 windows, B = 2, world = 2: S = 2 steps per epoch (3 windows of each epoch are dropped)."""
    tracks = [np.zeros(4 * 11, np.int16)]
    c = AudioCorpus.from_arrays(tracks, window=4, device="cpu")
    assert len(c) == 11
    return [AudioFeed(c, 2, seed=seed, shuffle=shuffle, rank=r, world=2) for r in (0, 1)]


def test_host_slot_rule():
    M, B, W, seed = 11, 2, 2, 77
    feeds = _feeds(True, seed)
    assert all(f.steps_per_epoch == 2 for f in feeds)
    per_epoch = {}
    for step in range(6):
        epoch, pos = divmod(step, 2)
        key = reset_perm.perm_key(seed, epoch, 0x46454544)
        for r, f in enumerate(feeds):
            ks = [(pos * W + r) * B + b for b in range(B)]
            want = reset_perm.perm_indices(key, M, ks).tolist()
            assert f.slots(step) == want
            assert f.slots(step) == feeds[0].slots(step, rank=r)
            per_epoch.setdefault(epoch, []).extend(want)
    for epoch, idx in per_epoch.items():  # within an epoch the S*B*world windows are distinct
        assert len(idx) == 8 and len(set(idx)) == 8 and all(0 <= i < M for i in idx)
    assert per_epoch[0] != per_epoch[1] and per_epoch[1] != per_epoch[2]


def test_audio_and_code_feeds_draw_the_same_slots():
    """include/vqa.h: vqa_code_batch resolves its window exactly as vqa_corpus_batch does. The same M = 11, B = 2,
    world = 2 and seed on both feeds: the same slots, which are the oracle's permutation of the rule's k."""
    M, B, W, seed = 11, 2, 2, 77
    codes = CodeCorpus.from_codes([[np.zeros(4 * M, np.int64)]], None, [8], 64, device="cpu")
    for r, audio in enumerate(_feeds(True, seed)):
        code = CodeFeed(codes, 0, 4, B, seed=seed, rank=r, world=W)
        assert len(code.starts_host) == M and code.steps_per_epoch == audio.steps_per_epoch == 2
        for step in range(6):
            epoch, pos = divmod(step, 2)
            ks = [(pos * W + r) * B + b for b in range(B)]
            want = reset_perm.perm_indices(reset_perm.perm_key(seed, epoch, 0x46454544), M, ks).tolist()
            assert audio.slots(step) == code.slots(step) == want
            assert audio.slots(step, rank=1 - r) == code.slots(step, rank=1 - r)


def test_host_slot_rule_sequential_without_shuffle():
    feeds = _feeds(False)
    got = [feeds[r].slots(step) for step in range(4) for r in (0, 1)]
    assert got == [[0, 1], [2, 3], [4, 5], [6, 7]] * 2


def test_feed_argument_checks():
    c = AudioCorpus.from_arrays([np.zeros(40, np.int16)], window=4, device="cpu")
    with pytest.raises(ValueError):
        AudioFeed(c, 11)            # 10 windows: no full step
    with pytest.raises(ValueError):
        AudioFeed(c, 2, rank=2, world=2)
    f = AudioFeed(c, 2, seed=5)
    assert (f.rank, f.world, len(f)) == (0, 1, 5)
    assert f.x.shape == (2, 4, 1) and f.x.dtype == torch.float32 and f.y is None
    with pytest.raises(V.VQAError):
        f.next()                    # a CPU corpus never reaches the kernel: device tensors only, no fallback
