"""Host-side parts of the code feed, no GPU: the chunk plan of the bounded-memory encode (encode_plan), the encoder's
halo against the fp64 oracle (a chunked run of the oracle's own encoder must reproduce its whole encode: the
arithmetic is identical, so only a halo that is too short can miss the bound), the checks of CodeCorpus.from_codes,
and the table arithmetic of CodeCorpus / CodeFeed on CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

from code_feed import CodeCorpus, CodeFeed
from oracle import vqvae_ref as R
from vqvae import decode_halo_for, encode_halo_for, encode_plan

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- encode_plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("total,chunk,halo,hop", [
    (40, 128, 3, 8),        # total < chunk: one chunk, nothing to widen
    (768, 128, 11, 8),      # a multiple of the chunk
    (800, 128, 11, 8),      # not a multiple: a short last core
    (776, 128, 40, 8),      # halo wider than a chunk
    (28, 4, 2, 4),          # chunk = one code
    (400, 64, 0, 8),        # halo = 0: input = core
    (1, 1, 0, 1),
    (9600, 1184, 13, 32),
])
def test_encode_plan_tiles_once_in_multiples_of_hop_and_clamps(total, chunk, halo, hop):
    plan = encode_plan(total, chunk, halo, hop)
    covered = np.zeros(total, np.int64)
    prev = 0
    for chunk_ in plan:
        in_lo, in_hi, core_lo, core_hi = chunk_
        assert all(v % hop == 0 for v in chunk_)
        assert core_lo == prev and core_lo < core_hi <= total and core_hi - core_lo <= chunk
        prev = core_hi
        covered[core_lo:core_hi] += 1
        assert in_lo == max(0, core_lo - halo * hop) and in_hi == min(total, core_hi + halo * hop)
    assert prev == total and np.array_equal(covered, np.ones(total, np.int64))
    assert len(plan) == -(-total // chunk) and plan[0][0] == 0 and plan[-1][1] == total


def test_encode_plan_cases_by_hand():
    assert encode_plan(96, 32, 1, 8) == [(0, 40, 0, 32), (24, 72, 32, 64), (56, 96, 64, 96)]
    assert encode_plan(16, 64, 5, 8) == [(0, 16, 0, 16)]


@pytest.mark.parametrize("total,chunk,halo,hop", [
    (0, 32, 1, 8), (-8, 32, 1, 8), (96, 0, 1, 8), (96, -32, 1, 8), (96, 32, -1, 8), (96, 32, 1, 0),
    (100, 32, 1, 8),   # total not a multiple of hop
    (96, 36, 1, 8),    # chunk not a multiple of hop
])
def test_encode_plan_rejects_bad_sizes(total, chunk, halo, hop):
    with pytest.raises(ValueError):
        encode_plan(total, chunk, halo, hop)


# ---- encode_halo against the fp64 oracle -----------------------------------------------------------------
def _micro_cfg():
    meta = json.load(open(os.path.join(HERE, "golden", "micro.json")))
    return R.RefConfig(**meta["config"])


ONE_LEVEL = R.RefConfig(input_len=768, levels=1, latent_dim=4, down_depth=[3], strides=[2], num_embeddings=32,
                        residual_width=8, residual_depth=3, dilation_factor=3)
CONFIGS = {"micro": _micro_cfg(), "one_level_d3": ONE_LEVEL}
CHUNK_CODES = 8


def _halo(cfg, level, fn=encode_halo_for):
    return fn(level, cfg.down_depth, cfg.strides, residual_width=cfg.residual_width,
              residual_depth=cfg.residual_depth, dilation_factor=cfg.dilation_factor, latent_dim=cfg.latent_dim)


def _hop(cfg, level):
    return int(np.prod([s ** d for s, d in zip(cfg.strides[:level + 1], cfg.down_depth[:level + 1])]))


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def oracle_case(request):
    cfg = CONFIGS[request.param]
    ref = R.RefVQVAE(cfg, R.init_params(cfg, 5), R.init_vq_state(cfg, 6), dtype=torch.float64)
    # biases are zero at init: random ones, so that a padded edge differs from a true interior
    rng = np.random.default_rng(11)
    for n in ref.p:
        if n.endswith("/bias"):
            ref.p[n] = torch.tensor(rng.uniform(-0.1, 0.1, size=tuple(ref.p[n].shape)), dtype=torch.float64)
    # long enough at every level that one core of CHUNK_CODES codes has both cuts in the interior:
    # in_lo > 0 and in_hi < total need (2 halo + 3 chunks) codes
    top = cfg.levels - 1
    codes = max(2 * _halo(cfg, l) + 3 * CHUNK_CODES + 1 for l in range(cfg.levels))
    T = -(-codes * max(_hop(cfg, l) for l in range(cfg.levels)) // _hop(cfg, top)) * _hop(cfg, top)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(2, T, 1)))
    return cfg, ref, x


def _chunked_max_diff(cfg, ref, x, level, halo):
    hop = _hop(cfg, level)
    T = x.shape[1]
    interior = 0
    with torch.no_grad():
        whole = ref.encoder(x, level)
        assert whole.shape[:2] == (x.shape[0], T // hop)
        worst = 0.0
        for in_lo, in_hi, core_lo, core_hi in encode_plan(T, CHUNK_CODES * hop, halo, hop):
            interior += in_lo > 0 and in_hi < T
            part = ref.encoder(x[:, in_lo:in_hi], level)
            core = part[:, (core_lo - in_lo) // hop:(core_hi - in_lo) // hop]
            worst = max(worst, float((core - whole[:, core_lo // hop:core_hi // hop]).abs().max()))
    return worst, interior


def test_encode_halo_covers_the_oracle_encoder(oracle_case):
    cfg, ref, x = oracle_case
    for level in range(cfg.levels):
        halo = _halo(cfg, level)
        assert halo > 0
        diff, interior = _chunked_max_diff(cfg, ref, x, level, halo)
        print(f"level {level}: halo {halo} codes, chunked vs whole max |diff| {diff:.3e}, {interior} interior chunks")
        assert interior >= 1, "no chunk with both cuts in the interior"
        assert diff <= 1e-12, (level, halo, diff)


def test_the_oracle_check_sees_a_short_halo(oracle_case):
    """The check above has teeth: with no halo at all the chunked oracle encode differs from the whole one."""
    cfg, ref, x = oracle_case
    assert _chunked_max_diff(cfg, ref, x, 0, 0)[0] > 1e-6


def test_encode_halo_values_by_hand():
    """micro level 0 (down_depth 2, stride 2: K = 4, pl = 1; residual depth 2, dilations [1, 3]): down
    max(ceil(1/2), floor(2/2)) = 1; block (1 + 1) + (3 + 1) -> 7; down max(ceil(8/2), floor(9/2)) = 4; block -> 10;
    proj -> 11 codes."""
    cfg = CONFIGS["micro"]
    assert _halo(cfg, 0) == 11
    # no dilation, depth 1, one stride-2 step: down 1, block 2 -> 3, proj -> 4 codes
    assert encode_halo_for(0, [1], [2], residual_width=8, residual_depth=1, dilation_factor=1, latent_dim=4) == 4
    # config 2 (down_depth [3, 2, 2], residual depth 4, dilation factor 3): as the decoder's, level by level
    for level, want in enumerate((79, 88, 90)):
        assert encode_halo_for(level, [3, 2, 2], [2, 2, 2], residual_width=64, residual_depth=4, dilation_factor=3) == want
        assert decode_halo_for(level, [3, 2, 2], [2, 2, 2], residual_width=64, residual_depth=4, dilation_factor=3) == want


# ---- CodeCorpus / CodeFeed on the host -------------------------------------------------------------------
UPPER, RATE, K = (37, 21, 9), 4, 64


def _tracks(seed=3, upper=UPPER, K=K):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, K, RATE * n) for n in upper], [rng.integers(0, K, n) for n in upper]]


def _corpus(labels=(5, 2, 5), K=K):
    return CodeCorpus.from_codes(_tracks(K=K), labels, [8, 32], K, device="cpu")


def test_from_codes_layout_and_storage():
    c = _corpus()
    assert [t.dtype for t in c.codes] == [torch.int16, torch.int16]
    assert c.code_lens == [RATE * sum(UPPER), sum(UPPER)]
    for l in range(2):
        assert c.codes[l].numel() * 2 % 16 == 0 and c.codes[l].numel() * 2 >= c.code_lens[l] * 2
        assert not c.codes[l][c.code_lens[l]:].any()                         # zero padded
    assert np.array_equal(c.offsets[0], RATE * c.offsets[1]) and c.rate(0) == RATE
    tr = _tracks()
    for l in range(2):
        for j in range(3):
            assert np.array_equal(c.track_codes(l, j).numpy(), tr[l][j])
    wide = CodeCorpus.from_codes(_tracks(K=40000), None, [8, 32], 40000, device="cpu")
    assert wide.codes[0].dtype == torch.int32 and wide.codes[0].numel() * 4 % 16 == 0
    assert CodeCorpus.from_codes(_tracks(K=32768), None, [8, 32], 32768, device="cpu").codes[0].dtype == torch.int16


def test_from_codes_rejects_mismatched_levels_and_codes_out_of_range():
    lo, up = _tracks()
    with pytest.raises(ValueError, match="do not agree with the hops"):
        CodeCorpus.from_codes([lo, [up[0], up[1][:-1], up[2]]], None, [8, 32], K, device="cpu")
    with pytest.raises(ValueError, match="do not agree with the hops"):
        CodeCorpus.from_codes([lo, up], None, [8, 16], K, device="cpu")       # the hops say rate 2, the lengths 4
    with pytest.raises(ValueError):
        CodeCorpus.from_codes([lo, up[:2]], None, [8, 32], K, device="cpu")   # a track missing at one level
    for bad in (K, -1):
        lo2 = [a.copy() for a in lo]
        lo2[1][7] = bad
        with pytest.raises(ValueError, match="outside"):
            CodeCorpus.from_codes([lo2, up], None, [8, 32], K, device="cpu")
    with pytest.raises(ValueError):
        CodeCorpus.from_codes([lo, up], [1, 2], [8, 32], K, device="cpu")     # two labels for three tracks


def test_window_table():
    c = _corpus()
    f = CodeFeed(c, 0, n_ctx=20, batch_size=2, hop=8)
    want, track = [], []
    for j, n in enumerate(UPPER):
        s = list(range(0, RATE * n - 20 + 1, 8))
        want += [int(c.offsets[0][j]) + v for v in s]
        track += [j] * len(s)
    assert f.starts_host.tolist() == want and f.track_host.tolist() == track
    assert [track.count(j) for j in range(3)] == [17, 9, 3]
    assert f.labels_host.tolist() == [(5, 2, 5)[j] for j in track]
    assert f.conditioned and f.rate == RATE and not np.any(f.starts_host % RATE)
    assert f.steps_per_epoch == 29 // 2 == len(f)
    assert (f.codes.shape, f.upper.shape, f.y.shape) == ((2, 20), (2, 5), (2,))
    assert f.codes.dtype == f.upper.dtype == f.y.dtype == f.index.dtype == torch.int64
    top = CodeFeed(c, 1, n_ctx=7, batch_size=3)                 # the top level: unconditioned, hop = n_ctx
    assert not top.conditioned and top.upper is None and top.rate == 1
    assert top.starts_host.tolist() == [0, 7, 14, 21, 28, 37, 44, 51, 58]
    codes, upper, y = f.host_batch(3)
    idx = f.slots(3)
    for b, i in enumerate(idx):
        s = f.starts_host[i]
        assert np.array_equal(codes[b], c.codes[0][s:s + 20].numpy())
        assert np.array_equal(upper[b], c.codes[1][s // 4:s // 4 + 5].numpy())
    assert y.tolist() == f.labels_host[idx].tolist()
    with pytest.raises(Exception):
        f.next()                                                # a CPU corpus never reaches the kernel: no fallback


def test_rate_alignment_and_other_constructor_errors():
    c = _corpus()
    with pytest.raises(ValueError, match="multiples of rate"):
        CodeFeed(c, 0, n_ctx=18, batch_size=2, hop=8)
    with pytest.raises(ValueError, match="multiples of rate"):
        CodeFeed(c, 0, n_ctx=20, batch_size=2, hop=6)
    assert CodeFeed(c, 0, n_ctx=18, batch_size=2, hop=3, conditioned=False).upper is None   # unconditioned: any
    with pytest.raises(ValueError):
        CodeFeed(c, 1, n_ctx=8, batch_size=2, conditioned=True)  # nothing above the top level
    with pytest.raises(ValueError):
        CodeFeed(c, 2, n_ctx=8, batch_size=2)
    with pytest.raises(ValueError):
        CodeFeed(c, 0, n_ctx=20, batch_size=30, hop=8)           # 29 windows: no full step
    with pytest.raises(ValueError):
        CodeFeed(c, 0, n_ctx=20, batch_size=2, hop=8, rank=2, world=2)


def test_save_load_round_trip(tmp_path):
    c = _corpus()
    c.save(tmp_path / "codes.npz")
    with np.load(tmp_path / "codes.npz", allow_pickle=False) as f:          # arrays only
        assert sorted(f.files) == ["codes0", "codes1", "hops", "labels", "lengths", "num_embeddings"]
    d = CodeCorpus.load(tmp_path / "codes.npz", device="cpu")
    assert d.hops == c.hops and d.num_embeddings == c.num_embeddings and d.code_lens == c.code_lens
    assert np.array_equal(d.track_labels, c.track_labels)
    for l in range(2):
        assert np.array_equal(d.lengths[l], c.lengths[l]) and torch.equal(d.codes[l], c.codes[l])
    sub = c.subset([2, 0])                                                   # a subset saves its own tracks
    sub.save(tmp_path / "sub.npz")
    e = CodeCorpus.load(tmp_path / "sub.npz", device="cpu")
    assert e.lengths[1].tolist() == [37, 9] and e.track_labels.tolist() == [5, 5]
    assert torch.equal(e.track_codes(0, 1), c.track_codes(0, 2))
    nolab = CodeCorpus.from_codes(_tracks(), None, [8, 32], K, device="cpu")
    nolab.save(tmp_path / "n.npz")
    assert CodeCorpus.load(tmp_path / "n.npz", device="cpu").track_labels is None


def test_split_is_by_track_and_shares_storage():
    rng = np.random.default_rng(9)
    upper = [int(n) for n in rng.integers(6, 30, 12)]
    labels = [j % 3 for j in range(12)]
    c = CodeCorpus.from_codes(_tracks(upper=upper), labels, [8, 32], K, device="cpu")
    train, test = c.split(0.25, seed=7)
    assert len(train) + len(test) == 12 and len(test) == 3 and not set(train.tracks) & set(test.tracks)
    assert sorted(c.track_labels[test.tracks].tolist()) == [0, 1, 2]          # stratified
    assert train.codes[0].data_ptr() == c.codes[0].data_ptr() == test.codes[0].data_ptr()
    ft, fv = (CodeFeed(s, 0, n_ctx=8, batch_size=1, hop=4) for s in (train, test))
    assert set(ft.track_host) == set(train.tracks) and set(fv.track_host) == set(test.tracks)
    assert not set(ft.starts_host) & set(fv.starts_host)
    assert len(ft.starts_host) + len(fv.starts_host) == len(CodeFeed(c, 0, 8, 1, hop=4).starts_host)
    again = c.split(0.25, seed=7)
    assert np.array_equal(again[1].tracks, test.tracks)
    inner_train, inner_test = train.split(0.34, seed=1)                      # a split of a split stays inside it
    assert set(inner_train.tracks) | set(inner_test.tracks) == set(train.tracks)
