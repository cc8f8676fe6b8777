"""Prompted long-form sampling (VQVAESampler.sample(prompt=...)) on the GPU.

The 2-level sampler of tests/test_gpu_render.py (down_depth [3, 2], n_ctxs [64, 16], 64 bins, random weights; level 0
conditioned on level 1), N = 2. total_length = 40 top-level codes gives 160 / 40 codes in four windows per level
(starts 0 32 64 96 and 0 8 16 24). As in a trained model the start token (bin 63) is never drawn: its output bias is
-1e4, so every prefix of a draw is a valid prompt. One unprompted draw with log-probabilities is shared; a prompt cut
from it must give it back bit for bit, since the persistent decode's noise is keyed by the absolute step. Prompt
lengths, in top-level codes (four times as many on level 0): 5 ends inside window 0, 16 exactly on window 0's end
(one window per level launches nothing), 27 past window 1's end (two per level launch nothing).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]

pytestmark = pytest.mark.gpu

BINS, N, SEED, TOTAL = 64, 2, 9, 40
TOTALS, RATE = [160, 40], 4
CASES = [(5, 0), (16, 1), (27, 2)]  # (top-level prompt length, windows per level that launch nothing)
_DRAW = []


def _draw():
    """(sampler, codes, log-probabilities) of the unprompted scored draw, made once."""
    if not _DRAW:
        from sampler import VQVAESampler
        s = VQVAESampler([3, 2], [2, 2], [64, 16], codebook_size=BINS, dtype="fp32", device="cuda", seed=4)
        for pr in s.priors:
            pr.prior.store.view(pr.prior.out_bias)[-1] = -1e4
        zs, lps = s.sample(N, seed=SEED, total_length=TOTAL, return_logprobs=True)
        torch.cuda.synchronize()
        assert [tuple(z.shape) for z in zs] == [(N, t) for t in TOTALS]
        assert all(0 <= int(z.min()) and int(z.max()) < BINS - 1 for z in zs)
        _DRAW.append((s, zs, lps))
    return _DRAW[0]


class _Launches:
    """Counts the decode launches that go through vqa_lib.prior_decode."""

    def __init__(self, monkeypatch):
        import vqa_lib as V
        self.n, real = 0, V.prior_decode

        def counted(*a, **kw):
            self.n += 1
            return real(*a, **kw)

        monkeypatch.setattr(V, "prior_decode", counted)


def _prompt(zs, p_top, lower=True):
    return [zs[0][:, :p_top * RATE] if lower else None, zs[1][:, :p_top]]


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("p_top,skipped", CASES)
def test_a_prompt_cut_from_a_draw_gives_the_draw_back(cuda, monkeypatch, p_top, skipped, lower):
    s, zs, _ = _draw()
    count = _Launches(monkeypatch)
    plain = s.sample(N, seed=SEED, total_length=TOTAL)
    assert count.n == 8 and all(torch.equal(a, b) for a, b in zip(plain, zs))
    count.n = 0
    got = s.sample(N, seed=SEED, total_length=TOTAL, prompt=_prompt(zs, p_top, lower))
    for level in range(2):
        assert got[level].dtype == torch.int64 and torch.equal(got[level], zs[level]), level
    assert count.n == 8 - skipped * (2 if lower else 1)


@pytest.mark.parametrize("p_top,skipped", CASES)
def test_log_probabilities_are_zero_on_the_prompt_and_the_draw_s_elsewhere(cuda, p_top, skipped):
    s, zs, lps = _draw()
    got, got_lps = s.sample(N, seed=SEED, total_length=TOTAL, prompt=_prompt(zs, p_top), return_logprobs=True)
    for level, p in ((0, p_top * RATE), (1, p_top)):
        assert torch.equal(got[level], zs[level])
        for k in range(2):
            g, want = got_lps[level][k], lps[level][k]
            assert g.shape == want.shape == (N, TOTALS[level]) and g.dtype == torch.float32
            assert int((g[:, :p] != 0).sum()) == 0, (level, k)
            assert torch.equal(g[:, p:], want[:, p:]), (level, k)  # bitwise
            assert bool((want[:, p:] < 0).any())


@pytest.mark.parametrize("p_top", [5, 27])
def test_another_prompt_comes_back_as_the_prefix(cuda, p_top):
    s, zs, _ = _draw()
    g = torch.Generator().manual_seed(3)
    prompt = [torch.randint(0, BINS - 1, (N, p_top * RATE), generator=g).cuda(),
              torch.randint(0, BINS - 1, (N, p_top), generator=g).cuda()]
    got = s.sample(N, seed=SEED, total_length=TOTAL, prompt=prompt)
    for level in range(2):
        p = prompt[level].shape[1]
        assert got[level].shape == (N, TOTALS[level])
        assert torch.equal(got[level][:, :p], prompt[level])
        assert 0 <= int(got[level].min()) and int(got[level].max()) < BINS - 1
    again = s.sample(N, seed=SEED, total_length=TOTAL, prompt=[z.cpu() for z in prompt])  # host prompts are taken too
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_best_of_two_keeps_the_prompt_on_the_winners(cuda, monkeypatch):
    s, zs, _ = _draw()
    prompt = _prompt(zs, 16)
    count = _Launches(monkeypatch)
    got, lps = s.sample(N, seed=SEED, total_length=TOTAL, prompt=prompt, best_of=2, return_logprobs=True)
    assert count.n == 6
    for level in range(2):
        p = prompt[level].shape[1]
        assert got[level].shape == (N, TOTALS[level]) and torch.equal(got[level][:, :p], prompt[level])
        assert int((lps[level][0][:, :p] != 0).sum()) == 0
    # candidate row s K of sample s draws what the plain call's row s K draws; the winners are rows of that batch
    empty = torch.zeros(N * 2, 0, dtype=torch.int64, device="cuda")
    both = s.sample_level([empty, empty], 1, seed=SEED, total_length=TOTAL, hop_length=8,
                          prompt=prompt[1].repeat_interleave(2, dim=0))
    for i in range(N):
        assert any(torch.equal(got[1][i], both[1][2 * i + k]) for k in range(2)), i


def test_one_window_prompt(cuda):
    """total_length=None: one window per level, primed with the prompt."""
    s, _, _ = _draw()
    one = s.sample(N, seed=SEED)
    got = s.sample(N, seed=SEED, prompt=[one[0][:, :12], one[1][:, :3]])
    assert all(torch.equal(a, b) for a, b in zip(got, one))


def test_every_bad_prompt_is_a_value_error_before_any_launch(cuda, monkeypatch):
    s, zs, _ = _draw()
    count = _Launches(monkeypatch)
    z0, z1 = zs
    token, negative = z1[:, :8].clone(), z1[:, :8].clone()
    token[1, 3] = BINS - 1
    negative[0, 0] = -1
    bad = [
        [z1[:, :8]],                                  # one entry for two levels
        [z0[:, :32], z1[:, :8], None],
        z1[:, :8],                                    # not a list
        [z0[:1, :32], z1[:1, :8]],                    # rows
        [None, z1[:, :0]],                            # empty
        [None, z1],                                   # nothing left to draw
        [z0, None],
        [z0[:, :33], z1[:, :8]],                      # not in the ratio of the hops
        [z0[:, :8], z1[:, :8]],
        [None, token],                                # the start token
        [None, negative],
        [None, z1[:, :8].to(torch.int32)],
        [None, z1[0, :8]],
    ]
    for prompt in bad:
        with pytest.raises(ValueError, match="prompt"):
            s.sample(N, seed=SEED, total_length=TOTAL, prompt=prompt)
    with pytest.raises(ValueError, match="prompt"):
        s.sample(N, seed=SEED, prompt=[None, z1[:, :16]])  # one window of 16 codes: nothing left to draw
    with pytest.raises(ValueError, match="prompt"):
        s.sample_level([z0[:, :0], z1], 0, seed=SEED, total_length=160, prompt=token.repeat(1, 4))
    with pytest.raises(ValueError, match="prompt"):
        s.sample(N, seed=SEED, total_length=TOTAL, prompt=[None, z1[:1, :8]], best_of=2)  # rows, before the repeat
    assert count.n == 0
