"""The host side of prompted sampling (VQVAESampler.sample(prompt=...)) without a GPU: stand-in priors whose windows
draw a fixed function of (seed, row, step) and honour a prime as the persistent decode does, so the window plan, the
seeds, the slicing of codes and log-probabilities, best_of and every refusal are checked on the CPU."""
import types

import numpy as np
import pytest
import torch

from sampler import VQVAESampler, prompt_windows

BINS = 64


class _FakePrior:
    """A window's token at step i of row r is hash(seed, r, i) unless primed; its log-probability -(1 + token)."""

    def __init__(self, n_ctx, rate):
        self.context_length, self.device, self.calls = n_ctx, torch.device("cpu"), []
        self.prior = types.SimpleNamespace(start_token=BINS - 1, cond_downsample_rate=rate)

    def get_cond(self, zs, start, end):
        return None if not self.prior.cond_downsample_rate else (start, end)

    def sample(self, n_samples, z_cond=None, y=None, seed=0, prime=None, return_logprobs=False, **kw):
        have = 0 if prime is None else prime.shape[1]
        assert have < self.context_length  # a fully known window must not be launched
        self.calls.append((seed, have, z_cond))
        r = np.arange(n_samples)[:, None]
        i = np.arange(self.context_length)[None, :]
        tok = torch.from_numpy((seed * 7919 + r * 104729 + i * 31) % (BINS - 1)).long()
        lp = -(1.0 + tok.float())
        if have:
            tok[:, :have] = prime
            lp[:, :have] = 0.0
        seq = torch.cat([torch.full((n_samples, 1), BINS - 1, dtype=torch.int64), tok], dim=1)
        return (seq, (lp, lp * 2)) if return_logprobs else seq


def _sampler():
    return VQVAESampler([3, 2], [2, 2], [64, 16], codebook_size=BINS, priors=[_FakePrior(64, 4), _FakePrior(16, 0)])


N, SEED, TOTAL, TOTALS = 2, 9, 40, [160, 40]


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("p_top,skipped", [(5, 0), (16, 1), (27, 2), (39, 3), (1, 0)])
def test_prompt_plan_seeds_and_slices(p_top, skipped, lower):
    s = _sampler()
    zs, lps = s.sample(N, seed=SEED, total_length=TOTAL, return_logprobs=True)
    assert [tuple(z.shape) for z in zs] == [(N, t) for t in TOTALS]
    plain = [list(pr.calls) for pr in s.priors]
    assert [len(c) for c in plain] == [4, 4]
    for pr in s.priors:
        pr.calls.clear()
    prompt = [zs[0][:, :4 * p_top] if lower else None, zs[1][:, :p_top]]
    got, got_lps = s.sample(N, seed=SEED, total_length=TOTAL, return_logprobs=True, prompt=prompt)
    for level, pr in enumerate(s.priors):
        p = 0 if prompt[level] is None else prompt[level].shape[1]
        plan = prompt_windows(TOTALS[level], pr.context_length, pr.context_length // 2, p)
        assert len(plan) == 4 - (skipped if p else 0)
        # every window that ran kept the seed and the conditioning of its index
        assert pr.calls == [(plain[level][w][0], have, plain[level][w][2]) for w, _, have in plan]
        assert [c[0] for c in pr.calls] == [SEED + level + 2 * w for w, _, _ in plan]
        for k in range(2):
            g, want = got_lps[level][k], lps[level][k]
            assert g.shape == want.shape and not g[:, :p].any() and torch.equal(g[:, p:], want[:, p:])
    # the stand-in's tokens depend on the window's seed, so a draw is not reproduced by its prefix as the persistent
    # decode's is; the prefix and the shapes are
    for level in range(2):
        if prompt[level] is not None:
            assert torch.equal(got[level][:, :prompt[level].shape[1]], prompt[level])
        assert got[level].shape == zs[level].shape


def test_log_probabilities_come_from_the_window_that_drew():
    s = _sampler()
    zs, lps = s.sample(N, seed=SEED, total_length=TOTAL, return_logprobs=True, prompt=None)
    for level in range(2):
        assert torch.equal(lps[level][0], -(1.0 + zs[level].float()))
    got, got_lps = s.sample(N, seed=SEED, total_length=TOTAL, return_logprobs=True,
                            prompt=[zs[0][:, :108], zs[1][:, :27]])
    for level, p in ((0, 108), (1, 27)):
        want = -(1.0 + got[level].float())
        want[:, :p] = 0.0
        assert torch.equal(got_lps[level][0], want) and torch.equal(got_lps[level][1], want * 2)


def test_best_of_repeats_the_top_prompt_rows():
    s = _sampler()
    zs = s.sample(N, seed=SEED, total_length=TOTAL)
    prompt = [zs[0][:, :64], torch.stack([zs[1][0, :16], zs[1][1, :16] // 2])]
    got = s.sample(N, seed=SEED, total_length=TOTAL, prompt=prompt, best_of=3)
    assert [c[1] for c in s.priors[1].calls[-3:]] == [8, 8, 8]  # window 0 launched nothing, the others are primed
    for level in range(2):
        assert got[level].shape == (N, TOTALS[level])
        assert torch.equal(got[level][:, :prompt[level].shape[1]], prompt[level])


def test_one_window_prompt():
    s = _sampler()
    one = s.sample(N, seed=SEED)
    got = s.sample(N, seed=SEED, prompt=[one[0][:, :12], one[1][:, :3]])
    assert all(torch.equal(a, b) for a, b in zip(got, one))  # one window per level: the same seed, so the same draw
    assert [pr.calls[-1][1] for pr in s.priors] == [12, 3]


def _bad_prompts(z0, z1):
    token, negative = z1[:, :8].clone(), z1[:, :8].clone()
    token[1, 3] = BINS - 1
    negative[0, 0] = -1
    return [
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


def test_every_bad_prompt_is_a_value_error_before_any_launch():
    s = _sampler()
    z0, z1 = s.sample(N, seed=SEED, total_length=TOTAL)
    for pr in s.priors:
        pr.calls.clear()
    for prompt in _bad_prompts(z0, z1):
        with pytest.raises(ValueError, match="prompt"):
            s.sample(N, seed=SEED, total_length=TOTAL, prompt=prompt)
    with pytest.raises(ValueError, match="prompt"):
        s.sample(N, seed=SEED, prompt=[None, z1[:, :16]])  # one window of 16 codes: nothing left to draw
    with pytest.raises(ValueError, match="prompt"):
        s.sample(N, seed=SEED, total_length=TOTAL, prompt=[None, z1[:1, :8]], best_of=2)  # rows, before the repeat
    with pytest.raises(ValueError, match="prompt"):
        s.sample_level([z0[:, :0], z1], 0, seed=SEED, total_length=160, prompt=z0)
    assert [pr.calls for pr in s.priors] == [[], []]


def test_continue_audio_refusals_before_anything_runs():
    s = _sampler()

    class _NoVQVAE:
        levels, decode_hops = 2, [8, 32]

        def __getattr__(self, name):
            raise AssertionError(f"continue_audio reached for the VQ-VAE ({name}) before refusing")

    audio = torch.zeros(N, 100)
    with pytest.raises(ValueError, match="shorter than one top-level code"):
        s.continue_audio(audio[:, :31], _NoVQVAE(), total_length=TOTAL)
    with pytest.raises(ValueError, match="not shorter than the piece"):
        s.continue_audio(torch.zeros(N, 40 * 32 + 5), _NoVQVAE(), total_length=TOTAL)
    with pytest.raises(ValueError, match="float32"):
        s.continue_audio(audio.double(), _NoVQVAE(), total_length=TOTAL)
    with pytest.raises(ValueError, match="level"):
        s.continue_audio(audio, _NoVQVAE(), total_length=TOTAL, level=2)
    with pytest.raises(ValueError, match="prompt"):
        s.continue_audio(audio, _NoVQVAE(), total_length=TOTAL, prompt=[None, None])
    with pytest.raises(ValueError, match="levels"):
        s.continue_audio(audio, types.SimpleNamespace(levels=3, decode_hops=[8, 32, 128]), total_length=TOTAL)
    with pytest.raises(ValueError, match="hop lengths"):
        s.continue_audio(audio, types.SimpleNamespace(levels=2, decode_hops=[8, 16]), total_length=TOTAL)
    assert [pr.calls for pr in s.priors] == [[], []]
