"""CPU-only side of the VQ-VAE kernel-parity suites (tests/vqvae_parity_ref.py): the planted-code inputs meet their
own conditions on every row of every shape the GPU tests use, the checks can fail (a reference perturbed the way a
kernel goes wrong lands outside the bound it is checked with, where the criteria they replace let it pass), and the
fp32 restatements agree with their fp64 forms to fp32 rounding."""
import pytest
import torch

import vqvae_parity_ref as R

DTS = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D,K,N", R.ARGMIN_SHAPES + R.SPLIT_SHAPES)
def test_planted_codes_answer_is_the_planted_code_on_every_row(D, K, N, dt):
    """A condition of the GPU tests, not a measurement: they leave out no row."""
    z, E, amin, margin, dmin = R.planted_codes(D, K, N, dt)
    assert z.dtype == dt and E.dtype == torch.float32
    assert torch.equal(amin, torch.arange(N) % K)
    assert bool(R.clear_margin(margin, dmin).all())
    assert N >= K and int(amin.max()) == K - 1        # every code, the last one included, is some row's answer


def test_split_shapes_take_the_paths_the_gpu_test_names():
    want = {(32, 70, 300): (2, 64), (64, 129, 257): (3, 64), (64, 2048, 2100): (32, 64), (32, 64, 300): (1, 64)}
    for D, K, N in R.SPLIT_SHAPES:
        assert R.split_spans(N, K) == want[(D, K, N)]
    assert R.split_spans(300, 64)[0] == 1              # the non-finite rows' unpacked case (K = 64)
    assert R.split_spans(300, 2048)[0] > 1             # ... and their packed one
    assert R.split_spans(262144, 2048) == (1, 2048)    # the benchmark's level 0: unpacked, one span


def _vq_case(dt):
    N, D, K = 5000, 64, 256
    g = R.gen(5)
    z = torch.randn(N, D, generator=g).to(dt)
    ET = (torch.randn(D, K, generator=g) * 0.3).t().contiguous()
    idx = torch.randint(0, K, (N,), generator=g)
    dq = torch.randn(N, D, generator=g).to(dt)
    return z, ET, idx, dq, N, D


def test_commitment_term_is_visible_at_scale_037_and_was_not_before():
    """bf16: at scale = 0.37 a kernel that drops or negates scale * (z - q) changes more than 90 % of dz's elements.
    At the scale the tests used before, 2 beta / (N D) = 1.6e-6, the term is 2000 times below one ulp of dq ~ N(0, 1):
    dropping or negating it changes no element with |dq| >= 2e-3, which leaves the few (under 0.2 %, measured 0.05 %)
    whose dq is itself so small that half its ulp is below the term: the check hung on those alone."""
    z, ET, idx, dq, N, D = _vq_case(torch.bfloat16)
    good = R.backward_dz(dq, z, ET, idx, 0.37)
    for wrong in (0, -1):
        bad = R.backward_dz(dq, z, ET, idx, 0.37, commit=wrong)
        assert float((bad != good).float().mean()) > 0.9
    old = 2 * 0.25 / (N * D)
    good = R.backward_dz(dq, z, ET, idx, old)
    for wrong in (0, -1):
        bad = R.backward_dz(dq, z, ET, idx, old, commit=wrong)
        moved = bad != good
        assert not bool(moved[dq.float().abs() >= 2e-3].any())
        assert float(moved.float().mean()) < 2e-3
    # fp32 at the old scale and tolerance: only elements with a large |z - q| noticed a dropped term
    z, ET, idx, dq, N, D = _vq_case(torch.float32)
    good, bad = R.backward_dz(dq, z, ET, idx, old), R.backward_dz(dq, z, ET, idx, old, commit=0)
    seen = (bad - good).abs() > 1e-6 + 1e-6 * good.abs()
    assert float(seen.float().mean()) < 0.5
    assert not torch.equal(R.backward_dz(dq, z, ET, idx, 0.37, commit=0), R.backward_dz(dq, z, ET, idx, 0.37))


def _l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_layernorm_per_element_bound_sees_what_the_l2_ratio_let_pass():
    C, rows = 128, 1000
    x, gamma, beta, dy = R.ln_inputs(C, rows, torch.float32)
    y = R.ln_fwd(x.double(), gamma.double(), beta.double())
    e32 = R.e32_of(R.ln_fwd, x, gamma, beta)
    bad = y.clone()
    bad[500, 77] += 0.4 * y.abs().max()               # one wrong lane of one row, off by 40 % of the tensor's range
    for dt in DTS:
        assert _l2(bad, y) < 1e-2                     # the criterion test_layernorm_kernels had for bf16: passes
        assert R.rel(bad, y) > 10 * R.bound(R.LN_TOL[dt], e32)
    bad[500, 77] = y[500, 77] + y.abs().max()         # off by the whole range: 0.02, twice that criterion at most
    assert _l2(bad, y) < 3e-2
    # a workgroup that drops the last row of its 64-row range: dgamma / dbeta leave their bound (the edge rows carry
    # edge_weights' gain), while dx, a per-row output, cannot tell
    dx, dg, db = R.ln_bwd(x.double(), dy.double(), gamma.double())
    eg, eb = R.e32_of(R.ln_bwd, x, dy, gamma)[1:]
    keep = torch.ones(rows, dtype=torch.bool)
    keep[63] = False
    _, dg2, db2 = R.ln_bwd(x.double()[keep], dy.double()[keep], gamma.double())
    assert R.rel(dg2, dg) > 10 * R.bound(R.LN_WGRAD_TOL, eg)
    assert R.rel(db2, db) > 10 * R.bound(R.LN_WGRAD_TOL, eb)


@pytest.mark.parametrize("C,rows", [(256, 300), (65, 7), (1, 5), (1000, 3), (128, 1)])
def test_layernorm_restatement_fp32_against_fp64(C, rows):
    """The bounds' own size: with a row whose mean is 1e5 times its spread e32 is large (the mean's rounding against
    the spread), far below 1 all the same; without that row it is fp32 rounding."""
    x, gamma, beta, dy = R.ln_inputs(C, rows, torch.float32)
    e = (R.e32_of(R.ln_fwd, x, gamma, beta),) + R.e32_of(R.ln_bwd, x, dy, gamma)
    assert max(e) < 0.2, e
    x[1:2] = x[0:1]
    e = (R.e32_of(R.ln_fwd, x, gamma, beta),) + R.e32_of(R.ln_bwd, x, dy, gamma)
    assert max(e) < 1e-5, e
    y = R.ln_fwd(x, gamma, beta)
    assert torch.equal(y[0], beta)                    # a constant row: exactly beta in fp32


def test_elementwise_restatements_against_fp64():
    z, ET, idx, dq, N, D = _vq_case(torch.float32)
    q = ET[idx].double()
    assert R.rel(R.quantize_st(z, ET, idx), q) < 1e-6
    assert R.rel(R.backward_dz(dq, z, ET, idx, 0.37), dq.double() + 0.37 * (z.double() - q)) < 1e-6
    g = R.gen(3)
    x, r, e = (torch.randn(4099, generator=g) for _ in range(3))
    assert R.rel(R.mse_grad(x, r, e), R.mse_grad64(x, r, e)) < 1e-6
    assert R.rel(R.mse_grad(x, r), R.mse_grad64(x, r)) < 1e-6
    m, v = torch.randn(4099, generator=g) * 0.1, torch.rand(4099, generator=g) * 1e-2
    b1, b2 = float(R.f32(0.9)), float(R.f32(0.999))
    m1, v1 = R.adam_mv(x, m, v, b1, b2, 0.5)
    m2, v2 = R.adam_mv64(x, m, v, b1, b2, 0.5)
    assert R.rel(m1, m2) < 1e-6 and R.rel(v1, v2) < 1e-6
    assert m1.dtype == torch.float32 and v1.dtype == torch.float32
