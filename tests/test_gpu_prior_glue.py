"""Direct checks of the prior's small glue kernels (vqa_prior.hip: colsum, axpy, tf_mix, scale, dropout, embed;
vqa_prior_head.hip: rowsum),
each against two lines of torch, including one case per grid-stride kernel with work just past the launch cap of
8192 workgroups x 256 threads so that the second trip of the loop runs.

Exact: tf_mix, scale, axpy in fp32, the embed without dropout in fp32. Sums: 2e-6 of max |ref| or 8 * e32
(prior_parity_ref). Worst observed err / bound (MI355X, profiles/prior_kernel_parity.txt): colsum 0.48, rowsum 0.06.
"""
import numpy as np
import pytest
import torch

import prior_parity_ref as R
from oracle import prior_ref as P

pytestmark = pytest.mark.gpu
NAN = float("nan")
CAP = 8192 * 256  # items one trip of a grid-stride kernel covers


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("nout,inner", [(1, 300), (7, 1000), (3, CAP + 513), (600, 130)])
def test_colsum(cuda, dt, nout, inner):
    import vqa_lib as V
    g = R.gen(nout + inner)
    x = torch.randn(nout, inner + 5, generator=g).to(dt)   # outer stride past inner
    base = torch.randn(inner, generator=g)
    ref = x[:, :inner].double().sum(0)
    e32 = R.rel(x[:, :inner].float().sum(0), ref)
    xd = x.cuda()
    for acc in (False, True):
        buf = torch.full((inner + 8,), NAN, device="cuda")
        out = buf[4:4 + inner]
        if acc:
            out.copy_(base)
        V.colsum(xd, out, nout, inner + 5, inner, accumulate=acc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + inner:]).all())
        want = ref + base.double() if acc else ref
        tol, err = R.bound(2e-6, e32), R.rel(out, want)
        R.record("colsum", f"{str(dt)[6:]} nout{nout} inner{inner} acc{int(acc)}", e32, tol, err)
        assert err < tol


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 1023, 4 * CAP + 4 * 77 + 3])
def test_axpy_tail_alias_and_second_trip(cuda, dt, n):
    import vqa_lib as V
    g = R.gen(n % 1000)
    x, y = torch.randn(n, generator=g).to(dt), torch.randn(n, generator=g).to(dt)
    want = (x.float() + y.float()).to(dt)
    buf = torch.full((n + 8,), NAN, dtype=dt, device="cuda")
    z = buf[4:4 + n]
    V.axpy(x.cuda(), y.cuda(), z)
    xa = x.cuda()
    V.axpy(xa, y.cuda(), xa)   # z aliasing x, as prior.py calls it
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + n:]).all())
    assert torch.equal(z.cpu(), want) and torch.equal(xa.cpu(), want)


@pytest.mark.parametrize("rows,n,scale", [(3, 4096 * 2 + 17, 0.37), (1, 5, 1.0), (2, 4096, -2.0),
                                          (5, 4096 * 300 + 1, 1.0 / 1024)])
def test_rowsum(cuda, rows, n, scale):
    import vqa_lib as V
    x = torch.randn(rows, n, generator=R.gen(rows + n))
    ref = x.double().sum(1) * scale
    e32 = R.rel(x.sum(1) * scale, ref)
    buf = torch.full((rows + 4,), NAN, device="cuda")
    V.rowsum(x.cuda(), rows, n, scale, buf[2:2 + rows])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:2]).all()) and bool(torch.isnan(buf[2 + rows:]).all())
    err, tol = R.rel(buf[2:2 + rows], ref), R.bound(2e-6, e32)
    R.record("rowsum", f"rows{rows} n{n}", e32, tol, err)
    assert err < tol


def test_scale_second_trip(cuda):
    import vqa_lib as V
    n = CAP + 257
    x = torch.randn(n, generator=R.gen(2))
    xd = x.cuda()
    V.scale_f32_(xd, 0.3)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x * torch.tensor(0.3))


def _uniform(seed, a, b, c):
    return P.gumbel_uniform(seed, a, b, np.asarray(c, dtype=np.uint64))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dropout_mask_and_second_trip(cuda, dt):
    import vqa_lib as V
    n, rate, seed, salt, off = CAP + 1000, 0.25, 11, 0x77, 123
    x = torch.randn(n, generator=R.gen(3)).to(dt)
    ctr = torch.tensor([5], dtype=torch.int64)
    xd = x.cuda()
    V.dropout_(xd, rate, seed, salt, counter=ctr.cuda(), elem_offset=off)
    torch.cuda.synchronize()
    sm = int(_splitmix(np.uint64(5)))   # the device counter enters as seed ^ splitmix64(counter)
    keep = torch.from_numpy(_uniform_b(seed ^ sm, salt, off, n) >= np.float32(rate))
    ks = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(rate))
    want = torch.where(keep, x.float() * ks, torch.zeros(())).to(dt)
    assert torch.equal(xd.cpu(), want)


def _splitmix(x):
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & M
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M
        return x ^ (x >> np.uint64(31))


def _uniform_b(seed, a, off, n):
    """prior_uniform(seed, a, b, 0) for b = off .. off + n - 1 (the hash chain of oracle.prior_ref.gumbel_uniform
    with the array in the third slot)."""
    with np.errstate(over="ignore"):
        h = _splitmix(np.uint64(seed))
        h = _splitmix(h ^ np.uint64(a))
        h = _splitmix(h ^ (np.arange(n, dtype=np.uint64) + np.uint64(off)))
        h = _splitmix(h ^ np.uint64(0))
    return ((h >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def test_uniform_restatement_matches_the_oracle():
    """The array-in-third-slot restatement above against oracle.prior_ref.gumbel_uniform (array in the last slot)."""
    for b in (0, 1, 77):
        want = float(P.gumbel_uniform(9, 0x77, b, np.array([0], dtype=np.uint64))[0])
        assert float(_uniform_b(9, 0x77, b, 1)[0]) == want


@pytest.mark.parametrize("N,T", [(3, 50), (2, 1), (CAP // 1024 + 1, 1024)])
def test_tf_mix(cuda, N, T):
    import vqa_lib as V
    g = R.gen(N + T)
    codes = torch.randint(0, 60, (N, T), generator=g)
    amax = torch.randint(0, 60, (N, T), generator=g)
    start = 63
    rows = N * T
    t0 = (torch.arange(rows) % T == 0).reshape(N, T)
    latent = torch.where(t0, torch.tensor(start), torch.roll(codes.reshape(-1), 1).reshape(N, T))
    pred = torch.where(t0, torch.tensor(start), torch.roll(amax.reshape(-1), 1).reshape(N, T))

    def run(amax_, mask_, **kw):
        buf = torch.full((rows + 4,), -7, dtype=torch.int64, device="cuda")
        out = buf[2:2 + rows].view(N, T)
        V.tf_mix(codes.cuda(), amax_, mask_, out, start, **kw)
        torch.cuda.synchronize()
        assert bool((buf[:2] == -7).all()) and bool((buf[2 + rows:] == -7).all())
        return out.cpu()

    assert torch.equal(run(None, None), latent)                          # no predictions: the shifted codes
    mask = torch.rand(N, T, generator=g) < 0.4
    mask[:, 0] = True                                                    # t = 0 under the mask: still the start token
    assert torch.equal(run(amax.cuda(), mask.to(torch.uint8).cuda()), torch.where(mask, pred, latent))
    # the rate path: uniform(seed, 0x5446, step + counter, row + row_offset) < rate
    seed, step, off, rate = 21, 3, 1000, 0.3
    ctr = torch.tensor([4], dtype=torch.int64).cuda()
    u = _uniform(seed, 0x5446, step + 4, np.arange(rows, dtype=np.uint64) + np.uint64(off))
    m = torch.from_numpy(u < np.float32(rate)).reshape(N, T)
    got = run(amax.cuda(), None, rate=rate, seed=seed, step=step, counter=ctr, row_offset=off)
    assert torch.equal(got, torch.where(m, pred, latent))
    assert 0.2 < float(m.float().mean()) < 0.4 or rows < 100


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,T,W", [(3, 20, 32), (CAP // 2 // 1024 + 1, 1024, 8)])
def test_embed_paths(cuda, dt, N, T, W):
    import vqa_lib as V
    g = R.gen(N + T + W)
    bins, scale = 12, 3.5
    table = torch.randn(bins, W, generator=g)
    pos = torch.randn(T, W, generator=g)
    tok = torch.randint(0, bins, (N, T), generator=g)
    tok[0, 1], tok[-1, -1], tok[0, 0] = -1, bins, bins + 5     # out of range: a zero row
    ycond = torch.randn(N, W, generator=g)
    xcond = torch.randn(N, T, W, generator=g).to(dt)
    valid = (tok >= 0) & (tok < bins)
    emb = torch.where(valid[..., None], table[tok.clamp(0, bins - 1)], torch.zeros(()))
    sc = torch.tensor(scale)

    def run(yc, xc):
        buf = torch.full((N * T + 2, W), NAN, dtype=dt, device="cuda")
        out = buf[1:1 + N * T].view(N, T, W)
        V.prior_embed_fwd(table.cuda(), pos.cuda(), tok.cuda(), out, scale, ycond=yc, xcond=xc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
        return out.cpu()

    plain = emb * sc + pos
    assert torch.equal(run(None, None), plain.to(dt))                    # exact: one multiply, one add, one rounding
    e = emb.clone()
    e[:, 0] = ycond                                                      # row 0 of every sequence, whatever its token
    withy = e * sc + pos
    assert torch.equal(run(ycond.cuda(), None), withy.to(dt))
    assert torch.equal(run(ycond.cuda(), xcond.cuda()), (withy + xcond.float()).to(dt))
