"""Kernel-level parity of the prior's sequence-linear family (vqa_prior_seqlin.hip: seqlin_kernel, seqlin_d_kernel,
seqlin_prep_kernel, seqlin_wgrad_kernel) against the plain fp64 reference of tests/prior_parity_ref.py, on every
route launch_seqlin can choose. Each case asserts the route it means to check through vqa_seqlin_route /
vqa_seqlin_wgrad_plan, writes into the middle of a NaN-filled buffer (guard rows and the padding columns of a
strided y must stay NaN) and compares on inputs rounded to the activation dtype, weights rounded where the kernel
rounds them (prepared images, and the staged kernel's LDS copy).

Bounds: 2e-6 (fp32) / 2e-2 (bf16) of max |ref|, the weight gradient 2e-6 in both dtypes (fp32 sums of exact
products: prior_parity_ref.WGRAD_TOL); long sums max(that, 8 * e32). Exact: the prepared images, LayerNorm-fused
against unfused. Worst observed err / bound per group (MI355X, profiles/prior_kernel_parity.txt): seqlin 0.44,
seqlin_long 0.29, wgrad 0.16, wgrad_long 0.12.
"""
import ctypes
import itertools
import math

import pytest
import torch

import prior_parity_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
DTS = [torch.float32, torch.bfloat16]
DIRECT = {(32, 1), (128, 1), (96, 3), (128, 3)}
GUARD = 2


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _expected_route(dt, K, N, taps, prepared, aligned=True):
    """(direct, waves, out_tiles) by the documented rule (include/vqa.h vqa_seqlin_route)."""
    esz = 4 if dt == torch.float32 else 2
    nt = 2 if N <= 32 else 8
    if prepared and (K, taps) in DIRECT and (aligned or taps == 3):
        waves = 8 if N >= 96 else 4
        lds = taps * N * (K + 16 // esz) * esz + (waves * 16 * (N + 4) * 4 if taps == 1 else 0) + (2 * K + N) * 4
        if lds <= 160 * 1024:
            return 1, waves, nt
    return 0, 4, nt


def _out(rows, N, dt, ld, c0):
    buf = torch.full((rows + 2 * GUARD, ld), NAN, dtype=dt, device="cuda")
    return buf, buf[GUARD:GUARD + rows, c0:c0 + N]


def _seqs(v, nseq, T):
    """(nseq, T, N) view of a row-strided (nseq * T, N) view (explicit strides: T = 1 leaves them ambiguous)."""
    return torch.as_strided(v, (nseq, T, v.shape[1]), (T * v.stride(0), v.stride(0), 1))


def _guards_intact(buf, rows, N, c0):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[GUARD:GUARD + rows, c0:c0 + N] = True
    nan = torch.isnan(buf)
    return bool(nan[~inside].all()) and not bool(nan[inside].any())


def _case(dt, K, N, taps, T, nseq=3, dir=-1, form="prep", wtrans=False, bias=True, res=False, acc=False, ld=None,
          c0=8, seed=0, expect=None, long_sum=False, min_trips=0, group="seqlin"):
    """One forward launch in the given form ("raw": fp32 weights, "prep": prepared image) against the reference."""
    import vqa_lib as V
    g = R.gen(1000 * seed + K + 7 * N + taps + T)
    rows = nseq * T
    x = torch.randn(nseq, T, K, generator=g).to(dt)
    w = torch.randn(taps, K, N, generator=g) / math.sqrt(K * taps)   # the logical Wv[tap][k][n], fp32
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(nseq, T, N, generator=g).to(dt) if res else None
    y0 = torch.randn(nseq, T, N, generator=g).to(dt) if acc else None
    dd = lambda t: None if t is None else t.double()  # noqa: E731
    wr = w.to(dt)  # both kernels compute with the weights in the activation dtype
    ref = R.seqlin_ref(dd(x), dd(wr), dd(b), dir, dd(r), dd(y0))
    tol, e32 = R.SEQLIN_TOL[dt], 0.0
    if long_sum:
        ff = lambda t: None if t is None else t.float()  # noqa: E731
        e32 = R.rel(R.seqlin_ref(ff(x), ff(wr), ff(b), dir, ff(r), ff(y0)), ref)
        tol = R.bound(tol, e32)
    ld = ld or N + 16
    buf, yv = _out(rows, N, dt, ld, c0)
    if acc:
        yv.copy_(y0.reshape(rows, N))
    y3 = _seqs(yv, nseq, T)
    rd = None
    if res:
        rbuf = torch.zeros(nseq, T, N + 8, dtype=dt, device="cuda")
        rd = rbuf[..., 8:]
        rd.copy_(r)
    xd, bd = x.cuda(), None if b is None else b.cuda()
    wst = (w.transpose(1, 2).contiguous() if wtrans else w).cuda()  # storage: (taps, N, K) when wtrans
    wst = wst[0] if taps == 1 else wst
    wp = None
    if form == "prep":
        wp = torch.full((taps, N, K), NAN, dtype=dt, device="cuda")
        V.seqlin_prep([(wst, wp, taps, K, N, wtrans)], dt)
        info = V.seqlin_route(xd, y3, T, wp=wp, b=bd, taps=taps, dir=dir, residual=rd, accumulate=acc)
        V.seqlin_fwd_prepped(xd, wp, bd, y3, T, taps=taps, dir=dir, residual=rd, accumulate=acc)
    else:
        info = V.seqlin_route(xd, y3, T, w=wst, b=bd, taps=taps, dir=dir, wtrans=wtrans, residual=rd, accumulate=acc)
        V.seqlin_fwd(xd, wst, bd, y3, T, taps=taps, dir=dir, wtrans=wtrans, residual=rd, accumulate=acc)
    torch.cuda.synchronize()
    aligned = ld % (16 // x.element_size()) == 0
    want = expect or _expected_route(dt, K, N, taps, form == "prep", aligned)
    assert (info.direct, info.waves, info.out_tiles) == want, (info, want)
    assert info.tile_rows == (16 * info.waves if info.direct else 128)
    assert info.tiles == nseq * -(-T // info.tile_rows) and info.workgroups <= info.tiles
    if min_trips:
        assert info.direct and info.tiles >= min_trips * info.workgroups + 1, info
        assert T % info.tile_rows != 0
    assert _guards_intact(buf, rows, N, c0), "guard rows / padding columns were written, or an output row was not"
    err = R.rel(yv, ref.reshape(rows, N))
    name = (f"{str(dt)[6:]} K{K} N{N} taps{taps} T{T} nseq{nseq} dir{dir:+d} {form}{'T' if wtrans else ''}"
            f"{' b' if bias else ''}{' r' if res else ''}{' acc' if acc else ''} ld{ld}")
    R.record(group, name, e32, tol, err)
    assert err < tol, (name, err, tol, info)
    return info


# every T edge: one row, fewer rows than taps, one short of / on / one past a 64-row tile, past a 128-row tile, ragged
T_EDGES = [1, 2, 63, 64, 65, 129, 200]
WIDTHS = [16, 32, 64, 96, 128]


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,taps", sorted(DIRECT))
def test_prepared_forms_on_every_width_class_and_T_edge(cuda, dt, K, taps):
    """Forward (dir -1, image of w) and data-gradient (dir +1, image of the transposed storage) forms; bias, residual
    and accumulate cycle through their combinations over the 35 (N, T) pairs."""
    flags = itertools.cycle(itertools.product([True, False], repeat=3))
    seen = set()
    for i, (N, T) in enumerate(itertools.product(WIDTHS, T_EDGES)):
        bias, res, acc = next(flags)
        fwd = (i + i // 8) % 2 == 0   # the direction decoupled from the flag cycle of period 8
        info = _case(dt, K, N, taps, T, dir=-1 if fwd else 1, wtrans=not fwd, bias=bias, res=res, acc=acc, seed=i)
        seen.add((info.direct, info.waves, info.out_tiles))
    want = {(1, 4, 2), (1, 4, 8), (1, 8, 8)}
    if dt == torch.float32 and (K, taps) == (128, 3):
        want.add((0, 4, 8))  # N = 128: the three images exceed 160 KiB, staged from the prepared image
    assert seen == want


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [48, 80])
def test_prepared_middle_width_class(cuda, dt, N):
    for K, taps in sorted(DIRECT):
        _case(dt, K, N, taps, 129, dir=-1, res=True, acc=True, seed=3, expect=(1, 4, 8))
        _case(dt, K, N, taps, 65, dir=1, wtrans=True, bias=False, seed=4, expect=(1, 4, 8))


def _long_nseq(dt, K, N, taps, T):
    """nseq for which the direct form takes tiles >= 2 * workgroups + 1 on this device, by the route query."""
    import vqa_lib as V
    p, info = ctypes.c_void_p(0x1000), V.SeqlinRouteInfo()
    code = V.dtype_code(dt)
    rc = V.lib().vqa_seqlin_route(p, K, None, p, None, None, 0, p, N + 16, 1 << 20, T, K, N, taps, -1, 0, 0, code, 0,
                                  ctypes.byref(info))
    assert rc == 0 and info.direct == 1, V.last_error()
    per_seq = -(-T // info.tile_rows)
    return -(-(2 * info.workgroups + 1) // per_seq)


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [32, 64, 128])
@pytest.mark.parametrize("K,taps,dir,res", [(128, 1, -1, True), (96, 3, 1, False), (96, 3, -1, True),
                                            (32, 1, 1, False)])
def test_persistent_loop_past_two_tiles_per_workgroup(cuda, dt, N, K, taps, dir, res):
    """tiles >= 2 * workgroups + 1 with a ragged last tile: the prefetch into the other register slot and the
    reload of the first slot (tile, tile + G, tile + 2G) of seqlin_d_kernel all run, in every width class."""
    T = 200
    nseq = _long_nseq(dt, K, N, taps, T)
    _case(dt, K, N, taps, T, nseq=nseq, dir=dir, wtrans=dir == 1, res=res, seed=9, long_sum=True, min_trips=2,
          group="seqlin_long")


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
def test_staged_route_from_a_prepared_image(cuda, dt):
    if dt == torch.float32:  # the three tap images of (128, 3, 128) need 3 * 128 * 132 * 4 bytes > 160 KiB
        _case(dt, 128, 128, 3, 200, res=True, acc=True, seed=1, expect=(0, 4, 8))
        _case(dt, 128, 128, 3, 65, dir=1, wtrans=True, bias=False, seed=2, expect=(0, 4, 8))
    for N in (16, 64, 128):   # no direct instantiation for K = 64
        _case(dt, 64, N, 1, 129, res=True, seed=3, expect=(0, 4, 2 if N <= 32 else 8))
        _case(dt, 64, N, 3, 130, dir=1, wtrans=True, acc=True, seed=4, expect=(0, 4, 2 if N <= 32 else 8))
    if dt == torch.bfloat16:  # 1 tap into a column slice whose row stride is a multiple of 4, not of 8
        for K, N in ((32, 32), (128, 96)):
            _case(dt, K, N, 1, 200, ld=100, c0=4, res=True, seed=5, expect=(0, 4, 2 if N <= 32 else 8))
        _case(dt, 128, 96, 3, 200, ld=100, c0=4, seed=6, expect=(1, 8, 8))   # 3 taps store 4 channels at a time


@pytest.mark.parametrize("dt,Ks", [(torch.float32, [4, 36, 256]), (torch.bfloat16, [32, 256])],
                         ids=["fp32", "bf16"])
def test_staged_route_from_raw_weights(cuda, dt, Ks):
    for i, (K, wtrans) in enumerate(itertools.product(Ks, [False, True])):
        for taps, N, T in ((1, 16, 129), (3, 16, 65), (1, 128 if dt == torch.bfloat16 or K < 256 else 16, 200)):
            _case(dt, K, N, taps, T, form="raw", wtrans=wtrans, dir=-1 if i % 2 else 1, res=i % 2 == 0,
                  acc=i % 3 == 0, seed=i, expect=(0, 4, 2 if N <= 32 else 8))


def test_staged_route_refuses_what_cannot_fit_before_launching(cuda):
    import vqa_lib as V
    x = torch.zeros(1, 8, 256, device="cuda")
    w = torch.zeros(3, 256, 128, device="cuda")
    y = torch.full((1, 8, 128), NAN, device="cuda")
    with pytest.raises(V.VQAError, match="bytes of LDS"):
        V.seqlin_fwd(x, w, None, y, 8, taps=3)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


@pytest.mark.parametrize("N,taps,dir,res,T,nseq", [(128, 3, -1, False, 1, 3), (96, 3, 1, False, 65, 3),
                                                   (32, 1, -1, True, 65, 3), (128, 1, -1, True, 1, 3),
                                                   (64, 1, -1, True, 129, 3), (128, 1, -1, True, 200, 0),
                                                   (32, 3, -1, False, 200, 0), (64, 3, 1, True, 200, 0)])
def test_layernorm_fused_form_is_bit_identical(cuda, N, taps, dir, res, T, nseq):
    """vqa_seqlin_fwd_ln_prepped against vqa_layernorm_fwd + vqa_seqlin_fwd_prepped, bit for bit, at T = 1, across a
    tile edge and (nseq = 0: sized by the route query) past two tiles per workgroup."""
    import vqa_lib as V
    dt, K = torch.bfloat16, 128
    long = nseq == 0
    nseq = nseq or _long_nseq(dt, K, N, taps, T)
    g = R.gen(N + taps + T)
    rows = nseq * T
    x = (torch.randn(nseq, T, K, generator=g) * 1.5 + 0.3).to(dt).cuda()
    w = (torch.randn(taps, K, N, generator=g) / math.sqrt(K * taps)).cuda()
    b = torch.randn(N, generator=g).cuda()
    r = torch.randn(nseq, T, N, generator=g).to(dt).cuda() if res else None
    gm = (1.0 + 0.2 * torch.randn(K, generator=g)).cuda()
    bt = (0.1 * torch.randn(K, generator=g)).cuda()
    wp = torch.empty(taps, N, K, dtype=dt, device="cuda")
    V.seqlin_prep([(w if taps == 3 else w[0], wp, taps, K, N, False)], dt)
    a = torch.empty_like(x)
    V.layernorm_fwd(x, gm, bt, a, 1e-6)
    b0, y0 = _out(rows, N, dt, N + 16, 8)
    b1, y1 = _out(rows, N, dt, N + 16, 8)
    V.seqlin_fwd_prepped(a, wp, b, _seqs(y0, nseq, T), T, taps=taps, dir=dir, residual=r)
    info = V.seqlin_route(x, _seqs(y1, nseq, T), T, wp=wp, b=b, taps=taps, dir=dir, residual=r, layernorm=True)
    V.seqlin_fwd_ln_prepped(x, gm, bt, 1e-6, wp, b, _seqs(y1, nseq, T), T, taps=taps, dir=dir, residual=r)
    torch.cuda.synchronize()
    assert info.direct == 1 and (info.waves, info.out_tiles) == (8 if N >= 96 else 4, 2 if N <= 32 else 8)
    if long:
        assert info.tiles >= 2 * info.workgroups + 1
    assert _guards_intact(b0, rows, N, 8) and _guards_intact(b1, rows, N, 8)
    assert torch.equal(y0, y1)
    # and the unfused pair is right: LayerNorm in fp64 of the bf16 rows, rounded as layernorm_fwd stores it
    xr = x.double().cpu()
    ar = a.double().cpu()
    mu, var = xr.mean(-1, keepdim=True), xr.var(-1, unbiased=False, keepdim=True)
    ln = (xr - mu) / torch.sqrt(var + 1e-6) * gm.double().cpu() + bt.double().cpu()
    assert R.rel(ar, ln) < 2e-2
    ref = R.seqlin_ref(ar, wp.double().cpu().transpose(1, 2), b.double().cpu(), dir,
                       None if r is None else r.double().cpu())
    assert R.rel(y1, ref.reshape(rows, N)) < R.SEQLIN_TOL[dt]


# ------------------------------------------------------------------ weight gradient
def _wgrad(dt, K, N, taps, T, nseq, strided=False, long_sum=False, seed=0, group="wgrad"):
    import vqa_lib as V
    g = R.gen(77 + seed + K + 3 * N + taps)
    ew = R.edge_weights(T).float()[None, :, None]
    x = (torch.randn(nseq, T, K, generator=g) * ew).to(dt)
    dy = (torch.randn(nseq, T, N, generator=g) * ew).to(dt)
    ref_w, ref_b = R.seqlin_wgrad_ref(x.double(), dy.double(), taps)
    tol_w = tol_b = R.WGRAD_TOL
    e_w = e_b = 0.0
    if long_sum:
        lo_w, lo_b = R.seqlin_wgrad_ref(x.float(), dy.float(), taps)
        e_w, e_b = R.rel(lo_w, ref_w), R.rel(lo_b, ref_b)
        tol_w, tol_b = R.bound(tol_w, e_w), R.bound(tol_b, e_b)
    if strided:
        xb = torch.zeros(nseq, T, K + 16, dtype=dt, device="cuda")
        yb = torch.zeros(nseq, T, N + 8, dtype=dt, device="cuda")
        xd, dyd = xb[..., 8:8 + K], yb[..., 8:]
        xd.copy_(x)
        dyd.copy_(dy)
    else:
        xd, dyd = x.cuda(), dy.cuda()
    dw = torch.full((taps, K, N), NAN, device="cuda")
    db = torch.full((N,), NAN, device="cuda")
    V.seqlin_wgrad(xd, dyd, dw if taps == 3 else dw[0], db, T, taps=taps)
    torch.cuda.synchronize()
    plan = V.seqlin_wgrad_plan(nseq, T, K, N, taps, dt)
    name = f"{str(dt)[6:]} K{K} N{N} taps{taps} T{T} nseq{nseq}{' strided' if strided else ''} plan{plan}"
    ew_, eb_ = R.rel(dw, ref_w), R.rel(db, ref_b)
    R.record(group, name + " dW", e_w, tol_w, ew_)
    R.record(group, name + " db", e_b, tol_b, eb_)
    assert ew_ < tol_w and eb_ < tol_b, (name, ew_, tol_w, eb_, tol_b)   # NaN (an unwritten output) fails too
    return plan


# (K, taps, N): 1, 2, 3, 4, 8, 9, 18 and 24 (tap, k-tile) pairs -> pairs per wave 1, 1, 1, 1, 2, 6, 6, 6
WG_SHAPES = [(16, 1, 16, 1), (32, 1, 48, 1), (16, 3, 128, 1), (64, 1, 16, 1), (128, 1, 48, 2), (48, 3, 128, 6),
             (96, 3, 16, 6), (128, 3, 128, 6), (96, 3, 48, 6)]


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
def test_wgrad_every_pair_count(cuda, dt):
    """nseq = 3, T = 200: four one-chunk segments per sequence, the 3-tap halo crossing each segment edge; ragged
    pair counts (9, 18), and 3 pairs where the bias wave owns none."""
    for K, taps, N, ppw in WG_SHAPES:
        seg_rows, segs, got = _wgrad(dt, K, N, taps, 200, 3)
        assert got == ppw and seg_rows == 64 and segs == 4


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
def test_wgrad_one_segment_of_several_chunks(cuda, dt):
    """nseq = 2 * CUs + 1: one segment per sequence, four 64-row chunks, the last with 8 rows."""
    nseq = 2 * _cus() + 1
    for taps in (1, 3):
        seg_rows, segs, _ = _wgrad(dt, 32, 32, taps, 200, nseq, long_sum=True, group="wgrad_long")
        assert segs == 1 and seg_rows >= 256


@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
def test_wgrad_strided_inputs(cuda, dt):
    for K, taps, N in ((32, 1, 32), (96, 3, 48), (128, 3, 128)):
        _wgrad(dt, K, N, taps, 200, 3, strided=True, seed=2)


# ------------------------------------------------------------------ prep
@pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
def test_prep_fifty_descriptors_in_one_call(cuda, dt):
    """More than kMaxPrep = 48 descriptors: the list is split over two launches; every image exact."""
    import vqa_lib as V
    g = R.gen(50)
    shapes = [(1, 32, 32), (3, 96, 128), (1, 128, 48), (3, 128, 16), (1, 64, 80), (3, 32, 96), (1, 4, 16)]
    descs, want = [], []
    for i in range(50):
        taps, K, N = shapes[i % len(shapes)]
        wtrans = i % 3 == 0
        w = torch.randn(taps, K, N, generator=g)
        st = (w.transpose(1, 2).contiguous() if wtrans else w).cuda()
        out = torch.full((taps * N * K + 8,), NAN, dtype=dt, device="cuda")
        descs.append((st, out, taps, K, N, wtrans))
        want.append(w.transpose(1, 2).contiguous().to(dt).reshape(-1))
    V.seqlin_prep(descs, dt)
    torch.cuda.synchronize()
    for i, ((_, out, taps, K, N, _), ref) in enumerate(zip(descs, want)):
        n = taps * K * N
        assert torch.equal(out[:n].cpu(), ref), i
        assert bool(torch.isnan(out[n:]).all()), i
