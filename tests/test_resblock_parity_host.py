"""CPU-only side of the residual block's parity suite: the plan table of vqa_resblock_plan (nothing is launched; the
library plans for the device's CU count, 256 without a device) and its refusals, the plain reference of
tests/resblock_parity_ref.py against autograd through oracle.vqvae_ref.conv1d at 1e-12, the condition on the
ambiguous ReLU set S, and the sensitivity of the bounds: the reference perturbed the way a kernel goes wrong must land
at least 10x outside the bound of its group, in both dtypes, at the inputs tests/test_gpu_resblock.py uses. The same
table shows which of these perturbations the old relative-L2 figures (1e-5 fp32, 1e-2 bf16) let through."""
import ctypes

import pytest
import torch

import resblock_parity_ref as R
import vqa_lib as V
from oracle.vqvae_ref import conv1d as ref_conv

PTR = ctypes.c_void_p(0x1000)
C = 32
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
DT_IDS = ["fp32", "bf16"]
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
OLD_L2 = {F32: 1e-5, BF16: 1e-2}


def _round16(v):
    return (v + 15) & ~15


def _bwd_lds(d, esz, rt):
    s, hr = C + 16 // esz, _round16(rt + 2 * d)
    return ((hr + 2 * d) + (hr + 2) + 2 * hr + 1) * s * esz


def _fwd_lds(d, esz, rt):
    s, hr = C + 16 // esz, rt + 16
    return ((hr + 2 * d) + hr + 1) * s * esz


def _want(B, T, d, dt, backward):
    """the documented plan (include/vqa.h vqa_resblock_plan)"""
    esz = 2 if dt == BF16 else 4
    model = d in (1, 3, 9, 27)
    if backward:
        rt = 160 if d in (1, 3, 9) and T >= 8192 else 128
        lds = _bwd_lds(d, esz, rt)
    else:
        rt = 176 if model else 128
        lds = max(_fwd_lds(32, esz, 128), _fwd_lds(27, esz, 176))
    ntm = -(-T // rt)
    tiles = B * ntm
    nwg = min(2 * CUS, max(1, tiles // 2)) if backward else min(3 * CUS, tiles)
    tpw = tiles // nwg
    return (rt, d if model else 0, ntm, tiles, nwg, tpw, tiles - tpw * nwg, nwg if backward else 0, lds)


def _got(B, T, d, dt, backward):
    p = V.resblock_plan(B, T, C, d, dt, backward)
    return (p.tile_rows, p.compiled_dilation, p.tiles_per_item, p.tiles, p.workgroups, p.tiles_per_workgroup,
            p.extra_tile_workgroups, p.partial_rows, p.lds_bytes)


# ------------------------------------------------------------------ the plan table
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_plan_routes(dt):
    """(tile rows, compiled dilation, LDS bytes) of every route; the LDS bytes do not depend on the device."""
    bf = dt == BF16
    for (T, d), want in {
        (8191, 1): (128, 1, 46480 if bf else 83664), (8192, 1): (160, 1, 56720 if bf else 102096),
        (8191, 3): (128, 3, None), (8192, 3): (160, 3, None),
        (8191, 9): (128, 9, 52880 if bf else None), (8192, 9): (160, 9, 63120 if bf else None),
        (8192 + 77, 9): (160, 9, 63120 if bf else None),
        (2049, 27): (128, 27, 66000 if bf else 118800), (32768, 27): (128, 27, 66000 if bf else 118800),
        (129, 32): (128, 0, 120240 if not bf else None), (300, 2): (128, 0, None), (32768, 2): (128, 0, None),
    }.items():
        got = _got(2, T, d, dt, True)
        assert got == _want(2, T, d, dt, True), (T, d, got)
        assert got[:2] == want[:2] and (want[2] is None or got[8] == want[2]), (T, d, got)
    for d, rt in ((1, 176), (3, 176), (9, 176), (27, 176), (2, 128), (32, 128)):
        for T in (100, 8191, 8192):
            got = _got(2, T, d, dt, False)
            assert got == _want(2, T, d, dt, False) and got[0] == rt and got[7] == 0, (T, d, got)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_plan_workgroup_cap_and_extra_tile_split(dt):
    assert _got(1, 1, 1, dt, True)[3:8] == (1, 1, 1, 0, 1)                 # one tile: one workgroup
    assert _got(3, 300, 1, dt, True)[2:8] == (3, 9, 4, 2, 1, 4)            # 9 tiles on 4 workgroups, one extra
    assert _got(3, 300, 27, dt, True)[2:8] == (3, 9, 4, 2, 1, 4)
    for backward, per_cu in ((True, 2), (False, 3)):
        for B, T, d in ((1, 300, 2), (7, 1000, 3), (63, 4097, 27), (40, 8269, 9), (32, 32768, 9), (513, 357, 3),
                        (1000, 129, 32), (4 * CUS + 3, 128, 27), (6 * CUS + 1, 128, 1)):
            got = _got(B, T, d, dt, backward)
            assert got == _want(B, T, d, dt, backward), (B, T, d, backward, got)
            rt, _, ntm, tiles, nwg, tpw, extra = got[:7]
            assert nwg <= per_cu * CUS and 0 <= extra < nwg and tpw * nwg + extra == tiles
            p = V.resblock_plan(B, T, C, d, dt, backward)
            runs = [p.run(w) for w in range(nwg)]
            assert runs[0][0] == 0 and runs[-1][1] == tiles
            assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
            assert sorted({e - s for s, e in runs}) == ([tpw, tpw + 1] if extra else [tpw])
    # the capped grid: every workgroup of a long launch holds at least 4 tiles and some one more
    big = V.resblock_plan(2 * CUS, 4 * 128 + 1, C, 27, dt, True)
    assert (big.workgroups, big.tiles_per_workgroup, big.extra_tile_workgroups) == (2 * CUS, 5, 0)
    if CUS == 256:
        assert _got(63, 4097, 27, dt, True)[3:7] == (2079, 512, 4, 31)
        assert _got(40, 8269, 9, dt, True)[3:7] == (2080, 512, 4, 32)
        assert _got(513, 357, 3, dt, False)[3:7] == (1539, 768, 2, 3)
        assert _got(32, 32768, 9, dt, True)[2:7] == (205, 6560, 512, 12, 416)


def test_plan_refusals():
    info = V.ResblockPlanInfo()

    def rc(B, T, Cc, d, dt, bw=1, out=info):
        return V.lib().vqa_resblock_plan(B, T, Cc, d, dt, bw, ctypes.byref(out) if out is not None else None)

    for bw in (0, 1):
        assert rc(2, 300, 64, 1, V.BF16, bw) == -2 and "unsupported C=64" in V.last_error()
        assert rc(2, 300, 32, 33, V.BF16, bw) == -2 and "dilation=33" in V.last_error()
        assert rc(2, 300, 32, 0, V.F32, bw) == -2
        assert rc(2, 300, 32, 1, 7, bw) == -2
        assert rc(1, 1 << 23, 32, 1, V.BF16, bw) == -1 and "too long for 32-bit" in V.last_error()
        assert rc(1, (1 << 23) - 1, 32, 1, V.BF16, bw) == 0
        assert rc(0, 300, 32, 1, V.F32, bw) == -1 and rc(2, 0, 32, 1, V.F32, bw) == -1
    assert rc(2, 300, 32, 1, V.F32, 1, None) == -1 and "null plan" in V.last_error()
    with pytest.raises(V.VQAError, match="vqa_resblock_plan"):
        V.resblock_plan(2, 300, 64, 1, F32, True)
    # the launches refuse the same sizes on the host, before anything touches the device (fake pointers)
    L = V.lib()
    assert L.vqa_resblock_fwd(PTR, PTR, PTR, PTR, PTR, PTR, None, 1, 1 << 23, 32, 1, V.BF16, None) == -1
    assert "resblock_fwd: item too long" in V.last_error()
    assert L.vqa_resblock_bwd(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 1, 1 << 23, 32, 1, V.BF16, PTR,
                              1 << 30, None, None) == -1
    assert "resblock_bwd: item too long" in V.last_error()
    assert L.vqa_resblock_fwd(PTR, PTR, PTR, PTR, PTR, PTR, None, 1, 300, 64, 1, V.BF16, None) == -2
    assert "vqa_resblock_plan" in V.EXPORTED and hasattr(L, "vqa_resblock_plan")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("B,T,d", [(2, 70, 1), (3, 70, 9), (2, 40, 27), (1, 27, 27), (1, 5, 27), (1, 1, 1), (2, 33, 32)])
def test_reference_matches_autograd_of_the_oracle(B, T, d):
    g = torch.Generator().manual_seed(B + T + d)
    x, dy = (torch.randn(B, T, C, generator=g, dtype=torch.float64) for _ in range(2))
    wa, wb = (torch.randn(3, C, C, generator=g, dtype=torch.float64) / 10 for _ in range(2))
    ba, bb = (torch.randn(C, generator=g, dtype=torch.float64) for _ in range(2))
    x.view(-1)[::17] = 0.0                                  # exact zeros: relu'(0) = 0 on both sides
    r = R.block(x, dy, wa, ba, wb, bb, d)
    xv, wav, bav, wbv, bbv = (t.clone().requires_grad_(True) for t in (x, wa, ba, wb, bb))
    h = ref_conv(torch.relu(xv), wav, bav, 1, d)
    y = xv + ref_conv(torch.relu(h), wbv, bbv, 1, 1)
    y.backward(dy)

    def rel(a, b):
        return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))

    assert rel(r["h"], h.detach()) < 1e-12 and rel(r["y"], y.detach()) < 1e-12
    for got, want in ((r["dx"], xv.grad), (r["wa"], wav.grad), (r["ba"], bav.grad), (r["wb"], wbv.grad),
                      (r["bb"], bbv.grad)):
        assert rel(got, want) < 1e-12


def test_bf16_boundary_helpers():
    v = torch.tensor([1.0, 1.00390625, 1.0078125, -1.20703133, 3.0, 0.0, 100.3], dtype=torch.float64)
    assert R.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 0.5]
    near = R.near_bf16_boundary(v, torch.full_like(v, 1e-6))
    assert near.tolist() == [False, True, False, True, False, False, False]


ALL_CASES = R.PLAN_CASES + R.CROSS_CASES + [(1, T, d) for T, d in R.STEADY_CASES]


def _case(B, T, d, dt, zeros=0, bias_a=True):
    rt = V.resblock_plan(B, T, C, d, dt, True).tile_rows
    return R.case(B, T, d, dt, rt, zeros, bias_a)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_ambiguous_relu_set_is_small_and_covers_the_fp32_run(dt):
    """S <= 1e-4 of the elements at every case's seed, from the reference alone; the fp32 run of the reference (its
    h carries an fp32 error as the kernel's does) takes another ReLU mask only inside S, and its h stays well inside
    the margin."""
    for B, T, d in ALL_CASES + [(2, 300, 3)]:
        for kw in ({}, {"zeros": 600} if (B, T, d) == (3, 300, 27) else {}, {"bias_a": False} if T == 300 and d == 3 else {}):
            _, ref = _case(B, T, d, dt, **kw)
            assert ref.s_share <= R.S_MAX, (B, T, d, ref.s_share)
            differ = ref.lo["hpos"] != ref.r["hpos"]
            assert not bool((differ & ~ref.S).any()), (B, T, d)
            assert float(((ref.lo["h"].double() - ref.r["h"]).abs() / ref.m_h.clamp_min(1e-300)).max()) < 0.25
            for k in ("dx",) + R.GRADS:   # the accumulation term stays the project's figure or close to it
                assert ref.c[k] < 8e-6, (B, T, d, k, ref.c[k])


# ------------------------------------------------------------------ sensitivity of the bounds
def _row_mask(B, T, keep_out):
    m = torch.ones(B, T, 1, dtype=torch.float64)
    for n, a, b in keep_out:
        m[n, a:b] = 0
    return m


def _tile_rows(pl, T, first, end):
    """(item, first row, end row) of the tiles [first, end)"""
    out = []
    for t in range(first, end):
        n, tm = divmod(t, pl.tiles_per_item)
        out.append((n, tm * pl.tile_rows, min(T, (tm + 1) * pl.tile_rows)))
    return out


def _wgrads(ref, m):
    """the four weight gradients with the rows where m = 0 left out of the sums"""
    r, a, d = ref.r, ref.a, ref.d
    wb, bb = R.wgrad(r["rh"], a["dy"] * m, 1)
    wa, ba = R.wgrad(r["rx"], r["dh"] * m, d)
    return {"wa": wa, "ba": ba, "wb": wb, "bb": bb}


def _mutations(B, T, d, dt, ref, pl):
    """name -> {output: the reference gone wrong}"""
    r, a = ref.r, ref.a
    out = {}
    if pl.tiles_per_item > 1 and pl.tile_rows >= d:
        t0 = pl.tile_rows                                   # the second tile of item 0: its first dh halo row as zero
        dx = r["dx"].clone()
        dx[0, t0] -= (r["dh"][0, t0 - d] @ a["wa"][2].t()) * r["xpos"][0, t0]
        out["first dh halo row zero"] = {"dx": dx}
    last = (pl.tiles_per_item - 1) * pl.tile_rows
    if pl.tiles > 1:
        out["ragged last tile skipped"] = _wgrads(ref, _row_mask(B, T, [(B - 1, last, T)]))
        w = pl.workgroups - 1
        out["one partial row lost"] = _wgrads(ref, _row_mask(B, T, _tile_rows(pl, T, *pl.run(w))))
    if T > d:
        out["taps 0 and 2 swapped"] = {"dx": a["dy"] + R.conv_t(r["dh"], a["wa"][[2, 1, 0]], d) * r["xpos"]}
    if bool((a["x"] == 0).any()):
        out["x >= 0 for x > 0"] = {"dx": a["dy"] + R.conv_t(r["dh"], a["wa"], d) * (a["x"] >= 0)}
    if B > 1:
        ext = {k: torch.cat([a[k][:1], a[k][1:2, :1]], 1) for k in ("x", "dy")}
        nxt = R.block(ext["x"], ext["dy"], a["wa"], a["ba"], a["wb"], a["bb"], d, act=dt)
        dx = r["dx"].clone()
        dx[0] = nxt["dx"][0, :T]
        out["row past the end from the next item"] = {"dx": dx}
    return out


SENS = [(B, T, d, 0) for B, T, d in ALL_CASES] + [(3, 300, 27, 600)]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_bounds_see_every_mutation_and_the_old_metric_does_not(dt, capsys):
    seen, through_old = set(), []
    for B, T, d, zeros in SENS:
        pl = V.resblock_plan(B, T, C, d, dt, True)
        _, ref = _case(B, T, d, dt, zeros)
        for name, outs in _mutations(B, T, d, dt, ref, pl).items():
            seen.add(name)
            for k, bad in outs.items():
                ratio = ref.ratio(k, bad)
                old = R.l2(bad, ref.r[k])
                if old < OLD_L2[dt]:
                    through_old.append((name, B, T, d, k, old))
                with capsys.disabled():
                    print(f"{R.dt_name(dt)} B={B} T={T} d={d} {name:36s} {k:2s} err/bound {ratio:10.3g}  "
                          f"old L2 {old:9.3e} {'passes the old bound' if old < OLD_L2[dt] else 'caught'}")
                assert ratio >= 10.0, (name, B, T, d, k, ratio)
    assert seen == {"first dh halo row zero", "ragged last tile skipped", "one partial row lost",
                    "taps 0 and 2 swapped", "x >= 0 for x > 0", "row past the end from the next item"}
    if dt == BF16:   # the gap this suite closes: the production dtype's old figure lets a lost dx row through
        halo = [t for t in through_old if t[0] == "first dh halo row zero"]
        assert {(B, T, d) for _, B, T, d, *_ in halo} >= {(1, 8269, 9), (2, 2049, 27), (3, 300, 27), (1, 4097, 27)}
