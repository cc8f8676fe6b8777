"""CPU-only side of the prior's kernel-parity suites: the route and plan tables of vqa_seqlin_route,
vqa_seqlin_wgrad_plan and vqa_head_bwd_plan (fake device pointers: nothing is launched; the library plans for the
device's CU count, 256 without a device), the host-side refusals, the plain reference of tests/prior_parity_ref.py against
oracle.prior_ref.causal_conv at 1e-12, and the sensitivity of the bounds: a reference perturbed the way a kernel goes
wrong (a tile's last row dropped, two taps swapped, the tile at index G skipped, one segment's partial lost) must
land at least 10x outside the bound its group is checked with."""
import ctypes

import pytest
import torch

import prior_parity_ref as R
import vqa_lib as V
from oracle import prior_ref as P

PTR = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1008)   # 8-byte aligned only
F32, BF16 = 0, 1
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _route(K, N, taps, dt, nseq=3, T=200, raw=False, r=None, ldr=0, y=PTR, ldy=None, ln=0, x=PTR):
    info = V.SeqlinRouteInfo()
    rc = V.lib().vqa_seqlin_route(x, K, PTR if raw else None, None if raw else PTR, None, r, ldr, y, ldy or N, nseq, T,
                                  K, N, taps, -1, 0, 0, dt, ln, ctypes.byref(info))
    return rc, info


@pytest.mark.parametrize("dt,K,taps,N,want", [
    # (direct, waves, tile rows, out tiles, LDS bytes)
    (BF16, 32, 1, 16, (1, 4, 64, 2, 6720)), (BF16, 32, 1, 32, (1, 4, 64, 2, 12160)),
    (BF16, 128, 1, 48, (1, 4, 64, 8, 27584)), (BF16, 128, 1, 64, (1, 4, 64, 8, 36096)),
    (BF16, 96, 3, 80, (1, 4, 64, 8, 51008)), (BF16, 96, 3, 96, (1, 8, 128, 8, 61056)),
    (BF16, 128, 3, 128, (1, 8, 128, 8, 105984)), (BF16, 128, 1, 128, (1, 8, 128, 8, 103936)),
    (F32, 32, 1, 16, (1, 4, 64, 2, 7744)), (F32, 128, 1, 128, (1, 8, 128, 8, 136704)),
    (F32, 96, 3, 128, (1, 8, 128, 8, 154880)), (F32, 128, 3, 96, (1, 8, 128, 8, 153472)),
    (F32, 128, 3, 64, (1, 4, 64, 8, 102656)),
    # a prepared image falls back onto the staged kernel: too large for LDS / no direct instantiation
    (F32, 128, 3, 128, (0, 4, 128, 8, 136224)), (F32, 64, 1, 32, (0, 4, 128, 2, 43520)),
    (BF16, 64, 3, 128, (0, 4, 128, 8, 37152)), (BF16, 256, 1, 128, (0, 4, 128, 8, 135168)),
])
def test_route_table_of_prepared_images(dt, K, taps, N, want):
    rc, i = _route(K, N, taps, dt)
    assert rc == 0, V.last_error()
    assert (i.direct, i.waves, i.tile_rows, i.out_tiles, i.lds_bytes) == want
    tiles = 3 * -(-200 // i.tile_rows)
    assert i.tiles == tiles and i.workgroups == tiles


def test_route_grid_is_capped_by_the_device():
    for N, per_cu in ((32, 2), (64, 2), (128, 1)):
        rc, i = _route(128, N, 1, BF16, nseq=5000)
        assert rc == 0 and i.direct == 1 and i.workgroups == CUS * per_cu and i.tiles == 5000 * -(-200 // i.tile_rows)
    rc, i = _route(128, 80, 3, F32, nseq=5000)      # 128064 bytes: one workgroup per CU although N < 96
    assert rc == 0 and i.direct == 1 and i.workgroups == CUS
    rc, i = _route(64, 64, 1, BF16, nseq=5000)      # staged: a workgroup per tile
    assert rc == 0 and i.direct == 0 and i.workgroups == i.tiles == 10000


def test_one_tap_rows_must_be_16_byte_aligned_for_the_direct_form():
    assert _route(32, 32, 1, BF16, ldy=96)[1].direct == 1
    assert _route(32, 32, 1, BF16, ldy=100)[1].direct == 0           # a multiple of 4, not of 8
    assert _route(32, 32, 1, BF16, y=ODD, ldy=96)[1].direct == 0
    assert _route(32, 32, 1, BF16, r=PTR, ldr=100)[1].direct == 0
    assert _route(32, 32, 1, BF16, r=ODD, ldr=96)[1].direct == 0
    assert _route(32, 32, 1, BF16, r=PTR, ldr=96)[1].direct == 1
    assert _route(96, 32, 3, BF16, ldy=100)[1].direct == 1           # 3 taps store 4 channels at a time
    assert _route(32, 32, 1, F32, ldy=100)[1].direct == 1            # fp32: 4 elements are 16 bytes


def test_raw_weights_always_stage_and_layernorm_needs_the_direct_form():
    for K, taps in ((32, 1), (128, 3), (4, 1), (36, 3), (256, 1)):
        rc, i = _route(K, 16, taps, F32, raw=True)
        assert rc == 0 and (i.direct, i.waves, i.tile_rows, i.out_tiles) == (0, 4, 128, 2)
    rc, i = _route(128, 128, 3, BF16, ln=1)
    assert rc == 0 and (i.direct, i.waves) == (1, 8)
    assert _route(128, 128, 3, F32, ln=1)[0] == -2 and "bf16, K = 128" in V.last_error()
    assert _route(128, 32, 1, BF16, ln=1, ldy=100)[0] == -2 and "no fused form" in V.last_error()


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(K=256, N=128, taps=3, dt=F32, raw=True), -2, "needs 268320 bytes of LDS"),
    (dict(K=256, N=128, taps=1, dt=F32, raw=True), -2, "needs 266240 bytes of LDS"),
    (dict(K=256, N=128, taps=3, dt=F32), -2, "bytes of LDS"),
    (dict(K=260, N=128, taps=1, dt=F32), -2, "K=260 N=128 unsupported"),
    (dict(K=48, N=16, taps=1, dt=BF16), -2, "unsupported"),
    (dict(K=32, N=24, taps=1, dt=F32), -2, "unsupported"),
    (dict(K=32, N=32, taps=2, dt=F32), -1, "bad arguments"),
    (dict(K=32, N=32, taps=1, dt=F32, x=None), -1, "bad arguments"),
    (dict(K=32, N=32, taps=1, dt=7), -1, "unknown dtype"),
    (dict(K=32, N=32, taps=1, dt=F32, ldy=30), -1, "strides"),
])
def test_route_refuses_what_the_launch_refuses(kw, rc, msg):
    got, _ = _route(**kw)
    assert got == rc and msg in V.last_error(), V.last_error()


def test_launch_refusal_is_host_side():
    """fp32 K = 256, taps = 3, N = 128 cannot fit LDS: refused with fake pointers, so before anything touches the
    device, by vqa_seqlin_fwd itself."""
    rc = V.lib().vqa_seqlin_fwd(PTR, 256, PTR, None, None, 0, PTR, 128, 1, 8, 256, 128, 3, -1, 0, 0, F32, None)
    assert rc == -2 and "needs 268320 bytes of LDS" in V.last_error()
    assert V.lib().vqa_seqlin_route(PTR, 32, None, PTR, None, None, 0, PTR, 32, 1, 8, 32, 32, 1, -1, 0, 0, F32, 0,
                                    None) == -1 and "null route" in V.last_error()


@pytest.mark.parametrize("K,taps,pairs,ppw", [(16, 1, 1, 1), (32, 1, 2, 1), (16, 3, 3, 1), (64, 1, 4, 1),
                                              (128, 1, 8, 2), (48, 3, 9, 6), (96, 3, 18, 6), (128, 3, 24, 6)])
def test_wgrad_plan_table(K, taps, pairs, ppw):
    assert taps * K // 16 == pairs
    for dt in (torch.float32, torch.bfloat16):
        assert V.seqlin_wgrad_plan(2 * CUS + 1, 200, K, 32, taps, dt) == (256, 1, ppw)
        if CUS >= 8:   # at least four segments wanted per sequence: one 64-row chunk each
            assert V.seqlin_wgrad_plan(3, 200, K, 32, taps, dt) == (64, 4, ppw)
    # about 2 * CUs segments in all, each a multiple of 64 rows
    for nseq, T in ((1, 64 * 2 * CUS), (8, 16 * CUS * 2), (8, 100 * CUS)):
        want = max(1, 2 * CUS // nseq)
        rows = max(64, -(-(-(-T // want)) // 64) * 64)
        assert V.seqlin_wgrad_plan(nseq, T, K, 32, taps, torch.float32) == (rows, -(-T // rows), ppw)
    if CUS == 256:
        assert V.seqlin_wgrad_plan(1, 8192 * 4, K, 32, taps, torch.float32) == (64, 512, ppw)
        assert V.seqlin_wgrad_plan(8, 8192, K, 32, taps, torch.float32) == (128, 64, ppw)


def test_wgrad_plan_refusals():
    for args in ((3, 200, 24, 32, 1), (3, 200, 32, 40, 1), (3, 200, 144, 32, 3), (3, 200, 32, 32, 2),
                 (0, 200, 32, 32, 1)):
        with pytest.raises(V.VQAError, match="seqlin_wgrad"):
            V.seqlin_wgrad_plan(*args, torch.float32)
    a = ctypes.c_int(-7)
    assert V.lib().vqa_seqlin_wgrad_plan(3, 200, 32, 32, 1, F32, None, ctypes.byref(a), ctypes.byref(a)) == -1
    assert a.value == -7


def _head_plan(M, Vb):
    """ceil(M / 64) chunks over at most 2 * CUs / ceil(V / 64) segments, each a multiple of 64 rows."""
    segs = min(max(1, 2 * CUS // -(-Vb // 64)), -(-M // 64))
    rows = -(-(-(-M // segs)) // 64) * 64
    return -(-M // rows), rows


def test_head_plan_table():
    assert V.head_bwd_plan(1, 128, 64) == (1, 64)
    for M, Vb in ((300, 64), (300, 2048), (1024, 2048), (1038, 2048), (2200, 2048), (65536, 65), (100000, 2048)):
        assert V.head_bwd_plan(M, 128, Vb) == _head_plan(M, Vb), (M, Vb)
    if CUS == 256:
        assert V.head_bwd_plan(300, 128, 2048) == (5, 64)
        assert V.head_bwd_plan(1024, 128, 2048) == (16, 64)
        assert V.head_bwd_plan(1038, 128, 2048) == (9, 128)     # 16 wanted: 65 rows each -> 128, nine segments
        assert V.head_bwd_plan(2200, 128, 2048) == (12, 192)
        assert V.head_bwd_plan(65536, 128, 65) == (256, 256)
    with pytest.raises(V.VQAError, match="head_bwd_plan"):
        V.head_bwd_plan(5, 64, 64)
    with pytest.raises(V.VQAError, match="head_bwd_plan"):
        V.head_bwd_plan(0, 128, 64)


def test_symbols_exported_and_bound():
    for s in ("vqa_seqlin_route", "vqa_seqlin_wgrad_plan", "vqa_head_bwd_plan"):
        assert s in V.EXPORTED and hasattr(V.lib(), s)


# ------------------------------------------------------------------ the reference
def test_reference_matches_the_oracle_and_its_own_gradients():
    g = R.gen(1)
    x = torch.randn(3, 70, 32, generator=g, dtype=torch.float64)
    w = torch.randn(3, 32, 48, generator=g, dtype=torch.float64)
    b = torch.randn(48, generator=g, dtype=torch.float64)
    assert R.rel(R.seqlin_ref(x, w, b, -1), P.causal_conv(x, w, b)) < 1e-12
    assert R.rel(R.seqlin_ref(x, w, b, 1), P.causal_conv(x.flip(1), w, b).flip(1)) < 1e-12
    assert R.rel(R.seqlin_ref(x, w[:1], b, -1), x @ w[0] + b) < 1e-12
    for T in (1, 2):
        assert R.rel(R.seqlin_ref(x[:, :T], w, b, -1), P.causal_conv(x[:, :T], w, b)) < 1e-12
    # the data gradient is the dir = +1 layer on the transposed taps, the weight gradient seqlin_wgrad_ref
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    dy = torch.randn(3, 70, 48, generator=g, dtype=torch.float64)
    P.causal_conv(xa, wa, ba).backward(dy)
    assert R.rel(R.seqlin_ref(dy, w.transpose(1, 2), None, 1), xa.grad) < 1e-12
    dw, db = R.seqlin_wgrad_ref(x, dy, 3)
    assert R.rel(dw, wa.grad) < 1e-12 and R.rel(db, ba.grad) < 1e-12


# ------------------------------------------------------------------ sensitivity of the bounds
def _inputs(dt, nseq, T, K, N, taps, seed, edge=False):
    g = R.gen(seed)
    ew = R.edge_weights(T).float()[None, :, None] if edge else 1.0
    x = (torch.randn(nseq, T, K, generator=g) * ew).to(dt).double()
    w = (torch.randn(taps, K, N, generator=g) / (K * taps) ** 0.5).to(dt).double()
    dy = (torch.randn(nseq, T, N, generator=g) * ew).to(dt).double()
    return x, w, dy


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,taps,N,tile", [(32, 1, 16, 64), (96, 3, 64, 64), (128, 3, 128, 128)])
def test_forward_bound_sees_a_lost_row_swapped_taps_and_a_skipped_tile(dt, K, taps, N, tile):
    T, nseq = 200, 3
    x, w, _ = _inputs(dt, nseq, T, K, N, taps, K + N)
    ref = R.seqlin_ref(x, w, None, -1)
    tol = R.SEQLIN_TOL[dt]
    lost = ref.clone()
    lost[1, tile - 1] = 0                                   # the last row of a tile never stored (or stored as zero)
    assert R.rel(lost, ref) > 10 * tol
    skipped = ref.clone()
    skipped[2, tile:2 * tile] = 0                           # a whole tile never computed
    assert R.rel(skipped, ref) > 10 * tol
    stale = ref.clone()
    stale[2, tile:2 * tile] = ref[0, tile:2 * tile]         # ... or computed from the other register slot's rows
    assert R.rel(stale, ref) > 10 * tol
    if taps == 3:
        assert R.rel(R.seqlin_ref(x, w[[1, 0, 2]], None, -1), ref) > 10 * tol
        assert R.rel(R.seqlin_ref(x, w, None, 1), ref) > 10 * tol


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,taps,N,nseq", [(16, 1, 16, 3), (96, 3, 48, 3), (128, 3, 128, 3), (32, 3, 32, 40)])
def test_wgrad_bound_sees_a_lost_row_swapped_taps_and_a_lost_partial(dt, K, taps, N, nseq):
    """The inputs of the weight-gradient cases carry their weight on the rows next to a 64-row chunk edge
    (prior_parity_ref.edge_weights): with plain unit-variance rows one row of a 600-row sum hides inside the bf16
    bound. nseq = 40 stands for the long case (its bound is the same 2e-2 / max(2e-6, 8 e32))."""
    T = 200
    x, _, dy = _inputs(dt, nseq, T, K, N, taps, K + N + nseq, edge=True)
    ref_w, ref_b = R.seqlin_wgrad_ref(x, dy, taps)
    e32 = R.rel(R.seqlin_wgrad_ref(x.float(), dy.float(), taps)[0], ref_w)
    tol = R.bound(R.WGRAD_TOL, e32)

    def without(rows):                                      # the sums with these rows of sequence 1 left out
        d = dy.clone()
        d[1, rows] = 0
        return R.seqlin_wgrad_ref(x, d, taps)

    lw, lb = without(slice(63, 64))                         # the last row of one chunk
    assert R.rel(lw, ref_w) > 10 * tol and R.rel(lb, ref_b) > 10 * tol
    sw, sb = without(slice(64, 128))                        # one segment's partial (a chunk of one sequence)
    assert R.rel(sw, ref_w) > 10 * tol and R.rel(sb, ref_b) > 10 * tol
    if taps == 3:
        assert R.rel(ref_w[[1, 0, 2]], ref_w) > 10 * tol
        # the halo rows (62, 63) of the chunk at row 64 read as zero: outputs 64, 65 lose their tap-0 and tap-1 terms
        lost = torch.zeros_like(ref_w)
        for tap in range(2):
            for t in (64, 65):
                src = t - (taps - 1 - tap)
                if src < 64:
                    lost[tap] += torch.outer(x[1, src], dy[1, t])
        assert R.rel(ref_w - lost, ref_w) > 10 * tol


def _head_grads(x, w, b, tgt, rows, M):
    p = torch.softmax(x[rows] @ w + b, -1)
    p[torch.arange(p.shape[0]), tgt[rows]] -= 1.0
    p = p / M
    return x[rows].t() @ p, p.sum(0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_head_bound_sees_a_lost_row_and_a_lost_segment(dt):
    """On the inputs of the multi-chunk case of tests/test_gpu_head.py (prior_parity_ref.head_inputs)."""
    M, Vb = 1038, 2048
    x, w, b, tgt = R.head_inputs(M, Vb, dt)
    x, w, b = x.double(), w.to(dt).double(), b.double()
    every = torch.ones(M, dtype=torch.bool)
    ref_w, ref_b = _head_grads(x, w, b, tgt, every, M)
    tol = 2 * R.HEAD_TOL[dt]
    seg = every.clone()
    seg[128:256] = False                                    # one 128-row segment's partial lost
    lw, lb = _head_grads(x, w, b, tgt, seg, M)
    assert R.rel(lw, ref_w) > 10 * tol and R.rel(lb, ref_b) > 10 * R.HEAD_DB_TOL
    # the last row of a segment, of a chunk inside a segment, and of the ragged last segment
    for r in (127, 191, M - 1):
        row = every.clone()
        row[r] = False
        lw, lb = _head_grads(x, w, b, tgt, row, M)
        assert R.rel(lw, ref_w) > 10 * tol and R.rel(lb, ref_b) > 10 * R.HEAD_DB_TOL, r
    # ... on the x side only (db does not see it)
    x0 = x.clone()
    x0[127] = 0
    p = torch.softmax(x @ w + b, -1)
    p[torch.arange(M), tgt] -= 1.0
    assert R.rel(x0.t() @ (p / M), ref_w) > 10 * tol


def test_long_wgrad_bound_sees_one_lost_row():
    """The one-segment case at its size on 256 CUs (nseq = 2 * 256 + 1, T = 200, K = N = 32): one row of 102600."""
    nseq, T = 513, 200
    for dt in (torch.float32, torch.bfloat16):
        for taps in (1, 3):
            x, _, dy = _inputs(dt, nseq, T, 32, 32, taps, 7, edge=True)
            ref_w, ref_b = R.seqlin_wgrad_ref(x, dy, taps)
            lo_w, lo_b = R.seqlin_wgrad_ref(x.float(), dy.float(), taps)
            tw, tb = R.bound(R.WGRAD_TOL, R.rel(lo_w, ref_w)), R.bound(R.WGRAD_TOL, R.rel(lo_b, ref_b))
            for t in (199, 63):                              # the last of the ragged chunk's 8 rows; a chunk's last
                dw1 = torch.stack([torch.outer(R.shift_rows(x[300:301], -(taps - 1 - tap))[0, t], dy[300, t])
                                   for tap in range(taps)])
                assert R.rel(ref_w - dw1, ref_w) > 10 * tw and R.rel(ref_b - dy[300, t], ref_b) > 10 * tb, (dt, t)


def test_colsum_and_rowsum_bounds_see_a_lost_term():
    """The shapes of tests/test_gpu_prior_glue.py: one of nout rows of a column sum, one 4096-chunk partial and one
    element of a row sum."""
    for nout, inner in ((7, 1000), (3, 8192 * 256 + 513), (600, 130)):
        for dt in (torch.float32, torch.bfloat16):
            x = torch.randn(nout, inner + 5, generator=R.gen(nout + inner)).to(dt)[:, :inner]
            ref = x.double().sum(0)
            tol = R.bound(2e-6, R.rel(x.float().sum(0), ref))
            assert R.rel(ref - x[nout - 1].double(), ref) > 10 * tol
    for rows, n in ((3, 4096 * 2 + 17), (2, 4096), (5, 4096 * 300 + 1)):
        x = torch.randn(rows, n, generator=R.gen(rows + n))
        ref = x.double().sum(1)
        tol = R.bound(2e-6, R.rel(x.sum(1), ref))
        big = int(ref.abs().argmax())
        part = ref.clone()
        part[big] -= x[big, -min(n, 4096):].double().sum()   # the last chunk's partial
        assert R.rel(part, ref) > 10 * tol
        one = ref.clone()
        one[big] -= x[big, n - 1].double()                   # the last element (a chunk of one when n % 4096 == 1)
        assert R.rel(one, ref) > 10 * tol
