"""C-ABI checks of vqa_resample / vqa_resample_route that need no GPU: every argument is settled on the host, so a bad
call returns VQA_E_INVALID_ARG with a "resample:" message before anything is launched (fake device pointers, as
tests/test_pcm_abi.py does), and the route query answers without a device."""
import ctypes

import pytest

import resample as RS
import vqa_lib as V

P = ctypes.c_void_p(0x1000)       # 16-byte aligned fake device pointer
ODD2 = ctypes.c_void_p(0x1002)    # 2-byte aligned only
ODD1 = ctypes.c_void_p(0x1001)    # not even 2-byte aligned
# 22050 -> 3000 best (L 20, M 147, W 249): a whole track of 4099 samples has ceil(4099 * 20 / 147) = 558 outputs
GOOD = dict(x=P, x_dtype=0, ldx=5000, in0=0, n_in=4099, track_len=4099, out=P, ldo=600, m0=0, n_out=558, B=3, up=20,
            down=147, taps=P, taps_per_phase=498)
ORDER = ["x", "x_dtype", "ldx", "in0", "n_in", "track_len", "out", "ldo", "m0", "n_out", "B", "up", "down", "taps",
         "taps_per_phase"]


def _call(**kw):
    a = {**GOOD, **kw}
    return V.lib().vqa_resample(*[a[k] for k in ORDER], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), "null x, out or taps"),
    (dict(out=None), "null x, out or taps"),
    (dict(taps=None), "null x, out or taps"),
    (dict(B=0), "B 0 outside [1, 65535]"),
    (dict(B=-3), "B -3 outside [1, 65535]"),
    (dict(B=65536), "B 65536 outside [1, 65535]"),
    (dict(up=0), "up 0 and down 147 must be positive"),
    (dict(down=-1), "up 20 and down -1 must be positive"),
    (dict(up=21), "up 21 and down 147 are not coprime"),
    (dict(up=40, down=294), "not coprime"),
    (dict(taps_per_phase=497), "taps_per_phase 497 is not even and in [2, 8192]"),
    (dict(taps_per_phase=0), "taps_per_phase 0 is not even and in [2, 8192]"),
    (dict(taps_per_phase=8194), "taps_per_phase 8194 is not even and in [2, 8192]"),
    (dict(x_dtype=2), "x_dtype 2 is neither 0 (fp32) nor 1 (int16)"),
    (dict(x=ODD2), "x is not 4-byte aligned"),
    (dict(x=ODD1, x_dtype=1), "x is not 2-byte aligned"),
    (dict(out=ODD2), "out is not 4-byte aligned"),
    (dict(taps=ODD2), "taps is not 4-byte aligned"),
    (dict(n_out=0), "n_out 0 and track_len 4099 must be positive"),
    (dict(n_out=-5), "n_out -5 and track_len 4099 must be positive"),
    (dict(track_len=0), "track_len 0 must be positive"),
    (dict(m0=-1), "negative m0 -1"),
    (dict(in0=-2), "in0 -2"),
    (dict(n_in=-1), "n_in -1"),
    (dict(n_out=559), "outputs [0, 0 + 559) exceed the track's 558 outputs"),
    (dict(m0=500, n_out=59), "outputs [500, 500 + 59) exceed the track's 558 outputs"),
    (dict(m0=(1 << 63) - 1, n_out=2), "exceed the track's 558 outputs"),
    (dict(ldx=4098), "ldx 4098 below n_in 4099"),
    (dict(ldo=557), "ldo 557 below n_out 558"),
    (dict(up=(1 << 31) - 1, down=(1 << 31) - 2, taps_per_phase=2, track_len=(1 << 63) - 1, n_in=1, m0=1 << 40,
          n_out=1), "(m0 + n_out) * down = 1099511627777 * 2147483646 does not fit in int64"),
    # outputs [0, 558) of the track read all of it; the call holds less
    (dict(n_in=4098), "need input samples [0, 4098], the call holds [0, 4098)"),
    (dict(in0=1, n_in=4098), "need input samples [0, 4098], the call holds [1, 4099)"),
    # outputs [100, 110): floor(100 * 147 / 20) - 248 = 487 .. floor(109 * 147 / 20) + 249 = 1050
    (dict(m0=100, n_out=10, in0=488, n_in=563), "need input samples [487, 1050], the call holds [488, 1051)"),
    (dict(m0=100, n_out=10, in0=487, n_in=563), "need input samples [487, 1050], the call holds [487, 1050)"),
])
def test_resample_rejects_bad_arguments_before_launch(kw, msg):
    rc = _call(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("resample:") and msg in err, err


def _route_raw(up, down, taps, lds=True, tile=True):
    a, b = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = V.lib().vqa_resample_route(up, down, taps, ctypes.byref(a) if lds else None, ctypes.byref(b) if tile else None)
    return rc, a.value, b.value


@pytest.mark.parametrize("args,msg", [
    ((20, 147, 498, False, True), "null table_in_lds or tile_outputs"),
    ((20, 147, 498, True, False), "null table_in_lds or tile_outputs"),
    ((0, 147, 498), "must be positive"),
    ((20, 148, 498), "not coprime"),
    ((20, 147, 499), "is not even"),
])
def test_route_rejects_bad_arguments(args, msg):
    rc, a, b = _route_raw(*args)
    assert rc == -1 and (a, b) == (-7, -7)
    assert V.last_error().startswith("resample:") and msg in V.last_error()


def test_symbols_exported_and_bound():
    lib = V.lib()
    for s in ("vqa_resample", "vqa_resample_route"):
        assert s in V.EXPORTED and hasattr(lib, s)
    assert callable(V.resample) and callable(V.resample_route)


def test_wrapper_checks_tensors_on_the_host():
    import torch
    x, out, taps = torch.zeros(2, 64), torch.zeros(2, 96), torch.zeros(3, 68)
    with pytest.raises(V.VQAError):
        V.resample(x, out, taps, 3, 2)                          # CPU tensors never reach the kernel
    with pytest.raises(V.VQAError):
        V.resample(x.double(), out, taps, 3, 2)
    with pytest.raises(V.VQAError):
        V.resample(x.to(torch.int32), out, taps, 3, 2)
    with pytest.raises(V.VQAError):
        V.resample(x, out.to(torch.int16), taps, 3, 2)
    with pytest.raises(V.VQAError):
        V.resample(x, out, taps.double(), 3, 2)
    with pytest.raises(V.VQAError):
        V.resample(x.to(torch.int16), out, taps, 3, 2)         # a good dtype, still a CPU tensor


def test_route_of_the_reference_conversion_and_of_coprime_rates():
    best = RS.design(22050, 3000, "best")
    lds, tile = V.resample_route(best.up, best.down, best.P)
    assert lds is True and 1 <= tile <= 256
    far = RS.design(22050, 16001, "best")
    assert far.up == 16001 and far.table.nbytes > 4_000_000
    lds, tile = V.resample_route(far.up, far.down, far.P)
    assert lds is False and 1 <= tile <= 256
    for key in ((22050, 3000, "fast"), (3000, 22050, "best"), (44100, 22050, "best"), (48000, 44100, "best"),
                (2, 3, "best")):
        p = RS.design(*key)
        assert V.resample_route(p.up, p.down, p.P)[0] is True, key
    with pytest.raises(V.VQAError, match="not coprime"):
        V.resample_route(4, 6, 68)
    # a steep ratio shrinks the tile until its input span fits, down to one output per workgroup
    assert V.resample_route(1, 100000, 8192)[1] < V.resample_route(1, 2, 136)[1]
