"""C-ABI checks of vqa_pcm_splice that need no GPU: every argument is settled on the host, so a bad call returns
VQA_E_INVALID_ARG with a "pcm_splice:" message before anything is launched (fake device pointers, as
tests/test_pcm_abi.py does): everything vqa_pcm_encode rejects, and the rules of the second source and the seam."""
import ctypes
import math

import pytest

import vqa_lib as V

P = ctypes.c_void_p(0x1000)       # 16-byte aligned fake device pointer
ODD2 = ctypes.c_void_p(0x1002)    # 2-byte aligned only
ODD1 = ctypes.c_void_p(0x1001)    # not even 2-byte aligned
GOOD = dict(x=P, ldx=1037, p=P, ldp=300, out=P, ldo=2051, B=3, x0=3, o0=5, n=515, seam=300, fade=40, gain=1.0,
            clipped=P)
ORDER = ["x", "ldx", "p", "ldp", "out", "ldo", "B", "x0", "o0", "n", "seam", "fade", "gain", "clipped"]


def _call(**kw):
    a = {**GOOD, **kw}
    return V.lib().vqa_pcm_splice(*[a[k] for k in ORDER], None)


@pytest.mark.parametrize("kw,msg", [
    # what vqa_pcm_encode rejects
    (dict(x=None), "null x or out"),
    (dict(out=None), "null x or out"),
    (dict(B=0), "must be positive"),
    (dict(B=-2), "must be positive"),
    (dict(n=0), "must be positive"),
    (dict(n=-7), "must be positive"),
    (dict(B=65536), "above 65535"),
    (dict(x0=-1), "negative x0 -1"),
    (dict(o0=-4), "negative x0 3 or o0 -4"),
    (dict(x0=523), "x0 523 + n 515 exceeds the row of ldx 1037"),
    (dict(x0=2000), "exceeds the row of ldx 1037"),
    (dict(n=1035), "x0 3 + n 1035 exceeds the row of ldx 1037"),
    (dict(o0=1537), "o0 1537 + n 515 exceeds the row of ldo 2051"),
    (dict(o0=3000), "exceeds the row of ldo 2051"),
    (dict(ldx=0), "exceeds the row of ldx 0"),
    (dict(ldo=-5), "exceeds the row of ldo -5"),
    (dict(n=(1 << 63) - 1), "exceeds the row"),
    (dict(x=ODD2), "x is not 4-byte aligned"),
    (dict(out=ODD1), "out is not 2-byte aligned"),
    (dict(clipped=ODD2), "clipped is not 4-byte aligned"),
    (dict(gain=-0.5), "gain"),
    (dict(gain=math.inf), "gain"),
    (dict(gain=-math.inf), "gain"),
    (dict(gain=math.nan), "gain"),
    # the second source and the seam
    (dict(p=None), "null p"),
    (dict(p=ODD2), "p is not 4-byte aligned"),
    (dict(seam=-1, fade=0), "negative seam -1"),
    (dict(fade=-1), "fade -1 outside [0, seam 300]"),
    (dict(fade=301), "fade 301 outside [0, seam 300]"),
    (dict(seam=0, fade=1, ldp=0), "fade 1 outside [0, seam 0]"),
    (dict(ldp=299), "ldp 299 is short of min(seam 300, o0 + n 520)"),       # the seam inside the launch
    (dict(seam=1000, ldp=519), "ldp 519 is short of min(seam 1000, o0 + n 520)"),  # the seam past the launch
    (dict(ldp=-1, seam=0, fade=0), "ldp -1 is short"),
])
def test_pcm_splice_rejects_bad_arguments_before_launch(kw, msg):
    rc = _call(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("pcm_splice:") and msg in err, err


def test_symbol_exported_and_bound():
    lib = V.lib()
    assert "vqa_pcm_splice" in V.EXPORTED and hasattr(lib, "vqa_pcm_splice")
    assert callable(V.pcm_splice)


def test_wrapper_checks_tensors_on_the_host():
    import torch
    x, p = torch.zeros(2, 16), torch.zeros(2, 8)
    out = torch.zeros(2, 16, dtype=torch.int16)
    with pytest.raises(V.VQAError):
        V.pcm_splice(x, p, out, 8)                                      # CPU tensors never reach the kernel
    with pytest.raises(V.VQAError):
        V.pcm_splice(x.double(), p, out, 8)
    with pytest.raises(V.VQAError):
        V.pcm_splice(x, p.double(), out, 8)
    with pytest.raises(V.VQAError):
        V.pcm_splice(x, p, out.to(torch.int32), 8)
    with pytest.raises(V.VQAError):
        V.pcm_splice(x, torch.zeros(3, 8), out, 8)
    with pytest.raises(V.VQAError):
        V.pcm_splice(x, p, torch.zeros(3, 16, dtype=torch.int16), 8)
    with pytest.raises(V.VQAError):
        V.pcm_splice(x, p, out, 8, clipped=torch.zeros(2, dtype=torch.int64))
