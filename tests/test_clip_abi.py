"""C-ABI checks of the gradient-clipping entry points (vqa_grad_norm, vqa_grad_norm_workspace,
vqa_adam_keras_clipped) that need no GPU: every argument is settled on the host, so a bad call returns
VQA_E_INVALID_ARG with its message before anything is launched (fake device pointers, as tests/test_feed_abi.py
does)."""
import ctypes
import math

import pytest

import vqa_lib as V

P = ctypes.c_void_p(0x1000)     # 16-byte aligned fake device pointer
ODD = ctypes.c_void_p(0x1004)   # 4-byte aligned only
N, NSEG = 90001, 8
WS = 1 << 20

NORM_ORDER = ["g", "n", "seg_start", "block_seg", "nseg", "grad_scale", "modes", "clipvalue", "clipnorm",
              "global_clipnorm", "seg_norm", "stats", "ws", "ws_bytes"]
NORM_GOOD = dict(g=P, n=N, seg_start=P, block_seg=P, nseg=NSEG, grad_scale=1.0, modes=V.CLIP_GLOBAL_NORM,
                 clipvalue=0.0, clipnorm=0.0, global_clipnorm=1.0, seg_norm=P, stats=P, ws=P, ws_bytes=WS)
ADAM_ORDER = ["w", "g", "m", "v", "n", "step", "lr", "lr_dev", "beta1", "beta2", "eps", "grad_scale", "seg_start",
              "block_seg", "nseg", "modes", "clipvalue", "clipnorm", "global_clipnorm", "seg_norm", "stats"]
ADAM_GOOD = dict(w=P, g=P, m=P, v=P, n=N, step=P, lr=1e-3, lr_dev=None, beta1=0.9, beta2=0.999, eps=1e-7,
                 grad_scale=1.0, seg_start=P, block_seg=P, nseg=NSEG, modes=V.CLIP_GLOBAL_NORM, clipvalue=0.0,
                 clipnorm=0.0, global_clipnorm=1.0, seg_norm=P, stats=P)


def _norm(**kw):
    a = {**NORM_GOOD, **kw}
    return V.lib().vqa_grad_norm(*[a[k] for k in NORM_ORDER], None)


def _adam(**kw):
    a = {**ADAM_GOOD, **kw}
    return V.lib().vqa_adam_keras_clipped(*[a[k] for k in ADAM_ORDER], None)


# cases both entry points share: sizes, tables, modes and thresholds
COMMON = [
    (dict(n=0), "n must be > 0"),
    (dict(n=-5), "n must be > 0"),
    (dict(nseg=0), "nseg must be > 0"),
    (dict(nseg=-1), "nseg must be > 0"),
    (dict(seg_start=None), "null variable table"),
    (dict(block_seg=None), "null variable table"),
    (dict(modes=8), "unknown mode bits"),
    (dict(modes=V.CLIP_NORM | V.CLIP_GLOBAL_NORM, clipnorm=1.0), "exclude each other"),
    (dict(modes=V.CLIP_VALUE | V.CLIP_NORM | V.CLIP_GLOBAL_NORM, clipvalue=1.0, clipnorm=1.0), "exclude each other"),
    (dict(global_clipnorm=0.0), "global_clipnorm must be finite and > 0"),
    (dict(global_clipnorm=-1.0), "global_clipnorm must be finite and > 0"),
    (dict(global_clipnorm=math.inf), "global_clipnorm must be finite and > 0"),
    (dict(global_clipnorm=math.nan), "global_clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_NORM, clipnorm=0.0), "clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_NORM, clipnorm=-2.0), "clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_NORM, clipnorm=math.inf), "clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_NORM, clipnorm=math.nan), "clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE, clipvalue=0.0), "clipvalue must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE, clipvalue=-0.5), "clipvalue must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE, clipvalue=-math.inf), "clipvalue must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE, clipvalue=math.nan), "clipvalue must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE | V.CLIP_GLOBAL_NORM, clipvalue=math.nan), "clipvalue must be finite and > 0"),
]


@pytest.mark.parametrize("kw,msg", COMMON + [
    (dict(g=None), "null pointer"),
    (dict(seg_norm=None), "null pointer"),
    (dict(stats=None), "null pointer"),
    (dict(g=ODD), "16-byte aligned"),
    (dict(ws=None), "workspace too small"),
    (dict(ws_bytes=0), "workspace too small"),
])
def test_grad_norm_rejects_bad_arguments_before_launch(kw, msg):
    rc = _norm(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("grad_norm:") and msg in err, err


def test_grad_norm_workspace_one_byte_short_is_rejected():
    need = V.grad_norm_workspace(N, NSEG)
    assert need > 0
    assert _norm(ws_bytes=need - 1) == -1 and "workspace too small" in V.last_error()


@pytest.mark.parametrize("kw,msg", COMMON + [
    (dict(w=None), "null pointer"),
    (dict(g=None), "null pointer"),
    (dict(m=None), "null pointer"),
    (dict(v=None), "null pointer"),
    (dict(step=None), "null pointer"),
    (dict(seg_norm=None), "null pointer"),
    (dict(stats=None), "null pointer"),
    (dict(w=ODD), "16-byte aligned"),
    (dict(v=ODD), "16-byte aligned"),
])
def test_adam_clipped_rejects_bad_arguments_before_launch(kw, msg):
    rc = _adam(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("adam_clipped:") and msg in err, err


def test_thresholds_of_modes_that_are_off_are_ignored():
    # only the workspace check is left to fail: every threshold check passed
    assert _norm(modes=V.CLIP_GLOBAL_NORM, clipvalue=math.nan, clipnorm=-1.0, ws_bytes=0) == -1
    assert "workspace too small" in V.last_error()


def test_workspace_query_is_monotone():
    W = V.grad_norm_workspace
    assert W(0, 4) == 0 and W(-3, 4) == 0 and W(100, 0) == 0
    ns = [1, 4, 4095, 4096, 4097, 90001, 968835, 1 << 24, (1 << 31) + 5]
    for nseg in (1, 8, 300):
        sizes = [W(n, nseg) for n in ns]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, sizes
    for n in (1, 4097, 968835):
        sizes = [W(n, s) for s in (1, 2, 8, 300, 5000)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # room for one 3-word slot per block and variable plus 3 words per variable
    assert W(90001, 8) >= 4 * (3 * (-(-90001 // V.CLIP_BLOCK) + 8) + 3 * 8)


def test_symbols_exported_and_bound_abi_still_2():
    lib = V.lib()
    for name in ("vqa_grad_norm", "vqa_grad_norm_workspace", "vqa_adam_keras_clipped"):
        assert name in V.EXPORTED and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert callable(V.grad_norm) and callable(V.adam_keras_clipped) and callable(V.grad_norm_workspace)
    assert lib.vqa_abi_version() == 2 and V.ABI_VERSION == 2


def test_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vqa.h")).read()
    assert int(re.search(r"#define VQA_CLIP_BLOCK (\d+)", hdr).group(1)) == V.CLIP_BLOCK
    assert int(re.search(r"#define VQA_CLIP_STATS (\d+)", hdr).group(1)) == V.CLIP_STATS
    m = re.search(r"VQA_CLIP_VALUE = (\d+), VQA_CLIP_NORM = (\d+), VQA_CLIP_GLOBAL_NORM = (\d+)", hdr)
    assert tuple(map(int, m.groups())) == (V.CLIP_VALUE, V.CLIP_NORM, V.CLIP_GLOBAL_NORM)
