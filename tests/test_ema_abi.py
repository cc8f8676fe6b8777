"""C-ABI checks of the weight-averaging entry points (vqa_adam_keras_ema, vqa_adam_keras_clipped_ema, vqa_swap_f32)
that need no GPU: every argument is settled on the host, so a bad call returns VQA_E_INVALID_ARG with its message
before anything is launched (fake device pointers, as tests/test_clip_abi.py does)."""
import ctypes
import math

import pytest

import vqa_lib as V

N, NSEG = 90001, 8
P = ctypes.c_void_p(0x1000)          # 16-byte aligned fake device pointer (w, g, m, v, tables)
A = ctypes.c_void_p(0x1000000)       # the average: aligned, N floats away from every other buffer
ODD = ctypes.c_void_p(0x1000004)     # 4-byte aligned only
INSIDE_W = ctypes.c_void_p(0x1000 + 4 * (N - 1))   # the last element of w

PLAIN_ORDER = ["w", "g", "m", "v", "n", "step", "lr", "lr_dev", "beta1", "beta2", "eps", "grad_scale", "ema",
               "average_decay", "start_step", "dynamic"]
PLAIN_GOOD = dict(w=P, g=P, m=P, v=P, n=N, step=P, lr=1e-3, lr_dev=None, beta1=0.9, beta2=0.999, eps=1e-7,
                  grad_scale=1.0, ema=A, average_decay=0.99, start_step=0, dynamic=0)
CLIP_ORDER = PLAIN_ORDER[:12] + ["seg_start", "block_seg", "nseg", "modes", "clipvalue", "clipnorm", "global_clipnorm",
                                 "seg_norm", "stats"] + PLAIN_ORDER[12:]
CLIP_GOOD = dict(PLAIN_GOOD, seg_start=P, block_seg=P, nseg=NSEG, modes=V.CLIP_GLOBAL_NORM, clipvalue=0.0,
                 clipnorm=0.0, global_clipnorm=1.0, seg_norm=P, stats=P)


def _plain(**kw):
    a = {**PLAIN_GOOD, **kw}
    return V.lib().vqa_adam_keras_ema(*[a[k] for k in PLAIN_ORDER], None)


def _clipped(**kw):
    a = {**CLIP_GOOD, **kw}
    return V.lib().vqa_adam_keras_clipped_ema(*[a[k] for k in CLIP_ORDER], None)


# what both averaging entry points refuse
COMMON = [
    (dict(ema=None), "null average"),
    (dict(n=0), "n must be > 0"),
    (dict(n=-7), "n must be > 0"),
    (dict(average_decay=1.0), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=1.5), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=-0.01), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=math.inf), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=-math.inf), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=math.nan), "average_decay must be finite and in [0, 1)"),
    (dict(start_step=-1), "start_step must be >= 0"),
    (dict(dynamic=2), "dynamic must be 0 or 1"),
    (dict(dynamic=-1), "dynamic must be 0 or 1"),
    (dict(ema=P), "must not alias the weights"),
    (dict(ema=INSIDE_W), "must not alias the weights"),
    (dict(w=None), "null pointer"),
    (dict(g=None), "null pointer"),
    (dict(m=None), "null pointer"),
    (dict(v=None), "null pointer"),
    (dict(step=None), "null pointer"),
]


@pytest.mark.parametrize("kw,msg", COMMON)
def test_adam_ema_rejects_bad_arguments_before_launch(kw, msg):
    rc = _plain(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("adam_ema:") and msg in err, err


@pytest.mark.parametrize("kw,msg", COMMON + [
    (dict(ema=ODD), "16-byte aligned"),
    (dict(w=ctypes.c_void_p(0x1004)), "16-byte aligned"),
    (dict(seg_norm=None), "null pointer"),
    (dict(stats=None), "null pointer"),
    # the clipping checks of vqa_adam_keras_clipped still hold
    (dict(nseg=0), "nseg must be > 0"),
    (dict(seg_start=None), "null variable table"),
    (dict(modes=8), "unknown mode bits"),
    (dict(modes=V.CLIP_NORM | V.CLIP_GLOBAL_NORM, clipnorm=1.0), "exclude each other"),
    (dict(global_clipnorm=0.0), "global_clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE, clipvalue=math.nan), "clipvalue must be finite and > 0"),
])
def test_adam_clipped_ema_rejects_bad_arguments_before_launch(kw, msg):
    rc = _clipped(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("adam_clipped_ema:") and msg in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(a=None), "null pointer"),
    (dict(b=None), "null pointer"),
    (dict(n=0), "n must be > 0"),
    (dict(n=-1), "n must be > 0"),
    (dict(b=P), "must not be the same or overlap"),
    (dict(b=INSIDE_W), "must not be the same or overlap"),
    (dict(a=INSIDE_W), "must not be the same or overlap"),
])
def test_swap_rejects_bad_arguments_before_launch(kw, msg):
    a = {**dict(a=P, b=A, n=N), **kw}
    if kw.get("a") is INSIDE_W:
        a["b"] = P
    rc = V.lib().vqa_swap_f32(a["a"], a["b"], a["n"], None)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("swap:") and msg in err, err


def test_the_bindings_refuse_mismatched_buffers():
    import torch
    with pytest.raises(V.VQAError, match="equal size"):
        V.swap_f32(torch.zeros(4), torch.zeros(5))
    with pytest.raises(V.VQAError, match="float32"):
        V.swap_f32(torch.zeros(4), torch.zeros(4, dtype=torch.float64))


def test_symbols_exported_and_bound_abi_still_2():
    lib = V.lib()
    for name in ("vqa_adam_keras_ema", "vqa_adam_keras_clipped_ema", "vqa_swap_f32"):
        assert name in V.EXPORTED and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert callable(V.adam_keras_ema) and callable(V.adam_keras_clipped_ema) and callable(V.swap_f32)
    assert lib.vqa_abi_version() == 2 and V.ABI_VERSION == 2


def test_the_header_declares_the_entry_points():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vqa.h")).read()
    for name in ("vqa_adam_keras_ema", "vqa_adam_keras_clipped_ema", "vqa_swap_f32"):
        assert re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"#define VQA_ABI_VERSION 2\b", hdr)
