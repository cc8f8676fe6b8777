"""C-ABI checks of the step guard's entry points (vqa_grad_finite, vqa_adam_keras_guarded, vqa_counter_add_if,
vqa_step_metrics_if, vqa_vq_ema_apply_guarded) that need no GPU: every argument is settled on the host, so a bad call
returns VQA_E_INVALID_ARG with its message before anything is launched (fake device pointers, as
tests/test_ema_abi.py does)."""
import ctypes
import math
import os
import re

import pytest

import vqa_lib as V

N, NSEG = 90001, 8
P = ctypes.c_void_p(0x1000)          # 16-byte aligned fake device pointer (w, g, m, v, tables)
A = ctypes.c_void_p(0x1000000)       # the average: aligned, N floats away from every other buffer
ODD = ctypes.c_void_p(0x1000004)     # 4-byte aligned only
INSIDE_W = ctypes.c_void_p(0x1000 + 4 * (N - 1))   # the last element of w
STEP = ctypes.c_void_p(0x2000000)    # the step counter (int64)
SKIPS = ctypes.c_void_p(0x2000100)   # the two skip counters (int64[2])
OK = ctypes.c_void_p(0x2000200)      # the flag (int32)

ORDER = ["w", "g", "m", "v", "n", "step", "lr", "lr_dev", "beta1", "beta2", "eps", "grad_scale", "seg_start",
         "block_seg", "nseg", "modes", "clipvalue", "clipnorm", "global_clipnorm", "seg_norm", "stats", "ema",
         "average_decay", "start_step", "dynamic", "ok", "skip_counters"]
PLAIN = dict(w=P, g=P, m=P, v=P, n=N, step=STEP, lr=1e-3, lr_dev=None, beta1=0.9, beta2=0.999, eps=1e-7,
             grad_scale=1.0, seg_start=None, block_seg=None, nseg=0, modes=0, clipvalue=0.0, clipnorm=0.0,
             global_clipnorm=0.0, seg_norm=None, stats=None, ema=None, average_decay=0.0, start_step=0, dynamic=0,
             ok=OK, skip_counters=SKIPS)
EMA = dict(PLAIN, ema=A, average_decay=0.99)
CLIPPED = dict(PLAIN, seg_start=P, block_seg=P, nseg=NSEG, modes=V.CLIP_GLOBAL_NORM, global_clipnorm=1.0, seg_norm=P,
               stats=P)
CLIPPED_EMA = dict(CLIPPED, ema=A, average_decay=0.99)
FORMS = {"plain": PLAIN, "ema": EMA, "clipped": CLIPPED, "clipped_ema": CLIPPED_EMA}


def _guarded(form, **kw):
    a = {**FORMS[form], **kw}
    return V.lib().vqa_adam_keras_guarded(*[a[k] for k in ORDER], None)


def _refused(rc, prefix, msg):
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith(prefix) and msg in err, err


# what every form of the guarded update refuses: the guard's own arguments, then its unguarded twins' checks
GUARD = [
    (dict(ok=None), "null ok flag"),
    (dict(skip_counters=None), "null skip counters"),
    (dict(skip_counters=STEP), "must not alias the step counter"),
    (dict(skip_counters=ctypes.c_void_p(0x2000000 - 8)), "must not alias the step counter"),   # counters[1] is step
    (dict(skip_counters=ctypes.c_void_p(0x2000000 + 4)), "must not alias the step counter"),   # a partial overlap
    (dict(n=0), "n must be > 0"),
    (dict(n=-7), "n must be > 0"),
    (dict(w=None), "null pointer"),
    (dict(g=None), "null pointer"),
    (dict(m=None), "null pointer"),
    (dict(v=None), "null pointer"),
    (dict(step=None), "null pointer"),
    (dict(w=ctypes.c_void_p(0x1004)), "16-byte aligned"),
    (dict(g=ctypes.c_void_p(0x1004)), "16-byte aligned"),
]
AVERAGE = [
    (dict(average_decay=1.0), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=-0.01), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=math.nan), "average_decay must be finite and in [0, 1)"),
    (dict(average_decay=math.inf), "average_decay must be finite and in [0, 1)"),
    (dict(start_step=-1), "start_step must be >= 0"),
    (dict(dynamic=2), "dynamic must be 0 or 1"),
    (dict(ema=P), "must not alias the weights"),
    (dict(ema=INSIDE_W), "must not alias the weights"),
    (dict(ema=ODD), "16-byte aligned"),
]
CLIP = [
    (dict(seg_norm=None), "null pointer"),
    (dict(stats=None), "null pointer"),
    (dict(nseg=0), "nseg must be > 0"),
    (dict(seg_start=None), "null variable table"),
    (dict(block_seg=None), "null variable table"),
    (dict(modes=8), "unknown mode bits"),
    (dict(modes=V.CLIP_NORM | V.CLIP_GLOBAL_NORM, clipnorm=1.0), "exclude each other"),
    (dict(global_clipnorm=0.0), "global_clipnorm must be finite and > 0"),
    (dict(modes=V.CLIP_VALUE, clipvalue=math.nan), "clipvalue must be finite and > 0"),
    (dict(modes=V.CLIP_NORM, clipnorm=-1.0), "clipnorm must be finite and > 0"),
]
CASES = ([(f, kw, msg) for f in FORMS for kw, msg in GUARD]
         + [(f, kw, msg) for f in ("ema", "clipped_ema") for kw, msg in AVERAGE]
         + [(f, kw, msg) for f in ("clipped", "clipped_ema") for kw, msg in CLIP])


@pytest.mark.parametrize("form,kw,msg", CASES)
def test_adam_guarded_rejects_bad_arguments_before_launch(form, kw, msg):
    _refused(_guarded(form, **kw), "adam_guarded:", msg)


def test_adam_guarded_without_an_average_ignores_its_settings():
    """ema == NULL: average_decay, start_step and dynamic are not looked at; the call gets past every check up to
    the one this test trips on purpose (a null gradient)."""
    _refused(_guarded("plain", average_decay=7.0, start_step=-3, dynamic=9, g=None), "adam_guarded:", "null pointer")


@pytest.mark.parametrize("kw,msg", [
    (dict(g=None), "null pointer"),
    (dict(ok=None), "null pointer"),
    (dict(n=0), "n must be > 0"),
    (dict(n=-1), "n must be > 0"),
    (dict(g=ctypes.c_void_p(0x1002)), "4-byte aligned"),
    (dict(ok=ctypes.c_void_p(0x2000202)), "4-byte aligned"),
])
def test_grad_finite_rejects_bad_arguments_before_launch(kw, msg):
    a = {**dict(g=P, n=N, ok=OK), **kw}
    _refused(V.lib().vqa_grad_finite(a["g"], a["n"], a["ok"], None), "grad_finite:", msg)


@pytest.mark.parametrize("kw,msg", [(dict(counter=None), "null pointer"), (dict(ok=None), "null ok flag")])
def test_counter_add_if_rejects_bad_arguments_before_launch(kw, msg):
    a = {**dict(counter=STEP, ok=OK), **kw}
    _refused(V.lib().vqa_counter_add_if(a["counter"], 1, a["ok"], None), "counter_add_if:", msg)


@pytest.mark.parametrize("kw,msg", [
    (dict(ok=None), "null ok flag"),
    (dict(loss_slots=None), "bad arguments"),
    (dict(vq_metrics=None), "bad arguments"),
    (dict(macc=None), "bad arguments"),
    (dict(levels=0), "bad arguments"),
])
def test_step_metrics_if_rejects_bad_arguments_before_launch(kw, msg):
    a = {**dict(loss_slots=P, vq_metrics=P, macc=P, levels=2, ok=OK), **kw}
    rc = V.lib().vqa_step_metrics_if(a["loss_slots"], a["vq_metrics"], a["macc"], a["levels"], 1.0, a["ok"], None)
    _refused(rc, "step_metrics_if:", msg)


EMA_APPLY_ORDER = ["E", "ET", "m_t", "N_t", "m_sumT", "n_sum", "RT", "gamma", "omg", "thresh", "metrics", "counter",
                   "esq", "E3", "D", "K", "ok"]
EMA_APPLY_GOOD = dict(E=P, ET=P, m_t=P, N_t=P, m_sumT=P, n_sum=P, RT=P, gamma=0.99, omg=0.01, thresh=1.0, metrics=P,
                      counter=STEP, esq=P, E3=P, D=64, K=256, ok=OK)


@pytest.mark.parametrize("kw,msg", [(dict(ok=None), "null ok flag")]
                         + [(dict({k: None}), "null pointer")
                            for k in ("E", "ET", "m_t", "N_t", "m_sumT", "n_sum", "RT", "counter")]
                         + [(dict(D=0), "supports D <= 64"), (dict(D=65), "supports D <= 64"),
                            (dict(K=0), "supports D <= 64")])
def test_vq_ema_apply_guarded_rejects_bad_arguments_before_launch(kw, msg):
    a = {**EMA_APPLY_GOOD, **kw}
    _refused(V.lib().vqa_vq_ema_apply_guarded(*[a[k] for k in EMA_APPLY_ORDER], None), "vq_ema_apply_guarded:", msg)


NAMES = ("vqa_grad_finite", "vqa_adam_keras_guarded", "vqa_counter_add_if", "vqa_step_metrics_if",
         "vqa_vq_ema_apply_guarded")


def test_symbols_exported_and_bound_abi_still_2():
    lib = V.lib()
    for name in NAMES:
        assert name in V.EXPORTED and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert all(callable(f) for f in (V.grad_finite, V.adam_keras_guarded, V.counter_add_if, V.step_metrics_if))
    assert lib.vqa_abi_version() == 2 and V.ABI_VERSION == 2


def test_the_header_declares_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vqa.h")).read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", hdr), name
    assert re.search(r"#define VQA_ABI_VERSION 2\b", hdr)
    assert re.search(rf"#define VQA_FINITE_MAX_BLOCKS {V.FINITE_MAX_BLOCKS}\b", hdr)


def test_the_bindings_refuse_a_flag_that_is_not_int32():
    import torch
    with pytest.raises(V.VQAError, match="int32"):
        V.grad_finite(torch.zeros(4), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(V.VQAError, match="float32"):
        V.grad_finite(torch.zeros(4, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
