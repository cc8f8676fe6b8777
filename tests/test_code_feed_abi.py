"""C-ABI checks of the code feed that need no GPU: vqa_code_batch settles its arguments on the host, so a bad call
returns VQA_E_INVALID_ARG with a "code_batch:" message before anything is launched (fake device pointers, as
tests/test_feed_abi.py does)."""
import ctypes

import pytest

import vqa_lib as V

P = ctypes.c_void_p(0x1000)      # 16-byte aligned fake device pointer
ODD = ctypes.c_void_p(0x1008)    # 8-byte aligned only
ODD4 = ctypes.c_void_p(0x1004)   # 4-byte aligned only
GOOD = dict(codes=P, codes_len=1 << 20, upper=P, upper_len=1 << 18, rate=4, width=0, starts=P, labels=P, M=64, z=P,
            z_upper=P, labels_out=P, index_out=P, B=4, T=4096, seed=1, counter=P, step=0, rank=0, world=2, shuffle=1)
ORDER = ["codes", "codes_len", "upper", "upper_len", "rate", "width", "starts", "labels", "M", "z", "z_upper",
         "labels_out", "index_out", "B", "T", "seed", "counter", "step", "rank", "world", "shuffle"]


def _call(**kw):
    a = {**GOOD, **kw}
    return V.lib().vqa_code_batch(*[a[k] for k in ORDER], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(codes=None), "null"),
    (dict(starts=None), "null"),
    (dict(z=None), "null"),
    (dict(B=0), "positive"),
    (dict(B=-3), "positive"),
    (dict(T=0), "positive"),
    (dict(T=-4), "positive"),
    (dict(M=0), "positive"),
    (dict(M=-1), "positive"),
    (dict(B=65536, M=1 << 20), "above 65535"),
    (dict(rate=0), "rate 0 < 1"),
    (dict(rate=-2), "rate -2 < 1"),
    (dict(rate=3), "not a multiple of rate 3"),
    (dict(z_upper=None), "given together"),
    (dict(upper=None), "given together"),
    (dict(width=2), "width 2"),
    (dict(width=-1), "width -1"),
    (dict(codes=ODD), "16-byte aligned"),
    (dict(upper=ODD), "16-byte aligned"),
    (dict(z=ODD4), "8-byte aligned"),
    (dict(z_upper=ODD4), "8-byte aligned"),
    (dict(labels_out=ODD4), "8-byte aligned"),
    (dict(index_out=ODD4), "8-byte aligned"),
    (dict(world=0), "world 0"),
    (dict(rank=-1), "rank -1 outside"),
    (dict(rank=2), "rank 2 outside"),
    (dict(M=7), "M 7 windows < B*world = 8"),
    (dict(labels=None), "labels_out given without labels"),
    (dict(step=-1), "negative"),
    (dict(codes_len=-1), "negative"),
])
def test_code_batch_rejects_bad_arguments_before_launch(kw, msg):
    rc = _call(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("code_batch:") and msg in err, err


def test_symbol_exported_and_constants():
    assert "vqa_code_batch" in V.EXPORTED and hasattr(V.lib(), "vqa_code_batch")
    assert (V.CODE_I16, V.CODE_I32) == (0, 1)
    assert V.lib().vqa_abi_version() == V.ABI_VERSION == 2     # a symbol is added, none changes
