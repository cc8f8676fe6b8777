"""C-ABI checks of vqa_attn_weights / vqa_attn_weights_elems that need no GPU: every argument is settled on the host,
so a bad call returns before anything is launched (fake device pointers, as tests/test_pcm_abi.py does) with an
"attn_weights:" message, VQA_E_INVALID_ARG for bad arguments and VQA_E_UNSUPPORTED for the shapes the attention
kernels do not take."""
import ctypes
import math

import pytest
import torch

import vqa_lib as V

P = ctypes.c_void_p(0x1000)     # 16-byte aligned fake device pointer
ODD = ctypes.c_void_p(0x1008)   # 8-byte aligned only
ORDER = ["q", "k", "lse", "w", "w_elems", "N", "T", "H", "head_dim", "l", "mode", "scale", "dtype"]
# mode 0: (2*3, 2, 64, 64)
GOOD = dict(q=P, k=P, lse=P, w=P, w_elems=2 * 3 * 2 * 64 * 64, N=2, T=192, H=2, head_dim=16, l=64, mode=0, scale=0.25,
            dtype=V.F32)


def _call(**kw):
    a = {**GOOD, **kw}
    return V.lib().vqa_attn_weights(*[a[k] for k in ORDER], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), "null q, k, lse or w"),
    (dict(k=None), "null q, k, lse or w"),
    (dict(lse=None), "null q, k, lse or w"),
    (dict(w=None), "null q, k, lse or w"),
    (dict(w=ODD), "w is not 16-byte aligned"),
    (dict(w_elems=2 * 3 * 2 * 64 * 64 - 1), "w holds 49151 elements, the layout of mode 0 has 49152"),
    (dict(w_elems=0), "w holds 0 elements"),
    (dict(mode=1, l=64), "the layout of mode 1 has 2304"),      # the mode-0 count for a column layer (2*64*2*3*3)
    (dict(scale=0.0), "scale"),
    (dict(scale=-0.25), "scale"),
    (dict(scale=math.inf), "scale"),
    (dict(scale=math.nan), "scale"),
    (dict(dtype=2), "dtype 2"),
    (dict(dtype=-1), "dtype -1"),
    (dict(N=0), "bad shape"),
    (dict(T=0), "bad shape"),
    (dict(H=-1), "bad shape"),
    (dict(l=0), "bad shape"),
    (dict(T=200), "bad shape"),                                 # not a whole number of blocks
    (dict(mode=3), "bad shape"),
    (dict(mode=-1), "bad shape"),
])
def test_attn_weights_rejects_bad_arguments_before_launch(kw, msg):
    rc = _call(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("attn_weights:") and msg in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(l=96, T=192, w_elems=2 * 2 * 2 * 96 * 96), "block length 96 not a multiple of 64"),
    (dict(l=96, T=192, mode=2, w_elems=2 * 2 * 2 * 96 * 96), "block length 96 not a multiple of 64"),
    (dict(mode=1, l=4, T=36, w_elems=2 * 4 * 2 * 9 * 9), "column attention supports 1..8 blocks (got 9)"),
    (dict(head_dim=32), "head_dim 32 unsupported"),
])
def test_attn_weights_unsupported_shapes(kw, msg):
    rc = _call(**kw)
    assert rc == -2, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("attn_weights:") and msg in err, err


def test_attn_weights_elems_layouts():
    f = V.lib().vqa_attn_weights_elems
    N, T, H, l = 3, 8 * 64, 5, 64
    nb = T // l
    assert f(N, T, H, l, 0) == N * nb * H * l * l
    assert f(N, T, H, l, 2) == N * nb * H * l * l
    assert f(N, T, H, l, 1) == N * l * H * nb * nb
    # ctx 8192 in blocks of 2048, 16 heads, batch 48: 3 * 2^32 elements, beyond 32 bits
    big = f(48, 8192, 16, 2048, 0)
    assert big == 48 * 4 * 16 * 2048 * 2048 and big > 1 << 32
    assert f(48, 8192, 16, 2048, 2) == big
    assert f(1 << 20, 1 << 20, 64, 1 << 17, 1) == (1 << 20) * (1 << 17) * 64 * 8 * 8 > 1 << 32
    for bad in ((0, T, H, l, 0), (N, 0, H, l, 0), (N, T, 0, l, 0), (N, T, H, 0, 0), (N, T + 1, H, l, 0),
                (N, T, H, l, 3), (N, T, H, l, -1), (-2, T, H, l, 1)):
        assert f(*bad) == 0, bad
    # a product beyond size_t is a bad shape too
    assert f(1 << 30, 1 << 30, 1 << 30, 1 << 30, 0) == 0


def test_symbols_exported_and_abi_version_unchanged():
    lib = V.lib()
    for name in ("vqa_attn_weights", "vqa_attn_weights_elems"):
        assert name in V.EXPORTED and hasattr(lib, name)
    assert V.ABI_VERSION == 2 and lib.vqa_abi_version() == 2
    assert callable(V.attn_weights) and callable(V.attn_weights_shape)


def test_attn_weights_shape():
    assert V.attn_weights_shape(2, 192, 3, 64, 0) == (6, 3, 64, 64)
    assert V.attn_weights_shape(2, 192, 3, 64, 2) == (6, 3, 64, 64)
    assert V.attn_weights_shape(2, 15, 3, 5, 1) == (10, 3, 3, 3)
    for bad in ((2, 100, 3, 64, 0), (0, 64, 1, 64, 0), (1, 64, 1, 64, 3)):
        with pytest.raises(V.VQAError, match="attn_weights: bad shape"):
            V.attn_weights_shape(*bad)


def test_wrapper_checks_tensors_on_the_host():
    q = torch.zeros(1, 64, 16)
    lse = torch.zeros(1, 64, 1)
    with pytest.raises(V.VQAError, match="CPU tensor"):                  # CPU tensors never reach the kernel
        V.attn_weights(q, q, lse, 0, 64, 1, 0.25)
    with pytest.raises(V.VQAError, match="float32 or both bfloat16"):
        V.attn_weights(q.double(), q.double(), lse, 0, 64, 1, 0.25)
    with pytest.raises(V.VQAError, match="float32 or both bfloat16"):
        V.attn_weights(q, q.bfloat16(), lse, 0, 64, 1, 0.25)
    with pytest.raises(V.VQAError, match="lse is float32"):
        V.attn_weights(q, q, lse.double(), 0, 64, 1, 0.25)
    with pytest.raises(V.VQAError, match=r"lse is \(1, 64, 1\)"):
        V.attn_weights(q, q, torch.zeros(1, 64, 2), 0, 64, 1, 0.25)
    with pytest.raises(V.VQAError, match="out is float32"):               # wrong shape
        V.attn_weights(q, q, lse, 0, 64, 1, 0.25, out=torch.zeros(1, 1, 64, 63))
    with pytest.raises(V.VQAError, match="out is float32"):               # column layout for a row layer
        V.attn_weights(q, q, lse, 0, 64, 1, 0.25, out=torch.zeros(64, 1, 1, 1))
    with pytest.raises(V.VQAError, match="out is float32"):               # not fp32
        V.attn_weights(q, q, lse, 0, 64, 1, 0.25, out=torch.zeros(1, 1, 64, 64, dtype=torch.bfloat16))
    with pytest.raises(V.VQAError, match="CPU tensor"):                  # a well-formed CPU out is still refused
        V.attn_weights(q, q, lse, 0, 64, 1, 0.25, out=torch.zeros(1, 1, 64, 64))
