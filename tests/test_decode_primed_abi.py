"""C-ABI checks of vqa_prior_decode_primed that need no GPU: the prime, the temperature and top-k are settled on
the host, so a bad combination returns VQA_E_INVALID_ARG and a message before anything is launched (fake device
pointers, as tests/test_abi.py does for the decoder tail)."""
import ctypes

import pytest

import vqa_lib as V

N, STEPS, CTX, WIDTH, HEADS, BLOCKS, BINS, DEPTH = 2, 16, 16, 128, 2, 4, 64, 2
P = ctypes.c_void_p(0x1000)


def _call(forced=None, prime=None, prime_len=0, temperature=1.0, top_k=0):
    lib = V.lib()
    layers = (V.PriorLayerDesc * DEPTH)()
    cache_bytes = lib.vqa_prior_decode_cache_bytes(N, DEPTH, CTX)
    assert cache_bytes > 0
    return lib.vqa_prior_decode_primed(layers, DEPTH, P, P, P, P, None, None, forced, None, P, P, cache_bytes, N,
                                       STEPS, CTX, WIDTH, HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, prime, prime_len,
                                       temperature, top_k, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(prime=P, prime_len=STEPS + 1), "prime_len 17 outside"),
    (dict(prime=P, prime_len=-1), "prime_len -1 outside"),
    (dict(prime=None, prime_len=3), "without a prime"),
    (dict(prime=P, prime_len=4, forced=P), "mutually exclusive"),
    (dict(temperature=0.0), "temperature"),
    (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("inf")), "temperature"),
    (dict(temperature=float("nan")), "temperature"),
    (dict(top_k=-1), "top_k -1 outside"),
    (dict(top_k=BINS + 1), "top_k 65 outside"),
])
def test_primed_decode_rejects_bad_arguments_before_launch(kw, msg):
    rc = _call(**kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("prior_decode:") and msg in err, err


def test_both_entry_points_resolve():
    lib = V.lib()
    assert hasattr(lib, "vqa_prior_decode") and hasattr(lib, "vqa_prior_decode_primed")
    assert "vqa_prior_decode" in V.EXPORTED and "vqa_prior_decode_primed" in V.EXPORTED
    # the old entry point keeps its argument list: it has no prime to reject and still checks its own arguments
    layers = (V.PriorLayerDesc * DEPTH)()
    rc = lib.vqa_prior_decode(layers, DEPTH, P, P, P, P, None, None, None, None, P, P, 0, N, STEPS + 1, CTX, WIDTH,
                              HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, None)
    assert rc == -1 and "prior_decode: bad arguments" in V.last_error()
