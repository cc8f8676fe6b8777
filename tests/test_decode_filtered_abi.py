"""C-ABI checks of vqa_prior_decode_filtered that need no GPU: top_p is settled on the host next to the prime, the
temperature and top-k, so a bad value returns VQA_E_INVALID_ARG and a message before anything is launched (fake
device pointers, as tests/test_decode_primed_abi.py does). The two older decode entry points keep their argument
lists and their checks."""
import ctypes

import pytest

import vqa_lib as V

N, STEPS, CTX, WIDTH, HEADS, BLOCKS, BINS, DEPTH = 2, 16, 16, 128, 2, 4, 64, 2
P = ctypes.c_void_p(0x1000)


def _call(forced=None, prime=None, prime_len=0, temperature=1.0, top_k=0, top_p=1.0, kept=None, steps=STEPS):
    lib = V.lib()
    layers = (V.PriorLayerDesc * DEPTH)()
    cache_bytes = lib.vqa_prior_decode_cache_bytes(N, DEPTH, CTX)
    assert cache_bytes > 0
    return lib.vqa_prior_decode_filtered(layers, DEPTH, P, P, P, P, None, None, forced, None, P, P, cache_bytes, N,
                                         steps, CTX, WIDTH, HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, prime, prime_len,
                                         temperature, top_k, top_p, kept, None)


def test_the_symbol_resolves_and_is_exported():
    assert hasattr(V.lib(), "vqa_prior_decode_filtered")
    assert "vqa_prior_decode_filtered" in V.EXPORTED


@pytest.mark.parametrize("top_p", [0.0, -0.1, 1.5, float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("kept", [None, P])
def test_bad_top_p_is_rejected_before_launch(top_p, kept):
    rc = _call(top_p=top_p, kept=kept)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("prior_decode:") and "top_p" in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(prime=P, prime_len=STEPS + 1), "prime_len 17 outside"),
    (dict(prime=P, prime_len=-1), "prime_len -1 outside"),
    (dict(prime=None, prime_len=3), "without a prime"),
    (dict(prime=P, prime_len=4, forced=P), "mutually exclusive"),
    (dict(temperature=0.0), "temperature"),
    (dict(temperature=float("nan")), "temperature"),
    (dict(top_k=-1), "top_k -1 outside"),
    (dict(top_k=BINS + 1), "top_k 65 outside"),
    (dict(steps=CTX + 1), "bad arguments"),
])
@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_the_old_errors_are_still_reported(kw, msg, top_p):
    rc = _call(top_p=top_p, **kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("prior_decode:") and msg in err, err


def test_the_two_old_entry_points_resolve_and_reject_what_they_rejected():
    lib = V.lib()
    assert hasattr(lib, "vqa_prior_decode") and hasattr(lib, "vqa_prior_decode_primed")
    assert "vqa_prior_decode" in V.EXPORTED and "vqa_prior_decode_primed" in V.EXPORTED
    layers = (V.PriorLayerDesc * DEPTH)()
    cache_bytes = lib.vqa_prior_decode_cache_bytes(N, DEPTH, CTX)
    rc = lib.vqa_prior_decode(layers, DEPTH, P, P, P, P, None, None, None, None, P, P, 0, N, STEPS + 1, CTX, WIDTH,
                              HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, None)
    assert rc == -1 and "prior_decode: bad arguments" in V.last_error()
    for kw, msg in [(dict(prime=None, prime_len=3), "without a prime"), (dict(temperature=0.0), "temperature"),
                    (dict(top_k=BINS + 1), "top_k 65 outside")]:
        a = dict(prime=None, prime_len=0, temperature=1.0, top_k=0)
        a.update(kw)
        rc = lib.vqa_prior_decode_primed(layers, DEPTH, P, P, P, P, None, None, None, None, P, P, cache_bytes, N,
                                         STEPS, CTX, WIDTH, HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, a["prime"],
                                         a["prime_len"], a["temperature"], a["top_k"], None)
        err = V.last_error()
        assert rc == -1 and err.startswith("prior_decode:") and msg in err, (rc, err)
