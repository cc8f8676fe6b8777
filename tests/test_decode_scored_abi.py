"""C-ABI checks of vqa_prior_decode_scored that need no GPU: it is vqa_prior_decode_filtered plus two trailing
log-probability outputs, so every argument that entry point rejects is rejected here with VQA_E_INVALID_ARG and a
message before anything is launched, whichever of the two outputs is asked for (fake device pointers, as
tests/test_decode_filtered_abi.py does). The older entry points keep their argument lists and their checks, and
VQVAESampler refuses a bad best_of before it touches a prior."""
import ctypes
import types

import pytest

import vqa_lib as V

N, STEPS, CTX, WIDTH, HEADS, BLOCKS, BINS, DEPTH = 2, 16, 16, 128, 2, 4, 64, 2
P = ctypes.c_void_p(0x1000)
OUTPUTS = [(None, None), (P, None), (None, P), (P, P)]


def _call(forced=None, prime=None, prime_len=0, temperature=1.0, top_k=0, top_p=1.0, kept=None, steps=STEPS,
          logp_model=None, logp_draw=None, cache_bytes=None):
    lib = V.lib()
    layers = (V.PriorLayerDesc * DEPTH)()
    if cache_bytes is None:
        cache_bytes = lib.vqa_prior_decode_cache_bytes(N, DEPTH, CTX)
        assert cache_bytes > 0
    return lib.vqa_prior_decode_scored(layers, DEPTH, P, P, P, P, None, None, forced, None, P, P, cache_bytes, N,
                                       steps, CTX, WIDTH, HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, prime, prime_len,
                                       temperature, top_k, top_p, kept, logp_model, logp_draw, None)


def test_the_symbol_resolves_and_is_exported():
    assert hasattr(V.lib(), "vqa_prior_decode_scored")
    assert "vqa_prior_decode_scored" in V.EXPORTED
    # a new entry point, no changed signature: the revision stays
    assert V.lib().vqa_abi_version() == V.ABI_VERSION == 2


def test_the_binding_takes_the_two_outputs_last_before_the_stream():
    fn = V.lib().vqa_prior_decode_scored
    assert fn.restype is ctypes.c_int
    assert len(fn.argtypes) == len(V.lib().vqa_prior_decode_filtered.argtypes) + 2
    assert list(fn.argtypes[-3:]) == [ctypes.c_void_p] * 3


@pytest.mark.parametrize("top_p", [0.0, -0.1, 1.5, float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("lm,ld", OUTPUTS)
def test_bad_top_p_is_rejected_before_launch(top_p, lm, ld):
    rc = _call(top_p=top_p, logp_model=lm, logp_draw=ld)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("prior_decode:") and "top_p" in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(prime=P, prime_len=STEPS + 1), "prime_len 17 outside"),
    (dict(prime=P, prime_len=-1), "prime_len -1 outside"),
    (dict(prime=None, prime_len=3), "without a prime"),
    (dict(prime=P, prime_len=4, forced=P), "mutually exclusive"),
    (dict(temperature=0.0), "temperature"),
    (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("nan")), "temperature"),
    (dict(temperature=float("inf")), "temperature"),
    (dict(top_k=-1), "top_k -1 outside"),
    (dict(top_k=BINS + 1), "top_k 65 outside"),
    (dict(steps=CTX + 1), "bad arguments"),
    (dict(steps=0), "bad arguments"),
    (dict(cache_bytes=16), "cache too small"),
])
@pytest.mark.parametrize("lm,ld", OUTPUTS)
@pytest.mark.parametrize("kept", [None, P])
def test_what_filtered_rejects_is_rejected(kw, msg, lm, ld, kept):
    rc = _call(logp_model=lm, logp_draw=ld, kept=kept, **kw)
    assert rc == -1, (rc, V.last_error())
    err = V.last_error()
    assert err.startswith("prior_decode:") and msg in err, err


def test_the_older_entry_points_resolve_and_reject_what_they_rejected():
    lib = V.lib()
    layers = (V.PriorLayerDesc * DEPTH)()
    cache_bytes = lib.vqa_prior_decode_cache_bytes(N, DEPTH, CTX)
    for name in ("vqa_prior_decode", "vqa_prior_decode_primed", "vqa_prior_decode_filtered"):
        assert hasattr(lib, name) and name in V.EXPORTED
    rc = lib.vqa_prior_decode_filtered(layers, DEPTH, P, P, P, P, None, None, None, None, P, P, cache_bytes, N, STEPS,
                                       CTX, WIDTH, HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, None, 0, 1.0, 0, 0.0, None,
                                       None)
    assert rc == -1 and "top_p" in V.last_error()
    rc = lib.vqa_prior_decode_primed(layers, DEPTH, P, P, P, P, None, None, None, None, P, P, cache_bytes, N, STEPS,
                                     CTX, WIDTH, HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, None, 3, 1.0, 0, None)
    assert rc == -1 and "without a prime" in V.last_error()
    rc = lib.vqa_prior_decode(layers, DEPTH, P, P, P, P, None, None, None, None, P, P, 0, N, STEPS + 1, CTX, WIDTH,
                              HEADS, BLOCKS, BINS, BINS, BINS - 1, 0, None)
    assert rc == -1 and "prior_decode: bad arguments" in V.last_error()


class _NoPrior:
    """Stands where a Prior would: any use of it is a launch that the argument check should have prevented."""

    def __getattr__(self, name):
        raise AssertionError(f"the sampler reached for its prior ({name}) before refusing best_of")


@pytest.mark.parametrize("best_of", [0, -1, 1.5, 2.0, "2", None, True])
def test_bad_best_of_is_a_value_error_before_any_launch(best_of):
    from sampler import VQVAESampler
    s = VQVAESampler([1], [2], [16], codebook_size=64, priors=[_NoPrior()])
    with pytest.raises(ValueError, match="best_of"):
        s.sample(2, best_of=best_of)
    with pytest.raises(ValueError, match="best_of"):
        s.sample(2, best_of=best_of, return_logprobs=True, total_length=32)
    vqvae = types.SimpleNamespace(levels=1, decode_hops=[2])
    with pytest.raises(ValueError, match="best_of"):
        s.sample_audio(2, vqvae, best_of=best_of)
