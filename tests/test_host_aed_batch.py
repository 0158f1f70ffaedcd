"""Host-side checks of the batched step-wise AED decoder's C ABI (eec_decoder_batch_*): sizing and argument checks run without a
device (every rejection below happens before any HIP call)."""
import ctypes as C

import pytest

from early_exit_transformer_amd import capi

GEO = (256, 8, 2048, 256, 6)  # d_model, n_heads, d_ff, vocab, n_layers: the bench's AED decoder


@pytest.fixture(scope="module")
def lib():
    import os
    from early_exit_transformer_amd.build import LIB_PATH
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _bytes(lib, E=6, B=8, S_max=85, Tq=256, geo=GEO):
    return lib.eec_decoder_batch_cache_bytes(*geo, E, B, S_max, Tq)


def test_batch_cache_bytes_is_exported_and_grows_with_exits_utterances_and_steps(lib):
    assert "eec_decoder_batch_cache_bytes" in capi.EXPORTS
    base = _bytes(lib)
    assert base > 0
    assert _bytes(lib, B=9) > base and _bytes(lib, B=64) > _bytes(lib, B=9)
    assert _bytes(lib, E=7) > base and _bytes(lib, E=5) < base
    assert _bytes(lib, S_max=86) > base
    assert _bytes(lib, Tq=257) > base
    # at least the memory and self-attention key / value caches: E * B * L * 2D * (Tq + 16 * S_max) floats
    E, B, L, D = 6, 8, GEO[4], GEO[0]
    assert base >= 4 * E * B * L * 2 * D * (256 + 16 * 85)
    # one utterance, one exit: at least the single-session cache
    assert _bytes(lib, E=1, B=1) >= lib.eec_decoder_cache_bytes(*GEO, 85, 256)


@pytest.mark.parametrize("geo,E,B", [((384, 8, 2048, 256, 6), 6, 4),   # head dim 48
                                     ((256, 8, 4096, 256, 6), 6, 4),   # d_ff beyond the step decoder's
                                     ((2048, 32, 2048, 256, 6), 6, 4),  # d_model beyond 1024
                                     (GEO, 0, 4), (GEO, 9, 4), (GEO, 6, 0)])
def test_batch_cache_bytes_is_zero_where_the_step_decoder_does_not_serve(lib, geo, E, B):
    assert lib.eec_decoder_batch_cache_bytes(*geo, E, B, 85, 256) == 0


def test_batch_cache_bytes_serves_what_the_step_decoder_serves(lib):
    for geo in [(256, 8, 2048, 256, 6), (512, 8, 2048, 256, 6), (64, 8, 128, 32, 2), (128, 16, 256, 500, 1), (1024, 16, 2048, 256, 2)]:
        assert lib.eec_decoder_cache_bytes(*geo, 40, 300) > 0
        assert lib.eec_decoder_batch_cache_bytes(*geo, 3, 5, 40, 300) > 0, geo


def _params():
    layers = (capi.EecDecoderLayerParams * 2)()
    for f, _ in capi.EecDecoderLayerParams._fields_:
        setattr(layers[0], f, 0x1000)
        setattr(layers[1], f, 0x1000)
    p = capi.EecDecoderParams(0x1000, 0x1000, layers, 2, 2000, 0x1000, 0x1000, 0x1000, 0x1000)
    return p, layers


def _err(lib):
    return lib.eec_decoder_step_last_error().decode()


def test_batch_begin_and_step_reject_bad_arguments_before_touching_the_device(lib):
    p, keep = _params()
    E, B, S_max, Tq = 2, 3, 10, 20
    geo = (64, 8, 128, 32)
    nbytes = lib.eec_decoder_batch_cache_bytes(*geo, 2, E, B, S_max, Tq)
    assert nbytes > 0
    ps = (C.POINTER(capi.EecDecoderParams) * E)(C.pointer(p), C.pointer(p))
    fake = C.c_void_p(0x10000)  # never dereferenced: every call below fails its checks first

    def begin(ps_=ps, taps=fake, cache=fake, size=nbytes, e=E, b=B):
        return lib.eec_decoder_batch_begin(ps_, e, b, *geo, taps, Tq, S_max, 3, cache, size, None)

    def step(ps_=ps, tok=fake, out=fake, cache=fake, size=nbytes, R=4, R_prev=4, s=1, e=E):
        return lib.eec_decoder_batch_step(ps_, e, B, *geo, 0, tok, None, R, R_prev, s, Tq, S_max, out, cache, size, None)

    assert begin(ps_=None) == 10001 and "null" in _err(lib)
    assert begin(taps=None) == 10001 and "null" in _err(lib)
    assert begin(cache=None) == 10001 and "null" in _err(lib)
    nullrow = (C.POINTER(capi.EecDecoderParams) * E)(C.pointer(p), C.POINTER(capi.EecDecoderParams)())
    assert begin(ps_=nullrow) == 10001 and "null" in _err(lib)
    assert begin(size=nbytes - 1) == 10003 and "cache too small" in _err(lib)
    assert begin(e=9) == 10001
    assert step(ps_=None) == 10001 and "null" in _err(lib)
    assert step(tok=None) == 10001 and "null" in _err(lib)
    assert step(out=None) == 10001 and "null" in _err(lib)
    assert step(cache=None) == 10001 and "null" in _err(lib)
    assert step(R=17) == 10001 and "16" in _err(lib)
    assert step(R=0) == 10001
    assert step(R_prev=17) == 10001 and "R_prev" in _err(lib)
    assert step(s=S_max) == 10001 and "S_max" in _err(lib)
    assert step(size=nbytes - 1) == 10003 and "cache too small" in _err(lib)
    # geometry outside the step decoder's: head dim 48
    bad = lib.eec_decoder_batch_step(ps, E, B, 384, 8, 128, 32, 0, fake, None, 4, 4, 1, Tq, S_max, fake, fake, nbytes, None)
    assert bad == 10002 and "geometry" in _err(lib)
