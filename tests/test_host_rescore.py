"""CPU tests of two-pass decoding's host side: the new entries are exported and reject bad arguments, with the stated codes,
before touching a device; the workspace arithmetic of eec_decoder_score; the fp64 mix and pick of tests/rescore_cases.py; and the
condition the N-best GPU test puts on its own inputs, under the oracle alone."""
import ctypes as C
import os

import pytest

import rescore_cases as X
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference, RescoredList
from early_exit_transformer_amd.build import LIB_PATH
from oracle.ctc_beam_ref import ctc_prefix_beam_search

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def test_the_new_entries_are_exported(lib):
    for name in ("eec_ctc_beam_decode_nbest", "eec_decoder_score_workspace_bytes", "eec_decoder_score", "eec_hypothesis_score"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.eec_abi_version() == 16


def test_nbest_entry_rejects_bad_arguments_before_any_launch(lib):
    buf = (C.c_int32 * 4096)()
    p = C.addressof(buf)

    def call(logp=p, em_len=None, n_seq=1, Tq=4, V=8, blank=0, beam=8, nbest=4, ws=p, tokens=p, counts=p, scores=p, n_hyp=p):
        return lib.eec_ctc_beam_decode_nbest(logp, em_len, n_seq, Tq, V, blank, beam, 0.95, 0, nbest, ws, tokens, counts, scores, n_hyp, None)
    for null in ("logp", "ws", "tokens", "counts", "scores", "n_hyp"):
        assert call(**{null: None}) == BAD_ARG and b"null" in lib.eec_last_error(), null
    assert call(n_seq=0) == BAD_ARG and call(Tq=0) == BAD_ARG
    assert call(V=257) == UNSUPPORTED and call(V=0) == UNSUPPORTED
    assert call(beam=17) == UNSUPPORTED and call(beam=0) == UNSUPPORTED
    assert call(blank=8) == UNSUPPORTED and call(blank=-1) == UNSUPPORTED
    assert call(nbest=0) == BAD_ARG and b"nbest" in lib.eec_last_error()
    assert call(nbest=9) == BAD_ARG and b"nbest" in lib.eec_last_error()  # above the beam


def _params(max_len=2000, n_layers=2):
    layers = (capi.EecDecoderLayerParams * n_layers)()
    ps = capi.EecDecoderParams()
    ps.layers, ps.n_layers, ps.max_len = layers, n_layers, max_len
    return ps, layers


def test_decoder_score_rejects_bad_arguments_before_any_launch(lib):
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 255) // 256 * 256
    ps, _keep = _params()
    need = lib.eec_decoder_score_workspace_bytes(256, 8, 512, 256, 2, 4, 9, 17)

    def call(params=ps, D=256, H=8, F=512, V=256, pad=126, sos=1, eos=2, tok=p, ln=p, enc=p, n=2, R=4, L=9, Tq=17, passes=3, out=p, ws=p,
             nbytes=need):
        return lib.eec_decoder_score(C.byref(params) if params is not None else None, D, H, F, V, pad, sos, eos, tok, ln, enc, n, R, L, Tq, passes,
                                     out, ws, nbytes, None)
    assert call(params=None) == BAD_ARG and b"null" in lib.eec_decoder_last_error()
    for null in ("tok", "ln", "enc", "out", "ws"):
        assert call(**{null: None}) == BAD_ARG and b"null" in lib.eec_last_error(), null
    empty = capi.EecDecoderParams()  # no layer array
    assert call(params=empty) == BAD_ARG
    # the geometry limits of eec_decoder_forward
    for bad in (dict(D=0), dict(D=1028, H=4), dict(H=0), dict(H=7), dict(V=0), dict(V=1025), dict(F=0), dict(R=0), dict(Tq=0), dict(n=-1),
                dict(L=-1), dict(passes=2)):
        assert call(**bad) == BAD_ARG, bad
    short, _k = _params(max_len=9)
    assert call(params=short) == BAD_ARG and b"geometry" in lib.eec_last_error()  # S = L + 1 = 10 > max_len
    for bad in (dict(sos=-1), dict(sos=256), dict(eos=-1), dict(eos=256), dict(pad=-1), dict(pad=256)):
        assert call(**bad) == BAD_ARG and b"[0, vocab)" in lib.eec_last_error(), bad
    assert call(n=20000) == BAD_ARG  # more batches than one call's grid takes
    assert call(nbytes=need - 1) == WORKSPACE and b"small" in lib.eec_last_error()
    assert call(ws=p + 4) == WORKSPACE and b"aligned" in lib.eec_last_error()
    # n = 0: a successful no-op, whatever the buffers
    assert call(n=0, tok=None, ln=None, enc=None, out=None, ws=None, nbytes=0) == 0


def test_hypothesis_score_rejects_bad_arguments_before_any_launch(lib):
    buf = (C.c_char * 1024)()
    p = (C.addressof(buf) + 255) // 256 * 256

    def call(logits=p, tok=p, ln=p, n=3, L=4, V=32, eos=1, out=p):
        return lib.eec_hypothesis_score(logits, tok, ln, n, L, V, eos, out, None)
    for null in ("logits", "tok", "ln", "out"):
        assert call(**{null: None}) == BAD_ARG and b"null" in lib.eec_last_error(), null
    for bad in (dict(n=-1), dict(L=-1), dict(V=0), dict(V=1025), dict(eos=-1), dict(eos=32), dict(logits=p + 4)):
        assert call(**bad) == BAD_ARG, bad
    assert call(n=0, logits=None, tok=None, ln=None, out=None) == 0


def test_decoder_score_workspace_arithmetic(lib):
    """The workspace holds the row buffers of M = n * R * S rows (x, ln, q, ctx: D each; qkv: 3D; h: F; logits: V), the memory's
    keys | values (n * T' * 2D), the attention probabilities n * R * H * S * max(S, T') and the rows' tokens and pad flags."""
    D, H, F, V, n, R, L, Tq = 256, 8, 2048, 256, 6, 10, 24, 256
    S = L + 1
    M = n * R * S
    floats = M * (4 * D + 3 * D + F + V) + n * Tq * 2 * D + n * R * H * S * max(S, Tq)
    got = lib.eec_decoder_score_workspace_bytes(D, H, F, V, n, R, L, Tq)
    assert 4 * floats + 9 * M <= got <= 4 * floats + 9 * M + 16 * 256
    # linear in the memories, and the cross-attention probabilities dominate the growth with T'
    one = lib.eec_decoder_score_workspace_bytes(D, H, F, V, 1, R, L, Tq)
    assert abs(got - n * one) <= n * 16 * 256
    longer = lib.eec_decoder_score_workspace_bytes(D, H, F, V, n, R, L, 2 * Tq)
    assert longer - got >= 4 * (n * R * H * S * Tq + n * Tq * 2 * D) - 16 * 256
    # short memories: the self-attention's S x S probabilities set the size
    assert lib.eec_decoder_score_workspace_bytes(D, H, F, V, n, R, L, 3) == lib.eec_decoder_score_workspace_bytes(D, H, F, V, n, R, L, S) - 4 * n * (S - 3) * 2 * D
    # geometries the entry rejects size to 0, and so does n = 0
    for bad in ((D, 7, F, V, n, R, L, Tq), (D, H, F, 1025, n, R, L, Tq), (D, H, F, V, 0, R, L, Tq), (D, H, F, V, n, 0, L, Tq),
                (D, H, F, V, n, R, -1, Tq), (D, H, F, V, 1000, R, L, Tq)):
        assert lib.eec_decoder_score_workspace_bytes(*bad) == 0, bad


def test_the_mix_and_the_pick():
    for ctc, att, w, joint, best in X.mix_examples():
        got = X.mix(ctc, att, w)
        assert got == joint and X.pick(got) == best, (ctc, att, w)
    assert RescoredList._fields == ("tokens", "ctc", "att", "joint")


def test_rescore_batch_rejects_a_weight_outside_the_unit_interval():
    for w in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="rescoring_ctc_weight"):
            BeamInference().rescore_batch(None, None, [1], None, None, 4, w)


def test_the_nbest_inputs_allow_enough_comparisons_under_the_oracle():
    """At least 3/4 of the (sequence, rank < 4) pairs of every oracle variant have all the oracle's gaps up to the next rank above
    BEAM_MARGIN, so the GPU test compares their token sequences.  Measured: 164 of 180 and 134 of 141."""
    for variant in X.ORACLE_VARIANTS:
        compared, present = X.rank_census(*variant)
        print(f"\n[nbest inputs {variant}] {compared} of {present} pairs comparable")
        assert present >= 100 and compared >= X.MIN_COMPARED * present, (variant, compared, present)
    # the lengths hold an empty and a full sequence, and the oracle of an empty one is the empty prefix alone
    for (T, V, scale, logp, lens), rows in zip(X.nbest_blocks(), X.oracle_beams(True, True)):
        assert int(lens.min()) == 0 and int(lens.max()) == T
        assert rows[0] == [([], 0.0)]


def test_the_unpruned_case_fits_the_beam():
    logp, total = X.unpruned_case()
    assert 1 < len(total) <= 16 and () in total
    final = ctc_prefix_beam_search(logp[0].double().numpy(), beam=16, blank=0, blank_skip_threshold=1.0, return_beams=True)[2]
    assert {tuple(p) for p, _ in final} == set(total)  # the oracle prunes nothing either, and agrees with the enumeration
    for p, s in final:
        assert abs(s - total[tuple(p)]) < 1e-9
