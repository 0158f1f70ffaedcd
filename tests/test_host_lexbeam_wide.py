"""CPU tests of the wide-beam lexicon CTC search (eec_ctc_lexbeam_wide_decode, csrc/ctc_lexbeam_wide.hip): the wide statement
(tests/lexbeam_wide_cases.py, candidate id (2 c + w) * 64 + i) against the four narrow statements at beams of 16 or less, the new
entry's argument errors and size arithmetic (all decided before any device work), and the conditions that keep the cases of
tests/test_gpu_lexbeam_wide.py from being vacuous, decided by the statement alone."""
import functools
import os

import numpy as np
import pytest

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_logadd_cases as A
import lexbeam_smear_cases as S
import lexbeam_wide_cases as W
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.build import LIB_PATH

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def identical(got, want):
    """Two batches of hypothesis lists: words, tokens, timesteps equal, scores equal as bit patterns."""
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), s
        for j, (x, y) in enumerate(zip(g, w)):
            assert x[:3] == y[:3], (s, j)
            assert np.float32(x[3]).view(np.int32) == np.float32(y[3]).view(np.int32), (s, j, x[3], y[3])


@functools.lru_cache(maxsize=None)
def lm_case():
    """The first 8 sequences of lexbeam_lm_cases.main_lm_case (order 3), 32 frames of each: (em, em_len, trie, words, model)."""
    em, em_len, spellings, words, lm = M.main_lm_case()
    return np.ascontiguousarray(em[:8, :32]), np.minimum(em_len[:8], 33), L.Trie(spellings, 256, 0, 126), words, lm


# ---------------------------------------------------------------------------------------------------------------------------
# the wide statement is the four narrow ones at beams of 16 or less
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [1, 10, 16])
def test_the_wide_statement_equals_lexbeam_cases(beam):
    """The model-free Viterbi statement on its own generators: the main case's first sequences with their ragged lengths, the wide
    lexicon, and tie emissions (equal scores in every frame: the id decides, and must decide alike)."""
    em, em_len, spellings, _ = L.main_case()
    ref = L.Trie(spellings, 256, 0, 126)
    for opts in (dict(), dict(beam_threshold=INF, word_score=1.5, sil_score=-0.5)):
        identical(W.decode_batch(em[:8, :40], ref, np.minimum(em_len[:8], 41), beam=beam, nbest=beam, **opts),
                  L.decode_batch(em[:8, :40], ref, np.minimum(em_len[:8], 41), beam=beam, nbest=beam, **opts))
    wide = L.wide_lexicon()
    ref = L.Trie(wide, 256, 0, 126)
    e = L.emissions(164, wide, 2, 12, 256, 0, 126)
    identical(W.decode_batch(e, ref, beam=beam, nbest=beam), L.decode_batch(e, ref, beam=beam, nbest=beam))
    ref = L.Trie(L.PREFIX_DOUBLED, 32)
    e = L.tie_emissions(7, L.PREFIX_DOUBLED, 12, 16, 32)
    identical(W.decode_batch(e, ref, beam=beam, nbest=beam, beam_threshold=INF), L.decode_batch(e, ref, beam=beam, nbest=beam, beam_threshold=INF))


@pytest.mark.parametrize("beam", [1, 10, 16])
def test_the_wide_statement_equals_lexbeam_lm_cases_and_lexbeam_smear_cases(beam):
    em, em_len, ref, words, lm = lm_case()
    for lm_weight in (0.0, 3.23):
        kw = dict(beam=beam, nbest=beam, lm=lm, lm_weight=lm_weight, lm_words=words)
        identical(W.decode_batch(em, ref, em_len, **kw), M.decode_batch(em, ref, em_len, **kw))
        smax = S.smear(ref, lm, words)
        identical(W.decode_batch(em, ref, em_len, smax=smax, **kw), S.decode_batch(em, ref, em_len, smax=smax, **kw))


@pytest.mark.parametrize("beam", [1, 10, 16])
def test_the_wide_statement_equals_lexbeam_logadd_cases(beam):
    em, em_len, ref, words, lm = lm_case()
    smax = S.smear(ref, lm, words)
    for kw in (dict(), dict(lm=lm, lm_weight=3.23, lm_words=words), dict(lm=lm, lm_weight=3.23, lm_words=words, smax=smax)):
        identical(W.decode_batch(em, ref, em_len, beam=beam, nbest=beam, log_add=True, **kw),
                  A.decode_batch(em, ref, em_len, beam=beam, nbest=beam, log_add=True, **kw))
    ref = L.Trie(L.PREFIX_DOUBLED, 32)
    e = L.tie_emissions(7, L.PREFIX_DOUBLED, 12, 16, 32)
    identical(W.decode_batch(e, ref, beam=beam, nbest=beam, beam_threshold=INF, log_add=True),
              A.decode_batch(e, ref, beam=beam, nbest=beam, beam_threshold=INF, log_add=True))


# ---------------------------------------------------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------------------------------------------------
def test_wide_argument_errors_come_before_any_device_use(lib):
    """Plausible but unusable addresses: every refusal is decided on the arguments alone, nothing is dereferenced.  The codes are the
    narrow entries' (tests/test_host_lexbeam.py), with the beam range 1..64."""
    fake = 0x10000
    dec, size = lib.eec_ctc_lexbeam_wide_decode, lib.eec_ctc_lexbeam_wide_workspace_bytes
    need = size(3, 7, 40)

    def call(logp=fake, n=3, T=7, V=40, em_len=None, trie=fake, blank=0, sil=-1, beam=40, nbest=2, thr=50.0, max_words=7, words=fake, wc=fake,
             tok=fake, tc=fake, ts=None, sc=fake, nh=fake, ws=fake, ws_bytes=need, lm=None, lm_weight=0.0, smear=None, log_add=0):
        return dec(logp, n, T, V, em_len, trie, blank, sil, beam, nbest, 0.0, 0.0, thr, max_words, words, wc, tok, tc, ts, sc, nh, ws, ws_bytes, None,
                   lm, lm_weight, smear, log_add)
    for name in ("logp", "trie", "words", "wc", "tok", "tc", "sc", "nh", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    assert b"null" in lib.eec_last_error()
    assert call(n=-1) == BAD_ARG and call(T=0) == BAD_ARG and call(max_words=0) == BAD_ARG
    assert call(blank=-1) == BAD_ARG and call(blank=40) == BAD_ARG and call(sil=40) == BAD_ARG and call(sil=-2) == BAD_ARG
    assert call(blank=5, sil=5) == BAD_ARG
    assert call(trie=fake + 4) == BAD_ARG and call(ws=fake + 4) == BAD_ARG
    assert call(lm=fake + 4) == BAD_ARG and call(lm=fake, smear=fake + 4) == BAD_ARG
    assert call(V=257) == UNSUPPORTED and call(V=1) == UNSUPPORTED
    assert call(beam=0) == UNSUPPORTED and call(beam=65) == UNSUPPORTED and call(beam=-3) == UNSUPPORTED
    assert b"64" in lib.eec_last_error()
    assert call(nbest=0) == UNSUPPORTED and call(nbest=41) == UNSUPPORTED and call(beam=17, nbest=18) == UNSUPPORTED
    assert call(beam=64, nbest=64) == WORKSPACE  # the boundary values pass the range check and reach the size check
    assert call(beam=64, nbest=64, log_add=1) == WORKSPACE
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(smear=fake) == BAD_ARG and b"smear without lm" in lib.eec_last_error()
    assert call(smear=fake, log_add=1) == BAD_ARG
    assert call(lm=fake, lm_weight=float("nan")) == BAD_ARG and call(lm=fake, lm_weight=INF) == BAD_ARG
    assert call(lm=None, lm_weight=float("nan"), ws_bytes=need - 1) == WORKSPACE  # without a model lm_weight is ignored
    assert call(n=0, logp=None, trie=None, words=None, wc=None, tok=None, tc=None, sc=None, nh=None, ws=None, ws_bytes=0) == 0  # nothing to do
    assert call(n=0, beam=65) == UNSUPPORTED  # the ranges are checked first, as in the narrow entries


def test_wide_workspace_is_the_stated_formula_and_monotonic(lib):
    ws = lib.eec_ctc_lexbeam_wide_workspace_bytes
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, 0) == 0 and ws(-1, 5, 5) == 0
    for n, T, beam in ((1, 1, 1), (3, 7, 17), (70, 16, 64), (384, 256, 64), (384, 256, 50)):
        assert ws(n, T, beam) == n * T * beam * 8  # the back-pointers, 8 bytes per (frame, rank); no other global scratch
    for k in range(3):
        grow = []
        for v in (1, 2, 7, 16, 17, 40, 64):
            a = [3, 5, 4]
            a[k] = v
            grow.append(ws(*a))
        assert grow == sorted(grow) and len(set(grow)) == len(grow) and grow[0] > 0, k
    assert ws(384, 256, 16) == lib.eec_ctc_lexbeam_workspace_bytes(384, 256, 16)


def test_the_python_entry_refuses_a_narrow_call_with_a_wide_beam():
    import torch
    from early_exit_transformer_amd.lexicon import TokenTrie
    from early_exit_transformer_amd.model import ctc_lexicon_decode
    trie = TokenTrie.from_spellings(L.ONE_WORD, 40)
    with pytest.raises(ValueError, match="wide=False"):
        ctc_lexicon_decode(torch.zeros(1, 3, 40), trie, beam_size=17, wide=False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc_lexicon_decode(torch.zeros(1, 3, 40), trie, beam_size=17)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU cases are not vacuous
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,T,beam,nbest,opts", W.WIDE_CASES, ids=[f"{c[0]}-n{c[1]}-T{c[2]}-b{c[3]}-k{c[4]}" for c in W.WIDE_CASES])
def test_the_wide_gpu_cases_hold_more_than_16_hypotheses(name, n, T, beam, nbest, opts):
    """In every case with a beam over 16 the beam holds more than 16 hypotheses after at least half of the frames the batch decodes
    (all sequences' frames counted together; ragged batches hold sequences of 1 or 2 frames, which cannot).  The `one` lexicon is
    there for the opposite reason -- a beam far larger than the candidates -- and must stay at or below 16.  The merge groups stay
    within the bound derived for the kernel's comment (4), and the 12 928-candidate frame is where the issue says it is."""
    spellings, V, sil, _ = W.lexicon(name)
    em, em_len = W.wide_case_inputs(name, n, T)
    stats = []
    W.decode_batch(em, L.Trie(spellings, V, 0, sil), em_len, stats=stats, beam=beam, nbest=nbest, **opts)
    assert max(st.get("max_group", 0) for st in stats) <= 4
    if name == "one":
        assert W.wide_share(stats) == 0.0
    else:
        assert W.wide_share(stats) >= 0.5, W.wide_share(stats)
    if (name, T) == ("wide", 12):
        assert max(st["max_alive"] for st in stats) == 12928  # far above the kernel's list of 1024: every overflow path
    if (name, T) == ("fixture+sil", 48):
        assert 1024 < max(st["max_alive"] for st in stats) < 2048 and min(st["max_alive"] for st in stats) >= 1


@pytest.mark.parametrize("beam", W.TIE_BEAMS)
@pytest.mark.parametrize("name,n,T", W.TIE_CASES)
def test_the_tie_cases_have_ties_that_only_a_wide_id_decides(name, n, T, beam):
    """tie_emissions at the sizes the GPU test uses, the uniform block at the length tie_emissions gives it (T' // 4 frames): ties
    decided by the id between candidates of which at least one has a rank of 16 or more occur at both beams."""
    spellings, V, sil, _ = W.lexicon(name)
    stats = []
    W.decode_batch(W.tie_case_inputs(name, n, T), L.Trie(spellings, V, 0, sil), stats=stats, beam=beam, nbest=beam, beam_threshold=INF)
    assert sum(st.get("wide_ties", 0) for st in stats) >= 1
    assert W.wide_share(stats) >= 0.5
