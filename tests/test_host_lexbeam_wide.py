"""CPU tests of the wide-beam lexicon CTC search (eec_ctc_lexbeam_wide_decode, csrc/ctc_lexbeam_wide.hip): the statement
(tests/lexbeam_statement.py, candidate id (2 c + w) * 64 + i) against what the four narrow statements it replaced returned at beams of
16 or less (tests/golden/lexbeam_statement_pins.json), the entry's argument errors and size arithmetic (all decided before any
device work), and the conditions that keep the cases of tests/test_gpu_lexbeam_wide.py from being vacuous, decided by the statement
alone."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_smear_cases as S
import lexbeam_statement as D
import lexbeam_wide_cases as W
from lexbeam_helpers import library

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    return library()


# ---------------------------------------------------------------------------------------------------------------------------
# at beams of 16 or less the statement returns what the four narrow statements (candidate id (2 c + w) * 16 + i) returned
# ---------------------------------------------------------------------------------------------------------------------------
with open(os.path.join(L.GOLDEN, "lexbeam_statement_pins.json"), encoding="utf-8") as _f:
    PINS = json.load(_f)


@functools.lru_cache(maxsize=None)
def pin_inputs(generator):
    """(emission, em_len or None, trie, words or None, model or None), as the record's ``generators`` describe them"""
    if generator == "main":  # the main case's first sequences with their ragged lengths
        em, em_len, spellings, _ = L.main_case()
        return em[:8, :40], np.minimum(em_len[:8], 41), L.Trie(spellings, 256, 0, 126), None, None
    if generator == "wide":
        wide = L.wide_lexicon()
        return L.emissions(164, wide, 2, 12, 256, 0, 126), None, L.Trie(wide, 256, 0, 126), None, None
    if generator == "ties":  # equal scores in every frame: the id decides, and must decide alike
        return L.tie_emissions(7, L.PREFIX_DOUBLED, 12, 16, 32), None, L.Trie(L.PREFIX_DOUBLED, 32), None, None
    assert generator == "lm"  # the first 8 sequences of lexbeam_lm_cases.main_lm_case (order 3), 32 frames of each
    em, em_len, spellings, words, lm = M.main_lm_case()
    return np.ascontiguousarray(em[:8, :32]), np.minimum(em_len[:8], 33), L.Trie(spellings, 256, 0, 126), words, lm


def digest(hyps):
    """The record's ``serialisation`` of a batch of hypothesis lists."""
    canon = [[[list(map(int, w)), list(map(int, tk)), list(map(int, st)), int(M.bits(sc))] for w, tk, st, sc in seq] for seq in hyps]
    return hashlib.sha256(json.dumps(canon, separators=(",", ":")).encode()).hexdigest()


def returns_the_pinned(narrow, beam, n_calls):
    """Every recorded call of the narrow statements ``narrow`` at ``beam``, made again with the one statement."""
    calls = [c for c in PINS["calls"] if c["narrow"] in narrow and c["beam"] == beam]
    assert len(calls) == n_calls
    for c in calls:
        em, em_len, ref, words, lm = pin_inputs(c["generator"])
        kw = {k: float(v) for k, v in c["options"].items()}
        if c["model"]:
            kw.update(lm=lm, lm_weight=c["lm_weight"], lm_words=words)
        if c["smear"]:
            kw.update(smax=S.smear(ref, lm, words))
        got = D.decode_batch(em, ref, em_len, beam=beam, nbest=beam, log_add=c["log_add"], **kw)
        assert [len(h) for h in got] == c["n_hyp"], c
        assert digest(got) == c["sha256"], c


@pytest.mark.parametrize("beam", [1, 10, 16])
def test_the_statement_returns_what_lexbeam_cases_returned(beam):
    """The model-free Viterbi statement on its own generators: the main case with and without options, the wide lexicon, ties."""
    returns_the_pinned(("lexbeam_cases",), beam, 4)


@pytest.mark.parametrize("beam", [1, 10, 16])
def test_the_statement_returns_what_lexbeam_lm_cases_and_lexbeam_smear_cases_returned(beam):
    """With the model at lm_weight 0 and 3.23, unsmeared (lexbeam_lm_cases) and smeared (lexbeam_smear_cases)."""
    returns_the_pinned(("lexbeam_lm_cases", "lexbeam_smear_cases"), beam, 4)


@pytest.mark.parametrize("beam", [1, 10, 16])
def test_the_statement_returns_what_lexbeam_logadd_cases_returned(beam):
    """Log-add merging without a model, with it, with it and smearing, and on ties."""
    returns_the_pinned(("lexbeam_logadd_cases",), beam, 4)


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
    spellings, V, sil, _ = L.lexicon(name)
    em, em_len = W.wide_case_inputs(name, n, T)
    stats = []
    D.decode_batch(em, L.Trie(spellings, V, 0, sil), em_len, stats=stats, beam=beam, nbest=nbest, **opts)
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
    spellings, V, sil, _ = L.lexicon(name)
    stats = []
    D.decode_batch(W.tie_case_inputs(name, n, T), L.Trie(spellings, V, 0, sil), stats=stats, beam=beam, nbest=beam, beam_threshold=INF)
    assert sum(st.get("wide_ties", 0) for st in stats) >= 1
    assert W.wide_share(stats) >= 0.5
