"""GPU tests of the wide-beam lexicon CTC search (csrc/ctc_lexbeam_wide.hip, eec_ctc_lexbeam_wide_decode, ``ctc_lexicon_decode`` with
``beam_size`` 17..64 or ``wide=True``, ``BeamInference`` at beam 64) against the narrow entries at beams of 16 or less and against the
plain-Python statement of tests/lexbeam_statement.py above that.  As in tests/test_gpu_lexbeam.py there is nothing to tolerate:
n_hyp, words, tokens, timesteps and counts are compared as integers and scores as bit patterns.  tests/test_host_lexbeam_wide.py
shows with the statement alone that these cases fill the beam past 16, overflow the kernel's candidate list and hold ties that only
the wide id decides."""
import functools

import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_smear_cases as S
import lexbeam_statement as D
import lexbeam_wide_cases as W
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.lexicon import TokenTrie
from early_exit_transformer_amd.model import ctc_lexicon_decode
from lexbeam_helpers import identical, lexicon, models, run, same, tries

pytestmark = pytest.mark.gpu
INF = float("inf")


# ----------------------------------------------------------------------------------------------------------------------------
# 1. at beams of 16 or less the wide kernel returns what the narrow entries return
# ----------------------------------------------------------------------------------------------------------------------------
MODES = {
    "viterbi": dict(),
    "model": dict(lm=True),
    "model+smear": dict(lm=True, smearing="max"),
    "logadd": dict(log_add=True),
    "logadd+model+smear": dict(lm=True, smearing="max", log_add=True),
}


@functools.lru_cache(maxsize=None)
def model_case(order=3, **variant):
    """(emission [4, 32, 256], model dict, packed model) over fixture+sil, emissions in the style of lexbeam_lm_cases.main_lm_case"""
    spellings, V, sil, words = lexicon("fixture+sil")
    lm, packed, favoured, disfavoured = models("fixture+sil", order, **variant)
    em = M.lm_emissions(300 + order, favoured, disfavoured, words, spellings, 4, 32, V, 0, sil, peaks=M.MAIN_PEAKS)
    return em, lm, packed


def mode_kwargs(mode, packed, lm_weight=3.23):
    kw = dict(MODES[mode])
    if kw.pop("lm", False):
        kw.update(lm=packed, lm_weight=lm_weight)
    return kw


@pytest.mark.parametrize("beam", [1, 10, 16])
@pytest.mark.parametrize("mode", list(MODES))
def test_wide_at_narrow_beams_equals_the_narrow_entry(mode, beam):
    packed_trie = tries("fixture+sil")[1]
    if "model" in mode:
        em, _, packed = model_case()
        settings = [mode_kwargs(mode, packed)]
    else:
        spellings, V, sil, _ = lexicon("fixture+sil")
        em = L.emissions(154, spellings, 6, 48, V, 0, sil)
        settings = [dict(MODES[mode], beam_threshold=50.0), dict(MODES[mode], beam_threshold=INF)]
    for kw in settings:
        narrow = run(em, packed_trie, beam_size=beam, nbest=beam, wide=False, **kw)
        wide = run(em, packed_trie, beam_size=beam, nbest=beam, wide=True, **kw)
        identical(wide, narrow)
        identical(narrow, run(em, packed_trie, beam_size=beam, nbest=beam, **kw))  # the default routing is the narrow entry
        assert (narrow[6] > 0).any() or beam == 1, "the case decodes something"


# ----------------------------------------------------------------------------------------------------------------------------
# 2. beams over 16 against the statement
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_reference(k):
    name, n, T, beam, nbest, opts = W.WIDE_CASES[k]
    em, em_len = W.wide_case_inputs(name, n, T)
    return em, em_len, D.decode_batch(em, tries(name)[0], em_len, beam=beam, nbest=nbest, **opts)


@pytest.mark.parametrize("k", range(len(W.WIDE_CASES)), ids=[f"{c[0]}-n{c[1]}-T{c[2]}-b{c[3]}-k{c[4]}" for c in W.WIDE_CASES])
def test_wide_beams_equal_the_statement(k):
    """A full beam of 64 with every hypothesis returned; an odd T' of 257 at word_score -4; 70 ragged sequences (0, 1, T', T' + 1) under
    a threshold of 2 at beam 17; the 12 928-candidate frames of the wide lexicon (the candidate list overflows many times over);
    child ranges over 64 at beam 33; nbest below the beam; a beam far larger than the candidates (`one`)."""
    name, n, T, beam, nbest, opts = W.WIDE_CASES[k]
    em, em_len, want = wide_reference(k)
    nh = same(run(em, tries(name)[1], em_len, beam_size=beam, nbest=nbest, **opts), want, nbest)
    assert T < 7 or (nh > 0).any(), "the case decodes something"


# ----------------------------------------------------------------------------------------------------------------------------
# 3. ties
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", W.TIE_BEAMS)
@pytest.mark.parametrize("name,n,T", W.TIE_CASES)
def test_wide_ties_are_decided_by_the_candidate_id(name, n, T, beam):
    ref, packed = tries(name)
    em = W.tie_case_inputs(name, n, T)
    want = D.decode_batch(em, ref, beam=beam, nbest=beam, beam_threshold=INF)
    same(run(em, packed, beam_size=beam, nbest=beam, beam_threshold=INF), want, beam)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. the drop rule
# ----------------------------------------------------------------------------------------------------------------------------
def test_minus_infinity_and_nan_follow_the_drop_rule_at_beam_64():
    """The case of tests/test_gpu_lexbeam.py at beam 64: a fifth of the entries -inf in every sequence; NaN entries in sequence 1
    and a whole NaN frame in sequence 2 (it ends without a hypothesis); the neighbours are what they are without them."""
    spellings, V, sil, _ = lexicon("prefix")
    ref, packed = tries("prefix")
    em = L.emissions(21, spellings, 6, 16, V, peaks=(4.0, 8.0))
    rng = np.random.default_rng(22)
    em[rng.random(em.shape) < 0.2] = -np.inf
    clean = em.copy()
    em[1][rng.random(em[1].shape) < 0.1] = np.nan
    em[2, 5, :] = np.nan
    want = D.decode_batch(em, ref, beam=64, nbest=64)
    assert want[2] == [] and any(want[s] for s in (0, 3, 4, 5))
    got = run(em, packed, beam_size=64, nbest=64)
    same(got, want, 64)
    untouched = run(clean, packed, beam_size=64, nbest=64)
    for a, b in zip(got, untouched):
        assert np.array_equal(a[[0, 3, 4, 5]], b[[0, 3, 4, 5]], equal_nan=True)


# ----------------------------------------------------------------------------------------------------------------------------
# 5. with a model
# ----------------------------------------------------------------------------------------------------------------------------
LM_MODES = ["model", "model+smear", "logadd", "logadd+model+smear"]
LM_CASES = ([(beam, mode, 3, 3.23, ()) for beam in (40, 64) for mode in LM_MODES] +
            [(beam, mode, 2, 1.0, ()) for beam in (40, 64) for mode in LM_MODES] +
            [(64, "model", 3, 0.0, ()), (64, "logadd+model+smear", 2, 0.0, ()), (40, "model+smear", 2, 0.0, ()),
             (64, "model", 3, 3.23, (("eos", False),)), (40, "logadd+model+smear", 2, 1.0, (("eos", False),))])


@pytest.mark.parametrize("beam,mode,order,lm_weight,variant", LM_CASES,
                         ids=[f"b{c[0]}-{c[1]}-o{c[2]}-w{c[3]}{'-noeos' if c[4] else ''}" for c in LM_CASES])
def test_wide_beams_with_a_model_equal_the_statement(beam, mode, order, lm_weight, variant):
    """4 sequences x 32 frames over fixture+sil, every hypothesis returned.  `logadd` runs without the model (the mode the other
    three do not cover at these beams); the others under a model of order 2 or 3, with and without </s>, at lm_weight 0 and not 0."""
    spellings, V, sil, words = lexicon("fixture+sil")
    ref, packed_trie = tries("fixture+sil")
    em, lm, packed = model_case(order, **dict(variant))
    kw = mode_kwargs(mode, packed, lm_weight)
    st = dict(log_add=kw.get("log_add", False))
    if "lm" in kw:
        st.update(lm=lm, lm_weight=lm_weight, lm_words=words, smax=S.smear(ref, lm, words) if kw.get("smearing") else None)
    stats = []
    want = D.decode_batch(em, ref, beam=beam, nbest=beam, stats=stats, **st)
    assert W.wide_share(stats) >= 0.5
    nh = same(run(em, packed_trie, beam_size=beam, nbest=beam, **kw), want, beam)
    assert (nh > 0).any(), "the case decodes something"


# ----------------------------------------------------------------------------------------------------------------------------
# 6. the launch
# ----------------------------------------------------------------------------------------------------------------------------
BATCH = next(k for k, c in enumerate(W.WIDE_CASES) if c[:3] == ("prefix", 70, 16))


def test_a_sequence_alone_equals_itself_in_the_batch_and_runs_repeat():
    em, em_len, want = wide_reference(BATCH)
    packed = tries("prefix")[1]
    first = run(em, packed, em_len, beam_size=64, nbest=10)
    identical(first, run(em, packed, em_len, beam_size=64, nbest=10))
    for s in (2, 7, 41, 69):
        alone = run(em[s:s + 1], packed, em_len[s:s + 1], beam_size=64, nbest=10)
        for a, b in zip(alone, first):
            assert a[0].tobytes() == b[s].tobytes(), s
        same(alone, want[s:s + 1], 10)


def test_the_wide_launch_replays_from_a_graph():
    """Captured with torch.cuda.graph, replayed twice over wiped outputs: identical outputs, the statement's."""
    em_host, em_len, want = wide_reference(BATCH)
    packed = tries("prefix")[1]
    em = torch.from_numpy(em_host).cuda()
    lens = torch.from_numpy(em_len).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the image is uploaded and the allocator is warm before the capture
        ctc_lexicon_decode(em, packed, beam_size=64, nbest=10, em_len=lens)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ctc_lexicon_decode(em, packed, beam_size=64, nbest=10, em_len=lens)
    runs = []
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        runs.append([o.cpu().numpy().copy() for o in out])
    identical(*runs)
    same(runs[1], want, 10)


def test_max_words_truncates_and_word_count_stays_true():
    em, em_len, want = wide_reference(BATCH)
    assert max(len(h[0]) for hyps in want for h in hyps) > 2
    got = run(em, tries("prefix")[1], em_len, beam_size=64, nbest=10, max_words=2)
    assert got[0].shape == (70, 10, 2)
    same(got, want, 10, max_words=2)


def test_a_trie_packed_for_other_labels_gives_no_hypothesis():
    spellings, V, sil, _ = lexicon("prefix")
    other = TokenTrie.from_spellings(spellings, V, blank=0, sil=None)
    other.sil = 20  # the call now states a sil token the image was not packed with
    em = L.emissions(5, spellings, 3, 7, V, peaks=(8.0,))
    got = run(em, other, beam_size=64, nbest=2)
    assert (got[6] == 0).all() and (got[5] == -np.inf).all() and (got[1] == 0).all() and (got[3] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------------
# 7. the Python layer
# ----------------------------------------------------------------------------------------------------------------------------
def test_beam_inference_at_beam_64():
    """The transcripts are the statement's at beam 64; pprob is the softmax over up to 64 of its scores (a float64 softmax of
    identical fp32 inputs: 1e-6 covers its rounding).  The small lexicon ends more than 16 complete hypotheses per utterance."""
    spellings, V, sil, words = lexicon("prefix")
    ref, packed = tries("prefix")
    em = L.emissions(31, spellings, 6, 16, V)
    want = D.decode_batch(em, ref, beam=64, nbest=64)
    assert any(len(h) > 16 for h in want), "more hypotheses than a narrow beam could return"

    class Args:
        beam_size = 64
    infer = BeamInference(Args(), trie=packed)
    dev = torch.from_numpy(em).cuda()
    texts = [" ".join(words[w] for w in hyps[0][0]).strip() if hyps else "" for hyps in want]
    assert infer.ctc_predict_(dev) == texts
    assert BeamInference(None, trie=packed).ctc_predict_(dev, beam_size=64, nbest=64) == texts
    for b, hyps in enumerate(want):
        text, pprob = infer.ctc_predict(dev[b:b + 1], beam_size=64, nbest=64)
        assert text == [texts[b]]
        if hyps:
            sc = np.array([h[3] for h in hyps], dtype=np.float64)
            p = np.exp(sc - sc.max())
            assert abs(float(pprob) - p[0] / p.sum()) <= 1e-6
        else:
            assert float(pprob) == 0.0


def test_beams_over_64_and_narrow_calls_with_wide_beams_are_refused():
    packed = tries("prefix")[1]
    em = torch.zeros(1, 3, 32, device="cuda")
    with pytest.raises(RuntimeError, match="eec_ctc_lexbeam_wide_decode"):
        ctc_lexicon_decode(em, packed, beam_size=65)
    with pytest.raises(ValueError, match="wide=False"):
        ctc_lexicon_decode(em, packed, beam_size=17, wide=False)
    with pytest.raises(RuntimeError, match="eec_ctc_lexbeam_wide_decode"):
        ctc_lexicon_decode(em, packed, beam_size=40, nbest=41)
