"""GPU tests of the lexicon-constrained CTC beam search (csrc/ctc_lexbeam.hip, ``ctc_lexicon_decode``, ``BeamInference.ctc_predict``)
against the plain-Python statement of tests/lexbeam_statement.py.  There is nothing to tolerate: the arithmetic is fp32 additions in
a stated order, so n_hyp, words, tokens, timesteps and counts are compared as integers and scores as bit patterns.  Lexica come from
the fixture tests/golden/bpe256_lexicon_slice.json and from the small hand-made ones of tests/lexbeam_cases.py."""
import functools

import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_statement as D
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.lexicon import TokenTrie
from early_exit_transformer_amd.model import ctc_lexicon_decode
from lexbeam_helpers import captured_nodes, lexicon, raw_buffers, raw_call, run, same, tries

pytestmark = pytest.mark.gpu
INF = float("inf")


@functools.lru_cache(maxsize=None)
def main_reference():
    em, em_len, spellings, _ = L.main_case()
    return em, em_len, D.decode_batch(em, tries("fixture+sil")[0], em_len, beam=10, nbest=10)


def test_the_main_case_has_both_outcomes_and_equals_the_statement():
    """70 sequences x 64 frames over the fixture lexicon, beam 10, all 10 hypotheses, sil on, ragged lengths with 1, T' and values
    outside [1, T'] (those give n_hyp = 0).  At least a quarter of the sequences end with a hypothesis and a tenth without."""
    em, em_len, want = main_reference()
    nh = same(run(em, tries("fixture+sil")[1], em_len, beam_size=10, nbest=10), want, 10)
    inside = (em_len >= 1) & (em_len <= 64)
    assert (nh[inside] > 0).sum() >= 0.25 * 70 and (nh[inside] == 0).sum() >= 0.10 * 70
    assert (nh[~inside] == 0).all() and (~inside).sum() == 3


CASES = [
    # lexicon, n_seq, T', beam, nbest, options
    ("fixture", 3, 257, 16, 16, dict(word_score=-4.0, beam_threshold=INF)),
    ("fixture+sil", 70, 7, 2, 1, dict(word_score=1.5, sil_score=-0.5, beam_threshold=2.0)),
    ("fixture+sil", 1, 64, 1, 1, dict(sil_score=-0.5)),
    ("fixture", 3, 2, 10, 10, dict()),
    ("fixture+sil", 3, 1, 2, 2, dict(beam_threshold=2.0)),
    ("wide", 3, 64, 16, 16, dict(sil_score=-0.5, word_score=1.5)),
    ("wide", 70, 2, 10, 1, dict(beam_threshold=INF)),
    ("one", 3, 7, 2, 2, dict()),
    ("one", 1, 1, 1, 1, dict(word_score=-4.0)),
    ("prefix", 70, 7, 10, 10, dict(beam_threshold=2.0)),
    ("prefix", 3, 64, 16, 1, dict(word_score=1.5)),
]


@pytest.mark.parametrize("name,n,T,beam,nbest,opts", CASES, ids=[f"{c[0]}-n{c[1]}-T{c[2]}-b{c[3]}-k{c[4]}" for c in CASES])
def test_shapes_lexica_and_options_equal_the_statement(name, n, T, beam, nbest, opts):
    spellings, V, sil, _ = lexicon(name)
    ref, packed = tries(name)
    em = L.emissions(100 + n + T, spellings, n, T, V, 0, -1 if sil is None else sil)
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)  # 0 and T' + 1 included
        em_len[:2] = [1, T]
    want = D.decode_batch(em, ref, em_len, beam=beam, nbest=nbest, **opts)
    same(run(em, packed, em_len, beam_size=beam, nbest=nbest, **opts), want, nbest)


@pytest.mark.parametrize("name,n,T,beam", [("prefix", 70, 16, 10), ("fixture+sil", 3, 64, 16), ("wide", 3, 7, 2)])
def test_ties_are_decided_by_the_candidate_id(name, n, T, beam):
    """Log-probs on a grid of 0.25 and a block of uniform frames: equal scores at every step, in merging, in pruning and in
    the final order."""
    spellings, V, sil, _ = lexicon(name)
    ref, packed = tries(name)
    em = L.tie_emissions(7, spellings, n, T, V, 0, -1 if sil is None else sil)
    want = D.decode_batch(em, ref, beam=beam, nbest=beam, beam_threshold=INF)
    nh = same(run(em, packed, beam_size=beam, nbest=beam, beam_threshold=INF), want, beam)
    if name == "prefix":  # the small lexicon keeps hypotheses alive through the uniform frames: equal scores reach the end
        scores = [float(h[3]) for hyps in want for h in hyps]
        assert len(scores) > len(set(scores)) and (nh > 0).sum() > n // 2


def test_minus_infinity_and_nan_follow_the_drop_rule():
    """A fifth of the entries -inf in every sequence; NaN entries in sequence 1 and a whole NaN frame in sequence 2: those follow
    the drop rule (sequence 2 ends without a hypothesis), the neighbours are what they are without them."""
    spellings, V, sil, _ = lexicon("prefix")
    ref, packed = tries("prefix")
    em = L.emissions(21, spellings, 6, 16, V, peaks=(4.0, 8.0))
    rng = np.random.default_rng(22)
    em[rng.random(em.shape) < 0.2] = -np.inf
    clean = em.copy()
    em[1][rng.random(em[1].shape) < 0.1] = np.nan
    em[2, 5, :] = np.nan
    want = D.decode_batch(em, ref, beam=10, nbest=10)
    assert want[2] == [] and any(want[s] for s in (0, 3, 4, 5))
    got = run(em, packed, beam_size=10, nbest=10)
    same(got, want, 10)
    untouched = run(clean, packed, beam_size=10, nbest=10)
    for a, b in zip(got, untouched):
        assert np.array_equal(a[[0, 3, 4, 5]], b[[0, 3, 4, 5]], equal_nan=True)


def test_a_sequence_alone_equals_itself_in_the_batch_and_runs_repeat():
    em, em_len, want = main_reference()
    packed = tries("fixture+sil")[1]
    first = run(em, packed, em_len, beam_size=10, nbest=10)
    again = run(em, packed, em_len, beam_size=10, nbest=10)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for s in (0, 7, 41, 69):
        alone = run(em[s:s + 1], packed, em_len[s:s + 1], beam_size=10, nbest=10)
        for a, b in zip(alone, first):
            assert a[0].tobytes() == b[s].tobytes(), s
        same(alone, want[s:s + 1], 10)


def test_max_words_truncates_and_word_count_stays_true():
    em, em_len, want = main_reference()
    assert max(len(h[0]) for hyps in want for h in hyps) > 2
    got = run(em[:20], tries("fixture+sil")[1], em_len[:20], beam_size=10, nbest=10, max_words=2)
    assert got[0].shape == (20, 10, 2)
    same(got, want[:20], 10, max_words=2)


def test_a_trie_packed_for_other_labels_gives_no_hypothesis():
    spellings, V, sil, _ = lexicon("prefix")
    other = TokenTrie.from_spellings(spellings, V, blank=0, sil=None)
    other.sil = 20  # the call now states a sil token the image was not packed with
    em = L.emissions(5, spellings, 3, 7, V, peaks=(8.0,))
    got = run(em, other, beam_size=4, nbest=2)
    assert (got[6] == 0).all() and (got[5] == -np.inf).all() and (got[1] == 0).all() and (got[3] == 0).all()


def test_an_emission_of_another_width_than_the_trie_is_refused():
    with pytest.raises(ValueError, match="packed for 32"):
        ctc_lexicon_decode(torch.zeros(1, 3, 40, device="cuda"), tries("prefix")[1])


def test_beam_inference_ctc_predict():
    """The transcripts are the statement's, pprob is the softmax of the statement's scores (a float64 softmax of identical fp32
    inputs: 1e-6 covers its rounding), every word is a lexicon entry; an utterance without a hypothesis gives "" and 0."""
    em, _, spellings, words = L.main_case()
    ref, packed = tries("fixture+sil")
    em = em[40:56]  # full-length sequences
    want = D.decode_batch(em, ref, beam=10, nbest=4)
    assert any(want) and not all(want)

    class Args:
        beam_size = 10
    infer = BeamInference(Args(), trie=packed)
    dev = torch.from_numpy(em).cuda()
    texts = infer.ctc_predict_(dev, nbest=4)
    assert texts == [" ".join(words[w] for w in hyps[0][0]).strip() if hyps else "" for hyps in want]
    known = set(words)
    assert all(w in known for t in texts for w in t.split(" ") if t)
    assert infer.ctc_predict_(dev) == texts  # N_BEST = 1: the same best hypothesis
    for b, hyps in enumerate(want):
        text, pprob = infer.ctc_predict(dev[b:b + 1], index=3, nbest=4)
        assert text == [texts[b]]
        if hyps:
            sc = np.array([h[3] for h in hyps], dtype=np.float64)
            p = np.exp(sc - sc.max())
            assert abs(float(pprob) - p[0] / p.sum()) <= 1e-6
            assert float(infer.ctc_predict(dev[b:b + 1])[1]) == 1.0  # the reference's N_BEST = 1
        else:
            assert float(pprob) == 0.0
    with pytest.raises(ValueError, match="args.lexicon"):
        BeamInference(Args()).ctc_predict_(dev)


def test_one_launch_whatever_the_batch_and_capturable():
    """The call is captured into a graph (never replayed): it enqueues the same number of nodes -- one kernel -- for 1 and for 384
    sequences, allocates nothing and synchronises nothing."""
    lib = capi.load()
    spellings, V, sil, _ = lexicon("prefix")
    packed = tries("prefix")[1]
    dev = torch.device("cuda", torch.cuda.current_device())
    counts = {}
    for n in (1, 384):
        em = torch.from_numpy(L.emissions(n, spellings, n, 16, V)).cuda()
        image, bufs = packed.on(dev), raw_buffers(lib, em, 10, 2)
        counts[n] = captured_nodes(lib, lambda stream: raw_call(lib, "eec_ctc_lexbeam_decode", em, image, 10, 2, bufs, stream=stream))
    assert counts[1] == counts[384] == 1, counts
