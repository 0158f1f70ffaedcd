"""GPU tests of the lexicon-constrained CTC beam search with an n-gram language model (csrc/ctc_lexbeam.hip,
``ctc_lexicon_decode(lm=...)``, ``BeamInference(..., lm=...)``) against the plain-Python statement of tests/lexbeam_statement.py.
There is nothing to tolerate: the arithmetic is fp32 additions and one separately rounded product in a stated order, so n_hyp,
words, tokens, timesteps and counts are compared as integers and scores as bit patterns.  Every model goes the whole way: generated
as a dict, written as ARPA text, read by ``NGramLM.from_arpa`` and packed."""
import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_statement as D
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie
from early_exit_transformer_amd.model import ctc_lexicon_decode
from lexbeam_helpers import arpa_path, captured_nodes, lexicon, main_lm_reference, models, raw_buffers, raw_call, run, same, tries

pytestmark = pytest.mark.gpu
INF = float("inf")
ENTRY = "eec_ctc_lexbeam_lm_decode"


# ----------------------------------------------------------------------------------------------------------------------------
# the main case
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_weight", [1.0, 3.23])
def test_the_main_case_makes_the_model_matter_and_equals_the_statement(lm_weight):
    """70 sequences x 64 frames over the fixture lexicon with sil, beam 10, all 10 hypotheses, a 3-gram model, ragged lengths with
    1, T' and values outside [1, T'].  Before the device is asked, the statement alone must show that the case exercises the model:
    it changes the best hypothesis in at least a quarter of the sequences that have one with and without it, the </s> term changes
    the order of the complete hypotheses in at least three sequences, every back-off depth 0 .. 2 is taken, a word the model lacks
    (scored as <unk>) is in a returned hypothesis, and at least a quarter of the in-range sequences end with a hypothesis and a
    tenth without."""
    em, em_len, packed, want, stats, free, words, lm = main_lm_reference(lm_weight)
    both = [s for s in range(70) if want[s] and free[s]]
    assert sum(1 for s in both if want[s][0][0] != free[s][0][0]) >= 0.25 * len(both) and len(both) >= 10
    assert stats.get("eos_reordered", 0) >= 3
    assert set(stats["depth"]) == {0, 1, 2} and min(stats["depth"].values()) >= 1
    assert any((words[w],) not in lm for hyps in want for h in hyps for w in h[0])
    inside = (em_len >= 1) & (em_len <= 64)
    nh_want = np.array([len(h) for h in want])
    assert (nh_want[inside] > 0).sum() >= 0.25 * 70 and (nh_want[inside] == 0).sum() >= 0.10 * 70
    assert (nh_want[~inside] == 0).all() and (~inside).sum() == 3 and {1, 64, 0, 65} <= set(em_len.tolist())
    nh = same(run(em, tries("fixture+sil")[1], em_len, beam_size=10, nbest=10, lm=packed, lm_weight=lm_weight), want, 10)
    assert nh.tolist() == nh_want.tolist()


# ----------------------------------------------------------------------------------------------------------------------------
# shapes, orders, lexica, options
# ----------------------------------------------------------------------------------------------------------------------------
CASES = [
    # lexicon, model order, model variant, n_seq, T', beam, nbest, options
    ("fixture+sil", 1, {}, 3, 64, 16, 16, dict(lm_weight=1.0)),
    ("fixture+sil", 2, {}, 3, 64, 16, 16, dict(lm_weight=1.0)),
    ("fixture+sil", 4, {}, 3, 64, 16, 16, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 70, 7, 2, 2, dict(lm_weight=1.0, beam_threshold=2.0)),
    ("fixture+sil", 3, {}, 1, 1, 10, 10, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 3, 2, 10, 10, dict(lm_weight=1.0)),
    ("prefix", 2, {}, 70, 16, 10, 10, dict(lm_weight=1.0)),
    ("wide", 2, {}, 3, 64, 16, 16, dict(lm_weight=1.0, sil_score=-0.5)),
    ("fixture+sil", 3, {}, 3, 64, 10, 10, dict(lm_weight=1.0, word_score=-4.0)),
    ("fixture+sil", 3, {}, 3, 64, 10, 10, dict(lm_weight=0.0)),
    ("fixture+sil", 4, dict(positive_backoff=True), 3, 64, 10, 10, dict(lm_weight=3.23)),
    ("fixture+sil", 3, dict(bos=False, eos=False), 3, 64, 10, 10, dict(lm_weight=1.0)),
]


@pytest.mark.parametrize("name,order,variant,n,T,beam,nbest,opts", CASES,
                         ids=[f"{c[0]}-o{c[1]}{''.join('-' + k for k in c[2])}-n{c[3]}-T{c[4]}-b{c[5]}-k{c[6]}-{'-'.join(f'{k}{v}' for k, v in c[7].items())}"
                              for c in CASES])
def test_shapes_orders_lexica_and_options_equal_the_statement(name, order, variant, n, T, beam, nbest, opts):
    spellings, V, sil, words = lexicon(name)
    ref, packed_trie = tries(name)
    lm, packed, favoured, disfavoured = models(name, order, **variant)
    em = M.lm_emissions(100 + n + T, favoured, disfavoured, words, spellings, n, T, V, 0, -1 if sil is None else sil, peaks=(4.0, 8.0, 6.0))
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)  # 0 and T' + 1 included
        em_len[:2] = [1, T]
    want = D.decode_batch(em, ref, em_len, beam=beam, nbest=nbest, lm=lm, lm_words=words, **opts)
    nh = same(run(em, packed_trie, em_len, beam_size=beam, nbest=nbest, lm=packed, **opts), want, nbest)
    if T >= 16:
        assert (nh > 0).any(), "the case decodes something"


@pytest.mark.parametrize("name,n,T,beam", [("prefix", 70, 16, 10), ("fixture+sil", 3, 64, 16)])
def test_ties_with_a_grid_valued_model_are_decided_by_the_candidate_id(name, n, T, beam):
    """Log-probs on a grid of 0.25 with a block of uniform frames, model values on a grid of 1/8, lm_weight 1: equal scores at every
    step, in merging, in pruning and in the final order."""
    spellings, V, sil, words = lexicon(name)
    ref, packed_trie = tries(name)
    lm, packed, _, _ = models(name, 2 if name == "prefix" else 3, grid=True)
    em = L.tie_emissions(7, spellings, n, T, V, 0, -1 if sil is None else sil)
    want = D.decode_batch(em, ref, beam=beam, nbest=beam, beam_threshold=INF, lm=lm, lm_weight=1.0, lm_words=words)
    nh = same(run(em, packed_trie, beam_size=beam, nbest=beam, beam_threshold=INF, lm=packed, lm_weight=1.0), want, beam)
    if name == "prefix":
        scores = [float(h[3]) for hyps in want for h in hyps]
        assert len(scores) > len(set(scores)) and (nh > 0).sum() > n // 2


# ----------------------------------------------------------------------------------------------------------------------------
# a model for another trie; determinism; the launch
# ----------------------------------------------------------------------------------------------------------------------------
def test_a_model_packed_for_another_trie_is_refused_or_gives_no_hypothesis():
    spellings, V, sil, words = lexicon("prefix")
    _, packed_trie = tries("prefix")
    lm, packed, favoured, disfavoured = models("prefix", 2)
    shorter = TokenTrie.from_spellings(spellings[:-1], V, blank=0, words=words[:-1])
    em = M.lm_emissions(5, favoured, disfavoured, words, spellings, 3, 7, V, peaks=(8.0,))
    with pytest.raises(ValueError, match="packed for a lexicon of 8 words, the trie has 7"):
        ctc_lexicon_decode(torch.from_numpy(em).cuda(), shorter, lm=packed, lm_weight=1.0)
    lib = capi.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    dev_em = torch.from_numpy(em).to(dev)
    out = raw_buffers(lib, dev_em, 4, 2)
    assert raw_call(lib, ENTRY, dev_em, packed_trie.on(dev), 4, 2, out, packed.on(dev).data_ptr(), 1.0) == 0 and (out[6] > 0).any()
    for dword, value in ((5, 7), (0, L.MAGIC)):  # the header's lexicon word count altered; another image's magic
        image = packed._image.clone()
        image.view(torch.int32)[dword] = value
        image = image.to(dev)  # held in a name: the call takes its address
        out = raw_buffers(lib, dev_em, 4, 2)
        assert raw_call(lib, ENTRY, dev_em, packed_trie.on(dev), 4, 2, out, image.data_ptr(), 1.0) == 0
        assert (out[6] == 0).all() and (out[5] == -np.inf).all() and (out[1] == 0).all() and (out[3] == 0).all() and (out[0] == -1).all()


def test_a_sequence_alone_equals_itself_in_the_batch_and_runs_repeat():
    em, em_len, packed, want, _, _, _, _ = main_lm_reference(1.0)
    packed_trie = tries("fixture+sil")[1]
    first = run(em, packed_trie, em_len, beam_size=10, nbest=10, lm=packed, lm_weight=1.0)
    again = run(em, packed_trie, em_len, beam_size=10, nbest=10, lm=packed, lm_weight=1.0)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for s in (0, 7, 41, 69):
        alone = run(em[s:s + 1], packed_trie, em_len[s:s + 1], beam_size=10, nbest=10, lm=packed, lm_weight=1.0)
        for a, b in zip(alone, first):
            assert a[0].tobytes() == b[s].tobytes(), s
        same(alone, want[s:s + 1], 10)


def test_one_launch_whatever_the_batch_and_capturable():
    """The call is captured into a graph (never replayed): it enqueues the same number of nodes -- one kernel -- for 1 and for 384
    sequences, allocates nothing and synchronises nothing."""
    lib = capi.load()
    spellings, V, sil, words = lexicon("prefix")
    packed_trie = tries("prefix")[1]
    packed = models("prefix", 2)[1]
    dev = torch.device("cuda", torch.cuda.current_device())
    counts = {}
    for n in (1, 384):
        em = torch.from_numpy(L.emissions(n, spellings, n, 16, V)).cuda()
        trie_image, lm_image, bufs = packed_trie.on(dev), packed.on(dev), raw_buffers(lib, em, 10, 2)
        counts[n] = captured_nodes(lib, lambda stream: raw_call(lib, ENTRY, em, trie_image, 10, 2, bufs, lm_image.data_ptr(), 1.0, stream=stream))
    assert counts[1] == counts[384] == 1, counts


# ----------------------------------------------------------------------------------------------------------------------------
# BeamInference
# ----------------------------------------------------------------------------------------------------------------------------
def test_beam_inference_with_a_model():
    """The transcripts are the statement's at LM_WEIGHT and at a given lm_weight, pprob is the softmax of the statement's final
    scores (a float64 softmax of identical fp32 inputs: 1e-6 covers its rounding); a path given as args.lm is read at the first
    use; without a model nothing changes."""
    em, _, packed, _, _, _, words, lm = main_lm_reference(1.0)
    ref, packed_trie = tries("fixture+sil")
    em = em[40:56]  # full-length sequences
    want = {wt: D.decode_batch(em, ref, beam=10, nbest=4, lm=lm, lm_weight=wt, lm_words=words) for wt in (1.0, 3.23)}
    assert any(want[1.0]) and not all(want[1.0])
    text = lambda hyps: " ".join(words[w] for w in hyps[0][0]).strip() if hyps else ""  # noqa: E731

    class Args:
        beam_size = 10
    assert BeamInference.LM_WEIGHT == 1.0
    infer = BeamInference(Args(), trie=packed_trie, lm=packed)
    dev = torch.from_numpy(em).cuda()
    assert infer.ctc_predict_(dev, nbest=4) == [text(h) for h in want[1.0]]
    assert infer.ctc_predict_(dev, nbest=4, lm_weight=3.23) == [text(h) for h in want[3.23]]
    assert [text(h) for h in want[1.0]] != [text(h) for h in want[3.23]]
    for b, hyps in enumerate(want[1.0]):
        got, pprob = infer.ctc_predict(dev[b:b + 1], index=3, nbest=4)
        assert got == [text(hyps)]
        if hyps:
            sc = np.array([h[3] for h in hyps], dtype=np.float64)
            p = np.exp(sc - sc.max())
            assert abs(float(pprob) - p[0] / p.sum()) <= 1e-6
        else:
            assert float(pprob) == 0.0

    with_path = Args()
    with_path.lm = arpa_path(lm, "by-path")
    by_path = BeamInference(with_path, trie=packed_trie)
    assert by_path._lm_read is None  # not read yet
    assert by_path.ctc_predict_(dev, nbest=4) == [text(h) for h in want[1.0]]
    assert isinstance(by_path._lm_read[1], NGramLM) and by_path._lm_read[0] is packed_trie
    first = by_path._lm_read[1]
    by_path.ctc_predict(dev[:1])
    assert by_path._lm_read[1] is first  # read once

    free = D.decode_batch(em, ref, beam=10, nbest=4)
    plain, none = BeamInference(Args(), trie=packed_trie), BeamInference(Args(), trie=packed_trie, lm=None)
    assert plain.ctc_predict_(dev, nbest=4) == none.ctc_predict_(dev, nbest=4) == [text(h) for h in free]
    assert plain.ctc_predict_(dev, nbest=4, lm_weight=3.23) == [text(h) for h in free]  # no model: the weight has nothing to weigh
    for b in (0, 1, 2):
        a, c = plain.ctc_predict(dev[b:b + 1], nbest=4), none.ctc_predict(dev[b:b + 1], nbest=4)
        assert a[0] == c[0] and float(a[1]) == float(c[1])
