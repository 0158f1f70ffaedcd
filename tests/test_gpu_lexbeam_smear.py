"""GPU tests of the lexicon-constrained CTC beam search with an n-gram model and LM look-ahead by max trie smearing
(csrc/ctc_lexbeam.hip, ``ctc_lexicon_decode(lm=..., smearing="max")``, ``BeamInference(..., smearing="max")``) against the
plain-Python statement of tests/lexbeam_statement.py (``smax=``).  As in tests/test_gpu_lexbeam_lm.py, with which it shares the
helpers and cached models of tests/lexbeam_helpers.py, there is nothing to tolerate: n_hyp, words, tokens, timesteps and counts are
compared as integers and scores as bit patterns, and every model goes the whole way: dict, ARPA text, ``NGramLM.from_arpa``,
``NGramLM.smear``."""
import functools

import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_smear_cases as S
import lexbeam_statement as D
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie
from early_exit_transformer_amd.model import ctc_lexicon_decode
from lexbeam_helpers import arpa_path, captured_nodes, lexicon, main_lm_reference, models, raw_buffers, raw_call, run, same, tries

pytestmark = pytest.mark.gpu
INF = float("inf")
ENTRY = "eec_ctc_lexbeam_lm_smear_decode"


@functools.lru_cache(maxsize=None)
def table(name, order, seed=50, **variant):
    """The statement's smear table for ``models(name, order, ...)`` over ``tries(name)``"""
    return S.smear(tries(name)[0], models(name, order, seed, **variant)[0], lexicon(name)[3])


# ----------------------------------------------------------------------------------------------------------------------------
# the main case
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_smeared(lm_weight):
    em, em_len, packed, plain, _, _, words, lm = main_lm_reference(lm_weight)
    ref = tries("fixture+sil")[0]
    smax = S.smear(ref, lm, words)
    return D.decode_batch(em, ref, em_len, beam=10, nbest=10, lm=lm, lm_weight=lm_weight, lm_words=words, smax=smax)


@pytest.mark.parametrize("lm_weight", [1.0, 3.23])
def test_the_main_case_makes_smearing_matter_and_equals_the_statement(lm_weight):
    """The LM suite's main case (70 x 64 frames, fixture lexicon with sil, a 3-gram, ragged lengths) at the reference's beam of 10,
    all 10 hypotheses.  Before the device is asked, the statement alone must show that smearing changes the search: among the
    sequences that end with a hypothesis with and without it -- at least 10 -- the best final score differs in at least 5, and
    in at least one of them smearing finds the better one."""
    em, em_len, packed, plain, _, _, words, lm = main_lm_reference(lm_weight)
    want = main_smeared(lm_weight)
    both = [s for s in range(70) if want[s] and plain[s]]
    changed = [s for s in both if M.bits(want[s][0][3]) != M.bits(plain[s][0][3])]
    print(f"lm_weight {lm_weight}: complete in both {len(both)}, best final score differs in {len(changed)}, "
          f"smeared better in {sum(1 for s in changed if want[s][0][3] > plain[s][0][3])}")
    assert len(both) >= 10 and len(changed) >= 5 and any(want[s][0][3] > plain[s][0][3] for s in changed)
    assert any(want[s][0][0] != plain[s][0][0] for s in changed), "... and with it the words"
    nh = same(run(em, tries("fixture+sil")[1], em_len, beam_size=10, nbest=10, lm=packed, lm_weight=lm_weight, smearing="max"), want, 10)
    assert nh.tolist() == [len(h) for h in want]


# ----------------------------------------------------------------------------------------------------------------------------
# the smallest shapes at which the kernel can still go wrong
# ----------------------------------------------------------------------------------------------------------------------------
CASES = [
    # lexicon, model order, model variant, n_seq, T', beam, nbest, options
    ("fixture+sil", 1, {}, 3, 16, 16, 16, dict(lm_weight=1.0)),
    ("fixture+sil", 2, {}, 3, 16, 2, 2, dict(lm_weight=1.0)),
    ("fixture+sil", 4, {}, 3, 16, 16, 16, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 70, 7, 2, 2, dict(lm_weight=1.0, beam_threshold=2.0)),
    ("fixture+sil", 3, {}, 70, 2, 1, 1, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 1, 1, 10, 10, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 3, 2, 16, 16, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 1, 16, 1, 1, dict(lm_weight=3.23)),
    ("prefix", 2, {}, 70, 16, 10, 10, dict(lm_weight=1.0)),
    ("prefix", 2, {}, 3, 1, 16, 16, dict(lm_weight=1.0)),
    ("wide", 2, {}, 3, 16, 16, 16, dict(lm_weight=1.0, sil_score=-0.5)),
    ("wide", 2, {}, 70, 1, 2, 2, dict(lm_weight=1.0)),
    ("fixture+sil", 3, {}, 3, 32, 10, 10, dict(lm_weight=1.0, word_score=-4.0)),
    ("fixture+sil", 4, dict(positive_backoff=True), 3, 32, 10, 10, dict(lm_weight=3.23)),
    ("fixture+sil", 3, dict(bos=False, eos=False), 3, 32, 10, 10, dict(lm_weight=1.0)),
]


@pytest.mark.parametrize("name,order,variant,n,T,beam,nbest,opts", CASES,
                         ids=[f"{c[0]}-o{c[1]}{''.join('-' + k for k in c[2])}-n{c[3]}-T{c[4]}-b{c[5]}-k{c[6]}-{'-'.join(f'{k}{v}' for k, v in c[7].items())}"
                              for c in CASES])
def test_shapes_orders_lexica_and_options_equal_the_statement(name, order, variant, n, T, beam, nbest, opts):
    """T' 1 and 2, beams 1, 2 and 16, 1, 3 and 70 sequences (ragged lengths with 0, 1, T' and T' + 1), V = 32 with words that are
    prefixes of words (a node both ends a word and has children), V = 256 where thread 255 owns a label and with sil, single-token
    words (pmax = 0 at the root), orders 1 to 4, no <s> / </s>, positive back-offs, word_score -4, a finite threshold."""
    spellings, V, sil, words = lexicon(name)
    ref, packed_trie = tries(name)
    lm, packed, favoured, disfavoured = models(name, order, **variant)
    em = M.lm_emissions(200 + n + T, favoured, disfavoured, words, spellings, n, T, V, 0, -1 if sil is None else sil, peaks=(4.0, 8.0, 6.0))
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)  # 0 and T' + 1 included
        em_len[:4] = [1, T, 0, T + 1]
    want = D.decode_batch(em, ref, em_len, beam=beam, nbest=nbest, lm=lm, lm_words=words, smax=table(name, order, **variant), **opts)
    nh = same(run(em, packed_trie, em_len, beam_size=beam, nbest=nbest, lm=packed, smearing="max", **opts), want, nbest)
    if T >= 16 and beam >= 10:
        assert (nh > 0).any(), "the case decodes something"


@pytest.mark.parametrize("name,order,n,T,beam", [("fixture+sil", 3, 3, 32, 10), ("prefix", 2, 70, 16, 16), ("wide", 2, 3, 2, 1)])
def test_at_lm_weight_0_smearing_is_the_unsmeared_entry_bitwise(name, order, n, T, beam):
    spellings, V, sil, words = lexicon(name)
    lm, packed, favoured, disfavoured = models(name, order)
    em = M.lm_emissions(300 + T, favoured, disfavoured, words, spellings, n, T, V, 0, -1 if sil is None else sil, peaks=(4.0, 8.0, 6.0))
    plain = run(em, tries(name)[1], beam_size=beam, nbest=beam, lm=packed, lm_weight=0.0)
    smeared = run(em, tries(name)[1], beam_size=beam, nbest=beam, lm=packed, lm_weight=0.0, smearing="max")
    for a, b in zip(plain, smeared):
        assert a.tobytes() == b.tobytes()
    assert T < 16 or (plain[6] > 0).any()


@pytest.mark.parametrize("name,n,T,beam", [("prefix", 70, 16, 10), ("fixture+sil", 3, 32, 16)])
def test_ties_with_a_grid_valued_model_are_decided_by_the_candidate_id(name, n, T, beam):
    """Log-probs on a grid of 0.25 with a block of uniform frames, model values -- and so the table's -- on a grid of 1/8,
    lm_weight 1: equal scores at every step, in merging, in pruning and in the final order."""
    spellings, V, sil, words = lexicon(name)
    ref, packed_trie = tries(name)
    order = 2 if name == "prefix" else 3
    lm, packed, _, _ = models(name, order, grid=True)
    em = L.tie_emissions(7, spellings, n, T, V, 0, -1 if sil is None else sil)
    want = D.decode_batch(em, ref, beam=beam, nbest=beam, beam_threshold=INF, lm=lm, lm_weight=1.0, lm_words=words, smax=table(name, order, grid=True))
    nh = same(run(em, packed_trie, beam_size=beam, nbest=beam, beam_threshold=INF, lm=packed, lm_weight=1.0, smearing="max"), want, beam)
    if name == "prefix":
        scores = [float(h[3]) for hyps in want for h in hyps]
        assert len(scores) > len(set(scores)) and (nh > 0).sum() > n // 2


# ----------------------------------------------------------------------------------------------------------------------------
# pruning and telescoping, on the device
# ----------------------------------------------------------------------------------------------------------------------------
def small_pair(tag, spellings, words, lm):
    trie = TokenTrie.from_spellings(spellings, S.PRUNE_V, blank=0, words=words)
    return trie, NGramLM.from_arpa(arpa_path(lm, tag), trie)


def test_at_beam_1_smearing_keeps_the_word_the_model_prefers():
    """{ab, cd}, unigrams -1 and -5, c acoustically ahead of a by 1/8: unsmeared cd at -6.875, smeared ab at -3.0.  With abd below
    ab the in-word and the word-end candidate tie at -3.0, the in-word one (the lower id) takes the single slot: no hypothesis."""
    spellings, words, lm, em = S.pruning_case()
    trie, packed = small_pair("prune", spellings, words, lm)
    kw = dict(beam_size=1, nbest=1, lm=packed, lm_weight=1.0)
    plain, smeared = run(em[None], trie, **kw), run(em[None], trie, smearing="max", **kw)
    assert plain[0][0, 0, :1].tolist() == [1] and plain[5][0, 0] == np.float32(-6.875) and plain[2][0, 0, :2].tolist() == [S.C_, S.D]
    assert smeared[0][0, 0, :1].tolist() == [0] and smeared[5][0, 0] == np.float32(-3.0) and smeared[2][0, 0, :2].tolist() == [S.A, S.B_]
    ref = L.Trie(spellings, S.PRUNE_V, 0, None)
    same(smeared, [D.decode(em, ref, beam=1, nbest=1, lm=lm, lm_weight=1.0, lm_words=words, smax=S.smear(ref, lm, words))], 1)

    spellings, words, lm, em = S.pruning_case(extra_abd=True)
    trie, packed = small_pair("prune-abd", spellings, words, lm)
    ref = L.Trie(spellings, S.PRUNE_V, 0, None)
    smax = S.smear(ref, lm, words)
    for beam, n_hyp in ((1, 0), (2, 1)):
        got = run(em[None], trie, beam_size=beam, nbest=beam, lm=packed, lm_weight=1.0, smearing="max")
        assert got[6].tolist() == [n_hyp]
        same(got, [D.decode(em, ref, beam=beam, nbest=beam, lm=lm, lm_weight=1.0, lm_words=words, smax=smax)], beam)


@pytest.mark.parametrize("T", [1, 2])
def test_where_nothing_is_pruned_the_payments_telescope(T):
    """Dyadic values, no threshold, beam 16, at most 16 candidates per frame (the statement's count, asserted): the smeared and the
    unsmeared entry return the same set of (words, tokens, timesteps, score bits) -- ranks may differ.  Eight models, one launch
    each way per model."""
    for seed in range(8):
        spellings, words, lm, em = S.telescoping_case(seed, T, n=6)
        trie, packed = small_pair(f"tele-{T}-{seed}", spellings, words, lm)
        ref = L.Trie(spellings, S.PRUNE_V, 0, None)
        stats = {}
        want = D.decode_batch(em, ref, beam=16, nbest=16, beam_threshold=INF, lm=lm, lm_weight=2.0, lm_words=words, smax=S.smear(ref, lm, words),
                              stats=stats)
        assert stats["max_candidates"] <= 16
        kw = dict(beam_size=16, nbest=16, beam_threshold=INF, lm=packed, lm_weight=2.0)
        plain, smeared = run(em, trie, **kw), run(em, trie, smearing="max", **kw)
        same(smeared, want, 16)

        def sets(out):
            words_, wc, toks, tc, ts, sc, nh = out
            return [{(tuple(words_[s, j, :wc[s, j]].tolist()), tuple(toks[s, j, :tc[s, j]].tolist()), tuple(ts[s, j, :tc[s, j]].tolist()),
                      int(sc[s, j].view(np.int32))) for j in range(nh[s])} for s in range(len(nh))]
        assert sets(plain) == sets(smeared) == [S.as_set(h) for h in want] and all(len(h) for h in want)


# ----------------------------------------------------------------------------------------------------------------------------
# a table for another trie; determinism; the launch
# ----------------------------------------------------------------------------------------------------------------------------
def test_a_table_for_another_trie_is_refused_or_gives_no_hypothesis():
    spellings, V, sil, words = lexicon("prefix")
    _, packed_trie = tries("prefix")
    lm, packed, favoured, disfavoured = models("prefix", 2)
    shorter = TokenTrie.from_spellings(spellings[:-1], V, blank=0, words=words[:-1])
    em = M.lm_emissions(5, favoured, disfavoured, words, spellings, 3, 7, V, peaks=(8.0,))
    with pytest.raises(ValueError, match="packed for a lexicon of 8 words, the trie has 7"):
        ctc_lexicon_decode(torch.from_numpy(em).cuda(), shorter, lm=packed, lm_weight=1.0, smearing="max")
    with pytest.raises(ValueError, match="needs lm="):
        ctc_lexicon_decode(torch.from_numpy(em).cuda(), packed_trie, smearing="max")
    lib = capi.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    dev_em = torch.from_numpy(em).to(dev)
    smear = packed.smear(packed_trie)
    out = raw_buffers(lib, dev_em, 4, 2)
    assert raw_call(lib, ENTRY, dev_em, packed_trie.on(dev), 4, 2, out, packed.on(dev).data_ptr(), 1.0, smear.on(dev).data_ptr()) == 0 and (out[6] > 0).any()
    for dword, value in ((1, packed_trie.n_nodes - 1), (1, packed_trie.n_nodes + 1), (0, M.LM_MAGIC)):  # another node count; another image's magic
        image = smear._image.clone()
        image.view(torch.int32)[dword] = value
        image = image.to(dev)  # held in a name: the call takes its address
        out = raw_buffers(lib, dev_em, 4, 2)
        assert raw_call(lib, ENTRY, dev_em, packed_trie.on(dev), 4, 2, out, packed.on(dev).data_ptr(), 1.0, image.data_ptr()) == 0
        assert (out[6] == 0).all() and (out[5] == -np.inf).all() and (out[1] == 0).all() and (out[3] == 0).all() and (out[0] == -1).all()


def test_a_sequence_alone_equals_itself_in_the_batch_and_runs_repeat():
    em, em_len, packed, _, _, _, _, _ = main_lm_reference(1.0)
    want = main_smeared(1.0)
    packed_trie = tries("fixture+sil")[1]
    kw = dict(beam_size=10, nbest=10, lm=packed, lm_weight=1.0, smearing="max")
    first, again = run(em, packed_trie, em_len, **kw), run(em, packed_trie, em_len, **kw)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for s in (0, 7, 41, 69):
        alone = run(em[s:s + 1], packed_trie, em_len[s:s + 1], **kw)
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
        trie_image, lm_image, smear_image, bufs = packed_trie.on(dev), packed.on(dev), packed.smear(packed_trie).on(dev), raw_buffers(lib, em, 10, 2)
        counts[n] = captured_nodes(lib, lambda stream: raw_call(lib, ENTRY, em, trie_image, 10, 2, bufs, lm_image.data_ptr(), 1.0, smear_image.data_ptr(),
                                                                stream=stream))
    assert counts[1] == counts[384] == 1, counts


# ----------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------------------------------------------
class _Counted:
    """Counts the calls of the library's three lexicon decoder entries."""
    NAMES = ("eec_ctc_lexbeam_decode", "eec_ctc_lexbeam_lm_decode", "eec_ctc_lexbeam_lm_smear_decode")

    def __init__(self, monkeypatch):
        self.calls = []
        lib = capi.load()
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, fn):
        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def test_beam_inference_with_smearing_and_the_default_issues_todays_calls(monkeypatch):
    """``BeamInference(..., smearing="max")`` and ``args.lm_smearing`` return the smeared statement's transcripts through one call
    of the new entry; with ``smearing=None`` the calls are the ones made before the keyword existed -- one eec_ctc_lexbeam_lm_decode
    with a model, one eec_ctc_lexbeam_decode without --, no table is built, and the outputs equal the call without the keyword."""
    em, _, packed, _, _, _, words, lm = main_lm_reference(1.0)
    ref, packed_trie = tries("fixture+sil")
    em = em[40:56]  # full-length sequences
    smax = S.smear(ref, lm, words)
    want = D.decode_batch(em, ref, beam=10, nbest=4, lm=lm, lm_weight=1.0, lm_words=words, smax=smax)
    plain = D.decode_batch(em, ref, beam=10, nbest=4, lm=lm, lm_weight=1.0, lm_words=words)
    text = lambda hyps: " ".join(words[w] for w in hyps[0][0]).strip() if hyps else ""  # noqa: E731
    assert any(want) and [text(h) for h in want] != [text(h) for h in plain]

    class Args:
        beam_size = 10
    dev = torch.from_numpy(em).cuda()
    fresh = NGramLM.from_arpa(arpa_path(lm, "main-fresh"), packed_trie)
    counted = _Counted(monkeypatch)
    off = BeamInference(Args(), trie=packed_trie, lm=fresh)
    assert off.ctc_predict_(dev, nbest=4) == [text(h) for h in plain]
    assert counted.calls == ["eec_ctc_lexbeam_lm_decode"] and fresh._smear is None
    a = ctc_lexicon_decode(dev, packed_trie, beam_size=10, nbest=4, lm=fresh, lm_weight=1.0, smearing=None)
    b = ctc_lexicon_decode(dev, packed_trie, beam_size=10, nbest=4, lm=fresh, lm_weight=1.0)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    ctc_lexicon_decode(dev, packed_trie, beam_size=10, nbest=4, smearing=None)
    assert counted.calls == ["eec_ctc_lexbeam_lm_decode"] * 3 + ["eec_ctc_lexbeam_decode"] and fresh._smear is None

    del counted.calls[:]
    on = BeamInference(Args(), trie=packed_trie, lm=fresh, smearing="max")
    assert on.ctc_predict_(dev, nbest=4) == [text(h) for h in want]
    assert counted.calls == ["eec_ctc_lexbeam_lm_smear_decode"] and fresh._smear[0] is packed_trie
    by_args = Args()
    by_args.lm_smearing = "max"
    assert BeamInference(by_args, trie=packed_trie, lm=fresh).ctc_predict_(dev, nbest=4) == [text(h) for h in want]
    for b_, hyps in enumerate(want[:4]):
        got, pprob = on.ctc_predict(dev[b_:b_ + 1], index=3, nbest=4)
        assert got == [text(hyps)]
        if hyps:
            sc = np.array([h[3] for h in hyps], dtype=np.float64)
            p = np.exp(sc - sc.max())
            assert abs(float(pprob) - p[0] / p.sum()) <= 1e-6
        else:
            assert float(pprob) == 0.0
    assert BeamInference(by_args, trie=packed_trie).ctc_predict_(dev, nbest=4) == [text(h) for h in D.decode_batch(em, ref, beam=10, nbest=4)]
