"""GPU tests of the lexicon-constrained CTC beam search with an n-gram language model (csrc/ctc_lexbeam.hip,
``ctc_lexicon_decode(lm=...)``, ``BeamInference(..., lm=...)``) against the plain-Python statement of tests/lexbeam_lm_cases.py.
There is nothing to tolerate: the arithmetic is fp32 additions and one separately rounded product in a stated order, so n_hyp,
words, tokens, timesteps and counts are compared as integers and scores as bit patterns.  Every model goes the whole way: generated
as a dict, written as ARPA text, read by ``NGramLM.from_arpa`` and packed."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_lm_cases as M
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie
from early_exit_transformer_amd.model import ctc_lexicon_decode

pytestmark = pytest.mark.gpu
INF = float("inf")
_TMP = tempfile.TemporaryDirectory(prefix="eec_lm_")


@functools.lru_cache(maxsize=None)
def lexicon(name):
    """(spellings, V, sil or None, words)"""
    if name.startswith("fixture"):
        _, words, spellings = L.load_fixture()
        return spellings, 256, (126 if name == "fixture+sil" else None), words
    spellings, V, sil = {"prefix": (L.PREFIX_DOUBLED, 32, None), "wide": (L.wide_lexicon(), 256, 126)}[name]
    return spellings, V, sil, [f"w{i}" for i in range(len(spellings))]


@functools.lru_cache(maxsize=None)
def tries(name):
    """(the statement's trie, the packed one)"""
    spellings, V, sil, words = lexicon(name)
    return L.Trie(spellings, V, 0, sil), TokenTrie.from_spellings(spellings, V, blank=0, sil=sil, words=words)


def arpa_path(lm, tag):
    path = os.path.join(_TMP.name, f"{tag}.arpa")
    M.write_arpa(path, lm)
    return path


@functools.lru_cache(maxsize=None)
def models(name, order, seed=50, **variant):
    """(model dict, packed NGramLM, favoured, disfavoured) over the words of lexicon ``name``"""
    lm, favoured, disfavoured = M.random_model(seed, lexicon(name)[3], order, **variant)
    packed = NGramLM.from_arpa(arpa_path(lm, f"{name}-{order}-{seed}-{'-'.join(variant)}"), tries(name)[1])
    return lm, packed, favoured, disfavoured


def run(em, packed, em_len=None, **kw):
    out = ctc_lexicon_decode(torch.from_numpy(em).cuda(), packed, em_len=None if em_len is None else torch.from_numpy(np.asarray(em_len, dtype=np.int32)),
                             **kw)
    return [o.cpu().numpy() for o in out]


def same(got, want, nbest, max_words=None):
    """Every output of a batch against the statement's hypothesis lists; returns n_hyp."""
    words, wc, toks, tc, ts, sc, nh = got
    assert nh.tolist() == [len(w) for w in want]
    for s, hyps in enumerate(want):
        for j in range(nbest):
            if j >= len(hyps):
                assert wc[s, j] == 0 and tc[s, j] == 0 and sc[s, j] == -np.inf, (s, j)
                assert (words[s, j] == -1).all() and (toks[s, j] == -1).all() and (ts[s, j] == -1).all(), (s, j)
                continue
            w, tk, st, score = hyps[j]
            kept = len(w) if max_words is None else min(len(w), max_words)
            assert wc[s, j] == len(w) and words[s, j, :kept].tolist() == w[:kept] and (words[s, j, kept:] == -1).all(), (s, j)
            assert tc[s, j] == len(tk) and toks[s, j, :len(tk)].tolist() == tk and ts[s, j, :len(tk)].tolist() == st, (s, j)
            assert (toks[s, j, len(tk):] == -1).all() and (ts[s, j, len(tk):] == -1).all(), (s, j)
            assert sc[s, j].view(np.int32) == np.float32(score).view(np.int32), (s, j, sc[s, j], score)
    return nh


# ----------------------------------------------------------------------------------------------------------------------------
# the main case
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_reference(lm_weight):
    """(emission, em_len, packed model, the statement's hypotheses, its stats, the model-free statement's hypotheses, words, model)"""
    em, em_len, spellings, words, lm = M.main_lm_case()
    ref, packed_trie = tries("fixture+sil")
    packed = NGramLM.from_arpa(arpa_path(lm, "main"), packed_trie)
    stats = {}
    want = M.decode_batch(em, ref, em_len, beam=10, nbest=10, lm=lm, lm_weight=lm_weight, lm_words=words, stats=stats)
    return em, em_len, packed, want, stats, main_free(), words, lm


@functools.lru_cache(maxsize=None)
def main_free():
    em, em_len, spellings, _, _ = M.main_lm_case()
    return L.decode_batch(em, tries("fixture+sil")[0], em_len, beam=10, nbest=10)


@pytest.mark.parametrize("lm_weight", [1.0, 3.23])
def test_the_main_case_makes_the_model_matter_and_equals_the_statement(lm_weight):
    """70 sequences x 64 frames over the fixture lexicon with sil, beam 10, all 10 hypotheses, a 3-gram model, ragged lengths with
    1, T' and values outside [1, T'].  Before the device is asked, the statement alone must show that the case exercises the model:
    it changes the best hypothesis in at least a quarter of the sequences that have one with and without it, the </s> term changes
    the order of the complete hypotheses in at least three sequences, every back-off depth 0 .. 2 is taken, a word the model lacks
    (scored as <unk>) is in a returned hypothesis, and at least a quarter of the in-range sequences end with a hypothesis and a
    tenth without."""
    em, em_len, packed, want, stats, free, words, lm = main_reference(lm_weight)
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
    want = M.decode_batch(em, ref, em_len, beam=beam, nbest=nbest, lm=lm, lm_words=words, **opts)
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
    want = M.decode_batch(em, ref, beam=beam, nbest=beam, beam_threshold=INF, lm=lm, lm_weight=1.0, lm_words=words)
    nh = same(run(em, packed_trie, beam_size=beam, nbest=beam, beam_threshold=INF, lm=packed, lm_weight=1.0), want, beam)
    if name == "prefix":
        scores = [float(h[3]) for hyps in want for h in hyps]
        assert len(scores) > len(set(scores)) and (nh > 0).sum() > n // 2


# ----------------------------------------------------------------------------------------------------------------------------
# a model for another trie; determinism; the launch
# ----------------------------------------------------------------------------------------------------------------------------
def raw_buffers(lib, em, beam, nbest):
    """(words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace) on the emission's device"""
    n, T, V = em.shape
    dev = em.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    sc = torch.empty((n, nbest), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.eec_ctc_lexbeam_workspace_bytes(n, T, beam), dtype=torch.uint8, device=dev)
    return i32(n, nbest, T), i32(n, nbest), i32(n, nbest, T), i32(n, nbest), i32(n, nbest, T), sc, i32(n), ws


def raw_call(lib, em, trie_image, lm_image, beam, nbest, bufs, stream=None, sil=-1, lm_weight=1.0):
    """The bare C entry on device buffers that exist already: the return code."""
    n, T, V = em.shape
    dev = em.device
    words, wc, toks, tc, ts, sc, nh, ws = bufs
    ws_bytes = ws.numel()
    return lib.eec_ctc_lexbeam_lm_decode(em.data_ptr(), n, T, V, None, trie_image.data_ptr(), 0, sil, beam, nbest, 0.0, 0.0, 50.0, T, words.data_ptr(),
                                       wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(), nh.data_ptr(), ws.data_ptr(),
                                       ws_bytes, capi.stream_ptr(dev) if stream is None else stream, lm_image.data_ptr(), lm_weight)


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
    assert raw_call(lib, dev_em, packed_trie.on(dev), packed.on(dev), 4, 2, out) == 0 and (out[6] > 0).any()
    for dword, value in ((5, 7), (0, L.MAGIC)):  # the header's lexicon word count altered; another image's magic
        image = packed._image.clone()
        image.view(torch.int32)[dword] = value
        out = raw_buffers(lib, dev_em, 4, 2)
        assert raw_call(lib, dev_em, packed_trie.on(dev), image.to(dev), 4, 2, out) == 0
        assert (out[6] == 0).all() and (out[5] == -np.inf).all() and (out[1] == 0).all() and (out[3] == 0).all() and (out[0] == -1).all()


def test_a_sequence_alone_equals_itself_in_the_batch_and_runs_repeat():
    em, em_len, packed, want, _, _, _, _ = main_reference(1.0)
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


def _hip():
    """The HIP runtime already in the process (torch's), for the capture calls torch does not expose."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


def test_one_launch_whatever_the_batch_and_capturable():
    """The call is captured into a graph (never replayed): it enqueues the same number of nodes -- one kernel -- for 1 and for 384
    sequences, allocates nothing and synchronises nothing."""
    hip, lib = _hip(), capi.load()
    spellings, V, sil, words = lexicon("prefix")
    packed_trie = tries("prefix")[1]
    packed = models("prefix", 2)[1]
    dev = torch.device("cuda", torch.cuda.current_device())
    counts = {}
    for n in (1, 384):
        em = torch.from_numpy(L.emissions(n, spellings, n, 16, V)).cuda()
        trie_image, lm_image, bufs = packed_trie.on(dev), packed.on(dev), raw_buffers(lib, em, 10, 2)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph, n_nodes = C.c_void_p(), C.c_size_t(0)
        assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0  # relaxed mode: other threads are not affected
        rc = raw_call(lib, em, trie_image, lm_image, 10, 2, bufs, stream=side.cuda_stream)
        assert hip.hipStreamEndCapture(side.cuda_stream, C.byref(graph)) == 0
        assert rc == 0, lib.eec_last_error()
        assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
        hip.hipGraphDestroy(graph)
        counts[n] = n_nodes.value
    assert counts[1] == counts[384] == 1, counts


# ----------------------------------------------------------------------------------------------------------------------------
# BeamInference
# ----------------------------------------------------------------------------------------------------------------------------
def test_beam_inference_with_a_model():
    """The transcripts are the statement's at LM_WEIGHT and at a given lm_weight, pprob is the softmax of the statement's final
    scores (a float64 softmax of identical fp32 inputs: 1e-6 covers its rounding); a path given as args.lm is read at the first
    use; without a model nothing changes."""
    em, _, packed, _, _, _, words, lm = main_reference(1.0)
    ref, packed_trie = tries("fixture+sil")
    em = em[40:56]  # full-length sequences
    want = {wt: M.decode_batch(em, ref, beam=10, nbest=4, lm=lm, lm_weight=wt, lm_words=words) for wt in (1.0, 3.23)}
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

    free = L.decode_batch(em, ref, beam=10, nbest=4)
    plain, none = BeamInference(Args(), trie=packed_trie), BeamInference(Args(), trie=packed_trie, lm=None)
    assert plain.ctc_predict_(dev, nbest=4) == none.ctc_predict_(dev, nbest=4) == [text(h) for h in free]
    assert plain.ctc_predict_(dev, nbest=4, lm_weight=3.23) == [text(h) for h in free]  # no model: the weight has nothing to weigh
    for b in (0, 1, 2):
        a, c = plain.ctc_predict(dev[b:b + 1], nbest=4), none.ctc_predict(dev[b:b + 1], nbest=4)
        assert a[0] == c[0] and float(a[1]) == float(c[1])
