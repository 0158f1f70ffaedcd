"""The scaffolding the lexicon beam search tests share (tests/test_gpu_lexbeam*.py and the host modules next to them): the library,
lexica with their two tries, generated models packed the whole way (dict, ARPA text, ``NGramLM.from_arpa``), the device call and
its comparison against the statement's hypothesis lists (tests/lexbeam_statement.py), the bare C entries on buffers that exist
already, a graph capture that counts nodes, and the LM suite's main case, which two modules decode."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import torch

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_statement as D
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.build import LIB_PATH
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie
from early_exit_transformer_amd.model import ctc_lexicon_decode

lexicon = L.lexicon
_TMP = tempfile.TemporaryDirectory(prefix="eec_lm_")


def library():
    """The body of every module's ``lib`` fixture."""
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


# ----------------------------------------------------------------------------------------------------------------------------
# lexica and models
# ----------------------------------------------------------------------------------------------------------------------------
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


# ----------------------------------------------------------------------------------------------------------------------------
# the device call and its judges
# ----------------------------------------------------------------------------------------------------------------------------
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


def identical(a, b):
    """Two calls' outputs: as many arrays, each of the same shape and type, byte for byte."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def same_hyps(got, want):
    """Two batches of hypothesis lists: words, tokens, timesteps equal, scores equal as bit patterns."""
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), s
        for j, (x, y) in enumerate(zip(g, w)):
            assert x[:3] == y[:3], (s, j)
            assert M.bits(x[3]) == M.bits(y[3]), (s, j, x[3], y[3])


# ----------------------------------------------------------------------------------------------------------------------------
# the bare C entries
# ----------------------------------------------------------------------------------------------------------------------------
def raw_buffers(lib, em, beam, nbest):
    """(words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace) on the emission's device"""
    n, T, V = em.shape
    dev = em.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    sc = torch.empty((n, nbest), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.eec_ctc_lexbeam_workspace_bytes(n, T, beam), dtype=torch.uint8, device=dev)
    return i32(n, nbest, T), i32(n, nbest), i32(n, nbest, T), i32(n, nbest), i32(n, nbest, T), sc, i32(n), ws


def raw_call(lib, entry, em, trie_image, beam, nbest, bufs, *more, stream=None, ws_bytes=None):
    """The bare C entry ``entry`` on device buffers that exist already: the return code.  ``more``: what the entry takes after the
    stream -- the model's address, lm_weight, the smear table's address, log_add --, as far as its signature goes."""
    n, T, V = em.shape
    words, wc, toks, tc, ts, sc, nh, ws = bufs
    return getattr(lib, entry)(em.data_ptr(), n, T, V, None, trie_image.data_ptr(), 0, -1, beam, nbest, 0.0, 0.0, 50.0, T, words.data_ptr(),
                               wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(), nh.data_ptr(), ws.data_ptr(),
                               ws.numel() if ws_bytes is None else ws_bytes, capi.stream_ptr(em.device) if stream is None else stream, *more)


def _hip():
    """The HIP runtime already in the process (torch's), for the capture calls torch does not expose."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


def captured_nodes(lib, call):
    """``call(stream)`` -- a bare C entry; its return code must be 0 -- captured into a graph on a side stream (never replayed): the
    number of nodes it enqueued."""
    hip = _hip()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph, n_nodes = C.c_void_p(), C.c_size_t(0)
    assert hip.hipStreamBeginCapture(side.cuda_stream, 2) == 0  # relaxed mode: other threads are not affected
    rc = call(side.cuda_stream)
    assert hip.hipStreamEndCapture(side.cuda_stream, C.byref(graph)) == 0
    assert rc == 0, lib.eec_last_error()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph)
    return n_nodes.value


# ----------------------------------------------------------------------------------------------------------------------------
# the LM suite's main case, decoded once for tests/test_gpu_lexbeam_lm.py and tests/test_gpu_lexbeam_smear.py
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_lm_reference(lm_weight):
    """(emission, em_len, packed model, the statement's hypotheses, its stats, the model-free statement's hypotheses, words, model)"""
    em, em_len, spellings, words, lm = M.main_lm_case()
    ref, packed_trie = tries("fixture+sil")
    packed = NGramLM.from_arpa(arpa_path(lm, "main"), packed_trie)
    stats = {}
    want = D.decode_batch(em, ref, em_len, beam=10, nbest=10, lm=lm, lm_weight=lm_weight, lm_words=words, stats=stats)
    return em, em_len, packed, want, stats, main_lm_free(), words, lm


@functools.lru_cache(maxsize=None)
def main_lm_free():
    em, em_len, spellings, _, _ = M.main_lm_case()
    return D.decode_batch(em, tries("fixture+sil")[0], em_len, beam=10, nbest=10)
