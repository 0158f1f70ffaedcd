"""GPU tests of log-add merging in the lexicon-constrained CTC beam search (csrc/ctc_lexbeam.hip, eec_ctc_lexbeam_logadd_decode,
``ctc_lexicon_decode(log_add=True)``, ``BeamInference.beam_predict``) against the plain-Python statement of
tests/lexbeam_statement.py (``log_add=True``).  ``log_add`` is a stated sequence of exactly rounded fp32 operations, so, as in
tests/test_gpu_lexbeam.py, there is nothing to tolerate: n_hyp, words, tokens, timesteps and counts are compared as integers and
scores as bit patterns.  Lexica, models and helpers are those of tests/lexbeam_helpers.py."""
import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_logadd_cases as A
import lexbeam_lm_cases as M
import lexbeam_smear_cases as S
import lexbeam_statement as D
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import ctc_lexicon_decode
from lexbeam_helpers import lexicon, models, raw_buffers, raw_call, run, same, tries

pytestmark = pytest.mark.gpu
INF = float("inf")
BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


# ----------------------------------------------------------------------------------------------------------------------------
# without a model
# ----------------------------------------------------------------------------------------------------------------------------
CASES = [
    # lexicon, n_seq, T', beam, nbest, options
    ("prefix", 70, 16, 10, 10, dict()),
    ("fixture+sil", 12, 64, 10, 10, dict()),
    ("wide", 3, 32, 16, 16, dict()),
    ("one", 4, 8, 16, 16, dict(beam_threshold=INF)),
    ("fixture", 3, 257, 16, 1, dict(word_score=-4.0)),
    ("fixture+sil", 70, 7, 2, 1, dict(beam_threshold=2.0)),
    ("one", 1, 1, 1, 1, dict()),
]


@pytest.mark.parametrize("name,n,T,beam,nbest,opts", CASES, ids=[f"{c[0]}-n{c[1]}-T{c[2]}-b{c[3]}-k{c[4]}" for c in CASES])
def test_model_free_log_add_equals_the_statement(name, n, T, beam, nbest, opts):
    """Ragged lengths with 0, 1, T' and T' + 1 where there are 70 sequences; child ranges over 64 (wide); a beam that never prunes
    (one); odd T' at word_score -4, the beam_predict setting; a finite threshold acting on merged scores; one frame, beam 1.  Every
    case of more than one frame must fold at least one pair in the statement, or it says nothing about the merge."""
    spellings, V, sil, _ = lexicon(name)
    ref, packed = tries(name)
    em = L.emissions(5, spellings, n, T, V, 0, -1 if sil is None else sil)
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)
        em_len[:4] = [0, 1, T, T + 1]
    stats = {}
    want = D.decode_batch(em, ref, em_len, beam=beam, nbest=nbest, log_add=True, stats=stats, **opts)
    assert T == 1 or stats.get("merges", 0) > 0
    nh = same(run(em, packed, em_len, beam_size=beam, nbest=nbest, log_add=True, **opts), want, nbest)
    assert T < 8 or (nh > 0).any(), "the case decodes something"


def test_ties_inside_merges_keep_the_lower_id_and_add_ln_2():
    """Log-probs on a grid of 0.25 with a block of uniform frames: equal raw scores inside merges (d = 0), counted in the statement."""
    spellings, V, sil, _ = lexicon("prefix")
    ref, packed = tries("prefix")
    em = L.tie_emissions(7, spellings, 70, 16, V)
    stats = {}
    want = D.decode_batch(em, ref, beam=10, nbest=10, beam_threshold=INF, log_add=True, stats=stats)
    assert stats.get("equal_merges", 0) >= 1
    nh = same(run(em, packed, beam_size=10, nbest=10, beam_threshold=INF, log_add=True), want, 10)
    assert (nh > 0).sum() > 35


# ----------------------------------------------------------------------------------------------------------------------------
# with the model, and with the model and smearing
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smearing", [None, "max"])
@pytest.mark.parametrize("name,order,n,T,lm_weight", [("fixture+sil", 3, 3, 32, 1.0), ("fixture+sil", 3, 3, 32, 3.23), ("prefix", 2, 70, 16, 1.0),
                                                      ("prefix", 2, 70, 16, 3.23)])
def test_log_add_with_the_model_and_with_smearing_equals_the_statement(name, order, n, T, lm_weight, smearing):
    spellings, V, sil, words = lexicon(name)
    ref, packed_trie = tries(name)
    lm, packed, favoured, disfavoured = models(name, order)
    em = M.lm_emissions(300 + n + T, favoured, disfavoured, words, spellings, n, T, V, 0, -1 if sil is None else sil, peaks=(4.0, 8.0, 6.0))
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)
        em_len[:4] = [1, T, 0, T + 1]
    smax = None if smearing is None else S.smear(ref, lm, words)
    stats = {}
    want = D.decode_batch(em, ref, em_len, beam=10, nbest=10, lm=lm, lm_weight=lm_weight, lm_words=words, smax=smax, log_add=True, stats=stats)
    assert stats.get("merges", 0) > 0
    nh = same(run(em, packed_trie, em_len, beam_size=10, nbest=10, lm=packed, lm_weight=lm_weight, smearing=smearing, log_add=True), want, 10)
    assert (nh > 0).any(), "the case decodes something"


# ----------------------------------------------------------------------------------------------------------------------------
# the function itself on the device
# ----------------------------------------------------------------------------------------------------------------------------
def test_device_log_add_equals_the_host_function_bit_for_bit():
    lib = capi.load()
    a, b = A.pair_grid()
    host = np.array([lib.eec_ctc_log_add_host(x, y) for x, y in zip(a.tolist(), b.tolist())], dtype=np.float32)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full_like(da, float("nan"))
    capi.check(lib.eec_ctc_log_add(da.data_ptr(), db.data_ptr(), out.data_ptr(), len(a), capi.stream_ptr(da.device)), "eec_ctc_log_add")
    got = out.cpu().numpy()
    wrong = np.flatnonzero(A.bits(got) != A.bits(host))
    assert wrong.size == 0, (wrong[:5], a[wrong[:5]], b[wrong[:5]], got[wrong[:5]], host[wrong[:5]])
    assert np.array_equal(A.bits(host), A.bits(A.log_add(a, b)))
    assert lib.eec_ctc_log_add(None, None, None, 0, None) == 0 and lib.eec_ctc_log_add(None, db.data_ptr(), out.data_ptr(), 4, None) == BAD_ARG


# ----------------------------------------------------------------------------------------------------------------------------
# the entry
# ----------------------------------------------------------------------------------------------------------------------------
def test_with_log_add_off_the_viterbi_entry_is_called_and_its_bits_come_back():
    lib = capi.load()
    spellings, V, _, _ = lexicon("prefix")
    packed = tries("prefix")[1]
    em = torch.from_numpy(L.emissions(5, spellings, 24, 16, V)).cuda()
    bufs = raw_buffers(lib, em, 10, 10)
    assert raw_call(lib, "eec_ctc_lexbeam_decode", em, packed.on(em.device), 10, 10, bufs) == 0
    got = ctc_lexicon_decode(em, packed, beam_size=10, nbest=10, log_add=False)
    for x, y in zip(got, bufs[:7]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    added = ctc_lexicon_decode(em, packed, beam_size=10, nbest=10, log_add=True)
    assert added[5].cpu().numpy().tobytes() != got[5].cpu().numpy().tobytes()


def test_the_log_add_launch_replays_from_a_graph():
    """Captured with torch.cuda.graph, replayed twice over wiped outputs: identical outputs, the statement's."""
    spellings, V, _, _ = lexicon("prefix")
    ref, packed = tries("prefix")
    em_host = L.emissions(5, spellings, 24, 16, V)
    em = torch.from_numpy(em_host).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the image is uploaded and the allocator is warm before the capture
        ctc_lexicon_decode(em, packed, beam_size=10, nbest=10, log_add=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ctc_lexicon_decode(em, packed, beam_size=10, nbest=10, log_add=True)
    runs = []
    for _ in range(2):
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        runs.append([o.cpu().numpy().copy() for o in out])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*runs))
    same(runs[1], D.decode_batch(em_host, ref, beam=10, nbest=10, log_add=True), 10)


def test_argument_errors_come_before_any_device_work():
    lib = capi.load()
    spellings, V, _, words = lexicon("prefix")
    packed_trie = tries("prefix")[1]
    packed = models("prefix", 2)[1]
    em = torch.from_numpy(L.emissions(5, spellings, 3, 16, V)).cuda()
    dev = em.device
    entry = "eec_ctc_lexbeam_logadd_decode"
    bufs = raw_buffers(lib, em, 16, 1)
    for b in bufs[:7]:
        b.fill_(-7)
    torch.cuda.synchronize()
    smear = packed.smear(packed_trie).on(dev)
    assert raw_call(lib, entry, em, packed_trie.on(dev), 10, 1, bufs, None, 1.0, smear.data_ptr()) == BAD_ARG
    assert b"smear without lm" in lib.eec_last_error()
    assert raw_call(lib, entry, em, packed_trie.on(dev), 17, 1, bufs, None, 0.0, None) == UNSUPPORTED
    assert raw_call(lib, entry, em, packed_trie.on(dev), 16, 1, bufs, None, 0.0, None, ws_bytes=bufs[7].numel() - 8) == WORKSPACE
    assert raw_call(lib, entry, em, packed_trie.on(dev), 10, 1, bufs, packed.on(dev).data_ptr(), float("nan"), None) == BAD_ARG
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs[:7]), "nothing was written"
    assert raw_call(lib, entry, em, packed_trie.on(dev), 16, 1, bufs, None, 0.0, None) == 0
    torch.cuda.synchronize()
    assert bool((bufs[6] >= 0).all())


# ----------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------------------------------------------
CHAR_TOKENS = ["-", "|"] + list("abcdefgh")
CHAR_WORDS = ["a", "ab", "abba", "bad", "add", "dab", "cab", "bead", "fad", "egg", "he", "had"]


def test_beam_predict_is_the_character_lexicon_decoder(tmp_path):
    """A stub model whose ``ctc_encoder`` returns a fixed emission; tokens ``-``, ``|``, letters; the lexicon and token files on disk.
    ``beam_predict`` returns the statement's transcript at word_score -4 with log-add merging, beam ``args.beam_size``, sil ``|``."""
    ids = {t: i for i, t in enumerate(CHAR_TOKENS)}
    spellings = [[ids[ch] for ch in w] for w in CHAR_WORDS]
    (tmp_path / "tokens.txt").write_text("\n".join(CHAR_TOKENS) + "\n", encoding="utf-8")
    (tmp_path / "lexicon.txt").write_text("".join(f"{w}\t{' '.join(w)}\n" for w in CHAR_WORDS), encoding="utf-8")
    V = len(CHAR_TOKENS)
    em = L.emissions(17, spellings, 2, 48, V, 0, 1, peaks=(3.0, 3.0))
    ref = L.Trie(spellings, V, 0, 1)
    want = D.decode(em[0], ref, beam=8, nbest=1, word_score=-4.0, log_add=True)
    text = " ".join(CHAR_WORDS[w] for w in want[0][0]).strip()
    assert want and len(want[0][0]) >= 2

    class Args:
        beam_size = 8
        lexicon = str(tmp_path / "lexicon.txt")
        tokens = str(tmp_path / "tokens.txt")

    class Model:
        def ctc_encoder(self, x):
            return x

    infer = BeamInference(Args())
    dev_em = torch.from_numpy(em).cuda()
    assert infer.beam_predict(Model(), dev_em) == text
    assert infer.beam_predict(Model(), dev_em[1:]) == " ".join(CHAR_WORDS[w] for w in D.decode(em[1], ref, beam=8, nbest=1, word_score=-4.0, log_add=True)[0][0])
    assert BeamInference.WORD_SCORE == -4 and infer._trie is None, "the character trie is kept apart from the BPE trie"


def test_ctc_predict_with_log_add_returns_the_statements_transcripts():
    spellings, V, _, words = lexicon("prefix")
    ref, packed = tries("prefix")
    em = L.emissions(5, spellings, 24, 16, V)
    text = lambda hyps: " ".join(words[w] for w in hyps[0][0]).strip() if hyps else ""  # noqa: E731
    added = [text(h) for h in D.decode_batch(em, ref, beam=10, log_add=True)]
    viterbi = [text(h) for h in D.decode_batch(em, ref, beam=10)]
    assert sum(a != v for a, v in zip(added, viterbi)) >= 4

    class Args:
        beam_size = 10

    class ArgsOn(Args):
        lm_log_add = True
    dev_em = torch.from_numpy(em).cuda()
    assert BeamInference(Args(), trie=packed, log_add=True).ctc_predict_(dev_em) == added
    assert BeamInference(ArgsOn(), trie=packed).ctc_predict_(dev_em) == added
    assert BeamInference(ArgsOn(), trie=packed, log_add=False).ctc_predict_(dev_em) == viterbi
    assert BeamInference(Args(), trie=packed).ctc_predict_(dev_em) == viterbi
    assert BeamInference(Args(), trie=packed, log_add=True).ctc_predict(dev_em)[0] == [added[0]]
