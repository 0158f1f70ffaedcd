"""CPU tests of the LM look-ahead's host side (max trie smearing: ``eec_ctc_trie_smear`` in csrc/ctc_lexbeam.hip,
``NGramLM.smear``): the packed table against the plain-Python statement of tests/lexbeam_smear_cases.py bit for bit, every refusal
of the host entry and of the decoder entry (all decided before any device work), and the statement itself: without a table it is
the unsmeared statement (tests/lexbeam_statement.py), with one it prunes differently (the {ab, cd} case) and -- where nothing is pruned -- returns the
same complete hypotheses with the same score bits (the payments telescope)."""
import numpy as np
import pytest
import torch

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_smear_cases as S
import lexbeam_statement as D
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie
from lexbeam_helpers import library, same_hyps

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    return library()


def lexicon(name):
    """(spellings, V, sil, words); this module's ``fixture`` is the fixture lexicon with sil"""
    return L.lexicon("fixture+sil" if name == "fixture" else name)


def packed_pair(tmp_path, spellings, V, sil, words, lm):
    trie = TokenTrie.from_spellings(spellings, V, blank=0, sil=sil, words=words)
    path = tmp_path / "model.arpa"
    M.write_arpa(path, lm)
    return trie, NGramLM.from_arpa(str(path), trie)


# ---------------------------------------------------------------------------------------------------------------------------
# the statement without a table
# ---------------------------------------------------------------------------------------------------------------------------
def test_without_a_table_the_statement_is_the_unsmeared_one():
    em, em_len, spellings, words, lm = M.main_lm_case()
    trie = L.Trie(spellings, 256, 0, 126)
    kw = dict(beam=10, nbest=10, lm=lm, lm_weight=1.0, lm_words=words)
    mine, theirs = D.decode_batch(em, trie, em_len, smax=None, **kw), D.decode_batch(em, trie, em_len, **kw)
    assert len(mine) == len(theirs) == 70 and sum(1 for h in mine if h) >= 10
    same_hyps(mine, theirs)


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
TABLES = [("fixture", 1, {}), ("fixture", 2, {}), ("fixture", 3, {}), ("fixture", 4, {}), ("fixture", 3, dict(bos=False, eos=False)),
          ("fixture", 3, dict(leave_out=0.5)), ("prefix", 2, {}), ("wide", 2, {})]


@pytest.mark.parametrize("name,order,variant", TABLES, ids=[f"{n}-o{o}{''.join('-' + k for k in v)}" for n, o, v in TABLES])
def test_the_packed_table_is_the_statements_bit_for_bit(lib, tmp_path, name, order, variant):
    """Orders 1 to 4, with and without <s>, a model that maps half of the lexicon to <unk>, words that are prefixes of words and a
    shadowed duplicate (``prefix``), nodes with more than 64 children (``wide``).  The statement's table is also checked against a
    maximum over the words taken without any trie."""
    spellings, V, sil, words = lexicon(name)
    lm, _, _ = M.random_model(60 + order, words, order, **variant)
    trie, packed = packed_pair(tmp_path, spellings, V, sil, words, lm)
    ref = L.Trie(spellings, V, 0, sil)
    smax = S.smear(ref, lm, words)
    brute = S.brute_force_smear(spellings, lm, words)
    assert {sp: M.bits(smax[n]) for n, sp in enumerate(S.statement_spellings(ref)) if n} == {sp: M.bits(v) for sp, v in brute.items()}

    image = trie._image.numpy().view(np.int32)
    table = packed.smear(trie)
    assert packed.smear(trie) is table, "built once per trie"
    n_nodes, n_words, got = S.read_smear_table(table._image.numpy().view(np.int32))
    assert n_nodes == trie.n_nodes == ref.n_nodes and n_words == len(words)
    assert table._image.numel() == lib.eec_ctc_trie_smear_bytes(n_nodes) and table._image.numel() % 8 == 0
    want = S.table_in_image_order(ref, smax, image)
    assert got == want
    assert got[0] == 0 and want[0] == M.bits(0.0), "smax[0] = +0.0 is stored"
    assert table.values.view(np.int32).tolist() == want and np.isfinite(table.values).all()
    unk = sum(1 for w in words if (w,) not in lm)
    if "leave_out" in variant:
        assert unk > 0.3 * len(words), "the case maps lexicon words to <unk>"
    if name == "prefix":
        assert trie.n_shadowed == 1 and any(ref.word[n] >= 0 and ref.kids[n] for n in range(ref.n_nodes))
    assert len(set(got[1:])) > 1, "the table is not flat"


def test_a_parent_carries_the_maximum_of_its_words_and_a_shadowed_duplicate_does_not_count(tmp_path):
    """{a: -3, ab: -1, ac: -2, second 'a' spelling (shadowed): -0.5}: the node of a carries -1, not the duplicate's -0.5."""
    spellings, words = [[1], [1, 2], [1, 3], [1]], ["a", "ab", "ac", "dup"]
    lm = {("a",): (L.F32(-3.0), L.F32(0.0)), ("ab",): (L.F32(-1.0), L.F32(0.0)), ("ac",): (L.F32(-2.0), L.F32(0.0)), ("dup",): (L.F32(-0.5), L.F32(0.0))}
    trie, packed = packed_pair(tmp_path, spellings, 8, None, words, lm)
    assert trie.n_shadowed == 1
    sp = S.image_spellings(trie._image.numpy().view(np.int32))
    by_spelling = dict(zip(sp, packed.smear(trie).values.tolist()))
    assert by_spelling == {(): 0.0, (1,): -1.0, (1, 2): -1.0, (1, 3): -2.0}


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_size_function_and_every_refusal_of_the_host_entry(lib, tmp_path):
    assert lib.eec_ctc_trie_smear_bytes(0) == 0 and lib.eec_ctc_trie_smear_bytes(-3) == 0
    assert [lib.eec_ctc_trie_smear_bytes(n) for n in (1, 2, 3, 4, 5)] == [24, 24, 32, 32, 40]  # 16 header bytes, 4 per node, 8-byte granules
    spellings, V, sil, words = lexicon("prefix")
    lm, _, _ = M.random_model(61, words, 2)
    trie, packed = packed_pair(tmp_path, spellings, V, sil, words, lm)
    t, m = trie._image, packed._image
    need = lib.eec_ctc_trie_smear_bytes(trie.n_nodes)
    buf = np.full(need // 4 + 2, 0x5A5A5A5A, dtype=np.int32)
    call = lambda tp, mp, bp, nb: lib.eec_ctc_trie_smear(tp, mp, bp, nb)  # noqa: E731
    assert call(t.data_ptr(), m.data_ptr(), buf.ctypes.data, need) == 0
    assert buf[need // 4:].tolist() == [0x5A5A5A5A] * 2, "nothing is written past the stated size"
    assert S.read_smear_table(buf[:need // 4])[0] == trie.n_nodes
    for args, what in (((None, m.data_ptr(), buf.ctypes.data, need), "null argument"),
                       ((t.data_ptr(), None, buf.ctypes.data, need), "null argument"),
                       ((t.data_ptr(), m.data_ptr(), None, need), "null argument"),
                       ((t.data_ptr(), m.data_ptr(), buf.ctypes.data + 4, need), "8-byte aligned"),
                       ((m.data_ptr(), m.data_ptr(), buf.ctypes.data, need), "no packed trie"),
                       ((t.data_ptr(), t.data_ptr(), buf.ctypes.data, need), "no packed n-gram model")):
        assert call(*args) == BAD_ARG and what in lib.eec_last_error().decode(), (what, lib.eec_last_error())
    assert call(t.data_ptr(), m.data_ptr(), buf.ctypes.data, need - 1) == WORKSPACE
    assert "eec_ctc_trie_smear_bytes" in lib.eec_last_error().decode()
    assert call(t.data_ptr(), m.data_ptr(), buf.ctypes.data, 0) == WORKSPACE

    # a model packed for another lexicon: lm[5] != trie[10]
    shorter = TokenTrie.from_spellings(spellings[:-1], V, blank=0, words=words[:-1])
    assert call(shorter._image.data_ptr(), m.data_ptr(), buf.ctypes.data, need) == BAD_ARG
    assert "packed for a lexicon of 8 words, the trie has 7" in lib.eec_last_error().decode()
    with pytest.raises(ValueError, match="packed for a lexicon of 8 words, the trie has 7"):
        packed.smear(shorter)
    altered = m.clone()
    altered.view(torch.int32)[5] = 7
    assert call(t.data_ptr(), altered.data_ptr(), buf.ctypes.data, need) == BAD_ARG


def test_the_decoder_entry_refuses_a_null_or_misaligned_table_before_any_device_work(lib):
    """No device is needed: the checks come first.  Every pointer is a host address that is never dereferenced."""
    keep = np.zeros(64, dtype=np.int64)
    p = keep.ctypes.data
    args = [p, 1, 4, 8, None, p, 0, -1, 2, 1, 0.0, 0.0, 50.0, 4, p, p, p, p, p, p, p, p, 1 << 20, None, p, 1.0]
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*args, None) == BAD_ARG and "null argument (smear)" in lib.eec_last_error().decode()
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*args, p + 4) == BAD_ARG and "smear must be 8-byte aligned" in lib.eec_last_error().decode()
    no_lm = args[:-2] + [None, 1.0]
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*no_lm, p) == BAD_ARG and "null argument (lm)" in lib.eec_last_error().decode()
    bad_weight = args[:-1] + [float("nan")]
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*bad_weight, p) == BAD_ARG
    wide_beam = list(args)
    wide_beam[8] = 17
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*wide_beam, p) == UNSUPPORTED
    small_ws = list(args)
    small_ws[22] = 8
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*small_ws, p) == WORKSPACE
    empty = list(args)
    empty[1] = 0
    assert lib.eec_ctc_lexbeam_lm_smear_decode(*empty, p) == 0  # n_seq == 0: a successful no-op


def test_smearing_without_a_model_is_a_value_error_in_python():
    from early_exit_transformer_amd.beam import BeamInference
    from early_exit_transformer_amd.model import ctc_lexicon_decode
    trie = TokenTrie.from_spellings(L.ONE_WORD, 40)
    with pytest.raises(ValueError, match="needs lm="):  # decided before the device is looked at
        ctc_lexicon_decode(torch.zeros((1, 2, 40)), trie, smearing="max")
    with pytest.raises(ValueError, match="None or 'max'"):
        ctc_lexicon_decode(torch.zeros((1, 2, 40)), trie, smearing="min")
    with pytest.raises(ValueError, match="None or 'max'"):
        BeamInference(None, smearing="sum")

    class Args:
        lm_smearing = "max"
    assert BeamInference(Args())._smearing == "max" and BeamInference(None)._smearing is None


# ---------------------------------------------------------------------------------------------------------------------------
# pruning: the model guides the search inside words
# ---------------------------------------------------------------------------------------------------------------------------
def test_at_beam_1_smearing_keeps_the_word_the_model_prefers():
    spellings, words, lm, em = S.pruning_case()
    trie = L.Trie(spellings, S.PRUNE_V, 0, None)
    kw = dict(beam=1, nbest=1, lm=lm, lm_weight=1.0, lm_words=words)
    plain = D.decode(em, trie, **kw)
    assert [(h[0], h[1], h[2], float(h[3])) for h in plain] == [([1], [S.C_, S.D], [0, 1], -6.875)]
    smax = S.smear(trie, lm, words)
    assert [float(v) for v in smax] == [0.0, -1.0, -1.0, -5.0, -5.0]
    smeared = D.decode(em, trie, smax=smax, **kw)
    assert [(h[0], h[1], h[2], float(h[3])) for h in smeared] == [([0], [S.A, S.B_], [0, 1], -3.0)]


def test_an_in_word_and_a_word_end_candidate_that_tie_are_decided_by_the_id():
    """With abd below ab both candidates of b score -3.0; the in-word one has the lower id (w = 0), takes the single slot, and the
    sequence ends inside a word: no hypothesis.  At beam 2 both stay and ab is returned."""
    spellings, words, lm, em = S.pruning_case(extra_abd=True)
    trie = L.Trie(spellings, S.PRUNE_V, 0, None)
    smax = S.smear(trie, lm, words)
    kw = dict(lm=lm, lm_weight=1.0, lm_words=words, smax=smax)
    assert D.decode(em, trie, beam=1, nbest=1, **kw) == []
    two = D.decode(em, trie, beam=2, nbest=2, **kw)
    assert [(h[0], float(h[3])) for h in two] == [([0], -3.0)]
    assert D.decode(em, trie, beam=1, nbest=1, lm=lm, lm_weight=1.0, lm_words=words) != []  # unsmeared: cd, as before


# ---------------------------------------------------------------------------------------------------------------------------
# telescoping: where nothing is pruned, smearing changes nothing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2])
def test_where_nothing_is_pruned_the_payments_telescope(T):
    """Dyadic emissions, model values and weight (every sum is exact), no threshold, beam 16 and shapes at which no frame has more
    than 16 candidates -- asserted, not assumed: smeared and unsmeared return the same set of (words, tokens, timesteps, score
    bits).  Ranks, and with them ids, may differ, so the lists are compared as sets."""
    for seed in range(50):
        spellings, words, lm, em = S.telescoping_case(seed, T)
        trie = L.Trie(spellings, S.PRUNE_V, 0, None)
        smax = S.smear(trie, lm, words)
        kw = dict(beam=16, nbest=16, beam_threshold=INF, lm=lm, lm_weight=2.0, lm_words=words)
        s_plain, s_smear = {}, {}
        plain = D.decode(em[0], trie, stats=s_plain, **kw)
        smeared = D.decode(em[0], trie, stats=s_smear, smax=smax, **kw)
        assert s_plain["max_candidates"] <= 16 and s_smear["max_candidates"] <= 16
        assert plain and S.as_set(plain) == S.as_set(smeared) and len(S.as_set(plain)) == len(plain)


def test_three_frames_pass_the_beam_and_the_count_shows_it():
    """At T' = 3 the same lexicon has more than 16 candidates in a frame: the condition of the telescoping test is a real one."""
    spellings, words, lm, em = S.telescoping_case(0, 3)
    trie = L.Trie(spellings, S.PRUNE_V, 0, None)
    stats = {}
    D.decode(em[0], trie, beam=16, nbest=16, beam_threshold=INF, lm=lm, lm_weight=2.0, lm_words=words, stats=stats, smax=S.smear(trie, lm, words))
    assert stats["max_candidates"] > 16
