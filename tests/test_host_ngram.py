"""CPU tests of the n-gram language model's host side (``lexicon.NGramLM``, ``eec_ngram_pack`` in csrc/ctc_lexbeam.hip): generated
models written as ARPA text, read back and packed, against a reader of the documented image layout; the plain-Python statement of
the search with a model (tests/lexbeam_statement.py, tests/lexbeam_lm_cases.py) against the model-free one and against a textbook back-off in float64;
and every refusal of the reader, the packer and the decoder entry, all decided before any device work."""
import ctypes as C

import numpy as np
import pytest

import lexbeam_cases as L
import lexbeam_lm_cases as M
import lexbeam_statement as D
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie
from lexbeam_helpers import library, same_hyps

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


@pytest.fixture(scope="module")
def lib():
    return library()


@pytest.fixture(scope="module")
def fixture_trie(lib):
    _, words, spellings = L.load_fixture()
    return words, spellings, TokenTrie.from_spellings(spellings, 256, blank=0, sil=126, words=words)


# ---------------------------------------------------------------------------------------------------------------------------
# round trip: generated model -> ARPA text -> NGramLM.from_arpa -> packed image -> the layout reader
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,variant", [(1, {}), (2, {}), (3, {}), (5, {}), (3, dict(grid=True)), (4, dict(positive_backoff=True)),
                                           (3, dict(bos=False, eos=False))],
                         ids=["1", "2", "3", "5", "3-grid", "4-positive-backoff", "3-no-bos-eos"])
def test_a_generated_model_survives_arpa_text_and_packing(fixture_trie, tmp_path, order, variant):
    """The image holds exactly the generated n-grams with their log-probs and back-offs as fp32 bit patterns; every suffix link
    is the longest present suffix (the reader checks that; here: some skip an order); absent lexicon words map to <unk>."""
    words, _, trie = fixture_trie
    lm, _, _ = M.random_model(40 + order, words, order, **variant)
    path = tmp_path / "model.arpa"
    M.write_arpa(path, lm)
    packed = NGramLM.from_arpa(str(path), trie)
    assert packed.order == order and packed.n_words == len(words)
    assert packed.n_grams == [sum(1 for g in lm if len(g) == n) for n in range(1, order + 1)]
    head, grams, links, word_map = M.read_lm_image(packed._image.numpy().view(np.int32))
    ids = {w: i for i, w in enumerate(packed.vocab)}
    assert {g: v[1:] for g, v in grams.items()} == {tuple(ids[w] for w in g): (M.bits(lp), M.bits(bo)) for g, (lp, bo) in lm.items()}
    assert head["order"] == order and head["lex_words"] == len(words) and head["n_nodes"] == 1 + len(lm) == packed.n_nodes
    assert head["bos_node"] == (ids[M.BOS] + 1 if (M.BOS,) in lm else 0) and head["eos_word"] == ids.get(M.EOS, -1)
    absent = [w for w in words if (w,) not in lm]
    assert 0.05 * len(words) < len(absent) < 0.2 * len(words)
    assert all(word_map[i] == ids[w if (w,) in lm else M.UNK] for i, w in enumerate(words))
    degree = {}
    for g in grams:
        if len(g) == 2:
            degree[g[0]] = degree.get(g[0], 0) + 1
    if order >= 2:
        assert max(degree.values()) > 256 and {1, 2} <= set(degree.values())
    if order >= 3:
        assert sum(1 for g, to in links.items() if len(to) < len(g) - 1) > len(links) // 10, "suffix links that skip an order"
        assert any(len(to) == len(g) - 1 for g, to in links.items() if len(g) >= 3), "... and some that do not"


def test_lexicon_entries_with_one_string_share_an_lm_word_and_normalize_is_applied(lib, tmp_path):
    trie = TokenTrie.from_spellings([[1], [2], [1, 2], [3]], 8, words=["a", "b", "a", "c"])
    path = tmp_path / "m.arpa"
    path.write_text("\\data\\\nngram 1=4\nngram 2=2\n\n\\1-grams:\n-1.5\tA\t-0.25\n-2\tB\n-3 <unk> -0.5\n-1 ZZZ -1\n\n\\2-grams:\n-0.5 A B\n-0.75 A ZZZ\n\n\\end\\\n")
    lm = NGramLM.from_arpa(str(path), trie, normalize=str.lower)
    assert lm.vocab == ["a", "b", "<unk>"] and lm.word_map.tolist() == [0, 1, 0, 2] and lm.n_grams == [3, 1] and (lm.bos, lm.eos, lm.unk) == (-1, -1, 2)
    head, grams, _, _ = M.read_lm_image(lm._image.numpy().view(np.int32))
    assert grams[(0, 1)][1:] == (M.bits(-0.5), M.bits(0.0)) and grams[(1,)][1:] == (M.bits(-2.0), M.bits(0.0)) and head["bos_node"] == 0
    exact = NGramLM.from_arpa(str(path), trie)  # the match is exact: without normalize every lexicon word is <unk>
    assert exact.vocab == ["<unk>"] and exact.word_map.tolist() == [0, 0, 0, 0] and exact.n_grams == [1, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the statement is sound
# ---------------------------------------------------------------------------------------------------------------------------
def test_without_a_model_the_statement_is_the_model_free_one():
    em, em_len, spellings, _ = L.main_case()
    trie = L.Trie(spellings, 256, 0, 126)
    same_hyps(D.decode_batch(em, trie, em_len, beam=10, nbest=10, lm=None), D.decode_batch(em, trie, em_len, beam=10, nbest=10))
    for spellings, V, sil, kw in ((L.ONE_WORD, 40, None, dict(beam=2, nbest=2)), (L.PREFIX_DOUBLED, 32, None, dict(beam=10, nbest=10, beam_threshold=2.0)),
                                  (L.wide_lexicon(), 256, 126, dict(beam=16, nbest=16, sil_score=-0.5, word_score=1.5))):
        trie = L.Trie(spellings, V, 0, sil)
        em = L.emissions(9, spellings, 3, 16, V, 0, -1 if sil is None else sil)
        same_hyps(D.decode_batch(em, trie, lm=None, **kw), D.decode_batch(em, trie, **kw))


def test_the_statements_word_score_is_the_textbook_back_off():
    """Every (history, word) pair a decode of the main LM case asks for, against the recursive definition in float64: at most
    order additions of values below 100 in fp32, 1e-5 covers their rounding."""
    em, em_len, spellings, words, lm = M.main_lm_case()
    trie = L.Trie(spellings, 256, 0, 126)
    stats = {}
    D.decode_batch(em[40:52], trie, beam=10, nbest=10, lm=lm, lm_weight=1.0, lm_words=words, stats=stats)
    assert len(stats["pairs"]) > 500 and set(stats["depth"]) == {0, 1, 2}
    for ctx, v in stats["pairs"]:
        assert abs(float(M.lm_score(lm, 3, ctx, v)) - M.textbook(lm, ctx, v)) <= 1e-5, (ctx, v)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
GOOD = ["\\data\\", "ngram 1=3", "ngram 2=2", "", "\\1-grams:", "-1 a -0.5", "-2 b -0.25", "-3 <unk>", "", "\\2-grams:", "-0.5 a b", "-0.75 b a", "", "\\end\\"]


def _arpa(tmp_path, lines):
    path = tmp_path / "bad.arpa"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


@pytest.mark.parametrize("lines,line_no,what", [
    (GOOD[:6] + GOOD[7:], 9, "holds 2 n-grams"),                  # a unigram fewer than \\data\\ states
    (GOOD[:11] + ["-0.1 b b"] + GOOD[11:], 15, "holds 3 n-grams"),  # a bigram more
    (GOOD[:2] + ["ngram 2=2", "ngram 3=1"] + GOOD[3:12] + ["", "\\3-grams:", "-0.1 a a b", "", "\\end\\"], 16, "prefix"),  # (a a) is no bigram
    (GOOD[:11] + ["-0.5 a b"] + GOOD[12:], 12, "duplicate"),
    (GOOD[:6] + ["-2 a"] + GOOD[7:], 7, "duplicate"),
    (["\\data\\"] + [f"ngram {n}=1" for n in range(1, 7)], 7, "above 5"),
    (GOOD[:5] + ["-inf a -0.5"] + GOOD[6:], 6, "non-finite"),
    (GOOD[:5] + ["-1 a nan"] + GOOD[6:], 6, "non-finite"),
    (GOOD[:10] + ["-0.5 a zzz"] + GOOD[11:], 11, "no unigram"),
    (GOOD[:5] + ["-1 a b c d"] + GOOD[6:], 6, "fields"),
    (GOOD[:5] + ["minus-one a"] + GOOD[6:], 6, "not a number"),
], ids=["count-low", "count-high", "prefix-absent", "duplicate-bigram", "duplicate-unigram", "order-6", "minus-inf", "nan", "word-without-unigram",
        "too-many-fields", "not-a-number"])
def test_a_malformed_file_is_refused_with_file_and_line(lib, tmp_path, lines, line_no, what):
    trie = TokenTrie.from_spellings([[1], [2]], 8, words=["a", "b"])
    path = _arpa(tmp_path, lines)
    with pytest.raises(ValueError) as err:
        NGramLM.from_arpa(path, trie)
    assert f"{path}:{line_no}:" in str(err.value) and what in str(err.value), str(err.value)


def test_the_good_file_reads_and_a_missing_unk_with_a_missing_word_is_refused(lib, tmp_path):
    trie = TokenTrie.from_spellings([[1], [2]], 8, words=["a", "b"])
    lm = NGramLM.from_arpa(_arpa(tmp_path, GOOD), trie)
    assert lm.order == 2 and lm.n_grams == [3, 2] and lm.unk == 2
    more = TokenTrie.from_spellings([[1], [2], [3], [4]], 8, words=["a", "b", "c", "d"])
    assert NGramLM.from_arpa(_arpa(tmp_path, GOOD), more).word_map.tolist() == [0, 1, 2, 2]
    without_unk = [line for line in GOOD if "<unk>" not in line]
    without_unk[1] = "ngram 1=2"
    assert NGramLM.from_arpa(_arpa(tmp_path, without_unk), trie).unk == -1
    with pytest.raises(ValueError, match=r"no <unk> and lacks 2 of the lexicon's words: 'c', 'd'"):
        NGramLM.from_arpa(_arpa(tmp_path, without_unk), more)


def _pack_args(order=2, lex_words=2, bos=-1, eos=-1, **over):
    """A small valid model as eec_ngram_pack takes it; ``over`` replaces arrays by name."""
    a = dict(counts=np.array([3, 2, 1][:order], dtype=np.int64),
             words=[np.array([0, 1, 2], dtype=np.int32), np.array([0, 1, 1, 0], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)][:order],
             logp=[np.array([-1, -2, -3], dtype=np.float32), np.array([-0.5, -0.75], dtype=np.float32), np.array([-0.1], dtype=np.float32)][:order],
             backoff=[np.array([-0.5, -0.25, 0], dtype=np.float32), np.zeros(2, dtype=np.float32), np.zeros(1, dtype=np.float32)][:order],
             word_map=np.array([0, 1], dtype=np.int32))
    a.update(over)
    return order, lex_words, bos, eos, a


def _pack(lib, order, lex_words, bos, eos, a, image_bytes=None, null=()):
    need = lib.eec_ngram_pack_bytes(order, a["counts"].ctypes.data, lex_words)
    image = np.zeros(max(need, 64) // 4, dtype=np.int32)
    ptrs = lambda arrays: (C.c_void_p * len(arrays))(*[x.ctypes.data for x in arrays])  # noqa: E731
    keep = [ptrs(a["words"]), ptrs(a["logp"]), ptrs(a["backoff"])]
    n_nodes = C.c_int32()
    at = lambda name, value: None if name in null else value  # noqa: E731
    rc = lib.eec_ngram_pack(order, at("counts", a["counts"].ctypes.data), at("words", keep[0]), at("logp", keep[1]), at("backoff", keep[2]),
                            at("word_map", a["word_map"].ctypes.data), lex_words, bos, eos, at("image", image.ctypes.data),
                            need if image_bytes is None else image_bytes, C.byref(n_nodes))
    return rc, image, n_nodes.value, need


def test_the_packer_refuses_bad_arguments(lib):
    rc, image, n_nodes, need = _pack(lib, *_pack_args(order=3, bos=2, eos=1))
    assert rc == 0 and n_nodes == 7 and need % 8 == 0
    head, grams, links, word_map = M.read_lm_image(image)
    assert head["bos_node"] == 3 and head["eos_word"] == 1 and links[(0, 1, 0)] == (1, 0) and word_map == [0, 1] and 4 * int(image[15]) <= need
    for name in ("counts", "words", "logp", "backoff", "word_map", "image"):
        assert _pack(lib, *_pack_args(), null=(name,))[0] == BAD_ARG, name
    assert b"null" in lib.eec_last_error()
    i32, f32 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.float32))
    base = _pack_args()[4]
    assert _pack(lib, *_pack_args(lex_words=0))[0] == BAD_ARG
    assert _pack(lib, *_pack_args(bos=3))[0] == BAD_ARG and _pack(lib, *_pack_args(eos=-2))[0] == BAD_ARG
    assert _pack(lib, *_pack_args(word_map=i32(0, 3)))[0] == BAD_ARG
    assert _pack(lib, *_pack_args(words=[i32(0, 1, 1), base["words"][1]]))[0] == BAD_ARG and b"duplicate" in lib.eec_last_error()
    assert _pack(lib, *_pack_args(words=[i32(0, 1, 3), base["words"][1]]))[0] == BAD_ARG
    assert _pack(lib, *_pack_args(words=[base["words"][0], i32(0, 1, 0, 1)]))[0] == BAD_ARG and b"duplicate" in lib.eec_last_error()
    assert _pack(lib, *_pack_args(words=[base["words"][0], i32(0, 1, 1, 5)]))[0] == BAD_ARG
    assert _pack(lib, *_pack_args(order=3, words=[base["words"][0], base["words"][1], i32(2, 2, 0)]))[0] == BAD_ARG and b"prefix" in lib.eec_last_error()
    assert _pack(lib, *_pack_args(logp=[f32(-1, np.inf, -3), base["logp"][1]]))[0] == BAD_ARG and b"non-finite" in lib.eec_last_error()
    assert _pack(lib, *_pack_args(backoff=[f32(0, 0, np.nan), base["backoff"][1]]))[0] == BAD_ARG
    assert _pack(lib, *_pack_args(counts=np.array([3, -1], dtype=np.int64)))[0] == BAD_ARG
    assert _pack(lib, 6, 2, -1, -1, dict(base, counts=np.array([3, 2, 0, 0, 0, 0], dtype=np.int64)))[0] == UNSUPPORTED
    assert _pack(lib, 0, 2, -1, -1, base)[0] == UNSUPPORTED
    assert _pack(lib, *_pack_args(), image_bytes=need - 100)[0] == WORKSPACE


def test_the_packers_size_arithmetic(lib):
    size = lambda order, counts, lex: lib.eec_ngram_pack_bytes(order, np.array(counts, dtype=np.int64).ctypes.data, lex)  # noqa: E731
    assert size(2, [3, 2], 2) == 4 * ((16 + 7 + 5 + 3 * 6 + 2 + 1) & ~1)
    assert size(0, [3], 2) == 0 and size(6, [1] * 6, 2) == 0 and size(1, [0], 2) == 0 and size(2, [3, -1], 2) == 0 and size(1, [3], 0) == 0
    assert lib.eec_ngram_pack_bytes(1, None, 2) == 0
    assert size(3, [2 ** 30, 2 ** 30, 2 ** 30], 5) == 0  # past 2^31 dwords
    assert size(3, [89114, 2000000, 2000000], 89114) > 0


def test_decode_argument_errors_come_before_any_device_use(lib):
    """Plausible but unusable addresses: a non-finite lm_weight, a null model and beam_size 17 are refused on the arguments alone."""
    fake = 0x10000
    dec, need = lib.eec_ctc_lexbeam_lm_decode, lib.eec_ctc_lexbeam_workspace_bytes(3, 7, 10)

    def call(beam=10, nbest=2, lm=fake, lm_weight=1.0, logp=fake, ws_bytes=need, n=3):
        return dec(logp, n, 7, 40, None, fake, 0, -1, beam, nbest, 0.0, 0.0, 50.0, 7, fake, fake, fake, fake, None, fake, fake, fake, ws_bytes, None,
                   lm, lm_weight)
    assert call(lm_weight=float("inf")) == BAD_ARG and b"lm_weight" in lib.eec_last_error()
    assert call(lm_weight=float("nan")) == BAD_ARG and call(lm_weight=float("-inf")) == BAD_ARG
    assert call(lm=None) == BAD_ARG and b"lm" in lib.eec_last_error()
    assert call(lm=fake + 4) == BAD_ARG
    assert call(beam=17) == UNSUPPORTED and call(beam=0) == UNSUPPORTED and call(nbest=11) == UNSUPPORTED
    assert call(logp=None) == BAD_ARG and call(ws_bytes=need - 1) == WORKSPACE
    assert call(n=0) == 0  # nothing to do


def test_the_python_entry_needs_a_device_and_the_models_trie(lib, tmp_path):
    import torch
    from early_exit_transformer_amd.model import ctc_lexicon_decode
    trie = TokenTrie.from_spellings([[1], [2]], 8, words=["a", "b"])
    lm = NGramLM.from_arpa(_arpa(tmp_path, GOOD), trie)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc_lexicon_decode(torch.zeros(1, 3, 8), trie, lm=lm, lm_weight=1.0)
