"""CPU tests of the lexicon-constrained CTC beam search's host side: the trie packer (host code in csrc/ctc_lexbeam.hip) against a
reader of the documented image layout, every argument error of both entry points (all decided before any device work), the
size arithmetic, and the plain-Python statement of the search (tests/lexbeam_statement.py) against cases worked out by hand."""
import ctypes as C

import numpy as np
import pytest

import lexbeam_cases as L
import lexbeam_statement as D
from early_exit_transformer_amd.lexicon import TokenTrie
from lexbeam_helpers import library

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003
NI = -np.inf


@pytest.fixture(scope="module")
def lib():
    return library()


def _pack(lib, spellings, V, blank=0, sil=-1, image_bytes=None):
    """eec_ctc_trie_pack through ctypes: (return code, image as int32, n_nodes, n_shadowed)."""
    lens = np.array([len(sp) for sp in spellings], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.array([t for sp in spellings for t in sp], dtype=np.int32)
    need = lib.eec_ctc_trie_pack_bytes(len(spellings), int(offsets[-1]))
    image = np.full((need if image_bytes is None else image_bytes) // 4 + 4, -7, dtype=np.int32)
    nodes, shadowed = C.c_int32(-7), C.c_int32(-7)
    rc = lib.eec_ctc_trie_pack(flat.ctypes.data, offsets.ctypes.data, len(spellings), V, blank, sil, image.ctypes.data,
                               need if image_bytes is None else image_bytes, C.byref(nodes), C.byref(shadowed))
    return rc, image, nodes.value, shadowed.value


# ---------------------------------------------------------------------------------------------------------------------------
# the packer
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spellings,V,sil", [
    ("one word", L.ONE_WORD, 40, -1),
    ("prefix, doubled token, duplicate", L.PREFIX_DOUBLED, 32, -1),
    ("more than 64 children", L.wide_lexicon(), 256, 126),
])
def test_pack_round_trips_through_the_documented_layout(lib, name, spellings, V, sil):
    rc, image, nodes, shadowed = _pack(lib, spellings, V, 0, sil)
    assert rc == 0
    head, words = L.read_image(image)
    ref = L.Trie(spellings, V, 0, None if sil < 0 else sil)
    assert words == L.first_words(spellings)  # every spelling reachable, the first word in file order wins
    assert head["n_nodes"] == nodes == ref.n_nodes and head["n_shadowed"] == shadowed == ref.shadowed
    assert (head["V"], head["blank"], head["sil"], head["n_words"]) == (V, 0, sil, len(spellings))
    need = lib.eec_ctc_trie_pack_bytes(len(spellings), sum(len(sp) for sp in spellings))
    assert image[9] * 4 <= need and (image[need // 4:] == -7).all() and len(image) > need // 4  # nothing written past the stated size


def test_pack_details_of_the_small_lexica(lib):
    _, image, nodes, shadowed = _pack(lib, L.ONE_WORD, 40)
    assert (nodes, shadowed) == (4, 0)  # root - 5 - 9 - 5
    _, image, nodes, shadowed = _pack(lib, L.PREFIX_DOUBLED, 32)
    head, words = L.read_image(image)
    assert shadowed == 1 and words[(3, 4)] == 1  # [3, 4] stands at 1 and at 5: the first wins, the second is counted
    assert words[(3,)] == 0 and words[(3, 4, 3, 3, 7)] == 2  # a word that is a prefix of another; a doubled token on the way
    wide = L.wide_lexicon()
    _, image, nodes, _ = _pack(lib, wide, 256, 0, 126)
    degree = np.diff(image[16:16 + nodes + 1])
    assert degree[0] == 150 and 64 < sorted(degree[1:])[-1] < 150  # the root and one inner node above 64 children


def test_pack_of_the_fixture(lib):
    tokens, words, spellings = L.load_fixture()
    assert len(tokens) == 256 and tokens[0] == "@" and tokens[126] == "<pad>" and 1900 < len(words) < 2100
    rc, image, nodes, shadowed = _pack(lib, spellings, 256, 0, 126)
    assert rc == 0
    head, got = L.read_image(image)
    ref = L.Trie(spellings, 256, 0, 126)
    assert got == L.first_words(spellings) and nodes == ref.n_nodes and shadowed == ref.shadowed
    assert any(ref.word[n] >= 0 and ref.kids[n] for n in range(ref.n_nodes))  # nodes that end a word AND have children
    # the Python class packs the same image
    trie = TokenTrie.from_spellings(spellings, 256, blank=0, sil=126, words=words)
    assert np.array_equal(trie._image.numpy().view(np.int32), image[:image[9]])
    assert (trie.n_nodes, trie.n_shadowed, trie.words, len(trie)) == (nodes, shadowed, words, len(words))


def test_token_trie_from_files_reads_the_reference_formats(tmp_path):
    tokens, words, spellings = L.load_fixture()
    (tmp_path / "t.tok").write_text("".join(t + "\n" for t in tokens), encoding="utf-8")
    (tmp_path / "l.lex").write_text("".join(f"{w}\t{' '.join(tokens[t] for t in sp)}\n" for w, sp in zip(words[:300], spellings[:300])),
                                    encoding="utf-8")
    trie = TokenTrie.from_files(str(tmp_path / "l.lex"), str(tmp_path / "t.tok"), blank_token="@", sil_token="<pad>")
    assert (trie.V, trie.blank, trie.sil, trie.words) == (256, 0, 126, words[:300])
    assert L.read_image(trie._image.numpy().view(np.int32))[1] == L.first_words(spellings[:300])
    (tmp_path / "crlf.lex").write_bytes("".join(f"{w}\t{' '.join(tokens[t] for t in sp)}\r\n" for w, sp in zip(words[:9], spellings[:9])).encode())
    (tmp_path / "crlf.tok").write_bytes("".join(t + "\r\n" for t in tokens).encode())
    crlf = TokenTrie.from_files(str(tmp_path / "crlf.lex"), str(tmp_path / "crlf.tok"), sil_token="<pad>")
    assert crlf.words == words[:9] and L.read_image(crlf._image.numpy().view(np.int32))[1] == L.first_words(spellings[:9])
    with pytest.raises(ValueError, match=r"no-tab.lex:2: expected word<TAB>tokens"):
        (tmp_path / "no-tab.lex").write_text(f"a\t{tokens[5]}\nword without a tab\n", encoding="utf-8")
        TokenTrie.from_files(str(tmp_path / "no-tab.lex"), str(tmp_path / "t.tok"))
    with pytest.raises(ValueError, match="not in"):
        (tmp_path / "bad.lex").write_text("word\tnot-a-token\n", encoding="utf-8")
        TokenTrie.from_files(str(tmp_path / "bad.lex"), str(tmp_path / "t.tok"))
    with pytest.raises(RuntimeError, match="eec_ctc_trie_pack"):
        TokenTrie.from_spellings([[1, 0]], 8)  # the blank inside a spelling


def test_pack_argument_errors(lib):
    flat, off = np.array([1, 2, 3], dtype=np.int32), np.array([0, 1, 3], dtype=np.int64)
    image = np.zeros(256, dtype=np.int32)
    pack = lib.eec_ctc_trie_pack

    def call(spell=flat, offsets=off, n=2, V=8, blank=0, sil=-1, img=image, nbytes=None):
        at = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return pack(at(spell), at(offsets), n, V, blank, sil, at(img), image.nbytes if nbytes is None else nbytes, None, None)
    assert call() == 0  # the count outputs are optional
    assert call(spell=None) == BAD_ARG and call(offsets=None) == BAD_ARG and call(img=None) == BAD_ARG
    assert call(n=0) == BAD_ARG and call(n=-1) == BAD_ARG
    assert call(offsets=np.array([1, 2, 3], dtype=np.int64)) == BAD_ARG          # not from 0
    assert call(offsets=np.array([0, 3, 2], dtype=np.int64)) == BAD_ARG          # descending
    assert call(offsets=np.array([0, 0, 3], dtype=np.int64)) == BAD_ARG          # an empty spelling
    assert call(spell=np.array([1, 8, 3], dtype=np.int32)) == BAD_ARG            # a token >= V
    assert call(spell=np.array([1, -1, 3], dtype=np.int32)) == BAD_ARG           # a negative token
    assert call(spell=np.array([1, 0, 3], dtype=np.int32)) == BAD_ARG            # the blank
    assert call(sil=3) == BAD_ARG                                                # the sil token in a spelling
    assert call(sil=0) == BAD_ARG and call(sil=8) == BAD_ARG and call(blank=8) == BAD_ARG and call(blank=-1) == BAD_ARG
    assert call(V=257, spell=np.array([1, 256, 3], dtype=np.int32)) == UNSUPPORTED
    assert call(V=256, spell=np.array([1, 255, 3], dtype=np.int32)) == 0
    need = lib.eec_ctc_trie_pack_bytes(2, 3)
    assert call(nbytes=need) == 0 and call(nbytes=need - 1) == WORKSPACE and call(nbytes=16) == WORKSPACE
    assert b"image_bytes" in lib.eec_last_error()


def test_size_functions_are_monotonic(lib):
    size = lib.eec_ctc_trie_pack_bytes
    assert size(0, 0) == 0 and size(-1, 5) == 0 and size(3, 2) == 0 and size(1, 1) > 0 and size(1, 1) % 8 == 0
    by_tokens = [size(10, t) for t in (10, 11, 100, 5000, 614000)]
    assert by_tokens == sorted(by_tokens) and len(set(by_tokens)) == len(by_tokens)
    by_words = [size(n, 614000) for n in (1, 10, 89114)]
    assert by_words == sorted(by_words)
    assert size(89114, 162620) < (2 << 20)  # the real lexicon's trie (162 621 nodes): inside an XCD's L2
    ws = lib.eec_ctc_lexbeam_workspace_bytes
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, 0) == 0 and ws(-1, 5, 5) == 0
    for k in range(3):
        grow = []
        for v in (1, 2, 7, 16):
            a = [3, 5, 4]
            a[k] = v
            grow.append(ws(*a))
        assert grow == sorted(grow) and len(set(grow)) == 4 and grow[0] > 0, k
    assert ws(384, 256, 16) == 384 * 256 * 16 * 8


def test_decode_argument_errors_come_before_any_device_use(lib):
    """Plausible but unusable addresses: every refusal is decided on the arguments alone, nothing is dereferenced."""
    fake = 0x10000
    dec, need = lib.eec_ctc_lexbeam_decode, lib.eec_ctc_lexbeam_workspace_bytes(3, 7, 10)

    def call(logp=fake, n=3, T=7, V=40, em_len=None, trie=fake, blank=0, sil=-1, beam=10, nbest=2, thr=50.0, max_words=7, words=fake, wc=fake,
             tok=fake, tc=fake, ts=None, sc=fake, nh=fake, ws=fake, ws_bytes=need):
        return dec(logp, n, T, V, em_len, trie, blank, sil, beam, nbest, 0.0, 0.0, thr, max_words, words, wc, tok, tc, ts, sc, nh, ws, ws_bytes, None)
    for name in ("logp", "trie", "words", "wc", "tok", "tc", "sc", "nh", "ws"):
        assert call(**{name: None}) == BAD_ARG, name
    assert b"null" in lib.eec_last_error()
    assert call(n=-1) == BAD_ARG and call(T=0) == BAD_ARG and call(max_words=0) == BAD_ARG
    assert call(blank=-1) == BAD_ARG and call(blank=40) == BAD_ARG and call(sil=40) == BAD_ARG and call(sil=-2) == BAD_ARG
    assert call(blank=5, sil=5) == BAD_ARG
    assert call(trie=fake + 4) == BAD_ARG and call(ws=fake + 4) == BAD_ARG
    assert call(V=257) == UNSUPPORTED and call(V=1) == UNSUPPORTED
    assert call(beam=0) == UNSUPPORTED and call(beam=17) == UNSUPPORTED
    assert call(nbest=0) == UNSUPPORTED and call(nbest=11) == UNSUPPORTED
    assert call(beam=16, nbest=16) == WORKSPACE  # the boundary values pass the range check and reach the size check
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(n=0, logp=None, trie=None, words=None, wc=None, tok=None, tc=None, sc=None, nh=None, ws=None, ws_bytes=0) == 0  # nothing to do


def test_the_python_entry_needs_a_device():
    import torch
    from early_exit_transformer_amd.model import ctc_lexicon_decode
    trie = TokenTrie.from_spellings(L.ONE_WORD, 40)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc_lexicon_decode(torch.zeros(1, 3, 40), trie)


# ---------------------------------------------------------------------------------------------------------------------------
# the statement against cases worked out by hand.  V = 3 or 4: blank 0, a = 1, b = 2, (sil 3).  Log-probs are small binary
# fractions, so every sum below is exact; NI = -inf switches a label off.  The candidate ids named below are the narrow
# kernels' (2 c + w) * 16 + i; the statement's (2 c + w) * 64 + i puts them in the same order.
# ---------------------------------------------------------------------------------------------------------------------------
def em(*rows):
    return np.array(rows, dtype=np.float32)


def hyp(words, tokens, steps, score):
    return (words, tokens, steps, np.float32(score))


A_AB = [[1], [1, 2]]  # word 0 = "a", word 1 = "ab": the node after a both ends a word and has a child
CASE1 = em([NI, -1, NI], [-2, NI, -0.5], [-0.25, NI, NI])


def test_statement_two_word_lexicon():
    """Frame 0: only a.  The edge a gives the in-word candidate (y, a) -1 [id 32] and the word end ("a",) -1 [id 48]: equal scores,
    rank 0 is the lower id.  Frame 1: from rank 0 blank -3 [id 0] and the edge b, which ends "ab": -1.5 [id 80]; from rank 1 blank
    -3 [id 1] (a after a without a blank is no new edge, and the repeat is -inf).  Frame 2: blank, -0.25 each."""
    trie = L.Trie(A_AB, 3)
    got = D.decode(CASE1, trie, beam=16, nbest=16, beam_threshold=np.inf)
    assert got == [hyp([1], [1, 2], [0, 1], -1.75), hyp([0], [1], [0], -3.25)]  # the in-word hypothesis (y, blank) is not complete
    assert D.decode(CASE1, trie, beam=16, nbest=1, beam_threshold=np.inf) == got[:1]
    assert D.decode(CASE1, trie, beam=1, nbest=1, beam_threshold=np.inf) == got[:1]  # beam 1 keeps id 32, which leads to "ab"
    assert D.decode(CASE1, trie, beam=16, nbest=16, beam_threshold=np.inf, length=2) == [hyp([1], [1, 2], [0, 1], -1.5), hyp([0], [1], [0], -3.0)]
    assert D.decode(CASE1, trie, beam=16, nbest=16, length=1) == [hyp([0], [1], [0], -1.0)]
    for bad in (0, -1, 4):
        assert D.decode(CASE1, trie, length=bad) == []


def test_statement_beam_threshold_leaves_fewer_than_beam():
    """CASE1 with threshold 1: at frame 1 the best is -1.5, the two -3 candidates fall below -2.5, one hypothesis is left."""
    assert D.decode(CASE1, L.Trie(A_AB, 3), beam=16, nbest=16, beam_threshold=1.0) == [hyp([1], [1, 2], [0, 1], -1.75)]
    # threshold 1.5 keeps them: -3 >= -1.5 - 1.5
    assert len(D.decode(CASE1, L.Trie(A_AB, 3), beam=16, nbest=16, beam_threshold=1.5)) == 2


def test_statement_repeat_after_word_end():
    """One word "a", three frames of a: the word ends at frame 0 [id 48], then a repeats through the repeat rule (-0.5, -0.25); it
    is not a second "a" (a after a needs a blank)."""
    e = em([NI, -1], [NI, -0.5], [NI, -0.25])
    assert D.decode(e, L.Trie([[1]], 2), beam=4, nbest=4) == [hyp([0], [1], [0], -1.75)]


def test_statement_blank_between_equal_tokens():
    """One word "aa".  Frame 1 offers blank -0.5 or a -0.25: the repeat scores higher (rank 0) but stays at the first a for good;
    only the hypothesis that took the blank can take the edge a again at frame 2 and end the word: -1 - 0.5 - 1 [id 49]."""
    e = em([NI, -1], [-0.5, -0.25], [NI, -1])
    assert D.decode(e, L.Trie([[1, 1]], 2), beam=4, nbest=4) == [hyp([0], [1, 1], [0, 2], -2.5)]
    assert D.decode(e, L.Trie([[1, 1]], 2), beam=1, nbest=1) == []  # beam 1 follows the repeat


def test_statement_sil_on_and_off():
    """One word "a", then a frame that prefers label 3.  Off, 3 is no label of any word: only blank continues, -1 - 3.  On
    (sil_score -0.25): (0, sil) = (-1 - 0.5) - 0.25 [id 96] ahead of blank -4 [id 0].  A third frame of sil: rank 0 repeats it,
    (-1.75 - 0.5) - 0.25 = -2.5, rank 1 (after blank) enters sil with (-4 - 0.5) - 0.25: the same state, merged, the higher stays."""
    e = em([NI, -1, NI, NI], [-3, NI, NI, -0.5])
    assert D.decode(e, L.Trie([[1]], 4), beam=4, nbest=4) == [hyp([0], [1], [0], -4.0)]
    on = L.Trie([[1]], 4, sil=3)
    assert D.decode(e, on, beam=4, nbest=4, sil_score=-0.25) == [hyp([0], [1, 3], [0, 1], -1.75), hyp([0], [1], [0], -4.0)]
    e3 = em([NI, -1, NI, NI], [-3, NI, NI, -0.5], [NI, NI, NI, -0.5])
    assert D.decode(e3, on, beam=4, nbest=4, sil_score=-0.25) == [hyp([0], [1, 3], [0, 1], -2.5)]
    assert D.decode(e3, on, beam=4, nbest=4, sil_score=0.0) == [hyp([0], [1, 3], [0, 1], -2.0)]
    # sil before any word, from the start state (pb): (0 - 0.5) + 0 at frame 0 needs label 3 there
    e0 = em([NI, NI, NI, -0.5], [NI, -1, NI, NI])
    assert D.decode(e0, on, beam=4, nbest=4) == [hyp([0], [3, 1], [0, 1], -1.5)]


def test_statement_word_score_changes_the_winner():
    """Words "a", "b", "ab"; frames a, b at -1 each.  "ab": (-1 - 1) + ws.  "a b": ((-1 + ws) - 1) + ws.  ws = -4: -6 against -10;
    ws = +1: -1 against 0 (and at frame 0 the word end, 0, ranks above the in-word candidate, -1)."""
    trie = L.Trie([[1], [2], [1, 2]], 3)
    e = em([NI, -1, NI], [NI, NI, -1])
    assert D.decode(e, trie, beam=4, nbest=4, word_score=-4.0, beam_threshold=np.inf) == [hyp([2], [1, 2], [0, 1], -6.0), hyp([0, 1], [1, 2], [0, 1], -10.0)]
    assert D.decode(e, trie, beam=4, nbest=4, word_score=1.0, beam_threshold=np.inf) == [hyp([0, 1], [1, 2], [0, 1], 0.0), hyp([2], [1, 2], [0, 1], -1.0)]
    assert D.decode(e, trie, beam=4, nbest=4, word_score=0.0, beam_threshold=np.inf) == [hyp([2], [1, 2], [0, 1], -2.0), hyp([0, 1], [1, 2], [0, 1], -2.0)]
    # equal scores: at frame 0 the in-word candidate [id 32] ranks above the word end [id 48], so "ab" has id 80 and "a b" id 81


def test_statement_no_complete_hypothesis_and_dead_frames():
    only_ab = L.Trie([[1, 2]], 3)
    assert D.decode(em([NI, -1, NI]), only_ab, beam=4, nbest=4) == []           # ends inside the word
    assert D.decode(em([-1, NI, NI]), only_ab, beam=4, nbest=4) == [hyp([], [], [], -1.0)]  # the empty transcript is complete
    dead = em([NI, -1, NI], [NI, NI, NI], [-1, -1, -1])
    assert D.decode(dead, L.Trie(A_AB, 3), beam=4, nbest=4) == []               # an all-(-inf) frame leaves no candidate
    nan = em([NI, -1, NI], [np.nan, np.nan, np.nan], [-1, -1, -1])
    assert D.decode(nan, L.Trie(A_AB, 3), beam=4, nbest=4) == []                # NaN scores are dropped like -inf
    part = em([NI, -1, NI], [np.nan, NI, -0.5], [-0.25, np.nan, NI])
    assert D.decode(part, L.Trie(A_AB, 3), beam=4, nbest=4) == [hyp([1], [1, 2], [0, 1], -1.75)]


def test_the_gpu_suite_will_see_both_outcomes():
    """The largest case of tests/test_gpu_lexbeam.py, decoded by the statement alone: at least a quarter of its sequences end
    with a hypothesis and at least a tenth without -- not counting the ones whose length is out of range."""
    e, em_len, spellings, _ = L.main_case()
    trie = L.Trie(spellings, 256, 0, 126)
    n = [len(r) for r, k in zip(D.decode_batch(e, trie, em_len, beam=10, nbest=10), em_len) if 1 <= k <= 64]
    assert len(n) == 67 and sum(1 for k in n if k > 0) >= 0.25 * 70 and sum(1 for k in n if k == 0) >= 0.10 * 70, n
