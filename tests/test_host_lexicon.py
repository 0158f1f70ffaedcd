"""CPU tests of the lexicon post-processing's host side (early_exit_transformer_amd/lexicon.py, the host half of
csrc/lexicon.hip): the test-side restatement against the fixture the reference's own ``apply_lex`` produced
(tests/golden/apply_lex.json), the packed image against a reader of its documented layout, size arithmetic, and argument errors
that must come before any device use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lex_cases as L
from conftest import ROOT
from early_exit_transformer_amd import capi, lexicon
from early_exit_transformer_amd.build import LIB_PATH
from early_exit_transformer_amd.lexicon import Lexicon, apply_lex, load_dict

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _pack(lib, words, image_bytes=None):
    """eec_lexicon_pack through ctypes: (return code, image as int32, code map, A)."""
    lens = np.array([len(w) for w in words], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    symbols = np.array([ord(ch) for w in words for ch in w], dtype=np.uint32)
    need = lib.eec_lexicon_pack_bytes(len(words), int(offsets[-1]), int(lens.max()))
    assert need > 0 and need % 8 == 0
    image = np.zeros((need if image_bytes is None else image_bytes) // 4, dtype=np.int32)
    code_map, A = np.zeros(256, dtype=np.int32), C.c_int32(-7)
    rc = lib.eec_lexicon_pack(symbols.ctypes.data, offsets.ctypes.data, len(words), image.ctypes.data, image.nbytes, code_map.ctypes.data,
                              C.byref(A))
    return rc, image, code_map, A.value


def test_the_restatement_equals_what_the_reference_returned():
    fx = L.load_fixture()
    assert len(fx["lexicon"]) > 2000 and max(len(w) for w in fx["lexicon"]) == 69
    required = ["the quik brown  fox jumpd ovr teh lazy dog", "", " ", "héllo wor1d a'll"]
    assert fx["inputs"][:4] == required and any(len(s) == 70 and " " not in s for s in fx["inputs"])
    known = set(fx["lexicon"])
    assert any(s and all(w in known for w in s.split(" ")) for s in fx["inputs"])
    for text, want in zip(fx["inputs"], fx["outputs"]):
        assert L.snap(text, fx["lexicon"]) == want, text


def test_header_constants_match_the_python_module():
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    assert int(re.search(r"#define EEC_LEX_MAX_QUERY (\d+)", header).group(1)) == lexicon.MAX_QUERY >= 256
    assert int(re.search(r"#define EEC_LEX_BLOCK_WORDS (\d+)", header).group(1)) == lexicon.BLOCK_WORDS
    assert int(re.search(r"#define EEC_LEX_TILE_SWITCH (\d+)", header).group(1)) == lexicon.TILE_SWITCH


def test_pack_round_trips_through_the_documented_layout(lib):
    """Every word recoverable by its original index, the stored order a stable sort by length, empty words and duplicates
    kept, the code map the lexicon's code points in ascending order."""
    words = ["", "b", "ab", "", "ü", "a'b", "b", "zebra", "añb", "x" * 69, "ab", "", "abcd", "abcde", "q" * 9]
    words += L.random_lexicon(700, seed=11, lengths=range(0, 15))
    rc, image, code_map, A = _pack(lib, words)
    assert rc == 0
    alphabet = sorted({ord(ch) for w in words for ch in w})
    assert A == len(alphabet) and code_map[1:A + 1].tolist() == alphabet
    assert code_map[0] == -1 and (code_map[A + 1:] == -1).all()
    got, lengths = L.unpack_image(image, code_map)
    assert got == words
    assert lengths == sorted(lengths)  # (length, original index) ascending: sorted by length, stable
    assert sum(1 for n, _ in lengths if n == 0) == words.count("")
    # the Python class packs the same image and maps symbols by the same table
    lex = Lexicon(words)
    assert np.array_equal(lex._image.numpy().view(np.int32), image) and lex.alphabet == A
    assert lex.index["b"] == 1 and lex.index[""] == 0 and lex.index["ab"] == 2 and len(lex) == len(words) and "zebra" in lex
    buf, longest = lex.encode(["añ?", "", "b€b"])
    assert longest == 3 and buf[:16].view(np.int32).tolist() == [0, 3, 3, 6]
    code = {cp: c for c, cp in enumerate(code_map.tolist()) if cp >= 0}
    assert buf[16:].tolist() == [code[ord("a")], code[ord("ñ")], 0, code[ord("b")], 0, code[ord("b")]]


def test_pack_of_a_single_and_of_only_empty_words(lib):
    for words in (["solo"], ["", ""], ["a"]):
        rc, image, code_map, A = _pack(lib, words)
        assert rc == 0 and L.unpack_image(image, code_map)[0] == words


def test_pack_bytes_is_monotonic(lib):
    size = lib.eec_lexicon_pack_bytes
    assert size(0, 0, 0) == 0 and size(-1, 5, 5) == 0 and size(3, -1, 5) == 0 and size(3, 100, 5) == 0
    assert 0 < size(1, 0, 0)
    rows = [size(n, 6 * n, 69) for n in (1, 2, 100, 1000, 89114)]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    syms = [size(1000, t, 69) for t in (0, 1000, 6000, 69000)]
    assert syms == sorted(syms) and syms[0] < syms[-1]
    longest = [size(1000, 6000, m) for m in (6, 7, 25, 69, 300)]
    assert longest == sorted(longest) and longest[0] < longest[-1]
    assert size(89114, 614000, 69) < (2 << 20)  # a lexicon of the real one's size: well inside an XCD's 4 MiB L2


def test_pack_argument_errors(lib):
    sym, off = np.array([97, 98], dtype=np.uint32), np.array([0, 1, 2], dtype=np.int64)
    image, cmap = np.zeros(256, dtype=np.int32), np.zeros(256, dtype=np.int32)
    pack = lib.eec_lexicon_pack
    assert pack(sym.ctypes.data, off.ctypes.data, 2, image.ctypes.data, image.nbytes, cmap.ctypes.data, None) == 0
    assert pack(None, off.ctypes.data, 2, image.ctypes.data, image.nbytes, cmap.ctypes.data, None) == BAD_ARG
    assert pack(sym.ctypes.data, None, 2, image.ctypes.data, image.nbytes, cmap.ctypes.data, None) == BAD_ARG
    assert pack(sym.ctypes.data, off.ctypes.data, 2, None, image.nbytes, cmap.ctypes.data, None) == BAD_ARG
    assert pack(sym.ctypes.data, off.ctypes.data, 2, image.ctypes.data, image.nbytes, None, None) == BAD_ARG
    assert pack(sym.ctypes.data, off.ctypes.data, 0, image.ctypes.data, image.nbytes, cmap.ctypes.data, None) == BAD_ARG
    assert pack(sym.ctypes.data, off.ctypes.data, 2, image.ctypes.data, 16, cmap.ctypes.data, None) == WORKSPACE
    down = np.array([0, 2, 1], dtype=np.int64)
    assert pack(sym.ctypes.data, down.ctypes.data, 2, image.ctypes.data, image.nbytes, cmap.ctypes.data, None) == BAD_ARG


def test_an_alphabet_of_256_symbols_is_refused_and_255_is_packed(lib):
    words255 = [chr(0x100 + i) for i in range(255)]
    rc, image, code_map, A = _pack(lib, words255)
    assert rc == 0 and A == 255 and L.unpack_image(image, code_map)[0] == words255
    rc, _, _, _ = _pack(lib, words255 + ["a"])
    assert rc == UNSUPPORTED
    with pytest.raises(ValueError, match="255"):
        Lexicon(words255 + ["a"])


def test_nearest_argument_errors_come_before_any_device_use(lib):
    """Plausible but unusable addresses: every refusal below is decided on the arguments alone, so nothing is dereferenced and
    no device is needed."""
    fake = 0x10000
    near, ws = lib.eec_lexicon_nearest, lib.eec_lexicon_nearest_workspace_bytes
    n = ws(5, 1000)
    assert n >= 5 * 8 and ws(0, 1000) == 0 and ws(5, 0) == 0
    assert ws(1, 89114) == 8 * ((89114 + lexicon.BLOCK_WORDS - 1) // lexicon.BLOCK_WORDS)  # one query: one share per workgroup of words
    assert ws(4096, 89114) <= ws(1, 89114) * 4096
    cap = lexicon.MAX_QUERY
    assert near(fake, 1000, fake, fake, 5, cap + 1, fake, fake, fake, n, None) == UNSUPPORTED
    assert near(fake, 1000, fake, fake, 5, -1, fake, fake, fake, n, None) == BAD_ARG
    assert near(fake, 0, fake, fake, 5, 8, fake, fake, fake, n, None) == BAD_ARG
    assert near(fake, 1000, fake, fake, -1, 8, fake, fake, fake, n, None) == BAD_ARG
    for hole in range(6):
        ptrs = [fake] * 6
        ptrs[hole] = None
        packed, q, qo, oi, od, w = ptrs
        assert near(packed, 1000, q, qo, 5, 8, oi, od, w, n, None) == BAD_ARG, hole
    assert near(fake + 4, 1000, fake, fake, 5, 8, fake, fake, fake, n, None) == BAD_ARG  # image not 8-byte aligned
    assert near(fake, 1000, fake, fake, 5, 8, fake, fake, fake, n - 1, None) == WORKSPACE
    assert near(None, 1000, None, None, 0, 0, None, None, None, 0, None) == 0  # no queries: nothing to do


def test_a_query_over_the_cap_and_a_missing_device_raise(monkeypatch):
    import torch
    lex = Lexicon(["alpha", "beta"])
    with pytest.raises(ValueError, match="EEC_LEX_MAX_QUERY"):
        lex.nearest(["x" * (lexicon.MAX_QUERY + 1)])
    with pytest.raises(ValueError, match="EEC_LEX_MAX_QUERY"):
        lex.apply("ok " + "x" * (lexicon.MAX_QUERY + 1))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        lex.nearest(["alpah"])
    with pytest.raises(RuntimeError, match="HIP device only"):
        apply_lex("alpah beta", lex)
    assert Lexicon(["alpha", "", "beta"]).apply("beta alpha  beta") == "beta alpha  beta"  # every piece is an entry: no search
    assert lex.launches == 0


def test_the_empty_lexicon_maps_every_word_to_nothing_without_a_launch(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    lex = Lexicon([])
    assert lex.apply("the quik  fox") == "   " and lex.apply("") == "" and lex.apply_batch(["a b", "c"]) == [" ", ""]
    assert apply_lex("the quik  fox", []) == "   "
    assert lex.launches == 0
    assert L.snap("the quik  fox", []) == "   "
    with pytest.raises(ValueError, match="empty"):
        lex.nearest(["a"])


def test_load_dict_keeps_blank_lines(tmp_path):
    p = tmp_path / "words.lex"
    p.write_text("alpha\n\nbéta \n'tis\n", encoding="utf-8")
    assert load_dict(str(p)) == ["alpha", "", "béta ", "'tis"]


def test_a_plain_list_is_packed_once_per_list_object(monkeypatch):
    words = ["alpha", "beta"]
    a = lexicon.as_lexicon(words)
    assert lexicon.as_lexicon(words) is a and lexicon.as_lexicon(list(words)) is not a and lexicon.as_lexicon(a) is a
    words.append("gamma")  # grown in place: packed again, once
    b = lexicon.as_lexicon(words)
    assert b is not a and "gamma" in b and len(b) == 3 and lexicon.as_lexicon(words) is b
