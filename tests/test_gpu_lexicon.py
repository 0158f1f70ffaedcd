"""The nearest-word kernel (csrc/lexicon.hip; ``Lexicon.nearest`` / ``apply`` / ``apply_batch``, ``apply_lex`` and the
``lexicon=`` keyword of ``BeamInference``) against the fixture the reference's own ``apply_lex`` produced
(tests/golden/apply_lex.json) and the plain-Python statement of tests/lex_cases.py.  Every comparison is of integers or strings
and exact."""
import random

import pytest
import torch

import lex_cases as L
from early_exit_transformer_amd import lexicon
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.lexicon import Lexicon, apply_lex

pytestmark = pytest.mark.gpu

SHARE = lexicon.BLOCK_WORDS  # lexicon words of one workgroup when few queries leave the lexicon to be split (include/eec.h)


def _nearest(lex, words):
    index, distance = lex.nearest(words)
    assert index.dtype == distance.dtype == torch.int32 and index.is_cuda and index.shape == distance.shape == (len(words),)
    return list(zip(index.cpu().tolist(), distance.cpu().tolist()))


@pytest.fixture(scope="module")
def fixture():
    fx = L.load_fixture()
    fx["lex"] = Lexicon(fx["lexicon"])
    return fx


def test_the_fixture_string_for_string(fixture):
    lex, inputs, outputs = fixture["lex"], fixture["inputs"], fixture["outputs"]
    for text, want in zip(inputs, outputs):
        assert lex.apply(text) == want, text
    before = lex.launches
    assert lex.apply_batch(inputs) == outputs
    assert lex.launches == before + 1  # the whole list: one search
    words = list(fixture["lexicon"])
    for text, want in list(zip(inputs, outputs))[:4]:
        assert apply_lex(text, words) == want
        assert apply_lex(text, lex) == want
    assert lexicon.as_lexicon(words) is lexicon.as_lexicon(words)  # a plain list is packed once
    assert "" not in lex  # the real lexicon has no blank line, so the empty words of "" and " " are searched too


def test_query_lengths_across_every_vector_width_and_carry():
    words = L.boundary_lexicon()
    assert len(words) == 512 and {0, 1, 69, 100} <= {len(w) for w in words}
    queries = L.boundary_queries(words)
    assert tuple(len(q) for q in queries) == L.QUERY_LENGTHS
    lex = Lexicon(words)
    want = [L.nearest_ref(q, words) for q in queries]
    assert _nearest(lex, queries) == want  # one call: the longest query puts all of them through the widest kernel
    for q, w in zip(queries, want):           # each alone: through the kernel of its own width
        assert _nearest(lex, [q]) == [w], len(q)
    short = [q for q in queries if len(q) <= 64]
    assert _nearest(lex, short) == want[:len(short)]


@pytest.fixture(scope="module")
def sized():
    words = L.random_lexicon(4099, seed=21, lengths=range(1, 9), letters="abcde")
    queries = ["", "abcab", words[4098], "eeeeeeeeee"]
    ref = {}  # per query: the running first minimum over every prefix of the lexicon
    for q in queries:
        best, run = (-1, 1 << 30), []
        for i, w in enumerate(words):
            d = L.levenshtein(q, w)
            if d < best[1]:
                best = (i, d)
            run.append(best)
        ref[q] = run
    return words, queries, ref


@pytest.mark.parametrize("n_words", [1, 63, 64, 65, SHARE - 1, SHARE, SHARE + 1, 2 * SHARE + 1, 4099])
def test_lexicon_sizes_around_a_wave_and_a_workgroup(sized, n_words):
    words, queries, ref = sized
    lex = Lexicon(words[:n_words])
    for qs in (queries[:3], queries):  # Q = 3 and 4
        assert _nearest(lex, qs) == [ref[q][n_words - 1] for q in qs]


def test_ties_go_to_the_lowest_index_and_runs_are_identical():
    words, expected = L.tie_lexicon(SHARE)
    order = sorted(range(len(words)), key=lambda i: len(words[i]))  # stable, as the packer's
    place = {i: s for s, i in enumerate(order)}
    copies = [i for i, w in enumerate(words) if w == "tie"]
    assert copies == [0, len(words) // 2, len(words) - 1]
    assert len({place[i] // SHARE for i in copies}) == 3 and len({place[i] // 64 for i in copies}) == 3
    near = [i for i, w in enumerate(words) if w in ("qqaq", "qqbq", "qqcq", "qqdq")]
    assert len({place[i] // 64 for i in near}) >= 2
    lex = Lexicon(words)
    queries = list(expected)
    want = [L.nearest_ref(q, words) for q in queries]
    assert [w[0] for w in want] == [expected[q] for q in queries]
    a = torch.stack(lex.nearest(queries)).cpu()
    b = torch.stack(lex.nearest(queries)).cpu()
    assert torch.equal(a, b)
    assert list(zip(*a.tolist())) == want


def test_words_of_the_lexicon_find_themselves_through_the_kernel(fixture):
    lex, words = fixture["lex"], fixture["lexicon"]
    rng = random.Random(3)
    picks = [rng.randrange(len(words)) for _ in range(60)] + [0, len(words) - 1, max(range(len(words)), key=lambda i: len(words[i]))]
    got = _nearest(lex, [words[i] for i in picks])
    assert got == [(words.index(words[i]), 0) for i in picks]
    dup = Lexicon(["abc", "xyz", "abc", "", "xyz", ""])
    assert _nearest(dup, ["xyz", "abc", ""]) == [(1, 0), (0, 0), (3, 0)]


def test_queries_of_unknown_symbols_only():
    words = L.boundary_lexicon()
    for w in (words, [w for w in words if w]):  # with and without empty entries
        lex = Lexicon(w)
        queries = ["1", "12", "#" * 5, "€" * 33, "é" * 70, "0" * 256]
        want = []
        for q in queries:  # nothing matches: the distance to a word is max(m, its length), the first minimum wins
            d = [max(len(q), len(x)) for x in w]
            want.append((d.index(min(d)), min(d)))
        assert _nearest(lex, queries) == want
        assert all(dist == len(q) and len(w[i]) <= len(q) for q, (i, dist) in zip(queries, want))


@pytest.fixture(scope="module")
def counted():
    """A 16 000-word lexicon and, once, the oracle's answers for five distinct queries."""
    words = L.random_lexicon(16000, seed=31, lengths=range(1, 7), letters="abcd")
    distinct = ["abdc", "", "dddddddd", words[15999] + "a", "ca"]
    return words, distinct, {q: L.nearest_ref(q, words) for q in distinct}


def test_query_counts(counted):
    words, distinct, want = counted
    lex = Lexicon(words)
    none = lex.nearest([])
    assert lex.launches == 0 and all(t.shape == (0,) and t.dtype == torch.int32 and t.is_cuda for t in none)
    assert _nearest(lex, distinct[:1]) == [want[distinct[0]]]  # Q = 1: the lexicon is split over the whole grid
    rng = random.Random(32)
    many = [rng.choice(distinct) for _ in range(300)]  # several chunks of the lexicon per workgroup
    assert _nearest(lex, many) == [want[q] for q in many]
    assert lex.launches == 2


@pytest.mark.parametrize("n_queries", [lexicon.TILE_SWITCH - 1, lexicon.TILE_SWITCH, lexicon.TILE_SWITCH + 3])
def test_query_counts_on_both_sides_of_the_wide_tile(counted, n_queries):
    """From ``EEC_LEX_TILE_SWITCH`` queries on the 32-bit kernel advances 8 queries per workgroup instead of 4: the last call of
    the narrow form, the first of the wide one, and a count that leaves the wide form's last tile short (3 of 8)."""
    words, distinct, want = counted
    assert lexicon.TILE_SWITCH % 8 == 0 and max(len(q) for q in distinct) <= 32
    lex = Lexicon(words)
    rng = random.Random(n_queries)
    many = [rng.choice(distinct) for _ in range(n_queries)]
    assert _nearest(lex, many) == [want[q] for q in many]
    assert lex.launches == 1


def test_on_a_stream_of_the_callers(fixture):
    lex = fixture["lex"]
    queries = ["quik", "jumpd", "wor1d", ""]
    want = _nearest(lex, queries)
    assert lex.last_stream == torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(side):
        index, distance = lex.nearest(queries)
    assert lex.last_stream == side.cuda_stream  # the handle the launch was given: the caller's stream, not the default one
    side.synchronize()
    assert list(zip(index.cpu().tolist(), distance.cpu().tolist())) == want


def test_ctc_cuda_predict_carries_the_snapped_text(fixture):
    lex = fixture["lex"]
    V, letters = 32, " " + L.LETTERS  # id 0 is the blank; id 1 the space
    logp = torch.log_softmax(torch.randn(3, 40, V, generator=torch.Generator().manual_seed(9)) * 3.0, -1).cuda()
    detok = lambda ids: "".join(letters[i - 1] if 1 <= i <= len(letters) else "?" for i in ids)  # noqa: E731
    inf = BeamInference()
    plain = inf.ctc_cuda_predict(logp, beam_size=4)
    before = lex.launches
    both = inf.ctc_cuda_predict(logp, beam_size=4, lexicon=lex, detokenize=detok)
    assert lex.launches <= before + 1
    for (p,), (h,) in zip(plain, both):
        assert h.tokens == p.tokens and h.score == p.score and p.text is None and p.words == []
        assert h.text == lex.apply(detok(h.tokens)) and h.words == h.text.split(" ")
        assert all(w in lex for w in h.words)


def test_decode_batch_carries_the_snapped_text(fixture):
    """``decode_batch(..., lexicon=, detokenize=)``: the same token lists as without, each with the ``apply_lex``-ed text of
    its detokenised ids, all E x B texts through one lexicon search."""
    import os
    import sys

    import numpy as np

    from conftest import GOLDEN
    from early_exit_transformer_amd import synth
    from early_exit_transformer_amd.beam import DecodedTokens
    from early_exit_transformer_amd.model import full_conformer
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=int(z["n_dec_layers"]), **eval(str(z["kwargs"]))).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    fc = fc.cuda()
    lex = fixture["lex"]
    chars = " " + L.LETTERS
    detok = lambda ids: "".join(chars[i % len(chars)] for i in ids[1:])  # noqa: E731  (ids[0] is SOS)
    args = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=0.6, beam_size=3)
    spec, vlen = synth.synth_mel(2, 80, 131, seed=4).cuda(), torch.tensor([131, 120])
    inf = BeamInference()
    plain = inf.decode_batch(fc, spec, vlen, **args)
    before = lex.launches
    both = inf.decode_batch(fc, spec, vlen, lexicon=lex, detokenize=detok, **args)
    assert lex.launches == before + 1
    assert both == plain and not any(isinstance(ids, DecodedTokens) for row in plain for ids in row)
    for row in both:
        for ids in row:
            assert isinstance(ids, DecodedTokens) and ids.text == lex.apply(detok(ids))
            assert all(w in lex for w in ids.text.split(" "))
    assert inf.decode_batch(fc, spec, vlen, lexicon=lex, **args) == plain  # one of the two alone: nothing changes
