"""CPU tests of log-add merging in the lexicon CTC beam search: the host entry ``eec_ctc_log_add_host`` -- the very function the
kernel calls -- against the numpy float32 statement of tests/lexbeam_logadd_cases.py bit for bit, that statement's accuracy against
float64, the statement of the search (tests/lexbeam_statement.py) against CTC itself (the forward log-likelihood, which no beam search computed), and that the
new statement with log-add off is the Viterbi statement."""
import os

import numpy as np
import pytest

import lexbeam_cases as L
import lexbeam_logadd_cases as A
import lexbeam_statement as D
from early_exit_transformer_amd.build import LIB_PATH
from lexbeam_helpers import library

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    return library()


def host_log_add(lib, a, b):
    fn = lib.eec_ctc_log_add_host
    return np.array([fn(float(x), float(y)) for x, y in zip(a.tolist(), b.tolist())], dtype=np.float32)


def test_host_log_add_equals_the_statement_bit_for_bit(lib):
    """Over 200 000 pairs with d in [cutoff - 1, 0] at magnitudes 1e-3 .. 1e4, both argument orders, the fp32 neighbours of the
    cutoff, of d = 0, of the sqrt 2 switch and of every d where ``n`` changes, and a == b."""
    a, b = A.pair_grid()
    assert len(a) >= 200_000
    d = np.minimum(a, b).astype(np.float64) - np.maximum(a, b)
    assert d.min() < float(A.CUTOFF) - 0.9 and (d == 0).sum() >= 100 and (d == float(A.CUTOFF)).any()
    n, halved, _ = A.softplus_parts(np.clip(d, float(A.CUTOFF) + 1e-3, 0).astype(np.float32))
    assert set(np.unique(n).astype(int).tolist()) == set(range(-25, 1)) and halved.any() and not halved.all()
    want = A.log_add(a, b)
    got = host_log_add(lib, a, b)
    wrong = np.flatnonzero(A.bits(got) != A.bits(want))
    assert wrong.size == 0, (wrong[:5], a[wrong[:5]], b[wrong[:5]], got[wrong[:5]], want[wrong[:5]])
    # symmetric bit for bit; a == b adds the stated ln 2; at and below the cutoff the higher argument comes back
    assert np.array_equal(A.bits(A.log_add(b, a)), A.bits(want))
    assert lib.eec_ctc_log_add_host(-3.0, -3.0) == float(np.float32(-3.0) + A.LN2)
    assert lib.eec_ctc_log_add_host(-3.0, -3.0 + float(A.CUTOFF)) == -3.0


def test_the_stated_softplus_is_within_its_written_bound_of_float64():
    """The maximum absolute deviation of the recipe from float64 log1p(exp(d)) over 2 000 001 points of [cutoff, 0], ends
    included: below the bound include/eec.h writes, which is below 1e-6."""
    d = np.linspace(float(A.CUTOFF), 0.0, 2_000_001).astype(np.float32)
    d[0], d[-1] = A.CUTOFF, 0.0
    err = np.abs(A.softplus(d).astype(np.float64) - np.log1p(np.exp(d.astype(np.float64))))
    worst = float(err.max())
    print(f"max |softplus - fp64| = {worst:.3e} at d = {d[err.argmax()]}")
    header = open(os.path.join(os.path.dirname(LIB_PATH), "..", "..", "include", "eec.h")).read()
    assert "the bound the tests assert is 1.2e-7" in header
    assert worst <= A.ERROR_BOUND < 1e-6


@pytest.mark.parametrize("T", [3, 5, 8])
def test_the_statement_sums_to_the_ctc_forward_likelihood(T):
    """One word, beam 16, all 16 hypotheses, no threshold: nothing is pruned (no frame leaves more than 13 states -- 5 before the
    first word end, 6 after it, 2 after the second --, counted by the statement and asserted against the beam), so the log-sum of the
    returned hypotheses with a given word sequence is the CTC forward log-likelihood of its labels -- float64, no beam search --
    within 1e-5."""
    trie = L.Trie(L.ONE_WORD, 40)
    em = L.emissions(9, L.ONE_WORD, 4, T, 40)
    for s in range(4):
        stats = {}
        hyps = D.decode(em[s], trie, beam=16, nbest=16, beam_threshold=INF, log_add=True, stats=stats)
        assert stats["max_alive"] <= 13 < 16
        for words in ([0], [0, 0]):
            labels = [c for w in words for c in L.ONE_WORD[w]]
            scores = [float(h[3]) for h in hyps if h[0] == words]
            if T < len(labels) + sum(a == b for a, b in zip(labels, labels[1:])):
                assert not scores  # it does not fit into the frames
                continue
            assert scores, (T, s, words)
            got, want = float(np.logaddexp.reduce(scores)), A.ctc_forward(em[s], labels)
            print(f"T' = {T} sequence {s} words {words}: log-sum {got:.7f} CTC forward {want:.7f} difference {abs(got - want):.2e}")
            assert abs(got - want) <= 1e-5


@pytest.mark.parametrize("name", ["one", "prefix", "wide", "fixture+sil"])
def test_with_log_add_off_the_new_statement_is_the_viterbi_statement(name):
    _, words, fixture = L.load_fixture()
    spellings, V, sil = {"one": (L.ONE_WORD, 40, None), "prefix": (L.PREFIX_DOUBLED, 32, None), "wide": (L.wide_lexicon(), 256, 126),
                         "fixture+sil": (fixture, 256, 126)}[name]
    trie = L.Trie(spellings, V, 0, sil)
    em = L.emissions(31, spellings, 3, 12, V, 0, -1 if sil is None else sil)
    kw = dict(beam=6, nbest=6, word_score=-0.5, sil_score=-0.25, beam_threshold=20.0)
    want = D.decode_batch(em, trie, **kw)
    got = D.decode_batch(em, trie, log_add=False, **kw)
    assert any(want) and len(got) == len(want)
    for g, w in zip(got, want):
        assert [(h[0], h[1], h[2], int(A.bits(h[3]))) for h in g] == [(h[0], h[1], h[2], int(A.bits(h[3]))) for h in w]


def test_the_two_merge_rules_really_differ():
    """On the doubled-prefix lexicon (24 x 16 frames) and on the fixture lexicon with sil (12 x 64 frames), beam 10, the best
    transcript under log-add differs from the Viterbi one in at least 4 and at least 1 sequences."""
    _, _, fixture = L.load_fixture()
    for spellings, V, sil, n, T, least in ((L.PREFIX_DOUBLED, 32, None, 24, 16, 4), (fixture, 256, 126, 12, 64, 1)):
        trie = L.Trie(spellings, V, 0, sil)
        em = L.emissions(5, spellings, n, T, V, 0, -1 if sil is None else sil)
        vit = D.decode_batch(em, trie, beam=10)
        add = D.decode_batch(em, trie, beam=10, log_add=True)
        differ = sum(1 for v, a in zip(vit, add) if [h[0] for h in v] != [h[0] for h in a])
        print(f"V = {V}: the best transcript differs in {differ} of {n} sequences")
        assert differ >= least
