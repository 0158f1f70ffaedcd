"""CPU tests of contextual biasing: the library's graph image against the plain-Python restatement (tests/ctxbias_cases.py) bit for
bit; the builder's refusals and their messages; the closed form (naive substring count) against the automaton's fold; the restated
biased search at boost 0 against oracle/ctc_beam_ref.py; ``ContextBiasSession``'s host path against the restated step and, inside
``_lockstep_search`` with ``beam_select``'s host path, against a plain Python beam search; the declarations; and the census of the
inputs the GPU test compares on."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ctc_cases as K
import ctxbias_cases as X
import rescore_cases as RC
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import _lockstep_search, sequence_length_penalty
from early_exit_transformer_amd.context import ContextBiasSession, ContextGraph
from oracle.ctc_beam_ref import ctc_prefix_beam_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def assert_image_is(graph, g, tab):
    delta, nxt, fin = graph.tables(g)
    assert delta.shape == (tab.S, tab.V)
    assert np.array_equal(nxt.numpy(), tab.next) and np.array_equal(fin.numpy(), tab.final)
    assert same_bits(delta.numpy(), tab.delta)


def test_the_image_equals_the_restated_tables():
    states = 0
    for k, (T, V, *_rest) in enumerate(X.blocks()):
        for b in X.BOOSTS:
            graph = ContextGraph(X.block_phrases(k), X.block_boosts(k, b), vocab_size=V)
            assert_image_is(graph, 0, X.block_tables(k, b))
            states += graph.states
    # boosts that are not dyadic (the fp64 order of the sums matters), another blank, eos and pad, a duplicate phrase
    phrases = [(3, 4, 5), (3, 4), (4, 5, 3, 4), (5,), (3, 4, 5), (9, 3, 4, 5, 3)]
    boosts = [0.1, 0.7, 1.3, 0.05, 0.3, 2.2]
    for eos, pad in ((None, None), (2, None), (2, 11), (None, 11)):
        graph = ContextGraph(phrases, boosts, vocab_size=12, blank=1, eos=eos, pad=pad)
        assert_image_is(graph, 0, X.Tables(phrases, boosts, 12, blank=1, eos=eos, pad=pad))
    empty = ContextGraph([], vocab_size=7)
    assert empty.states == 1 and not empty.tables()[0].any() and not empty.tables()[1].any()
    print(f"{states} states compared")


def test_a_bank_holds_its_graphs_in_order():
    V = 32
    parts = [ContextGraph(X.block_phrases(k), X.block_boosts(k, 1.5), vocab_size=V) for k in (3, 4, 5)] + [ContextGraph([], vocab_size=V)]
    bank = ContextGraph.bank(parts)
    assert bank.n_graphs == 4 and bank.states == sum(p.states for p in parts)
    img = bank.image
    assert int(img[0]) == 0x43545847 and int(img[1]) == 4 and int(img[2]) == img.numel() and int(img[3]) == V
    for g, k in enumerate((3, 4, 5)):
        assert_image_is(bank, g, X.block_tables(k, 1.5))
    assert bank.bias_of(X.block_phrases(4)[0], graph=1) > 0 and bank.bias_of(X.block_phrases(4)[0], graph=7) == 0.0
    with pytest.raises(ValueError, match="share"):
        ContextGraph.bank([parts[0], ContextGraph([], vocab_size=7)])


def _raw(G, n_phrases, lens, toks, boosts, V=8, blank=0, eos=-1, pad=-1, image=True, short=False):
    lib = capi.load()
    a = [np.asarray(x, dtype=t) if x is not None else None for x, t in ((n_phrases, np.int32), (lens, np.int32), (toks, np.int32), (boosts, np.float64))]
    ptr = [None if x is None else x.ctypes.data for x in a]
    head = (G, *ptr, V, blank, eos, pad)
    buf = np.zeros(1 << 16, dtype=np.int32)
    size = lib.eec_context_graph_bytes(*head)
    rc = lib.eec_context_graph(*head, buf.ctypes.data if image else None, 16 if short else buf.nbytes)
    return size, rc, lib.eec_last_error().decode()


REFUSALS = {
    "blank inside a phrase": dict(lens=[2], toks=[3, 0]),
    "an empty phrase": dict(lens=[0], toks=[1]),
    "a token outside": dict(lens=[2], toks=[3, 8]),
    "a token outside [0, V)": dict(lens=[2], toks=[-1, 3]),
    "boost must be finite": dict(boosts=[float("inf")]),
    "a boost must be finite": dict(boosts=[float("nan")]),
    "must be finite and >= 0": dict(boosts=[-0.5]),
    "eos or pad inside a phrase": dict(eos=4),
    "phrase of more than 64 tokens": dict(lens=[65], toks=[1 + i % 7 for i in range(65)]),
    "1 .. 1024 graphs": dict(G=1025, n_phrases=[0] * 1025, lens=None, toks=None, boosts=None),
    "1 .. 1024": dict(G=0),
    "more than 32768 states": dict(G=1000, n_phrases=[1] * 1000, lens=[40] * 1000, toks=[1 + (i // 40 + i) % 7 for i in range(40000)], boosts=[1.0] * 1000),
    "null argument (n_phrases)": dict(n_phrases=None),
    "null argument (phrase_len, tokens, boost)": dict(toks=None),
    "1 <= V <= 256": dict(V=257),
    "blank in [0, V)": dict(blank=8),
    "other than blank": dict(eos=0),
}


@pytest.mark.parametrize("message", list(REFUSALS))
def test_the_builder_refuses_with_a_message(message):
    kw = dict(G=1, n_phrases=[1], lens=[3], toks=[3, 4, 5], boosts=[1.5])
    kw.update(REFUSALS[message])
    size, rc, err = _raw(**kw)
    assert size == 0 and rc == 10001 and message in err, (size, rc, err)


def test_the_builder_refuses_a_null_or_short_image_and_accepts_the_limits():
    ok = dict(G=1, n_phrases=[1], lens=[3], toks=[3, 4, 5], boosts=[1.5])
    size, rc, err = _raw(**ok)
    assert size == 4 * (4 + 4 + 4 * (2 * 8 + 1)) and rc == 0
    size, rc, err = _raw(**ok, image=False)
    assert size > 0 and rc == 10001 and "null argument (image)" in err
    size, rc, err = _raw(**ok, short=True)
    assert rc == 10003 and "image too small" in err
    size, rc, err = _raw(G=1, n_phrases=[1], lens=[64], toks=[1 + i % 7 for i in range(64)], boosts=[0.0])  # 64 tokens, boost 0: allowed
    assert size > 0 and rc == 0


def test_the_closed_form_equals_the_fold_of_the_automaton():
    """Random rows over a small alphabet, so that overlapping ((1, 2, 1) in 1 2 1 2 1) and nested ((2, 1) inside (1, 2, 1, 3)) occurrences
    are frequent; with eos / pad the row's bias stops at the first of them."""
    phrases = [(1, 2, 1), (2, 1), (1, 2, 1, 3), (3, 3), (1,), (2, 1, 3, 3, 2)]
    boosts = [1.5, 0.75, 4.0, 2.0, 0.5, 1.25]
    rng = np.random.RandomState(2)
    hits = 0
    for eos, pad in ((None, None), (5, 6)):
        tab = X.Tables(phrases, boosts, 7, eos=eos, pad=pad)
        graph = ContextGraph(phrases, boosts, vocab_size=7, eos=eos, pad=pad)
        for case in range(300):
            hi = 4 if eos is None or case % 2 else 7
            row = [int(t) for t in rng.randint(0 if case % 3 == 0 else 1, hi, size=rng.randint(0, 14))]
            want = X.closed_form(tab, row)
            assert float(X.bias32(tab, row)) == want == graph.bias_of(row), (row, X.bias32(tab, row), want, graph.bias_of(row))
            hits += want > 0
    assert hits > 300
    # a token shared by several phrases carries the largest of their boosts: node (1) lies on (1, 2, 1, 3), whose boost is 4.0
    assert graph.score_of((1, 2, 1, 3)) == 4 * 4.0 and graph.score_of((1,)) == 4.0 and graph.score_of((2, 1)) == 1.25 + 1.25
    # overlapping and nested, by hand: 1 2 1 2 1 3 holds (1, 2, 1) twice, (2, 1) twice, (1, 2, 1, 3) once and (1,) three times
    want = 2 * graph.score_of((1, 2, 1)) + 2 * graph.score_of((2, 1)) + graph.score_of((1, 2, 1, 3)) + 3 * graph.score_of((1,))
    assert graph.bias_of([1, 2, 1, 2, 1, 3]) == want == float(X.bias32(tab, [1, 2, 1, 2, 1, 3]))
    assert graph.bias_of([1, 2, 5, 1, 2, 1]) == graph.bias_of([1, 2]) == 4.0  # cut at eos: (1,) once; the open (1, 2) pays nothing


def test_boost_zero_reproduces_the_oracle_search():
    for k, (T, V, scale, logp, lens, plain) in enumerate(X.blocks()):
        if V > 32:
            continue
        for s in range(logp.size(0)):
            x = logp[s].double().numpy()
            for tab in (None, X.block_tables(k, 0.0)):
                got = X.biased_beam_search(x, tab)
                assert [(p, t) for p, t, _, _ in got] == [(p, t) for p, t in plain[s]]
                assert all(b == 0.0 and key == t for _, t, b, key in got)
    x = X.blocks()[4][3][1].double().numpy()
    for beam, skip in ((10, True), (5, False), (1, True)):
        want = ctc_prefix_beam_search(x, beam=beam, return_beams=True, skip_drops_frame=skip)[2]
        got = X.biased_beam_search(x, X.block_tables(4, 0.0), beam=beam, skip_drops_frame=skip)
        assert [(p, t) for p, t, _, _ in got] == [(p, t) for p, t in want]


def test_the_inputs_separate_the_ranks_and_move_the_best_hypothesis():
    """A condition on the inputs, not a measurement: over every (sequence, rank < 4) pair the share of ranks whose consecutive key gaps
    in the fp64 restatement all exceed BEAM_MARGIN is at least MIN_COMPARED, and at boost 1.5 the best hypothesis differs from the
    unbiased one in at least a quarter of the sequences (else no test could tell a biased search from an unbiased one)."""
    for with_len in (False, True):
        for b in X.BOOSTS:
            if with_len and b == 0.0:
                continue
            compared = present = changed = n = 0
            for k, rows in enumerate(X.restated_beams(b, with_len)):
                for s, final in enumerate(rows):
                    present += min(X.NBEST, len(final))
                    compared += len(X.comparable_ranks(final))
                    n += 1
                    changed += final[0][0] != X.blocks()[k][5][s][0][0]
                    for p, _, fb, _ in final:
                        assert fb == float(X.bias32(X.block_tables(k, b), p)) == X.closed_form(X.block_tables(k, b), p)
            print(f"own lengths {with_len}, b = {b}: {compared} of {present} ranks comparable, best changed in {changed} of {n}")
            assert compared >= RC.MIN_COMPARED * present
            if not with_len:
                assert changed == 0 if b == 0.0 else 4 * changed >= n


def _host_session_against_the_restated_step(graph, tabs, graph_of, n, V, rows, seed):
    g = torch.Generator().manual_seed(seed)
    sess = ContextBiasSession(graph, n, max(rows), graph_of)
    state, last, parent, R_prev = None, torch.ones((n, 1), dtype=torch.long), None, 0
    for s, R in enumerate(rows):
        R_in = last.size(1)
        local = torch.randn(n, R_in, V, generator=g)
        local[torch.rand(n, R_in, V, generator=g) < 0.2] = NEG
        got = sess.step(local, last, parent)
        want, state = X.aed_step(tabs, None if graph_of is None else graph_of.tolist(), state, None if parent is None else parent.tolist(),
                                 last.tolist(), local.numpy(), s, R_prev)
        assert same_bits(got.numpy(), want) and sess.states().tolist() == state, s
        R_prev = R_in
        parent = torch.randint(-1, R_in + 1, (n, R), generator=g)  # -1 and R_in: outside the range, the state goes back to the root
        last = torch.randint(-1, V + 1, (n, R), generator=g)
    return sess


def test_the_host_step_equals_the_restated_step():
    V = 7
    phrases = [(1, 2, 1), (2, 1), (1, 2, 1, 3), (3, 3)]
    kinds = [([1.5, 0.75, 4.0, 2.0], phrases), ([0.3, 0.1], phrases[:2]), ([], [])]
    graphs = [ContextGraph(p, b, vocab_size=V, eos=5, pad=6) for b, p in kinds]
    tabs = [X.Tables(p, b, V, eos=5, pad=6) for b, p in kinds]
    _host_session_against_the_restated_step(graphs[0], tabs[:1], None, 3, V, [4, 1, 16, 5, 5, 2], 1)
    _host_session_against_the_restated_step(ContextGraph.bank(graphs), tabs, torch.tensor([2, 0, -1, 1, 3]), 5, V, [3, 3, 7, 2], 2)


def test_a_biased_lockstep_search_on_the_host_equals_a_plain_python_beam_search():
    """A toy decoder whose next-token log-probs depend on the step and the last token (so that two orders of the same tokens do not
    tie); ``_lockstep_search`` with ``ContextBiasSession`` and ``beam_select`` on CPU tensors against a beam search written out in
    Python over the restated tables (fp32 adds in the same order); at alpha 0 every final score is the unbiased score of its tokens
    plus their bias."""
    V, beam, steps, sos, eos, pad, n = 9, 4, 7, 1, 2, 8, 3
    g = torch.Generator().manual_seed(11)
    table = torch.log_softmax(torch.randn(n, steps, V, V, generator=g) * 1.5, -1)
    phrases, boosts = [(3, 4), (4, 3, 4), (5, 5), (3, 4, 6)], [1.5, 0.75, 4.0, 2.0]
    graph = ContextGraph(phrases, boosts, vocab_size=V, eos=eos, pad=pad)
    tab = X.Tables(phrases, boosts, V, eos=eos, pad=pad)

    def stepper():
        at = iter(range(steps))

        def step(last, parent):
            k = next(at)
            return torch.stack([table[i, k][last[i]] for i in range(n)])
        return step
    moved = 0
    for alpha in (0.0, 0.6):
        found = _lockstep_search(stepper(), n, torch.device("cpu"), steps, sos, beam, alpha, scorers=[ContextBiasSession(graph, n, beam)])
        plain = _lockstep_search(stepper(), n, torch.device("cpu"), steps, sos, beam, alpha)
        for i in range(n):
            beams = [([sos], np.float32(0.0), 0)]
            for k in range(steps):
                pen = np.float32(sequence_length_penalty(k + 1, alpha))
                cands = []
                for toks, sc, st in beams:
                    row = table[i, k][toks[-1]].numpy()
                    for v in range(V):
                        x = np.float32(row[v] + tab.delta[st, v])
                        cands.append((np.float32(sc + np.float32(x / pen)), toks + [v], int(tab.next[st, v])))
                cands.sort(key=lambda c: -c[0])
                beams = [(t, s, st) for s, t, st in cands[:beam]]
            # every row is final as it stands: the bonus of an open partial match is given back, at the last step's penalty
            beams = [(t, np.float32(s + np.float32(tab.final[st] / pen)), st) for t, s, st in beams]
            tokens, scores, best = found[i]
            assert [t.tolist() for t in tokens] == [t for t, _, _ in beams]
            assert np.allclose([float(s) for s in scores], [float(s) for _, s, _ in beams], rtol=0, atol=1e-5)
            assert best == max(beams, key=lambda e: e[1])[0]
            moved += best != plain[i][2]
            if alpha == 0.0:
                for t, s in zip(tokens, scores):
                    t = t.tolist()
                    own = sum(float(table[i, k][a, b]) for k, (a, b) in enumerate(zip(t[:-1], t[1:])))
                    assert abs(float(s) - own - graph.bias_of(t[1:])) < 1e-4
    assert moved >= 1


def test_the_entries_are_declared_and_exported():
    lib = capi.load()
    names = ["eec_context_graph_bytes", "eec_context_graph", "eec_ctc_beam_decode_ctx", "eec_ctc_beam_decode_nbest_ctx",
             "eec_context_bias_state_bytes", "eec_context_bias_step"]
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    assert "Contextual biasing" in header and lib.eec_abi_version() == 16
    for name in names:
        assert name in capi.EXPORTS and getattr(lib, name).argtypes is not None
        assert re.search(r"\b" + name + r"\(", header), name
    assert len([e for e in capi.EXPORTS if e.endswith("_last_error")]) == len(set(re.findall(r"\beec_\w*last_error\b", header)))
    import early_exit_transformer_amd as pkg
    assert pkg.ContextGraph is ContextGraph and pkg.ContextBiasSession is ContextBiasSession
    # the device entries refuse before any device work
    assert lib.eec_context_bias_step(None, 0, None, 1, 1, 1, 4, 7, 0, None, None, None, None, None, 0, None) == 10001
    assert "null argument" in lib.eec_last_error().decode()
    assert lib.eec_context_bias_step(None, 0, None, 1, 5, 1, 4, 7, 0, None, None, None, None, None, 0, None) == 10001
    assert lib.eec_context_bias_step(None, 0, None, 0, 1, 1, 4, 7, 0, None, None, None, None, None, 0, None) == 0
    assert lib.eec_context_bias_state_bytes(3, 16) == 2 * 3 * 16 * 4
    assert lib.eec_ctc_beam_decode_ctx(None, None, 1, 5, 7, 0, 4, 0.95, 0, None, None, None, None, None, 0, None, None, None) == 10001
    assert "eec_ctc_beam_decode_ctx: null argument" in lib.eec_last_error().decode()
