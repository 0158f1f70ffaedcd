"""CPU tests of the CTC prefix scorer behind one-pass joint CTC / attention decoding: the float64 statement
(tests/ctc_prefix_cases.py) against a brute-force enumeration of all paths and against ``F.ctc_loss``; ``CtcPrefixSession``'s host
path and ``BeamInference.joint_search_batch`` (over a stub decoder session) against the statement; the new keyword and symbols; the
argument checks of the C entries, which run before any device call."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_prefix_cases as P
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference

NINF = float("-inf")


def emission(T, V, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, V, generator=g, dtype=torch.float64) * scale, -1)


def close(a, b, tol):
    return (a == NINF and b == NINF) or (a != NINF and b != NINF and abs(a - b) <= tol)


def test_the_statement_equals_the_brute_force_over_all_paths():
    worst, cases = 0.0, 0
    rng = np.random.RandomState(5)
    for case in range(30):
        T, V = int(rng.randint(1, 7)), int(rng.randint(2, 5))
        blank = int(rng.choice([0, V - 1]))
        x = emission(T, V, float(rng.choice([1.0, 3.0])), 100 + case).numpy()
        labelling, prefix, rn, rb = P.brute_force(x, T, blank)
        labels = [c for c in range(V) if c != blank]
        root = P.begin(x, T, blank)
        todo = [((), root)]
        for depth in range(4):
            nxt = []
            for g, h in todo:
                want = [P.log_or_ninf(prefix.get(g, 0.0)), P.log_or_ninf(labelling.get(g, 0.0))]
                got = [h.pfx, P.full(h, T)]
                for t in range(T):
                    want += [P.log_or_ninf(rn.get((g, t), 0.0)), P.log_or_ninf(rb.get((g, t), 0.0))]
                    got += [h.rn[t], h.rb[t]]
                for a, b in zip(got, want):
                    assert close(a, b, 1e-12), (case, T, V, blank, g, a, b)
                    if a != NINF:
                        worst = max(worst, abs(a - b))
                cases += 1
                every = P.psi_all(h, x, T, blank)
                for c in range(V):  # the vectorised psi the search statement ranks is extend's
                    assert close(float(every[c]), P.extend(h, x, T, blank, c)[0], 1e-12), (case, g, c)
                if depth < 3:
                    nxt += [(g + (c,), P.extend(h, x, T, blank, c)[1]) for c in labels]  # repeated labels included
            todo = nxt
        assert P.extend(root, x, T, blank, blank)[0] == NINF
    print(f"{cases} prefixes, worst difference {worst:.3g}")


def test_the_full_sequence_score_is_minus_the_ctc_loss():
    T, V = 40, 29
    x = emission(T, V, 2.0, 29)
    for labels in ([5, 5, 17, 1, 28, 9, 9], [3], [7, 7, 7, 7]):
        h = P.begin(x.numpy(), T, 0)
        for c in labels:
            h = P.extend(h, x.numpy(), T, 0, c)[1]
        loss = F.ctc_loss(x.unsqueeze(1), torch.tensor([labels]), torch.tensor([T]), torch.tensor([len(labels)]), blank=0, reduction="none")
        assert abs(P.full(h, T) + float(loss[0])) <= 1e-9, labels


def test_the_host_path_stays_within_the_bound_of_the_statement():
    from early_exit_transformer_amd.model import ctc_prefix_session
    V, Tq = 8, 12
    xs = [emission(Tq, V, 2.0, 40 + i).float() for i in range(3)]
    em_len = [12, 9, 5]
    for w, min_length in ((0.3, 0), (1.0, 3)):
        res = P.scripted(lambda: ctc_prefix_session(torch.stack(xs), torch.tensor(em_len), 4, w, 1, 2, blank=0, min_length=min_length), xs, em_len,
                       V, w, 1, 2, 0, min_length)
        print(f"w = {w}: worst error / bound = {P.assert_within_bound(res):.3g}")
        done_rows = res[3][1][0]  # step 3: row 0 is the done beam: PAD alone
        assert done_rows[0, 2] == 0.0 and (np.delete(done_rows[0], 2) == NINF).all()
        if min_length:
            assert (res[2][1][:, :, 1] == NINF).all() and (res[3][1][0, 1:, 1] != NINF).any()


class StubSession:
    """A batch session that returns fixed pseudo-random log-probs: step s, whatever the tokens."""
    max_beams = 16

    def __init__(self, E, B, V, steps, seed):
        self.E, self.B, self.V, self.dev, self.s = E, B, V, torch.device("cpu"), 0
        g = torch.Generator().manual_seed(seed)
        self.table = torch.log_softmax(torch.randn(steps, E, B, self.max_beams, V, generator=g) * 2.0, -1)

    def step(self, last, parent=None):
        self.s += 1
        return self.table[self.s - 1, :, :, : last.size(-1)].contiguous()


class StubModel:
    def __init__(self, *a):
        self.a = a

    def decoder_batch_session(self, taps, layer_ns, max_length):
        return StubSession(*self.a)


def test_the_search_equals_the_statements_search_over_a_stub_decoder():
    E, B, V, Tq, beam, L, alpha = 2, 10, 8, 10, 4, 6, 0.6
    sos, eos, pad = 7, 1, 2
    g = torch.Generator().manual_seed(11)
    em = torch.log_softmax(torch.randn(E, B, Tq, V, generator=g) * 2.0, -1)
    em_len = torch.tensor([10, 10, 9, 8, 7, 6, 5, 4, 3, 2])
    n = E * B
    for w in (0.3, 1.0):
        found = BeamInference().joint_search_batch(StubModel(E, B, V, L, 23), None, [1, 2], em, em_len, w, L, vocab_size=V, SOS_token=sos,
                                                   EOS_token=eos, PAD_token=pad, beam_size=beam, pen_alpha=alpha)
        stub = StubSession(E, B, V, L, 23)

        def step(last, parent):
            return stub.step(torch.tensor(last).view(E, B, -1)).reshape(n, -1, V).double().numpy()
        want = P.joint_search([em[i // B, i % B].double().numpy() for i in range(n)], em_len.repeat(E).tolist(), step, n, w, sos, eos, pad, beam,
                              alpha, L)
        clear = [i for i in range(n) if want[i]["margin"] > 2 * P.bound(want[i]["T"], want[i]["M"])]
        assert len(clear) >= 0.9 * n, f"the statement alone pins {len(clear)} of {n} searches"
        pinned = 0
        for i in range(n):
            ft, fs, best = found[i % B][i // B]
            rows = [t.tolist() for t in ft]
            for row in rows:  # after EOS only PAD
                if eos in row:
                    assert all(t == pad for t in row[row.index(eos) + 1:]), row
            if i not in clear:
                continue
            pinned += 1
            b = P.bound(want[i]["T"], want[i]["M"])
            for r in range(beam):
                ws = want[i]["scores"][r]
                assert close(float(fs[r]), ws, 2 * L * b), (w, i, r)
                if ws != NINF:
                    assert rows[r] == want[i]["tokens"][r], (w, i, r)
            assert best == want[i]["best"], (w, i)
        print(f"w = {w}: {pinned} of {n} searches pinned")
        assert pinned >= 0.75 * n


def test_with_weight_one_the_search_finds_the_most_likely_labelling():
    """w = 1, beam 16, T = 5, V = 3 (blank 0, EOS 1, PAD 2; the CTC head gives EOS probability zero, so every labelling it can
    produce is one the search can spell), no length penalty: the best hypothesis is the brute-force argmax."""
    T, V, L = 5, 3, 6
    for seed in range(4):
        g = torch.Generator().manual_seed(70 + seed)
        z = torch.randn(T, V, generator=g, dtype=torch.float64) * 2.0
        z[:, 1] = NINF
        x = torch.log_softmax(z, -1)
        labelling = P.brute_force(x.numpy(), T, 0)[0]
        ranked = sorted(labelling.items(), key=lambda kv: -kv[1])
        assert ranked[0][1] > ranked[1][1] * (1 + 1e-3), "the fixture needs a clear winner"
        found = BeamInference().joint_search_batch(StubModel(1, 1, V, L, seed), None, [1], x.float().view(1, 1, T, V), None, 1.0, L, vocab_size=V,
                                                   SOS_token=2, EOS_token=1, PAD_token=2, beam_size=16, pen_alpha=0.0)
        ft, fs, best = found[0][0]
        assert best[0] == 2 and 1 in best
        assert tuple(best[1: best.index(1)]) == ranked[0][0], (seed, best, ranked[:3])
        M = T * float(x[torch.isfinite(x)].abs().max())  # no state value exceeds the sum of T emissions
        assert abs(float(max(fs)) - math.log(ranked[0][1])) <= P.bound(T, M)


def test_keywords_and_exports():
    from early_exit_transformer_amd.model import CtcPrefixSession, ctc_prefix_session  # noqa: F401
    for name in ("eec_ctc_prefix_state_bytes", "eec_ctc_prefix_begin", "eec_ctc_prefix_step"):
        assert name in capi.EXPORTS and hasattr(capi.load(), name)
    model = types.SimpleNamespace(_cfg=types.SimpleNamespace(n_exits=2))
    inf = BeamInference()
    spec, vlen = torch.zeros(1, 80, 50), torch.tensor([50])
    with pytest.raises(ValueError, match="exclude"):
        inf.decode_batch(model, spec, vlen, ctc_weight=0.3, joint_ctc_weight=0.3)
    with pytest.raises(ValueError, match="exclude"):
        inf.decode_all_exits(model, spec[0], vlen, ctc_weight=0.3, joint_ctc_weight=0.3)
    for w in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            inf.decode_batch(model, spec, vlen, joint_ctc_weight=w)
    with pytest.raises(ValueError, match="distinct"):
        ctc_prefix_session(torch.zeros(1, 4, 8), None, 4, 0.5, 1, 1)


def test_sizing_and_argument_checks_run_without_a_device():
    lib = capi.load()
    assert lib.eec_ctc_prefix_state_bytes(3, 16, 1024) == 2 * 3 * 16 * (4 + 256 + 3 * 1024) * 4
    assert lib.eec_ctc_prefix_state_bytes(0, 16, 64) == 0
    fake, big = 4096, 1 << 40  # never dereferenced: every call below is refused before a device call
    good = dict(n=1, Tq=8, V=16, blank=0, R_max=4)

    def begin(**kw):
        a = {**good, **kw}
        return lib.eec_ctc_prefix_begin(fake, None, a["n"], a["Tq"], a["V"], a["blank"], a["R_max"], fake, a.get("bytes", big), None)

    def step(**kw):
        a = {**good, "R": 2, "R_prev": 1, "s": 1, "w": 0.5, "eos": 1, "pad": 2, **kw}
        return lib.eec_ctc_prefix_step(fake, None, a["n"], a["Tq"], a["V"], a["blank"], a["R_max"], None, fake, a["R"], a["R_prev"], a["s"], fake,
                                       a["w"], a["eos"], a["pad"], 0, fake, a.get("state", fake), a.get("bytes", big), None)
    for call in (begin, step):
        assert call(blank=16) == 10001 and call(blank=-1) == 10001 and call(Tq=0) == 10001 and call(n=-1) == 10001
        assert call(V=257, blank=0) == 10002 and call(R_max=17) == 10002 and call(Tq=2049) == 10002
        assert call(bytes=lib.eec_ctc_prefix_state_bytes(1, 4, 8) - 1) == 10003
        assert call(n=0) == 0
    for kw in (dict(eos=16), dict(pad=-1), dict(eos=2), dict(eos=0), dict(pad=0), dict(R=5), dict(R=0), dict(R_prev=5), dict(s=-1), dict(w=0.0),
               dict(w=1.5), dict(w=float("nan"))):
        assert step(**kw) == 10001, kw
    assert step(state=fake + 4) == 10003
    assert step(V=300) == 10002
