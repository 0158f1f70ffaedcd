"""CPU checks of the CTC forced alignment's yardsticks: the restated semantics (tests/align_cases.py) against the fixture the
reference's own get_trellis / backtrack produced (tests/golden/ctc_align.npz), the inclusion condition of the path comparison,
the claim that the +inf cells are never read, the two new C-ABI symbols, and the joint-score formula of ``ctc_rescore``."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import align_cases as A
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.build import LIB_PATH


@pytest.fixture(scope="module")
def fixture():
    return A.load_fixture()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_equals_the_reference_fixture(fixture, dtype):
    """Fixture (the reference, fp32 on the CPU) and the restatement in ``dtype`` against the fp64 restatement: trellis within
    ``bound`` with the infinities in the same cells, path identical where the margin clears ``2 * bound``, scores within their
    bound.  At most a quarter of the cases may fall under the margin."""
    pinned = []
    for name, c in fixture.items():
        em, T = c["em"].numpy(), c["em"].size(0)
        tr64, path64, margin64, ok = A.align_ref(em, c["tok"], c["blank"], np.float64)
        assert ok and tr64.shape == (T + 1, len(c["tok"]) + 1), name
        assert math.isclose(margin64, c["margin"], rel_tol=1e-9, abs_tol=1e-12), (name, margin64, c["margin"])
        assert c["path"][0][0] == 0 and c["path"][-1][1] == T - 1, name
        pinned.append(A.compare(name, c["trellis"], c["path"], tr64, path64, margin64, T))
        tr, path, _, ok = A.align_ref(em, c["tok"], c["blank"], dtype)
        assert ok, name
        A.compare(name + "-restated", tr, path, tr64, path64, margin64, T)
        if pinned[-1]:
            assert [(j, t) for j, t, _ in path] == [(j, t) for j, t, _ in c["path"]], name
    print(f"{sum(pinned)} of {len(pinned)} cases clear 2 * bound")
    assert len(pinned) == 34 and sum(pinned) >= math.ceil(0.75 * len(pinned)), pinned


def test_quirks_show_in_the_fixture(fixture):
    """blank_id = 3: column 0 is the running sum of em[:, 0] (not em[:, 3]) and a stay adds em[t, 0] to the score."""
    c = fixture["blank3"]
    em, tr, T, N = c["em"].numpy(), c["trellis"], c["em"].size(0), len(c["tok"])
    first_inf = T + 1 - N
    want = np.cumsum(em[:, 0].astype(np.float64))[: first_inf - 1]
    assert np.abs(tr[1:first_inf, 0] - want).max() <= A.bound(T, tr[np.isfinite(tr)])
    assert np.abs(want - np.cumsum(em[:, 3].astype(np.float64))[: first_inf - 1]).max() > 1.0
    assert np.isposinf(tr[first_inf:, 0]).all() and np.isneginf(tr[0, 1:]).all()
    for j in range(N + 1):  # the +inf cells: rows >= T + 1 - N + j
        assert np.isposinf(tr[min(first_inf + j, T + 1):, j]).all() and np.isfinite(tr[max(j, 1):first_inf + j, j]).all(), j
    steps = {t: s for _, t, s in c["path"]}
    stays = [t for (j, t, _), (j2, _, _) in zip(c["path"][1:], c["path"][:-1]) if j == j2]
    assert stays, "the case has no stay"
    for t in stays:
        step = steps[t] - steps.get(t + 1, 0.0)
        assert abs(step - em[t, 0]) <= 1e-4 * max(1.0, abs(steps[t])) and abs(em[t, 0] - em[t, 3]) > 1e-3, t


def test_inf_cells_are_never_read_by_the_backtrack(fixture):
    for name, c in fixture.items():
        em = c["em"].numpy()
        tr = A.trellis_ref(em, c["tok"], c["blank"], np.float32)
        want = A.backtrack_ref(tr, em, c["tok"], c["blank"], np.float32)
        hole = np.isposinf(tr)
        assert hole.sum() >= len(c["tok"]), name
        for fill in (-1e30, 0.0, 1e30, np.nan):
            tr2 = tr.copy()
            tr2[hole] = fill
            got = A.backtrack_ref(tr2, em, c["tok"], c["blank"], np.float32)
            assert got[0] == want[0] and got[2], (name, fill)


def test_alignment_symbols_are_exported_and_size_without_a_device(lib):
    for sym in ("eec_ctc_align_workspace_bytes", "eec_ctc_align"):
        assert sym in capi.EXPORTS and hasattr(lib, sym)
    base = (3840, 256, 85)
    size = lambda *a: lib.eec_ctc_align_workspace_bytes(*a)  # noqa: E731
    for i in range(3):
        prev = None
        for v in (1, 2, 64, 255, 1024, 4096):
            args = list(base)
            args[i] = v
            n = size(*args)
            assert prev is None or n >= prev, (i, v, n, prev)
            prev = n


def test_alignment_rejects_bad_arguments_before_touching_a_device(lib):
    """Every one of these returns before a launch (no GPU is needed); the pointers are never dereferenced on the host."""
    p = C.c_void_p(256)  # a non-null placeholder

    def call(logp=p, n_em=1, Tq=8, V=16, tokens=p, tok_len=p, n_hyp=1, tok_stride=4, blank=0, outs=(p, p, p, p, p)):
        return lib.eec_ctc_align(logp, n_em, Tq, V, None, tokens, tok_len, None, n_hyp, tok_stride, blank, *outs, None, None, None)
    BAD, UNSUPPORTED = 10001, 10002
    assert call(n_hyp=0) == 0  # a successful no-op
    assert call(n_hyp=0, logp=None, tokens=None, tok_len=None, outs=(None,) * 5) == 0
    assert call(logp=None) == BAD and call(tokens=None) == BAD and call(tok_len=None) == BAD
    for i in range(5):
        assert call(outs=tuple(None if k == i else p for k in range(5))) == BAD, i
    assert call(blank=-1) == BAD and call(blank=16) == BAD
    assert call(tok_stride=0) == BAD and call(n_hyp=-1) == BAD and call(Tq=0) == BAD
    assert call(tok_stride=256) == UNSUPPORTED  # more than 255 tokens
    assert call(Tq=1 << 20) == UNSUPPORTED       # decisions do not fit the LDS


def test_joint_score_formula_on_hand_made_scores():
    """``ctc_rescore``'s arithmetic (util/beam_infer.py:350-378): s_ctc = exp(path score / tokens), s_pred = exp(score), each over
    its own maximum, mixed by the weight; argmax with ties to the lower index; an unalignable beam has s_ctc = 0."""
    from early_exit_transformer_amd.beam import _first_argmax, _joint_scores
    path = torch.tensor([-30.0, -12.0, -45.0, -math.inf])
    status = torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    lens = torch.tensor([10, 6, 9, 12], dtype=torch.int32)
    pred = torch.tensor([-1.0, -3.0, -0.5, -0.25])
    for w in (0.0, 0.3, 0.7, 1.0):
        s_ctc = [math.exp(-3.0), math.exp(-2.0), math.exp(-5.0), 0.0]
        s_pred = [math.exp(v) for v in pred.tolist()]
        want = [w * c / max(s_ctc) + (1 - w) * p / max(s_pred) for c, p in zip(s_ctc, s_pred)]
        got = _joint_scores(path, status, lens, pred, w)
        assert torch.allclose(got, torch.tensor(want), rtol=1e-6, atol=1e-7), (w, got, want)
        assert int(_first_argmax(got)) == int(np.argmax(want))
    assert int(_first_argmax(_joint_scores(path, status, lens, pred, 0.0))) == 3   # the decoder's best
    assert int(_first_argmax(_joint_scores(path, status, lens, pred, 1.0))) == 1   # the best CTC alignment per token
    # ties go to the lower index, batched over a leading dimension
    assert _first_argmax(torch.tensor([[1.0, 2.0, 2.0], [3.0, 3.0, 1.0], [0.0, 0.0, 0.0]])).tolist() == [1, 0, 0]
    # every beam failed: s_ctc stays 0 (no 0 / 0), the decoder's order decides
    dead = _joint_scores(torch.full((4,), -math.inf), torch.ones(4, dtype=torch.int32), lens, pred, 0.5)
    assert torch.isfinite(dead).all() and int(_first_argmax(dead)) == 3
