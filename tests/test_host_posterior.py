"""CTC posteriors in the standard topology without a device: the fp64 restatement of tests/posterior_cases.py against a brute force
over all frame labellings and against torch's fp64 CTC loss and its gradient, the identities of every served row, the NumPy host path
of ``ctc_posteriors`` against the restatement, a planted labelling against ``ctc_forced_align``, the span layer, and the refusals of
the package and of the library's entry."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import forced_align_cases as fc
import posterior_cases as pc
from early_exit_transformer_amd import (Posteriors, SoftSpan, SoftWordSpan, capi, ctc_forced_align, ctc_posteriors, nbest_posteriors,
                                        soft_word_spans, starts_word_from_pieces)
from early_exit_transformer_amd.build import LIB_PATH

NEG = float("-inf")
BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eec.h")


def _log_softmax_trials(n_trials=300, seed=0):
    """fc.brute_trials' rows (V = 3, T <= 6, N <= 3, repeats included) on log_softmax emissions."""
    rng = np.random.default_rng(seed)
    for (_, T, y, blank), scale in zip(fc.brute_trials(n_trials, seed), (1.0, 3.0, 0.25) * n_trials):
        x = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, 3)) * scale), dim=-1).numpy()
        yield x, T, y, blank


def test_restatement_equals_brute_force():
    """ll, the occupancy, the first- and last-frame distributions and the blank's share by enumeration of all V^T labellings,
    allowed difference 1e-12 (worst observed 3.8e-15); a row is refused exactly when no labelling collapses to it."""
    served = refused = 0
    worst = 0.0
    for x, T, y, blank in _log_softmax_trials():
        r, want = pc.restate(x, T, y, blank), pc.brute(x, T, y, blank)
        assert (r is None) == (want is None), (T, y)
        if r is None:
            refused += 1
            continue
        served += 1
        ll, occ, first, last, share = want
        got = (r["ll"], r["gamma"][:, 1::2], r["first"], r["last"], r["gamma"][:, 0::2].sum(1))
        for a, b in zip(got, want):
            d = float(np.abs(np.asarray(a) - np.asarray(b)).max())
            worst = max(worst, d)
            assert d <= 1e-12, (T, y, d)
    print(f"brute force: {served} served, {refused} refused, worst difference {worst:.3e}")
    assert served >= 150 and refused >= 30


@pytest.mark.parametrize("Tq,V,scale", [(37, 5, 1), (37, 37, 8), (70, 37, 1), (70, 256, 8)])
def test_restatement_equals_torch_ctc_loss_and_its_gradient(Tq, V, scale):
    """ll == -loss, and per frame and label the occupancy summed over the states of that label is exp(x) - grad: torch's gradient
    with respect to log_softmax rows folds the softmax in.  Both are fp64; the differences are roundings (<= 1e-9 asserted)."""
    x, em_len, rows, tok_len, em_index = fc.gpu_case(Tq, V, scale)
    checked = 0
    for h, got in enumerate(pc.expected(Tq, V, scale)):
        if got is None:
            continue
        r, _ = got
        T, N, y = r["T"], r["N"], list(rows[h][:tok_len[h]])
        em = x[em_index[h], :T].double()[:, None, :].requires_grad_(True)
        loss = F.ctc_loss(em, torch.tensor([y]), torch.tensor([T]), torch.tensor([N]), blank=0, reduction="sum", zero_infinity=False)
        loss.backward()
        loss = float(loss.detach())
        assert abs(r["ll"] + loss) <= 1e-9 * max(1.0, abs(r["ll"])), (h, r["ll"], loss)
        occ = np.zeros((T, V))
        lab = [0 if s % 2 == 0 else y[s // 2] for s in range(2 * N + 1)]
        for s, v in enumerate(lab):
            occ[:, v] += r["gamma"][:, s]
        want = (em.detach().exp() - em.grad)[:, 0, :].numpy()
        assert float(np.abs(occ - want).max()) <= 1e-9, h
        checked += 1
    assert checked >= 10


@pytest.mark.parametrize("Tq,V,scale", pc.GPU_CASES)
def test_identities_hold_on_every_served_row(Tq, V, scale):
    """Every status-0 row: the first- and last-frame posteriors of a token sum to 1, tok_end - tok_start == tok_frames (a token's
    frames are contiguous), the tokens' frames and the blank's share add up to T, the variances are >= 0 -- up to the fp64
    rounding of sums of T terms of magnitude <= T^2."""
    n = 0
    for got in pc.expected(Tq, V, scale):
        if got is None:
            continue
        r, s = got
        T = r["T"]
        eps = 1e-12 * T
        assert float(np.abs(s["first_mass"] - 1.0).max()) <= eps and float(np.abs(s["last_mass"] - 1.0).max()) <= eps
        assert float(np.abs(s["tok_end"] - s["tok_start"] - s["tok_frames"]).max()) <= eps * T
        assert abs(s["tok_frames"].sum() + r["gamma"][:, 0::2].sum() - T) <= eps * T
        assert float(s["tok_start_var"].min()) >= -eps * T * T and float(s["tok_end_var"].min()) >= -eps * T * T
        assert math.isfinite(r["ll"])
        n += 1
    assert n >= 8


def _host(Tq, V, scale, **kw):
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    return ctc_posteriors(x, *fc.case_tensors(Tq, V, scale), em_len, **kw)


@pytest.mark.parametrize("Tq,V,scale", pc.GPU_CASES)
def test_host_path_equals_the_restatement(Tq, V, scale):
    """The package's vectorised fp64 path and the row-by-row restatement are two programs for one definition: they agree to the
    fp32 rounding of the outputs plus the fp64 noise of differently ordered sums (1e-9 relative to the sum's absolute terms);
    statuses and fills exactly."""
    got = _host(Tq, V, scale, want_gamma=True)
    assert got.gamma.shape == (got.status.numel(), Tq, fc.S_MAX) and got.gamma.dtype == torch.float32
    for h, want in enumerate(pc.expected(Tq, V, scale)):
        if want is None:
            assert int(got.status[h]) == 1 and float(got.row_logp[h]) == NEG and not bool(got.gamma[h].any())
            assert all(bool((getattr(got, n)[h] == -1.0).all()) for n in pc.TOKEN_FIELDS)
            continue
        r, s = want
        N, T = r["N"], r["T"]
        assert int(got.status[h]) == 0
        assert abs(float(got.row_logp[h]) - r["ll"]) <= 2.0 ** -23 * abs(r["ll"]) + 1e-9
        scale_of = dict(tok_frames=s["tok_frames"], tok_score=s["abs_score"], tok_start=s["m1s"], tok_end=s["m1e"],
                        tok_start_var=s["m2s"] + s["m1s"] ** 2, tok_end_var=s["m2e"] + s["m1e"] ** 2)
        for name in pc.TOKEN_FIELDS:
            out = getattr(got, name)[h].double().numpy()
            assert bool((out[N:] == -1.0).all()), (h, name)
            assert bool((np.abs(out[:N] - s[name]) <= 2.0 ** -23 * np.abs(s[name]) + 1e-9 * scale_of[name] + 1e-30).all()), (h, name)
        g = got.gamma[h].double().numpy()
        assert not g[T:].any() and not g[:, N:].any()
        ref = r["gamma"][:, 1::2]
        assert bool((np.abs(g[:T, :N] - ref) <= 2.0 ** -23 * ref + 1e-12).all()), h
    assert _host(Tq, V, scale).gamma is None


def test_planted_labelling_agrees_with_the_forced_alignment():
    """0 on the planted path and -40 elsewhere: all but exp(-40) of the mass is on one path per alignment choice, so the expected
    boundaries and frame counts are the Viterbi ones within 1e-6 and the variances are below 1e-6."""
    V, y = 7, [3, 5, 5, 2]
    frames = [0, 0, 3, 3, 3, 0, 5, 5, 0, 0, 5, 2, 2, 2, 2, 0, 0, 0]
    x = pc.planted(len(frames), V, frames)
    x2 = torch.cat([x, torch.full((4, V), float("nan"))])  # frames past the length are never read
    for em, kw in ((x[None], {}), (x2[None], dict(em_len=torch.tensor([len(frames)])))):
        po = ctc_posteriors(em, torch.tensor([y]), want_gamma=True, **kw)
        al = ctc_forced_align(em, torch.tensor([y]), **kw)
        assert po.status.tolist() == [0] and al.status.tolist() == [0]
        assert float((po.tok_start[0] - al.tok_start[0]).abs().max()) <= 1e-6
        assert float((po.tok_end[0] - al.tok_end[0]).abs().max()) <= 1e-6
        assert float((po.tok_frames[0] - (al.tok_end[0] - al.tok_start[0])).abs().max()) <= 1e-6
        assert float(po.tok_start_var[0].abs().max()) < 1e-6 and float(po.tok_end_var[0].abs().max()) < 1e-6
        assert abs(float(po.row_logp[0]) - float(al.path_score[0])) < 1e-6
        want = torch.zeros(em.size(1), len(y))
        for t, j in enumerate(al.frame_token[0].tolist()):
            if j >= 0:
                want[t, j] = 1.0
        assert float((po.gamma[0] - want).abs().max()) <= 1e-6
        spans = po.spans(0)
        assert [sp.token for sp in spans] == y and all(abs(sp.confidence - 1.0) < 1e-6 and sp.start_sd < 1e-3 for sp in spans)


def test_minus_infinity_emissions_and_status_two():
    """-inf is an ordinary value: a label the emission forbids at some frames is aligned around them, and a row every alignment of
    which crosses a forbidden frame has status 2 and the fill values."""
    T, V = 6, 4
    x = torch.log_softmax(torch.randn(1, T, V, generator=torch.Generator().manual_seed(3)), -1)
    x[0, :3, 2] = NEG  # label 2 cannot be said in frames 0 .. 2
    po = ctc_posteriors(x, torch.tensor([[1, 2]]), want_gamma=True)
    assert po.status.tolist() == [0] and math.isfinite(float(po.row_logp[0]))
    assert not bool(po.gamma[0, :3, 1].any()) and float(po.tok_start[0, 1]) >= 3.0 and bool(torch.isfinite(po.tok_score[0]).all())
    x[0, :, 2] = NEG
    po = ctc_posteriors(x, torch.tensor([[1, 2], [1, 3]]), em_index=torch.tensor([0, 0]), want_gamma=True)
    assert po.status.tolist() == [2, 0] and float(po.row_logp[0]) == NEG and not bool(po.gamma[0].any())
    assert all(bool((getattr(po, n)[0] == -1.0).all()) for n in pc.TOKEN_FIELDS) and po.spans(0) == []


def test_spans_words_and_nbest_on_hand_made_posteriors():
    po = Posteriors(row_logp=torch.tensor([-3.0, NEG]), tok_frames=torch.tensor([[3.0, 2.0, 1.0, -1.0], [-1.0] * 4]),
                    tok_score=torch.tensor([[-0.75, -2.0, 0.0, -1.0], [-1.0] * 4]),
                    tok_start=torch.tensor([[2.0, 6.0, 10.0, -1.0], [-1.0] * 4]), tok_end=torch.tensor([[5.0, 8.0, 11.0, -1.0], [-1.0] * 4]),
                    tok_start_var=torch.tensor([[0.25, 4.0, -1e-7, -1.0], [-1.0] * 4]),
                    tok_end_var=torch.tensor([[1.0, 0.0, 2.25, -1.0], [-1.0] * 4]), gamma=None,
                    status=torch.tensor([0, 1], dtype=torch.int32), tokens=torch.tensor([[7, 3, 9, 0], [1, 2, 3, 4]], dtype=torch.int32),
                    tok_len=torch.tensor([3, 4], dtype=torch.int32))
    spans = po.spans(0)
    assert spans == [SoftSpan(7, 2.0, 5.0, 0.5, 1.0, 3.0, math.exp(-0.25)), SoftSpan(3, 6.0, 8.0, 2.0, 0.0, 2.0, math.exp(-1.0)),
                     SoftSpan(9, 10.0, 11.0, 0.0, 1.5, 1.0, 1.0)]
    assert po.spans(1) == []
    sec = po.spans(0, frame_seconds=0.04)
    assert [(s.start, s.end, s.start_sd, s.frames) for s in sec] == [(2 * 0.04, 5 * 0.04, 0.5 * 0.04, 3.0), (6 * 0.04, 8 * 0.04, 2 * 0.04, 2.0),
                                                                     (10 * 0.04, 11 * 0.04, 0.0, 1.0)]
    pieces = ["<blk>", "a", "b", "ing", "c", "d", "e", "▁wor", "f", "▁d"]
    words = soft_word_spans(spans, starts_word_from_pieces(pieces))
    assert [w.tokens for w in words] == [(7, 3), (9,)] and isinstance(words[0], SoftWordSpan)
    assert (words[0].start, words[0].end, words[0].start_sd, words[0].end_sd) == (2.0, 8.0, 0.5, 0.0)
    assert abs(words[0].confidence - math.exp((-0.75 - 2.0) / 5)) < 1e-12 and words[1].confidence == 1.0
    assert soft_word_spans(spans[1:], lambda t: False)[0].tokens == (3, 9) and soft_word_spans([], lambda t: True) == []
    # the N-best confidence: a softmax per group, -inf rows get nothing, an all -inf group gets zeros
    p = nbest_posteriors(torch.tensor([-1.0, -2.0, NEG, -5.0, NEG]), torch.tensor([4, 4, 4, 9, 2]))
    a, b = math.exp(-1.0), math.exp(-2.0)
    assert p.dtype == torch.float64 and np.allclose(p.numpy(), [a / (a + b), b / (a + b), 0.0, 1.0, 0.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="5 rows, 2 group ids"):
        nbest_posteriors(torch.zeros(5), torch.zeros(2, dtype=torch.int64))


def test_refusals_of_the_package():
    x = torch.zeros(2, 8, 5)
    ok = torch.tensor([[1, 2]])
    for match, call in [
        (r"ctc_posteriors: logp must be \[n_em, T', V\] or \[E, B, T', V\]", lambda: ctc_posteriors(x[0], ok)),
        ("ctc_posteriors: logp must be fp32", lambda: ctc_posteriors(x.double(), ok)),
        ("ctc_posteriors: tokens must be an integer tensor", lambda: ctc_posteriors(x, ok.float())),
        (r"1 \.\. 255 tokens, got S = 256", lambda: ctc_posteriors(x, torch.ones((1, 256), dtype=torch.int64))),
        ("tok_len must have 1 entries, got 2", lambda: ctc_posteriors(x, ok, tok_len=torch.tensor([2, 2]))),
        ("em_len must have 2 entries, got 3", lambda: ctc_posteriors(x, ok, em_len=torch.tensor([8, 8, 8]))),
        ("3 rows, 2 emissions and no em_index", lambda: ctc_posteriors(x, torch.ones((3, 2), dtype=torch.int64))),
        (r"blank in \[0, V\)", lambda: ctc_posteriors(x, ok, blank=5)),
    ]:
        with pytest.raises(ValueError, match=match):
            call()
    # [E, B, T', V] input with lengths [B] shared by the exits equals its flattened form
    x4 = torch.log_softmax(torch.randn(2, 2, 9, 5, generator=torch.Generator().manual_seed(1)), -1)
    rows, idx, lens = torch.tensor([[1, 2, 0], [3, 3, 1], [2, 0, 0]]), torch.tensor([3, 0, 2]), torch.tensor([7, 9])
    a = ctc_posteriors(x4, rows, torch.tensor([2, 3, 1]), idx, lens, want_gamma=True)
    b = ctc_posteriors(x4.reshape(4, 9, 5), rows.to(torch.int16), torch.tensor([2, 3, 1]), idx, lens.repeat(2), want_gamma=True)
    assert a.status.tolist() == [0, 0, 0] and not bool(a.gamma[1, 7:].any()) and bool(a.gamma[0, 8].any())
    assert all(pc.same_bits(getattr(a, n), getattr(b, n)) for n in pc.TOKEN_FIELDS + ("row_logp", "gamma", "status"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _entry(lib, **over):
    """eec_ctc_posteriors on made-up addresses: every refusal below comes before any device work."""
    a = dict(logp=0x1000, n_em=2, Tq=16, V=8, em_len=None, tokens=0x2000, tok_len=0x3000, em_index=None, n_hyp=3, tok_stride=4, blank=0,
             row_logp=0x4000, tok_frames=0x5000, tok_score=0x6000, tok_start=0x7000, tok_end=0x8000, tok_start_var=0x9000,
             tok_end_var=0xa000, gamma=None, status=0xb000, ws=0x10000, ws_bytes=1 << 20)
    a.update(over)
    rc = lib.eec_ctc_posteriors(*a.values(), None)
    return rc, lib.eec_last_error().decode()


def test_entry_refusals_exports_and_workspace_size(lib):
    header = open(HEADER, encoding="utf-8").read()
    assert "CTC posteriors, standard topology" in header
    for name in ("eec_ctc_posteriors_workspace_bytes", "eec_ctc_posteriors"):
        assert name in capi.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header)
    assert not hasattr(lib, "eec_ctc_posteriors_last_error") and lib.eec_abi_version() == 16
    size = lib.eec_ctc_posteriors_workspace_bytes
    need = size(3, 16, 4)
    assert need == 3 * 16 * 1 * 256 and size(3840, 256, 200) == 3840 * 256 * 8 * 256 and size(384, 256, 85) == 384 * 256 * 4 * 256
    for args in ((0, 16, 4), (3, 0, 4), (3, 16, 0), (-1, 16, 4)):
        assert size(*args) == 0
    prev = 0
    for args in ((1, 1, 1), (1, 1, 31), (1, 1, 32), (1, 17, 32), (1, 17, 63), (1, 17, 64), (2, 17, 64), (2, 300, 127), (2, 300, 128),
                 (2, 300, 255), (2, 300, 256), (2, 301, 1000), (7, 301, 1000)):  # non-decreasing in each argument, multiples of 8
        cur = size(*args)
        assert cur >= prev and cur > 0 and cur % 8 == 0, args
        prev = cur
    for over, code, msg in [
        (dict(n_hyp=-1), BAD_ARG, "n_hyp >= 0"),
        (dict(Tq=0), BAD_ARG, "Tq, tok_stride, n_em, V >= 1"),
        (dict(tok_stride=0), BAD_ARG, "Tq, tok_stride, n_em, V >= 1"),
        (dict(n_em=0), BAD_ARG, "Tq, tok_stride, n_em, V >= 1"),
        (dict(blank=8), BAD_ARG, "blank in [0, V)"),
        (dict(blank=-1), BAD_ARG, "blank in [0, V)"),
        (dict(logp=None), BAD_ARG, "null argument"),
        (dict(tok_len=None), BAD_ARG, "null argument"),
        (dict(tok_end_var=None), BAD_ARG, "null argument"),
        (dict(row_logp=None), BAD_ARG, "null argument"),
        (dict(status=None), BAD_ARG, "null argument"),
        (dict(tok_stride=256), UNSUPPORTED, "tok_stride <= 255"),
        (dict(V=1), UNSUPPORTED, "V >= 2"),
        (dict(ws=None), WORKSPACE, "null workspace"),
        (dict(ws_bytes=need - 1), WORKSPACE, "workspace too small"),
        (dict(ws=0x10008), WORKSPACE, "256-byte aligned"),
    ]:
        rc, err = _entry(lib, **over)
        assert rc == code and msg in err, (over, rc, err)
    assert _entry(lib, n_hyp=0, logp=None, ws=None)[0] == 0  # a successful no-op, before the pointers are looked at
    with pytest.raises(C.ArgumentError):  # the binding's typed pointers: a CPU tensor never reaches a device slot
        lib.eec_ctc_posteriors(torch.zeros(2, 16, 8), 2, 16, 8, None, 0x2000, 0x3000, None, 3, 4, 0, 0x4000, 0x5000, 0x6000, 0x7000,
                               0x8000, 0x9000, 0xa000, None, 0xb000, 0x10000, 1 << 20, None)
