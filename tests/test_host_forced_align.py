"""CTC forced alignment in the standard topology without a device: the scalar restatement of tests/forced_align_cases.py against a
brute force over all frame labellings, the NumPy host path of ``ctc_forced_align`` against the restatement bit for bit on every case
the GPU test runs, a planted and a flat emission, the bound by the CTC loss, the invariants of every aligned row, the span layer and
the refusals of the package and of the library's entry."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import forced_align_cases as fc
from early_exit_transformer_amd import Alignment, TokenSpan, WordSpan, capi, ctc_forced_align, starts_word_from_pieces, word_spans
from early_exit_transformer_amd.alignment import FRAME_SECONDS, exit_rows, transcript_rows
from early_exit_transformer_amd.build import LIB_PATH

NEG = float("-inf")
BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


def test_restatement_equals_brute_force():
    """Every trial: the restatement aligns exactly when some labelling collapses to the labels; its score is the best labelling's
    within the fp64 rounding of that sum (the inputs are dyadic, so the fp32 sums of the restatement are exact and the two differ in
    nothing but the order of the additions: worst difference observed 0.0); and its own frame labelling collapses to the labels and
    attains that score."""
    aligned = refused = 0
    worst = 0.0
    for x, T, y, blank in fc.brute_trials():
        status, score, state = fc.restate(x, T, y, blank)
        best = fc.brute_best(x, T, y, blank)
        assert (status == 1) == (best is None), (T, y)
        if status == 1:
            refused += 1
            continue
        aligned += 1
        worst = max(worst, abs(float(score) - best))
        assert abs(float(score) - best) <= T * 2.0 ** -52 * max(1.0, abs(best)), (T, y, float(score), best)
        labels = [blank if s % 2 == 0 else y[s // 2] for s in state]
        assert fc.collapse(labels, blank) == tuple(y)
        assert sum(float(x[t, labels[t]]) for t in range(T)) == best
        assert state[0] <= 1 and state[-1] >= 2 * len(y) - 1
    print(f"brute force: {aligned} aligned, {refused} not alignable, worst |restatement - best labelling| = {worst:.3e}")
    assert aligned >= 150 and refused >= 30


def _host(Tq, V, scale):
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    return ctc_forced_align(x, *fc.case_tensors(Tq, V, scale), em_len)


@pytest.mark.parametrize("Tq,V,scale", fc.GPU_CASES)
def test_host_path_equals_restatement_and_keeps_the_invariants(Tq, V, scale):
    got = _host(Tq, V, scale)
    for name, ref in zip(fc.FIELDS, fc.gpu_case_expected(Tq, V, scale)):
        out = getattr(got, name)
        assert out.dtype == ref.dtype and fc.same_bits(out, ref), name
    x, em_len, rows, tok_len, em_index = fc.gpu_case(Tq, V, scale)
    xs = x.numpy()
    n_ok = 0
    for h, y in enumerate(rows):
        if int(got.status[h]) != 0:
            assert float(got.path_score[h]) == NEG and bool((got.frame_token[h] == -2).all())
            assert bool((got.tok_start[h] == -1).all()) and bool((got.tok_end[h] == -1).all()) and bool((got.tok_score[h] == NEG).all())
            continue
        n_ok += 1
        em, T, N = xs[em_index[h]], int(em_len[em_index[h]]), tok_len[h]
        ft = got.frame_token[h].tolist()
        assert ft[T:] == [-2] * (Tq - T) and all(v >= -1 for v in ft[:T])
        assert fc.collapse([0 if j < 0 else y[j] for j in ft[:T]], 0) == tuple(y[:N])  # the frame labels collapse to the row
        a, b = got.tok_start[h, :N].tolist(), got.tok_end[h, :N].tolist()
        assert a[0] >= 0 and b[-1] <= T and all(a[j] < b[j] for j in range(N)) and all(b[j] <= a[j + 1] for j in range(N - 1))
        assert got.tok_start[h, N:].tolist() == [-1] * (fc.S_MAX - N) and bool((got.tok_score[h, N:] == NEG).all())
        total = None
        for j in range(N):
            assert ft[a[j]:b[j]] == [j] * (b[j] - a[j])
            acc = em[a[j], y[j]]
            for t in range(a[j] + 1, b[j]):
                acc = np.float32(acc + em[t, y[j]])
            assert np.float32(got.tok_score[h, j].item()).tobytes() == np.float32(acc).tobytes(), (h, j)
        for t in range(T):  # the frame scores summed in order are the path score
            v = em[t, 0 if ft[t] < 0 else y[ft[t]]]
            total = v if total is None else np.float32(total + v)
        assert np.float32(total).tobytes() == np.float32(got.path_score[h].item()).tobytes(), h
    assert n_ok >= 15


@pytest.mark.parametrize("Tq,V,scale", [c for c in fc.GPU_CASES if c[0] <= 70])
def test_path_score_is_bounded_by_the_ctc_loss(Tq, V, scale):
    """The best path cannot beat the sum over paths: path_score <= -ctc_loss in fp64, up to the fp32 rounding of the T adds of
    path_score (each within 2^-24 of its partial sum, which the sum of the |frame scores| bounds)."""
    got = _host(Tq, V, scale)
    x, em_len, rows, tok_len, em_index = fc.gpu_case(Tq, V, scale)
    checked = 0
    for h, y in enumerate(rows):
        if int(got.status[h]) != 0:
            continue
        T, N = int(em_len[em_index[h]]), tok_len[h]
        em = x[em_index[h], :T].double()
        loss = F.ctc_loss(em[:, None, :], torch.tensor([list(y[:N])]), torch.tensor([T]), torch.tensor([N]), blank=0, reduction="none",
                          zero_infinity=False)
        ft = got.frame_token[h, :T].tolist()
        mass = sum(abs(float(em[t, 0 if ft[t] < 0 else y[ft[t]]])) for t in range(T))
        assert float(got.path_score[h]) <= -float(loss[0]) + T * 2.0 ** -24 * mass, (h, float(got.path_score[h]), -float(loss[0]))
        checked += 1
    assert checked >= 15


def _planted(Tq, V, labels):
    """Log-probs [T', V]: 0.0 at ``labels[t]`` and -20 elsewhere."""
    x = torch.full((Tq, V), -20.0)
    x[torch.arange(Tq), torch.tensor(labels)] = 0.0
    return x


def test_planted_labelling_is_found_exactly():
    V, y = 7, [3, 5, 5, 2]
    frames = [0, 0, 3, 3, 3, 0, 5, 5, 0, 0, 5, 2, 2, 2, 2, 0, 0, 0]  # _ _ 3 3 3 _ 5 5 _ _ 5 2 2 2 2 _ _ _
    x = _planted(len(frames), V, frames)
    got = ctc_forced_align(x[None], torch.tensor([y]))
    assert got.status.tolist() == [0] and float(got.path_score[0]) == 0.0
    assert got.frame_token[0].tolist() == [-1, -1, 0, 0, 0, -1, 1, 1, -1, -1, 2, 3, 3, 3, 3, -1, -1, -1]
    assert got.tok_start[0].tolist() == [2, 6, 10, 11] and got.tok_end[0].tolist() == [5, 8, 11, 15]
    assert got.tok_score[0].tolist() == [0.0] * 4
    # near equality with the sum over paths: every other path pays at least one -20, and fewer than 2 T (V - 1) paths pay only one
    T = len(frames)
    loss = F.ctc_loss(x.double()[:, None, :], torch.tensor([y]), torch.tensor([T]), torch.tensor([len(y)]), reduction="none")
    assert 0.0 <= -float(loss[0]) - float(got.path_score[0]) < 2 * T * (V - 1) * math.exp(-20.0)
    # with frame lengths: the part past the length is never read
    x2 = torch.cat([x, torch.full((4, V), float("nan"))])
    cut = ctc_forced_align(x2[None], torch.tensor([y + [1, 1]]), tok_len=torch.tensor([4]), em_len=torch.tensor([T]))
    assert cut.frame_token[0].tolist() == got.frame_token[0].tolist() + [-2] * 4 and float(cut.path_score[0]) == 0.0
    assert cut.tok_start[0].tolist() == [2, 6, 10, 11, -1, -1]


def test_flat_emission_pins_the_tie_rule():
    """Every entry equal: every reachable state has the same score at a frame, so every choice is a tie.  Ties go stay, then step,
    then skip, and the end prefers the last label (2N only if strictly greater).  The decision d[t][s] is therefore `stay` whenever
    s was reachable at t - 1, and the walk back from (T - 1, 2N - 1) stays in a state down to the state's EARLIEST frame e(s):
    e(1) = 0, e(2j + 1) = e(2j - 1) + 1 for y_j != y_{j-1} (the skip; the blank between them is reachable only one frame later),
    else e(2j - 1) + 2 (through the blank).  Every token but the last holds the one frame e(2j + 1), blanks stand only between equal
    neighbours, and the last token holds every frame from e(2N - 1) to the end."""
    V, T = 6, 23
    for y in ([4], [1, 2, 3], [2, 2], [1, 1, 2, 2, 2, 3, 1], [5, 4, 5, 5, 4]):
        x = torch.full((1, T, V), -1.75)
        got = ctc_forced_align(x, torch.tensor([y]))
        status, score, state = fc.restate(x[0].numpy(), T, y, 0)
        assert status == 0 and got.status.tolist() == [0]
        e = [0]
        for j in range(1, len(y)):
            e.append(e[-1] + (1 if y[j] != y[j - 1] else 2))
        want = [-1] * T
        for j, t in enumerate(e):
            want[t] = j
        want[e[-1]:] = [len(y) - 1] * (T - e[-1])
        assert got.frame_token[0].tolist() == want == [s // 2 if s % 2 else -1 for s in state], y
        assert got.tok_start[0].tolist() == e and got.tok_end[0].tolist() == [t + 1 for t in e[:-1]] + [T]
        assert float(got.path_score[0]) == float(score) == -1.75 * T  # exact: a multiple of 1/4


def test_spans_words_and_seconds_on_a_hand_made_alignment():
    al = Alignment(tok_start=torch.tensor([[2, 6, 10, -1], [-1, -1, -1, -1]], dtype=torch.int32),
                   tok_end=torch.tensor([[5, 8, 11, -1], [-1, -1, -1, -1]], dtype=torch.int32),
                   tok_score=torch.tensor([[-0.75, -2.0, 0.0, NEG], [NEG] * 4]), frame_token=torch.zeros((2, 12), dtype=torch.int32),
                   path_score=torch.tensor([-3.0, NEG]), status=torch.tensor([0, 1], dtype=torch.int32),
                   tokens=torch.tensor([[7, 3, 9, 0], [1, 2, 3, 4]], dtype=torch.int32), tok_len=torch.tensor([3, 4], dtype=torch.int32))
    spans = al.spans(0)
    assert spans == [TokenSpan(7, 2, 5, -0.75, math.exp(-0.25), 3), TokenSpan(3, 6, 8, -2.0, math.exp(-1.0), 2),
                     TokenSpan(9, 10, 11, 0.0, 1.0, 1)]
    assert al.spans(1) == []
    sec = al.spans(0, frame_seconds=FRAME_SECONDS)
    assert FRAME_SECONDS == 4 * 160 / 16000
    assert [(s.start, s.end) for s in sec] == [(2 * 0.04, 5 * 0.04), (6 * 0.04, 8 * 0.04), (10 * 0.04, 11 * 0.04)]
    assert [s.confidence for s in sec] == [s.confidence for s in spans]
    pieces = ["<blk>", "a", "b", "ing", "c", "d", "e", "▁wor", "f", "▁d"]
    table = starts_word_from_pieces(pieces)
    assert table.dtype == bool and table.tolist() == [p.startswith("▁") for p in pieces]
    words = word_spans(sec, table)
    assert words == [WordSpan((7, 3), 2 * 0.04, 8 * 0.04, math.exp((-0.75 - 2.0) / 5)), WordSpan((9,), 10 * 0.04, 11 * 0.04, 1.0)]
    assert word_spans(spans, lambda t: t == 9) == [WordSpan((7, 3), 2, 8, math.exp(-2.75 / 5)), WordSpan((9,), 10, 11, 1.0)]
    assert word_spans(spans[1:], lambda t: False) == [WordSpan((3, 9), 6, 11, math.exp(-2.0 / 3))]  # the first token opens a word
    assert word_spans([], table) == []


def test_refusals_of_the_package():
    x = torch.zeros(2, 8, 5)
    ok = torch.tensor([[1, 2]])
    with pytest.raises(ValueError, match=r"logp must be \[n_em, T', V\] or \[E, B, T', V\]"):
        ctc_forced_align(x[0], ok)
    with pytest.raises(ValueError, match="logp must be fp32"):
        ctc_forced_align(x.double(), ok)
    with pytest.raises(ValueError, match="tokens must be an integer tensor"):
        ctc_forced_align(x, ok.float())
    with pytest.raises(ValueError, match="tokens must be an integer tensor"):
        ctc_forced_align(x, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match=r"1 \.\. 255 tokens, got S = 256"):
        ctc_forced_align(x, torch.ones((1, 256), dtype=torch.int64))
    with pytest.raises(ValueError, match="tok_len must have 1 entries, got 2"):
        ctc_forced_align(x, ok, tok_len=torch.tensor([2, 2]))
    with pytest.raises(ValueError, match="em_len must have 2 entries, got 3"):
        ctc_forced_align(x, ok, em_len=torch.tensor([8, 8, 8]))
    with pytest.raises(ValueError, match="em_index must have 1 entries"):
        ctc_forced_align(x, ok, em_index=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="3 rows, 2 emissions and no em_index"):
        ctc_forced_align(x, torch.ones((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"blank in \[0, V\)"):
        ctc_forced_align(x, ok, blank=5)
    # decoder output as rows: special ids leave, a blank is refused with a message
    class Hyp:
        tokens = [1, 4, 4, 2]
    assert transcript_rows([[1, 7, 3, 2], torch.tensor([7, 8]), Hyp(), [Hyp(), [9]]], drop={1, 2}) == [[7, 3], [7, 8], [4, 4], [4, 4]]
    with pytest.raises(ValueError, match=r"utterance 1 holds the blank \(0\)"):
        transcript_rows([[5], [5, 0, 6]], drop={1, 2})
    # any integer dtype, and ids that int32 cannot hold stay outside the vocabulary
    x = torch.log_softmax(torch.randn(1, 8, 5, generator=torch.Generator().manual_seed(1)), -1)
    a = ctc_forced_align(x, torch.tensor([[1, 2]], dtype=torch.uint8))
    for dt in (torch.int16, torch.int32, torch.int64):
        b = ctc_forced_align(x, torch.tensor([[1, 2]], dtype=dt))
        assert all(fc.same_bits(getattr(a, n), getattr(b, n)) for n in fc.FIELDS)
    assert ctc_forced_align(x, torch.tensor([[1, (1 << 32) + 2]])).status.tolist() == [1]


def test_exit_rows_pairs_padding_and_refusals():
    """What ``BeamInference.timestamps`` / ``.confidences`` hand to the kernels, against a literal table: E = 3 exits, B = 2
    utterances of 3 and 1 tokens after the special ids 1 and 2 left."""
    hyps = [[1, 7, 3, 9, 2], torch.tensor([8])]
    last = ([(2, 0), (2, 1)], [[7, 3, 9], [8, 0, 0]], [3, 1], [4, 5])
    table = {"none": (None, last),
             "list": ([1, 0], ([(1, 0), (0, 1)], [[7, 3, 9], [8, 0, 0]], [3, 1], [2, 1])),
             "tensor": (torch.tensor([0, 2]), ([(0, 0), (2, 1)], [[7, 3, 9], [8, 0, 0]], [3, 1], [0, 5])),
             "all": ("all", ([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], [[7, 3, 9], [8, 0, 0]] * 3, [3, 1] * 3, [0, 1, 2, 3, 4, 5]))}
    for exits, want in table.values():
        pairs, tokens, tok_len, em_index = exit_rows("confidences", hyps, exits, 3, 2, drop={1, 2})
        assert all(t.dtype == torch.int32 for t in (tokens, tok_len, em_index))
        assert (pairs, tokens.tolist(), tok_len.tolist(), em_index.tolist()) == want
        assert em_index.tolist() == [e * 2 + b for e, b in pairs]
    # the padding is max(1, longest): rows without a token still have a column
    pairs, tokens, tok_len, em_index = exit_rows("timestamps", [[1, 2], []], None, 3, 2, drop={1, 2})
    assert (tuple(tokens.shape), tokens.tolist(), tok_len.tolist(), em_index.tolist()) == ((2, 1), [[0], [0]], [0, 0], [4, 5])
    for name in ("timestamps", "confidences"):
        with pytest.raises(ValueError, match=rf"^{name}: 2 utterances, 3 hypotheses$"):
            exit_rows(name, hyps + [[5]], None, 3, 2)
        with pytest.raises(ValueError, match=rf"^{name}: exits must be None, one exit per utterance or 'all', got 'every'$"):
            exit_rows(name, hyps, "every", 3, 2)
        for bad in ([0, 3], [-1, 0], [0], torch.tensor([0, 1, 2])):
            with pytest.raises(ValueError, match=rf"^{name}: exits must hold one exit of 0 \.\. 2 per utterance \(2\)$"):
                exit_rows(name, hyps, bad, 3, 2)
        with pytest.raises(ValueError, match=rf"^{name}: the transcript of utterance 1 holds the blank \(0\)$"):
            exit_rows(name, [[5], [5, 0, 6]], None, 3, 2)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _entry(lib, **over):
    """eec_ctc_forced_align on fake addresses: every refusal below comes before any device work."""
    a = dict(logp=0x1000, n_em=2, Tq=16, V=8, em_len=None, tokens=0x2000, tok_len=0x3000, em_index=None, n_hyp=3, tok_stride=4, blank=0,
             tok_start=0x4000, tok_end=0x5000, tok_score=0x6000, frame_token=0x7000, path_score=0x8000, status=0x9000, ws=0x10000,
             ws_bytes=1 << 20)
    a.update(over)
    rc = lib.eec_ctc_forced_align(*a.values(), None)
    return rc, lib.eec_last_error().decode()


def test_entry_refusals_exports_and_workspace_size(lib):
    for name in ("eec_ctc_forced_align_workspace_bytes", "eec_ctc_forced_align"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert not hasattr(lib, "eec_ctc_forced_align_last_error") and lib.eec_abi_version() == 16
    size = lib.eec_ctc_forced_align_workspace_bytes
    need = size(3, 16, 4)
    assert need == 3 * 1 * 256 and size(3840, 256, 200) == 3840 * 128 * 256 and size(3840, 256, 85) == 3840 * 64 * 256
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
        (dict(tok_score=None), BAD_ARG, "null argument"),
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
        lib.eec_ctc_forced_align(torch.zeros(2, 16, 8), 2, 16, 8, None, 0x2000, 0x3000, None, 3, 4, 0, 0x4000, 0x5000, 0x6000, 0x7000,
                                 0x8000, 0x9000, 0x10000, 1 << 20, None)
