"""CTC segmentation without a device: the scalar restatement of tests/segment_cases.py against a brute force over all frame
labellings under the four flag settings, the NumPy host path of ``ctc_segment`` against the restatement bit for bit on rows on
either side of the one-wave limit, its equality with ``ctc_forced_align`` where both apply, a planted transcript found under free
ends, ``utterance_spans`` against an ``fsum`` restatement, and the refusals of the package and of the library's entry."""
import math
import os
import types

import numpy as np
import pytest
import torch

import forced_align_cases as fc
import segment_cases as sc
from early_exit_transformer_amd import Alignment, UtteranceSpan, capi, ctc_forced_align, ctc_segment, utterance_spans, windowed_emission
from early_exit_transformer_amd.build import LIB_PATH

NEG = float("-inf")
BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


def _kw(flags):
    return dict(free_start=bool(flags & sc.FREE_START), free_end=bool(flags & sc.FREE_END))


def test_restatement_equals_brute_force():
    """Every trial: the restatement aligns exactly when some labelling collapses to the labels; its score is the best labelling's,
    the free frames costing nothing, within the fp64 rounding of that sum (the inputs are dyadic, so the restatement's fp32 sums are
    exact); and its own labelling collapses to the labels and attains that score."""
    aligned = refused = 0
    per_flag = {f: 0 for f in sc.ALL_FLAGS}
    worst = 0.0
    for x, T, y, blank, flags in sc.brute_trials():
        status, score, state = sc.restate(x, T, y, blank, flags)
        best = sc.brute_best(x, T, y, blank, flags)
        assert (status == 1) == (best is None), (T, y, flags)
        if status == 1:
            refused += 1
            continue
        aligned += 1
        per_flag[flags] += 1
        worst = max(worst, abs(score - best))
        assert abs(score - best) <= T * 2.0 ** -52 * max(1.0, abs(best)), (T, y, flags, score, best)
        N = len(y)
        labels = [blank if s % 2 == 0 else y[s // 2] for s in state]
        assert fc.collapse(labels, blank) == tuple(y)
        own = sum(float(x[t, labels[t]]) for t in range(T)
                  if not (flags & sc.FREE_START and state[t] == 0) and not (flags & sc.FREE_END and state[t] == 2 * N))
        assert own == best
        assert state[0] <= 1 and state[-1] >= 2 * N - 1
    print(f"brute force: {aligned} aligned ({per_flag}), {refused} not alignable, worst |restatement - best labelling| = {worst:.3e}")
    assert aligned >= 150 and refused >= 20 and min(per_flag.values()) >= 30


def _against_restatement(x, em_len, rows, em_index, flags, S=None):
    tokens, tok_len = sc.pad_rows(rows, S)
    got = ctc_segment(x, tokens, tok_len, torch.tensor(em_index, dtype=torch.int32), em_len, **_kw(flags))
    xs = x.numpy()
    for h, row in enumerate(rows):
        want = sc.outputs(xs[em_index[h]], int(em_len[em_index[h]]), list(row), 0, flags, tokens.size(1))
        for name, ref in zip(sc.FIELDS, want):
            out = getattr(got, name)[h]
            assert out.dtype == ref.dtype and fc.same_bits(out, ref), (h, name)
    return got


@pytest.mark.parametrize("flags", sc.ALL_FLAGS)
@pytest.mark.parametrize("N", sc.HOST_N)
def test_host_path_equals_restatement(N, flags):
    """Rows of 1 .. 300 tokens -- on either side of the one-wave limit of 255 -- against emissions of N + R, 37, 70 and 330 frames
    where they fit, NaN from every length on."""
    x, em_len, row = sc.host_case(N, flags)
    got = _against_restatement(x, em_len, [row] * x.size(0), list(range(x.size(0))), flags)
    assert got.status.tolist() == [0] * x.size(0)
    assert int(em_len[0]) == N + fc.adjacent_equal(row)  # the tight fit is among them


@pytest.mark.parametrize("flags", sc.ALL_FLAGS)
def test_host_path_at_lengths_0_1_and_either_side_of_the_fit(flags):
    x, em_len = sc.length_case(flags)
    got = _against_restatement(x, em_len, [sc.TIGHT] * 5, list(range(5)), flags)
    assert got.status.tolist() == [1, 1, 1, 0, 0]
    assert all(sc.is_fill(got, h) for h in range(3))


@pytest.mark.parametrize("Tq,V,scale", [(37, 5, 1), (70, 37, 8), (300, 32, 8)])
def test_without_flags_it_is_ctc_forced_align(Tq, V, scale):
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    tokens, tok_len, em_index = fc.case_tensors(Tq, V, scale)
    sc.same(ctc_segment(x, tokens, tok_len, em_index, em_len), ctc_forced_align(x, tokens, tok_len, em_index, em_len))


def test_planted_transcript_is_found_under_free_ends():
    """40 tokens planted in frames [200, 420) of 600 -- four frames a token and a blank, then 20 blanks; 0.0 at the planted label and
    -30 elsewhere -- and every entry -log V outside.  With both ends free the outside costs nothing: the score is the planted sum,
    0.0, which only paths whose label frames all lie on planted frames attain.  Without the flags the 380 frames outside are paid
    for, and by the tie rule (stay first) the first token holds every frame from 0 on."""
    V, T = 50, 600
    y = list(range(1, 41))
    x = torch.full((T, V), -math.log(V))
    labels = [0] * 220
    for j in range(40):
        labels[5 * j:5 * j + 4] = [y[j]] * 4
    x[200:420] = -30.0
    x[torch.arange(200, 420), torch.tensor(labels)] = 0.0
    free = ctc_segment(x[None], torch.tensor([y]), free_start=True, free_end=True)
    assert free.status.tolist() == [0] and float(free.path_score[0]) == 0.0
    assert int(free.tok_start[0, 0]) >= 200 and int(free.tok_end[0, -1]) <= 420
    assert free.tok_start[0].tolist() == [200 + 5 * j for j in range(40)] and free.tok_score[0].tolist() == [0.0] * 40
    plain = ctc_segment(x[None], torch.tensor([y]))
    assert plain.status.tolist() == [0]
    assert int(plain.tok_start[0, 0]) < int(free.tok_start[0, 0]) and float(plain.path_score[0]) < float(free.path_score[0])
    assert int(plain.tok_start[0, 0]) == 0


def _hand_alignment(T, starts, ends, status=0):
    ft = torch.full((1, T), -1, dtype=torch.int32)
    for j, (a, b) in enumerate(zip(starts, ends)):
        ft[0, a:b] = j
    n = len(starts)
    return Alignment(tok_start=torch.tensor([starts], dtype=torch.int32), tok_end=torch.tensor([ends], dtype=torch.int32),
                     tok_score=torch.zeros((1, n)), frame_token=ft, path_score=torch.zeros(1), status=torch.tensor([status], dtype=torch.int32),
                     tokens=torch.tensor([[7, 3, 9, 4, 3, 11]], dtype=torch.int32), tok_len=torch.tensor([n], dtype=torch.int32))


def test_utterance_spans_against_an_fsum_restatement():
    """Three utterances of 3, 1 and 2 tokens: 66 frames (windows of 30, 30 and a short one of 6), 7 frames (shorter than a window)
    and 43 frames.  Within 1e-9 * max(1, |value|), which covers the fp64 rounding of a sum of 65536 terms."""
    T, V, window = 200, 12, 30
    starts, ends = [5, 20, 40, 90, 120, 150], [12, 33, 71, 97, 140, 163]
    al = _hand_alignment(T, starts, ends)
    ids = al.tokens[0].tolist()
    logp = torch.log_softmax(torch.randn(T, V, generator=torch.Generator().manual_seed(3)) * 3.0, -1)
    got = utterance_spans(al, 0, [3, 1, 2], logp, blank=0, window=window)
    ft = al.frame_token[0].tolist()
    p = [float(logp[f, ids[ft[f]] if ft[f] >= 0 else 0]) for f in range(T)]
    want = []
    for first, last in ((0, 2), (3, 3), (4, 5)):
        s, e = starts[first], ends[last]
        means = [math.fsum(p[c:min(c + window, e)]) / (min(c + window, e) - c) for c in range(s, e, window)]
        want.append((s, e, last - first + 1, math.fsum(p[s:e]) / (e - s), min(means)))
    assert [len(range(s, e, window)) for s, e, *_ in want] == [3, 1, 2]
    assert len(got) == 3 and all(isinstance(u, UtteranceSpan) for u in got)
    for u, (s, e, n, mean, worst) in zip(got, want):
        assert (u.start, u.end, u.n_tokens) == (s, e, n)
        assert abs(u.mean_logp - mean) <= 1e-9 * max(1.0, abs(mean)) and abs(u.min_window_logp - worst) <= 1e-9 * max(1.0, abs(worst))
        assert u.min_window_logp <= u.mean_logp + 1e-12
    sec = utterance_spans(al, 0, [3, 1, 2], logp, window=window, frame_seconds=0.04)
    assert [(u.start, u.end) for u in sec] == [(s * 0.04, e * 0.04) for s, e, *_ in want]
    assert [u[2:] for u in sec] == [u[2:] for u in got]
    assert utterance_spans(_hand_alignment(T, starts, ends, status=1), 0, [3, 1, 2], logp) == []
    with pytest.raises(ValueError, match="hold 5 tokens, row 0 has 6"):
        utterance_spans(al, 0, [3, 2], logp)
    with pytest.raises(ValueError, match="at least one token"):
        utterance_spans(al, 0, [3, 0, 3], logp)


def test_refusals_of_the_package():
    x = torch.zeros(1, 8, 5)
    with pytest.raises(ValueError, match=r"ctc_segment: a row has 1 \.\. 4095 tokens, got S = 4096"):
        ctc_segment(x, torch.ones((1, 4096), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"ctc_forced_align: a row has 1 \.\. 255 tokens, got S = 256"):
        ctc_forced_align(x, torch.ones((1, 256), dtype=torch.int64))
    assert ctc_segment(x, torch.ones((1, 256), dtype=torch.int64)).status.tolist() == [1]  # accepted; 256 tokens do not fit 8 frames
    with pytest.raises(ValueError, match=r"blank in \[0, V\)"):
        ctc_segment(x, torch.tensor([[1, 2]]), blank=5)
    model = types.SimpleNamespace(_cfg=types.SimpleNamespace(max_len=2000))  # refused before the model is looked at any further
    spec = torch.zeros(80, 5000)
    with pytest.raises(ValueError, match="window - overlap must be a multiple of 4"):
        windowed_emission(model, spec, 202, 40)
    with pytest.raises(ValueError, match="overlap must be a multiple of 8"):
        windowed_emission(model, spec, 204, 44)
    with pytest.raises(ValueError, match="exceeds the model's max_len = 2000"):
        windowed_emission(model, spec, 2040, 40)
    with pytest.raises(ValueError, match="0 <= overlap < window"):
        windowed_emission(model, spec, 40, 40)
    with pytest.raises(ValueError, match=r"spec must be \[n_mels, T\] or \[1, n_mels, T\]"):
        windowed_emission(model, torch.zeros(2, 80, 500), 200, 40)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _entry(lib, **over):
    """eec_ctc_segment on fake addresses: every refusal below comes before any device work."""
    a = dict(logp=0x1000, n_em=2, Tq=16, V=8, em_len=None, tokens=0x2000, tok_len=0x3000, em_index=None, n_hyp=3, tok_stride=4, blank=0,
             flags=0, tok_start=0x4000, tok_end=0x5000, tok_score=0x6000, frame_token=0x7000, path_score=0x8000, status=0x9000, ws=0x10000,
             ws_bytes=1 << 20)
    a.update(over)
    rc = lib.eec_ctc_segment(*a.values(), None)
    return rc, lib.eec_last_error().decode()


def test_entry_refusals_exports_and_workspace_size(lib):
    for name in ("eec_ctc_segment_workspace_bytes", "eec_ctc_segment"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert not hasattr(lib, "eec_ctc_segment_last_error") and lib.eec_abi_version() == 16
    size = lib.eec_ctc_segment_workspace_bytes
    need = size(3, 16, 4)
    assert need == 3 * 8 * 1 * 256  # n_hyp * ceil(T' / 2) * W * 256
    assert size(1, 32768, 4095) == 16384 * 16 * 256 and size(64, 512, 300) == 64 * 256 * 2 * 256 and size(2, 17, 256) == 2 * 9 * 2 * 256
    assert size(1, 2, 255) == 256 and size(1, 2, 256) == 512 and size(1, 2, 511) == 512 and size(1, 2, 512) == 768
    for args in ((0, 16, 4), (3, 0, 4), (3, 16, 0), (-1, 16, 4), (3, -5, 4), (3, 16, -1)):
        assert size(*args) == 0
    prev = 0
    for args in ((1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 2, 256), (1, 3, 256), (1, 3, 511), (1, 3, 512), (2, 3, 512), (2, 300, 1000),
                 (2, 300, 4095), (2, 300, 4096), (2, 301, 10000), (7, 301, 10000)):  # non-decreasing in each argument
        cur = size(*args)
        assert cur >= prev and cur > 0 and cur % 256 == 0, args
        prev = cur
    for over, code, msg in [
        (dict(flags=4), BAD_ARG, "flags"),
        (dict(flags=-1), BAD_ARG, "flags"),
        (dict(n_hyp=-1), BAD_ARG, "n_hyp >= 0"),
        (dict(Tq=0), BAD_ARG, "Tq, tok_stride, n_em, V >= 1"),
        (dict(tok_stride=0), BAD_ARG, "Tq, tok_stride, n_em, V >= 1"),
        (dict(blank=8), BAD_ARG, "blank in [0, V)"),
        (dict(logp=None), BAD_ARG, "null argument"),
        (dict(status=None), BAD_ARG, "null argument"),
        (dict(tok_stride=4096, ws_bytes=1 << 30), UNSUPPORTED, "tok_stride <= 4095"),
        (dict(V=1), UNSUPPORTED, "V >= 2"),
        (dict(ws=None), WORKSPACE, "null workspace"),
        (dict(ws_bytes=need - 1), WORKSPACE, "workspace too small"),
        (dict(ws=0x10008), WORKSPACE, "256-byte aligned"),
    ]:
        rc, err = _entry(lib, **over)
        assert rc == code and msg in err, (over, rc, err)
    for flags in sc.ALL_FLAGS:  # every valid setting passes the flag check: a successful no-op, before the pointers are looked at
        assert _entry(lib, n_hyp=0, logp=None, ws=None, flags=flags)[0] == 0
