"""Keyword spotting on CTC emissions, without a GPU: the scalar restatement (tests/kws_cases.py) against a brute force over all
segments and label paths, the NumPy host path of ``keyword_search`` against the restatement bit for bit, planted keywords,
invariances, and the refusals."""
import ctypes as C
import math
import os

import pytest
import torch

import kws_cases as kc
from early_exit_transformer_amd import KeywordHits, KeywordSet, capi, keyword_search
from early_exit_transformer_amd.build import LIB_PATH

BAD_ARG, UNSUPPORTED, WORKSPACE = 10001, 10002, 10003


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def test_restatement_equals_brute_force():
    """Every (trial, end frame): the per-end-frame score is the brute-force maximum exactly (dyadic inputs: every sum is exact), and
    the reported segment [start, end] attains it.  The tie rules are local, so the start is held to that and to nothing more."""
    cells = tied = 0
    for x, T, y, blank in kc.brute_trials(300):
        score, start, end, ts, tb = kc.restate(x, T, y, blank)
        seg = kc.brute_segments(x, T, y, blank)
        per_end = [max(seg[a][b] for a in range(b + 1)) for b in range(T)]
        for b in range(T):
            cells += 1
            assert ts[b] == per_end[b], (x, y, b)
            if per_end[b] == kc.NEG:
                assert tb[b] == -1, (x, y, b)
            else:
                assert 0 <= tb[b] <= b and seg[tb[b]][b] == per_end[b], (x, y, b)
                tied += sum(1 for a in range(b + 1) if seg[a][b] == per_end[b]) > 1
        best = max(per_end, default=kc.NEG)
        assert score == best
        if best == kc.NEG:
            assert (start, end) == (-1, -1)
        else:
            assert end == per_end.index(best) and seg[start][end] == best
        if y == [1, 1] and T < 3:
            assert score == kc.NEG  # adjacent equal tokens need a blank frame between them
    assert cells > 900 and tied > 0


HOST_CASES = [(37, 5, 8), (70, 37, 1), (70, 32, 8), (37, 256, 1)]


def _search(Tq, V, scale, **kw):
    x, em_len, phrases, _ = kc.gpu_case(Tq, V, scale)
    return keyword_search(x, KeywordSet(phrases, V), em_len, want_trace=True, **kw)


def _assert_hits_equal(a: KeywordHits, b, what=""):
    b = (b.score, b.start, b.end, b.trace_score, b.trace_start) if isinstance(b, KeywordHits) else b
    for name, got, want in zip(("score", "start", "end", "trace_score", "trace_start"), (a.score, a.start, a.end, a.trace_score, a.trace_start), b):
        assert got.dtype == want.dtype and kc.same_bits(got, want), (what, name)


@pytest.mark.parametrize("Tq,V,scale", HOST_CASES)
def test_host_path_equals_restatement(Tq, V, scale):
    hits = _search(Tq, V, scale)
    want = kc.gpu_case_expected(Tq, V, scale)
    _assert_hits_equal(hits, want)
    x, em_len, phrases, _ = kc.gpu_case(Tq, V, scale)
    for n in range(kc.N_EM):
        for k, y in enumerate(phrases):
            if int(em_len[n]) >= len(y) + kc.adjacent_equal(y):
                assert math.isfinite(float(hits.score[n, k])) and math.isfinite(float(want[0][n, k])), (n, k)
    no_trace = keyword_search(x, KeywordSet(phrases, V), em_len)
    assert no_trace.trace_score is None and no_trace.trace_start is None
    for got, ref in zip((no_trace.score, no_trace.start, no_trace.end), want[:3]):
        assert kc.same_bits(got, ref)


def _planted(T, V, spans, blank=0):
    """Logits whose greedy path is blank except for the (token, first frame, last frame) runs of ``spans``."""
    x = torch.zeros((T, V))
    x[:, blank] = 8.0
    for tok, a, b in spans:
        x[a:b + 1, blank] = 0.0
        x[a:b + 1, tok] = 8.0
    return x + 0.25 * torch.arange(V, dtype=torch.float32) / V  # no two logits of a frame equal, none of them the path's rival


def test_planted_keyword_scores_zero_at_its_frames():
    V = 7
    x = _planted(30, V, [(3, 4, 6), (5, 7, 8), (5, 11, 13), (2, 14, 14), (2, 15, 16)])  # 3 3 3 5 5 _ _ 5 5 5 2 2 2: [3, 5, 5, 2]
    hits = keyword_search(x[None], KeywordSet([[3, 5, 5, 2], [3, 5, 2], [5, 5]], V), want_trace=True)
    assert hits.score[0].tolist() == [0.0, hits.score[0, 1].item(), 0.0] and hits.score[0, 1] < 0
    # the end is the FIRST frame that attains the maximum (the first frame of the last token's run), the start the first frame of y_1
    assert (hits.start[0, 0].item(), hits.end[0, 0].item()) == (4, 14)
    assert (hits.start[0, 2].item(), hits.end[0, 2].item()) == (7, 11)
    assert hits.trace_score[0, 0, 14:17].tolist() == [0.0, 0.0, 0.0] and hits.trace_start[0, 0, 14:17].tolist() == [4, 4, 4]
    assert bool((hits.trace_score[0, 0, :14] < 0).all()) and bool((hits.trace_score[0, 0, 17:] < 0).all())


def test_detections_return_both_planted_occurrences_without_overlap():
    V = 6
    x = _planted(40, V, [(2, 3, 5), (4, 6, 7), (2, 20, 21), (4, 23, 26)])  # [2, 4] at 3 .. 7 and at 20 .. 26 (blanks inside)
    hits = keyword_search(x[None], KeywordSet([[2, 4], [4, 3]], V), want_trace=True)
    found = hits.detections(0.0)
    assert [(s, e) for s, e, _ in found[0][0]] == [(3, 6), (20, 23)] and all(sc == 0.0 for _, _, sc in found[0][0])
    assert found[0][1] == []  # [4, 3] is spelled nowhere
    loose = hits.detections([-1.0e9, 0.0])[0][0]  # every end frame is a candidate: still no two accepted segments overlap
    assert loose[:2] == found[0][0]
    spans = sorted((s, e) for s, e, _ in loose)
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
    with pytest.raises(ValueError, match="want_trace"):
        keyword_search(x[None], KeywordSet([[2, 4]], V)).detections(0.0)


def test_first_exit_is_the_shallowest_exit_that_hits():
    V = 6
    miss, hit = _planted(20, V, [(3, 2, 4)]), _planted(20, V, [(2, 3, 5), (4, 6, 7)])
    x = torch.stack([torch.stack([miss, miss]), torch.stack([miss, hit]), torch.stack([hit, hit])])  # [E = 3, B = 2, T', V]
    hits = keyword_search(x, KeywordSet([[2, 4], [3]], V), em_len=torch.tensor([20, 20]))
    assert tuple(hits.score.shape) == (3, 2, 2)
    assert hits.first_exit(0.0).tolist() == [[2, 0], [1, 0]]
    assert hits.first_exit([0.0, 1.0]).tolist() == [[2, -1], [1, -1]]
    flat = keyword_search(x.reshape(6, 20, V), KeywordSet([[2, 4], [3]], V))
    assert kc.same_bits(flat.score, hits.score.reshape(6, 2)) and kc.same_bits(flat.end, hits.end.reshape(6, 2))
    with pytest.raises(ValueError, match="E, B"):
        flat.first_exit(0.0)


def test_invariances():
    Tq, V, scale = 37, 32, 8
    x, em_len, phrases, _ = kc.gpu_case(Tq, V, scale)
    kws = KeywordSet(phrases, V)
    # a per-frame constant that is a power of two: on emissions that are multiples of 2^-10 below 2^13 in size the shifted values
    # are fp32 numbers too, so every x - m keeps its bits
    x = torch.round(x * 1024) / 1024
    base = keyword_search(x, kws, em_len, want_trace=True)
    finite = torch.nan_to_num(x, nan=0.0)
    shift = torch.tensor([4.0, -8.0, 16.0])[torch.arange(Tq) % 3].view(1, Tq, 1)
    assert bool(((finite + shift) - shift == finite).all()) and float(finite.abs().max()) < 8192
    _assert_hits_equal(keyword_search(x + shift, kws, em_len, want_trace=True), base, "shift")
    assert bool(torch.isfinite(base.score[4, :9]).sum() >= 7)  # the comparison is not one of fill values
    # em_len = None against lengths all T'
    clean = torch.log_softmax(torch.randn(3, Tq, V, generator=torch.Generator().manual_seed(5)) * 8, -1)
    _assert_hits_equal(keyword_search(clean, kws, want_trace=True), keyword_search(clean, kws, torch.full((3,), Tq), want_trace=True), "lengths")
    _assert_hits_equal(keyword_search(clean, kws, want_trace=True), keyword_search(clean, kws, torch.full((3,), Tq + 9), want_trace=True), "clamp")
    # a split over keywords, a split over emissions
    halves = [keyword_search(x, KeywordSet(phrases[a:b], V), em_len, want_trace=True) for a, b in ((0, 6), (6, 13))]
    joined = [torch.cat([getattr(h, f) for h in halves], dim=1) for f in ("score", "start", "end", "trace_score", "trace_start")]
    _assert_hits_equal(base, joined, "keywords")
    parts = [keyword_search(x[a:b], kws, em_len[a:b], want_trace=True) for a, b in ((0, 2), (2, 5))]
    joined = [torch.cat([getattr(h, f) for h in parts], dim=0) for f in ("score", "start", "end", "trace_score", "trace_start")]
    _assert_hits_equal(base, joined, "emissions")


def test_keyword_set_refusals():
    ok = [[1, 2]]
    with pytest.raises(ValueError, match=r"a keyword has 1 \.\. 64 tokens, keyword 1 has 0"):
        KeywordSet(ok + [[]], 8)
    with pytest.raises(ValueError, match=r"a keyword has 1 \.\. 64 tokens, keyword 0 has 65"):
        KeywordSet([[1, 2] * 32 + [1]], 8)
    assert len(KeywordSet([[1, 2] * 32], 8)) == 1
    with pytest.raises(ValueError, match=r"1 \.\. 65536 keywords, got 0"):
        KeywordSet([], 8)
    with pytest.raises(ValueError, match=r"1 \.\. 65536 keywords, got 65537"):
        KeywordSet([[1]] * 65537, 8)
    with pytest.raises(ValueError, match=r"keyword 1 holds the blank \(3\)"):
        KeywordSet(ok + [[1, 3]], 8, blank=3)
    for bad in (8, -1):
        with pytest.raises(ValueError, match=r"keyword 0 holds token -?\d+, outside \[0, 8\)"):
            KeywordSet([[1, bad]], 8)
    with pytest.raises(ValueError, match="blank in"):
        KeywordSet(ok, 8, blank=8)
    kws = KeywordSet.from_texts(["ab", "c"], lambda s: [ord(ch) - ord("a") + 1 for ch in s], vocab_size=8)
    assert [kws.phrase(k) for k in range(len(kws))] == [[1, 2], [3]]
    with pytest.raises(ValueError, match="over 8 tokens, logp has 9"):
        keyword_search(torch.zeros(1, 4, 9), kws)
    with pytest.raises(ValueError, match=r"T' must be in 1 \.\. 2\^20, got 1048577"):
        keyword_search(torch.zeros(1, (1 << 20) + 1, 8), kws)
    with pytest.raises(ValueError, match="em_len must have 2 entries"):
        keyword_search(torch.zeros(2, 4, 8), kws, torch.tensor([4, 4, 4]))


def _entry(lib, **over):
    """eec_keyword_search on fake addresses: every refusal below comes before any device work."""
    a = dict(logp=0x1000, n_em=2, Tq=16, V=8, em_len=None, tokens=0x2000, tok_len=0x3000, K=3, tok_stride=4, blank=0, score=0x4000,
             start=0x5000, end=0x6000, trace_score=None, trace_start=None, ws=0x10000, ws_bytes=1 << 20)
    a.update(over)
    rc = lib.eec_keyword_search(*a.values(), None)
    return rc, lib.eec_last_error().decode()


def test_entry_refusals_and_exports(lib):
    for name in ("eec_keyword_search_workspace_bytes", "eec_keyword_search"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert not hasattr(lib, "eec_keyword_last_error") and lib.eec_abi_version() == 16
    need = lib.eec_keyword_search_workspace_bytes(2, 16)
    assert need >= 2 * 16 * 4 and need % 256 == 0 and lib.eec_keyword_search_workspace_bytes(0, 16) == 0
    for over, code, msg in [
        (dict(K=0), BAD_ARG, "K must be in 1..65536, got 0"),
        (dict(K=65537), BAD_ARG, "K must be in 1..65536, got 65537"),
        (dict(tok_stride=0), BAD_ARG, "a keyword has 1..64 tokens, got tok_stride 0"),
        (dict(tok_stride=65), BAD_ARG, "a keyword has 1..64 tokens, got tok_stride 65"),
        (dict(Tq=(1 << 20) + 1), BAD_ARG, "Tq must be in 1..2^20, got 1048577"),
        (dict(Tq=0), BAD_ARG, "Tq must be in 1..2^20, got 0"),
        (dict(blank=8), BAD_ARG, "blank in [0, V)"),
        (dict(V=1), BAD_ARG, "V >= 2"),
        (dict(tokens=None), BAD_ARG, "null argument"),
        (dict(score=None), BAD_ARG, "null argument"),
        (dict(trace_score=0x7000), BAD_ARG, "together"),
        (dict(n_em=1 << 12, Tq=1 << 20, ws_bytes=1 << 40), UNSUPPORTED, "below 2^31"),
        (dict(ws=None), WORKSPACE, "null workspace"),
        (dict(ws_bytes=need - 1), WORKSPACE, "workspace too small"),
        (dict(ws=0x10004), WORKSPACE, "256-byte aligned"),
    ]:
        rc, err = _entry(lib, **over)
        assert rc == code and msg in err, (over, rc, err)
    with pytest.raises(C.ArgumentError):  # the binding's typed pointers: a CPU tensor never reaches a device slot
        lib.eec_keyword_search(torch.zeros(2, 16, 8), 2, 16, 8, None, 0x2000, 0x3000, 3, 4, 0, 0x4000, 0x5000, 0x6000, None, None, 0x10000, 1 << 20, None)
