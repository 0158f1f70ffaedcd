"""Keyword spotting on CTC emissions on the device (csrc/keyword.hip) against the scalar restatement of tests/kws_cases.py, bit for
bit: every (emission, keyword) pair of every case, nothing excluded.  The cases cross the lane boundaries of the state layout
(L = 31, 32, 33, 63, 64: one state per lane up to 32 tokens, two above), the 64-frame trace words and the look-ahead (T' = 70),
vocabularies that are no multiple of 4, storage 4 bytes off a 16-byte boundary, lengths 0, 1, 2, 36 and T' with NaN from every
length on, adjacent equal tokens, a keyword longer than every emission and a planted one."""
import math

import pytest
import torch

import kws_cases as kc
from early_exit_transformer_amd import KeywordSet, capi, keyword_search

pytestmark = pytest.mark.gpu
FIELDS = ("score", "start", "end", "trace_score", "trace_start")


def _on_device(x: torch.Tensor, off: int) -> torch.Tensor:
    """``x`` on the device, its first element ``off`` floats behind the allocation's (256-byte aligned) start."""
    buf = torch.empty(x.numel() + off, dtype=torch.float32, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


@pytest.mark.parametrize("Tq,V,scale", kc.GPU_CASES)
def test_device_equals_restatement(Tq, V, scale):
    x, em_len, phrases, planted = kc.gpu_case(Tq, V, scale)
    want = kc.gpu_case_expected(Tq, V, scale)
    kws = KeywordSet(phrases, V)
    off = 1 if (Tq + V + scale) % 2 else 0  # half of the cases read storage 4 bytes off a 16-byte boundary
    xd = _on_device(x, off)
    hits = keyword_search(xd, kws, em_len.cuda(), want_trace=True)
    for name, ref in zip(FIELDS, want):
        got = getattr(hits, name)
        assert got.dtype == ref.dtype and kc.same_bits(got, ref), name
    for n in range(kc.N_EM):
        for k, y in enumerate(phrases):
            if int(em_len[n]) >= len(y) + kc.adjacent_equal(y):
                assert math.isfinite(float(want[0][n, k])) and math.isfinite(float(hits.score[n, k])), (n, k)
    for n in (3, 4):  # the planted phrase: exactly 0, from the first frame of y_1 to the first frame of y_L
        assert float(hits.score[n, planted]) == 0.0
        assert (int(hits.start[n, planted]), int(hits.end[n, planted])) == (kc.PLANT_FRAMES[0], kc.PLANT_FRAMES[0] + 6)
    host = keyword_search(x, kws, em_len, want_trace=True)  # the NumPy host path
    again = keyword_search(xd, kws, em_len.cuda(), want_trace=True)
    for name in FIELDS:
        assert kc.same_bits(getattr(hits, name), getattr(host, name)), name
        assert kc.same_bits(getattr(hits, name), getattr(again, name)), name
    lean = keyword_search(xd, kws, em_len.cuda())
    assert lean.trace_score is None and lean.trace_start is None
    for name in FIELDS[:3]:
        assert kc.same_bits(getattr(lean, name), getattr(hits, name)), name


def test_exits_by_batch_input_and_splits():
    Tq, V, scale = 70, 37, 8
    x, _, phrases, _ = kc.gpu_case(Tq, V, scale)
    kws = KeywordSet(phrases, V)
    x = torch.nan_to_num(x[1:], nan=-1.0).cuda().reshape(2, 2, Tq, V)  # [E = 2, B = 2]
    lens = torch.tensor([33, 70], dtype=torch.int32, device="cuda")
    hits = keyword_search(x, kws, lens, want_trace=True)
    assert tuple(hits.score.shape) == (2, 2, 13) and tuple(hits.trace_start.shape) == (2, 2, 13, Tq)
    flat = keyword_search(x.reshape(4, Tq, V), kws, lens.repeat(2), want_trace=True)
    split = keyword_search(x, kws, lens, want_trace=True, max_workspace_bytes=4 * Tq * 8 * 5)  # five keywords per launch
    for name in FIELDS:
        assert kc.same_bits(getattr(hits, name).reshape(getattr(flat, name).shape), getattr(flat, name)), name
        assert kc.same_bits(getattr(hits, name), getattr(split, name)), name
    assert hits.first_exit(-1.0e30).shape == (2, 13)
    assert bool((hits.trace_score[:, 0, :, 33:] == float("-inf")).all()) and bool((hits.trace_start[:, 0, :, 33:] == -1).all())


def test_spot_is_one_encoder_pass_and_the_search_over_all_exits():
    from conftest import base_kwargs
    from early_exit_transformer_amd import synth
    from early_exit_transformer_amd.beam import BeamInference
    from early_exit_transformer_amd.model import Early_conformer, encoder_lengths, greedy_ctc

    gpu = Early_conformer(**base_kwargs(n_enc_exits=3, n_enc_layers=1, d_feed_forward=128, device="cuda")).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=61, style="trained"), strict=True)
    gpu = gpu.cuda()
    mel, lens = synth.synth_mel(3, 80, 203, seed=61).cuda(), torch.tensor([203, 150, 77])
    with torch.no_grad():
        out = gpu(mel, lens)  # [E, B, T', V]
    fl = encoder_lengths(lens.cuda(), out.size(2))
    # a phrase the last exit's greedy path of utterance 0 spells (synthetic weights: any tokens), and two it need not
    tok, cnt = greedy_ctc(out[-1], em_len=fl)
    spelled = tok[0, : int(cnt[0])].tolist()[:3] or [5]
    kws = KeywordSet([spelled, [7, 9], [11]], out.size(3))
    hits, first = BeamInference().spot(gpu, mel, lens, kws, threshold=0.0)
    want = keyword_search(out, kws, fl, want_trace=True)
    for name in FIELDS:
        assert kc.same_bits(getattr(hits, name), getattr(want, name)), name
    assert tuple(hits.score.shape) == (3, 3, 3) and tuple(first.shape) == (3, 3)
    if int(cnt[0]) >= 1:
        assert float(hits.score[-1, 0, 0]) == 0.0 and int(first[0, 0]) in (0, 1, 2)
    assert torch.equal(first, want.first_exit(0.0))
    plain = BeamInference().spot(gpu, mel, lens, kws)
    assert kc.same_bits(plain.score, want.score)


def test_graph_replay_returns_the_eager_bits():
    Tq, V, scale = 70, 32, 8
    x, em_len, phrases, _ = kc.gpu_case(Tq, V, scale)
    kws = KeywordSet(phrases, V)
    xd, ld = x.cuda(), em_len.cuda()
    eager = keyword_search(xd, kws, ld, want_trace=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        keyword_search(xd, kws, ld, want_trace=True)  # the allocator's and the keyword set's first use, outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = keyword_search(xd, kws, ld, want_trace=True)
    for name in FIELDS:
        getattr(captured, name).fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for name in FIELDS:
        assert kc.same_bits(getattr(captured, name), getattr(eager, name)), name


def test_refusals_reach_the_error_string_without_a_launch():
    lib = capi.load()
    x = torch.zeros(2, 16, 8, device="cuda")
    kws = KeywordSet([[1, 2], [3]], 8)
    tokens, lengths = kws.to(x.device)
    out_f = torch.full((2, 2), 5.0, device="cuda")
    out_i = torch.full((2, 2), 5, dtype=torch.int32, device="cuda")
    need = lib.eec_keyword_search_workspace_bytes(2, 16)
    ws, ptr = capi.aligned_ws(need, x.device)

    def call(**over):
        a = dict(logp=x, n_em=2, Tq=16, V=8, em_len=None, tokens=tokens, tok_len=lengths, K=2, tok_stride=2, blank=0, score=out_f, start=out_i,
                 end=out_i, trace_score=None, trace_start=None, ws=ptr, ws_bytes=need)
        a.update(over)
        with pytest.raises(RuntimeError) as err:
            capi.launch("eec_keyword_search", x.device, *a.values())
        return str(err.value)

    assert "K must be in 1..65536, got 0" in call(K=0)
    assert "K must be in 1..65536, got 65537" in call(K=65537)
    assert "a keyword has 1..64 tokens, got tok_stride 65" in call(tok_stride=65)
    assert "Tq must be in 1..2^20" in call(Tq=(1 << 20) + 1)
    assert "blank in [0, V)" in call(blank=8)
    assert "workspace too small" in call(ws_bytes=need - 1)
    assert "null argument" in call(tok_len=None)
    torch.cuda.synchronize()
    assert bool((out_f == 5.0).all()) and bool((out_i == 5).all())  # nothing was launched
    # what only the table's contents show is KeywordSet's to refuse ...
    for bad, msg in (([[1, 0]], "holds the blank"), ([[1, 8]], "outside"), ([[]], "1 .. 64 tokens"), ([[1] * 65], "1 .. 64 tokens")):
        with pytest.raises(ValueError, match=msg):
            KeywordSet(bad, 8)
    # ... and the device trusts no table: a blank, a token past V and a length past the table give fill values, the good row its score
    x = torch.log_softmax(torch.randn(2, 16, 8, generator=torch.Generator().manual_seed(3)), -1).cuda()
    tokens = torch.tensor([[1, 0], [1, 2], [1, 1 << 30], [1, 2]], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([2, 2, 2, 3], dtype=torch.int32, device="cuda")
    score = torch.empty((2, 4), device="cuda")
    start, end = (torch.empty((2, 4), dtype=torch.int32, device="cuda") for _ in range(2))
    capi.launch("eec_keyword_search", x.device, x, 2, 16, 8, None, tokens, lengths, 4, 2, 0, score, start, end, None, None, ptr, need)
    good = keyword_search(x, KeywordSet([[1, 2]], 8))
    assert kc.same_bits(score[:, 1:2], good.score) and kc.same_bits(end[:, 1:2], good.end)
    for k in (0, 2, 3):
        assert score[:, k].tolist() == [float("-inf")] * 2 and start[:, k].tolist() == [-1, -1] and end[:, k].tolist() == [-1, -1]
    del ws
