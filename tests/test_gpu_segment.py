"""CTC segmentation on the device (csrc/ctc_segment.hip) against the NumPy host path of ``ctc_segment`` (which
tests/test_host_segment.py holds to the scalar restatement), every field of every row, bit for bit: rows on either side of every
wave boundary of the state layout (512 states, 256 tokens a wave), equal and unequal neighbours exactly at such a boundary, short
rows in the widest launch, the rows answered with fill values, every way of calling, and the layers above -- the windowed encoder
pass and ``BeamInference.segment``."""
import functools

import numpy as np
import pytest
import torch

import forced_align_cases as fc
import segment_cases as sc
from early_exit_transformer_amd import capi, ctc_forced_align, ctc_segment, utterance_spans, windowed_emission

pytestmark = pytest.mark.gpu
WAVE_N = (255, 256, 257, 511, 512, 513, 767, 1023, 1024, 2047, 2048, 4095)


def _on_device(x: torch.Tensor, off: int) -> torch.Tensor:
    """``x`` on the device, its first element ``off`` floats behind the allocation's (256-byte aligned) start."""
    buf = torch.empty(x.numel() + off, dtype=torch.float32, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


def _flags(flags):
    return dict(free_start=bool(flags & sc.FREE_START), free_end=bool(flags & sc.FREE_END))


def _both(x, tokens, tok_len, em_index, em_len, flags, off=0):
    """(device result, host result) of one call."""
    dev = ctc_segment(_on_device(x, off), tokens.cuda(), tok_len.cuda(), None if em_index is None else em_index.cuda(),
                      None if em_len is None else em_len.cuda(), **_flags(flags))
    return dev, ctc_segment(x, tokens, tok_len, em_index, em_len, **_flags(flags))


@pytest.mark.parametrize("V", (5, 37))
@pytest.mark.parametrize("N", WAVE_N)
def test_rows_on_either_side_of_every_wave_boundary(N, V):
    """One row of N tokens against emissions of N + R + 0, 1 and 65 frames (NaN from each length on), the flag settings in turn
    across the set, the storage 4 bytes off a 16-byte boundary in half of the cases."""
    k = WAVE_N.index(N) + (V == 37)
    flags = sc.ALL_FLAGS[k % 4]
    rng = np.random.default_rng(31 * N + V)
    row = sc.random_row(rng, N, V)
    need = N + fc.adjacent_equal(row)
    lens = torch.tensor([need, need + 1, need + 65], dtype=torch.int32)
    x = sc.emission(rng, 3, need + 65, V, 8 if k % 3 else 1)
    for n in range(3):
        x[n, int(lens[n]):] = float("nan")
    tokens, tok_len = sc.pad_rows([row] * 3)
    dev, host = _both(x, tokens, tok_len, torch.arange(3, dtype=torch.int32), lens, flags, off=k % 2)
    sc.same(dev, host, (N, V, flags))
    assert host.status.tolist() == [0, 0, 0]
    assert [int((dev.frame_token[n] == -2).sum()) for n in range(3)] == [65, 64, 0]


def _equal_at(row, pairs):
    """``row`` (no adjacent equal labels, of 1 .. 8) with token b made equal to token a for every pair, and no other pair equal."""
    row = list(row)
    for a, b in pairs:
        row[b] = row[a]
        row[b + 1] = next(v for v in range(1, 9) if v != row[b] and v != row[b + 2])
    return row


def test_neighbours_exactly_at_a_wave_boundary():
    """Tokens 255 | 256, 511 | 512 and 2047 | 2048 are the last label of one wave and the first of the next: equal, the skip across
    the edge is forbidden and a blank frame is forced (R counts them: one frame fewer is not alignable); unequal, it is allowed."""
    pairs = ((255, 256), (511, 512), (2047, 2048))
    rng = np.random.default_rng(5)
    N = 2100
    ne = sc.random_row(rng, N, 9, repeats=False)
    eq = _equal_at(ne, pairs)
    assert all(eq[a] == eq[b] and ne[a] != ne[b] for a, b in pairs)
    R = fc.adjacent_equal(eq)
    assert R == 3 and fc.adjacent_equal(ne) == 0
    x = sc.emission(rng, 2, N + R + 2, 9, 8)
    lens = torch.tensor([N + R, N + R - 1], dtype=torch.int32)
    tokens, tok_len = sc.pad_rows([eq, ne, eq, ne])
    em_index = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    for flags in (0, 3):
        dev, host = _both(x, tokens, tok_len, em_index, lens, flags)
        sc.same(dev, host, flags)
        assert host.status.tolist() == [0, 0, 1, 0]  # the equal row needs all N + R frames
        for a, b in pairs:  # a blank frame stands between the equal neighbours
            assert int(dev.tok_start[0, b]) > int(dev.tok_end[0, a])


def test_all_equal_row_of_300_tokens_needs_2n_minus_1_frames():
    rng = np.random.default_rng(6)
    x = sc.emission(rng, 2, 599, 5, 8)
    tokens, tok_len = sc.pad_rows([[3] * 300] * 2)
    dev, host = _both(x, tokens, tok_len, None, torch.tensor([599, 598], dtype=torch.int32), 0)
    sc.same(dev, host)
    assert dev.status.tolist() == [0, 1] and dev.frame_token[0].tolist() == [j // 2 if j % 2 == 0 else -1 for j in range(599)]


@functools.lru_cache(maxsize=None)
def _wide_launch():
    """tok_stride = 4095: rows of 1, 3, 255, 256 and 4095 tokens with the rows the statement refuses between them."""
    rng = np.random.default_rng(8)
    V, S = 11, 4095
    good = {n: sc.random_row(rng, n, V, repeats=False) for n in (1, 3, 255, 256, 4095)}
    rows = [good[1], [1, 2, 3], good[3], [1, 2, V, 3], good[255], [1, 0, 2], good[256], [1, 2, 3], [1, 2, 3], good[4095], [1, 2, 3],
            [4, 3, 2, 1]]
    tokens, tok_len = sc.pad_rows(rows, S)
    tok_len[1] = 4096   # more tokens than the stride
    tok_len[8] = 0      # N = 0
    em_index = torch.tensor([0, 0, 1, 0, 1, 0, 0, 2, 0, 1, -1, 1], dtype=torch.int32)  # rows 7 and 10: no such emission
    x = sc.emission(rng, 2, 4100, V, 8)
    bad = [1, 3, 5, 7, 8, 10]
    return _both(x, tokens, tok_len, em_index, None, 3) + (bad,)


def test_short_rows_in_the_widest_launch():
    dev, host, bad = _wide_launch()
    sc.same(dev, host)
    assert [int(s) for s in dev.status] == [1 if h in bad else 0 for h in range(12)]
    assert int(dev.tok_end[9, 4094]) > int(dev.tok_start[9, 4094]) >= 4094


def test_bad_rows_get_the_fill_values_and_leave_their_neighbours_alone():
    dev, host, bad = _wide_launch()
    for h in range(12):
        assert sc.is_fill(dev, h) == (h in bad), h
    for name in sc.FIELDS:  # the neighbours hold exactly what the host path gives them
        for h in (0, 2, 4, 6, 9, 11):
            assert fc.same_bits(getattr(dev, name)[h], getattr(host, name)[h]), (name, h)


def test_rows_of_at_most_255_tokens_equal_the_one_wave_kernel():
    for Tq, V, scale in ((70, 37, 8), (300, 5, 1)):
        x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
        tokens, tok_len, em_index = (t.cuda() for t in fc.case_tensors(Tq, V, scale))
        xd, ld = x.cuda(), em_len.cuda()
        sc.same(ctc_segment(xd, tokens, tok_len, em_index, ld), ctc_forced_align(xd, tokens, tok_len, em_index, ld), (Tq, V, scale))


@functools.lru_cache(maxsize=None)
def _calling_case():
    rng = np.random.default_rng(9)
    V, Tq = 13, 700
    rows = [sc.random_row(rng, n, V) for n in (600, 257, 1, 512, 300)] + [[1, 0, 2]]
    tokens, tok_len = sc.pad_rows(rows)
    x = sc.emission(rng, 4, Tq, V, 8)
    em_index = torch.tensor([0, 1, 2, 3, 1, 0], dtype=torch.int32)
    lens = torch.tensor([Tq, 500, 40, Tq], dtype=torch.int32)
    return x, tokens, tok_len, em_index, lens


def test_same_bits_under_every_way_of_calling():
    x, tokens, tok_len, em_index, lens = _calling_case()
    xd, tokens, tok_len, em_index, ld = x.cuda(), tokens.cuda(), tok_len.cuda(), em_index.cuda(), lens.cuda()
    kw = _flags(3)
    first = ctc_segment(xd, tokens, tok_len, em_index, ld, **kw)
    sc.same(first, ctc_segment(x, tokens.cpu(), tok_len.cpu(), em_index.cpu(), lens, **kw), "host path")
    assert first.status.tolist() == [0, 0, 0, 0, 0, 1]
    sc.same(first, ctc_segment(xd, tokens, tok_len, em_index, ld, **kw), "a second run")
    H = tokens.size(0)
    for cut in (1, 3, H - 1):  # a split over rows
        parts = [ctc_segment(xd, tokens[a:b], tok_len[a:b], em_index[a:b], ld, **kw) for a, b in ((0, cut), (cut, H))]
        for name in sc.FIELDS:
            assert fc.same_bits(torch.cat([getattr(p, name) for p in parts]), getattr(first, name)), (cut, name)
    per_row = capi.load().eec_ctc_segment_workspace_bytes(1, x.size(1), tokens.size(1))
    assert per_row == 350 * 3 * 256
    sc.same(first, ctc_segment(xd, tokens, tok_len, em_index, ld, max_workspace_bytes=per_row, **kw), "one row per launch")
    sc.same(first, ctc_segment(xd, tokens, tok_len, em_index, ld, max_workspace_bytes=2 * per_row + 1, **kw), "two rows per launch")
    with pytest.raises(ValueError, match=f"needs {per_row} bytes"):
        ctc_segment(xd, tokens, tok_len, em_index, ld, max_workspace_bytes=per_row - 1, **kw)
    # [E, B, T', V] input against its flattened form; lengths [B] shared by the exits
    x4 = xd.reshape(2, 2, x.size(1), x.size(2))
    idx = torch.tensor([0, 3, 2, 1, 3], dtype=torch.int32)
    l2 = torch.tensor([450, 700], dtype=torch.int32)
    a = ctc_segment(x4, tokens[1:], tok_len[1:], idx, l2, **kw)
    sc.same(a, ctc_segment(xd, tokens[1:], tok_len[1:], idx, l2.repeat(2), **kw), "flattened")
    assert bool((a.frame_token[0, 450:] == -2).all()) and int(a.frame_token[1, 699]) != -2


def test_graph_replay_returns_the_eager_bits():
    x, tokens, tok_len, em_index, lens = (t.cuda() for t in _calling_case())
    kw = _flags(1)
    eager = ctc_segment(x, tokens, tok_len, em_index, lens, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ctc_segment(x, tokens, tok_len, em_index, lens, **kw)  # the allocator's first use, outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ctc_segment(x, tokens, tok_len, em_index, lens, **kw)
    for name in sc.FIELDS:
        getattr(captured, name).fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    sc.same(captured, eager, "replay")


def test_refusals_reach_the_error_string_without_a_launch():
    lib = capi.load()
    x = torch.zeros(2, 16, 8, device="cuda")
    tokens = torch.tensor([[1, 2], [3, 0]], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    out_i = torch.full((2, 16), 5, dtype=torch.int32, device="cuda")
    out_f = torch.full((2, 2), 5.0, device="cuda")
    need = lib.eec_ctc_segment_workspace_bytes(2, 16, 2)
    ws, ptr = capi.aligned_ws(need, x.device)

    def call(**over):
        a = dict(logp=x, n_em=2, Tq=16, V=8, em_len=None, tokens=tokens, tok_len=lengths, em_index=None, n_hyp=2, tok_stride=2, blank=0,
                 flags=0, tok_start=out_i, tok_end=out_i, tok_score=out_f, frame_token=out_i, path_score=out_f, status=out_i, ws=ptr,
                 ws_bytes=need)
        a.update(over)
        with pytest.raises(RuntimeError) as err:
            capi.launch("eec_ctc_segment", x.device, *a.values())
        return str(err.value)

    assert "blank in [0, V)" in call(blank=8)
    assert "blank in [0, V)" in call(tok_stride=0)
    assert "tok_stride <= 4095" in call(tok_stride=4096)
    assert "flags" in call(flags=4)
    assert "null argument" in call(tok_len=None)
    assert "workspace too small" in call(ws_bytes=need - 1)
    assert "256-byte aligned" in call(ws=ptr + 8)
    torch.cuda.synchronize()
    assert bool((out_f == 5.0).all()) and bool((out_i == 5).all())  # nothing was launched
    del ws


@functools.lru_cache(maxsize=None)
def _small_model():
    from conftest import base_kwargs
    from early_exit_transformer_amd import synth
    from early_exit_transformer_amd.model import Early_conformer

    gpu = Early_conformer(**base_kwargs(n_enc_exits=3, n_enc_layers=1, d_feed_forward=128, device="cuda")).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=61, style="trained"), strict=True)
    return gpu.cuda(), synth.synth_mel(1, 80, 603, seed=62).cuda()[0]


def _windows_by_hand(model, mel, window, hop):
    """Every window's own forward: the windows of ``mel`` zero-padded to ``window`` frames, run with their true lengths."""
    T = mel.size(1)
    starts = list(range(0, T - window + hop, hop)) if T > window else [0]
    batch = mel.new_zeros((len(starts), mel.size(0), window))
    true = [min(window, T - s) for s in starts]
    for k, s in enumerate(starts):
        batch[k, :, :true[k]] = mel[:, s:s + true[k]]
    with torch.no_grad():
        return model(batch, torch.tensor(true)), true


def test_windowed_emission_stitches_each_windows_own_forward():
    model, mel = _small_model()
    window, overlap = 200, 40
    hop = window - overlap
    got = windowed_emission(model, mel, window, overlap)
    own, true = _windows_by_hand(model, mel, window, hop)
    n_win = own.size(1)
    assert n_win == 4 and true[-1] == 603 - 3 * hop
    total = (n_win - 1) * hop // 4 + min(true[-1] // 4, own.size(2))
    assert tuple(got.shape) == (3, 1, total, own.size(3))
    for g in range(total):  # the stated rule, frame by frame
        i = min(max((g - overlap // 8) // (hop // 4), 0), n_win - 1)
        assert torch.equal(got[:, 0, g], own[:, i, g - i * hop // 4]), g
    again = windowed_emission(model, mel[None], window, overlap, batch=3)  # [1, n_mels, T] input, two batches
    assert tuple(again.shape) == tuple(got.shape)
    short = mel[:, :180]
    with torch.no_grad():
        assert torch.equal(windowed_emission(model, short, window, overlap), model(short[None], torch.tensor([180])))


def test_segment_is_the_composition_of_its_three_calls():
    from early_exit_transformer_amd.beam import BeamInference

    model, mel = _small_model()
    V = 256
    utterances = [[5, 9, 9, 17], [33], [120, 7, 64, 64, 2, 19]]
    pieces = ["▁w%d" % v if v % 3 == 0 else "p%d" % v for v in range(V)]
    bi = BeamInference()
    got = bi.segment(model, mel, utterances, exit=1, window=200, overlap=40, pieces=pieces, score_window=7)
    logp = windowed_emission(model, mel, 200, 40)
    row = logp[1, 0]
    al = ctc_segment(row[None], torch.tensor([[t for u in utterances for t in u]]), free_start=True, free_end=True)
    sc.same(got.alignment, al)
    assert int(al.status[0]) == 0
    want = utterance_spans(al, 0, [4, 1, 6], row, window=7, frame_seconds=0.04)
    assert got.utterances == want and len(want) == 3 and [u.n_tokens for u in want] == [4, 1, 6]
    assert all(0.0 <= a.start < a.end <= b.start for a, b in zip(want, want[1:]))
    assert [sum(len(w.tokens) for w in ws) for ws in got.words] == [4, 1, 6]
    last = bi.segment(model, mel, utterances, window=200, overlap=40)  # the last exit by default, no words
    sc.same(last.alignment, ctc_segment(logp[2, 0][None], torch.tensor([[t for u in utterances for t in u]]), free_start=True, free_end=True))
    assert last.words is None
