"""CTC forced alignment in the standard topology on the device (csrc/ctc_forced_align.hip) against the scalar restatement of
tests/forced_align_cases.py and the NumPy host path, bit for bit: every row of every case, nothing excluded.  The cases cross every
strip width of the state layout (N = 31 / 32, 63 / 64, 127 / 128 and 255 tokens: 1, 2, 4, 8 states per lane), the 64-frame blocks of
the walk back and the look-ahead (T' = 37, 70, 300), vocabularies that are no multiple of 4, storage 4 bytes off a 16-byte boundary,
lengths 0, 1, N + R - 1, N + R and T' with NaN from every length on, rows that share an emission, an all-equal row that needs
2N - 1 frames, and the rows the statement answers with fill values."""
import pytest
import torch

import forced_align_cases as fc
from early_exit_transformer_amd import capi, ctc_forced_align

pytestmark = pytest.mark.gpu
NEG = float("-inf")


def _on_device(x: torch.Tensor, off: int) -> torch.Tensor:
    """``x`` on the device, its first element ``off`` floats behind the allocation's (256-byte aligned) start."""
    buf = torch.empty(x.numel() + off, dtype=torch.float32, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


def _same(a, b, what=""):
    for name in fc.FIELDS:
        assert fc.same_bits(getattr(a, name), getattr(b, name)), (what, name)


@pytest.mark.parametrize("Tq,V,scale", fc.GPU_CASES)
def test_device_equals_restatement_and_host_path(Tq, V, scale):
    x, em_len, rows, _, _ = fc.gpu_case(Tq, V, scale)
    want = fc.gpu_case_expected(Tq, V, scale)
    tokens, tok_len, em_index = fc.case_tensors(Tq, V, scale)
    off = 1 if (Tq + V + scale) % 2 else 0  # half of the cases read storage 4 bytes off a 16-byte boundary
    got = ctc_forced_align(_on_device(x, off), tokens.cuda(), tok_len.cuda(), em_index.cuda(), em_len.cuda())
    for name, ref in zip(fc.FIELDS, want):
        out = getattr(got, name)
        assert out.dtype == ref.dtype and fc.same_bits(out, ref), name
    _same(got, ctc_forced_align(x, tokens, tok_len, em_index, em_len), "host path")
    # status-1 rows hold exactly the fill values (their neighbours were compared above: they are untouched)
    bad = (want[5] == 1).nonzero().flatten().tolist()
    assert len(bad) >= 10 and int(want[5][-1]) == 0
    for h in bad:
        assert int(got.status[h]) == 1 and float(got.path_score[h]) == NEG
        assert bool((got.frame_token[h] == -2).all()) and bool((got.tok_start[h] == -1).all()) and bool((got.tok_end[h] == -1).all())
        assert bool((got.tok_score[h] == NEG).all())


def test_same_bits_under_every_way_of_calling():
    Tq, V, scale = 70, 37, 8
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    tokens, tok_len, em_index = (t.cuda() for t in fc.case_tensors(Tq, V, scale))
    xd, ld = x.cuda(), em_len.cuda()
    first = ctc_forced_align(xd, tokens, tok_len, em_index, ld)
    _same(first, ctc_forced_align(xd, tokens, tok_len, em_index, ld), "a second run")
    H = tokens.size(0)
    for cut in (1, 7, H - 1):  # a split over hypotheses
        parts = [ctc_forced_align(xd, tokens[a:b], tok_len[a:b], em_index[a:b], ld) for a, b in ((0, cut), (cut, H))]
        for name in fc.FIELDS:
            assert fc.same_bits(torch.cat([getattr(p, name) for p in parts]), getattr(first, name)), (cut, name)
    per_row = capi.load().eec_ctc_forced_align_workspace_bytes(1, Tq, fc.S_MAX)
    _same(first, ctc_forced_align(xd, tokens, tok_len, em_index, ld, max_workspace_bytes=5 * per_row), "five rows per launch")
    _same(first, ctc_forced_align(xd, tokens, tok_len, em_index, ld, max_workspace_bytes=1), "one row per launch")
    # em_len = None against lengths all T', and no em_index against the rows' own indices (split and unsplit)
    clean = torch.nan_to_num(xd[4:6], nan=-1.0)
    rows = tokens[:2]
    whole = ctc_forced_align(clean, rows, tok_len[:2])
    _same(whole, ctc_forced_align(clean, rows, tok_len[:2], torch.tensor([0, 1]), torch.tensor([Tq, Tq])), "em_len and em_index spelled out")
    _same(whole, ctc_forced_align(clean, rows, tok_len[:2], max_workspace_bytes=1), "no em_index, split")
    assert whole.status.tolist() == [0, 0]
    # [E, B, T', V] input against its flattened form; lengths [B] shared by the exits
    x4 = torch.nan_to_num(xd[2:6], nan=-1.0).reshape(2, 2, Tq, V)
    idx = torch.tensor([0, 3, 2, 1, 3], dtype=torch.int32)
    lens = torch.tensor([33, Tq], dtype=torch.int32)
    a = ctc_forced_align(x4, tokens[:5], tok_len[:5], idx, lens)
    _same(a, ctc_forced_align(x4.reshape(4, Tq, V), tokens[:5], tok_len[:5], idx, lens.repeat(2)), "flattened")
    assert bool((a.frame_token[0, 33:] == -2).all()) and int(a.frame_token[1, Tq - 1]) != -2


def test_graph_replay_returns_the_eager_bits():
    Tq, V, scale = 70, 32, 8
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    tokens, tok_len, em_index = (t.cuda() for t in fc.case_tensors(Tq, V, scale))
    xd, ld = x.cuda(), em_len.cuda()
    eager = ctc_forced_align(xd, tokens, tok_len, em_index, ld)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ctc_forced_align(xd, tokens, tok_len, em_index, ld)  # the allocator's first use, outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ctc_forced_align(xd, tokens, tok_len, em_index, ld)
    for name in fc.FIELDS:
        getattr(captured, name).fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    _same(captured, eager, "replay")


def test_timestamps_is_one_encoder_pass_and_one_alignment():
    from conftest import base_kwargs
    from early_exit_transformer_amd import synth
    from early_exit_transformer_amd.beam import BeamInference
    from early_exit_transformer_amd.model import Early_conformer, encoder_lengths

    gpu = Early_conformer(**base_kwargs(n_enc_exits=3, n_enc_layers=1, d_feed_forward=128, device="cuda")).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=61, style="trained"), strict=True)
    gpu = gpu.cuda()
    mel, lens = synth.synth_mel(3, 80, 203, seed=61).cuda(), torch.tensor([203, 150, 77])
    with torch.no_grad():
        out = gpu(mel, lens)  # [E, B, T', V]
    E, B, Tq, V = out.shape
    fl = encoder_lengths(lens.cuda(), Tq)
    greedy = gpu.greedy_decode(out, lengths=fl)  # [E][B] token lists
    hyps = [h or [5] for h in greedy[-1]]  # synthetic weights: any tokens
    S = max(len(h) for h in hyps)

    def by_hand(rows, em_index):
        tokens = torch.zeros((len(rows), max(len(r) for r in rows)), dtype=torch.int32)
        for h, r in enumerate(rows):
            tokens[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
        return ctc_forced_align(out, tokens, torch.tensor([len(r) for r in rows]), torch.tensor(em_index), fl)

    bi = BeamInference()
    last = bi.timestamps(gpu, mel, lens, hyps)
    _same(last.alignment, by_hand(hyps, [(E - 1) * B + b for b in range(B)]), "exits=None")
    assert tuple(last.alignment.tok_start.shape) == (B, S) and last.words is None and len(last.tokens) == B
    per = bi.timestamps(gpu, mel, lens, hyps, exits=[0, 2, 1])
    _same(per.alignment, by_hand(hyps, [0 * B + 0, 2 * B + 1, 1 * B + 2]), "one exit per utterance")
    every = bi.timestamps(gpu, mel, lens, hyps, exits="all", pieces=["▁w%d" % v if v % 3 == 0 else "p%d" % v for v in range(V)])
    _same(every.alignment, by_hand([hyps[b] for _ in range(E) for b in range(B)], list(range(E * B))), "all")
    assert len(every.tokens) == E and len(every.tokens[0]) == B and len(every.words) == E
    # aligning greedy decoding's own output at an exit follows the greedy frame labels, and scores the sum of the frame maxima
    said = [h for h in range(E * B) if greedy[h // B][h % B]]
    assert said
    own = by_hand([greedy[h // B][h % B] for h in said], said)
    assert own.status.tolist() == [0] * len(said)
    top, arg = (t.cpu() for t in out.reshape(E * B, Tq, V).max(dim=-1))
    for i, h in enumerate(said):
        T, row = int(fl[h % B]), greedy[h // B][h % B]
        ft, lab = own.frame_token[i, :T].tolist(), arg[h, :T].tolist()
        for t in range(T):
            if lab[t] != 0:  # wherever the greedy frame label is a label, the aligned token is that label
                assert ft[t] >= 0 and row[ft[t]] == lab[t], (h, t)
        acc = top[h, 0]
        for t in range(1, T):
            acc = acc + top[h, t]  # one fp32 add per frame, in frame order
        assert fc.same_bits(acc.reshape(1), own.path_score[i].reshape(1)), h
    spans = every.tokens[E - 1][0]
    assert [sp.token for sp in spans] == hyps[0] and all(0.0 <= sp.start < sp.end <= Tq * 0.04 + 1e-9 for sp in spans)
    assert sum(len(w.tokens) for w in every.words[E - 1][0]) == len(hyps[0])


def test_refusals_reach_the_error_string_without_a_launch():
    lib = capi.load()
    x = torch.zeros(2, 16, 8, device="cuda")
    tokens = torch.tensor([[1, 2], [3, 0]], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    out_i = torch.full((2, 16), 5, dtype=torch.int32, device="cuda")
    out_f = torch.full((2, 2), 5.0, device="cuda")
    need = lib.eec_ctc_forced_align_workspace_bytes(2, 16, 2)
    ws, ptr = capi.aligned_ws(need, x.device)

    def call(**over):
        a = dict(logp=x, n_em=2, Tq=16, V=8, em_len=None, tokens=tokens, tok_len=lengths, em_index=None, n_hyp=2, tok_stride=2, blank=0,
                 tok_start=out_i, tok_end=out_i, tok_score=out_f, frame_token=out_i, path_score=out_f, status=out_i, ws=ptr, ws_bytes=need)
        a.update(over)
        with pytest.raises(RuntimeError) as err:
            capi.launch("eec_ctc_forced_align", x.device, *a.values())
        return str(err.value)

    assert "blank in [0, V)" in call(blank=8)
    assert "blank in [0, V)" in call(tok_stride=0)
    assert "tok_stride <= 255" in call(tok_stride=256)
    assert "null argument" in call(tok_len=None)
    assert "workspace too small" in call(ws_bytes=need - 1)
    assert "256-byte aligned" in call(ws=ptr + 8)
    torch.cuda.synchronize()
    assert bool((out_f == 5.0).all()) and bool((out_i == 5).all())  # nothing was launched
    del ws
