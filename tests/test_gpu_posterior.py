"""CTC posteriors in the standard topology on the device (csrc/ctc_posterior.hip) against the fp64 restatement of
tests/posterior_cases.py: every row of every case, nothing excluded.  The cases are tests/forced_align_cases.py's: every strip
width of the state layout (1, 2, 3, 15, 16, 17, 31 | 32, 33, 63 | 64, 65, 127 | 128, 255 tokens), T' = 37, 70 and 300, vocabularies
that are no multiple of 4, storage 4 bytes off a 16-byte boundary, flat and peaky emissions, lengths 0, 1, N + R - 1, N + R and T'
with NaN from every length on, rows that share an emission, an all-equal row that needs 2N - 1 frames, and the rows the statement
answers with fill values.  Emissions are finite inside the lengths, so every row the restatement serves has a finite ll and every
such row is compared.

The bounds are derived (posterior_cases.tolerances), not measured: bound(T, M) = T * (2^-22 * M + 4e-7) for ll, and
e = expm1(3 bound) + 2^-22 times the fp64 sum of a sum's absolute terms, plus one fp32 rounding, for every sum of posteriors and
every gamma entry.  Worst fraction of its bound per output, measured on an MI355X over all cases:
    row_logp 0.044, tok_frames 0.023, tok_score 0.023, tok_start 0.018, tok_end 0.023, tok_start_var 0.0092, tok_end_var 0.0077,
    gamma 0.023
The device has no output that holds a token's first-frame mass, so "first-frame mass = 1" is held where it shows: tok_end -
tok_start = tok_frames, the occupancy summed over the frames = tok_frames, and a frame's occupancy summed over the tokens <= 1."""
import math

import numpy as np
import pytest
import torch

import forced_align_cases as fc
import posterior_cases as pc
from early_exit_transformer_amd import capi, ctc_posteriors

pytestmark = pytest.mark.gpu
NEG = float("-inf")
FIELDS = ("row_logp",) + pc.TOKEN_FIELDS + ("gamma", "status")


def _on_device(x: torch.Tensor, off: int) -> torch.Tensor:
    """``x`` on the device, its first element ``off`` floats behind the allocation's (256-byte aligned) start."""
    buf = torch.empty(x.numel() + off, dtype=torch.float32, device="cuda")
    view = buf[off:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


def _same(a, b, what=""):
    for name in FIELDS:
        assert pc.same_bits(getattr(a, name), getattr(b, name)), (what, name)


def _check_row(out, h, want, worst):
    """Row ``h`` of the device's outputs (CPU tensors by name) against ``want``: None -- the fill values, exactly -- or the restated
    row and its sums, within the derived bounds; ``worst`` collects the largest fraction of its bound per output."""
    if want is None:
        assert int(out["status"][h]) in (1, 2) and float(out["row_logp"][h]) == NEG and not bool(out["gamma"][h].any()), h
        assert all(bool((out[n][h] == -1.0).all()) for n in pc.TOKEN_FIELDS), h
        return
    r, s = want
    N, T = r["N"], r["T"]
    assert math.isfinite(r["ll"]) and int(out["status"][h]) == 0, h
    b, e, tol = pc.tolerances(r, s)
    frac = abs(float(out["row_logp"][h]) - r["ll"]) / b
    worst["row_logp"] = max(worst["row_logp"], frac)
    assert frac <= 1.0, (h, "row_logp", float(out["row_logp"][h]), r["ll"], b)
    dev = {n: out[n][h].double().numpy() for n in pc.TOKEN_FIELDS}
    for name in pc.TOKEN_FIELDS:
        assert bool((dev[name][N:] == -1.0).all()), (h, name)
        frac = float((np.abs(dev[name][:N] - s[name]) / tol[name]).max())
        worst[name] = max(worst[name], frac)
        assert frac <= 1.0, (h, name, frac)
    g = out["gamma"][h].double().numpy()
    assert not g[T:].any() and not g[:, N:].any(), h
    ref = r["gamma"][:, 1::2]
    frac = float((np.abs(g[:T, :N] - ref) / (e * ref + 2.0 ** -24 * ref + 2.0 ** -126)).max())
    worst["gamma"] = max(worst["gamma"], frac)
    assert frac <= 1.0, (h, "gamma", frac)
    # the identities, on the device's own numbers, within the same bounds
    gap = np.abs(dev["tok_end"][:N] - dev["tok_start"][:N] - dev["tok_frames"][:N])
    assert bool((gap <= tol["tok_end"] + tol["tok_start"] + tol["tok_frames"]).all()), (h, "end - start = frames")
    assert bool((np.abs(g[:T, :N].sum(0) - dev["tok_frames"][:N]) <= 2.0 * tol["tok_frames"]).all()), (h, "sum of gamma")
    assert float(g[:T].sum(1).max()) <= 1.0 + e + N * 2.0 ** -24, (h, "a frame's occupancy")


def _worst():
    return dict.fromkeys(("row_logp",) + pc.TOKEN_FIELDS + ("gamma",), 0.0)


@pytest.mark.parametrize("Tq,V,scale", pc.GPU_CASES)
def test_device_is_within_the_derived_bounds_of_the_restatement(Tq, V, scale):
    x, em_len, rows, _, _ = fc.gpu_case(Tq, V, scale)
    tokens, tok_len, em_index = fc.case_tensors(Tq, V, scale)
    off = 1 if (Tq + V + scale) % 2 else 0  # half of the cases read storage 4 bytes off a 16-byte boundary
    got = ctc_posteriors(_on_device(x, off), tokens.cuda(), tok_len.cuda(), em_index.cuda(), em_len.cuda(), want_gamma=True)
    out = {n: getattr(got, n).cpu() for n in FIELDS}
    assert out["gamma"].shape == (len(rows), Tq, fc.S_MAX) and all(out[n].dtype == torch.float32 for n in FIELDS[:-1])
    worst = _worst()
    expected = pc.expected(Tq, V, scale)
    for h, want in enumerate(expected):  # every row: statuses and fills exactly, served rows within the bounds
        assert int(out["status"][h]) == (1 if want is None else 0), h
        _check_row(out, h, want, worst)
    served = sum(w is not None for w in expected)
    print(f"T'={Tq} V={V} scale={scale}: {served} rows served, {len(expected) - served} refused; worst fraction of the bound: "
          + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    assert served >= 8 and len(expected) - served >= 10


def test_minus_infinity_emissions_and_status_two_on_the_device():
    """-inf is an ordinary value: rows are aligned around the frames an emission forbids a label in, within the same bounds (the
    restatement's M is the largest FINITE magnitude), and a row every alignment of which crosses a forbidden frame has status 2
    and the fill values; its neighbours are untouched."""
    Tq, V = 41, 9
    x = torch.log_softmax(torch.randn(2, Tq, V, generator=torch.Generator().manual_seed(5)) * 2.0, -1)
    x[0, :20, 2] = NEG     # label 2 cannot be said in the first 20 frames of emission 0
    x[0, 30:, 0] = NEG     # ... and its last frames cannot be blank
    x[1, :, 2] = NEG       # emission 1 never says label 2
    rows = [[1, 2, 3], [1, 2, 3], [1, 3], [2], [4, 5] * 15 + [2, 6, 4], [3, 1] * 10]
    em = [0, 1, 1, 1, 0, 1]
    tokens = torch.zeros((len(rows), 40), dtype=torch.int32)
    for h, r in enumerate(rows):
        tokens[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
    tok_len = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    got = ctc_posteriors(x.cuda(), tokens.cuda(), tok_len.cuda(), torch.tensor(em).cuda(), want_gamma=True)
    out = {n: getattr(got, n).cpu() for n in FIELDS}
    assert out["status"].tolist() == [0, 2, 0, 2, 0, 0]
    worst = _worst()
    for h, r in enumerate(rows):
        want = pc.restate(x[em[h]].numpy(), Tq, r, 0)
        assert want is not None
        _check_row(out, h, (want, pc.token_sums(want)) if math.isfinite(want["ll"]) else None, worst)
    assert not bool(out["gamma"][0, :20, 1].any()) and bool(torch.isfinite(out["tok_score"][0, :3]).all())
    print("-inf emissions: worst fraction of the bound: " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


def test_same_bits_under_every_way_of_calling():
    Tq, V, scale = 70, 37, 8
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    tokens, tok_len, em_index = (t.cuda() for t in fc.case_tensors(Tq, V, scale))
    xd, ld = x.cuda(), em_len.cuda()
    first = ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True)
    assert int((first.status == 0).sum()) >= 8
    _same(first, ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True), "a second run")
    lean = ctc_posteriors(xd, tokens, tok_len, em_index, ld)
    assert lean.gamma is None and all(pc.same_bits(getattr(lean, n), getattr(first, n)) for n in FIELDS if n != "gamma")
    H = tokens.size(0)
    for cut in (1, 7, H - 1):  # a split over rows
        parts = [ctc_posteriors(xd, tokens[a:b], tok_len[a:b], em_index[a:b], ld, want_gamma=True) for a, b in ((0, cut), (cut, H))]
        for name in FIELDS:
            assert pc.same_bits(torch.cat([getattr(p, name) for p in parts]), getattr(first, name)), (cut, name)
    per_row = capi.load().eec_ctc_posteriors_workspace_bytes(1, Tq, fc.S_MAX)
    _same(first, ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True, max_workspace_bytes=5 * per_row), "five rows per launch")
    _same(first, ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True, max_workspace_bytes=1), "one row per launch")
    # a narrower token table: the strip width comes from the row's own length, not from the table's
    narrow = ctc_posteriors(xd, tokens[:8, :32], tok_len[:8], em_index[:8], ld)
    for name in ("row_logp", "status"):
        assert pc.same_bits(getattr(narrow, name), getattr(first, name)[:8]), name
    for name in pc.TOKEN_FIELDS:
        assert pc.same_bits(getattr(narrow, name), getattr(first, name)[:8, :32].contiguous()), name
    # em_len = None against lengths all T', and no em_index against the rows' own indices (split and unsplit)
    clean = torch.nan_to_num(xd[4:6], nan=-1.0)
    rows = tokens[:2]
    whole = ctc_posteriors(clean, rows, tok_len[:2], want_gamma=True)
    _same(whole, ctc_posteriors(clean, rows, tok_len[:2], torch.tensor([0, 1]), torch.tensor([Tq, Tq]), want_gamma=True), "spelled out")
    _same(whole, ctc_posteriors(clean, rows, tok_len[:2], want_gamma=True, max_workspace_bytes=1), "no em_index, split")
    assert whole.status.tolist() == [0, 0]
    # [E, B, T', V] input against its flattened form; lengths [B] shared by the exits
    x4 = torch.nan_to_num(xd[2:6], nan=-1.0).reshape(2, 2, Tq, V)
    idx = torch.tensor([0, 3, 2, 1, 3], dtype=torch.int32)
    lens = torch.tensor([33, Tq], dtype=torch.int32)
    a = ctc_posteriors(x4, tokens[:5], tok_len[:5], idx, lens, want_gamma=True)
    _same(a, ctc_posteriors(x4.reshape(4, Tq, V), tokens[:5], tok_len[:5], idx, lens.repeat(2), want_gamma=True), "flattened")
    assert not bool(a.gamma[0, 33:].any()) and bool(a.gamma[1, Tq - 1].any())


def test_graph_replay_returns_the_eager_bits():
    Tq, V, scale = 70, 37, 8
    x, em_len, _, _, _ = fc.gpu_case(Tq, V, scale)
    tokens, tok_len, em_index = (t.cuda() for t in fc.case_tensors(Tq, V, scale))
    xd, ld = x.cuda(), em_len.cuda()
    eager = ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True)  # the allocator's first use, outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ctc_posteriors(xd, tokens, tok_len, em_index, ld, want_gamma=True)
    for name in FIELDS:
        getattr(captured, name).fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    _same(captured, eager, "replay")


def test_confidences_is_one_encoder_pass_and_one_posterior_call():
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
    hyps = [h or [5] for h in gpu.greedy_decode(out, lengths=fl)[-1]]  # a greedy transcript (synthetic weights: any tokens)
    S = max(len(h) for h in hyps)

    def by_hand(rows, em_index):
        tokens = torch.zeros((len(rows), max(len(r) for r in rows)), dtype=torch.int32)
        for h, r in enumerate(rows):
            tokens[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
        return ctc_posteriors(out, tokens, torch.tensor([len(r) for r in rows]), torch.tensor(em_index), fl)

    bi = BeamInference()
    every = bi.confidences(gpu, mel, lens, hyps, exits="all", pieces=["▁w%d" % v if v % 3 == 0 else "p%d" % v for v in range(V)])
    direct = by_hand([hyps[b] for _ in range(E) for b in range(B)], list(range(E * B)))
    _same(every.posteriors, direct, "all")
    assert len(every.tokens) == E and len(every.tokens[0]) == B and len(every.words) == E
    host = {n: getattr(direct, n).cpu() for n in FIELDS if n != "gamma"}
    for e in range(E):
        for b in range(B):
            h, spans = e * B + b, every.tokens[e][b]
            if int(host["status"][h]) != 0:
                assert spans == []
                continue
            assert [sp.token for sp in spans] == hyps[b]
            for j, sp in enumerate(spans):  # the row of exit e equals the direct call on that exit's emission
                assert sp.start == float(host["tok_start"][h, j]) * 0.04 and sp.end == float(host["tok_end"][h, j]) * 0.04
                assert sp.frames == float(host["tok_frames"][h, j]) and 0.0 < sp.confidence <= 1.0 + 1e-6
                assert sp.confidence == math.exp(float(host["tok_score"][h, j]) / float(host["tok_frames"][h, j]))
            assert sum(len(w.tokens) for w in every.words[e][b]) == len(hyps[b])
    assert int((host["status"][(E - 1) * B:] == 0).sum()) == B  # the last exit said these tokens: it can align them
    last = bi.confidences(gpu, mel, lens, hyps)
    _same(last.posteriors, by_hand(hyps, [(E - 1) * B + b for b in range(B)]), "exits=None")
    assert tuple(last.posteriors.tok_start.shape) == (B, S) and last.words is None and len(last.tokens) == B
    per = bi.confidences(gpu, mel, lens, hyps, exits=[0, 2, 1])
    _same(per.posteriors, by_hand(hyps, [0 * B + 0, 2 * B + 1, 1 * B + 2]), "one exit per utterance")


def test_refusals_reach_the_error_string_without_a_launch():
    lib = capi.load()
    x = torch.zeros(2, 16, 8, device="cuda")
    tokens = torch.tensor([[1, 2], [3, 0]], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    out_i = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    out_f = torch.full((2, 16, 2), 5.0, device="cuda")
    need = lib.eec_ctc_posteriors_workspace_bytes(2, 16, 2)
    ws, ptr = capi.aligned_ws(need, x.device)

    def call(**over):
        a = dict(logp=x, n_em=2, Tq=16, V=8, em_len=None, tokens=tokens, tok_len=lengths, em_index=None, n_hyp=2, tok_stride=2, blank=0,
                 row_logp=out_f, tok_frames=out_f, tok_score=out_f, tok_start=out_f, tok_end=out_f, tok_start_var=out_f, tok_end_var=out_f,
                 gamma=out_f, status=out_i, ws=ptr, ws_bytes=need)
        a.update(over)
        with pytest.raises(RuntimeError) as err:
            capi.launch("eec_ctc_posteriors", x.device, *a.values())
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
