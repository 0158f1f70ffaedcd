"""GPU tests of error-rate scoring (run with -m gpu on an MI355X): the edit-distance kernel (csrc/edit_distance.hip) against the
restatement of tests/edit_cases.py -- exact integer equality on every shared case, counts, ``n_ops`` and the written op bytes --,
its reproducibility and slice independence, and the pipeline on top of it against the host path and against decoding the exits
the adaptive walk chooses."""
import pytest
import torch

import edit_cases as X
from conftest import base_kwargs
from early_exit_transformer_amd import capi, ctc, scoring, synth
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import Early_conformer, encoder_lengths

pytestmark = pytest.mark.gpu
SENTINEL = 0xEE


def _entry(batch, want_ops=True):
    """One eec_edit_distance call on a batch of tests/edit_cases.py, the op buffer pre-filled with SENTINEL: ``EditCounts`` on the host."""
    hyp, hl, ref, rl, of = (None if t is None else t.cuda() for t in batch)
    P, Lh, Lr, R = hyp.size(0), hyp.size(1), ref.size(1), ref.size(0)
    dev = hyp.device
    lib = capi.load()
    counts = torch.full((P, 4), -7, dtype=torch.int32, device=dev)
    ops = torch.full((P, Lr + Lh), SENTINEL, dtype=torch.uint8, device=dev) if want_ops else None
    n_ops = torch.full((P,), -7, dtype=torch.int32, device=dev) if want_ops else None
    nbytes = lib.eec_edit_distance_workspace_bytes(P, Lr, Lh, int(want_ops))
    ws, ws_ptr = capi.aligned_ws(nbytes, dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    capi.check(lib.eec_edit_distance(ptr(hyp), ptr(hl), P, Lh, ptr(ref), ptr(rl), R, Lr, ptr(of), ptr(counts), ptr(ops), ptr(n_ops),
                                     ws_ptr if nbytes else None, nbytes, capi.stream_ptr(dev)), "eec_edit_distance")
    torch.cuda.synchronize()
    c = counts.cpu()
    lens = rl.clamp(0, Lr).cpu()
    of_h = torch.arange(P) if of is None else of.cpu().long()
    ok = (of_h >= 0) & (of_h < R)
    hits = torch.where(ok, lens[of_h.clamp(0, R - 1)] - c[:, 1] - c[:, 2], torch.full_like(c[:, 0], -1))
    return scoring.EditCounts(c[:, 0], c[:, 1], c[:, 2], c[:, 3], hits.to(torch.int32), None if ops is None else ops.cpu(),
                              None if n_ops is None else n_ops.cpu())


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(X.cases()))
def test_kernel_equals_the_restatement(name):
    """Counts, ``n_ops`` and the op bytes up to ``n_ops`` are the restatement's; the bytes past ``n_ops`` keep their sentinel; the launch
    without ops returns the same counts; a second run returns the same bits."""
    batch = X.cases()[name]
    got = _entry(batch)
    X.check_against_expected(name, got, sentinel=SENTINEL)
    assert _same(_entry(batch), got)
    plain = _entry(batch, want_ops=False)
    assert _same(plain[:5], got[:5])


@pytest.mark.parametrize("name", ["binary-961", "random-A5-strip4", "ref-of", "lengths-clamped"])
def test_a_call_on_a_slice_returns_the_rows_of_the_whole_call(name):
    """Slices that start inside a workgroup's four pairs, of one pair and of many; with ``ref_of`` the references stay whole,
    without it they are sliced alongside."""
    hyp, hl, ref, rl, of = X.cases()[name]
    whole = _entry((hyp, hl, ref, rl, of))
    P = hyp.size(0)
    for a, b in ((0, 1), (1, P), (P // 2 - 1, P // 2 + 2), (P - 1, P), (3, min(P, 3 + 130))):
        part = _entry((hyp[a:b].contiguous(), hl[a:b].contiguous(), ref, rl, of[a:b].contiguous()) if of is not None else
                      (hyp[a:b].contiguous(), hl[a:b].contiguous(), ref[a:b].contiguous(), rl[a:b].contiguous(), None))
        assert _same(part, [None if t is None else t[a:b] for t in whole]), (name, a, b)


def test_the_961_binary_pairs_run_in_one_launch_through_edit_counts():
    """The Python entry on device tensors: one chunk, the restatement's counts and ops (zeros past ``n_ops``); split over pairs by a
    small ``max_workspace_bytes`` the same bits."""
    batch = X.cases()["binary-961"]
    dev_batch = [None if t is None else t.cuda() for t in batch]
    got = scoring.edit_counts(*dev_batch, want_ops=True)
    assert got.distance.is_cuda and got.ops.is_cuda
    host = scoring.EditCounts(*(t.cpu() for t in got))
    X.check_against_expected("binary-961", host, sentinel=0)
    per_pair = capi.load().eec_edit_distance_workspace_bytes(1, 6, 6, 1)
    split = scoring.edit_counts(*dev_batch, want_ops=True, max_workspace_bytes=100 * per_pair)  # 10 chunks
    assert _same([t.cpu() for t in split], host)
    assert _same([t.cpu() for t in scoring.edit_counts(*dev_batch)[:5]], host[:5])
    assert _same(scoring.edit_counts(*batch, want_ops=True), host)  # the host path


def test_edit_counts_without_ref_of_is_split_with_its_references():
    hyp, hl, ref, rl = (t.cuda() for t in X.cases()["random-A5-strip4"][:4])
    whole = scoring.edit_counts(hyp, hl, ref, rl, want_ops=True)
    per_pair = capi.load().eec_edit_distance_workspace_bytes(1, ref.size(1), hyp.size(1), 1)
    split = scoring.edit_counts(hyp, hl, ref, rl, want_ops=True, max_workspace_bytes=5 * per_pair)
    assert _same(split, whole)
    X.check_against_expected("random-A5-strip4", scoring.EditCounts(*(t.cpu() for t in whole)), sentinel=0)


# ---------------------------------------------------------------------------------------------------------------------------
# end to end on the small model
# ---------------------------------------------------------------------------------------------------------------------------
def test_exit_tradeoff_equals_scoring_what_the_adaptive_decoder_returns():
    """The small model of ``conftest.base_kwargs``, B = 4, peaky heads (tests/test_gpu_exit.py's fixture).  First the table: every exit
    of ``forward`` decoded by ``ctc_cuda_predict`` and scored against synthetic references; then ``exit_tradeoff`` at two thresholds of the
    entropy.  At each threshold the error rate and the mean exit equal those of scoring what ``ctc_adaptive_predict`` returns."""
    gpu = Early_conformer(**base_kwargs(device="cuda")).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=42, style="init", head_scale=8.0), strict=True)
    gpu = gpu.cuda()
    B = 4
    mel, lens = synth.synth_mel(B, 80, 203, seed=42).cuda(), torch.tensor([203, 202, 150, 77])
    tgt, tl = synth.synth_targets(B, 12, 256, seed=42)
    refs = [tgt[b, : int(tl[b])].tolist() for b in range(B)]
    inf = BeamInference()
    with torch.no_grad():
        out = gpu(mel, lens)
    E = out.size(0)
    fl = encoder_lengths(lens.cuda(), out.size(2))
    decoded = [inf.ctc_cuda_predict(out[e], beam_size=5, lengths=fl) for e in range(E)]
    table = inf.error_table(decoded, refs, device="cuda")
    assert table.errors.shape == (E, B, 1) and (table.errors >= 0).all() and table.ref_len.tolist() == tl.tolist()
    host = inf.error_table(decoded, refs)
    assert all(torch.equal(a, b) for a, b in zip(table, host))
    errors = table.errors[..., 0]
    entropy = ctc.exit_statistics(out, fl).entropy
    srt = entropy.flatten().sort().values
    thresholds = [float(srt[srt.numel() // 3]) * (1 + 1e-3) + 1e-6, float(srt[2 * srt.numel() // 3]) * (1 + 1e-3) + 1e-6]
    curve = scoring.exit_tradeoff(errors, table.ref_len, entropy, thresholds)
    assert curve.exit_of.shape == (2, B) and curve.histogram.sum(dim=1).tolist() == [B, B]
    for k, thr in enumerate(thresholds):
        hyps, exit_of = inf.ctc_adaptive_predict(gpu, mel, lens, threshold=thr, beam_size=5)
        assert torch.equal(exit_of.cpu(), curve.exit_of[k])
        chosen = inf.error_table((hyps, exit_of), refs, device="cuda")
        assert chosen.errors.shape == (1, B, 1)
        assert chosen.rate().item() == curve.rate[k].item()
        assert exit_of.double().mean().item() == curve.mean_exit[k].item()


def test_beam_inference_error_table_on_decode_batch_output_equals_the_host_path():
    """The small full_conformer of tests/test_gpu_aed_batch.py: ``decode_batch``'s ``out[b][e]`` scored on the device and on the host."""
    from test_gpu_aed_batch import ARGS, _fixture_model, _ragged_batch
    fc, kw = _fixture_model()
    B = 4
    spec, vlen = _ragged_batch(B, 131, seed=3)
    inf = BeamInference()
    out = inf.decode_batch(fc, spec, vlen, beam_size=5, **ARGS)
    tgt, tl = synth.synth_targets(B, 10, 256, seed=9)
    on_device = inf.error_table(out, (tgt, tl), device="cuda")
    on_host = inf.error_table(out, (tgt, tl))
    assert on_device.errors.shape == (kw["n_enc_exits"], B) and on_device.ref_len.tolist() == tl.tolist()
    assert all(torch.equal(a, b) for a, b in zip(on_device, on_host))
    assert torch.equal(on_device.errors, on_device.subs + on_device.dels + on_device.ins) and on_device.errors.sum() > 0
    want = torch.tensor([[X.restate(tgt[b, : int(tl[b])].tolist(), list(out[b][e]))[0] for b in range(B)] for e in range(kw["n_enc_exits"])])
    assert torch.equal(on_device.errors.long(), want)
