"""GPU tests of adaptive inference (run with -m gpu on an MI355X): the exit statistics and routing kernels (csrc/exit_stats.hip)
against the fp64 restatement of tests/exit_cases.py, ``forward_adaptive`` against ``forward`` -- bit for bit: the walk runs the
launches of the full forward on fewer utterances --, and the two decoders on top of it against decoding the chosen rows of the full
forward."""
import pytest
import torch

import exit_cases as X
from conftest import base_kwargs
from early_exit_transformer_amd import ctc, synth
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import Early_conformer, Splitformer, ctc_beam_decode, encoder_lengths

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev_stats(x, fl):
    return torch.stack(list(ctc.exit_statistics(x.cuda(), None if fl is None else fl.cuda()))).cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.cases()))
def test_statistics_kernel_against_fp64(name):
    """|err| <= max(2e-5 + 2e-5 |want|, 2 err32) on every shared case, err32 the fp32 host path's own error; two runs are
    bit-equal; the E = 1 call on every exit's slice, and the call on every utterance's slice, return the bits of the batched
    call.  Measured on an MI355X: the worst case (the trained-like fixture) uses 0.017 of the bound, the others 0.004 to 0.011."""
    x, fl = X.cases()[name]
    want, err32 = X.reference(name)
    got = _dev_stats(x, fl)
    frac = ((got.double() - want).abs() / X.stats_bound(want, err32)).max().item()
    print(f"\n[exit stats {name}] worst error: {frac:.3f} of the bound")
    assert torch.isfinite(got).all() and frac <= 1.0
    assert torch.equal(_dev_stats(x, fl), got)
    for e in range(x.size(0)):
        assert torch.equal(_dev_stats(x[e:e + 1], fl), got[:, e:e + 1]), e
    for b in range(x.size(1)):
        assert torch.equal(_dev_stats(x[:, b:b + 1], None if fl is None else fl[b:b + 1]), got[:, :, b:b + 1]), b


def test_statistics_kernel_nan_placement():
    """A NaN at or past a length is never read; a NaN inside reaches the three statistics of its own (e, b) and nothing else."""
    bad, fl, clean = X.nan_past_length()
    assert torch.equal(_dev_stats(bad, fl), _dev_stats(clean, fl))
    bad, fl, (e, b) = X.nan_inside_length()
    got = _dev_stats(bad, fl)
    ok = X.ref_stats(bad, fl)
    for k in range(3):
        hit = torch.isnan(got[k])
        assert hit[e, b] and hit.sum() == 1
    keep = ~torch.isnan(ok)
    assert ((got.double() - ok)[keep].abs() <= (2e-5 + 2e-5 * ok[keep].abs())).all()


@pytest.mark.parametrize("n", [1, 5, 64, 1000])
def test_route_kernel_equals_the_restatement(n):
    g = torch.Generator().manual_seed(n)
    score = torch.rand(n, generator=g)
    score[torch.rand(n, generator=g) < 0.15] = NAN
    score[n // 2] = 0.5  # a tie at the threshold stays
    settings = [(0.5, False, False), (0.5, True, False), (-1.0, False, False), (2.0, False, False), (2.0, True, False),
                (-1.0, True, False), (0.5, False, True), (NAN, True, True)]
    for thr, hib, force in settings:
        stay, leave, counts = ctc.exit_route(score.cuda(), thr, hib, force)
        want_stay, want_leave = X.ref_route(score, thr, hib, force)
        assert counts.tolist() == [len(want_stay), len(want_leave)], (thr, hib, force)
        assert stay.dtype == leave.dtype == counts.dtype == torch.int32
        assert stay[: len(want_stay)].tolist() == want_stay and leave[: len(want_leave)].tolist() == want_leave, (thr, hib, force)
        assert (stay[len(want_stay):] == n).all() and (leave[len(want_leave):] == n).all()  # the tail is left alone
    clean = torch.rand(n, generator=g)
    assert ctc.exit_route(clean.cuda(), 2.0)[2].tolist() == [0, n] and ctc.exit_route(clean.cuda(), -1.0)[2].tolist() == [n, 0]


def test_select_exits_on_the_device_equals_the_host_path():
    g = torch.Generator().manual_seed(8)
    table = torch.rand(6, 70, generator=g)
    table[torch.rand(6, 70, generator=g) < 0.1] = NAN
    for hib, lo, hi, thr in ((False, 0, None, 0.3), (True, 1, 4, 0.6), (False, 2, 2, 0.5), (True, 0, None, [0.9, 0.8, 0.7, 0.6, 0.5, 0.4])):
        got = ctc.select_exits(table.cuda(), thr, hib, lo, hi)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), X.ref_select(table, thr, hib, lo, hi))
    assert ctc.select_exits(table[:, :1].cuda(), 0.3).tolist() == X.ref_select(table[:, :1], 0.3).tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# forward_adaptive
# ---------------------------------------------------------------------------------------------------------------------------
KW = dict(n_enc_exits=4, n_enc_layers=1, d_feed_forward=128)
LENS = [403, 402, 300, 77, 5]  # T' = 99: ragged last row tile


def _model(seed, **synth_kw):
    gpu = Early_conformer(**base_kwargs(**KW, device="cuda")).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=seed, **synth_kw), strict=True)
    return gpu.cuda()


def _full(gpu, mel, lens):
    """(log-probs [E, B, T', V], taps [E, B, T', D], frame counts [B]) of the full forward."""
    with torch.no_grad():
        out, taps, _ = gpu._run_encoder(mel, lens, want_taps=True)
        assert torch.equal(out, gpu(mel, lens))
    return out, taps, encoder_lengths(lens.cuda(), out.size(2))


@pytest.fixture(scope="module")
def prescribed():
    gpu = _model(61, style="trained")
    mel, lens = synth.synth_mel(5, 80, 403, seed=61).cuda(), torch.tensor(LENS)
    return gpu, mel, lens, _full(gpu, mel, lens)


def _check_rows(ad, exit_of, out, taps, score_table):
    """Every utterance's rows are the full forward's rows of its exit, bit for bit; scores where reached, NaN elsewhere."""
    assert ad.exit_of.dtype == torch.int32 and ad.exit_of.tolist() == list(exit_of)
    E = out.size(0)
    for b, e in enumerate(exit_of):
        if ad.taps is not None:
            assert torch.equal(ad.taps[b], taps[e, b]), ("taps", b, e)
        assert torch.equal(ad.logp[b], out[e, b]), ("logp", b, e)
        assert torch.equal(ad.scores[: e + 1, b], score_table[: e + 1, b]), ("scores", b, e)
        assert torch.isnan(ad.scores[e + 1:, b]).all() and ad.scores.shape == (E, len(exit_of))


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("routing", [[0, 0, 0, 0, 0], [3, 3, 3, 3, 3], [0, 3, 1, 3, 0], [3, 0, 0, 0, 0], [2]],
                         ids=["all-0", "all-3", "mixed", "longest-stays", "B1"])
def test_forward_adaptive_with_a_prescribed_routing(prescribed, routing, compact):
    """``taps[b]`` and ``logp[b]`` are ``torch.equal`` to the full forward's rows of exit ``exit_of[b]``: the walk's group launches are
    the full forward's layer plan on independent utterances, and the single-exit head launch rounds like the batched one -- both run
    ``head_body`` (csrc/linear.hip) with the same operand format on row tiles whose rows do not interact.  "mixed": the longest
    utterance leaves first, so every key length that goes on is below T'."""
    gpu, mel, lens, (out, taps, fl) = prescribed
    B = len(routing)
    if B != mel.size(0):
        mel, lens = mel[:B], lens[:B]
        out, taps, fl = _full(gpu, mel, lens)
    table = ctc.exit_statistics(out, fl).entropy
    ad = gpu.forward_adaptive(mel, lens, exit_of=torch.tensor(routing), compact=compact, want_taps=True)
    assert ad.logp.shape == out.shape[1:] and ad.taps.shape == taps.shape[1:]
    _check_rows(ad, routing, out, taps, table)
    ad = gpu.forward_adaptive(mel, lens, exit_of=routing, criterion="greedy_logp", compact=compact)
    assert ad.taps is None
    _check_rows(ad, routing, out, taps, X.routing_scores(torch.stack(list(ctc.exit_statistics(out, fl))), fl, "greedy_logp"))


@pytest.fixture(scope="module")
def peaky():
    """Heads with the peaky scaling of the greedy fixture (config1_peaky: style "init", head_scale 8)."""
    gpu = _model(42, style="init", head_scale=8.0)
    mel, lens = synth.synth_mel(5, 80, 403, seed=42).cuda(), torch.tensor(LENS)
    out, taps, fl = _full(gpu, mel, lens)
    return gpu, mel, lens, (out, taps, fl), torch.stack(list(ctc.exit_statistics(out, fl)))


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("criterion", list(X.CRITERIA))
def test_forward_adaptive_with_thresholds(peaky, criterion, compact):
    """Each exit's threshold is the midpoint of the widest gap between its sorted scores; the gap is at least 100 x the statistics
    bound (a condition on the inputs, met by seed 42 on the CPU oracle).  The chosen exits are ``select_exits`` of the full forward's
    statistics, the rows the full forward's."""
    gpu, mel, lens, (out, taps, fl), stats = peaky
    table = X.routing_scores(stats, fl, criterion)
    thr, gap = X.widest_gap_thresholds(table.cpu())
    need = 100 * X.score_bound(out.cpu(), fl.cpu().long(), criterion).max(dim=1).values
    print(f"\n[adaptive {criterion}] gap / (100 x bound) per exit: {(gap / need).tolist()}")
    assert (gap >= need).all()
    higher = X.CRITERIA[criterion][1]
    want = ctc.select_exits(table, thr.tolist(), higher)
    assert torch.equal(want.cpu(), X.ref_select(table.cpu(), thr.tolist(), higher))
    ad = gpu.forward_adaptive(mel, lens, thr.tolist(), criterion=criterion, compact=compact, want_taps=True)
    _check_rows(ad, want.tolist(), out, taps, table)
    for lo, hi in ((0, 1), (2, None), (1, 2), (3, 3)):
        want = ctc.select_exits(table, thr.tolist(), higher, lo, hi)
        ad = gpu.forward_adaptive(mel, lens, thr.tolist(), criterion=criterion, min_exit=lo, max_exit=hi, compact=compact)
        _check_rows(ad, want.tolist(), out, taps, table)
    one = float(thr[0])  # one threshold for every exit
    _check_rows(gpu.forward_adaptive(mel, lens, one, criterion=criterion, compact=compact), ctc.select_exits(table, one, higher).tolist(),
                out, taps, table)


def test_forward_adaptive_refuses_what_it_does_not_serve(peaky):
    gpu, mel, lens = peaky[:3]
    with pytest.raises(ValueError, match="exactly one"):
        gpu.forward_adaptive(mel, lens)
    with pytest.raises(ValueError, match="exactly one"):
        gpu.forward_adaptive(mel, lens, 0.5, exit_of=[0] * 5)
    with pytest.raises(ValueError, match="criterion"):
        gpu.forward_adaptive(mel, lens, 0.5, criterion="margin")
    with pytest.raises(ValueError, match="one exit in 0 .. 3 per utterance"):
        gpu.forward_adaptive(mel, lens, exit_of=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="per utterance"):
        gpu.forward_adaptive(mel, lens, exit_of=[0, 1])
    with pytest.raises(ValueError, match="min_exit"):
        gpu.forward_adaptive(mel, lens, 0.5, max_exit=4)
    with pytest.raises(ValueError, match="one per exit"):
        gpu.forward_adaptive(mel, lens, [0.5, 0.5])
    gpu.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            gpu.forward_adaptive(mel, lens, 0.5)
    finally:
        gpu.eval()
    sf = Splitformer(**base_kwargs(**KW, device="cuda")).eval().cuda()
    with pytest.raises(NotImplementedError):
        sf.forward_adaptive(mel, lens, 0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# decoding the chosen exit
# ---------------------------------------------------------------------------------------------------------------------------
def test_ctc_adaptive_predict_equals_the_beam_search_of_the_chosen_rows(peaky):
    gpu, mel, lens, (out, _, fl), stats = peaky
    inf = BeamInference()
    thr, _ = X.widest_gap_thresholds(stats[0].cpu())
    for kw in (dict(threshold=thr.tolist()), dict(exit_of=[0, 3, 1, 3, 0], compact=False)):
        hyps, exit_of = inf.ctc_adaptive_predict(gpu, mel, lens, beam_size=10, **kw)
        rows = torch.stack([out[e, b] for b, e in enumerate(exit_of.tolist())])
        tok, cnt, score = ctc_beam_decode(rows, beam_size=10, blank=0, blank_skip_threshold=0.95, em_len=fl)
        assert len(hyps) == 5 and len(set(exit_of.tolist())) > 1
        for b, (h,) in enumerate(hyps):
            assert h.tokens == tok[b, : int(cnt[b])].tolist() and h.score == float(score[b])
    assert any(len(h.tokens) for (h,) in hyps)


def test_decode_batch_adaptive_equals_decode_batch_at_the_chosen_exits():
    """The small full_conformer of tests/test_gpu_aed_batch.py: ``out[b] = (decode_batch(...)[b][exit], exit)`` for a prescribed
    routing, plain and with the one-pass joint search."""
    from test_gpu_aed_batch import ARGS, _fixture_model, _ragged_batch
    fc, kw = _fixture_model()
    E = kw["n_enc_exits"]
    spec, vlen = _ragged_batch(4, 131, seed=3)
    routing = [0, E - 1, 2, E - 1]
    inf = BeamInference()
    for extra in ({}, dict(joint_ctc_weight=0.3)):
        want = inf.decode_batch(fc, spec, vlen, beam_size=5, **ARGS, **extra)
        got = inf.decode_batch_adaptive(fc, spec, vlen, exit_of=routing, beam_size=5, **ARGS, **extra)
        assert [e for _, e in got] == routing
        for b, (best, e) in enumerate(got):
            assert best == want[b][e], (extra, b, e)
