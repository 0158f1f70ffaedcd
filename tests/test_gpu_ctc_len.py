"""GPU tests of per-utterance input lengths in the CTC family: the loss and its gradient (csrc/ctc.hip compiled with lengths by
csrc/ctc_len.hip: eec_ctc_loss_len, eec_ctc_loss_forward_len / _backward_len), the greedy decoder (csrc/pack.hip:
eec_greedy_ctc_len) and the prefix beam search (csrc/ctc_beam.hip: eec_ctc_beam_decode_len, eec_ctc_beam_decode_nbest), whose
kernels serve the calls without lengths too.

Judge of the loss and gradient: torch's CPU nn.CTCLoss(blank, 'mean', zero_infinity=True) in fp64 with the real input_lengths,
per exit (ctc_len_cases.ref_ctc); of the decoders: the oracle's greedy decode and oracle/ctc_beam_ref.py on ``logp[s, :len_s]``.
Inputs: tests/ctc_len_cases.py, whose own checks tests/test_host_ctc_len.py runs without a GPU.

Bounds -- the project's own, from tests/test_gpu_ctc.py; none is taken from the kernels under test:
    loss      |err| <= max(2e-5 + 2e-5 |want|, 2 err32)
    gradient  |err| <= max(1e-5 max|grad| + 1e-9, 2 gerr32);  every frame's gradient row sums to zero over the classes within
              1e-5 max(max|grad|, 1e-6) V
    beam      score within 2e-3 max(1, |score|); tokens identical where the oracle's best leads by more than 5e-3, on >= 0.75
err32 / gerr32: the fp32 evaluation of the same torch loop against fp64 on the same input.
"""
import math

import pytest
import torch

import ctc_cases as C
import ctc_len_cases as L
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import (Early_conformer, ctc_beam_decode, exit_ctc_losses, exit_distill_losses, exit_training_losses,
                                              greedy_ctc)

pytestmark = pytest.mark.gpu


def hip_losses(logp, tgt, tl, il, blank=0):
    """The no-grad entry (eec_ctc_loss_len)."""
    with torch.no_grad():
        return exit_ctc_losses(logp.cuda(), tgt, tl, blank=blank, input_len=il).cpu()


def hip_loss_and_grad(logp, tgt, tl, il, blank=0, w=None):
    """The autograd pair (eec_ctc_loss_forward_len / _backward_len)."""
    x = logp.detach().clone().cuda().requires_grad_(True)
    losses = exit_ctc_losses(x, tgt, tl, blank=blank, input_len=il)
    ww = torch.ones_like(losses) if w is None else w.cuda()
    (losses * ww).sum().backward()
    return losses.detach().cpu(), x.grad.cpu()


def check_against_fp64(tag, logp, tgt, tl, il, blank=0, w=None):
    """Both entries against the fp64 judge with the module's bounds; the gradient rows at and past each length must be exactly 0."""
    logp = logp.float()
    T, V = logp.shape[2:]
    want, gw = L.ref_ctc(logp, tgt, tl, il, blank, torch.float64, w)
    want32, g32 = L.ref_ctc(logp, tgt, tl, il, blank, torch.float32, w)
    lerr32 = (want32.double() - want).abs()
    bound = torch.maximum(2e-5 + 2e-5 * want.abs(), 2 * lerr32)
    got0 = hip_losses(logp, tgt, tl, il, blank).double()
    got1, g = hip_loss_and_grad(logp, tgt, tl, il, blank, w)
    got1, g = got1.double(), g.double()
    lerr0, lerr1 = (got0 - want).abs(), (got1 - want).abs()
    scale = gw.abs().max().item()
    gerr, gerr32 = (g - gw).abs().max().item(), (g32.double() - gw).abs().max().item()
    print(f"\n[ctc len {tag}] loss {want.max().item():.4f}: HIP err {lerr0.max().item():.2e} (no-grad) {lerr1.max().item():.2e} (autograd), "
          f"torch-fp32 err {lerr32.max().item():.2e}; max|grad| {scale:.3e}: HIP err {gerr:.2e}, torch-fp32 err {gerr32:.2e}")
    assert torch.isfinite(got0).all() and (lerr0 <= bound).all(), (tag, got0.tolist(), want.tolist(), lerr32.tolist())
    assert torch.isfinite(got1).all() and (lerr1 <= bound).all(), (tag, got1.tolist(), want.tolist(), lerr32.tolist())
    assert torch.isfinite(g).all(), tag
    assert gerr <= max(1e-5 * scale + 1e-9, 2 * gerr32), (tag, gerr, gerr32, scale)
    assert g.sum(-1).abs().max().item() < 1e-5 * max(scale, 1e-6) * V, tag
    pad = ~L.valid_mask(il, T)
    assert (g[:, pad] == 0).all(), tag
    return got0, got1, g


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the loss and its gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("scale", sorted(C.PEAKY_SCALES))
def test_ragged_ctc_loss_and_gradient_on_peaky_logprobs(scale, P):
    """log_softmax(randn * scale), E = 2, B = 6, T' = 64, input lengths 64, 33, 1, 0, 17, 2; the targets are exit 0's greedy decode
    of the valid frames (exit 1: mismatched), padded to the width that selects 2 / 4 / 8 states per lane.
    Measured on MI355X, error against fp64 (HIP | torch's own fp32 evaluation) at P = 4 and 8 (P = 2, its widest target cut to 63
    labels: loss 5.2e-7, 1.4e-6, 1.0e-6 at randn*5, 9, 16):
        loss      randn*2 1.4e-8 | 1.4e-8   randn*5 7.8e-7 | 7.8e-7   randn*9 1.5e-6 | 1.5e-6   randn*16 1.9e-6 | 1.9e-6
        gradient  randn*2 4.4e-9 | 4.0e-7   randn*5 5.5e-9 | 7.2e-7   randn*9 7.8e-9 | 1.0e-6   randn*16 5.7e-9 | 2.1e-6   (max|grad| 0.25)
    The bounds of the module hold on every case; 2 * err32 is not needed."""
    lp, tgt, tl, il = L.ragged_case(scale, P)
    check_against_fp64(f"scale{scale:g} P{P}", lp, tgt, tl, il, w=torch.linspace(0.5, 1.5, lp.size(0)))


@pytest.mark.parametrize("P", [2, 8])
def test_input_lengths_around_the_lookahead_rings_and_the_meeting_point(P):
    """T' = 40, one utterance per input length 0, 1, 2, 3 (the short-lattice cases of the loss kernel), 4, 8, 9, 16, 17, 33 (exact
    groups and ragged tails of the 4- / 8- / 16-deep rings), 39, 40, with min(3, len) labels, and one empty target."""
    lp, tgt, tl, il = L.ring_case(P)
    check_against_fp64(f"ring P{P}", lp, tgt, tl, il)
    # every utterance on its own gives its own term of the batch mean: no cross-talk between lattices of different lengths
    B = lp.size(1)
    whole = hip_losses(lp, tgt, tl, il).double()
    alone = torch.stack([hip_losses(lp[:, b:b + 1], tgt[b:b + 1], tl[b:b + 1], il[b:b + 1]).double() for b in range(B)], 1)
    assert torch.allclose(alone.sum(1) / B, whole, rtol=1e-5, atol=1e-6)  # fp32 sums of 13 terms in another order
    assert (alone[:, il == 0] == 0).all()  # no frame: 0 for the empty target


@pytest.mark.parametrize("P", [2, 4, 8])
def test_feasibility_edge_follows_the_input_length(P):
    """A target that needs 10 frames in T' = 16: input_len 10 leaves the single alignment (its log-prob is the loss), input_len 9
    is infeasible: loss 0 and an all-zero gradient."""
    lp, tgt, tl = L.feasibility_case(P)
    il = torch.tensor([10])
    check_against_fp64(f"single alignment P{P}", lp, tgt, tl, il)
    want = torch.stack([-sum(lp[e, 0, t, c].double() for t, c in enumerate(L.FEASIBLE_PATH)) / len(L.FEASIBLE_TARGET) for e in range(2)])
    assert ((hip_losses(lp, tgt, tl, il).double() - want).abs() < 2e-5 * (1 + want)).all()
    il = torch.tensor([9])
    assert L.ref_ctc(lp, tgt, tl, il)[0].abs().max().item() == 0.0
    assert hip_losses(lp, tgt, tl, il).abs().max().item() == 0.0
    loss, g = hip_loss_and_grad(lp, tgt, tl, il)
    assert loss.abs().max().item() == 0.0 and (g == 0).all()


def test_no_frames_with_a_non_empty_target_is_zeroed():
    lp = C.peaky_logp(2.0, E=2, B=2, T=8)
    tgt, tl, il = torch.tensor([[3, 4], [3, 4]]), torch.tensor([0, 2]), torch.tensor([0, 0])
    assert hip_losses(lp, tgt, tl, il).tolist() == [0.0, 0.0]
    loss, g = hip_loss_and_grad(lp, tgt, tl, il)
    assert loss.tolist() == [0.0, 0.0] and (g == 0).all()


@pytest.mark.parametrize("scale,P", [(5.0, 2), (16.0, 4), (9.0, 8)])
def test_ctc_results_do_not_depend_on_the_padding(scale, P):
    """Frames t >= len overwritten by NaN and by other log-prob rows: the losses and the gradient on t < len are bit-identical to
    the clean input's, the gradient on t >= len is exactly 0."""
    lp, tgt, tl, il = L.ragged_case(scale, P)
    pad = ~L.valid_mask(il, lp.size(2))
    clean0 = hip_losses(lp, tgt, tl, il)
    clean1, g = hip_loss_and_grad(lp, tgt, tl, il)
    assert torch.isfinite(clean0).all() and torch.isfinite(g).all()
    for kind in ("nan", "random"):
        dirty = L.overwrite_pad(lp, il, kind)
        assert torch.equal(hip_losses(dirty, tgt, tl, il), clean0), kind
        got1, gd = hip_loss_and_grad(dirty, tgt, tl, il)
        assert torch.equal(got1, clean1), kind
        assert torch.equal(gd[:, ~pad].view(torch.int32), g[:, ~pad].view(torch.int32)), kind
        assert (gd[:, pad] == 0).all(), kind


@pytest.mark.parametrize("P", [2, 8])
def test_wide_path_lattices_with_padding_behind_them(P):
    """The hand-built lattices of ctc_cases.range_cases() (T' = 40; blank and labels at -20 .. -95 on chosen frames), which the
    training forward marks for the wide format, as the first 40 of 49 frames: the fp64 bounds against the judge, and bit-identical
    results whether the 9 frames behind hold log-probs or NaN."""
    # (without the masked vocabulary, on whose exact -inf inputs the judge's own gradient is NaN)
    sel = [c for c in C.range_cases() if c[2] == (3, 4) and c[0] != "masked-vocabulary"]
    lp = torch.stack([c[1] for c in sel]).unsqueeze(1).float()  # [E, 1, 40, 8]
    g = torch.Generator().manual_seed(49)
    tail = torch.log_softmax(torch.randn(lp.size(0), 1, 9, lp.size(3), generator=g), -1)
    x = torch.cat([lp, tail], 2).contiguous()
    tgt, tl, il = C.pad_targets(torch.tensor([[3, 4]]), C.WIDTH_FOR_P[P]), torch.tensor([2]), torch.tensor([40])
    got0, got1, gr = check_against_fp64(f"range lattices + 9 pad frames P{P}", x, tgt, tl, il)
    want, _ = C.ref_ctc(lp, tgt, tl)
    assert ((got0 - want).abs() <= torch.maximum(2e-5 + 2e-5 * want.abs(), 2 * (C.ref_ctc(lp, tgt, tl, dtype=torch.float32)[0].double() - want).abs())).all()
    dirty = L.overwrite_pad(x, il, "nan")
    assert torch.equal(hip_losses(dirty, tgt, tl, il).double(), got0)
    loss, gd = hip_loss_and_grad(dirty, tgt, tl, il)
    assert torch.equal(loss.double(), got1) and torch.equal(gd.double(), gr)


def test_gradient_buffer_is_written_in_full():
    """The backward writes its zeros: the same backward twice through a caching allocator, whose second buffer holds the first
    call's (non-zero, differently placed) values, gives zeros on the padding both times."""
    lp, tgt, tl, il = L.ragged_case(5.0, 2)
    _, g_full = hip_loss_and_grad(lp, tgt, tl, torch.full((6,), 64))
    assert g_full.abs().min(-1).values.max() > 0
    _, g = hip_loss_and_grad(lp, tgt, tl, il)
    assert (g[:, ~L.valid_mask(il, 64)] == 0).all()


def test_without_lengths_nothing_changes():
    """input_len=None is the existing call bit for bit; lengths all T' (and beyond: clamped) stay within the fp64 bounds and are
    bit-identical to None -- the loss, the training forward's loss and the gradient: the same arithmetic over the same Tb."""
    lp, tgt, tl, _ = L.ragged_case(5.0, 4)
    with torch.no_grad():
        base0 = exit_ctc_losses(lp.cuda(), tgt, tl).cpu()
    x = lp.cuda().requires_grad_(True)
    base1 = exit_ctc_losses(x, tgt, tl)
    base1.sum().backward()
    none0 = hip_losses(lp, tgt, tl, None)
    none1, gn = hip_loss_and_grad(lp, tgt, tl, None)
    assert torch.equal(none0.view(torch.int32), base0.view(torch.int32)) and torch.equal(none1.view(torch.int32), base1.detach().cpu().view(torch.int32))
    assert torch.equal(gn.view(torch.int32), x.grad.cpu().view(torch.int32))
    for il in (torch.full((6,), 64), torch.tensor([64, 65, 1000, 64, 2 ** 31 - 1, 64]), torch.full((6,), 64, dtype=torch.int32).cuda()):
        got0, got1, g = check_against_fp64("all T'", lp, tgt, tl, il)
        same = (torch.equal(got0.float(), base0), torch.equal(got1.float(), none1), torch.equal(g.float(), gn))
        print(f"[ctc len all T'] bit-identical to None: loss {same[0]} / {same[1]}, gradient {same[2]}")
        assert torch.equal(got0.float().view(torch.int32), base0.view(torch.int32)), il
        assert torch.equal(got1.float().view(torch.int32), none1.view(torch.int32)), il
        assert torch.equal(g.float().view(torch.int32), gn.view(torch.int32)), il
    # negative lengths clamp to 0
    assert hip_losses(lp, tgt, torch.zeros(6, dtype=torch.long), torch.tensor([-1, -5, 0, -2 ** 31, -1, 0])).tolist() == [0.0, 0.0]


def test_blank_other_than_zero_with_lengths():
    g = torch.Generator().manual_seed(17)
    lp = torch.log_softmax(torch.randn(2, 3, 25, 32, generator=g) * 2, -1)
    tgt = torch.randint(0, 31, (3, 6), generator=g)  # label 0 is an ordinary class, 31 the blank
    check_against_fp64("blank 31", lp, tgt, torch.tensor([6, 3, 0]), torch.tensor([25, 11, 4]), blank=31)


def test_combined_node_with_both_masks():
    """exit_training_losses(frame_len=fl, input_len=fl): the losses are the two functions' bit for bit, the one-buffer gradient is
    within 1e-6 max|grad| (the distillation test's tolerance) of the sum of the two separate gradients, and exactly 0 on the
    padding, where the CTC backward wrote zeros and the accumulating distillation backward wrote nothing."""
    lp, tgt, tl, il = L.ragged_case(2.0, 2)
    x = L.overwrite_pad(lp, il, "random")
    fl = il.to(torch.int32)

    def grad_of(loss_fn):
        xg = x.cuda().requires_grad_(True)
        loss_fn(xg).backward()
        return xg.grad

    with torch.no_grad():
        ctc, kd = exit_training_losses(x.cuda(), tgt, tl, fl, "last", 2.0, input_len=il)
        assert torch.equal(ctc, exit_ctc_losses(x.cuda(), tgt, tl, input_len=il)) and torch.equal(kd, exit_distill_losses(x.cuda(), fl, "last", 2.0))
    g_ctc = grad_of(lambda xg: exit_ctc_losses(xg, tgt, tl, input_len=il).sum())
    g_kd = grad_of(lambda xg: 0.5 * exit_distill_losses(xg, fl, "last", 2.0).sum())
    both = grad_of(lambda xg: (lambda c, k: c.sum() + 0.5 * k.sum())(*exit_training_losses(xg, tgt, tl, fl, "last", 2.0, input_len=il)))
    sep = g_ctc + g_kd
    err, scale = (both - sep).abs().max().item(), sep.abs().max().item()
    print(f"\n[ctc len training] one node vs the sum of the two gradients: {err:.2e} of max|grad| {scale:.3e}")
    assert err <= 1e-6 * scale
    pad = ~L.valid_mask(il, 64)
    assert (both.cpu()[:, pad] == 0).all() and g_kd.abs().max() > 0
    only_ctc = grad_of(lambda xg: exit_training_losses(xg, tgt, tl, fl, "last", 2.0, input_len=il)[0].sum())
    assert torch.equal(only_ctc.view(torch.int32), g_ctc.view(torch.int32))
    # frame_len alone keeps its meaning: the CTC term is unmasked
    with torch.no_grad():
        ctc_unmasked, _ = exit_training_losses(lp.cuda(), tgt, tl, fl, "last", 2.0)
        assert torch.equal(ctc_unmasked, exit_ctc_losses(lp.cuda(), tgt, tl))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the decoders
# ---------------------------------------------------------------------------------------------------------------------------
def run_greedy(logp, lens, blank=0):
    tok, cnt = (t.cpu() for t in greedy_ctc(logp.cuda(), blank, em_len=lens))
    return [tok[s, : int(cnt[s])].tolist() for s in range(logp.size(0))]


def run_beam(logp, lens, beam, blank=0, thr=0.95, drop=False):
    tok, cnt, sc = (t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=beam, blank=blank, blank_skip_threshold=thr, skip_drops_frame=drop,
                                                     em_len=lens))
    return [tok[s, : int(cnt[s])].tolist() for s in range(logp.size(0))], sc


def check_beam(tag, logp, lens, beam, blank=0, thr=0.95, min_share=0.75):
    """test_gpu_ctc.check_beam's rule against the oracle on logp[s, :len_s], under both readings of the skip rule."""
    N = logp.size(0)
    for drop in (False, True):
        got, sc = run_beam(logp, lens, beam, blank, thr, drop)
        checked = 0
        for n in range(N):
            want, wscore, final = L.ref_beam(logp[n], min(max(int(lens[n]), 0), logp.size(1)), beam, blank, thr, drop)
            assert abs(float(sc[n]) - wscore) < 2e-3 * max(1.0, abs(wscore)), (tag, drop, n, float(sc[n]), wscore)
            if C.safe_margin(final):
                assert got[n] == list(want), (tag, drop, n)
                checked += 1
        assert checked >= math.ceil(min_share * N), (tag, drop, checked, N)


@pytest.mark.parametrize("N,T,V,beam,scale", C.BEAM_CASES)
def test_decoders_with_lengths_equal_the_oracle_on_the_slices(N, T, V, beam, scale):
    logp, lens = C.beam_logp(N, T, V, scale), L.decoder_lens(N, T)
    assert run_greedy(logp, lens) == L.ref_greedy(logp, lens)
    check_beam(f"scale {scale}", logp, lens, beam)
    # pad independence: the same tokens, counts and scores (bit for bit) with NaN and with other rows past the lengths
    clean = [run_beam(logp, lens, beam, drop=d) for d in (False, True)]
    for kind in ("nan", "random"):
        dirty = L.overwrite_pad(logp, lens, kind)
        assert run_greedy(dirty, lens) == L.ref_greedy(logp, lens), kind
        for d, (tok, sc) in zip((False, True), clean):
            tok2, sc2 = run_beam(dirty, lens, beam, drop=d)
            assert tok2 == tok and torch.equal(sc2.view(torch.int32), sc.view(torch.int32)), (kind, d)


@pytest.mark.parametrize("N,T,V,beam,scale", sorted(C.BEAM_CASES, key=lambda c: c[0] * c[1] * c[2])[:2])
def test_decoders_with_lengths_all_T_equal_the_calls_without(N, T, V, beam, scale):
    """em_len all T' against em_len=None, at the smallest entry of BEAM_CASES (beam 1) and at the next (beam 16, where the N-best
    end has a beam to rank): greedy, the beam search and its N-best form with nbest = beam give the same counts, scores and n_hyp
    (torch.equal) and the same tokens up to each count.  Both calls run one kernel with the same Ts."""
    logp, full = C.beam_logp(N, T, V, scale).cuda(), torch.full((N,), T)
    (tok0, cnt0), (tok1, cnt1) = greedy_ctc(logp, 0, em_len=None), greedy_ctc(logp, 0, em_len=full)
    live = torch.arange(T, device="cuda") < cnt0.unsqueeze(-1)
    assert torch.equal(cnt0, cnt1) and torch.equal(tok0[live], tok1[live])
    for nbest in (None, beam):
        a, b = (ctc_beam_decode(logp, beam_size=beam, em_len=el, nbest=nbest) for el in (None, full))
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), nbest
        live = torch.arange(T, device="cuda") < a[1].unsqueeze(-1)
        assert torch.equal(a[0][live], b[0][live]), nbest
        assert nbest is None or (torch.equal(a[3], b[3]) and int(a[3].min()) >= 1), nbest


def test_decoder_length_edges():
    logp = C.beam_logp(8, 40, 32, 4.0, blank=31)
    # no frame: count 0, score 0; lengths outside [0, T'] are clamped; int32 lengths on the device
    lens = torch.tensor([0, -3, 40, 41, 10 ** 6, 0, 7, 1])
    want = L.ref_greedy(logp, lens.clamp(0, 40), blank=31)
    assert run_greedy(logp, lens, blank=31) == want and want[0] == want[1] == want[5] == []
    assert run_greedy(logp, lens.to(torch.int32).cuda(), blank=31) == want
    tok, sc = run_beam(logp, lens, 10, blank=31)
    assert tok[0] == tok[1] == tok[5] == [] and sc[[0, 1, 5]].tolist() == [0.0, 0.0, 0.0]
    check_beam("blank V-1", logp, lens, 10, blank=31)
    # without lengths: the existing calls bit for bit
    a, b = greedy_ctc(logp.cuda(), 31), greedy_ctc(logp.cuda(), 31, em_len=None)
    assert torch.equal(a[1], b[1]) and run_greedy(logp, None, blank=31) == L.ref_greedy(logp, [40] * 8, blank=31)
    full = run_beam(logp, torch.full((8,), 40), 10, blank=31)
    none = run_beam(logp, None, 10, blank=31)
    assert full[0] == none[0] and torch.equal(full[1], none[1])


def test_decoders_full_batch_with_lengths():
    """One launch of 6 x 64 sequences at the benchmark geometry with lengths spread over [0, T']: EVERY sequence is bit-identical
    (tokens, count, score) in launches of subsets, greedy equals the oracle on all, the beam search on 16 sampled sequences."""
    logp = C.big_batch_logp()
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(0, 257, (384,), generator=g)
    lens[:4] = torch.tensor([0, 1, 256, 255])
    dev = logp.cuda()
    assert run_greedy(logp, lens) == L.ref_greedy(logp, lens)
    tok, sc = run_beam(logp, lens, 10)
    for sub in (torch.arange(0, 384, 3), torch.arange(2, 384, 3).flip(0)):
        t3, s3 = run_beam(dev[sub].contiguous(), lens[sub], 10)
        assert t3 == [tok[i] for i in sub.tolist()] and torch.equal(s3, sc[sub])
    checked = 0
    for n in C.BIG_SAMPLE:
        want, wscore, final = L.ref_beam(logp[n], lens[n], 10)
        assert abs(float(sc[n]) - wscore) < 2e-3 * max(1.0, abs(wscore)), (n, float(sc[n]), wscore)
        if C.safe_margin(final):
            assert tok[n] == list(want), n
            checked += 1
    assert checked >= 12, checked


def test_model_and_beam_inference_take_lengths():
    """Early_conformer.greedy_decode(lengths=) applies [B] lengths to every exit; BeamInference.ctc_cuda_predict(lengths=) is
    ctc_beam_decode with em_len."""
    E, B, T, V = 2, 4, 40, 32
    logp = C.beam_logp(E * B, T, V, 4.0).view(E, B, T, V)
    lens = torch.tensor([40, 0, 13, 1])
    got = Early_conformer.greedy_decode(None, logp.cuda(), 0, lengths=lens)
    assert got == [L.ref_greedy(logp[e], lens) for e in range(E)]
    assert Early_conformer.greedy_decode(None, logp.cuda(), 0) == [L.ref_greedy(logp[e], [T] * B) for e in range(E)]
    hyps = BeamInference().ctc_cuda_predict(logp[1].cuda(), beam_size=10, lengths=lens)
    tok, sc = run_beam(logp[1], lens, 10)
    assert [h[0].tokens for h in hyps] == tok and [h[0].score for h in hyps] == sc.tolist()
    assert hyps[1][0].tokens == [] and hyps[1][0].score == 0.0
