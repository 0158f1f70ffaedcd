"""GPU tests of MWER training of the CTC exits (csrc/ctc_mwer.hip behind eec_ctc_hyp_logp / eec_ctc_mwer_forward / _backward;
ctc.ctc_hyp_logp, ctc.exit_mwer_losses, ctc.mwer_nbest, ctc.exit_mwer_training_losses) against the fp64 restatement of
tests/mwer_cases.py, whose own checks tests/test_host_mwer.py runs without a GPU.

Bounds -- the project's own, from tests/test_gpu_ctc.py and distill_cases, carried through the softmax over the list; none is taken
from the kernels under test.  With dW = max - min risk of the list and A = 2e-5 + 2e-5 max_i |ll_i|:
    ll        |err| <= max(2e-5 + 2e-5 |want|, 2 err32)            (-inf and NaN places must agree exactly)
    loss_eb   |err| <= max(dW A, 2 err32)
    gradient  |err| <= max(1e-5 max|grad| + 2 dW A + 1e-9, 2 gerr32)   per (e, b), max|grad| that of the utterance's rows
err32 / gerr32: the same statement evaluated in fp32 on the CPU, against fp64.
Measured on MI355X over the module's comparisons: at most 0.015 (ll), 0.0030 (loss_eb) and 0.0019 (gradient) of the bounds.
"""
import numpy as np
import pytest
import torch

import ctc_cases as CC
import mwer_cases as M
from early_exit_transformer_amd import ctc, scoring, synth
from early_exit_transformer_amd.model import MwerLists, ctc_hyp_logp, exit_ctc_losses, exit_mwer_losses, exit_mwer_training_losses, mwer_nbest

pytestmark = pytest.mark.gpu

def device_forward(x, il, hyp, hl, risk, max_ws=2 << 30):
    """(loss [E], ll [E, B, N], loss_eb [E, B]) of the forward entry, on the CPU."""
    xa, ila, ha, hla, ra = ctc._mwer_args("test", x.cuda(), hyp.cuda(), hl.cuda(), risk.cuda(), il)
    loss, ll, loss_eb, _ = ctc._mwer_forward(xa, ila, ha, hla, ra, 0, max_ws)
    return loss.cpu(), ll.cpu(), loss_eb.cpu()


def device_loss_and_grad(x, il, hyp, hl, risk, w=None, **kw):
    xg = x.detach().clone().cuda().requires_grad_(True)
    loss = exit_mwer_losses(xg, hyp.cuda(), hl.cuda(), risk.cuda(), il, **kw)
    ww = torch.ones_like(loss) if w is None else w.to(loss)
    (loss * ww).sum().backward()
    return loss.detach().cpu(), xg.grad.cpu()


def check_against_fp64(tag, case, w=None, ref=None):
    """Both paths against the fp64 restatement with the module's bounds; returns (loss, ll, loss_eb, grad) of the device."""
    x, il, hyp, hl, risk = case
    want, got32 = ref if ref is not None else (M.statement(*case, dtype=np.float64, w=w), M.statement(*case, dtype=np.float32, w=w))
    ll_bound, loss_bound, grad_bound = M.bounds(want, got32)
    with torch.no_grad():
        loss0 = exit_mwer_losses(x.cuda(), hyp.cuda(), hl.cuda(), risk.cuda(), il).cpu()
        ll0 = ctc_hyp_logp(x.cuda(), hyp.cuda(), hl.cuda(), il).cpu()
    loss1, g = device_loss_and_grad(x, il, hyp, hl, risk, w)
    loss2, ll, loss_eb = device_forward(x, il, hyp, hl, risk)
    assert torch.equal(loss0, loss1) and torch.equal(loss0, loss2), tag  # one forward entry behind every path
    assert torch.equal(ll0, ll) or (torch.equal(torch.isnan(ll0), torch.isnan(ll)) and torch.equal(ll0.nan_to_num(), ll.nan_to_num())), tag
    fin = np.isfinite(want["ll"])
    lln = ll.double().numpy()
    assert (lln[~fin] == want["ll"][~fin]).all(), (tag, lln[~fin], want["ll"][~fin])
    f_ll = (np.abs(lln[fin] - want["ll"][fin]) / ll_bound[fin]).max() if fin.any() else 0.0
    zero_ok = (loss_eb.numpy()[loss_bound == 0] == 0).all()  # a list of equal risks: dW = 0 and the loss is exactly 0
    f_loss = (np.abs(loss_eb.double().numpy() - want["loss_eb"])[loss_bound > 0] / loss_bound[loss_bound > 0]).max() if (loss_bound > 0).any() else 0.0
    gerr = np.abs(g.double().numpy() - want["grad"]).max(axis=(2, 3))
    f_grad = (gerr / grad_bound).max()
    mean_err, mean_bound = np.abs(loss1.double().numpy() - want["loss"]), loss_bound.mean(1)  # loss[e]: the mean of the lists' bounds
    zero_ok = zero_ok and (mean_err[mean_bound == 0] == 0).all()
    f_mean = (mean_err[mean_bound > 0] / mean_bound[mean_bound > 0]).max() if (mean_bound > 0).any() else 0.0
    print(f"\n[mwer {tag}] fractions of the bounds: ll {f_ll:.3f}, loss_eb {f_loss:.2e}, loss {f_mean:.2e}, gradient {f_grad:.2e} "
          f"(max|grad| {np.abs(want['grad']).max():.3e}, max|ll| {np.abs(want['ll'][fin]).max() if fin.any() else 0:.1f})")
    assert zero_ok and f_ll <= 1 and f_loss <= 1 and f_mean <= 1 and f_grad <= 1, tag
    assert torch.isfinite(g).all() and torch.isfinite(loss1).all(), tag
    return loss1, ll, loss_eb, g


def random_case(E, B, T, V, N, max_len, seed=0, scale=2.0, il=None):
    """Random log-probs and random lists with distinct risks 0 .. N - 1 per list."""
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(E, B, T, V, generator=g) * scale, -1)
    hyp = torch.randint(1, V, (E, B, N, max(max_len, 1)), generator=g, dtype=torch.int32)
    hl = torch.randint(0, max_len + 1, (E, B, N), generator=g, dtype=torch.int32)
    risk = torch.argsort(torch.rand(E, B, N, generator=g), -1).float()
    return x, il, hyp, hl, risk


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against fp64 on the shared cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_mwer_matches_fp64_on_peaky_and_trained_like_rows(name):
    """Peaky log-probs (logit scales 2, 8, 16; [2, 3, 19, 256]) and the committed trained-like fixture ([6, 4, 16, 256]) with lists
    of 4 that hold the greedy path, a deletion, a substitution, the empty hypothesis and, rotating, an absent, an infeasible and a
    duplicate entry, frame lengths cycling [T, 1, 7, 0]: the no-grad and the autograd path (equal bits), ctc_hyp_logp, unweighted
    (the shared reference) and with per-exit weights.
    Measured on MI355X, as fractions of the bounds (every comparison prints its own): ll at most 0.015 (the fixture, max|ll| 492), loss_eb 2.1e-3, the gradient
    2.4e-5 -- its bound is dominated by 2 dW A; on the peaky cases one entry holds nearly all the mass and max|grad| is 3e-9 (scale 8)
    to 1.5e-2 (scale 2).  The first terms of the bounds hold everywhere, 2 * err32 is not needed."""
    case, r64, r32 = M.reference(name)
    check_against_fp64(name, case, ref=(r64, r32))
    _, w64, w32 = M.reference(name, weighted=True)
    check_against_fp64(name + " weighted", case, w=M.exit_weights(case[0].size(0)), ref=(w64, w32))


def test_wrapper_normalises_fp64_and_non_contiguous_inputs():
    x, il, hyp, hl, risk = M.cases()["scale2"]
    loss, g = device_loss_and_grad(x, il, hyp, hl, risk)
    x64 = x.double().cuda().requires_grad_(True)
    l64 = exit_mwer_losses(x64, hyp.cuda(), hl.cuda(), risk.cuda(), il)
    l64.sum().backward()
    assert torch.equal(l64.cpu(), loss) and x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float().cpu(), g)
    xt = x.transpose(0, 1).contiguous().cuda().requires_grad_(True)
    lt = exit_mwer_losses(xt.transpose(0, 1), hyp.cuda(), hl.cuda(), risk.double().cuda(), il)
    lt.sum().backward()
    assert torch.equal(lt.cpu(), loss) and torch.equal(xt.grad.transpose(0, 1).cpu(), g)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. one gradient buffer with the CTC loss
# ---------------------------------------------------------------------------------------------------------------------------
def test_training_losses_are_the_two_calls_and_share_one_gradient_buffer():
    """exit_mwer_training_losses: the values of exit_ctc_losses and exit_mwer_losses bit for bit; the gradient of
    0.7 ctc.sum() + mwer.sum() is the sum of the two gradients within one rounding of that sum; with the MWER output unused it is
    the CTC gradient bit for bit."""
    x, il, hyp, hl, risk = M.cases()["fixture"]
    tgt, tl = CC.greedy_targets(x[0])
    lists = MwerLists(hyp.cuda(), hl.cuda(), risk.cuda(), torch.zeros_like(risk).cuda())

    def grad_of(f):
        xg = x.detach().clone().cuda().requires_grad_(True)
        f(xg).backward()
        return xg.grad.cpu()
    with torch.no_grad():
        c0, m0 = exit_mwer_training_losses(x.cuda(), tgt, tl, lists, input_len=il)
    assert torch.equal(c0, exit_ctc_losses(x.cuda(), tgt, tl, input_len=il)) and torch.equal(m0.cpu(), device_forward(x, il, hyp, hl, risk)[0])
    xg = x.detach().clone().cuda().requires_grad_(True)
    c1, m1 = exit_mwer_training_losses(xg, tgt, tl, lists, input_len=il)
    c_alone = exit_ctc_losses(x.detach().clone().cuda().requires_grad_(True), tgt, tl, input_len=il)  # the training forward of the CTC loss
    assert torch.equal(c1.detach(), c_alone.detach()) and torch.equal(m1.detach(), m0)
    (0.7 * c1.sum() + m1.sum()).backward()
    g_ctc = grad_of(lambda t: 0.7 * exit_ctc_losses(t, tgt, tl, input_len=il).sum())
    g_mwer = grad_of(lambda t: exit_mwer_losses(t, lists.tokens, lists.lengths, lists.risk, il).sum())
    assert g_mwer.abs().max() > 0
    want = g_ctc.double() + g_mwer.double()
    err = (xg.grad.cpu().double() - want).abs()
    assert (err <= 2.0 ** -23 * want.abs()).all(), err.max().item()
    g_unused = grad_of(lambda t: 0.7 * exit_mwer_training_losses(t, tgt, tl, lists, input_len=il)[0].sum())
    assert torch.equal(g_unused, g_ctc)
    g_only = grad_of(lambda t: exit_mwer_training_losses(t, tgt, tl, lists, input_len=il)[1].sum())
    assert torch.equal(g_only, g_mwer)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. shapes at which the code takes another path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [63, 64, 127, 128, 255])
def test_hypothesis_lengths_at_the_states_per_lane_boundaries(S):
    """2 S + 1 states against 64 lanes x 2 / 4 / 8 states: T' = 2 S + 6, V = 64, one list of a hypothesis and a substitution of it."""
    g = torch.Generator().manual_seed(S)
    T, V = 2 * S + 6, 64
    x = torch.log_softmax(torch.randn(1, 1, T, V, generator=g), -1)
    h = torch.randint(1, V, (S,), generator=g, dtype=torch.int32)
    h2 = h.clone()
    h2[S // 2] = 1 + (int(h[S // 2]) % (V - 1))
    hyp = torch.stack([h, h2]).view(1, 1, 2, S)
    check_against_fp64(f"S={S}", (x, None, hyp, torch.full((1, 1, 2), S, dtype=torch.int32), torch.tensor([[[0.0, 1.0]]])))


@pytest.mark.parametrize("V", [4, 32, 252, 256])
def test_vocabulary_sizes(V):
    check_against_fp64(f"V={V}", random_case(2, 2, 9, V, 3, 4, seed=V))


@pytest.mark.parametrize("N", [1, 2, 16])
def test_list_sizes(N):
    case = random_case(2, 3, 11, 32, N, 5, seed=N, il=torch.tensor([11, 6, 2]))
    loss, _, loss_eb, g = check_against_fp64(f"N={N}", case)
    if N == 1:
        assert (loss == 0).all() and (loss_eb == 0).all() and (g == 0).all()


def test_one_frame():
    check_against_fp64("T'=1", random_case(2, 3, 1, 16, 4, 2, seed=5))


def test_absent_lists_and_utterances_without_frames():
    """A list that is all absent, and Tb = 0: loss 0, zero gradient rows, nothing NaN."""
    x, _, hyp, hl, risk = random_case(2, 3, 8, 16, 4, 3, seed=7)
    hl[1, 2] = -1
    il = torch.tensor([8, 0, 5])
    loss, ll, loss_eb, g = check_against_fp64("absent / Tb=0", (x, il, hyp, hl, risk))
    assert loss_eb[1, 2] == 0 and (g[1, 2] == 0).all() and (ll[1, 2] == float("-inf")).all()
    assert (loss_eb[:, 1] == 0).all() and (g[:, 1] == 0).all()
    assert ((ll[:, 1] == 0) == (hl[:, 1] == 0)).all() and ((ll[:, 1] == float("-inf")) == (hl[:, 1] != 0)).all()
    assert g.abs().max() > 0


def test_nan_placement():
    """NaN at frames at or past Tb reaches nothing; NaN inside the valid frames reaches its (e, b) only."""
    case = random_case(2, 3, 8, 16, 4, 3, seed=11, il=torch.tensor([8, 5, 3]))
    x, il, hyp, hl, risk = case
    loss, ll, loss_eb = device_forward(*case)
    _, g = device_loss_and_grad(*case)
    past = x.clone()
    past[:, 1, 5:] = float("nan")
    past[:, 2, 3:] = float("nan")
    loss_p, ll_p, loss_eb_p = device_forward(past, il, hyp, hl, risk)
    assert torch.equal(loss_p, loss) and torch.equal(ll_p, ll) and torch.equal(loss_eb_p, loss_eb)
    assert torch.equal(device_loss_and_grad(past, il, hyp, hl, risk)[1], g)
    inside = x.clone()
    inside[0, 1, 2, 0] = float("nan")  # the blank of a valid frame: every lattice of (0, 1) reads it
    loss_i, ll_i, loss_eb_i = device_forward(inside, il, hyp, hl, risk)
    _, g_i = device_loss_and_grad(inside, il, hyp, hl, risk)
    keep = torch.ones(2, 3, dtype=torch.bool)
    keep[0, 1] = False
    assert torch.equal(ll_i[keep], ll[keep]) and torch.equal(loss_eb_i[keep], loss_eb[keep]) and torch.equal(g_i[keep], g[keep])
    assert torch.isnan(loss_eb_i[0, 1]) and torch.isnan(loss_i[0]) and loss_i[1] == loss[1]
    assert torch.isnan(ll_i[0, 1][hl[0, 1] >= 0]).all() and torch.isnan(g_i[0, 1, :5]).all() and (g_i[0, 1, 5:] == 0).all()


@pytest.mark.parametrize("what", ["length above the pitch", "length below -1", "label V", "label -1", "label blank"])
def test_refused_input_gives_nan_in_its_own_loss_only(what):
    case = random_case(2, 3, 8, 16, 4, 3, seed=13)
    x, il, hyp, hl, risk = case
    loss, ll, loss_eb = device_forward(*case)
    _, g = device_loss_and_grad(*case)
    hyp, hl = hyp.clone(), hl.clone()
    hl[1, 0, 2] = 2
    if what.startswith("length"):
        hl[1, 0, 2] = 4 if "above" in what else -2
    else:
        hyp[1, 0, 2, 1] = {"label V": 16, "label -1": -1, "label blank": 0}[what]
    loss_b, ll_b, loss_eb_b = device_forward(x, il, hyp, hl, risk)
    _, g_b = device_loss_and_grad(x, il, hyp, hl, risk)
    keep = torch.ones(2, 3, dtype=torch.bool)
    keep[1, 0] = False
    assert torch.isnan(loss_eb_b[1, 0]) and torch.isnan(loss_b[1]) and torch.isnan(ll_b[1, 0, 2])
    assert loss_b[0] == loss[0] and torch.equal(loss_eb_b[keep], loss_eb[keep]) and torch.equal(ll_b[keep], ll[keep])
    others = torch.tensor([0, 1, 3])
    assert torch.equal(ll_b[1, 0, others], ll[1, 0, others])
    assert torch.equal(g_b[keep], g[keep]) and (g_b[1, 0] == 0).all()


def test_runs_slices_and_splits_return_the_same_bits():
    """Two runs; a call on enc_out[1:] and one on enc_out[:, 1:] (ll and loss_eb: the loss and the gradient carry 1 / B); a split
    under a tiny max_workspace_bytes."""
    case = M.cases()["fixture"]
    x, il, hyp, hl, risk = case
    loss, ll, loss_eb = device_forward(*case)
    _, g = device_loss_and_grad(*case)
    again = device_forward(*case)
    assert torch.equal(again[0], loss) and torch.equal(again[1], ll) and torch.equal(again[2], loss_eb)
    assert torch.equal(device_loss_and_grad(*case)[1], g)
    le, lle, lebe = device_forward(x[1:], il, hyp[1:], hl[1:], risk[1:])
    assert torch.equal(le, loss[1:]) and torch.equal(lle, ll[1:]) and torch.equal(lebe, loss_eb[1:])
    assert torch.equal(device_loss_and_grad(x[1:], il, hyp[1:], hl[1:], risk[1:])[1], g[1:])
    _, llb, lebb = device_forward(x[:, 1:], il[1:], hyp[:, 1:], hl[:, 1:], risk[:, 1:])
    assert torch.equal(llb, ll[:, 1:]) and torch.equal(lebb, loss_eb[:, 1:])
    assert len(ctc._mwer_chunks(x.cuda(), 4, hyp.size(3), 1)) == x.size(1)
    ls, lls, lebs = device_forward(*case, max_ws=1)
    assert torch.equal(ls, loss) and torch.equal(lls, ll) and torch.equal(lebs, loss_eb)
    ls2, gs = device_loss_and_grad(*case, max_workspace_bytes=1)
    assert torch.equal(ls2, loss) and torch.equal(gs, g)
    w = M.exit_weights(x.size(0)).float()
    assert torch.equal(device_loss_and_grad(*case, w=w, max_workspace_bytes=1)[1], device_loss_and_grad(*case, w=w)[1])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. with the decoder and the scorer
# ---------------------------------------------------------------------------------------------------------------------------
def test_exact_scores_of_the_beams_lists_are_no_smaller_than_the_pruned_ones():
    """ctc_hyp_logp of mwer_nbest's lists on beam_logp(8, 64, 64, 3.0): ll >= score - 2e-3 max(1, |score|) -- pruning only loses
    mass, the margin is the beam test's SCORE_RTOL --; ranks past n_hyp come back absent; the risks are the edit distances."""
    x = CC.beam_logp(8, 64, 64, 3.0).view(2, 4, 64, 64)
    tgt, tl = synth.synth_targets(4, 12, 64, seed=3)
    lists = mwer_nbest(x.cuda(), tgt, tl, nbest=4, beam_size=10)
    assert lists.tokens.shape[:3] == (2, 4, 4) and lists.tokens.size(3) == max(int(lists.lengths.max()), 1)
    ll = ctc_hyp_logp(x.cuda(), lists.tokens, lists.lengths).cpu()
    scores, lengths = lists.scores.cpu(), lists.lengths.cpu()
    present = lengths >= 0
    assert present[:, :, 0].all() and torch.equal(present, scores > float("-inf"))
    assert (ll[~present] == float("-inf")).all() and torch.isfinite(ll[present]).all()
    slack = ll[present] - (scores[present] - 2e-3 * scores[present].abs().clamp(min=1))
    print(f"\n[mwer nbest] exact - pruned score: min {(ll[present] - scores[present]).min().item():.2e}, max {(ll[present] - scores[present]).max().item():.2e}")
    assert (slack >= 0).all()
    ref_of = (torch.arange(8, dtype=torch.int32) % 4).repeat_interleave(4)
    want = scoring.edit_counts(lists.tokens.cpu().view(16 + 16, -1), lengths.clamp(min=0).view(-1), tgt.to(torch.int32), tl.to(torch.int32), ref_of=ref_of)
    assert torch.equal(lists.risk.cpu().view(-1), want.distance.float())
    # a narrow beam leaves ranks empty: they come back absent
    narrow = mwer_nbest(x.cuda(), tgt, tl, nbest=4, beam_size=4, blank_skip_threshold=0.5)
    absent = narrow.lengths.cpu() < 0
    assert torch.equal(absent, narrow.scores.cpu() == float("-inf"))
    assert (ctc_hyp_logp(x.cuda(), narrow.tokens, narrow.lengths).cpu()[absent] == float("-inf")).all()
    c, m = exit_mwer_training_losses(x.cuda(), tgt, tl, nbest=4, beam_size=10)
    assert torch.equal(m, exit_mwer_losses(x.cuda(), lists.tokens, lists.lengths, lists.risk)) and torch.equal(c, exit_ctc_losses(x.cuda(), tgt, tl))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. descent
# ---------------------------------------------------------------------------------------------------------------------------
def test_descent_on_the_device_follows_the_restatement():
    """20 plain gradient steps on logits [1, 2, 24, 16] under log_softmax, fixed lists of 4 with distinct risks: the restatement
    decreases at every step at mwer_cases.DESCENT_LR (tests/test_host_mwer.py checks that on the CPU), the device path must too, and ends within 1e-3 of the restatement's trajectory."""
    want = M.restatement_trajectory()
    assert all(b < a for a, b in zip(want, want[1:])), want
    logits, hyp, hl, risk = M.descent_case()
    z = logits.float().cuda().requires_grad_(True)
    got = []
    for _ in range(21):
        loss = exit_mwer_losses(torch.log_softmax(z, -1), hyp.cuda(), hl.cuda(), risk.cuda()).sum()
        got.append(loss.item())
        (g,) = torch.autograd.grad(loss, z)
        z = (z - M.DESCENT_LR * g).detach().requires_grad_(True)
    print(f"\n[mwer descent] restatement {want[0]:.5f} -> {want[-1]:.5f}, device {got[0]:.5f} -> {got[-1]:.5f}")
    assert all(b < a for a, b in zip(got, got[1:])), got
    assert abs(got[-1] - want[-1]) <= 1e-3 and max(abs(a - b) for a, b in zip(got, want)) <= 1e-3
