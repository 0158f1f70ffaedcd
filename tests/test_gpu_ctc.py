"""GPU tests of the CTC family (csrc/ctc.hip: loss, beta recursion, dense gradient, reduce; csrc/ctc_beam.hip: prefix beam
search) on trained-like (peaky) log-probs, at the edge of the loss kernel's dynamic range and at the shape and argument edges.

Reference of the loss and gradient: nn.CTCLoss(blank, 'mean', zero_infinity=True) through the reference's per-exit loop in fp64
on the CPU (ctc_cases.ref_ctc); of the beam search: oracle/ctc_beam_ref.py (fp64).  Inputs: tests/ctc_cases.py, whose
reference values and inclusion shares tests/test_oracle.py asserts without a GPU.

Bounds (none of them chosen from what the kernels give):
    loss      rtol = atol = 2e-5 against fp64                      (test_exit_ctc_losses_match_torch_ctc)
    gradient  1e-5 * max|grad| + 1e-9 against fp64                 (test_ctc_gradient_matches_torch_autograd)
    either    or, where that is exceeded, 2 x the reference's OWN fp32 error against fp64 on the same input (err32)
    beam      score 2e-3 * max(1, |score|); tokens identical when the oracle's best leads by more than 5e-3
"""
import math

import pytest
import torch

import ctc_cases as C
from early_exit_transformer_amd.model import ctc_beam_decode, exit_ctc_losses
from oracle.ctc_beam_ref import ctc_prefix_beam_search

pytestmark = pytest.mark.gpu


def hip_losses(logp, tgt, tl, blank=0):
    """The no-grad entry (eec_ctc_loss)."""
    with torch.no_grad():
        return exit_ctc_losses(logp.cuda(), tgt, tl, blank=blank).cpu().double()


def hip_loss_and_grad(logp, tgt, tl, blank=0, w=None):
    """The autograd pair (eec_ctc_loss_forward / _backward)."""
    x = logp.detach().clone().cuda().requires_grad_(True)
    losses = exit_ctc_losses(x, tgt, tl, blank=blank)
    ww = torch.ones_like(losses) if w is None else w.cuda()
    (losses * ww).sum().backward()
    return losses.detach().cpu().double(), x.grad.cpu().double()


def check_against_fp64(tag, logp, tgt, tl, blank=0, w=None, grad=True):
    """Both entries against the fp64 reference with the module's bounds; returns the figures it printed."""
    logp = logp.float()
    want, gw = C.ref_ctc(logp, tgt, tl, blank, torch.float64, w)
    want32, g32 = C.ref_ctc(logp, tgt, tl, blank, torch.float32, w)
    lerr32 = (want32.double() - want).abs()
    bound = torch.maximum(2e-5 + 2e-5 * want.abs(), 2 * lerr32)
    got0 = hip_losses(logp, tgt, tl, blank)
    lerr0 = (got0 - want).abs()
    line = f"[ctc {tag}] loss {want.max().item():.4f}: HIP err {lerr0.max().item():.2e} (no-grad)"
    if grad:
        got1, g = hip_loss_and_grad(logp, tgt, tl, blank, w)
        lerr1 = (got1 - want).abs()
        ok = torch.isfinite(gw)  # the reference's gradient is NaN at exact -inf inputs outside the target; the kernel's is 0 there
        scale = gw[ok].abs().max().item()
        gerr, gerr32 = (g - gw)[ok].abs().max().item(), (g32.double() - gw)[ok].abs().max().item()
        line += f" {lerr1.max().item():.2e} (autograd), torch-fp32 err {lerr32.max().item():.2e}; max|grad| {scale:.3e}: HIP err {gerr:.2e}, torch-fp32 err {gerr32:.2e}"
    print("\n" + line)
    assert torch.isfinite(got0).all() and (lerr0 <= bound).all(), (tag, got0.tolist(), want.tolist(), lerr32.tolist())
    if grad:
        assert torch.isfinite(got1).all() and (lerr1 <= bound).all(), (tag, got1.tolist(), want.tolist(), lerr32.tolist())
        assert torch.isfinite(g).all(), tag
        assert (g[~ok] == 0).all(), tag
        assert gerr <= max(1e-5 * scale + 1e-9, 2 * gerr32), (tag, gerr, gerr32, scale)
        # the gradient with respect to log-softmax outputs sums to zero over the classes of every frame
        assert g.sum(-1).abs().max().item() < 1e-5 * max(scale, 1e-6) * logp.size(-1), tag
    return line


def per_lattice(logp, tgt, tl):
    """One-utterance batches: every lattice's own loss, [E, B] (0 where the lattice is infeasible: zero_infinity)."""
    return torch.stack([hip_losses(logp[:, b:b + 1], tgt[b:b + 1], tl[b:b + 1]) for b in range(logp.size(1))], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. peaky log-probs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("kind", ["matching", "mismatched"])
@pytest.mark.parametrize("name", ["scale2", "scale5", "scale9", "scale16", "fixture"])
def test_ctc_loss_and_gradient_on_peaky_logprobs(name, kind, P):
    """Loss (both entries) and dense gradient on log_softmax(randn * scale) with max |log-prob| 17 / 38 / 68 / 120 and on the
    committed peaky fixture's rows (59), with the greedy decode as target (a dominant path: loss < 50) and with unrelated
    targets (every path improbable: loss 50 .. 330 per utterance), at 2 / 4 / 8 states per lane (the padded target width
    selects the template instance).  Every lattice's loss is also compared on its own (finite where the reference's is).
    Measured on MI355X, error against fp64 (HIP | torch's own fp32 evaluation = err32), the same at P = 2, 4, 8:
        loss      randn*2 5.0e-6 | 8.8e-6   randn*5 6.9e-6 | 1.5e-5   randn*9 1.9e-5 | 1.8e-5   randn*16 1.4e-5 | 6.7e-5   fixture 2.2e-6 | 4.1e-6
        gradient  randn*2 4.8e-8 | 7.5e-6   randn*5 4.8e-8 | 2.3e-5   randn*9 2.9e-8 | 2.9e-5   randn*16 2.7e-8 | 5.0e-5   fixture 1.8e-8 | 4.0e-6
    (mismatched targets; matching ones are 3 to 10 times closer).  The existing bounds hold on every case; 2 * err32 is not needed.
    Before the kernels watched their range ("CTC loss: dynamic range") the same cases gave 9.90 for 14.62 (randn*5,
    P = 4), 0 for 329.5 (randn*16) and gradients of 1e26 and NaN (randn*5 P = 4, fixture P = 4 and 8)."""
    lp, match, mism = C.part1_cases()[name]
    tgt, tl = match if kind == "matching" else mism
    if tgt.size(1) > C.WIDTH_FOR_P[P]:
        assert P == 2 and tgt.size(1) == 64  # the greedy decode of 64 distinct frames: one label per frame, P = 4
        tgt, tl = tgt[:, :63], tl.clamp(max=63)
    tgt = C.pad_targets(tgt, C.WIDTH_FOR_P[P])
    w = torch.linspace(0.5, 1.5, lp.size(0))
    check_against_fp64(f"{name} {kind} P{P}", lp, tgt, tl, w=w)
    E, B = lp.shape[:2]
    want = torch.tensor([[C.ref_nll(lp[e, b], tgt[b, : int(tl[b])].tolist()) / max(int(tl[b]), 1) for b in range(B)] for e in range(E)], dtype=torch.float64)
    got = per_lattice(lp, tgt, tl)
    assert torch.isfinite(want).all()
    assert torch.allclose(got, want, rtol=2e-5, atol=2e-5), (got - want).abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the dynamic range of the loss kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 4, 8])
def test_ctc_dynamic_range(P):
    """Hand-built lattices (T' = 40, V = 8) whose blank and target labels all sit at -x, x = 20 .. 80, on frames that share a
    renormalisation of the block-floating recursion, straddle one, open the sequence, lie past the first look-ahead group or in
    the ragged tail (forward) and at the start of the beta recursion; one frame at -95 (below the fp32 range of exp); exact -inf
    on classes outside the target.  The fp64 reference loss is finite on every one (120 .. 320): the kernel's must be finite and
    within the bound of the module, and so must the gradient.  One launch holds all lattices of a target (E = 38, B = 1), so every
    lattice's loss is returned on its own.
    Measured on MI355X against fp64 (HIP | err32): loss 1.0e-5 | 3.3e-5, gradient 2.5e-7 | 3.8e-5 of a scale of 0.5, at every P.
    The block-floating recursion alone returned 0 (zero_infinity) from x = 60 on every pair inside one renormalisation, from
    x = 40 on frames 0-2 and on both x = 95 lattices, and 90.046 for 90.053 at x = 50; such lattices now take the wide path."""
    cases = C.range_cases()
    for target in ((3, 4), (3,)):
        sel = [c for c in cases if c[2] == target]
        lp = torch.stack([c[1] for c in sel]).unsqueeze(1).float()  # [E, 1, T', V]
        tgt = C.pad_targets(torch.tensor([list(target)]), C.WIDTH_FOR_P[P])
        tl = torch.tensor([len(target)])
        want, _ = C.ref_ctc(lp, tgt, tl)
        got = hip_losses(lp, tgt, tl)
        for (nm, _, _), g, w_ in zip(sel, got.tolist(), want.tolist()):
            print(f"[ctc range P{P}] {nm}: HIP {g:.5f} fp64 {w_:.5f}")
        check_against_fp64(f"range P{P} target {target}", lp, tgt, tl)


@pytest.mark.parametrize("P", [2, 4, 8])
def test_ctc_infeasible_by_masking_is_zero_with_zero_gradient(P):
    """-inf on a class every alignment needs: the reference's loss is +inf, 0 under zero_infinity, with a zero gradient; the
    kernel agrees (no NaN), also next to a feasible lattice in the same launch."""
    for nm, lp, target in C.infeasible_cases():
        lp = lp.float().view(1, 1, *lp.shape)
        tgt = C.pad_targets(torch.tensor([list(target)]), C.WIDTH_FOR_P[P])
        tl = torch.tensor([len(target)])
        assert hip_losses(lp, tgt, tl).item() == 0.0, nm
        loss, g = hip_loss_and_grad(lp, tgt, tl)
        assert loss.item() == 0.0 and (g == 0).all(), nm
        both = torch.cat([lp, torch.log_softmax(torch.zeros_like(lp), -1)], 0)  # exit 1: uniform rows, feasible
        want, gw = C.ref_ctc(both, tgt, tl)
        loss, g = hip_loss_and_grad(both, tgt, tl)
        assert want[0].item() == 0.0 and loss[0].item() == 0.0 and (g[0] == 0).all(), nm
        assert torch.allclose(loss, want, rtol=2e-5, atol=2e-5) and (g[1] - gw[1]).abs().max().item() < 1e-5 * gw[1].abs().max().item() + 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# 3. shape and argument edges
# ---------------------------------------------------------------------------------------------------------------------------
def rand_logp(E, B, T, V, seed=0, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(E, B, T, V, generator=g) * scale, -1)


def rand_targets(B, S, V, seed=0, blank=0, lens=None):
    g = torch.Generator().manual_seed(seed + 5)
    tgt = torch.randint(1, V, (B, S), generator=g)
    if blank != 0:
        tgt = torch.where(tgt == blank, torch.zeros_like(tgt), tgt)  # label 0 is an ordinary class then
    tl = torch.full((B,), S, dtype=torch.int64) if lens is None else torch.tensor(lens, dtype=torch.int64)
    return tgt, tl


def test_ctc_empty_targets():
    """Target length 0: the loss is minus the sum of the blank log-probs (max(len, 1) in the mean): for one utterance of a batch,
    for all of them, and mixed lengths 0, 1 and S."""
    lp = rand_logp(2, 4, 20, 32, seed=1)
    tgt, _ = rand_targets(4, 7, 32, seed=1)
    for lens in ([7, 0, 3, 7], [0, 0, 0, 0], [0, 1, 7, 1]):
        check_against_fp64(f"lens {lens}", lp, tgt, torch.tensor(lens))
    got = hip_losses(lp, tgt, torch.zeros(4, dtype=torch.int64))
    assert torch.allclose(got, -lp[..., 0].double().sum(-1).mean(-1), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("S", [63, 64, 127, 128, 255])
def test_ctc_target_width_at_the_states_per_lane_boundaries(S):
    """S = 63 | 64, 127 | 128 switch between 2, 4 and 8 states per lane; 255 fills all 512 states of a wave."""
    T = 2 * S + 6
    lp = rand_logp(1, 3, T, 64, seed=S)
    tgt, tl = rand_targets(3, S, 64, seed=S, lens=[S, S // 2, 1])
    check_against_fp64(f"S{S}", lp, tgt, tl)


def test_ctc_target_width_256_is_refused():
    lp = rand_logp(1, 1, 8, 32).cuda()
    tgt, tl = torch.ones(1, 256, dtype=torch.int64), torch.tensor([2])
    with pytest.raises(Exception, match="255"):
        with torch.no_grad():
            exit_ctc_losses(lp, tgt, tl)
    with pytest.raises(Exception, match="255"):
        exit_ctc_losses(lp.clone().requires_grad_(True), tgt, tl)


@pytest.mark.parametrize("P", [2, 8])
@pytest.mark.parametrize("T", [1, 2, 8, 9, 16, 17, 33])
def test_ctc_frame_counts_around_the_lookahead_ring(T, P):
    """T' shorter than one look-ahead group, exact groups and ragged tails for both ring depths (16 for P <= 4, 8 for P = 8)."""
    S = min(3, T)
    lp = rand_logp(2, 3, T, 32, seed=T)
    tgt, tl = rand_targets(3, S, 32, seed=T, lens=[S, 1, 0])
    check_against_fp64(f"T{T} P{P}", lp, C.pad_targets(tgt, C.WIDTH_FOR_P[P]), tl)


@pytest.mark.parametrize("P", [2, 4, 8])
def test_ctc_single_feasible_alignment_and_one_frame_less(P):
    """T' == len + repeats: exactly one alignment (its log-prob is the loss); T' one less: infeasible, 0 with a zero gradient."""
    target = [5, 5, 6, 7, 7, 7, 3]  # 3 adjacent repeats
    need = len(target) + 3
    tgt, tl = C.pad_targets(torch.tensor([target]), C.WIDTH_FOR_P[P]), torch.tensor([len(target)])
    lp = rand_logp(2, 1, need, 32, seed=3)
    check_against_fp64(f"single alignment P{P}", lp, tgt, tl)
    path = [5, 0, 5, 6, 7, 0, 7, 0, 7, 3]
    want = -sum(lp[0, 0, t, c].double() for t, c in enumerate(path)) / len(target)
    assert abs(hip_losses(lp, tgt, tl)[0] - want) < 2e-5 * (1 + want)
    short = lp[:, :, :-1].contiguous()
    assert C.ref_ctc(short, tgt, tl)[0].abs().max().item() == 0.0
    assert hip_losses(short, tgt, tl).abs().max().item() == 0.0
    loss, g = hip_loss_and_grad(short, tgt, tl)
    assert loss.abs().max().item() == 0.0 and (g == 0).all()


@pytest.mark.parametrize("P", [2, 4, 8])
def test_ctc_repeats_within_and_across_lanes(P):
    """One label repeated S times, and adjacent repeats placed on every state offset of a lane (state 2k + 1 of label k: the
    pair (k, k + 1) sweeps all positions lane * P - 1 .. lane * P + 1, where the skip flag of a lane's first states and the
    neighbour lane's values meet)."""
    S = 32
    lp = rand_logp(2, 2, 4 * S, 32, seed=P)
    tgt = C.pad_targets(torch.full((2, S), 9), C.WIDTH_FOR_P[P])
    check_against_fp64(f"one label x{S} P{P}", lp, tgt, torch.tensor([S, S // 2]))
    base, _ = rand_targets(1, S, 32, seed=P)
    base[0, 1:] = torch.where(base[0, 1:] == base[0, :-1], base[0, 1:] % 30 + 1, base[0, 1:])  # no accidental repeats
    rows = []
    for k in range(2 * P + 2):  # label pairs (k, k + 1), (k + P, k + P + 1): states 2k + 1 .. 2k + 3 cross every lane offset
        r = base[0].clone()
        r[k + 1] = r[k]
        r[k + P + 1] = r[k + P]
        rows.append(r)
    tgt = C.pad_targets(torch.stack(rows), C.WIDTH_FOR_P[P])
    lp = rand_logp(1, len(rows), 3 * S, 32, seed=P + 10)
    check_against_fp64(f"repeats across lanes P{P}", lp, tgt, torch.full((len(rows),), S))


@pytest.mark.parametrize("V", [4, 96, 160, 252])
def test_ctc_vocabulary_sizes(V):
    """The gradient kernel writes one float4 per lane under c0 < V: V = 4 (one lane), not a multiple of 64, the last multiple of 4."""
    lp = rand_logp(2, 3, 30, V, seed=V)
    tgt, tl = rand_targets(3, 6, V, seed=V, lens=[6, 3, 1])
    check_against_fp64(f"V{V}", lp, tgt, tl)


@pytest.mark.parametrize("V", [30, 257, 260])
def test_ctc_autograd_refuses_unsupported_vocabularies(V):
    """V % 4 != 0 or V > 256: the autograd path raises; the no-grad loss has no such limit and still matches."""
    lp = rand_logp(1, 2, 12, V, seed=V)
    tgt, tl = rand_targets(2, 3, V, seed=V)
    with pytest.raises(ValueError, match="multiple of 4"):
        exit_ctc_losses(lp.cuda().requires_grad_(True), tgt, tl)
    check_against_fp64(f"V{V} no-grad", lp, tgt, tl, grad=False)


@pytest.mark.parametrize("blank", [1, 17, 31])
def test_ctc_blank_other_than_zero(blank):
    lp = rand_logp(2, 3, 25, 32, seed=blank)
    tgt, tl = rand_targets(3, 8, 32, seed=blank, blank=blank, lens=[8, 4, 0])
    tgt[0, 1] = 0  # label 0 is an ordinary class
    check_against_fp64(f"blank {blank}", lp, tgt, tl, blank=blank)


@pytest.mark.parametrize("E,B", [(1, 1), (1, 63), (6, 64), (1, 65), (6, 130)])
def test_ctc_batch_sizes_around_the_reduce_kernels_walk(E, B):
    """ctc_reduce_kernel adds 64 utterances' terms per pass: one short pass, one full, one full + 1, two full + 2; E = 1 and 6."""
    lp = rand_logp(E, B, 12, 32, seed=B)
    tgt, _ = rand_targets(B, 4, 32, seed=B)
    tl = torch.arange(B) % 5
    check_against_fp64(f"E{E} B{B}", lp, tgt, tl, w=torch.linspace(0.5, 1.5, E))


def test_ctc_backward_twice_raises_and_live_forwards_keep_their_workspaces():
    lp1, lp2 = rand_logp(2, 3, 20, 32, seed=1), rand_logp(2, 3, 20, 32, seed=2)
    tgt, tl = rand_targets(3, 5, 32, seed=1, lens=[5, 2, 3])
    _, g1 = hip_loss_and_grad(lp1, tgt, tl)
    _, g2 = hip_loss_and_grad(lp2, tgt, tl)
    x1, x2 = lp1.cuda().requires_grad_(True), lp2.cuda().requires_grad_(True)
    l1 = exit_ctc_losses(x1, tgt, tl).sum()
    l2 = exit_ctc_losses(x2, tgt, tl).sum()  # both forwards alive
    l2.backward()
    l1.backward(retain_graph=True)
    assert torch.equal(x1.grad.cpu().double(), g1) and torch.equal(x2.grad.cpu().double(), g2)
    with pytest.raises(RuntimeError, match="twice"):
        l1.backward()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. prefix beam search
# ---------------------------------------------------------------------------------------------------------------------------
def check_beam(tag, logp, beam, blank=0, thr=0.95, readings=(False, True), min_share=0.75):
    """Score within 2e-3 * max(1, |score|) on every sequence; tokens identical on every sequence whose oracle margin is safe, which
    must be at least ``min_share`` of them."""
    N = logp.size(0)
    for drop in readings:
        tok, cnt, sc = (t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=beam, blank=blank, blank_skip_threshold=thr, skip_drops_frame=drop))
        checked = 0
        for n in range(N):
            want, wscore, final = ctc_prefix_beam_search(logp[n].double().numpy(), beam=beam, blank=blank, blank_skip_threshold=thr,
                                                         return_beams=True, skip_drops_frame=drop)
            assert abs(float(sc[n]) - wscore) < 2e-3 * max(1.0, abs(wscore)), (tag, drop, n, float(sc[n]), wscore)
            if C.safe_margin(final):
                assert int(cnt[n]) == len(want) and tok[n, : int(cnt[n])].tolist() == want, (tag, drop, n)
                checked += 1
        assert checked >= math.ceil(min_share * N), (tag, drop, checked, N)


@pytest.mark.parametrize("N,T,V,beam,scale", C.BEAM_CASES)
def test_ctc_beam_on_peaky_logprobs(N, T, V, beam, scale):
    check_beam(f"scale {scale}", C.beam_logp(N, T, V, scale), beam)


def test_ctc_beam_on_the_peaky_fixture():
    check_beam("fixture", C.fixture_beam_logp(), 10)


@pytest.mark.parametrize("case", range(len(C.BEAM_CASES) + 1))
def test_ctc_beam_scores_never_exceed_the_ctc_probability(case):
    """A check that shares nothing with the search: with the skip rule off, the score of the returned prefix is the mass of the
    alignments the pruned search kept, so it cannot exceed log p_ctc(tokens) (fp64 CTCLoss, reduction 'sum')."""
    logp = C.fixture_beam_logp() if case == len(C.BEAM_CASES) else C.beam_logp(*C.BEAM_CASES[case][:3], C.BEAM_CASES[case][4])
    beam = 10 if case == len(C.BEAM_CASES) else C.BEAM_CASES[case][3]
    tok, cnt, sc = (t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=beam, blank_skip_threshold=1.0))
    for n in range(logp.size(0)):
        full = -C.ref_nll(logp[n], tok[n, : int(cnt[n])].tolist())
        assert float(sc[n]) <= full + 2e-3 * max(1.0, abs(full)), (n, float(sc[n]), full)


def test_ctc_beam_is_exact_where_it_cannot_prune():
    """V = 3, T' <= 3: at most 7 prefixes exist, beam 16 keeps them all, so score == log p_ctc(tokens) and the prefix is the most
    probable labelling."""
    g = torch.Generator().manual_seed(3)
    for T in (1, 2, 3):
        logp = torch.log_softmax(torch.randn(16, T, 3, generator=g) * 2, -1)
        tok, cnt, sc = (t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=16, blank_skip_threshold=1.0))
        for n in range(16):
            got = tok[n, : int(cnt[n])].tolist()
            full = -C.ref_nll(logp[n], got)
            assert abs(float(sc[n]) - full) < 2e-3 * max(1.0, abs(full)), (T, n)
            cands = [[]] + [[a] for a in (1, 2)] + [[a, b] for a in (1, 2) for b in (1, 2)] + [[1, 2, 1], [2, 1, 2]]
            best = max(-C.ref_nll(logp[n], c) for c in cands)
            assert full >= best - 5e-3, (T, n, got)


def test_ctc_beam_edges():
    g = torch.Generator().manual_seed(11)
    # T' = 1
    check_beam("T1", torch.log_softmax(torch.randn(8, 1, 32, generator=g) * 3, -1), 10)
    # every frame above the skip threshold: empty result, count 0, the oracle's score
    x = torch.randn(4, 20, 32, generator=g)
    x[:, :, 0] += 12.0
    logp = torch.log_softmax(x, -1)
    assert (logp[:, :, 0] > math.log(0.95)).all()
    tok, cnt, sc = (t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=10))
    assert (cnt == 0).all()
    check_beam("all frames skipped", logp, 10)
    # fewer candidates than beams: V = 2 and V = 3 with beam 16 (the live beam count grows 1, 2, ...)
    check_beam("V2", torch.log_softmax(torch.randn(8, 12, 2, generator=g) * 2, -1), 16)
    check_beam("V3", torch.log_softmax(torch.randn(8, 12, 3, generator=g) * 2, -1), 16)
    # V = 255; blank = V - 1; beam 1
    check_beam("V255", C.beam_logp(4, 30, 255, 4.0), 10)
    check_beam("blank V-1", C.beam_logp(8, 40, 32, 4.0, blank=31), 10, blank=31)
    check_beam("beam 1", C.beam_logp(8, 40, 32, 6.0), 1)
    # rows with -inf entries (a masked vocabulary)
    x = torch.randn(8, 30, 32, generator=g) * 3
    x[:, :, 5:20] = -math.inf
    x[:, ::3, 0] += 8.0
    check_beam("masked vocabulary", torch.log_softmax(x, -1), 10)


def test_ctc_beam_full_batch():
    """One launch of 6 x 64 sequences at the benchmark geometry (T' = 256, V = 256, beam 10; near-uniform to peaky): 16 sampled
    sequences equal the oracle; EVERY sequence is bit-identical (tokens, count, score) in a second run of the launch and in
    launches of subsets (no cross-talk through the per-sequence workspace)."""
    logp = C.big_batch_logp()
    dev = logp.cuda()
    tok, cnt, sc = (t.cpu() for t in ctc_beam_decode(dev, beam_size=10))
    tok2, cnt2, sc2 = (t.cpu() for t in ctc_beam_decode(dev, beam_size=10))
    assert torch.equal(cnt, cnt2) and torch.equal(sc, sc2)
    idx = torch.arange(256).view(1, -1) < cnt.view(-1, 1)
    assert torch.equal(tok[idx], tok2[idx])
    for sub in (torch.arange(0, 384, 3), torch.arange(1, 384, 3), torch.arange(2, 384, 3).flip(0)):
        t3, c3, s3 = (t.cpu() for t in ctc_beam_decode(dev[sub].contiguous(), beam_size=10))
        assert torch.equal(c3, cnt[sub]) and torch.equal(s3, sc[sub])
        assert torch.equal(t3[idx[sub]], tok[sub][idx[sub]])
    checked = 0
    for n in C.BIG_SAMPLE:
        want, wscore, final = ctc_prefix_beam_search(logp[n].double().numpy(), beam=10, return_beams=True)
        assert abs(float(sc[n]) - wscore) < 2e-3 * max(1.0, abs(wscore)), (n, float(sc[n]), wscore)
        if C.safe_margin(final):
            assert tok[n, : int(cnt[n])].tolist() == want, n
            checked += 1
    assert checked >= 12, checked
