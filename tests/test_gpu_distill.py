"""GPU tests of the self-distillation loss between exits (csrc/distill.hip behind eec_exit_distill_forward / _backward;
ctc.exit_distill_losses, ctc.exit_training_losses) against the definition of include/eec.h in fp64 on the CPU
(distill_cases.ref_distill), whose own checks tests/test_host_distill.py runs without a GPU.

Bounds -- the project's own, from tests/test_gpu_ctc.py; none is taken from the kernels under test:
    loss      |err| <= max(2e-5 + 2e-5 |want|, 2 err32)
    gradient  |err| <= max(1e-5 max|grad| + 1e-9, 2 gerr32)
err32 / gerr32: the CPU fp32 evaluation's own error against fp64 on the same input (at most 0.014 / 0.025 of the first terms on the
cases of distill_cases.cases(): the first terms decide).
"""
import ctypes as C

import pytest
import torch

import ctc_cases as CC
import distill_cases as D
from conftest import base_kwargs
from early_exit_transformer_amd import capi, synth
from early_exit_transformer_amd.model import encoder_lengths, exit_ctc_losses, exit_distill_losses, exit_training_losses
from oracle import conformer_ref as R

pytestmark = pytest.mark.gpu

MAX_EXITS = 16


def hip_losses(x, fl, teacher, tau):
    """The no-grad path (the forward entry alone)."""
    with torch.no_grad():
        return exit_distill_losses(x.cuda(), fl, teacher, tau).cpu().double()


def hip_loss_and_grad(x, fl, teacher, tau, w=None):
    """The autograd pair (eec_exit_distill_forward / _backward)."""
    xg = x.detach().clone().cuda().requires_grad_(True)
    losses = exit_distill_losses(xg, fl, teacher, tau)
    ww = torch.ones_like(losses) if w is None else w.to(losses)
    (losses * ww).sum().backward()
    return losses.detach().cpu().double(), xg.grad.cpu().double()


def check_against_fp64(tag, x, fl, teacher, tau, w=None, ref=None):
    """Both paths against the fp64 definition with the module's bounds; returns (losses, gradient) of the autograd path."""
    x = x.float()
    if ref is None:
        ref = D.ref_distill(x, fl, teacher, tau, torch.float64, w), D.ref_distill(x, fl, teacher, tau, torch.float32, w)
    (want, gw), (want32, g32) = ref
    lerr32 = (want32.double() - want).abs()
    bound = D.loss_bound(want, lerr32)
    got0 = hip_losses(x, fl, teacher, tau)
    got1, g = hip_loss_and_grad(x, fl, teacher, tau, w)
    lerr0, lerr1 = (got0 - want).abs(), (got1 - want).abs()
    scale = gw.abs().max().item()
    gerr, gerr32 = (g - gw).abs().max().item(), (g32.double() - gw).abs().max().item()
    print(f"\n[distill {tag}] loss {want.max().item():.5f}: HIP err {lerr0.max().item():.2e} (no-grad) {lerr1.max().item():.2e} (autograd), "
          f"fp32 statement err {lerr32.max().item():.2e}; max|grad| {scale:.3e}: HIP err {gerr:.2e}, fp32 statement err {gerr32:.2e}")
    assert torch.isfinite(got0).all() and (lerr0 <= bound).all(), (tag, got0.tolist(), want.tolist(), lerr32.tolist())
    assert torch.isfinite(got1).all() and (lerr1 <= bound).all(), (tag, got1.tolist(), want.tolist(), lerr32.tolist())
    assert torch.equal(got0, got1), tag  # one forward entry behind both paths
    assert torch.isfinite(g).all(), tag
    assert gerr <= D.grad_bound(scale, gerr32), (tag, gerr, gerr32, scale)
    return got1, g


def rand_x(E, B, T, V, seed=0, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, B, T, V, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against fp64 on the shared cases
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in D.cases()])
def test_distill_matches_fp64_on_peaky_and_trained_like_rows(name):
    """Peaky log-probs (logit scales 1, 8, 16; [3, 3, 19, 256]) and the committed trained-like fixture ([6, 4, 16, 256]) at
    tau = 0.5, 1, 2 with frame lengths cycling [T, 1, 7, 0]: both paths, unweighted (the shared reference) and with per-exit weights.
    Measured on MI355X, over this module's comparisons: the loss errs by at most 0.014 of 2e-5 + 2e-5 |want| (4.7e-6 at a loss of 37),
    the gradient by at most 0.036 of 1e-5 max|grad| + 1e-9 (7.8e-8 at max|grad| 0.77) -- about the fp32 statement's own errors; the first
    terms of the bounds hold everywhere, 2 * err32 is not needed."""
    (_, x, fl, teacher, tau), r64, r32 = D.reference(name)
    check_against_fp64(name, x, fl, teacher, tau, ref=(r64, r32))
    check_against_fp64(name + " weighted", x, fl, teacher, tau, w=torch.linspace(0.5, 1.5, x.size(0)))


def test_distill_wrapper_normalises_fp64_and_non_contiguous_inputs():
    """A float64 tensor and a transposed view: the wrapper hands the kernels contiguous fp32, the gradient comes back in the
    caller's dtype and layout."""
    x = D.inputs()["scale8"]
    fl = D.cycle_lens(3, 19)
    (want, gw), _ = D.ref_distill(x, fl, "last", 2.0), None
    x64 = x.double().cuda().requires_grad_(True)
    exit_distill_losses(x64, fl, "last", 2.0).sum().backward()
    assert x64.grad.dtype == torch.float64
    assert (x64.grad.cpu() - gw).abs().max().item() <= 1e-5 * gw.abs().max().item() + 1e-9
    base = x.permute(0, 2, 1, 3).contiguous().cuda().requires_grad_(True)  # [E, T, B, V]
    view = base.permute(0, 2, 1, 3)
    assert not view.is_contiguous()
    losses = exit_distill_losses(view, fl, "last", 2.0)
    losses.sum().backward()
    assert ((losses.detach().cpu().double() - want).abs() <= 2e-5 + 2e-5 * want.abs()).all()
    assert (base.grad.permute(0, 2, 1, 3).cpu().double() - gw).abs().max().item() <= 1e-5 * gw.abs().max().item() + 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# 2. shapes where the kernels can go wrong
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4, 32, 252, 256])
def test_distill_vocabulary_sizes(V):
    """A row is one float4 per lane under c0 < V: one lane, half a wave's rows of 16 bytes, the last multiple of 4, a full wave."""
    check_against_fp64(f"V{V}", rand_x(3, 3, 9, V, seed=V), torch.tensor([9, 4, 0]), "last", 2.0, w=torch.linspace(0.5, 1.5, 3))


@pytest.mark.parametrize("B,T", [(3, 1), (1, 7), (3, 19), (5, 64), (2, 65), (17, 3)])
def test_distill_frame_and_batch_counts(B, T):
    """T = 1; B = 1; B * T no multiple of the four waves of a workgroup (3 x 19 = 57); the reduction's 64-frame loads exactly
    filled and with one frame over; more utterances than the reduction's 16 waves."""
    fl = torch.tensor([(T, 1, 7, 0)[b % 4] for b in range(B)]).clamp(max=T)
    check_against_fp64(f"B{B} T{T}", rand_x(3, B, T, 32, seed=B * 100 + T), fl, "last", 1.0)
    check_against_fp64(f"B{B} T{T} no lengths", rand_x(3, B, T, 32, seed=B * 100 + T), None, "next", 0.5)


@pytest.mark.parametrize("E", [2, 4, 5, 6, 8, 9, MAX_EXITS])
def test_distill_exit_counts(E):
    """E = 2, 6 and the maximum, and both sides of the kernels' register layouts (4 | 5, 8 | 9 exits), with "last", "next" and a
    map that mixes shallower teachers, chains and exits that are no students."""
    x = rand_x(E, 2, 5, 32, seed=E)
    fl = torch.tensor([5, 3])
    w = torch.linspace(0.5, 1.5, E)
    check_against_fp64(f"E{E} last", x, fl, "last", 2.0, w=w)
    check_against_fp64(f"E{E} next", x, fl, "next", 1.0, w=w)
    mixed = [(e + 2) % E if e % 3 else -1 for e in range(E)]
    mixed = [-1 if k == e else k for e, k in enumerate(mixed)]
    if E > 2:
        mixed[E - 1] = 0  # the deepest exit learns from the shallowest
    check_against_fp64(f"E{E} {mixed}", x, fl, mixed, 0.5, w=w)


def test_distill_more_exits_than_the_maximum_is_refused():
    x = rand_x(MAX_EXITS + 1, 1, 2, 8).cuda()
    with pytest.raises(RuntimeError, match=f"at most {MAX_EXITS} exits"):
        exit_distill_losses(x)
    with pytest.raises(RuntimeError, match=f"at most {MAX_EXITS} exits"):
        exit_distill_losses(x.requires_grad_(True))
    with pytest.raises(ValueError, match="multiple of 4"):
        exit_distill_losses(rand_x(2, 1, 2, 30).cuda())
    with pytest.raises(RuntimeError, match="own teacher"):
        exit_distill_losses(rand_x(3, 1, 2, 8).cuda(), teacher=[1, 1, -1])
    with pytest.raises(RuntimeError, match="temperature"):
        exit_distill_losses(rand_x(3, 1, 2, 8).cuda(), temperature=0.0)


@pytest.mark.parametrize("teacher", ["last", "next", [-1, -1, -1], [2, 0, -1], [1, 2, -1]], ids=str)
def test_distill_teacher_maps(teacher):
    """The named maps, no student at all (all zeros out), a teacher shallower than its student, and a chain (exit 1 is a student of
    2 and the teacher of 0)."""
    x = D.inputs()["scale8"]
    losses, g = check_against_fp64(f"teacher {teacher}", x, D.cycle_lens(3, 19), teacher, 2.0, w=torch.tensor([1.5, 0.5, 1.0]))
    if teacher == [-1, -1, -1]:
        assert (losses == 0).all() and (g == 0).all()


def test_distill_frame_lengths_zero_full_and_above_T():
    """Lengths of 0, of T, above T (clamped to T) and below 0 (clamped to 0), as int32 on the device and as int64 on the host."""
    x = rand_x(3, 4, 6, 32, seed=7)
    fl = torch.tensor([0, 6, 9, -3])
    l_a, g_a = check_against_fp64("lengths [0, T, T + 3, -3]", x, fl, "last", 1.0)
    l_b, g_b = check_against_fp64("lengths [0, T, T, 0] int32 on the device", x, torch.tensor([0, 6, 6, 0], dtype=torch.int32).cuda(), "last", 1.0)
    assert torch.equal(l_a, l_b) and torch.equal(g_a, g_b)
    assert (g_a[:, 0] == 0).all() and (g_a[:, 3] == 0).all()
    l_c, _ = check_against_fp64("all lengths 0", x, torch.zeros(4, dtype=torch.int64), "last", 1.0)
    assert (l_c == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. structure of the gradient
# ---------------------------------------------------------------------------------------------------------------------------
def test_distill_gradient_structure():
    """Exactly 0 on masked frames, on every row of an exit that is nobody's student and on teacher-only exits; every frame's
    gradient sums to 0 over the classes within the CTC test's 1e-5 * max|grad| * V."""
    x = D.inputs()["fixture"]  # [6, 4, 16, 256]
    E, B, T, V = x.shape
    fl = D.cycle_lens(B, T)
    teacher = [5, -1, 5, 0, -1, -1]  # exit 5: teacher only; 1, 4: neither; 0: a student and a teacher
    _, g = hip_loss_and_grad(x, fl, teacher, 2.0, w=torch.linspace(0.5, 1.5, E))
    mask, _ = D.frame_mask(fl, B, T)
    assert (g[:, ~mask] == 0).all()
    for e in (1, 4, 5):
        assert (g[e] == 0).all(), e
    for e in (0, 2, 3):
        assert (g[e][mask] != 0).any(), e
    scale = g.abs().max().item()
    assert scale > 0 and g.sum(-1).abs().max().item() < 1e-5 * scale * V


@pytest.mark.parametrize("name", ["scale1", "scale16", "fixture"])
def test_distill_is_invariant_under_a_per_row_shift(name):
    """Every row is normalised inside: adding a constant per row (randn * 4; the sum rounds every logit anew) changes the losses by
    no more than the loss bound, and the shifted losses are within it of their own fp64 reference."""
    x = D.inputs()[name]
    E, B, T, _ = x.shape
    fl = D.cycle_lens(B, T)
    g = torch.Generator().manual_seed(3)
    shifted = x + torch.randn(E, B, T, 1, generator=g) * 4
    want, _ = D.ref_distill(x, fl, "last", 1.0)
    want32, _ = D.ref_distill(x, fl, "last", 1.0, torch.float32)
    bound = D.loss_bound(want, (want32.double() - want).abs())
    got, got_s = hip_losses(x, fl, "last", 1.0), hip_losses(shifted, fl, "last", 1.0)
    print(f"\n[distill shift {name}] losses change by {(got - got_s).abs().max().item():.2e} (bound {bound.min().item():.2e})")
    assert ((got - got_s).abs() <= bound).all()
    check_against_fp64(f"{name} shifted", shifted, fl, "last", 1.0)


def test_distill_nan_rows_reach_the_exits_that_read_them_only():
    """A NaN logit in exit 1 (a student of 2, the teacher of 0): losses 0 and 1 are NaN, loss 3 (a student of 2) is not, and
    the gradient is NaN on that frame's rows of exits 0 and 1 only.  A NaN on a masked frame is not read."""
    x = rand_x(4, 2, 5, 32, seed=11)
    x[1, 0, 2, 7] = float("nan")
    x[2, 1, 4, 0] = float("nan")  # utterance 1 has 3 frames: masked
    fl = torch.tensor([5, 3])
    losses, g = hip_loss_and_grad(x, fl, [1, 2, -1, 2], 1.0)
    assert torch.isnan(losses[:2]).all() and torch.isfinite(losses[2:]).all()
    bad = torch.isnan(g)
    assert bad[0, 0, 2].all() and bad[1, 0, 2].all()
    bad[0, 0, 2] = bad[1, 0, 2] = False
    assert not bad.any()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. accumulate = 1
# ---------------------------------------------------------------------------------------------------------------------------
def test_distill_backward_accumulates_into_a_filled_buffer():
    """accumulate = 1 adds the gradient into a pre-filled buffer -- the sum a + g in fp32, bit for bit -- and leaves the rows it does
    not own (exits without a teacher, exits with a zero weight, masked frames) untouched; accumulate = 0 writes zeros there."""
    x = D.inputs()["fixture"].cuda()
    E, B, T, V = x.shape
    fl = D.cycle_lens(B, T)
    fl_dev = fl.to(torch.int32).cuda()
    teacher = [5, -1, 5, 0, 3, -1]
    w = torch.tensor([0.5, 1.0, 1.5, 2.0, 0.0, 1.0]).cuda()  # exit 4 is a student with a zero weight
    lib = capi.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tarr = (C.c_int32 * E)(*teacher)

    def backward(accumulate, dx):
        capi.check(lib.eec_exit_distill_backward(x.data_ptr(), fl_dev.data_ptr(), tarr, E, B, T, V, 2.0, w.data_ptr(), accumulate,
                                                 dx.data_ptr(), st), "eec_exit_distill_backward")
        return dx

    g = backward(0, torch.full_like(x, float("nan")))
    _, gw = D.ref_distill(x.cpu(), fl, teacher, 2.0, w=w.cpu())
    assert (g.cpu().double() - gw).abs().max().item() <= 1e-5 * gw.abs().max().item() + 1e-9
    fill = torch.randn(x.shape, generator=torch.Generator().manual_seed(1)).cuda()
    acc = backward(1, fill.clone())
    assert torch.equal(acc, fill + g)
    mask, _ = D.frame_mask(fl, B, T)
    assert torch.equal(acc[:, ~mask.cuda()], fill[:, ~mask.cuda()])
    for e in (1, 4, 5):
        assert torch.equal(acc[e], fill[e]) and (g[e] == 0).all(), e
    # rows it does not own may hold anything: a NaN there is neither read nor written
    fill[1] = float("nan")
    acc = backward(1, fill.clone())
    assert torch.isnan(acc[1]).all() and torch.isfinite(acc[0]).all() and torch.isfinite(acc[2:]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. exit_training_losses
# ---------------------------------------------------------------------------------------------------------------------------
def training_inputs():
    x = D.inputs()["fixture"]  # log-probs [6, 4, 16, 256]
    tgt, tl = synth.synth_targets(4, 5, 256, seed=9)
    return x, tgt, tl, D.cycle_lens(4, 16)


def test_exit_training_losses_are_the_two_losses_bit_for_bit():
    x, tgt, tl, fl = training_inputs()
    with torch.no_grad():
        ctc, kd = exit_training_losses(x.cuda(), tgt, tl, fl, "last", 2.0)
        assert torch.equal(ctc, exit_ctc_losses(x.cuda(), tgt, tl)) and torch.equal(kd, exit_distill_losses(x.cuda(), fl, "last", 2.0))
    xg = x.cuda().requires_grad_(True)
    ctc, kd = exit_training_losses(xg, tgt, tl, fl, "last", 2.0)
    assert ctc.requires_grad and kd.requires_grad
    assert torch.equal(ctc.detach(), exit_ctc_losses(xg, tgt, tl).detach())
    assert torch.equal(kd.detach(), exit_distill_losses(xg, fl, "last", 2.0).detach())
    want_ctc, _ = CC.ref_ctc(x, tgt, tl)
    want_kd, _ = D.ref_distill(x, fl, "last", 2.0)
    assert torch.allclose(ctc.detach().cpu().double(), want_ctc, rtol=2e-5, atol=2e-5)
    assert ((kd.detach().cpu().double() - want_kd).abs() <= 2e-5 + 2e-5 * want_kd.abs()).all()


def test_exit_training_losses_gradient_is_the_sum_of_the_two_gradients():
    """One node, one gradient buffer: within 1e-6 * max|grad| of the sum of the two separate autograd gradients; with weight 0 on
    the distillation term bit-identical to the CTC gradient alone; each output alone gives its own loss's gradient bit for bit."""
    x, tgt, tl, fl = training_inputs()

    def grad_of(loss_fn):
        xg = x.cuda().requires_grad_(True)
        loss_fn(xg).backward()
        return xg.grad

    g_ctc = grad_of(lambda xg: exit_ctc_losses(xg, tgt, tl).sum())
    g_kd = grad_of(lambda xg: 0.5 * exit_distill_losses(xg, fl, "last", 2.0).sum())
    both = grad_of(lambda xg: (lambda ctc, kd: ctc.sum() + 0.5 * kd.sum())(*exit_training_losses(xg, tgt, tl, fl, "last", 2.0)))
    sep = g_ctc + g_kd
    err, scale = (both - sep).abs().max().item(), sep.abs().max().item()
    print(f"\n[distill training] one node vs the sum of the two gradients: {err:.2e} of max|grad| {scale:.3e}")
    assert err <= 1e-6 * scale
    zero = grad_of(lambda xg: (lambda ctc, kd: ctc.sum() + 0.0 * kd.sum())(*exit_training_losses(xg, tgt, tl, fl, "last", 2.0)))
    assert torch.equal(zero, g_ctc) and torch.equal(zero.view(torch.int32), g_ctc.view(torch.int32))
    only_ctc = grad_of(lambda xg: exit_training_losses(xg, tgt, tl, fl, "last", 2.0)[0].sum())
    assert torch.equal(only_ctc.view(torch.int32), g_ctc.view(torch.int32))
    only_kd = grad_of(lambda xg: 0.5 * exit_training_losses(xg, tgt, tl, fl, "last", 2.0)[1].sum())
    assert torch.equal(only_kd, g_kd)
    # the whole gradient against fp64
    _, gw_ctc = CC.ref_ctc(x, tgt, tl)
    _, gw_kd = D.ref_distill(x, fl, "last", 2.0, w=torch.full((6,), 0.5))
    gw = gw_ctc + gw_kd
    assert (both.cpu().double() - gw).abs().max().item() <= 1e-5 * gw.abs().max().item() + 1e-9
    xg = x.cuda().requires_grad_(True)
    ctc, kd = exit_training_losses(xg, tgt, tl, fl, "last", 2.0)
    loss = ctc.sum() + kd.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        loss.backward()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the benchmark geometry
# ---------------------------------------------------------------------------------------------------------------------------
def test_distill_benchmark_geometry_is_finite_and_reproducible():
    """[6, 64, 256, 256] with ragged lengths: finite losses and gradient, bit-identical in a second run (no atomics anywhere); three
    sampled utterances against fp64."""
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.log_softmax(torch.randn(6, 64, 256, 256, generator=g, device="cuda") * 3.0, -1)
    fl = (256 - (torch.arange(64) * 37) % 200).to(torch.int32).cuda()
    w = torch.linspace(0.5, 1.5, 6).cuda()

    def run():
        xg = x.detach().requires_grad_(True)
        losses = exit_distill_losses(xg, fl, "last", 2.0)
        (losses * w).sum().backward()
        return losses.detach(), xg.grad

    l1, g1 = run()
    l2, g2 = run()
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and (l1[:5] > 0).all() and l1[5] == 0
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    # utterances 0, 31, 63 as one-utterance batches against fp64: their gradient rows are the batch's times B
    for b in (0, 31, 63):
        xb, flb = x[:, b:b + 1].cpu(), fl[b:b + 1].cpu()
        _, gw = D.ref_distill(xb, flb, "last", 2.0, w=w.cpu())
        got = g1[:, b:b + 1].cpu().double() * 64
        assert (got - gw).abs().max().item() <= 1e-5 * gw.abs().max().item() + 1e-9, b


# ---------------------------------------------------------------------------------------------------------------------------
# 7. through the Module
# ---------------------------------------------------------------------------------------------------------------------------
def test_distill_training_step_through_the_module_matches_oracle_autograd():
    """Early_conformer (2 exits x 1 layer, dropout 0, train mode), B = 2, T = 67 (T' = 16), ragged lengths: every parameter's gradient
    of ctc.sum() + 0.5 * kd.sum() against the same loss on the float64 oracle encoder's autograd, at the training-step test's bound
    (test_gpu_train.compare_grads, 2e-3 of each gradient's largest entry for the bf16x3 GEMMs)."""
    from test_gpu_train import compare_grads, grads_of, make_train_pair64
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=1)
    ref, gpu = make_train_pair64(kw, seed=23)
    mel, lens = synth.synth_mel(2, 80, 67, seed=23), torch.tensor([67, 41])
    tgt, tl = synth.synth_targets(2, 4, kw["dec_voc_size"], seed=23)
    want_out = ref(mel.double(), lens)
    Tq = want_out.size(2)
    fl = torch.clamp(lens // 4, max=Tq)
    want_kd = D.torch_distill(want_out, fl, "last", 2.0)
    want_loss = R.summed_exit_ctc_loss(want_out, tgt, tl) + 0.5 * want_kd.sum()
    want_loss.backward()
    out = gpu(mel.cuda(), lens)
    assert out.requires_grad and out.shape == want_out.shape
    fl_dev = encoder_lengths(lens.cuda(), Tq)
    assert fl_dev.cpu().tolist() == fl.tolist() and fl.tolist() == [16, 10]
    ctc, kd = exit_training_losses(out, tgt, tl, fl_dev, "last", 2.0)
    loss = ctc.sum() + 0.5 * kd.sum()
    print(f"\n[distill module] loss {loss.item():.6f} vs the fp64 oracle {want_loss.item():.6f}; kd {kd.tolist()} vs {want_kd.tolist()}")
    assert abs(loss.item() - want_loss.item()) < 2e-4 * max(1.0, abs(want_loss.item()))
    assert kd[0].item() > 0 and kd[1].item() == 0
    loss.backward()
    compare_grads(grads_of(gpu), grads_of(ref), 2e-3, "distill, bf16x3", oracle64=True)
