"""The two step-wise AED decoders against an fp64 oracle at their edges (cases, driver and oracle: tests/aed_step_cases.py; what
this rests on: tests/test_host_aed_step.py).  The device runs every step of a case; the oracle -- the reference's own modules in
float64 on the whole prefixes, last position -- is evaluated at the case's check steps.

Bounds: the per-utterance decoder (csrc/decoder_step.hip, plain fp32) is held to the project's bound for it,
2e-5 * max(10, max |logp|); the batched decoder (csrc/decoder_batch.hip, f16x3 MFMA linears) to twice that, the ceiling the suite
implies through test_gpu_aed_batch.py (batched against per-utterance) chained with test_gpu_parity.py (per-utterance against the
reference).  Both are derived from the project, not from what the kernels give.

Measured on an MI355X, worst error / asserted bound over the check steps (every |logp| < 10, so the bounds are 2e-4 and 4e-4):
  per-utterance   P1 0.050   P2 0.009   P3 (1 / 3 / 6 sessions, worst exit) 0.010 / 0.010 / 0.011   P4 0.020   P5 0.029
  batched         B1 0.036   B2 (Tq 255 / 256 / 257 / 513) 0.005 / 0.005 / 0.005 / 0.005   B3 0.012   B4 0.013   B5 0.018
The batched worst, 0.036 of its doubled bound, is 0.07 of the single bound: on these inputs the batched decoder is below half
of the per-utterance bound, and the factor two is headroom, not need.  The asserted bound stays the derived one.
  weight domain W (per-utterance / batched / whole prefix), e = 0: 0.028 / 0.014 / 0.197   e = 4: 0.028 / 0.017 / 0.197
                                                            e = 8: 0.028 / 0.112 / 0.197
  Before batch_linear_kernel scaled its weight fragments by 2^8 the batched column read 0.017 / 0.077 / 1.301: the lo halves of
  small weights fell into fp16's subnormals (which the device keeps, hence the gradual loss).  The fp32 step decoder and the
  bf16x3 whole-prefix path do not move with e, to every printed digit.
Two deliberately wrong kernels, built aside and never committed, each failed here and passed every earlier AED test
(test_gpu_aed_batch.py and the decoder tests of test_gpu_parity.py): the self-attention P.V loops skipping their last key when
nk > 256 (P1 at 97, B1 at 40 times the bound), and load8 dropping its second half when K % 8 == 4 (B1 at 5500 times the bound).
"""
import copy
import functools

import pytest
import torch

import aed_step_cases as A

pytestmark = pytest.mark.gpu


def _open(fc, case, mem, kind):
    """The sessions that serve ``case`` on memory ``mem`` [E, B, Tq, D] (on the device): one batch session, or one session (group)
    per utterance."""
    E, B = case.EB
    exits = list(range(1, E + 1))
    if kind == "batch":
        sess = [fc.decoder_batch_session(mem, exits, case.steps)]
    elif case.lead == ():
        sess = [fc.decoder_session(mem[0, 0], 1, case.steps)]
    else:
        sess = [fc.decoder_session_group([mem[e, b:b + 1] for e in range(E)], exits, case.steps) for b in range(B)]
    assert all(s is not None for s in sess), "the geometry must be served by the step-wise decoder"
    return sess


def _step(sess, case, kind, tok, parent):
    """One step of every search -> log-probs [E, B, R, V]; tok, parent [E, B, R] on the device."""
    if kind == "batch":
        return sess[0].step(tok, parent)
    if case.lead == ():
        return sess[0].step(tok[0, 0], None if parent is None else parent[0, 0])[None, None]
    return torch.stack([s.step(tok[:, b], None if parent is None else parent[:, b]) for b, s in enumerate(sess)], dim=1)


def _run(fc, case, kind, whole_prefix=False):
    """Every step of ``case`` on the device; {check step: log-probs [E, B, R, V] on the host}.  With ``whole_prefix`` also what
    ``_decoder_`` gives on the whole prefixes, last position, at the check steps."""
    E, B = case.EB
    mem = A.memory(case).cuda()
    sess = _open(fc, case, mem, kind)
    got, whole = {}, {}
    for s, tok, parent, prefixes in A.drive(case):
        R = tok.size(-1)
        out = _step(sess, case, kind, tok.reshape(E, B, R).cuda(), None if parent is None else parent.reshape(E, B, R).cuda())
        assert out.shape == (E, B, R, case.geo[3])
        if s in case.checks:
            got[s] = out.cpu()
            if whole_prefix:
                with torch.no_grad():
                    whole[s] = torch.stack([fc._decoder_(prefixes[e].reshape(B * R, s + 1).cuda(), mem[e].repeat_interleave(R, dim=0), e + 1)[:, -1]
                                            .reshape(B, R, -1) for e in range(E)]).cpu()
    return (got, whole) if whole_prefix else got


def _worst(case, got, batched):
    """Largest error / bound over the check steps, per exit; finiteness must agree with the oracle at every one."""
    want = A.oracle(case)
    assert sorted(got) == sorted(want) == sorted(case.checks)
    ratio = torch.zeros(case.EB[0])
    for s in case.checks:
        w, g = want[s], got[s].double()
        assert g.shape == w.shape
        assert torch.equal(torch.isfinite(g), torch.isfinite(w)), (case.id, s)
        ratio = torch.maximum(ratio, (g - w).abs().amax(dim=(1, 2, 3)).float() / A.bound(w, batched))
    return ratio


@pytest.mark.parametrize("cid", [c.id for c in A.PER_UTTERANCE])
def test_per_utterance_step_decoder_against_the_fp64_oracle(cid):
    """decoder_session / decoder_session_group; every exit of a group against its own oracle (own decoder weights, own memory)."""
    case = A.BY_ID[cid]
    fc = copy.deepcopy(A.build_model(case)).cuda()
    ratio = _worst(case, _run(fc, case, "groups"), batched=False)
    print(f"{cid}: worst error / bound per exit: {[round(r, 4) for r in ratio.tolist()]}")
    assert ratio.max().item() < 1.0, (cid, ratio.tolist())


@pytest.mark.parametrize("cid", [c.id for c in A.BATCHED])
def test_batched_step_decoder_against_the_fp64_oracle(cid):
    case = A.BY_ID[cid]
    fc = copy.deepcopy(A.build_model(case)).cuda()
    ratio = _worst(case, _run(fc, case, "batch"), batched=True)
    print(f"{cid}: worst error / bound per exit: {[round(r, 4) for r in ratio.tolist()]} (x 2 against the single bound)")
    assert ratio.max().item() < 1.0, (cid, ratio.tolist())


@functools.lru_cache(maxsize=None)
def _weight_domain(e):
    """Worst error / bound of the three inference paths on rescale(model, e), against the fp64 oracle of the UNSCALED model:
    (per-utterance sessions, batched session, ``_decoder_`` on whole prefixes)."""
    case = A.W_CASE
    fc = A.rescale(A.build_model(case), e).cuda()
    step = _worst(case, _run(fc, case, "groups"), batched=False).max().item()
    got, whole = _run(fc, case, "batch", whole_prefix=True)
    return step, _worst(case, got, batched=True).max().item(), _worst(case, whole, batched=False).max().item()


@pytest.mark.parametrize("e", A.W_EXPONENTS)
def test_weight_domain(e):
    """The decoder's function does not depend on e (test_rescaling_leaves_the_fp64_oracle_unchanged); only the magnitudes of the
    feed-forward and value weights and of the activations between them do: x 2^-e.  All three paths stay within their bounds
    (the whole-prefix path: that of test_hip_decoder_matches_the_reference_decoder_modules, 2e-5 * max(10, max |logp|))."""
    step, batch, whole = _weight_domain(e)
    print(f"W e = {e}: error / bound: per-utterance {step:.4f}, batched {batch:.4f} (x 2 against the single bound), whole prefix {whole:.4f}")
    assert step < 1.0 and batch < 1.0 and whole < 1.0, (e, step, batch, whole)


def test_weight_domain_leaves_the_fp32_step_decoder_where_it_was():
    """Plain fp32 is scale-free short of its range: the per-utterance decoder's error at e = 8 may not exceed its error at e = 0
    by more than a quarter of the bound."""
    assert _weight_domain(8)[0] <= _weight_domain(0)[0] + 0.25


def test_beam_select_refuses_a_half_precision_logp_before_any_launch():
    """eec_beam_select reads ``logp`` as fp32 through its address: an fp16 tensor (half the bytes) is refused by the binding as a
    Python exception, nothing is launched and the outputs stay untouched; with fp32 the launch equals the host path of the same
    function.  n = 1, R = 2, V = 4, one step."""
    import ctypes
    from early_exit_transformer_amd.decoding import beam_select
    logp = torch.tensor([[[-0.5, -2.0, -0.25, -3.0], [-1.0, -0.125, -4.0, -1.5]]])
    scores = torch.tensor([[0.0, -0.75]])
    old = torch.tensor([[[7, 0], [9, 0]]])
    want_new = torch.full_like(old, -1)
    want = beam_select(logp, scores, 1.0, 2, old, want_new, 1)  # CPU tensors: the host path
    new = torch.full_like(old, -1).cuda()
    with pytest.raises(ctypes.ArgumentError, match=r"argument 5: TypeError: expected a float tensor, got torch\.float16"):
        beam_select(logp.cuda().half(), scores.cuda(), 1.0, 2, old.cuda(), new, 1)
    torch.cuda.synchronize()
    assert (new.cpu() == -1).all()
    got = beam_select(logp.cuda(), scores.cuda(), 1.0, 2, old.cuda(), new, 1)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)
    assert want[2].tolist() == [[2, 0]] and want[1].tolist() == [[0, 0]] and torch.equal(new.cpu(), want_new)
