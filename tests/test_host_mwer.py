"""CPU tests of MWER training of the CTC exits (include/eec.h, "Minimum word error rate training"; csrc/ctc_mwer.hip): the fp64
restatement of tests/mwer_cases.py against torch's own CTC loss, against a brute force over every path and against finite
differences; the properties the statement promises (exact zeros, coefficients that add up to 0); the CPU host path of the Python
wrappers; and the host side of the entries: declared, exported, bad arguments refused before anything is launched (no device)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mwer_cases as M
from conftest import ROOT
from early_exit_transformer_amd import capi, ctc
from early_exit_transformer_amd.build import LIB_PATH

ENTRIES = ("eec_ctc_mwer_workspace_bytes", "eec_ctc_hyp_logp", "eec_ctc_mwer_forward", "eec_ctc_mwer_backward")
BAD_ARG, WORKSPACE = 10001, 10003


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def torch_ll(logp, il, hyp, hyp_len, blank=0):
    """ll [E, B, N] fp64 with grad: -F.ctc_loss(reduction='none', zero_infinity=False) per lattice (None where the entry is
    absent or has no frames: torch's loss does not take an empty input)."""
    E, B, T, V = logp.shape
    out = {}
    for e, b, i in itertools.product(range(E), range(B), range(hyp.size(2))):
        n, Tb = int(hyp_len[e, b, i]), int(min(max(int(il[b]), 0), T))
        if n < 0 or Tb == 0:
            continue
        tg = hyp[e, b, i, :n].long().view(1, n)
        out[e, b, i] = -F.ctc_loss(logp[e, b, :Tb].unsqueeze(1), tg, torch.tensor([Tb]), torch.tensor([n]), blank=blank, reduction="none",
                                   zero_infinity=False)[0]
    return out


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_restatement_ll_is_torchs_ctc_loss(name):
    """The restatement's ll equals -F.ctc_loss(fp64, reduction='none', zero_infinity=False) within 1e-10 relative; -inf where
    torch says +inf; the cases hold every kind of entry."""
    (x, il, hyp, hl, risk), want, _ = M.reference(name)
    ref = torch_ll(x.double(), il, hyp, hl)
    worst = 0.0
    for (e, b, i), v in ref.items():
        got = want["ll"][e, b, i]
        if torch.isinf(v):
            assert got == -np.inf, (e, b, i)
        else:
            worst = max(worst, abs(got - v.item()) / max(1.0, abs(v.item())))
    print(f"\n[mwer {name}] restatement ll vs torch: {worst:.2e} relative")
    assert worst <= 1e-10
    kinds = {"absent": (hl == -1).any().item(), "infeasible": bool(((hl >= 0).numpy() & (want["ll"] == -np.inf)).any()),
             "empty": (hl == 0).any().item(), "finite": bool(np.isfinite(want["ll"]).any())}
    assert all(kinds.values()), kinds


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_restatement_gradient_is_autograd_through_softmax_over_torchs_ll(name):
    """sum_i c_i gamma_i equals what torch autograd returns for mean_b sum_i softmax(ll)_i (risk_i - k) through F.ctc_loss, within
    1e-9 of max|grad|, with per-exit weights.  The gradient does not depend on the constant k (the softmax adds up to 1); k is the
    likeliest entry's risk, not the mean: on the peaky cases one entry holds all but 1e-9 of the mass, the whole gradient is of
    that size, and with k = mean risk autograd's own softmax backward p (g - sum p g) cancels to an absolute error of 1e-16 --
    more than 1e-9 of such a gradient."""
    (x, il, hyp, hl, risk), want, _ = M.reference(name, weighted=True)
    xx = x.double().requires_grad_(True)
    ref = torch_ll(xx, il, hyp, hl)
    E, B, N = hl.shape
    w = M.exit_weights(E)
    total = xx.new_zeros(())
    for e, b in itertools.product(range(E), range(B)):
        idx = [i for i in range(N) if (e, b, i) in ref and torch.isfinite(ref[e, b, i])]
        if not idx:
            continue
        ll = torch.stack([ref[e, b, i] for i in idx])
        r = risk[e, b, idx].double()
        total = total + w[e] * (torch.softmax(ll, 0) * (r - r[ll.argmax()])).sum() / B
    total.backward()
    scale = xx.grad.abs().max().item()
    err = np.abs(want["grad"] - xx.grad.numpy()).max()
    print(f"\n[mwer {name}] restatement gradient vs autograd: {err:.2e} of max|grad| {scale:.3e}")
    assert scale > 0 and err <= 1e-9 * scale


def test_brute_force_over_all_paths_pins_ll_and_gamma():
    """V = 3, T = 5: ll and gamma from the 243 paths, for hypotheses with and without a repeat, the empty one and an infeasible one."""
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(5, 3, generator=g, dtype=torch.float64), -1).numpy()
    for tokens in ([], [1], [1, 2], [2, 2], [1, 2, 1], [1, 1, 1], [2, 2, 2, 2]):
        p_total, gam = 0.0, np.zeros((5, 3))
        for path in itertools.product(range(3), repeat=5):
            col = [v for k, v in enumerate(path) if v != 0 and (k == 0 or v != path[k - 1])]
            if col == tokens:
                p = np.exp(sum(lp[t, v] for t, v in enumerate(path)))
                p_total += p
                for t, v in enumerate(path):
                    gam[t, v] += p
        ll, gamma = M.lattice(lp, tokens)
        if p_total == 0:
            assert ll == -np.inf and gamma is None, tokens
            continue
        assert abs(ll - np.log(p_total)) <= 1e-12 * max(1.0, abs(ll)), tokens
        assert np.abs(gamma - gam / p_total).max() <= 1e-12, tokens
        assert np.abs(gamma.sum(1) - 1).max() <= 1e-12


def _small_case(seed=0, E=2, B=2, T=7, V=8, N=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(E, B, T, V, generator=g, dtype=torch.float64) * 2, -1)
    hyp = torch.randint(1, V, (E, B, N, 3), generator=g, dtype=torch.int32)
    hl = torch.randint(0, 4, (E, B, N), generator=g, dtype=torch.int32)
    risk = torch.randint(0, 5, (E, B, N), generator=g).float()
    return x, torch.tensor([T, T - 2][:B]), hyp, hl, risk


def test_equal_risks_and_single_entries_give_exact_zeros():
    x, il, hyp, hl, risk = _small_case()
    for dtype in (np.float64, np.float32):
        out = M.statement(x, il, hyp, hl, torch.full_like(risk, 0.1), dtype=dtype)
        assert (out["loss_eb"] == 0).all() and (out["c"] == 0).all() and (out["grad"] == 0).all()
        out = M.statement(x, il, hyp[:, :, :1], hl[:, :, :1], risk[:, :, :1], dtype=dtype)
        assert (out["loss_eb"] == 0).all() and (out["c"] == 0).all() and (out["grad"] == 0).all()
    for t in (x, x.float()):  # the host path promises the same
        assert (ctc.exit_mwer_losses(t, hyp, hl, torch.full_like(risk, 0.1), il) == 0).all()
        assert (ctc.exit_mwer_losses(t, hyp[:, :, :1], hl[:, :, :1], risk[:, :, :1], il) == 0).all()


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_coefficients_add_up_to_zero(name):
    _, want, _ = M.reference(name)
    assert np.abs(want["c"].sum(-1)).max() <= 1e-12
    assert np.isfinite(want["loss_eb"]).all() and np.abs(want["loss_eb"]).max() > 0


def test_finite_differences_of_the_statement():
    """Central differences of loss (fp64) along random directions against the stated gradient, on a case with ragged lengths."""
    x, il, hyp, hl, risk = _small_case(seed=4)
    w = M.exit_weights(x.size(0))
    out = M.statement(x, il, hyp, hl, risk, w=w)
    assert np.abs(out["grad"]).max() > 1e-3
    g = torch.Generator().manual_seed(9)
    f = lambda z: float((M.statement(z, il, hyp, hl, risk)["loss"] * w.numpy()).sum())  # noqa: E731
    for _ in range(4):
        d = torch.randn(x.shape, generator=g, dtype=torch.float64)
        h = 1e-6
        num = (f(x + h * d) - f(x - h * d)) / (2 * h)
        ana = float((out["grad"] * d.numpy()).sum())
        assert abs(num - ana) <= 1e-7 * max(1.0, abs(ana)), (num, ana)


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_host_path_of_the_wrappers_is_the_restatement(name):
    """ctc_hyp_logp and exit_mwer_losses on CPU fp64 tensors (torch's ctc_loss and autograd) against the restatement: ll, the
    losses and the weighted gradient."""
    (x, il, hyp, hl, risk), want, _ = M.reference(name, weighted=True)
    ll = ctc.ctc_hyp_logp(x.double(), hyp, hl, il).numpy()
    fin = np.isfinite(want["ll"])
    assert (ll[~fin] == want["ll"][~fin]).all()
    assert np.abs(ll[fin] - want["ll"][fin]).max() <= 1e-10 * np.abs(want["ll"][fin]).max()
    xx = x.double().requires_grad_(True)
    loss = ctc.exit_mwer_losses(xx, hyp, hl, risk, il)
    assert loss.dtype == torch.float64 and np.abs(loss.detach().numpy() - want["loss"]).max() <= 1e-10
    (loss * M.exit_weights(x.size(0))).sum().backward()
    scale = np.abs(want["grad"]).max()
    assert np.abs(xx.grad.numpy() - want["grad"]).max() <= 1e-9 * scale
    # fp32 input stays fp32 and sits inside the fp32 evaluation's own error, doubled
    l32 = ctc.exit_mwer_losses(x, hyp, hl, risk, il)
    assert l32.dtype == torch.float32 and np.abs(l32.double().numpy() - want["loss"]).max() <= 1e-3


def test_host_path_refuses_what_the_device_turns_into_nan():
    x, il, hyp, hl, risk = _small_case(seed=2)
    clean = ctc.exit_mwer_losses(x, hyp, hl, risk, il)
    for what in ("length", "label", "blank"):
        h2, l2 = hyp.clone(), hl.clone()
        l2[1, 0, 1] = 2
        if what == "length":
            l2[1, 0, 1] = 4
        elif what == "label":
            h2[1, 0, 1, 0] = x.size(3)
        else:
            h2[1, 0, 1, 1] = 0
        got = ctc.exit_mwer_losses(x, h2, l2, risk, il)
        assert torch.isnan(got[1]) and got[0] == clean[0], what
        assert torch.isnan(ctc.ctc_hyp_logp(x, h2, l2, il)[1, 0, 1])
        want = M.statement(x, il, h2, l2, risk)
        assert np.isnan(want["loss_eb"][1, 0]) and np.isfinite(want["loss_eb"][0]).all() and np.isnan(want["ll"][1, 0, 1])
    with pytest.raises(ValueError, match="1 to 16"):
        ctc.exit_mwer_losses(x, hyp.new_zeros((2, 2, 17, 3)), hl.new_zeros((2, 2, 17)), risk.new_zeros((2, 2, 17)))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc.mwer_nbest(x, hyp[0, :, 0], hl[0, :, 0])
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc.exit_mwer_training_losses(x, hyp[0, :, 0], hl[0, :, 0])
    from early_exit_transformer_amd import model
    assert model.exit_mwer_losses is ctc.exit_mwer_losses and model.mwer_nbest is ctc.mwer_nbest
    assert model.exit_mwer_training_losses is ctc.exit_mwer_training_losses and model.ctc_hyp_logp is ctc.ctc_hyp_logp


def test_entries_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/eec.h"
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert int(re.search(r"#define\s+EEC_MWER_MAX_NBEST\s+(\d+)", header).group(1)) == ctc.MWER_MAX_NBEST == 16
    assert lib.eec_abi_version() == 16


def _call(lib, which, E=2, B=3, b0=0, nb=None, T=5, V=32, N=4, L=6, blank=0, null=(), ws=0x1000, ws_bytes=None):
    """One call of an entry with made-up device addresses: every case here must be refused before anything is dereferenced or
    launched.  ``null``: names of the pointers passed as NULL."""
    fake = lambda name: None if name in null else C.c_void_p(0x1000)  # noqa: E731  (256-byte aligned, never read)
    nb = B if nb is None else nb
    nbytes = lib.eec_ctc_mwer_workspace_bytes(E, nb, T, N, L) if ws_bytes is None else ws_bytes
    wsp = None if "workspace" in null else C.c_void_p(ws)
    if which == "hyp_logp":
        return lib.eec_ctc_hyp_logp(fake("logp"), fake("input_len"), fake("hyp"), fake("hyp_len"), E, B, T, V, N, L, blank, fake("ll"), None)
    if which == "forward":
        return lib.eec_ctc_mwer_forward(fake("logp"), fake("input_len"), fake("hyp"), fake("hyp_len"), fake("risk"), E, B, b0, nb, T, V, N, L, blank,
                                        fake("ll"), fake("loss_eb"), fake("loss"), wsp, nbytes, None)
    return lib.eec_ctc_mwer_backward(fake("logp"), fake("input_len"), fake("hyp"), fake("hyp_len"), E, B, b0, nb, T, V, N, L, blank, wsp, nbytes,
                                     fake("grad_loss"), 0, fake("dlogp"), None)


BAD = [("N 0", dict(N=0), r"N must lie in \[1, EEC_MWER_MAX_NBEST = 16\]"), ("N 17", dict(N=17), r"N must lie in \[1, EEC_MWER_MAX_NBEST = 16\]"),
       ("E 0", dict(E=0), "positive"), ("B 0", dict(B=0), "positive"), ("T 0", dict(T=0), "positive"), ("V 0", dict(V=0), "positive"),
       ("L 0", dict(L=0), "positive"), ("blank V", dict(blank=32), r"blank must lie in \[0, V\)")]


@pytest.mark.parametrize("which", ["hyp_logp", "forward", "backward"])
@pytest.mark.parametrize("what,kw,msg", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_without_a_device(lib, which, what, kw, msg):
    assert _call(lib, which, **kw) == BAD_ARG, what
    assert re.search(msg, lib.eec_last_error().decode()), (what, lib.eec_last_error())


def test_backward_refuses_a_vocabulary_that_is_no_row_of_float4(lib):
    for V in (6, 260):
        assert _call(lib, "backward", V=V) == BAD_ARG
        assert b"multiple of 4, <= 256" in lib.eec_last_error()
    assert _call(lib, "forward", V=6, ws_bytes=16) == WORKSPACE  # the forward serves any vocabulary: it gets as far as the workspace


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_chunks_outside_the_batch_and_workspaces_are_refused(lib, which):
    for kw in (dict(b0=-1, nb=1), dict(b0=2, nb=2), dict(nb=0)):
        assert _call(lib, which, **kw) == BAD_ARG, kw
    assert _call(lib, which, ws_bytes=16) == WORKSPACE and b"workspace too small" in lib.eec_last_error()
    assert _call(lib, which, ws=0x1004) == WORKSPACE and b"aligned" in lib.eec_last_error()


@pytest.mark.parametrize("which,name", [("hyp_logp", n) for n in ("logp", "hyp", "hyp_len", "ll")]
                         + [("forward", n) for n in ("logp", "hyp", "hyp_len", "risk", "ll", "loss_eb", "loss", "workspace")]
                         + [("backward", n) for n in ("logp", "hyp", "hyp_len", "workspace", "grad_loss", "dlogp")])
def test_null_pointers_are_refused_without_a_device(lib, which, name):
    assert _call(lib, which, null=(name,)) == BAD_ARG
    assert b"null" in lib.eec_last_error()


def test_workspace_bytes(lib):
    ws = lib.eec_ctc_mwer_workspace_bytes
    for E, B, T, N, L in itertools.product((0, -1, 2), repeat=5):
        if min(E, B, T, N, L) <= 0:
            assert ws(E, B, T, N, L) == 0
    for L, P in ((1, 2), (63, 2), (64, 4), (127, 4), (128, 8), (255, 8), (1000, 8)):
        assert ws(6, 64, 256, 10, L) >= 6 * 64 * 10 * 256 * 64 * P * 4
        assert ws(6, 64, 256, 10, L) < 6 * 64 * 10 * 256 * 64 * P * 4 + (1 << 20)
    assert ws(6, 64, 256, 10, 255) > 1 << 30  # the case the Python layer splits
    assert ws(2, 4, 8, 4, 10) % 256 == 0 and ws(2, 5, 8, 4, 10) > ws(2, 4, 8, 4, 10)


def test_descent_step_size_makes_the_restatement_decrease_at_every_step():
    """The step size the GPU descent test uses: 20 plain gradient steps of the fp64 restatement on logits [1, 2, 24, 16], every one
    a decrease of the expected risk."""
    tr = M.restatement_trajectory()
    assert len(tr) == 21 and all(b < a for a, b in zip(tr, tr[1:])), tr
    assert tr[0] - tr[-1] > 0.1
