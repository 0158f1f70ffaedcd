"""CPU tests of the self-distillation loss between exits (include/eec.h; csrc/distill.hip): the statement itself -- the closed-form
gradient of the header against fp64 autograd, the fp32 evaluation against the bounds the GPU tests hold the kernels to -- and the
host side of the three entries: declared, exported, every bad argument refused before anything is launched (no device here),
workspace sizing."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import distill_cases as D
from conftest import ROOT
from early_exit_transformer_amd import capi, ctc
from early_exit_transformer_amd.build import LIB_PATH

ENTRIES = ("eec_exit_distill_workspace_bytes", "eec_exit_distill_forward", "eec_exit_distill_backward")
BAD_ARG = 10001
MAX_EXITS = 16

CASE_NAMES = [c[0] for c in D.cases()]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_closed_form_gradient_is_the_autograd_gradient_in_fp64(name):
    """d loss[e] / dx[e, b, t, v] = tau (q_v - p_v) / (B max(len_b, 1)) for t < len_b, 0 elsewhere and on the teachers' rows: equal to
    the fp64 autograd gradient of the definition to 1e-12 relative, with per-exit weights."""
    (_, x, fl, teacher, tau), _, _ = D.reference(name)
    w = torch.linspace(0.5, 1.5, x.size(0), dtype=torch.float64)
    _, g_auto = D.ref_distill(x, fl, teacher, tau, torch.float64, w)
    g_closed = D.closed_form_grad(x, fl, teacher, tau, torch.float64, w)
    scale = g_auto.abs().max().item()
    assert scale > 0
    err = (g_closed - g_auto).abs().max().item()
    print(f"\n[distill {name}] closed form vs autograd: {err:.2e} of max|grad| {scale:.3e}")
    assert err <= 1e-12 * scale
    # exactly zero where the header says so
    mask, _ = D.frame_mask(fl, x.size(1), x.size(2))
    assert (g_auto[:, ~mask] == 0).all()
    for e, k in enumerate(D.teacher_map(teacher, x.size(0))):
        if k < 0:
            assert (g_auto[e] == 0).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fp32_statement_sits_inside_the_bounds(name):
    """The definition evaluated in fp32 on the CPU errs against fp64 by less than the first terms of the GPU tests' bounds
    (loss 2e-5 + 2e-5 |want|, gradient 1e-5 max|grad| + 1e-9) on every case: those terms decide, and they have room."""
    _, (want, gw), (l32, g32) = D.reference(name)
    assert torch.isfinite(want).all() and torch.isfinite(gw).all()
    lerr = (l32.double() - want).abs()
    lroom = (lerr / (2e-5 + 2e-5 * want.abs())).max().item()
    scale = gw.abs().max().item()
    groom = (g32.double() - gw).abs().max().item() / (1e-5 * scale + 1e-9)
    print(f"\n[distill {name}] fp32 statement: loss error {lroom:.3f} of its bound, gradient error {groom:.3f} of its bound")
    assert lroom <= 1.0 and groom <= 1.0


def test_losses_of_the_definition_behave():
    """KL is non-negative, 0 for an exit without a teacher, 0 between equal rows, and invariant under a per-row shift (fp64)."""
    x = D.inputs()["scale8"].double()
    losses, _ = D.ref_distill(x, None, [2, -1, 0], 2.0)
    assert losses[0] > 0 and losses[1] == 0 and losses[2] > 0
    same = torch.stack([x[0], x[0] + 3.0])
    assert D.ref_distill(same, None, "last", 1.0)[0].abs().max().item() < 1e-12
    g = torch.Generator().manual_seed(5)
    shifted = x + torch.randn(*x.shape[:3], 1, generator=g, dtype=torch.float64) * 4
    a, b = D.ref_distill(x, None, "last", 0.5)[0], D.ref_distill(shifted, None, "last", 0.5)[0]
    assert (a - b).abs().max().item() < 1e-10 * a.abs().max().item()


def test_entries_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/eec.h"
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert int(re.search(r"#define\s+EEC_DISTILL_MAX_EXITS\s+(\d+)", header).group(1)) == MAX_EXITS >= 16
    assert lib.eec_abi_version() == 16


def _call(lib, which, E=3, B=2, T=5, V=32, tau=1.0, teacher=(2, 2, -1), null=()):
    """One call of an entry with made-up device addresses: every case here must be refused before anything is dereferenced or
    launched.  ``null``: names of the pointers passed as NULL."""
    fake = lambda name: None if name in null else C.c_void_p(0x1000)  # noqa: E731  (256-byte aligned, never read)
    t = None if "teacher" in null else (C.c_int32 * max(len(teacher), 1))(*teacher)
    if which == "forward":
        return lib.eec_exit_distill_forward(fake("x"), fake("frame_len"), t, E, B, T, V, tau, fake("kl"), fake("loss"), fake("workspace"),
                                            lib.eec_exit_distill_workspace_bytes(E, B, T), None)
    return lib.eec_exit_distill_backward(fake("x"), fake("frame_len"), t, E, B, T, V, tau, fake("grad_loss"), 0, fake("dx"), None)


BAD = [
    ("a teacher that is its own student", dict(teacher=(2, 1, -1)), "own teacher"),
    ("a teacher index of E", dict(teacher=(3, 2, -1)), r"outside \[-1, E\)"),
    ("a teacher index of -2", dict(teacher=(2, -2, -1)), r"outside \[-1, E\)"),
    ("tau 0", dict(tau=0.0), "temperature"),
    ("tau below 0", dict(tau=-1.0), "temperature"),
    ("tau NaN", dict(tau=float("nan")), "temperature"),
    ("tau inf", dict(tau=float("inf")), "temperature"),
    ("V 260", dict(V=260), "multiple of 4, <= 256"),
    ("V 30", dict(V=30), "multiple of 4, <= 256"),
    ("E above the maximum", dict(E=MAX_EXITS + 1, teacher=tuple([MAX_EXITS] * MAX_EXITS + [-1])), f"at most {MAX_EXITS} exits"),
    ("E 0", dict(E=0, teacher=()), "positive"),
    ("B 0", dict(B=0), "positive"),
    ("T 0", dict(T=0), "positive"),
    ("V 0", dict(V=0), "positive"),
]


@pytest.mark.parametrize("which", ["forward", "backward"])
@pytest.mark.parametrize("what,kw,msg", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_without_a_device(lib, which, what, kw, msg):
    assert _call(lib, which, **kw) == BAD_ARG, what
    assert re.search(msg, lib.eec_last_error().decode()), (what, lib.eec_last_error())


@pytest.mark.parametrize("which,name", [("forward", n) for n in ("x", "teacher", "kl", "loss", "workspace")]
                         + [("backward", n) for n in ("x", "teacher", "grad_loss", "dx")])
def test_null_pointers_are_refused_without_a_device(lib, which, name):
    assert _call(lib, which, null=(name,)) == BAD_ARG
    assert b"null" in lib.eec_last_error()


def test_the_maximum_number_of_exits_passes_the_checks_up_to_the_workspace(lib):
    """E = 16 is served: with a short workspace the call gets past every argument check and is refused for the workspace (still
    without a device)."""
    t = (C.c_int32 * MAX_EXITS)(*([MAX_EXITS - 1] * (MAX_EXITS - 1) + [-1]))
    p = C.c_void_p(0x1000)
    rc = lib.eec_exit_distill_forward(p, None, t, MAX_EXITS, 2, 5, 32, 1.0, p, p, p, 16, None)
    assert rc == 10003 and b"workspace too small" in lib.eec_last_error()
    rc = lib.eec_exit_distill_forward(p, None, t, MAX_EXITS, 2, 5, 32, 1.0, p, p, C.c_void_p(0x1004), 1 << 20, None)
    assert rc == 10003 and b"aligned" in lib.eec_last_error()


def test_workspace_bytes_is_monotonic_and_zero_for_non_positive_sizes(lib):
    ws = lib.eec_exit_distill_workspace_bytes
    for E, B, T in itertools.product((0, -1, 3), repeat=3):
        if min(E, B, T) <= 0:
            assert ws(E, B, T) == 0, (E, B, T)
    sizes = (1, 2, 6, 16, 64, 257)
    for E, B, T in itertools.product(sizes, repeat=3):
        here = ws(E, B, T)
        assert here >= E * B * T * 4
        assert ws(E + 1, B, T) >= here and ws(E, B + 1, T) >= here and ws(E, B, T + 1) >= here
    assert ws(6, 64, 256) == 6 * 64 * 256 * 4
    assert ws(16, 4096, 65536) == 16 * 4096 * 65536 * 4  # above 2^32 bytes: size_t arithmetic


def test_python_wrappers_have_no_cpu_path_and_parse_the_teacher_map():
    x = torch.zeros(3, 2, 4, 8)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc.exit_distill_losses(x)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc.exit_training_losses(x, torch.ones(2, 2, dtype=torch.int64), torch.tensor([2, 2]))
    assert ctc._teacher_map("last", 4) == (3, 3, 3, -1) == tuple(D.teacher_map("last", 4))
    assert ctc._teacher_map("next", 4) == (1, 2, 3, -1) == tuple(D.teacher_map("next", 4))
    assert ctc._teacher_map([2, 0, -1], 3) == (2, 0, -1)
    assert ctc._teacher_map("last", 1) == (-1,)
    with pytest.raises(ValueError, match="one entry per exit"):
        ctc._teacher_map([1, 0], 3)
    with pytest.raises(ValueError, match="'last', 'next'"):
        ctc._teacher_map("first", 3)
    from early_exit_transformer_amd import model
    assert model.exit_distill_losses is ctc.exit_distill_losses and model.exit_training_losses is ctc.exit_training_losses
