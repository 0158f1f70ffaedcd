"""CPU tests of adaptive inference's exit statistics and exit choice (include/eec.h, "Adaptive inference"; csrc/exit_stats.hip): the
fp64 restatement against a brute-force loop, the host path of ``exit_statistics`` against fp64, ``select_exits`` on hand-made
tables, the wrappers' argument errors, and the host side of the three entries: declared, exported, every bad argument refused with
its own message before anything is launched (no device here)."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import exit_cases as X
from conftest import ROOT
from early_exit_transformer_amd import capi, ctc
from early_exit_transformer_amd.build import LIB_PATH

ENTRIES = ("eec_exit_stats_workspace_bytes", "eec_exit_stats", "eec_exit_route")
BAD_ARG, BAD_WS = 10001, 10003
MAX_EXITS = 16
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


@pytest.mark.parametrize("name", ["scale8-ragged", "V32", "E16", "neg-inf", "lengths-clamped"])
def test_restatement_equals_the_brute_force_loop(name):
    x, fl = X.cases()[name]
    want = X.loop_stats(x.double(), fl)
    got = X.ref_stats(x, fl)
    assert torch.isfinite(want).all()
    assert (got - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("name", list(X.cases()))
def test_host_path_against_fp64(name):
    """The fp32 host path errs by less than the first term of the bound the GPU test holds the kernel to."""
    want, err32 = X.reference(name)
    assert torch.isfinite(want).all()
    room = (err32 / (2e-5 + 2e-5 * want.abs())).max().item()
    print(f"\n[exit stats {name}] fp32 host path: {room:.3f} of its bound")
    assert room <= 1.0
    x, fl = X.cases()[name]
    st = ctc.exit_statistics(x, fl)
    assert all(t.shape == x.shape[:2] and t.dtype == torch.float32 for t in st)
    assert (st.entropy >= 0).all() and (st.confidence <= 1 + 1e-6).all() and (st.greedy_logp <= 0).all()
    if fl is not None:
        empty = fl.clamp(0, x.size(2)) == 0
        assert all((t[:, empty] == 0).all() for t in st)


def test_host_path_nan_placement():
    bad, fl, clean = X.nan_past_length()
    assert all(torch.equal(a, b) for a, b in zip(ctc.exit_statistics(bad, fl), ctc.exit_statistics(clean, fl)))
    bad, fl, (e, b) = X.nan_inside_length()
    for t in ctc.exit_statistics(bad, fl):
        hit = torch.isnan(t)
        assert hit[e, b] and hit.sum() == 1


def test_select_exits_on_hand_made_tables():
    s = torch.tensor([[0.9, 0.5, 0.1, NAN],
                      [0.4, 0.5, 0.1, NAN],
                      [0.1, 0.5, 0.1, 0.0]])
    # below 0.5 passes; a tie does not, a NaN never does; the last exit takes whoever is left
    assert ctc.select_exits(s, 0.5).tolist() == [1, 2, 0, 2]
    assert ctc.select_exits(s, 0.5).dtype == torch.int32
    assert ctc.select_exits(s, 0.5, max_exit=1).tolist() == [1, 1, 0, 1]
    assert ctc.select_exits(s, 0.5, min_exit=1).tolist() == [1, 2, 1, 2]
    assert ctc.select_exits(s, 0.5, min_exit=2).tolist() == [2, 2, 2, 2]
    assert ctc.select_exits(s, [1.0, 0.0, 0.0]).tolist() == [0, 0, 0, 2]
    assert ctc.select_exits(s, (0.0, 0.45, 0.0)).tolist() == [1, 2, 1, 2]
    # higher is better: above passes
    assert ctc.select_exits(s, 0.45, higher_is_better=True).tolist() == [0, 0, 2, 2]
    assert ctc.select_exits(s, 0.5, higher_is_better=True).tolist() == [0, 2, 2, 2]
    assert ctc.select_exits(s[:, 2:3], 0.5).tolist() == [0]  # B = 1
    assert ctc.select_exits(s[:1], 0.0).tolist() == [0] * 4  # E = 1
    g = torch.Generator().manual_seed(3)
    table = torch.rand(6, 40, generator=g)
    table[torch.rand(6, 40, generator=g) < 0.1] = NAN
    for hib, lo, hi, thr in itertools.product((False, True), (0, 2), (None, 4), (0.3, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6])):
        assert torch.equal(ctc.select_exits(table, thr, hib, lo, hi), X.ref_select(table, thr, hib, lo, hi))


def test_python_wrappers_refuse_bad_arguments():
    x = torch.zeros(2, 3, 5, 8)
    with pytest.raises(ValueError, match=r"\[E, B, T', V\]"):
        ctc.exit_statistics(x[0])
    with pytest.raises(ValueError, match="floating-point"):
        ctc.exit_statistics(x.long())
    with pytest.raises(ValueError, match="multiple of 4"):
        ctc.exit_statistics(torch.zeros(2, 3, 5, 6))
    with pytest.raises(ValueError, match="multiple of 4"):
        ctc.exit_statistics(torch.zeros(1, 1, 2, 260))
    with pytest.raises(ValueError, match="at most 16 exits"):
        ctc.exit_statistics(torch.zeros(17, 1, 2, 8))
    with pytest.raises(ValueError, match="3 entries"):
        ctc.exit_statistics(x, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="int32 or int64"):
        ctc.exit_statistics(x, torch.tensor([1.0, 2.0, 3.0]))
    s = torch.zeros(3, 4)
    with pytest.raises(ValueError, match=r"\[E, B\]"):
        ctc.select_exits(s[0], 0.5)
    with pytest.raises(ValueError, match="floating-point"):
        ctc.select_exits(s.long(), 0.5)
    with pytest.raises(ValueError, match="one per exit"):
        ctc.select_exits(s, [0.5, 0.5])
    with pytest.raises(ValueError, match="NaN"):
        ctc.select_exits(s, NAN)
    for lo, hi in ((-1, None), (2, 1), (0, 3), (3, None)):
        with pytest.raises(ValueError, match="min_exit"):
            ctc.select_exits(s, 0.5, min_exit=lo, max_exit=hi)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ctc.exit_route(torch.zeros(4), 0.5)
    from early_exit_transformer_amd import model
    assert model.exit_statistics is ctc.exit_statistics and model.select_exits is ctc.select_exits
    assert model.ExitStatistics is ctc.ExitStatistics and model.AdaptiveOutput._fields == ("logp", "exit_of", "scores", "taps")


def test_entries_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/eec.h"
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert int(re.search(r"#define\s+EEC_EXIT_STATS_MAX_EXITS\s+(\d+)", header).group(1)) == MAX_EXITS
    assert lib.eec_abi_version() == 16


def _stats(lib, E=3, B=2, T=5, V=32, null=(), ws_bytes=None, ws=0x1000):
    """One eec_exit_stats call with made-up device addresses: every case here must be refused before anything is dereferenced."""
    fake = lambda name: None if name in null else C.c_void_p(0x1000)  # noqa: E731  (256-byte aligned, never read)
    nbytes = lib.eec_exit_stats_workspace_bytes(E, B, T) if ws_bytes is None else ws_bytes
    return lib.eec_exit_stats(fake("x"), fake("frame_len"), E, B, T, V, fake("stats"), None if "workspace" in null else C.c_void_p(ws),
                              nbytes, None)


def _route(lib, n=4, threshold=0.5, force_all=0, null=()):
    fake = lambda name: None if name in null else C.c_void_p(0x1000)  # noqa: E731
    return lib.eec_exit_route(fake("score"), n, threshold, 0, force_all, fake("stay"), fake("leave"), fake("counts"), None)


BAD_STATS = [
    ("E above the maximum", dict(E=MAX_EXITS + 1), f"at most {MAX_EXITS} exits, got 17"),
    ("V 260", dict(V=260), "multiple of 4, <= 256"),
    ("V 30", dict(V=30), "multiple of 4, <= 256"),
    ("E 0", dict(E=0), "positive"),
    ("B 0", dict(B=0), "positive"),
    ("T 0", dict(T=0), "positive"),
    ("V -4", dict(V=-4), "positive"),
    ("B * T above int", dict(B=1 << 16, T=1 << 15), r"B \* T above"),
    ("3 * E * B above int", dict(E=16, B=1 << 26, T=1), r"3 \* E \* B above"),
]


@pytest.mark.parametrize("what,kw,msg", BAD_STATS, ids=[b[0] for b in BAD_STATS])
def test_statistics_entry_refuses_bad_sizes_without_a_device(lib, what, kw, msg):
    _route(lib, n=0)  # another entry's message stands before the call: the one read below must be fresh
    assert _stats(lib, **kw) == BAD_ARG, what
    err = lib.eec_last_error().decode()
    assert err.startswith("exit statistics:") and re.search(msg, err), (what, err)


@pytest.mark.parametrize("name", ["x", "stats", "workspace"])
def test_statistics_entry_refuses_null_pointers(lib, name):
    _route(lib, n=0)
    assert _stats(lib, null=(name,)) == BAD_ARG
    assert lib.eec_last_error() == b"exit statistics: null argument"


def test_statistics_entry_checks_its_workspace(lib):
    """E = 16 and a NULL frame_len pass every argument check; a short or misaligned workspace is refused (still no device)."""
    assert _stats(lib, E=MAX_EXITS, null=("frame_len",), ws_bytes=16) == BAD_WS and b"workspace too small" in lib.eec_last_error()
    assert _stats(lib, E=MAX_EXITS, null=("frame_len",), ws_bytes=1 << 20, ws=0x1004) == BAD_WS and b"aligned" in lib.eec_last_error()
    ws = lib.eec_exit_stats_workspace_bytes
    for E, B, T in itertools.product((0, -1, 3), repeat=3):
        if min(E, B, T) <= 0:
            assert ws(E, B, T) == 0, (E, B, T)
    assert ws(6, 64, 256) == 3 * 6 * 64 * 256 * 4 and ws(1, 1, 1) == 12
    assert ws(16, 4096, 65536) == 3 * 16 * 4096 * 65536 * 4  # above 2^32 bytes: size_t arithmetic


def test_route_entry_refuses_bad_arguments(lib):
    for name in ("score", "stay", "leave", "counts"):
        _stats(lib, E=0)
        assert _route(lib, null=(name,)) == BAD_ARG
        assert lib.eec_last_error() == b"exit route: null argument"
    for n in (0, -5):
        _stats(lib, E=0)
        assert _route(lib, n=n) == BAD_ARG
        assert lib.eec_last_error().decode() == f"exit route: n must be positive, got {n}"
    _stats(lib, E=0)
    assert _route(lib, threshold=NAN) == BAD_ARG and b"threshold is NaN" in lib.eec_last_error()
