"""CPU tests of the mel front end's oracles (oracle/frontend_ref.py) and of the host-only part of its C ABI: the fp32
torch.stft statement against the float64 statement on the shared cases (tests/frontend_cases.py), the closed forms that
localise a frame or a reflection, and the argument checks that come before the library's first HIP call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import frontend_cases as FC
from oracle import frontend_ref as FR


def test_fp32_statement_against_fp64():
    """``mel_frontend`` (torch.stft, an fp32 FFT) against ``mel_frontend_fp64`` for every signal and every valid length above
    n_fft // 2 = 512 (torch raises below): both measures stay under one fifth of the kernel's bounds, 4e-6 and 2e-5.  The
    figures printed here are the table of frontend_cases.py."""
    worst_all = (0.0, 0.0)
    for name, x in FC.signals().items():
        worst = (0.0, 0.0)
        for n in FC.LENGTHS:
            if n <= FC.N_FFT:
                continue
            got, want = FR.mel_frontend(x[:n]), FR.mel_frontend_fp64(x[:n])
            assert got.shape == want.shape == (FC.N_MELS, FC.n_frames(n))
            worst = tuple(max(a, b) for a, b in zip(worst, FC.measures(got, want)))
        print(f"    {name:<10} {worst[0]:.1e}    {worst[1]:.1e}")
        worst_all = tuple(max(a, b) for a, b in zip(worst_all, worst))
        assert worst[0] < FC.REF_BOUND_PEAK and worst[1] < FC.REF_BOUND_REL, (name, worst)
    assert worst_all[0] > 0  # the two statements are not the same computation


def test_fp64_frames_are_torchs_reflect_padding():
    """Above n_fft // 2 samples the oracle's gather is torch's centred reflect padding restricted to the window; at and below,
    where torch raises, it is reflect-once-then-clamp; the frame count is 1 + L // hop and 0 for L = 0."""
    for n in FC.LENGTHS:
        idx = FR.frame_indices(n, FC.WIN, FC.HOP)
        assert idx.shape == (FC.n_frames(n), FC.WIN)
        if n == 0:
            continue
        assert idx.min() >= 0 and idx.max() <= n - 1
        if n > FC.N_FFT:
            pad = FC.N_FFT
            padded = torch.nn.functional.pad(torch.arange(n, dtype=torch.float64).view(1, 1, -1), (pad, pad), mode="reflect").view(-1).long()
            lo = pad - FC.WIN // 2
            want = torch.stack([padded[lo + FC.HOP * t: lo + FC.HOP * t + FC.WIN] for t in range(idx.shape[0])])
            assert np.array_equal(idx, want.numpy()), n
    assert FR.frame_indices(1, FC.WIN, FC.HOP).max() == 0
    # L = 161: frame 0 reflects to 160, 159 .. 1 | 0 .. 159; frame 1 runs 0 .. 160 and reflects back from 159 down to 1
    idx = FR.frame_indices(161, FC.WIN, FC.HOP)
    assert list(idx[0, :3]) == [160, 159, 158] and list(idx[1, 159:163]) == [159, 160, 159, 158] and idx[1, -1] == 1
    # L = 100 (shorter than half a window): reflect, then reflect back, then clamp
    idx = FR.frame_indices(100, FC.WIN, FC.HOP)
    assert idx.shape[0] == 1 and idx[0, 0] == 38 and idx[0, 160] == 0 and idx[0, 259] == 99 and idx[0, 261] == 97 and idx[0, 319] == 39
    assert FR.mel_frontend_fp64(torch.zeros(0)).shape == (FC.N_MELS, 0)
    x = torch.randn(3, 400, generator=torch.Generator().manual_seed(1))
    batch = FR.mel_frontend_fp64_batch(x, torch.tensor([400, 0, 161]))
    assert batch.shape == (3, FC.N_MELS, 3) and batch.dtype == torch.float64
    assert torch.equal(batch[0], FR.mel_frontend_fp64(x[0])) and not batch[1].any()
    assert torch.equal(batch[2, :, :2], FR.mel_frontend_fp64(x[2, :161])) and not batch[2, :, 2:].any()
    assert torch.equal(FR.mel_frontend_fp64_batch(x), FR.mel_frontend_fp64_batch(x, torch.tensor([407, 400, 400])))


@pytest.mark.parametrize("sample_rate,n_mels", [(16000, 80), FC.EMPTY_16K_256, (8000, 23)])
def test_impulse_identity(sample_rate, n_mels):
    """A unit impulse at n0 well inside the signal: mel[m][t] = w[n0 - hop t + win / 2]^2 sum_k fb[k][m] on the at most two
    frames that cover it, exactly 0 elsewhere."""
    n = FC.IMPULSE_LEN
    for n0 in (FC.IMPULSE_N0, FC.IMPULSE_N0 + 1, FC.IMPULSE_N0 + 77, FC.IMPULSE_N0 + 159, FC.IMPULSE_N0 + 160, FC.IMPULSE_LEN - FC.HOP - 2):
        got = FR.mel_frontend_fp64(FC.impulse(n, n0), sample_rate=sample_rate, n_mels=n_mels)
        want = FC.impulse_mel(n, n0, sample_rate, n_mels)
        cover = [t for t in range(got.size(1)) if 0 < n0 - FC.HOP * t + FC.WIN // 2 < FC.WIN]
        reads = FC.covering_frames(n, n0)  # these include a frame that holds n0 at slot 0, where the window weight is 0
        assert 1 <= len(cover) <= 2 and set(cover) <= set(reads) and all(n0 - FC.HOP * t + FC.WIN // 2 == 0 for t in set(reads) - set(cover))
        rest = [t for t in range(got.size(1)) if t not in cover]
        assert (got[:, rest] == 0).all() and (want[:, rest] == 0).all()
        assert (got[:, cover] - want[:, cover]).abs().max().item() <= 1e-12 * want.max().item()
    for m in FC.empty_filters(sample_rate, n_mels):
        assert (got[m] == 0).all()


def test_edge_reflection_closed_forms():
    """Reflection without edge repeat: an impulse at sample 0 appears once in frame 0 (slot 160, window weight 1), an impulse
    at sample 1 twice (slots 159 and 161), and the two copies add coherently: P_k = 4 w[159]^2 cos^2(2 pi k / 1024)."""
    fs = FC.filter_sums()
    w = FR.hann_fp64(FC.WIN)
    assert w[0] == 0 and w[160] == 1 and abs(w[159] - w[161]) < 1e-15
    got0 = FR.mel_frontend_fp64(FC.impulse(1600, 0))
    assert (got0[:, 0] - fs).abs().max().item() <= 1e-12 * fs.max().item()  # once: with an edge repeat it would be (1 + w[159])^2-ish
    assert (got0[:, 1] == 0).all() and (got0[:, 2:] == 0).all()             # frame 1 holds it at slot 0, weight 0
    got1 = FR.mel_frontend_fp64(FC.impulse(1600, 1))
    want1 = FC.impulse_at_one_frame0()
    assert (got1[:, 0] - want1).abs().max().item() <= 1e-12 * want1.max().item()
    assert (got1[:, 1] - w[1] ** 2 * fs).abs().max().item() <= 1e-12 * (w[1] ** 2 * fs).max().item()
    assert (got1[:, 2:] == 0).all()
    # the low filters see the two copies in phase (4 w^2), which an incoherent sum (2 w^2) or a single copy (w^2) would miss
    assert abs(want1[0].item() / (w[159] ** 2 * fs[0].item()) - 4.0) < 1e-3
    # the far end: L a multiple of the hop -- the last frame is centred on the first sample past the end
    for L, n0 in FC.edge_impulses():
        got = FR.mel_frontend_fp64(FC.impulse(L, n0))
        cover = FC.covering_frames(L, n0)
        assert 1 <= len(cover) <= 3 and (got[:, [t for t in range(got.size(1)) if t not in cover]] == 0).all()
    got = FR.mel_frontend_fp64(FC.impulse(1600, 1599))  # frame 10 reads 1440 .. 1599 then 1598 .. 1439: sample 1599 once
    assert (got[:, 10] - w[159] ** 2 * fs).abs().max().item() <= 1e-12 * fs.max().item()


def test_case_tables_are_what_the_kernel_branches_on():
    """The shared cases hit the paths they are named for."""
    assert [1 + n // FC.HOP for n, _ in FC.LMAX_TMAX] == [t for _, t in FC.LMAX_TMAX] == [1, 31, 32, 33, 33]
    assert len(FC.CONFIGS) == 30
    have_empty = [c for c in FC.CONFIGS if FC.empty_filters(*c)]
    assert have_empty and set(have_empty) == set(FC.EMPTY_FILTER_CONFIGS)
    assert FC.empty_filters(*FC.EMPTY_16K_256) == [0] and FC.empty_filters(*FC.EMPTY_44K_128) == [0]
    for sr, nm in FC.CONFIGS:  # torch's table gives the Nyquist bin no weight: the kernel's Nyquist path is not observable
        assert FR.melscale_fbanks(FC.N_BINS, 0.0, float(sr // 2), nm, sr)[-1].abs().max().item() == 0
    x = FC.signal("nyquist")
    p = FR.power_spectrum_fp64(x.numpy())
    assert (p[:, -8:].sum(axis=1) > 0.999 * p.sum(axis=1)).all() and (p.argmax(axis=1) == FC.N_BINS - 1).all()  # the window's main lobe
    assert FC.signal("int16").abs().max().item() > 15000 and torch.equal(FC.signal("int16"), FC.signal("int16").round())
    assert torch.equal(FC.signal("tone"), FC.signal("tone"))


@pytest.fixture(scope="module")
def lib():
    from early_exit_transformer_amd import capi
    from early_exit_transformer_amd.build import LIB_PATH
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def test_frontend_frames_is_host_arithmetic(lib):
    for n, want in ((0, 0), (1, 1), (159, 1), (160, 2), (161, 2), (320, 3), (-160, 0), (-1, 0)):
        assert lib.eec_frontend_frames(n, 160) == want == FC.n_frames(max(n, 0)), n
    assert lib.eec_frontend_frames(1000, 0) == 0 and lib.eec_frontend_frames(1000, -160) == 0


@pytest.mark.parametrize("what,args", [("n_fft", (16000, 512, 320, 160, 80)), ("n_fft", (16000, 2048, 320, 160, 80)),
                                       ("win", (16000, 1024, 400, 160, 80)), ("hop", (16000, 1024, 320, 80, 80)),
                                       ("n_mels", (16000, 1024, 320, 160, 0)), ("n_mels", (16000, 1024, 320, 160, 257)),
                                       ("sample_rate", (0, 1024, 320, 160, 80)), ("sample_rate", (-16000, 1024, 320, 160, 80))])
def test_frontend_create_refuses_before_touching_a_device(lib, what, args):
    """Every refusal comes before the first HIP call (the test runs without a device), leaves the handle alone and carries its
    own non-empty message."""
    from early_exit_transformer_amd import capi
    ps = capi.EecDecoderParams()
    assert lib.eec_decoder_forward(C.byref(ps), 256, 8, 2048, 256, 126, None, None, 1, 1, 1, 0, 3, 1, None, None, 0, None) != 0
    stale = lib.eec_frontend_last_error()
    h = C.c_void_p()
    assert lib.eec_frontend_create(*args, C.byref(h)) != 0, what
    msg = lib.eec_frontend_last_error()
    assert msg and msg != stale and not h.value, (what, msg)


def test_frontend_create_refuses_a_null_handle(lib):
    assert lib.eec_frontend_create(16000, 1024, 320, 160, 80, None) != 0
    assert b"out" in lib.eec_frontend_last_error()
    lib.eec_frontend_destroy(None)  # a no-op
