"""Reverberation by FFT without a device: the spectral image eec_rir_spectra builds against the restated fp64 DFT, its refusals, the
method switch of the bank, and the NumPy host path of an FFT bank against the fp64 convolution of reverb_fft_cases."""
import numpy as np
import pytest
import torch

import reverb_fft_cases as F
from early_exit_transformer_amd import augment, capi


ERR_BAD_ARG, ERR_WORKSPACE = 10001, 10003  # EEC_ERR_BAD_ARG, EEC_ERR_WORKSPACE


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def _error():
    return capi.load().eec_last_error().decode()


def test_the_constants_mirror_the_header_and_the_method_is_validated():
    assert augment.REVERB_FFT_BLOCK == F.S == 2048 and augment.REVERB_MAX_TAPS == F.MAX_TAPS
    assert F.S % augment.WAVEAUG_TILE == 0  # energy tiles never straddle blocks
    rirs = F.rirs()[:3]
    assert augment.RirBank(rirs).method == "direct" and augment.RirBank(rirs, method="direct").method == "direct"
    assert augment.RirBank(rirs, method="fft").method == "fft"
    # "auto" resolves once, by the longest stored RIR, on both sides of the threshold
    T = augment.REVERB_FFT_MIN_TAPS
    assert T == 256  # EEC_REVERB_FFT_MIN_TAPS: the smallest timed tap count from which the FFT path measured faster
    short, long_ = np.ones(T - 1, dtype=np.float32), np.ones(T, dtype=np.float32)
    assert augment.RirBank([short, short[:5]], method="auto").method == "direct"
    assert augment.RirBank([short, long_, short[:1]], method="auto").method == "fft"
    padded = np.concatenate([np.zeros(3, dtype=np.float32), long_[:T - 1], np.zeros(9, dtype=np.float32)])  # stored taps count, not given ones
    assert augment.RirBank([padded], method="auto").method == "direct" and augment.RirBank([padded], method="auto").max_taps == T - 1
    for bad in ("FFT", "", None, 1, "toeplitz"):
        with pytest.raises(ValueError, match="RirBank: method must be one of"):
            augment.RirBank(rirs, method=bad)
    bank, x = augment.RirBank(rirs), torch.zeros(2, 10)
    with pytest.raises(ValueError, match="reverberate: method must be one of"):
        augment.reverberate(x, None, bank, 0, method="auto?")
    assert bank.spectra is None  # built lazily: the host path of an FFT call does not need it either
    augment.reverberate(x, None, bank, 0, method="fft")
    assert bank.spectra is None and bank.spectra_image()[0] == augment.RIR_SPECTRA_MAGIC and bank.spectra is bank.spectra_image()


def test_the_spectral_image_is_the_restated_fp64_dft_rounded_once():
    """Header, records, offsets and twiddles by the documented layout; every stored bin against np.fft.rfft of the stored taps in
    float64 rounded once: equal bits, but for at most 1 bin in 10 000 where the two fp64 evaluations straddle a rounding boundary
    (then 1 ulp).  NumPy itself is held against a term-by-term fp64 DFT on a sample of bins."""
    for bank in (augment.RirBank(F.rirs(), method="fft"), augment.RirBank(F.impulses(), normalize="none", shift=False, method="fft")):
        image = bank.spectra_image()
        R = len(bank)
        at = (8 + 2 * R + 3) // 4 * 4
        assert image.dtype == np.int32 and list(image[:8]) == [augment.RIR_SPECTRA_MAGIC, R, image.shape[0], F.S, at, 0, 0, 0]
        u = np.arange(F.N // 2, dtype=np.float64)
        tw = image[at:at + F.N].view(np.float32).reshape(-1, 2)
        assert np.max(np.abs(tw[:, 0] - np.cos(2 * np.pi * u / F.N))) <= 2.0 ** -25 and np.max(np.abs(tw[:, 1] + np.sin(2 * np.pi * u / F.N))) <= 2.0 ** -25
        assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0 and tw[F.N // 4, 0] == 0.0 and tw[F.N // 4, 1] == -1.0  # exact on the axes
        at += F.N
        bins = off = 0
        for r in range(R):
            d, taps = bank.rir(r)
            P = -(-taps.shape[0] // F.S)
            assert list(image[8 + 2 * r:10 + 2 * r]) == [P, at]
            got, want64 = bank.spectrum(r), F.spectra_fp64(taps)
            assert got.shape == (P, F.N) and got.dtype == np.float32
            want = want64.astype(np.float32)
            differ = got != want  # by value: NumPy returns -0.0 in some imaginary bins of a one-tap partition, the library +0.0
            # where they differ: neighbours in fp32, and the fp64 value within 1e-9 of an ulp of the boundary between them
            if differ.any():
                ulp = np.spacing(np.abs(want[differ])).astype(np.float64)
                assert (np.abs(got[differ].astype(np.float64) - want[differ]) <= ulp).all(), r
                assert (np.abs(np.abs(want64[differ] - (got[differ].astype(np.float64) + want[differ]) / 2)) <= 1e-6 * ulp).all(), r
            bins, off = bins + differ.size, off + int(differ.sum())
            # NumPy against the term-by-term DFT on 16 bins of the last partition
            ks = np.unique(np.concatenate([[0, 1, F.N // 4, F.N // 2 - 1, F.N // 2], np.random.default_rng(r).integers(0, F.N // 2, 11)]))
            seg = taps[(P - 1) * F.S:].astype(np.float64)
            naive = F.naive_dft(seg, ks)
            ref = np.fft.rfft(seg, F.N)[ks]
            assert np.max(np.abs(naive - ref)) <= 64 * 2.0 ** -53 * np.sum(np.abs(seg)), r
            at += P * F.N
        assert at == image.shape[0] and off * 10000 <= bins, (off, bins)
        print(f"spectral image: {off} of {bins} bins one ulp from NumPy's")


def test_the_refusals_and_their_messages():
    lib = capi.load()
    bank = augment.RirBank(F.rirs()[:2])
    image = bank.image.copy()
    assert lib.eec_rir_spectra_bytes(None) == 0 and "rir spectra: null tap image" in _error()
    need = lib.eec_rir_spectra_bytes(image.ctypes.data)
    assert need == 4 * (12 + F.N + 2 * F.N)
    out = np.zeros(need // 4, dtype=np.int32)
    assert lib.eec_rir_spectra(image.ctypes.data, None, need) == ERR_BAD_ARG and "rir spectra: null image" in _error()
    assert lib.eec_rir_spectra(image.ctypes.data, out.ctypes.data, need - 4) == ERR_WORKSPACE
    assert f"rir spectra: the image needs {need} bytes, got {need - 4}" in _error() and not out.any()
    for word, value, message in ((0, 0, "is not one eec_rir_bank wrote"), (1, 0, "is not one eec_rir_bank wrote"),
                                 (1, augment.WAVEAUG_MAX_BANK + 1, "is not one eec_rir_bank wrote"), (4, 0, "RIR 0 of the tap image is out of range"),
                                 (8, augment.REVERB_MAX_TAPS + 1, "RIR 1 of the tap image is out of range"),
                                 (10, int(image[2]), "RIR 1 of the tap image is out of range")):
        broken = image.copy()
        broken[word] = value
        assert lib.eec_rir_spectra_bytes(broken.ctypes.data) == 0 and message in _error(), (word, value)
        assert lib.eec_rir_spectra(broken.ctypes.data, out.ctypes.data, need) == ERR_BAD_ARG and not out.any()
    # the device entry refuses before any device work
    assert lib.eec_reverb_fft_workspace_bytes(3, 2 * F.S + 1) == 3 * (3 + F.MAX_TAPS // F.S - 1) * F.N * 4
    assert lib.eec_reverb_fft_workspace_bytes(0, 0) == (F.MAX_TAPS // F.S - 1) * F.N * 4
    assert lib.eec_reverb_fft_workspace_bytes(-1, 4) == 0 and "B must not be negative" in _error()
    x, y, rows = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32), np.zeros(5, dtype=np.int32)
    call = lambda *a: lib.eec_reverb_fft(*a, None)  # noqa: E731
    assert call(None, None, None, 1, 4, None, None, None, None, None, 0) == ERR_BAD_ARG and "reverb fft: null argument" in _error()
    assert call(x.ctypes.data, None, rows.ctypes.data, 1, 4, None, None, x.ctypes.data, None, None, 0) == ERR_BAD_ARG
    assert "reverb fft: out must not be wave" in _error()
    assert call(x.ctypes.data, None, rows.ctypes.data, 1, (1 << 30) + 1, None, None, y.ctypes.data, None, None, 0) == ERR_BAD_ARG
    assert call(x.ctypes.data, None, rows.ctypes.data, 1, 4, None, None, y.ctypes.data, 4, None, 0) == ERR_BAD_ARG and "8-byte aligned" in _error()
    assert call(x.ctypes.data, None, rows.ctypes.data, 1, 4, image.ctypes.data, out.ctypes.data, y.ctypes.data, None, None, 0) == ERR_WORKSPACE
    assert "reverb fft: the workspace must be 16-byte aligned and not null" in _error()
    work = np.zeros(64, dtype=np.float64)
    assert call(x.ctypes.data, None, rows.ctypes.data, 1, 4, image.ctypes.data, out.ctypes.data, y.ctypes.data, None,
                work.ctypes.data // 16 * 16 + 16, 64) == ERR_WORKSPACE and "reverb fft: the workspace needs" in _error()
    assert call(x.ctypes.data, None, rows.ctypes.data, 0, 4, None, None, y.ctypes.data, None, None, 0) == 0  # B == 0: a no-op
    assert lib.eec_reverb_fft_stage(x.ctypes.data, None, rows.ctypes.data, 1, 4, None, None, y.ctypes.data, None, None, 0, 4, None) == ERR_BAD_ARG
    # Python refuses what the library would
    with pytest.raises(ValueError, match="rirs must be a RirBank"):
        augment.reverberate(torch.zeros(4), None, [np.ones(3)], 0, method="fft")


@pytest.mark.parametrize("shift", [True, False], ids=["shift", "causal"])
def test_the_numpy_host_path_of_an_fft_bank_is_inside_both_tolerances(shift):
    bank = augment.RirBank(F.rirs(), shift=shift, method="fft")
    x = torch.from_numpy(F.wave_batch())
    pairs = F.pairs_of(("rirs", shift), [bank.rir(r) for r in range(len(bank))], F.INDEX_ROWS)
    got = {}
    for row in F.INDEX_ROWS:
        out = augment.reverberate(x, torch.tensor(F.LENGTHS), bank, torch.tensor(row)).numpy()
        assert not np.isnan(out).any()
        for b, r in enumerate(row):
            assert (_bits(out[b, F.LENGTHS[b]:]) == 0).all()
            got.setdefault((r, b), out[b, :F.LENGTHS[b]])
    worst, share, _ = F.judge(pairs, got, f"host path, shift={shift}")
    assert worst <= 1.0  # fp64 rounded once: no worse than the fp32 transform it is measured with


def test_the_host_path_copies_keeps_zeros_and_leaves_the_direct_method_alone():
    x = F.wave_batch()
    fft, direct = augment.RirBank(F.rirs()[:6], method="fft"), augment.RirBank(F.rirs()[:6])
    index = torch.tensor([5, -1, 3, 6, 1, 0, 5, 99])
    lens = torch.tensor(F.LENGTHS)
    out = augment.reverberate(torch.from_numpy(x), lens, fft, index).numpy()
    for b in (1, 3, 7):
        n = F.LENGTHS[b]
        assert np.array_equal(_bits(out[b, :n]), _bits(x[b, :n])) and (_bits(out[b, n:]) == 0).all()
    zeros = np.where(np.isnan(x), x, np.float32(0.0))
    assert not augment.reverberate(torch.from_numpy(zeros), lens, fft, index).numpy().any()
    # method="direct", by the bank or by the call: the tap-order sum's bits
    a = augment.reverberate(torch.from_numpy(x), lens, direct, index).numpy()
    b = augment.reverberate(torch.from_numpy(x), lens, fft, index, method="direct").numpy()
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(out))
    for u, r in enumerate(index.tolist()):
        if 0 <= r < 6 and F.LENGTHS[u]:
            assert np.array_equal(_bits(a[u, :F.LENGTHS[u]]), _bits(augment._host_reverb(x[u, :F.LENGTHS[u]], *direct.rir(r))))
    # wave_augment follows the bank
    noises = augment.NoiseBank([np.ones(5, dtype=np.float32)])
    kw = dict(seed=3, noises=noises, p_noise=0.0)
    via_fft = augment.wave_augment(torch.from_numpy(x), lens, rirs=fft, **kw)
    via_direct = augment.wave_augment(torch.from_numpy(x), lens, rirs=direct, **kw)
    assert torch.equal(via_fft[1], via_direct[1]) and not np.array_equal(_bits(via_fft[0]), _bits(via_direct[0]))
    assert np.allclose(via_fft[0].numpy(), via_direct[0].numpy(), atol=1e-4)
