"""CPU tests of waveform augmentation (include/eec.h, "Waveform augmentation: reverberation, noise, volume"): the restatement of
tests/waveaug_cases.py against numpy.convolve and torchaudio's add_noise formula in fp64; the bank images of the library against the
restated normalisation, and their refusals; the NumPy host path of ``augment.wave_augment`` / ``reverberate`` / ``add_noise`` against
the restatement within the bounds the GPU tests hold the kernels to; the host draw against the restated draw; the module."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import waveaug_cases as S
from early_exit_transformer_amd import augment, capi
from early_exit_transformer_amd.build import LIB_PATH

BAD_ARG, WORKSPACE = 10001, 10003
FAKE = 0x10000
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against other statements of the same thing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [True, False])
def test_the_restated_convolution_is_numpy_convolve_shifted_by_the_peak(shift):
    x = S.wave_batch(pad=0.0)
    for r, h in enumerate(S.rirs()):
        taps, d, peak = S.rir_fp64(h, "none", shift)
        lo = S.RIR_PEAKS[r] - peak
        assert (d == peak) if shift else (d == -lo)
        for b, n in enumerate(S.LENGTHS):
            y, mag = S.reverb_fp64(x[b], n, taps, d)
            full = np.convolve(x[b, :n].astype(np.float64), np.asarray(h, dtype=np.float64)) if n else np.zeros(0)
            first = S.RIR_PEAKS[r] if shift else 0  # the output keeps the input's length: full[first : first + n]
            want = np.concatenate([full, np.zeros(n)])[first:first + n]
            assert y.shape == (n,) and np.abs(y - want).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want).max(initial=0.0)), (r, b)
            assert (mag >= np.abs(y) * (1 - 1e-12)).all()


def test_the_restated_mix_is_torchaudios_add_noise_formula():
    x = S.wave_batch(pad=0.0)
    for m, noise in enumerate(S.noises()[:5]):
        for start in S.starts(noise.shape[0]):
            for b, n in enumerate(S.LENGTHS[1:], start=1):
                seg = S.noise_segment(noise, start, n)
                snr = S.SNRS[(m + b) % len(S.SNRS)]
                out, scale, _ = S.mix_fp64(x[b, :n], seg, snr, 1.0)
                xt, nt = torch.from_numpy(x[b, :n]).double(), torch.from_numpy(seg).double()
                es, en = (xt ** 2).sum(), (nt ** 2).sum()
                orig = 10 * (torch.log10(es) - torch.log10(en))
                want = xt + 10 ** ((orig - snr) / 20) * nt
                size = (np.abs(x[b, :n]) + abs(scale) * np.abs(seg)).max()  # the two terms may cancel: relative to their sizes
                assert np.abs(out - want.numpy()).max() <= 1e-12 * size, (m, start, b)
    # the tiling and the start reduced mod len_m
    assert S.noise_segment(np.arange(5), 3, 9).tolist() == [3, 4, 0, 1, 2, 3, 4, 0, 1] and S.noise_segment(np.arange(5), 13, 2).tolist() == [3, 4]
    out, scale, _ = S.mix_fp64(np.zeros(4, dtype=np.float32), np.ones(4), 5.0, 2.0)
    assert scale == 0.0 and not out.any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the bank images
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", ["l2", "peak", "none"])
@pytest.mark.parametrize("shift", [True, False])
def test_the_rir_image_is_the_restated_normalisation_rounded_once(lib, normalize, shift):
    rirs = S.rirs()
    bank = augment.RirBank(rirs, normalize=normalize, shift=shift)
    img = bank.image
    assert img[0] == augment.RIR_MAGIC == 0x52495242
    assert img[1] == len(rirs) == len(bank) and img[2] == img.shape[0] and img[3] == (augment.RIR_NORMS[normalize] | int(shift) << 8)
    at = 4 + 4 * len(rirs)
    for r, h in enumerate(rirs):
        taps, d, peak = S.rir_fp64(h, normalize, shift)
        K, d_img, off, peak_img = (int(v) for v in img[4 + 4 * r:8 + 4 * r])
        assert (K, d_img, off, peak_img) == (taps.shape[0], d, at, peak), r
        got_d, got = bank.rir(r)
        assert got_d == d and got.dtype == np.float32 and got[0] != 0 and got[-1] != 0
        err = np.abs(got.astype(np.float64) - taps)  # one rounding of the fp64 quotient (whose own error is far below)
        assert (err <= np.abs(taps) * 2.0 ** -24 * (1 + 1e-6)).all(), r
        if normalize == "l2":
            assert abs(float(np.sum(got.astype(np.float64) ** 2)) - 1.0) < 1e-5
        if normalize == "peak":
            assert abs(got[peak]) == 1.0 and np.abs(got).max() == 1.0
        if normalize == "none":
            assert np.array_equal(got, h[np.flatnonzero(h)[0]:np.flatnonzero(h)[-1] + 1])
        at += K
    assert at == img.shape[0]
    assert int(img[4 + 4 * 7]) == 28 and int(img[4 + 4 * 7 + 3]) == 6  # five zeros in front and seven behind are not stored


def test_the_noise_image_round_trips(lib):
    rows = S.noises()
    bank = augment.NoiseBank(rows)
    img = bank.image
    assert img[0] == 0x4E4F4953 and img[1] == len(rows) == len(bank) and img[2] == img.shape[0] and img[3] == 0
    at = 4 + 2 * len(rows)
    for m, row in enumerate(rows):
        assert (int(img[4 + 2 * m]), int(img[5 + 2 * m])) == (row.shape[0], at)
        assert np.array_equal(_bits(bank.noise(m)), _bits(row))
        at += row.shape[0]
    assert at == img.shape[0] and bank.lengths.tolist() == [r.shape[0] for r in rows]
    # torch tensors and float64 arrays are taken too; the image is cached per device
    again = augment.NoiseBank([torch.from_numpy(r) for r in rows[:2]] + [r.astype(np.float64) for r in rows[2:]])
    assert np.array_equal(again.image, img) and bank.on(torch.device("cpu")) is bank.on(torch.device("cpu"))


def _stale(lib):
    assert lib.eec_specaug_apply(None, None, None, 1, 1, 1, 0, 0, 1, 0.0, None, None) != 0
    return lib.eec_last_error()


def _f32(values):
    return (C.c_float * len(values))(*values)


def _i32(values):
    return (C.c_int32 * len(values))(*values)


def test_the_bank_entries_refuse_bad_arguments(lib):
    buf = np.zeros(70000, dtype=np.int32)
    ok, one = _f32([0.0, 1.0, 0.5]), _i32([3])
    many = _i32([1] * 4097)
    lots = _f32([1.0] * 4097)
    rir_cases = {
        "R = 0": (0, ok, one, 1, 1), "R = 4097": (4097, lots, many, 1, 1), "null taps": (1, None, one, 1, 1), "null counts": (1, ok, None, 1, 1),
        "no taps": (1, ok, _i32([0]), 1, 1), "16385 taps": (1, _f32([1.0] * 16385), _i32([16385]), 1, 1), "normalize 3": (1, ok, one, 3, 1),
        "normalize -1": (1, ok, one, -1, 1), "a NaN": (1, _f32([1.0, NAN, 0.5]), one, 1, 1), "an inf": (1, _f32([1.0, math.inf, 0.5]), one, 0, 1),
        "all zero": (1, _f32([0.0, 0.0, 0.0]), one, 1, 1), "all zero, none": (1, _f32([0.0, -0.0, 0.0]), one, 0, 0),
    }
    for name, args in rir_cases.items():
        stale = _stale(lib)
        assert lib.eec_rir_bank_bytes(*args) == 0, name
        msg = lib.eec_last_error()
        assert msg.startswith(b"rir bank: ") and msg != stale, (name, msg)
        stale = _stale(lib)
        assert lib.eec_rir_bank(*args, buf.ctypes.data, buf.nbytes) == BAD_ARG, name
        assert lib.eec_last_error().startswith(b"rir bank: ") and lib.eec_last_error() != stale, name
    noise_cases = {"M = 0": (0, ok, one), "M = 4097": (4097, lots, many), "null samples": (1, None, one), "null counts": (1, ok, None),
                   "an empty row": (1, ok, _i32([0])), "2^30 + 1 samples": (1, ok, _i32([(1 << 30) + 1])), "a NaN": (1, _f32([1.0, NAN, 0.5]), one),
                   "an inf": (1, _f32([-math.inf]), _i32([1]))}
    for name, args in noise_cases.items():
        stale = _stale(lib)
        assert lib.eec_noise_bank_bytes(*args) == 0, name
        msg = lib.eec_last_error()
        assert msg.startswith(b"noise bank: ") and msg != stale, (name, msg)
        assert lib.eec_noise_bank(*args, buf.ctypes.data, buf.nbytes) == BAD_ARG, name
    assert not buf.any()
    # the limits themselves are served: 4096 rows, 16384 taps
    assert lib.eec_rir_bank_bytes(4096, lots, many, 1, 1) == 4 * (4 + 4 * 4096 + 4096)
    assert lib.eec_rir_bank_bytes(1, _f32([1.0] * 16384), _i32([16384]), 1, 1) == 4 * (4 + 4 + 16384)
    assert lib.eec_noise_bank_bytes(4096, lots, many) == 4 * (4 + 2 * 4096 + 4096)
    need = lib.eec_rir_bank_bytes(1, ok, one, 1, 1)
    assert need == 4 * (4 + 4 + 2)
    assert lib.eec_rir_bank(1, ok, one, 1, 1, None, need) == BAD_ARG and b"null image" in lib.eec_last_error()
    assert lib.eec_rir_bank(1, ok, one, 1, 1, buf.ctypes.data, need - 1) == WORKSPACE and not buf.any()
    assert lib.eec_rir_bank(1, ok, one, 1, 1, buf.ctypes.data, need) == 0 and buf[0] == 0x52495242 and buf[10:].any() == 0
    buf[:] = 0
    need = lib.eec_noise_bank_bytes(1, ok, one)
    assert lib.eec_noise_bank(1, ok, one, None, need) == BAD_ARG and b"null image" in lib.eec_last_error()
    assert lib.eec_noise_bank(1, ok, one, buf.ctypes.data, need - 1) == WORKSPACE and not buf.any()
    assert lib.eec_noise_bank(1, ok, one, buf.ctypes.data, need) == 0 and buf[0] == 0x4E4F4953


def test_the_device_entries_refuse_bad_arguments_before_any_device_work(lib):
    """The addresses are plausible but unusable: a call that got past its checks would fault, not return."""
    table = (C.c_double * 2)(0.1, 1.0)

    def draw(**over):
        a = dict(B=3, thr_r=1 << 32, thr_n=0, n_snrs=2, volume=1, lo=0.5, hi=2.0, params=FAKE)
        a.update(over)
        return lib.eec_waveaug_draw(a["B"], 1, 0, FAKE, a["thr_r"], FAKE, a["thr_n"], a["n_snrs"], a["volume"], a["lo"], a["hi"], a["params"], None)

    def reverb(**over):
        a = dict(wave=FAKE, params=FAKE, B=3, L=100, out=2 * FAKE, partials=FAKE)
        a.update(over)
        return lib.eec_reverb(a["wave"], FAKE, a["params"], a["B"], a["L"], FAKE, a["out"], a["partials"], None)

    def energy(**over):
        a = dict(params=FAKE, B=3, L=100, partials=FAKE)
        a.update(over)
        return lib.eec_noise_energy(FAKE, FAKE, a["params"], a["B"], a["L"], FAKE, a["partials"], None)

    def mix(**over):
        a = dict(y=FAKE, params=FAKE, B=3, L=100, table=table, n_snrs=2, partials=FAKE, out=FAKE)
        a.update(over)
        return lib.eec_noise_mix(a["y"], FAKE, a["params"], a["B"], a["L"], FAKE, a["table"], a["n_snrs"], a["partials"], a["out"], FAKE, None)

    shape = [dict(B=-1), dict(L=-1), dict(L=(1 << 30) + 1)]
    bad = (C.c_double * 2)(0.1, NAN)
    for call, who, cases in ((draw, b"waveaug draw: ", [dict(B=-1), dict(thr_r=(1 << 32) + 1), dict(thr_n=(1 << 32) + 1), dict(n_snrs=-1), dict(n_snrs=65),
                                                        dict(lo=NAN), dict(hi=math.inf), dict(params=None)]),
                             (reverb, b"reverb: ", shape + [dict(wave=None), dict(params=None), dict(out=None), dict(out=FAKE), dict(partials=FAKE + 4)]),
                             (energy, b"noise energy: ", shape + [dict(params=None), dict(partials=None), dict(partials=FAKE + 4)]),
                             (mix, b"noise mix: ", shape + [dict(y=None), dict(params=None), dict(out=None), dict(n_snrs=65), dict(n_snrs=-1),
                                                            dict(table=None), dict(table=bad), dict(partials=FAKE + 4)])):
        for case in cases:
            stale = _stale(lib)
            assert call(**case) == BAD_ARG, (who, case)
            assert lib.eec_last_error().startswith(who) and lib.eec_last_error() != stale, (who, case)
        assert call(B=0) == 0
    assert lib.eec_waveaug_partials_bytes(3, 1025) == 3 * 2 * 16 and lib.eec_waveaug_partials_bytes(3, 0) == 3 * 16
    assert lib.eec_waveaug_partials_bytes(-1, 10) == 0 and lib.eec_last_error().startswith(b"waveaug partials: ")


def test_the_python_layer_refuses_with_value_errors():
    wave, n = torch.zeros(2, 50), torch.tensor([50, 20])
    rirs, noises = augment.RirBank([np.array([1.0, 0.5])]), augment.NoiseBank([np.ones(7)])
    cases = [
        lambda: augment.wave_augment(wave.double(), seed=0), lambda: augment.wave_augment(torch.zeros(2, 3, 4), seed=0),
        lambda: augment.wave_augment(wave, torch.tensor([1.0, 2.0]), seed=0), lambda: augment.wave_augment(wave, torch.tensor([1, 2, 3]), seed=0),
        lambda: augment.wave_augment(wave, seed=0, rirs=[np.ones(3)]), lambda: augment.wave_augment(wave, seed=0, noises=rirs),
        lambda: augment.wave_augment(wave, seed=0, p_reverb=1.5), lambda: augment.wave_augment(wave, seed=0, p_noise=-0.1),
        lambda: augment.wave_augment(wave, seed=0, p_noise=NAN), lambda: augment.wave_augment(wave, seed=0, snrs=()),
        lambda: augment.wave_augment(wave, seed=0, snrs=list(range(65))), lambda: augment.wave_augment(wave, seed=0, snrs=(NAN,)),
        lambda: augment.wave_augment(wave, seed=0, volume=(1.0,)), lambda: augment.wave_augment(wave, seed=0, volume=(0.5, math.inf)),
        lambda: augment.wave_augment(wave, seed=0, params=torch.zeros(2, 4, dtype=torch.int32)),
        lambda: augment.wave_augment(wave, seed=0, params=torch.zeros(2, 5)),
        lambda: augment.reverberate(wave, n, noises, 0), lambda: augment.reverberate(wave, n, rirs, torch.tensor([0])),
        lambda: augment.reverberate(wave, n, rirs, 0.5), lambda: augment.add_noise(wave, n, rirs, 0, 0, 10.0),
        lambda: augment.add_noise(wave, n, noises, 0, 0, [10.0]), lambda: augment.add_noise(wave, n, noises, 0, torch.tensor([0.0, 1.0]), 10.0),
        lambda: augment.add_noise(wave, n, noises, 0, 0, NAN),
        lambda: augment.RirBank([]), lambda: augment.RirBank([np.ones(3)], normalize="max"), lambda: augment.RirBank([np.ones((2, 3))]),
        lambda: augment.RirBank([np.ones(16385)]), lambda: augment.RirBank([np.zeros(4)]), lambda: augment.RirBank([np.array([1.0, NAN])]),
        lambda: augment.RirBank(np.ones(3)), lambda: augment.RirBank([np.ones(1)] * 4097), lambda: augment.NoiseBank([np.zeros(0)]),
        lambda: augment.NoiseBank([np.array([math.inf])]), lambda: augment.NoiseBank([np.array(["a"])]),
        lambda: augment.WaveAugment(seed=1, p_reverb=2.0), lambda: augment.WaveAugment(seed=1, rirs=[np.zeros(3)]),
    ]
    for k, case in enumerate(cases):
        with pytest.raises(ValueError):
            case()
            pytest.fail(f"case {k} was accepted")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the host path
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_host_reverberation_is_the_restatement_within_the_bound():
    x, lens = S.wave_batch(), torch.tensor(S.LENGTHS)
    bank = augment.RirBank(S.rirs())
    worst = 0.0
    for r in range(len(bank)):
        d, taps = bank.rir(r)
        out = augment.reverberate(torch.from_numpy(x), lens, bank, r).numpy()
        assert not np.isnan(out).any()
        for b, n in enumerate(S.LENGTHS):
            assert (_bits(out[b, n:]) == 0).all()
            y, mag = S.reverb_fp64(x[b], n, taps, d)
            share = S.share_of_bound(out[b, :n], y, S.reverb_bound(taps.shape[0], mag))
            assert share <= 1.0, (r, b, share)
            worst = max(worst, share)
    assert 0.0 < worst
    # no RIR, an index outside the bank: the utterance itself
    for index in (-1, len(bank), torch.tensor([-1, 8, 99, -7, 2 ** 40, -2 ** 40, 8, -1])):
        out = augment.reverberate(torch.from_numpy(x), lens, bank, index).numpy()
        for b, n in enumerate(S.LENGTHS):
            assert np.array_equal(_bits(out[b, :n]), _bits(x[b, :n])) and (_bits(out[b, n:]) == 0).all()


@pytest.mark.parametrize("where", [0, 1, 17, 63, 499])
def test_shift_puts_a_delta_with_its_peak_anywhere_back_to_a_copy(where):
    x, lens = S.wave_batch(), torch.tensor(S.LENGTHS)
    h = np.zeros(500, dtype=np.float32)
    h[where] = -3.0
    out = augment.reverberate(torch.from_numpy(x), lens, augment.RirBank([h], normalize="peak"), 0).numpy()
    late = augment.reverberate(torch.from_numpy(x), lens, augment.RirBank([h], normalize="peak", shift=False), 0).numpy()
    for b, n in enumerate(S.LENGTHS):
        assert np.array_equal(_bits(out[b, :n]), _bits(-x[b, :n])) and (_bits(out[b, n:]) == 0).all()
        k = min(where, n)  # without the shift the utterance is delayed by the delta's index and cut to its length
        assert not late[b, :k].any() and np.array_equal(late[b, k:n], -x[b, :n - k]) and (_bits(late[b, n:]) == 0).all()


def test_the_host_mix_is_the_restatement_within_the_bounds():
    x, lens = S.wave_batch(), torch.tensor(S.LENGTHS)
    x[5, :] = np.where(np.isnan(x[5]), x[5], 0.0)  # one all-zero utterance
    noises = S.noises()
    bank = augment.NoiseBank(noises)
    worst = 0.0
    for m, row in enumerate(noises):
        for start in S.starts(row.shape[0]):
            snr = [S.SNRS[(m + b) % len(S.SNRS)] for b in range(S.B)]
            out = augment.add_noise(torch.from_numpy(x), lens, bank, m, start, snr).numpy()
            assert not np.isnan(out).any()
            for b, n in enumerate(S.LENGTHS):
                assert (_bits(out[b, n:]) == 0).all()
                want, scale, allow = S.mix_fp64(x[b, :n], S.noise_segment(row, start, n), snr[b], 1.0)
                if m == 5 or b == 5 or n == 0:
                    assert scale == 0.0 and np.array_equal(_bits(out[b, :n]), _bits(x[b, :n]))
                share = S.share_of_bound(out[b, :n], want, allow)
                assert share <= 1.0, (m, start, b, share)
                worst = max(worst, share)
    assert 0.0 < worst
    # a noise index outside the bank: the utterance itself
    out = augment.add_noise(torch.from_numpy(x), lens, bank, torch.tensor([-1, 6, 99, -7, 6, -1, 6, 7]), 0, 10.0).numpy()
    for b, n in enumerate(S.LENGTHS):
        assert np.array_equal(_bits(out[b, :n]), _bits(x[b, :n])) and (_bits(out[b, n:]) == 0).all()


def test_the_host_chain_reports_scale_and_gain_within_two_ulps():
    x, lens = S.wave_batch(), torch.tensor(S.LENGTHS)
    rirs, noises = augment.RirBank(S.rirs()[:5]), augment.NoiseBank(S.noises())
    out, params, applied = augment.wave_augment(torch.from_numpy(x), lens, seed=11, utt_offset=3, rirs=rirs, noises=noises, snrs=S.SNRS,
                                                volume=(0.125, 2.0))
    want, _ = S.draw(11, 3, S.B, 5, 1.0, [r.shape[0] for r in S.noises()], 1.0, len(S.SNRS), (0.125, 2.0))
    assert params.dtype == torch.int32 and np.array_equal(params.numpy(), want) and applied.shape == (S.B, 2)
    y = augment.reverberate(torch.from_numpy(x), lens, rirs, params[:, 0]).numpy()
    for b, n in enumerate(S.LENGTHS):
        r, m, start, snr_idx, bits = (int(v) for v in want[b])
        gain = S.bits_f32(bits)
        assert 0.125 <= gain <= 2.0 and _bits(applied[b, 1:])[0] == bits
        ref, scale, allow = S.mix_fp64(y[b, :n], S.noise_segment(S.noises()[m], start, n), S.SNRS[snr_idx], gain)
        assert S.ulps32(applied[b, 0].item(), scale) <= 2.0, (b, applied[b, 0].item(), scale)
        assert S.share_of_bound(out[b, :n].numpy(), ref, allow) <= 1.0 and (_bits(out[b, n:]) == 0).all()
    # a slice with utt_offset advanced, lengths = None against lengths all L, and prescribed rows equal to the drawn ones
    lo = augment.wave_augment(torch.from_numpy(x[:3].copy()), lens[:3], seed=11, utt_offset=3, rirs=rirs, noises=noises, snrs=S.SNRS, volume=(0.125, 2.0))
    hi = augment.wave_augment(torch.from_numpy(x[3:].copy()), lens[3:], seed=11, utt_offset=6, rirs=rirs, noises=noises, snrs=S.SNRS, volume=(0.125, 2.0))
    for k in range(3):
        assert np.array_equal(np.concatenate([_bits(lo[k]), _bits(hi[k])]), _bits((out, params, applied)[k]))
    again = augment.wave_augment(torch.from_numpy(x), lens, seed=0, rirs=rirs, noises=noises, snrs=S.SNRS, params=params)
    assert np.array_equal(_bits(again[0]), _bits(out)) and np.array_equal(_bits(again[2]), _bits(applied))
    full = torch.from_numpy(S.wave_batch(pad=0.25))
    a = augment.wave_augment(full, None, seed=5, rirs=rirs, noises=noises)
    b = augment.wave_augment(full, torch.full((S.B,), S.L), seed=5, rirs=rirs, noises=noises)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))
    one = augment.wave_augment(full[2], seed=5, utt_offset=2, rirs=rirs, noises=noises)
    assert one[0].shape == (S.L,) and all(np.array_equal(_bits(u), _bits(v[2])) for u, v in zip(one, a))


def test_the_host_energy_order_is_the_stated_one():
    """Eight consecutive samples in order, 64 such sums by halving, block 0 + block 1, the tiles in order: written out with Python
    floats for a length that ends inside the second tile."""
    rng = np.random.default_rng(8)
    v = (rng.standard_normal(1500) * np.exp(rng.standard_normal(1500) * 4)).astype(np.float32)
    total = 0.0
    for tile in range(2):
        sums = []
        for t in range(128):
            e = 0.0
            for j in range(8):
                i = 1024 * tile + 8 * t + j
                if i < 1500:
                    e = e + float(v[i]) * float(v[i])
            sums.append(e)
        blocks = []
        for blk in (sums[:64], sums[64:]):
            blk, s = list(blk), 32
            while s >= 1:
                for t in range(s):
                    blk[t] = blk[t] + blk[t + s]
                s //= 2
            blocks.append(blk[0])
        total = total + (blocks[0] + blocks[1])
    assert augment._host_energy(v) == total and augment._host_energy(v[:0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the draw and the module
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_host_draw_is_the_restated_draw():
    B, seed, utt = 257, 20240917, (1 << 32) - 100
    rirs, noises = augment.RirBank(S.rirs()), augment.NoiseBank(S.noises())
    lens = [r.shape[0] for r in S.noises()]
    wave = torch.zeros(B, 50)
    for p_r, p_n, volume in ((1.0, 1.0, (0.5, 1.5)), (0.0, 0.0, None), (0.5, 0.5, (2.0, 0.25)), (1.0, 0.0, None)):
        _, params, applied = augment.wave_augment(wave, seed=seed, utt_offset=utt, rirs=rirs, noises=noises, p_reverb=p_r, p_noise=p_n, snrs=S.SNRS,
                                                  volume=volume)
        want, words = S.draw(seed, utt, B, 8, p_r, lens, p_n, len(S.SNRS), volume)
        assert np.array_equal(params.numpy(), want), (p_r, p_n)
        assert np.array_equal(params[:, 0].numpy() >= 0, words[:, 0] < S.threshold(p_r))  # the coins, word for word
        assert np.array_equal(params[:, 1].numpy() >= 0, words[:, 2] < S.threshold(p_n))
        assert np.array_equal(_bits(applied[:, 1]), want[:, 4]) and not applied[:, 0].any()  # silence: E_s == 0, nothing added
        if p_r == 1.0:
            assert set(want[:, 0].tolist()) == set(range(8))
        if p_n == 1.0:
            assert set(want[:, 1].tolist()) == set(range(6)) and (want[:, 2] < np.array(lens)[want[:, 1]]).all() and set(want[:, 3].tolist()) == set(range(6))
        if p_r == 0.5:
            assert 0 < (want[:, 0] >= 0).sum() < B and 0 < (want[:, 1] >= 0).sum() < B
        if volume is None:
            assert (want[:, 4] == S.ONE_BITS).all()
    # without banks every stage is off
    _, params, _ = augment.wave_augment(wave, seed=seed)
    assert (params[:, :2] == -1).all() and (params[:, 4] == S.ONE_BITS).all()


def test_p_zero_and_eval_mode_return_the_input():
    x, lens = S.wave_batch(pad=0.0), torch.tensor(S.LENGTHS)
    wave = torch.from_numpy(x)
    rirs, noises = S.rirs()[:4], S.noises()
    out, params, applied = augment.wave_augment(wave, lens, seed=4, rirs=augment.RirBank(rirs), noises=augment.NoiseBank(noises), p_reverb=0.0,
                                                p_noise=0.0)
    assert np.array_equal(_bits(out), _bits(wave)) and (params[:, :2] == -1).all() and torch.equal(applied, torch.tensor([[0.0, 1.0]] * S.B))
    aug = augment.WaveAugment(seed=7, rirs=rirs, noises=noises, volume=(0.5, 2.0))
    assert not list(aug.parameters()) and not list(aug.buffers()) and not aug.state_dict() and "rirs=4" in repr(aug)
    aug.eval()
    assert aug(wave, lens) is wave and aug.get_state() == {"seed": 7, "calls": 0} and aug.last_params is None
    aug.train()
    first, p1 = aug(wave, lens), aug.last_params
    second, p2 = aug(wave, lens), aug.last_params
    assert aug.get_state() == {"seed": 7, "calls": 2} and not torch.equal(p1, p2) and not torch.equal(first, second)
    assert first.shape == wave.shape and aug.last_applied.shape == (S.B, 2)
    direct = augment.wave_augment(wave, lens, seed=(7 + 0x9E3779B97F4A7C15) & S.M64, rirs=aug.rirs, noises=aug.noises, volume=(0.5, 2.0))
    assert np.array_equal(_bits(direct[0]), _bits(second)) and torch.equal(direct[1], p2)
    aug.set_state({"seed": 7, "calls": 1})
    assert np.array_equal(_bits(aug(wave, lens)), _bits(second)) and aug.get_state()["calls"] == 2
    sliced = aug(wave[3:].contiguous(), lens[3:], utt_offset=3)  # call 2, a slice of the batch
    aug.set_state({"seed": 7, "calls": 2})
    assert np.array_equal(_bits(aug(wave, lens)[3:]), _bits(sliced))
    assert isinstance(augment.WaveAugment().seed, int)
