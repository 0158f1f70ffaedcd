"""Inputs, closed forms and bounds shared by tests/test_oracle_frontend.py (CPU) and tests/test_gpu_frontend.py (the HIP kernel
behind ``frontend.MelFrontend``, csrc/frontend.hip).  Everything is built from seeds; all shapes are small.

Reference: ``oracle.frontend_ref.mel_frontend_fp64`` -- frames gathered by index (reflect once at either end, then clamp), a
periodic hann window and a direct 1024-point DFT in float64, torch's fp32 htk filter table cast to float64.

Measures and bounds (the ones of test_mel_frontend_against_oracle, tests/test_gpu_parity.py):
  * ``err_peak``: |got - want| over the largest mel value of the same frame;          kernel bound 2e-5
  * ``err_rel`` : |got - want| / want where want exceeds 1e-3 of that frame's peak;   kernel bound 1e-4
The fp32 statement of the reference (``mel_frontend``: torch.stft + the same table) is held to one fifth of either bound
against the float64 oracle, so that a bound on the kernel is not a distance between two rounded results.

Measured: the fp32 torch.stft statement against the float64 oracle, worst over the valid lengths above 512 of LENGTHS
(tests/test_oracle_frontend.py::test_fp32_statement_against_fp64 prints these figures):

    signal     err_peak   err_rel
    noise      4.0e-07    2.9e-06
    tone       2.1e-07    1.7e-06
    ramp       2.5e-07    1.2e-06
    square     1.6e-07    9.5e-07
    dc         1.9e-07    4.3e-07
    int16      2.8e-07    1.3e-06
    nyquist    1.3e-07    1.3e-07
    bound      4.0e-06    2.0e-05
"""
import functools
import math

import torch

from oracle import frontend_ref as FR

SAMPLE_RATE, N_FFT, WIN, HOP, N_MELS = 16000, 512, 320, 160, 80   # the reference's defaults (n_fft is doubled for the transform)
N_BINS = N_FFT + 1
BOUND_PEAK, BOUND_REL = 2e-5, 1e-4                                # the kernel against the float64 oracle
REF_BOUND_PEAK, REF_BOUND_REL = BOUND_PEAK / 5, BOUND_REL / 5     # the fp32 statement against the float64 oracle

SIGNAL_LEN = 5121
SIGNAL_NAMES = ("noise", "tone", "ramp", "square", "dc", "int16", "nyquist")

# valid lengths inside a padded batch; the last two are Lmax + 7 (taken as Lmax) and -3 (taken as 0)
LENGTHS = (0, 1, 2, 159, 160, 161, 319, 320, 321, 512, 513, 4959, 4960, 4961, 5119, 5120, 5121)
LENGTHS_LMAX = 5121
LENGTH_OVER, LENGTH_NEGATIVE = LENGTHS_LMAX + 7, -3

# Lmax -> Tmax = 1 + Lmax // 160: the last 32-frame workgroup is full (32), holds one frame (33) or is absent (1, 31)
LMAX_TMAX = ((100, 1), (4800, 31), (4960, 32), (5120, 33), (5121, 33))

CONFIG_N_MELS = (1, 23, 40, 80, 128, 256)
CONFIG_SAMPLE_RATES = (8000, 11025, 16000, 22050, 44100)
CONFIGS = tuple((sr, nm) for sr in CONFIG_SAMPLE_RATES for nm in CONFIG_N_MELS)
# settings at which torch's table has a filter with no non-zero bin at all (its two points fall between two bin frequencies):
# the packer's empty-support branch.  The first two are the smallest such settings; each has filter 0 empty.
EMPTY_16K_256, EMPTY_44K_128 = (16000, 256), (44100, 128)
EMPTY_FILTER_CONFIGS = (EMPTY_16K_256, EMPTY_44K_128, (22050, 256), (44100, 256))

SCALES = (2.0 ** -10, 2.0 ** -4, 2.0 ** 8, 2.0 ** 15)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def signal(name, n=SIGNAL_LEN):
    """One named fp32 test signal of ``n`` samples at 16 kHz."""
    i = SIGNAL_NAMES.index(name)
    noise = torch.randn(n, generator=_gen(100 + i))
    t = torch.arange(n, dtype=torch.float64) / SAMPLE_RATE
    if name == "noise":
        return 0.3 * noise
    if name == "tone":      # a loud 440 Hz tone over noise
        return 0.3 * noise + (3.0 * torch.sin(2 * math.pi * 440.0 * t)).float()
    if name == "ramp":      # quiet -> loud
        return 0.3 * noise * torch.linspace(1e-3, 1.0, n)
    if name == "square":    # 100 Hz square wave: rich harmonics (phase-shifted off the zero crossings)
        return torch.sign(torch.sin(2 * math.pi * 100.0 * t + 0.1)).float()
    if name == "dc":        # noise on a DC offset of 1000
        return 1000.0 + noise
    if name == "int16":     # noise rounded at int16 scale
        return (6000.0 * noise).round().clamp(-20000.0, 20000.0)
    if name == "nyquist":   # (-1)^n + 1e-3 noise: all the energy at the Nyquist bin, seen through the top filter's neighbours
        return (1.0 - 2.0 * (torch.arange(n) % 2)).float() + 1e-3 * noise
    raise KeyError(name)


def signals():
    return {name: signal(name) for name in SIGNAL_NAMES}


def noise_tone(rows, n, seed):
    """[rows, n]: 0.3 noise, a loud 440 Hz tone on row 0."""
    x = 0.3 * torch.randn(rows, n, generator=_gen(seed))
    x[0] += (3.0 * torch.sin(2 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / SAMPLE_RATE)).float()
    return x


def pad_nan(wave, lengths):
    """A copy of wave [B, Lmax] with NaN past each row's valid length (taken into [0, Lmax]): a finite output proves that
    those samples are not read, not even through a zero window weight."""
    out = wave.clone()
    for b, n in enumerate(lengths):
        out[b, min(max(int(n), 0), wave.size(1)):] = float("nan")
    return out


def n_frames(n):
    return 1 + n // HOP if n > 0 else 0


def measures(got, want):
    """(err_peak, err_rel) of got against want, both [n_mels, T] (or [B, n_mels, T]): the two measures of the module
    docstring, the frame peak taken over the mel axis."""
    got, want = got.double(), want.double()
    if want.numel() == 0:
        return 0.0, 0.0
    peak = want.amax(dim=-2, keepdim=True).clamp_min(1e-300)
    err = (got - want).abs()
    big = want > 1e-3 * peak
    e_rel = (err[big] / want[big]).max().item() if big.any() else 0.0
    return (err / peak).max().item(), e_rel


@functools.lru_cache(maxsize=None)
def filter_sums(sample_rate=SAMPLE_RATE, n_mels=N_MELS):
    """sum_k fb[k][m] of torch's table, float64 [n_mels] (shared: leave it unchanged)."""
    return FR.melscale_fbanks(N_BINS, 0.0, float(sample_rate // 2), n_mels, sample_rate).double().sum(dim=0)


def empty_filters(sample_rate, n_mels):
    """The mel bins whose filter has no non-zero weight in torch's table."""
    fb = FR.melscale_fbanks(N_BINS, 0.0, float(sample_rate // 2), n_mels, sample_rate)
    return [m for m in range(n_mels) if not bool((fb[:, m] > 0).any())]


def impulse_mel(n_samples, n0, sample_rate=SAMPLE_RATE, n_mels=N_MELS):
    """Closed form for a unit impulse at sample n0, HOP <= n0 <= n_samples - HOP - 2 (no reflection reaches it with a non-zero
    window weight: the last frame reads up to sample L + 159, which reflects to L - 161): float64
    [n_mels, T], mel[m][t] = w[n0 - hop t + win / 2]^2 sum_k fb[k][m] on the at most two frames that cover n0, exactly 0
    elsewhere (slot 0 carries the window weight 0: that frame is 0 too)."""
    assert HOP <= n0 <= n_samples - HOP - 2
    w = torch.from_numpy(FR.hann_fp64(WIN))
    out = torch.zeros(n_mels, n_frames(n_samples), dtype=torch.float64)
    fs = filter_sums(sample_rate, n_mels)
    for t in range(out.size(1)):
        j = n0 - HOP * t + WIN // 2
        if 0 <= j < WIN:
            out[:, t] = w[j] ** 2 * fs
    return out


def impulse_at_one_frame0(sample_rate=SAMPLE_RATE, n_mels=N_MELS):
    """Frame 0 for a unit impulse at sample 1: the reflection shows it at window slots win / 2 - 1 and win / 2 + 1, whose
    window weights are equal, so X_k = w (e^{-i a (c-1)} + e^{-i a (c+1)}), a = 2 pi k / 1024, and
    P_k = 4 w[159]^2 cos^2(2 pi k / 1024);  mel[m][0] = 4 w[159]^2 sum_k fb[k][m] cos^2(2 pi k / 1024).  float64 [n_mels]."""
    w = FR.hann_fp64(WIN)
    k = torch.arange(N_BINS, dtype=torch.float64)
    fb = FR.melscale_fbanks(N_BINS, 0.0, float(sample_rate // 2), n_mels, sample_rate).double()
    return 4.0 * w[WIN // 2 - 1] ** 2 * (torch.cos(2 * math.pi * k / (2 * N_FFT)) ** 2) @ fb


def covering_frames(n_samples, n):
    """The frames of an utterance of n_samples whose window reads sample n (directly or through the reflection)."""
    idx = FR.frame_indices(n_samples, WIN, HOP)
    return [t for t in range(idx.shape[0]) if bool((idx[t] == n).any())]


def impulse(n_samples, n0):
    x = torch.zeros(n_samples)
    x[n0] = 1.0
    return x


# impulse sweep: row i holds a unit impulse at IMPULSE_N0 + i -- every window slot of the two covering frames, both parities
IMPULSE_LEN, IMPULSE_N0, IMPULSE_ROWS = 1600, 480, 330


def impulse_sweep():
    x = torch.zeros(IMPULSE_ROWS, IMPULSE_LEN)
    x[torch.arange(IMPULSE_ROWS), IMPULSE_N0 + torch.arange(IMPULSE_ROWS)] = 1.0
    return x


def edge_impulses():
    """[(n_samples, n0)]: impulses at samples 0, 1, L - 2, L - 1 for L a multiple of the hop and one more than a multiple."""
    return [(L, n0) for L in (1600, 1601) for n0 in (0, 1, L - 2, L - 1)]


def config_reference(power, sample_rate, n_mels):
    """float64 mel [B, n_mels, T] from the float64 power spectra [B][T, 513] of one batch (shared by every configuration:
    only the filter table depends on the setting)."""
    fb = FR.melscale_fbanks(N_BINS, 0.0, float(sample_rate // 2), n_mels, sample_rate).double().numpy()
    T = max(p.shape[0] for p in power)
    out = torch.zeros(len(power), n_mels, T, dtype=torch.float64)
    for b, p in enumerate(power):
        out[b, :, : p.shape[0]] = torch.from_numpy(p @ fb).T
    return out
