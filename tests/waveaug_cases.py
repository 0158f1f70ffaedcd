"""Waveform augmentation (include/eec.h, "Waveform augmentation: reverberation, noise, volume"; csrc/waveaug.hip;
early_exit_transformer_amd/augment.py) restated for the tests: the draw in Python integers, the RIR normalisation, the convolution, the
noise mix and the gain in float64 with explicit index arithmetic, and the utterances, RIRs and noises the host and GPU tests share.

Nothing here imports the product: the restatement is an independent second statement of the header."""
import math
import struct

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
SITE = 0x57415547
ONE_BITS = 0x3F800000


# ---------------------------------------------------------------------------------------------------------------------------
# the draw, from Python integers
# ---------------------------------------------------------------------------------------------------------------------------
def key_of(seed):
    x = ((seed & M64) * 0x9E3779B97F4A7C15 + ((SITE << 32) | SITE)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return ((x >> 32) ^ x) & M32


def word(key, index):
    h = ((index & M32) * 0x9E3779B1 + (index >> 32) * 0x85EBCA77 + key) & M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def f32_bits(v):
    """The bits of ``v`` (a Python float, fp64) rounded once to fp32, as a signed 32-bit integer."""
    return struct.unpack("<i", struct.pack("<f", v))[0]


def bits_f32(bits):
    return struct.unpack("<f", struct.pack("<i", bits))[0]


def threshold(p):
    return math.floor(p * 4294967296.0)


def draw(seed, utt_offset, B, n_rirs, p_reverb, noise_lens, p_noise, n_snrs, volume):
    """int32 [B, 5] rows rir, noise, start, snr_idx, gain_bits and the seven words of every utterance (uint64 [B, 7])."""
    key, thr_r, thr_n = key_of(seed), threshold(p_reverb), threshold(p_noise)
    rows, words = [], []
    for b in range(B):
        at = (((utt_offset + b) & M64) * 64) & M64
        u = [word(key, (at + slot) & M64) for slot in range(7)]
        rir = (u[1] * n_rirs) >> 32 if n_rirs > 0 and u[0] < thr_r else -1
        noise, start, snr = -1, 0, 0
        if len(noise_lens) > 0 and n_snrs > 0 and u[2] < thr_n:
            noise = (u[3] * len(noise_lens)) >> 32
            start = (u[4] * int(noise_lens[noise])) >> 32
            snr = (u[5] * n_snrs) >> 32
        gain = ONE_BITS if volume is None else f32_bits(volume[0] + (volume[1] - volume[0]) * (u[6] * 2.0 ** -32))
        rows.append([rir, noise, start, snr, gain])
        words.append(u)
    return np.array(rows, dtype=np.int32), np.array(words, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# the three stages in fp64
# ---------------------------------------------------------------------------------------------------------------------------
def rir_fp64(h, normalize, shift):
    """``(taps float64 before the single rounding, d, peak - lo)`` of the RIR ``h`` as given: the peak is the first index of max |h|,
    the divisor is evaluated in fp64, zero heads and tails (after rounding to fp32) are dropped."""
    h = [float(np.float32(v)) for v in h]
    p = max(range(len(h)), key=lambda k: (abs(h[k]), -k))
    div = {"none": 1.0, "peak": abs(h[p]), "l2": math.sqrt(math.fsum(v * v for v in h))}[normalize]
    v = np.array([x / div for x in h], dtype=np.float64)
    nz = np.flatnonzero(v.astype(np.float32))
    lo, hi = int(nz[0]), int(nz[-1]) + 1
    return v[lo:hi], (p - lo if shift else -lo), p - lo


def reverb_fp64(x, length, h, d):
    """``(y, mag)`` float64 [length]: y[i] = sum_k h[k] x[i + d - k] over the taps whose sample lies in [0, length) -- nothing at or
    past ``length`` is touched -- and mag[i] = sum_k |h[k]| |x[i + d - k]|."""
    x64 = np.asarray(x[:length], dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    y, mag = np.zeros(length, dtype=np.float64), np.zeros(length, dtype=np.float64)
    for k in range(h.shape[0]):
        # i + d - k in [0, length)  <=>  i in [k - d, length + k - d)
        i_lo, i_hi = max(0, k - d), min(length, length + k - d)
        if i_hi <= i_lo:
            continue
        seg = x64[i_lo + d - k:i_hi + d - k]
        y[i_lo:i_hi] += h[k] * seg
        mag[i_lo:i_hi] += abs(h[k]) * np.abs(seg)
    return y, mag


def reverb_bound(K, mag):
    """(K_nz + 1) * 2^-24 * sum |h| |x| per output sample: the K-term fp32 dot product, in any order."""
    return (K + 1.0) * 2.0 ** -24 * mag


def noise_segment(noise, start, length):
    """n[i] = noise[(s + i) mod len_m], s = start mod len_m."""
    noise = np.asarray(noise)
    return noise[[((start % noise.shape[0]) + i) % noise.shape[0] for i in range(length)]] if length else noise[:0]


def mix_fp64(y, seg, snr_db, gain):
    """``(out, scale, allow)`` in float64: scale = sqrt(E_s / E_n) * 10^(-snr / 20), out = (y + scale n) gain, and the per-sample
    allowance 4 * 2^-24 * (|y| + |scale n|) * |gain|.  seg None, or a zero energy: scale = 0 and out = y gain."""
    y64 = np.asarray(y, dtype=np.float64)
    scale, n64 = 0.0, np.zeros_like(y64)
    if seg is not None:
        n64 = np.asarray(seg, dtype=np.float64)
        es, en = math.fsum(v * v for v in y64), math.fsum(v * v for v in n64)
        if es > 0.0 and en > 0.0:
            scale = math.sqrt(es / en) * 10.0 ** (-snr_db / 20.0)
    out = (y64 + scale * n64) * float(gain)
    return out, scale, 4.0 * 2.0 ** -24 * (np.abs(y64) + np.abs(scale * n64)) * abs(float(gain))


def share_of_bound(got, want, allow):
    """The worst |got - want| / allow (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err > 0, np.inf, 0.0))))


def ulps32(got, want):
    """|got - want| in units of the fp32 spacing at ``want`` (a float64)."""
    if want == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return abs(float(got) - want) / float(np.spacing(np.float32(abs(want))))


# ---------------------------------------------------------------------------------------------------------------------------
# the shared utterances, RIRs and noises
# ---------------------------------------------------------------------------------------------------------------------------
B, L = 8, 3000
LENGTHS = [0, 1, 7, 1023, 1024, 1025, 2999, 3000]
SNRS = (20.0, 15.0, 10.0, 5.0, 0.0, -3.5)


def wave_batch(seed=1, pad=float("nan")):
    """Standard-normal fp32 samples [B, L]; ``pad`` at and past every length."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L)).astype(np.float32)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = pad
    return x


def rirs():
    """Eight RIRs: 1, 2, 63, 64, 65, 1025 and 2500 taps (longer than a chunk of 512 taps and, for most utterances, than the utterance)
    with the peak at the first, a middle and the last index in turn, decaying away from it; and one of 40 taps with five zeros in front
    and seven behind."""
    rng = np.random.default_rng(2)
    out = []
    for k, (K, where) in enumerate(zip((1, 2, 63, 64, 65, 1025, 2500), ("first", "last", "middle", "first", "last", "middle", "last"))):
        p = {"first": 0, "middle": K // 2, "last": K - 1}[where]
        h = rng.standard_normal(K) * np.exp(-np.abs(np.arange(K) - p) / (1.0 + K / 8.0)) * 0.3
        h[p] = 1.0 + 0.1 * k
        out.append(h.astype(np.float32))
    h = np.zeros(40, dtype=np.float32)
    h[5:33] = (rng.standard_normal(28) * 0.2).astype(np.float32)
    h[11] = -0.9
    out.append(h)
    return out


RIR_PEAKS = [0, 1, 31, 0, 64, 512, 2499, 11]


def noises():
    """Rows of 1, 5, 2999, 3000 and 4001 samples and an all-zero row of 17."""
    rng = np.random.default_rng(3)
    return [(rng.standard_normal(n) * 0.5 + 0.01).astype(np.float32) for n in (1, 5, 2999, 3000, 4001)] + [np.zeros(17, dtype=np.float32)]


def starts(len_m):
    """0, the last sample, and a start whose segment wraps in the middle of the longer utterances."""
    return [0, len_m - 1, len_m - min(len_m, 2001) // 2]
