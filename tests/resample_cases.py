"""Resampling and speed perturbation (include/eec.h, "Resampling / speed perturbation"; csrc/resample.hip;
early_exit_transformer_amd/augment.py) restated for the tests: the filter table from the formula in float64, the sum written per
output sample with explicit index arithmetic, the draw in Python integers, and the lengths and batches the host and GPU tests share.

Nothing here imports the product: the restatement is an independent second statement of the header."""
import math

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
SITE = 0x53504545


def reduce(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def speed_ratio(factor, sample_rate=16000):
    return reduce(int(factor * sample_rate), sample_rate)


def out_len(length, o, n):
    return (n * length + o - 1) // o


# ---------------------------------------------------------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------------------------------------------------------
def plan_fp64(o, n, lpw=6, rolloff=0.99):
    """``{"o", "n", "width", "K", "h": float64 [n, K]}`` of the reduced ratio (o, n), element by element from the formula."""
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    K = 2 * width + o
    h = np.zeros((n, K), dtype=np.float64)
    for j in range(n):
        for k in range(K):
            t = (-j / n + (k - width) / o) * base
            t = min(max(t, -float(lpw)), float(lpw))
            sinc = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            h[j, k] = sinc * math.cos(math.pi * t / (2 * lpw)) ** 2 * base / o
    return {"o": o, "n": n, "width": width, "K": K, "h": h}


def dense(o, n, width, K, first, count, weights):
    """The same record from a compact table: phase j's stored weights are the taps first[j] .. first[j] + count[j] - 1, the rest 0."""
    h = np.zeros((n, K), dtype=np.float64)
    for j in range(n):
        assert 0 <= first[j] and first[j] + count[j] <= K and len(weights[j]) == count[j]
        h[j, first[j]:first[j] + count[j]] = np.asarray(weights[j], dtype=np.float64)
    return {"o": o, "n": n, "width": width, "K": K, "h": h}


def resample_fp64(x, length, table):
    """``(y, mag)`` float64 [out_len]: y[i] = sum_k h(i % n, k) * x[(i // n) * o + k - width] over the taps whose sample lies in
    [0, length) -- nothing at or past ``length`` is touched -- and mag[i] = sum_k |h| |x| over the same taps."""
    o, n, width, K, h = table["o"], table["n"], table["width"], table["K"], table["h"]
    x = np.asarray(x)
    m = out_len(length, o, n)
    y, mag = np.zeros(m, dtype=np.float64), np.zeros(m, dtype=np.float64)
    for i in range(m):
        q, j = divmod(i, n)
        g0 = q * o - width                      # the sample of tap 0
        k_lo, k_hi = max(0, -g0), min(K, length - g0)
        if k_hi <= k_lo:
            continue
        taps = h[j, k_lo:k_hi]
        seg = x[g0 + k_lo:g0 + k_hi].astype(np.float64)
        y[i] = float(np.sum(taps * seg))
        mag[i] = float(np.sum(np.abs(taps) * np.abs(seg)))
    return y, mag


def nonzero_taps(table):
    """Per phase, the number of taps from the first to the last non-zero fp32 weight."""
    out = []
    for row in table["h"].astype(np.float32):
        nz = np.flatnonzero(row)
        out.append(int(nz[-1] - nz[0] + 1) if nz.size else 0)
    return out


def bound(table, mag):
    """(K_nz + 1) * 2^-24 * sum |h| |x| per output sample: the K-term fp32 dot product, in any order."""
    knz = np.array(nonzero_taps(table), dtype=np.float64)
    return (knz[np.arange(mag.shape[0]) % table["n"]] + 1.0) * 2.0 ** -24 * mag


def share_of_bound(got, want, allow):
    """The worst |got - want| / allow (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err > 0, np.inf, 0.0))))


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


def draw(seed, utt_offset, B, R):
    key = key_of(seed)
    return np.array([(word(key, (((utt_offset + b) & M64) * 64) & M64) * R) >> 32 for b in range(B)], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the shared batches of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
B, L = 8, 3000
# 2304 samples at 9 -> 10 and 2816 at 11 -> 10 give exactly 2560 outputs; the neighbours end one before and after
LENGTHS = [0, 1, 6, 7, 9, 23, 2303, 2304, 2305, 2816, 3000]
SPEED_RATIOS = [(9, 10), (11, 10), (1, 1)]
RATE_RATIOS = [(441, 160), (1, 2)]
# as speed factors, (int(f * sample_rate), sample_rate): 441.5 / 160 is safely inside [441, 442) whatever the rounding of the product
SPEED_FACTORS, SPEED_RATE = (0.9, 1.1, 1.0), 16000
RATE_FACTORS, RATE_RATE = (441.5 / 160, 0.5), 160


def batches(n_ratios):
    """(lengths, choices) of B utterances each: every ratio meets every length; the last batch is filled from the start of the list."""
    pairs = [(n, c) for c in range(n_ratios) for n in LENGTHS]
    pairs += pairs[:(-len(pairs)) % B]
    return [([n for n, _ in pairs[a:a + B]], [c for _, c in pairs[a:a + B]]) for a in range(0, len(pairs), B)]


def wave_batch(seed, lengths, pad=float("nan")):
    """Standard-normal fp32 samples [len(lengths), L]; ``pad`` at and past every length."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(lengths), L)).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, n:] = pad
    return x
