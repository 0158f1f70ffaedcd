"""SpecAugment (include/eec.h, "SpecAugment"; csrc/specaug.hip; early_exit_transformer_amd/augment.py) restated for the tests: the
draw in Python integers, the warp's source positions in exact integers with fp64 weights, the masks as loops -- one element at a time
where that is the plainest way to say it -- and the tables of shapes and prescribed parameter rows the host and GPU tests share.

Nothing here imports the product: the restatement is an independent second statement of the header."""
import math

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
SITE = 0x53504341
W = 5  # the warp window of the shared cases

# shapes of the GPU tests: partial groups of 32 mel rows (23, and 80 = 32 + 32 + 16), T not a multiple of 4, one partial and two tiles of 128 frames
SHAPES = [(80, 37), (23, 131), (23, 37), (80, 131)]


def lengths_of(T):
    """Empty, one frame, the longest length without a warp, the shortest with one, everything."""
    return [0, 1, 2 * W, 2 * W + 1, T]


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


def draw_row(n, n_mels, seed, utt, window, n_freq, F, n_time, ratio, Tmax):
    """The parameter row of utterance number ``utt`` (utt_offset + b) of ``n`` valid frames; ``ratio`` is taken as fp32, as the C ABI
    passes it."""
    key, at = key_of(seed), ((utt & M64) * 64) & M64
    below = lambda slot, m: (word(key, (at + slot) & M64) * m) >> 32  # noqa: E731
    row = [0, 0]
    if window > 0 and n > 2 * window:
        c = window + below(0, n - 2 * window)
        row = [c, c - window + 1 + below(1, 2 * window)]
    for k in range(n_freq):
        fw = below(2 + 2 * k, min(F, n_mels) + 1)
        row += [below(3 + 2 * k, n_mels - fw + 1), fw]
    most = min(Tmax, n, math.floor(float(np.float32(ratio)) * n))
    for k in range(n_time):
        slot = 2 + 2 * n_freq + 2 * k
        tw = below(slot, most + 1)
        row += [below(slot + 1, n - tw + 1), tw]
    return row


def draw(lengths, n_mels, T, seed, utt_offset=0, window=W, n_freq=2, F=27, n_time=5, ratio=0.05, Tmax=None):
    rows = [draw_row(min(max(int(n), 0), T), n_mels, seed, utt_offset + b, window, n_freq, F, n_time, ratio, T if Tmax is None else Tmax)
            for b, n in enumerate(lengths)]
    return np.array(rows, dtype=np.int32).reshape(len(rows), 2 + 2 * n_freq + 2 * n_time)


# ---------------------------------------------------------------------------------------------------------------------------
# the warp and the masks
# ---------------------------------------------------------------------------------------------------------------------------
def source(d, n_in, n_out, cubic):
    """Taps (indices inside the segment) and fp64 weights of output frame ``d`` of a segment of ``n_in`` source and ``n_out`` output
    frames: the position in exact integers, the fraction as the correctly rounded quotient of two exact integers."""
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    if not cubic:
        num = max(num, 0)
    i = num // den
    f = (num - i * den) / den
    if not cubic:
        return [i, min(i + 1, n_in - 1)], [1.0 - f, f]
    k1 = lambda x: (1.25 * x - 2.25) * x * x + 1.0            # noqa: E731  ((A + 2) x - (A + 3)) x x + 1, A = -0.75
    k2 = lambda x: ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0   # noqa: E731  ((A x - 5 A) x + 8 A) x - 4 A
    return [min(max(i - 1 + k, 0), n_in - 1) for k in range(4)], [k2(f + 1.0), k1(f), k1(1.0 - f), k2(2.0 - f)]


def warp_valid(n, c, w):
    return 1 <= c <= n - 1 and 1 <= w <= n - 1


def warp(x, c, w, cubic):
    """``x`` [rows, n] fp64 warped: (values, sum_k |w_k| |x_k| over the taps read), both [rows, n]."""
    n = x.shape[1]
    out, mag = np.empty_like(x), np.empty_like(x)
    for t in range(n):
        d, n_in, n_out, base = (t, c, w, 0) if t < w else (t - w, n - c, n - w, c)
        taps, wts = source(d, n_in, n_out, cubic)
        assert all(0 <= j < n_in for j in taps)  # never across c, never outside the utterance
        out[:, t] = sum(wk * x[:, base + j] for j, wk in zip(taps, wts))
        mag[:, t] = sum(abs(wk) * np.abs(x[:, base + j]) for j, wk in zip(taps, wts))
    return out, mag


def in_masks(pairs, limit, x):
    return any(max(s, 0) <= x < min(s + width, limit) for s, width in pairs)


COPIED, MASKED, WARPED = 0, 1, 2


def apply(mel, lengths, params, n_freq, n_time, cubic, mask_value=0.0):
    """``(out fp64, kind uint8, mag fp64)`` [B, n_mels, T]: COPIED elements equal the input bit for bit, MASKED ones equal
    ``mask_value``, WARPED ones are the fp64 value with ``mag`` = sum_k |w_k| |x_k|.  ``lengths`` None: T."""
    B, n_mels, T = mel.shape
    out, kind, mag = mel.astype(np.float64), np.zeros(mel.shape, np.uint8), np.zeros(mel.shape, np.float64)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        row = [int(v) for v in params[b]]
        c, w = row[:2]
        fm = list(zip(row[2:2 + 2 * n_freq:2], row[3:3 + 2 * n_freq:2]))
        tm = list(zip(row[2 + 2 * n_freq::2], row[3 + 2 * n_freq::2]))
        if warp_valid(n, c, w):
            out[b, :, :n], mag[b, :, :n] = warp(mel[b, :, :n].astype(np.float64), c, w, cubic)  # only the valid frames go in
            kind[b, :, :n] = WARPED
        rows = np.array([in_masks(fm, n_mels, r) for r in range(n_mels)], dtype=bool)
        frames = np.array([in_masks(tm, n, t) for t in range(n)], dtype=bool)
        hit = rows[:, None] | frames[None, :]
        out[b, :, :n][hit], kind[b, :, :n][hit] = mask_value, MASKED
    return out, kind, mag


BOUND = 6.0 * 2.0 ** -24  # one rounding per weight, one per product, three additions


def check_output(got, mel, want, kind, mag, mask_value=0.0):
    """``got`` fp32 against the restatement; returns the worst share of the bound a warped element used."""
    assert got.shape == mel.shape and got.dtype == np.float32
    same = got.view(np.int32) == mel.view(np.int32)
    assert same[kind == COPIED].all(), "a copied element is not a bit-for-bit copy"
    assert (got[kind == MASKED] == np.float32(mask_value)).all(), "a masked element is not mask_value"
    sel = kind == WARPED
    if not sel.any():
        return 0.0
    assert np.isfinite(got[sel]).all(), "a warped element is not finite: the padding reached a valid frame"
    err, allow = np.abs(got[sel].astype(np.float64) - want[sel]), BOUND * mag[sel]
    share = float(np.max(np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err > 0, np.inf, 0.0))))
    assert share <= 1.0, f"a warped element is off by {share:.3f} of the bound"
    return share


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def mel_batch(B, n_mels, T, seed, lengths=None, pad=None):
    """Signed fp32 values over four decades (cancellation between taps is part of the test); with ``lengths`` and ``pad`` the frames
    at or past a length hold ``pad`` (NaN: whatever reads the padding shows)."""
    rng = np.random.default_rng(seed)
    mel = (rng.standard_normal((B, n_mels, T)) * 10.0 ** rng.uniform(-2, 2, (B, n_mels, T))).astype(np.float32)
    if lengths is not None and pad is not None:
        for b, n in enumerate(lengths):
            mel[b, :, min(max(int(n), 0), T):] = pad
    return mel


def prescribed(n_mels, T):
    """(length, row) with two frequency and two time masks per row: the warp's edges, rows that must be ignored or clipped, zero and
    negative widths, masks that cover everything and masks that overlap.  A multiple of five rows: the GPU tests run them five at a time."""
    big = (1 << 31) - 1
    none = [0, 0, 0, 0, 0, 0, 0, 0]
    rows = [
        (T, [W, 1] + none),                               # the left segment squeezed onto one frame
        (T, [W, 2 * W] + none),                           # w = c + W
        (2 * W + 1, [W, 1] + none),                       # the shortest utterance that is warped
        (2 * W + 1, [W, 2 * W] + none),                   # w = n - 1: the right segment squeezed onto one frame
        (T, [T - 1, 1] + none),                           # c = n - 1 and w = 1: both segments at their extremes
        (T, [1, T - 1] + none),
        (T - 8, [10, 14, 3, 5, 5, 5, 2, 6, 4, 9]),        # a warp, overlapping masks, a length short of T
        (T, [0, 3] + none),                               # ignored: c = 0
        (T, [T, 1] + none),                               # ignored: c = n
        (T, [3, T] + none),                               # ignored: w = n
        (T, [-4, 2] + none),
        (T - 3, [big, -big] + none),
        (1, [1, 1, 0, 1, 0, 0, 0, 1, 0, 0]),              # n = 1: no warp fits; the one frame is time-masked
        (0, [3, 3, 0, n_mels, 0, 0, 0, T, 0, 0]),         # n = 0: nothing is touched
        (T, [0, 0, -3, 5, n_mels - 2, 10, -2, 4, T - 1, big]),   # clipped at both ends of both axes, a sum past int32
        (T - 5, [0, 0, n_mels, 4, -big, big - 1, T - 5, 3, T + 7, 2]),  # entirely outside: nothing masked
        (T, [0, 0, 2, 0, 4, -3, 5, 0, 9, -1]),            # zero and negative widths are no-ops
        (T, [0, 0, 0, n_mels, 0, 0, 0, 0, 0, 0]),         # a frequency mask over everything
        (T - 2, [0, 0, 0, 0, 0, 0, 0, T - 2, 0, 0]),      # a time mask over everything valid
        (T, [7, 9, 1, 3, 2, 4, 20, 8, 24, 9]),            # overlapping masks of both kinds under a warp
    ]
    assert len(rows) % 5 == 0
    return rows
