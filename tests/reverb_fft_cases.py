"""Reverberation by FFT (include/eec.h, "Reverberation by FFT"; csrc/reverb_fft.hip; early_exit_transformer_amd/augment.py) restated for the
tests: the layout of a stored spectrum, the derived worst-case bound, the working tolerance measured against an independent fp32 FFT,
and the utterances and RIRs the host and GPU tests share.  The shapes are the smallest at which the partitioning can go wrong, in
terms of the block S.

Nothing here imports the product: the restatement is an independent second statement of the header."""
import math

import numpy as np
import torch

S = 2048      # EEC_REVERB_FFT_BLOCK
N = 2 * S
MAX_TAPS = 16384
MARGIN = 4.0  # the working tolerance is MARGIN * e_ref (see judge())

B, L = 8, 3 * S + 907
LENGTHS = [0, 1, S - 1, S, S + 1, 2 * S, L - 1, L]
RIR_TAPS = (1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, MAX_TAPS)
IMPULSES = (0, 1, S - 1, S, S + 1, 2 * S - 1)
# the (RIR, utterance) pairs compared: three prescribed rows, RIR (b + s) mod 9 for utterance b, so that every RIR meets a short, a
# middle and a long utterance and the 16384-tap RIR (7) meets lengths 1, S + 1 and L
INDEX_ROWS = [[(b + s) % 9 for b in range(B)] for s in (0, 3, 6)]


def wave_batch(seed=11, pad=float("nan")):
    """Standard-normal fp32 samples [B, L]; ``pad`` at and past every length."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L)).astype(np.float32)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = pad
    return x


def rirs():
    """Nine RIRs: 1, 2, S - 1, S, S + 1, 2 S, 2 S + 1 and 16384 taps with the peak at the first, a middle and the last index in turn
    (so the shift d runs from 0 to K - 1), decaying away from it; and one of 2 S + 40 taps with five zeros in front and seven behind."""
    rng = np.random.default_rng(12)
    out = []
    for k, K in enumerate(RIR_TAPS):
        p = (0, K // 2, K - 1)[k % 3]
        h = rng.standard_normal(K) * np.exp(-np.abs(np.arange(K) - p) / (1.0 + K / 8.0)) * 0.3
        h[p] = 1.0 + 0.1 * k
        out.append(h.astype(np.float32))
    h = np.zeros(2 * S + 40, dtype=np.float32)
    h[5:-7] = (rng.standard_normal(2 * S + 28) * np.exp(-np.arange(2 * S + 28) / 600.0) * 0.2).astype(np.float32)
    h[11] = -0.9
    out.append(h)
    return out


RIR_PEAKS = [0, 1, S - 2, 0, S // 2, 2 * S - 1, 0, MAX_TAPS // 2, 6]  # peak - lo of the nine


def impulses():
    """Unit impulses at 0, 1, S - 1, S, S + 1, 2 S - 1 (to be banked with normalize="none", shift=False: y[i] = x[i - at])."""
    out = []
    for at in IMPULSES:
        h = np.zeros(at + 1, dtype=np.float32)
        h[at] = 1.0
        out.append(h)
    return out


def packed(X):
    """A spectrum X[0 .. N/2] (complex) in the stored order: (X[0], X[N/2]) both real, then (Re X[k], Im X[k]), 0 < k < N/2."""
    out = np.empty(N, dtype=np.float64)
    out[0], out[1] = X[0].real, X[N // 2].real
    out[2::2], out[3::2] = X[1:N // 2].real, X[1:N // 2].imag
    return out


def spectra_fp64(taps):
    """float64 [P, N]: the N-point DFT of every partition of S taps, by np.fft.rfft in float64, in the stored order."""
    taps = np.asarray(taps, dtype=np.float64)
    P = -(-taps.shape[0] // S)
    return np.stack([packed(np.fft.rfft(taps[p * S:(p + 1) * S], N)) for p in range(P)])


def naive_dft(seg, bins):
    """X[k] for k in ``bins`` of the N-point DFT of ``seg`` (at most S taps) term by term in float64 with exactly reduced angles."""
    n = np.arange(seg.shape[0], dtype=np.int64)
    out = []
    for k in bins:
        ang = -2.0 * np.pi * ((n * int(k)) % N).astype(np.float64) / N
        out.append(complex(math.fsum(seg * np.cos(ang)), math.fsum(seg * np.sin(ang))))
    return np.array(out)


def conv_fp64(x, length, h, d):
    """float64 [length]: y[i] = sum_k h[k] x[i + d - k], x = 0 outside [0, length), by one np.convolve in float64."""
    if length == 0:
        return np.zeros(0, dtype=np.float64)
    full = np.convolve(np.asarray(x[:length], dtype=np.float64), np.asarray(h, dtype=np.float64))
    at = np.arange(length, dtype=np.int64) + d
    return np.where((at >= 0) & (at < full.shape[0]), full[np.clip(at, 0, full.shape[0] - 1)], 0.0)


def fft32(x, length, h, d):
    """The independent fp32 FFT: irfft(rfft(x32, n) * rfft(h32, n)) by torch on the CPU in fp32, one transform of n points, n the power
    of two at least length + K, cut at d."""
    if length == 0:
        return np.zeros(0, dtype=np.float32)
    K = h.shape[0]
    n = 1 << (length + K - 1).bit_length()
    xs, hs = torch.from_numpy(np.ascontiguousarray(x[:length], dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32))
    full = torch.fft.irfft(torch.fft.rfft(xs, n) * torch.fft.rfft(hs, n), n).numpy()[:length + K - 1]
    at = np.arange(length, dtype=np.int64) + d
    return np.where((at >= 0) & (at < full.shape[0]), full[np.clip(at, 0, full.shape[0] - 1)], np.float32(0.0))


def bound(x, length, h, d):
    """The derived worst case of include/eec.h for one utterance: (14 log2 N + P + 8) 2^-24 ||h||_1 max_j ||x_j||_2, x_j the N-sample
    windows x[(j - 1) S + d, (j + 1) S + d) (zeros outside [0, length)).  Forward and inverse transform 7 u log2 N each (Higham Thm
    24.2 with fp32 twiddles rounded from fp64), one rounding of H, the complex product, P - 1 accumulations."""
    K = h.shape[0]
    P = -(-K // S)
    x64 = np.asarray(x[:length], dtype=np.float64)
    worst = 0.0
    for j in range(-P, -(-length // S) + 1):
        lo, hi = max((j - 1) * S + d, 0), min((j + 1) * S + d, length)
        if hi > lo:
            worst = max(worst, float(np.sqrt(np.sum(x64[lo:hi] ** 2))))
    return (14 * math.log2(N) + P + 8) * 2.0 ** -24 * float(np.sum(np.abs(np.asarray(h, dtype=np.float64)))) * worst


class Pair:
    """One compared (RIR, utterance) pair: the fp64 result, the error of the independent fp32 FFT and the derived bound."""

    def __init__(self, x, length, h, d):
        self.y = conv_fp64(x, length, h, d)
        self.e_ref = float(np.max(np.abs(fft32(x, length, h, d).astype(np.float64) - self.y))) if length else 0.0
        self.bound = bound(x, length, h, d)
        self.peak = float(np.max(np.abs(self.y))) if length else 0.0

    def error(self, got):
        return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - self.y))) if self.y.shape[0] else 0.0


_PAIRS = {}


def pairs_of(key, records, rows):
    """{(r, b): Pair} for the pairs ``rows`` names (utterance b against RIR rows[s][b]) of the bank ``records`` = [(d, taps)]; computed
    once per ``key`` and shared by the tests, never written."""
    if key not in _PAIRS:
        x = wave_batch()
        got = {}
        for row in rows:
            for b, r in enumerate(row):
                if (r, b) not in got and 0 <= r < len(records):
                    d, taps = records[r]
                    got[(r, b)] = Pair(x[b], LENGTHS[b], np.asarray(taps), int(d))
        _PAIRS[key] = got
    return _PAIRS[key]


def judge(pairs, outputs, what):
    """``outputs`` {(r, b): fp32 [length]} against the pairs: every output inside the derived bound; per RIR, the worst error over its
    compared utterances at most MARGIN times the worst error of the independent fp32 FFT over the same utterances.  Prints the ratio
    per RIR; returns (worst ratio, worst share of the derived bound, {r: worst error / max |y|})."""
    by_rir = {}
    worst_share = 0.0
    for (r, b), pair in sorted(pairs.items()):
        err = pair.error(outputs[(r, b)])
        assert not np.isnan(outputs[(r, b)]).any(), (what, r, b)
        if pair.bound > 0.0:
            assert err <= pair.bound, (what, r, b, err, pair.bound)
            worst_share = max(worst_share, err / pair.bound)
        else:
            assert err == 0.0, (what, r, b, err)
        e, ref, peak = by_rir.get(r, (0.0, 0.0, 0.0))
        by_rir[r] = (max(e, err), max(ref, pair.e_ref), max(peak, pair.peak))
    worst, rel = 0.0, {}
    for r, (e, ref, peak) in sorted(by_rir.items()):
        ratio = e / ref if ref > 0.0 else (0.0 if e == 0.0 else math.inf)
        rel[r] = e / peak if peak > 0.0 else 0.0
        print(f"{what}: RIR {r}: error {e:.3e} = {ratio:.3f} of e_ref {ref:.3e}; {rel[r]:.2e} of max |y|")
        worst = max(worst, ratio)
    for r, (e, ref, peak) in by_rir.items():
        assert e <= MARGIN * ref, (what, r, e, ref)
    print(f"{what}: worst ratio to e_ref {worst:.3f} (margin {MARGIN}), worst share of the derived bound {worst_share:.2e}")
    return worst, worst_share, rel
