"""torch-CPU restatements of the reference's mel front end, fp32 and float64 (the oracles for csrc/frontend.hip).

TEST INFRASTRUCTURE -- see oracle/__init__.py for who may import this.

Reference: util/data_loader.py:7-18
    spec = torchaudio.transforms.Spectrogram(n_fft=args.n_fft * 2, hop_length=args.hop_length, win_length=args.win_length)(wave)
    mel  = torchaudio.transforms.MelScale(sample_rate=args.sample_rate, n_mels=args.n_mels, n_stft=args.n_fft + 1)(spec)
with util/conf.py defaults n_fft 512 (-> a 1024-point transform, 513 bins), win_length 320, hop_length 160, 80 mel bins,
16 kHz.  torchaudio is a third-party dependency that is NOT in the reference tree and not installed here (version
unpinned): both transforms are restated from their published definitions --

* ``Spectrogram`` defaults: hann window (periodic), power 2, not normalised, center=True with reflect padding, one-sided:
  ``|torch.stft(wave, n_fft, hop, win_length, window=hann(win_length), center=True, pad_mode="reflect")| ** 2``.
* ``MelScale`` defaults: f_min 0, f_max sample_rate // 2, norm None, mel_scale "htk":
  ``melscale_fbanks``: triangular filters between points equally spaced on m = 2595 log10(1 + f / 700).

Parity unpinned by the reference (it holds no vectors for the front end); torch.stft is the installed torch's kernel.

``mel_frontend`` is that fp32 statement.  ``mel_frontend_fp64`` states the same transform in float64 without an FFT and without
a padded copy of the wave (frames gathered by index, a direct DFT as two matrix products); it is what the kernel and the fp32
statement are both measured against, and it pins the one case torch leaves open: an utterance of n_fft // 2 samples or fewer,
where torch's reflect padding raises and the device front end reflects once and then clamps.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
from torch import Tensor


@functools.lru_cache(maxsize=None)
def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> Tensor:
    """[n_freqs, n_mels] triangular filterbank, htk mel scale, no area normalisation.  One table per setting, shared by every
    caller: read it, do not write to it."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0)


def mel_frontend(wave: Tensor, sample_rate: int = 16000, n_fft: int = 512, win_length: int = 320, hop_length: int = 160,
                 n_mels: int = 80) -> Tensor:
    """wave [L] or [B, L] fp32 -> power mel [n_mels, T] / [B, n_mels, T], T = 1 + L // hop (un-logged, as the reference)."""
    nfft = 2 * n_fft
    spec = torch.stft(wave, nfft, hop_length, win_length, window=torch.hann_window(win_length), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True).abs().pow(2.0)
    fb = melscale_fbanks(nfft // 2 + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate)
    return torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)


def mel_frontend_batch(wave: Tensor, lengths: Tensor, **kw) -> Tensor:
    """Per-utterance front end + zero padding to the longest, as the reference's collate does (data_loader.py:20-26,
    pad_sequence with 0): wave [B, Lmax], lengths [B] -> [B, n_mels, 1 + Lmax // hop]."""
    hop = kw.get("hop_length", 160)
    outs = [mel_frontend(wave[b, : int(lengths[b])], **kw) for b in range(wave.size(0))]
    T = max(o.size(1) for o in outs)
    out = torch.zeros(wave.size(0), outs[0].size(0), T)
    for b, o in enumerate(outs):
        out[b, :, : o.size(1)] = o
    return out


def frame_indices(n_samples: int, win_length: int = 320, hop_length: int = 160) -> np.ndarray:
    """[T, win] sample index read by slot j of frame t: hop t - win / 2 + j, reflected once at either end (-idx below 0,
    2 (L - 1) - idx at or above L; no edge repeat) and then clamped to [0, L - 1].  T = 1 + L // hop, 0 frames for L <= 0.
    For L > n_fft // 2 this is torch's centred reflect padding restricted to the samples under the window."""
    L = int(n_samples)
    T = 1 + L // hop_length if L > 0 else 0
    idx = hop_length * np.arange(T, dtype=np.int64)[:, None] - win_length // 2 + np.arange(win_length, dtype=np.int64)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= L, 2 * (L - 1) - idx, idx)
    return np.clip(idx, 0, max(L - 1, 0))


def hann_fp64(win_length: int = 320) -> np.ndarray:
    """Periodic hann window, float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)


def power_spectrum_fp64(wave, n_fft: int = 512, win_length: int = 320, hop_length: int = 160) -> np.ndarray:
    """wave [L] -> [T, n_fft + 1] float64 power of the (2 n_fft)-point transform of the centred, hann-windowed frames: a direct
    DFT over the win_length samples under the window (the window's offset inside the frame is a unit-modulus phase)."""
    x = np.asarray(wave, dtype=np.float64).reshape(-1)
    nfft = 2 * n_fft
    idx = frame_indices(x.shape[0], win_length, hop_length)
    if idx.shape[0] == 0:
        return np.zeros((0, n_fft + 1))
    frames = x[idx] * hann_fp64(win_length)[None, :]
    kj = (np.arange(win_length, dtype=np.int64)[:, None] * np.arange(n_fft + 1, dtype=np.int64)[None, :]) % nfft
    ang = 2.0 * np.pi * kj.astype(np.float64) / nfft
    re, im = frames @ np.cos(ang), frames @ np.sin(ang)
    return re * re + im * im


def mel_frontend_fp64(wave, sample_rate: int = 16000, n_fft: int = 512, win_length: int = 320, hop_length: int = 160,
                      n_mels: int = 80) -> Tensor:
    """wave [L] (any real dtype) -> float64 power mel [n_mels, T], T = 1 + L // hop (0 frames for L = 0).  The filter table is
    ``melscale_fbanks`` (torch's fp32 table, which is the reference's) cast to float64."""
    P = power_spectrum_fp64(wave.detach().cpu().numpy() if isinstance(wave, Tensor) else wave, n_fft, win_length, hop_length)
    fb = melscale_fbanks(n_fft + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate).double().numpy()
    return torch.from_numpy(np.ascontiguousarray((P @ fb).T))


def mel_frontend_fp64_batch(wave, lengths=None, **kw) -> Tensor:
    """The float64 front end per utterance + the collate's zero padding: wave [B, Lmax], lengths [B] (None: Lmax for all;
    a length is taken into [0, Lmax]) -> float64 [B, n_mels, 1 + Lmax // hop]."""
    hop = kw.get("hop_length", 160)
    B, Lmax = wave.shape
    lens = [Lmax] * B if lengths is None else [min(max(int(l), 0), Lmax) for l in lengths]
    out = torch.zeros(B, kw.get("n_mels", 80), 1 + Lmax // hop if Lmax > 0 else 0, dtype=torch.float64)
    for b in range(B):
        o = mel_frontend_fp64(wave[b, : lens[b]], **kw)
        out[b, :, : o.size(1)] = o
    return out
