"""SpecAugment on the device: the stage between the mel front end and the encoder in training (include/eec.h, "SpecAugment";
csrc/specaug.hip).

* ``spec_augment``   time warp, frequency masks and time masks of a mel batch ``[B, n_mels, T]``: one launch that draws a row of
  integer parameters per utterance from ``(seed, utt_offset + b)`` (the dropout generator, counter-based) and one that applies them
  -- or rows the caller prescribes.  No host synchronisation, graph-capturable.  CPU tensors take a host path that is the same
  statement in NumPy.
* ``SpecAugment``    the module form: identity in eval mode, fresh parameters every call in train mode, a resumable call counter.

The warp is ``F.interpolate(align_corners=False)`` of the frames left and right of a drawn centre, separately (ESPnet's and lhotse's
``time_warp``), bicubic or linear; frames at or past an utterance's length are copied through and never read.  Out of scope: speed
perturbation, mean-value fill, a backward (the input is data)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import capi

MAX_FREQ_MASKS, MAX_TIME_MASKS = 8, 16  # EEC_SPECAUG_MAX_FREQ_MASKS, EEC_SPECAUG_MAX_TIME_MASKS
SITE = 0x53504341                       # EEC_SPECAUG_SITE
MODES = {"linear": 0, "bicubic": 1}     # EEC_SPECAUG_LINEAR, EEC_SPECAUG_BICUBIC
_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# host path: the statement of include/eec.h in NumPy
# ---------------------------------------------------------------------------------------------------------------------------
def _key(seed: int, site: int) -> int:
    x = ((seed & _M64) * 0x9E3779B97F4A7C15 + ((site << 32) | site)) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return ((x >> 32) ^ x) & 0xFFFFFFFF


def _words(key: int, index: np.ndarray) -> np.ndarray:
    """lowbias32 of the keyed 64-bit index -> uint32."""
    with np.errstate(over="ignore"):
        h = (index & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1) + \
            (index >> np.uint64(32)).astype(np.uint32) * np.uint32(0x85EBCA77) + np.uint32(key)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    return h


def _host_draw(n: np.ndarray, n_mels: int, seed: int, utt_offset: int, W: int, n_freq: int, F: int, n_time: int, ratio: float,
               Tmax: int) -> np.ndarray:
    """``params`` int32 [B, P] of utterances of ``n`` [B] (clamped) frames."""
    B = n.shape[0]
    key = _key(seed, SITE)
    with np.errstate(over="ignore"):
        at = (np.arange(B, dtype=np.uint64) + np.uint64(utt_offset & _M64)) * np.uint64(64)

    def below(slot: int, m: np.ndarray) -> np.ndarray:
        with np.errstate(over="ignore"):
            u = _words(key, at + np.uint64(slot)).astype(np.uint64)
        return ((u * m.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)

    n = n.astype(np.int64)
    p = np.zeros((B, 2 + 2 * n_freq + 2 * n_time), dtype=np.int64)
    on = (n > 2 * W) if W > 0 else np.zeros(B, dtype=bool)
    c = W + below(0, np.where(on, n - 2 * W, 1))
    w = c - W + 1 + below(1, np.full(B, max(2 * W, 1)))
    p[:, 0], p[:, 1] = np.where(on, c, 0), np.where(on, w, 0)
    for k in range(n_freq):
        fw = below(2 + 2 * k, np.full(B, min(F, n_mels) + 1))
        p[:, 2 + 2 * k], p[:, 3 + 2 * k] = below(3 + 2 * k, n_mels - fw + 1), fw
    cap = np.floor(float(np.float32(ratio)) * n.astype(np.float64))
    most = np.minimum(Tmax, np.minimum(cap, n.astype(np.float64)).astype(np.int64))
    for k in range(n_time):
        slot = 2 + 2 * n_freq + 2 * k
        tw = below(slot, most + 1)
        p[:, slot], p[:, slot + 1] = below(slot + 1, n - tw + 1), tw
    return p.astype(np.int32)


def _host_taps(n: int, c: int, w: int, cubic: bool):
    """Tap indices int64 [K, n] and fp32 weights [K, n] of the output frames 0 .. n - 1 of a warped utterance."""
    t = np.arange(n, dtype=np.int64)
    right = t >= w
    d, n_in, n_out, base = np.where(right, t - w, t), np.where(right, n - c, c), np.where(right, n - w, w), np.where(right, c, 0)
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    if not cubic:
        num = np.maximum(num, 0)
    i = num // den
    f = (num - i * den).astype(np.float64) / den.astype(np.float64)
    if cubic:
        idx = [base + np.clip(i - 1 + k, 0, n_in - 1) for k in range(4)]
        k1 = lambda x: (1.25 * x - 2.25) * x * x + 1.0            # noqa: E731
        k2 = lambda x: ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0   # noqa: E731
        wt = [k2(f + 1.0), k1(f), k1(1.0 - f), k2(2.0 - f)]
    else:
        idx = [base + i, base + np.minimum(i + 1, n_in - 1)]
        wt = [1.0 - f, f]
    return np.stack(idx), np.stack(wt).astype(np.float32)


def _in_masks(m: np.ndarray, limit: int, size: int) -> np.ndarray:
    """bool [size]: the positions inside one of the (start, width) rows of ``m``, each clipped to [0, limit)."""
    x = np.arange(size, dtype=np.int64)
    hit = np.zeros(size, dtype=bool)
    for s, width in m.astype(np.int64):
        hit |= (x >= max(s, 0)) & (x < min(s + width, limit))
    return hit


def _host_apply(mel: np.ndarray, n_all: np.ndarray, params: np.ndarray, n_freq: int, n_time: int, cubic: bool, mask_value: float) -> np.ndarray:
    B, n_mels, T = mel.shape
    out = mel.copy()
    for b in range(B):
        n, (c, w) = int(n_all[b]), (int(v) for v in params[b, :2])
        if 1 <= c <= n - 1 and 1 <= w <= n - 1:
            idx, wt = _host_taps(n, c, w, cubic)
            acc = wt[0] * mel[b][:, idx[0]]
            for k in range(1, idx.shape[0]):
                acc = acc + wt[k] * mel[b][:, idx[k]]
            out[b, :, :n] = acc
        rows = _in_masks(params[b, 2:2 + 2 * n_freq].reshape(n_freq, 2), n_mels, n_mels)
        frames = _in_masks(params[b, 2 + 2 * n_freq:].reshape(n_time, 2), n, n)
        out[b, :, :n][rows[:, None] | frames[None, :]] = np.float32(mask_value)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------------------------------------------------
def spec_augment(mel: Tensor, frame_len: Optional[Tensor] = None, *, seed: int, utt_offset: int = 0, params: Optional[Tensor] = None,
                 time_warp_window: int = 5, time_warp_mode: str = "bicubic", n_freq_masks: int = 2, freq_mask_width: int = 27,
                 n_time_masks: int = 5, time_mask_ratio: float = 0.05, time_mask_width: Optional[int] = None,
                 mask_value: float = 0.0) -> Tuple[Tensor, Tensor]:
    """``(out, params)``: the augmented copy of ``mel`` [B, n_mels, T] (fp32; what ``MelFrontend`` returns and the models take) and the
    int32 ``[B, 2 + 2 * n_freq_masks + 2 * n_time_masks]`` parameters it was made with -- ``c, w`` of the warp, ``f0, fw`` per frequency
    mask, ``t0, tw`` per time mask.  ``frame_len`` [B]: valid frames per utterance, clamped to [0, T]; None: T.  Frames at or past
    a length are copied through bit for bit and never read.

    ``params`` None: drawn from ``(seed, utt_offset + b)`` -- a warp centre at least ``time_warp_window`` frames from both ends moved
    by less than that (none for utterances of at most twice the window), frequency masks of up to ``freq_mask_width`` rows, time masks
    of up to ``time_mask_ratio`` of the utterance and ``time_mask_width`` frames (None: no cap) -- so a call on a slice of the batch with
    ``utt_offset`` advanced returns the rows of the whole call.  Given: applied as they are, clipped to the utterance; a warp outside
    ``1 <= c, w <= n - 1`` is ignored.  The defaults are the customary LibriSpeech Conformer recipe values, a choice rather than a
    measurement.  Masked elements become ``mask_value`` (0.0: the collate's padding, silence for an un-logged power spectrum)."""
    if not isinstance(mel, Tensor) or mel.dim() != 3 or mel.dtype != torch.float32:
        raise ValueError(f"spec_augment: mel must be an fp32 tensor [B, n_mels, T], got {getattr(mel, 'dtype', None)} {tuple(getattr(mel, 'shape', ()))}")
    B, n_mels, T = mel.shape
    if n_mels < 1 or T < 1:
        raise ValueError(f"spec_augment: n_mels and T must be positive, got {n_mels} and {T}")
    if time_warp_mode not in MODES:
        raise ValueError(f"spec_augment: time_warp_mode must be 'bicubic' or 'linear', got {time_warp_mode!r}")
    n_freq, n_time = int(n_freq_masks), int(n_time_masks)
    if not 0 <= n_freq <= MAX_FREQ_MASKS or not 0 <= n_time <= MAX_TIME_MASKS:
        raise ValueError(f"spec_augment: at most {MAX_FREQ_MASKS} frequency and {MAX_TIME_MASKS} time masks, got {n_freq} and {n_time}")
    W, F = int(time_warp_window), int(freq_mask_width)
    Tmax = T if time_mask_width is None else min(int(time_mask_width), T)
    ratio, mask_value = float(time_mask_ratio), float(mask_value)
    if W < 0 or F < 0 or Tmax < 0:
        raise ValueError("spec_augment: time_warp_window, freq_mask_width and time_mask_width must not be negative")
    if not 0.0 <= ratio <= float(np.finfo(np.float32).max):  # the C ABI takes it as fp32
        raise ValueError(f"spec_augment: time_mask_ratio must be finite and not negative, got {time_mask_ratio}")
    if math.isnan(mask_value):
        raise ValueError("spec_augment: mask_value is NaN")
    dev = mel.device
    mel = mel.contiguous()
    P = 2 + 2 * n_freq + 2 * n_time
    if frame_len is not None:
        if not isinstance(frame_len, Tensor) or frame_len.shape != (B,) or frame_len.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"spec_augment: frame_len must be an int32 or int64 tensor of {B} entries")
        frame_len = capi.to_device(frame_len, dev, frame_len.dtype).clamp(0, T).to(torch.int32).contiguous()
    if params is not None:
        if not isinstance(params, Tensor) or params.shape != (B, P) or params.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"spec_augment: params must be an int32 or int64 tensor [{B}, {P}]")
        lim = (1 << 31) - 1  # anything beyond int32 is as far outside every axis as the limit itself
        params = params.to(dev).clamp(-lim, lim).to(torch.int32).contiguous()
    seed, utt_offset = int(seed) & _M64, int(utt_offset) & _M64

    if not mel.is_cuda:
        n = np.full(B, T, dtype=np.int64) if frame_len is None else frame_len.numpy().astype(np.int64)
        if params is None:
            params = torch.from_numpy(_host_draw(n, n_mels, seed, utt_offset, W, n_freq, F, n_time, ratio, Tmax))
        out = _host_apply(mel.numpy(), n, params.numpy(), n_freq, n_time, time_warp_mode == "bicubic", mask_value)
        return torch.from_numpy(out), params

    lib = capi.load()
    fl_ptr = None if frame_len is None or B == 0 else frame_len.data_ptr()
    out = torch.empty_like(mel)
    with torch.cuda.device(dev):
        if params is None:
            params = torch.empty((B, P), dtype=torch.int32, device=dev)
            capi.check(lib.eec_specaug_draw(fl_ptr, B, n_mels, T, seed, utt_offset, W, n_freq, F, n_time, ratio, Tmax, params.data_ptr(),
                                            capi.stream_ptr(dev)), "eec_specaug_draw")
        capi.check(lib.eec_specaug_apply(mel.data_ptr(), fl_ptr, params.data_ptr(), B, n_mels, T, n_freq, n_time, MODES[time_warp_mode],
                                         mask_value, out.data_ptr(), capi.stream_ptr(dev)), "eec_specaug_apply")
    return out, params


class SpecAugment(nn.Module):
    """``mel = aug(mel, frames)`` between the front end and the model: ``spec_augment`` with the arguments given here in train mode,
    the input itself in eval mode.  Call k (``get_state()["calls"]``, advanced by every train-mode call) draws from the seed
    ``seed + k * 0x9E3779B97F4A7C15`` (mod 2^64), so every step has fresh parameters and ``set_state`` on resuming reproduces the
    steps that follow.  ``seed`` None: one from torch's CPU generator (``torch.manual_seed`` fixes it).  ``last_params`` holds the
    parameters of the last train-mode call.  No parameters, no buffers: a model's ``state_dict`` is not touched."""

    def __init__(self, seed: Optional[int] = None, time_warp_window: int = 5, time_warp_mode: str = "bicubic", n_freq_masks: int = 2,
                 freq_mask_width: int = 27, n_time_masks: int = 5, time_mask_ratio: float = 0.05, time_mask_width: Optional[int] = None,
                 mask_value: float = 0.0):
        super().__init__()
        if time_warp_mode not in MODES:
            raise ValueError(f"SpecAugment: time_warp_mode must be 'bicubic' or 'linear', got {time_warp_mode!r}")
        self.seed = capi.new_seed() if seed is None else int(seed)
        self.kwargs = dict(time_warp_window=time_warp_window, time_warp_mode=time_warp_mode, n_freq_masks=n_freq_masks,
                           freq_mask_width=freq_mask_width, n_time_masks=n_time_masks, time_mask_ratio=time_mask_ratio,
                           time_mask_width=time_mask_width, mask_value=mask_value)
        self.calls = 0
        self.last_params: Optional[Tensor] = None

    def get_state(self) -> Dict[str, int]:
        return {"seed": self.seed, "calls": self.calls}

    def set_state(self, state: Dict[str, int]) -> None:
        self.seed, self.calls = int(state["seed"]), int(state["calls"])

    def forward(self, mel: Tensor, lengths: Optional[Tensor] = None, utt_offset: int = 0) -> Tensor:
        if not self.training:
            return mel
        seed = (self.seed + self.calls * 0x9E3779B97F4A7C15) & _M64
        self.calls += 1
        out, self.last_params = spec_augment(mel, lengths, seed=seed, utt_offset=utt_offset, **self.kwargs)
        return out

    def extra_repr(self) -> str:
        return ", ".join(f"{k}={v!r}" for k, v in self.kwargs.items())
