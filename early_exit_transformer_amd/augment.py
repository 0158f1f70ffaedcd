"""Augmentation on the device: SpecAugment between the mel front end and the encoder (include/eec.h, "SpecAugment";
csrc/specaug.hip), speed perturbation / resampling in front of the mel front end (include/eec.h, "Resampling / speed perturbation";
csrc/resample.hip) and, between the two, reverberation, additive noise and volume perturbation of the waveform (include/eec.h,
"Waveform augmentation: reverberation, noise, volume"; csrc/waveaug.hip).

* ``spec_augment``   time warp, frequency masks and time masks of a mel batch ``[B, n_mels, T]``: one launch that draws a row of
  integer parameters per utterance from ``(seed, utt_offset + b)`` (the dropout generator, counter-based) and one that applies them
  -- or rows the caller prescribes.  No host synchronisation, graph-capturable.  CPU tensors take a host path that is the same
  statement in NumPy.
* ``SpecAugment``    the module form: identity in eval mode, fresh parameters every call in train mode, a resumable call counter.
* ``resample``       polyphase sinc resampling (Hann window) of a waveform batch ``[B, L]`` from one sample rate to another:
  torchaudio's ``functional.resample``, every utterance as if resampled alone and padded afterwards.
* ``speed_perturb``  the same kernel with one ratio per utterance, drawn from ``(seed, utt_offset + b)`` among ``factors`` or
  prescribed: torchaudio's ``transforms.Speed``.  ``SpeedPerturb`` is its module form, built like ``SpecAugment``.
* ``wave_augment``   Kaldi's ``wav-reverberate`` order on a waveform batch: convolution with a room impulse response of a ``RirBank``
  (the direct path stays in place, the length does not change), a tiled noise row of a ``NoiseBank`` added at a signal-to-noise ratio
  drawn among ``snrs``, a volume gain; every stage switched per utterance by a row drawn from ``(seed, utt_offset + b)`` or
  prescribed.  ``reverberate`` and ``add_noise`` are the prescribed single stages, ``WaveAugment`` the module form.

The chain of a training step: ``wave, n = speed(wave, n); wave = waveaug(wave, n); mel = frontend(wave, n); mel = specaug(mel, frames)``.

The warp is ``F.interpolate(align_corners=False)`` of the frames left and right of a drawn centre, separately (ESPnet's and lhotse's
``time_warp``), bicubic or linear; frames at or past an utterance's length are copied through and never read.  Out of scope:
mean-value fill, ``sinc_interp_kaiser``, tempo change without pitch change, reverberated point-source noises, babble, codec and
clipping effects, FFT convolution, a backward (the input is data)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

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

    fl = None if B == 0 else frame_len
    out = torch.empty_like(mel)
    if params is None:
        params = torch.empty((B, P), dtype=torch.int32, device=dev)
        capi.launch("eec_specaug_draw", dev, fl, B, n_mels, T, seed, utt_offset, W, n_freq, F, n_time, ratio, Tmax, params)
    capi.launch("eec_specaug_apply", dev, mel, fl, params, B, n_mels, T, n_freq, n_time, MODES[time_warp_mode], mask_value, out)
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


# ---------------------------------------------------------------------------------------------------------------------------
# resampling and speed perturbation
# ---------------------------------------------------------------------------------------------------------------------------
RESAMPLE_MAX_RATIOS, RESAMPLE_MAX_RATE, RESAMPLE_MAX_LPW = 8, 640, 64  # EEC_RESAMPLE_MAX_RATIOS, _MAX_RATE, _MAX_LPW
RESAMPLE_MAGIC = 0x52534D50                                             # EEC_RESAMPLE_MAGIC
SPEED_SITE = 0x53504545                                                 # EEC_SPEED_SITE
MAX_SAMPLES = 1 << 30


class ResamplePlan:
    """The image ``eec_resample_plan`` builds for ``ratios`` (include/eec.h has the layout): ``image`` int32 on the host, ``ratios``
    reduced, ``on(device)`` the uploaded copy, made once per device."""

    def __init__(self, ratios: Sequence[Tuple[int, int]], lowpass_filter_width: int, rolloff: float):
        lib = capi.load()
        R = len(ratios)
        orig, new = (C.c_int32 * R)(*[o for o, _ in ratios]), (C.c_int32 * R)(*[n for _, n in ratios])
        nbytes = lib.eec_resample_plan_bytes(R, orig, new, lowpass_filter_width, rolloff)
        if nbytes == 0:
            raise ValueError(lib.eec_last_error().decode(errors="replace"))
        self.image = np.zeros(nbytes // 4, dtype=np.int32)
        capi.call("eec_resample_plan", R, orig, new, lowpass_filter_width, rolloff, self.image.ctypes.data, nbytes)
        self.ratios = [(int(self.image[4 + 8 * r]), int(self.image[5 + 8 * r])) for r in range(R)]
        self._dev: Dict[torch.device, Tensor] = {}

    def on(self, dev: torch.device) -> Tensor:
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = torch.from_numpy(self.image).to(dev)
        return t

    def out_samples(self, L: int) -> int:
        """The width that holds every utterance of ``L`` samples under every ratio."""
        return max((n * L + o - 1) // o for o, n in self.ratios)

    def table(self, r: int):
        """``(o, n, width, K, first [n], count [n], weights: n fp32 arrays)`` of ratio ``r``."""
        o, n, width, K, phases, weights = (int(v) for v in self.image[4 + 8 * r:10 + 8 * r])
        ph = self.image[phases:phases + 3 * n].reshape(n, 3)
        w = self.image[weights:].view(np.float32)
        return o, n, width, K, ph[:, 0].copy(), ph[:, 1].copy(), [w[a:a + c] for _, c, a in ph]


_plans: Dict[tuple, ResamplePlan] = {}


def resample_plan(ratios: Sequence[Tuple[int, int]], lowpass_filter_width: int = 6, rolloff: float = 0.99) -> ResamplePlan:
    """The cached plan of ``ratios`` [(orig, new), ...]; ``ValueError`` for what the library refuses."""
    if isinstance(lowpass_filter_width, bool) or int(lowpass_filter_width) != lowpass_filter_width or \
            not 1 <= int(lowpass_filter_width) <= RESAMPLE_MAX_LPW:
        raise ValueError(f"resample: lowpass_filter_width must be an integer in [1, {RESAMPLE_MAX_LPW}], got {lowpass_filter_width!r}")
    rolloff = float(rolloff)
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"resample: rolloff must lie in (0, 1], got {rolloff}")
    if not 1 <= len(ratios) <= RESAMPLE_MAX_RATIOS:
        raise ValueError(f"resample: between 1 and {RESAMPLE_MAX_RATIOS} ratios per call, got {len(ratios)}")
    red = []
    for o, n in ratios:
        if int(o) != o or int(n) != n or o < 1 or n < 1:
            raise ValueError(f"resample: sample rates must be positive integers, got {o!r} and {n!r}")
        g = math.gcd(int(o), int(n))
        if max(int(o), int(n)) // g > RESAMPLE_MAX_RATE:
            raise ValueError(f"resample: ratio {int(o) // g} / {int(n) // g} exceeds {RESAMPLE_MAX_RATE} after reduction")
        red.append((int(o) // g, int(n) // g))
    key = (tuple(red), int(lowpass_filter_width), rolloff)
    plan = _plans.get(key)
    if plan is None:
        if len(_plans) > 15:
            _plans.clear()
        plan = _plans[key] = ResamplePlan(red, int(lowpass_filter_width), rolloff)
    return plan


def speed_ratios(factors: Sequence[float], sample_rate: int) -> list:
    """``(int(f * sample_rate), sample_rate)`` per factor, as ``torchaudio.transforms.Speed`` computes it."""
    if len(factors) == 0:
        raise ValueError("speed_perturb: factors is empty")
    if int(sample_rate) != sample_rate or sample_rate < 1:
        raise ValueError(f"speed_perturb: sample_rate must be a positive integer, got {sample_rate!r}")
    out = []
    for f in factors:
        if not (isinstance(f, (int, float)) and math.isfinite(f) and f > 0 and int(f * sample_rate) >= 1):
            raise ValueError(f"speed_perturb: a factor must be positive and finite, got {f!r}")
        out.append((int(f * sample_rate), int(sample_rate)))
    return out


def _host_choice(seed: int, utt_offset: int, B: int, R: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        at = (np.arange(B, dtype=np.uint64) + np.uint64(utt_offset & _M64)) * np.uint64(64)
    u = _words(_key(seed, SPEED_SITE), at).astype(np.uint64)
    return ((u * np.uint64(R)) >> np.uint64(32)).astype(np.int32)


def _host_resample(wave: np.ndarray, n_all: np.ndarray, choice: np.ndarray, plan: ResamplePlan, L_out: int):
    """The statement in NumPy: per phase, the taps in order, one fp32 multiply and one fp32 add each."""
    B = wave.shape[0]
    out, out_len = np.zeros((B, L_out), dtype=np.float32), np.zeros(B, dtype=np.int64)
    tables: Dict[int, tuple] = {}
    for b in range(B):
        length, c = int(n_all[b]), int(choice[b])
        if not 0 <= c < len(plan.ratios) or plan.ratios[c] == (1, 1):
            out_len[b] = min(length, L_out)
            out[b, :out_len[b]] = wave[b, :out_len[b]]
            continue
        o, n, width, K, first, count, weights = tables.setdefault(c, plan.table(c))
        m = out_len[b] = min((n * length + o - 1) // o, L_out)
        if m == 0:
            continue
        x = np.zeros(((m - 1) // n + 1) * o + K, dtype=np.float32)  # x[g + width] = sample g; zeros outside [0, length)
        x[width:width + length] = wave[b, :length]
        for j in range(min(n, m)):
            start = np.arange((m - 1 - j) // n + 1, dtype=np.int64) * o + int(first[j])
            acc = np.zeros(start.shape[0], dtype=np.float32)
            for k in range(int(count[j])):
                acc = acc + weights[j][k] * x[start + k]
            out[b, j:m:n] = acc
    return out, out_len


def _resample_with(who: str, wave: Tensor, lengths: Optional[Tensor], plan_of, choice, seed: int, utt_offset: int):
    """Checks, then the host path or the launches.  ``plan_of()`` builds the plan once the tensors are known to be sound; ``choice``
    None: drawn; an integer: that ratio for every utterance."""
    if not isinstance(wave, Tensor) or wave.dim() not in (1, 2) or wave.dtype != torch.float32:
        raise ValueError(f"{who}: wave must be an fp32 tensor [B, L] or [L], got {getattr(wave, 'dtype', None)} {tuple(getattr(wave, 'shape', ()))}")
    squeeze = wave.dim() == 1
    if squeeze:
        wave = wave.unsqueeze(0)
    B, L = wave.shape
    if L > MAX_SAMPLES:
        raise ValueError(f"{who}: at most 2^30 samples per utterance, got {L}")
    dev = wave.device
    wave = wave.contiguous()
    if lengths is not None:
        if not isinstance(lengths, Tensor) or lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != B or lengths.dim() > 1:
            raise ValueError(f"{who}: lengths must be an int32 or int64 tensor of {B} entries")
        lengths = capi.to_device(lengths.reshape(B), dev, torch.int64).clamp(0, L).contiguous()
    if isinstance(choice, int):
        choice = torch.full((B,), choice, dtype=torch.int32, device=dev)
    elif choice is not None:
        if not isinstance(choice, Tensor) or choice.dtype not in (torch.int32, torch.int64) or choice.numel() != B or choice.dim() > 1:
            raise ValueError(f"{who}: choice must be an int32 or int64 tensor of {B} entries")
        choice = choice.reshape(B).to(dev).clamp(-1, RESAMPLE_MAX_RATIOS).to(torch.int32).contiguous()  # outside the plan: a copy
    plan = plan_of()
    R, L_out = len(plan.ratios), plan.out_samples(L)
    if L_out >= 1 << 31:
        raise ValueError(f"{who}: {L} samples grow to {L_out}, past 2^31 - 1")

    if not wave.is_cuda:
        n = np.full(B, L, dtype=np.int64) if lengths is None else lengths.numpy()
        if choice is None:
            choice = torch.from_numpy(_host_choice(seed, utt_offset, B, R))
        out, out_len = _host_resample(wave.numpy(), n, choice.numpy(), plan, L_out)
        out, out_len = torch.from_numpy(out), torch.from_numpy(out_len)
    else:
        image = plan.on(dev)
        lens = None if B == 0 else lengths
        out = torch.empty((B, L_out), dtype=torch.float32, device=dev)
        out_len = torch.empty((B,), dtype=torch.int64, device=dev)
        if choice is None:
            choice = torch.empty((B,), dtype=torch.int32, device=dev)
            capi.launch("eec_speed_draw", dev, lens, B, L, seed, utt_offset, image, choice, out_len)
        capi.launch("eec_resample", dev, wave, lens, choice, B, L, image, out, L_out, out_len)
    return (out[0], out_len[0], choice[0]) if squeeze else (out, out_len, choice)


def resample(wave: Tensor, lengths: Optional[Tensor] = None, *, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
             rolloff: float = 0.99) -> Tuple[Tensor, Tensor]:
    """``(out, out_len)``: ``wave`` [B, L] or [L] (fp32) resampled from ``orig_freq`` to ``new_freq`` -- torchaudio's
    ``functional.resample`` with ``sinc_interp_hann`` -- as ``out`` [B, ceil(new * L / orig)] and the int64 lengths
    ``ceil(new * lengths / orig)`` (what ``MelFrontend`` takes).  ``lengths`` [B]: valid samples, clamped to [0, L]; None: L.  Samples
    at or past a length are never read, outputs at or past an ``out_len`` are 0.0: every utterance comes out as if resampled alone
    and padded afterwards.  Equal rates return a copy.  The reduced ratio may not exceed 640 on either side (8 / 16 / 22.05 / 24 / 32 /
    44.1 / 48 kHz pairs all fit).  No host synchronisation; a CPU tensor takes the NumPy host path, bit-identical for finite input."""
    out, out_len, _ = _resample_with("resample", wave, lengths, lambda: resample_plan([(orig_freq, new_freq)], lowpass_filter_width, rolloff), 0, 0, 0)
    return out, out_len


def speed_perturb(wave: Tensor, lengths: Optional[Tensor] = None, *, seed: int, utt_offset: int = 0,
                  factors: Sequence[float] = (0.9, 1.0, 1.1), sample_rate: int = 16000, choice: Optional[Tensor] = None,
                  lowpass_filter_width: int = 6, rolloff: float = 0.99) -> Tuple[Tensor, Tensor, Tensor]:
    """``(out, out_len, choice)``: every utterance of ``wave`` [B, L] or [L] played at one of ``factors`` -- resampled by
    ``(int(f * sample_rate), sample_rate)``, torchaudio's ``transforms.Speed``, so 0.9 makes it longer and lower --, the int64 lengths
    and the int32 index into ``factors`` each utterance took.  ``choice`` None: drawn uniformly from ``(seed, utt_offset + b)``, so a
    call on a slice of the batch with ``utt_offset`` advanced returns the rows of the whole call.  Given: applied as it is; an entry
    outside the factors copies its utterance.  ``out`` is as wide as the slowest factor needs for ``L`` samples, whatever was drawn
    (nothing is read back).  At most eight factors; the rest as ``resample``."""
    return _resample_with("speed_perturb", wave, lengths, lambda: resample_plan(speed_ratios(factors, sample_rate), lowpass_filter_width, rolloff),
                          choice, int(seed) & _M64, int(utt_offset) & _M64)


class SpeedPerturb(nn.Module):
    """``wave, n = speed(wave, n)`` in front of the mel front end: ``speed_perturb`` with the arguments given here in train mode, the
    input and its lengths in eval mode.  The call counter, the seed rule (call k draws from ``seed + k * 0x9E3779B97F4A7C15``) and
    ``get_state`` / ``set_state`` are ``SpecAugment``'s; ``last_choice`` holds the choices of the last train-mode call.  No parameters,
    no buffers.  The plan is uploaded at the first call on a device: make that call before capturing a graph."""

    def __init__(self, seed: Optional[int] = None, factors: Sequence[float] = (0.9, 1.0, 1.1), sample_rate: int = 16000,
                 lowpass_filter_width: int = 6, rolloff: float = 0.99):
        super().__init__()
        resample_plan(speed_ratios(factors, sample_rate), lowpass_filter_width, rolloff)  # refused here rather than at the first step
        self.seed = capi.new_seed() if seed is None else int(seed)
        self.kwargs = dict(factors=tuple(factors), sample_rate=sample_rate, lowpass_filter_width=lowpass_filter_width, rolloff=rolloff)
        self.calls = 0
        self.last_choice: Optional[Tensor] = None

    def get_state(self) -> Dict[str, int]:
        return {"seed": self.seed, "calls": self.calls}

    def set_state(self, state: Dict[str, int]) -> None:
        self.seed, self.calls = int(state["seed"]), int(state["calls"])

    def forward(self, wave: Tensor, lengths: Optional[Tensor] = None, utt_offset: int = 0) -> Tuple[Tensor, Optional[Tensor]]:
        if not self.training:
            return wave, lengths
        seed = (self.seed + self.calls * 0x9E3779B97F4A7C15) & _M64
        self.calls += 1
        out, out_len, self.last_choice = speed_perturb(wave, lengths, seed=seed, utt_offset=utt_offset, **self.kwargs)
        return out, out_len

    def extra_repr(self) -> str:
        return ", ".join(f"{k}={v!r}" for k, v in self.kwargs.items())


# ---------------------------------------------------------------------------------------------------------------------------
# waveform augmentation: reverberation, noise, volume
# ---------------------------------------------------------------------------------------------------------------------------
WAVEAUG_SITE = 0x57415547                                                     # EEC_WAVEAUG_SITE
WAVEAUG_PARAMS, WAVEAUG_TILE, WAVEAUG_MAX_BANK, WAVEAUG_MAX_SNRS = 5, 1024, 4096, 64  # EEC_WAVEAUG_PARAMS, _TILE, _MAX_BANK, _MAX_SNRS
REVERB_MAX_TAPS = 16384                                                       # EEC_REVERB_MAX_TAPS
RIR_NORMS = {"none": 0, "l2": 1, "peak": 2}                                   # EEC_RIR_NORM_NONE, _L2, _PEAK
RIR_MAGIC, NOISE_MAGIC = 0x52495242, 0x4E4F4953                               # EEC_RIR_MAGIC, EEC_NOISE_MAGIC
REVERB_FFT_BLOCK = 2048                                                       # EEC_REVERB_FFT_BLOCK
RIR_SPECTRA_MAGIC = 0x52495246                                                # EEC_RIR_SPECTRA_MAGIC
REVERB_FFT_MIN_TAPS = 256                                                     # EEC_REVERB_FFT_MIN_TAPS
REVERB_METHODS = ("direct", "fft")
_ONE_BITS = 0x3F800000                                                     # 1.0f


def _rows_fp32(who: str, rows, most: int) -> Tuple[np.ndarray, np.ndarray]:
    """The 1-D arrays or tensors of ``rows`` as one fp32 array and their int32 counts; what the library would refuse, refused here."""
    if isinstance(rows, (Tensor, np.ndarray)) or not hasattr(rows, "__len__"):
        raise ValueError(f"{who}: a list of 1-D arrays or tensors is expected")
    if not 1 <= len(rows) <= WAVEAUG_MAX_BANK:
        raise ValueError(f"{who}: between 1 and {WAVEAUG_MAX_BANK} rows, got {len(rows)}")
    flat = []
    for r, row in enumerate(rows):
        a = row.detach().cpu().numpy() if isinstance(row, Tensor) else np.asarray(row)
        if a.ndim != 1 or a.dtype.kind not in "fiu":
            raise ValueError(f"{who}: row {r} must be a 1-D array of numbers, got {a.dtype} {a.shape}")
        if not 1 <= a.shape[0] <= most:
            raise ValueError(f"{who}: row {r} must have between 1 and {most} values, got {a.shape[0]}")
        a = a.astype(np.float32)
        if not np.isfinite(a).all():
            raise ValueError(f"{who}: row {r} holds a value that is not finite")
        flat.append(a)
    return np.ascontiguousarray(np.concatenate(flat)), np.array([a.shape[0] for a in flat], dtype=np.int32)


class _Bank:
    """An image of int32 words on the host and its uploaded copies, made once per device."""

    image: np.ndarray

    def _build(self, entry: str, *args) -> None:
        """``entry(*args, image, its bytes)`` into an image of ``entry_bytes(*args)`` bytes."""
        lib = capi.load()
        nbytes = getattr(lib, entry + "_bytes")(*args)
        if nbytes == 0:
            raise ValueError(lib.eec_last_error().decode(errors="replace"))
        self.image = np.zeros(nbytes // 4, dtype=np.int32)
        capi.call(entry, *args, self.image.ctypes.data, nbytes)
        self.count = int(self.image[1])
        self._dev: Dict[torch.device, Tensor] = {}

    def on(self, dev: torch.device) -> Tensor:
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = torch.from_numpy(self.image).to(dev)
        return t

    def __len__(self) -> int:
        return self.count


class RirBank(_Bank):
    """The image ``eec_rir_bank`` builds of ``rirs``, a list of 1-D arrays or tensors of at most 16384 taps each (include/eec.h has
    the layout).  ``normalize``: "l2" (unit energy), "peak" or "none", in fp64, each tap rounded once; zero heads and tails are
    dropped.  ``shift`` True (Kaldi's ``--shift-output``): the peak of a RIR -- the first index of ``max |h|`` -- stays where the
    sample was, so frame counts and CTC targets are untouched; False: the plain causal convolution cut to the input's length.

    ``method``: how ``reverberate``, ``wave_augment`` and ``WaveAugment`` evaluate the convolution with this bank.  "direct" (the
    default): the tap-order fp32 sum of ``eec_reverb``, bit-identical between kernel and host path, whose cost grows with the taps.
    "fft": ``eec_reverb_fft``, partitioned overlap-save with blocks of ``REVERB_FFT_BLOCK`` samples, for RIRs of thousands of taps:
    the same definition inside a stated error bound (include/eec.h, "Reverberation by FFT"), deterministic, but bit-identical neither
    to the direct path nor to the host path, which for an FFT bank is ``np.fft`` in fp64 rounded once.  The spectral image is built
    at the first FFT use of the bank and uploaded once per device.  ``max_workspace_bytes`` (an attribute, 2 GiB): above it the FFT
    path splits a call over utterances, which changes no bit.  "auto": "fft" when the longest stored RIR has at least
    ``REVERB_FFT_MIN_TAPS`` taps -- the smallest timed tap count from which the FFT path measured faster
    (profiles/waveaug_fft_time.json) --, "direct" otherwise; resolved here, once, and kept as ``bank.method``."""

    max_workspace_bytes = 2 << 30

    def __init__(self, rirs, normalize: str = "l2", shift: bool = True, method: str = "direct"):
        if normalize not in RIR_NORMS:
            raise ValueError(f"RirBank: normalize must be 'l2', 'peak' or 'none', got {normalize!r}")
        if method not in REVERB_METHODS + ("auto",):
            raise ValueError(f"RirBank: method must be one of {', '.join(repr(m) for m in REVERB_METHODS)} or 'auto', got {method!r}")
        taps, n = _rows_fp32("RirBank", rirs, REVERB_MAX_TAPS)
        self._build("eec_rir_bank", len(n), taps.ctypes.data, n.ctypes.data, RIR_NORMS[normalize], int(bool(shift)))
        self.normalize, self.shift = normalize, bool(shift)
        self.max_taps = int(self.image[4:4 + 4 * self.count:4].max())  # the longest stored RIR
        self.method = method if method != "auto" else "fft" if self.max_taps >= REVERB_FFT_MIN_TAPS else "direct"
        self.spectra: Optional[np.ndarray] = None
        self._spectra_dev: Dict[torch.device, Tensor] = {}

    def spectra_image(self) -> np.ndarray:
        """The image ``eec_rir_spectra`` builds of the tap image (int32 words; include/eec.h has the layout), made once."""
        if self.spectra is None:
            lib = capi.load()
            nbytes = lib.eec_rir_spectra_bytes(self.image.ctypes.data)
            if nbytes == 0:
                raise ValueError(lib.eec_last_error().decode(errors="replace"))
            image = np.zeros(nbytes // 4, dtype=np.int32)
            capi.call("eec_rir_spectra", self.image.ctypes.data, image.ctypes.data, nbytes)
            self.spectra = image
        return self.spectra

    def spectra_on(self, dev: torch.device) -> Tensor:
        t = self._spectra_dev.get(dev)
        if t is None:
            t = self._spectra_dev[dev] = torch.from_numpy(self.spectra_image()).to(dev)
        return t

    def spectrum(self, r: int) -> np.ndarray:
        """fp32 ``[P, 2 * REVERB_FFT_BLOCK]``: the stored spectra of RIR ``r``, partition after partition."""
        image = self.spectra_image()
        P, at = (int(v) for v in image[8 + 2 * r:10 + 2 * r])
        return image[at:at + P * 2 * REVERB_FFT_BLOCK].view(np.float32).reshape(P, 2 * REVERB_FFT_BLOCK)

    def rir(self, r: int) -> Tuple[int, np.ndarray]:
        """``(d, taps)`` of RIR ``r``: the shift and the stored fp32 taps."""
        K, d, at, _ = (int(v) for v in self.image[4 + 4 * r:8 + 4 * r])
        return d, self.image[at:at + K].view(np.float32)


class NoiseBank(_Bank):
    """The image ``eec_noise_bank`` builds of ``noises``, a list of 1-D arrays or tensors of 1 to 2^30 samples each."""

    def __init__(self, noises):
        samples, n = _rows_fp32("NoiseBank", noises, MAX_SAMPLES)
        self._build("eec_noise_bank", len(n), samples.ctypes.data, n.ctypes.data)
        self.lengths = self.image[4:4 + 2 * self.count:2].copy()

    def noise(self, m: int) -> np.ndarray:
        n, at = (int(v) for v in self.image[4 + 2 * m:6 + 2 * m])
        return self.image[at:at + n].view(np.float32)


def _host_waveaug_draw(B: int, seed: int, utt_offset: int, R: int, thr_reverb: int, noise_len: np.ndarray, thr_noise: int, n_snrs: int,
                       volume: Optional[Tuple[float, float]]) -> np.ndarray:
    key = _key(seed, WAVEAUG_SITE)
    with np.errstate(over="ignore"):
        at = (np.arange(B, dtype=np.uint64) + np.uint64(utt_offset & _M64)) * np.uint64(64)
        u = [_words(key, at + np.uint64(slot)).astype(np.uint64) for slot in range(7)]
    below = lambda w, m: ((w * np.asarray(m, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)  # noqa: E731
    p = np.zeros((B, WAVEAUG_PARAMS), dtype=np.int64)
    M = noise_len.shape[0]
    p[:, 0] = np.where(u[0] < np.uint64(thr_reverb), below(u[1], R), -1) if R > 0 else -1
    if M > 0 and n_snrs > 0:
        on = u[2] < np.uint64(thr_noise)
        m = below(u[3], M)
        p[:, 1] = np.where(on, m, -1)
        p[:, 2] = np.where(on, below(u[4], noise_len[m]), 0)
        p[:, 3] = np.where(on, below(u[5], n_snrs), 0)
    else:
        p[:, 1] = -1
    gain = np.ones(B, dtype=np.float32)
    if volume is not None:
        lo, hi = volume
        gain = (lo + (hi - lo) * (u[6].astype(np.float64) * 2.0 ** -32)).astype(np.float32)
    p[:, 4] = gain.view(np.int32)
    return p.astype(np.int32)


def _host_energy(v: np.ndarray) -> float:
    """sum v^2 in fp64 in the stated order: groups of 8 in order, 64 groups by halving, two blocks, then the tiles in order."""
    n = v.shape[0]
    tiles = -(-n // WAVEAUG_TILE)
    sq = np.zeros(tiles * WAVEAUG_TILE, dtype=np.float64)
    sq[:n] = v.astype(np.float64) ** 2
    a = sq.reshape(tiles, WAVEAUG_TILE // 8, 8)
    e = np.zeros(a.shape[:2], dtype=np.float64)
    for j in range(8):
        e = e + a[:, :, j]
    e = e.reshape(tiles, 2, 64)
    for s in (32, 16, 8, 4, 2, 1):
        e = e[:, :, :s] + e[:, :, s:2 * s]
    total = 0.0
    for part in e[:, 0, 0] + e[:, 1, 0]:
        total = total + float(part)
    return total


def _host_reverb(x: np.ndarray, d: int, h: np.ndarray) -> np.ndarray:
    """y[i] = sum_k h[k] x[i + d - k], the taps in order, one fp32 multiply and one fp32 add each."""
    n, K = x.shape[0], h.shape[0]
    pad = K + abs(d)
    xp = np.zeros(n + 2 * pad, dtype=np.float32)
    xp[pad:pad + n] = x
    acc = np.zeros(n, dtype=np.float32)
    for k in range(K):
        acc = acc + h[k] * xp[pad + d - k:pad + d - k + n]
    return acc


def _host_reverb_fft(x: np.ndarray, d: int, h: np.ndarray) -> np.ndarray:
    """The same y by ``np.fft`` in fp64: the full linear convolution, cut at ``d``, rounded once to fp32."""
    n, K = x.shape[0], h.shape[0]
    size = 1 << (n + K - 1).bit_length()
    full = np.fft.irfft(np.fft.rfft(x.astype(np.float64), size) * np.fft.rfft(h.astype(np.float64), size), size)[:n + K - 1]
    at = np.arange(n, dtype=np.int64) + d
    inside = (at >= 0) & (at < n + K - 1)
    return np.where(inside, full[np.clip(at, 0, n + K - 2)], 0.0).astype(np.float32)


def _reverb_method(who: str, rirs: Optional["RirBank"], method: Optional[str]) -> str:
    if method is None:
        return "direct" if rirs is None else rirs.method
    if method not in REVERB_METHODS:
        raise ValueError(f"{who}: method must be one of {', '.join(repr(m) for m in REVERB_METHODS)} or None, got {method!r}")
    return method


def _host_waveaug(wave: np.ndarray, n_all: np.ndarray, params: np.ndarray, rirs: Optional[RirBank], noises: Optional[NoiseBank],
                  snr_gain: Sequence[float], reverb: bool = True, mix: bool = True, method: str = "direct"):
    B = wave.shape[0]
    out, applied = np.zeros_like(wave), np.zeros((B, 2), dtype=np.float32)
    for b in range(B):
        n = int(n_all[b])
        r, m, start, snr_idx, bits = (int(v) for v in params[b])
        y = wave[b, :n].copy()
        if reverb and rirs is not None and 0 <= r < len(rirs) and n > 0:
            y = (_host_reverb_fft if method == "fft" else _host_reverb)(y, *rirs.rir(r))
        gain = np.array([bits], dtype=np.int32).view(np.float32)[0]
        scale = np.float32(0.0)
        if mix:
            if noises is not None and 0 <= m < len(noises) and 0 <= snr_idx < len(snr_gain) and n > 0:
                row = noises.noise(m)
                seg = row[(start % row.shape[0] + np.arange(n, dtype=np.int64)) % row.shape[0]]
                es, en = _host_energy(y), _host_energy(seg)
                if es > 0.0 and en > 0.0:
                    scale = np.float32(np.sqrt(np.float64(es) / np.float64(en)) * np.float64(snr_gain[snr_idx]))
                if scale != 0.0:
                    y = y + scale * seg
            y = y * gain
            applied[b] = scale, gain
        out[b, :n] = y
    return out, applied


def _waveaug_batch(who: str, wave: Tensor, lengths: Optional[Tensor]):
    if not isinstance(wave, Tensor) or wave.dim() not in (1, 2) or wave.dtype != torch.float32:
        raise ValueError(f"{who}: wave must be an fp32 tensor [B, L] or [L], got {getattr(wave, 'dtype', None)} {tuple(getattr(wave, 'shape', ()))}")
    squeeze = wave.dim() == 1
    if squeeze:
        wave = wave.unsqueeze(0)
    B, L = wave.shape
    if L > MAX_SAMPLES:
        raise ValueError(f"{who}: at most 2^30 samples per utterance, got {L}")
    if lengths is not None:
        if not isinstance(lengths, Tensor) or lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != B or lengths.dim() > 1:
            raise ValueError(f"{who}: lengths must be an int32 or int64 tensor of {B} entries")
    return wave.contiguous(), squeeze


def _waveaug_bank(who: str, name: str, bank, cls):
    if bank is not None and not isinstance(bank, cls):
        raise ValueError(f"{who}: {name} must be a {cls.__name__} or None, got {type(bank).__name__}")
    return bank


def _coin(who: str, name: str, p) -> int:
    if not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError(f"{who}: {name} must lie in [0, 1], got {p!r}")
    return int(math.floor(float(p) * 4294967296.0))


def _snr_gains(who: str, snrs) -> list:
    snrs = [snrs] if isinstance(snrs, (int, float)) else list(snrs)
    if not 1 <= len(snrs) <= WAVEAUG_MAX_SNRS:
        raise ValueError(f"{who}: between 1 and {WAVEAUG_MAX_SNRS} SNRs, got {len(snrs)}")
    if not all(isinstance(s, (int, float)) and math.isfinite(s) and abs(s) <= 2000 for s in snrs):
        raise ValueError(f"{who}: an SNR must be a finite number of dB, got {snrs!r}")
    return [10.0 ** (-float(s) / 20.0) for s in snrs]


def _volume(who: str, volume) -> Optional[Tuple[float, float]]:
    if volume is None:
        return None
    if not hasattr(volume, "__len__") or len(volume) != 2 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in volume):
        raise ValueError(f"{who}: volume must be None or a finite pair (lo, hi), got {volume!r}")
    return float(volume[0]), float(volume[1])


def _waveaug_run(who: str, wave: Tensor, lengths: Optional[Tensor], params: Optional[Tensor], draw, rirs: Optional[RirBank],
                 noises: Optional[NoiseBank], gains: Sequence[float], reverb: bool = True, mix: bool = True, method: Optional[str] = None,
                 max_workspace_bytes: Optional[int] = None):
    """The host path or the launches for a checked batch.  ``params`` None: drawn with ``draw`` = (seed, utt_offset, thr_reverb,
    thr_noise, volume).  ``reverb`` / ``mix`` False: that launch is left out (the prescribed single-stage forms).  ``method`` and
    ``max_workspace_bytes`` None: the bank's."""
    B, L = wave.shape
    method = _reverb_method(who, rirs, method)
    dev = wave.device
    if lengths is not None:
        lengths = capi.to_device(lengths.reshape(B), dev, torch.int64).clamp(0, L).contiguous()
    if params is not None:
        if not isinstance(params, Tensor) or params.shape != (B, WAVEAUG_PARAMS) or params.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{who}: params must be an int32 or int64 tensor [{B}, {WAVEAUG_PARAMS}]")
        lim = (1 << 31) - 1
        params = params.to(dev).clamp(-lim - 1, lim).to(torch.int32).contiguous()

    if not wave.is_cuda:
        n = np.full(B, L, dtype=np.int64) if lengths is None else lengths.numpy()
        if params is None:
            seed, utt_offset, thr_r, thr_n, volume = draw
            params = torch.from_numpy(_host_waveaug_draw(B, seed, utt_offset, 0 if rirs is None else len(rirs), thr_r,
                                                         np.zeros(0, dtype=np.int32) if noises is None else noises.lengths, thr_n, len(gains),
                                                         volume))
        out, applied = _host_waveaug(wave.numpy(), n, params.numpy(), rirs, noises, gains, reverb, mix, method)
        return torch.from_numpy(out), params, torch.from_numpy(applied)

    lib = capi.load()
    rir_bank = None if rirs is None else rirs.on(dev)
    noise_bank = None if noises is None else noises.on(dev)
    lens = None if B == 0 else lengths
    out = torch.empty_like(wave)
    applied = torch.zeros((B, 2), dtype=torch.float32, device=dev) if not mix else torch.empty((B, 2), dtype=torch.float32, device=dev)
    table = (C.c_double * max(len(gains), 1))(*gains)
    if params is None:
        seed, utt_offset, thr_r, thr_n, volume = draw
        lo, hi = volume if volume is not None else (1.0, 1.0)
        params = torch.empty((B, WAVEAUG_PARAMS), dtype=torch.int32, device=dev)
        capi.launch("eec_waveaug_draw", dev, B, seed, utt_offset, rir_bank, thr_r, noise_bank, thr_n, len(gains), int(volume is not None), lo, hi,
                    params)
    partials = None
    if mix and noises is not None:
        partials = torch.empty(max(lib.eec_waveaug_partials_bytes(B, L) // 8, 1), dtype=torch.float64, device=dev)
    if reverb and method == "fft" and rirs is not None and B > 0:
        # the spectra of every window go to a workspace; above max_workspace_bytes the call is split over utterances
        most = int(rirs.max_workspace_bytes if max_workspace_bytes is None else max_workspace_bytes)
        step = min(B, max(1, most // lib.eec_reverb_fft_workspace_bytes(1, L)))
        nbytes = lib.eec_reverb_fft_workspace_bytes(step, L)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        spectra, tiles = rirs.spectra_on(dev), max(-(-L // WAVEAUG_TILE), 1)
        for b0 in range(0, B, step):
            capi.launch("eec_reverb_fft", dev, wave[b0:], None if lens is None else lens[b0:], params[b0:], min(step, B - b0), L, rir_bank,
                        spectra, out[b0:], None if partials is None else partials[2 * tiles * b0:], work, nbytes)
    elif reverb:
        capi.launch("eec_reverb", dev, wave, lens, params, B, L, rir_bank, out, partials)
    if mix:
        if partials is not None:
            capi.launch("eec_noise_energy", dev, None if reverb else wave, lens, params, B, L, noise_bank, partials)
        capi.launch("eec_noise_mix", dev, out if reverb else wave, lens, params, B, L, noise_bank, table, len(gains), partials, out, applied)
    return out, params, applied


def wave_augment(wave: Tensor, lengths: Optional[Tensor] = None, *, seed: int, utt_offset: int = 0, rirs: Optional[RirBank] = None,
                 noises: Optional[NoiseBank] = None, p_reverb: float = 1.0, p_noise: float = 1.0, snrs: Sequence[float] = (20, 15, 10, 5, 0),
                 volume: Optional[Tuple[float, float]] = None, params: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``(out, params, applied)``: ``wave`` [B, L] or [L] (fp32) reverberated, with noise added and its volume changed, in Kaldi's
    ``wav-reverberate`` order; the int32 rows ``rir, noise, start, snr_idx, gain_bits`` it was made with; and the fp32 ``[B, 2]``
    noise scale (0.0: none added) and gain applied.  ``lengths`` [B]: valid samples, clamped to [0, L]; None: L.  Samples at or past
    a length are never read, outputs there are 0.0, the lengths do not change, and every utterance comes out as if processed alone.

    ``params`` None: drawn from ``(seed, utt_offset + b)`` -- with probability ``p_reverb`` a RIR of ``rirs``, with probability
    ``p_noise`` a row of ``noises``, a start inside it and one of ``snrs`` (dB; the noise is scaled so that the utterance's energy over
    the noise segment's is that SNR), a gain uniform in ``volume`` = (lo, hi) (None: 1) -- so a call on a slice of the batch with
    ``utt_offset`` advanced returns the rows of the whole call.  Given: applied as they are; an index outside its bank (-1) switches
    the stage off, a start is reduced mod the row's length.  No host synchronisation; a CPU tensor takes the NumPy host path,
    bit-identical for finite input (with a bank of ``method="fft"``: the same definition inside its bound, not the same bits).  The
    banks are uploaded at the first call on a device."""
    who = "wave_augment"
    wave, squeeze = _waveaug_batch(who, wave, lengths)
    rirs, noises = _waveaug_bank(who, "rirs", rirs, RirBank), _waveaug_bank(who, "noises", noises, NoiseBank)
    draw = (int(seed) & _M64, int(utt_offset) & _M64, _coin(who, "p_reverb", p_reverb), _coin(who, "p_noise", p_noise), _volume(who, volume))
    out, params, applied = _waveaug_run(who, wave, lengths, params, draw, rirs, noises, _snr_gains(who, snrs))
    return (out[0], params[0], applied[0]) if squeeze else (out, params, applied)


def _rows_of(who: str, name: str, value, B: int, dev) -> Tensor:
    if isinstance(value, int) and not isinstance(value, bool):
        return torch.full((B,), value, dtype=torch.int64, device=dev).clamp(-(1 << 31), (1 << 31) - 1)
    if not isinstance(value, Tensor) or value.dtype not in (torch.int32, torch.int64) or value.numel() != B or value.dim() > 1:
        raise ValueError(f"{who}: {name} must be an integer or an int32 or int64 tensor of {B} entries")
    return value.reshape(B).to(dev).to(torch.int64).clamp(-(1 << 31), (1 << 31) - 1)


def reverberate(wave: Tensor, lengths: Optional[Tensor], rirs: RirBank, index, *, method: Optional[str] = None,
                max_workspace_bytes: Optional[int] = None) -> Tensor:
    """``wave`` [B, L] or [L] convolved with the RIRs ``index`` (an integer or [B]) of ``rirs``; -1 or an index outside the bank copies
    the utterance.  ``method`` ("direct", "fft") and ``max_workspace_bytes`` override the bank's for this call.  The rest as
    ``wave_augment``."""
    who = "reverberate"
    wave, squeeze = _waveaug_batch(who, wave, lengths)
    if not isinstance(rirs, RirBank):
        raise ValueError(f"{who}: rirs must be a RirBank, got {type(rirs).__name__}")
    B, dev = wave.shape[0], wave.device
    params = torch.zeros((B, WAVEAUG_PARAMS), dtype=torch.int64, device=dev)
    params[:, 0], params[:, 1], params[:, 4] = _rows_of(who, "index", index, B, dev), -1, _ONE_BITS
    out, _, _ = _waveaug_run(who, wave, lengths, params, None, rirs, None, [], mix=False, method=_reverb_method(who, rirs, method),
                             max_workspace_bytes=max_workspace_bytes)
    return out[0] if squeeze else out


def add_noise(wave: Tensor, lengths: Optional[Tensor], noises: NoiseBank, index, start, snr) -> Tensor:
    """``wave`` [B, L] or [L] plus the noise rows ``index`` of ``noises`` read from ``start`` on (integers or [B]; tiled), scaled so that
    the utterance's energy over the noise segment's is ``snr`` dB -- a number or B numbers on the host, at most 64 distinct --:
    torchaudio's ``functional.add_noise`` up to rounding.  The rest as ``wave_augment``."""
    who = "add_noise"
    wave, squeeze = _waveaug_batch(who, wave, lengths)
    if not isinstance(noises, NoiseBank):
        raise ValueError(f"{who}: noises must be a NoiseBank, got {type(noises).__name__}")
    B, dev = wave.shape[0], wave.device
    snr = [snr] * B if isinstance(snr, (int, float)) else (snr.tolist() if isinstance(snr, (Tensor, np.ndarray)) else list(snr))
    if len(snr) != B:
        raise ValueError(f"{who}: snr must be a number or {B} numbers, got {len(snr)}")
    levels = sorted(set(snr)) if B else [0.0]
    gains = _snr_gains(who, levels)
    params = torch.zeros((B, WAVEAUG_PARAMS), dtype=torch.int64, device=dev)
    params[:, 1], params[:, 2] = _rows_of(who, "index", index, B, dev), _rows_of(who, "start", start, B, dev)
    params[:, 3], params[:, 4] = torch.tensor([levels.index(s) for s in snr], dtype=torch.int64, device=dev), _ONE_BITS
    out, _, _ = _waveaug_run(who, wave, lengths, params, None, None, noises, gains, reverb=False)
    return out[0] if squeeze else out


class WaveAugment(nn.Module):
    """``wave = waveaug(wave, n)`` between ``SpeedPerturb`` and the mel front end: ``wave_augment`` with the arguments given here in
    train mode, the input itself in eval mode; the lengths do not change.  ``rirs`` / ``noises``: a bank, or a list of 1-D arrays to
    build one from.  The call counter, the seed rule (call k draws from ``seed + k * 0x9E3779B97F4A7C15``) and ``get_state`` /
    ``set_state`` are ``SpecAugment``'s; ``last_params`` and ``last_applied`` hold the rows and the scale and gain of the last
    train-mode call.  No parameters, no buffers.  The banks are uploaded at the first call on a device: make that call before
    capturing a graph."""

    def __init__(self, seed: Optional[int] = None, rirs=None, noises=None, p_reverb: float = 1.0, p_noise: float = 1.0,
                 snrs: Sequence[float] = (20, 15, 10, 5, 0), volume: Optional[Tuple[float, float]] = None, normalize: str = "l2",
                 shift: bool = True):
        super().__init__()
        who = "WaveAugment"
        if rirs is not None and not isinstance(rirs, RirBank):
            rirs = RirBank(rirs, normalize=normalize, shift=shift)
        if noises is not None and not isinstance(noises, NoiseBank):
            noises = NoiseBank(noises)
        _coin(who, "p_reverb", p_reverb), _coin(who, "p_noise", p_noise), _snr_gains(who, snrs), _volume(who, volume)  # refused here
        self.seed = capi.new_seed() if seed is None else int(seed)
        self.rirs, self.noises = rirs, noises
        self.kwargs = dict(p_reverb=p_reverb, p_noise=p_noise, snrs=tuple(snrs), volume=None if volume is None else tuple(volume))
        self.calls = 0
        self.last_params: Optional[Tensor] = None
        self.last_applied: Optional[Tensor] = None

    def get_state(self) -> Dict[str, int]:
        return {"seed": self.seed, "calls": self.calls}

    def set_state(self, state: Dict[str, int]) -> None:
        self.seed, self.calls = int(state["seed"]), int(state["calls"])

    def forward(self, wave: Tensor, lengths: Optional[Tensor] = None, utt_offset: int = 0) -> Tensor:
        if not self.training:
            return wave
        seed = (self.seed + self.calls * 0x9E3779B97F4A7C15) & _M64
        self.calls += 1
        out, self.last_params, self.last_applied = wave_augment(wave, lengths, seed=seed, utt_offset=utt_offset, rirs=self.rirs,
                                                                noises=self.noises, **self.kwargs)
        return out

    def extra_repr(self) -> str:
        banks = f"rirs={0 if self.rirs is None else len(self.rirs)}, noises={0 if self.noises is None else len(self.noises)}, "
        return banks + ", ".join(f"{k}={v!r}" for k, v in self.kwargs.items())
