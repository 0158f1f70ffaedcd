"""Timing of waveform augmentation on the device (csrc/waveaug.hip; ``early_exit_transformer_amd/augment.py``) at the benchmarked
batch as waveforms, [64, 164 000] samples with lengths of 100 433 to 164 000.

    python tools/waveaug_time.py [--rounds 7] [--reps 20] [--out profiles/waveaug_time.json]
    python tools/waveaug_time.py --fft [--rounds 7] [--reps 20] [--out profiles/waveaug_fft_time.json]

One process; the legs run in turn, ``--rounds`` times, each as a train of calls between two device events (alternating puts all of
them under the same box noise); the record holds the median, minimum and maximum per call:
* ``draw``: eec_waveaug_draw alone, through ctypes on preallocated tensors;
* ``reverb_{800,4000,16000}_{all,half}``: eec_reverb alone (with the partial energies) on prescribed rows, RIRs of 800, 4000 and
  16 000 taps (50 ms, 250 ms and 1 s at 16 kHz), every utterance reverberated or every other one, and ``reverb_none`` (all copied);
  with the multiply-adds per second of the reverberated utterances' valid samples;
* ``energy``: eec_noise_energy alone; ``mix``: eec_noise_mix alone, every utterance with noise and a gain;
* ``wave_augment_{800,4000}``: the Python entry as a training loop calls it -- draw, reverberation with probability 0.5 from a bank of
  four RIRs of that size, noise from a bank of eight rows of 3 to 20 s, volume, and the allocations;
* ``plain_copy``: ``out.copy_(wave)``, what moving a batch of that size costs under this way of timing;
* ``torch_ops_{800,4000,16000}``: the same augmentation from torch ops on the device -- ``torch.fft.rfft`` / ``irfft`` convolution of the
  whole batch with one RIR, then add_noise from elementwise ops and ``sum`` (lengths are not honoured, which only makes it cheaper).
For scale the record repeats the default model's training step, 22.9 ms (README).  The device results are also compared with the
host path on a slice and with the torch composition.  Records, not targets; a run without a HIP device fails.

``--fft``: the same batch and protocol for the reverberation alone at 256, 512, 1024, 2048, 4000 and 16 000 taps, every utterance
(``all``) or every other one (``half``) reverberated: ``direct_*`` eec_reverb, ``fft_*`` eec_reverb_fft (both launches),
``fft_windows_*`` and ``fft_blocks_*`` each launch alone (eec_reverb_fft_stage), ``torch_rfft_*`` the ``rfft`` / ``irfft`` convolution
of the whole batch with one RIR (lengths and the ``half`` switch not honoured).  ``fft_faster_from_taps`` is the smallest timed tap
count from which the FFT path's median is below the direct path's in both setups (null: none).  The FFT path's output is compared
with the direct path's and with an fp64 FFT on a full-length utterance.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import augment, capi  # noqa: E402

B, L = 64, 164000
TAPS = (800, 4000, 16000)
SNRS = (20, 15, 10, 5, 0)
TRAIN_STEP_MS = 22.9
ONE = 0x3F800000


def spread(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def train_of(fn, reps):
    """Device milliseconds per call of a train of ``reps`` calls (events on the current stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def rir(K, rng):
    h = rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 6.0))
    h[K // 50] = 3.0
    return h.astype(np.float32)


def torch_ops(wave, h, noise, gain_db, n_fft):
    """FFT convolution with the direct path kept in place, then torchaudio's add_noise formula; one RIR and one SNR for the batch."""
    p = int(h.abs().argmax())
    y = torch.fft.irfft(torch.fft.rfft(wave, n_fft) * torch.fft.rfft(h, n_fft), n_fft)[:, p:p + wave.shape[1]]
    es, en = (y * y).sum(-1, keepdim=True), (noise * noise).sum(-1, keepdim=True)
    return y + torch.sqrt(es / en) * gain_db * noise


FFT_TAPS = (256, 512, 1024, 2048, 4000, 16000)


def main_fft(args):
    lib = capi.load()
    dev = torch.device("cuda", 0)
    st = capi.stream_ptr(dev)
    rng = np.random.default_rng(0)
    gen = torch.Generator().manual_seed(0)
    wave = (torch.randn(B, L, generator=gen) * 0.1).to(dev)
    lens_host = [L - (1009 * b) % 64001 for b in range(B)]  # ragged: 100 433 .. 164 000 samples
    lens = torch.tensor(lens_host, dtype=torch.int64, device=dev)
    sized = augment.RirBank([rir(K, rng) for K in FFT_TAPS], method="fft")
    rir_img, spec_img = sized.on(dev), sized.spectra_on(dev)
    out, ref = torch.empty_like(wave), torch.empty_like(wave)
    partials = torch.zeros(lib.eec_waveaug_partials_bytes(B, L) // 8, dtype=torch.float64, device=dev)
    nbytes = lib.eec_reverb_fft_workspace_bytes(B, L)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    params = {(K, name): torch.tensor([[k if b % every == 0 else -1, -1, 0, 0, ONE] for b in range(B)], dtype=torch.int32, device=dev)
              for k, K in enumerate(FFT_TAPS) for name, every in (("all", 1), ("half", 2))}

    def direct(kind, to=out):
        capi.check(lib.eec_reverb(wave.data_ptr(), lens.data_ptr(), params[kind].data_ptr(), B, L, rir_img.data_ptr(), to.data_ptr(), partials.data_ptr(),
                                  st), "eec_reverb")

    def fft(kind, stages=3):
        capi.check(lib.eec_reverb_fft_stage(wave.data_ptr(), lens.data_ptr(), params[kind].data_ptr(), B, L, rir_img.data_ptr(), spec_img.data_ptr(),
                                            out.data_ptr(), partials.data_ptr(), work.data_ptr(), nbytes, stages, st), "eec_reverb_fft_stage")

    n_fft = 1 << 18
    assert n_fft >= L + max(FFT_TAPS) - 1
    legs, slow = {}, {}
    for k, K in enumerate(FFT_TAPS):
        h = torch.from_numpy(sized.rir(k)[1].copy()).to(dev)
        p = int(h.abs().argmax())
        slow[f"torch_rfft_{K}"] = lambda h=h, p=p: torch.fft.irfft(torch.fft.rfft(wave, n_fft) * torch.fft.rfft(h, n_fft), n_fft)[:, p:p + L]
        for name in ("all", "half"):
            kind = (K, name)
            (slow if K > 2048 else legs)[f"direct_{K}_{name}"] = lambda kind=kind: direct(kind)
            legs[f"fft_{K}_{name}"] = lambda kind=kind: fft(kind)
            legs[f"fft_windows_{K}_{name}"] = lambda kind=kind: fft(kind, 1)
            legs[f"fft_blocks_{K}_{name}"] = lambda kind=kind: fft(kind, 2)

    checks = {}
    full = lens_host.index(L)
    for k, K in enumerate(FFT_TAPS):
        direct((K, "all"), ref)
        fft((K, "all"))
        h = torch.from_numpy(sized.rir(k)[1].copy()).to(dev)
        p = int(h.abs().argmax())
        y = torch.fft.irfft(torch.fft.rfft(wave[full].double(), n_fft) * torch.fft.rfft(h.double(), n_fft), n_fft)[p:p + L]
        checks[f"fft_{K}_max_abs_diff_vs_fp64_fft_over_max_abs"] = float((out[full].double() - y).abs().max() / y.abs().max())
        checks[f"direct_{K}_max_abs_diff_vs_fp64_fft_over_max_abs"] = float((ref[full].double() - y).abs().max() / y.abs().max())
        checks[f"fft_{K}_max_abs_diff_vs_direct_over_max_abs"] = float((out.double() - ref.double()).abs().max() / ref.abs().max())

    for fn in list(legs.values()) + list(slow.values()):
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(legs) + list(slow)}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(train_of(fn, args.reps))
        for k, fn in slow.items():
            ms[k].append(train_of(fn, 2))
    med = {k: statistics.median(v) for k, v in ms.items()}
    faster = [K for K in FFT_TAPS if all(med[f"fft_{K}_{name}"] < med[f"direct_{K}_{name}"] for name in ("all", "half"))]
    from_taps = None
    for K in reversed(FFT_TAPS):  # the smallest tap count from which every timed one is faster
        if K not in faster:
            break
        from_taps = K
    rec = {"what": "waveaug_fft", "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "shape": [B, L], "lengths": [min(lens_host), max(lens_host)], "taps": list(FFT_TAPS), "block": augment.REVERB_FFT_BLOCK,
           "workspace_bytes": nbytes, "fft_size_of_torch_rfft": n_fft, "rounds": args.rounds, "calls_per_train": args.reps,
           "calls_per_train_slow_legs": 2, "slow_legs": list(slow), "training_step_ms_for_scale": TRAIN_STEP_MS, "agreement": checks,
           "fft_faster_from_taps": from_taps}
    for k, v in ms.items():
        rec[k + "_ms_per_call"] = spread(v)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump([rec], f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fft", action="store_true", help="time the reverberation by FFT against the direct path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "waveaug_fft_time.json" if args.fft else "waveaug_time.json")
    if not torch.cuda.is_available():
        raise SystemExit("waveaug_time.py measures on a HIP device; none found")
    if args.fft:
        return main_fft(args)

    lib = capi.load()
    dev = torch.device("cuda", 0)
    st = capi.stream_ptr(dev)
    rng = np.random.default_rng(0)
    gen = torch.Generator().manual_seed(0)
    wave = (torch.randn(B, L, generator=gen) * 0.1).to(dev)
    lens_host = [L - (1009 * b) % 64001 for b in range(B)]  # ragged: 100 433 .. 164 000 samples
    lens = torch.tensor(lens_host, dtype=torch.int64, device=dev)
    sized = augment.RirBank([rir(K, rng) for K in TAPS])
    noises = augment.NoiseBank([(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (48000, 80000, 120000, 160000, 200000, 240000, 280000, 320000)])
    banks = {K: augment.RirBank([rir(K, rng) for _ in range(4)]) for K in TAPS[:2]}
    rir_img, noise_img = sized.on(dev), noises.on(dev)
    out, ref = torch.empty_like(wave), torch.empty_like(wave)
    partials = torch.zeros(lib.eec_waveaug_partials_bytes(B, L) // 8, dtype=torch.float64, device=dev)
    applied = torch.empty((B, 2), device=dev)
    drawn = torch.empty((B, 5), dtype=torch.int32, device=dev)
    table = (C.c_double * len(SNRS))(*[10.0 ** (-s / 20.0) for s in SNRS])

    def rows(r, every):
        return torch.tensor([[r if b % every == 0 else -1, b % len(noises), (7919 * b) % 48000, b % len(SNRS), ONE + 4096 * b] for b in range(B)],
                            dtype=torch.int32, device=dev)

    params = {f"{K}_{name}": rows(k, every) for k, K in enumerate(TAPS) for name, every in (("all", 1), ("half", 2))}
    params["none"] = rows(-1, 1)

    def draw():
        capi.check(lib.eec_waveaug_draw(B, 1, 0, rir_img.data_ptr(), 1 << 31, noise_img.data_ptr(), 1 << 32, len(SNRS), 1, 0.5, 2.0, drawn.data_ptr(), st),
                   "eec_waveaug_draw")

    def reverb(kind):
        capi.check(lib.eec_reverb(wave.data_ptr(), lens.data_ptr(), params[kind].data_ptr(), B, L, rir_img.data_ptr(), out.data_ptr(), partials.data_ptr(),
                                  st), "eec_reverb")

    def energy():
        capi.check(lib.eec_noise_energy(None, lens.data_ptr(), params["none"].data_ptr(), B, L, noise_img.data_ptr(), partials.data_ptr(), st),
                   "eec_noise_energy")

    def mix():
        capi.check(lib.eec_noise_mix(out.data_ptr(), lens.data_ptr(), params["none"].data_ptr(), B, L, noise_img.data_ptr(), table, len(SNRS),
                                     partials.data_ptr(), ref.data_ptr(), applied.data_ptr(), st), "eec_noise_mix")

    legs = {"draw": draw, "plain_copy": lambda: ref.copy_(wave), "reverb_none": lambda: reverb("none"), "reverb_800_all": lambda: reverb("800_all"),
            "reverb_800_half": lambda: reverb("800_half"), "energy": energy, "mix": mix}
    for K, bank in banks.items():
        legs[f"wave_augment_{K}"] = lambda bank=bank: augment.wave_augment(wave, lens, seed=1, rirs=bank, noises=noises, p_reverb=0.5, snrs=SNRS,
                                                                           volume=(0.5, 2.0))
    slow = {f"reverb_{K}_{name}": (lambda kind=f"{K}_{name}": reverb(kind)) for K in TAPS[1:] for name in ("all", "half")}
    n_fft = 1 << 18
    assert n_fft >= L + max(TAPS) - 1
    noise_rows = (torch.randn(B, L, generator=gen) * 0.05).to(dev)
    for k, K in enumerate(TAPS):
        h = torch.from_numpy(sized.rir(k)[1].copy()).to(dev)
        slow[f"torch_ops_{K}"] = lambda h=h: torch_ops(wave, h, noise_rows, 0.316, n_fft)

    # agreement: the host path on a slice; the FFT convolution where an utterance is full length (it ignores the lengths)
    checks = {}
    small, small_n = wave[:3, :5000].contiguous(), torch.tensor([5000, 4999, 1023])
    small_rows = torch.tensor([[0, 1, 47000, 2, ONE + 77], [0, 0, 5, 0, ONE], [-1, 3, 0, 4, ONE - 99]], dtype=torch.int32)
    got = augment.wave_augment(small, small_n.to(dev), seed=0, rirs=sized, noises=noises, snrs=SNRS, params=small_rows.to(dev))
    host = augment.wave_augment(small.cpu(), small_n, seed=0, rirs=sized, noises=noises, snrs=SNRS, params=small_rows)
    checks["bit_identical_to_host_path"] = bool(np.array_equal(got[0].cpu().numpy().view(np.int32), host[0].numpy().view(np.int32)) and
                                                np.array_equal(got[2].cpu().numpy().view(np.int32), host[2].numpy().view(np.int32)))
    full = lens_host.index(L)
    for k, K in enumerate(TAPS):
        reverb(f"{K}_all")
        h = torch.from_numpy(sized.rir(k)[1].copy()).to(dev)
        p = int(h.abs().argmax())
        y = torch.fft.irfft(torch.fft.rfft(wave[full].double(), n_fft) * torch.fft.rfft(h.double(), n_fft), n_fft)[p:p + L]
        checks[f"reverb_{K}_max_abs_diff_vs_fp64_fft_over_max_abs"] = float((out[full].double() - y).abs().max() / y.abs().max())

    for fn in list(legs.values()) + list(slow.values()):
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(legs) + list(slow)}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(train_of(fn, args.reps))
        for k, fn in slow.items():
            ms[k].append(train_of(fn, 2))
    rec = {"what": "waveaug", "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "shape": [B, L], "lengths": [min(lens_host), max(lens_host)], "taps": list(TAPS), "snrs": list(SNRS), "fft_size_of_torch_ops": n_fft,
           "rounds": args.rounds, "calls_per_train": args.reps, "calls_per_train_slow_legs": 2, "slow_legs": list(slow),
           "training_step_ms_for_scale": TRAIN_STEP_MS, "agreement": checks}
    for k, v in ms.items():
        rec[k + "_ms_per_call"] = spread(v)
        if k.startswith("reverb_") and k != "reverb_none":
            K, every = int(k.split("_")[1]), 1 if k.endswith("all") else 2
            macs = K * sum(n for b, n in enumerate(lens_host) if b % every == 0)
            rec[k + "_multiply_adds"] = macs
            rec[k + "_T_multiply_adds_per_s"] = round(macs / (statistics.median(v) * 1e-3) / 1e12, 3)
        if k == "plain_copy":
            rec[k + "_bytes_moved"] = 8 * B * L
            rec[k + "_TB_per_s"] = round(8 * B * L / (statistics.median(v) * 1e-3) / 1e12, 3)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump([rec], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
