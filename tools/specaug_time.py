"""Timing of SpecAugment on the device (csrc/specaug.hip; ``early_exit_transformer_amd/augment.py``) at the benchmarked batch,
mel [64, 80, 1027] with ragged lengths, under the default recipe (W = 5, 2 frequency masks of up to 27 rows, 5 time masks of up to 5 %).

    python tools/specaug_time.py [--rounds 7] [--reps 50] [--out profiles/specaug_time.json]

One process; the legs run in turn, ``--rounds`` times, each as a train of ``--reps`` calls between two device events (alternating puts
all of them under the same box noise); the record holds the median, minimum and maximum per call:
* ``draw``: eec_specaug_draw alone, through ctypes on preallocated tensors;
* ``apply_{bicubic,linear}_{warp,nowarp}``: eec_specaug_apply alone, on parameters drawn with W = 5 and with W = 0 (masks only: the
  copy path), with the bytes it has to move (one read and one write of the batch) over its median time;
* ``plain_copy``: ``out.copy_(mel)``, what moving the same bytes costs under this way of timing;
* ``spec_augment``: the Python entry, draw and apply and the two allocations, as a training loop calls it;
* ``torch_ops``: the same augmentation written with torch ops on the device -- per utterance two ``F.interpolate`` calls on slices and
  index assignments for the masks -- from parameters already on the host (a user's loop would first have to draw or fetch them).
For scale the record repeats the default model's training step, 22.9 ms (README).  The device result is also compared with the host
path of ``spec_augment`` on the same parameters.  Records, not targets; a run without a HIP device fails.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import augment, capi, synth  # noqa: E402

B, MELS, FRAMES, W, N_FREQ, N_TIME = 64, 80, 1027, 5, 2, 5
TRAIN_STEP_MS = 22.9


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


def torch_ops(mel, lens, rows, mode):
    """The augmentation of ``spec_augment`` from torch ops: ``rows`` and ``lens`` are host lists."""
    out = mel.clone()
    for b, (n, row) in enumerate(zip(lens, rows)):
        c, w = row[:2]
        if 1 <= c <= n - 1 and 1 <= w <= n - 1:
            x = mel[b, :, :n]
            if mode == "bicubic":
                one = lambda seg, size: F.interpolate(seg[None, None], size=(seg.size(0), size), mode="bicubic", align_corners=False)[0, 0]  # noqa: E731
            else:
                one = lambda seg, size: F.interpolate(seg[None], size=size, mode="linear", align_corners=False)[0]  # noqa: E731
            out[b, :, :w] = one(x[:, :c], w)
            out[b, :, w:n] = one(x[:, c:], n - w)
        for k in range(N_FREQ):
            f0, fw = row[2 + 2 * k], row[3 + 2 * k]
            out[b, f0:f0 + fw, :n] = 0.0
        for k in range(N_TIME):
            t0, tw = row[2 + 2 * N_FREQ + 2 * k], row[3 + 2 * N_FREQ + 2 * k]
            out[b, :, t0:t0 + tw] = 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specaug_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specaug_time.py measures on a HIP device; none found")

    lib = capi.load()
    dev = torch.device("cuda", 0)
    mel = synth.synth_mel(B, MELS, FRAMES, seed=0).to(dev)
    lens_host = [FRAMES - (37 * b) % 400 for b in range(B)]  # ragged: 628 .. 1027 frames
    lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
    P = 2 + 2 * N_FREQ + 2 * N_TIME
    params = {W: torch.empty((B, P), dtype=torch.int32, device=dev), 0: torch.empty((B, P), dtype=torch.int32, device=dev)}
    out = torch.empty_like(mel)
    st = capi.stream_ptr(dev)

    def draw(window):
        capi.check(lib.eec_specaug_draw(lens.data_ptr(), B, MELS, FRAMES, 1, 0, window, N_FREQ, 27, N_TIME, 0.05, FRAMES, params[window].data_ptr(), st),
                   "eec_specaug_draw")

    def apply(window, mode):
        capi.check(lib.eec_specaug_apply(mel.data_ptr(), lens.data_ptr(), params[window].data_ptr(), B, MELS, FRAMES, N_FREQ, N_TIME, augment.MODES[mode],
                                         0.0, out.data_ptr(), st), "eec_specaug_apply")

    draw(W), draw(0)
    torch.cuda.synchronize()
    rows = params[W].cpu().tolist()
    kw = dict(seed=1, time_warp_window=W, n_freq_masks=N_FREQ, n_time_masks=N_TIME)
    legs = {"draw": lambda: draw(W), "plain_copy": lambda: out.copy_(mel)}
    for mode in ("bicubic", "linear"):
        legs[f"apply_{mode}_warp"] = lambda mode=mode: apply(W, mode)
        legs[f"apply_{mode}_nowarp"] = lambda mode=mode: apply(0, mode)
    legs["spec_augment"] = lambda: augment.spec_augment(mel, lens, **kw)
    slow = {f"torch_ops_{mode}": (lambda mode=mode: torch_ops(mel, lens_host, rows, mode)) for mode in ("bicubic", "linear")}

    # the device against the host path and the torch composition, on the same parameters
    checks = {}
    for mode in ("bicubic", "linear"):
        got, _ = augment.spec_augment(mel, lens, params=params[W], **{**kw, "seed": 0, "time_warp_mode": mode})
        host, _ = augment.spec_augment(mel.cpu(), lens.cpu(), params=params[W].cpu(), **{**kw, "seed": 0, "time_warp_mode": mode})
        comp = torch_ops(mel, lens_host, rows, mode)
        scale = float(mel.abs().max())
        checks[mode] = {"max_abs_diff_vs_host_path_over_max_abs_mel": float((got.cpu() - host).abs().max()) / scale,
                        "bit_identical_to_host_path": round(float((got.cpu().view(torch.int32) == host.view(torch.int32)).float().mean()), 6),
                        "max_abs_diff_vs_torch_ops_over_max_abs_mel": float((got - comp).abs().max()) / scale}

    for fn in list(legs.values()) + list(slow.values()):
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(legs) + list(slow)}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(train_of(fn, args.reps))
        for k, fn in slow.items():
            ms[k].append(train_of(fn, 2))
    nbytes = 2 * mel.numel() * 4
    rec = {"what": "specaug", "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "shape": [B, MELS, FRAMES], "lengths": [min(lens_host), max(lens_host)], "warped_utterances": int((params[W][:, 0] > 0).sum()),
           "recipe": {"time_warp_window": W, "n_freq_masks": N_FREQ, "freq_mask_width": 27, "n_time_masks": N_TIME, "time_mask_ratio": 0.05},
           "bytes_moved": nbytes, "rounds": args.rounds, "calls_per_train": args.reps, "training_step_ms_for_scale": TRAIN_STEP_MS,
           "agreement": checks}
    for k, v in ms.items():
        rec[k + "_ms_per_call"] = spread(v)
        if k.startswith("apply_"):
            rec[k + "_TB_per_s"] = round(nbytes / (statistics.median(v) * 1e-3) / 1e12, 3)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump([rec], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
