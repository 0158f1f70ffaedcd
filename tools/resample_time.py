"""Timing of resampling / speed perturbation on the device (csrc/resample.hip; ``early_exit_transformer_amd/augment.py``) at the
benchmarked batch as waveforms, [64, 164 000] samples with lengths of 100 000 to 164 000, under the factors 0.9 / 1.0 / 1.1 at 16 kHz,
and of 44.1 kHz -> 16 kHz at [8, 441 000].

    python tools/resample_time.py [--rounds 7] [--reps 20] [--out profiles/resample_time.json]

One process; the legs run in turn, ``--rounds`` times, each as a train of ``--reps`` calls between two device events (alternating puts
all of them under the same box noise); the record holds the median, minimum and maximum per call:
* ``draw``: eec_speed_draw alone, through ctypes on preallocated tensors;
* ``resample_{all_0.9,all_1.1,thirds,all_copy}``: eec_resample alone on prescribed choices -- every utterance at 9 / 10, every one at
  11 / 10, a third at each factor, every one copied --, with the bytes it has to move (the valid input once, the whole output once)
  over its median time;
* ``plain_copy``: ``out.copy_(wave)``, what moving a batch of that size costs under this way of timing;
* ``speed_perturb``: the Python entry, draw and resampling and the allocations, as a training loop calls it;
* ``torch_ops_thirds``: the same resampling written with torch ops on the device -- per ratio group ``F.pad``, ``F.conv1d(stride=o)``
  with the n phase rows, transpose and reshape -- from choices already on the host;
* ``resample_44k1_16k`` and ``torch_ops_44k1_16k``: 441 -> 160 at [8, 441 000].
For scale the record repeats the default model's training step, 22.9 ms (README).  The device results are also compared with the
host path on a slice and with the torch composition.  Records, not targets; a run without a HIP device fails.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import augment, capi  # noqa: E402

B, L = 64, 164000
FACTORS = (0.9, 1.0, 1.1)
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


def dense_kernel(plan, r, dev):
    """The n phase rows of ratio ``r`` as a conv1d weight [n, 1, K]."""
    o, n, width, K, first, count, weights = plan.table(r)
    h = np.zeros((n, K), dtype=np.float32)
    for j in range(n):
        h[j, first[j]:first[j] + count[j]] = weights[j]
    return o, n, width, torch.from_numpy(h)[:, None, :].to(dev)


def torch_ops(wave, out, groups):
    """``groups``: (row indices on the device, o, n, width, kernel, width of the result) per ratio; lengths are not honoured (the
    padding is resampled with the rest), which only makes this leg cheaper."""
    out.zero_()
    for idx, o, n, width, kernel, m in groups:
        x = wave if idx is None else wave[idx]
        if kernel is None:
            y = x
        else:
            y = F.conv1d(F.pad(x[:, None], (width, width + o)), kernel, stride=o).transpose(1, 2).reshape(x.shape[0], -1)[:, :m]
        if idx is None:
            out[:, :y.shape[1]] = y
        else:
            out[idx, :y.shape[1]] = y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py measures on a HIP device; none found")

    lib = capi.load()
    dev = torch.device("cuda", 0)
    st = capi.stream_ptr(dev)
    gen = torch.Generator().manual_seed(0)
    wave = (torch.randn(B, L, generator=gen) * 0.1).to(dev)
    lens_host = [L - (1009 * b) % 64001 for b in range(B)]  # ragged: 100 000 .. 164 000 samples
    lens = torch.tensor(lens_host, dtype=torch.int64, device=dev)
    plan = augment.resample_plan(augment.speed_ratios(FACTORS, 16000))
    image = plan.on(dev)
    L_out = plan.out_samples(L)
    out = torch.empty((B, L_out), device=dev)
    out_len = torch.empty((B,), dtype=torch.int64, device=dev)
    drawn = torch.empty((B,), dtype=torch.int32, device=dev)
    choices = {"all_0.9": [0] * B, "all_1.1": [2] * B, "thirds": [b % 3 for b in range(B)], "all_copy": [1] * B}
    choice_dev = {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in choices.items()}

    def draw():
        capi.check(lib.eec_speed_draw(lens.data_ptr(), B, L, 1, 0, image.data_ptr(), drawn.data_ptr(), out_len.data_ptr(), st), "eec_speed_draw")

    def run(kind):
        capi.check(lib.eec_resample(wave.data_ptr(), lens.data_ptr(), choice_dev[kind].data_ptr(), B, L, image.data_ptr(), out.data_ptr(), L_out,
                                    out_len.data_ptr(), st), "eec_resample")

    def moved(kind):
        n_out = [(plan.ratios[c][1] * n + plan.ratios[c][0] - 1) // plan.ratios[c][0] for n, c in zip(lens_host, choices[kind])]
        return 4 * (sum(lens_host) + B * L_out), n_out

    # 44.1 kHz -> 16 kHz
    B2, L2 = 8, 441000
    wave2 = (torch.randn(B2, L2, generator=gen) * 0.1).to(dev)
    plan2 = augment.resample_plan([(44100, 16000)])
    image2, L2_out = plan2.on(dev), plan2.out_samples(L2)
    out2, zeros2 = torch.empty((B2, L2_out), device=dev), torch.zeros(B2, dtype=torch.int32, device=dev)

    def run2():
        capi.check(lib.eec_resample(wave2.data_ptr(), None, zeros2.data_ptr(), B2, L2, image2.data_ptr(), out2.data_ptr(), L2_out, None, st),
                   "eec_resample")

    groups = []
    for r in range(3):
        idx = torch.tensor([b for b in range(B) if choices["thirds"][b] == r], device=dev)
        if plan.ratios[r] == (1, 1):
            groups.append((idx, 1, 1, 0, None, L))
        else:
            o, n, width, kernel = dense_kernel(plan, r, dev)
            groups.append((idx, o, n, width, kernel, (n * L + o - 1) // o))
    o2, n2, width2, kernel2 = dense_kernel(plan2, 0, dev)
    groups2 = [(None, o2, n2, width2, kernel2, L2_out)]
    ref, ref2 = torch.empty_like(out), torch.empty_like(out2)

    legs = {"draw": draw, "plain_copy": lambda: ref.copy_(out)}
    for kind in choices:
        legs[f"resample_{kind}"] = lambda kind=kind: run(kind)
    legs["speed_perturb"] = lambda: augment.speed_perturb(wave, lens, seed=1, factors=FACTORS)
    legs["resample_44k1_16k"] = run2
    slow = {"torch_ops_thirds": lambda: torch_ops(wave, ref, groups), "torch_ops_44k1_16k": lambda: torch_ops(wave2, ref2, groups2)}

    # agreement: the host path on a slice, the torch composition where an utterance is full length (it ignores the lengths)
    checks = {}
    run("thirds")
    torch.cuda.synchronize()
    got = out[:3, :20000].cpu()
    host, _, _ = augment.speed_perturb(wave[:3, :18000].cpu(), torch.tensor([18000] * 3), seed=0, choice=torch.tensor(choices["thirds"][:3]), factors=FACTORS)
    dev_small, _, _ = augment.speed_perturb(wave[:3, :18000].contiguous(), torch.tensor([18000] * 3), seed=0, choice=choice_dev["thirds"][:3], factors=FACTORS)
    checks["bit_identical_to_host_path"] = bool(np.array_equal(dev_small.cpu().numpy().view(np.int32), host.numpy().view(np.int32)))
    checks["a_slice_of_the_batch_equals_its_head_alone"] = bool(torch.equal(got[:, :15000], dev_small.cpu()[:, :15000]))
    torch_ops(wave, ref, groups)
    full = lens_host.index(L)
    m = (plan.ratios[choices["thirds"][full]][1] * L + plan.ratios[choices["thirds"][full]][0] - 1) // plan.ratios[choices["thirds"][full]][0]
    checks["max_abs_diff_vs_torch_ops_over_max_abs_wave"] = float((out[full, :m - 64] - ref[full, :m - 64]).abs().max() / wave.abs().max())
    run2()
    torch_ops(wave2, ref2, groups2)
    checks["max_abs_diff_vs_torch_ops_44k1_16k_over_max_abs_wave"] = float((out2 - ref2).abs().max() / wave2.abs().max())

    for fn in list(legs.values()) + list(slow.values()):
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(legs) + list(slow)}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(train_of(fn, args.reps))
        for k, fn in slow.items():
            ms[k].append(train_of(fn, 2))
    rec = {"what": "resample", "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "shape": [B, L], "out_width": L_out, "lengths": [min(lens_host), max(lens_host)], "factors": list(FACTORS), "sample_rate": 16000,
           "ratios": [list(r) for r in plan.ratios], "shape_44k1_16k": [B2, L2], "out_width_44k1_16k": L2_out,
           "rounds": args.rounds, "calls_per_train": args.reps, "training_step_ms_for_scale": TRAIN_STEP_MS, "agreement": checks}
    for k, v in ms.items():
        rec[k + "_ms_per_call"] = spread(v)
        nbytes = None
        if k.startswith("resample_") and k[9:] in choices:
            nbytes, _ = moved(k[9:])
        elif k == "resample_44k1_16k":
            nbytes = 4 * B2 * (L2 + L2_out)
        elif k == "plain_copy":
            nbytes = 8 * B * L_out
        if nbytes is not None:
            rec[k + "_bytes_moved"] = nbytes
            rec[k + "_TB_per_s"] = round(nbytes / (statistics.median(v) * 1e-3) / 1e12, 3)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump([rec], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
