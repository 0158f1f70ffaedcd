"""Same-box timing of self-distillation between exits (csrc/distill.hip; ``exit_training_losses``) in the training step of the default
model: 12 layers (6 exits x 2), B = 64, mel 80 x 1027 (T' = 256, V = 256), dropout 0.1, bf16x3 -- forward, loss, backward, gradient
clipping, fused AdamW, as tools/train_step_time.py runs it.

    python tools/distill_time.py [--rounds 7] [--steps 5] [--reps 50] [--out profiles/distill_time.json]

* ``step``: one process, the two losses in turn -- ``exit_ctc_losses(out).sum()`` and ``exit_training_losses(out, ..., "last", tau=2)``
  with ``ctc.sum() + 0.5 * kd.sum()`` -- each measured ``--rounds`` times as a train of ``--steps`` steps between two device
  synchronisations (host clock), after three warm-up steps of each.  Alternating them puts both under the same box noise; the
  spread of each (min .. max over the rounds) is what their difference has to be read against.
* ``launch``: the two distillation entries alone on the encoder output of that model ([6, 64, 256, 256]): device events around a
  train of ``--reps`` calls, per call -- the forward (two kernels), the backward adding into a gradient buffer (accumulate = 1, as
  the training node runs it) and writing one (accumulate = 0) -- with the bytes each has to move and the rate that makes.
  ``eec_ctc_loss_backward``'s own time on the same buffers is the yardstick beside them.
There is no pass mark: the record is the finding.  A run without a HIP device fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from early_exit_transformer_amd import ctc, synth  # noqa: E402
from early_exit_transformer_amd.model import Early_conformer, encoder_lengths, exit_ctc_losses, exit_training_losses  # noqa: E402

B, FRAMES, TAU, WEIGHT = 64, 1027, 2.0, 0.5


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def train_of(fn, reps):
    """Device milliseconds per call of a train of ``reps`` calls (events on the current stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_time.py measures on a HIP device; none found")

    m = Early_conformer(device="cuda", **bench.CFG)
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed=2, style="init"))
    m = m.cuda().train()
    m.train_passes = 3
    params = list(m.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.1, fused=True)
    mel, lens = synth.synth_mel(B, 80, FRAMES, seed=0).cuda(), torch.full((B,), FRAMES)
    tgt, tl = synth.synth_targets(B, 42, 256, seed=0)
    tgt, tl = tgt.cuda(), tl.cuda()
    with torch.no_grad():
        t_out = m(mel, lens).size(2)
    frame_len = encoder_lengths(lens.cuda(), t_out)

    def loss_ctc(out):
        return exit_ctc_losses(out, tgt, tl).sum()

    def loss_distill(out):
        c, kd = exit_training_losses(out, tgt, tl, frame_len, "last", TAU)
        return c.sum() + WEIGHT * kd.sum()

    def step(loss_fn):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(m(mel, lens))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        return loss

    legs = {"ctc": loss_ctc, "ctc_plus_distill": loss_distill}
    for fn in legs.values():
        for _ in range(3):
            step(fn)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(fn)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    info = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}
    rec_step = {"what": "step", "model": "default (6 exits x 2 layers, d_model 256)", "batch": B, "mel_frames": FRAMES, "teacher": "last",
                "temperature": TAU, "weight": WEIGHT, "rounds": args.rounds, "steps_per_round": args.steps,
                "ctc_ms_per_step": spread(ms["ctc"]), "ctc_plus_distill_ms_per_step": spread(ms["ctc_plus_distill"])}
    rec_step["added_ms_per_step_median"] = round(rec_step["ctc_plus_distill_ms_per_step"]["median"] - rec_step["ctc_ms_per_step"]["median"], 4)
    print(json.dumps(rec_step))

    # the entries alone, on this model's encoder output
    with torch.no_grad():
        x = m(mel, lens).float().contiguous()
    E, _, T, V = x.shape
    teacher = ctc._teacher_map("last", E)
    g = torch.full((E,), WEIGHT, device="cuda")
    ones = torch.ones((E,), device="cuda")
    dx = torch.zeros_like(x)
    row_bytes = B * T * V * 4
    students = sum(k >= 0 for k in teacher)
    # the CTC backward on the same buffers (each call needs its own forward: the forward is timed alone and taken out)
    xg = x.clone().requires_grad_(True)

    def ctc_fwd():
        return exit_ctc_losses(xg, tgt, tl)

    def ctc_fwd_bwd():
        exit_ctc_losses(xg, tgt, tl).backward(ones)
        xg.grad = None

    launches = {
        "distill_forward": (lambda: ctc._distill_forward(x, frame_len, teacher, TAU), E * row_bytes),
        "distill_backward_accumulate": (lambda: ctc._distill_backward(x, frame_len, teacher, TAU, g, True, dx), (E + 2 * students) * row_bytes),
        "distill_backward_write": (lambda: ctc._distill_backward(x, frame_len, teacher, TAU, g, False, dx), (E + E) * row_bytes),
        "ctc_loss_forward": (ctc_fwd, None),
        "ctc_loss_forward_and_backward": (ctc_fwd_bwd, None),
    }
    rec_launch = {"what": "launch", "shape": [E, B, T, V], "teacher": "last", "temperature": TAU, "calls_per_train": args.reps, "trains": 5}
    for name, (fn, nbytes) in launches.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per_call = [train_of(fn, args.reps) for _ in range(5)]
        rec_launch[name + "_ms_per_call"] = spread(per_call)
        if nbytes:
            rec_launch[name + "_bytes"] = nbytes
            rec_launch[name + "_GB_per_s"] = round(nbytes / (statistics.median(per_call) * 1e-3) / 1e9, 1)
    rec_launch["distill_forward_plus_backward_accumulate_ms"] = round(
        rec_launch["distill_forward_ms_per_call"]["median"] + rec_launch["distill_backward_accumulate_ms_per_call"]["median"], 4)
    print(json.dumps(rec_launch))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump([info, rec_step, rec_launch], f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
