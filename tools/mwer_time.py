"""Timing of MWER training of the CTC exits (csrc/ctc_mwer.hip; ``mwer_nbest``, ``exit_mwer_losses``) on the encoder output of the
default model with synthetic weights: [6, 64, 256, 256] (6 exits, B = 64, T' = 256, V = 256), lists from ``mwer_nbest`` at N = 4 and
N = 10 (beam 10) against ``synth_targets`` references.

    python tools/mwer_time.py [--rounds 7] [--reps 3] [--out profiles/mwer_time.json]

One process; per list size the legs run in turn, ``--rounds`` times, each as a train of ``--reps`` calls between two device events
(alternating puts all of them under the same box noise); the record holds the median, minimum and maximum per call:
* ``mwer_nbest``: the beam search with N-best, the length bookkeeping (one host synchronisation for the token pitch) and the edit
  distances;
* ``forward``: ``exit_mwer_losses`` without a gradient (the alphas of all lattices, the coefficients, the means);
* ``forward_backward``: the same with ``.sum().backward()``;
* ``naive_composition``: N calls of the existing ``exit_ctc_losses`` forward and backward pair, call i on the rank-i hypotheses of
  the last exit as targets -- what composing the loss from the per-target CTC entries would at least cost (it would also need N
  gradient buffers and a weighted sum, and still not have the exact log-likelihoods).
The weights are synthetic: the record says what the launches cost, nothing about any error rate.  There is no pass mark; a run
without a HIP device fails.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from early_exit_transformer_amd import capi, synth  # noqa: E402
from early_exit_transformer_amd.model import Early_conformer, exit_ctc_losses, exit_mwer_losses, mwer_nbest  # noqa: E402

B, FRAMES, BEAM = 64, 1027, 10


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mwer_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mwer_time.py measures on a HIP device; none found")

    m = Early_conformer(device="cuda", **bench.CFG)
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed=2, style="init"))
    m = m.cuda().eval()
    mel, lens = synth.synth_mel(B, 80, FRAMES, seed=0).cuda(), torch.full((B,), FRAMES)
    tgt, tl = synth.synth_targets(B, 42, 256, seed=0)
    tgt, tl = tgt.cuda(), tl.cuda()
    with torch.no_grad():
        x = m(mel, lens).float().contiguous()
    E, _, T, V = x.shape
    xg = x.clone().requires_grad_(True)
    ones = torch.ones((E,), device="cuda")
    records = [{"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
                "weights": "synthetic (synth_state_dict, style init): timings only, no error rate is claimed"}]
    for N in (4, 10):
        lists = mwer_nbest(x, tgt, tl, nbest=N, beam_size=BEAM)
        L = lists.tokens.size(3)
        naive_tl = lists.lengths[E - 1].clamp(min=0).to(torch.int64)  # [B, N]
        naive_tg = lists.tokens[E - 1].to(torch.int64)                # [B, N, L]

        def forward():
            with torch.no_grad():
                return exit_mwer_losses(x, lists.tokens, lists.lengths, lists.risk)

        def forward_backward():
            exit_mwer_losses(xg, lists.tokens, lists.lengths, lists.risk).backward(ones)
            xg.grad = None

        def naive():
            for i in range(N):
                exit_ctc_losses(xg, naive_tg[:, i].contiguous(), naive_tl[:, i].contiguous()).backward(ones)
            xg.grad = None

        legs = {"mwer_nbest": lambda: mwer_nbest(x, tgt, tl, nbest=N, beam_size=BEAM), "forward": forward,
                "forward_backward": forward_backward, "naive_composition": naive}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k].append(train_of(fn, args.reps))
        present = lists.lengths >= 0
        rec = {"what": "mwer", "shape": [E, B, T, V], "nbest": N, "beam": BEAM, "token_pitch": L,
               "present_hypotheses": int(present.sum()), "mean_tokens": round(float(lists.lengths[present].float().mean()), 1),
               "workspace_bytes": int(capi.load().eec_ctc_mwer_workspace_bytes(E, B, T, N, L)),
               "loss_per_exit": [round(v, 5) for v in forward().tolist()], "rounds": args.rounds, "calls_per_train": args.reps}
        for k, v in ms.items():
            rec[k + "_ms_per_call"] = spread(v)
        rec["backward_ms_median"] = round(rec["forward_backward_ms_per_call"]["median"] - rec["forward_ms_per_call"]["median"], 4)
        print(json.dumps(rec))
        records.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
