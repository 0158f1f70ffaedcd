"""Same-box timing of adaptive inference (``forward_adaptive``, csrc/exit_stats.hip) beside what it replaces, on the default model
(6 exits x 2 layers, d_model 256, synthetic weights) at B = 64, T = 1027 (T' = 256).

    python tools/adaptive_time.py [--rounds 7] [--reps 10] [--out profiles/adaptive_exit_time.json]

* ``forward``: ``forward`` (all exits, one call into the library) against ``forward_adaptive`` with PRESCRIBED routings -- every
  utterance to the last exit (the pure overhead of the walk: per-exit launches, statistics, routes and host reads), every utterance
  out at exit 0, and the utterances spread evenly over the exits, with and without ``compact``.  Host milliseconds per call, the
  device drained at both ends: the walk's host reads are part of its cost.  Once at B = 64 and once at B = 256: 64 utterances are a
  single round of row tiles over the chip, where fewer rows per group do not make a group shorter.
* ``statistics``: the eec_exit_stats launch pair alone at [6, 64, 256, 256] (device events around a train of calls).
* ``decode``: ``ctc_beam_decode`` (beam 10) of all 384 exit x utterance sequences against the 64 an adaptive pass hands over.

The legs of a record are measured in turn, ``--rounds`` times each; min .. max over the rounds is what a difference between two legs
has to be read against.  These are records, not targets: there is no pass mark, and with synthetic weights nothing here says
anything about accuracy.  A run without a HIP device fails.
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
from early_exit_transformer_amd import ctc, synth  # noqa: E402
from early_exit_transformer_amd.model import Early_conformer  # noqa: E402

E, B, T, V = 6, 64, 1027, 256
KW = dict(src_pad_idx=0, n_enc_exits=E, enc_voc_size=V, dec_voc_size=V, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
          n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31, device="cuda")


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def host_train(fn, reps):
    """Host milliseconds per call of ``reps`` calls, the device drained before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def device_train(fn, reps):
    """Device milliseconds per call of a train of ``reps`` calls (events on the current stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(legs, rounds, reps, train):
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(train(fn, reps))
    return {k + "_ms_per_call": spread(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_exit_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_time.py measures on a HIP device; none found")
    model = Early_conformer(**KW).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0, style="trained"))
    model = model.cuda()
    records = [{"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__, "rounds": args.rounds,
                "calls_per_train": args.reps, "model": {k: v for k, v in KW.items() if k != "device"}, "B": B, "T": T,
                "precision": model.precision}]
    with torch.no_grad():
        # B = 64 is one round of row tiles over the chip (the forward takes 2.6 ms at B = 1 and 3.2 ms at B = 64: profiles/
        # r04_batch_sweep_f16x3.txt), so there the depth decides the time; the larger batch shows what compaction saves
        for nb in (B, 4 * B):
            mel, lens = synth.synth_mel(nb, 80, T, seed=0).cuda(), synth.synth_lengths(nb, T, seed=0)
            routings = {"all_last": torch.full((nb,), E - 1), "all_exit0": torch.zeros(nb, dtype=torch.int64),
                        "spread_evenly": torch.arange(nb) % E}
            legs = {"forward": lambda: model(mel, lens)}
            for name, routing in routings.items():
                for compact in (True, False):
                    legs[f"adaptive_{name}_{'compact' if compact else 'whole_batch'}"] = \
                        lambda r=routing, c=compact: model.forward_adaptive(mel, lens, exit_of=r, compact=c)
            rec = {"what": "forward", "B": nb, "clock": "host, device drained at both ends"}
            rec.update(measure(legs, args.rounds, args.reps, host_train))
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del legs
        mel, lens = synth.synth_mel(B, 80, T, seed=0).cuda(), synth.synth_lengths(B, T, seed=0)
        routings = {"spread_evenly": torch.arange(B) % E}
        out = model(mel, lens)
        frames = ctc.encoder_lengths(lens.cuda(), out.size(2))

        rec = {"what": "statistics", "shape": list(out.shape), "clock": "device events"}
        rec.update(measure({"exit_statistics": lambda: ctc.exit_statistics(out, frames),
                            "exit_statistics_one_exit": lambda: ctc.exit_statistics(out[:1], frames)}, args.rounds, 5 * args.reps, device_train))
        print(json.dumps(rec), flush=True)
        records.append(rec)

        chosen = model.forward_adaptive(mel, lens, exit_of=routings["spread_evenly"]).logp
        every = out.reshape(E * B, out.size(2), V)
        rec = {"what": "decode", "beam": 10, "clock": "device events"}
        rec.update(measure({"ctc_beam_decode_384_sequences": lambda: ctc.ctc_beam_decode(every, beam_size=10, em_len=frames.repeat(E)),
                            "ctc_beam_decode_64_chosen": lambda: ctc.ctc_beam_decode(chosen, beam_size=10, em_len=frames)},
                           args.rounds, max(1, args.reps // 2), device_train))
        print(json.dumps(rec), flush=True)
        records.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
