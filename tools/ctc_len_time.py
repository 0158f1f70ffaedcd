"""Same-box timing of the CTC entries with per-utterance input lengths (csrc/ctc_len.hip) beside the entries without, at the
benchmark's loss shape: log-probs [6, 64, 256, 256], targets of length 42; the two decoders on the same 384 sequences.

    python tools/ctc_len_time.py [--rounds 7] [--reps 50] [--out profiles/ctc_input_len_time.json]

Per entry four legs: the existing entry, the ``_len`` entry with NULL lengths (the same launches), with lengths all T', and with
lengths uniform in [T'/2, T'].  The legs of an entry are measured in turn, ``--rounds`` times each, as device events around a train
of ``--reps`` calls on the current stream; min .. max over the rounds is what a difference between two legs has to be read against.
The forward + backward pair is one forward and one backward call per repetition on the same workspace.
These are records, not targets: there is no pass mark.  A run without a HIP device fails.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import capi, synth  # noqa: E402

E, B, T, V, S = 6, 64, 256, 256, 42
BEAM = 10


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


def measure(legs, rounds, reps):
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(train_of(fn, reps))
    return {k + "_ms_per_call": spread(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_input_len_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_len_time.py measures on a HIP device; none found")
    dev = torch.device("cuda")
    lib = capi.load()
    st = capi.stream_ptr(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(E, B, T, V, generator=g) * 3.0, -1).to(dev)
    tgt, tl = synth.synth_targets(B, S, V, seed=0)
    tgt, tl = tgt.to(dev), tl.to(dev)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    ragged = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    lens = {"len_null": None, "len_all_T": full, "len_uniform_half_to_T": ragged}
    nll = torch.empty(E * B, device=dev)
    out = torch.empty(E, device=dev)
    ones = torch.ones(E, device=dev)
    dlogp = torch.empty_like(x)
    ws, ws_ptr = capi.aligned_ws(lib.eec_ctc_backward_workspace_bytes(E, B, T, S), dev)
    xp, tp, lp = x.data_ptr(), tgt.data_ptr(), tl.data_ptr()

    def ptr(t):
        return None if t is None else t.data_ptr()

    def loss(il, with_len):
        if with_len:
            return lambda: capi.check(lib.eec_ctc_loss_len(xp, tp, lp, ptr(il), E, B, T, V, S, 0, nll.data_ptr(), out.data_ptr(), st), "loss")
        return lambda: capi.check(lib.eec_ctc_loss(xp, tp, lp, E, B, T, V, S, 0, nll.data_ptr(), out.data_ptr(), st), "loss")

    def pair(il, with_len):
        def run_len():
            capi.check(lib.eec_ctc_loss_forward_len(xp, tp, lp, ptr(il), E, B, T, V, S, 0, nll.data_ptr(), out.data_ptr(), ws_ptr, st), "fwd")
            capi.check(lib.eec_ctc_loss_backward_len(xp, tp, lp, ptr(il), E, B, T, V, S, 0, nll.data_ptr(), ws_ptr, ones.data_ptr(),
                                                     dlogp.data_ptr(), st), "bwd")

        def run():
            capi.check(lib.eec_ctc_loss_forward(xp, tp, lp, E, B, T, V, S, 0, nll.data_ptr(), out.data_ptr(), ws_ptr, st), "fwd")
            capi.check(lib.eec_ctc_loss_backward(xp, tp, lp, E, B, T, V, S, 0, nll.data_ptr(), ws_ptr, ones.data_ptr(), dlogp.data_ptr(), st), "bwd")
        return run_len if with_len else run

    # the decoders: the same rows as 384 sequences, lengths per sequence (every exit of an utterance shares its length)
    N = E * B
    tokens = torch.empty((N, T), dtype=torch.int32, device=dev)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    scores = torch.empty((N,), device=dev)
    bws = torch.empty((lib.eec_ctc_beam_workspace_bytes(N, T),), dtype=torch.uint8, device=dev)
    seq_lens = {k: (None if v is None else v.repeat(E)) for k, v in lens.items()}

    def greedy(el, with_len):
        if with_len:
            return lambda: capi.check(lib.eec_greedy_ctc_len(xp, ptr(el), N, T, V, 0, tokens.data_ptr(), counts.data_ptr(), st), "greedy")
        return lambda: capi.check(lib.eec_greedy_ctc(xp, N, T, V, 0, tokens.data_ptr(), counts.data_ptr(), st), "greedy")

    def beam(el, with_len):
        if with_len:
            return lambda: capi.check(lib.eec_ctc_beam_decode_len(xp, ptr(el), N, T, V, 0, BEAM, 0.95, 0, bws.data_ptr(), tokens.data_ptr(),
                                                                  counts.data_ptr(), scores.data_ptr(), st), "beam")
        return lambda: capi.check(lib.eec_ctc_beam_decode_ex(xp, N, T, V, 0, BEAM, 0.95, 0, bws.data_ptr(), tokens.data_ptr(), counts.data_ptr(),
                                                             scores.data_ptr(), st), "beam")

    info = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__, "rounds": args.rounds,
            "calls_per_train": args.reps, "lengths_uniform_half_to_T": {"min": int(ragged.min()), "max": int(ragged.max()),
                                                                       "mean": round(float(ragged.float().mean()), 1)}}
    records = [info]
    with torch.cuda.device(dev):
        for what, make, shape, table, reps in (("eec_ctc_loss", loss, [E, B, T, V], lens, args.reps),
                                               ("eec_ctc_loss_forward + eec_ctc_loss_backward", pair, [E, B, T, V], lens, args.reps),
                                               ("eec_greedy_ctc", greedy, [N, T, V], seq_lens, args.reps),
                                               ("eec_ctc_beam_decode_ex (beam 10)", beam, [N, T, V], seq_lens, max(1, args.reps // 10))):
            legs = {"existing": make(None, False)}
            legs.update({k: make(v, True) for k, v in table.items()})
            rec = {"what": what, "shape": shape, "target_len": S if make in (loss, pair) else None}
            rec.update(measure(legs, args.rounds, reps))
            print(json.dumps(rec), flush=True)
            records.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
