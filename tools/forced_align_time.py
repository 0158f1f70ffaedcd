"""Same-box timing of CTC forced alignment in the standard topology (``ctc_forced_align``, csrc/ctc_forced_align.hip) at the default
model's emissions: E x B = 6 x 64 = 384 emissions of T' = 256 frames over V = 256 tokens.

    python tools/forced_align_time.py [--rounds 7] [--out profiles/forced_align_time.json]

Shapes: the 3840 hypotheses (6 exits x 64 utterances x 10 beams, the beams of one utterance next to each other) of the benchmarked
batch at about 85 and about 200 tokens a row, and 384 hypotheses, one per emission, at about 85.
Medians over ``--rounds`` alternating rounds in one process (every variant once per round), device time between events:
* ``ctc_forced_align`` as called (the launch, the output and workspace allocations included);
* the existing ``ctc_align`` (``eec_ctc_align``: the reference's one-frame-per-token trellis) on the same rows;
* the same recurrence and walk back written with torch ops on the device, one step per frame over [H, 2S + 1] (its bits are
  compared with the kernel's);
* the NumPy host path on a slice of 32 rows, host clock.
The emissions are log_softmax of scaled noise and the rows random tokens: timings only, no statement about alignment accuracy.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from early_exit_transformer_amd import capi, ctc_forced_align  # noqa: E402
from early_exit_transformer_amd.model import ctc_align  # noqa: E402

E, B, BEAM, TQ, V = 6, 64, 10, 256, 256
NEG = float("-inf")


def rows(H, mean_len, seed):
    """[H, S] int32 random labels, lengths mean_len - 8 .. mean_len + 8 (S = mean_len + 8); an adjacent repeat is replaced, so few
    remain."""
    g = torch.Generator().manual_seed(seed)
    S = mean_len + 8
    tokens = torch.randint(1, V, (H, S), generator=g, dtype=torch.int32)
    same = tokens[:, 1:] == tokens[:, :-1]
    tokens[:, 1:][same] = (tokens[:, 1:][same] % (V - 1)) + 1  # a repeat becomes its successor label: R stays near 0
    lens = torch.randint(mean_len - 8, S + 1, (H,), generator=g, dtype=torch.int32)
    return tokens, lens


def torch_ops(logp, tokens, tok_len, em_index):
    """The statement of include/eec.h with tensor ops on the device, one step per frame; lengths all T'.  Returns
    ``(frame_token, path_score)``."""
    dev = logp.device
    H, S = tokens.shape
    Tq = logp.size(1)
    NS = 2 * S + 1
    N = tok_len.to(torch.int64)
    s_idx = torch.arange(NS, device=dev)[None, :]
    lab = torch.zeros((H, NS), dtype=torch.int64, device=dev)
    lab[:, 1::2] = tokens.to(torch.int64)
    lab = torch.where(s_idx <= 2 * N[:, None], lab, torch.zeros_like(lab))
    skip = torch.zeros((H, NS), dtype=torch.bool, device=dev)
    skip[:, 3::2] = tokens[:, 1:] != tokens[:, :-1]
    skip &= s_idx <= 2 * N[:, None] - 1
    ei = em_index.to(torch.int64)
    rows_ = torch.arange(H, device=dev)
    a = torch.full((H, NS), NEG, device=dev)
    a[:, 0] = logp[ei, 0, 0]
    a[:, 1] = logp[ei, 0, lab[:, 1]]
    neg1, neg2 = torch.full((H, 1), NEG, device=dev), torch.full((H, 2), NEG, device=dev)
    dec = torch.zeros((Tq, H, NS), dtype=torch.uint8, device=dev)
    one, two_ = torch.ones((), dtype=torch.uint8, device=dev), torch.full((), 2, dtype=torch.uint8, device=dev)
    for t in range(1, Tq):
        e = logp[ei, t, :].gather(1, lab)
        step = torch.cat([neg1, a[:, :-1]], 1)
        take = step > a
        best, d = torch.where(take, step, a), torch.where(take, one, torch.zeros_like(dec[t]))
        two = torch.cat([neg2, a[:, :-2]], 1)
        take = skip & (two > best)
        best, d = torch.where(take, two, best), torch.where(take, two_, d)
        a = best + e
        dec[t] = d
    hi, lo = a[rows_, 2 * N], a[rows_, 2 * N - 1]
    s = torch.where(hi > lo, 2 * N, 2 * N - 1)
    score = torch.where(hi > lo, hi, lo)
    state = torch.empty((H, Tq), dtype=torch.int64, device=dev)
    for t in range(Tq - 1, 0, -1):
        state[:, t] = s
        s = s - dec[t, rows_, s].to(torch.int64)
    state[:, 0] = s
    return torch.where(state % 2 == 1, state // 2, torch.full_like(state, -1)).to(torch.int32), score


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "forced_align_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__, "n_em": E * B, "Tq": TQ,
              "V": V, "rounds": args.rounds, "inputs": "log_softmax(3 * noise), random rows: timings only"}
    g = torch.Generator().manual_seed(384)
    logp = torch.log_softmax(torch.randn(E * B, TQ, V, generator=g) * 3.0, -1).to(dev)
    beams = torch.arange(E * B, dtype=torch.int32).repeat_interleave(BEAM)  # the beams of an utterance follow each other
    shapes = {}
    for name, H, mean_len, idx in (("3840 rows, ~85 tokens", E * B * BEAM, 85, beams), ("3840 rows, ~200 tokens", E * B * BEAM, 200, beams),
                                   ("384 rows, ~85 tokens", E * B, 85, torch.arange(E * B, dtype=torch.int32))):
        tokens, lens = rows(H, mean_len, seed=H + mean_len)
        shapes[name] = (tokens.to(dev), lens.to(dev), idx.to(dev))
    lib = capi.load()
    record["workspace_bytes"] = {name: lib.eec_ctc_forced_align_workspace_bytes(t.size(0), TQ, t.size(1)) for name, (t, _, _) in shapes.items()}
    variants, same = {}, {}
    for name, (tokens, lens, idx) in shapes.items():
        variants[f"ctc_forced_align {name}"] = lambda a=(tokens, lens, idx): ctc_forced_align(logp, *a)
        variants[f"ctc_align {name}"] = lambda a=(tokens, lens, idx): ctc_align(logp, a[0].to(torch.int64), a[1], a[2])
        variants[f"torch ops {name}"] = lambda a=(tokens, lens, idx): torch_ops(logp, *a)
        got, ref = ctc_forced_align(logp, tokens, lens, idx), torch_ops(logp, tokens, lens, idx)  # warm-up, and the bits
        same[name] = bool(int(got.status.sum()) == 0 and torch.equal(got.frame_token, ref[0]) and torch.equal(got.path_score, ref[1]))
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    record["device_ms"] = {name: med(v) for name, v in times.items()}
    record["torch_ops_bits_equal_kernel"] = same
    for name in shapes:
        k = record["device_ms"][f"ctc_forced_align {name}"]["median"]
        record.setdefault("torch_ops_over_kernel", {})[name] = round(record["device_ms"][f"torch ops {name}"]["median"] / k, 1)
        record.setdefault("ctc_align_over_kernel", {})[name] = round(record["device_ms"][f"ctc_align {name}"]["median"] / k, 2)
    tokens, lens, idx = (t[:32].cpu() for t in shapes["3840 rows, ~85 tokens"])
    host_x = logp[:4].cpu()
    ctc_forced_align(host_x, tokens, lens, idx)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctc_forced_align(host_x, tokens, lens, idx)
        host.append(1e3 * (time.perf_counter() - t0))
    record["numpy_host_path_ms"] = {"rows": 32, "tokens": "~85", **med(host)}
    print(json.dumps(record, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
