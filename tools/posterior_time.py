"""Same-box timing of the CTC posteriors in the standard topology (``ctc_posteriors``, csrc/ctc_posterior.hip) at the default model's
emissions: E x B = 6 x 64 = 384 emissions of T' = 256 frames over V = 256 tokens -- the batch of tools/forced_align_time.py.

    python tools/posterior_time.py [--rounds 7] [--out profiles/ctc_posterior_time.json]

Shapes: the 3840 rows (6 exits x 64 utterances x 10 beams, the beams of one utterance next to each other) at about 85 and about
200 tokens a row, and 384 rows, one per emission, at about 85.
Medians over ``--rounds`` alternating rounds in one process (every variant once per round), device time between events:
* ``ctc_posteriors`` as called (the launch, the output and workspace allocations included), without and with ``want_gamma``;
* ``ctc_forced_align`` on the same rows;
* the same recursions and sums written with torch ops on the device, one step per frame over [H, 2S + 1], forward and backward
  (fp32 recursions with ``torch.logaddexp``, fp64 sums; its largest differences from the kernel are recorded).
The workspace per row is recorded too.  The emissions are log_softmax of scaled noise and the rows random tokens: timings only.
These are records, not targets: no time is promised for this kernel.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from early_exit_transformer_amd import capi, ctc_forced_align, ctc_posteriors  # noqa: E402

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
    """The statement of include/eec.h with tensor ops on the device, one step per frame each way; lengths all T'.  Returns
    ``(row_logp [H], tok_frames, tok_score, tok_start, tok_end, tok_start_var, tok_end_var [H, S])``; columns past a row's length
    hold unspecified values."""
    dev = logp.device
    H, S = tokens.shape
    Tq = logp.size(1)
    NS = 2 * S + 1
    N = tok_len.to(torch.int64)
    s_idx = torch.arange(NS, device=dev)[None, :]
    valid = s_idx <= 2 * N[:, None]
    lab = torch.zeros((H, NS), dtype=torch.int64, device=dev)
    lab[:, 1::2] = tokens.to(torch.int64)
    lab = torch.where(valid, lab, torch.zeros_like(lab))
    skip = torch.zeros((H, NS), dtype=torch.bool, device=dev)
    skip[:, 3::2] = tokens[:, 1:] != tokens[:, :-1]
    skip &= valid
    give = torch.zeros_like(skip)
    give[:, :-2] = skip[:, 2:]
    ei = em_index.to(torch.int64)
    rows_ = torch.arange(H, device=dev)
    neg = torch.full((H, 2), NEG, device=dev)
    ninf = torch.full((), NEG, device=dev)

    def left(v, n):
        return torch.cat([neg[:, :n], v[:, :-n]], 1)

    def right(v, n):
        return torch.cat([v[:, n:], neg[:, :n]], 1)

    alpha = torch.empty((Tq, H, NS), device=dev)
    a = torch.full((H, NS), NEG, device=dev)
    a[:, 0] = logp[ei, 0, 0]
    a[:, 1] = logp[ei, 0, lab[:, 1]]
    alpha[0] = a
    for t in range(1, Tq):
        v = torch.logaddexp(torch.logaddexp(a, left(a, 1)), torch.where(skip, left(a, 2), ninf))
        a = torch.where(valid, v + logp[ei, t, :].gather(1, lab), ninf)
        alpha[t] = a
    ll = torch.logaddexp(a[rows_, 2 * N], a[rows_, 2 * N - 1])[:, None]
    beta = torch.where((s_idx == 2 * N[:, None]) | (s_idx == 2 * N[:, None] - 1), torch.zeros((), device=dev), ninf)
    sums = [torch.zeros((H, S), dtype=torch.float64, device=dev) for _ in range(6)]
    leave = None
    for t in range(Tq - 1, -1, -1):
        e = logp[ei, t, :].gather(1, lab)
        g = torch.exp(alpha[t] + beta - ll)
        if t >= 1:
            enter = torch.logaddexp(left(alpha[t - 1], 1), torch.where(skip, left(alpha[t - 1], 2), ninf))
            f = torch.exp(enter + e + beta - ll)
        else:
            f = torch.where(s_idx == 1, g, torch.zeros_like(g))
        l = g if leave is None else torch.exp(alpha[t] + leave - ll)
        g, f, l, ex = (v[:, 1::2].double() for v in (g, f, l, e))
        sums[0] += g
        sums[1] += torch.where(g > 0, g * ex, torch.zeros_like(g))
        sums[2] += t * f
        sums[3] += float(t * t) * f
        sums[4] += (t + 1) * l
        sums[5] += float((t + 1) * (t + 1)) * l
        c = torch.where(valid, e + beta, ninf)
        one, two = right(c, 1), torch.where(give, right(c, 2), ninf)
        beta, leave = torch.logaddexp(torch.logaddexp(c, one), two), torch.logaddexp(one, two)
    return (ll[:, 0], sums[0].float(), sums[1].float(), sums[2].float(), sums[4].float(), (sums[3] - sums[2] * sums[2]).float(),
            (sums[5] - sums[4] * sums[4]).float())


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
                                                  "ctc_posterior_time.json"))
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
    record["workspace_bytes"] = {name: lib.eec_ctc_posteriors_workspace_bytes(t.size(0), TQ, t.size(1)) for name, (t, _, _) in shapes.items()}
    record["workspace_bytes_per_row"] = {name: lib.eec_ctc_posteriors_workspace_bytes(1, TQ, t.size(1)) for name, (t, _, _) in shapes.items()}
    variants, diff = {}, {}
    for name, (tokens, lens, idx) in shapes.items():
        variants[f"ctc_posteriors {name}"] = lambda a=(tokens, lens, idx): ctc_posteriors(logp, *a)
        variants[f"ctc_posteriors, gamma {name}"] = lambda a=(tokens, lens, idx): ctc_posteriors(logp, *a, want_gamma=True)
        variants[f"ctc_forced_align {name}"] = lambda a=(tokens, lens, idx): ctc_forced_align(logp, *a)
        variants[f"torch ops {name}"] = lambda a=(tokens, lens, idx): torch_ops(logp, *a)
        got, ref = ctc_posteriors(logp, tokens, lens, idx), torch_ops(logp, tokens, lens, idx)  # warm-up, and the differences
        inside = torch.arange(tokens.size(1), device=dev)[None, :] < lens[:, None]
        diff[name] = {"served": int((got.status == 0).sum()), "row_logp": float((got.row_logp - ref[0]).abs().max())}
        for k, field in enumerate(("tok_frames", "tok_score", "tok_start", "tok_end", "tok_start_var", "tok_end_var")):
            diff[name][field] = float(torch.where(inside, getattr(got, field) - ref[k + 1], torch.zeros_like(ref[k + 1])).abs().max())
        del got, ref
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    record["device_ms"] = {name: med(v) for name, v in times.items()}
    record["largest_difference_from_torch_ops"] = diff
    for name in shapes:
        k = record["device_ms"][f"ctc_posteriors {name}"]["median"]
        record.setdefault("torch_ops_over_kernel", {})[name] = round(record["device_ms"][f"torch ops {name}"]["median"] / k, 1)
        record.setdefault("kernel_over_ctc_forced_align", {})[name] = round(k / record["device_ms"][f"ctc_forced_align {name}"]["median"], 2)
    print(json.dumps(record, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
