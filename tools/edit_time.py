"""Same-process timing of the batched edit distance (scoring.edit_counts; csrc/edit_distance.hip) at the two sizes scoring meets:

* 3840 pairs of about 200 tokens -- E x B x N = 6 x 64 x 10 hypotheses of the benchmarked batch against its 64 references, token ids;
* 384 pairs of about 40 word ids -- the best hypothesis of every exit and utterance after detokenising.

    python tools/edit_time.py [--rounds 7] [--out profiles/edit_distance_time.json]

Legs, measured in turn ``--rounds`` times each after a warm-up of every leg (medians; min .. max is what a difference between two
legs has to be read against): the device call without and with op strings (device events around ``edit_counts``: one launch, two
with ops, and the allocation of its outputs), and the host path (NumPy row sweeps, host seconds) on the same inputs, without and
with ops.  For scale the file also carries the N-best launch that produces such lists (``nbest_launch_384_sequences_ms`` of
profiles/rescore_time.json, read from there, not measured again).  The inputs are random: hypotheses are their references with
about 15 % of the tokens substituted, deleted or inserted.  Device and host results are compared before anything is timed.
Records, not targets: there is no pass mark.  A run without a HIP device fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import scoring  # noqa: E402


def spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def host_s(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(legs, rounds, clock):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(clock(fn))
    return {k: spread(v) for k, v in got.items()}


def corrupted(rng, ref, vocab, rate=0.15):
    """``ref`` with about ``rate`` of its tokens substituted, deleted or followed by an inserted one."""
    u, new = rng.random(len(ref)), rng.integers(0, vocab, len(ref)).tolist()
    out = []
    for t, v, w in zip(ref, u.tolist(), new):
        if v < rate / 3:
            continue
        out.append(w if v < 2 * rate / 3 else t)
        if 2 * rate / 3 <= v < rate:
            out.append(w)
    return out


def make(rng, n_refs, per_ref, mean_len, vocab):
    lens = rng.integers(int(0.75 * mean_len), int(1.25 * mean_len) + 1, n_refs).tolist()
    refs = [rng.integers(0, vocab, n).tolist() for n in lens]
    hyps = [corrupted(rng, refs[r], vocab) for r in range(n_refs) for _ in range(per_ref)]
    ref_of = torch.arange(n_refs, dtype=torch.int32).repeat_interleave(per_ref)
    h, r = scoring.TokenRows.from_lists(hyps), scoring.TokenRows.from_lists(refs)
    return h.rows, h.lens, r.rows, r.lens, ref_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_distance_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_time.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    for name, (n_refs, per_ref, mean_len, vocab) in {"nbest_tokens_3840x200": (64, 60, 200, 256), "best_words_384x40": (64, 6, 40, 5000)}.items():
        host = make(rng, n_refs, per_ref, mean_len, vocab)
        on_dev = [t.to(dev) for t in host]
        want = scoring.edit_counts(*host, want_ops=True)
        got = scoring.edit_counts(*on_dev, want_ops=True)
        assert all(torch.equal(a, b.cpu()) for a, b in zip(want, got)), name
        rec = {"pairs": int(host[0].size(0)), "hyp_pitch": int(host[0].size(1)), "ref_pitch": int(host[2].size(1)),
               "mean_hyp_len": round(float(host[1].float().mean()), 1), "mean_ref_len": round(float(host[3].float().mean()), 1),
               "mean_distance": round(float(want.distance.float().mean()), 2),
               "cell_updates": int((host[1].long() * host[3][host[4].long()].long()).sum())}
        rec.update(measure({"device_counts_ms": lambda: scoring.edit_counts(*on_dev),
                            "device_counts_and_ops_ms": lambda: scoring.edit_counts(*on_dev, want_ops=True)}, args.rounds, device_ms))
        rec.update(measure({"host_counts_s": lambda: scoring.edit_counts(*host),
                            "host_counts_and_ops_s": lambda: scoring.edit_counts(*host, want_ops=True)}, max(3, args.rounds // 2), host_s))
        out[name] = rec
    try:
        with open(os.path.join(ROOT, "profiles", "rescore_time.json")) as f:
            out["nbest_launch_384_sequences_ms_from_rescore_time"] = json.load(f)["nbest_launch_384_sequences_ms"]["median"]
    except (OSError, KeyError):
        out["nbest_launch_384_sequences_ms_from_rescore_time"] = None
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
