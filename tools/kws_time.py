"""Same-box timing of keyword spotting on CTC emissions (``keyword_search``, csrc/keyword.hip) at the default model's emissions:
E x B = 6 x 64 = 384 emissions of T' = 256 frames over V = 256 tokens, K in {1, 16, 256} keywords of 8 tokens.

    python tools/kws_time.py [--rounds 7] [--out profiles/kws_time.json]

Medians over ``--rounds`` alternating rounds in one process (every variant once per round), device time between events:
* ``keyword_search`` as called (both launches, the output allocations included), with and without the trace;
* each launch alone: the device durations of the two kernels as the profiler of torch reports them for one call (null where that
  profiler is not available);
* the same recurrence written with torch ops on the device, one step per frame over [n_em, K, S] (its bits are compared with the
  kernel's);
* ``ctc_beam_decode`` (beam 10) on the same emissions: what a full decode costs beside spotting;
* the NumPy host path on a slice of 8 emissions and 16 keywords, host clock.
The emissions are log_softmax of scaled noise and the keywords random tokens: timings only, no statement about detection accuracy.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from early_exit_transformer_amd import KeywordSet, keyword_search  # noqa: E402
from early_exit_transformer_amd.model import ctc_beam_decode  # noqa: E402

N_EM, TQ, V, N_TOK, KS = 384, 256, 256, 8, (1, 16, 256)
NEG = float("-inf")


def keywords(K, seed=0):
    g = torch.Generator().manual_seed(seed + K)
    return KeywordSet(torch.randint(1, V, (K, N_TOK), generator=g).tolist(), V)


def torch_ops(logp, kws):
    """The statement of include/eec.h with tensor ops on the device, one step per frame; returns (score, start, end)."""
    dev = logp.device
    n, Tq, _ = logp.shape
    tokens, lengths = kws.to(dev)
    K, S = tokens.size(0), 2 * tokens.size(1) - 1
    lab = torch.full((K, S), kws.blank, dtype=torch.int64, device=dev)
    lab[:, 0::2] = tokens.to(torch.int64)
    s_idx = torch.arange(S, device=dev)[None, :]
    inside = s_idx <= 2 * lengths.to(torch.int64)[:, None] - 2
    lab = torch.where(inside, lab, torch.full_like(lab, kws.blank))
    skip = torch.zeros((K, S), dtype=torch.bool, device=dev)
    skip[:, 2::2] = lab[:, 2::2] != lab[:, :-2:2]
    skip &= inside
    last = (2 * lengths.to(torch.int64) - 2).view(1, K, 1).expand(n, K, 1)
    d = torch.full((n, K, S), NEG, device=dev)
    st = torch.full((n, K, S), -1, dtype=torch.int32, device=dev)
    best = torch.full((n, K), NEG, device=dev)
    b_start = torch.full((n, K), -1, dtype=torch.int32, device=dev)
    b_end = torch.full((n, K), -1, dtype=torch.int32, device=dev)
    neg1, neg2 = torch.full((n, K, 1), NEG, device=dev), torch.full((n, K, 2), NEG, device=dev)
    m1, m2 = torch.full((n, K, 1), -1, dtype=torch.int32, device=dev), torch.full((n, K, 2), -1, dtype=torch.int32, device=dev)
    zero = torch.zeros((), device=dev)
    m_all = logp.amax(dim=2)
    for t in range(Tq):
        m = m_all[:, t].view(n, 1, 1)
        e = torch.where(torch.isfinite(m), logp[:, t, :][:, lab] - m, torch.full_like(m, NEG))
        p1, s1 = torch.cat([neg1, d[:, :, :-1]], 2), torch.cat([m1, st[:, :, :-1]], 2)
        p2, s2 = torch.cat([neg2, d[:, :, :-2]], 2), torch.cat([m2, st[:, :, :-2]], 2)
        take = p1 > d
        c, cs = torch.where(take, p1, d), torch.where(take, s1, st)
        take = skip[None] & (p2 > c)
        c, cs = torch.where(take, p2, c), torch.where(take, s2, cs)
        fresh = zero > c[:, :, 0]
        c[:, :, 0] = torch.where(fresh, zero, c[:, :, 0])
        cs[:, :, 0] = torch.where(fresh, torch.full_like(cs[:, :, 0], t), cs[:, :, 0])
        d = c + e
        st = torch.where(d == NEG, torch.full_like(cs, -1), cs)
        fv, fs = d.gather(2, last)[:, :, 0], st.gather(2, last)[:, :, 0]
        up = fv > best
        best, b_start, b_end = torch.where(up, fv, best), torch.where(up, fs, b_start), torch.where(up, torch.full_like(b_end, t), b_end)
    return best, b_start, b_end


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_times(fn):
    """{kernel name fragment: device microseconds} of the two launches of one call, from torch's profiler; None if it is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for frag in ("kw_frame_max_kernel", "kw_lattice_kernel"):
                if frag in ev.key:
                    total = getattr(ev, "device_time_total", None)
                    total = ev.cuda_time_total if total is None else total
                    out[frag] = round(total / max(ev.count, 1), 2)
        return out or None
    except Exception as exc:  # the profiler is an optional part of a torch build
        print(json.dumps({"profiler": f"unavailable: {type(exc).__name__}: {exc}"}), flush=True)
        return None


def med(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kws_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__, "n_em": N_EM, "Tq": TQ,
              "V": V, "tokens_per_keyword": N_TOK, "rounds": args.rounds, "inputs": "log_softmax(3 * noise), random keywords: timings only"}
    g = torch.Generator().manual_seed(384)
    logp = torch.log_softmax(torch.randn(N_EM, TQ, V, generator=g) * 3.0, -1).to(dev)
    sets = {K: keywords(K) for K in KS}
    variants = {}
    for K, kws in sets.items():
        variants[f"keyword_search K={K}"] = lambda kws=kws: keyword_search(logp, kws)
        variants[f"keyword_search K={K} trace"] = lambda kws=kws: keyword_search(logp, kws, want_trace=True)
        variants[f"torch ops K={K}"] = lambda kws=kws: torch_ops(logp, kws)
    variants["ctc_beam_decode beam=10"] = lambda: ctc_beam_decode(logp, beam_size=10)
    same = {}
    for K, kws in sets.items():  # warm-up, and the baseline's bits against the kernel's
        hits, ref = keyword_search(logp, kws), torch_ops(logp, kws)
        same[K] = bool(torch.equal(hits.score, ref[0]) and torch.equal(hits.start, ref[1]) and torch.equal(hits.end, ref[2]))
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    record["device_ms"] = {name: med(v) for name, v in times.items()}
    record["torch_ops_bits_equal_kernel"] = same
    record["launches_us"] = {f"K={K}": kernel_times(lambda kws=kws: keyword_search(logp, kws)) for K, kws in sets.items()}
    record["launches_us_trace"] = {f"K={K}": kernel_times(lambda kws=kws: keyword_search(logp, kws, want_trace=True)) for K, kws in sets.items()}
    for K in KS:
        k, t = record["device_ms"][f"keyword_search K={K}"]["median"], record["device_ms"][f"torch ops K={K}"]["median"]
        record.setdefault("torch_ops_over_kernel", {})[f"K={K}"] = round(t / k, 1)
    host_x, host_k = logp[:8].cpu(), sets[16]
    keyword_search(host_x, host_k)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        keyword_search(host_x, host_k)
        host.append(1e3 * (time.perf_counter() - t0))
    record["numpy_host_path_ms"] = {"n_em": 8, "K": 16, **med(host)}
    print(json.dumps(record, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
