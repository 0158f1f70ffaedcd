"""Same-box timing of the nearest-word search (``Lexicon.nearest``, csrc/lexicon.hip) on a synthetic lexicon of the real one's
size: 89 114 words over 27 symbols drawn from a seed with the length histogram of librispeech.lex (the file itself is not part
of this repository).  Queries are lexicon words with one to three random edits, the shape of an early exit's misspellings.

    python tools/lexicon_time.py [--reps 30] [--queries 1,64,1024,4096]              JSON lines
    python tools/lexicon_time.py --profile out/prof_lexicon                           + a rocprofv3 --kernel-trace --stats run

* launch: device time by events around one ``eec_lexicon_nearest`` call on prepared device buffers (the search kernel and the
  reduction of its shares), median of ``--reps`` after a warm-up, and per call in a train of 20 calls, which takes the launch gap out.
* call: host clock around ``Lexicon.nearest`` + the copy of the indices to the host (encoding, one upload, the launch, one
  download), best of five.
* scale: the test-side pure-Python statement (tests/lex_cases.py) on the 2 248-word fixture slice, labelled as such -- the
  reference's C++ ``editdistance`` is not installed here, so there is no fair CPU figure.
* --profile: a fresh child under ``rocprofv3 --kernel-trace --stats`` (a run of its own: tracing slows the host), summarised by
  tools/rocprof_db_summary.py.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from early_exit_transformer_amd import capi  # noqa: E402
from early_exit_transformer_amd.lexicon import Lexicon  # noqa: E402
import lex_cases as L  # noqa: E402  (tests/: the synthetic lexicon's histogram and generator, and the pure-Python statement)

LETTERS = L.LETTERS


def misspelt(words, n, seed=2):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        w = list(rng.choice(words))
        for _ in range(rng.randint(1, 3)):
            at = rng.randrange(len(w) + 1)
            kind = rng.randrange(3)
            if kind == 0 or not w:
                w.insert(at, rng.choice(LETTERS))
            elif kind == 1:
                del w[min(at, len(w) - 1)]
            else:
                w[min(at, len(w) - 1)] = rng.choice(LETTERS)
        out.append("".join(w))
    return out


def event_ms(fn, reps, per=1):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return statistics.median(out), min(out), max(out)


def prepared_call(lex, words, dev):
    """The bare ``eec_lexicon_nearest`` call on buffers that are already on the device."""
    lib = capi.load()
    buf, longest = lex.encode(words)
    Q = len(words)
    query = torch.from_numpy(buf).to(dev)
    packed = lex._packed_on(dev)
    out = torch.empty((2, Q), dtype=torch.int32, device=dev)
    ws_bytes = lib.eec_lexicon_nearest_workspace_bytes(Q, len(lex))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    keep = (query, packed, out, ws)

    def call():
        capi.check(lib.eec_lexicon_nearest(packed.data_ptr(), len(lex), query.data_ptr() + 4 * (Q + 1), query.data_ptr(), Q, longest,
                                           out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), ws_bytes, capi.stream_ptr(dev)),
                   "eec_lexicon_nearest")
        return keep
    return call, out, longest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--queries", default="1,64,1024,4096")
    ap.add_argument("--profile", default=None, help="directory for a rocprofv3 --kernel-trace --stats run of a child")
    ap.add_argument("--kernel-only", action="store_true", help="the launch times alone (variant comparisons, the profiled child)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
                      "library": os.path.basename(capi.LIB_PATH)}), flush=True)
    words = L.synthetic_full_lexicon()
    t0 = time.perf_counter()
    lex = Lexicon(words, device=dev)
    pack_s = time.perf_counter() - t0
    symbols = sum(len(w) for w in words)
    print(json.dumps({"what": "lexicon", "words": len(words), "symbols": symbols, "alphabet": lex.alphabet,
                      "image_bytes": lex._image.numel(), "pack_s": round(pack_s, 3)}), flush=True)
    counts = [int(q) for q in args.queries.split(",")]
    pool = misspelt(words, max(counts))
    launch = {}
    for Q in counts:
        qs = pool[:Q]
        call, out, longest = prepared_call(lex, qs, dev)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        one = event_ms(call, args.reps)
        train = event_ms(call, max(args.reps // 5, 3), per=20)
        launch[Q] = train[0]
        rec = {"what": "launch", "Q": Q, "longest_query": longest,
               "one_call_ms": {"median": round(one[0], 4), "min": round(one[1], 4), "max": round(one[2], 4)},
               "train_of_20_ms_per_call": {"median": round(train[0], 4), "min": round(train[1], 4), "max": round(train[2], 4)},
               "pairs_per_s": float(f"{Q * len(words) / (train[0] * 1e-3):.4g}"),
               "pair_symbols_per_s": float(f"{Q * symbols / (train[0] * 1e-3):.4g}"),
               "mean_distance": round(float(out[1].float().mean()), 3)}
        if not args.kernel_only:
            best = None
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lex.nearest(qs)[0].cpu()
                best = min(best or 1e9, time.perf_counter() - t0)
            rec["nearest_and_copy_back_ms_host_clock"] = round(1e3 * best, 3)
        print(json.dumps(rec), flush=True)
    if len(counts) > 1:
        steps = [(a, b, round(launch[b] / launch[a], 2), round(b / a, 2)) for a, b in zip(counts, counts[1:])]
        print(json.dumps({"what": "growth", "steps": [{"from_Q": a, "to_Q": b, "time_ratio": t, "Q_ratio": q} for a, b, t, q in steps]}), flush=True)
    if args.kernel_only:
        return

    fx = L.load_fixture()  # the test-side statement: for scale only
    known = set(fx["lexicon"])
    missing = [w for s in fx["inputs"] for w in s.split(" ") if w not in known]
    t0 = time.perf_counter()
    for w in missing:
        L.nearest_ref(w, fx["lexicon"])
    d = time.perf_counter() - t0
    pairs = len(missing) * len(fx["lexicon"])
    print(json.dumps({"what": "pure-Python test helper on the fixture slice (for scale; not the reference's C++ editdistance)",
                      "words_looked_up": len(missing), "lexicon_words": len(fx["lexicon"]), "s": round(d, 3),
                      "us_per_pair": round(1e6 * d / pairs, 2)}), flush=True)

    if args.profile:
        os.makedirs(args.profile, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.profile, "--", sys.executable, os.path.abspath(__file__), "--kernel-only",
               "--reps", "10", "--queries", "1024"]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            raise SystemExit(f"rocprofv3 run failed ({res.returncode}):\n{res.stderr[-3000:]}")
        summary = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocprof_db_summary.py"), args.profile, "--top", "8"],
                                 capture_output=True, text=True, timeout=300)
        print(summary.stdout + summary.stderr[-2000:], flush=True)


if __name__ == "__main__":
    main()
