"""Same-process timing of contextual biasing (csrc/ctc_beam_ctx.hip, csrc/ctx_graph.hip) on ctc_cases.big_batch_logp's geometry,
[384, 256, 256] log-probs (6 exits x 64 utterances, T' = 256, V = 256), at beam 10.

    python tools/ctxbias_time.py [--rounds 7] [--parent-lib path/to/the/parent/commit's/libeec.so] [--out profiles/ctxbias_time.json]

Legs, measured in turn ``--rounds`` times each after a warm-up of every leg, by device events (medians; min .. max is what a
difference between two legs has to be read against):
* ``ctc_beam_decode`` as it was (eec_ctc_beam_decode_len), and -- with ``--parent-lib`` -- the same entry of a library built from the
  parent commit, loaded beside this one: the device code of that object is unchanged (tools/isa_diff.sh), so no change is expected;
* the biased entry (eec_ctc_beam_decode_ctx) with graphs of 0, 100 and 1000 random 4-token phrases;
* the AED step launch alone (eec_context_bias_step) on [384, 10, 256] rows, under the 1000-phrase graph.
The emissions are random and the phrases are random: the figures say what the mode costs and nothing about any error rate.
Records, not targets: there is no pass mark.  A run without a HIP device fails."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import capi  # noqa: E402
from early_exit_transformer_amd.context import ContextBiasSession, ContextGraph  # noqa: E402
from early_exit_transformer_amd.ctc import ctc_beam_decode  # noqa: E402

N, T, V, BEAM, R = 384, 256, 256, 10, 10


def spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def emissions():
    """ctc_cases.big_batch_logp without the tests' path: logit scales cycling 1 .. 16, about half the frames above the skip threshold."""
    g = torch.Generator().manual_seed(384)
    x = torch.randn(N, T, V, generator=g)
    scale = torch.tensor([1.0, 3.0, 8.0, 16.0])[torch.arange(N) % 4].view(-1, 1, 1)
    x = x * scale
    x[:, :, 0] += (scale * 3.0 + 8.0).view(-1, 1) * (torch.rand(N, T, generator=g) < 0.5)
    return torch.log_softmax(x, -1)


def graph(n_phrases, **kw):
    rng = np.random.RandomState(n_phrases)
    return ContextGraph([tuple(int(t) for t in rng.randint(3, V, size=4)) for _ in range(n_phrases)], 1.5, vocab_size=V, **kw)


def parent_entry(path, logp):
    """eec_ctc_beam_decode_len of another build of the library, on buffers of its own."""
    lib = C.CDLL(path)
    lib.eec_ctc_beam_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_beam_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.eec_ctc_beam_decode_len.argtypes = capi.load().eec_ctc_beam_decode_len.argtypes
    dev = logp.device
    ws = torch.empty(lib.eec_ctc_beam_workspace_bytes(N, T), dtype=torch.uint8, device=dev)
    tokens = torch.empty((N, T), dtype=torch.int32, device=dev)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    scores = torch.empty((N,), dtype=torch.float32, device=dev)

    def run():
        rc = lib.eec_ctc_beam_decode_len(logp.data_ptr(), None, N, T, V, 0, BEAM, 0.95, 0, ws.data_ptr(), tokens.data_ptr(), counts.data_ptr(),
                                         scores.data_ptr(), capi.stream_ptr(dev))
        assert rc == 0, rc
        return tokens, counts, scores
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctxbias_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctxbias_time.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    logp = emissions().to(dev)
    graphs = {n: graph(n) for n in (0, 100, 1000)}
    legs = {"ctc_beam_decode_ms": lambda: ctc_beam_decode(logp, beam_size=BEAM)}
    if args.parent_lib:
        legs["ctc_beam_decode_parent_commit_ms"] = parent_entry(args.parent_lib, logp)
    for n, g in graphs.items():
        legs[f"ctc_beam_decode_context_{n}_phrases_ms"] = lambda g=g: ctc_beam_decode(logp, beam_size=BEAM, context=g)
    aed = graph(1000, eos=1, pad=2)
    local = torch.randn(N, R, V, device=dev)
    last = torch.randint(3, V, (N, R), device=dev)
    parent = torch.randint(0, R, (N, R), device=dev)
    sess = ContextBiasSession(aed, N, R)
    sess.step(local[:, :1].contiguous(), last[:, :1].contiguous(), None)
    sess.step(local, last, parent[:, :R] * 0)
    legs["context_bias_step_384x10x256_ms"] = lambda: sess.step(local, last, parent)

    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            got[k].append(device_ms(fn))
    out = {"device": torch.cuda.get_device_name(0), "shape": [N, T, V], "beam": BEAM, "rounds": args.rounds,
           "states": {str(n): g.states for n, g in graphs.items()}, "image_bytes": {str(n): g.nbytes for n, g in graphs.items()}}
    out.update({k: spread(v) for k, v in got.items()})
    base = out["ctc_beam_decode_ms"]["median"]
    for n in graphs:
        out[f"context_{n}_phrases_over_plain"] = round(out[f"ctc_beam_decode_context_{n}_phrases_ms"]["median"] / base, 4)
    if args.parent_lib:
        out["plain_over_parent_commit"] = round(base / out["ctc_beam_decode_parent_commit_ms"]["median"], 4)
        want, have = legs["ctc_beam_decode_parent_commit_ms"](), ctc_beam_decode(logp, beam_size=BEAM)
        torch.cuda.synchronize()
        out["same_bits_as_parent_commit"] = bool(torch.equal(want[1], have[1]) and torch.equal(want[2].view(torch.int32), have[2].view(torch.int32)))
    else:
        out["ctc_beam_decode_parent_commit_ms"] = None  # not measured in this run
    moved = ctc_beam_decode(logp, beam_size=BEAM, context=graphs[1000])
    out["sequences_with_a_bias_at_1000_phrases"] = int((moved[3] != 0).sum())
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
