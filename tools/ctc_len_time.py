"""Same-box, same-process timing of the CTC entries (csrc/ctc.hip, ctc_beam.hip, the greedy decoder of pack.hip) without and with
per-utterance input lengths, at the benchmark's loss shape: log-probs [6, 64, 256, 256]; targets of length 42, 100 and 200 (2, 4 and
8 lattice states per lane); the decoders on the same rows as 384 sequences, the N-best end with nbest 10 of beam 10.

    python tools/ctc_len_time.py [--parent-lib PATH] [--rounds 7] [--reps 50] [--out profiles/ctc_one_set_time.json]

Per entry three legs: NULL lengths, lengths all T', lengths uniform in [T'/2, T'].  ``--parent-lib`` names a second libeec.so (built
from another commit; it must export the same ABI), loaded beside this tree's: every leg is then run through both libraries, and
    * the parent's NULL leg is its entry WITHOUT lengths, this tree's is the ``_len`` entry with NULL;
    * on the same seeded inputs every output of the two is compared bit for bit: nll, the per-exit losses, dlogp on the frames
      t < Tb (and whether the rows past Tb are zeros in both); tokens up to each count, counts, scores, n_hyp;
    * a leg's time mark: this tree's median may exceed the parent's by no more than the parent's own min .. max range of that leg.
The legs of an entry are measured in turn (parent, new, parent, new, ...), ``--rounds`` times each, as device events around a train
of ``--reps`` calls on the current stream.  The forward + backward pair is one forward and one backward call per repetition on the
same workspace.  With a parent the exit status is 1 when a time mark or a comparison with lengths given is missed (the record is
written first).  A run without a HIP device fails.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import capi, synth  # noqa: E402

E, B, T, V = 6, 64, 256, 256
TARGET_LENS = (42, 100, 200)  # P = 2, 4, 8 states per lane
BEAM = 10
ENTRIES = ("eec_ctc_loss", "eec_ctc_loss_len", "eec_ctc_loss_forward", "eec_ctc_loss_forward_len", "eec_ctc_loss_backward",
           "eec_ctc_loss_backward_len", "eec_greedy_ctc", "eec_greedy_ctc_len", "eec_ctc_beam_decode_ex", "eec_ctc_beam_decode_len",
           "eec_ctc_beam_decode_nbest")


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
    return {k: spread(v) for k, v in ms.items()}


def bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a libeec.so built from the commit to compare against")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_one_set_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_len_time.py measures on a HIP device; none found")
    dev = torch.device("cuda")
    new = capi.load()
    libs = {"new": new}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        if parent.eec_abi_version() != new.eec_abi_version():
            raise SystemExit(f"{args.parent_lib}: ABI v{parent.eec_abi_version()}, this tree has v{new.eec_abi_version()}")
        for name in ENTRIES:
            getattr(parent, name).argtypes = getattr(new, name).argtypes
        libs = {"parent": parent, "new": new}
    st = capi.stream_ptr(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.log_softmax(torch.randn(E, B, T, V, generator=g) * 3.0, -1).to(dev)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    ragged = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    lens = {"len_null": None, "len_all_T": full, "len_uniform_half_to_T": ragged}
    nll = torch.empty(E * B, device=dev)
    out = torch.empty(E, device=dev)
    ones = torch.ones(E, device=dev)
    dlogp = torch.empty_like(x)
    xp = x.data_ptr()

    def ptr(t):
        return None if t is None else t.data_ptr()

    def call(rc):
        if rc != 0:
            raise SystemExit(f"a CTC entry returned {rc}: {new.eec_last_error().decode()}")

    # every maker returns (fn, outputs): fn runs the entry of `lib` once; the parent's NULL leg is its entry without lengths
    def loss(lib, which, il, S, tgt, tl, ws_ptr):
        a = (xp, tgt.data_ptr(), tl.data_ptr())
        z = (E, B, T, V, S, 0, nll.data_ptr(), out.data_ptr(), st)
        if which == "parent" and il is None:
            return (lambda: call(lib.eec_ctc_loss(*a, *z))), (nll, out)
        return (lambda: call(lib.eec_ctc_loss_len(*a, ptr(il), *z))), (nll, out)

    def pair(lib, which, il, S, tgt, tl, ws_ptr):
        a = (xp, tgt.data_ptr(), tl.data_ptr())
        f = (E, B, T, V, S, 0, nll.data_ptr(), out.data_ptr(), ws_ptr, st)
        b = (E, B, T, V, S, 0, nll.data_ptr(), ws_ptr, ones.data_ptr(), dlogp.data_ptr(), st)

        def run():
            call(lib.eec_ctc_loss_forward(*a, *f))
            call(lib.eec_ctc_loss_backward(*a, *b))

        def run_len():
            call(lib.eec_ctc_loss_forward_len(*a, ptr(il), *f))
            call(lib.eec_ctc_loss_backward_len(*a, ptr(il), *b))
        return (run if which == "parent" and il is None else run_len), (nll, out, dlogp)

    # the decoders: the same rows as 384 sequences, lengths per sequence (every exit of an utterance shares its length)
    N = E * B
    tokens = torch.empty((N, BEAM, T), dtype=torch.int32, device=dev)
    counts = torch.empty((N, BEAM), dtype=torch.int32, device=dev)
    scores = torch.empty((N, BEAM), device=dev)
    n_hyp = torch.empty((N,), dtype=torch.int32, device=dev)
    bws = torch.empty((new.eec_ctc_beam_workspace_bytes(N, T),), dtype=torch.uint8, device=dev)
    seq_lens = {k: (None if v is None else v.repeat(E)) for k, v in lens.items()}
    o = (tokens.data_ptr(), counts.data_ptr())

    def greedy(lib, which, el):
        if which == "parent" and el is None:
            return (lambda: call(lib.eec_greedy_ctc(xp, N, T, V, 0, *o, st))), (tokens, counts)
        return (lambda: call(lib.eec_greedy_ctc_len(xp, ptr(el), N, T, V, 0, *o, st))), (tokens, counts)

    def beam(lib, which, el):
        if which == "parent" and el is None:
            return (lambda: call(lib.eec_ctc_beam_decode_ex(xp, N, T, V, 0, BEAM, 0.95, 0, bws.data_ptr(), *o, scores.data_ptr(), st))), \
                (tokens, counts, scores)
        return (lambda: call(lib.eec_ctc_beam_decode_len(xp, ptr(el), N, T, V, 0, BEAM, 0.95, 0, bws.data_ptr(), *o, scores.data_ptr(), st))), \
            (tokens, counts, scores)

    def nbest(lib, which, el):
        return (lambda: call(lib.eec_ctc_beam_decode_nbest(xp, ptr(el), N, T, V, 0, BEAM, 0.95, 0, BEAM, bws.data_ptr(), *o, scores.data_ptr(),
                                                           n_hyp.data_ptr(), st))), (tokens, counts, scores, n_hyp)

    def compare(make, extra, leg_lens, rows):
        """Both libraries once on cleared outputs: {output: bit-identical?}.  ``rows`` [n]: the valid frames (loss) per row."""
        got = {}
        for which, lib in libs.items():
            fn, outs = make(lib, which, leg_lens, *extra)
            for t in outs:
                t.zero_()
            fn()
            torch.cuda.synchronize()
            got[which] = [t.clone() for t in outs]
        p, n = got["parent"], got["new"]
        if make in (loss, pair):
            res = {"nll": bits_equal(p[0], n[0]), "loss_per_exit": bits_equal(p[1], n[1])}
            if make is pair:
                valid = (torch.arange(T, device=dev).view(1, T) < rows.view(B, 1)).view(1, B, T, 1).expand(E, B, T, V)
                res["dlogp_on_valid_frames"] = bits_equal(p[2][valid], n[2][valid])
                res["dlogp_past_Tb_zero_in_both"] = bool((p[2][~valid] == 0).all() and (n[2][~valid] == 0).all())
            return res
        width = 1 if make in (greedy, beam) else BEAM  # rows of (tokens, counts, scores) per sequence that the entry writes
        cp, cn = (counts_.view(-1)[: N * width] for counts_ in (p[1], n[1]))
        res = {"counts": bits_equal(cp, cn)}
        live = torch.arange(T, device=dev).view(1, T) < cn.view(-1, 1).clamp(0, T)
        tp, tn = (t.view(-1)[: N * width * T].view(N * width, T) for t in (p[0], n[0]))
        res["tokens_up_to_count"] = bool(res["counts"] and torch.equal(tp[live], tn[live]))
        if make is not greedy:
            res["scores"] = bits_equal(p[2].view(-1)[: N * width], n[2].view(-1)[: N * width])
        if make is nbest:
            res["n_hyp"] = bits_equal(p[3], n[3])
        return res

    info = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__, "rounds": args.rounds,
            "calls_per_train": args.reps, "parent_lib": bool(args.parent_lib),
            "lengths_uniform_half_to_T": {"min": int(ragged.min()), "max": int(ragged.max()), "mean": round(float(ragged.float().mean()), 1)}}
    records = [info]
    missed = []
    jobs = []
    for S in TARGET_LENS:
        tgt, tl = synth.synth_targets(B, S, V, seed=0)
        tgt, tl = tgt.to(dev), tl.to(dev)
        ws, ws_ptr = capi.aligned_ws(new.eec_ctc_backward_workspace_bytes(E, B, T, S), dev)
        jobs.append((f"eec_ctc_loss (S = {S})", loss, (S, tgt, tl, ws_ptr), [E, B, T, V], lens, args.reps, ws))
        jobs.append((f"eec_ctc_loss_forward + eec_ctc_loss_backward (S = {S})", pair, (S, tgt, tl, ws_ptr), [E, B, T, V], lens, args.reps, ws))
    jobs.append(("eec_greedy_ctc", greedy, (), [N, T, V], seq_lens, args.reps, None))
    jobs.append(("eec_ctc_beam_decode_ex (beam 10)", beam, (), [N, T, V], seq_lens, max(1, args.reps // 10), None))
    jobs.append(("eec_ctc_beam_decode_nbest (nbest 10 of beam 10)", nbest, (), [N, T, V], seq_lens, max(1, args.reps // 10), None))
    with torch.cuda.device(dev):
        for what, make, extra, shape, table, reps, _keep in jobs:
            legs = {f"{k}/{which}": make(lib, which, v, *extra)[0] for k, v in table.items() for which, lib in libs.items()}
            rec = {"what": what, "shape": shape, "ms_per_call": measure(legs, args.rounds, reps)}
            if args.parent_lib:
                rec["time_mark"], rec["bit_identical"] = {}, {}
                for k, v in table.items():
                    p, n = rec["ms_per_call"][f"{k}/parent"], rec["ms_per_call"][f"{k}/new"]
                    allowed = round(p["max"] - p["min"], 4)
                    ok = n["median"] - p["median"] <= p["max"] - p["min"]
                    rec["time_mark"][k] = {"new_minus_parent_median_ms": round(n["median"] - p["median"], 4), "parent_range_ms": allowed, "met": ok}
                    rows = full if v is None else v.clamp(0, T)
                    same = compare(make, extra, v, rows[:B])
                    rec["bit_identical"][k] = same
                    if not ok:
                        missed.append(f"{what} {k}: time")
                    if not all(same.values()) and (v is not None or make in (greedy, beam, nbest)):
                        missed.append(f"{what} {k}: results {same}")
            print(json.dumps(rec), flush=True)
            records.append(rec)
    records[0]["missed"] = missed
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    if missed:
        print("MISSED:\n  " + "\n  ".join(missed), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
