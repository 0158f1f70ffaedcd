#!/usr/bin/env python3
"""Headline benchmark: mel-frames/sec of the early-exit Conformer encoder forward (all exits).

Workload (BASELINE.json configs[1], SURVEY.md 8d "config 2"): the default 12-layer model
(d_model 256, 8 heads, FFN 2048, depthwise K 31, 6 exits x 2 layers, vocab 256), batch 64 per GPU of
synthetic log-normal mel [64, 80, 1027] (-> T' = 256), random-init weights from the portable
generator.  One step = one ``Early_conformer.forward`` through the drop-in nn.Module (stem -> 12
layers -> 6 CTC heads -> [6, 64, 256, 256] fp32 log-probs resident in HBM) followed by the fused
per-exit CTC loss (one launch for all 6 x 64 lattices; reference train.py:53-65) and, for N > 1, the
RCCL all-reduce of the 6 per-exit losses -- the only exchange of the batch-sharded path.  The same
work runs at every N (weak scaling).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes its outputs (--dump-outputs) and prints the record; nothing else.

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step computed -- the per-exit losses
(``exit_losses.npy``, [6] fp32) and the log-probs of a fixed, seeded sample of the batch's utterances
(``log_probs.npy``, [6, n, T', 256] fp32; ``log_probs_utterances.npy`` holds the sampled batch indices) -- at most 64 MB
in all.  Inputs and weights come from seeded generators, so runs with the same arguments compare output for output.

N > 1: either started under ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`` (the ranks read
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), or started plainly, in which case this process becomes a
launcher: it starts the N rank processes itself BEFORE touching the GPU (it never initialises HIP), relays rank 0's JSON
line and exits non-zero if any rank fails.

Prints ONE JSON line on rank 0: the headline (metric, value, unit, higher_is_better, dtype, ms_per_step), its configuration
and what follows from its timing alone.  Extra objects, measured under --full only:
  forward_only the encoder forward alone (N=1)
  roofline     dominant kernel (fused row-tile chain: conv tail + feed-forward stages + in_proj): algorithmic flop per launch / mean launch
               duration from HIP events on the launch stream, vs the 2.5 PFLOP/s dense 16-bit MFMA peak
  cpu_baseline the CPU oracle (oracle/conformer_ref.py, a port of the reference path) timed on
               this box's host cores on a bounded sample of the same workload (rank 0, N=1 only)
  modes        the same step in the faster, lower-precision operand modes (not the headline value)
  secondary_shapes  forward-only at SURVEY 8d's secondary shapes: ragged lengths, T=2051 (T'=512)
  also         kernel_time, parity, step_ms, config3, frontend, aed_decode and train_step
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Rank 0 of a multi-rank run: SIGTERM (the launcher's answer to a failed peer) is BLOCKED in every thread from here on -- before
# torch or the backend start any -- and consumed by one dedicated thread (RecordGuard.catch_sigterm), which emits the record as
# far as it got and leaves non-zero.  A Python-level handler would not do: the main thread sits inside a collective (C code)
# when the signal comes.
_TERM = {"guard": None}
if os.environ.get("RANK") == "0" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
    import signal
    signal.pthread_sigmask(signal.SIG_BLOCK, {signal.SIGTERM})

    def _sigterm_thread():
        signal.sigwait({signal.SIGTERM})
        g = _TERM["guard"]
        if g is not None and not g._done.is_set():
            g.fail("terminated by the launcher: a peer rank failed; headline unaffected", 5)
        os._exit(143)  # no record to save yet (or the run was over): die as SIGTERM would have had it
    threading.Thread(target=_sigterm_thread, daemon=True).start()

import torch  # noqa: E402

MFMA_PEAK_FLOPS = 2.5e15  # MI355X dense bf16/fp16 MFMA peak (MI355X_MICROARCH.md)

CFG = dict(src_pad_idx=0, n_enc_exits=6, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000,
           d_feed_forward=2048, n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31)


def flops_per_forward(B, T, D=256, L=2):
    F, K, E, V, NM = 2048, 31, 6, 256, 80
    T1 = (T - 3) // 2 + 1
    Tq = (T1 - 3) // 2 + 1
    mac_frame = E * L * (4 * D * F + 7 * D * D + K * D + 2 * Tq * D) + E * D * V + 3 * D * D + 3 * NM * D * T1 / Tq
    return 2.0 * mac_frame * B * Tq, Tq


def launch_ranks(n, argv):
    """Parent side of ``python bench.py --gpus N`` outside torch.distributed.run: start N copies of this script as child
    processes, one rank per GPU, with the rendezvous environment torchrun would set.  The parent makes no GPU call (a
    process that has initialised HIP must not be replaced or forked into ranks).  Rank 0's stdout (the ONE JSON line) is
    relayed; the exit status is non-zero if any rank failed (the others are then terminated)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", str(port)),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    rc, live = 0, set(range(n))
    while live:  # poll every rank: a rank that dies must not leave the others waiting in a collective for ever
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0:
                print(f"bench.py: rank {r} exited with status {code}", file=sys.stderr)
                rc = rc or (code if code > 0 else 1)
                for o in live:
                    procs[o].terminate()  # exactly the children started above
        time.sleep(0.05)
    reader.join(timeout=10)
    out0 = b"".join(chunks).decode()
    sys.stdout.write(out0)
    sys.stdout.flush()
    return rc


# The ONE JSON line goes to the process's original stdout; everything else that writes to file descriptor 1 -- RCCL's version
# banner, gloo's connection notes, library chatter -- is sent to stderr (main() re-points fd 1 before any backend is initialised).
_RECORD_OUT = sys.stdout


def _isolate_stdout():
    global _RECORD_OUT
    sys.stdout.flush()
    keep = os.dup(1)
    os.dup2(2, 1)
    _RECORD_OUT = os.fdopen(keep, "w")


class RecordGuard:
    """Exactly ONE record per run, whatever happens in the last (training-step) section: the main thread emits it when the
    section is done; a rank that fails inside a step, or whose section does not finish in time (a hung collective), emits the
    record as far as it got -- rank 0 only -- and ends the process with a NON-ZERO status without entering another collective
    (its peers may be stuck in one; the launcher terminates them when it sees the status).  No re-exec, no retry in a
    GPU-initialised process."""

    def __init__(self, rank, line):
        self.rank, self.line = rank, line
        self._lock, self._emitted, self._done = threading.Lock(), False, threading.Event()

    def emit(self, train_obj=None):
        with self._lock:  # whichever of the main thread and the watchdog gets here first
            if self._emitted:
                return
            self._emitted = True
            if self.rank == 0 and self.line is not None:
                if train_obj is not None:  # None: the section did not run (plain run, --no-train)
                    self.line["train_step"] = train_obj
                _RECORD_OUT.write(json.dumps(self.line) + "\n")
                _RECORD_OUT.flush()

    def fail(self, msg, code):
        self.emit({"error": msg})
        _RECORD_OUT.flush()
        sys.stderr.write(f"bench.py: rank {self.rank}: {msg}\n")
        sys.stderr.flush()
        os._exit(code)

    def start_watchdog(self, timeout_s):
        def run():
            if not self._done.wait(timeout_s):
                self.fail("the training-step section did not finish in time (a rank or a collective hung); headline unaffected", 3)
        threading.Thread(target=run, daemon=True).start()

    def catch_sigterm(self):
        """Rank 0 only, SIGTERM blocked at start-up (module top): a peer failed and the launcher is tearing the job down while
        this rank may be blocked in a collective.  The record is complete but for the section under way: emit it, leave non-zero."""
        _TERM["guard"] = self

    def finish(self):
        self._done.set()


def plumbing_check(args, rank, world):
    """EEC_BENCH_PLUMBING=1 (host tests, no GPU): the N > 1 control flow only -- rendezvous, barrier, the loss all-reduce
    through parallel.combine_exit_losses, max-over-ranks timing, rank 0's one JSON line and, under --full, the guarded last
    section -- over gloo on CPU tensors."""
    import torch.distributed as dist
    from early_exit_transformer_amd import parallel
    if os.environ.get("EEC_BENCH_FAIL_RANK") == str(rank):
        return 7  # failure propagation test
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    local = torch.arange(6, dtype=torch.float32) + rank  # per-exit "losses" of this rank's shard
    t0 = time.perf_counter()
    for _ in range(args.steps):
        combined = parallel.combine_exit_losses(local, args.batch + rank)
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    line = {"plumbing": True, "n_gpus": world, "steps": args.steps, "combined": combined.tolist(),
            "max_rank_seconds": float(dt.item())} if rank == 0 else None
    # the guarded last section, as in the real run (--full only): EEC_BENCH_FAIL_STEP_RANK makes that rank fail INSIDE a step,
    # i.e. before the step's collectives, which its peers then wait in for ever -- until the launcher has seen the non-zero status
    guard = RecordGuard(rank, line)
    guard.catch_sigterm()
    if args.full:
        guard.start_watchdog(float(os.environ.get("EEC_BENCH_TRAIN_TIMEOUT", "240")))
        try:
            if os.environ.get("EEC_BENCH_FAIL_STEP_RANK") == str(rank):
                raise RuntimeError("injected failure inside a training step")
            if world > 1 and os.environ.get("EEC_BENCH_FAIL_STEP_RANK") is not None:
                dist.all_reduce(torch.zeros(1))  # the collective of a step the failed rank never reaches
        except Exception as e:
            if world > 1:
                guard.fail(f"{type(e).__name__}: {e}", 4)
            raise
    guard.finish()
    guard.emit("ok" if args.full else None)
    if world > 1:
        dist.destroy_process_group()
    return 0


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(out_dir, logp, losses):
    """--dump-outputs: the arrays a caller of the timed step receives, as float32 .npy files -- the per-exit losses [E] whole and
    the log-probs [E, B, T', V] of a fixed sample of utterances (seeded, independent of the run; their batch indices as float64)
    that keeps the total under DUMP_LIMIT_BYTES."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    E, Bo, Tq, V = logp.shape
    per_utt = E * Tq * V * 4
    n = max(1, min(Bo, (DUMP_LIMIT_BYTES - (1 << 20)) // per_utt))  # 1 MiB left for the losses, indices and .npy headers
    pick = torch.randperm(Bo, generator=torch.Generator().manual_seed(0))[:n].sort().values
    assert n * per_utt + (1 << 20) <= DUMP_LIMIT_BYTES, "one utterance's log-probs exceed the dump limit"
    arrays = {"exit_losses": losses.float(), "log_probs": logp[:, pick.to(logp.device)].float(),
              "log_probs_utterances": pick.double()}
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), t.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64, help="utterances per GPU")
    ap.add_argument("--frames", type=int, default=1027, help="mel frames per utterance")
    # default = the mode whose log-probs stay within the north-star 1e-3 (flat) on every committed fixture, trained-like (peaky)
    # outputs included; "f16f8" (fp8 correction products) is the faster opt-in that keeps 1e-3 on near-uniform outputs only
    ap.add_argument("--precision", default="f16x3", choices=["f16f8", "f16x3", "mixed", "f16"])
    ap.add_argument("--full", action="store_true",
                    help="also measure every secondary figure (roofline, parity, other modes and shapes, CPU baseline, training step)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-modes", action="store_true", help="with --full: skip the other modes, shapes and geometries and the training step")
    ap.add_argument("--no-train", action="store_true", help="with --full: skip the training-step secondary lines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (rank 0; at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))  # launcher mode: no GPU call in this process
    _isolate_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start {args.gpus} ranks (or none: bench.py launches them)")
    if os.environ.get("EEC_BENCH_PLUMBING") == "1":
        raise SystemExit(plumbing_check(args, rank, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback; the CPU oracle is only the baseline leg)")
    # rehearsal knobs (a one-GPU box cannot host two RCCL ranks): EEC_BENCH_BACKEND=gloo EEC_BENCH_DEVICE=0 runs the N > 1
    # control flow -- barriers, the loss all-reduce, the max-over-ranks timing -- with every rank on the same device
    backend = os.environ.get("EEC_BENCH_BACKEND", "nccl")
    dev_index = int(os.environ.get("EEC_BENCH_DEVICE", local_rank))
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    # EEC_BENCH_SINGLE_RANK=1 (N = 1 only): a process group of ONE rank on the real backend, every collective of the path issued
    # through it (parallel.SINGLE_RANK_COLLECTIVES) -- what RCCL's call path costs a step on a box that has a single GPU
    single_rank = world == 1 and os.environ.get("EEC_BENCH_SINGLE_RANK") == "1"
    if world > 1 or single_rank:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if single_rank:
            os.environ.setdefault("MASTER_PORT", "29577")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from early_exit_transformer_amd import parallel, synth
    from early_exit_transformer_amd.model import Early_conformer, exit_ctc_losses
    if single_rank:
        parallel.SINGLE_RANK_COLLECTIVES = True

    # what the BACKEND saw (not what the environment said): its name and world size, an all-reduce of ones (= the number of
    # ranks that really took part in a collective) and every rank's device identity, gathered to rank 0 for the record
    dist_info = None
    if dist is not None:
        ones = torch.ones(1, dtype=torch.float32, device=dev)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        props = torch.cuda.get_device_properties(dev)
        ident = {"rank": rank, "local_rank": local_rank, "device_index": dev_index, "name": props.name,
                 "pci_bus_id": "{:04x}:{:02x}:{:02x}".format(int(getattr(props, "pci_domain_id", 0)), int(getattr(props, "pci_bus_id", -1)) & 0xff,
                                                             int(getattr(props, "pci_device_id", 0)) & 0xff),
                 "uuid": str(getattr(props, "uuid", "")), "cus": int(props.multi_processor_count), "pid": os.getpid()}
        idents = [None] * dist.get_world_size()
        dist.all_gather_object(idents, ident)
        dist_info = {"backend": str(dist.get_backend()), "world_size": int(dist.get_world_size()), "env_world_size": world,
                     "collective_ranks": int(round(float(ones.item()))), "devices": idents,
                     "distinct_devices": len({(d["pci_bus_id"], d["uuid"]) for d in idents})}

    B, T = args.batch, args.frames
    model = Early_conformer(device=dev, **CFG).eval()
    sd = synth.synth_state_dict(model.state_dict(), seed=0, style="init")
    model.load_state_dict(sd)
    model = model.to(dev)
    model.precision = args.precision
    mel = synth.synth_mel(B, CFG["features_length"], T, seed=rank).to(dev)
    lengths = torch.full((B,), T, dtype=torch.int64)  # padded positions count as work; full-length batch
    tgt, tgt_len = synth.synth_targets(B, 42, CFG["dec_voc_size"], seed=rank)  # 40 BPE ids + BOS/EOS
    tgt, tgt_len = tgt.to(dev), tgt_len.to(dev)

    def sync_all():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def run_steps(n, with_loss=True):
        out, loss = None, None
        for _ in range(n):
            with torch.no_grad():
                out = model(mel, lengths)
                if with_loss:
                    # summed per-exit CTC loss of this rank's shard, then the one collective of the
                    # path: global-batch mean of the 6 per-exit losses (7 floats over RCCL/xGMI)
                    loss = parallel.combine_exit_losses(exit_ctc_losses(out, tgt, tgt_len), B)
        return out, loss

    run_steps(args.warmup)
    sync_all()
    t0 = time.perf_counter()
    last_out, last_loss = run_steps(args.steps)
    sync_all()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_out, last_loss)
    del last_out, last_loss
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    ms_per_step = dt / args.steps * 1e3
    value = world * B * T * args.steps / dt
    flop_fwd, Tq = flops_per_forward(B, T)

    # A plain run ends here: the record below carries the headline and what follows from its timing alone.  Every other figure
    # -- per-kernel times and the roofline, parity against the fixtures, other modes, shapes and geometries, the CPU baseline,
    # the training step -- takes runs of its own and is measured under --full only.
    full0 = args.full and rank == 0
    solo = full0 and world == 1

    # ---- roofline of the dominant kernel (the fused chain), HIP events on the launch stream ----
    roofline, kernel_ms = None, None
    if full0:
        model.set_profiling(True)
        run_steps(max(3, min(args.steps, 10)), with_loss=False)  # forward only: no collective outside the timed region
        torch.cuda.synchronize()
        prof = model.read_profile()
        model.set_profiling(False)
        # dominant kernel = the chain kernel: [depthwise + pointwise-2 ->] FFN stage(s) [-> in_proj] of one row tile
        # (csrc/ffn.hip).  Algorithmic flop of everything the chain launches of ONE forward execute, divided by
        # the launches of one forward (E*L + 1), against the mean launch duration measured with HIP events.
        ch_ms, ch_n = prof["chain"]
        if ch_n == 0:
            raise SystemExit("bench.py: the library did not run the fused production plan (no chain-kernel launches)")
        M = B * Tq
        D, F, K = CFG["d_model"], CFG["d_feed_forward"], CFG["depthwise_kernel_size"]
        n_layers = CFG["n_enc_exits"] * CFG["n_enc_layers"]
        chain_flop_fwd = 2.0 * M * n_layers * (4 * D * F + 3 * D * D + D * D + K * D)
        chain_flop = chain_flop_fwd / (n_layers + 1)
        achieved = chain_flop / (ch_ms / ch_n * 1e-3) / 1e12
        passes = {"f16x3": 3.0, "f16f8": 2.0, "mixed": 1.4, "f16": 1.0}[args.precision]  # executed MFMA work per algorithmic flop (fp16-rate equivalents)
        roofline = {"bound": "mfma", "kernel": "ffn_chain_kernel", "achieved": round(achieved, 2),
                    "peak": MFMA_PEAK_FLOPS / 1e12, "unit": "TFLOP/s", "frac": round(achieved * 1e12 / MFMA_PEAK_FLOPS, 4),
                    "traffic": None, "avg_launch_us": round(ch_ms / ch_n * 1e3, 2), "launches": ch_n,
                    "flop_per_launch": chain_flop,
                    "executed_mfma_tflops": round(achieved * passes, 1),
                    "executed_note": f"this operand mode executes {passes:g} fp16-rate MFMA pass-equivalents per algorithmic flop (the hi / lo split "
                                     "that keeps the 1e-3 tolerance); on random data this chip sustains 1.6-1.7 PFLOP/s of 32x32x16 and 1.9-1.95 of "
                                     "16x16x32 fp16 MFMA in bare register-operand loops and lowers its clock as the MFMA density rises "
                                     "(profiles/r04_micro_mfma_shape_clock.txt, r04_micro_ffn_pair.txt)",
                    "note": "mean over the chain launches of a forward: 1 x [ffn1 -> in_proj], (E*L-1) x [dw+pw2 -> ffn2 -> "
                            "ffn1 -> in_proj], 1 x [dw+pw2 -> ffn2]"}
        tot = sum(v[0] for v in prof.values())
        kernel_ms = {k: {"share": round(v[0] / tot, 4), "avg_us": round(v[0] / max(v[1], 1) * 1e3, 2), "n": v[1]}
                     for k, v in prof.items()}

    forward_only = None
    if solo:
        run_steps(3, with_loss=False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_steps(args.steps, with_loss=False)
        torch.cuda.synchronize()
        d = time.perf_counter() - t1
        forward_only = {"value": round(B * T * args.steps / d, 1), "ms_per_step": round(d / args.steps * 1e3, 4)}

    # ---- parity against the committed golden fixtures (tests/golden/*.npz: produced by the reference's own class body in the
    # build container, make_golden.py), measured in this run for the mode that is timed: the default 12-layer model on
    # B = 4, T = 1027 with random-init heads (near-uniform outputs) and with heads x8 (peaky, trained-like outputs) ----
    parity = None
    if solo:
        import numpy as np
        parity = {"policy": "the default mode f16x3 is held to the north-star tolerance FLAT (|dlogp| <= 1e-3 on every fixture, the peaky "
                            "trained-like one included: within_flat_tol).  The opt-in faster modes state a weaker bound, tol * max(1, "
                            "max|logp| / 8) (within_policy): their operand rounding is a relative error of the logits "
                            "(tests/test_gpu_parity.py::logp_tolerance)",
                  "tol": {"f16f8": 1e-3, "f16x3": 1e-3, "mixed": 2.5e-3, "f16": 6e-3}[args.precision], "fixtures": {}}
        for name in ("config1", "config1_peaky"):
            z = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
            pm = Early_conformer(device=dev, **CFG).eval()
            pm.load_state_dict(synth.synth_state_dict(pm.state_dict(), seed=int(z["seed"]), style=str(z["style"]),
                                                      head_scale=float(z["head_scale"])))
            pm = pm.to(dev)
            pm.precision = args.precision
            with torch.no_grad():
                got = pm(synth.synth_mel(int(z["B"]), 80, int(z["T"]), seed=int(z["seed"])).to(dev), torch.from_numpy(z["lengths"]))
            err = np.abs(got[:, :, ::int(z["stride"])].cpu().numpy() - z["logp"])
            top = z["logp"] >= -10.0  # the entries a decoder reads
            parity["fixtures"][name] = {"max_abs_logp": round(float(np.abs(z["logp"]).max()), 2), "max_err": float(f"{err.max():.3e}"),
                                        "max_err_where_logp_ge_minus10": float(f"{err[top].max():.3e}"),
                                        "within_flat_tol": bool(err.max() < parity["tol"]),
                                        "within_policy": bool(err.max() < parity["tol"] * max(1.0, float(np.abs(z["logp"]).max()) / 8.0))}
            del pm
        parity["reference_fp32_noise"] = ("the reference's own fp32 forward differs from an fp64 evaluation of itself by 3.5e-6 "
                                          "(config1) / 3.9e-5 (config1_peaky) max |dlogp| on the CPU: the same 11x growth with the logit scale")

    # ---- training step (secondary lines; BASELINE.json configs[3] on every rank, configs[2] geometry at N = 1) ----
    # one step = train.py:53-70: forward in train mode (dropout 0.1, batch-statistics BatchNorm), summed per-exit CTC loss,
    # backward (HIP training kernels), gradient all-reduce over the ranks (bucketed RCCL, N > 1), clip_grad_norm_, AdamW.
    def train_bench(cfg, passes, n_steps, label):
        tm = Early_conformer(device=dev, **cfg)
        tm.load_state_dict(synth.synth_state_dict(tm.state_dict(), seed=2, style="init"))
        tm = tm.to(dev).train()
        tm.train_passes = passes
        params = list(tm.parameters())
        opt = torch.optim.AdamW(params, lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.1, fused=True)  # one multi-tensor kernel (torch's own)
        torch.manual_seed(rank)

        # gradients live in flat per-exit-group buckets; with N > 1 each bucket's RCCL all-reduce starts as the backward
        # finishes that exit group (eec_train_backward_ex) and runs under the backward of the earlier groups
        tm.enable_data_parallel(B)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = exit_ctc_losses(tm(mel, lengths), tgt, tgt_len).sum()
            loss.backward()
            tm.sync_gradients()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
            return loss

        err = ""
        d = float("nan")
        try:
            for _ in range(2):
                loss = step()
            sync_all()
            t1 = time.perf_counter()
            for _ in range(n_steps):
                loss = step()
            torch.cuda.synchronize()
            d = (time.perf_counter() - t1) / n_steps
            if not torch.isfinite(loss).item():
                err = "non-finite loss"
        except Exception as e:
            err = f"{type(e).__name__}: {e}"[:300]
            if dist is not None:
                # a rank that failed inside a step has skipped collectives its peers are waiting in: nothing sensible can be
                # exchanged any more.  Emit the record (rank 0), then leave with a non-zero status -- the launcher (or torchrun)
                # tears the other ranks down and the job is recorded as failed, never as rc 0.
                fail_section(f"{label}: {err}", 4)
        if dist is not None:
            t = torch.tensor([d if not err else float("inf")], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            d = float(t.item())
        del tm, opt, params
        torch.cuda.empty_cache()
        if rank != 0:
            return None
        f_fwd, _ = flops_per_forward(B, T, D=cfg["d_model"], L=cfg["n_enc_layers"])
        ok = not err and d == d and d != float("inf")
        return {"workload": label, "value": round(world * B * T / d, 1) if ok else None, "unit": "mel-frames/s",
                "ms_per_step": round(d * 1e3, 3) if ok else None, "n_gpus": world, "steps": n_steps,
                "operands": "bf16x3 (hi/lo split, 3 MFMA products, ~fp32 results)" if passes == 3 else "bf16",
                "algorithmic_flop_per_step": 3 * f_fwd,
                "frac_of_mfma_peak": round(3 * f_fwd / d / MFMA_PEAK_FLOPS, 4) if ok else None, "error": err or None}

    # ---- BASELINE.json configs[2] geometry (secondary line): 6 exits x 3 layers, d_model 512, forward + fused exit losses ----
    config3 = None
    if solo and not args.no_modes:
        cfg3 = dict(CFG, d_model=512, n_enc_layers=3)
        m3 = Early_conformer(device=dev, **cfg3).eval()
        m3.load_state_dict(synth.synth_state_dict(m3.state_dict(), seed=1, style="init"))
        m3 = m3.to(dev)
        m3.precision = args.precision

        def run3(n):
            for _ in range(n):
                with torch.no_grad():
                    exit_ctc_losses(m3(mel, lengths), tgt, tgt_len)
        run3(3)
        torch.cuda.synchronize()
        n3 = max(5, args.steps // 2)
        t1 = time.perf_counter()
        run3(n3)
        torch.cuda.synchronize()
        d = (time.perf_counter() - t1) / n3
        f3, _ = flops_per_forward(B, T, D=512, L=3)
        config3 = {"workload": f"early_conformer ctc 18-layer d_model=512 (6 exits x 3, 8 heads x 64), batch {B}, mel [80 x {T}], "
                               "forward + fused per-exit CTC losses (BASELINE.json configs[2] geometry, inference path; the training step of this geometry is train_step.config3_bf16)",
                   "value": round(B * T / d, 1), "unit": "mel-frames/s", "ms_per_step": round(d * 1e3, 4),
                   "algorithmic_flop_per_forward": f3, "frac_of_mfma_peak": round(f3 / d / MFMA_PEAK_FLOPS, 4),
                   "precision_mode": args.precision}
        del m3
        torch.cuda.empty_cache()

    # ---- AED inference (BASELINE.json configs[4] substitute; secondary line): evaluate_batch_ae of inference.py:18-62 for one
    # synthetic utterance -- ONE HIP encoder run for all exits, then beam search (beam 10) per exit with the HIP decoder ----
    aed = None
    if solo and not args.no_modes:
        try:
            from early_exit_transformer_amd.beam import BeamInference
            from early_exit_transformer_amd.model import full_conformer
            fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device=dev, **{k: v for k, v in CFG.items() if k != "src_pad_idx"}).eval()
            fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
            fc = fc.to(dev)
            spec, vlen = mel[0], torch.tensor(T)
            inf = BeamInference()
            kw5 = dict(vocab_size=CFG["dec_voc_size"], SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=1.0)
            def timed(**more):
                inf.decode_all_exits(fc, spec, vlen, beam_size=10, **kw5, **more)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                hyps = inf.decode_all_exits(fc, spec, vlen, beam_size=10, **kw5, **more)
                torch.cuda.synchronize()
                return time.perf_counter() - t1, hyps
            d, hyps = timed()
            d_full, hyps_full = timed(kv_cache=False)  # the reference's way: the decoder re-run on the whole prefix at every step
            steps5 = int(T / 12)
            aed = {"workload": f"full_conformer (6 x 2 encoder, 6 decoder layers per exit), 1 utterance of {T} mel frames: encoder once, "
                               f"beam search (beam 10, {steps5} steps) for each of the 6 exits, step-wise decoder over a key / value cache, the 6 "
                               "searches in lockstep through the same launches (eec_decoder_begin / eec_decoder_step_multi)",
                   "seconds_per_utterance": round(d, 4), "decoder_steps": 6 * steps5, "ms_per_decoder_step": round(d / (6 * steps5) * 1e3, 3),
                   "tokens_out": [len(h) for h in hyps],
                   "whole_prefix_decoder": {"what": "same search, eec_decoder_forward on the whole prefix per step (no cache)",
                                            "seconds_per_utterance": round(d_full, 4),
                                            "ms_per_decoder_step": round(d_full / (6 * steps5) * 1e3, 3),
                                            "same_best_beams": hyps == hyps_full}}
            del fc
            torch.cuda.empty_cache()
        except Exception as e:  # a secondary line never takes the headline down
            aed = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- mel front end: waveform -> [B, 80, T] power mel for the same batch (secondary line) ----
    frontend = None
    if solo and not args.no_modes:
        from early_exit_transformer_amd.frontend import MelFrontend
        fe = MelFrontend()
        n_samples = (T - 1) * 160  # the waveform length whose front end yields T mel frames
        wave = torch.randn(B, n_samples, device=dev) * 0.1
        for _ in range(3):
            fe(wave)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n_fe = max(5, args.steps // 2)
        for _ in range(n_fe):
            fe(wave)
        torch.cuda.synchronize()
        d = (time.perf_counter() - t1) / n_fe
        frontend = {"workload": f"{B} x {n_samples} samples (16 kHz) -> mel [{B}, 80, {T}]: 1024-point power spectrum (exact-fp32 MFMA DFT) + 80 mel filters",
                    "ms": round(d * 1e3, 4), "mel_frames_per_s": round(B * T / d, 1),
                    "audio_seconds_per_second": round(B * n_samples / 16000.0 / d, 1),
                    "fp32_flop": 2.0 * B * T * (320 * 1024 + 1026), "frac_of_fp32_mfma_peak": round(2.0 * B * T * (320 * 1024 + 1026) / d / 157.3e12, 4)}
        del wave

    # HBM-side bytes per FFN launch from the committed PMC passes of this round (rocprofv3 --pmc FETCH_SIZE /
    # WRITE_SIZE in separate passes, tools/pmc_passes.sh; FETCH_SIZE doubled: on gfx950 it reports half of a wide
    # coalesced read, MI355X_MICROARCH.md).  Static evidence, not re-measured here: PMC needs rocprofv3.
    PMC_EVIDENCE = {"f16f8": ("r03_c_pmc_chain_kernel_f16f8.txt", "ffn_chain_kernel<256, 8, 0, 8, 8, 2>"),
                    "f16x3": ("r04_d_pmc_chain_kernel_f16x3.txt", "ffn_chain_kernel<256, 3, 0, 3, 3, 2, 0>")}
    if roofline is not None and args.precision in PMC_EVIDENCE:
        pmc_file, pmc_kernel = PMC_EVIDENCE[args.precision]
        pmc = os.path.join(ROOT, "profiles", pmc_file)
        if os.path.exists(pmc):
            fetch, write = [], []
            for ln in open(pmc):
                if pmc_kernel in ln and "FETCH_SIZE" in ln:
                    fetch.append(float(ln.split("avg/dispatch")[1].split()[0]))
                if pmc_kernel in ln and "WRITE_SIZE" in ln:
                    write.append(float(ln.split("avg/dispatch")[1].split()[0]))
            if fetch and write:
                roofline["traffic"] = round((2.0 * sum(fetch) / len(fetch) + sum(write) / len(write)) * 1024.0)
                roofline["traffic_source"] = (f"STATIC evidence, not measured in this run: profiles/{pmc_file} "
                                              "(rocprofv3 --pmc passes of this build; 2*FETCH_SIZE + WRITE_SIZE, KiB -> B; the "
                                              "two-stage variant = 11 of the 13 launches)")

    # ---- the other operand modes (reported, never the headline) ----
    modes = {}
    if solo and not args.no_modes:
        for prec in ("f16f8", "f16x3", "mixed", "f16"):
            if prec == args.precision:
                continue
            model.precision = prec
            run_steps(3)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            run_steps(args.steps)
            torch.cuda.synchronize()
            d = time.perf_counter() - t1
            modes[prec] = {"value": round(B * T * args.steps / d, 1), "ms_per_step": round(d / args.steps * 1e3, 4),
                           "frac_of_mfma_peak": round(flop_fwd * args.steps / d / MFMA_PEAK_FLOPS, 4)}
        model.precision = args.precision

    # ---- per-step distribution (median, p10 / p90): HIP events between consecutive steps of a second pass ----
    step_ms = None
    if solo:
        n_ev = min(args.steps, 50)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_ev + 1)]
        run_steps(2)
        evs[0].record()
        for i in range(n_ev):
            run_steps(1)
            evs[i + 1].record()
        torch.cuda.synchronize()
        ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(n_ev))
        step_ms = {"median": round(ts[n_ev // 2], 4), "p10": round(ts[n_ev // 10], 4), "p90": round(ts[(9 * n_ev) // 10], 4),
                   "n": n_ev, "how": "hipEvent pairs around single steps on the launch stream"}

    # ---- secondary shapes: forward-only, same model; reported, never the headline ----
    secondary = {}
    if solo and not args.no_modes:
        def timed_forward(mel_s, len_s, n):
            with torch.no_grad():
                for _ in range(3):
                    model(mel_s, len_s)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(n):
                    model(mel_s, len_s)
                torch.cuda.synchronize()
            return (time.perf_counter() - t1) / n
        n_sec = max(5, args.steps // 2)
        g = torch.Generator().manual_seed(1)
        ragged = torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int64)
        ragged[0] = T  # the reference needs max(lengths) == T
        d = timed_forward(mel, ragged, n_sec)
        secondary["ragged_lengths"] = {"shape": f"B={B}, T={T}, lengths uniform in [T/2, T] (one == T)",
                                       "value": round(B * T / d, 1), "ms_per_step": round(d * 1e3, 4),
                                       "note": "padded frames are computed like the reference computes them; only keys are masked"}
        B2, T2 = max(B // 2, 1), 2 * T - 3  # T' doubles, B halves: the same number of encoder frames
        mel2 = synth.synth_mel(B2, CFG["features_length"], T2, seed=7).to(dev)
        d = timed_forward(mel2, torch.full((B2,), T2, dtype=torch.int64), n_sec)
        secondary["long_utterances"] = {"shape": f"B={B2}, T={T2} -> T'={(((T2 - 3) // 2 + 1) - 3) // 2 + 1}",
                                        "value": round(B2 * T2 / d, 1), "ms_per_step": round(d * 1e3, 4)}
        del mel2

    # ---- CPU baseline: the oracle on the host cores, the FULL batch of this workload ----
    cpu = None
    if solo and not args.no_cpu_baseline:
        from oracle import conformer_ref as R
        ref = R.EarlyConformerRef(device="cpu", **CFG).eval()
        ref.load_state_dict(sd)
        cmel, clen = mel.cpu(), lengths

        def cpu_run(threads, budget_s):
            torch.set_num_threads(threads)
            times = []
            with torch.no_grad():
                ref(cmel[:8], clen[:8])  # warm-up (thread pool, oneDNN primitives)
                t_all = time.perf_counter()
                while len(times) < 5 and (len(times) < 2 or time.perf_counter() - t_all < budget_s):
                    t1 = time.perf_counter()
                    ref(cmel, clen)
                    times.append(time.perf_counter() - t1)
            times.sort()
            return B * T / times[len(times) // 2], len(times)
        # the box advertises every host core but grants this job a share of them (16 for a one-GPU box): more threads
        # than the share only thrash.  Two settings, as BASELINE.md section 3 asks: the whole share, and the reference's
        # own default --n_threads 10 (util/conf.py:150-158).
        share = min(len(os.sched_getaffinity(0)), 16)
        v_share, n_share = cpu_run(share, 12.0)
        v_10, n_10 = cpu_run(min(10, share), 12.0)
        cpu = {"value": round(v_share, 1), "unit": "mel-frames/s", "cores": share, "kind": "port",
               "sample": f"median of {n_share} forwards of the full batch {B} x {T} mel frames after a warm-up (same model and "
                         "inputs, fp32, eval, no_grad); host reports " f"{os.cpu_count()} logical cores",
               "n_threads_10": {"value": round(v_10, 1), "cores": min(10, share), "forwards": n_10,
                                "note": "the reference's default --n_threads (util/conf.py:150-158)"}}

    if rank == 0:
        line = {
            "metric": "mel-frames/sec encoder forward (all exits) + summed per-exit CTC loss, d_model=256 12-layer",
            "value": round(value, 1), "unit": "mel-frames/s",
            "n_gpus": dist_info["world_size"] if dist_info is not None and not single_rank else world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": {"f16f8": "fp16 + 2x fp8-correction MFMA (feed-forward, projections), fp16x3 exit heads and stem, fp32 accumulate",
                                                             "f16x3": "fp16x3 (hi/lo-split fp16 MFMA operands, three products per GEMM, fp32 accumulate; v_mfma_f32_16x16x32_f16)",
                                                             "mixed": "fp16 FFN + fp16x3 projections", "f16": "fp16"}[args.precision],
            "data": "synthetic",
            "config": {"workload": f"early_conformer ctc 12-layer d_model=256 (6 exits x 2), batch {B}/GPU, mel [80 x {T}] -> T'={Tq}, log-normal synthetic mel, random-init weights (BASELINE.json configs[1])",
                       "global_batch": B * world, "mel_frames": T, "parallelism": f"dp{world} (utterance-batch shards)",
                       "precision_mode": args.precision,
                       **({"single_rank_rehearsal": f"every collective of the path issued through a process group of ONE rank on backend {backend!r} (EEC_BENCH_SINGLE_RANK=1)"} if single_rank else {})},
            "frac_of_mfma_peak_whole_forward": round(flop_fwd * world * args.steps / dt / (MFMA_PEAK_FLOPS * world), 4),
            "algorithmic_flop_per_mel_frame": round(flop_fwd / (B * T), 1),
            "distributed": dist_info,
        }
        if args.full:
            line.update({"parity": parity, "roofline": roofline, "cpu_baseline": cpu, "forward_only": forward_only,
                         "kernel_time": kernel_ms, "step_ms": step_ms, "modes": modes, "secondary_shapes": secondary,
                         "config3": config3, "frontend": frontend, "train_step": None, "aed_decode": aed})
    else:
        line = None

    # ---- training-step lines LAST, under a watchdog: every other number of the record is complete by now, and a collective
    # that never returns on some rank (N > 1) must not take the headline line down with it ----
    guard = RecordGuard(rank, line)
    emit, fail_section = guard.emit, guard.fail

    guard.catch_sigterm()
    if args.full and not args.no_modes and not args.no_train:
        guard.start_watchdog(float(os.environ.get("EEC_BENCH_TRAIN_TIMEOUT", "240")))
        n_tr = max(3, args.steps // 10)
        lab4 = (f"CTC training step, default 12-layer d_model=256, batch {B}/GPU x {world} GPU(s), mel [80 x {T}] "
                "(BASELINE.json configs[3]; at N > 1 the per-exit-group gradient buckets are all-reduced under the backward)")
        t_x3 = train_bench(CFG, 3, n_tr, lab4)
        t_bf = train_bench(CFG, 1, n_tr, lab4)
        t3 = None
        if world == 1:
            t3 = train_bench(dict(CFG, d_model=512, n_enc_layers=3), 1, max(2, n_tr // 2),
                             f"CTC training step, 18-layer d_model=512 (6 exits x 3), batch {B}, mel [80 x {T}] (BASELINE.json configs[2])")
        # AED training step (train.py:36-52, --decoder_mode aed; secondary line, N = 1): full_conformer = the same encoder + six
        # attention decoders of six layers; forward in train mode, summed exit CTC + cross-entropy losses, backward, clip, AdamW --
        # encoder AND decoders on the HIP training kernels (eec_train_*, eec_decoder_train_*)
        t_aed = None
        if world == 1:
            try:
                from early_exit_transformer_amd.model import full_conformer
                fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device=dev, **{k: v for k, v in CFG.items() if k != "src_pad_idx"})
                fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
                fc = fc.to(dev).train()
                fparams = list(fc.parameters())
                fopt = torch.optim.AdamW(fparams, lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=0.1, fused=True)
                ce = torch.nn.CrossEntropyLoss(ignore_index=126)
                trg_in, trg_out = tgt[:, :-1].contiguous(), tgt[:, 1:].contiguous()

                def aed_step():
                    fopt.zero_grad(set_to_none=True)
                    dec, enc = fc(mel, lengths, trg_in)
                    loss = exit_ctc_losses(enc, tgt, tgt_len).sum() + sum(ce(d.reshape(-1, d.size(-1)), trg_out.reshape(-1)) for d in dec)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(fparams, 1.0)
                    fopt.step()
                    return loss
                for _ in range(2):
                    loss = aed_step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                n_aed = max(2, n_tr // 2)
                for _ in range(n_aed):
                    loss = aed_step()
                torch.cuda.synchronize()
                d = (time.perf_counter() - t1) / n_aed
                t_aed = {"workload": f"AED training step: full_conformer (12-layer encoder + 6 decoders x 6 layers), batch {B}, mel [80 x {T}], "
                                     f"{trg_in.size(1)} target tokens; CTC + CE losses, backward, clip, AdamW; encoder and decoders on the HIP training kernels",
                         "ms_per_step": round(d * 1e3, 3), "value": round(B * T / d, 1), "unit": "mel-frames/s", "steps": n_aed,
                         "finite_loss": bool(torch.isfinite(loss).item())}
                del fc, fopt, fparams
                torch.cuda.empty_cache()
            except Exception as e:  # a secondary line never takes the record down
                t_aed = {"error": f"{type(e).__name__}: {e}"[:300]}
        if rank == 0:
            train = {"config4_bf16x3": t_x3, "config4_bf16": t_bf, "config3_bf16": t3, "aed_bf16x3": t_aed}

        guard.finish()
        emit(train if rank == 0 else None)
    else:
        guard.finish()
        emit()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
