"""Same-box timing of CTC segmentation (``ctc_segment``, csrc/ctc_segment.hip): records, not targets.

    python tools/segment_time.py [--rounds 7] [--out profiles/segment_time.json]
    python tools/segment_time.py --resources-only     # no device: (re)reads the kernel's figures from the built object into the record

Shapes:
* one recording: T' = 32768 frames (about 22 minutes at 40 ms a frame), V = 256, one row of N = 4095 tokens, both ends free -- one
  workgroup of 16 waves;
* character mode: 64 rows of N = 300 tokens (S = 300, two waves a row) at T' = 512, V = 64;
* the benchmarked batch of ``tools/forced_align_time.py``: 3840 rows of about 200 tokens at T' = 256 through ``ctc_segment`` beside
  ``ctc_forced_align`` on the same rows.  The one-wave kernel remains the path for rows of at most 255 tokens; this only records what
  the barrier per frame and the workgroup per row cost.
Medians over ``--rounds`` alternating rounds in one process (every variant once per round), device time between events, the launch
and the output and workspace allocations included; the NumPy host path on the first two shapes, host clock; and the kernel's
register, LDS and spill figures read from the built object csrc/build/ctc_segment.o (tools/kernel_resources.py).
The emissions are log_softmax of scaled noise and the rows random tokens: timings only, no statement about alignment accuracy."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import capi, ctc_forced_align, ctc_segment  # noqa: E402

OBJECT = os.path.join(ROOT, "early_exit_transformer_amd", "csrc", "build", "ctc_segment.o")


def rows(H, S, lo, V, seed):
    """[H, S] int32 random labels, lengths lo .. S; an adjacent repeat is replaced, so few remain."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(1, V, (H, S), generator=g, dtype=torch.int32)
    same = tokens[:, 1:] == tokens[:, :-1]
    tokens[:, 1:][same] = (tokens[:, 1:][same] % (V - 1)) + 1
    lens = torch.randint(lo, S + 1, (H,), generator=g, dtype=torch.int32)
    return tokens, lens


def emission(n, Tq, V, seed):
    return torch.log_softmax(torch.randn(n, Tq, V, generator=torch.Generator().manual_seed(seed)) * 3.0, -1)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def kernel_resources():
    """The ctc_segment_kernel line of tools/kernel_resources.py on the built object."""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), OBJECT, "ctc_segment_kernel"],
                             capture_output=True, text=True, timeout=300).stdout
        line = [ln for ln in out.splitlines() if "ctc_segment_kernel" in ln][0].split()
        keys = ("vgpr", "vgpr_spill", "sgpr", "sgpr_spill", "scratch", "lds_static")
        return {"what": "tools/kernel_resources.py on build/ctc_segment.o; lds_static excludes the 8 * tok_stride bytes of spans per launch",
                **{k: int(v) for k, v in zip(keys, line[1:])}}
    except Exception as err:  # the record says so
        return {"error": repr(err)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_time.json"))
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    if args.resources_only:
        with open(args.out) as f:
            record = json.load(f)
        record["kernel_resources"] = kernel_resources()
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda:0")
    record = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__, "rounds": args.rounds,
              "inputs": "log_softmax(3 * noise), random rows: timings only, records and not targets"}
    lib = capi.load()
    host_x, host_rows = {}, {}

    rec_x = emission(1, 32768, 256, 1)
    rec_t, rec_l = rows(1, 4095, 4095, 256, 2)
    host_x["recording"], host_rows["recording"] = rec_x, (rec_t, rec_l, dict(free_start=True, free_end=True))
    chr_x = emission(64, 512, 64, 3)
    chr_t, chr_l = rows(64, 300, 300, 64, 4)
    host_x["character mode"], host_rows["character mode"] = chr_x, (chr_t, chr_l, {})
    E, B, BEAM = 6, 64, 10
    bat_x = emission(E * B, 256, 256, 384)
    bat_t, bat_l = rows(E * B * BEAM, 208, 192, 256, 3840 + 200)
    bat_i = torch.arange(E * B, dtype=torch.int32).repeat_interleave(BEAM)

    rx, rt, rl = rec_x.to(dev), rec_t.to(dev), rec_l.to(dev)
    cx, ct, cl = chr_x.to(dev), chr_t.to(dev), chr_l.to(dev)
    bx, bt, bl, bi = bat_x.to(dev), bat_t.to(dev), bat_l.to(dev), bat_i.to(dev)
    variants = {
        "ctc_segment recording: 1 row, N = 4095, T' = 32768, free ends": lambda: ctc_segment(rx, rt, rl, free_start=True, free_end=True),
        "ctc_segment character mode: 64 rows, N = 300, T' = 512": lambda: ctc_segment(cx, ct, cl),
        "ctc_segment batch: 3840 rows, ~200 tokens, T' = 256": lambda: ctc_segment(bx, bt, bl, bi),
        "ctc_forced_align batch: 3840 rows, ~200 tokens, T' = 256": lambda: ctc_forced_align(bx, bt, bl, bi),
    }
    record["workspace_bytes"] = {"recording": lib.eec_ctc_segment_workspace_bytes(1, 32768, 4095),
                                 "character mode": lib.eec_ctc_segment_workspace_bytes(64, 512, 300),
                                 "batch, ctc_segment": lib.eec_ctc_segment_workspace_bytes(3840, 256, 208),
                                 "batch, ctc_forced_align": lib.eec_ctc_forced_align_workspace_bytes(3840, 256, 208)}
    first = {name: fn() for name, fn in variants.items()}  # warm-up, and what came out
    torch.cuda.synchronize()
    record["aligned_rows"] = {name: int((al.status == 0).sum()) for name, al in first.items()}
    a, b = first["ctc_segment batch: 3840 rows, ~200 tokens, T' = 256"], first["ctc_forced_align batch: 3840 rows, ~200 tokens, T' = 256"]
    record["batch_bits_equal_one_wave_kernel"] = all(
        torch.equal(getattr(a, n).view(torch.int32), getattr(b, n).view(torch.int32))
        for n in ("tok_start", "tok_end", "tok_score", "frame_token", "path_score", "status"))
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    record["device_ms"] = {name: med(v) for name, v in times.items()}
    k = record["device_ms"]
    record["batch_segment_over_one_wave_kernel"] = round(k["ctc_segment batch: 3840 rows, ~200 tokens, T' = 256"]["median"] /
                                                         k["ctc_forced_align batch: 3840 rows, ~200 tokens, T' = 256"]["median"], 2)
    record["numpy_host_path_ms"] = {}
    for name, reps in (("character mode", 3), ("recording", 2)):
        tokens, lens, kw = host_rows[name]
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctc_segment(host_x[name], tokens, lens, **kw)
            host.append(1e3 * (time.perf_counter() - t0))
        record["numpy_host_path_ms"][name] = med(host)
        got = first[[n for n in first if n.startswith("ctc_segment " + name)][0]]
        want = ctc_segment(host_x[name], tokens, lens, **kw)
        record.setdefault("device_bits_equal_host_path", {})[name] = all(
            torch.equal(getattr(got, n).cpu().view(torch.int32), getattr(want, n).view(torch.int32))
            for n in ("tok_start", "tok_end", "tok_score", "frame_token", "path_score", "status"))
    record["kernel_resources"] = kernel_resources()
    print(json.dumps(record, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
