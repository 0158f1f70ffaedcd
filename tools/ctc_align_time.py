"""Same-box timing of the CTC forced alignment (``ctc_align``, csrc/ctc_align.hip) at the alignment shape of the batched AED
search's standard run (tools/aed_batch_time.py: 6 exits x 64 utterances x beam 10 = 3840 hypotheses, T' = 256 frames, V = 256),
85 tokens per hypothesis, 10 hypotheses per emission that share most of their prefix.

    python tools/ctc_align_time.py [--reps 50] [--baseline-hyps 32] [--no-decode]      JSON lines

* kernel: device time by events around one launch, median of ``--reps`` launches after a warm-up; and the same for a train of
  20 launches (per launch), which takes the launch gap out.
* baseline: the formulation the kernel replaces -- per hypothesis a trellis built frame by frame with tensor ops (T' steps of a
  few launches each) and a backtrack that reads two device scalars per frame on the host --, on ``--baseline-hyps``
  hypotheses, host clock around work that ends in a synchronise, scaled to all 3840.  Its results are compared with the
  kernel's.
* decode_batch at B = 64 (T = 1027 mel frames, beam 10) with and without ``ctc_weight``: host clock, best of two after a warm-up.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from early_exit_transformer_amd import synth  # noqa: E402
from early_exit_transformer_amd.beam import BeamInference  # noqa: E402
from early_exit_transformer_amd.model import ctc_align, full_conformer  # noqa: E402

CFG = dict(n_enc_exits=6, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
           n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31)
KW = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=1.0)
N_EM, BEAM, TQ, V, N_TOK = 384, 10, 256, 256, 85


def workload(dev):
    g = torch.Generator().manual_seed(3840)
    logp = torch.log_softmax(torch.randn(N_EM, TQ, V, generator=g) * 3.0, -1).to(dev)
    base = torch.randint(1, V, (N_EM, 1, N_TOK), generator=g).expand(N_EM, BEAM, N_TOK).clone()
    tail = torch.randint(1, V, (N_EM, BEAM, 6), generator=g)  # the beams of a search differ in their last tokens
    base[:, :, -6:] = tail
    tokens = base.reshape(N_EM * BEAM, N_TOK).to(dev)
    em_index = torch.arange(N_EM, dtype=torch.int32, device=dev).repeat_interleave(BEAM)
    return logp, tokens, em_index


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


def frame_by_frame(em, tok, blank=0):
    """The alignment of one hypothesis the way the kernel's callers would have to write it with tensor ops: one trellis row per
    step, then a walk back that asks the device for every decision.  Returns (path score, trellis[T, N])."""
    T, N = em.size(0), tok.numel()
    tr = torch.full((T + 1, N + 1), float("-inf"), device=em.device)
    tr[:, 0] = torch.cat([em.new_zeros(1), torch.cumsum(em[:, 0], 0)])
    tr[T + 1 - N:, 0] = float("inf")
    for t in range(T):
        tr[t + 1, 1:] = torch.maximum(tr[t, 1:] + em[t, blank], tr[t, :-1] + em[t, tok])
    j, score = N, 0.0
    for t in range(T, 0, -1):
        stay = (tr[t - 1, j] + em[t - 1, blank]).item()
        move = (tr[t - 1, j - 1] + em[t - 1, tok[j - 1]]).item()
        score += em[t - 1, tok[j - 1] if move > stay else 0].item()
        if move > stay:
            j -= 1
            if j == 0:
                break
    return score, float(tr[T, N])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--baseline-hyps", type=int, default=32)
    ap.add_argument("--no-decode", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda:0")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}), flush=True)
    logp, tokens, em_index = workload(dev)
    call = lambda: ctc_align(logp, tokens, em_index=em_index)  # noqa: E731
    for _ in range(5):
        out = call()
    torch.cuda.synchronize()
    assert int(out[4].sum()) == 0
    one = event_ms(call, args.reps)
    train = event_ms(call, max(args.reps // 5, 3), per=20)
    kernel_ms = train[0]
    print(json.dumps({"what": "ctc_align", "hypotheses": N_EM * BEAM, "Tq": TQ, "tokens": N_TOK, "V": V, "per_emission": BEAM,
                      "one_launch_ms": {"median": round(one[0], 4), "min": round(one[1], 4), "max": round(one[2], 4)},
                      "train_of_20_ms_per_launch": {"median": round(train[0], 4), "min": round(train[1], 4), "max": round(train[2], 4)},
                      "us_per_hypothesis": round(1e3 * kernel_ms / (N_EM * BEAM), 4)}), flush=True)

    n = args.baseline_hyps
    pick = list(range(0, N_EM * BEAM, (N_EM * BEAM) // n))[:n]
    frame_by_frame(logp[int(em_index[pick[0]])], tokens[pick[0]])  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    base = [frame_by_frame(logp[int(em_index[h])], tokens[h]) for h in pick]
    torch.cuda.synchronize()
    d = time.perf_counter() - t0
    worst = max(abs(s - float(out[2][h])) / max(1.0, abs(s)) for (s, _), h in zip(base, pick))
    scaled_ms = 1e3 * d / n * N_EM * BEAM
    print(json.dumps({"what": "frame-by-frame tensor ops", "hypotheses_timed": n, "s": round(d, 3), "ms_per_hypothesis": round(1e3 * d / n, 2),
                      "scaled_to_all_ms": round(scaled_ms, 1), "ratio_to_kernel": round(scaled_ms / kernel_ms, 1),
                      "worst_relative_path_score_difference": float(f"{worst:.3g}")}), flush=True)
    del logp, tokens, em_index, out

    if args.no_decode:
        return
    fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device=dev, **CFG).eval()
    fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
    fc = fc.to(dev)
    inf, B, T = BeamInference(), 64, 1027
    mel = synth.synth_mel(B, 80, T, seed=4).to(dev)
    vlen = torch.full((B,), T)
    res = {}
    for w in (None, 0.3):
        best, got = None, None
        for i in range(3):  # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = inf.decode_batch(fc, mel, vlen, beam_size=10, ctc_weight=w, **KW)
            torch.cuda.synchronize()
            if i:
                best = min(best or 1e9, time.perf_counter() - t0)
        res[w] = (best, got)
    moved = sum(a != b for ra, rb in zip(res[None][1], res[0.3][1]) for a, b in zip(ra, rb))
    print(json.dumps({"what": "decode_batch", "B": B, "T": T, "beam": 10, "steps": int(T / 12), "plain_s": round(res[None][0], 4),
                      "ctc_weight_0.3_s": round(res[0.3][0], 4), "added_s": round(res[0.3][0] - res[None][0], 4),
                      "best_beams_changed": f"{moved}/{B * 6}"}), flush=True)


if __name__ == "__main__":
    main()
