"""Same-box timing of the batched AED search (BeamInference.decode_batch, csrc/decoder_batch.hip) against evaluate_batch_ae's loop
(inference.py:18-62: decode_all_exits per utterance) at the bench's AED geometry: full_conformer (6 exits x 2 encoder layers,
6 decoder layers per exit, d_model 256, d_ff 2048, vocab 256), beam 10, T = 1027 mel frames (85 decoder steps).

    python tools/aed_batch_time.py [--batches 1 8 32 64] [--reps 2]      utterances/s of both paths per batch size (JSON lines)
    python tools/aed_batch_time.py --trace-batch 8                       one decode_batch only (for a kernel trace)

Both paths run the encoder and the search; the times are host clocks around work that ends in a device synchronise, after a
warm-up of the same shape.  Outputs of the two paths are compared (best sequences per utterance and exit)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from early_exit_transformer_amd import synth  # noqa: E402
from early_exit_transformer_amd.beam import BeamInference  # noqa: E402
from early_exit_transformer_amd.model import full_conformer  # noqa: E402

CFG = dict(n_enc_exits=6, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
           n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31)
KW = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=1.0)


def timed(fn, reps):
    fn()  # warm-up of the same shape
    torch.cuda.synchronize()
    best, out = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        d = time.perf_counter() - t0
        best = d if best is None else min(best, d)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--T", type=int, default=1027)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--trace-batch", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda:0")
    fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device=dev, **CFG).eval()
    fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
    fc = fc.to(dev)
    inf = BeamInference()
    T = args.T
    if args.trace_batch:
        B = args.trace_batch
        mel = synth.synth_mel(B, 80, T, seed=4).to(dev)
        vlen = torch.full((B,), T)
        inf.decode_batch(fc, mel, vlen, beam_size=10, **KW)
        torch.cuda.synchronize()
        print(json.dumps({"traced_batch": B, "steps": int(T / 12)}))
        return
    for B in args.batches:
        mel = synth.synth_mel(B, 80, T, seed=4).to(dev)
        vlen = torch.full((B,), T)
        d_loop, want = timed(lambda: [inf.decode_all_exits(fc, mel[b], vlen[b], beam_size=10, **KW) for b in range(B)], args.reps)
        d_batch, got = timed(lambda: inf.decode_batch(fc, mel, vlen, beam_size=10, **KW), args.reps)
        same = sum(g == w for gr, wr in zip(got, want) for g, w in zip(gr, wr))
        print(json.dumps({"B": B, "T": T, "beam": 10, "steps": int(T / 12),
                          "loop_s": round(d_loop, 4), "loop_utt_per_s": round(B / d_loop, 2),
                          "batch_s": round(d_batch, 4), "batch_utt_per_s": round(B / d_batch, 2),
                          "speedup": round(d_loop / d_batch, 2), "same_best_beams": f"{same}/{B * 6}"}), flush=True)
        del mel
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
