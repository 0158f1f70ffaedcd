"""Same-process timing of one-pass joint CTC / attention decoding (BeamInference.decode_batch(joint_ctc_weight=w),
csrc/ctc_prefix.hip) against the plain batched search and the CTC-rescored one (ctc_weight=w), at the bench's AED geometry:
full_conformer (6 exits x 2 encoder layers, 6 decoder layers per exit, d_model 256, d_ff 2048, vocab 256), beam 10, B = 64,
T = 1027 mel frames (85 decoder steps, T' = 256 CTC frames).

    python tools/joint_search_time.py [--batch 64] [--reps 2] [--out profiles/joint_search_time.json]

The yardstick is the plain decode_batch of the same process.  The joint search is timed twice: as it runs (beams that take EOS
cost nothing afterwards) and with min_length = the number of steps, so that no beam may end and every step scores E * B * beam open
beams.  The prefix launch alone is timed with device events over a session of open beams that grow by random labels.  Host clocks
around work that ends in a device synchronise, after a warm-up of the same shape.  The model has synthetic weights: the figures say
what the search costs, nothing about the word error rate."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from early_exit_transformer_amd import synth  # noqa: E402
from early_exit_transformer_amd.beam import BeamInference, default_max_length  # noqa: E402
from early_exit_transformer_amd.model import ctc_prefix_session, encoder_lengths, full_conformer  # noqa: E402

CFG = dict(n_enc_exits=6, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
           n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31)
KW = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=1.0)


def timed(fn, reps):
    fn()  # warm-up of the same shape
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        d = time.perf_counter() - t0
        best = d if best is None else min(best, d)
    return best


def prefix_alone_ms(logp, frames, beam, steps, w):
    """Milliseconds per eec_ctc_prefix_step over ``steps`` steps of E * B searches with ``beam`` open beams each."""
    E, B, Tq, V = logp.shape
    n = E * B
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(3, 126, (steps, n, beam), generator=g).cuda()
    parents = torch.randint(0, beam, (steps, n, beam), generator=g).cuda()
    att = torch.log_softmax(torch.randn(n, beam, V, generator=g), -1).cuda()
    best = None
    for _ in range(2):
        sess = ctc_prefix_session(logp.reshape(n, Tq, V), frames.repeat(E), beam, w, KW["EOS_token"], KW["PAD_token"], min_length=steps)
        sess.step(att[:, :1].contiguous(), labels[0, :, :1].contiguous())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for s in range(1, steps):
            sess.step(att, labels[s], parents[s] if s > 1 else torch.zeros_like(parents[s]))
        t1.record()
        torch.cuda.synchronize()
        d = t0.elapsed_time(t1) / (steps - 1)
        best = d if best is None else min(best, d)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=1027)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "joint_search_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda:0")
    fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device=dev, **CFG).eval()
    fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
    fc = fc.to(dev)
    inf = BeamInference()
    B, T, w, beam = args.batch, args.T, args.weight, 10
    steps = default_max_length(T)
    mel = synth.synth_mel(B, 80, T, seed=4).to(dev)
    vlen = torch.full((B,), T)
    plain = timed(lambda: inf.decode_batch(fc, mel, vlen, beam_size=beam, **KW), args.reps)
    rescored = timed(lambda: inf.decode_batch(fc, mel, vlen, beam_size=beam, ctc_weight=w, **KW), args.reps)
    joint = timed(lambda: inf.decode_batch(fc, mel, vlen, beam_size=beam, joint_ctc_weight=w, **KW), args.reps)
    joint_open = timed(lambda: inf.decode_batch(fc, mel, vlen, beam_size=beam, joint_ctc_weight=w, min_length=steps, **KW), args.reps)
    logp = fc._run_encoder(mel, vlen, want_out=True, want_taps=False, n_groups=CFG["n_enc_exits"])[0]
    frames = encoder_lengths(vlen.to(dev), logp.size(2))
    alone = prefix_alone_ms(logp, frames, beam, steps, w)
    out = {"B": B, "T": T, "beam": beam, "steps": steps, "ctc_frames": int(logp.size(2)), "weight": w,
           "plain_s": round(plain, 4), "plain_utt_per_s": round(B / plain, 2),
           "ctc_weight_s": round(rescored, 4), "ctc_weight_over_plain": round(rescored / plain, 3),
           "joint_s": round(joint, 4), "joint_over_plain": round(joint / plain, 3),
           "joint_no_eos_s": round(joint_open, 4), "joint_no_eos_over_plain": round(joint_open / plain, 3),
           "prefix_step_ms": round(alone, 4), "plain_step_ms": round(1e3 * plain / steps, 4),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
