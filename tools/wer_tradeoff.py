"""The scoring pipeline end to end, as a demonstration: the default model (6 exits x 2 layers, d_model 256) with SYNTHETIC weights,
a synthetic batch, ``synth_targets`` as references.

    python tools/wer_tradeoff.py [--batch 64] [--T 1027] [--nbest 10] [--points 5]

One full forward, one N-best CTC decode of every exit, then
* the per-exit table: token error rate of the best hypothesis, its substitution / deletion / insertion split, and the N-best oracle;
* the oracle exit: the shallowest exit with the fewest errors per utterance;
* for each of the three criteria of adaptive inference (entropy, confidence, greedy_logp) the accuracy-against-depth curve at
  ``--points`` thresholds spread over the criterion's observed range: error rate, mean exit and exit histogram (``exit_tradeoff``,
  whose exits are ``select_exits``' own).

With synthetic weights the hypotheses have nothing to do with the references: every rate printed here is near or above 100 % and
says NOTHING about accuracy.  The tool shows that the pieces fit and what their output looks like.  A run without a HIP device fails."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import ctc, scoring, synth  # noqa: E402
from early_exit_transformer_amd.beam import BeamInference  # noqa: E402
from early_exit_transformer_amd.model import Early_conformer, encoder_lengths  # noqa: E402

E, V = 6, 256
KW = dict(src_pad_idx=0, n_enc_exits=E, enc_voc_size=V, dec_voc_size=V, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
          n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=1027)
    ap.add_argument("--nbest", type=int, default=10)
    ap.add_argument("--points", type=int, default=5)
    ap.add_argument("--target-len", type=int, default=60)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wer_tradeoff.py runs the model on a HIP device; none found")
    B = args.batch
    model = Early_conformer(**KW).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=0, style="trained"))
    model = model.cuda()
    mel, lens = synth.synth_mel(B, 80, args.T, seed=0).cuda(), synth.synth_lengths(B, args.T, seed=0)
    tgt, tl = synth.synth_targets(B, args.target_len, V, seed=0)
    inf = BeamInference()
    print("SYNTHETIC WEIGHTS AND SYNTHETIC REFERENCES: a demonstration of the pipeline; the rates below say nothing about accuracy.\n")
    with torch.no_grad():
        out = model(mel, lens)
        fl = encoder_lengths(lens.cuda(), out.size(2))
        decoded = [inf.ctc_cuda_predict(out[e], beam_size=max(10, args.nbest), lengths=fl, nbest=args.nbest) for e in range(E)]
        stats = ctc.exit_statistics(out, fl)
    table = inf.error_table(decoded, (tgt, tl), device="cuda")
    best = table.errors[..., 0]
    pick, oracle = scoring.nbest_oracle(table.errors)
    n_ref = int(table.ref_len.sum())
    print(f"{B} utterances, {n_ref} reference tokens, {E} exits, N-best lists of up to {args.nbest}\n")
    print("exit   TER %   subs   dels    ins   N-best oracle TER %")
    rate, oracle_rate = table.rate(), table.rate(oracle)
    for e in range(E):
        print(f"{e:4d} {100 * rate[e]:7.2f} {int(table.subs[e, :, 0].sum()):6d} {int(table.dels[e, :, 0].sum()):6d} "
              f"{int(table.ins[e, :, 0].sum()):6d} {100 * oracle_rate[e]:12.2f}")
    exit_of, fewest = scoring.oracle_exit(best)
    print(f"\noracle exit: TER {100 * scoring.error_rate(fewest, table.ref_len).item():.2f} % at mean exit {exit_of.double().mean().item():.2f}, "
          f"histogram {torch.bincount(exit_of.long(), minlength=E).tolist()}\n")
    for criterion, higher in ctc.EXIT_CRITERIA.items():
        score = getattr(stats, criterion)
        lo, hi = float(score.min()), float(score.max())
        thresholds = [lo + (hi - lo) * k / (args.points - 1) for k in range(args.points)] if args.points > 1 else [lo]
        curve = scoring.exit_tradeoff(best, table.ref_len, score, thresholds, higher_is_better=higher)
        print(f"criterion {criterion} ({'above' if higher else 'below'} the threshold passes)")
        print("   threshold   TER %   mean exit   utterances per exit")
        for k, thr in enumerate(thresholds):
            print(f"{thr:12.4f} {100 * curve.rate[k]:7.2f} {curve.mean_exit[k]:11.2f}   {curve.histogram[k].tolist()}")
        print()
    print("SYNTHETIC WEIGHTS: no accuracy is claimed.")


if __name__ == "__main__":
    main()
