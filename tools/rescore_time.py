"""Same-process timing of two-pass decoding (BeamInference.decode_batch_rescoring: CTC N-best, csrc/ctc_beam.hip, rescored by the
attention decoder in one teacher-forced pass, csrc/decoder_score.hip) beside the autoregressive searches it stands next to, at
the bench's AED geometry: full_conformer (6 exits x 2 encoder layers, 6 decoder layers per exit, d_model 256, d_ff 2048, vocab
256), B = 64, T = 1027 mel frames (T' = 256 CTC frames), beam 10, nbest 10.

    python tools/rescore_time.py [--rounds 5] [--out profiles/rescore_time.json]

Legs, measured in turn ``--rounds`` times each after a warm-up of every leg (medians; min .. max is what a difference between two
legs has to be read against):
* ``decode_batch`` plain and with ``joint_ctc_weight=0.3``, and ``decode_batch_rescoring`` as a whole (encoder pass included in all
  three): host seconds per call, the device drained at both ends;
* the N-best launch alone over all 384 exit x utterance emissions, beside the 1-best launch: device events;
* the second pass alone -- ``score_hypotheses`` (eec_decoder_score, with the split over memories its workspace bound asks for)
  over the 64 x 10 hypotheses of ONE exit, and the same for all six: device events.
The length of the decoder rows is whatever the N-best lists of this model's emissions hold (``rows_L``): the weights are synthetic,
so the figures say what the mode costs at that length and nothing about the word error rate.  Records, not targets: there is no
pass mark.  A run without a HIP device fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from early_exit_transformer_amd import capi, synth  # noqa: E402
from early_exit_transformer_amd.beam import BeamInference, default_max_length  # noqa: E402
from early_exit_transformer_amd.model import ctc_beam_decode, encoder_lengths, full_conformer  # noqa: E402

CFG = dict(n_enc_exits=6, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
           n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31)
KW = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=1.0)
TOK = dict(SOS_token=1, EOS_token=2)


def spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def host_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(legs, rounds, clock):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(clock(fn))
    return {k: spread(v) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=1027)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rescore_time.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device=dev, **CFG).eval()
    fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
    fc = fc.to(dev)
    inf = BeamInference()
    B, T, E, beam, nbest = args.batch, args.T, CFG["n_enc_exits"], 10, 10
    mel = synth.synth_mel(B, 80, T, seed=4).to(dev)
    vlen = torch.full((B,), T)
    out = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "E": E, "beam": beam, "nbest": nbest, "rounds": args.rounds,
           "decoder_steps_of_the_searches": default_max_length(T), "rescoring_ctc_weight": args.weight}
    with torch.no_grad():
        whole = measure({"decode_batch_plain_s": lambda: inf.decode_batch(fc, mel, vlen, beam_size=beam, **KW),
                         "decode_batch_joint_0.3_s": lambda: inf.decode_batch(fc, mel, vlen, beam_size=beam, joint_ctc_weight=0.3, **KW),
                         "decode_batch_rescoring_s": lambda: inf.decode_batch_rescoring(fc, mel, vlen, nbest=nbest, rescoring_ctc_weight=args.weight,
                                                                                        beam_size=beam, **TOK)}, args.rounds, host_s)
        out.update(whole)
        out["rescoring_over_plain"] = round(whole["decode_batch_rescoring_s"]["median"] / whole["decode_batch_plain_s"]["median"], 4)
        out["encoder_pass_s"] = measure({"e": lambda: fc._run_encoder(mel, vlen, want_out=True, want_taps=True, n_groups=E)}, args.rounds, host_s)["e"]

        logp, taps = fc._run_encoder(mel, vlen, want_out=True, want_taps=True, n_groups=E)[:2]
        frames = encoder_lengths(vlen.to(dev), logp.size(2)).repeat(E)
        every = logp.reshape(E * B, logp.size(2), logp.size(3))
        out["ctc_frames"] = int(logp.size(2))
        out.update(measure({"nbest_launch_384_sequences_ms": lambda: ctc_beam_decode(every, beam_size=beam, em_len=frames, nbest=nbest),
                            "onebest_launch_384_sequences_ms": lambda: ctc_beam_decode(every, beam_size=beam, em_len=frames)}, args.rounds, device_ms))

        tokens, counts, _, n_hyp = ctc_beam_decode(every, beam_size=beam, em_len=frames, nbest=nbest)
        present = torch.arange(nbest, device=dev).view(1, -1) < n_hyp.view(-1, 1)
        lengths = torch.where(present, counts, torch.full_like(counts, -1))
        L = max(int(counts.max()), 1)
        tokens = tokens[:, :, :L].contiguous()
        out["rows_L"] = L
        out["mean_hypothesis_length"] = round(float(counts[present].float().mean()), 2)
        out["hypotheses_present"] = int(present.sum())
        out["decoder_rows"] = E * B * nbest * (L + 1)
        cfg = fc._cfg
        need = capi.load().eec_decoder_score_workspace_bytes(cfg.d_model, cfg.n_heads, CFG["d_feed_forward"], 256, B, nbest, L, int(logp.size(2)))
        out["score_workspace_bytes_one_exit_unsplit"] = int(need)

        def score(e):
            return fc.score_hypotheses(taps[e], e + 1, tokens[e * B:(e + 1) * B], lengths[e * B:(e + 1) * B], TOK["SOS_token"], TOK["EOS_token"])
        # the same lists cut to the length the autoregressive searches decode (their step count): equal output length on both sides
        steps = default_max_length(T)
        cut_tokens, cut_lengths = tokens[:, :, :steps].contiguous(), torch.where(present, counts.clamp(max=steps), lengths)

        def score_cut(e):
            return fc.score_hypotheses(taps[e], e + 1, cut_tokens[e * B:(e + 1) * B], cut_lengths[e * B:(e + 1) * B], TOK["SOS_token"],
                                       TOK["EOS_token"])
        out["decoder_rows_cut_to_the_searches_steps"] = E * B * nbest * (min(L, steps) + 1)
        out.update(measure({"score_hypotheses_one_exit_ms": lambda: score(E - 1),
                            "score_hypotheses_six_exits_ms": lambda: [score(e) for e in range(E)],
                            "score_hypotheses_six_exits_cut_to_the_searches_steps_ms": lambda: [score_cut(e) for e in range(E)]},
                           args.rounds, device_ms))
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
