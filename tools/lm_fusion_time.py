"""Same-process timing of shallow fusion with a token-level n-gram model (csrc/ctc_beam_lm.hip, csrc/lm_fusion.hip) on
ctc_cases.big_batch_logp's geometry, [384, 256, 256] log-probs (6 exits x 64 utterances, T' = 256, V = 256), at beam 10, under a
synthetic 3-gram over the 256 pieces.

    python tools/lm_fusion_time.py [--rounds 7] [--parent-lib path/to/the/parent/commit's/libeec.so] [--out profiles/lm_fusion_time.json]

Legs, measured in turn ``--rounds`` times each after a warm-up of every leg (medians; min .. max is what a difference between two
legs has to be read against):
* ``ctc_beam_decode`` as it was (eec_ctc_beam_decode_len), and -- with ``--parent-lib`` -- the same entry of a library built from the
  parent commit, loaded beside this one: the device code of that object is unchanged (tools/isa_diff.sh), so no change is expected;
* the fused entry (eec_ctc_beam_decode_lm) at weight 0.3, by device events;
* the AED step launch alone (eec_lm_fusion_step) on [384, 10, 256] rows, by device events;
* ``decode_batch`` of the bench's AED model at B = 64 (``--batch``) with and without ``token_lm``, by host clocks around work that ends
  in a device synchronise (``--no-aed`` leaves it out).
The emissions, the model's weights and the n-gram are random: the figures say what the mode costs and nothing about any error rate.
Records, not targets: there is no pass mark.  A run without a HIP device fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ctxbias_time import device_ms, emissions, parent_entry, spread  # noqa: E402
from early_exit_transformer_amd.ctc import ctc_beam_decode  # noqa: E402
from early_exit_transformer_amd.lm_fusion import DEFAULT_LM_WEIGHT, LMFusionSession, TokenLM  # noqa: E402

N, T, V, BEAM, R = 384, 256, 256, 10, 10
SOS, EOS, PAD = 1, 2, 126


def trigram(seed=3, per_context=24, contexts=120):
    """A random, prefix-closed 3-gram over the 252 ordinary pieces and <s>, </s>, <unk>: every word has a unigram, ``contexts`` words
    have ``per_context`` bigrams each, and as many bigrams have ``per_context`` trigrams each."""
    rng = np.random.RandomState(seed)
    ordinary = [v for v in range(V) if v not in (0, SOS, EOS, PAD)]
    W = len(ordinary) + 3
    bos, eos, unk = W - 3, W - 2, W - 1
    word_map = np.full(V, unk, dtype=np.int32)
    word_map[ordinary] = np.arange(len(ordinary))
    uni = np.arange(W, dtype=np.int32).reshape(-1, 1)
    heads = rng.choice([w for w in range(W) if w != eos], size=contexts, replace=False)
    bi = np.array([(h, w) for h in heads for w in rng.choice([w for w in range(W) if w != bos], size=per_context, replace=False)], dtype=np.int32)
    open_bi = bi[bi[:, 1] != eos]
    tri_heads = open_bi[rng.choice(len(open_bi), size=contexts, replace=False)]
    tri = np.array([(a, b, w) for a, b in tri_heads for w in rng.choice([w for w in range(W) if w != bos], size=per_context, replace=False)],
                   dtype=np.int32)
    words = [uni, bi, tri]
    logp = [(-4.0 * rng.rand(len(g))).astype(np.float32) for g in words]
    backoff = [(-rng.rand(len(g))).astype(np.float32) for g in words[:2]] + [np.zeros(len(tri), dtype=np.float32)]
    return TokenLM(words, logp, backoff, V, word_map, bos=bos, eos_word=eos, unk=unk, blank=0, sos=SOS, eos=EOS, pad=PAD)


def decode_batch_legs(lm, batch, dev):
    """(plain, fused) decode_batch at the bench's AED geometry, as tools/joint_search_time.py builds it."""
    from early_exit_transformer_amd import synth
    from early_exit_transformer_amd.beam import BeamInference
    from joint_search_time import CFG, KW
    from early_exit_transformer_amd.model import full_conformer
    fc = full_conformer(trg_pad_idx=PAD, n_dec_layers=6, device=dev, **CFG).eval()
    fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
    fc = fc.to(dev)
    inf = BeamInference()
    mel = synth.synth_mel(batch, 80, 1027, seed=4).to(dev)
    vlen = torch.full((batch,), 1027)

    def host_s(fn):
        def run():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return run
    return (host_s(lambda: inf.decode_batch(fc, mel, vlen, beam_size=BEAM, **KW)),
            host_s(lambda: inf.decode_batch(fc, mel, vlen, beam_size=BEAM, token_lm=lm, **KW)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-aed", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_fusion_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_fusion_time.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    logp = emissions().to(dev)
    lm = trigram()
    w = DEFAULT_LM_WEIGHT
    legs = {"ctc_beam_decode_ms": lambda: device_ms(lambda: ctc_beam_decode(logp, beam_size=BEAM))}
    if args.parent_lib:
        parent = parent_entry(args.parent_lib, logp)
        legs["ctc_beam_decode_parent_commit_ms"] = lambda: device_ms(parent)
    legs["ctc_beam_decode_lm_ms"] = lambda: device_ms(lambda: ctc_beam_decode(logp, beam_size=BEAM, lm=lm, lm_weight=w))
    local = torch.randn(N, R, V, device=dev)
    last = torch.randint(3, V, (N, R), device=dev)
    parent_rows = torch.randint(0, R, (N, R), device=dev)
    sess = LMFusionSession(lm, N, R, w)
    sess.step(local[:, :1].contiguous(), last[:, :1].contiguous(), None)
    for _ in range(3):  # states of every depth
        sess.step(local, last, parent_rows)
    legs["lm_fusion_step_384x10x256_ms"] = lambda: device_ms(lambda: sess.step(local, last, parent_rows))
    if not args.no_aed:
        plain, fused = decode_batch_legs(lm, args.batch, dev)
        legs["decode_batch_s"], legs["decode_batch_token_lm_s"] = plain, fused

    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            got[k].append(fn())
    out = {"device": torch.cuda.get_device_name(0), "shape": [N, T, V], "beam": BEAM, "rounds": args.rounds, "lm_weight": w,
           "model": {"order": lm.order, "n_grams": lm.ngram.n_grams, "image_bytes": lm.nbytes}}
    out.update({k: spread(v) for k, v in got.items()})
    base = out["ctc_beam_decode_ms"]["median"]
    out["fused_over_plain"] = round(out["ctc_beam_decode_lm_ms"]["median"] / base, 4)
    if args.parent_lib:
        out["plain_over_parent_commit"] = round(base / out["ctc_beam_decode_parent_commit_ms"]["median"], 4)
        want, have = parent(), ctc_beam_decode(logp, beam_size=BEAM)
        torch.cuda.synchronize()
        out["same_bits_as_parent_commit"] = bool(torch.equal(want[1], have[1]) and torch.equal(want[2].view(torch.int32), have[2].view(torch.int32)))
    else:
        out["ctc_beam_decode_parent_commit_ms"] = None  # not measured in this run
    if not args.no_aed:
        out["decode_batch_B"] = args.batch
        out["decode_batch_token_lm_over_plain"] = round(out["decode_batch_token_lm_s"]["median"] / out["decode_batch_s"]["median"], 4)
    plain_out, fused_out = ctc_beam_decode(logp, beam_size=BEAM), ctc_beam_decode(logp, beam_size=BEAM, lm=lm, lm_weight=w)
    moved = sum(plain_out[0][i, : int(plain_out[1][i])].tolist() != fused_out[0][i, : int(fused_out[1][i])].tolist() for i in range(N))
    out["sequences_whose_best_hypothesis_moved"] = int(moved)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
