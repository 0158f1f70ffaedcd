"""Search quality of the lexicon CTC beam search with an n-gram model, with and without LM look-ahead (max trie smearing), on
synthetic utterances.  Not a gate: a record of what smearing changes at small beams.

    python tools/lexbeam_search_quality.py [--utts 256] [--frames 96] [--out profiles/lexbeam_smear_quality.json]       JSON lines

* lexicon and trie: the synthetic spellings of tools/lexbeam_time.py (the real lexicon's size).
* model: synthetic, built as arrays: Zipf unigrams over the lexicon's words plus ``<unk>``, ``<s>``, ``</s>``, and ``--bigrams``
  bigrams whose contexts and successors are Zipf-drawn and whose log-probs lie well above the unigrams'.
* sentences: sampled from that model -- from ``<s>``, a successor of the current word by its bigram probabilities where it has any
  (else a Zipf unigram), 2 to 7 words.  Emissions: the sentence's spelled label path (runs of 1 or 2 frames, a blank between
  doubled tokens, blanks and sil between words) plus unit Gaussian noise at every label, log-softmax; the path's peak height is one
  of ``--peaks`` in turn.
* configurations: beams 2, 5, 10 and 16 (``--beams``: any of 1 .. 64, e.g. ``2,5,10,16,32,50,64``; beams over 16 run the wide-beam
  kernel, csrc/ctc_lexbeam_wide.hip), each with and without smearing, at every ``--lm-weights``.  Per utterance the best final
  score ANY configuration found is the yardstick (final scores are comparable: for one hypothesis the smeared payments telescope
  to the unsmeared word scores).  Per configuration: the share of utterances whose best hypothesis falls short of the yardstick
  (none counts as short), the share without a hypothesis, and the word errors (edit distance against the sampled sentence, an
  utterance without a hypothesis counting all its words) over the sampled words, per peak height and overall.

Synthetic emissions cannot settle what real speech under a real model would show."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from early_exit_transformer_amd.ctc import ctc_lexicon_decode  # noqa: E402
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie  # noqa: E402
import lexbeam_cases as L  # noqa: E402  (tests/: log_softmax)
from lexbeam_time import synthetic_spellings  # noqa: E402

BLANK, SIL = 0, 126


def zipf(n, s=1.0):
    p = 1.0 / np.arange(1, n + 1) ** s
    return p / p.sum()


def synthetic_model(n_words, n_bigrams, seed=5):
    """(NGramLM of order 2, successors {word: (successor ids, probabilities)}, unigram probabilities over the lexicon's words)"""
    rng = np.random.default_rng(seed)
    W = n_words + 3
    unk, bos, eos = n_words, n_words + 1, n_words + 2
    rank = rng.permutation(n_words)                      # word -> its frequency rank
    p_uni = zipf(n_words)[rank]
    lp1 = np.concatenate([np.log10(p_uni * 0.9), [-3.0, -99.0, -1.3]]).astype(np.float32)
    by_rank = np.argsort(rank)
    ctx = np.concatenate([by_rank[rng.choice(n_words, size=n_bigrams, p=zipf(n_words))], np.full(4000, bos)])
    suc = by_rank[rng.choice(n_words, size=len(ctx), p=zipf(n_words, 0.7))]
    key = np.unique(ctx.astype(np.int64) * W + suc)
    bi = np.stack([key // W, key % W], axis=1).astype(np.int32)
    lp2 = rng.uniform(-2.0, -0.3, size=len(bi)).astype(np.float32)
    ends = np.stack([by_rank[:2000], np.full(2000, eos)], axis=1).astype(np.int32)  # frequent words like to end a sentence
    order = np.lexsort((np.concatenate([bi[:, 1], ends[:, 1]]), np.concatenate([bi[:, 0], ends[:, 0]])))
    bi2 = np.concatenate([bi, ends])[order]
    lp2 = np.concatenate([lp2, np.full(2000, -0.7, dtype=np.float32)])[order]
    words = [np.arange(W, dtype=np.int32)[:, None], bi2]
    backoff = [rng.uniform(-0.8, -0.2, size=W).astype(np.float32), np.zeros(len(bi2), dtype=np.float32)]
    lm = NGramLM(words, [lp1, lp2], backoff, np.arange(n_words, dtype=np.int32), bos, eos, unk)
    starts = np.flatnonzero(np.diff(np.concatenate([[-1], bi2[:, 0]])))
    succ = {}
    for a, b in zip(starts, np.concatenate([starts[1:], [len(bi2)]])):
        keep = bi2[a:b, 1] < n_words
        if keep.any():
            p = 10.0 ** lp2[a:b][keep].astype(np.float64)
            succ[int(bi2[a, 0])] = (bi2[a:b, 1][keep], p / p.sum())
    return lm, succ, p_uni, bos


def sample_sentence(rng, succ, p_uni, bos):
    words, at = [], bos
    for _ in range(int(rng.integers(2, 8))):
        if at in succ and rng.random() < 0.8:
            ids, p = succ[at]
            at = int(ids[rng.choice(len(ids), p=p)])
        else:
            at = int(rng.choice(len(p_uni), p=p_uni))
        words.append(at)
    return words


def spelled_path(rng, sentence, spellings, T):
    """The label path of ``sentence`` in at most T frames (words that no longer fit are cut off the sentence), padded with blanks."""
    path, kept = [], []
    for w in sentence:
        word = []
        for c in spellings[w]:
            if (word or path) and (word or path)[-1] == c:
                word.append(BLANK)
            word += [c] * int(rng.integers(1, 3))
        word += [SIL if rng.random() < 0.5 else BLANK] * int(rng.integers(1, 3))
        if len(path) + len(word) > T:
            break
        path += word
        kept.append(w)
    return path + [BLANK] * (T - len(path)), kept


def edit_distance(a, b):
    d = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, y in enumerate(b, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (x != y))
    return d[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--bigrams", type=int, default=1000000)
    ap.add_argument("--peaks", default="3,4,5,7")
    ap.add_argument("--lm-weights", default="1.0,3.23")
    ap.add_argument("--beams", default="2,5,10,16", help="comma-separated beam sizes, each 1 .. 64")
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the search runs there")
    peaks = [float(p) for p in args.peaks.split(",")]
    rng = np.random.default_rng(17)
    spellings = synthetic_spellings()
    trie = TokenTrie.from_spellings(spellings, 256, blank=BLANK, sil=SIL)
    lm, succ, p_uni, bos = synthetic_model(len(spellings), args.bigrams)
    records = [{"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__},
               {"what": "setup", "words": len(spellings), "trie_nodes": trie.n_nodes, "n_grams": lm.n_grams, "utterances": args.utts,
                "frames": args.frames, "peaks": peaks}]
    x = rng.standard_normal((args.utts, args.frames, 256))
    truth = []
    for s in range(args.utts):
        path, kept = spelled_path(rng, sample_sentence(rng, succ, p_uni, bos), spellings, args.frames)
        x[s, np.arange(args.frames), path] += peaks[s % len(peaks)]
        truth.append(kept)
    records[1]["sampled_words"] = sum(len(t) for t in truth)
    print(json.dumps(records[1]), flush=True)
    em = torch.from_numpy(L.log_softmax(x)).cuda()
    for weight in (float(w) for w in args.lm_weights.split(",")):
        found = {}
        beams = [int(b) for b in args.beams.split(",")]
        if not all(1 <= b <= 64 for b in beams):
            ap.error("--beams: every beam must be 1 .. 64")
        for beam in beams:
            for smearing in (None, "max"):
                words, wc, _, _, _, scores, nh = ctc_lexicon_decode(em, trie, beam_size=beam, nbest=1, lm=lm, lm_weight=weight, smearing=smearing)
                words, wc, scores, nh = words[:, 0].cpu().numpy(), wc[:, 0].cpu().numpy(), scores[:, 0].cpu().numpy(), nh.cpu().numpy()
                found[(beam, smearing)] = (scores, [words[s, :wc[s]].tolist() if nh[s] else None for s in range(args.utts)])
        best = np.max(np.stack([f[0] for f in found.values()]), axis=0)  # -inf where no configuration found a hypothesis
        for (beam, smearing), (scores, hyps) in found.items():
            rec = {"what": "quality", "lm_weight": weight, "beam": beam, "smearing": smearing or "off"}
            groups = [("all", range(args.utts))] + [(f"peak_{p:g}", range(k, args.utts, len(peaks))) for k, p in enumerate(peaks)]
            for name, idx in groups:
                idx = list(idx)
                errors = sum(len(truth[s]) if hyps[s] is None else edit_distance(hyps[s], truth[s]) for s in idx)
                rec[name] = {"short_of_best_share": round(float(np.mean([not scores[s] >= best[s] for s in idx])), 4),
                             "no_hypothesis_share": round(float(np.mean([hyps[s] is None for s in idx])), 4),
                             "word_errors": errors, "words": sum(len(truth[s]) for s in idx),
                             "wer": round(errors / max(sum(len(truth[s]) for s in idx), 1), 4)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
