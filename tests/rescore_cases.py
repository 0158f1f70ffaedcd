"""Inputs and fp64 restatements shared by tests/test_host_rescore.py and tests/test_gpu_rescore.py (two-pass decoding: the
N-best end of the CTC prefix beam search, the hypothesis scoring kernel, eec_decoder_score and the mode on top of them).
Everything here is seeded and runs on the CPU; the oracle of the search is oracle/ctc_beam_ref.py (``return_beams=True``)."""
import functools
import itertools
import math

import numpy as np
import torch

import ctc_cases as K
from oracle.ctc_beam_ref import ctc_prefix_beam_search

NEG = -float("inf")

# ---------------------------------------------------------------------------------------------------------------------------
# N-best: sequences of ctc_cases.beam_logp at small shapes, N = 4 per (shape, scale)
# ---------------------------------------------------------------------------------------------------------------------------
NBEST_SHAPES = ((1, 5), (9, 7), (23, 32), (40, 256))
NBEST_SCALES = (3.0, 8.0, 16.0)
NBEST_N = 4
ORACLE_BEAM, ORACLE_NBEST = 16, 4
SCORE_RTOL = 2e-3  # the existing beam test's bound: |score - oracle| <= 2e-3 * max(1, |oracle|)
MIN_COMPARED = 0.75


def nbest_blocks():
    """[(T', V, scale, logp [N, T', V] fp32, em_len int32 [N])]: the lengths hold 0, T', and two in between."""
    out = []
    for (T, V), scale in itertools.product(NBEST_SHAPES, NBEST_SCALES):
        lens = torch.tensor([0, T, max(1, T // 2), max(0, T - 1)], dtype=torch.int32)
        out.append((T, V, scale, K.beam_logp(NBEST_N, T, V, scale, seed=int(scale)).float(), lens))
    return out


# the (lengths?, skip reading) pairs whose scores and token sequences are held to the oracle's; the size of the list is held to
# the oracle's final beam under all four
ORACLE_VARIANTS = ((False, False), (True, True))
ALL_VARIANTS = ((False, False), (False, True), (True, False), (True, True))


@functools.lru_cache(maxsize=None)
def oracle_beams(with_len: bool, skip_drops: bool, beam: int = ORACLE_BEAM, max_vocab: int = 256):
    """Per block, per sequence: the oracle's final beam [(prefix, total log-probability)], best first, ties to the lower beam
    index (the oracle's sort is stable), at the reference's skip threshold; None for a block whose V is above ``max_vocab`` (the
    oracle's time is T' * beam * V Python steps per sequence: the smaller beams are run on the smaller vocabularies only)."""
    out = []
    for T, V, scale, logp, lens in nbest_blocks():
        if V > max_vocab:
            out.append(None)
            continue
        rows = []
        for s in range(logp.size(0)):
            Ts = int(lens[s]) if with_len else T
            rows.append(ctc_prefix_beam_search(logp[s, :Ts].double().numpy().reshape(Ts, V), beam=beam, blank=0, blank_skip_threshold=0.95,
                                               return_beams=True, skip_drops_frame=skip_drops)[2])
        out.append(rows)
    return out


def comparable_ranks(final, nbest=ORACLE_NBEST):
    """The ranks k < min(nbest, len(final)) whose token sequence is compared: every consecutive gap of the oracle's scores up to
    rank k + 1 exceeds BEAM_MARGIN (an fp32 search may order a closer pair the other way)."""
    ok = []
    for k in range(min(nbest, len(final))):
        gaps = [final[j][1] - final[j + 1][1] for j in range(min(k + 1, len(final) - 1))]
        if all(g > K.BEAM_MARGIN for g in gaps):
            ok.append(k)
        else:
            break
    return ok


def rank_census(with_len, skip_drops):
    """(compared, present) over every (sequence, rank < 4) pair of one variant."""
    compared = present = 0
    for rows in oracle_beams(with_len, skip_drops):
        for final in rows:
            present += min(ORACLE_NBEST, len(final))
            compared += len(comparable_ranks(final))
    return compared, present


def unpruned_case():
    """V = 3, T' = 3: every label sequence that 3 frames can spell fits a beam of 16, so nothing is pruned.  Returns (logp [1, 3, 3]
    fp32, {prefix tuple: log-probability}) -- the brute-force sum over all V^T' paths in fp64."""
    g = torch.Generator().manual_seed(33)
    logp = torch.log_softmax(torch.randn(1, 3, 3, generator=g, dtype=torch.float64) * 2.0, -1).float()
    lp = logp[0].double().numpy()
    total = {}
    for path in itertools.product(range(3), repeat=3):
        p = sum(lp[t, c] for t, c in enumerate(path))
        labels = tuple(c for i, c in enumerate(path) if c != 0 and (i == 0 or path[i - 1] != c))
        total[labels] = p if labels not in total else float(np.logaddexp(total[labels], p))
    return logp, total


# ---------------------------------------------------------------------------------------------------------------------------
# the scoring kernel alone
# ---------------------------------------------------------------------------------------------------------------------------
SCORE_VOCABS = (2, 32, 256, 1000, 37)  # 2 and 37: the scalar-load path; 1000: four float4 steps with a ragged last one
SCORE_L = 6
SCORE_LENS = (0, 1, SCORE_L, -1, 3, SCORE_L, 2, -1, 0, SCORE_L, 1, 4)
SCORE_EOS = 1


def score_case(V):
    """(logits [n_hyp * (L + 1), V] fp32, tokens [n_hyp, L] int32, lengths [n_hyp] int32): randn rows at scales 1 .. 20, so that
    |logit| reaches about 60 on some rows and stays near 1 on others."""
    g = torch.Generator().manual_seed(V)
    n, S = len(SCORE_LENS), SCORE_L + 1
    scale = torch.tensor([1.0, 4.0, 20.0, 0.1])[torch.arange(n * S) % 4].view(-1, 1)
    logits = torch.randn(n * S, V, generator=g) * scale
    for row in (2 * S + 2, 5 * S + 3):  # inside hypotheses of full length
        logits[row] = logits[row] / logits[row].abs().max() * 60.0
    tokens = torch.randint(0, V, (n, SCORE_L), generator=g, dtype=torch.int32)
    return logits, tokens, torch.tensor(SCORE_LENS, dtype=torch.int32)


def score_reference(logits, tokens, lengths, eos):
    """The fp64 definition: (scores [n_hyp] fp64, -inf where absent; bound [n_hyp] = (k + 1) * (2^-22 * M + 4e-7), M the largest
    |logit| of the hypothesis' k + 1 rows)."""
    n, L = tokens.shape
    S = L + 1
    lp = torch.log_softmax(logits.double(), -1).view(n, S, -1)
    mag = logits.double().abs().view(n, S, -1)
    want, bound = torch.full((n,), NEG, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for h in range(n):
        k = int(lengths[h])
        if k < 0:
            continue
        targets = tokens[h, :k].tolist() + [eos]
        want[h] = sum(lp[h, t, y] for t, y in enumerate(targets))
        bound[h] = (k + 1) * (2.0 ** -22 * mag[h, : k + 1].max().item() + 4e-7)
    return want, bound


# ---------------------------------------------------------------------------------------------------------------------------
# the mix and the pick, in fp64
# ---------------------------------------------------------------------------------------------------------------------------
def mix(ctc, att, w):
    """joint[r] = (1 - w) * att[r] + w * ctc[r] in fp64; a score whose weight is 0 does not enter (so w = 1 ranks by the CTC
    score alone whatever the attention score is, and the other way round)."""
    out = []
    for c, a in zip(ctc, att):
        j = 0.0
        if w < 1.0:
            j += (1.0 - w) * float(a)
        if w > 0.0:
            j += w * float(c)
        out.append(j)
    return out


def pick(joint):
    """The rank of the highest joint score, ties to the lower rank; hypotheses that are absent are not in the list."""
    best = 0
    for r, j in enumerate(joint):
        if j > joint[best]:
            best = r
    return best


def mix_examples():
    """[(ctc, att, w, joint, best)] worked by hand."""
    return [([-1.0, -2.0, -3.0], [-9.0, -4.0, -1.0], 0.5, [-5.0, -3.0, -2.0], 2),
            ([-1.0, -2.0, -3.0], [-9.0, -4.0, -1.0], 1.0, [-1.0, -2.0, -3.0], 0),
            ([-1.0, -2.0, -3.0], [-9.0, -4.0, -1.0], 0.0, [-9.0, -4.0, -1.0], 2),
            ([-1.0, -3.0], [-3.0, -1.0], 0.5, [-2.0, -2.0], 0),              # a tie goes to the lower rank
            ([-1.0, -2.0], [NEG, -4.0], 1.0, [-1.0, -2.0], 0),               # weight 0 on an infinite score: no NaN
            ([-0.5], [-7.25], 0.25, [-5.5625], 0)]


# ---------------------------------------------------------------------------------------------------------------------------
# eec_decoder_score
# ---------------------------------------------------------------------------------------------------------------------------
DEC_MODELS = (dict(d_model=64, n_head=4, d_feed_forward=128, n_dec_layers=2), dict(d_model=256, n_head=8, d_feed_forward=512, n_dec_layers=3))
DEC_N, DEC_TQ, DEC_R, DEC_L = 3, 17, 4, 9
DEC_SOS, DEC_EOS, DEC_PAD = 1, 2, 126
DEC_LENS = ((0, 1, 5, 9), (9, -1, 5, 1), (5, 9, 0, 1))  # every length of {0, 1, 5, 9} in every memory but one, one absent
DEC_PAD_AT = (2, 0, 2)  # hypothesis (memory 2, rank 0), of length 5, holds pad_idx at position 2


def decoder_case(d_model):
    """(enc [n, T', D], tokens [n, R, L] int32, lengths [n, R] int32): ids in [3, 256) without pad_idx, except the one placed."""
    g = torch.Generator().manual_seed(d_model)
    enc = torch.randn(DEC_N, DEC_TQ, d_model, generator=g)
    tokens = torch.randint(3, 256, (DEC_N, DEC_R, DEC_L), generator=g, dtype=torch.int32)
    tokens[tokens == DEC_PAD] = DEC_PAD + 1
    i, r, t = DEC_PAD_AT
    tokens[i, r, t] = DEC_PAD
    return enc, tokens, torch.tensor(DEC_LENS, dtype=torch.int32)


def decoder_row(tokens_row, k):
    """The decoder input of a hypothesis run alone (SOS, y_1 .. y_k: S = k + 1) and its targets (y_1 .. y_k, EOS)."""
    y = [int(t) for t in tokens_row[:k]]
    return torch.tensor([[DEC_SOS] + y], dtype=torch.int64), y + [DEC_EOS]


def gather_sum(logp_row, targets):
    """sum_t logp[t][target_t] in fp64 of one row's log-probs [k + 1, V]."""
    return math.fsum(float(logp_row[t, y]) for t, y in enumerate(targets))
