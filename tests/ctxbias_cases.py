"""Inputs and restatements shared by tests/test_host_ctxbias.py and tests/test_gpu_ctxbias.py (contextual biasing: the graph builder,
the biased CTC prefix beam search, the AED step).  Everything is restated from include/eec.h ("Contextual biasing") in fp64 and
Python integers: the trie and its failure links, the tables, the fp32 bias chain, the closed form by naive substring count, the
biased prefix beam search (oracle/ctc_beam_ref.py's algorithm with the ranking by total + bias) and the AED step.  Seeded, CPU only."""
import functools
import math

import numpy as np
import torch

import ctc_cases as K
import rescore_cases as RC
from oracle.ctc_beam_ref import _lae

NEG = -float("inf")
BOOSTS = (0.0, 1.5, 4.0)
BEAM, NBEST = RC.ORACLE_BEAM, RC.ORACLE_NBEST


# ---------------------------------------------------------------------------------------------------------------------------
# the graph
# ---------------------------------------------------------------------------------------------------------------------------
class Tables:
    """The restated image of one graph: S, delta [S][V] fp32, next [S][V], final [S] fp32, and the fp64 node scores."""

    def __init__(self, phrases, boosts, V, blank=0, eos=None, pad=None):
        child, tscore, end = [{}], [0.0], [False]
        for p, b in zip(phrases, boosts):
            n = 0
            for t in p:
                if t not in child[n]:
                    child[n][t] = len(child)
                    child.append({})
                    tscore.append(0.0)
                    end.append(False)
                n = child[n][t]
                tscore[n] = max(tscore[n], float(b))
            end[n] = True
        N = len(child)
        nscore, out, fail = [0.0] * N, [0.0] * N, [0] * N
        go = [[0] * V for _ in range(N)]
        order = [0]
        for n in order:  # breadth first; the list grows while it is walked
            for t in range(V):
                via = 0 if n == 0 else go[fail[n]][t]
                c = child[n].get(t)
                if c is None:
                    go[n][t] = via
                    continue
                go[n][t] = c
                fail[c] = via
                nscore[c] = nscore[n] + tscore[c]
                out[c] = (nscore[c] if end[c] else 0.0) + out[via]
                order.append(c)
        closing = eos is not None or pad is not None
        S = N + (1 if closing else 0)
        delta, nxt, fin = np.zeros((S, V), np.float32), np.zeros((S, V), np.int32), np.zeros(S, np.float32)
        for s in range(N):
            for t in range(V):
                if t == blank:
                    nxt[s, t], delta[s, t] = s, 0.0
                elif t == eos or t == pad:
                    nxt[s, t], delta[s, t] = N, np.float32(0.0 - nscore[s])
                else:
                    d = go[s][t]
                    nxt[s, t], delta[s, t] = d, np.float32((nscore[d] - nscore[s]) + out[d])
            fin[s] = np.float32(0.0 - nscore[s])
        if closing:
            nxt[N, :] = N
        self.S, self.V, self.delta, self.next, self.final = S, V, delta, nxt, fin
        self.node_score, self.fail, self.end, self.blank, self.eos, self.pad = nscore, fail, end, blank, eos, pad
        self.phrases, self.boosts = [tuple(p) for p in phrases], [float(b) for b in boosts]


def chain32(tab, tokens, state=0, bias=np.float32(0.0)):
    """The fp32 bias chain along ``tokens``: one rounded add per token.  Returns (bias fp32, state)."""
    bias = np.float32(bias)
    for t in tokens:
        bias = np.float32(bias + tab.delta[state, t])
        state = int(tab.next[state, t])
    return bias, state


def bias32(tab, tokens):
    """The bias of the finished hypothesis in fp32: the chain, then fl(bias + final[state])."""
    bias, state = chain32(tab, tokens)
    return np.float32(bias + tab.final[state])


def closed_form(tab, tokens):
    """Sum over every occurrence of every phrase (naive, position by position; overlapping and nested ones count) of the fp64
    node score of the phrase's end node; blanks are taken out and the row is cut at its first eos / pad."""
    row = []
    for t in tokens:
        if t == tab.eos or t == tab.pad:
            break
        if t != tab.blank:
            row.append(int(t))
    total = 0.0
    for p in dict.fromkeys(tab.phrases):
        score = 0.0
        for k in range(1, len(p) + 1):
            score = score + max(b for q, b in zip(tab.phrases, tab.boosts) if q[:k] == p[:k])
        for i in range(len(row) - len(p) + 1):
            if tuple(row[i: i + len(p)]) == p:
                total += score
    return total


# ---------------------------------------------------------------------------------------------------------------------------
# the biased prefix beam search in fp64: oracle/ctc_beam_ref.py line by line, ranked by key = total + bias
# ---------------------------------------------------------------------------------------------------------------------------
def biased_beam_search(logp, tab, beam=BEAM, blank=0, blank_skip_threshold=0.95, skip_drops_frame=False):
    """logp [T', V] -> the final beam [(prefix list, total log-probability, final bias, key)], best key first, ties to the lower
    beam index.  ``tab`` None: no biasing (bias 0 everywhere)."""
    T, V = logp.shape
    log_thr = math.log(blank_skip_threshold) if 0.0 < blank_skip_threshold < 1.0 else 0.0
    beams = [((), 0.0, NEG, 0, 0.0)]  # (prefix, log p_blank, log p_nonblank, graph state, bias)
    for t in range(T):
        lp = logp[t].astype(np.float64)
        lpb = float(lp[blank])
        if blank_skip_threshold < 1.0 and lpb > log_thr:
            if not skip_drops_frame:
                beams = [(p, _lae(pb, pnb) + lpb, NEG, st, bi) for p, pb, pnb, st, bi in beams]
            continue
        index = {b[0]: i for i, b in enumerate(beams)}
        stay_pb = [_lae(pb, pnb) + lpb for _, pb, pnb, _, _ in beams]
        stay_pnb = [(pnb + float(lp[p[-1]])) if p else NEG for p, _, pnb, _, _ in beams]
        cands = []  # (key, id, prefix, pb, pnb, state, bias)
        for i, (p, pb, pnb, st, bi) in enumerate(beams):
            tot = _lae(pb, pnb)
            for c in range(V):
                if c == blank:
                    continue
                v = (pb if (p and p[-1] == c) else tot) + float(lp[c])
                q = p + (c,)
                j = index.get(q)
                if j is not None:
                    stay_pnb[j] = _lae(stay_pnb[j], v)
                else:
                    nb = bi + (float(tab.delta[st, c]) if tab is not None else 0.0)
                    ns = int(tab.next[st, c]) if tab is not None else 0
                    cands.append((v + nb, 16 + c * 16 + i, q, NEG, v, ns, nb))
        for i, (p, _, _, st, bi) in enumerate(beams):
            cands.append((_lae(stay_pb[i], stay_pnb[i]) + bi, i, p, stay_pb[i], stay_pnb[i], st, bi))
        cands = [c for c in cands if c[0] > NEG]
        cands.sort(key=lambda c: (-c[0], c[1]))
        beams = [c[2:] for c in cands[:beam]]
    final = []
    for p, pb, pnb, st, bi in beams:
        fb = bi + (float(tab.final[st]) if tab is not None else 0.0)
        tot = _lae(pb, pnb)
        final.append((list(p), tot, fb, tot + fb))
    final.sort(key=lambda e: -e[3])  # stable: ties to the lower beam index
    return final


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs: the nine N-best blocks of rescore_cases with V >= 7 (searched over all T' frames and over their own lengths), and the
# phrases of each, cut from the unbiased oracle's hypotheses over all T' frames
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blocks():
    """[(T', V, scale, logp [N, T', V] fp32, em_len int32 [N], unbiased oracle beams per sequence)]"""
    plain = RC.oracle_beams(False, False)
    return [blk + (plain[i],) for i, blk in enumerate(RC.nbest_blocks()) if blk[1] >= 7]


@functools.lru_cache(maxsize=None)
def block_phrases(k):
    """The phrases of block k (without boosts): a substring of 2 .. 5 tokens of the unbiased oracle's rank-1 and rank-3 hypotheses
    of each sequence, one random 3-token phrase, and one phrase that is a proper prefix of another (one phrase extended by a token
    when there is none): the nested-occurrence and failure-link paths."""
    T, V, scale, _, _, plain = blocks()[k]
    rng = np.random.RandomState(1000 * k + 7)
    out = []
    for final in plain:
        for rank in (0, 2):
            if rank < len(final) and len(final[rank][0]) >= 2:
                hyp = final[rank][0]
                n = min(len(hyp), int(rng.randint(2, 6)))
                at = int(rng.randint(0, len(hyp) - n + 1))
                out.append(tuple(hyp[at: at + n]))
    out.append(tuple(int(t) for t in rng.randint(1, V, size=3)))
    out = list(dict.fromkeys(out))
    if not any(p != q and q[: len(p)] == p for p in out for q in out):
        base = max(out, key=len)
        out.append(base + (int(rng.randint(1, V)),) if len(base) < 5 else base[:-1])
    return tuple(out)


def block_boosts(k, b):
    """b and b / 2 in turn."""
    return [b if i % 2 == 0 else b / 2 for i in range(len(block_phrases(k)))]


@functools.lru_cache(maxsize=None)
def block_tables(k, b):
    return Tables(block_phrases(k), block_boosts(k, b), blocks()[k][1])


@functools.lru_cache(maxsize=None)
def restated_beams(b, with_len=False):
    """Per block, per sequence: ``biased_beam_search``'s final beam at boost b, over all T' frames or the sequence's own."""
    out = []
    for k, (T, V, scale, logp, lens, _) in enumerate(blocks()):
        tab = block_tables(k, b)
        frames = [int(lens[s]) if with_len else T for s in range(logp.size(0))]
        out.append([biased_beam_search(logp[s, :Ts].double().numpy().reshape(Ts, V), tab) for s, Ts in enumerate(frames)])
    return out


def comparable_ranks(final, nbest=NBEST):
    """rescore_cases.comparable_ranks on the keys: the ranks whose consecutive key gaps up to rank k + 1 all exceed BEAM_MARGIN."""
    ok = []
    for k in range(min(nbest, len(final))):
        gaps = [final[j][3] - final[j + 1][3] for j in range(min(k + 1, len(final) - 1))]
        if all(g > K.BEAM_MARGIN for g in gaps):
            ok.append(k)
        else:
            break
    return ok


# ---------------------------------------------------------------------------------------------------------------------------
# the AED step
# ---------------------------------------------------------------------------------------------------------------------------
def aed_step(tabs, graph_of, prev_state, parent, last, local, s, R_prev):
    """One eec_context_bias_step in Python integers and fp32 adds: tabs [G] Tables, graph_of [n] or None, prev_state [n][R_prev],
    parent / last [n][R] (parent None: r), local [n][R][V] fp32 numpy.  Returns (out, state [n][R])."""
    n, R, V = local.shape
    out = local.copy()
    state = [[0] * R for _ in range(n)]
    for i in range(n):
        g = 0 if graph_of is None else int(graph_of[i])
        if not 0 <= g < len(tabs):
            continue
        tab = tabs[g]
        for r in range(R):
            st = 0
            if s > 0:
                p = r if parent is None else int(parent[i][r])
                c = int(last[i][r])
                if 0 <= p < R_prev and 0 <= c < V:
                    st = int(tab.next[prev_state[i][p], c])
                    st = st if 0 <= st < tab.S else 0
            state[i][r] = st
            for v in range(V):
                if local[i, r, v] != NEG:
                    out[i, r, v] = np.float32(local[i, r, v] + tab.delta[st, v])
    return out, state
