"""The float64 statement of the CTC prefix scores and of the one-pass joint CTC / attention beam search (include/eec.h, "CTC
prefix scores"), a brute-force enumerator over all V^T paths that pins the statement, and the bound the fp32 implementations
(csrc/ctc_prefix.hip, ``CtcPrefixSession``'s host path) are held to.  Plain Python and numpy; no product code (the helpers at the end
drive a session the caller builds).

The bound is derived, not tuned.  Every value at frame t depends on a chain of at most T frame transitions, and log_add is
1-Lipschitz in each argument, so errors add along the chain and are never amplified.  A transition adds three fp32 roundings of
magnitude at most M (2^-24 * M each, 2^-22 * M with margin for the final subtraction and the mix) and two log_add errors (the
project's log_add: 9.9e-8 measured, 1.2e-7 asserted; 4e-7 for two with margin):
    bound(T, M) = T * (2^-22 * M + 4e-7),   M = the largest finite magnitude in the fp64 state (rn, rb, psi, pfx)."""
import itertools
import math

import numpy as np
import torch

NINF = float("-inf")


def bound(T, M):
    return T * (2.0 ** -22 * M + 4e-7)


def log_add(a, b):
    if a == NINF:
        return b
    if b == NINF:
        return a
    hi, lo = (a, b) if a > b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


class Hyp:
    """State of a hypothesis: rn[t], rb[t] for t < T, pfx, the last label (None for empty g) and done."""

    def __init__(self, rn, rb, pfx, last, done=False, labels=()):
        self.rn, self.rb, self.pfx, self.last, self.done, self.labels = rn, rb, pfx, last, done, tuple(labels)
        self.children, self.psi = {}, None

    def magnitude(self):
        vals = [abs(v) for v in self.rn + self.rb + [self.pfx] + ([] if self.psi is None else self.psi.tolist()) if v != NINF]
        return max(vals) if vals else 0.0


def begin(x, T, blank):
    rb, acc = [], 0.0
    for t in range(T):
        acc = x[t][blank] if t == 0 else acc + x[t][blank]
        rb.append(float(acc))
    return Hyp([NINF] * T, rb, 0.0, None)


def extend(h, x, T, blank, c):
    """``(psi, Hyp)``: the prefix log-probability of g.c and its state; a sequence that contains the blank has probability zero."""
    if c == blank:
        return NINF, Hyp([NINF] * T, [NINF] * T, NINF, c, labels=h.labels + (c,))
    nn = [float(x[0][c]) if h.last is None else NINF]
    nb = [NINF]
    psi = nn[0]
    for t in range(1, T):
        phi = h.rb[t - 1] if c == h.last else log_add(h.rn[t - 1], h.rb[t - 1])
        nn.append(log_add(nn[t - 1], phi) + float(x[t][c]))
        nb.append(log_add(nn[t - 1], nb[t - 1]) + float(x[t][blank]))
        psi = log_add(psi, phi + float(x[t][c]))
    return psi, Hyp(nn, nb, psi, c, labels=h.labels + (c,))


def full(h, T):
    return log_add(h.rn[T - 1], h.rb[T - 1])


def child(h, x, T, blank, c):
    if c not in h.children:
        h.children[c] = extend(h, x, T, blank, c)
    return h.children[c]


def psi_all(h, x, T, blank):
    """psi(g.v) of ``extend`` for every v at once: the same recurrence, the frames in the same order, numpy over the vocabulary
    (psi does not depend on the candidate's own nn / nb).  tests/test_host_ctc_prefix.py holds it to ``extend``."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[1]
    psi = x[0].copy() if h.last is None else np.full(V, NINF)
    for t in range(1, T):
        phi = np.full(V, log_add(h.rn[t - 1], h.rb[t - 1]))
        if h.last is not None:
            phi[h.last] = h.rb[t - 1]
        psi = np.logaddexp(psi, phi + x[t])
    psi[blank] = NINF
    return psi


def local_scores(h, x, T, blank, att, w, one_w, eos, pad, step, min_length):
    """The joint local scores of one beam for every token: V floats."""
    V = len(att)
    out = np.full(V, NINF)
    if h.done:
        out[pad] = 0.0
        return out
    if h.pfx == NINF:
        return out
    if h.psi is None:
        h.psi = psi_all(h, x, T, blank)
    ctc = h.psi - h.pfx
    ctc[eos] = NINF if step < min_length else full(h, T) - h.pfx
    ctc[blank] = NINF
    with np.errstate(invalid="ignore"):
        val = one_w * np.asarray(att, dtype=np.float64) + w * ctc
    val[(ctc == NINF) | (val != val)] = NINF
    return val


def after_selection(p, x, T, blank, eos, v):
    if p.done:
        return Hyp(p.rn, p.rb, p.pfx, p.last, True, p.labels)
    if v == eos:
        return Hyp(p.rn, p.rb, full(p, T), p.last, True, p.labels)
    return child(p, x, T, blank, v)[1]


class PrefixStatement:
    """The statement behind ``CtcPrefixSession``: ``step(att [n][R][V], last [n][R], parent [n][R] | None) -> local`` (float64
    numpy [n, R, V]).  ``xs``: n emissions [T', V]; ``Ts``: their frames (None: T').  ``M[i]``: the largest finite magnitude in the
    state of search i so far."""

    def __init__(self, xs, Ts, weight, eos, pad, blank=0, min_length=0):
        self.xs = [np.asarray(x, dtype=np.float64) for x in xs]
        self.Ts = [min(max(int(T), 1), len(x)) for x, T in zip(self.xs, Ts or [len(x) for x in self.xs])]
        self.w = float(np.float32(weight))
        self.one_w = float(np.float32(1.0) - np.float32(weight))
        self.eos, self.pad, self.blank, self.min_length = eos, pad, blank, min_length
        self.hyps = [[begin(x, T, blank)] for x, T in zip(self.xs, self.Ts)]
        self.M = [h[0].magnitude() for h in self.hyps]
        self.s = 0

    def step(self, att, last, parent=None):
        n, R = len(self.xs), len(last[0])
        if self.s == 0:
            self.hyps = [[self.hyps[i][0]] * R for i in range(n)]
        else:
            self.hyps = [[after_selection(self.hyps[i][int(parent[i][r]) if parent is not None else r], self.xs[i], self.Ts[i], self.blank,
                                          self.eos, int(last[i][r])) for r in range(R)] for i in range(n)]
        local = np.empty((n, R, len(att[0][0])))
        for i in range(n):
            for r in range(R):
                h = self.hyps[i][r]
                local[i, r] = local_scores(h, self.xs[i], self.Ts[i], self.blank, att[i][r], self.w, self.one_w, self.eos, self.pad, self.s,
                                           self.min_length)
                self.M[i] = max(self.M[i], h.magnitude())
        self.s += 1
        return local


def length_penalty(length, alpha):
    return ((5 + length) / (5 + 1)) ** alpha


def select(local, scores, penalty, K):
    """eec_beam_select for one search: cand = scores[r] + local[r][v] / penalty (penalty as fp32), the K best, best first, ties to the
    lower r * V + v; when nothing above -inf is left, index 0 with -inf.  Returns (scores, parents, tokens, margin): margin is the
    smallest gap between neighbours among the K + 1 best candidates (a swap of either pair would change the result)."""
    pen = float(np.float32(penalty))
    R, V = local.shape
    cand = (np.asarray(scores, dtype=np.float64)[:, None] + local / pen).reshape(-1)
    order = np.argsort(-cand, kind="stable")[: K + 1]
    top = cand[order]
    margin = math.inf
    for a, b in zip(top[:-1], top[1:]):
        if a != NINF:
            margin = min(margin, a - b)
    out_s, out_p, out_t = [], [], []
    for k in range(K):
        idx = int(order[k]) if k < len(order) and top[k] != NINF else 0
        out_s.append(float(cand[order[k]]) if k < len(order) and top[k] != NINF else NINF)
        out_p.append(idx // V)
        out_t.append(idx % V)
    return out_s, out_p, out_t, margin


def joint_search(xs, Ts, step, n, weight, sos, eos, pad, beam, alpha, max_length, blank=0, min_length=0):
    """The statement's one-pass joint search of n searches in lockstep.  ``step(last [n][R], parent [n][R] | None)`` returns the
    attention log-probs [n][R][V] (anything indexable).  Returns per search ``dict(tokens [beam][max_length + 1], scores [beam],
    best (row), margin, M, T)``: margin is the smallest selection margin of the search, the final choice of the best beam included."""
    st = PrefixStatement(xs, Ts, weight, eos, pad, blank, min_length)
    scores = [[0.0] for _ in range(n)]
    rows = [[[sos]] for _ in range(n)]
    last, parent = [[sos] for _ in range(n)], None
    margins = [math.inf] * n
    for i in range(max_length):
        local = st.step(step(last, parent), last, parent)
        new_last, new_parent = [], []
        for k in range(n):
            s, p, t, m = select(local[k], scores[k], length_penalty(i + 1, alpha), beam)
            margins[k] = min(margins[k], m)
            rows[k] = [rows[k][pp] + [tt] for pp, tt in zip(p, t)]
            scores[k] = s
            new_last.append(t)
            new_parent.append(p)
        last, parent = new_last, new_parent
    out = []
    for k in range(n):
        clean = []
        for row in rows[k]:  # after EOS a row holds only PAD (rows of score -inf too)
            cut = row.index(eos) + 1 if eos in row else len(row)
            clean.append(row[:cut] + [pad] * (len(row) - cut))
        ranked = sorted(scores[k], reverse=True)
        if len(ranked) > 1 and ranked[0] != NINF:
            margins[k] = min(margins[k], ranked[0] - ranked[1])
        best = max(range(len(scores[k])), key=lambda b: (scores[k][b], -b))
        out.append(dict(tokens=clean, scores=scores[k], best=clean[best], margin=margins[k], M=st.M[k], T=st.Ts[k]))
    return out


# ---- brute force over all V^T paths -------------------------------------------------------------------------------------------

def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def brute_force(x, T, blank):
    """``(labelling, prefix, rn, rb)`` by enumeration: labelling[g] = P(collapse(path) == g), prefix[g] = P(collapse(path) starts
    with g) over all V^T paths; rn[(g, t)] / rb[(g, t)] = P(paths over frames 0..t that collapse to g and end in a non-blank / the
    blank).  Probabilities, float64."""
    V = len(x[0])
    p = np.exp(np.asarray(x, dtype=np.float64))
    labelling, prefix, rn, rb = {}, {}, {}, {}
    for t in range(T):
        for path in itertools.product(range(V), repeat=t + 1):
            pr = 1.0
            for f, c in enumerate(path):
                pr *= p[f][c]
            g = collapse(path, blank)
            into = rb if path[-1] == blank else rn
            into[(g, t)] = into.get((g, t), 0.0) + pr
            if t == T - 1:
                labelling[g] = labelling.get(g, 0.0) + pr
                for k in range(len(g) + 1):
                    prefix[g[:k]] = prefix.get(g[:k], 0.0) + pr
    return labelling, prefix, rn, rb


def log_or_ninf(p):
    return math.log(p) if p > 0 else NINF


# ---- scripted sequences of (parent, token) choices: a session under test against the statement -------------------------------------

# (parent, token) of every beam, step by step; sos = 7, eos = 1, pad = 2, blank = 0.  Step 1: three children of one parent, two of
# them alike.  Step 2: a repeated label (3, 3), EOS.  Step 3: the done beam moves from row 2 to row 0, another EOS.  Step 4: two done
# beams reordered again, a third label of a repeat.
SCRIPT = [([0, 0, 0], [3, 4, 3]),
          ([0, 0, 1, 2], [3, 5, 1, 4]),
          ([2, 0, 0, 1], [2, 3, 1, 6]),
          ([2, 0, 1], [2, 2, 3])]


def scripted(make, xs, em_len, V, w, eos, pad, blank, min_length, script=SCRIPT, seed=3):
    """The local scores of every step of ``script`` from the session ``make`` builds and from the statement, with the statement's
    per-search bound: [(got [n, R, V] float64 numpy, want, bounds [n])]."""
    n = len(xs)
    sess = make()
    st = PrefixStatement([x.double().numpy() for x in xs], em_len, w, eos, pad, blank, min_length)
    g = torch.Generator().manual_seed(seed)
    out = []
    last, parent = torch.full((n, 1), 7, dtype=torch.long), None
    for s in range(len(script) + 1):
        R = last.size(1)
        att = torch.log_softmax(torch.randn(n, R, V, generator=g) * 2.0, -1)
        dev = sess.dev
        got = sess.step(att.to(dev), last.to(dev), None if parent is None else parent.to(dev)).double().cpu().numpy()
        want = st.step(att.double().numpy(), last.tolist(), None if parent is None else parent.tolist())
        out.append((got, want, [bound(T, M) for T, M in zip(st.Ts, st.M)]))
        if s < len(script):
            parent = torch.tensor([script[s][0]] * n)
            last = torch.tensor([script[s][1]] * n)
    return out


def assert_within_bound(results):
    worst = 0.0
    for s, (got, want, bounds) in enumerate(results):
        assert not np.isnan(got).any(), s
        assert ((got == NINF) == (want == NINF)).all(), f"step {s}: -inf in other cells"
        assert not np.isposinf(got).any()
        for i, b in enumerate(bounds):
            fin = want[i] != NINF
            err = np.abs(got[i][fin] - want[i][fin]).max() if fin.any() else 0.0
            worst = max(worst, err / b)
            assert err <= b, f"step {s} search {i}: error {err:.3g} over the bound {b:.3g}"
    return worst


def make_script(R_seq, labels, eos, pad, seed, p_eos=0.2):
    """A pseudo-random script with ``R_seq[k]`` beams at step k + 1: parents drawn from the previous step's rows (several children of
    one parent, rows reordered), tokens from the few ``labels`` (so labels repeat) or EOS; a child of a done beam takes PAD."""
    rng = np.random.RandomState(seed)
    done, script = [False], []
    for R in R_seq:
        parents = rng.randint(0, len(done), R).tolist()
        tokens = [pad if done[p] else (eos if rng.rand() < p_eos else int(rng.choice(labels))) for p in parents]
        done = [done[p] or t == eos for p, t in zip(parents, tokens)]
        script.append((parents, tokens))
    return script
