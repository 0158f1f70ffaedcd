"""Keyword spotting on CTC emissions (include/eec.h): the statement in plain scalar loops, a brute force it is checked against,
and the cases the host and the GPU tests share.  Nothing here is shared with the product code.

fp32 in Python floats: every value below is a float that fp32 holds exactly, and ``fl`` rounds the double result of one subtraction
or addition of two such values to fp32.  A sum or difference of two fp32 numbers rounded to fp64 and then to fp32 is the fp32 result
(53 >= 2 * 24 + 2 bits: the double rounding is innocuous), so this is the kernel's arithmetic."""
import functools
import itertools
import math

import numpy as np
import torch

NEG = float("-inf")


def fl(v: float) -> float:
    return float(np.float32(v))


def restate(x, T, y, blank):
    """``x``: T' rows of V floats (lists), ``T`` its frame count (clamped here), ``y`` the keyword.  Returns
    ``(score, start, end, trace_score [T'], trace_start [T'])``."""
    Tq = len(x)
    T = min(max(int(T), 0), Tq)
    L = len(y)
    S = 2 * L - 1
    lab = [y[s // 2] if s % 2 == 0 else blank for s in range(S)]
    d, st = [NEG] * S, [-1] * S
    trace_score, trace_start = [NEG] * Tq, [-1] * Tq
    for t in range(T):
        row = x[t]
        m = row[0]
        for v in row[1:]:
            if v > m:
                m = v
        finite = math.isfinite(m)
        nd, ns = [NEG] * S, [-1] * S
        for s in range(S):
            c, cs = d[s], st[s]
            if s >= 1 and d[s - 1] > c:
                c, cs = d[s - 1], st[s - 1]
            if s >= 2 and s % 2 == 0 and lab[s] != lab[s - 2] and d[s - 2] > c:
                c, cs = d[s - 2], st[s - 2]
            if s == 0 and 0.0 > c:
                c, cs = 0.0, t
            e = fl(row[lab[s]] - m) if finite else NEG
            v = fl(c + e)
            nd[s], ns[s] = v, (cs if v != NEG else -1)
        d, st = nd, ns
        trace_score[t], trace_start[t] = d[S - 1], st[S - 1]
    score, start, end = NEG, -1, -1
    for t in range(T):
        if trace_score[t] > score:
            score, start, end = trace_score[t], trace_start[t], t
    return score, start, end, trace_score, trace_start


# ---- the brute force: every segment, every label path that CTC-collapses to the keyword ------------------------------------------
def collapse(path, blank):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return tuple(out)


@functools.lru_cache(maxsize=None)
def matching_paths(V, n, y, blank):
    """The label paths of n frames over V symbols that collapse to ``y``, begin with y_1 and end with y_L."""
    return [p for p in itertools.product(range(V), repeat=n) if p[0] == y[0] and p[-1] == y[-1] and collapse(p, blank) == y]


def brute_segments(x, T, y, blank):
    """seg[a][b]: the best score of a path over frames a .. b (-inf: none).  Exact for dyadic ``x``: sums in any order agree."""
    V = len(x[0])
    e = []
    for t in range(T):
        m = max(x[t])
        e.append([v - m if math.isfinite(m) else NEG for v in x[t]])
    seg = [[NEG] * T for _ in range(T)]
    for a in range(T):
        for b in range(a, T):
            for p in matching_paths(V, b - a + 1, tuple(y), blank):
                s = sum(e[a + i][p[i]] for i in range(len(p)))
                if s > seg[a][b]:
                    seg[a][b] = s
    return seg


def brute_trials(n_trials=300, seed=0):
    """(x, T, y, blank) with dyadic x (multiples of 1/4), V 3 .. 4, T <= 6, L <= 3; repeated tokens included, [1, 1] on short
    emissions first."""
    rng = np.random.default_rng(seed)
    fixed = [(2, [1, 1]), (3, [1, 1]), (1, [1]), (4, [1, 1, 2]), (5, [2, 2, 2]), (6, [1, 2, 1])]
    for i in range(n_trials):
        V = int(rng.integers(3, 5))
        if i < len(fixed):
            T, y = fixed[i]
        else:
            T = int(rng.integers(1, 7))
            y = [int(t) for t in rng.integers(1, V, size=int(rng.integers(1, 4)))]
        steps = 4 if i % 3 else 2  # coarser values: more ties
        x = (-rng.integers(0, 9, size=(T, V)) / steps).astype(np.float32)
        yield x.tolist(), T, y, 0


# ---- the cases of the GPU test (the host path runs them too) ----------------------------------------------------------------------
N_EM = 5
KEYWORD_LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64)  # lane boundaries and the switch from one state per lane to two
PLANT_FRAMES = (5, 13)  # the planted phrase occupies frames 5 .. 12 of the emissions that are long enough


def _no_repeat(rng, L, V, blank):
    row = []
    while len(row) < L:
        t = int(rng.integers(0, V))
        if t != blank and (not row or t != row[-1]):
            row.append(t)
    return row


def adjacent_equal(y):
    return sum(1 for a, b in zip(y, y[1:]) if a == b)


@functools.lru_cache(maxsize=None)
def gpu_case(Tq, V, scale, blank=0):
    """``(x [5, T', V] fp32, em_len [5] int32, phrases (13 rows), planted keyword index)``: log_softmax of normal noise times
    ``scale`` (8: peaky, so that frame terms of exactly 0 and ties occur), lengths 0, 1, 2, 36, T', NaN from every length on."""
    rng = np.random.default_rng(1000 * Tq + 10 * V + scale)
    phrases = [_no_repeat(rng, L, V, blank) for L in KEYWORD_LENGTHS]
    a, b = _no_repeat(rng, 2, V, blank)
    phrases.append([a, a, b])            # adjacent equal tokens: a blank frame has to part them
    phrases.append([a] * 64)             # needs 127 frames: longer than every emission
    planted = _no_repeat(rng, 3, V, blank)
    phrases.append(planted)              # the planted path
    phrases.append(_no_repeat(rng, 5, V, blank))
    phrases.append(_no_repeat(rng, 17, V, blank))
    assert len(phrases) == 13
    noise = torch.from_numpy(rng.standard_normal((N_EM, Tq, V)).astype(np.float32)) * float(scale)
    runs = [planted[0]] * 2 + [planted[1]] * 3 + [blank] + [planted[2]] * 2  # frames 5 .. 12, run lengths above 1
    for n in (3, 4):
        noise[n, PLANT_FRAMES[0] - 1, blank] += 100.0  # the frames around the phrase are blank, so the planted segment is the only 0
        noise[n, PLANT_FRAMES[1], blank] += 100.0
        for i, tok in enumerate(runs):
            noise[n, PLANT_FRAMES[0] + i, tok] += 100.0
    x = torch.log_softmax(noise, dim=-1)
    em_len = torch.tensor([0, 1, 2, 36, Tq], dtype=torch.int32)
    for n in range(N_EM):
        x[n, int(em_len[n]):] = float("nan")
    return x, em_len, tuple(tuple(p) for p in phrases), 10


@functools.lru_cache(maxsize=None)
def gpu_case_expected(Tq, V, scale, blank=0):
    """The restatement of ``gpu_case`` as tensors: score [5, 13] fp32, start, end int32, trace_score [5, 13, T'], trace_start."""
    x, em_len, phrases, _ = gpu_case(Tq, V, scale, blank)
    rows = x.tolist()
    K = len(phrases)
    score = torch.empty((N_EM, K), dtype=torch.float32)
    start = torch.empty((N_EM, K), dtype=torch.int32)
    end = torch.empty((N_EM, K), dtype=torch.int32)
    t_score = torch.empty((N_EM, K, Tq), dtype=torch.float32)
    t_start = torch.empty((N_EM, K, Tq), dtype=torch.int32)
    for n in range(N_EM):
        for k, y in enumerate(phrases):
            sc, s, e, ts, tb = restate(rows[n], int(em_len[n]), list(y), blank)
            score[n, k], start[n, k], end[n, k] = sc, s, e
            t_score[n, k] = torch.tensor(ts, dtype=torch.float32)
            t_start[n, k] = torch.tensor(tb, dtype=torch.int32)
    return score, start, end, t_score, t_start


GPU_CASES = [(Tq, V, scale) for Tq in (37, 70) for V in (5, 32, 37, 256) for scale in (1, 8)]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns: -inf equals -inf, and a NaN would have to be the same NaN."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
