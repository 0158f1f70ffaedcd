"""CTC segmentation (include/eec.h, "CTC segmentation: long rows, free ends"): the statement with its two flags in plain scalar
loops on fp32 values, a brute force over all frame labellings it is checked against, and the seeded cases the host and the GPU tests
share.  Nothing here is shared with the product code."""
import functools

import numpy as np
import torch

import forced_align_cases as fc

NEG = float("-inf")
FREE_START, FREE_END = 1, 2
ALL_FLAGS = (0, FREE_START, FREE_END, FREE_START | FREE_END)
FIELDS = fc.FIELDS


def _f32(v):
    """One fp32 rounding.  The sum of two fp32 values is exact in fp64 or rounds there harmlessly (53 >= 2 * 24 + 2 bits), so
    ``_f32(a + b)`` on Python floats that hold fp32 values is the fp32 add."""
    return float(np.float32(v))


def restate(x, T, y, blank, flags=0):
    """``fc.restate`` with the flags: the emission term of state 0 is 0.0 under FREE_START, that of state 2N is 0.0 for t >= 1 under
    FREE_END.  ``x`` [T', V] float32.  Returns ``(status, path_score, state)``."""
    Tq, V = x.shape
    T = min(max(int(T), 0), Tq)
    N = len(y)
    if N == 0 or any(t < 0 or t >= V or t == blank for t in y) or T < N + fc.adjacent_equal(y):
        return 1, NEG, None
    S = 2 * N + 1
    lab = [blank if s % 2 == 0 else y[(s - 1) // 2] for s in range(S)]
    skip = [s % 2 == 1 and s >= 3 and y[(s - 1) // 2] != y[(s - 3) // 2] for s in range(S)]
    rows = x[:T].tolist()
    a = [NEG] * S
    a[0], a[1] = (0.0 if flags & FREE_START else rows[0][blank]), rows[0][y[0]]
    dec = [None] * T
    for t in range(1, T):
        row = rows[t]
        na, d = [NEG] * S, [0] * S
        for s in range(S):
            best = a[s]
            if s >= 1 and a[s - 1] > best:
                best, d[s] = a[s - 1], 1
            if skip[s] and a[s - 2] > best:
                best, d[s] = a[s - 2], 2
            e = row[lab[s]]
            if (s == 0 and flags & FREE_START) or (s == 2 * N and flags & FREE_END):
                e = 0.0
            na[s] = _f32(best + e)
        a, dec[t] = na, d
    s = 2 * N if a[2 * N] > a[2 * N - 1] else 2 * N - 1
    score = a[s]
    state = [0] * T
    for t in range(T - 1, 0, -1):
        state[t] = s
        s -= dec[t][s]
        assert 0 <= s <= 2 * N
    state[0] = s
    if not (score > NEG) or s > 1:  # the first test is False for a NaN
        return 1, NEG, None
    return 0, score, state


def outputs(x, T, y, blank, flags=0, S=None):
    """The statement's outputs for one row as tensors: ``(tok_start [S], tok_end [S], tok_score [S], frame_token [T'], path_score,
    status)``; ``S`` defaults to the row's length."""
    Tq = x.shape[0]
    S = max(1, len(y)) if S is None else S
    T = min(max(int(T), 0), Tq)
    status, score, state = restate(x, T, y, blank, flags) if len(y) <= S else (1, NEG, None)
    ts, te, sc = [-1] * S, [-1] * S, [NEG] * S
    ft = [-2] * Tq
    if status == 0:
        rows = x[:T].tolist()
        for t in range(T):
            s = state[t]
            ft[t] = s // 2 if s % 2 else -1
            if s % 2:
                j, v = s // 2, rows[t][y[s // 2]]
                if ts[j] < 0:
                    ts[j], sc[j] = t, v
                else:
                    sc[j] = _f32(sc[j] + v)
                te[j] = t + 1
    return (torch.tensor(ts, dtype=torch.int32), torch.tensor(te, dtype=torch.int32), torch.tensor(sc, dtype=torch.float32),
            torch.tensor(ft, dtype=torch.int32), torch.tensor(score, dtype=torch.float32), torch.tensor(status, dtype=torch.int32))


# ---- the brute force: every labelling that collapses to the labels, the free frames costing nothing -----------------------------------
def brute_best(x, T, y, blank, flags):
    """Best score in fp64 over the labellings of T frames that CTC-collapse to ``y`` (None: there is none).  Under FREE_START the
    blank frames before the first label frame are free, under FREE_END the blank frames after the last label frame."""
    best = None
    for p in fc.labellings(x.shape[1], T, tuple(y), blank):
        first = next(t for t in range(T) if p[t] != blank)
        last = max(t for t in range(T) if p[t] != blank)
        s = 0.0
        for t in range(T):
            if (flags & FREE_START and t < first) or (flags & FREE_END and t > last):
                continue
            s += float(x[t, p[t]])
        if best is None or s > best:
            best = s
    return best


def brute_trials(n_trials=300, seed=11):
    """(x, T, y, blank, flags): V <= 4, T <= 7, N <= 3, repeated labels included, the four flag settings in turn; x dyadic, so that
    every fp32 sum is exact and the restatement differs from the fp64 brute force in nothing but the order of its additions."""
    rng = np.random.default_rng(seed)
    for i in range(n_trials):
        V = int(rng.integers(2, 5))
        T = int(rng.integers(1, 8 if V <= 3 else 7))
        y = [int(t) for t in rng.integers(1, V, size=int(rng.integers(1, 4)))]
        x = (-rng.integers(0, 9, size=(T, V)) / (4 if i % 3 else 2)).astype(np.float32)  # coarser values: more ties
        yield x, T, y, 0, ALL_FLAGS[i % 4]


# ---- seeded rows and emissions ---------------------------------------------------------------------------------------------------------
def random_row(rng, n, V, blank=0, repeats=True):
    """``n`` labels of [0, V) without the blank; with ``repeats`` adjacent equal pairs occur by chance, else never."""
    row = []
    while len(row) < n:
        t = int(rng.integers(0, V))
        if t != blank and (repeats or not row or t != row[-1]):
            row.append(t)
    return row


def emission(rng, n_em, Tq, V, scale):
    """log_softmax of normal noise times ``scale`` (1: flat; 8: peaky, so that ties and -inf-free extremes occur) [n_em, T', V]."""
    return torch.log_softmax(torch.from_numpy(rng.standard_normal((n_em, Tq, V)).astype(np.float32)) * float(scale), dim=-1)


def pad_rows(rows, S=None):
    """``(tokens [H, S] int32 zero-padded, tok_len [H] int32)``."""
    S = max(1, max(len(r) for r in rows)) if S is None else S
    tokens = torch.zeros((len(rows), S), dtype=torch.int32)
    for h, r in enumerate(rows):
        tokens[h, :min(len(r), S)] = torch.tensor(r[:S], dtype=torch.int32)
    return tokens, torch.tensor([len(r) for r in rows], dtype=torch.int32)


HOST_N = (1, 5, 31, 64, 255, 256, 257, 300)


@functools.lru_cache(maxsize=None)
def host_case(N, flags):
    """``(x [n_em, T', V], em_len [n_em], row)``: one row of N labels (chance repeats: R adjacent equal pairs) against emissions of
    N + R, 37, 70 and 330 frames where the row fits them, each in a table of T' = its length + 3 frames with NaN from the length
    on."""
    rng = np.random.default_rng(100 * N + flags)
    V = 5 if N % 2 else 11
    row = random_row(rng, N, V)
    need = N + fc.adjacent_equal(row)
    lens = sorted({need} | {T for T in (37, 70, 330) if T >= need})
    Tq = max(lens) + 3
    x = emission(rng, len(lens), Tq, V, 8 if N % 3 else 1)
    for n, T in enumerate(lens):
        x[n, T:] = float("nan")
    return x, torch.tensor(lens, dtype=torch.int32), tuple(row)


TIGHT = (1, 1, 2, 3, 4)  # N = 5, R = 1: needs 6 frames


@functools.lru_cache(maxsize=None)
def length_case(flags):
    """The tight row against lengths 0, 1, N + R - 1, N + R and T', with NaN from every length on."""
    rng = np.random.default_rng(900 + flags)
    need = len(TIGHT) + fc.adjacent_equal(TIGHT)
    lens = [0, 1, need - 1, need, 12]
    x = emission(rng, len(lens), 12, 6, 8)
    for n, T in enumerate(lens):
        x[n, T:] = float("nan")
    return x, torch.tensor(lens, dtype=torch.int32)


def same(a, b, what=""):
    for name in FIELDS:
        assert fc.same_bits(getattr(a, name), getattr(b, name)), (what, name)


def is_fill(al, h):
    return (int(al.status[h]) == 1 and float(al.path_score[h]) == NEG and bool((al.frame_token[h] == -2).all())
            and bool((al.tok_start[h] == -1).all()) and bool((al.tok_end[h] == -1).all()) and bool((al.tok_score[h] == NEG).all()))
