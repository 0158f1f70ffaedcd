"""CTC forced alignment in the standard topology (include/eec.h): the statement in plain scalar loops on ``numpy.float32`` values, a
brute force over all frame labellings it is checked against, and the cases the host and the GPU tests share.  Nothing here is
shared with the product code."""
import functools
import itertools

import numpy as np
import torch

F = np.float32
NEG = F("-inf")
S_MAX = 255  # the width of every case's token table


def adjacent_equal(y):
    return sum(1 for a, b in zip(y, y[1:]) if a == b)


def restate(x, T, y, blank):
    """``x``: [T', V] float32 array, ``T`` its frame count (clamped here), ``y`` the labels.  Returns
    ``(status, path_score, state)``: ``state`` the T states of the path (None with status 1)."""
    Tq, V = x.shape
    T = min(max(int(T), 0), Tq)
    N = len(y)
    if N == 0 or any(t < 0 or t >= V or t == blank for t in y) or T < N + adjacent_equal(y):
        return 1, NEG, None
    S = 2 * N + 1
    lab = [blank if s % 2 == 0 else y[(s - 1) // 2] for s in range(S)]
    skip = [s % 2 == 1 and s >= 3 and y[(s - 1) // 2] != y[(s - 3) // 2] for s in range(S)]
    a = [NEG] * S
    a[0], a[1] = x[0, blank], x[0, y[0]]
    dec = [None] * T
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            row = x[t]
            na, d = [NEG] * S, [0] * S
            for s in range(S):
                best = a[s]
                if s >= 1 and a[s - 1] > best:
                    best, d[s] = a[s - 1], 1
                if skip[s] and a[s - 2] > best:
                    best, d[s] = a[s - 2], 2
                na[s] = F(best + row[lab[s]])
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
    return 0, F(score), state


def outputs(x, T, y, blank, S=S_MAX):
    """The statement's outputs for one row: ``(tok_start [S], tok_end [S], tok_score [S], frame_token [T'], path_score, status)``."""
    Tq = x.shape[0]
    T = min(max(int(T), 0), Tq)
    status, score, state = restate(x, T, y, blank)
    ts, te, sc = [-1] * S, [-1] * S, [NEG] * S
    ft = [-2] * Tq
    if status == 0:
        for t in range(T):
            s = state[t]
            ft[t] = s // 2 if s % 2 else -1
            if s % 2:
                j, v = s // 2, x[t, y[s // 2]]
                if ts[j] < 0:
                    ts[j], sc[j] = t, v
                else:
                    sc[j] = F(sc[j] + v)
                te[j] = t + 1
    return ts, te, sc, ft, score, status


# ---- the brute force: every labelling of the frames that CTC-collapses to the labels --------------------------------------------------
def collapse(path, blank):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return tuple(out)


@functools.lru_cache(maxsize=None)
def labellings(V, T, y, blank):
    return [p for p in itertools.product(range(V), repeat=T) if collapse(p, blank) == y]


def brute_best(x, T, y, blank):
    """(best score in fp64, or None if no labelling collapses to ``y``)."""
    best = None
    for p in labellings(x.shape[1], T, tuple(y), blank):
        s = sum(float(x[t, p[t]]) for t in range(T))
        if best is None or s > best:
            best = s
    return best


def brute_trials(n_trials=300, seed=0):
    """(x, T, y, blank): V = 3, T <= 6, N <= 3, repeated labels included; x dyadic (multiples of 1/4 or 1/2), so that every fp32
    sum is exact and the fp32 restatement differs from the fp64 brute force in nothing but the order of its additions."""
    rng = np.random.default_rng(seed)
    fixed = [(1, [1]), (2, [1, 1]), (3, [1, 1]), (4, [1, 1, 2]), (5, [2, 2, 2]), (6, [1, 2, 1]), (2, [1, 2, 1])]
    for i in range(n_trials):
        if i < len(fixed):
            T, y = fixed[i]
        else:
            T = int(rng.integers(1, 7))
            y = [int(t) for t in rng.integers(1, 3, size=int(rng.integers(1, 4)))]
        x = (-rng.integers(0, 9, size=(T, 3)) / (4 if i % 3 else 2)).astype(np.float32)  # coarser values: more ties
        yield x, T, y, 0


# ---- the cases of the GPU test (the host path runs them too) --------------------------------------------------------------------------
ROW_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 255)  # every boundary of the 1 / 2 / 4 / 8 states per lane
N_EM = 6
TIGHT = (1, 1, 2, 3, 4)  # N = 5, R = 1: needs 6 frames (every case has the labels 1 .. 4)


def _no_repeat(rng, n, V, blank):
    row = []
    while len(row) < n:
        t = int(rng.integers(0, V))
        if t != blank and (not row or t != row[-1]):
            row.append(t)
    return row


@functools.lru_cache(maxsize=None)
def gpu_case(Tq, V, scale, blank=0):
    """``(x [6, T', V] fp32, em_len [6] int32, rows, tok_len, em_index)``: log_softmax of normal noise times ``scale`` (1: flat,
    8: peaky, so that ties occur), lengths 0, 1, 5 (the tight row's N + R - 1), 6 (N + R), T', T' and NaN from every length on.
    ``rows``: lists of ids; ``tok_len`` is the row's length unless the row tests a length; several rows share emissions 4 and 5."""
    rng = np.random.default_rng(7000 * Tq + 10 * V + scale)
    x = torch.log_softmax(torch.from_numpy(rng.standard_normal((N_EM, Tq, V)).astype(np.float32)) * float(scale), dim=-1)
    need = len(TIGHT) + adjacent_equal(TIGHT)
    em_len = torch.tensor([0, 1, need - 1, need, Tq, Tq], dtype=torch.int32)
    for n in range(N_EM):
        x[n, int(em_len[n]):] = float("nan")
    rows, tok_len, em_index = [], [], []

    def add(row, em, n=None):
        rows.append([int(t) for t in row]), tok_len.append(len(row) if n is None else n), em_index.append(em)

    for i, n in enumerate(ROW_LENGTHS):  # rows longer than T' are not alignable; the others cross every strip width
        add(_no_repeat(rng, n, V, blank), 4 + i % 2)
    for em in range(5):  # lengths 0 and 1 and N + R - 1: status 1; N + R: the one tight alignment; T'
        add(TIGHT, em)
    add([2], 1)                                   # one token, one frame
    add([3] * ((Tq + 1) // 2), 4)                 # all equal: needs exactly 2N - 1 = T' (or T' - 1) frames
    add([3] * ((Tq + 1) // 2 + 1), 4)             # ... and one token too many
    add([int(t) for t in rng.integers(1, min(V, 4), size=12)], 5)  # chance repeats
    add([1, 2, V, 3], 4)                          # a token >= V
    add([1, 2, 1 << 20, 3], 4)
    add([1, blank, 2], 4)                         # a blank inside
    add([1, 2, 3], 4, n=0)                        # N = 0
    add([1, 2, 3], 4, n=S_MAX + 1)                # N > tok_stride
    add([1, 2, 3], N_EM)                          # em_index outside the emissions
    add([1, 2, 3], -1)
    add([1, 2, 3, 1], 5)                          # a good row behind the bad ones
    return x, em_len, tuple(tuple(r) for r in rows), tuple(tok_len), tuple(em_index)


def case_tensors(Tq, V, scale):
    """``(tokens [H, 255] int32, tok_len [H] int32, em_index [H] int32)`` of ``gpu_case``."""
    _, _, rows, tok_len, em_index = gpu_case(Tq, V, scale)
    tokens = torch.zeros((len(rows), S_MAX), dtype=torch.int32)
    for h, r in enumerate(rows):
        tokens[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return tokens, torch.tensor(tok_len, dtype=torch.int32), torch.tensor(em_index, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def gpu_case_expected(Tq, V, scale, blank=0):
    """The restatement of ``gpu_case`` as tensors, in the order of ``FIELDS``."""
    x, em_len, rows, tok_len, em_index = gpu_case(Tq, V, scale, blank)
    xs = x.numpy()
    H = len(rows)
    ts = torch.empty((H, S_MAX), dtype=torch.int32)
    te = torch.empty((H, S_MAX), dtype=torch.int32)
    sc = torch.empty((H, S_MAX), dtype=torch.float32)
    ft = torch.empty((H, Tq), dtype=torch.int32)
    ps = torch.empty((H,), dtype=torch.float32)
    st = torch.empty((H,), dtype=torch.int32)
    for h in range(H):
        em, n = em_index[h], tok_len[h]
        if 0 <= em < N_EM and 0 <= n <= S_MAX:
            out = outputs(xs[em], int(em_len[em]), list(rows[h][:n]), blank)
        else:  # a bad row: the fill values
            out = ([-1] * S_MAX, [-1] * S_MAX, [NEG] * S_MAX, [-2] * Tq, NEG, 1)
        ts[h], te[h] = torch.tensor(out[0], dtype=torch.int32), torch.tensor(out[1], dtype=torch.int32)
        sc[h] = torch.from_numpy(np.asarray(out[2], dtype=np.float32))
        ft[h] = torch.tensor(out[3], dtype=torch.int32)
        ps[h], st[h] = float(out[4]), out[5]
    return ts, te, sc, ft, ps, st


FIELDS = ("tok_start", "tok_end", "tok_score", "frame_token", "path_score", "status")
GPU_CASES = [(Tq, V, scale) for Tq in (37, 70, 300) for V in (5, 32, 37, 256) for scale in (1, 8)]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns: -inf equals -inf, and a NaN would have to be the same NaN."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
