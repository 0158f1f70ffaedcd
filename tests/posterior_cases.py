"""CTC posteriors in the standard topology (include/eec.h): the statement in fp64, one row at a time, a brute force over all frame
labellings it is checked against, and the expected values and error bounds the host and the GPU tests share.  Nothing here is
shared with the product code; the cases are those of tests/forced_align_cases.py (its generator is imported, not edited)."""
import functools
import math

import numpy as np
import torch

import forced_align_cases as fc
from ctc_prefix_cases import bound

NEG = -np.inf
S_MAX = fc.S_MAX
TOKEN_FIELDS = ("tok_frames", "tok_score", "tok_start", "tok_end", "tok_start_var", "tok_end_var")
# T' 37 and 70 with V 5, 37, 256; one T' = 300, V = 32 for the long rows (127, 128, 255 tokens); flat and peaky
GPU_CASES = [(Tq, V, scale) for Tq in (37, 70) for V in (5, 37, 256) for scale in (1, 8)] + [(300, 32, 1), (300, 32, 8)]


def restate(x, T, y, blank):
    """``x``: [T', V] array, ``T`` its frame count (clamped here), ``y`` the labels.  Returns None for a row that fails the row
    checks (status 1), else a dict: ``ll``; ``alpha``, ``beta`` [T, 2N + 1]; ``gamma`` [T, 2N + 1] (all states); ``first``, ``last``
    [T, N] the first- and last-frame posteriors of the tokens; ``M`` the largest finite magnitude in alpha and beta."""
    Tq, V = x.shape
    T = min(max(int(T), 0), Tq)
    N = len(y)
    if N == 0 or any(t < 0 or t >= V or t == blank for t in y) or T < N + fc.adjacent_equal(y):
        return None
    NS = 2 * N + 1
    x = np.asarray(x[:T], dtype=np.float64)
    lab = np.array([blank if s % 2 == 0 else y[s // 2] for s in range(NS)])
    skip = np.array([s % 2 == 1 and s >= 3 and y[s // 2] != y[s // 2 - 1] for s in range(NS)])
    give = np.concatenate([skip[2:], [False, False]])  # skip(s + 2)
    e = x[:, lab]  # e[t][s] = x_t(lab(s))

    def left(v, n):
        return np.concatenate([np.full(n, NEG), v[:-n]])

    def right(v, n):
        return np.concatenate([v[n:], np.full(n, NEG)])

    alpha, beta = np.full((T, NS), NEG), np.full((T, NS), NEG)
    first, last = np.zeros((T, NS)), np.zeros((T, NS))
    alpha[0, 0], alpha[0, 1] = e[0, 0], e[0, 1]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a = alpha[t - 1]
            alpha[t] = np.logaddexp(np.logaddexp(a, left(a, 1)), np.where(skip, left(a, 2), NEG)) + e[t]
        beta[T - 1, 2 * N] = beta[T - 1, 2 * N - 1] = 0.0
        leave = np.full((T, NS), NEG)
        for t in range(T - 2, -1, -1):
            c = e[t + 1] + beta[t + 1]
            two = np.where(give, right(c, 2), NEG)
            beta[t] = np.logaddexp(np.logaddexp(c, right(c, 1)), two)
            leave[t] = np.logaddexp(right(c, 1), two)
        ll = np.logaddexp(alpha[T - 1, 2 * N], alpha[T - 1, 2 * N - 1])
        gamma = np.exp(alpha + beta - ll)
        first[0, 1] = gamma[0, 1]
        for t in range(1, T):
            a = alpha[t - 1]
            first[t] = np.exp(np.logaddexp(left(a, 1), np.where(skip, left(a, 2), NEG)) + e[t] + beta[t] - ll)
        last[:T - 1] = np.exp(alpha[:T - 1] + leave[:T - 1] - ll)
        last[T - 1] = gamma[T - 1]
    both = np.concatenate([alpha.ravel(), beta.ravel()])
    M = float(np.abs(both[np.isfinite(both)]).max())
    return dict(ll=float(ll), alpha=alpha, beta=beta, gamma=gamma, first=first[:, 1::2], last=last[:, 1::2], M=M, e=e[:, 1::2], T=T, N=N)


def token_sums(r):
    """The per-token sums of a restated row, fp64: ``{name: [N]}`` for TOKEN_FIELDS plus the moments (``m1s``, ``m2s``, ``m1e``,
    ``m2e``), the first- and last-frame masses and ``abs_score`` = sum_t gamma |x|."""
    T = r["T"]
    g = r["gamma"][:, 1::2]
    t0, t1 = np.arange(T, dtype=np.float64)[:, None], np.arange(1, T + 1, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        gx = np.where(g > 0.0, g * r["e"], 0.0)
    out = dict(tok_frames=g.sum(0), tok_score=gx.sum(0), abs_score=np.abs(gx).sum(0), m1s=(t0 * r["first"]).sum(0),
               m2s=(t0 * t0 * r["first"]).sum(0), m1e=(t1 * r["last"]).sum(0), m2e=(t1 * t1 * r["last"]).sum(0),
               first_mass=r["first"].sum(0), last_mass=r["last"].sum(0))
    out["tok_start"], out["tok_end"] = out["m1s"], out["m1e"]
    out["tok_start_var"] = out["m2s"] - out["m1s"] ** 2
    out["tok_end_var"] = out["m2e"] - out["m1e"] ** 2
    return out


# ---- the brute force: every labelling of the frames that CTC-collapses to the labels --------------------------------------------------
def brute(x, T, y, blank):
    """By enumeration, fp64: ``(ll, occupancy [T, N], first [T, N], last [T, N], blank share [T])``, or None if no labelling collapses
    to ``y``.  A labelling's frames belong to token j from the j-th time a non-blank label begins."""
    paths = fc.labellings(x.shape[1], T, tuple(y), blank)
    if not paths:
        return None
    N = len(y)
    occ, first, last, share = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N)), np.zeros(T)
    total = 0.0
    for p in paths:
        w = math.exp(sum(float(x[t, p[t]]) for t in range(T)))
        total += w
        j, prev, owner = -1, None, []
        for t in range(T):
            if p[t] != blank and p[t] != prev:
                j += 1
            owner.append(j if p[t] != blank else -1)
            prev = p[t]
        for t in range(T):
            if owner[t] < 0:
                share[t] += w
                continue
            occ[t, owner[t]] += w
            if t == 0 or owner[t - 1] != owner[t]:
                first[t, owner[t]] += w
            if t == T - 1 or owner[t + 1] != owner[t]:
                last[t, owner[t]] += w
    return math.log(total), occ / total, first / total, last / total, share / total


# ---- what the GPU test expects (the host tests run the host path over it too) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(Tq, V, scale, blank=0):
    """Per row of ``fc.gpu_case(Tq, V, scale)``: None (status 1) or ``(restated row, its token sums)``."""
    x, em_len, rows, tok_len, em_index = fc.gpu_case(Tq, V, scale, blank)
    xs = x.numpy()
    out = []
    for h in range(len(rows)):
        em, n = em_index[h], tok_len[h]
        r = restate(xs[em], int(em_len[em]), list(rows[h][:n]), blank) if 0 <= em < fc.N_EM and 0 <= n <= S_MAX else None
        out.append(None if r is None else (r, token_sums(r)))
    return out


def tolerances(r, sums):
    """The derived bounds of one status-0 row: ``(bound on ll, e, {field: [N] absolute tolerance})``.  bound(T, M) is the error of a
    log_add lattice (tests/ctc_prefix_cases.py); alpha, beta and ll each carry one, so a posterior's exponent is off by at most
    delta = 3 bound and the posterior by the factor e = expm1(delta) + 2^-22 (the fp32 exponential and the adds in front of it).
    A sum of posteriors is held to e times the fp64 sum of its absolute terms plus one fp32 rounding of the result (2^-24 of it;
    2^-126 where it is below the normal range)."""
    b = bound(r["T"], r["M"])
    e = math.expm1(3.0 * b) + 2.0 ** -22
    one = lambda v: 2.0 ** -24 * np.abs(v) + 2.0 ** -126  # noqa: E731
    tol = dict(tok_frames=e * sums["tok_frames"] + one(sums["tok_frames"]), tok_score=e * sums["abs_score"] + one(sums["tok_score"]),
               tok_start=e * sums["m1s"] + one(sums["m1s"]), tok_end=e * sums["m1e"] + one(sums["m1e"]),
               tok_start_var=e * (sums["m2s"] + 2.0 * sums["m1s"] ** 2) + one(sums["tok_start_var"]),
               tok_end_var=e * (sums["m2e"] + 2.0 * sums["m1e"] ** 2) + one(sums["tok_end_var"]))
    return b, e, tol


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return fc.same_bits(a, b)


def planted(Tq, V, labels, low=-40.0):
    """Log-probs [T', V]: 0.0 at ``labels[t]`` and ``low`` elsewhere."""
    x = torch.full((Tq, V), low)
    x[torch.arange(Tq), torch.tensor(labels)] = 0.0
    return x
