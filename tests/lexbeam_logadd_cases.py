"""Test side of LOG-ADD merging in the lexicon-constrained CTC beam search (include/eec.h, csrc/ctc_lexbeam.hip,
eec_ctc_lexbeam_logadd_decode): the merge -- the members of a group folded in the stated pair order -- and ``log_add``, the stated
sequence of fp32 operations, in ``np.float32``: every step is an exactly rounded IEEE operation, so comparisons against the
statement of the search (tests/lexbeam_statement.py, which calls ``fold`` under ``log_add=True``) stay exact, scores bit for bit.
Also here: the CTC forward log-likelihood in float64, the oracle that is independent of any beam search."""
import numpy as np

from lexbeam_cases import F32

# ----------------------------------------------------------------------------------------------------------------------------
# log_add: the constants and the order of include/eec.h
# ----------------------------------------------------------------------------------------------------------------------------
CUTOFF = F32(-17.34375)
LOG2E, LN2_HI, LN2_LO = F32(1.44269502), F32(0.693145751953125), F32(1.42860677e-06)
EXP_C = [F32(c) for c in (1.98412701e-04, 1.38888892e-03, 8.33333377e-03, 4.16666679e-02, 0.166666672, 0.5, 1.0, 1.0)]
SQRT2, LN2 = F32(1.41421354), F32(0.693147182)
LOG_C = [F32(c) for c in (0.0657233745, -0.116206668, 0.119458839, -0.12420819, 0.142122895, -0.166665554, 0.20002535, -0.250000626,
                          0.333333015, -0.5, 1.0)]
ERROR_BOUND = 1.2e-7  # the bound include/eec.h writes for |softplus - log1p(exp(d))| (measured there: 9.9e-8)


def softplus_parts(d):
    """The intermediate values of the recipe for float32 ``d`` in (CUTOFF, 0], elementwise: (n, halved, s)."""
    d = np.asarray(d, dtype=np.float32)
    n = np.rint(d * LOG2E)
    r = d - n * LN2_HI
    r = r - n * LN2_LO
    p = np.full_like(r, EXP_C[0])
    for c in EXP_C[1:]:
        p = p * r + c
    x = np.ldexp(p, n.astype(np.int32))
    u = F32(1.0) + x
    halved = u > SQRT2
    u = np.where(halved, u * F32(0.5), u)
    m = u - F32(1.0)
    q = np.full_like(m, LOG_C[0])
    for c in LOG_C[1:]:
        q = q * m + c
    s = m * q
    s = np.where(halved, s + LN2, s)
    assert all(v.dtype == np.float32 for v in (n, r, p, x, u, m, q, s))
    return n, halved, s


def softplus(d):
    """log1p(exp(d)) by the recipe; 0 at and below the cutoff, where log_add returns ``hi`` alone."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(all="ignore"):
        inside = d > CUTOFF
        return np.where(inside, softplus_parts(np.where(inside, d, F32(0.0)))[2], F32(0.0)).astype(np.float32)


def log_add(a, b):
    """Elementwise on float32 arrays (or scalars): hi + softplus(lo - hi), ``hi`` alone when not lo - hi > CUTOFF."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        a_hi = a > b
        hi, lo = np.where(a_hi, a, b), np.where(a_hi, b, a)
        d = lo - hi
        inside = d > CUTOFF
        s = softplus_parts(np.where(inside, d, F32(0.0)))[2]
        out = np.where(inside, hi + s, hi)
    assert out.dtype == np.float32
    return out


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def pair_grid(n=200_000, seed=3):
    """(a, b) float32: the pairs both log_add entries are held to the statement on.  ``n`` pairs with d = b - a spread over
    [CUTOFF - 1, 0] at magnitudes 1e-3 .. 1e4 and both signs, half of them swapped; then d on and next to the cutoff and every value
    where the recipe branches -- ``n`` changing (d = (k + 1/2) ln 2), the sqrt 2 switch (exp(d) = sqrt 2 - 1 and, after a halving of
    the exponent range, nowhere else) --, each with its fp32 neighbours; then a == b."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-3, 4, size=n)
    a = (mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    d = np.linspace(float(CUTOFF) - 1.0, 0.0, n)
    b = (a.astype(np.float64) + d).astype(np.float32)
    swap = rng.random(n) < 0.5
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    # exact d at small magnitude: hi = 0 and hi = -3 keep lo - hi = d exactly (for hi = -3 up to the rounding of lo)
    edges = [float(CUTOFF), 0.0, np.log(np.sqrt(2.0) - 1.0)] + [(k + 0.5) * np.log(2.0) for k in range(-26, 0)]
    near = []
    for e in edges:
        v = np.float32(e)
        for _ in range(4):
            v = np.nextafter(v, np.float32(-np.inf))
        for _ in range(9):
            near.append(v)
            v = np.nextafter(v, np.float32(np.inf))
    near = np.array([v for v in near if v <= 0], dtype=np.float32)
    ea = np.concatenate([np.zeros_like(near), np.full_like(near, -3.0), near])
    eb = np.concatenate([near, near - np.float32(3.0), np.zeros_like(near)])
    same = (10.0 ** np.linspace(-3, 4, 64)).astype(np.float32)
    same = np.concatenate([same, -same, [np.float32(0.0)]]).astype(np.float32)
    return np.concatenate([a, ea, same]).astype(np.float32), np.concatenate([b, eb, same]).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# the merge
# ----------------------------------------------------------------------------------------------------------------------------
def fold(members, stats=None):
    """One group: ``members`` = [(raw score, id, ...)] in ascending id order.  Returns (survivor index, merged score): the stated
    pair loop -- p < q in id order, both alive; the raw scores decide, the winner's accumulator takes log_add(acc_p, acc_q)."""
    raw = [m[0] for m in members]
    acc = list(raw)
    alive = [True] * len(members)
    for p in range(len(members)):
        for q in range(p + 1, len(members)):
            if not (alive[p] and alive[q]):
                continue
            total = F32(log_add(acc[p], acc[q]))
            if stats is not None:
                stats["merges"] = stats.get("merges", 0) + 1
                if acc[p] == acc[q]:
                    stats["equal_merges"] = stats.get("equal_merges", 0) + 1
            if raw[q] > raw[p]:
                acc[q], alive[p] = total, False
            else:
                acc[p], alive[q] = total, False
    (k,) = [i for i, v in enumerate(alive) if v]
    return k, acc[k]


# ----------------------------------------------------------------------------------------------------------------------------
# CTC itself: the forward log-likelihood of a label sequence, float64
# ----------------------------------------------------------------------------------------------------------------------------
def ctc_forward(e, labels, blank=0):
    """log p(labels | e) under CTC: the sum over all alignments of ``e`` [T, V], by the textbook forward recursion in float64."""
    e = np.asarray(e, dtype=np.float64)
    ext = [blank]
    for c in labels:
        ext += [c, blank]
    alpha = np.full(len(ext), -np.inf)
    alpha[0] = e[0, blank]
    if len(ext) > 1:
        alpha[1] = e[0, ext[1]]
    for t in range(1, e.shape[0]):
        new = np.full(len(ext), -np.inf)
        for s in range(len(ext)):
            terms = [alpha[s]]
            if s >= 1:
                terms.append(alpha[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                terms.append(alpha[s - 2])
            new[s] = np.logaddexp.reduce(terms) + e[t, ext[s]]
        alpha = new
    return float(np.logaddexp.reduce(alpha[-2:])) if len(ext) > 1 else float(alpha[-1])
