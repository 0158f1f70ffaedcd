"""Inputs, the restated semantics and the bounds shared by tests/test_align_oracle.py (CPU), tests/test_gpu_align.py (the HIP
kernel behind ``ctc_align`` / ``BeamInference.get_trellis`` / ``backtrack``) and the generator of tests/golden/ctc_align.npz.

The restatement below is independent of the package and of the reference's text: it is written from the stated semantics of
the CTC forced alignment (BeamInference.get_trellis / backtrack, util/beam_infer.py:129-191), quirks included.

  em [T, V] log-probs, tok N ids, tr [T+1, N+1]:
  tr[0,0] = 0; tr[t+1,0] = tr[t,0] + em[t,0] (column 0, not blank); tr[0,1:] = -inf; tr[T+1-N:,0] = +inf after the running sum;
  tr[t+1,j] = max(tr[t,j] + em[t,blank], tr[t,j-1] + em[t,tok[j-1]])
  backtrack from (T, N): change only if changed > stayed; prob += em[t-1, changed ? tok[j-1] : 0]; Point(j-1, t-1, prob).

Bounds (derived, not measured).  A trellis cell is a sum of at most T emission terms taken in fp32: T dependent roundings of
partial sums none of which exceeds the largest finite cell in magnitude, so ``bound = T * 2^-23 * max |finite tr64|``.  The
path scores are sums of at most T terms of one sign, so the same bound holds with ``|path score|`` in any summation order.  A
decision of the backtrack compares two such cells: it is only pinned where the fp64 margin exceeds ``2 * bound``.
"""
import math
import os

import numpy as np
import torch

import ctc_cases as C
from oracle import conformer_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "ctc_align.npz")

PEAKY_SCALES = (2.0, 5.0, 9.0, 16.0)
PEAKY_PER_SCALE = 4   # emissions (exit, utterance) 0 .. 3 of ctc_cases.peaky_logp(scale)
GREEDY_CUT, N_RANDOM = 40, 12


def trellis_ref(em, tok, blank=0, dtype=np.float64):
    em = np.asarray(em, dtype=dtype)
    tok = np.asarray(tok, dtype=np.int64)
    T, N = em.shape[0], len(tok)
    tr = np.empty((T + 1, N + 1), dtype=dtype)
    tr[0, 0] = 0
    tr[1:, 0] = np.cumsum(em[:, 0], dtype=dtype)
    tr[0, 1:] = -np.inf
    tr[T + 1 - N:, 0] = np.inf
    for t in range(T):
        tr[t + 1, 1:] = np.maximum(tr[t, 1:] + em[t, blank], tr[t, :-1] + em[t, tok])
    return tr


def backtrack_ref(tr, em, tok, blank=0, dtype=np.float64):
    """(path [(token_index, time_index, score)] in time order, min |changed - stayed| along the path, aligned?)."""
    em = np.asarray(em, dtype=dtype)
    tr = np.asarray(tr, dtype=dtype)
    j, prob, path, margin = tr.shape[1] - 1, dtype(0), [], math.inf
    for t in range(tr.shape[0] - 1, 0, -1):
        stayed = tr[t - 1, j] + em[t - 1, blank]
        changed = tr[t - 1, j - 1] + em[t - 1, tok[j - 1]]
        if np.isfinite(stayed) and np.isfinite(changed):
            margin = min(margin, abs(float(changed) - float(stayed)))
        take = bool(changed > stayed)
        prob = dtype(prob + em[t - 1, tok[j - 1] if take else 0])
        path.append((j - 1, t - 1, float(prob)))
        if take:
            j -= 1
            if j == 0:
                break
    return path[::-1], margin, j == 0


def align_ref(em, tok, blank=0, dtype=np.float64):
    tr = trellis_ref(em, tok, blank, dtype)
    path, margin, ok = backtrack_ref(tr, em, tok, blank, dtype)
    return tr, path, margin, ok


def finite_max(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.abs(a[np.isfinite(a)]).max())


def bound(T, tr64):
    return T * 2.0 ** -23 * finite_max(tr64)


def score_bound(T, path64):
    return T * 2.0 ** -23 * max(abs(s) for _, _, s in path64)


def same_infinities(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)))


def compare(name, tr, path, tr64, path64, margin64, T):
    """The three comparisons of one case against an fp64 statement: trellis within ``bound`` with the infinities in the same
    cells; (token_index, time_index) identical where the margin clears ``2 * bound`` (returns whether it did); scores within
    their bound wherever the paths coincide."""
    bd = bound(T, tr64)
    tr = np.asarray(tr, dtype=np.float64)
    assert tr.shape == tr64.shape, (name, tr.shape, tr64.shape)
    assert same_infinities(tr, tr64), name
    fin = np.isfinite(tr64)
    err = float(np.abs(tr[fin] - tr64[fin]).max())
    assert err <= bd, (name, err, bd)
    pinned = margin64 > 2 * bd
    same = [(j, t) for j, t, _ in path] == [(j, t) for j, t, _ in path64]
    if pinned:
        assert same, name
    if same:
        sb = score_bound(T, path64)
        serr = max(abs(a[2] - b[2]) for a, b in zip(path, path64))
        assert serr <= sb, (name, serr, sb)
    return pinned


# ---------------------------------------------------------------------------------------------------------------------------
# the fixture's cases: name -> (emission [T', V] fp32 tensor, tokens, blank)
# ---------------------------------------------------------------------------------------------------------------------------
def peaky_emissions(scale):
    lp = C.peaky_logp(scale)
    return lp.reshape(-1, lp.size(2), lp.size(3))[:PEAKY_PER_SCALE]


def small_emission(T, V, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, V, generator=g, dtype=torch.float64) * scale, -1).float()


def random_tokens(n, V, seed, low=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(low, V, (n,), generator=g).tolist()


def fixture_cases():
    cases = {}
    for scale in PEAKY_SCALES:
        for i, em in enumerate(peaky_emissions(scale)):
            cases[f"scale{scale:g}-{i}-greedy"] = (em, R.greedy_ctc(em, 0)[:GREEDY_CUT], 0)
            cases[f"scale{scale:g}-{i}-random"] = (em, random_tokens(N_RANDOM, 256, 100 * int(scale) + i), 0)
    cases["v29-t20"] = (small_emission(20, 29, 3.0, 29), [5, 5, 17, 1, 28, 9, 9], 0)  # repeats get no special treatment
    # blank_id = 3: column 0 still accumulates em[:, 0] and a stay still scores em[t, 0]; ids 0 and 3 are ordinary tokens
    cases["blank3"] = (small_emission(30, 32, 4.0, 3), [7, 0, 3, 12, 12, 31, 3, 1, 0, 20], 3)
    return cases


def load_fixture():
    """name -> dict(em fp32 [T', V], tok, blank, trellis fp32, path [(j, t, score)], margin): what the reference's own
    get_trellis / backtrack returned on the CPU (tests/golden/make_align_golden.py).  The peaky emissions are regenerated from
    their seeds (64 KB each; the fixture keeps their fp64 sums as a check) -- everything else is read from the file."""
    z = np.load(FIXTURE)
    out = {}
    for name, (em, tok, blank) in fixture_cases().items():
        if f"{name}/em" in z:
            em = torch.from_numpy(z[f"{name}/em"])
        else:
            assert abs(float(em.double().sum()) - float(z[f"{name}/em_sum"])) < 1e-6 * abs(float(z[f"{name}/em_sum"])), name
        assert list(z[f"{name}/tok"]) == list(tok) and int(z[f"{name}/blank"]) == blank, name
        p = z[f"{name}/path"]
        out[name] = dict(em=em, tok=list(tok), blank=blank, trellis=z[f"{name}/trellis"],
                         path=[(int(j), int(t), float(s)) for j, t, s in p], margin=float(z[f"{name}/margin"]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# lane-boundary and edge shapes for the kernel: (name, T', V, N, blank)
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(f"n{n}", 160 if n > 80 else 80, 64, n, 0) for n in (1, 63, 64, 65, 127, 128, 129)] + [
    ("n-equals-t", 80, 64, 80, 0), ("t1-n1", 1, 64, 1, 0), ("v29", 80, 29, 23, 0), ("blank3", 80, 64, 30, 3)]
LONG_SHAPE = ("t1024-n255", 1024, 64, 255, 0)


def edge_case(name, T, V, N, blank):
    seed = sum(map(ord, name))
    return small_emission(T, V, 3.0, seed), random_tokens(N, V, seed + 1, low=0), blank
