"""Shared cases of the edit-distance tests (tests/test_host_scoring.py, tests/test_gpu_scoring.py): the statement of include/eec.h
("Edit distance") restated as a plain Python double loop with its walk-back, a brute-force enumerator of ALL alignments of a pair,
and the batches every implementation is held to -- exact integer equality, no tolerance.

A batch is ``(hyp [P, Lh], hyp_len [P], ref [R, Lr], ref_len [R], ref_of [P] or None)``, int32 CPU tensors.  The rows are padded
with garbage that would change the result if it were read: a hypothesis row goes on with the reference's tokens at the same
positions (its last token where the reference has ended), so a token read past the hypothesis' length is a hit that is not there;
a reference row goes on with the first symbol of the batch's alphabet, which the hypotheses are made of."""
import functools
import itertools

import torch

STEP, SUB = 1 << 16, (1 << 16) + 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)  # the lane and strip boundaries of the kernel


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement and the brute force
# ---------------------------------------------------------------------------------------------------------------------------
def restate(r, h):
    """``(distance, subs, dels, ins, ops)`` of reference ``r`` and hypothesis ``h`` (lists): the recurrence of include/eec.h cell by
    cell, dir = the FIRST of (diag, del, ins) that attains K, the walk back from (m, n), ops in forward order."""
    m, n = len(r), len(h)
    K = [[0] * (n + 1) for _ in range(m + 1)]
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(1, n + 1):
        K[0][j], D[0][j] = j * STEP, 3
    for i in range(1, m + 1):
        K[i][0], D[i][0] = i * STEP, 2
        Ki, Kp, Di, ri = K[i], K[i - 1], D[i], r[i - 1]
        for j in range(1, n + 1):
            eq = ri == h[j - 1]
            cd, cu, cl = Kp[j - 1] + (0 if eq else SUB), Kp[j] + STEP, Ki[j - 1] + STEP
            v = min(cd, cu, cl)
            Ki[j] = v
            Di[j] = (0 if eq else 1) if v == cd else 2 if v == cu else 3
    dist, subs = K[m][n] >> 16, K[m][n] & 0xffff
    assert (dist - subs - (n - m)) % 2 == 0
    dels = (dist - subs - (n - m)) // 2
    ops, i, j = [], m, n
    while i > 0 or j > 0:
        code = D[i][j]
        ops.append(code)
        i -= code != 3
        j -= code != 2
    return dist, subs, dels, dels + n - m, ops[::-1]


def brute_force(r, h):
    """``(minimum cost, fewest substitutions among the minimum-cost alignments)`` by enumerating every alignment of the pair."""
    best = [None]

    def walk(i, j, cost, subs):
        if i == len(r) and j == len(h):
            if best[0] is None or (cost, subs) < best[0]:
                best[0] = (cost, subs)
            return
        if i < len(r) and j < len(h):
            miss = r[i] != h[j]
            walk(i + 1, j + 1, cost + miss, subs + miss)
        if i < len(r):
            walk(i + 1, j, cost + 1, subs)
        if j < len(h):
            walk(i, j + 1, cost + 1, subs)
    walk(0, 0, 0, 0)
    return best[0]


def replay(r, h, ops):
    """Whether ``ops`` turns ``r`` into ``h``, and the (subs, dels, ins, hits) it spends."""
    i = j = 0
    n = [0, 0, 0, 0]
    for op in ops:
        n[op] += 1
        if op in (0, 1):
            if i >= len(r) or j >= len(h) or (r[i] == h[j]) != (op == 0):
                return False, None
            i, j = i + 1, j + 1
        elif op == 2:
            i += 1
        elif op == 3:
            j += 1
        else:
            return False, None
    return i == len(r) and j == len(h), (n[1], n[2], n[3], n[0])


# ---------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------
def _batch(pairs=None, hyps=None, refs=None, ref_of=None, hyp_pitch=None, ref_pitch=None, fill=0):
    """Padded rows of ``pairs`` [(ref, hyp)] (pair p against reference p), or of ``hyps`` / ``refs`` with ``ref_of``."""
    if pairs is not None:
        refs, hyps = [p[0] for p in pairs], [p[1] for p in pairs]
    Lh = hyp_pitch if hyp_pitch is not None else max(len(h) for h in hyps) + 3
    Lr = ref_pitch if ref_pitch is not None else max(len(r) for r in refs) + 3
    R = len(refs)
    hyp = torch.zeros((len(hyps), Lh), dtype=torch.int64)
    for p, h in enumerate(hyps):
        q = p if ref_of is None else ref_of[p]
        r = refs[q] if 0 <= q < R else []
        tail = [(r[k] if k < len(r) else r[-1] if r else fill) for k in range(len(h), Lh)]
        hyp[p] = torch.tensor(list(h) + tail, dtype=torch.int64)
    ref = torch.full((R, Lr), fill, dtype=torch.int64)
    for q, r in enumerate(refs):
        ref[q, :len(r)] = torch.tensor(list(r), dtype=torch.int64)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    return (hyp.to(torch.int32), i32([len(h) for h in hyps]), ref.to(torch.int32), i32([len(r) for r in refs]),
            None if ref_of is None else i32(list(ref_of)))


def _rand(g, n, alphabet):
    return [alphabet[k] for k in torch.randint(0, len(alphabet), (n,), generator=g).tolist()]


def binary_sequences():
    """Every sequence over {0, 1} of length 0 to 4: 31 of them."""
    return [list(s) for n in range(5) for s in itertools.product((0, 1), repeat=n)]


@functools.lru_cache(maxsize=None)
def cases():
    g = torch.Generator().manual_seed(20)
    out = {}
    seqs = binary_sequences()
    # every pair of sequences over {0, 1} of lengths 0 .. 4: 961 pairs against 31 references, one launch
    out["binary-961"] = _batch(hyps=[seqs[p % 31] for p in range(961)], refs=seqs, ref_of=[p // 31 for p in range(961)], hyp_pitch=6, ref_pitch=6)
    # random pairs, lengths from LENGTHS: every length is a reference length and a hypothesis length at least twice per alphabet.  Hypotheses
    # of up to 256 tokens at pitch 256 (strips of 4: a 256-token row fills all 64 lanes), the 257-token ones at pitch 260 (strips of 8)
    for A in (2, 5, 1000):
        alphabet = list(range(A))
        shapes = [(LENGTHS[k], LENGTHS[(5 * k + 1 + A) % 12]) for k in range(12)] + [(LENGTHS[(7 * k + 3 + A) % 12], LENGTHS[k]) for k in range(12)]
        pairs = [(_rand(g, m, alphabet), _rand(g, n, alphabet)) for m, n in shapes]
        out[f"random-A{A}-strip4"] = _batch([p for p in pairs if len(p[1]) <= 256], hyp_pitch=256, ref_pitch=260)
        out[f"random-A{A}-strip8"] = _batch([p for p in pairs if len(p[1]) > 256], hyp_pitch=260, ref_pitch=257)
    # the wider strips away from their smallest size: 512 columns in strips of 8, 513 in strips of 16
    out["strip8-512"] = _batch([(_rand(g, 300, [0, 1, 2]), _rand(g, 512, [0, 1, 2]))], hyp_pitch=512, ref_pitch=300)
    out["strip16-513"] = _batch([(_rand(g, 200, [0, 1, 2]), _rand(g, 513, [0, 1, 2]))], hyp_pitch=513, ref_pitch=203)
    # identical pairs, disjoint pairs, an empty reference, an empty hypothesis, both empty
    same = [_rand(g, n, list(range(7))) for n in (1, 5, 70)]
    out["identical-disjoint-empty"] = _batch([(s, list(s)) for s in same] + [(s, [v + 100 for v in s]) for s in same] +
                                             [([], s) for s in same] + [(s, []) for s in same] + [([], [])])
    # ids at the int32 extremes, and negative ids
    ext = [I32_MIN, I32_MAX, -1, 0, 1, I32_MIN + 1, I32_MAX - 1]
    out["int32-extremes"] = _batch([(_rand(g, m, ext), _rand(g, n, ext)) for m, n in ((10, 12), (70, 64), (33, 5), (1, 1))], fill=I32_MIN)
    # the longest rows
    five = list(range(5))
    out["1024x1024"] = _batch([(_rand(g, 1024, five), _rand(g, 1024, five))], hyp_pitch=1024, ref_pitch=1024)
    out["1024x1"] = _batch([(_rand(g, 1024, five), _rand(g, 1, five))], hyp_pitch=1, ref_pitch=1024)
    out["1x1024"] = _batch([(_rand(g, 1, five), _rand(g, 1024, five))], hyp_pitch=1024, ref_pitch=1)
    # many hypotheses against a few references, out of order, two entries that name no reference
    refs = [_rand(g, n, five) for n in (9, 0, 30, 17, 64)]
    of = [(3 * p + 1) % 5 for p in range(40)]
    of[7], of[22] = -1, 5
    out["ref-of"] = _batch(hyps=[_rand(g, (11 * p) % 37, five) for p in range(40)], refs=refs, ref_of=of)
    # lengths above the pitch and below 0: clamped to the whole row and to nothing
    hyp, hl, ref, rl, _ = _batch([(_rand(g, 20, five), _rand(g, 24, five)) for _ in range(6)], hyp_pitch=24, ref_pitch=20)
    hl, rl = hl.clone(), rl.clone()
    hl[0], hl[1], rl[2], rl[3], hl[4], rl[4], hl[5], rl[5] = 27, -2, 23, -1, 1 << 30, -(1 << 30), -7, 900
    out["lengths-clamped"] = (hyp, hl, ref, rl, None)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """``(counts int32 [P, 4], n_ops int32 [P], ops: list of lists)`` of a batch by the restatement; (-1, -1, -1, -1), 0 and [] for a
    pair whose ``ref_of`` names no reference."""
    hyp, hl, ref, rl, of = cases()[name]
    counts, n_ops, ops = [], [], []
    for p in range(hyp.size(0)):
        q = p if of is None else int(of[p])
        if not 0 <= q < ref.size(0):
            counts.append([-1] * 4), n_ops.append(0), ops.append([])
            continue
        n, m = min(max(int(hl[p]), 0), hyp.size(1)), min(max(int(rl[q]), 0), ref.size(1))
        d, s, dl, ins, op = restate(ref[q, :m].tolist(), hyp[p, :n].tolist())
        counts.append([d, s, dl, ins]), n_ops.append(len(op)), ops.append(op)
    return torch.tensor(counts, dtype=torch.int32).reshape(-1, 4), torch.tensor(n_ops, dtype=torch.int32), ops


def check_against_expected(name, got, sentinel=None):
    """``got``: an ``EditCounts`` (CPU tensors) of batch ``name`` with ops.  Counts, hits, ``n_ops`` and the written op bytes equal the
    restatement's; with ``sentinel`` every byte past ``n_ops`` still holds it."""
    counts, n_ops, ops = expected(name)
    hyp, hl, ref, rl, of = cases()[name]
    assert torch.equal(torch.stack([got.distance, got.subs, got.dels, got.ins], dim=1), counts), name
    assert got.distance.dtype == torch.int32 and got.hits.dtype == torch.int32
    assert torch.equal(got.n_ops, n_ops), name
    assert got.ops.shape == (hyp.size(0), ref.size(1) + hyp.size(1)) and got.ops.dtype == torch.uint8
    for p, op in enumerate(ops):
        assert got.ops[p, :len(op)].tolist() == op, (name, p)
        if sentinel is not None:
            assert (got.ops[p, len(op):] == sentinel).all(), (name, p)
        q = p if of is None else int(of[p])
        if 0 <= q < ref.size(0):
            m = min(max(int(rl[q]), 0), ref.size(1))
            assert int(got.hits[p]) == m - int(counts[p, 1]) - int(counts[p, 2])
        else:
            assert int(got.hits[p]) == -1
