"""Inputs and the reference shared by tests/test_host_exit.py and tests/test_gpu_exit.py (adaptive inference: csrc/exit_stats.hip
behind eec_exit_stats / eec_exit_route).  Everything here is seeded and runs on the CPU; nothing is read but the committed fixture
tests/golden/config1_peaky.npz (through ctc_cases).

Reference: the statement of include/eec.h in fp64 torch ops -- lp = log_softmax(x), p = exp(lp), len_b = clamp(frame_len[b], 0, T),
n_b = max(len_b, 1):
    entropy[e, b] = (1 / n_b) sum_{t < len_b} -sum_v p_v lp_v  (p_v = 0: 0),  confidence[e, b] = (1 / n_b) sum_{t < len_b} max_v p_v,
    greedy_logp[e, b] = sum_{t < len_b} max_v lp_v
and the routing: row i leaves when score[i] < threshold (> with higher_is_better; a tie or a NaN stays; force_all: every row)."""
import torch

import ctc_cases as CC
import distill_cases as D


def ref_stats(x, frame_len=None, dtype=torch.float64):
    """[3, E, B] (entropy, confidence, greedy_logp) of the statement in ``dtype`` on the CPU."""
    xx = x.detach().cpu().to(dtype)
    E, B, T, _ = xx.shape
    mask, denom = D.frame_mask(frame_len, B, T)
    lp = torch.log_softmax(xx, -1)
    p = lp.exp()
    ent = -torch.where(p == 0, torch.zeros_like(p), p * lp).sum(-1)
    top = lp.max(-1).values
    add = lambda term: torch.where(mask, term, torch.zeros_like(term)).sum(-1)  # noqa: E731
    n = denom.to(dtype)
    return torch.stack([add(ent) / n, add(top.exp()) / n, add(top)])


def loop_stats(x, frame_len=None):
    """The same by a brute-force loop over (e, b, t) in fp64 Python floats: no masks, no broadcasting."""
    import math
    E, B, T, V = x.shape
    out = torch.zeros(3, E, B, dtype=torch.float64)
    for b in range(B):
        n = T if frame_len is None else min(max(int(frame_len[b]), 0), T)
        for e in range(E):
            ent = conf = logp = 0.0
            for t in range(n):
                row = [float(v) for v in x[e, b, t]]
                m = max(row)
                lse = m + math.log(sum(math.exp(v - m) for v in row))
                lps = [v - lse for v in row]
                ent -= sum(math.exp(l) * l for l in lps if math.exp(l) != 0.0)
                conf += math.exp(max(lps))
                logp += max(lps)
            out[0, e, b], out[1, e, b], out[2, e, b] = ent / max(n, 1), conf / max(n, 1), logp
    return out


def ref_route(score, threshold, higher_is_better=False, force_all=False):
    """(stay [..], leave [..]) as Python lists, ascending."""
    s = [float(v) for v in score]
    leaves = [True if force_all else (v > threshold if higher_is_better else v < threshold) for v in s]
    return [i for i, l in enumerate(leaves) if not l], [i for i, l in enumerate(leaves) if l]


def ref_select(score, threshold, higher_is_better=False, min_exit=0, max_exit=None):
    """select_exits on a table [E, B], by a loop."""
    E, B = score.shape
    hi = E - 1 if max_exit is None else max_exit
    thr = list(threshold) if isinstance(threshold, (list, tuple)) else [threshold] * E
    out = []
    for b in range(B):
        pick = hi
        for e in range(min_exit, hi + 1):
            v = float(score[e, b])
            if (v > thr[e]) if higher_is_better else (v < thr[e]):
                pick = e
                break
        out.append(pick)
    return torch.tensor(out, dtype=torch.int32)


_CASES = None


def cases():
    """name -> (x [E, B, T, V] fp32, frame_len int64 [B] or None), built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    c = {}
    for s in (1.0, 8.0, 16.0):
        x = CC.peaky_logp(s, E=3, B=3, T=19)
        c[f"scale{s:g}"] = (x, None)
        c[f"scale{s:g}-ragged"] = (x, D.cycle_lens(3, 19))
    c["V32"] = (CC.peaky_logp(4.0, E=2, B=5, T=19, V=32, seed=1), D.cycle_lens(5, 19))
    c["V160"] = (CC.peaky_logp(4.0, E=2, B=5, T=19, V=160, seed=2), D.cycle_lens(5, 19))
    c["E1"] = (CC.peaky_logp(8.0, E=1, B=5, T=70, seed=3), torch.tensor([70, 64, 65, 1, 0]))  # the 64-frame path of the reduction
    c["E16"] = (CC.peaky_logp(2.0, E=16, B=2, T=9, V=64, seed=4), torch.tensor([9, 4]))
    fx = CC.fixture_logp()
    c["fixture"] = (fx, None)
    c["fixture-ragged"] = (fx, D.cycle_lens(fx.size(1), fx.size(2)))
    # logits (not normalised) with exact -inf entries, one row with a single finite entry
    g = torch.Generator().manual_seed(9)
    z = torch.randn(2, 3, 11, 64, generator=g) * 3
    z[:, :, :, ::3] = float("-inf")
    z[0, 1, 4, 1:] = float("-inf")
    z[0, 1, 4, 0] = 2.5
    c["neg-inf"] = (z, torch.tensor([11, 11, 6]))
    # lengths out of range: clamped to [0, T]
    c["lengths-clamped"] = (CC.peaky_logp(1.0, E=2, B=3, T=19, seed=5), torch.tensor([25, -3, 19]))
    _CASES = c
    return c


def nan_past_length():
    """(x with NaN at and past every length, frame_len, the same x with those frames zeroed)."""
    x, fl = cases()["scale8-ragged"]
    mask, _ = D.frame_mask(fl, x.size(1), x.size(2))
    bad = x.clone()
    bad[:, ~mask] = float("nan")
    clean = x.clone()
    clean[:, ~mask] = 0.0
    return bad, fl, clean


def nan_inside_length():
    """(x with one NaN inside the valid frames of (e, b) = (1, 2), frame_len, (1, 2))."""
    x, _ = cases()["scale8"]
    fl = torch.tensor([19, 7, 12])
    bad = x.clone()
    bad[1, 2, 5, 17] = float("nan")
    return bad, fl, (1, 2)


CRITERIA = {"entropy": (0, False), "confidence": (1, True), "greedy_logp": (2, True)}  # criterion -> (statistic, higher is better)


def routing_scores(stats, frame_len, criterion):
    """The score [E, B] ``forward_adaptive`` routes by, from statistics [3, E, B]: the statistic itself, greedy_logp / max(len, 1)."""
    s = stats[CRITERIA[criterion][0]]
    return s / frame_len.clamp(min=1).to(s.dtype) if criterion == "greedy_logp" else s


def widest_gap_thresholds(score):
    """Per exit (thresholds [E], gaps [E]) in fp64: the midpoint of, and the width of, the widest gap between the exit's sorted scores."""
    s = score.double().sort(dim=1).values
    gap, i = (s[:, 1:] - s[:, :-1]).max(dim=1)
    lo = s.gather(1, i.view(-1, 1)).view(-1)
    return lo + gap / 2, gap


def score_bound(logp, frame_len, criterion):
    """The statistics bound on the routing score of ``logp`` [E, B, T', V] (fp32, CPU): ``stats_bound`` of the statistic, divided by
    max(len, 1) where the score is."""
    want = ref_stats(logp, frame_len)
    from early_exit_transformer_amd import ctc
    err32 = (torch.stack(list(ctc.exit_statistics(logp, frame_len))).double() - want).abs()
    k = CRITERIA[criterion][0]
    b = stats_bound(want, err32)[k]
    return b / frame_len.clamp(min=1).double() if criterion == "greedy_logp" else b


_REFS = {}


def reference(name):
    """(want fp64 [3, E, B], err32 [3, E, B]: the fp32 host path's own error against it), computed once and shared."""
    if name not in _REFS:
        from early_exit_transformer_amd import ctc
        x, fl = cases()[name]
        want = ref_stats(x, fl)
        got32 = torch.stack(list(ctc.exit_statistics(x, fl)))
        _REFS[name] = (want, (got32.double() - want).abs())
    return _REFS[name]


def stats_bound(want, err32):
    """The project's loss bound (tests/test_gpu_ctc.py): |err| <= max(2e-5 + 2e-5 |want|, 2 err32)."""
    return torch.maximum(2e-5 + 2e-5 * want.abs(), 2 * err32)
