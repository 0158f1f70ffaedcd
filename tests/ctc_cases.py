"""Inputs and the fp64 reference shared by tests/test_gpu_ctc.py (the HIP CTC loss, gradient and prefix beam search) and the
host checks of those inputs in tests/test_oracle.py.  Everything here is seeded and runs on the CPU; nothing is read but the
committed fixture tests/golden/config1_peaky.npz.

Reference of the loss and gradient: torch.nn.CTCLoss(blank, 'mean', zero_infinity=True) through the reference's per-exit loop
(train.py:53-68), evaluated in fp64 (``dtype=torch.float32`` gives the reference's own fp32 result: the yardstick ``err32``).
"""
import math
import os

import numpy as np
import torch

from early_exit_transformer_amd import synth
from oracle import conformer_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# logit scale -> the band max |log-prob| of log_softmax(randn(.., 256) * scale) must land in (asserted by the host test):
# today's regime, 30, the committed peaky fixture's 59, and twice that (beyond the fp32 range of exp)
PEAKY_SCALES = {2.0: (8.0, 20.0), 5.0: (24.0, 40.0), 9.0: (48.0, 75.0), 16.0: (95.0, 140.0)}
# padded target width -> states per lane of the loss kernels (2 S + 1 <= 64 P)
WIDTH_FOR_P = {2: 63, 4: 100, 8: 200}


def ref_ctc(logp, tgt, tl, blank=0, dtype=torch.float64, w=None):
    """(per-exit losses [E], d(sum_e w_e loss_e)/d logp) of the reference's loop in ``dtype`` on the CPU."""
    E, B, T, _ = logp.shape
    ctc = torch.nn.CTCLoss(blank=blank, reduction="mean", zero_infinity=True)
    il = torch.full((B,), T, dtype=torch.long)
    x = logp.detach().clone().to(dtype).requires_grad_(True)
    losses = torch.stack([ctc(x[e].permute(1, 0, 2), tgt, il, tl) for e in range(E)])
    ww = torch.ones(E, dtype=dtype) if w is None else w.to(dtype)
    (losses * ww).sum().backward()
    return losses.detach(), x.grad


def ref_nll(logp_tv, target, blank=0):
    """-log p_ctc(target) of ONE lattice [T', V] in fp64 (reduction 'sum', zero_infinity off: +inf when infeasible)."""
    T = logp_tv.shape[0]
    tg = torch.as_tensor(list(target) or [blank], dtype=torch.long).view(1, -1)
    return float(torch.nn.functional.ctc_loss(torch.as_tensor(logp_tv, dtype=torch.float64).view(T, 1, -1), tg, torch.tensor([T]),
                                              torch.tensor([len(target)]), blank=blank, reduction="sum", zero_infinity=False))


def pad_targets(tgt, width, pad=126):
    out = torch.full((tgt.size(0), width), pad, dtype=torch.int64)
    out[:, : tgt.size(1)] = tgt
    return out


def greedy_targets(logp_btv, blank=0, min_width=1):
    """Matching targets: the greedy decode of every utterance's own log-probs, [B, S] (padded with 126) + lengths."""
    dec = [R.greedy_ctc(logp_btv[b], blank) for b in range(logp_btv.size(0))]
    S = max([len(d) for d in dec] + [min_width])
    tgt = torch.full((len(dec), S), 126, dtype=torch.int64)
    for b, d in enumerate(dec):
        tgt[b, : len(d)] = torch.tensor(d, dtype=torch.int64)
    return tgt, torch.tensor([len(d) for d in dec], dtype=torch.int64)


def peaky_logp(scale, E=2, B=3, T=64, V=256, seed=0):
    g = torch.Generator().manual_seed(1000 + int(scale * 10) + seed)
    return torch.log_softmax(torch.randn(E, B, T, V, generator=g, dtype=torch.float64) * scale, -1).float()


def fixture_logp():
    """The committed peaky fixture's log-prob rows (every 16th frame of config1_peaky), used directly as [6, 4, 16, 256]."""
    z = np.load(os.path.join(GOLDEN, "config1_peaky.npz"))
    return torch.from_numpy(z["logp"].astype(np.float32))


def part1_cases():
    """name -> (logp [E, B, T', V], matching (tgt, tl) from exit 0's greedy decode, mismatched (tgt, tl))."""
    cases = {}
    for scale in PEAKY_SCALES:
        lp = peaky_logp(scale)
        cases[f"scale{scale:g}"] = (lp, greedy_targets(lp[0]), synth.synth_targets(lp.size(1), 12, 256, seed=int(scale)))
    lp = fixture_logp()
    cases["fixture"] = (lp, greedy_targets(lp[0]), synth.synth_targets(4, 6, 256, seed=59))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# part 2: hand-built lattices.  V = 8, blank 0, target labels among {3, 4}; on the NAMED frames blank and the target's labels
# all sit at -x (class 7, outside the target, takes the row's mass); every other frame is likely (log_softmax(randn)).
# ---------------------------------------------------------------------------------------------------------------------------
RANGE_T, RANGE_V = 40, 8
RANGE_X = (20.0, 40.0, 50.0, 60.0, 80.0)
# (1, 2) share a renormalisation of the forward recursion, (2, 3) straddle one, (0, 1, 2) is the start (three emissions before
# the first one); (17, 18) lies past the first look-ahead group of either ring depth (16 / 8), (33, 34) in the ragged tail of the
# 16-deep ring; (38, 39) / (37, 38) are the first pairs of the beta recursion (walking down from T' - 1: shared / straddling)
RANGE_FRAMES = ((1, 2), (2, 3), (0, 1, 2), (17, 18), (33, 34), (38, 39), (37, 38))


def range_lattice(frames, x, target=(3, 4), T=RANGE_T, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    z = torch.randn(T, RANGE_V, generator=g, dtype=torch.float64)
    for t in frames:
        z[t] = -x - 5.0
        z[t, 7] = 0.0
        z[t, [0] + list(target)] = -x
    return torch.log_softmax(z, -1)


def range_cases():
    """[(name, logp [T', V] fp64, target)]: every one has a FINITE fp64 reference loss (asserted by the host test)."""
    out = []
    for fr in RANGE_FRAMES:
        for x in RANGE_X:
            out.append((f"frames{fr}-x{x:g}", range_lattice(fr, x), (3, 4)))
    out.append(("frames(1, 2)-x60-one-label", range_lattice((1, 2), 60.0, target=(3,)), (3,)))
    # one frame below the fp32 range of exp
    out.append(("frame5-x95", range_lattice((5,), 95.0), (3, 4)))
    out.append(("frame0-x95", range_lattice((0,), 95.0), (3, 4)))
    # a masked vocabulary: exact -inf on classes outside the target, everywhere
    lp = range_lattice((), 0.0)
    z = lp.clone()
    z[:, [1, 2, 5]] = -math.inf
    out.append(("masked-vocabulary", torch.log_softmax(z, -1), (3, 4)))
    return out


def infeasible_cases():
    """[(name, logp, target)]: -inf on a class every feasible path needs -> reference loss +inf (0 under zero_infinity)."""
    lp = range_lattice((), 0.0)
    a = lp.clone()
    a[:, 4] = -math.inf                 # label 4 is never possible
    b = range_lattice((), 0.0, T=3)     # T' = 3, target [3, 4]: the alignments need label 3 at frame 0 or 1 ...
    b = b.clone()
    b[0, 3] = b[1, 3] = -math.inf       # ... and it is masked on both
    return [("label-masked-everywhere", a, (3, 4)), ("label-masked-where-needed", b, (3, 4))]


# ---------------------------------------------------------------------------------------------------------------------------
# part 4: beam-search inputs (the existing test's generator: randn * scale, about half the frames blank-boosted)
# ---------------------------------------------------------------------------------------------------------------------------
BEAM_MARGIN = 5e-3
# (N, T', V, beam, scale): today's regime and the peaky scales of part 1
BEAM_CASES = ((8, 64, 64, 10, 3.0), (8, 64, 64, 10, 8.0), (8, 64, 64, 10, 16.0), (8, 40, 16, 16, 6.0), (3, 50, 32, 1, 9.0))


def beam_logp(N, T, V, scale, seed=0, blank=0):
    g = torch.Generator().manual_seed(N * 1000 + T + seed)
    x = torch.randn(N, T, V, generator=g) * scale
    x[:, :, blank] += scale * 2.0 * (torch.rand(N, T, generator=g) < 0.5)
    x[0, 5:9] = x[0, 5:6]
    return torch.log_softmax(x, -1)


def fixture_beam_logp():
    lp = fixture_logp()
    return lp.reshape(24, 16, 256)[::3].contiguous()  # 8 of the 24 (exit, utterance) rows


def big_batch_logp():
    """[384, 256, 256]: 6 exits x 64 utterances at the benchmark geometry, logit scales cycling 1 (near-uniform) .. 16 (peaky).
    Every frame's largest logit is raised by 0.6 so that no frame is a near-tie between two labels: among 256 frames of
    randn * scale the closest pair is otherwise ~1e-3 * scale apart, and the oracle's margin with it."""
    g = torch.Generator().manual_seed(384)
    x = torch.randn(384, 256, 256, generator=g)
    scale = torch.tensor([1.0, 3.0, 8.0, 16.0])[torch.arange(384) % 4].view(-1, 1, 1)
    x = x * scale
    x[:, :, 0] += (scale * 3.0 + 8.0).view(-1, 1) * (torch.rand(384, 256, generator=g) < 0.5)  # blank above the skip threshold
    x.scatter_add_(2, x.argmax(-1, keepdim=True), torch.full((384, 256, 1), 0.6))
    return torch.log_softmax(x, -1)


BIG_SAMPLE = tuple(range(5, 5 + 23 * 16, 23))  # 16 sequences, four of each scale (the stride is odd)


def safe_margin(final):
    return len(final) < 2 or final[0][1] - final[1][1] > BEAM_MARGIN
