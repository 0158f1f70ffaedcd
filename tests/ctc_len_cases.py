"""Inputs and the fp64 reference shared by tests/test_gpu_ctc_len.py (the CTC loss, its gradient, the greedy decoder and the prefix
beam search with per-utterance input lengths) and the host checks of those inputs in tests/test_host_ctc_len.py.  Everything here
is seeded and runs on the CPU; generators and the fixture are those of tests/ctc_cases.py.

Reference of the loss and gradient: torch.nn.CTCLoss(blank, 'mean', zero_infinity=True) through the reference's per-exit loop
(train.py:53-68) in fp64, given the real ``input_lengths`` instead of the reference's T' (train.py:57-58).  Of the decoders: the
oracle's greedy decode and oracle/ctc_beam_ref.py on the slice ``logp[s, :len_s]``.
"""
import torch

import ctc_cases as C
from oracle import conformer_ref as R
from oracle.ctc_beam_ref import ctc_prefix_beam_search

RAGGED_LENS = (64, 33, 1, 0, 17, 2)  # input_len of the peaky cases: E = 2, B = 6, T' = 64
RING_T = 40
RING_LENS = (0, 1, 2, 3, 4, 8, 9, 16, 17, 33, 39, 40)  # around the look-ahead rings (16 / 8 / 4 deep) and the meeting point


def ref_ctc(logp, tgt, tl, il, blank=0, dtype=torch.float64, w=None):
    """(per-exit losses [E], d(sum_e w_e loss_e)/d logp) of the reference's loop in ``dtype`` on the CPU, input lengths ``il`` [B]
    (clamped to [0, T'] as the kernels clamp them)."""
    E, B, T, _ = logp.shape
    ctc = torch.nn.CTCLoss(blank=blank, reduction="mean", zero_infinity=True)
    il = torch.as_tensor(il).cpu().to(torch.long).clamp(0, T)
    x = logp.detach().clone().to(dtype).requires_grad_(True)
    losses = torch.stack([ctc(x[e].permute(1, 0, 2), tgt, il, tl) for e in range(E)])
    ww = torch.ones(E, dtype=dtype) if w is None else w.to(dtype)
    (losses * ww).sum().backward()
    return losses.detach(), x.grad


def valid_mask(il, T):
    """[B, T'] bool: frame t of utterance b is below its (clamped) length."""
    il = torch.as_tensor(il).cpu().to(torch.long).clamp(0, T)
    return torch.arange(T).view(1, -1) < il.view(-1, 1)


def overwrite_pad(logp, il, kind, seed=0):
    """A copy of ``logp`` [..., B, T', V] whose frames t >= len_b hold NaN (``kind`` "nan") or other log-prob rows ("random")."""
    out = logp.clone()
    T = logp.size(-2)
    pad = ~valid_mask(il, T)
    if kind == "nan":
        fill = torch.full_like(out, float("nan"))
    else:
        g = torch.Generator().manual_seed(4242 + seed)
        fill = torch.log_softmax(torch.randn(out.shape, generator=g) * 7.0, -1).to(out.dtype)
    m = pad.view(*([1] * (out.dim() - 3)), *pad.shape, 1).expand_as(out)
    return torch.where(m, fill, out)


def greedy_targets_of_valid_frames(logp_btv, il, blank=0, min_width=1):
    """The greedy decode of every utterance's VALID frames, [B, S] (padded with 126) + lengths."""
    dec = [R.greedy_ctc(logp_btv[b, : int(n)], blank) if int(n) > 0 else [] for b, n in enumerate(il)]
    S = max([len(d) for d in dec] + [min_width])
    tgt = torch.full((len(dec), S), 126, dtype=torch.int64)
    for b, d in enumerate(dec):
        tgt[b, : len(d)] = torch.tensor(d, dtype=torch.int64)
    return tgt, torch.tensor([len(d) for d in dec], dtype=torch.int64)


def ragged_case(scale, P):
    """(logp [2, 6, 64, 256], targets padded to P's width, target_len, input_len): targets are exit 0's greedy decode over each
    utterance's valid frames, so exit 0 is the matching and exit 1 the mismatched case."""
    lp = C.peaky_logp(scale, E=2, B=6, T=64)
    il = torch.tensor(RAGGED_LENS)
    tgt, tl = greedy_targets_of_valid_frames(lp[0], il)
    width = C.WIDTH_FOR_P[P]
    if tgt.size(1) > width:  # 64 distinct frames decode to 64 labels: one more than the widest P = 2 target
        tgt, tl = tgt[:, :width], tl.clamp(max=width)
    return lp, C.pad_targets(tgt, width), tl, il


def ring_case(P, V=32, seed=40):
    """(logp [2, 13, 40, V], targets, target_len, input_len): one utterance per length of RING_LENS with min(3, len) labels, and
    one more of length 40 with an empty target."""
    g = torch.Generator().manual_seed(seed)
    il = torch.tensor(RING_LENS + (RING_T,))
    B = il.numel()
    lp = torch.log_softmax(torch.randn(2, B, RING_T, V, generator=g) * 2.0, -1)
    tgt = torch.randint(1, V, (B, 3), generator=g)
    tl = il.clamp(max=3)
    tl[-1] = 0
    return lp, C.pad_targets(tgt, C.WIDTH_FOR_P[P]), tl, il


FEASIBLE_TARGET = [5, 5, 6, 7, 7, 7, 3]  # 3 adjacent repeats: needs 10 frames
FEASIBLE_PATH = [5, 0, 5, 6, 7, 0, 7, 0, 7, 3]


def feasibility_case(P, T=16, V=32):
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(2, 1, T, V, generator=g) * 2.0, -1)
    return lp, C.pad_targets(torch.tensor([FEASIBLE_TARGET]), C.WIDTH_FOR_P[P]), torch.tensor([len(FEASIBLE_TARGET)])


def decoder_lens(N, T):
    return torch.tensor([T, 1, 2, T // 2, T - 1, 3, T // 3, T // 2 + 1][:N])


def ref_greedy(logp, lens, blank=0):
    return [R.greedy_ctc(logp[s, : int(n)], blank) if int(n) > 0 else [] for s, n in enumerate(lens)]


def ref_beam(logp_tv, n, beam, blank=0, thr=0.95, drop=False):
    """(tokens, score, final beams) of the oracle on the first n frames; no frame: the empty prefix with log-probability 0."""
    if int(n) <= 0:
        return [], 0.0, [((), 0.0)]
    return ctc_prefix_beam_search(logp_tv[: int(n)].double().numpy(), beam=beam, blank=blank, blank_skip_threshold=thr,
                                  return_beams=True, skip_drops_frame=drop)


def safe_share(N, T, V, beam, scale):
    """How many of a BEAM_CASES entry's sliced sequences are margin-safe, per skip reading: {drop: count}."""
    logp, lens = C.beam_logp(N, T, V, scale), decoder_lens(N, T)
    return {drop: sum(C.safe_margin(ref_beam(logp[s], lens[s], beam, drop=drop)[2]) for s in range(N)) for drop in (False, True)}
