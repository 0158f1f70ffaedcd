"""Inputs and the reference shared by tests/test_host_distill.py and tests/test_gpu_distill.py (self-distillation between exits:
csrc/distill.hip behind eec_exit_distill_forward / _backward).  Everything here is seeded and runs on the CPU; nothing is read
but the committed fixture tests/golden/config1_peaky.npz (through ctc_cases).

Reference: the definition of include/eec.h written with torch.log_softmax -- with p = softmax(x[k] / tau), q = softmax(x[e] / tau),
k = teacher[e], the teacher detached:
    kl[e, b] = sum_{t < len_b} sum_v p_v (log p_v - log q_v),     loss[e] = tau^2 * mean_b( kl[e, b] / max(len_b, 1) )
evaluated in fp64, its gradient by autograd (``dtype=torch.float32`` gives the statement's own fp32 result: the yardstick err32).
"""
import torch

import ctc_cases as CC

TAUS = (0.5, 1.0, 2.0)
LEN_CYCLE = ("T", 1, 7, 0)


def teacher_map(teacher, E):
    if teacher == "last":
        return [E - 1] * (E - 1) + [-1]
    if teacher == "next":
        return list(range(1, E)) + [-1]
    return [int(k) for k in teacher]


def cycle_lens(B, T):
    """frame_len cycling [T, 1, 7, 0] over the batch."""
    return torch.tensor([T if LEN_CYCLE[b % 4] == "T" else LEN_CYCLE[b % 4] for b in range(B)], dtype=torch.int64)


def frame_mask(frame_len, B, T):
    """(mask [B, T] bool, max(len, 1) [B]) with the lengths clamped to [0, T]; None: T everywhere."""
    lens = torch.full((B,), T, dtype=torch.int64) if frame_len is None else torch.as_tensor(frame_len).cpu().to(torch.int64).clamp(0, T)
    return torch.arange(T).view(1, T) < lens.view(B, 1), lens.clamp(min=1)


def torch_distill(x, frame_len, teacher, tau):
    """The losses [E] as a differentiable function of ``x`` (any float dtype, any device), teachers detached."""
    E, B, T, _ = x.shape
    mask, denom = frame_mask(frame_len, B, T)
    mask, denom = mask.to(x.device), denom.to(device=x.device, dtype=x.dtype)
    losses = []
    for e, k in enumerate(teacher_map(teacher, E)):
        if k < 0:
            losses.append(x.new_zeros(()))
            continue
        lp = torch.log_softmax(x[k].detach() / tau, -1)
        lq = torch.log_softmax(x[e] / tau, -1)
        per_frame = (lp.exp() * (lp - lq)).sum(-1)  # [B, T]
        kl = torch.where(mask, per_frame, torch.zeros_like(per_frame)).sum(-1)
        losses.append(tau * tau * (kl / denom).mean())
    return torch.stack(losses)


def ref_distill(x, frame_len, teacher, tau, dtype=torch.float64, w=None):
    """(losses [E], d(sum_e w_e loss_e)/dx) of the definition in ``dtype`` on the CPU."""
    xx = x.detach().cpu().clone().to(dtype).requires_grad_(True)
    losses = torch_distill(xx, frame_len, teacher, tau)
    ww = torch.ones(x.size(0), dtype=dtype) if w is None else w.detach().cpu().to(dtype)
    total = (losses * ww).sum()
    if total.requires_grad:
        total.backward()
    grad = xx.grad if xx.grad is not None else torch.zeros_like(xx)
    return losses.detach(), grad


def closed_form_grad(x, frame_len, teacher, tau, dtype=torch.float64, w=None):
    """The gradient as include/eec.h states it, without autograd:
    d(sum_e w_e loss_e) / dx[e, b, t, :] = w_e * tau * (q - p) / (B * max(len_b, 1)) for t < len_b, else 0; teachers get none."""
    xx = x.detach().cpu().to(dtype)
    E, B, T, _ = xx.shape
    mask, denom = frame_mask(frame_len, B, T)
    ww = torch.ones(E, dtype=dtype) if w is None else w.to(dtype)
    g = torch.zeros_like(xx)
    for e, k in enumerate(teacher_map(teacher, E)):
        if k < 0:
            continue
        q, p = torch.softmax(xx[e] / tau, -1), torch.softmax(xx[k] / tau, -1)
        scale = ww[e] * tau / (B * denom.to(dtype))  # [B]
        g[e] = torch.where(mask.unsqueeze(-1), scale.view(B, 1, 1) * (q - p), torch.zeros_like(q))
    return g


_INPUTS = None


def inputs():
    """name -> x [E, B, T, V] fp32, built once: peaky log-probs at logit scales 1, 8, 16 ([3, 3, 19, 256]) and the committed
    trained-like fixture ([6, 4, 16, 256])."""
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = {f"scale{s:g}": CC.peaky_logp(s, E=3, B=3, T=19) for s in (1.0, 8.0, 16.0)}
        _INPUTS["fixture"] = CC.fixture_logp()
    return _INPUTS


def cases():
    """[(name, x, frame_len, teacher, tau)]: every input at every temperature with ragged lengths [T, 1, 7, 0, ...] and the last
    exit as the teacher; the fixture also with every exit learning from the next one and without lengths."""
    out = []
    for name, x in inputs().items():
        _, B, T, _ = x.shape
        for tau in TAUS:
            out.append((f"{name}-tau{tau:g}-last", x, cycle_lens(B, T), "last", tau))
    x = inputs()["fixture"]
    out.append(("fixture-tau2-next", x, cycle_lens(x.size(1), x.size(2)), "next", 2.0))
    out.append(("fixture-tau1-last-nolen", x, None, "last", 1.0))
    return out


_REFS = {}


def reference(name):
    """(case, (loss64, grad64), (loss32, grad32)) of the case ``name``, unweighted; computed once and shared."""
    if name not in _REFS:
        case = next(c for c in cases() if c[0] == name)
        _REFS[name] = (case, ref_distill(*case[1:], dtype=torch.float64), ref_distill(*case[1:], dtype=torch.float32))
    return _REFS[name]


def loss_bound(want, err32):
    return torch.maximum(2e-5 + 2e-5 * want.abs(), 2 * err32)


def grad_bound(scale, gerr32):
    return max(1e-5 * scale + 1e-9, 2 * gerr32)
