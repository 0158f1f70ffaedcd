"""Inputs and the fp64 restatement shared by tests/test_host_mwer.py and tests/test_gpu_mwer.py (MWER training of the CTC exits:
csrc/ctc_mwer.hip behind eec_ctc_hyp_logp / eec_ctc_mwer_forward / _backward).  Everything here is seeded and runs on the CPU;
nothing is read but the committed fixture tests/golden/config1_peaky.npz (through ctc_cases).

The restatement is the statement of include/eec.h ("Minimum word error rate training") with explicit alpha and beta recursions in
NumPy log space -- written without the kernel and without torch's ctc_loss, which the host test compares it against.
``dtype=np.float32`` evaluates the same statement in fp32: the yardsticks err32 / gerr32 of the GPU bounds.
"""
import numpy as np
import torch

import ctc_cases as CC
from distill_cases import cycle_lens

N_LIST = 4
SCALES = (2.0, 8.0, 16.0)
NINF = -np.inf


def _shift(a, k):
    """a[s - k] at place s, -inf where there is no such state."""
    pad = np.full(abs(k), NINF, a.dtype)
    return np.concatenate([pad, a])[: a.size] if k > 0 else np.concatenate([a, pad])[-k:]


def lattice(lp, tokens, blank=0):
    """(ll, gamma [Tb, V]) of ONE hypothesis against the rows ``lp`` [Tb, V]: the exact CTC log-likelihood and the posterior
    probability that an alignment emits label v at frame t.  gamma is None when ll is -inf.  The backward variable is kept WITHOUT
    its own frame's emission, so nothing is ever subtracted."""
    dt = lp.dtype
    Tb, V = lp.shape
    n = len(tokens)
    if Tb == 0:
        return (dt.type(0.0) if n == 0 else dt.type(NINF)), np.zeros((0, V), dt)
    lab = np.full(2 * n + 1, blank, dtype=np.int64)
    lab[1::2] = tokens
    S = lab.size
    skip = np.zeros(S, dtype=bool)  # state s may be entered from s - 2
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    em = lp[:, lab]  # [Tb, S]
    with np.errstate(invalid="ignore"):
        alpha = np.full((Tb, S), NINF, dt)
        alpha[0, :2] = em[0, :2]
        for t in range(1, Tb):
            a = alpha[t - 1]
            x = np.logaddexp(a, _shift(a, 1))
            x = np.logaddexp(x, np.where(skip, _shift(a, 2), NINF).astype(dt))
            alpha[t] = x + em[t]
        ll = np.logaddexp(alpha[-1, S - 1], alpha[-1, S - 2]) if n else alpha[-1, 0]
        if not np.isfinite(ll):
            return dt.type(ll), None
        bx = np.full((Tb, S), NINF, dt)
        bx[-1, max(S - 2, 0):] = 0.0
        skip_out = np.concatenate([skip, [False, False]])[2:]
        for t in range(Tb - 2, -1, -1):
            b = bx[t + 1] + em[t + 1]
            x = np.logaddexp(b, _shift(b, -1))
            bx[t] = np.logaddexp(x, np.where(skip_out, _shift(b, -2), NINF).astype(dt))
        post = np.exp((alpha + bx) - ll)  # [Tb, S]
    gamma = np.zeros((Tb, V), dt)
    for s in range(S):
        gamma[:, lab[s]] += post[:, s]
    return dt.type(ll), gamma


def entry_ok(tokens, length, L, V, blank):
    """The entry's state: 'absent', 'refused' (a length or label the statement turns into NaN) or 'present'."""
    if length == -1:
        return "absent"
    if length < -1 or length > min(L, 255):
        return "refused"
    if any(v < 0 or v >= V or v == blank for v in tokens[:length]):
        return "refused"
    return "present"


def statement(logp, input_len, hyp, hyp_len, risk, blank=0, dtype=np.float64, w=None):
    """dict(ll [E, B, N], loss_eb [E, B], loss [E], c [E, B, N], grad [E, B, T, V] = d(sum_e w_e loss_e) / d logp) of the statement
    evaluated in ``dtype``."""
    lp = np.asarray(logp.detach().cpu().double().numpy(), dtype=dtype)
    hyp, hyp_len = np.asarray(hyp), np.asarray(hyp_len)
    rk = np.asarray(torch.as_tensor(risk).double().numpy(), dtype=dtype)
    E, B, T, V = lp.shape
    N, L = hyp.shape[2:]
    Tb = np.full(B, T) if input_len is None else np.clip(np.asarray(input_len), 0, T)
    ww = np.ones(E, dtype) if w is None else np.asarray(torch.as_tensor(w).double().numpy(), dtype=dtype)
    ll = np.full((E, B, N), NINF, dtype)
    c = np.zeros((E, B, N), dtype)
    loss_eb = np.zeros((E, B), dtype)
    grad = np.zeros((E, B, T, V), dtype)
    for e in range(E):
        for b in range(B):
            gam, refused = [None] * N, False
            for i in range(N):
                state = entry_ok(list(hyp[e, b, i]), int(hyp_len[e, b, i]), L, V, blank)
                if state == "refused":
                    ll[e, b, i], refused = np.nan, True
                elif state == "present":
                    ll[e, b, i], gam[i] = lattice(lp[e, b, : Tb[b]], list(hyp[e, b, i, : hyp_len[e, b, i]]), blank)
            if refused:
                loss_eb[e, b] = np.nan
                continue
            P = np.isfinite(ll[e, b])
            if not P.any():
                continue
            m = ll[e, b][P].max()
            phat = np.where(P, np.exp(np.where(P, ll[e, b], m) - m), 0).astype(dtype)
            phat = phat / phat.sum()
            rP = rk[e, b][P]
            rbar = rP[0] if (rP == rP[0]).all() else rP.mean()
            r = np.where(P, rk[e, b] - rbar, 0).astype(dtype)
            loss_eb[e, b] = (phat * r).sum()
            c[e, b] = phat * (phat[None, :] * (rk[e, b][:, None] - rk[e, b][None, :])).sum(1)  # = phat (r - loss), without its cancellation
            for i in range(N):
                if P[i] and c[e, b, i] != 0:
                    grad[e, b, : Tb[b]] += (ww[e] / dtype(B)) * c[e, b, i] * gam[i]
    return dict(ll=ll, loss_eb=loss_eb, loss=loss_eb.mean(1), c=c, grad=grad, dW=risk_spread(ll, risk))


def greedy_path(lp_tv, blank=0):
    best = lp_tv.argmax(-1).tolist()
    out, prev = [], None
    for v in best:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def build_lists(logp, input_len, blank=0):
    """(hyp [E, B, 4, L] int32, hyp_len [E, B, 4] int32, risk [E, B, 4] fp32) built on the CPU: the greedy path of the utterance's
    valid frames, the path with one token dropped, with one token substituted, and the empty hypothesis; per (e, b), k = e B + b,
    one slot (k + k // 4) % 4 is replaced when k % 4 is 1 (an absent entry), 2 (an infeasible one: a label repeated until it needs
    more than Tb frames) or 3 (a duplicate of the next slot).  Risks: the host-path ``edit_counts`` distance to the greedy path of
    the LAST exit over all T frames of the utterance."""
    from early_exit_transformer_amd import scoring
    E, B, T, V = logp.shape
    Tb = [T] * B if input_len is None else [int(min(max(int(v), 0), T)) for v in input_len]
    rows, lens = [], []
    for e in range(E):
        for b in range(B):
            k = e * B + b
            g = greedy_path(logp[e, b, : Tb[b]], blank)
            drop = g[: len(g) // 2] + g[len(g) // 2 + 1:]
            sub = list(g)
            if sub:
                v = (sub[-1] + 7) % V
                sub[-1] = v if v != blank else (v + 1) % V
            cand = [g, drop, sub, []]
            ln = [len(h) for h in cand]
            slot = (k + k // 4) % 4
            if k % 4 == 1:
                ln[slot] = -1
            elif k % 4 == 2:
                label = g[0] if g else (blank + 1) % V
                cand[slot] = [label] * ((Tb[b] + 1) // 2 + 1)  # needs 2 n - 1 > Tb frames
                ln[slot] = len(cand[slot])
            elif k % 4 == 3:
                cand[slot] = list(cand[(slot + 1) % 4])
                ln[slot] = len(cand[slot])
            rows += cand
            lens += ln
    L = max([len(h) for h in rows] + [1])
    hyp = torch.zeros((len(rows), L), dtype=torch.int32)
    for j, h in enumerate(rows):
        hyp[j, : len(h)] = torch.tensor(h, dtype=torch.int32)
    hyp_len = torch.tensor(lens, dtype=torch.int32)
    refs = [greedy_path(logp[E - 1, b], blank) for b in range(B)]
    ref = torch.zeros((B, max([len(r) for r in refs] + [1])), dtype=torch.int32)
    for b, r in enumerate(refs):
        ref[b, : len(r)] = torch.tensor(r, dtype=torch.int32)
    ref_of = (torch.arange(E * B, dtype=torch.int32) % B).repeat_interleave(N_LIST)
    dist = scoring.edit_counts(hyp, hyp_len.clamp(min=0), ref, torch.tensor([len(r) for r in refs], dtype=torch.int32), ref_of=ref_of).distance
    return hyp.view(E, B, N_LIST, L), hyp_len.view(E, B, N_LIST), dist.float().view(E, B, N_LIST)


_CASES = None


def cases():
    """name -> (logp [E, B, T, V] fp32, input_len [B] int64, hyp, hyp_len, risk): peaky log-probs at scales 2, 8, 16
    ([2, 3, 19, 256]) and the committed fixture ([6, 4, 16, 256]), lengths cycling [T, 1, 7, 0]."""
    global _CASES
    if _CASES is None:
        _CASES = {}
        inputs = {f"scale{s:g}": CC.peaky_logp(s, E=2, B=3, T=19) for s in SCALES}
        inputs["fixture"] = CC.fixture_logp()
        for name, x in inputs.items():
            il = cycle_lens(x.size(1), x.size(2))
            _CASES[name] = (x, il) + build_lists(x, il)
    return _CASES


CASE_NAMES = [f"scale{s:g}" for s in SCALES] + ["fixture"]
_REFS = {}


def exit_weights(E):
    return torch.linspace(0.5, 1.5, E, dtype=torch.float64)


def reference(name, weighted=False):
    """(case, fp64 statement, fp32 statement) of the case ``name``, unweighted or with ``exit_weights``; computed once and shared."""
    key = (name, weighted)
    if key not in _REFS:
        case = cases()[name]
        w = exit_weights(case[0].size(0)) if weighted else None
        _REFS[key] = (case, statement(*case, dtype=np.float64, w=w), statement(*case, dtype=np.float32, w=w))
    return _REFS[key]


def bounds(want, got32):
    """The bounds of the GPU tests from the fp64 statement ``want`` and its fp32 evaluation ``got32``:
    (ll [E, B, N], loss_eb [E, B], grad [E, B] on the largest element error of the utterance's rows), with dW = ``want['dW']``, the
    spread of the list's risks, and A = 2e-5 + 2e-5 max_i |ll_i|."""
    ll, l32 = want["ll"], got32["ll"].astype(np.float64)
    fin = np.isfinite(ll)
    with np.errstate(invalid="ignore"):
        err32 = np.where(fin, np.abs(l32 - ll), 0.0)
        ll_bound = np.maximum(2e-5 + 2e-5 * np.abs(np.where(fin, ll, 0.0)), 2 * err32)
        A = 2e-5 + 2e-5 * np.where(fin, np.abs(ll), 0.0).max(-1)
        dW = want["dW"]
        loss_bound = np.maximum(dW * A, 2 * np.abs(got32["loss_eb"].astype(np.float64) - want["loss_eb"]))
        gmax = np.abs(want["grad"]).max(axis=(2, 3))
        gerr32 = np.abs(got32["grad"].astype(np.float64) - want["grad"]).max(axis=(2, 3))
        grad_bound = np.maximum(1e-5 * gmax + 2 * dW * A + 1e-9, 2 * gerr32)
    return ll_bound, loss_bound, grad_bound


def risk_spread(ll, risk):
    """dW [E, B]: max - min risk over the present, feasible entries of every list (0 for a list without any)."""
    fin = np.isfinite(ll)
    rk = np.asarray(torch.as_tensor(risk).double().numpy())
    hi = np.where(fin, rk, -np.inf).max(-1)
    lo = np.where(fin, rk, np.inf).min(-1)
    return np.where(fin.any(-1), hi - lo, 0.0)


# descent: the leaf is logits [1, 2, 24, 16] under log_softmax, fixed lists of 4 with distinct risks
DESCENT_LR = 2.0  # checked on the CPU: the fp64 restatement's expected risk decreases at each of the 20 steps (tests/test_host_mwer.py)


def descent_case():
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(1, 2, 24, 16, generator=g, dtype=torch.float64)
    hyp = torch.randint(1, 16, (1, 2, 4, 6), generator=g, dtype=torch.int32)
    hl = torch.tensor([[[6, 5, 4, 3], [3, 6, 2, 5]]], dtype=torch.int32)
    risk = torch.tensor([[[3.0, 1.0, 0.0, 2.0], [0.0, 2.0, 3.0, 1.0]]])
    return logits, hyp, hl, risk


def restatement_trajectory(steps=20, lr=None):
    """The losses of `steps` plain gradient steps on the logits, by the fp64 restatement (the log-softmax backward in NumPy)."""
    logits, hyp, hl, risk = descent_case()
    z = logits.numpy().copy()
    lr = DESCENT_LR if lr is None else lr
    out = []
    for _ in range(steps + 1):
        lp = z - np.logaddexp.reduce(z, axis=-1, keepdims=True)
        st = statement(torch.from_numpy(lp), None, hyp, hl, risk)
        out.append(float(st["loss"].sum()))
        z = z - lr * (st["grad"] - np.exp(lp) * st["grad"].sum(-1, keepdims=True))
    return out
