"""Token posteriors and soft timestamps from CTC emissions (include/eec.h, "CTC posteriors, standard topology";
csrc/ctc_posterior.hip): how sure the model is of each token of a transcript summed over EVERY alignment, where the token begins
and ends in expectation, and how uncertain those boundaries are.  ``ctc_posteriors`` is the forward-backward occupancy of the
lattice ``ctc_forced_align`` takes the best path of, in one launch (``eec_ctc_posteriors``); ``Posteriors.spans`` turns a row into
soft token spans, ``soft_word_spans`` merges those into words, ``nbest_posteriors`` turns the rows' log-likelihoods into the
utterance-level confidence of an N-best list.

Not served: a star / wildcard token; rows over 255 tokens; posteriors inside the lexicon decoders; alpha checkpointing to shrink
the workspace (it is one 256-byte line per frame and slot of the state strip: T' * C * 256 bytes a row); a backward -- the outputs
are analysis, not a loss."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .alignment import group_words, host_lattice, host_row_checks, launch_rows, row_arguments

TOKEN_FIELDS = ("tok_frames", "tok_score", "tok_start", "tok_end", "tok_start_var", "tok_end_var")


class SoftSpan(NamedTuple):
    """``token`` id; ``start`` / ``end`` the expected first frame and the expected last frame plus 1 over all alignments, with their
    standard deviations ``start_sd`` / ``end_sd`` (frames, or seconds with ``frame_seconds``); ``frames`` the expected number of
    frames the token holds (end - start, always in frames); ``confidence`` = exp(tok_score / tok_frames), the posterior-weighted
    geometric mean of the token's frame posteriors."""
    token: int
    start: float
    end: float
    start_sd: float
    end_sd: float
    frames: float
    confidence: float


class SoftWordSpan(NamedTuple):
    tokens: tuple
    start: float
    end: float
    start_sd: float
    end_sd: float
    confidence: float


@dataclass
class Posteriors:
    """What ``ctc_posteriors`` returns for H rows of at most S tokens.  ``row_logp`` [H] fp32 the log-likelihood of the row summed
    over all alignments; per token [H, S] fp32 ``tok_frames`` (expected frames), ``tok_score`` (posterior-weighted sum of its
    emissions), ``tok_start`` / ``tok_end`` (expected first frame, expected last frame plus 1) and ``tok_start_var`` /
    ``tok_end_var`` (their variances, in frames squared); ``gamma`` [H, T', S] fp32 the occupancy of token j at frame t, or None;
    ``status`` [H] int32 (0: served, 1: not alignable, 2: no alignment of finite likelihood).  Past a row's length and in rows
    with another status than 0 the token outputs are -1, ``row_logp`` is -inf and ``gamma`` is 0.  ``tokens`` / ``tok_len``: the
    rows as the kernel read them."""
    row_logp: Tensor
    tok_frames: Tensor
    tok_score: Tensor
    tok_start: Tensor
    tok_end: Tensor
    tok_start_var: Tensor
    tok_end_var: Tensor
    gamma: Optional[Tensor]
    status: Tensor
    tokens: Optional[Tensor] = None
    tok_len: Optional[Tensor] = None

    def spans(self, h: int, frame_seconds: Optional[float] = None) -> List[SoftSpan]:
        """The soft spans of row ``h``, in order; [] for a row whose status is not 0.  ``confidence`` and the standard deviations
        (the square root of a variance, a slightly negative one taken as 0) are evaluated in fp64.  With ``frame_seconds`` the
        boundaries and their deviations are seconds (see ``Alignment.spans`` for what a frame's time means); ``frames`` stays a
        number of frames."""
        if int(self.status[h]) != 0:
            return []
        n = int(self.tok_len[h])
        ids = self.tokens[h, :n].tolist()
        fr, sc, a, b, va, vb = (getattr(self, name)[h, :n].double().tolist() for name in TOKEN_FIELDS)
        k = 1.0 if frame_seconds is None else float(frame_seconds)
        return [SoftSpan(ids[j], a[j] * k, b[j] * k, math.sqrt(max(va[j], 0.0)) * k, math.sqrt(max(vb[j], 0.0)) * k, fr[j],
                         math.exp(sc[j] / fr[j]) if fr[j] > 0.0 else 0.0) for j in range(n)]


def soft_word_spans(spans: Sequence[SoftSpan], starts_word: Union[Sequence[bool], Callable[[int], bool]]) -> List[SoftWordSpan]:
    """Soft token spans merged into words, on the host, by ``word_spans``' rule: a token for which ``starts_word`` (a bool array over
    the vocabulary -- ``starts_word_from_pieces`` makes one --, or a callable on the id) holds opens a word, as does the first
    token.  A word runs from its first token's start (and deviation) to its last token's end; its confidence is
    exp(sum of scores / sum of frames) in fp64, a token's score being frames * log(confidence)."""
    out = []
    for g in group_words(spans, starts_word):
        frames = math.fsum(sp.frames for sp in g)
        dead = frames <= 0.0 or any(sp.confidence <= 0.0 and sp.frames > 0.0 for sp in g)
        conf = 0.0 if dead else math.exp(math.fsum(sp.frames * math.log(sp.confidence) for sp in g if sp.frames > 0.0) / frames)
        out.append(SoftWordSpan(tuple(sp.token for sp in g), g[0].start, g[-1].end, g[0].start_sd, g[-1].end_sd, conf))
    return out


def nbest_posteriors(row_logp, group) -> Tensor:
    """The utterance-level confidence of an N-best list: the softmax of ``row_logp`` [H] over the rows that share a ``group`` [H]
    id (the utterance of every hypothesis), in fp64 on the host.  A row of -inf (status 1 or 2) gets 0; a group with no finite
    row gets 0 throughout.  Returns fp64 [H]."""
    lp = torch.as_tensor(row_logp).detach().reshape(-1).double().cpu().numpy()
    grp = torch.as_tensor(group).reshape(-1).cpu().numpy()
    if lp.shape != grp.shape:
        raise ValueError(f"nbest_posteriors: {lp.size} rows, {grp.size} group ids")
    out = np.zeros_like(lp)
    _, inv = np.unique(grp, return_inverse=True)
    live = np.isfinite(lp)
    top = np.full(int(inv.max()) + 1 if inv.size else 0, -np.inf)
    np.maximum.at(top, inv[live], lp[live])
    w = np.zeros_like(lp)
    w[live] = np.exp(lp[live] - top[inv[live]])
    tot = np.zeros_like(top)
    np.add.at(tot, inv, w)
    np.divide(w, tot[inv], out=out, where=tot[inv] > 0.0)
    return torch.from_numpy(out)


def _host_rows(x: np.ndarray, T: np.ndarray, ei: np.ndarray, y: np.ndarray, N: np.ndarray, blank: int, want_gamma: bool):
    """The header's statement in fp64 for K rows that passed its row checks, one step per frame over [K, 2S + 1] states.  ``x``
    [n_em, T', V], ``T`` / ``ei`` / ``N`` [K], ``y`` [K, S] (blank past N).  Returns ``(ll [K], sums [6, K, S], gamma [K, T', S] or
    None)``; a row whose ll is not finite holds unspecified sums."""
    K, S = y.shape
    Tq = x.shape[1]
    NS = 2 * S + 1
    NEG = -np.inf
    rows = np.arange(K)
    s_idx = np.arange(NS)[None, :]
    lab, skip, skipn, valid = host_lattice(y, N, blank)
    t_max = int(T.max())

    def emit(t):
        return np.take_along_axis(x[ei, min(t, Tq - 1), :].astype(np.float64), lab, axis=1)

    def from_left(v, n):
        return np.concatenate([np.full((K, n), NEG), v[:, :-n]], axis=1)

    def from_right(v, n):
        return np.concatenate([v[:, n:], np.full((K, n), NEG)], axis=1)

    alpha = np.full((t_max, K, NS), NEG)
    a = np.full((K, NS), NEG)
    e0 = emit(0)
    a[:, 0], a[:, 1] = e0[:, 0], e0[:, 1]
    alpha[0] = a
    for t in range(1, t_max):
        v = np.logaddexp(np.logaddexp(a, from_left(a, 1)), np.where(skip, from_left(a, 2), NEG))
        a = np.where((T > t)[:, None], np.where(valid, v + emit(t), NEG), a)  # a row past its length: kept, its last frame is read below
        alpha[t] = a
    last = alpha[T - 1, rows]
    ll = np.logaddexp(last[rows, 2 * N], last[rows, 2 * N - 1])
    sums = np.zeros((6, K, S))
    gamma = np.zeros((K, Tq, S)) if want_gamma else None
    init = np.where((s_idx == 2 * N[:, None]) | (s_idx == 2 * N[:, None] - 1), 0.0, NEG)
    c = np.full((K, NS), NEG)  # c_{t+1}(s) = x_{t+1}(lab(s)) + beta_{t+1}(s)
    lln = ll[:, None]
    for t in range(t_max - 1, -1, -1):
        act, end = (T > t)[:, None], (T - 1 == t)[:, None]
        e = emit(t)
        one, two = from_right(c, 1), np.where(skipn, from_right(c, 2), NEG)
        beta = np.where(end, init, np.logaddexp(np.logaddexp(c, one), two))
        leave = np.logaddexp(one, two)
        g = np.exp(alpha[t] + beta - lln)
        if t >= 1:
            enter = np.logaddexp(from_left(alpha[t - 1], 1), np.where(skip, from_left(alpha[t - 1], 2), NEG))
            f = np.exp(enter + e + beta - lln)
        else:
            f = np.where(s_idx == 1, g, 0.0)
        l = np.where(end, g, np.exp(alpha[t] + leave - lln))
        g, f, l, ex = (np.where(act & valid, v, 0.0)[:, 1::2] for v in (g, f, l, e))
        sums[0] += g
        sums[1] += np.where(g > 0.0, g * ex, 0.0)
        sums[2] += t * f
        sums[3] += float(t) * t * f
        sums[4] += (t + 1) * l
        sums[5] += float(t + 1) * (t + 1) * l
        if want_gamma:
            gamma[:, t, :] = g
        c = np.where(act & valid, e + beta, NEG)
    return ll, sums, gamma


def _host_posteriors(x, lens, tokens, tok_len, em_index, blank: int, want_gamma: bool):
    n_em, Tq, V = x.shape
    H, S = tokens.shape
    row_logp = np.full((H,), -np.inf, dtype=np.float32)
    tok = np.full((6, H, S), -1.0, dtype=np.float32)
    gamma = np.zeros((H, Tq, S), dtype=np.float32) if want_gamma else None
    status = np.ones((H,), dtype=np.int32)
    ok, N, ei, inside, tk, T_all = host_row_checks(x.shape, lens, tokens, tok_len, em_index, blank)
    keep = np.nonzero(ok)[0]
    step = max(1, (1 << 24) // max(1, Tq * (2 * S + 1)))  # bounds the [T, K, 2S + 1] alpha
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c0 in range(0, keep.size, step):
            r = keep[c0:c0 + step]
            ll, sums, g = _host_rows(x, T_all[ei[r]], ei[r], np.where(inside[r], tk[r], blank), N[r], blank, want_gamma)
            good = np.isfinite(ll)
            status[r] = np.where(good, 0, 2)
            rg = r[good]
            row_logp[rg] = ll[good]
            sums = sums[:, good]
            sums[3] -= sums[2] * sums[2]
            sums[5] -= sums[4] * sums[4]
            tok[:, rg] = np.where(inside[rg][None], sums[[0, 1, 2, 4, 3, 5]], -1.0)
            if want_gamma:
                gamma[rg] = g[good]
    return (row_logp, *tok, gamma, status)


def _device_posteriors(logp: Tensor, lens, tokens: Tensor, tok_len: Tensor, em_index, blank: int, want_gamma: bool,
                       max_workspace_bytes: int):
    dev, Tq = logp.device, logp.size(1)
    H, S = tokens.shape
    row_logp = torch.empty((H,), dtype=torch.float32, device=dev)
    tok = [torch.empty((H, S), dtype=torch.float32, device=dev) for _ in TOKEN_FIELDS]
    gamma = torch.empty((H, Tq, S), dtype=torch.float32, device=dev) if want_gamma else None
    status = torch.empty((H,), dtype=torch.int32, device=dev)
    launch_rows("eec_ctc_posteriors", logp, lens, tokens, tok_len, em_index, blank, (row_logp, *tok, gamma, status), max_workspace_bytes)
    return (row_logp, *tok, gamma, status)


def ctc_posteriors(logp: Tensor, tokens: Tensor, tok_len: Optional[Tensor] = None, em_index: Optional[Tensor] = None,
                   em_len: Optional[Tensor] = None, blank: int = 0, want_gamma: bool = False,
                   max_workspace_bytes: int = 2 << 30) -> Posteriors:
    """Forward-backward posteriors of H token rows in the standard CTC topology (the statement: include/eec.h).  The arguments are
    ``ctc_forced_align``'s: ``logp`` [n_em, T', V] or [E, B, T', V] fp32 log-probs; ``tokens`` [H, S] of any integer dtype with
    ``tok_len`` [H] labels each (None: S), S <= 255; ``em_index`` [H] the emission of every row -- e * B + b for [E, B, ...] input --
    (None: its own index); ``em_len`` frames per emission, int32 / int64 -- [n_em], or for [E, B, ...] input [B] (shared by the
    exits) or [E, B] --, clamped to [0, T'], None: T' for all.  Frames from a length on are never read.  ``want_gamma``: also the
    occupancy [H, T', S].  A row that fails ``ctc_forced_align``'s row checks has status 1, a row without an alignment of finite
    likelihood (-inf emissions on every path) status 2; both hold the fill values.  Device tensors: one launch on the current
    stream, nothing read back, graph-capturable; a call whose alpha lines (``eec_ctc_posteriors_workspace_bytes``) exceed
    ``max_workspace_bytes`` is split over rows, which changes no bit.  CPU tensors take a vectorised NumPy host path in FP64,
    rounded once to fp32: the same definition, NOT the same bits as the kernel, whose recursions are fp32 (the two agree within
    the bound the header states)."""
    flat, lens, tokens, tok_len, em_index, blank = row_arguments("ctc_posteriors", logp, tokens, tok_len, em_index, em_len, blank)
    if logp.is_cuda:
        out = _device_posteriors(flat, lens, tokens, tok_len, em_index, blank, bool(want_gamma), max_workspace_bytes)
    else:
        out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)) for a in _host_posteriors(
            flat.detach().numpy(), None if lens is None else lens.numpy(), tokens.numpy(), tok_len.numpy(),
            None if em_index is None else em_index.numpy(), blank, bool(want_gamma))]
    return Posteriors(*out, tokens=tokens, tok_len=tok_len)
