"""Keyword and phrase spotting on CTC emissions (include/eec.h, "Keyword spotting on CTC emissions"; csrc/keyword.hip): does an
emission contain one of a set of phrases, and where -- without decoding the utterance.  ``KeywordSet`` holds the phrases as token rows,
``keyword_search`` scores every (emission, keyword) pair in two launches (``eec_keyword_search``; CPU tensors take a NumPy host path
of the same statement, bit-identical to the kernel), ``KeywordHits`` turns the per-frame trace into non-overlapping detections and
the per-exit scores into the shallowest exit that hits.  Scores are max-over-paths: 0.0 means greedy decoding spells the phrase."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import capi

MAX_TOKENS = 64       # tokens of one keyword
MAX_KEYWORDS = 65536  # keywords of one set
MAX_FRAMES = 1 << 20  # T'


class KeywordSet:
    """``phrases``: 1 .. 65536 rows of 1 .. 64 token ids of [0, vocab_size), none of them ``blank``.  Adjacent equal tokens are
    legal (they need a blank frame between them).  ``tokens`` [K, longest] int32 (rows padded with 0) and ``lengths`` [K] int32 are
    the table the kernel reads; this class is its one maker and refuses what the kernel could only answer with fill values."""

    def __init__(self, phrases: Sequence[Sequence[int]], vocab_size: int, blank: int = 0):
        rows = [[int(t) for t in p] for p in phrases]
        V, blank = int(vocab_size), int(blank)
        if V < 2 or not 0 <= blank < V:
            raise ValueError(f"KeywordSet: needs vocab_size >= 2 and blank in [0, vocab_size), got {V} and {blank}")
        if not 1 <= len(rows) <= MAX_KEYWORDS:
            raise ValueError(f"KeywordSet: 1 .. {MAX_KEYWORDS} keywords, got {len(rows)}")
        for k, row in enumerate(rows):
            if not 1 <= len(row) <= MAX_TOKENS:
                raise ValueError(f"KeywordSet: a keyword has 1 .. {MAX_TOKENS} tokens, keyword {k} has {len(row)}")
            for t in row:
                if t == blank:
                    raise ValueError(f"KeywordSet: keyword {k} holds the blank ({blank})")
                if not 0 <= t < V:
                    raise ValueError(f"KeywordSet: keyword {k} holds token {t}, outside [0, {V})")
        self.vocab_size, self.blank = V, blank
        self.lengths = np.asarray([len(r) for r in rows], dtype=np.int32)
        self.tokens = np.zeros((len(rows), int(self.lengths.max())), dtype=np.int32)
        for k, row in enumerate(rows):
            self.tokens[k, :len(row)] = row
        self._on = {}

    @classmethod
    def from_texts(cls, texts: Sequence[str], encode: Callable[[str], Sequence[int]], vocab_size: int, blank: int = 0) -> "KeywordSet":
        """The set of ``encode(text)`` for every text: ``encode`` is a tokenizer's text -> ids callable."""
        return cls([list(encode(t)) for t in texts], vocab_size, blank)

    def __len__(self) -> int:
        return int(self.lengths.size)

    def phrase(self, k: int) -> List[int]:
        return self.tokens[k, :int(self.lengths[k])].tolist()

    def to(self, device) -> Tuple[Tensor, Tensor]:
        """(tokens, lengths) on ``device``, uploaded once per device and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = (torch.from_numpy(self.tokens).to(device), torch.from_numpy(self.lengths).to(device))
        return self._on[device]


@dataclass
class KeywordHits:
    """What ``keyword_search`` returns, over the leading shape of its input ([n_em] or [E, B]):
    ``score`` [..., K] fp32 the best segment's score (at most 0; -inf: the keyword does not fit), ``start`` / ``end`` [..., K] int32
    its first and last frame (-1 with no segment); with ``want_trace`` ``trace_score`` / ``trace_start`` [..., K, T']: the best score
    of a segment ending at each frame and that segment's first frame (-inf / -1 past the emission's length), else None."""
    score: Tensor
    start: Tensor
    end: Tensor
    trace_score: Optional[Tensor] = None
    trace_start: Optional[Tensor] = None

    def _thresholds(self, threshold) -> np.ndarray:
        K = self.score.size(-1)
        thr = np.asarray(threshold, dtype=np.float64).reshape(-1)
        if thr.size not in (1, K):
            raise ValueError(f"threshold: one float or one per keyword ({K}), got {thr.size}")
        if np.isnan(thr).any():
            raise ValueError("threshold is NaN")
        return np.broadcast_to(thr, (K,))

    def detections(self, threshold: Union[float, Sequence[float]]):
        """Non-overlapping occurrences per (emission, keyword), on the host from the trace: the candidates are the end frames with
        ``trace_score >= threshold`` (a float, or one per keyword), taken by score descending, then end ascending; a candidate is
        accepted if its segment [start, end] meets no accepted one.  Returns nested lists over the leading shape and the keywords,
        ``out[n][k]`` or ``out[e][b][k]``: the accepted ``(start, end, score)`` in order of acceptance."""
        if self.trace_score is None:
            raise ValueError("detections needs the trace: keyword_search(..., want_trace=True)")
        thr = self._thresholds(threshold)
        lead = tuple(self.score.shape[:-1])
        K, Tq = self.trace_score.shape[-2:]
        ts = self.trace_score.detach().cpu().numpy().reshape(-1, K, Tq)
        tb = self.trace_start.detach().cpu().numpy().reshape(-1, K, Tq)
        flat = []
        for n in range(ts.shape[0]):
            per_kw = []
            for k in range(K):
                ends = np.nonzero((ts[n, k] >= thr[k]) & (tb[n, k] >= 0))[0]
                ends = ends[np.argsort(-ts[n, k, ends], kind="stable")]  # stable: equal scores stay in ascending end order
                taken: List[Tuple[int, int, float]] = []
                for e in ends.tolist():
                    s = int(tb[n, k, e])
                    if all(e < a or s > b for a, b, _ in taken):
                        taken.append((s, e, float(ts[n, k, e])))
                per_kw.append(taken)
            flat.append(per_kw)
        if len(lead) == 1:
            return flat
        return [flat[e * lead[1]:(e + 1) * lead[1]] for e in range(lead[0])]

    def first_exit(self, threshold: Union[float, Sequence[float]]) -> Tensor:
        """For [E, B, ...] input: the shallowest exit (0-based) whose best score reaches the threshold, int64 [B, K]; -1 if none."""
        if self.score.dim() != 3:
            raise ValueError("first_exit needs the scores of [E, B, T', V] emissions")
        thr = torch.as_tensor(self._thresholds(threshold).copy(), dtype=torch.float64, device=self.score.device)
        hit = self.score.double() >= thr  # [E, B, K]
        first = hit.to(torch.int64).argmax(dim=0)
        return torch.where(hit.any(dim=0), first, torch.full_like(first, -1))


def _host_search(x: np.ndarray, lens: np.ndarray, kw: KeywordSet, want_trace: bool):
    """The header's statement over [n, K, S] arrays, one step per frame: fp32 subtract, add and compare in its order."""
    n, Tq, V = x.shape
    K, S = len(kw), 2 * kw.tokens.shape[1] - 1
    NEG = np.float32(-np.inf)
    lab = np.full((K, S), kw.blank, dtype=np.int64)
    lab[:, 0::2] = kw.tokens
    s_idx = np.arange(S)[None, :]
    inside = s_idx <= 2 * kw.lengths.astype(np.int64)[:, None] - 2
    lab = np.where(inside, lab, kw.blank)  # states past the last one compute on the blank and feed nothing
    skip = np.zeros((K, S), dtype=bool)
    skip[:, 2::2] = lab[:, 2::2] != lab[:, :-2:2]
    skip &= inside & (s_idx % 2 == 0)
    last = (2 * kw.lengths.astype(np.int64) - 2)[None, :, None]  # [1, K, 1]
    d = np.full((n, K, S), NEG, dtype=np.float32)
    st = np.full((n, K, S), -1, dtype=np.int32)
    best = np.full((n, K), NEG, dtype=np.float32)
    b_start = np.full((n, K), -1, dtype=np.int32)
    b_end = np.full((n, K), -1, dtype=np.int32)
    t_score = np.full((n, K, Tq), NEG, dtype=np.float32) if want_trace else None
    t_start = np.full((n, K, Tq), -1, dtype=np.int32) if want_trace else None
    minus1 = np.int32(-1)
    with np.errstate(invalid="ignore"):
        for t in range(int(lens.max()) if n else 0):
            act = lens > t
            xt = np.where(act[:, None], x[:, t, :], np.float32(0))  # a frame past a length is not read
            m = xt.max(axis=1)
            fin = np.isfinite(m)[:, None, None]
            e = np.where(fin, xt[:, lab] - m[:, None, None], NEG).astype(np.float32)
            c, cs = d.copy(), st.copy()
            p1 = np.concatenate([np.full((n, K, 1), NEG, np.float32), d[:, :, :-1]], axis=2)
            s1 = np.concatenate([np.full((n, K, 1), -1, np.int32), st[:, :, :-1]], axis=2)
            take = p1 > c
            c, cs = np.where(take, p1, c), np.where(take, s1, cs)
            if S > 2:
                p2 = np.concatenate([np.full((n, K, 2), NEG, np.float32), d[:, :, :-2]], axis=2)
                s2 = np.concatenate([np.full((n, K, 2), -1, np.int32), st[:, :, :-2]], axis=2)
                take = skip[None] & (p2 > c)
                c, cs = np.where(take, p2, c), np.where(take, s2, cs)
            fresh = np.float32(0) > c[:, :, 0]
            c[:, :, 0] = np.where(fresh, np.float32(0), c[:, :, 0])
            cs[:, :, 0] = np.where(fresh, np.int32(t), cs[:, :, 0])
            nd = (c + e).astype(np.float32)
            ns = np.where(nd == NEG, minus1, cs).astype(np.int32)
            d = np.where(act[:, None, None], nd, d)
            st = np.where(act[:, None, None], ns, st)
            fv = np.take_along_axis(d, last, axis=2)[:, :, 0]
            fs = np.take_along_axis(st, last, axis=2)[:, :, 0]
            up = act[:, None] & (fv > best)
            best = np.where(up, fv, best)
            b_start = np.where(up, fs, b_start)
            b_end = np.where(up, np.int32(t), b_end)
            if want_trace:
                t_score[:, :, t] = np.where(act[:, None], fv, NEG)
                t_start[:, :, t] = np.where(act[:, None], fs, minus1)
    return best, b_start, b_end, t_score, t_start


def _host_path(logp: Tensor, lens: Optional[Tensor], kw: KeywordSet, want_trace: bool):
    x = logp.detach().numpy()
    n, Tq, _ = x.shape
    ln = np.full(n, Tq, dtype=np.int64) if lens is None else np.clip(lens.numpy().astype(np.int64), 0, Tq)
    step = max(1, (1 << 22) // max(1, len(kw) * (2 * kw.tokens.shape[1] - 1)))  # bounds the [n, K, S] temporaries
    parts = [_host_search(x[i:i + step], ln[i:i + step], kw, want_trace) for i in range(0, n, step)]
    return [None if parts[0][j] is None else torch.from_numpy(np.concatenate([p[j] for p in parts])) for j in range(5)]


def _device_path(logp: Tensor, lens: Optional[Tensor], kw: KeywordSet, want_trace: bool, max_workspace_bytes: int):
    dev = logp.device
    n, Tq, V = logp.shape
    K = len(kw)
    tokens, lengths = kw.to(dev)
    ws_bytes = capi.load().eec_keyword_search_workspace_bytes(n, Tq)
    ws, ws_ptr = capi.aligned_ws(ws_bytes, dev)
    # a call whose trace would not fit the budget is split over keywords: a wave's result depends on its own keyword alone
    Kc = K if not want_trace else max(1, min(K, int(max_workspace_bytes) // max(1, n * Tq * 8)))
    parts = []
    for k0 in range(0, K, Kc):
        kc = min(Kc, K - k0)
        score = torch.empty((n, kc), dtype=torch.float32, device=dev)
        start = torch.empty((n, kc), dtype=torch.int32, device=dev)
        end = torch.empty((n, kc), dtype=torch.int32, device=dev)
        t_score = torch.empty((n, kc, Tq), dtype=torch.float32, device=dev) if want_trace else None
        t_start = torch.empty((n, kc, Tq), dtype=torch.int32, device=dev) if want_trace else None
        capi.launch("eec_keyword_search", dev, logp, n, Tq, V, lens, tokens[k0:k0 + kc], lengths[k0:k0 + kc], kc, tokens.size(1), kw.blank,
                    score, start, end, t_score, t_start, ws_ptr, ws_bytes)
        parts.append((score, start, end, t_score, t_start))
    if len(parts) == 1:
        return list(parts[0])
    return [None if parts[0][j] is None else torch.cat([p[j] for p in parts], dim=1) for j in range(5)]


def keyword_search(logp: Tensor, keywords: KeywordSet, em_len: Optional[Tensor] = None, want_trace: bool = False,
                   max_workspace_bytes: int = 2 << 30) -> KeywordHits:
    """Every keyword against every emission.  ``logp`` [n_em, T', V] or [E, B, T', V] fp32, log-probs or logits (the score is
    invariant to a per-frame shift); ``em_len`` int32 / int64 frames per emission -- [n_em], or for [E, B, ...] input [B] (shared by
    the exits) or [E, B] --, clamped to [0, T'], None: T' for all.  Frames from a length on are never read.  Device tensors: two
    launches on the current stream, nothing read back, graph-capturable; CPU tensors: a NumPy host path with the same bits.  The
    trace ([..., K, T'] fp32 and int32) is returned with ``want_trace``; a call whose trace would exceed ``max_workspace_bytes`` is
    split over keywords."""
    if not isinstance(keywords, KeywordSet):
        raise TypeError("keyword_search: keywords must be a KeywordSet")
    if logp.dim() not in (3, 4):
        raise ValueError(f"keyword_search: logp must be [n_em, T', V] or [E, B, T', V], got {tuple(logp.shape)}")
    if logp.dtype != torch.float32:
        raise ValueError(f"keyword_search: logp must be fp32, got {logp.dtype}")
    lead = tuple(logp.shape[:-2])
    Tq, V = int(logp.size(-2)), int(logp.size(-1))
    if V != keywords.vocab_size:
        raise ValueError(f"keyword_search: the keywords are over {keywords.vocab_size} tokens, logp has {V}")
    if not 1 <= Tq <= MAX_FRAMES:
        raise ValueError(f"keyword_search: T' must be in 1 .. 2^20, got {Tq}")
    n = int(np.prod(lead))
    if n < 1:
        raise ValueError("keyword_search: no emissions")
    flat = logp.reshape(n, Tq, V)
    if not flat.is_contiguous():
        flat = flat.contiguous()
    lens = None
    if em_len is not None:
        lens = torch.as_tensor(em_len)
        if lens.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"keyword_search: em_len must be an int32 or int64 tensor, got {lens.dtype}")
        if len(lead) == 2 and lens.numel() == lead[1] and lead[0] != 1:
            lens = lens.reshape(1, lead[1]).expand(lead[0], lead[1])
        if lens.numel() != n:
            raise ValueError(f"keyword_search: em_len must have {n} entries" + (f" or {lead[1]}" if len(lead) == 2 else "") +
                             f", got {lens.numel()}")
        lens = lens.to(torch.int64).clamp(0, Tq).reshape(n).to(device=logp.device, dtype=torch.int32).contiguous()
    if logp.is_cuda:
        out = _device_path(flat, lens, keywords, want_trace, max_workspace_bytes)
    else:
        out = _host_path(flat, lens, keywords, want_trace)
    K = len(keywords)
    shaped = [None if t is None else t.reshape(*lead, K, *t.shape[2:]) for t in out]
    return KeywordHits(*shaped)
