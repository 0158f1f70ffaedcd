"""Word and token timestamps from CTC emissions (include/eec.h, "CTC forced alignment, standard topology";
csrc/ctc_forced_align.hip): when each token of a transcript was said, for how long and how surely.  ``ctc_forced_align`` is the
Viterbi path of token rows through the real CTC topology (2N + 1 states, optional blanks, a blank forced between equal neighbours)
in one launch (``eec_ctc_forced_align``; CPU tensors take a NumPy host path of the same statement, bit-identical to the kernel);
``Alignment.spans`` turns a row into token spans with a confidence, ``word_spans`` merges those into words.  ``ctc_align`` in ctc.py
is the reference's one-frame-per-token trellis and has neither durations nor spans."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import capi
from .ctc import _frame_counts

MAX_TOKENS = 255      # tokens of one row
FRAME_SECONDS = 0.04  # 4 * hop_length / sample_rate at the front end's defaults (160 / 16000): the stem's stride times the hop


class TokenSpan(NamedTuple):
    """``token`` id, ``start`` / ``end`` (end exclusive; frames, or seconds with ``frame_seconds``), ``score`` the summed emission
    of the token's ``frames`` frames, ``confidence`` = exp(score / frames)."""
    token: int
    start: Union[int, float]
    end: Union[int, float]
    score: float
    confidence: float
    frames: int


class WordSpan(NamedTuple):
    tokens: tuple
    start: Union[int, float]
    end: Union[int, float]
    confidence: float


@dataclass
class Alignment:
    """What ``ctc_forced_align`` returns for H rows of at most S tokens: ``tok_start`` / ``tok_end`` [H, S] int32 the first frame of
    token j and its last frame plus 1, ``tok_score`` [H, S] fp32 the sum of the token's emissions over those frames (-1, -1, -inf
    past a row's length and in rows that are not alignable), ``frame_token`` [H, T'] int32 the token index of every frame (-1: a
    blank frame, -2: past the emission's length, or the row is not alignable), ``path_score`` [H] fp32, ``status`` [H] int32 (0:
    aligned, 1: not alignable).  ``tokens`` / ``tok_len``: the rows that were aligned, as the kernel read them."""
    tok_start: Tensor
    tok_end: Tensor
    tok_score: Tensor
    frame_token: Tensor
    path_score: Tensor
    status: Tensor
    tokens: Optional[Tensor] = None
    tok_len: Optional[Tensor] = None

    def spans(self, h: int, frame_seconds: Optional[float] = None) -> List[TokenSpan]:
        """The token spans of row ``h``, in order; [] for a row that is not alignable.  ``confidence`` is
        exp(tok_score / (end - start)) evaluated in fp64: the geometric mean of the frame posteriors when ``logp`` held log-probs.
        ``start`` / ``end`` are frames; with ``frame_seconds`` they are ``frame * frame_seconds`` (``FRAME_SECONDS`` = 0.04 is the
        default model's: the stem's stride of 4 times the front end's 10 ms hop).  The stem's receptive-field offset is NOT corrected:
        frame f is reported as beginning at ``f * frame_seconds``, although the stem's two stride-2 convolutions see a few spectrogram
        frames on either side of it."""
        if int(self.status[h]) != 0:
            return []
        n = int(self.tok_len[h])
        ids = self.tokens[h, :n].tolist()
        a, b, sc = self.tok_start[h, :n].tolist(), self.tok_end[h, :n].tolist(), self.tok_score[h, :n].double().tolist()
        k = 1 if frame_seconds is None else float(frame_seconds)
        return [TokenSpan(ids[j], a[j] * k, b[j] * k, sc[j], math.exp(sc[j] / (b[j] - a[j])), b[j] - a[j]) for j in range(n)]


def starts_word_from_pieces(pieces: Sequence[str], marker: str = "\u2581") -> np.ndarray:
    """bool [V]: piece v begins a word (it starts with the sentence-piece ``marker``)."""
    return np.asarray([str(p).startswith(marker) for p in pieces], dtype=bool)


def group_words(spans, starts_word: Union[Sequence[bool], Callable[[int], bool]]) -> List[list]:
    """``spans`` (anything with a ``.token``) cut into words: a token for which ``starts_word`` holds opens one, as does the first."""
    opens = starts_word if callable(starts_word) else (lambda t, table=np.asarray(starts_word, dtype=bool): bool(table[t]))
    groups: List[list] = []
    for sp in spans:
        if not groups or opens(sp.token):
            groups.append([])
        groups[-1].append(sp)
    return groups


def word_spans(spans: Sequence[TokenSpan], starts_word: Union[Sequence[bool], Callable[[int], bool]]) -> List[WordSpan]:
    """Token spans merged into words, on the host: a token for which ``starts_word`` (a bool array over the vocabulary, or a callable
    on the id) holds opens a word, as does the first token.  A word runs from its first token's start to its last token's end; its
    confidence is the geometric mean over all of its label frames, exp(sum of scores / sum of frames) in fp64."""
    return [WordSpan(tuple(sp.token for sp in g), g[0].start, g[-1].end,
                     math.exp(math.fsum(sp.score for sp in g) / sum(sp.frames for sp in g))) for g in group_words(spans, starts_word)]


def transcript_rows(hyps, drop=(), blank: int = 0, name: str = "timestamps") -> List[List[int]]:
    """Decoder output as label rows: ``hyps[b]`` is a list of ids, a tensor, a hypothesis with ``.tokens``, or an n-best list of
    those, whose first is taken; the ids of ``drop`` (SOS, EOS, PAD) are removed.  A ``blank`` in a row is refused: it is no
    label, and the alignment could only answer it with status 1.  ``name``: the caller, for the message."""
    rows = []
    for b, hyp in enumerate(hyps):
        if isinstance(hyp, (list, tuple)) and hyp and not isinstance(hyp[0], (int, np.integer)) and not torch.is_tensor(hyp[0]):
            hyp = hyp[0]
        ids = hyp.tokens if hasattr(hyp, "tokens") else hyp
        ids = [int(t) for t in (ids.reshape(-1).tolist() if torch.is_tensor(ids) else ids)]
        ids = [t for t in ids if t not in drop]
        if blank in ids:
            raise ValueError(f"{name}: the transcript of utterance {b} holds the blank ({blank})")
        rows.append(ids)
    return rows


def exit_rows(name: str, hyps, exits, E: int, B: int, drop=(), blank: int = 0):
    """The rows ``BeamInference.timestamps`` / ``.confidences`` (``name``, for the messages) hand to the lattice kernels: the
    transcripts of ``hyps`` (``transcript_rows``) paired with exits -- ``exits`` None: the last of the E exits for each of the B
    utterances; one 0-based exit per utterance; ``"all"``: every exit, exit-major.  Returns ``(pairs [(e, b)], tokens int32 [H, S]
    zero-padded to S = max(1, longest), tok_len int32 [H], em_index int32 [H] = e * B + b)``."""
    if len(hyps) != B:
        raise ValueError(f"{name}: {B} utterances, {len(hyps)} hypotheses")
    rows = transcript_rows(hyps, drop, blank, name)
    if isinstance(exits, str):
        if exits != "all":
            raise ValueError(f"{name}: exits must be None, one exit per utterance or 'all', got {exits!r}")
        pairs = [(e, b) for e in range(E) for b in range(B)]
    else:
        of = [E - 1] * B if exits is None else [int(e) for e in (exits.tolist() if torch.is_tensor(exits) else exits)]
        if len(of) != B or any(not 0 <= e < E for e in of):
            raise ValueError(f"{name}: exits must hold one exit of 0 .. {E - 1} per utterance ({B})")
        pairs = [(e, b) for b, e in enumerate(of)]
    S = max(1, max(len(r) for r in rows))
    tokens = torch.zeros((len(pairs), S), dtype=torch.int32)
    for h, (_, b) in enumerate(pairs):
        tokens[h, :len(rows[b])] = torch.tensor(rows[b], dtype=torch.int32)
    tok_len = torch.tensor([len(rows[b]) for _, b in pairs], dtype=torch.int32)
    em_index = torch.tensor([e * B + b for e, b in pairs], dtype=torch.int32)
    return pairs, tokens, tok_len, em_index


def host_lattice(y: np.ndarray, N: np.ndarray, blank: int):
    """The lattice of K rows ``y`` [K, S] (blank past ``N`` [K]) over [K, 2S + 1] states: ``(lab int64 the label of every state --
    the states past 2N compute on the blank and feed nothing --, skip bool: state s takes from s - 2, skipn bool: state s gives to
    s + 2, valid bool: s <= 2N)``."""
    K, S = y.shape
    NS = 2 * S + 1
    valid = np.arange(NS)[None, :] <= 2 * N[:, None]
    lab = np.full((K, NS), blank, dtype=np.int64)
    lab[:, 1::2] = y
    skip = np.zeros((K, NS), dtype=bool)
    if S > 1:
        skip[:, 3::2] = y[:, 1:] != y[:, :-1]
    skip &= valid  # skip is set on odd states only: s <= 2N is s <= 2N - 1 there
    skipn = np.zeros((K, NS), dtype=bool)
    skipn[:, :-2] = skip[:, 2:]
    return lab, skip, skipn, valid


def _host_rows(x: np.ndarray, T: np.ndarray, ei: np.ndarray, y: np.ndarray, N: np.ndarray, blank: int, free_start: bool = False,
               free_end: bool = False):
    """The header's statement for K rows that passed its row checks, one step per frame over [K, 2S + 1] states: fp32 adds and
    compares in its order.  ``x`` [n_em, T', V], ``T`` / ``ei`` / ``N`` [K], ``y`` [K, S] (blank past N).  ``free_start`` /
    ``free_end``: eec_ctc_segment's flags -- the emission term of state 0 (of state 2N, from frame 1 on) is 0.0f.  Returns
    ``(state [K, T'] (-1 past T), path_score [K], ok [K])``."""
    K, S = y.shape
    Tq = x.shape[1]
    NS = 2 * S + 1
    NEG = np.float32(-np.inf)
    lab, skip, _, _ = host_lattice(y, N, blank)
    rows = np.arange(K)
    a = np.full((K, NS), NEG, dtype=np.float32)
    a[:, 0] = np.float32(0.0) if free_start else x[ei, 0, blank]
    a[:, 1] = x[ei, 0, y[:, 0]]
    t_max = int(T.max())
    dec = np.zeros((t_max, K, NS), dtype=np.uint8)
    neg1, neg2 = np.full((K, 1), NEG, np.float32), np.full((K, 2), NEG, np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(1, t_max):
            act = T > t
            e = np.take_along_axis(x[ei, min(t, Tq - 1), :], lab, axis=1)  # a row past its length: computed, not kept
            if free_start:
                e[:, 0] = 0.0
            if free_end:
                e[rows, 2 * N] = 0.0
            best, d = a, np.zeros((K, NS), dtype=np.uint8)
            step = np.concatenate([neg1, a[:, :-1]], axis=1)
            take = step > best
            best, d = np.where(take, step, best), np.where(take, np.uint8(1), d)
            two = np.concatenate([neg2, a[:, :-2]], axis=1)
            take = skip & (two > best)
            best, d = np.where(take, two, best), np.where(take, np.uint8(2), d)
            a = np.where(act[:, None], (best + e).astype(np.float32), a)
            dec[t] = d
        hi, lo = a[rows, 2 * N], a[rows, 2 * N - 1]
        at_blank = hi > lo
        score = np.where(at_blank, hi, lo).astype(np.float32)
        ok = score > NEG  # False for a NaN
    s = np.where(at_blank, 2 * N, 2 * N - 1)
    state = np.full((K, Tq), -1, dtype=np.int64)
    for t in range(t_max - 1, 0, -1):
        m = T - 1 >= t
        state[m, t] = s[m]
        s = np.where(m, s - dec[t, rows, s], s)
    state[:, 0] = s
    return state, score, ok & (s <= 1)


def host_row_checks(shape, lens: Optional[np.ndarray], tokens: np.ndarray, tok_len: np.ndarray, em_index: Optional[np.ndarray],
                    blank: int):
    """The header's row checks on the host: ``(ok [H] bool, N [H], ei [H], inside [H, S] bool, tk [H, S] int64, T_all [n_em])``."""
    n_em, Tq, V = shape
    H, S = tokens.shape
    N = tok_len.astype(np.int64)
    ei = np.arange(H, dtype=np.int64) if em_index is None else em_index.astype(np.int64)
    ok = (ei >= 0) & (ei < n_em) & (N >= 1) & (N <= S)
    inside = np.arange(S)[None, :] < np.where(ok, N, 0)[:, None]
    tk = tokens.astype(np.int64)
    ok &= ~(inside & ((tk < 0) | (tk >= V) | (tk == blank))).any(axis=1)
    R = (inside[:, 1:] & (tk[:, 1:] == tk[:, :-1])).sum(axis=1)
    ei_c = np.clip(ei, 0, n_em - 1)
    T_all = np.full(n_em, Tq, dtype=np.int64) if lens is None else np.clip(lens.astype(np.int64), 0, Tq)
    ok &= T_all[ei_c] >= N + R
    return ok, N, ei, inside, tk, T_all


def _host_align(x: np.ndarray, lens: Optional[np.ndarray], tokens: np.ndarray, tok_len: np.ndarray, em_index: Optional[np.ndarray],
                blank: int, free_start: bool = False, free_end: bool = False):
    n_em, Tq, V = x.shape
    H, S = tokens.shape
    NEG = np.float32(-np.inf)
    tok_start = np.full((H, S), -1, dtype=np.int32)
    tok_end = np.full((H, S), -1, dtype=np.int32)
    tok_score = np.full((H, S), NEG, dtype=np.float32)
    frame_token = np.full((H, Tq), -2, dtype=np.int32)
    path_score = np.full((H,), NEG, dtype=np.float32)
    status = np.ones((H,), dtype=np.int32)
    ok, N, ei, inside, tk, T_all = host_row_checks(x.shape, lens, tokens, tok_len, em_index, blank)
    keep = np.nonzero(ok)[0]
    step = max(1, (1 << 26) // max(1, Tq * (2 * S + 1)))  # bounds the [T, K, 2S + 1] decisions
    for c0 in range(0, keep.size, step):
        r = keep[c0:c0 + step]
        Tr, er, Nr = T_all[ei[r]], ei[r], N[r]
        y = np.where(inside[r], tk[r], blank)
        state, score, good = _host_rows(x, Tr, er, y, Nr, blank, free_start, free_end)
        g = np.nonzero(good)[0]
        state, rg, Tg, eg, yg = state[g], r[g], Tr[g], er[g], y[g]
        path_score[rg], status[rg] = score[g], 0
        valid = np.arange(Tq)[None, :] < Tg[:, None]
        frame_token[rg] = np.where(valid, np.where(state & 1, state >> 1, -1), -2)
        # spans and scores, frame by frame: a token's sum begins with its first frame's value and adds in frame order
        ts, te, sc = tok_start[rg], tok_end[rg], tok_score[rg]
        k = np.arange(g.size)
        for t in range(int(Tg.max()) if g.size else 0):
            m = (Tg > t) & ((state[:, t] & 1) == 1)
            kk, j = k[m], state[m, t] >> 1
            v = x[eg[m], t, yg[m, j]]
            first = ts[kk, j] < 0
            sc[kk, j] = np.where(first, v, (sc[kk, j] + v).astype(np.float32))
            ts[kk, j] = np.where(first, t, ts[kk, j])
            te[kk, j] = t + 1
        tok_start[rg], tok_end[rg], tok_score[rg] = ts, te, sc
    return tok_start, tok_end, tok_score, frame_token, path_score, status


def launch_rows(entry: str, logp: Tensor, lens, tokens: Tensor, tok_len: Tensor, em_index, blank: int, outs, max_workspace_bytes: int,
                extra=()):
    """``entry`` (``eec_ctc_forced_align``, ``eec_ctc_posteriors``, ``eec_ctc_segment``) over the H rows into ``outs``, the entry's
    outputs in its order (tensors with a leading H; None where it takes a null); ``extra``: what the entry takes between ``blank``
    and its outputs.  A call whose workspace exceeds the bound is split over rows: a row's result depends on that row alone."""
    dev = logp.device
    n_em, Tq, V = logp.shape
    H, S = tokens.shape
    if H == 0:
        return
    size = getattr(capi.load(), entry + "_workspace_bytes")
    Hc = max(1, min(H, int(max_workspace_bytes) // max(1, size(1, Tq, S))))
    if em_index is None and Hc < H:  # the rows of a later part are no longer their emissions' indices
        em_index = torch.arange(H, dtype=torch.int32, device=dev)
    ws_bytes = size(Hc, Tq, S)
    ws, ws_ptr = capi.aligned_ws(ws_bytes, dev)
    for h0 in range(0, H, Hc):
        h1 = min(H, h0 + Hc)
        capi.launch(entry, dev, logp, n_em, Tq, V, lens, tokens[h0:h1], tok_len[h0:h1], None if em_index is None else em_index[h0:h1],
                    h1 - h0, S, blank, *extra, *(None if t is None else t[h0:h1] for t in outs), ws_ptr, ws_bytes)
    del ws


def _device_align(logp: Tensor, lens, tokens: Tensor, tok_len: Tensor, em_index, blank: int, max_workspace_bytes: int):
    dev, Tq = logp.device, logp.size(1)
    H, S = tokens.shape
    out = (torch.empty((H, S), dtype=torch.int32, device=dev), torch.empty((H, S), dtype=torch.int32, device=dev),
           torch.empty((H, S), dtype=torch.float32, device=dev), torch.empty((H, Tq), dtype=torch.int32, device=dev),
           torch.empty((H,), dtype=torch.float32, device=dev), torch.empty((H,), dtype=torch.int32, device=dev))
    launch_rows("eec_ctc_forced_align", logp, lens, tokens, tok_len, em_index, blank, out, max_workspace_bytes)
    return out


def row_arguments(name: str, logp: Tensor, tokens, tok_len, em_index, em_len, blank: int, max_tokens: int = MAX_TOKENS):
    """The arguments ``ctc_forced_align``, ``ctc_posteriors`` and ``ctc_segment`` share, checked and in the kernels' form: ``(flat
    [n_em, T', V], lens int32 [n_em] or None, tokens int32 [H, S], tok_len int32 [H], em_index int32 [H] or None, blank)``, all on
    ``logp``'s device.  ``max_tokens``: the entry's limit on S."""
    if logp.dim() not in (3, 4):
        raise ValueError(f"{name}: logp must be [n_em, T', V] or [E, B, T', V], got {tuple(logp.shape)}")
    if logp.dtype != torch.float32:
        raise ValueError(f"{name}: logp must be fp32, got {logp.dtype}")
    lead = tuple(logp.shape[:-2])
    Tq, V = int(logp.size(-2)), int(logp.size(-1))
    n = int(np.prod(lead))
    blank = int(blank)
    if n < 1 or Tq < 1:
        raise ValueError(f"{name}: no emissions")
    if V < 2 or not 0 <= blank < V:
        raise ValueError(f"{name}: needs V >= 2 and blank in [0, V), got {V} and {blank}")
    tokens = torch.as_tensor(tokens)
    if tokens.dim() != 2 or tokens.dtype.is_floating_point or tokens.dtype == torch.bool:
        raise ValueError(f"{name}: tokens must be an integer tensor [H, S], got {tokens.dtype} {tuple(tokens.shape)}")
    H, S = tokens.shape
    if not 1 <= S <= max_tokens:
        raise ValueError(f"{name}: a row has 1 .. {max_tokens} tokens, got S = {S}")
    dev = logp.device
    flat = logp.reshape(n, Tq, V)
    if not flat.is_contiguous():
        flat = flat.contiguous()
    # an id that int32 cannot hold is outside every vocabulary: it stays outside after the narrowing
    tokens = tokens.to(torch.int64).clamp(-1, 2 ** 31 - 1).to(device=dev, dtype=torch.int32).contiguous()
    tok_len = torch.full((H,), S, dtype=torch.int32, device=dev) if tok_len is None else \
        _frame_counts(name, "tok_len", tok_len, H, dev)
    em_index = _frame_counts(name, "em_index", em_index, H, dev)
    if em_index is None and H > n:
        raise ValueError(f"{name}: {H} rows, {n} emissions and no em_index")
    if em_len is not None:
        em_len = torch.as_tensor(em_len)
        if len(lead) == 2 and em_len.numel() == lead[1] and lead[0] != 1:
            em_len = em_len.reshape(1, lead[1]).expand(lead[0], lead[1]).reshape(-1)
    lens = _frame_counts(name, "em_len", em_len, n, dev)
    return flat, lens, tokens, tok_len, em_index, blank


def ctc_forced_align(logp: Tensor, tokens: Tensor, tok_len: Optional[Tensor] = None, em_index: Optional[Tensor] = None,
                     em_len: Optional[Tensor] = None, blank: int = 0, max_workspace_bytes: int = 2 << 30) -> Alignment:
    """Viterbi forced alignment of H token rows in the standard CTC topology (the statement: include/eec.h).  ``logp``
    [n_em, T', V] or [E, B, T', V] fp32, log-probs or logits; ``tokens`` [H, S] of any integer dtype with ``tok_len`` [H] labels
    each (None: S), S <= 255; ``em_index`` [H] the emission of every row -- e * B + b for [E, B, ...] input -- (None: its own index);
    ``em_len`` frames per emission, int32 / int64 -- [n_em], or for [E, B, ...] input [B] (shared by the exits) or [E, B] --, clamped
    to [0, T'], None: T' for all.  Frames from a length on are never read.  A row the statement cannot align (no tokens, fewer frames
    than tokens plus adjacent equal pairs, a token outside [0, V) or equal to ``blank``, an ``em_index`` outside the emissions)
    has status 1 and the fill values.  Device tensors: one launch on the current stream, nothing read back, graph-capturable; a
    call whose decisions (``eec_ctc_forced_align_workspace_bytes``) exceed ``max_workspace_bytes`` is split over rows, which changes
    no bit.  CPU tensors: a NumPy host path with the same bits."""
    flat, lens, tokens, tok_len, em_index, blank = row_arguments("ctc_forced_align", logp, tokens, tok_len, em_index, em_len, blank)
    if logp.is_cuda:
        out = _device_align(flat, lens, tokens, tok_len, em_index, blank, max_workspace_bytes)
    else:
        out = [torch.from_numpy(a) for a in _host_align(flat.detach().numpy(), None if lens is None else lens.numpy(), tokens.numpy(),
                                                        tok_len.numpy(), None if em_index is None else em_index.numpy(), blank)]
    return Alignment(*out, tokens=tokens, tok_len=tok_len)
