"""Aligning long transcripts (include/eec.h, "CTC segmentation: long rows, free ends"; csrc/ctc_segment.hip): ``ctc_segment`` is
``ctc_forced_align`` for rows of up to 4095 tokens -- a character-level utterance, or the concatenated transcript of a recording --
with optional free ends, so that the audio before the first and after the last token costs nothing; ``utterance_spans`` cuts such
a row back into its utterances with CTC segmentation's confidence (Kuerzinger et al. 2020); ``windowed_emission`` is the encoder
over a recording longer than ``max_len`` frames, in overlapping windows stitched at the middle of each overlap."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import capi
from .alignment import Alignment, _host_align, launch_rows, row_arguments

MAX_TOKENS = 4095  # EEC_SEG_MAX_TOKENS
FREE_START, FREE_END = 1, 2  # EEC_SEG_FREE_START, EEC_SEG_FREE_END


class UtteranceSpan(NamedTuple):
    """``start`` / ``end`` (end exclusive; frames, or seconds with ``frame_seconds``) of an utterance of ``n_tokens`` tokens: its
    first token's start and its last token's end.  ``mean_logp``: the mean over those frames of the emission at the frame's own
    label (its token, or the blank); ``min_window_logp``: the least such mean over the consecutive windows of the span."""
    start: Union[int, float]
    end: Union[int, float]
    n_tokens: int
    mean_logp: float
    min_window_logp: float


def ctc_segment(logp: Tensor, tokens: Tensor, tok_len: Optional[Tensor] = None, em_index: Optional[Tensor] = None,
                em_len: Optional[Tensor] = None, blank: int = 0, free_start: bool = False, free_end: bool = False,
                max_workspace_bytes: int = 2 << 30) -> Alignment:
    """``ctc_forced_align`` -- its arguments, its statement, its ``Alignment`` -- for rows of S <= 4095 tokens, one workgroup per
    row (``eec_ctc_segment``).  ``free_start``: the blank before the first token costs nothing, whatever the emission says there;
    ``free_end``: likewise the blank after the last token.  With both off the result is ``ctc_forced_align``'s, bit for bit; rows of
    at most 255 tokens are served faster there.  Device tensors: one launch on the current stream, nothing read back,
    graph-capturable; a call whose decisions (``eec_ctc_segment_workspace_bytes``) exceed ``max_workspace_bytes`` is split over
    rows, which changes no bit, and a single row that exceeds it is refused.  CPU tensors: a NumPy host path with the same bits."""
    name = "ctc_segment"
    flat, lens, tokens, tok_len, em_index, blank = row_arguments(name, logp, tokens, tok_len, em_index, em_len, blank, MAX_TOKENS)
    free_start, free_end = bool(free_start), bool(free_end)
    if not logp.is_cuda:
        out = [torch.from_numpy(a) for a in _host_align(flat.detach().numpy(), None if lens is None else lens.numpy(), tokens.numpy(),
                                                        tok_len.numpy(), None if em_index is None else em_index.numpy(), blank,
                                                        free_start, free_end)]
        return Alignment(*out, tokens=tokens, tok_len=tok_len)
    dev, Tq = flat.device, flat.size(1)
    H, S = tokens.shape
    per_row = capi.load().eec_ctc_segment_workspace_bytes(1, Tq, S)
    if per_row > int(max_workspace_bytes):
        raise ValueError(f"{name}: one row of {S} tokens over {Tq} frames needs {per_row} bytes of workspace, "
                         f"max_workspace_bytes is {int(max_workspace_bytes)}")
    out = (torch.empty((H, S), dtype=torch.int32, device=dev), torch.empty((H, S), dtype=torch.int32, device=dev),
           torch.empty((H, S), dtype=torch.float32, device=dev), torch.empty((H, Tq), dtype=torch.int32, device=dev),
           torch.empty((H,), dtype=torch.float32, device=dev), torch.empty((H,), dtype=torch.int32, device=dev))
    flags = (FREE_START if free_start else 0) | (FREE_END if free_end else 0)
    launch_rows("eec_ctc_segment", flat, lens, tokens, tok_len, em_index, blank, out, max_workspace_bytes, extra=(flags,))
    return Alignment(*out, tokens=tokens, tok_len=tok_len)


def utterance_spans(alignment: Alignment, h: int, utt_len: Sequence[int], logp_row: Tensor, blank: int = 0, window: int = 30,
                    frame_seconds: Optional[float] = None) -> List[UtteranceSpan]:
    """Row ``h`` of ``alignment`` cut into its utterances: ``utt_len[u]`` tokens each, in order, together the row's ``tok_len``.
    ``logp_row`` [T', V]: the emission the row was aligned against.  An utterance runs from its first token's ``tok_start`` to its
    last token's ``tok_end``; with p_f = logp_row[f][label of frame f] (the frame's token, or ``blank``) over those frames -- one
    gather on the emission's device, everything after it in fp64 on the host -- ``mean_logp`` is the mean of p_f and
    ``min_window_logp`` the minimum over the consecutive windows of ``window`` frames from the start on (the last one may be
    shorter) of the window's mean: CTC segmentation's confidence, by which an utterance is kept or dropped.  ``frame_seconds``
    scales the bounds, as ``Alignment.spans`` does.  [] for a row that is not alignable."""
    utt_len = [int(n) for n in utt_len]
    window = int(window)
    if window < 1:
        raise ValueError(f"utterance_spans: window must be >= 1, got {window}")
    if any(n < 1 for n in utt_len):
        raise ValueError("utterance_spans: every utterance has at least one token")
    n = int(alignment.tok_len[h])
    if sum(utt_len) != n:
        raise ValueError(f"utterance_spans: the utterances hold {sum(utt_len)} tokens, row {h} has {n}")
    if logp_row.dim() != 2 or logp_row.size(0) != alignment.frame_token.size(1):
        raise ValueError(f"utterance_spans: logp_row must be [T', V] with T' = {alignment.frame_token.size(1)}, got {tuple(logp_row.shape)}")
    if int(alignment.status[h]) != 0:
        return []
    a, b = alignment.tok_start[h, :n].tolist(), alignment.tok_end[h, :n].tolist()
    f0, f1 = a[0], b[-1]
    dev = logp_row.device
    ft = alignment.frame_token[h, f0:f1].to(device=dev, dtype=torch.int64)
    ids = alignment.tokens[h].to(device=dev, dtype=torch.int64)
    lab = torch.where(ft >= 0, ids[ft.clamp(min=0)], torch.full_like(ft, int(blank)))
    p = logp_row[f0:f1].gather(1, lab[:, None])[:, 0].double().cpu().numpy()
    k = 1 if frame_seconds is None else float(frame_seconds)
    out, j = [], 0
    for m in utt_len:
        s, e = a[j], b[j + m - 1]
        q = p[s - f0:e - f0]
        worst = min(float(q[c:c + window].sum()) / len(q[c:c + window]) for c in range(0, e - s, window))
        out.append(UtteranceSpan(s * k, e * k, m, float(q.sum()) / (e - s), worst))
        j += m
    return out


def window_plan(T: int, window: int, overlap: int, max_len: int):
    """``windowed_emission``'s arithmetic: ``(n_win, hop)`` for ``T`` mel frames; refuses what the stitching rule cannot serve."""
    window, overlap = int(window), int(overlap)
    hop = window - overlap
    if overlap < 0 or hop < 1:
        raise ValueError(f"windowed_emission: needs 0 <= overlap < window, got window = {window}, overlap = {overlap}")
    if hop % 4:
        raise ValueError(f"windowed_emission: window - overlap must be a multiple of 4 (the stem's stride), got {hop}")
    if overlap % 8:
        raise ValueError(f"windowed_emission: overlap must be a multiple of 8 (the seam is the middle of the overlap), got {overlap}")
    if window > max_len:
        raise ValueError(f"windowed_emission: window = {window} exceeds the model's max_len = {max_len}")
    return (1 if T <= window else -(-(T - window) // hop) + 1), hop


def windowed_emission(model, spec: Tensor, window: int, overlap: int, batch: int = 16) -> Tensor:
    """The log-probs of every exit for ONE recording that may be longer than the model's ``max_len``: ``spec`` [n_mels, T] or
    [1, n_mels, T] -> [E, 1, T', V].  ``window`` and ``overlap`` are mel frames, hop = window - overlap a multiple of 4, overlap a
    multiple of 8, window <= max_len.  Window i covers the mel frames [i * hop, i * hop + window), the last one zero-padded and run
    with its true length; the windows go through ``model.forward`` in batches of ``batch`` under ``no_grad``.  Output frame g is
    window i's local frame g - i * hop / 4 with i = clamp((g - overlap / 8) // (hop / 4), 0, n_win - 1): each seam lies in the
    middle of an overlap, where both windows have the most context.  T' is the last window's offset plus its valid output length.
    A recording that fits one window is ``model.forward``'s output as it is."""
    if spec.dim() == 3 and spec.size(0) == 1:
        spec = spec[0]
    if spec.dim() != 2:
        raise ValueError(f"windowed_emission: spec must be [n_mels, T] or [1, n_mels, T], got {tuple(spec.shape)}")
    n_mels, T = spec.shape
    n_win, hop = window_plan(T, window, overlap, int(model._cfg.max_len))
    window, batch = int(window), max(1, int(batch))
    with torch.no_grad():
        if n_win == 1:
            return model.forward(spec[None], torch.tensor([T]))
        h4, o8 = hop // 4, int(overlap) // 8
        result, total = None, 0
        for i0 in range(0, n_win, batch):
            i1 = min(n_win, i0 + batch)
            mel = spec.new_zeros((i1 - i0, n_mels, window))
            true = [min(window, T - i * hop) for i in range(i0, i1)]
            for k, i in enumerate(range(i0, i1)):
                mel[k, :, :true[k]] = spec[:, i * hop:i * hop + true[k]]
            out = model.forward(mel, torch.tensor(true))  # [E, n, Tw, V]
            Tw = int(out.size(2))
            if h4 + o8 > Tw:
                raise ValueError(f"windowed_emission: a window of {window} frames gives {Tw} output frames, the seams need "
                                 f"{h4 + o8}: the overlap is too small for the stem")
            if result is None:
                last_true = T - (n_win - 1) * hop  # in (overlap, window]
                total = (n_win - 1) * h4 + min(last_true // 4, Tw)
                result = out.new_empty((out.size(0), 1, total, out.size(3)))
            for k, i in enumerate(range(i0, i1)):
                g0 = 0 if i == 0 else i * h4 + o8
                g1 = total if i == n_win - 1 else (i + 1) * h4 + o8
                result[:, 0, g0:g1] = out[:, k, g0 - i * h4:g1 - i * h4]
        return result
