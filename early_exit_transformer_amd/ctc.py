"""The CTC operators on encoder log-probs: per-exit losses with their gradient (train.py:53-68), self-distillation between the exits
(the reference's unimplemented ``--distill``), MWER training against N-best lists, greedy, prefix-beam and
lexicon-constrained beam decoding and forced alignment (util/beam_infer.py) and the encoder's frame lengths.  Each is one call into libeec.so on the caller's current HIP
stream; there is no CPU path, except for the CTC prefix scorer of one-pass joint decoding (``ctc_prefix_session``), whose host path lets a
search loop be tested without a device, for the exit statistics and the exit choice of adaptive inference (``exit_statistics``,
``select_exits``), whose host paths state them in torch ops, and for MWER training (``ctc_hyp_logp``, ``exit_mwer_losses``), whose host
path is the statement through torch's own ``F.ctc_loss`` and autograd."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import capi
from .capi import launch, to_device
from .decoding import ScorerSession


def encoder_lengths(lengths: Tensor, t_out: int) -> Tensor:
    """``clamp(lengths / 4, max=T').to(int)`` (early_exit.py:623) on the device: int64 [B] -> int32 [B]."""
    if not lengths.is_cuda:
        raise RuntimeError("encoder_lengths runs on a HIP device only")
    lengths = lengths.to(torch.int64).contiguous()
    out = torch.empty((lengths.numel(),), dtype=torch.int32, device=lengths.device)
    launch("eec_encoder_lengths", lengths.device, lengths, lengths.numel(), int(t_out), out)
    return out


def _frame_counts(name: str, arg: str, lens: Optional[Tensor], n: int, dev: torch.device, any_dtype: bool = False) -> Optional[Tensor]:
    """A per-sequence frame count argument (int32 or int64, any device) as the kernels read it: int32 [n] on ``dev``, or None.
    The kernels clamp a count to [0, T']: one that int32 cannot hold is clamped before it is narrowed, so that it stays on its own
    side of that range.  ``any_dtype``: the callers that have always converted whatever they were given keep doing so."""
    if lens is None:
        return None
    if not isinstance(lens, Tensor):
        lens = torch.as_tensor(lens)
    if lens.dtype not in (torch.int32, torch.int64) and not any_dtype:
        raise ValueError(f"{name}: {arg} must be an int32 or int64 tensor, got {lens.dtype}")
    if lens.numel() != n:
        raise ValueError(f"{name}: {arg} must have {n} entries, got {lens.numel()}")
    if lens.dtype != torch.int32:
        lens = lens.to(torch.int64).clamp(-2 ** 31, 2 ** 31 - 1)
    return lens.reshape(n).to(device=dev, dtype=torch.int32).contiguous()


def greedy_ctc(logp: Tensor, blank: int = 0, em_len: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """[N, T', V] fp32 log-probs on the GPU -> (tokens [N, T'] int32, counts [N] int32).  ``em_len`` [N] (None: T' for every
    sequence): sequence s is its first ``clamp(em_len[s], 0, T')`` frames (eec_greedy_ctc_len)."""
    if not logp.is_cuda:
        raise RuntimeError("greedy_ctc runs on a HIP device only")
    logp = logp.contiguous().float()
    N, Tq, V = logp.shape
    el = _frame_counts("greedy_ctc", "em_len", em_len, N, logp.device)
    tokens = torch.empty((N, Tq), dtype=torch.int32, device=logp.device)
    counts = torch.empty((N,), dtype=torch.int32, device=logp.device)
    launch("eec_greedy_ctc_len", logp.device, logp, el, N, Tq, V, blank, tokens, counts)
    return tokens, counts


def ctc_beam_decode(logp: Tensor, beam_size: int = 10, blank: int = 0, blank_skip_threshold: float = 0.95,
                    skip_drops_frame: bool = False, em_len: Optional[Tensor] = None, nbest: Optional[int] = None, context=None,
                    graph_of=None, lm=None, lm_weight: Optional[float] = None, token_score: float = 0.0):
    """CTC prefix beam search of [N, T', V] log-probs on the device (eec_ctc_beam_decode): the best hypothesis per
    sequence, as ``BeamInference.ctc_cuda_predict`` uses torchaudio's cuda_ctc_decoder (util/beam_infer.py:102-112).
    ``skip_drops_frame``: a frame above ``blank_skip_threshold`` is dropped instead of being taken as a blank frame (the two
    readings of the third-party decoder's skip rule, include/eec.h).  ``em_len`` [N] (None: T' for every sequence, the
    reference's ``encoder_out_lens``): sequence s is its first ``clamp(em_len[s], 0, T')`` frames; none gives count 0, score 0
    (eec_ctc_beam_decode_len).  Returns (tokens [N, T'] int32, counts [N] int32, scores [N] fp32).
    ``nbest`` (None: the call and the three return values above, unchanged): an integer in [1, beam_size] returns the beam the
    same search ends with instead of its best prefix alone (eec_ctc_beam_decode_nbest) -- (tokens [N, nbest, T'] int32, counts
    [N, nbest] int32, scores [N, nbest] fp32, n_hyp [N] int32), best first, ties to the lower beam index; hypothesis 0 is the
    hypothesis the call without ``nbest`` returns, an absent one (rank >= n_hyp) has count 0 and score -inf.
    ``context`` (None: the call and its return values, unchanged): a ``context.ContextGraph`` -- the search ranks by total
    log-probability + bias (eec_ctc_beam_decode_ctx / _nbest_ctx, include/eec.h "Contextual biasing") and ``bias`` ([N] or [N, nbest]
    fp32, shaped like ``scores``) is appended to the tuple; ``scores`` stays the CTC log-probability alone.  ``graph_of`` [N] chooses a
    graph of a bank per sequence (None: graph 0; an index outside the bank: no biasing for that sequence).
    ``lm`` (None: the call and its return values, unchanged): a ``lm_fusion.TokenLM`` over the V labels -- shallow fusion: the search
    ranks by total log-probability + fusion, where every label adds ``lm_weight`` (None: 0.3, customary and not tuned) times the
    model's log10 score plus ``token_score`` and the model's ``</s>`` closes a prefix (eec_ctc_beam_decode_lm / _nbest_lm,
    include/eec.h "Shallow fusion"); ``fusion`` (shaped like ``scores``, which stay the CTC log-probability alone) is appended to the
    tuple.  Not together with ``context``: a graph and a model in one CTC call are not served."""
    if lm is not None and context is not None:
        raise ValueError("ctc_beam_decode: a context graph and a language model in one CTC call are not served; choose one")
    if lm is None and (lm_weight is not None or token_score != 0.0):
        raise ValueError("ctc_beam_decode: lm_weight / token_score weigh lm=, which was not given")
    if not logp.is_cuda:
        raise RuntimeError("ctc_beam_decode runs on a HIP device only")
    logp = logp.contiguous().float()
    N, Tq, V = logp.shape
    dev = logp.device
    el = _frame_counts("ctc_beam_decode", "em_len", em_len, N, dev)
    if context is None and graph_of is not None:
        raise ValueError("ctc_beam_decode: graph_of chooses among the graphs of context=, which was not given")
    k = () if nbest is None else (int(nbest),)
    ws = torch.empty((capi.load().eec_ctc_beam_workspace_bytes(N, Tq),), dtype=torch.uint8, device=dev)
    if lm is not None:
        from .lm_fusion import DEFAULT_LM_WEIGHT, check_lm
        lm_weight = DEFAULT_LM_WEIGHT if lm_weight is None else float(lm_weight)
        check_lm("ctc_beam_decode", lm, V, beam_size, lm_weight, token_score)
        if lm.blank != blank:
            raise ValueError(f"ctc_beam_decode: the language model was built with blank {lm.blank}, the emission has blank {blank}")
    tokens = (torch.empty if nbest is None and context is None and lm is None else torch.zeros)((N, *k, Tq), dtype=torch.int32, device=dev)
    outs = [tokens, torch.empty((N, *k), dtype=torch.int32, device=dev), torch.empty((N, *k), dtype=torch.float32, device=dev)]
    if k:
        outs.append(torch.empty((N,), dtype=torch.int32, device=dev))  # n_hyp
    tail = ()
    if context is not None:
        from .context import graph_rows
        if context.vocab_size != V or context.blank != blank:
            raise ValueError(f"ctc_beam_decode: the context graph is over {context.vocab_size} tokens with blank {context.blank}, "
                             f"the emission over {V} with blank {blank}")
        tail = (context.to(dev), context.nbytes, graph_rows("ctc_beam_decode", graph_of, N, dev),
                torch.empty((N, *k), dtype=torch.float32, device=dev))  # image, its bytes, graph_of, bias
    if lm is not None:
        tail = (lm.on(dev), lm.nbytes, lm_weight, float(token_score), torch.empty((N, *k), dtype=torch.float32, device=dev))  # .., fusion
    entry = "eec_ctc_beam_decode" + (("_nbest" if k else "") + ("_lm" if lm is not None else "_ctx" if tail else "") or "_len")
    launch(entry, dev, logp, el, N, Tq, V, blank, beam_size, blank_skip_threshold, int(bool(skip_drops_frame)), *k, ws, *outs, *tail)
    return (*outs, tail[-1]) if tail else tuple(outs)


def ctc_lexicon_decode(emission: Tensor, trie, beam_size: int = 10, nbest: int = 1, word_score: float = 0.0, sil_score: float = 0.0,
                       beam_threshold: float = 50.0, em_len: Optional[Tensor] = None, max_words: Optional[int] = None, lm=None,
                       lm_weight: float = 0.0, smearing: Optional[str] = None, log_add: bool = False, wide: Optional[bool] = None):
    """Lexicon-constrained CTC beam search with N-best of [n, T', V] log-probs on the device (eec_ctc_lexbeam_decode): the
    decoder behind the reference's ``ctc_predict`` / ``ctc_predict_`` (torchaudio ``ctc_decoder(lexicon=...)``,
    util/beam_infer.py:51-65; the algorithm is stated in include/eec.h, parity with the third-party decoder is unpinned).
    ``lm``: None, or a ``lexicon.NGramLM`` packed for this trie -- its score times ``lm_weight`` joins at every word end and at the
    end of the sentence (eec_ctc_lexbeam_lm_decode), and ``scores`` are the final scores.
    ``smearing``: None, or ``"max"`` (needs ``lm``) -- LM look-ahead by max trie smearing (eec_ctc_lexbeam_lm_smear_decode): every
    step inside a word is charged the increase of the best score the model gives any word still reachable, and the word end takes
    that advance back.  A complete hypothesis scores what it scores without smearing; what changes is which hypotheses survive
    pruning.  The third-party decoder always smears; the default here stays off, so existing calls return what they returned.
    ``log_add``: False -- Viterbi merging: of the candidates that reach the same state the best one's score stays -- or True
    (eec_ctc_lexbeam_logadd_decode; torchaudio's ``log_add=True``, the reference's ``beam_predict`` setting): the survivor scores the
    log of the sum of their probabilities, by the bit-reproducible ``log_add`` of include/eec.h.  It combines with every ``lm`` /
    ``smearing`` setting.
    ``beam_size`` 1..64, ``nbest`` 1..``beam_size``.  Beams of 16 or less run the narrow kernels (a thread's candidates in registers),
    beams of 17 to 64 the wide kernel (eec_ctc_lexbeam_wide_decode, csrc/ctc_lexbeam_wide.hip: the frame's merged candidates in LDS,
    survivors by radix select), every ``lm`` / ``smearing`` / ``log_add`` setting included; a beam over 64 raises the library's
    error.  ``wide``: None -- by beam size --, True -- the wide kernel at any beam (at 16 or less it returns what the narrow ones
    return, bit for bit) --, or False -- the narrow kernels, a ``ValueError`` for a beam over 16.
    ``trie``: a ``lexicon.TokenTrie`` (it carries V, blank and sil); ``em_len`` [n] frames per sequence (None: T'); ``max_words``
    (None: T', always enough): the words kept per hypothesis -- ``word_count`` is the true count even above it.  Returns
    ``(words [n, nbest, max_words] int32 indices into trie.words, word_count [n, nbest], tokens [n, nbest, T'], token_count [n, nbest],
    timesteps [n, nbest, T'], scores [n, nbest] fp32, n_hyp [n])``: hypotheses best first, absent ones with score -inf and counts
    0, entries past a count -1.  One launch on the current stream, no host synchronisation."""
    if smearing not in (None, "max"):
        raise ValueError(f"ctc_lexicon_decode: smearing must be None or 'max', got {smearing!r}")
    if smearing is not None and lm is None:
        raise ValueError("ctc_lexicon_decode: smearing='max' needs lm=: it is the model's scores that are smeared over the trie")
    if wide is None:
        wide = int(beam_size) > 16
    elif not wide and int(beam_size) > 16:
        raise ValueError(f"ctc_lexicon_decode: wide=False serves beams up to 16, got beam_size={beam_size}")
    if not emission.is_cuda:
        raise RuntimeError("ctc_lexicon_decode runs on a HIP device only")
    logp = emission.contiguous().float()
    n, Tq, V = logp.shape
    if V != trie.V:
        raise ValueError(f"ctc_lexicon_decode: the emission has {V} labels, the trie was packed for {trie.V}")
    if lm is not None and lm.n_words != len(trie.words):
        raise ValueError(f"ctc_lexicon_decode: the model was packed for a lexicon of {lm.n_words} words, the trie has {len(trie.words)}")
    dev = logp.device
    lib = capi.load()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    max_words = Tq if max_words is None else int(max_words)
    words, word_count, tokens, token_count, timesteps, n_hyp = i32(n, nbest, max(max_words, 0)), i32(n, nbest), i32(n, nbest, Tq), i32(n, nbest), i32(n, nbest, Tq), i32(n)
    scores = torch.empty((n, nbest), dtype=torch.float32, device=dev)
    em_len = _frame_counts("ctc_lexicon_decode", "em_len", em_len, n, dev, any_dtype=True)
    ws_bytes = (lib.eec_ctc_lexbeam_wide_workspace_bytes if wide else lib.eec_ctc_lexbeam_workspace_bytes)(n, Tq, beam_size)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=dev)
    lm_image = None if lm is None else lm.on(dev)
    smear = None if smearing is None else lm.smear(trie).on(dev)
    if wide:
        entry, more = "eec_ctc_lexbeam_wide_decode", (lm_image, float(lm_weight), smear, int(bool(log_add)))
    elif log_add:
        entry, more = "eec_ctc_lexbeam_logadd_decode", (lm_image, float(lm_weight), smear)
    elif lm is None:
        entry, more = "eec_ctc_lexbeam_decode", ()
    elif smearing is None:
        entry, more = "eec_ctc_lexbeam_lm_decode", (lm_image, float(lm_weight))
    else:
        entry, more = "eec_ctc_lexbeam_lm_smear_decode", (lm_image, float(lm_weight), smear)
    launch(entry, dev, logp, n, Tq, V, em_len, trie.on(dev), trie.blank, trie.sil, int(beam_size), int(nbest), float(word_score),
           float(sil_score), float(beam_threshold), max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, ws,
           ws_bytes, *more)  # the stream sits in front of ``more``
    return words, word_count, tokens, token_count, timesteps, scores, n_hyp


def ctc_align(logp: Tensor, tokens: Tensor, tok_len: Optional[Tensor] = None, em_index: Optional[Tensor] = None,
              em_len: Optional[Tensor] = None, blank: int = 0, want_trellis: bool = False):
    """Viterbi forced alignment of H token sequences against CTC log-probs on the device (eec_ctc_align): what
    ``BeamInference.get_trellis`` + ``backtrack`` compute per hypothesis (util/beam_infer.py:129-191; semantics and quirks in
    include/eec.h).  ``logp`` [n_em, T', V]; ``tokens`` [H, S] int64 with ``tok_len`` [H] valid ids each (None: S);
    ``em_index`` [H] the emission of every hypothesis (None: its own index); ``em_len`` [n_em] frames per emission (None: T').
    Returns ``(point_token [H, T'] int32, point_score [H, T'], path_score [H], final_score [H], status [H] int32, trellis)``:
    the Point of every frame (token index -1 / score -inf before the first token's frame and past the emission's length),
    ``path[0].score``, ``trellis[T, N]``, 0 / 1 = aligned / not alignable (its row holds the fill values), and the trellis
    [H, T' + 1, S + 1] when ``want_trellis`` (else None)."""
    if not logp.is_cuda:
        raise RuntimeError("ctc_align runs on a HIP device only")
    logp = logp.contiguous().float()
    dev = logp.device
    n_em, Tq, V = logp.shape
    tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
    H, S = tokens.shape

    i32 = lambda t, n, name: _frame_counts("ctc_align", name, t, n, dev, any_dtype=True)  # noqa: E731
    tok_len = torch.full((H,), S, dtype=torch.int32, device=dev) if tok_len is None else i32(tok_len, H, "tok_len")
    em_index, em_len = i32(em_index, H, "em_index"), i32(em_len, n_em, "em_len")
    if em_index is None and H > n_em:
        raise ValueError(f"ctc_align: {H} hypotheses, {n_em} emissions and no em_index")
    point_token = torch.empty((H, Tq), dtype=torch.int32, device=dev)
    point_score = torch.empty((H, Tq), dtype=torch.float32, device=dev)
    path_score = torch.empty((H,), dtype=torch.float32, device=dev)
    final_score = torch.empty((H,), dtype=torch.float32, device=dev)
    status = torch.empty((H,), dtype=torch.int32, device=dev)
    trellis = torch.empty((H, Tq + 1, S + 1), dtype=torch.float32, device=dev) if want_trellis else None
    ws = torch.empty((capi.load().eec_ctc_align_workspace_bytes(H, Tq, S),), dtype=torch.uint8, device=dev)
    launch("eec_ctc_align", dev, logp, n_em, Tq, V, em_len, tokens, tok_len, em_index, H, S, int(blank), point_token, point_score,
           path_score, final_score, status, trellis, ws if ws.numel() else None)
    return point_token, point_score, path_score, final_score, status, trellis


_LA_EXP = (1.98412701e-04, 1.38888892e-03, 8.33333377e-03, 4.16666679e-02, 0.166666672, 0.5, 1.0, 1.0)
_LA_LOG = (0.0657233745, -0.116206668, 0.119458839, -0.12420819, 0.142122895, -0.166665554, 0.20002535, -0.250000626, 0.333333015, -0.5, 1.0)


def log_add32(a: Tensor, b: Tensor) -> Tensor:
    """``log(exp(a) + exp(b))`` on fp32 tensors as the fixed sequence of fp32 operations include/eec.h states for
    ``eec_ctc_log_add`` (every torch op is one IEEE operation, nothing contracts): the host restatement of the kernels'
    log_add; ``log_add(-inf, a) = a``."""
    a, b = torch.broadcast_tensors(a, b)
    hi, lo = torch.where(a > b, a, b), torch.where(a > b, b, a)
    d = lo - hi
    near = d > -17.34375
    d = torch.where(near, d, torch.zeros_like(d))
    n = torch.round(d * 1.44269502)
    r = d - n * 0.693145751953125
    r = r - n * 1.42860677e-06
    p = torch.full_like(d, _LA_EXP[0])
    for c in _LA_EXP[1:]:
        p = p * r + c
    u = 1.0 + torch.ldexp(p, n.to(torch.int32))
    halved = u > 1.41421354
    m = torch.where(halved, u * 0.5, u) - 1.0
    q = torch.full_like(d, _LA_LOG[0])
    for c in _LA_LOG[1:]:
        q = q * m + c
    s = m * q
    s = torch.where(halved, s + 0.693147182, s)
    return torch.where(near, hi + s, hi)


class CtcPrefixSession(ScorerSession):
    """CTC prefix scores of n lockstep beam searches for one-pass joint CTC / attention decoding (include/eec.h,
    csrc/ctc_prefix.hip): ``step(att [n, R, V], last [n, R], parent [n, R] | None)`` first advances the state to the R current
    beams -- beam r extends row ``parent[i, r]`` of the previous step by the token ``last[i, r]`` --, then returns the joint local
    scores ``local`` [n, R, V] that ``beam_select`` ranks: ``(1 - w) * att + w * ctc``, -inf where the CTC head gives probability
    zero, ``[pad] = 0`` alone for a beam that has taken EOS.  For a device emission every step is one launch on the current
    stream (no allocation beyond the result, no synchronisation); for a CPU emission the same arithmetic runs as fp32 tensor ops
    with a loop over the frames, so a search loop can be tested without a device."""

    MAX_BEAMS, MAX_VOCAB, MAX_FRAMES = 16, 256, 2048

    def __init__(self, emission: Tensor, em_len: Optional[Tensor], R_max: int, weight: float, eos: int, pad: int, blank: int = 0,
                 min_length: int = 0):
        if emission.dim() != 3 or emission.dtype != torch.float32:
            raise ValueError(f"emission must be fp32 [n, T', V], got {emission.dtype} {tuple(emission.shape)}")
        n, Tq, V = emission.shape
        if not 0 < float(weight) <= 1:
            raise ValueError(f"the CTC weight must be in (0, 1], got {weight}")
        if len({int(blank), int(eos), int(pad)}) != 3:
            raise ValueError("blank, eos and pad must be pairwise distinct")
        self.n, self.Tq, self.V, self.R_max = n, Tq, V, int(R_max)
        self.blank, self.eos, self.pad, self.weight, self.min_length = int(blank), int(eos), int(pad), float(weight), int(min_length)
        self.dev = emission.device
        self.emission = emission.contiguous()
        self.em_len = _frame_counts("ctc_prefix_session", "em_len", em_len, n, self.dev, any_dtype=True)
        if not self.emission.is_cuda:
            self._host_begin()
            return
        self.nbytes = capi.load().eec_ctc_prefix_state_bytes(n, self.R_max, Tq)
        self._state = capi.aligned_ws(self.nbytes, self.dev)
        launch("eec_ctc_prefix_begin", self.dev, *self._head(), self._state[1], self.nbytes)

    def _head(self):
        return (self.emission, self.em_len, self.n, self.Tq, self.V, self.blank, self.R_max)

    _arg = "att"

    def step(self, att: Tensor, last: Tensor, parent: Optional[Tensor] = None) -> Tensor:
        return super().step(att, last, parent)

    def _device(self, att: Tensor):
        return self.dev  # the emission's

    def _check_rows(self, R: int) -> None:
        if not self.emission.is_cuda:  # the device entry refuses a count outside its range itself
            super()._check_rows(R)

    def _launch(self, att, tok, par, R, local) -> None:
        launch("eec_ctc_prefix_step", self.dev, *self._head(), par, tok, R, self.rows, self.s, att, self.weight, self.eos, self.pad,
               self.min_length, local, self._state[1], self.nbytes)

    def prefix_scores(self) -> Tensor:
        """``pfx`` [n, R] of the current beams (after the last ``step``): the CTC log prefix probability of an open beam's
        labels, the full-sequence CTC log-likelihood of a done one."""
        if not self.emission.is_cuda:
            return self._pfx.clone()
        off = self._state[1] - self._state[0].data_ptr()
        slots = self._state[0][off: off + self.nbytes].view(torch.float32).view(2, self.n, self.R_max, -1)
        return slots[self.s & 1, :, : max(self.rows, 1), 0].clone()

    # ---- the host path: the statement of include/eec.h as fp32 tensor ops ----
    def _host_begin(self):
        n, Tq = self.n, self.Tq
        x = self.emission
        T = torch.full((n,), Tq, dtype=torch.int64) if self.em_len is None else self.em_len.to(torch.int64).clamp(1, Tq)
        self._T = T
        self._live = torch.arange(Tq).unsqueeze(0) < T.unsqueeze(1)  # [n, Tq]
        ninf = torch.full((n, 1, Tq), float("-inf"))
        rb = ninf.clone()
        acc = x[:, 0, self.blank].clone()
        rb[:, 0, 0] = acc
        for t in range(1, Tq):
            acc = acc + x[:, t, self.blank]
            rb[:, 0, t] = acc
        rb = torch.where(self._live.unsqueeze(1), rb, ninf)
        self._rn, self._rb, self._u = ninf, rb, rb.clone()
        self._pfx = torch.zeros((n, 1))
        self._last = torch.full((n, 1), -1, dtype=torch.int64)
        self._done = torch.zeros((n, 1), dtype=torch.bool)
        self._psi = torch.full((n, 1, self.V), float("-inf"))

    def _host_step(self, att: Tensor, c: Tensor, parent: Optional[Tensor], R: int) -> Tensor:
        n, Tq, V, x = self.n, self.Tq, self.V, self.emission
        NINF = float("-inf")
        at_T = (self._T - 1).view(n, 1, 1)
        if self.s == 0:
            grow = lambda t: t.expand(n, R, *t.shape[2:]).clone()  # noqa: E731
            rn, rb, u, pfx, last, done = (grow(t) for t in (self._rn, self._rb, self._u, self._pfx, self._last, self._done))
        else:
            p = torch.arange(R).expand(n, R) if parent is None else parent
            ok = (p >= 0) & (p < self.rows)
            p = p.clamp(0, self.rows - 1)
            pT = p.unsqueeze(2).expand(n, R, Tq)
            p_rn, p_rb, p_u = self._rn.gather(1, pT), self._rb.gather(1, pT), self._u.gather(1, pT)
            p_pfx, p_last, p_done = self._pfx.gather(1, p), self._last.gather(1, p), self._done.gather(1, p)
            c_ok = (c >= 0) & (c < V)
            cc = c.clamp(0, V - 1)
            psi_c = self._psi.gather(1, p.unsqueeze(2).expand(n, R, V)).gather(2, cc.unsqueeze(2)).squeeze(2)
            dead = ~ok | (~p_done & ~c_ok)
            copy = ~dead & p_done
            finish = ~dead & ~copy & (cc == self.eos)
            ext = ~dead & ~copy & ~finish
            e_pfx = torch.where(cc == self.blank, torch.full_like(psi_c, NINF), psi_c)
            # the extension of every (parent, token), one frame at a time
            same = (cc == p_last).unsqueeze(2)
            phi = torch.where(same, p_rb, p_u)  # [n, R, Tq]: phi[t] reads column t - 1
            xc = x.gather(2, cc.unsqueeze(1).expand(n, Tq, R)).transpose(1, 2)  # [n, R, Tq]
            xb = x[:, :, self.blank].unsqueeze(1)  # [n, 1, Tq]
            nn = torch.where(p_last < 0, xc[:, :, 0], torch.full_like(psi_c, NINF))
            nb = torch.full_like(nn, NINF)
            e_rn, e_rb = [nn], [nb]
            for t in range(1, Tq):
                nn, nb = log_add32(nn, phi[:, :, t - 1]) + xc[:, :, t], log_add32(nn, nb) + xb[:, :, t]
                e_rn.append(nn)
                e_rb.append(nb)
            e_rn, e_rb = torch.stack(e_rn, 2), torch.stack(e_rb, 2)
            gone = (~self._live.unsqueeze(1)) | (dead | (ext & (e_pfx == NINF))).unsqueeze(2)
            keep = (copy | finish).unsqueeze(2)
            ninf = torch.full_like(e_rn, NINF)
            rn = torch.where(gone, ninf, torch.where(keep, p_rn, e_rn))
            rb = torch.where(gone, ninf, torch.where(keep, p_rb, e_rb))
            u = torch.where(gone, ninf, torch.where(keep, p_u, log_add32(e_rn, e_rb)))
            full_p = p_u.gather(2, at_T.expand(n, R, 1)).squeeze(2)
            pfx = torch.where(dead, torch.full_like(p_pfx, NINF), torch.where(copy, p_pfx, torch.where(finish, full_p, e_pfx)))
            last = torch.where(dead, torch.full_like(cc, -1), torch.where(ext, cc, p_last))
            done = copy | finish
        # psi of every token of every current beam
        v = torch.arange(V).view(1, 1, V)
        same = v == last.unsqueeze(2)
        psi = torch.where((last < 0).unsqueeze(2), x[:, 0, :].unsqueeze(1).expand(n, R, V), torch.full((n, R, V), NINF))
        for t in range(1, Tq):
            phi = torch.where(same, rb[:, :, t - 1].unsqueeze(2), u[:, :, t - 1].unsqueeze(2))
            psi = torch.where(self._live[:, t].view(n, 1, 1), log_add32(psi, phi + x[:, t, :].unsqueeze(1)), psi)
        closed = done | (pfx == NINF)
        psi = torch.where(closed.unsqueeze(2), torch.full_like(psi, NINF), psi)
        self._rn, self._rb, self._u, self._pfx, self._last, self._done, self._psi = rn, rb, u, pfx, last, done, psi
        base = torch.where(closed, torch.zeros_like(pfx), pfx).unsqueeze(2)
        full = u.gather(2, at_T.expand(n, R, 1))
        ctc = psi - base
        ctc = torch.where(v == self.eos, torch.full_like(ctc, NINF) if self.s < self.min_length else (full - base).expand(n, R, V), ctc)
        ctc = torch.where((v == self.blank) | closed.unsqueeze(2), torch.full_like(ctc, NINF), ctc)
        w = torch.tensor(self.weight, dtype=torch.float32)
        mixed = (1.0 - w) * att + w * torch.where(ctc == NINF, torch.zeros_like(ctc), ctc)
        local = torch.where((ctc == NINF) | (mixed != mixed), torch.full_like(ctc, NINF), mixed)
        pad_only = torch.where(v == self.pad, torch.zeros_like(local), torch.full_like(local, NINF))
        return torch.where(done.unsqueeze(2), pad_only, local)


def ctc_prefix_session(emission: Tensor, em_len: Optional[Tensor], R_max: int, weight: float, eos: int, pad: int, blank: int = 0,
                       min_length: int = 0) -> CtcPrefixSession:
    """A ``CtcPrefixSession`` over ``emission`` [n, T', V] (fp32 CTC log-probs; ``em_len`` [n] frames each, None = T') for up to
    ``R_max`` beams per search: the CTC half of one-pass joint decoding at weight ``weight`` in (0, 1]."""
    return CtcPrefixSession(emission, em_len, R_max, weight, eos, pad, blank=blank, min_length=min_length)


def _ctc_forward(x: Tensor, tg: Tensor, tl: Tensor, blank: int, il: Optional[Tensor]):
    """The training forward (eec_ctc_loss_forward_len): (losses [E], nll [E * B], the backward workspace and its aligned pointer)."""
    E, B, Tq, V = x.shape
    dev = x.device
    lib = capi.load()
    nll = torch.empty((E * B,), dtype=torch.float32, device=dev)
    out = torch.empty((E,), dtype=torch.float32, device=dev)
    ws, ws_ptr = capi.aligned_ws(lib.eec_ctc_backward_workspace_bytes(E, B, Tq, tg.size(1)), dev)
    launch("eec_ctc_loss_forward_len", dev, x, tg, tl, il, E, B, Tq, V, tg.size(1), blank, nll, out, ws_ptr)
    return out, nll, ws, ws_ptr


def _ctc_backward(x: Tensor, tg: Tensor, tl: Tensor, blank: int, il: Optional[Tensor], nll: Tensor, ws_ptr: int, grad_loss: Tensor,
                  dlogp: Tensor) -> None:
    """eec_ctc_loss_backward_len into ``dlogp`` (every element is written); consumes the workspace of ``_ctc_forward``."""
    E, B, Tq, V = x.shape
    dev = x.device
    g = grad_loss.to(device=dev, dtype=torch.float32).contiguous()
    launch("eec_ctc_loss_backward_len", dev, x, tg, tl, il, E, B, Tq, V, tg.size(1), blank, nll, ws_ptr, g, dlogp)


class _ExitCtcLossFn(torch.autograd.Function):
    """Per-exit CTC losses [E] with their gradient with respect to the log-probs (``_ctc_forward`` / ``_ctc_backward``): what autograd computes through the reference's loop of E nn.CTCLoss calls
    (train.py:60-68)."""

    @staticmethod
    def forward(ctx, enc_out, tg, tl, blank, il=None):
        E, B, Tq, V = enc_out.shape
        if V > 256 or V % 4:
            raise ValueError(f"exit_ctc_losses with a gradient needs a vocabulary of at most 256 entries, a multiple of 4 (got {V}): "
                             "the CTC gradient kernel holds a vocabulary row in one wave")
        out, nll, ws, ws_ptr = _ctc_forward(enc_out, tg, tl, blank, il)
        ctx.save_for_backward(enc_out, tg, tl, nll, ws, il)
        ctx.blank, ctx.ws_ptr = blank, ws_ptr
        return out

    @staticmethod
    def backward(ctx, grad_out):
        enc_out, tg, tl, nll, ws, il = ctx.saved_tensors
        if getattr(ctx, "used", False):
            raise RuntimeError("exit_ctc_losses: backward through the same forward twice (its workspace is consumed)")
        ctx.used = True
        dlogp = torch.empty_like(enc_out)
        _ctc_backward(enc_out, tg, tl, ctx.blank, il, nll, ctx.ws_ptr, grad_out, dlogp)
        return dlogp, None, None, None, None


def exit_ctc_losses(enc_out: Tensor, targets: Tensor, target_len: Tensor, blank: int = 0, input_len: Optional[Tensor] = None) -> Tensor:
    """Per-exit CTC losses [E] of an encoder output [E, B, T', V] in ONE launch: what train.py:53-65 computes with
    E separate nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) calls and input length T' for every
    utterance.  ``.sum()`` is the reference's training loss.  Differentiable with respect to ``enc_out`` (HIP backward:
    beta recursion + dense gradient, the values torch autograd returns for the reference's loop).
    ``input_len`` [B] (None: T' for every utterance, the reference's convention; ``encoder_lengths(lengths, T')`` gives the
    encoder's own) is nn.CTCLoss's ``input_lengths``, shared by the exits and clamped to [0, T']: the frames at or past it are not
    read, whatever they hold, and their gradient rows are written as zeros.  The loss is still divided by the target length only."""
    if not enc_out.is_cuda:
        raise RuntimeError("exit_ctc_losses runs on a HIP device only")
    enc_out = enc_out.contiguous().float()
    dev = enc_out.device
    tg, tl = to_device(targets, dev), to_device(target_len, dev)
    E, B, Tq, V = enc_out.shape
    il = _frame_counts("exit_ctc_losses", "input_len", input_len, B, dev)
    if torch.is_grad_enabled() and enc_out.requires_grad:
        return _ExitCtcLossFn.apply(enc_out, tg, tl, blank, il)
    nll = torch.empty((E * B,), dtype=torch.float32, device=dev)
    out = torch.empty((E,), dtype=torch.float32, device=dev)
    launch("eec_ctc_loss_len", dev, enc_out, tg, tl, il, E, B, Tq, V, tg.size(1), blank, nll, out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Self-distillation between exits (include/eec.h states the loss; csrc/distill.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _teacher_map(teacher: Union[str, Sequence[int]], E: int) -> Tuple[int, ...]:
    """``"last"`` (every exit but the last learns from the last), ``"next"`` (exit e learns from e + 1) or E ints (-1: no student)."""
    if isinstance(teacher, str):
        if teacher == "last":
            return tuple([E - 1] * (E - 1) + [-1])
        if teacher == "next":
            return tuple(list(range(1, E)) + [-1])
        raise ValueError(f"teacher must be 'last', 'next' or a sequence of {E} exit indices, got {teacher!r}")
    if isinstance(teacher, Tensor):
        teacher = teacher.tolist()
    t = tuple(int(k) for k in teacher)
    if len(t) != E:
        raise ValueError(f"teacher must have one entry per exit ({E}), got {len(t)}")
    return t


def _distill_args(name: str, enc_out: Tensor, frame_len: Optional[Tensor], teacher, temperature: float):
    """What both distillation wrappers check and normalise: (enc_out fp32 contiguous, frame_len int32 [B] on its device or None,
    the teacher map, tau)."""
    if not enc_out.is_cuda:
        raise RuntimeError(f"{name} runs on a HIP device only")
    if enc_out.dim() != 4:
        raise ValueError(f"{name}: enc_out must be [E, B, T', V], got {tuple(enc_out.shape)}")
    enc_out = enc_out.contiguous().float()
    E, B, _, V = enc_out.shape
    if V > 256 or V % 4:
        raise ValueError(f"{name} needs a vocabulary of at most 256 entries, a multiple of 4 (got {V}): "
                         "the distillation kernels hold a vocabulary row in one wave")
    return enc_out, _frame_counts(name, "frame_len", frame_len, B, enc_out.device, any_dtype=True), _teacher_map(teacher, E), float(temperature)


def _distill_forward(x: Tensor, frame_len: Optional[Tensor], teacher: Tuple[int, ...], tau: float) -> Tensor:
    E, B, Tq, V = x.shape
    dev = x.device
    lib = capi.load()
    kl = torch.empty((E * B,), dtype=torch.float32, device=dev)
    out = torch.empty((E,), dtype=torch.float32, device=dev)
    nbytes = lib.eec_exit_distill_workspace_bytes(E, B, Tq)
    ws, ws_ptr = capi.aligned_ws(nbytes, dev)
    launch("eec_exit_distill_forward", dev, x, frame_len, (C.c_int32 * E)(*teacher), E, B, Tq, V, tau, kl, out, ws_ptr, nbytes)
    return out


def _distill_backward(x: Tensor, frame_len: Optional[Tensor], teacher: Tuple[int, ...], tau: float, grad_loss: Tensor, accumulate: bool,
                      dx: Tensor) -> None:
    E, B, Tq, V = x.shape
    dev = x.device
    g = grad_loss.to(device=dev, dtype=torch.float32).contiguous()
    launch("eec_exit_distill_backward", dev, x, frame_len, (C.c_int32 * E)(*teacher), E, B, Tq, V, tau, g, int(accumulate), dx)


class _ExitDistillFn(torch.autograd.Function):
    """Per-exit distillation losses [E] with their gradient with respect to the students' rows (eec_exit_distill_forward /
    _backward); the teachers' rows receive none."""

    @staticmethod
    def forward(ctx, enc_out, frame_len, teacher, tau):
        out = _distill_forward(enc_out, frame_len, teacher, tau)
        ctx.save_for_backward(enc_out, frame_len)
        ctx.teacher, ctx.tau = teacher, tau
        return out

    @staticmethod
    def backward(ctx, grad_out):
        enc_out, frame_len = ctx.saved_tensors
        dx = torch.empty_like(enc_out)
        _distill_backward(enc_out, frame_len, ctx.teacher, ctx.tau, grad_out, False, dx)
        return dx, None, None, None


def exit_distill_losses(enc_out: Tensor, frame_len: Optional[Tensor] = None, teacher: Union[str, Sequence[int]] = "last",
                        temperature: float = 1.0) -> Tensor:
    """Per-exit self-distillation losses [E] of an encoder output [E, B, T', V] (logits or log-probs: every row is normalised
    inside): ``loss[e] = tau^2 * mean_b( KL(softmax(x[k] / tau) || softmax(x[e] / tau)) summed over the frames t < frame_len[b],
    / max(frame_len[b], 1) )`` with ``k = teacher[e]`` -- what the reference's ``--distill`` flag ("whether to use knowledge
    distillation") names and util/conf.py:48-57 leaves unimplemented.  ``teacher``: ``"last"`` -- every exit but the last learns
    from the last --, ``"next"`` -- exit e learns from e + 1 --, or E ints (-1: the exit is no student, its loss is 0; a teacher
    may be shallower than its student).  ``frame_len`` [B] (None: T' for every utterance, the reference's CTC convention;
    ``encoder_lengths(lengths, T')`` gives the encoder's own).  The teacher is a constant: the gradient with respect to
    ``enc_out`` (HIP backward) is non-zero on the students' rows only.  One pass over ``enc_out`` per direction."""
    x, fl, tmap, tau = _distill_args("exit_distill_losses", enc_out, frame_len, teacher, temperature)
    if torch.is_grad_enabled() and x.requires_grad:
        return _ExitDistillFn.apply(x, fl, tmap, tau)
    return _distill_forward(x, fl, tmap, tau)


# ---------------------------------------------------------------------------------------------------------------------------
# Adaptive inference: exit statistics and exit choice (include/eec.h states both; csrc/exit_stats.hip)
# ---------------------------------------------------------------------------------------------------------------------------
class ExitStatistics(NamedTuple):
    """Per exit and utterance, [E, B] fp32 each: the average frame entropy (nats), the average frame confidence ``max_v p_v`` and
    the log-probability of the greedy CTC path (a sum over the frames, not divided by their number)."""
    entropy: Tensor
    confidence: Tensor
    greedy_logp: Tensor


EXIT_CRITERIA = {"entropy": False, "confidence": True, "greedy_logp": True}  # criterion -> higher is better


def _exit_stats_args(name: str, enc_out: Tensor, frame_len: Optional[Tensor]):
    """(enc_out fp32 contiguous, frame_len int32 [B] on its device or None), checked as ``_distill_args`` checks them; a CPU tensor
    is allowed (the host path)."""
    if not isinstance(enc_out, Tensor) or enc_out.dim() != 4:
        raise ValueError(f"{name}: enc_out must be [E, B, T', V], got {tuple(getattr(enc_out, 'shape', ()))}")
    if not enc_out.is_floating_point():
        raise ValueError(f"{name}: enc_out must be a floating-point tensor, got {enc_out.dtype}")
    if min(enc_out.shape) < 1:
        raise ValueError(f"{name}: enc_out must not be empty, got {tuple(enc_out.shape)}")
    enc_out = enc_out.contiguous().float()
    E, B, _, V = enc_out.shape
    if E > 16:
        raise ValueError(f"{name}: at most 16 exits, got {E}")
    if V > 256 or V % 4:
        raise ValueError(f"{name} needs a vocabulary of at most 256 entries, a multiple of 4 (got {V}): "
                         "the statistics kernel holds a vocabulary row in one wave")
    return enc_out, _frame_counts(name, "frame_len", frame_len, B, enc_out.device)


def _exit_statistics_host(x: Tensor, frame_len: Optional[Tensor]) -> Tensor:
    """[3, E, B]: the statement of include/eec.h in fp32 torch ops."""
    E, B, T, _ = x.shape
    lens = torch.full((B,), T, dtype=torch.int64, device=x.device) if frame_len is None else frame_len.to(torch.int64).clamp(0, T)
    mask = torch.arange(T, device=x.device).view(1, T) < lens.view(B, 1)
    lp = torch.log_softmax(x, dim=-1)
    p = lp.exp()
    ent = -torch.where(p == 0, torch.zeros_like(p), p * lp).sum(-1)
    top = lp.max(dim=-1).values  # a NaN row gives NaN
    n = lens.clamp(min=1).to(x.dtype)
    add = lambda term: torch.where(mask, term, torch.zeros_like(term)).sum(-1)  # noqa: E731  (a masked frame reaches nothing)
    return torch.stack([add(ent) / n, add(top.exp()) / n, add(top)])


def exit_statistics(enc_out: Tensor, frame_len: Optional[Tensor] = None) -> ExitStatistics:
    """``ExitStatistics(entropy, confidence, greedy_logp)``, each [E, B], of an encoder output [E, B, T', V] (logits or log-probs:
    every row is normalised inside) over the frames ``t < clamp(frame_len[b], 0, T')`` (None: T' for every utterance;
    ``encoder_lengths(lengths, T')`` gives the encoder's own) -- what an early-exit model chooses an utterance's exit by
    (``select_exits``).  An utterance without frames gives 0 / 0 / 0; frames past the length are never read; a NaN inside reaches
    its own (e, b) only.  On the device one pass over ``enc_out`` (eec_exit_stats), bit-reproducible; a CPU tensor takes the host
    path, the same statement in fp32 torch ops."""
    x, fl = _exit_stats_args("exit_statistics", enc_out, frame_len)
    if not x.is_cuda:
        return ExitStatistics(*_exit_statistics_host(x, fl))
    E, B, Tq, V = x.shape
    dev = x.device
    lib = capi.load()
    stats = torch.empty((3, E, B), dtype=torch.float32, device=dev)
    nbytes = lib.eec_exit_stats_workspace_bytes(E, B, Tq)
    ws, ws_ptr = capi.aligned_ws(nbytes, dev)
    launch("eec_exit_stats", dev, x, fl, E, B, Tq, V, stats, ws_ptr, nbytes)
    return ExitStatistics(stats[0], stats[1], stats[2])


def exit_route(score: Tensor, threshold: float, higher_is_better: bool = False, force_all: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """The stable partition of the rows of ``score`` [n] (fp32, on the device) into stayers and leavers (eec_exit_route): row i
    leaves when ``score[i] < threshold`` (``>`` with ``higher_is_better``; a tie or a NaN stays), every row with ``force_all``.
    Returns ``(stay_idx, leave_idx, counts)``, int32 on the device: ``counts = [stayers, leavers]``, the first ``counts[0]``
    entries of ``stay_idx`` and the first ``counts[1]`` of ``leave_idx`` hold the rows in ascending order, the rest hold n."""
    if not score.is_cuda:
        raise RuntimeError("exit_route runs on a HIP device only (select_exits has the host path)")
    if score.dim() != 1 or score.numel() < 1:
        raise ValueError(f"exit_route: score must be [n] with n >= 1, got {tuple(score.shape)}")
    score = score.contiguous().float()
    n, dev = score.numel(), score.device
    idx = torch.full((2, n), n, dtype=torch.int32, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    launch("eec_exit_route", dev, score, n, float(threshold), int(bool(higher_is_better)), int(bool(force_all)), idx[0], idx[1], counts)
    return idx[0], idx[1], counts


def _exit_thresholds(name: str, threshold, E: int) -> Tuple[float, ...]:
    """``threshold`` as one float per exit: a number, or E of them."""
    if isinstance(threshold, Tensor):
        threshold = threshold.tolist()
    t = tuple(float(v) for v in threshold) if isinstance(threshold, (list, tuple)) else (float(threshold),) * E
    if len(t) != E:
        raise ValueError(f"{name}: threshold must be a number or one per exit ({E}), got {len(t)}")
    if any(v != v for v in t):
        raise ValueError(f"{name}: a threshold is NaN")
    return t


def _exit_range(name: str, E: int, min_exit: int, max_exit: Optional[int]) -> Tuple[int, int]:
    lo, hi = int(min_exit), E - 1 if max_exit is None else int(max_exit)
    if not 0 <= lo <= hi < E:
        raise ValueError(f"{name}: need 0 <= min_exit <= max_exit < {E}, got min_exit {lo}, max_exit {hi}")
    return lo, hi


def select_exits(score: Tensor, threshold, higher_is_better: bool = False, min_exit: int = 0, max_exit: Optional[int] = None) -> Tensor:
    """The exit of every utterance, int32 [B], 0-based, from a table ``score`` [E, B] (a field of ``exit_statistics``, or any
    caller-supplied criterion such as the N-best posterior ``ctc_predict`` returns): the first exit e in ``[min_exit, max_exit]``
    whose score passes ``threshold[e]`` -- is below it, or above it with ``higher_is_better``; a tie or a NaN does not pass --, and
    ``max_exit`` (default E - 1) where none does.  ``threshold``: a float, or E floats.  On the device one eec_exit_route launch per
    exit considered and no host synchronisation; a CPU table takes the host path."""
    if not isinstance(score, Tensor) or score.dim() != 2 or min(score.shape) < 1:
        raise ValueError(f"select_exits: score must be [E, B], got {tuple(getattr(score, 'shape', ()))}")
    if not score.is_floating_point():
        raise ValueError(f"select_exits: score must be a floating-point tensor, got {score.dtype}")
    E, B = score.shape
    thr = _exit_thresholds("select_exits", threshold, E)
    lo, hi = _exit_range("select_exits", E, min_exit, max_exit)
    score = score.float()
    out = torch.full((B,), hi, dtype=torch.int32, device=score.device)
    for e in range(hi - 1, lo - 1, -1):  # the last exit takes whoever is left: its own score is not looked at
        if score.is_cuda:
            leave_idx = exit_route(score[e], thr[e], higher_is_better)[1]
            passed = torch.zeros((B + 1,), dtype=torch.bool, device=score.device)
            passed[leave_idx.long()] = True  # the unwritten tail of leave_idx holds B
            passed = passed[:B]
        else:
            passed = score[e] > thr[e] if higher_is_better else score[e] < thr[e]
        out = torch.where(passed, torch.full_like(out, e), out)
    return out


class _ExitTrainingFn(torch.autograd.Function):
    """(CTC losses [E], distillation losses [E]) as ONE node: its backward runs eec_ctc_loss_backward[_len] into a fresh gradient
    buffer -- every element of it is written, the rows past an utterance's ``input_len`` as zeros -- and the distillation backward
    adds into the same buffer, so autograd neither copies nor re-adds the CTC gradient."""

    @staticmethod
    def forward(ctx, enc_out, tg, tl, blank, frame_len, teacher, tau, il=None):
        ctc, nll, ws, ws_ptr = _ctc_forward(enc_out, tg, tl, blank, il)
        kd = _distill_forward(enc_out, frame_len, teacher, tau)
        ctx.set_materialize_grads(False)  # a loss that uses one of the two outputs only: None for the other, and its launch is skipped
        ctx.save_for_backward(enc_out, tg, tl, nll, ws, frame_len, il)
        ctx.blank, ctx.ws_ptr, ctx.teacher, ctx.tau = blank, ws_ptr, teacher, tau
        return ctc, kd

    @staticmethod
    def backward(ctx, grad_ctc, grad_kd):
        enc_out, tg, tl, nll, ws, frame_len, il = ctx.saved_tensors
        if getattr(ctx, "used", False):
            raise RuntimeError("exit_training_losses: backward through the same forward twice (its workspace is consumed)")
        ctx.used = True
        dlogp = torch.empty_like(enc_out)
        if grad_ctc is not None:
            _ctc_backward(enc_out, tg, tl, ctx.blank, il, nll, ctx.ws_ptr, grad_ctc, dlogp)
        if grad_kd is not None:
            _distill_backward(enc_out, frame_len, ctx.teacher, ctx.tau, grad_kd, grad_ctc is not None, dlogp)
        elif grad_ctc is None:
            dlogp.zero_()
        return dlogp, None, None, None, None, None, None, None


def exit_training_losses(enc_out: Tensor, targets: Tensor, target_len: Tensor, frame_len: Optional[Tensor] = None,
                         teacher: Union[str, Sequence[int]] = "last", temperature: float = 1.0, blank: int = 0,
                         input_len: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``(exit_ctc_losses(enc_out, targets, target_len, blank, input_len), exit_distill_losses(enc_out, frame_len, teacher,
    temperature))``, the same values bit for bit, as one autograd node: ``ctc.sum() + w * kd.sum()`` is the training loss with
    distillation, and its backward writes the CTC gradient into a fresh buffer and adds the distillation gradient into the same
    buffer (with ``w = 0`` that is the gradient of ``exit_ctc_losses`` bit for bit).  The two masks are separate arguments:
    ``frame_len`` masks the distillation term only and ``input_len`` the CTC loss only (None: T' for every utterance, the
    reference's convention, for either).  On a ragged batch pass ``encoder_lengths(lengths, T')`` as both."""
    x, fl, tmap, tau = _distill_args("exit_training_losses", enc_out, frame_len, teacher, temperature)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return exit_ctc_losses(x, targets, target_len, blank, input_len), _distill_forward(x, fl, tmap, tau)
    dev = x.device
    il = _frame_counts("exit_training_losses", "input_len", input_len, x.size(1), dev)
    return _ExitTrainingFn.apply(x, to_device(targets, dev), to_device(target_len, dev), blank, fl, tmap, tau, il)


# ---------------------------------------------------------------------------------------------------------------------------
# MWER training of the CTC exits (include/eec.h states the loss; csrc/ctc_mwer.hip)
# ---------------------------------------------------------------------------------------------------------------------------
MWER_MAX_NBEST, MWER_MAX_LEN = 16, 255


class MwerLists(NamedTuple):
    """The N-best lists of every exit and utterance as MWER training takes them: ``tokens`` [E, B, N, L] int32, ``lengths``
    [E, B, N] int32 (-1: no such hypothesis), ``risk`` [E, B, N] fp32 (the token edit distance to the utterance's target) and
    ``scores`` [E, B, N] fp32 (the beam's pruned scores, -inf for an absent entry)."""
    tokens: Tensor
    lengths: Tensor
    risk: Tensor
    scores: Tensor


def _mwer_args(name: str, enc_out: Tensor, hyp: Tensor, hyp_len: Tensor, risk: Optional[Tensor], input_len: Optional[Tensor]):
    """(enc_out contiguous -- fp32 on a device, its own floating dtype on the CPU --, input_len int32 [B] or None, hyp int32
    [E, B, N, L >= 1], hyp_len int32 [E, B, N], risk [E, B, N] in enc_out's dtype or None), all on enc_out's device."""
    if not isinstance(enc_out, Tensor) or enc_out.dim() != 4 or not enc_out.is_floating_point() or min(enc_out.shape) < 1:
        raise ValueError(f"{name}: enc_out must be a non-empty floating-point [E, B, T', V], got {tuple(getattr(enc_out, 'shape', ()))}")
    dev = enc_out.device
    x = enc_out.contiguous().float() if enc_out.is_cuda else enc_out.contiguous()
    E, B = x.shape[:2]
    if not isinstance(hyp, Tensor) or hyp.dim() != 4 or tuple(hyp.shape[:2]) != (E, B) or hyp.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: hyp must be an int32 or int64 [E, B, N, L] = [{E}, {B}, N, L], got {tuple(getattr(hyp, 'shape', ()))}")
    N = hyp.size(2)
    if not 1 <= N <= MWER_MAX_NBEST:
        raise ValueError(f"{name}: lists of 1 to {MWER_MAX_NBEST} hypotheses are served, got N = {N}")
    if hyp.dtype == torch.int64:
        hyp = hyp.clamp(-1, 2 ** 31 - 1)  # a label int32 cannot hold is refused on the device like any label outside [0, V)
    hyp = hyp.to(device=dev, dtype=torch.int32)
    if hyp.size(3) == 0:
        hyp = hyp.new_zeros((E, B, N, 1))
    if not isinstance(hyp_len, Tensor) or tuple(hyp_len.shape) != (E, B, N) or hyp_len.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: hyp_len must be an int32 or int64 [{E}, {B}, {N}], got {tuple(getattr(hyp_len, 'shape', ()))}")
    if hyp_len.dtype == torch.int64:
        hyp_len = hyp_len.clamp(-2, 2 ** 31 - 1)
    hl = hyp_len.to(device=dev, dtype=torch.int32).contiguous()
    if risk is not None:
        if not isinstance(risk, Tensor) or tuple(risk.shape) != (E, B, N):
            raise ValueError(f"{name}: risk must be [{E}, {B}, {N}], got {tuple(getattr(risk, 'shape', ()))}")
        risk = risk.detach().to(device=dev, dtype=x.dtype).contiguous()
    return x, _frame_counts(name, "input_len", input_len, B, dev), hyp.contiguous(), hl, risk


def _mwer_host_ll(x: Tensor, il: Optional[Tensor], hyp: Tensor, hl: Tensor, blank: int):
    """The host path: (ll [E, B, N] in ``x``'s dtype, differentiable through torch's ``F.ctc_loss``; refused [E, B, N] bool)."""
    E, B, T, V = x.shape
    N, L = hyp.shape[2:]
    G = E * B * N
    ninf = float("-inf")
    Tb = torch.full((B,), T, dtype=torch.int64) if il is None else il.to(torch.int64).clamp(0, T)
    len_ok = (hl >= -1) & (hl <= min(L, MWER_MAX_LEN))
    lens = torch.where(len_ok, hl, torch.full_like(hl, -1)).to(torch.int64)
    tok = hyp.to(torch.int64)
    inside = torch.arange(L).view(1, 1, 1, L) < lens.unsqueeze(-1)
    refused = ~len_ok | (inside & ((tok < 0) | (tok >= V) | (tok == blank))).any(-1)
    present = (lens >= 0) & ~refused
    frames = Tb.view(1, B, 1).expand(E, B, N).reshape(G)
    lp = x.unsqueeze(2).expand(E, B, N, T, V).reshape(G, T, V).permute(1, 0, 2)
    lp = torch.where(torch.arange(T).view(T, 1, 1) < frames.view(1, G, 1), lp, torch.zeros_like(lp))  # frames at or past Tb are not read
    tl = torch.where(present, lens, torch.zeros_like(lens)).reshape(G)
    tg = tok.clamp(0, V - 1).reshape(G, L)
    args = (tg, frames.clamp(min=1), tl)
    with torch.no_grad():
        infeasible = torch.nn.functional.ctc_loss(lp.detach(), *args, blank=blank, reduction="none", zero_infinity=False) == float("inf")
    ll = -torch.nn.functional.ctc_loss(lp, *args, blank=blank, reduction="none", zero_infinity=True)
    ll = torch.where(infeasible, torch.full_like(ll, ninf), ll)
    ll = torch.where(frames == 0, torch.where(tl == 0, torch.zeros_like(ll), torch.full_like(ll, ninf)), ll)
    ll = torch.where(present.reshape(G), ll, torch.full_like(ll, ninf))
    ll = torch.where(refused.reshape(G), torch.full_like(ll, float("nan")), ll)
    return ll.view(E, B, N), refused


def _mwer_host_loss(ll: Tensor, refused: Tensor, risk: Tensor) -> Tensor:
    """loss_eb [E, B] of include/eec.h from ll and risk [E, B, N], in torch ops (autograd gives sum_i c_i d ll_i)."""
    ninf = float("-inf")
    in_p = torch.isfinite(ll)
    llm = torch.where(in_p, ll, torch.full_like(ll, ninf))
    m = llm.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m)).detach()
    w = torch.where(in_p, (llm - m).exp(), torch.zeros_like(ll))
    z = w.sum(-1, keepdim=True)
    phat = w / torch.where(z > 0, z, torch.ones_like(z))
    cnt = in_p.sum(-1, keepdim=True)
    rk = torch.where(in_p, risk, torch.zeros_like(risk))
    rmin = torch.where(in_p, risk, torch.full_like(risk, float("inf"))).min(-1, keepdim=True).values
    rmax = torch.where(in_p, risk, torch.full_like(risk, ninf)).max(-1, keepdim=True).values
    rbar = torch.where(rmin == rmax, rmin, rk.sum(-1, keepdim=True) / cnt.clamp(min=1).to(risk.dtype))
    # sum_i phat_i (risk_i - rbar) with the risks measured from the likeliest entry's, which changes neither the value nor the
    # gradient; autograd's softmax backward then cancels nothing when that entry holds nearly all the mass
    rdom = torch.where(in_p.any(-1, keepdim=True), risk.gather(-1, llm.argmax(-1, keepdim=True)), torch.zeros_like(rbar))
    loss_eb = (phat * torch.where(in_p, risk - rdom, torch.zeros_like(risk))).sum(-1) + (rdom - rbar).squeeze(-1)
    poisoned = refused.any(-1) | (torch.isnan(ll) & ~refused).any(-1)
    return torch.where(poisoned, torch.full_like(loss_eb, float("nan")), loss_eb)


def _mwer_chunks(x: Tensor, N: int, L: int, max_workspace_bytes: int):
    """[(b0, nb)]: the batch in runs of utterances whose workspace stays inside ``max_workspace_bytes`` (one utterance at least)."""
    E, B, Tq, _ = x.shape
    per_utt = max(capi.load().eec_ctc_mwer_workspace_bytes(E, 1, Tq, N, L), 1)
    step = min(B, max(1, int(max_workspace_bytes) // per_utt))
    return [(b0, min(step, B - b0)) for b0 in range(0, B, step)]


def _mwer_forward_chunk(x, il, hyp, hl, risk, blank, b0, nb, ll, loss_eb, loss, ws_ptr, nbytes):
    E, B, Tq, V = x.shape
    N, L = hyp.shape[2:]
    launch("eec_ctc_mwer_forward", x.device, x, il, hyp, hl, risk, E, B, b0, nb, Tq, V, N, L, int(blank), ll, loss_eb, loss, ws_ptr, nbytes)


def _mwer_forward(x: Tensor, il: Optional[Tensor], hyp: Tensor, hl: Tensor, risk: Tensor, blank: int, max_workspace_bytes: int):
    """(loss [E], ll [E, B, N], loss_eb [E, B], kept): ``kept`` = (workspace tensor, aligned address, bytes) when the batch went
    through as one chunk -- the backward reads it --, None when it was split (the backward then redoes the forward chunk by chunk)."""
    E, B, Tq, _ = x.shape
    N, L = hyp.shape[2:]
    dev = x.device
    lib = capi.load()
    ll = torch.empty((E, B, N), dtype=torch.float32, device=dev)
    loss_eb = torch.empty((E, B), dtype=torch.float32, device=dev)
    loss = torch.empty((E,), dtype=torch.float32, device=dev)
    chunks = _mwer_chunks(x, N, L, max_workspace_bytes)
    with torch.cuda.device(dev):
        nbytes = lib.eec_ctc_mwer_workspace_bytes(E, chunks[0][1], Tq, N, L)  # the first chunk is the largest
        ws, ws_ptr = capi.aligned_ws(nbytes, dev)
        for b0, nb in chunks:
            _mwer_forward_chunk(x, il, hyp, hl, risk, blank, b0, nb, ll, loss_eb, loss, ws_ptr, nbytes)
    return loss, ll, loss_eb, ((ws, ws_ptr, nbytes) if len(chunks) == 1 else None)


def _mwer_backward(x: Tensor, il: Optional[Tensor], hyp: Tensor, hl: Tensor, risk: Tensor, blank: int, max_workspace_bytes: int, kept,
                   grad_loss: Tensor, accumulate: bool, dlogp: Tensor) -> None:
    """eec_ctc_mwer_backward into ``dlogp`` (written in full, or added into)."""
    E, B, Tq, V = x.shape
    N, L = hyp.shape[2:]
    dev = x.device
    lib = capi.load()
    g = grad_loss.to(device=dev, dtype=torch.float32).contiguous()

    def back(b0, nb, ws_ptr, nbytes):
        launch("eec_ctc_mwer_backward", dev, x, il, hyp, hl, E, B, b0, nb, Tq, V, N, L, int(blank), ws_ptr, nbytes, g,
               int(bool(accumulate)), dlogp)
    with torch.cuda.device(dev):
        if kept is not None:
            back(0, B, kept[1], kept[2])
            return
        chunks = _mwer_chunks(x, N, L, max_workspace_bytes)
        nbytes = lib.eec_ctc_mwer_workspace_bytes(E, chunks[0][1], Tq, N, L)
        ws, ws_ptr = capi.aligned_ws(nbytes, dev)
        scratch = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((E, B, N), (E, B), (E,))]
        for b0, nb in chunks:
            _mwer_forward_chunk(x, il, hyp, hl, risk, blank, b0, nb, *scratch, ws_ptr, nbytes)
            back(b0, nb, ws_ptr, nbytes)


def _mwer_check_vocab(name: str, V: int) -> None:
    if V > 256 or V % 4:
        raise ValueError(f"{name} with a gradient needs a vocabulary of at most 256 entries, a multiple of 4 (got {V}): "
                         "a gradient row is one float4 per lane")


class _ExitMwerFn(torch.autograd.Function):
    """Per-exit MWER losses [E] with their gradient with respect to the log-probs (eec_ctc_mwer_forward / _backward)."""

    @staticmethod
    def forward(ctx, enc_out, il, hyp, hl, risk, blank, max_ws):
        _mwer_check_vocab("exit_mwer_losses", enc_out.size(3))
        loss, _, _, kept = _mwer_forward(enc_out, il, hyp, hl, risk, blank, max_ws)
        ctx.save_for_backward(enc_out, il, hyp, hl, risk)
        ctx.blank, ctx.max_ws, ctx.kept = blank, max_ws, kept
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        enc_out, il, hyp, hl, risk = ctx.saved_tensors
        dlogp = torch.empty_like(enc_out)
        _mwer_backward(enc_out, il, hyp, hl, risk, ctx.blank, ctx.max_ws, ctx.kept, grad_out, False, dlogp)
        return dlogp, None, None, None, None, None, None


def ctc_hyp_logp(enc_out: Tensor, hyp: Tensor, hyp_len: Tensor, input_len: Optional[Tensor] = None, blank: int = 0) -> Tensor:
    """The exact CTC log-likelihood ``ll`` [E, B, N] of every hypothesis ``hyp[e, b, i, :hyp_len[e, b, i]]`` of N-best lists
    [E, B, N, L] against the log-probs ``enc_out[e, b, :input_len[b]]`` (eec_ctc_hyp_logp): the full forward sum, divided by
    nothing -- where a beam's score is a pruned sum and ``exit_ctc_losses`` divides by the target length.  -inf for an infeasible
    hypothesis and for an absent one (``hyp_len`` -1), NaN for a length outside [-1, min(L, 255)] or a label outside the
    vocabulary or equal to ``blank``.  One launch, no workspace; not differentiable (``exit_mwer_losses`` is).  CPU tensors take
    the host path: torch's own ``F.ctc_loss`` in the tensor's dtype."""
    x, il, hyp, hl, _ = _mwer_args("ctc_hyp_logp", enc_out, hyp, hyp_len, None, input_len)
    if not x.is_cuda:
        with torch.no_grad():
            return _mwer_host_ll(x, il, hyp, hl, int(blank))[0]
    E, B, Tq, V = x.shape
    N, L = hyp.shape[2:]
    ll = torch.empty((E, B, N), dtype=torch.float32, device=x.device)
    launch("eec_ctc_hyp_logp", x.device, x, il, hyp, hl, E, B, Tq, V, N, L, int(blank), ll)
    return ll


def exit_mwer_losses(enc_out: Tensor, hyp: Tensor, hyp_len: Tensor, risk: Tensor, input_len: Optional[Tensor] = None, blank: int = 0,
                     max_workspace_bytes: int = 2 << 30) -> Tensor:
    """Per-exit MWER losses [E] of an encoder output [E, B, T', V] (log-probs) against N-best lists ``hyp`` [E, B, N, L] /
    ``hyp_len`` [E, B, N] (-1: absent) with the caller's error counts ``risk`` [E, B, N] (``mwer_nbest`` makes all three):
    ``loss[e] = mean_b sum_i phat_i (risk_i - mean risk)``, ``phat`` the softmax over the list of the hypotheses' exact CTC
    log-likelihoods (include/eec.h has the statement and its edge cases).  Differentiable with respect to ``enc_out``: the HIP
    backward walks the N lattices of a list over the same frames and writes one gradient row per frame.  The lists and the risks
    are constants.  The alphas of all lattices go to a workspace; above ``max_workspace_bytes`` the batch is split over utterances
    (the backward then redoes each chunk's forward), with the bits of the unsplit call.  fp64 and non-contiguous device input is
    converted; CPU tensors take the host path, the same statement through torch's ``F.ctc_loss`` and autograd in the tensor's dtype."""
    x, il, hyp, hl, risk = _mwer_args("exit_mwer_losses", enc_out, hyp, hyp_len, risk, input_len)
    if not x.is_cuda:
        ll, refused = _mwer_host_ll(x, il, hyp, hl, int(blank))
        return _mwer_host_loss(ll, refused, risk).mean(1)
    if torch.is_grad_enabled() and x.requires_grad:
        return _ExitMwerFn.apply(x, il, hyp, hl, risk, int(blank), int(max_workspace_bytes))
    return _mwer_forward(x, il, hyp, hl, risk, int(blank), int(max_workspace_bytes))[0]


def mwer_nbest(enc_out: Tensor, targets: Tensor, target_len: Tensor, nbest: int = 4, beam_size: int = 10, input_len: Optional[Tensor] = None,
               blank: int = 0, blank_skip_threshold: float = 0.95) -> MwerLists:
    """The ``MwerLists`` of an encoder output [E, B, T', V] on the device, under ``no_grad``: one ``ctc_beam_decode(nbest=)`` call
    over the E * B emissions, the token pitch cut to the longest hypothesis, ``lengths`` -1 for the ranks at or past the beam's
    ``n_hyp`` and for hypotheses of more than 255 tokens, and ``risk`` the token edit distance to ``targets[b, :target_len[b]]``
    from one ``scoring.edit_counts`` call."""
    from . import scoring
    if not enc_out.is_cuda:
        raise RuntimeError("mwer_nbest runs on a HIP device only")
    with torch.no_grad():
        x = enc_out.detach().contiguous().float()
        E, B, Tq, V = x.shape
        dev = x.device
        il = _frame_counts("mwer_nbest", "input_len", input_len, B, dev)
        tokens, counts, scores, n_hyp = ctc_beam_decode(x.view(E * B, Tq, V), beam_size, blank, blank_skip_threshold,
                                                        em_len=None if il is None else il.repeat(E), nbest=int(nbest))
        present = torch.arange(int(nbest), device=dev).view(1, -1) < n_hyp.view(-1, 1)
        lengths = torch.where(present & (counts <= MWER_MAX_LEN), counts, torch.full_like(counts, -1))
        L = max(int(lengths.max()), 1)
        tokens = tokens[:, :, :L].contiguous()
        ref = targets.to(device=dev)
        ref_of = (torch.arange(E * B, device=dev, dtype=torch.int32) % B).repeat_interleave(int(nbest))
        dist = scoring.edit_counts(tokens.view(-1, L), lengths.clamp(min=0).reshape(-1), ref if ref.dtype == torch.int32 else ref.to(torch.int64),
                                   target_len.to(device=dev), ref_of=ref_of).distance
        return MwerLists(tokens.view(E, B, int(nbest), L), lengths.view(E, B, int(nbest)), dist.to(torch.float32).view(E, B, int(nbest)),
                         scores.view(E, B, int(nbest)))


class _ExitMwerTrainingFn(torch.autograd.Function):
    """(CTC losses [E], MWER losses [E]) as ONE node, in the manner of ``_ExitTrainingFn``: the backward writes the CTC gradient
    into a fresh buffer and the MWER backward adds into the same buffer."""

    @staticmethod
    def forward(ctx, enc_out, tg, tl, blank, il, hyp, hl, risk, max_ws):
        ctc, nll, ws, ws_ptr = _ctc_forward(enc_out, tg, tl, blank, il)
        mwer, _, _, kept = _mwer_forward(enc_out, il, hyp, hl, risk, blank, max_ws)
        ctx.set_materialize_grads(False)  # a loss that uses one of the two outputs only: None for the other, and its launch is skipped
        ctx.save_for_backward(enc_out, tg, tl, nll, ws, il, hyp, hl, risk)
        ctx.blank, ctx.ws_ptr, ctx.max_ws, ctx.kept = blank, ws_ptr, max_ws, kept
        return ctc, mwer

    @staticmethod
    def backward(ctx, grad_ctc, grad_mwer):
        enc_out, tg, tl, nll, ws, il, hyp, hl, risk = ctx.saved_tensors
        if getattr(ctx, "used", False):
            raise RuntimeError("exit_mwer_training_losses: backward through the same forward twice (the CTC workspace is consumed)")
        ctx.used = True
        dlogp = torch.empty_like(enc_out)
        if grad_ctc is not None:
            _ctc_backward(enc_out, tg, tl, ctx.blank, il, nll, ctx.ws_ptr, grad_ctc, dlogp)
        if grad_mwer is not None:
            _mwer_backward(enc_out, il, hyp, hl, risk, ctx.blank, ctx.max_ws, ctx.kept, grad_mwer, grad_ctc is not None, dlogp)
        elif grad_ctc is None:
            dlogp.zero_()
        return (dlogp,) + (None,) * 8


def exit_mwer_training_losses(enc_out: Tensor, targets: Tensor, target_len: Tensor, lists: Optional[MwerLists] = None, nbest: int = 4,
                              beam_size: int = 10, input_len: Optional[Tensor] = None, blank: int = 0,
                              max_workspace_bytes: int = 2 << 30) -> Tuple[Tensor, Tensor]:
    """``(exit_ctc_losses(enc_out, targets, target_len, blank, input_len), exit_mwer_losses(enc_out, lists.tokens, lists.lengths,
    lists.risk, input_len, blank))``, the same values bit for bit, as one autograd node: ``ctc.sum() * lam + mwer.sum()`` is the
    usual interpolated MWER objective, and its backward writes the CTC gradient into a fresh buffer and adds the MWER gradient into
    it (with the MWER output unused that is the gradient of ``exit_ctc_losses`` bit for bit).  ``lists``: None -- decoded here,
    ``mwer_nbest(enc_out, targets, target_len, nbest, beam_size, input_len, blank)`` --, or lists made earlier."""
    if not enc_out.is_cuda:
        raise RuntimeError("exit_mwer_training_losses runs on a HIP device only")
    if lists is None:
        lists = mwer_nbest(enc_out, targets, target_len, nbest, beam_size, input_len, blank)
    x, il, hyp, hl, risk = _mwer_args("exit_mwer_training_losses", enc_out, lists.tokens, lists.lengths, lists.risk, input_len)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return (exit_ctc_losses(x, targets, target_len, blank, input_len),
                _mwer_forward(x, il, hyp, hl, risk, int(blank), int(max_workspace_bytes))[0])
    _mwer_check_vocab("exit_mwer_training_losses", x.size(3))
    dev = x.device
    return _ExitMwerTrainingFn.apply(x, to_device(targets, dev), to_device(target_len, dev), int(blank), il, hyp, hl, risk,
                                     int(max_workspace_bytes))
