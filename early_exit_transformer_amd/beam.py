"""Decoders on top of the HIP encoder: mirrors of the reference's ``util/beam_infer.py``, served without torchaudio.

* ``GreedyCTCDecoder``            util/beam_infer.py:9-24, on the batched HIP kernel (``eec_greedy_ctc``).
* ``BeamInference.beam_search``   util/beam_infer.py:198-307: the AED beam search that ``inference.py:44-51`` drives per
  utterance and exit.  Same signature, same arithmetic and the same quirks (the length penalty DIVIDES the step's
  log-probs; ``min_length`` defaults to 300, so EOS never finalises a beam inside ``max_length`` steps; the best beam
  is the one with the highest accumulated score), but the candidate bookkeeping runs as tensor ops on the device
  instead of a Python loop over beams, and ``decode_all_exits`` runs the encoder ONCE for all exits (one
  ``eec_encoder_forward`` with taps) where the reference re-runs the first n exit groups for every n
  (inference.py:44-46: O(E^2) groups per utterance), and the decoder advances step-wise over a key / value cache
  (``model.decoder_session``, csrc/decoder_step.hip) where the reference re-runs it on the whole prefix per step.
* ``BeamInference.get_trellis`` / ``backtrack``  util/beam_infer.py:129-191: the Viterbi forced alignment of a token
  sequence against one exit's CTC log-probs, on the device (``ctc_align``, csrc/ctc_align.hip); ``ctc_rescore`` and the
  ``ctc_weight`` keyword of the batched searches are the reference's dormant joint choice (util/beam_infer.py:309-383): the
  best beam by ``weight_ctc * s_ctc + (1 - weight_ctc) * s_pred``.
* ``BeamInference.decode_batch``  inference.py:18-62 (evaluate_batch_ae) for a whole padded batch: the encoder once per
  batch, then the searches of every exit and utterance in lockstep (``beam_search_batch``, csrc/decoder_batch.hip).
* ``BeamInference.ctc_predict`` / ``ctc_predict_``  util/beam_infer.py:93-126: the lexicon-constrained CTC beam search with
  N-best (torchaudio's ``ctc_decoder(lexicon=..., lm=..., lm_weight=LM_WEIGHT)``) on the device (``ctc_lexicon_decode``,
  csrc/ctc_lexbeam.hip): words that are lexicon entries by construction, and the posterior of the top hypothesis; with ``lm=`` or
  ``args.lm`` -- an ARPA file -- under a back-off n-gram word model (``lexicon.NGramLM``), else without one; with
  ``smearing="max"`` or ``args.lm_smearing`` with LM look-ahead inside words (max trie smearing, which the third-party decoder
  always applies; off by default here); with ``log_add=True`` or ``args.lm_log_add`` with log-add merging.
* ``BeamInference.beam_predict``  util/beam_infer.py:66-75, 85-90: the character-lexicon decoder (``log_add=True``,
  ``word_score=WORD_SCORE``, torchaudio's default token names) over ``model.ctc_encoder``'s emission, on the same kernel.
* ``BeamInference.joint_search_batch`` / ``joint_search_exits`` and ``joint_ctc_weight=`` on ``decode_batch`` /
  ``decode_all_exits``: one-pass joint CTC / attention decoding (Watanabe et al. 2017; not in the reference).  Every candidate of
  every step is scored by the decoder AND by the CTC prefix probability of the extended labels (``ctc_prefix_session``,
  csrc/ctc_prefix.hip), EOS by the full-sequence CTC likelihood, so a beam can end; semantics in include/eec.h.
* ``BeamInference.rescore_batch`` / ``decode_batch_rescoring`` and ``rescoring_ctc_weight=`` on ``decode_batch_adaptive``: two-pass
  decoding (not in the reference).  The CTC head proposes an N-best list (``ctc_beam_decode(nbest=)``, csrc/ctc_beam.hip), the
  attention decoder scores the whole list in one teacher-forced pass (``model.score_hypotheses``, csrc/decoder_score.hip), and the
  best hypothesis is the one with the highest ``(1 - w) * att + w * ctc``: no autoregressive loop, no key / value cache.
* ``BeamInference.spot``: keyword and phrase spotting (not in the reference): one encoder pass, then every keyword of a
  ``KeywordSet`` against the CTC emissions of all exits (``keyword_search``, csrc/keyword.hip), and the shallowest exit that hits.
* ``BeamInference.timestamps``: token and word timestamps with confidences (not in the reference): one encoder pass, then the
  transcripts any decoder above returned aligned against the CTC emission of an exit, or of every exit, in the standard CTC
  topology (``ctc_forced_align``, csrc/ctc_forced_align.hip).
* ``lexicon=`` / ``detokenize=`` on ``decode_batch`` and ``ctc_cuda_predict``: the ``apply_lex`` step inference.py:51,71 puts
  every printed hypothesis through, for all hypotheses of the call in one device search (``lexicon.Lexicon.apply_batch``).
* ``BeamInference.error_table``: what any of the decoders above returned, scored against references (``scoring.error_table``;
  csrc/edit_distance.hip): errors with their substitution / deletion / insertion split per exit and utterance, in tokens, or in
  words / characters after ``detokenize`` and ``apply_lex``.  The reference leaves this to tools outside its tree.

Every lockstep search, plain and joint, is one loop (``_lockstep_search``) over an ordered sequence of scorers -- the CTC prefix
session, the context bias, the language model: sessions over ``decoding.ScorerSession`` -- and a call's ``context`` / ``graph_of`` /
``token_lm`` / ``token_lm_weight`` / ``token_score`` are resolved once into ``_Modifiers``, which the public methods hand to each other.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .alignment import FRAME_SECONDS, Alignment, ctc_forced_align, exit_rows, starts_word_from_pieces, transcript_rows, word_spans
from .context import ContextBiasSession, ContextGraph
from .keyword import KeywordSet, keyword_search
from .lm_fusion import DEFAULT_LM_WEIGHT, LMFusionSession, TokenLM, check_lm
from .lexicon import NGramLM, TokenTrie, as_lexicon
from .model import beam_select, ctc_align, ctc_beam_decode, ctc_lexicon_decode, ctc_prefix_session, encoder_lengths, greedy_ctc
from .posterior import TOKEN_FIELDS, Posteriors, ctc_posteriors, soft_word_spans
from .segment import ctc_segment, utterance_spans, windowed_emission


class GreedyCTCDecoder(torch.nn.Module):
    """``forward(emission[T', V]) -> List[int]``: argmax, collapse repeats, drop blank (util/beam_infer.py:9-24)."""

    def __init__(self, blank: int = 0):
        super().__init__()
        self.blank = blank

    def forward(self, emission: Tensor) -> List[int]:
        tokens, counts = greedy_ctc(emission.unsqueeze(0), self.blank)
        return tokens[0, : int(counts[0])].tolist()


@dataclass
class Point:
    """util/beam_infer.py:27-31: one frame of an alignment path (score: cumulative, summed from the last frame)."""
    token_index: int
    time_index: int
    score: float


def sequence_length_penalty(length: int, alpha: float = 0.6) -> float:
    """util/beam_infer.py:194-195."""
    return ((5 + length) / (5 + 1)) ** alpha


class CTCHypothesis:
    """One CTC beam-search hypothesis, with the attribute names of torchaudio's ``CUCTCHypothesis`` (tokens: List[int] without
    blanks / repeats, words: List[str] -- empty here, as for a lexicon-free decoder --, score: float).  ``bias`` is set by a search
    under a context graph only: the contextual bias the hypothesis was ranked with, beside its ``score``; ``fusion`` by a search under
    a token-level language model only: its shallow-fusion score, in the same way."""
    __slots__ = ("tokens", "words", "score", "text", "bias", "fusion")

    def __init__(self, tokens, words, score, text=None):
        self.tokens, self.words, self.score, self.text = tokens, words, score, text

    def __repr__(self):
        return f"CTCHypothesis(tokens={self.tokens}, words={self.words}, score={self.score:.4f})"


class DecodedTokens(list):
    """The token ids of one decoded hypothesis -- a plain list to every caller -- that also carry ``text``: the detokenised ids
    after ``apply_lex``."""
    text: Optional[str] = None


class RescoredList(NamedTuple):
    """The N-best list of one two-pass search (``BeamInference.rescore_batch``), best CTC score first: the present hypotheses'
    ids, their CTC and attention log-probabilities and the joint score the best one was chosen by."""
    tokens: List[List[int]]
    ctc: List[float]
    att: List[float]
    joint: List[float]


class Timestamps(NamedTuple):
    """What ``BeamInference.timestamps`` returns: per utterance ([B], or [E][B] for ``exits="all"``) the ``TokenSpan`` list and --
    with ``pieces`` -- the ``WordSpan`` list (else ``words`` is None), and the ``Alignment`` they were read off."""
    tokens: list
    words: Optional[list]
    alignment: Alignment


class Segmentation(NamedTuple):
    """What ``BeamInference.segment`` returns: the ``Alignment`` of the concatenated transcript (one row), the ``UtteranceSpan``
    of every utterance and -- with ``pieces`` -- the ``WordSpan`` list of every utterance (else ``words`` is None)."""
    alignment: Alignment
    utterances: list
    words: Optional[list]


class Confidences(NamedTuple):
    """What ``BeamInference.confidences`` returns: per utterance ([B], or [E][B] for ``exits="all"``) the ``SoftSpan`` list and --
    with ``pieces`` -- the ``SoftWordSpan`` list (else ``words`` is None), and the ``Posteriors`` they were read off."""
    tokens: list
    words: Optional[list]
    posteriors: Posteriors


class FusedRescoredList(RescoredList):
    """``RescoredList`` of a two-pass search under a token-level language model: it also carries ``fusion``, the shallow-fusion
    scores of the list, which entered ``joint``."""
    fusion: List[float]


def _snapped_texts(token_lists, lexicon, detokenize) -> List[str]:
    """inference.py:50-51 / 70-71 for many hypotheses: ``apply_lex(detokenize(ids), lexicon)`` each, the lexicon searched once."""
    return as_lexicon(lexicon).apply_batch([detokenize(list(t)) for t in token_lists])


def _with_texts(out, lexicon, detokenize, cut=lambda ids: ids):
    """The table ``out[b][e]`` of decoded ids, with ``lexicon`` and ``detokenize`` both given as ``DecodedTokens`` that carry their
    ``.text``: the snapped text of ``cut(ids)``, all of them resolved in one lexicon search."""
    if lexicon is None or detokenize is None:
        return out
    texts = iter(_snapped_texts([cut(ids) for row in out for ids in row], lexicon, detokenize))
    out = [[DecodedTokens(ids) for ids in row] for row in out]
    for row in out:
        for ids in row:
            ids.text = next(texts)
    return out


def default_max_length(T: int) -> int:
    """inference.py:31-39 (p = 30, m = 5 / 200): the decoding length for T input frames."""
    return int(30 - T * 5 / 200) if T < 200 else int(T / 12)


def _lockstep_kw(kw: dict) -> Optional[dict]:
    """The keywords for a lockstep search (it has no ``kv_cache`` switch), or None when the caller turned the cache off."""
    return {k: v for k, v in kw.items() if k != "kv_cache"} if kw.get("kv_cache", True) else None


def _joint_scores(path_score: Tensor, status: Tensor, n_tokens, pred: Tensor, weight_ctc: float) -> Tensor:
    """util/beam_infer.py:350-378 over the last dimension (the beams of one search): ``s_ctc = exp(path[0].score / len(f_t))``
    (0 for a beam that could not be aligned), ``s_pred = exp(final_scores)``, each divided by its own maximum, mixed by
    ``weight_ctc``.  A vector whose maximum is 0 (every beam underflowed or failed) is left as it is instead of becoming 0 / 0."""
    s_ctc = torch.where(status == 0, torch.exp(path_score / n_tokens), torch.zeros_like(path_score))
    s_pred = torch.exp(pred.to(torch.float32))

    def by_max(v):
        m = v.max(dim=-1, keepdim=True).values
        return torch.where(m > 0, v / m, v)
    return by_max(s_ctc) * weight_ctc + by_max(s_pred) * (1 - weight_ctc)


def _first_argmax(v: Tensor) -> Tensor:
    """argmax over the last dimension, ties to the lower index."""
    K = v.size(-1)
    at = torch.where(v == v.max(dim=-1, keepdim=True).values, torch.arange(K, device=v.device), K)
    return at.min(dim=-1).values.clamp(max=K - 1)


def _ctc_pick(emission: Tensor, em_len: Optional[Tensor], weight_ctc: float, blank: int = 0):
    """The best-beam rule of n lockstep searches under a CTC weight: ``pick(tokens [n, R, L], scores [n, R]) -> best [n]``.
    Search i's beams are aligned against ``emission[i]`` ([n, T', V], ``em_len`` [n] frames or None) in ONE ``ctc_align``
    call, as given (SOS included, as in the reference); the joint score is tensor ops on the device."""
    def pick(tokens: Tensor, scores: Tensor) -> Tensor:
        n, R, L = tokens.shape
        em_index = torch.arange(n, device=tokens.device, dtype=torch.int32).repeat_interleave(R)
        _, _, path_score, _, status, _ = ctc_align(emission, tokens.reshape(n * R, L), em_index=em_index, em_len=em_len, blank=blank)
        return _first_argmax(_joint_scores(path_score.view(n, R), status.view(n, R), L, scores, weight_ctc))
    return pick


class _Modifiers(NamedTuple):
    """The search modifiers of one call, resolved once (``BeamInference._modifiers``): the context graph (or None), the graph of its
    bank per utterance (``graph_of``, 1-D, or None: graph 0) and the shallow-fusion triple (model, weight, bonus) (or None)."""
    context: Optional[ContextGraph] = None
    graph_of: Optional[Tensor] = None
    fusion: Optional[tuple] = None

    def chunk(self, c0: int, step: int) -> "_Modifiers":
        """The modifiers of utterances ``c0 .. c0 + step``."""
        return self if self.graph_of is None else self._replace(graph_of=self.graph_of[c0:c0 + step])

    def over_exits(self, E: int, B: int) -> "_Modifiers":
        """The modifiers of E * B searches (search e * B + b): the B graph rows repeated over the exits."""
        return self if self.graph_of is None else self._replace(graph_of=self.graph_of.reshape(B).repeat(E))

    def scorers(self, E: int, B: int, beam: int, V: int) -> list:
        """The sessions of E * B lockstep searches, in their order of application: the ``ContextBiasSession``, then the
        ``LMFusionSession``."""
        out = []
        if self.context is not None:
            if self.context.vocab_size != V:
                raise ValueError(f"the context graph is over {self.context.vocab_size} tokens, the decoder over {V}")
            out.append(ContextBiasSession(self.context, E * B, beam, self.over_exits(E, B).graph_of))
        if self.fusion is not None:
            lm, w, ts = self.fusion
            check_lm("shallow fusion", lm, V, beam, w, ts)
            out.append(LMFusionSession(lm, E * B, beam, w, ts))
        return out

    def ctc_kw(self) -> dict:
        """The keywords of ``ctc_beam_decode``, whose extra output, if there is one, is the bias or the fusion."""
        kw = {} if self.context is None else {"context": self.context, "graph_of": self.graph_of}
        if self.fusion is not None:
            kw.update(lm=self.fusion[0], lm_weight=self.fusion[1], token_score=self.fusion[2])
        return kw


def _exit_emission(word: str, emission, emission_len, E: int, B: Optional[int] = None):
    """What ``word`` needs: ``emission`` [E, B, T', V] and ``emission_len`` [B] (None: T') as the E * B searches read them (search
    e * B + b) -> (emission [E * B, T', V], em_len int32 [E * B] or None)."""
    if emission is None or emission.dim() != 4 or emission.size(0) != E or B not in (None, emission.size(1)):
        raise ValueError(f"{word} needs emission [{E}, {'B' if B is None else B}, T', V]: the CTC log-probs of every exit and utterance")
    B = emission.size(1)
    em_len = None if emission_len is None else emission_len.to(emission.device, torch.int32).reshape(B).repeat(E)
    return emission.reshape(E * B, emission.size(2), emission.size(3)), em_len


def _lockstep_search(step, n: int, dev, max_length: int, sos: int, beam: int, alpha: float, pick=None, scorers=()):
    """``max_length`` steps of n independent beam searches in lockstep, none of which finalises a beam on the way:
    ``step(last [n, R], parent [n, R] | None)`` returns the next token's log-probs [n, R, V] of every live beam.  The
    bookkeeping of a step is ``beam_select`` over two token buffers.  Returns ``(final_tokens, final_scores, best_tokens)``
    per search; the best beam is the one with the highest score, or ``pick(tokens [n, R, L], scores [n, R]) -> [n]``'s, which may
    also finish the rows in place.  ``scorers``: sessions (``decoding.ScorerSession``) whose ``step(logp, last, parent)`` rewrites the
    step's scores before the selection, applied in their order -- the CTC prefix scores of a joint search, then the contextual
    bias, then the language model's increments; the last two are additive.  After the last step every row is final as it stands:
    a scorer with a ``final(last, parent)`` adds it then, at the last step's penalty (the bias takes the provisional bonus of a
    still open partial match back, as an EOS would have)."""
    scores = torch.zeros((n, 1), dtype=torch.float32, device=dev)
    bufs = [torch.zeros((n, max(beam, 1), max_length + 1), dtype=torch.long, device=dev) for _ in range(2)]
    bufs[0][:, 0, 0] = sos
    last = bufs[0][:, :1, 0].contiguous()
    parent: Optional[Tensor] = None
    for i in range(max_length):
        logp = step(last, parent)
        for scorer in scorers:
            logp = scorer.step(logp, last, parent)
        scores, parent, last = beam_select(logp, scores, sequence_length_penalty(i + 1, alpha), beam, bufs[i & 1], bufs[(i + 1) & 1], i + 1)
    for scorer in scorers:
        if hasattr(scorer, "final"):
            scores = scores + scorer.final(last, parent) / sequence_length_penalty(max(max_length, 1), alpha)
    tokens = bufs[max_length & 1][:, :beam]
    best = (scores.argmax(dim=1) if pick is None else pick(tokens, scores)).tolist()
    tokens_h = tokens.cpu()
    return [(list(tokens[i]), list(scores[i]), tokens_h[i, best[i]].tolist()) for i in range(n)]


def _joint_lockstep_search(step, prefix, n: int, dev, max_length: int, sos: int, eos: int, pad: int, beam: int, alpha: float, scorers=()):
    """``_lockstep_search`` as the one-pass joint CTC / attention search (include/eec.h, "CTC prefix scores"): ``prefix.step`` (a
    ``CtcPrefixSession``) mixes the CTC prefix scores into the decoder's log-probs and closes the beams that took EOS, before the
    other ``scorers``; at the end a row holds only PAD after its EOS, and the best beam is the one with the highest score, ties to
    the lower index."""
    def pick(tokens: Tensor, scores: Tensor) -> Tensor:
        ended = torch.cumsum((tokens == eos).to(torch.int32), dim=2) > 0
        tokens[:, :, 1:] = torch.where(ended[:, :, :-1], torch.full_like(tokens[:, :, 1:], pad), tokens[:, :, 1:])  # rows of score -inf too
        return _first_argmax(scores)
    return _lockstep_search(step, n, dev, max_length, sos, beam, alpha, pick, (prefix, *scorers))


def _before_eos(ids, eos: int):
    """``ids`` up to, and excluding, the first EOS."""
    ids = list(ids)
    return ids[: ids.index(eos)] if eos in ids else ids


def _check_rescoring_weight(rescoring_ctc_weight) -> float:
    w = float(rescoring_ctc_weight)
    if not 0.0 <= w <= 1.0:
        raise ValueError(f"rescoring_ctc_weight must lie in [0, 1], got {rescoring_ctc_weight!r}")
    return w


def _check_joint_weight(joint_ctc_weight, ctc_weight=None) -> float:
    if ctc_weight is not None:
        raise ValueError("ctc_weight (the CTC head picks among the final beams) and joint_ctc_weight (one-pass joint decoding) exclude each other")
    w = float(joint_ctc_weight)
    if not 0 < w <= 1:
        raise ValueError(f"joint_ctc_weight must be in (0, 1], got {joint_ctc_weight}")
    return w


class BeamInference:
    """``args`` needs ``dec_voc_size, trg_sos_idx, trg_eos_idx, trg_pad_idx, beam_size, pen_alpha, device`` (the fields
    util/conf.py:455-486 injects); every one of them can also be given per call, as in the reference."""

    N_BEST = 1       # util/beam_infer.py:42
    W_INS = 0        # the word score of the reference's six lexicon decoders (w_ins, util/beam_infer.py:54)
    WORD_SCORE = -4  # util/beam_infer.py:41,74: the word score of the character-lexicon decoder behind beam_predict

    LM_WEIGHT = 1.0  # util/beam_infer.py:40 (its comment keeps 3.23, the value of the "bigger LM" setting)

    def __init__(self, args=None, trie: Optional[TokenTrie] = None, lm=None, smearing: Optional[str] = None,
                 log_add: Optional[bool] = None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None):
        """``lm``: an ``NGramLM``, or the path of an ARPA file (None: ``args.lm`` if there is one) that is read at the first use
        against the trie in use.  ``smearing``: None (then ``args.lm_smearing`` if there is one) or ``"max"``: LM look-ahead by max
        trie smearing in ``ctc_predict`` / ``ctc_predict_``.  The third-party decoder always smears; here the default is off, so
        a model alone decodes as before.  Without a model there is nothing to smear and the setting is not used.
        ``log_add``: None (then ``args.lm_log_add`` if there is one, else False) or a bool: log-add instead of Viterbi merging in
        ``ctc_predict`` / ``ctc_predict_``.  ``beam_predict`` always merges by log-add, as the reference's decoder does.
        ``token_lm``: a ``lm_fusion.TokenLM``, or the path of an ARPA file over the pieces (None: ``args.token_lm`` if there is one;
        a path is read at the first use against the lines of ``args.tokens``, with blank 0 and the special tokens of ``args``) --
        shallow fusion in the lexicon-free searches: ``ctc_cuda_predict``, ``ctc_adaptive_predict``, ``decode_batch`` (plain and
        joint), ``decode_all_exits``, the lockstep searches and the two-pass rescoring, each of which also takes the three keywords
        per call.  ``token_lm_weight`` (None: ``args.token_lm_weight``, else 0.3: customary, a choice and not tuned) and
        ``token_score`` (None: ``args.token_score``, else 0: the per-token insertion bonus).  Without a model nothing changes."""
        self.args = args
        self._token_lm = token_lm if token_lm is not None else getattr(args, "token_lm", None)
        self._token_lm_weight = token_lm_weight if token_lm_weight is not None else getattr(args, "token_lm_weight", None)
        self._token_score = token_score if token_score is not None else getattr(args, "token_score", None)
        self._trie = trie
        self._lm = lm if lm is not None else getattr(args, "lm", None)
        self._smearing = smearing if smearing is not None else getattr(args, "lm_smearing", None)
        if self._smearing not in (None, "max"):
            raise ValueError(f"BeamInference: smearing must be None or 'max', got {self._smearing!r}")
        self._log_add = bool(getattr(args, "lm_log_add", False) if log_add is None else log_add)
        self._lm_read = None  # (the trie a path was read against, its NGramLM)
        self._char_trie = None  # beam_predict's trie, apart from the BPE one

    sequence_length_penalty = staticmethod(sequence_length_penalty)

    def _lexicon_trie(self, trie: Optional[TokenTrie]) -> TokenTrie:
        """``trie``, the one given to the constructor, or -- built at the first use -- the one of ``args.lexicon`` / ``args.tokens``
        with the reference's ``blank_token="@"`` and ``sil_token="<pad>"`` (util/beam_infer.py:56-65)."""
        if trie is not None:
            return trie
        if self._trie is None:
            if self.args is None or not hasattr(self.args, "lexicon") or not hasattr(self.args, "tokens"):
                raise ValueError("ctc_predict: no trie= was given and there is no args.lexicon / args.tokens")
            self._trie = TokenTrie.from_files(self.args.lexicon, self.args.tokens, blank_token="@", sil_token="<pad>")
        return self._trie

    def _lexicon_lm(self, trie: TokenTrie) -> Optional[NGramLM]:
        """The model given to the constructor; a path is read against ``trie`` at its first use (and again for another trie)."""
        if self._lm is None or isinstance(self._lm, NGramLM):
            return self._lm
        if self._lm_read is None or self._lm_read[0] is not trie:
            self._lm_read = (trie, NGramLM.from_arpa(self._lm, trie))
        return self._lm_read[1]

    def _fusion(self, token_lm=None, token_lm_weight=None, token_score=None):
        """(model, weight, bonus) of a call's shallow fusion -- the call's keywords before the constructor's --, or None without a
        model.  A path is read once."""
        lm = token_lm if token_lm is not None else self._token_lm
        if lm is None:
            if token_lm_weight is not None or token_score is not None:
                raise ValueError("token_lm_weight / token_score weigh token_lm=, which was not given")
            return None
        if not isinstance(lm, TokenLM):
            if self.args is None or not hasattr(self.args, "tokens"):
                raise ValueError("token_lm is a path: its pieces are the lines of args.tokens, which is missing")
            with open(self.args.tokens, encoding="utf-8") as f:
                pieces = [line.rstrip("\r\n") for line in f]
            lm = TokenLM.from_arpa(lm, pieces, blank=0, sos=self._arg(None, "trg_sos_idx"), eos=self._arg(None, "trg_eos_idx"),
                                   pad=self._arg(None, "trg_pad_idx"))
            if token_lm is None:
                self._token_lm = lm
        w = token_lm_weight if token_lm_weight is not None else self._token_lm_weight
        ts = token_score if token_score is not None else self._token_score
        return lm, float(DEFAULT_LM_WEIGHT if w is None else w), float(0.0 if ts is None else ts)

    def _modifiers(self, name: str, context, graph_of, token_lm, token_lm_weight, token_score, given: Optional[_Modifiers] = None) -> _Modifiers:
        """The modifiers of a call of the public method ``name`` from its five keywords, or ``given``: the ones a calling method has
        resolved already (its ``_mods=``)."""
        if given is not None:
            return given
        if context is None and graph_of is not None:
            raise ValueError(f"{name}: graph_of chooses among the graphs of context=, which was not given")
        return _Modifiers(context, None if graph_of is None else torch.as_tensor(graph_of).reshape(-1),
                          self._fusion(token_lm, token_lm_weight, token_score))

    def _lexicon_decode(self, emission: Tensor, trie, nbest, beam_size, lm_weight=None, log_add=None, word_score=None):
        """(transcript of the best hypothesis per utterance, scores [B, nbest] and n_hyp [B] on the host)."""
        trie = self._lexicon_trie(trie)
        nbest = self.N_BEST if nbest is None else nbest
        log_add = self._log_add if log_add is None else log_add
        lm = self._lexicon_lm(trie)
        with_lm = {} if lm is None else {"lm": lm, "lm_weight": self.LM_WEIGHT if lm_weight is None else lm_weight}
        if lm is not None and self._smearing is not None:
            with_lm["smearing"] = self._smearing
        words, word_count, _, _, _, scores, n_hyp = ctc_lexicon_decode(emission, trie, beam_size=self._arg(beam_size, "beam_size"), nbest=nbest,
                                                                       word_score=self.W_INS if word_score is None else word_score,
                                                                       log_add=log_add, **with_lm)
        words, word_count, n_hyp = words[:, 0].cpu(), word_count[:, 0].cpu().tolist(), n_hyp.cpu().tolist()
        texts = [" ".join(trie.words[w] for w in words[b, : word_count[b]].tolist()).strip() if n_hyp[b] else "" for b in range(len(n_hyp))]
        return texts, scores.cpu(), n_hyp

    def beam_predict(self, model, input_sequence) -> str:
        """util/beam_infer.py:85-90: ``model.ctc_encoder(input_sequence)`` -- any object with that method, [B, T', V] log-probs --
        decoded by the reference's character-lexicon decoder (util/beam_infer.py:66-75): log-add merging, ``word_score=WORD_SCORE``,
        ``nbest=1``, ``args.beam_size``, the trie of ``args.lexicon`` / ``args.tokens`` with torchaudio's default ``blank_token="-"``
        and ``sil_token="|"`` (built at the first use and kept apart from the BPE trie), the configured model, if there is one, at
        ``LM_WEIGHT``.  Returns the transcript of the FIRST utterance's best hypothesis, its words joined by spaces and stripped;
        no complete hypothesis gives ``""`` (the reference would raise an IndexError: a stated divergence, as in ``ctc_predict_``).
        The emission stays on the device (the reference moves it to the host for the third-party decoder)."""
        emission = model.ctc_encoder(input_sequence)
        if self._char_trie is None:
            if self.args is None or not hasattr(self.args, "lexicon") or not hasattr(self.args, "tokens"):
                raise ValueError("beam_predict: there is no args.lexicon / args.tokens")
            self._char_trie = TokenTrie.from_files(self.args.lexicon, self.args.tokens, blank_token="-", sil_token="|")
        return self._lexicon_decode(emission[:1], self._char_trie, 1, None, None, log_add=True, word_score=self.WORD_SCORE)[0][0]

    def ctc_predict_(self, emission: Tensor, index: int = 5, trie: Optional[TokenTrie] = None, nbest: Optional[int] = None,
                     beam_size: Optional[int] = None, lm_weight: Optional[float] = None) -> List[str]:
        """util/beam_infer.py:93-99: the transcript of the best lexicon-constrained hypothesis of every utterance of ``emission``
        [B, T', V] (on the device; it stays there), its words joined by spaces and stripped.  ``index`` selects the reference's
        per-exit decoder; all six are configured alike (w_ins = 0), so it is accepted and unused.  An utterance with no complete
        hypothesis gives ``""`` (the reference would raise an IndexError: a stated divergence).  With a model (``lm=`` of the
        constructor or ``args.lm``) the search runs under it at ``lm_weight`` (None: ``LM_WEIGHT``); with ``log_add`` of the
        constructor (or ``args.lm_log_add``) hypotheses that meet are summed instead of the best one kept."""
        return self._lexicon_decode(emission, trie, nbest, beam_size, lm_weight)[0]

    def ctc_predict(self, emission: Tensor, index: int = 5, trie: Optional[TokenTrie] = None, nbest: Optional[int] = None,
                    beam_size: Optional[int] = None, lm_weight: Optional[float] = None):
        """util/beam_infer.py:115-126: ``([transcript], pprob)`` for the FIRST utterance of ``emission`` [B, T', V]: the best
        hypothesis' words, and ``softmax(scores of the returned hypotheses)[0]`` as a 0-D tensor -- with the reference's
        ``N_BEST = 1`` that is always 1; ``nbest=`` returns a meaningful posterior.  No complete hypothesis: ``([""], 0.0)`` (the
        reference would raise an IndexError: a stated divergence).  ``lm_weight``: as for ``ctc_predict_``."""
        texts, scores, n_hyp = self._lexicon_decode(emission[:1], trie, nbest, beam_size, lm_weight)
        if n_hyp[0] == 0:
            return [""], torch.tensor(0.0)
        return [texts[0]], torch.softmax(scores[0, : n_hyp[0]].double(), dim=0)[0].float()

    def ctc_cuda_predict(self, emission: Tensor, tokens=None, beam_size: Optional[int] = None, lexicon=None,
                         detokenize=None, lengths: Optional[Tensor] = None, nbest: Optional[int] = None, context=None,
                         graph_of=None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None) -> List[List["CTCHypothesis"]]:
        """util/beam_infer.py:102-112: the nbest (= 1) beam-search hypotheses of one exit's log-probs ``emission`` [B, T', V],
        input length T' for every utterance (``lengths`` [B] in encoder frames: the decoder's ``encoder_out_lens``), beam ``args.beam_size``, blank_skip_threshold 0.95 -- per utterance a list of
        hypothesis objects with ``.tokens`` / ``.words`` / ``.score`` like torchaudio's, so the reference's call sites
        (``best[0][0].tokens`` train.py:82, ``best_[0].tokens`` inference.py:70) work unchanged.  ``tokens`` (the token file
        the torchaudio decoder takes) is accepted and unused: ids are returned, blank = 0.  With ``lexicon`` (a
        ``lexicon.Lexicon`` or the list ``load_dict`` returns) and ``detokenize`` (ids -> str: the caller's ``sp.decode`` or
        ``int_to_text``) every hypothesis also carries ``.text``, its ``apply_lex``-ed transcript (inference.py:70-71), and
        ``.words``, that text's words; with either None nothing changes.  ``nbest`` (None: as above, one hypothesis): up to that
        many hypotheses per utterance, best first, as torchaudio's ``nbest`` -- the beam the same search ends with
        (``ctc_beam_decode(nbest=)``), so an utterance whose final beam is smaller returns fewer.  ``context`` (a
        ``context.ContextGraph``; None: unchanged) and ``graph_of`` [B]: the search is biased towards the graph's phrases
        (``ctc_beam_decode(context=)``); ``.score`` stays the CTC log-probability and every hypothesis also carries ``.bias``.
        ``token_lm`` / ``token_lm_weight`` / ``token_score`` (or the constructor's): shallow fusion with a token-level n-gram model
        (``ctc_beam_decode(lm=)``); every hypothesis then carries ``.fusion`` beside its ``.score``.  Not together with ``context``."""
        beam = self._arg(beam_size, "beam_size")
        mods = self._modifiers("ctc_cuda_predict", context, graph_of, token_lm, token_lm_weight, token_score)
        out = [t.cpu() for t in ctc_beam_decode(emission, beam_size=beam, blank=0, blank_skip_threshold=0.95, em_len=lengths, nbest=nbest,
                                                **mods.ctc_kw())]
        if nbest is None:  # the best prefix alone: an N-best list of one
            out = [t.unsqueeze(1) for t in out[:3]] + [torch.ones(out[0].size(0), dtype=torch.int32)] + [t.unsqueeze(1) for t in out[3:]]
        tok, cnt, score, n_hyp, *bias = out
        hyps = [[CTCHypothesis(tok[b, r, : int(cnt[b, r])].tolist(), [], float(score[b, r])) for r in range(int(n_hyp[b]))]
                for b in range(tok.size(0))]
        for b, row in enumerate(hyps if bias else []):
            for r, h in enumerate(row):
                setattr(h, "bias" if mods.fusion is None else "fusion", float(bias[0][b, r]))
        if lexicon is not None and detokenize is not None:
            flat = [h for row in hyps for h in row]
            for h, text in zip(flat, _snapped_texts([h.tokens for h in flat], lexicon, detokenize)):
                h.text, h.words = text, text.split(" ")
        return hyps

    @staticmethod
    def _align_one(emission: Tensor, tokens, blank_id: int, want_trellis: bool):
        """One hypothesis through ``ctc_align``; ValueError where the reference prints "Failed to align" (a stated
        divergence: no tokens, or more tokens than frames) and for ids outside the vocabulary."""
        if emission.dim() != 2:
            raise ValueError(f"emission must be [T', V], got {tuple(emission.shape)}")
        tok = torch.as_tensor(tokens, dtype=torch.long).reshape(1, -1)
        T, N = emission.size(0), tok.size(1)
        if N < 1 or N > T:
            raise ValueError(f"Failed to align: {N} tokens against {T} frames")
        out = ctc_align(emission.unsqueeze(0), tok, blank=blank_id, want_trellis=want_trellis)
        if int(out[4][0]) != 0:
            raise ValueError("Failed to align: a token id outside the vocabulary, or non-finite emissions")
        return out

    @torch.no_grad()
    def get_trellis(self, emission: Tensor, tokens, blank_id: int = 0) -> Tensor:
        """util/beam_infer.py:129-150: the Viterbi trellis [T' + 1, N + 1] of ``tokens`` against ``emission`` [T', V], with
        the reference's quirks (column 0 accumulates ``emission[:, 0]`` whatever ``blank_id`` is; +inf below ``T' + 1 - N``
        in column 0 and what it feeds).  One kernel call."""
        return self._align_one(emission, tokens, blank_id, True)[5][0]

    @torch.no_grad()
    def backtrack(self, trellis: Tensor, emission: Tensor, tokens, blank_id: int = 0) -> List[Point]:
        """util/beam_infer.py:153-191: the best path from the last frame back to the first token's frame, returned in time
        order.  The kernel aligns ``(emission, tokens)`` itself; ``trellis`` is accepted for the signature and only its shape
        is checked."""
        N = torch.as_tensor(tokens).numel()
        if tuple(trellis.shape) != (emission.size(0) + 1, N + 1):
            raise ValueError(f"trellis must be [{emission.size(0) + 1}, {N + 1}], got {tuple(trellis.shape)}")
        point_token, point_score = (t[0].cpu() for t in self._align_one(emission, tokens, blank_id, False)[:2])
        return [Point(int(j), t, float(point_score[t])) for t, j in enumerate(point_token.tolist()) if j >= 0]

    @torch.no_grad()
    def ctc_rescore(self, final_tokens, final_scores, emission: Tensor, weight_ctc: float, blank_id: int = 0) -> Tuple[Tensor, int]:
        """The dormant second half of the reference's ``beam_search`` (util/beam_infer.py:350-378) for the K final beams of ONE
        search: every beam is aligned, as given (SOS included), against ``emission`` [T', V] in one kernel call;
        ``s_ctc_i = exp(path[0].score_i / len(f_t_i))`` (0 for a beam that cannot be aligned), ``s_pred_i = exp(final_scores_i)``,
        each vector divided by its own maximum, ``joint = weight_ctc * s_ctc + (1 - weight_ctc) * s_pred``.  Returns
        ``(joint [K], best_index)``, ties to the lower index."""
        dev = emission.device
        toks = [torch.as_tensor(t, dtype=torch.long).reshape(-1) for t in final_tokens]
        lens = torch.tensor([t.numel() for t in toks], dtype=torch.int32)
        tokens = torch.nn.utils.rnn.pad_sequence(toks, batch_first=True).to(dev)
        pred = torch.stack([torch.as_tensor(s, dtype=torch.float32, device=dev).reshape(()) for s in final_scores])
        em_index = torch.zeros(len(toks), dtype=torch.int32, device=dev)
        _, _, path_score, _, status, _ = ctc_align(emission.unsqueeze(0), tokens, tok_len=lens, em_index=em_index, blank=blank_id)
        joint = _joint_scores(path_score, status, lens.to(dev), pred, weight_ctc)
        return joint, int(_first_argmax(joint))

    def _arg(self, value, name):
        if value is not None:
            return value
        if self.args is None or not hasattr(self.args, name):
            raise ValueError(f"beam_search: {name} was not given and there is no args.{name}")
        return getattr(self.args, name)

    @torch.no_grad()
    def beam_search(self, model, encoder_output: Tensor, layer_n: int, vocab_size: Optional[int] = None, max_length: int = 500,
                    min_length: int = 300, SOS_token: Optional[int] = None, EOS_token: Optional[int] = None,
                    PAD_token: Optional[int] = None, beam_size: Optional[int] = None, pen_alpha: Optional[float] = None,
                    return_best_beam: bool = True, kv_cache: bool = True):
        """Returns ``(final_tokens, final_scores, best_tokens)`` like the reference: lists of 1-D token tensors / 0-D score
        tensors, and the best beam as a Python list (SOS included).  ``kv_cache`` (not in the reference): decode step-wise
        through ``model.decoder_session`` (only the new position of every beam is computed; same log-probs to fp32
        rounding) when the model offers one for this geometry; False re-runs ``_decoder_`` on the whole prefix per step."""
        V = self._arg(vocab_size, "dec_voc_size")
        sos, eos = self._arg(SOS_token, "trg_sos_idx"), self._arg(EOS_token, "trg_eos_idx")
        self._arg(PAD_token, "trg_pad_idx")  # accepted and unused, as in the reference
        beam = self._arg(beam_size, "beam_size")
        alpha = self._arg(pen_alpha, "pen_alpha")
        dev = encoder_output.device
        count = beam
        tokens = torch.tensor([[sos]], dtype=torch.long, device=dev)  # [live beams, s]
        scores = torch.zeros(1, dtype=torch.float32, device=dev)
        final_tokens: List[Tensor] = []
        final_scores: List[Tensor] = []
        if kv_cache and return_best_beam and encoder_output.is_cuda and encoder_output.size(0) == 1:
            # no beam can finish inside max_length (the reference's defaults): the lockstep search with one member, whose
            # per-step bookkeeping is one launch
            one = self.beam_search_exits(model, [encoder_output], [layer_n], vocab_size=V, max_length=max_length, min_length=min_length,
                                         SOS_token=sos, EOS_token=eos, PAD_token=self._arg(PAD_token, "trg_pad_idx"), beam_size=beam,
                                         pen_alpha=alpha)
            if one is not None:
                return one[0]
        session = None
        if kv_cache and max_length >= 1 and hasattr(model, "decoder_session") and encoder_output.size(0) == 1:
            session = model.decoder_session(encoder_output, layer_n, max_length)
            if session is not None and beam > session.max_beams:
                session = None
        parent: Optional[Tensor] = None
        i = -1
        for i in range(max_length):
            if session is not None:
                logp = session.step(tokens[:, -1], parent)
            else:
                enc = encoder_output if i == 0 else encoder_output.expand(tokens.size(0), *encoder_output.shape[1:])
                logp = model._decoder_(tokens, enc, layer_n)[:, -1]
            logp = logp / sequence_length_penalty(i + 1, alpha)
            cand, idx = torch.topk((scores.unsqueeze(1) + logp).reshape(-1), count)
            beam_idx = torch.div(idx, V, rounding_mode="floor")
            tok_idx = torch.remainder(idx, V)
            grown = torch.cat([tokens[beam_idx], tok_idx.unsqueeze(1)], dim=1)
            parent = beam_idx
            if i > min_length:  # never while max_length <= min_length (the reference's defaults): no host sync per step then
                done = tok_idx == eos
                if bool(done.any()):
                    for j in torch.nonzero(done).flatten().tolist():
                        final_tokens.append(grown[j])
                        final_scores.append(cand[j])
                        count -= 1
                    grown, cand, parent = grown[~done], cand[~done], beam_idx[~done]
            scores = cand
            if len(final_scores) == beam:
                break
            tokens = grown
        if i == max_length - 1:  # ran out of steps: every live beam is final
            for t, s in zip(tokens, scores):
                final_tokens.append(t)
                final_scores.append(s)
            assert len(final_tokens) == beam and len(final_scores) == beam, \
                "Final_tokens and final_scores lists do not match beam_size size!"
        best = None
        if return_best_beam:
            best = final_tokens[int(torch.stack(final_scores).argmax())].tolist()
        return final_tokens, final_scores, best

    @torch.no_grad()
    def decode_all_exits(self, model, spec: Tensor, valid_len: Tensor, max_length: Optional[int] = None, beam_size: int = 10,
                         ctc_weight: Optional[float] = None, joint_ctc_weight: Optional[float] = None, context=None, graph_of=None,
                         token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None, _mods=None, **kw) -> List[List[int]]:
        """What inference.py:31-51 does for ONE utterance: the best beam of every exit.  ``spec`` [n_mels, T],
        ``valid_len`` 0-D / [1].  The encoder runs once (taps of all exits).  ``ctc_weight``: the best beam of every exit is
        chosen jointly with that exit's CTC log-probs (``ctc_rescore``'s rule; they come from the same encoder pass).
        ``joint_ctc_weight`` (None: unchanged): the search itself is the one-pass joint one (``joint_search_exits``; ``min_length=``
        defaults to 0 there); not together with ``ctc_weight``.  ``context`` / ``graph_of`` [1]: contextual biasing of the lockstep
        searches (``beam_search_batch``); ValueError where only the step-by-step ``beam_search`` could serve the call.  ``token_lm`` /
        ``token_lm_weight`` / ``token_score``: shallow fusion in the lockstep searches, under the same condition."""
        if max_length is None:
            max_length = default_max_length(spec.size(1))
        mods = self._modifiers("decode_all_exits", context, graph_of, token_lm, token_lm_weight, token_score, _mods)
        if joint_ctc_weight is not None:
            _check_joint_weight(joint_ctc_weight, ctc_weight)
            logp, taps = model._run_encoder(spec.unsqueeze(0), valid_len.reshape(1), want_out=True, want_taps=True, n_groups=model._cfg.n_exits)[:2]
            exits = list(range(1, model._cfg.n_exits + 1))
            found = self.joint_search_exits(model, [taps[n - 1] for n in exits], exits, logp,
                                            encoder_lengths(valid_len.reshape(1).to(logp.device), logp.size(2)), joint_ctc_weight,
                                            max_length, beam_size=beam_size, **(_lockstep_kw(kw) or {}), _mods=mods)
            return [best for _, _, best in found]
        logp, taps = model._run_encoder(spec.unsqueeze(0), valid_len.reshape(1), want_out=ctc_weight is not None, want_taps=True,
                                        n_groups=model._cfg.n_exits)[:2]
        exits = list(range(1, model._cfg.n_exits + 1))
        ctc = {}
        if ctc_weight is not None:
            ctc = dict(ctc_weight=ctc_weight, emission=logp, emission_len=encoder_lengths(valid_len.reshape(1).to(logp.device), logp.size(2)))
        lockstep = _lockstep_kw(kw)
        if lockstep is not None:
            together = self.beam_search_exits(model, [taps[n - 1] for n in exits], exits, max_length=max_length, beam_size=beam_size,
                                              **lockstep, **ctc, _mods=mods)
            if together is not None:
                return [best for _, _, best in together]
        if mods.context is not None or mods.fusion is not None:
            raise ValueError("decode_all_exits: contextual biasing and shallow fusion run in the lockstep searches only, and none serves this call "
                             "(kv_cache=False, max_length - 1 > min_length, or no session group for this model / geometry)")
        found = [self.beam_search(model, taps[n - 1], n, max_length=max_length, beam_size=beam_size, **kw) for n in exits]
        if ctc_weight is None:
            return [best for _, _, best in found]
        frames = int(ctc["emission_len"][0])
        return [ft[self.ctc_rescore(ft, fs, logp[n - 1, 0, :frames], ctc_weight)[1]].tolist() for n, (ft, fs, _) in zip(exits, found)]

    @torch.no_grad()
    def beam_search_exits(self, model, encoder_outputs: Sequence[Tensor], layer_ns: Sequence[int], vocab_size: Optional[int] = None,
                          max_length: int = 500, min_length: int = 300, SOS_token: Optional[int] = None, EOS_token: Optional[int] = None,
                          PAD_token: Optional[int] = None, beam_size: Optional[int] = None, pen_alpha: Optional[float] = None,
                          ctc_weight: Optional[float] = None, emission: Optional[Tensor] = None, emission_len: Optional[Tensor] = None,
                          context=None, graph_of=None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None,
                          _mods=None):
        """``beam_search`` for several exits of one utterance in lockstep: the searches are independent, so every decoder
        launch and every bookkeeping op covers all of them (``model.decoder_session_group``).  Returns the list of
        ``(final_tokens, final_scores, best_tokens)`` per exit, the same values as ``beam_search`` exit by exit -- or None
        when the lockstep does not apply: no session group for this model / geometry, or EOS could finalise beams
        (``max_length - 1 > min_length``), which would let the exits' beam counts diverge.  ``ctc_weight`` with ``emission``
        [len(layer_ns), 1, T', V] (and ``emission_len`` [1]): as in ``beam_search_batch``; ``context`` / ``graph_of`` [1] too."""
        V, sos, beam, alpha = self._lockstep_args(vocab_size, SOS_token, EOS_token, PAD_token, beam_size, pen_alpha)
        mods = self._modifiers("beam_search_exits", context, graph_of, token_lm, token_lm_weight, token_score, _mods)
        if max_length < 1 or max_length - 1 > min_length or not hasattr(model, "decoder_session_group"):
            return None
        if any(e.size(0) != 1 for e in encoder_outputs):
            return None
        group = model.decoder_session_group(encoder_outputs, layer_ns, max_length)
        if group is None or beam > group.max_beams:
            return None
        return _lockstep_search(group.step, len(layer_ns), encoder_outputs[0].device, max_length, sos, beam, alpha,
                                self._pick(ctc_weight, emission, emission_len, len(layer_ns), 1), mods.scorers(len(layer_ns), 1, beam, V))

    @staticmethod
    def _pick(ctc_weight, emission, emission_len, E: int, B: int):
        """The best-beam rule of E * B lockstep searches (search e * B + b): None without a CTC weight."""
        if ctc_weight is None:
            return None
        return _ctc_pick(*_exit_emission("ctc_weight", emission, emission_len, E, B), float(ctc_weight))

    def _lockstep_args(self, vocab_size, SOS_token, EOS_token, PAD_token, beam_size, pen_alpha):
        self._arg(EOS_token, "trg_eos_idx"), self._arg(PAD_token, "trg_pad_idx")  # accepted and unused: no beam finalises
        return self._arg(vocab_size, "dec_voc_size"), self._arg(SOS_token, "trg_sos_idx"), self._arg(beam_size, "beam_size"), self._arg(pen_alpha, "pen_alpha")

    @torch.no_grad()
    def beam_search_batch(self, model, taps, layer_ns: Sequence[int], vocab_size: Optional[int] = None, max_length: int = 500,
                          min_length: int = 300, SOS_token: Optional[int] = None, EOS_token: Optional[int] = None,
                          PAD_token: Optional[int] = None, beam_size: Optional[int] = None, pen_alpha: Optional[float] = None,
                          ctc_weight: Optional[float] = None, emission: Optional[Tensor] = None, emission_len: Optional[Tensor] = None,
                          context=None, graph_of=None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None,
                          _mods=None):
        """``beam_search_exits`` for every utterance of a padded batch at once: ``taps`` [E, B, T', D] (or E tensors [B, T', D]),
        exit ``layer_ns[e]``'s encoder output of every utterance.  The E * B searches are independent and run in lockstep through
        one ``model.decoder_batch_session`` (every decoder launch covers all of them) and one ``eec_beam_select`` per step.
        Returns ``out[b][e] = (final_tokens, final_scores, best_tokens)``, what ``beam_search`` returns for utterance b and exit
        ``layer_ns[e]`` -- or None where ``beam_search_exits`` declines: EOS could finalise beams (``max_length - 1 >
        min_length``), or no batch session for this model / geometry / device.  ``ctc_weight`` (None: the highest score, no
        extra launch): ``best_tokens`` is chosen by ``ctc_rescore``'s joint score instead -- the E * B * beam final beams are
        aligned in one ``ctc_align`` call against ``emission`` [E, B, T', V], the exits' CTC log-probs of the same encoder pass
        (``emission_len`` [B]: their frames, None = T'); ``final_tokens`` / ``final_scores`` are untouched.  ``context`` (a
        ``context.ContextGraph`` built with ``eos=`` / ``pad=``; None: unchanged, no new launch) and ``graph_of`` [B]: one
        ``eec_context_bias_step`` per step adds the contextual bias to the step's log-probs before the selection, so it shares the
        step's length penalty (include/eec.h, "Contextual biasing").  ``token_lm`` (a ``lm_fusion.TokenLM`` built with the decoder's
        ``sos=`` / ``eos=`` / ``pad=``; or the constructor's), ``token_lm_weight``, ``token_score``: shallow fusion -- one
        ``eec_lm_fusion_step`` per step in the same place (include/eec.h, "Shallow fusion"); it composes with ``context``."""
        V, sos, beam, alpha = self._lockstep_args(vocab_size, SOS_token, EOS_token, PAD_token, beam_size, pen_alpha)
        mods = self._modifiers("beam_search_batch", context, graph_of, token_lm, token_lm_weight, token_score, _mods)
        if max_length < 1 or max_length - 1 > min_length or not hasattr(model, "decoder_batch_session"):
            return None
        session = model.decoder_batch_session(taps, layer_ns, max_length)
        if session is None or beam > session.max_beams:
            return None
        E, B = session.E, session.B
        n = E * B  # search i = e * B + b

        def step(last, parent):
            return session.step(last.view(E, B, -1), None if parent is None else parent.view(E, B, -1)).view(n, -1, V)
        found = _lockstep_search(step, n, session.dev, max_length, sos, beam, alpha, self._pick(ctc_weight, emission, emission_len, E, B),
                                 mods.scorers(E, B, beam, V))
        return [[found[e * B + b] for e in range(E)] for b in range(B)]

    def _joint_args(self, emission, emission_len, E: int, B: int, V: int, joint_ctc_weight, EOS_token, PAD_token, blank: int):
        """The checked arguments of a joint search over E * B lockstep searches (search e * B + b)."""
        w = _check_joint_weight(joint_ctc_weight)
        eos, pad = self._arg(EOS_token, "trg_eos_idx"), self._arg(PAD_token, "trg_pad_idx")
        em, em_len = _exit_emission("joint_ctc_weight", emission, emission_len, E, B)
        if em.size(2) != V:
            raise ValueError(f"joint decoding needs one vocabulary for both heads: the decoder has {V} tokens, the emission {em.size(2)}")
        return w, eos, pad, em.float(), em_len, int(blank)

    @torch.no_grad()
    def joint_search_batch(self, model, taps, layer_ns: Sequence[int], emission: Tensor, emission_len: Optional[Tensor],
                           joint_ctc_weight: float, max_length: int, min_length: int = 0, vocab_size: Optional[int] = None,
                           SOS_token: Optional[int] = None, EOS_token: Optional[int] = None, PAD_token: Optional[int] = None,
                           beam_size: Optional[int] = None, pen_alpha: Optional[float] = None, blank: int = 0, context=None, graph_of=None,
                           token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None, _mods=None):
        """One-pass joint CTC / attention decoding (Watanabe et al. 2017; include/eec.h states the semantics) of every exit and
        utterance of a padded batch in lockstep: ``taps`` as for ``beam_search_batch``, ``emission`` [E, B, T', V] the exits' CTC
        log-probs of the same encoder pass (``emission_len`` [B]: their frames, None = T').  At every step the local score of a
        candidate is ``(1 - w) * decoder log-prob + w * (CTC prefix log-prob of the extended labels - that of the beam)``; EOS is
        scored by the full-sequence CTC likelihood (never before ``min_length`` steps), a beam that takes it is done and grows by
        PAD at no cost, and a candidate the CTC head gives probability zero is dropped.  One decoder step, one
        ``eec_ctc_prefix_step`` and one ``eec_beam_select`` per step.  Returns ``out[b][e] = (final_tokens, final_scores,
        best_tokens)``; rows are ``max_length + 1`` long, SOS first.  ValueError where no batch session exists for the model /
        geometry / device: there is no reference search to fall back to.  ``context`` / ``graph_of`` [B]: as in ``beam_search_batch``,
        applied after the CTC prefix scores; ``token_lm`` / ``token_lm_weight`` / ``token_score`` too."""
        V, sos, beam, alpha = self._lockstep_args(vocab_size, SOS_token, EOS_token, PAD_token, beam_size, pen_alpha)
        mods = self._modifiers("joint_search_batch", context, graph_of, token_lm, token_lm_weight, token_score, _mods)
        session = model.decoder_batch_session(taps, layer_ns, max_length) if max_length >= 1 and hasattr(model, "decoder_batch_session") else None
        if session is None or beam > session.max_beams:
            raise ValueError("joint_search_batch: no batched decoder session for this model, geometry, device or beam size")
        E, B = session.E, session.B
        n = E * B
        w, eos, pad, em, em_len, blank = self._joint_args(emission, emission_len, E, B, V, joint_ctc_weight, EOS_token, PAD_token, blank)
        prefix = ctc_prefix_session(em, em_len, beam, w, eos, pad, blank=blank, min_length=min_length)

        def step(last, parent):
            return session.step(last.view(E, B, -1), None if parent is None else parent.view(E, B, -1)).view(n, -1, V)
        found = _joint_lockstep_search(step, prefix, n, session.dev, max_length, sos, eos, pad, beam, alpha, mods.scorers(E, B, beam, V))
        return [[found[e * B + b] for e in range(E)] for b in range(B)]

    @torch.no_grad()
    def joint_search_exits(self, model, encoder_outputs: Sequence[Tensor], layer_ns: Sequence[int], emission: Tensor,
                           emission_len: Optional[Tensor], joint_ctc_weight: float, max_length: int, min_length: int = 0,
                           vocab_size: Optional[int] = None, SOS_token: Optional[int] = None, EOS_token: Optional[int] = None,
                           PAD_token: Optional[int] = None, beam_size: Optional[int] = None, pen_alpha: Optional[float] = None, blank: int = 0,
                           context=None, graph_of=None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None,
                           _mods=None):
        """``joint_search_batch`` for the exits of ONE utterance (``model.decoder_session_group``): ``encoder_outputs[i]`` [1, T', D]
        is exit ``layer_ns[i]``'s encoder output, ``emission`` [len(layer_ns), 1, T', V].  Returns the list of ``(final_tokens,
        final_scores, best_tokens)`` per exit; ValueError where no session group exists."""
        V, sos, beam, alpha = self._lockstep_args(vocab_size, SOS_token, EOS_token, PAD_token, beam_size, pen_alpha)
        mods = self._modifiers("joint_search_exits", context, graph_of, token_lm, token_lm_weight, token_score, _mods)
        group = None
        if max_length >= 1 and hasattr(model, "decoder_session_group") and all(e.size(0) == 1 for e in encoder_outputs):
            group = model.decoder_session_group(encoder_outputs, layer_ns, max_length)
        if group is None or beam > group.max_beams:
            raise ValueError("joint_search_exits: no decoder session group for this model, geometry, device or beam size")
        n = len(layer_ns)
        w, eos, pad, em, em_len, blank = self._joint_args(emission, emission_len, n, 1, V, joint_ctc_weight, EOS_token, PAD_token, blank)
        prefix = ctc_prefix_session(em, em_len, beam, w, eos, pad, blank=blank, min_length=min_length)
        return _joint_lockstep_search(group.step, prefix, n, encoder_outputs[0].device, max_length, sos, eos, pad, beam, alpha,
                                      mods.scorers(n, 1, beam, V))

    @torch.no_grad()
    def decode_batch(self, model, spec: Tensor, valid_len: Tensor, max_length: Optional[int] = None, beam_size: int = 10,
                     max_batch: Optional[int] = None, ctc_weight: Optional[float] = None, lexicon=None, detokenize=None,
                     joint_ctc_weight: Optional[float] = None, context=None, graph_of=None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None,
                     **kw) -> List[List[List[int]]]:
        """What inference.py:18-62 (evaluate_batch_ae) computes for a padded batch: the best beam of every exit of every
        utterance, ``out[b][e]``.  ``spec`` [B, n_mels, T], ``valid_len`` [B].  The encoder runs once per chunk of at most
        ``max_batch`` utterances (taps of all exits), then ``beam_search_batch`` decodes all exits and utterances of the chunk in
        lockstep.  Where the batched search declines, every utterance goes through ``decode_all_exits``, so the result is
        always the reference's.  ``ctc_weight`` (None: unchanged, the encoder computes no log-probs): the two heads vote --
        the encoder pass also returns the exits' CTC log-probs and every search's best beam is ``ctc_rescore``'s.
        ``lexicon`` and ``detokenize`` (ids -> str) together: every ``out[b][e]`` is a ``DecodedTokens`` list whose ``.text`` is
        ``apply_lex(detokenize(ids), lexicon)`` (inference.py:50-51), all E x B texts resolved in one lexicon search; with either
        None nothing changes.  ``joint_ctc_weight`` w in (0, 1] (None: unchanged, no new launch): the search is the one-pass
        joint CTC / attention one (``joint_search_batch``: every candidate of every step is also scored by the CTC prefix
        probability, EOS ends a beam; ``min_length=`` defaults to 0 there).  Each ``out[b][e]`` is then the best row as it stands
        -- SOS, the tokens, EOS, PAD up to ``max_length + 1`` -- and the lexicon step sees the tokens before EOS.  Not together
        with ``ctc_weight``; ValueError where no batch session serves the model (there is no reference search to fall back to).
        ``context`` (a ``context.ContextGraph`` over the decoder's vocabulary, built with ``eos=`` / ``pad=``; None: unchanged) and
        ``graph_of`` [B] (a graph of a bank per utterance, the same for all its exits): the searches are biased towards the graph's
        phrases, plain and joint alike (``beam_search_batch``).  ``token_lm`` / ``token_lm_weight`` / ``token_score`` (or the
        constructor's): shallow fusion with a token-level n-gram model in the same searches; without a model nothing changes."""
        if max_length is None:  # one length for the whole padded batch
            max_length = default_max_length(spec.size(2))
        mods = self._modifiers("decode_batch", context, graph_of, token_lm, token_lm_weight, token_score)
        E = model._cfg.n_exits
        exits = list(range(1, E + 1))
        valid_len = valid_len.reshape(-1)
        step = max_batch or spec.size(0)
        out: List[List[List[int]]] = []
        if joint_ctc_weight is not None:
            _check_joint_weight(joint_ctc_weight, ctc_weight)
        for c0 in range(0, spec.size(0), step):
            sp, vl = spec[c0:c0 + step], valid_len[c0:c0 + step]
            together, lockstep = None, _lockstep_kw(kw)
            if joint_ctc_weight is not None:
                logp, taps = model._run_encoder(sp, vl, want_out=True, want_taps=True, n_groups=E)[:2]
                together = self.joint_search_batch(model, taps, exits, logp, encoder_lengths(vl.to(logp.device), logp.size(2)), joint_ctc_weight,
                                                   max_length, beam_size=beam_size, **(lockstep or {}), _mods=mods.chunk(c0, step))
                del taps, logp
            elif lockstep is not None:
                logp, taps = model._run_encoder(sp, vl, want_out=ctc_weight is not None, want_taps=True, n_groups=E)[:2]
                ctc = {}
                if ctc_weight is not None:
                    ctc = dict(ctc_weight=ctc_weight, emission=logp, emission_len=encoder_lengths(vl.to(logp.device), logp.size(2)))
                together = self.beam_search_batch(model, taps, exits, max_length=max_length, beam_size=beam_size, **lockstep, **ctc,
                                                  _mods=mods.chunk(c0, step))
                del taps, logp, ctc
            if together is None:
                out += [self.decode_all_exits(model, sp[b], vl[b], max_length=max_length, beam_size=beam_size, ctc_weight=ctc_weight,
                                              _mods=mods.chunk(c0 + b, 1), **kw) for b in range(sp.size(0))]
            else:
                out += [[best for _, _, best in row] for row in together]
        cut = (lambda ids: ids) if joint_ctc_weight is None else (lambda ids: _before_eos(ids, self._arg(kw.get("EOS_token"), "trg_eos_idx")))
        return _with_texts(out, lexicon, detokenize, cut)

    # -- two-pass decoding: the CTC head proposes an N-best list, the attention decoder scores it in one teacher-forced pass ---
    @torch.no_grad()
    def rescore_batch(self, model, taps, layer_ns: Sequence[int], emission: Tensor, emission_len: Optional[Tensor], nbest: int,
                      rescoring_ctc_weight: float, beam_size: Optional[int] = None, SOS_token: Optional[int] = None,
                      EOS_token: Optional[int] = None, blank: int = 0, max_workspace_bytes: int = 2 << 30, context=None, graph_of=None,
                      token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None, _mods=None):
        """Two-pass decoding of exits ``layer_ns`` for every utterance of a padded batch: ``taps`` [E, B, T', D] (or E tensors
        [B, T', D]) and ``emission`` [E, B, T', V], the exits' encoder outputs and CTC log-probs of one encoder pass
        (``emission_len`` [B]: their frames, None = T').  First pass: the N-best lists of all E * B emissions in ONE prefix beam
        search (``ctc_beam_decode(nbest=)``: beam ``beam_size``, blank_skip_threshold 0.95, no lexicon, no language model).
        Second pass, per exit: ``model.score_hypotheses`` -- every hypothesis of the exit's B lists through the attention decoder
        at once, no autoregressive loop.  Then ``joint = (1 - w) * att + w * ctc`` with w = ``rescoring_ctc_weight`` in [0, 1]
        (the convention of the one-pass joint search; a score with weight 0 does not enter), in fp64, and the best hypothesis
        is the one with the highest joint score, ties to the lower rank; an absent hypothesis is never chosen.  No length
        normalisation.  Returns ``out[b][e] = (best_tokens, RescoredList)``: the chosen ids (no SOS / EOS), and ``tokens``,
        ``ctc``, ``att``, ``joint`` of that search's whole list, best CTC score first.  ``context`` (a ``context.ContextGraph`` over
        the CTC vocabulary; None: unchanged) and ``graph_of`` [B]: the first pass is the biased search (``ctc_beam_decode(context=)``:
        the list is ordered by CTC score + bias) and ``joint = (1 - w) * att + w * ctc + bias`` in fp64, ties to the lower rank.
        ``token_lm`` / ``token_lm_weight`` / ``token_score`` (or the constructor's; not together with ``context``): the first pass is the
        fused search (``ctc_beam_decode(lm=)``), ``joint = (1 - w) * att + w * ctc + fusion`` in fp64, and each list is a
        ``FusedRescoredList`` that also carries ``fusion``."""
        w = _check_rescoring_weight(rescoring_ctc_weight)
        if not hasattr(model, "score_hypotheses"):
            raise ValueError("rescore_batch: the model has no attention decoder to rescore with (full_conformer)")
        beam = self._arg(beam_size, "beam_size")
        sos, eos = self._arg(SOS_token, "trg_sos_idx"), self._arg(EOS_token, "trg_eos_idx")
        E = len(layer_ns)
        em, em_len = _exit_emission("rescore_batch", emission, emission_len, E)
        B = emission.size(1)
        if len(taps) != E or taps[0].size(0) != B:
            raise ValueError(f"rescore_batch needs taps [{E}, B, T', D] and emission [{E}, B, T', V] of one encoder pass")
        groups = [(layer_ns[e], taps[e], torch.arange(e * B, (e + 1) * B, device=em.device)) for e in range(E)]
        mods = self._modifiers("rescore_batch", context, graph_of, token_lm, token_lm_weight, token_score, _mods)
        found = self._rescore(model, em, em_len, groups, nbest, w, beam, sos, eos, blank, max_workspace_bytes, mods.over_exits(E, B))
        return [[found[e * B + b] for e in range(E)] for b in range(B)]

    @staticmethod
    def _rescore(model, em: Tensor, em_len: Optional[Tensor], groups, nbest: int, w: float, beam: int, sos: int, eos: int, blank: int,
                 max_workspace_bytes: int, mods: _Modifiers = _Modifiers()):
        """The two passes over n searches (``em`` [n, T', V], ``em_len`` [n] or None): one N-best launch for all of them, then one
        ``score_hypotheses`` call per ``(layer_n, enc [m, T', D], rows int64 [m])`` of ``groups`` -- the searches ``rows`` belong to
        exit ``layer_n``, search ``rows[i]`` has the memory ``enc[i]``; every search is in exactly one group.  Returns the list
        of ``(best_tokens, RescoredList)`` per search.  ``mods`` (its ``graph_of`` [n]): under a context graph the first pass is biased
        and its bias enters ``joint``; under a language model it is fused instead and its fusion scores enter ``joint``."""
        dev = em.device
        tokens, counts, ctc, n_hyp, *extra = ctc_beam_decode(em, beam_size=beam, blank=blank, blank_skip_threshold=0.95, em_len=em_len, nbest=nbest,
                                                             **mods.ctc_kw())
        bias = extra[0] if extra else None
        present = torch.arange(nbest, device=dev).view(1, -1) < n_hyp.view(-1, 1)
        lengths = torch.where(present, counts, torch.full_like(counts, -1))
        L = max(int(counts.max()), 1)  # the one host read in front of the second pass: the decoder rows are L + 1 long
        tokens = tokens[:, :, :L].contiguous()
        att = torch.empty_like(ctc)
        for layer_n, enc, rows in groups:
            att[rows] = model.score_hypotheses(enc, layer_n, tokens[rows], lengths[rows], sos, eos, max_workspace_bytes=max_workspace_bytes)
        joint = torch.zeros_like(att, dtype=torch.float64)
        if w < 1.0:
            joint = joint + (1.0 - w) * att.double()
        if w > 0.0:
            joint = joint + w * ctc.double()
        if bias is not None:
            joint = joint + bias.double()
        joint = torch.where(present, joint, torch.full_like(joint, -float("inf")))
        best = _first_argmax(joint).cpu().tolist()
        tokens, counts, n_hyp, ctc, att, joint = (t.cpu().tolist() for t in (tokens, counts, n_hyp, ctc, att, joint))
        fused = None if mods.fusion is None else bias.cpu().tolist()

        def one(i):
            k = n_hyp[i]
            toks = [tokens[i][r][: counts[i][r]] for r in range(k)]
            if fused is None:
                return toks[best[i]], RescoredList(toks, ctc[i][:k], att[i][:k], joint[i][:k])
            lst = FusedRescoredList(toks, ctc[i][:k], att[i][:k], joint[i][:k])
            lst.fusion = fused[i][:k]
            return toks[best[i]], lst
        return [one(i) for i in range(em.size(0))]

    @torch.no_grad()
    def decode_batch_rescoring(self, model, spec: Tensor, valid_len: Tensor, nbest: int = 10, rescoring_ctc_weight: float = 0.5,
                               beam_size: Optional[int] = None, max_batch: Optional[int] = None, lexicon=None, detokenize=None,
                               context=None, graph_of=None, **kw) -> List[List[List[int]]]:
        """``decode_batch`` by two-pass decoding (``rescore_batch``): ``out[b][e]`` is the hypothesis of exit e's CTC N-best list
        (``nbest`` of a beam of ``beam_size``, default ``max(args.beam_size, nbest)``) that scores best under ``(1 - w) * attention +
        w * CTC``.  One encoder pass per chunk of at most ``max_batch`` utterances (taps and log-probs of all exits), one N-best
        launch and one ``score_hypotheses`` call per exit; no decoder step loop.  ``rescoring_ctc_weight`` defaults to 0.5, WeNet's
        customary value; it is not tuned here.  The ids carry no SOS / EOS.  ``lexicon`` / ``detokenize`` as in ``decode_batch``.
        ``token_lm=`` / ``token_lm_weight=`` / ``token_score=`` are ``rescore_batch``'s; the other keywords go to it as they are."""
        mods = self._modifiers("decode_batch_rescoring", context, graph_of, *(kw.pop(k, None) for k in ("token_lm", "token_lm_weight", "token_score")))
        if beam_size is None:
            beam_size = max(int(getattr(self.args, "beam_size", nbest)), nbest)
        E = model._cfg.n_exits
        exits = list(range(1, E + 1))
        valid_len = valid_len.reshape(-1)
        step = max_batch or spec.size(0)
        out: List[List[List[int]]] = []
        for c0 in range(0, spec.size(0), step):
            sp, vl = spec[c0:c0 + step], valid_len[c0:c0 + step]
            logp, taps = model._run_encoder(sp, vl, want_out=True, want_taps=True, n_groups=E)[:2]
            found = self.rescore_batch(model, taps, exits, logp, encoder_lengths(vl.to(logp.device), logp.size(2)), nbest,
                                       rescoring_ctc_weight, beam_size=beam_size, _mods=mods.chunk(c0, step), **kw)
            out += [[best for best, _ in row] for row in found]
            del taps, logp
        return _with_texts(out, lexicon, detokenize)

    # -- adaptive inference: every utterance decoded at the one exit it left the encoder at --------------------------------
    @torch.no_grad()
    def ctc_adaptive_predict(self, model, src: Tensor, lengths: Tensor, threshold=None, beam_size: Optional[int] = None, lexicon=None,
                             detokenize=None, context=None, graph_of=None, token_lm=None, token_lm_weight: Optional[float] = None, token_score: Optional[float] = None,
                             **adaptive) -> Tuple[List[List["CTCHypothesis"]], Tensor]:
        """``model.forward_adaptive(src, lengths, threshold, **adaptive)`` (``criterion=``, ``min_exit=``, ``max_exit=``, ``exit_of=``,
        ``compact=``) and then ONE ``ctc_cuda_predict`` over the B emissions of the chosen exits, over the encoder's own frame counts
        -- where decoding every exit of ``forward`` searches E * B sequences.  Returns ``(hypotheses, exit_of)``: per utterance the
        list ``ctc_cuda_predict`` returns, and the 0-based exit int32 [B] it was decoded at.  ``context`` / ``graph_of`` [B]: as in
        ``ctc_cuda_predict``; ``token_lm`` / ``token_lm_weight`` / ``token_score`` too."""
        if adaptive.get("want_taps"):
            raise ValueError("ctc_adaptive_predict: the CTC search reads no taps")
        out = model.forward_adaptive(src, lengths, threshold, **adaptive)
        em_len = encoder_lengths(lengths.to(out.logp.device), out.logp.size(1))
        return self.ctc_cuda_predict(out.logp, beam_size=beam_size, lexicon=lexicon, detokenize=detokenize, lengths=em_len, context=context,
                                     graph_of=graph_of, token_lm=token_lm, token_lm_weight=token_lm_weight, token_score=token_score), out.exit_of

    # -- keyword spotting: which phrases an utterance contains, and where, at every exit, without decoding it -----------------
    @torch.no_grad()
    def spot(self, model, spec: Tensor, valid_len: Tensor, keywords: KeywordSet, threshold=None):
        """One encoder pass (the log-probs of all exits, no taps) and ``keyword_search`` over the E * B emissions and the encoder's
        own frame counts.  Returns ``KeywordHits`` over [E, B, K], with the trace; with ``threshold`` (a float, or one per keyword)
        ``(hits, hits.first_exit(threshold))``: the shallowest exit int64 [B, K] at which each keyword's best score reaches it."""
        valid_len = valid_len.reshape(-1)
        logp = model._run_encoder(spec, valid_len, want_out=True, want_taps=False, n_groups=model._cfg.n_exits)[0]
        hits = keyword_search(logp, keywords, encoder_lengths(valid_len.to(logp.device), logp.size(2)), want_trace=True)
        return hits if threshold is None else (hits, hits.first_exit(threshold))

    # -- timestamps: when each token (and word) of a transcript was said, at any exit ------------------------------------------
    def _lattice_rows(self, name: str, model, spec: Tensor, valid_len: Tensor, hyps, exits, blank: int):
        """What ``timestamps`` and ``confidences`` (``name``) begin with: one encoder pass (the log-probs of all exits, no taps), the
        encoder's own frame counts, and ``exit_rows`` over the transcripts without the SOS, EOS and PAD ids of ``args``."""
        valid_len = valid_len.reshape(-1)
        logp = model._run_encoder(spec, valid_len, want_out=True, want_taps=False, n_groups=model._cfg.n_exits)[0]
        drop = {int(getattr(self.args, n)) for n in ("trg_sos_idx", "trg_eos_idx", "trg_pad_idx") if hasattr(self.args, n)} - {int(blank)}
        return (logp, encoder_lengths(valid_len.to(logp.device), logp.size(2)),
                exit_rows(name, hyps, exits, int(logp.size(0)), int(logp.size(1)), drop, int(blank)))

    def _frame_seconds(self, frame_seconds: Optional[float]) -> float:
        if frame_seconds is not None:
            return frame_seconds
        hop, rate = getattr(self.args, "hop_length", None), getattr(self.args, "sample_rate", None)
        return 4.0 * hop / rate if hop and rate else FRAME_SECONDS

    @staticmethod
    def _per_exit(rows, exits, logp: Tensor):
        """``rows`` [H] as they are, or nested ``[E][B]`` where ``exits`` was ``"all"``."""
        if rows is None or not isinstance(exits, str):
            return rows
        E, B = int(logp.size(0)), int(logp.size(1))
        return [rows[e * B:(e + 1) * B] for e in range(E)]

    @torch.no_grad()
    def timestamps(self, model, spec: Tensor, valid_len: Tensor, hyps, exits=None, pieces: Optional[Sequence[str]] = None,
                   frame_seconds: Optional[float] = None, blank: int = 0) -> Timestamps:
        """One encoder pass (the log-probs of all exits, no taps) and ONE ``ctc_forced_align`` call that aligns the transcript of
        every utterance against the CTC emission of an exit, over the encoder's own frame counts.  ``hyps[b]``: the tokens of
        utterance b as any ``decode_batch*``, ``ctc_cuda_predict`` or ``greedy_decode`` call returns them (a list of ids, a tensor, a
        hypothesis with ``.tokens``, or a list of those, whose first is taken); the SOS, EOS and PAD ids of ``args`` are removed, a
        ``blank`` in a row is refused.  ``exits``: None -- the last exit --, one 0-based exit per utterance, or ``"all"``: every
        exit, and the results are nested ``[E][B]`` instead of ``[B]``.  Returns ``Timestamps(tokens, words, alignment)``: the
        ``TokenSpan`` list of every utterance in seconds (``frame_seconds``; None: 4 * args.hop_length / args.sample_rate, 0.04
        without those; the stem's receptive-field offset is not corrected, see ``Alignment.spans``), the ``WordSpan`` lists where
        ``pieces`` (the vocabulary's pieces: a piece beginning with U+2581 opens a word) is given, else None, and the ``Alignment``
        itself, row e * B + b for ``"all"`` and row b otherwise.  An utterance whose transcript does not fit its frames has
        status 1 there and empty lists here."""
        logp, lens, (pairs, tokens, tok_len, em_index) = self._lattice_rows("timestamps", model, spec, valid_len, hyps, exits, blank)
        al = ctc_forced_align(logp, tokens, tok_len, em_index, lens, blank=int(blank))
        frame_seconds = self._frame_seconds(frame_seconds)
        host = Alignment(*(t.cpu() for t in (al.tok_start, al.tok_end, al.tok_score, al.frame_token, al.path_score, al.status)),
                         tokens=al.tokens.cpu(), tok_len=al.tok_len.cpu())  # one copy each, not one per span
        tok = [host.spans(h, frame_seconds) for h in range(len(pairs))]
        words = None if pieces is None else [word_spans(sp, starts_word_from_pieces(pieces)) for sp in tok]
        return Timestamps(self._per_exit(tok, exits, logp), self._per_exit(words, exits, logp), al)

    @torch.no_grad()
    def segment(self, model, spec: Tensor, utterances, exit: Optional[int] = None, window: Optional[int] = None, overlap: int = 64,
                pieces: Optional[Sequence[str]] = None, frame_seconds: Optional[float] = None, score_window: int = 30,
                blank: int = 0) -> Segmentation:
        """CTC segmentation of ONE recording, which may be longer than the model's ``max_len``: where each of its ``utterances``
        (token lists as ``timestamps`` takes them, in the order they were said; the SOS, EOS and PAD ids of ``args`` are removed)
        lies in ``spec`` [n_mels, T], and how surely.  ``windowed_emission`` at ``exit`` (0-based; None: the last) with ``window``
        (None: the largest the model takes) and ``overlap`` mel frames, ONE ``ctc_segment`` of the concatenated utterances with
        both ends free, and ``utterance_spans`` with ``score_window`` frames per confidence window; bounds in seconds
        (``frame_seconds`` as in ``timestamps``).  With ``pieces``: ``word_spans`` per utterance.  A transcript that does not fit
        the recording has status 1 in the alignment and empty lists here."""
        drop = {int(getattr(self.args, n)) for n in ("trg_sos_idx", "trg_eos_idx", "trg_pad_idx") if hasattr(self.args, n)} - {int(blank)}
        rows = transcript_rows(utterances, drop, int(blank), "segment")
        if not rows or any(not r for r in rows):
            raise ValueError("segment: every utterance needs at least one token")
        overlap = int(overlap)
        if window is None:
            window = overlap + (int(model._cfg.max_len) - overlap) // 4 * 4
        logp = windowed_emission(model, spec, window, overlap)
        E = int(logp.size(0))
        e = E - 1 if exit is None else int(exit)
        if not 0 <= e < E:
            raise ValueError(f"segment: exit must be one of 0 .. {E - 1}, got {exit}")
        row = logp[e, 0]
        tokens = torch.tensor([[t for r in rows for t in r]], dtype=torch.int32)
        al = ctc_segment(row[None], tokens, blank=int(blank), free_start=True, free_end=True)
        frame_seconds = self._frame_seconds(frame_seconds)
        host = Alignment(*(t.cpu() for t in (al.tok_start, al.tok_end, al.tok_score, al.frame_token, al.path_score, al.status)),
                         tokens=al.tokens.cpu(), tok_len=al.tok_len.cpu())  # one copy each, not one per span
        utts = utterance_spans(host, 0, [len(r) for r in rows], row, int(blank), score_window, frame_seconds)
        words = None
        if pieces is not None:
            tok, table, words, j = host.spans(0, frame_seconds), starts_word_from_pieces(pieces), [], 0
            for r in rows:
                words.append(word_spans(tok[j:j + len(r)], table) if tok else [])
                j += len(r)
        return Segmentation(al, utts, words)

    @torch.no_grad()
    def confidences(self, model, spec: Tensor, valid_len: Tensor, hyps, exits=None, pieces: Optional[Sequence[str]] = None,
                    frame_seconds: Optional[float] = None, blank: int = 0) -> Confidences:
        """``timestamps`` summed over every alignment instead of read off the best one: one encoder pass and ONE ``ctc_posteriors``
        call over the transcripts, the CTC emission of an exit and the encoder's own frame counts.  ``hyps``, ``exits`` (None -- the
        last exit --, one 0-based exit per utterance, or ``"all"``: every exit, results nested ``[E][B]``), ``pieces`` and
        ``frame_seconds`` are ``timestamps``'.  Returns ``Confidences(tokens, words, posteriors)``: the ``SoftSpan`` list of every
        utterance (expected boundaries with their standard deviations, in seconds; expected frames; confidence), the
        ``SoftWordSpan`` lists where ``pieces`` is given, else None, and the ``Posteriors`` itself, row e * B + b for ``"all"`` and
        row b otherwise -- ``nbest_posteriors(posteriors.row_logp, ...)`` compares an utterance's exits or hypotheses.  An utterance
        whose transcript does not fit its frames has status 1 there and empty lists here."""
        logp, lens, (pairs, tokens, tok_len, em_index) = self._lattice_rows("confidences", model, spec, valid_len, hyps, exits, blank)
        po = ctc_posteriors(logp, tokens, tok_len, em_index, lens, blank=int(blank))
        frame_seconds = self._frame_seconds(frame_seconds)
        host = Posteriors(po.row_logp.cpu(), *(getattr(po, n).cpu() for n in TOKEN_FIELDS), None, po.status.cpu(),
                          tokens=po.tokens.cpu(), tok_len=po.tok_len.cpu())  # one copy each, not one per span
        tok = [host.spans(h, frame_seconds) for h in range(len(pairs))]
        words = None if pieces is None else [soft_word_spans(sp, starts_word_from_pieces(pieces)) for sp in tok]
        return Confidences(self._per_exit(tok, exits, logp), self._per_exit(words, exits, logp), po)

    @torch.no_grad()
    def decode_batch_adaptive(self, model, spec: Tensor, valid_len: Tensor, threshold=None, max_length: Optional[int] = None,
                              beam_size: int = 10, joint_ctc_weight: Optional[float] = None, criterion: str = "entropy",
                              min_exit: int = 0, max_exit: Optional[int] = None, exit_of: Optional[Tensor] = None, compact: bool = True,
                              rescoring_ctc_weight: Optional[float] = None, nbest: int = 10, **kw) -> List[Tuple[List[int], int]]:
        """``decode_batch`` at ONE exit per utterance: the adaptive encoder pass (``model.forward_adaptive(..., want_taps=True)``) and
        then, for every distinct chosen exit, one ``beam_search_batch`` over that exit's utterances (``joint_search_batch`` with
        ``joint_ctc_weight=``, over the chosen exits' CTC log-probs and the encoder's frame counts) -- where ``decode_batch`` searches
        all E * B pairs.  Returns ``out[b] = (best_tokens, exit)``, the exit 0-based; ``best_tokens`` is what ``decode_batch``
        returns as ``out[b][exit]``.  Where the batched search declines, the exit's utterances go through ``beam_search`` one by one.
        ``rescoring_ctc_weight`` (None: unchanged): two-pass decoding instead (``rescore_batch``) -- ONE N-best launch over the B
        chosen emissions (``nbest`` of a beam of ``max(beam_size, nbest)``) and one ``score_hypotheses`` call per distinct chosen exit;
        ``best_tokens`` is then what ``decode_batch_rescoring`` returns as ``out[b][exit]``.  Not together with ``joint_ctc_weight``.
        There is no step loop, so ``max_length`` is not used, and the only further keywords are ``SOS_token``, ``EOS_token``,
        ``blank`` and ``max_workspace_bytes`` (``rescore_batch``'s): any other one is a TypeError."""
        if max_length is None:
            max_length = default_max_length(spec.size(2))
        if joint_ctc_weight is not None:
            _check_joint_weight(joint_ctc_weight)
        if rescoring_ctc_weight is not None:
            if joint_ctc_weight is not None:
                raise ValueError("decode_batch_adaptive: rescoring_ctc_weight and joint_ctc_weight are two different searches; give one")
            w = _check_rescoring_weight(rescoring_ctc_weight)
            unknown = sorted(set(kw) - {"SOS_token", "EOS_token", "blank", "max_workspace_bytes"})
            if unknown:
                raise TypeError(f"decode_batch_adaptive: with rescoring_ctc_weight the keywords {unknown} have no meaning")
        ad = model.forward_adaptive(spec, valid_len.reshape(-1), threshold, criterion=criterion, min_exit=min_exit, max_exit=max_exit,
                                    exit_of=exit_of, compact=compact, want_taps=True)
        dev = ad.logp.device
        chosen = ad.exit_of.cpu().tolist()
        if rescoring_ctc_weight is not None:
            groups = []
            for e in sorted(set(chosen)):
                rows = torch.tensor([b for b, c in enumerate(chosen) if c == e], dtype=torch.int64, device=dev)
                groups.append((e + 1, ad.taps[rows], rows))
            found = self._rescore(model, ad.logp, encoder_lengths(valid_len.reshape(-1).to(dev), ad.logp.size(1)), groups, nbest, w,
                                  max(int(beam_size), nbest), self._arg(kw.get("SOS_token"), "trg_sos_idx"),
                                  self._arg(kw.get("EOS_token"), "trg_eos_idx"), int(kw.get("blank", 0)), int(kw.get("max_workspace_bytes", 2 << 30)))
            return [(best, e) for (best, _), e in zip(found, chosen)]
        em_len = encoder_lengths(valid_len.reshape(-1).to(dev), ad.logp.size(1)) if joint_ctc_weight is not None else None
        lockstep = _lockstep_kw(kw)
        out: List[Optional[Tuple[List[int], int]]] = [None] * len(chosen)
        for e in sorted(set(chosen)):
            members = [b for b, c in enumerate(chosen) if c == e]
            rows = torch.tensor(members, dtype=torch.int64, device=dev)
            tap_rows = ad.taps[rows]
            if joint_ctc_weight is not None:
                together = self.joint_search_batch(model, [tap_rows], [e + 1], ad.logp[rows].unsqueeze(0), em_len[rows], joint_ctc_weight,
                                                   max_length, beam_size=beam_size, **(lockstep or {}))
            else:
                together = None if lockstep is None else \
                    self.beam_search_batch(model, [tap_rows], [e + 1], max_length=max_length, beam_size=beam_size, **lockstep)
            if together is None:
                together = [[self.beam_search(model, tap_rows[i:i + 1], e + 1, max_length=max_length, beam_size=beam_size, **kw)]
                            for i in range(len(members))]
            for b, row in zip(members, together):
                out[b] = (row[0][2], e)
        return out

    # -- error-rate scoring of what the decoders above return (scoring.py) ---------------------------------------------------------
    def error_table(self, decoded, refs, unit: str = "token", detokenize=None, lexicon=None, device=None):
        """``scoring.ErrorTable`` of ``decoded`` against ``refs`` [B].  ``decoded`` is what any decoder of this class returns:
        ``decode_batch`` / ``decode_batch_rescoring``'s ``out[b][e]`` (errors [E, B]); ``ctc_cuda_predict``'s per-utterance hypothesis
        lists of one exit, or a list of them over the exits (errors [E, B, N], -1 for a hypothesis a list does not have);
        ``ctc_adaptive_predict``'s ``(hypotheses, exit_of)`` and ``decode_batch_adaptive``'s ``(tokens, exit)`` rows (E = 1: the
        chosen exits).  ``unit="token"``: ids against ids, ``refs`` a list of id lists or ``(targets [B, L], lengths [B])``;
        whatever SOS / EOS / PAD the ids carry is scored as it stands.  ``unit="word"`` / ``"char"``: ``refs`` are strings and every
        hypothesis is ``detokenize(ids)`` -- with ``lexicon`` after ``apply_lex``, as inference.py prints it: the ``.text`` the decoder
        left where it was given the same two, else one lexicon search for all hypotheses of the call.  ``device``: where to score
        (None: ``args.device`` if that is a HIP device, else the host path)."""
        from . import scoring
        if isinstance(decoded, tuple) and len(decoded) == 2 and isinstance(decoded[1], Tensor):
            decoded = decoded[0]  # (hypotheses, exit_of)
        decoded = list(decoded)
        is_hyp = lambda x: hasattr(x, "tokens")  # noqa: E731
        is_ids = lambda x: isinstance(x, (list, tuple)) and all(isinstance(v, int) for v in x)  # noqa: E731
        if decoded and isinstance(decoded[0], tuple) and len(decoded[0]) == 2 and isinstance(decoded[0][1], int) and is_ids(decoded[0][0]):
            hyps, nbest = [[ids for ids, _ in decoded]], False  # (tokens, exit) rows
        elif any(is_hyp(h) for row in decoded for h in row):
            hyps, nbest = [decoded], True  # one exit's [B][N]
        elif any(is_hyp(h) for ex in decoded for row in ex if not is_ids(row) or not row for h in row):
            hyps, nbest = decoded, True  # [E][B][N]
        else:
            E = len(decoded[0]) if decoded else 0
            hyps, nbest = [[row[e] for row in decoded] for e in range(E)], False  # out[b][e]
        if isinstance(refs, tuple) and len(refs) == 2 and isinstance(refs[0], Tensor):
            refs = [refs[0][b, : int(refs[1][b])].tolist() for b in range(refs[0].size(0))]
        if unit != "token":
            if detokenize is None:
                raise ValueError("error_table: scoring words or characters needs detokenize (ids -> str)")
            leaves = [h for ex in hyps for row in ex for h in (row if nbest else [row])]
            ids_of = lambda h: list(getattr(h, "tokens", h))  # noqa: E731
            if lexicon is None:
                texts = [detokenize(ids_of(h)) for h in leaves]
            elif all(getattr(h, "text", None) is not None for h in leaves):
                texts = [h.text for h in leaves]
            else:
                texts = _snapped_texts([ids_of(h) for h in leaves], lexicon, detokenize)
            it = iter(texts)
            hyps = [[[next(it) for _ in row] if nbest else next(it) for row in ex] for ex in hyps]
        if device is None:
            dev = torch.device(getattr(self.args, "device", "cpu"))
            device = dev if dev.type == "cuda" else None
        return scoring.error_table(hyps, refs, unit=unit, layout="EB", device=device, want_nbest=nbest)
