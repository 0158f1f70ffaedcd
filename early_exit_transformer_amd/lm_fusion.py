"""Shallow fusion with a token-level n-gram language model in the lexicon-free searches (include/eec.h, "Shallow fusion: token-level
n-gram model"; what WeNet, ESPnet and icefall offer beside a hybrid CTC / attention model): ``TokenLM`` is a back-off n-gram over the
model's own tokens, read from an ARPA file whose words are the pieces, packed by ``eec_ngram_pack`` (the image ``lexicon.NGramLM``
makes) and kept on the device.  ``LMFusionSession`` adds its increments to the step scores of a lockstep AED search
(``eec_lm_fusion_step``; CPU tensors take a host path of the same statement, bit for bit); the CTC prefix beam search takes a model
through ``ctc_beam_decode(lm=)``.  ``DEFAULT_LM_WEIGHT`` = 0.3 is the customary starting point, a choice and not a tuned value."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import capi
from .decoding import BeamStateSession
from .lexicon import NGramLM

DEFAULT_LM_WEIGHT = 0.3
MAX_VOCAB, MAX_BEAMS, MAX_WORDS = 256, 16, 512  # include/eec.h
DEAD = -1  # the state of a row after its EOS
_NEG_INF = np.float32("-inf")


class _Pieces:
    """What ``NGramLM.from_arpa`` reads of a lexicon: its ``words``."""

    def __init__(self, words):
        self.words = list(words)


def _token(name: str, t, V: int) -> int:
    if t is None:
        return -1
    if not 0 <= int(t) < V:
        raise ValueError(f"TokenLM: {name} = {t} is no token of [0, {V})")
    return int(t)


class TokenLM:
    """A back-off n-gram model over the ``V`` tokens of a model.  ``blank`` / ``sos`` / ``pad`` (None: none) are the tokens that pay 0
    and keep the state, ``eos`` (None: none) scores as the model's ``</s>`` and ends a row; they are arguments of the kernels, never
    looked up.  ``order``, ``n_nodes``, ``vocab``, ``word_map`` [V], ``bos`` / ``eos_word`` / ``unk`` (LM words, or -1): as
    ``lexicon.NGramLM`` has them."""

    def __init__(self, words: Sequence[np.ndarray], logp: Sequence[np.ndarray], backoff: Sequence[np.ndarray], V: int, word_map=None, *,
                 bos: int = -1, eos_word: int = -1, unk: int = -1, vocab: Optional[Sequence[str]] = None, blank: Optional[int] = 0,
                 sos: Optional[int] = None, eos: Optional[int] = None, pad: Optional[int] = None):
        """From arrays per order, as ``NGramLM`` takes them; ``word_map`` [V]: the LM word of every token (None: token v is LM word v)."""
        V = int(V)
        if not 1 <= V <= MAX_VOCAB:
            raise ValueError(f"TokenLM: vocabularies of 1 to {MAX_VOCAB} tokens are served, got {V}")
        if len(words) > NGramLM.MAX_ORDER:
            raise ValueError(f"TokenLM: orders 1 to {NGramLM.MAX_ORDER} are served, got {len(words)}")
        W = len(np.asarray(words[0]).reshape(-1)) if len(words) else 0
        if W > MAX_WORDS:
            raise ValueError(f"TokenLM: a token-level model has at most {MAX_WORDS} LM words (the pieces and <s>, </s>, <unk>), got {W}")
        if word_map is None:
            if W < V:
                raise ValueError(f"TokenLM: without word_map token v is LM word v, but the model has {W} LM words for {V} tokens")
            word_map = np.arange(V, dtype=np.int32)
        word_map = np.asarray(word_map, dtype=np.int32).reshape(-1)
        if word_map.size != V:
            raise ValueError(f"TokenLM: word_map must hold {V} LM words, one per token, got {word_map.size}")
        self._wrap(NGramLM(words, logp, backoff, word_map, bos, eos_word, unk, vocab), V, blank, sos, eos, pad)

    def _wrap(self, ngram: NGramLM, V: int, blank, sos, eos, pad) -> None:
        self.ngram, self.V = ngram, V
        self.blank, self.sos, self.eos, self.pad = (_token(k, t, V) for k, t in (("blank", blank), ("sos", sos), ("eos", eos), ("pad", pad)))
        self.order, self.n_nodes, self.vocab, self.word_map = ngram.order, ngram.n_nodes, ngram.vocab, ngram.word_map
        self.bos, self.eos_word, self.unk = ngram.bos, ngram.eos, ngram.unk
        # the sections of the host image (include/eec.h), for the host path and the closed form
        im = ngram._image.numpy().view(np.int32)
        h = [int(x) for x in im[:16]]
        self._n_edges, self._W, self._start, self._eos_word, self._top = h[3], h[4], h[6], h[7], h[8]
        self._begin, self._eword = im[h[9]: h[9] + h[2] + 1], im[h[10]: h[10] + h[3]]
        self._logp, self._backoff = im[h[11]: h[11] + h[2]].view(np.float32), im[h[12]: h[12] + h[2]].view(np.float32)
        self._suffix, self._map = im[h[13]: h[13] + h[2]], im[h[14]: h[14] + V]
        self._rows: Dict[int, np.ndarray] = {}

    @classmethod
    def from_arpa(cls, path, pieces: Sequence[str], blank: Optional[int] = 0, sos: Optional[int] = None, eos: Optional[int] = None,
                  pad: Optional[int] = None) -> "TokenLM":
        """The ARPA file ``path`` whose words are piece strings, read against ``pieces`` (token v is ``pieces[v]``) by
        ``NGramLM.from_arpa``: a piece the model lacks scores as ``<unk>``; without an ``<unk>`` the pieces it lacks are counted in
        a ``ValueError``, the special tokens exempt (they are never looked up).  The file's log10 values are kept as they are."""
        V = len(pieces)
        if not 1 <= V <= MAX_VOCAB:
            raise ValueError(f"TokenLM: vocabularies of 1 to {MAX_VOCAB} tokens are served, got {V}")
        special = [_token(k, t, V) for k, t in (("blank", blank), ("sos", sos), ("eos", eos), ("pad", pad))]
        names = list(pieces)
        if special[1] >= 0:
            names[special[1]] = NGramLM.BOS
        if special[2] >= 0:
            names[special[2]] = NGramLM.EOS  # so that the CTC search, which has no eos argument, scores the label as </s> too
        out = cls.__new__(cls)
        out._wrap(NGramLM.from_arpa(path, _Pieces(names), exempt=[t for t in special if t >= 0]), V, blank, sos, eos, pad)
        return out

    # ---- the image ----
    @property
    def nbytes(self) -> int:
        return int(self.ngram._image.numel())

    def on(self, dev) -> Tensor:
        """The packed image on ``dev`` (uploaded once; follows a change of device)."""
        return self.ngram.on(torch.device(dev))

    @property
    def skip(self) -> Tuple[int, int, int]:
        """(blank, sos, pad), -1 where there is none: the tokens that pay 0 and keep the state."""
        return self.blank, self.sos, self.pad

    # ---- the statement on the host: fp32, in the walk's order ----
    def _node(self, s: int) -> int:
        return s if 0 <= s < self.n_nodes else 0

    def walk(self, s: int, u: int) -> Tuple[np.float32, int]:
        """(acc, next) of LM word ``u`` from node ``s``: the back-off walk of include/eec.h, fp32 additions in its order."""
        acc = np.float32(0.0)
        s = self._node(int(s))
        for d in range(NGramLM.MAX_ORDER + 1):
            x = u + 1
            if s != 0 and d < NGramLM.MAX_ORDER:
                lo, end = int(self._begin[s]), int(self._begin[s + 1])
                k = lo + int(np.searchsorted(self._eword[lo:end], u))
                x = k + 1 if k < end and self._eword[k] == u else -1
            if x >= 0:
                acc = np.float32(acc + self._logp[x])
                return acc, (x if x < self._top else self._node(int(self._suffix[x])))
            acc = np.float32(acc + self._backoff[s])
            s = self._node(int(self._suffix[s]))
        return acc, 0

    def acc_row(self, s: int) -> np.ndarray:
        """``acc`` [W] fp32 of every LM word from node ``s``, the way the step kernel forms it: the suffix chain of ``s`` walked once
        with the back-offs passed in front of each node, then the root's unigrams and each chain node's edges written, the deepest
        node last.  ``walk``'s bits."""
        s = self._node(int(s))
        if s not in self._rows:
            chain, node, b = [], s, np.float32(0.0)
            for k in range(NGramLM.MAX_ORDER + 1):
                if k == NGramLM.MAX_ORDER:
                    node = 0
                chain.append((node, b))
                if node == 0:
                    break
                b = np.float32(b + self._backoff[node])
                node = self._node(int(self._suffix[node]))
            row = (chain[-1][1] + self._logp[1: self._W + 1]).astype(np.float32)
            for node, b in reversed(chain[:-1]):
                lo, end = int(self._begin[node]), int(self._begin[node + 1])
                row[self._eword[lo:end]] = b + self._logp[lo + 1: end + 1]
            self._rows[s] = row
        return self._rows[s]

    def after(self, s: int, token: int) -> int:
        """The state after ``token`` from state ``s`` (the AED reading: ``eos`` ends the row, skip tokens keep the state)."""
        if s == DEAD or token == self.eos:
            return DEAD
        if token in self.skip:
            return self._node(s)
        return self.walk(s, int(self._map[token]))[1]

    def inc_row(self, s: int, lm_weight: float, token_score: float) -> np.ndarray:
        """inc(s, v) [V] fp32 for every token: fl(fl(lm_weight * acc) + token_score); 0 for a skip token and in the dead state."""
        inc = np.zeros(self.V, dtype=np.float32)
        w, ts = np.float32(lm_weight), np.float32(token_score)
        if s == DEAD or (w == 0 and ts == 0):
            return inc
        acc = self.acc_row(s)
        inc = (w * acc[self._map]).astype(np.float32) + ts
        if self.eos >= 0:
            inc[self.eos] = np.float32(w * (acc[self._eos_word] if self._eos_word >= 0 else np.float32(0.0))) + ts
        for t in self.skip:
            if t >= 0 and t != self.eos:
                inc[t] = 0.0
        return inc.astype(np.float32)

    def score_of(self, tokens: Sequence[int], lm_weight: float = DEFAULT_LM_WEIGHT, token_score: float = 0.0, ctc: bool = False) -> float:
        """The fusion score of the token row ``tokens``, the closed form on the host: fl(fusion + inc) in fp32 along the row.  A row of
        an AED search (a leading SOS is not scored; ``eos`` pays ``</s>`` and ends the row; skip tokens pay 0), or with ``ctc=True`` a
        row of the CTC search: the blank is its only skip token, every other label is scored through ``word_map``, and the model's
        ``</s>`` is paid once at the end, without the bonus."""
        w, ts = np.float32(lm_weight), np.float32(token_score)
        row = [int(t) for t in tokens]
        if any(not 0 <= t < self.V for t in row):
            raise ValueError(f"TokenLM.score_of: a token outside [0, {self.V})")
        if not ctc and row and row[0] == self.sos:
            row = row[1:]
        total, s = np.float32(0.0), self._node(self._start)
        if w == 0 and ts == 0:
            return 0.0
        for t in row:
            if s == DEAD:
                break
            if not ctc and t == self.eos:
                acc, s = (self.walk(s, self._eos_word)[0] if self._eos_word >= 0 else np.float32(0.0)), DEAD
            elif (t == self.blank) if ctc else (t in self.skip):
                continue
            else:
                acc, s = self.walk(s, int(self._map[t]))
            inc = np.float32(np.float32(w * acc) + ts)
            if inc != 0:
                total = np.float32(total + inc)
        if ctc and self._eos_word >= 0:
            total = np.float32(total + np.float32(w * self.walk(s, self._eos_word)[0]))
        return float(total)


def image_trusted(image: np.ndarray, V: int) -> bool:
    """Whether the kernels fuse with the packed image ``image`` (int32 words) for a vocabulary of ``V`` tokens: the checks of
    include/eec.h, "Never trust the image" (csrc/eec_lm.h: tlm_view)."""
    words = int(image.size)
    if words < 16:
        return False
    h = [int(x) for x in image[:16]]
    if h[0] != 0x4E434545 or h[5] != V:
        return False
    order, n_nodes, n_edges, W = h[1:5]
    if not 1 <= order <= NGramLM.MAX_ORDER or n_nodes < 2 or n_edges != n_nodes - 1 or not 1 <= W <= min(MAX_WORDS, n_edges):
        return False
    if h[15] > words or not 0 <= h[6] < n_nodes or not -1 <= h[7] < W:
        return False
    return all(at >= 16 and at + size <= words for at, size in zip(h[9:15], (n_nodes + 1, n_edges, n_nodes, n_nodes, n_nodes, V)))


def check_lm(name: str, lm, V: int, beam: int, lm_weight: float, token_score: float) -> None:
    """The refusals every fused search makes before any device work."""
    if not isinstance(lm, TokenLM):
        raise TypeError(f"{name}: lm must be a lm_fusion.TokenLM, got {type(lm).__name__}")
    if lm.V != V:
        raise ValueError(f"{name}: the language model is over {lm.V} tokens, the search over {V}")
    if not 1 <= V <= MAX_VOCAB:
        raise ValueError(f"{name}: shallow fusion serves vocabularies of up to {MAX_VOCAB} tokens, got {V}")
    if not 1 <= int(beam) <= MAX_BEAMS:
        raise ValueError(f"{name}: shallow fusion serves 1 .. {MAX_BEAMS} beams per search, got {beam}")
    if not (np.isfinite(lm_weight) and np.isfinite(token_score)):
        raise ValueError(f"{name}: lm_weight and token_score must be finite")


class LMFusionSession(BeamStateSession):
    """Shallow fusion for n lockstep beam searches of up to ``R`` beams each: ``step(local [n, R', V], last [n, R'], parent [n, R'] |
    None) -> local`` first advances every beam's LM state -- beam r extends row ``parent[i, r]`` of the previous step by the token
    ``last[i, r]``; the first call starts at the model's start state and does not read ``last`` (SOS) -- and then adds
    ``inc(state, v)`` to the row (-inf stays -inf).  ``ContextBiasSession.step``'s signature and place in the loop; the two compose,
    both are additive; ``states()`` are the LM states, -1 for a row past its EOS.  Device tensors: one launch per step on the current
    stream (eec_lm_fusion_step), no synchronisation.  CPU tensors: the same statement in NumPy fp32, bit for bit -- per row, the back-off
    walk's additions in its order, one rounded product ``lm_weight * acc``, one rounded sum with ``token_score``, one rounded sum with
    the entry."""

    def __init__(self, lm: TokenLM, n: int, R: int, lm_weight: float = DEFAULT_LM_WEIGHT, token_score: float = 0.0, image: Optional[Tensor] = None):
        """``image`` (None: the model's own): the packed image the session hands to the kernel instead, a host uint8 tensor -- for
        the checks of an image that is not trusted, which switch fusion off."""
        check_lm("LMFusionSession", lm, lm.V, R, lm_weight, token_score)
        self._host_image = image
        self.lm, self.n, self.R_max, self.V = lm, int(n), int(R), lm.V
        self.lm_weight, self.token_score = float(lm_weight), float(token_score)

    def _begin(self, dev) -> None:
        if dev.type != "cuda":
            return
        self._image = self.lm.on(dev) if self._host_image is None else self._host_image.to(dev)
        self._image_bytes = self.lm.nbytes if self._host_image is None else int(self._host_image.numel() * self._host_image.element_size())
        self._new_state(capi.load().eec_lm_fusion_state_bytes(self.n, self.R_max))

    def _launch(self, local, tok, par, R, out) -> None:
        capi.launch("eec_lm_fusion_step", self._dev, self._image, self._image_bytes, self.n, R, self.rows, self.R_max, self.V, self.s, par, tok,
                    local, out, self._state, self._nbytes, self.lm_weight, self.token_score, self.lm.eos, *self.lm.skip)

    def _host_step(self, local: Tensor, last: Tensor, parent: Optional[Tensor], R: int) -> Tensor:
        n, V, lm = self.n, self.V, self.lm
        if self._host_image is not None and not image_trusted(self._host_image.numpy().view(np.int32), V):
            self._host_state = torch.zeros((n, R), dtype=torch.int64)
            return local.clone()
        start = lm._node(lm._start)
        st = np.full((n, R), start, dtype=np.int64)
        if self.s > 0:
            tok = last.numpy()
            par = np.broadcast_to(np.arange(R), (n, R)) if parent is None else parent.numpy()
            prev = self._host_state.numpy()
            for i in range(n):
                for r in range(R):
                    if 0 <= par[i, r] < self.rows and 0 <= tok[i, r] < V:
                        st[i, r] = lm.after(int(prev[i, par[i, r]]), int(tok[i, r]))
        self._host_state = torch.from_numpy(st)
        x = local.numpy()
        out = x.copy()
        for i in range(n):
            for r in range(R):
                inc = lm.inc_row(int(st[i, r]), self.lm_weight, self.token_score)
                out[i, r] = np.where((x[i, r] == _NEG_INF) | (inc == 0), x[i, r], (x[i, r] + inc).astype(np.float32))
        return torch.from_numpy(out)
