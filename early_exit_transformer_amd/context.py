"""Contextual biasing (hot phrases) for the CTC prefix beam search and the AED lockstep searches (include/eec.h, "Contextual
biasing"; WeNet's context graph, icefall's ContextGraph): ``ContextGraph`` holds phrases and their per-token boosts and builds the
image the kernels read (``eec_context_graph``, on the host), ``ContextBiasSession`` applies it to the step scores of a lockstep
search (``eec_context_bias_step``; CPU tensors take a host path of the same statement).  The CTC search takes a graph through
``ctc_beam_decode(context=, graph_of=)``."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import capi
from .decoding import BeamStateSession


class ContextGraph:
    """``phrases``: rows of token ids of [0, vocab_size), none of them ``blank``, ``eos`` or ``pad``; ``boost``: one finite float
    >= 0 per token for all phrases, or one per phrase.  A hypothesis gains, for every occurrence of a phrase in it (overlapping and
    nested ones count), ``score_of(phrase)``: the boosts along the phrase, where a token shared by several phrases carries the
    largest of theirs.  A partial match carries its bonus provisionally and pays it back when it breaks off or the hypothesis ends.
    ``eos`` / ``pad`` (the AED searches): a hypothesis' bias stops at its first EOS or PAD.  ``bank`` packs several graphs into one
    image, among which ``graph_of`` chooses per sequence."""

    def __init__(self, phrases: Sequence[Sequence[int]], boost: Union[float, Sequence[float]] = 1.5, *, vocab_size: int, blank: int = 0,
                 eos: Optional[int] = None, pad: Optional[int] = None):
        phrases = [tuple(int(t) for t in p) for p in phrases]
        boosts = [float(boost)] * len(phrases) if isinstance(boost, (int, float)) else [float(b) for b in boost]
        if len(boosts) != len(phrases):
            raise ValueError(f"ContextGraph: {len(phrases)} phrases but {len(boosts)} boosts")
        self.vocab_size, self.blank, self.eos, self.pad = int(vocab_size), int(blank), eos, pad
        self._graphs: List[Tuple[List[Tuple[int, ...]], List[float]]] = [(phrases, boosts)]
        self._build()

    @classmethod
    def bank(cls, graphs: Sequence["ContextGraph"]) -> "ContextGraph":
        """One image of all ``graphs`` (same vocabulary and special tokens), graph g of the bank = ``graphs[g]``."""
        graphs = list(graphs)
        if not graphs:
            raise ValueError("ContextGraph.bank: no graphs")
        key = lambda g: (g.vocab_size, g.blank, g.eos, g.pad)  # noqa: E731
        if any(key(g) != key(graphs[0]) for g in graphs):
            raise ValueError("ContextGraph.bank: the graphs must share vocab_size, blank, eos and pad")
        out = cls.__new__(cls)
        out.vocab_size, out.blank, out.eos, out.pad = key(graphs[0])
        out._graphs = [member for g in graphs for member in g._graphs]
        out._build()
        return out

    def _build(self) -> None:
        lib = capi.load()
        n_phr = np.asarray([len(p) for p, _ in self._graphs], dtype=np.int32)
        lens = np.asarray([len(row) for p, _ in self._graphs for row in p], dtype=np.int32)
        toks = np.asarray([t for p, _ in self._graphs for row in p for t in row], dtype=np.int32)
        boost = np.asarray([b for _, bs in self._graphs for b in bs], dtype=np.float64)
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        head = (len(self._graphs), n_phr.ctypes.data, ptr(lens), ptr(toks), ptr(boost), self.vocab_size, self.blank,
                -1 if self.eos is None else int(self.eos), -1 if self.pad is None else int(self.pad))
        nbytes = lib.eec_context_graph_bytes(*head)
        if nbytes == 0:
            capi.check(10001, "eec_context_graph_bytes")  # EEC_ERR_BAD_ARG: the message says what was refused
        image = torch.empty(nbytes // 4, dtype=torch.int32)
        capi.call("eec_context_graph", *head, image, nbytes)
        self.image = image
        self._on = {}
        self._flat = None

    # ---- what the image holds ----
    @property
    def n_graphs(self) -> int:
        return len(self._graphs)

    @property
    def states(self) -> int:
        """The states of the image, over all its graphs."""
        return sum(int(self.image[4 + 4 * g]) for g in range(self.n_graphs))

    @property
    def nbytes(self) -> int:
        return self.image.numel() * 4

    def tables(self, g: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
        """(delta [S, V] fp32, next [S, V] int32, final [S] fp32) of graph g: views of the host image."""
        S, od, on, of = (int(x) for x in self.image[4 + 4 * g: 8 + 4 * g])
        V = self.vocab_size
        return (self.image[od: od + S * V].view(torch.float32).view(S, V), self.image[on: on + S * V].view(S, V),
                self.image[of: of + S].view(torch.float32))

    def to(self, device) -> Tensor:
        """The image on ``device`` (int32 words), uploaded once per device and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = self.image.to(device)
        return self._on[device]

    # ---- the closed form on the host ----
    def score_of(self, phrase: Sequence[int], graph: int = 0) -> float:
        """What one occurrence of ``phrase`` pays in graph ``graph``: the sum over its prefixes of the largest boost among the phrases
        that share the prefix (fp64, in the order of the tokens)."""
        phrase = tuple(int(t) for t in phrase)
        phrases, boosts = self._graphs[graph]
        if phrase not in phrases:
            raise KeyError(f"{phrase} is not a phrase of graph {graph}")
        total = 0.0
        for k in range(1, len(phrase) + 1):
            total = total + max(b for p, b in zip(phrases, boosts) if p[:k] == phrase[:k])
        return total

    def bias_of(self, tokens: Sequence[int], graph: int = 0) -> float:
        """The bias of the finished hypothesis ``tokens``: ``score_of`` summed over every occurrence of every phrase (counted naively,
        position by position), blanks taken out, the row cut at its first ``eos`` / ``pad``.  Outside the bank: 0."""
        if not 0 <= graph < self.n_graphs:
            return 0.0
        row = []
        for t in tokens:
            t = int(t)
            if t in (self.eos, self.pad):
                break
            if t != self.blank:
                row.append(t)
        row = tuple(row)
        total = 0.0
        for p in dict.fromkeys(self._graphs[graph][0]):
            hits = sum(1 for i in range(len(row) - len(p) + 1) if row[i: i + len(p)] == p)
            if hits:
                total += hits * self.score_of(p, graph)
        return total

    def _flat_tables(self):
        """(delta [sum S, V], next [sum S, V] int64, base [G], S [G]) on the host, for ``ContextBiasSession``'s host path."""
        if self._flat is None:
            parts = [self.tables(g) for g in range(self.n_graphs)]
            sizes = torch.tensor([p[0].size(0) for p in parts], dtype=torch.int64)
            self._flat = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]).to(torch.int64), torch.cumsum(sizes, 0) - sizes, sizes)
        return self._flat


def graph_rows(name: str, graph_of, n: int, dev) -> Optional[Tensor]:
    """``graph_of`` as the kernels read it: int32 [n] on ``dev``, or None (graph 0 for every sequence)."""
    if graph_of is None:
        return None
    g = torch.as_tensor(graph_of)
    if g.dtype not in (torch.int32, torch.int64) or g.numel() != n:
        raise ValueError(f"{name}: graph_of must be {n} int32 / int64 graph indices")
    return g.reshape(n).clamp(-1, 2 ** 31 - 1).to(device=dev, dtype=torch.int32).contiguous()


class ContextBiasSession(BeamStateSession):
    """The bias of n lockstep beam searches of up to ``R`` beams each: ``step(local [n, R', V], last [n, R'], parent [n, R'] | None)
    -> local`` first advances every beam's graph state -- beam r extends row ``parent[i, r]`` of the previous step by the token
    ``last[i, r]``; the first call starts at the root and does not read ``last`` (SOS) -- and then adds ``delta[state][v]`` to the row
    (-inf stays -inf).  The signature ``CtcPrefixSession.step`` has; it goes between the decoder's step and ``beam_select``.  Device
    tensors: one launch per step on the current stream (eec_context_bias_step), no synchronisation; CPU tensors: the same statement in
    tensor ops.  ``graph_of`` [n] chooses a graph of a bank per search (None: graph 0; outside the bank: no biasing)."""

    def __init__(self, graph: ContextGraph, n: int, R: int, graph_of=None):
        if not 1 <= int(R) <= 16:
            raise ValueError(f"1 .. 16 beams per search, got {R}")
        self.graph, self.n, self.R_max, self.V = graph, int(n), int(R), graph.vocab_size
        self._graph_of = graph_rows("ContextBiasSession", graph_of, self.n, "cpu")

    def _begin(self, dev) -> None:
        if dev.type != "cuda":
            return
        self._image = self.graph.to(dev)
        self._g = None if self._graph_of is None else self._graph_of.to(dev)
        self._new_state(capi.load().eec_context_bias_state_bytes(self.n, self.R_max))

    def _launch(self, local, tok, par, R, out) -> None:
        capi.launch("eec_context_bias_step", self._dev, self._image, self.graph.nbytes, self._g, self.n, R, self.rows, self.R_max, self.V,
                    self.s, par, tok, local, out, self._state, self._nbytes)

    def final(self, last: Tensor, parent: Optional[Tensor] = None) -> Tensor:
        """``final[state]`` [n, R'] fp32 of the beams the last selection made -- beam r extends row ``parent[i, r]`` of the last ``step``
        by ``last[i, r]`` --: what a search that ends its rows without an EOS adds to their scores, so that an open partial match gives
        its provisional bonus back (0 for a row in the dead state, and where biasing is off).  Tensor ops on the image, once per
        search; no launch of the library."""
        n, V, dev = self.n, self.V, last.device
        if self.s == 0:
            return torch.zeros(tuple(last.shape), dtype=torch.float32, device=dev)
        image = self.graph.to(dev)
        g = torch.zeros(n, dtype=torch.int64) if self._graph_of is None else self._graph_of.to(torch.int64)
        on = (g >= 0) & (g < self.graph.n_graphs)
        rec = self.graph.image[4: 4 + 4 * self.graph.n_graphs].view(-1, 4).to(torch.int64)[g.clamp(0, self.graph.n_graphs - 1)]
        S, o_next, o_fin, on = (t.to(dev).view(n, 1) for t in (rec[:, 0], rec[:, 2], rec[:, 3], on))
        last = last.to(torch.int64)
        p = torch.arange(last.size(1), device=dev).expand_as(last) if parent is None else parent.to(torch.int64)
        ok = (p >= 0) & (p < self.rows) & (last >= 0) & (last < V) & on
        prev = self.states().to(device=dev, dtype=torch.int64).gather(1, p.clamp(0, self.rows - 1))
        st = image[o_next + prev * V + last.clamp(0, V - 1)].to(torch.int64)
        st = torch.where(ok & (st >= 0) & (st < S), st, torch.zeros_like(st))
        fin = image[o_fin + st].view(torch.float32)
        return torch.where(on, fin, torch.zeros_like(fin))

    def _host_step(self, local: Tensor, last: Tensor, parent: Optional[Tensor], R: int) -> Tensor:
        n, V = self.n, self.V
        delta, nxt, base, sizes = self.graph._flat_tables()
        g = torch.zeros(n, dtype=torch.int64) if self._graph_of is None else self._graph_of.to(torch.int64)
        on = (g >= 0) & (g < self.graph.n_graphs)
        g = g.clamp(0, self.graph.n_graphs - 1)
        b, S = base[g].view(n, 1), sizes[g].view(n, 1)
        st = torch.zeros((n, R), dtype=torch.int64)
        if self.s > 0:
            p = torch.arange(R).expand(n, R) if parent is None else parent
            ok = (p >= 0) & (p < self.rows) & (last >= 0) & (last < V)
            ps = self._host_state.gather(1, p.clamp(0, self.rows - 1))
            cand = nxt[b + ps, last.clamp(0, V - 1)]
            cand = torch.where((cand >= 0) & (cand < S), cand, torch.zeros_like(cand))
            st = torch.where(ok & on.view(n, 1), cand, st)
        self._host_state = st
        biased = local + delta[b + st]  # [n, R, V]; -inf + a finite boost is -inf
        return torch.where(on.view(n, 1, 1) & (local != float("-inf")), biased, local)
