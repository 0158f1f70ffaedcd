"""Attention-decoder side of ``full_conformer`` on the HIP path: one step of beam bookkeeping (``beam_select``), the step-wise
decoding sessions over key / value caches (csrc/decoder_step.hip, decoder_batch.hip), the base of the sessions that rescore a
step of a lockstep search (``ScorerSession``) and the decoder's training step behind autograd (csrc/decoder_train.hip)."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import capi
from .capi import aligned_ws, launch


def beam_select(logp: Tensor, scores: Tensor, penalty: float, k: int, tokens_old: Tensor, tokens_new: Tensor, length: int):
    """One step of beam-search bookkeeping for n searches in lockstep, in one launch (eec_beam_select): the ``k`` best of
    ``scores[i, r] + logp[i, r, v] / penalty`` per search i, best first -> ``(scores [n, k], parent [n, k], token [n, k])``,
    and ``tokens_new[i, b, :length + 1] = cat(tokens_old[i, parent[i, b], :length], token[i, b])``.  What
    util/beam_infer.py:241-262 does with topk / index / cat, for every exit of an utterance at once."""
    n, R, V = logp.shape
    dev = logp.device
    if tokens_old.shape != tokens_new.shape or tokens_old.dim() != 3 or tokens_old.size(0) != n:
        raise ValueError("token buffers: two [n, rows, steps] int64 tensors")
    if not logp.is_cuda:  # the same step as tensor ops, for sessions that live on the host (tests/test_host.py)
        cand = (scores.unsqueeze(2) + logp / penalty).reshape(n, -1)
        if k > R * V:  # fewer candidates than beams: the kernel fills up with candidate 0 at -inf
            cand = torch.cat([cand, cand.new_full((n, k - R * V), float("-inf"))], dim=1)
        out_s, idx = torch.topk(cand, k, dim=1)
        idx = torch.where(idx >= R * V, torch.zeros_like(idx), idx)
        parent, tok = torch.div(idx, V, rounding_mode="floor"), torch.remainder(idx, V)
        tokens_new[:, :k, :length] = torch.gather(tokens_old[:, :, :length], 1, parent.unsqueeze(2).expand(-1, -1, length))
        tokens_new[:, :k, length] = tok
        return out_s, parent, tok
    out_s = torch.empty((n, k), dtype=torch.float32, device=dev)
    parent = torch.empty((n, k), dtype=torch.int64, device=dev)
    tok = torch.empty((n, k), dtype=torch.int64, device=dev)
    logp, scores = logp.contiguous(), scores.contiguous()  # named: they live across the call
    launch("eec_beam_select", dev, n, R, V, int(k), logp, scores, float(penalty), out_s, parent, tok, tokens_old, tokens_new, int(length),
           tokens_old.size(2), tokens_old.size(1))
    return out_s, parent, tok


class DecoderStepSession:
    """Step-wise AED decoding state over key / value caches (include/eec.h): ``step(tokens [*lead, R], parent [*lead, R] | None)``
    returns the log-probs of the NEXT token of every live beam, [*lead, R, V] -- what
    ``model._decoder_(prefixes, enc, layer_n)[:, -1]`` returns (util/beam_infer.py:236-240) -- from the last token of every
    beam and the row of the previous step it extends.  ``lead`` is the shape of the searches advanced in lockstep by the same
    launches; a subclass owns the cache(s) and contributes the two launches, ``_begin`` (one per tensor of ``encs`` and cache)
    and ``_step``."""

    MAX = 8  # decoders per call

    def __init__(self, model, ps_list, d_ff: int, V: int, encs: List[Tensor], lead: Tuple[int, ...], max_steps: int, nbytes: int):
        lib = capi.load()
        cfg = model._cfg
        self.lead, self.V, self.max_steps, self.nbytes = lead, V, max_steps, nbytes
        self.dev, self.Tq = encs[0].device, encs[0].size(-2)
        self.s, self.rows = 0, 0
        self.max_beams = lib.eec_decoder_step_max_beams()
        self._ps_keep = ps_list
        self.ps = (C.POINTER(capi.EecDecoderParams) * len(ps_list))(*[C.pointer(p) for p in ps_list])
        self.geo = (cfg.d_model, cfg.n_heads, d_ff, V)
        self.pad_idx, passes = int(model.trg_pad_idx), int(model.decoder_passes)
        stream = torch.cuda.current_stream(self.dev)
        self._caches = [aligned_ws(nbytes, self.dev) for _ in encs]
        self.ptrs = (C.c_void_p * len(encs))(*[ptr for _, ptr in self._caches])
        for i, enc in enumerate(encs):
            enc_c = enc.contiguous().float()  # named: it lives across the call
            self._begin(i, enc_c, passes)
            enc_c.record_stream(stream)
            self._caches[i][0].record_stream(stream)

    def step(self, last_tokens: Tensor, parent: Optional[Tensor] = None, log_softmax: bool = True) -> Tensor:
        lead = self.lead
        if last_tokens.dim() != len(lead) + 1 or last_tokens.shape[:-1] != lead:
            raise ValueError(f"last_tokens must be [{', '.join(map(str, lead + ('live beams',)))}]")
        R = int(last_tokens.size(-1))
        if not 1 <= R <= self.max_beams:
            raise ValueError(f"1 .. {self.max_beams} live beams per search and step, got {R}")
        if self.s >= self.max_steps:
            raise RuntimeError(f"the session was opened for {self.max_steps} steps")
        if parent is not None and parent.shape != last_tokens.shape:
            raise ValueError("parent: one row of the previous step per live beam of every search")
        dev = self.dev
        tok = last_tokens.to(device=dev, dtype=torch.int64).contiguous()
        par = parent.to(device=dev, dtype=torch.int64).contiguous() if parent is not None and self.s > 0 else None
        out = torch.empty((*lead, R, self.V), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        self._step(tok, par, R, int(log_softmax), out)
        tok.record_stream(stream)
        if par is not None:
            par.record_stream(stream)
        self.s += 1
        self.rows = R
        return out


class ScorerSession:
    """What the scorers of a lockstep search share (``ctc.CtcPrefixSession``, ``context.ContextBiasSession``,
    ``lm_fusion.LMFusionSession``): ``step(local [n, R, V], last [n, R], parent [n, R] | None) -> [n, R, V]`` checks the shapes,
    hands fp32 / int64 tensors to the host path (CPU tensors) or to the one launch of the device path -- on the current stream, no
    synchronisation; ``parent`` is not read at step 0 -- and counts the step (``s``) and its live beams (``rows``).  A subclass has
    ``n``, ``V`` and ``R_max`` and contributes ``_device(local)`` (where the session lives), ``_launch(local, tok, par, R, out)``
    and ``_host_step(local, last, parent, R) -> out``."""

    _arg = "local"  # the first argument's name in messages
    s = rows = 0

    def _check_rows(self, R: int) -> None:
        if not 1 <= R <= self.R_max:
            raise ValueError(f"1 .. {self.R_max} live beams per search and step, got {R}")

    def step(self, local: Tensor, last: Tensor, parent: Optional[Tensor] = None) -> Tensor:
        n, V = self.n, self.V
        if local.dim() != 3 or local.size(0) != n or local.size(2) != V:
            raise ValueError(f"{self._arg} must be [{n}, live beams, {V}], got {tuple(local.shape)}")
        R = int(local.size(1))
        self._check_rows(R)
        if tuple(last.shape) != (n, R) or (parent is not None and tuple(parent.shape) != (n, R)):
            raise ValueError(f"last and parent must be [{n}, {R}]")
        dev = self._device(local)
        if dev.type != "cuda":
            out = self._host_step(local.float(), last.to(torch.int64), None if parent is None else parent.to(torch.int64), R)
        else:
            local = capi.require_fp32(self._arg, local, dev)
            if last.device != dev or (parent is not None and parent.device != dev):
                raise RuntimeError(f"last and parent must be on {dev}")
            tok = last.to(torch.int64).contiguous()
            par = parent.to(torch.int64).contiguous() if parent is not None and self.s > 0 else None
            out = torch.empty_like(local)
            self._launch(local, tok, par, R, out)
            stream = torch.cuda.current_stream(dev)
            for t in (local, tok, par):
                if t is not None:
                    t.record_stream(stream)
        self.s += 1
        self.rows = R
        return out


class BeamStateSession(ScorerSession):
    """A scorer whose state is one int32 per beam, double-buffered on the device ([2, n, R_max] in ``_state``: step s reads half
    ``s & 1`` and writes the other) and ``_host_state`` [n, R'] on the host.  It lives where the tensors of its first step live;
    ``_begin(dev)`` prepares that device."""

    _dev = _host_state = None

    def _device(self, local: Tensor):
        if self._dev is None:
            self._dev = local.device
            self._begin(local.device)
        elif local.device != self._dev:
            raise RuntimeError(f"the session lives on {self._dev}, local is on {local.device}")
        return self._dev

    def _new_state(self, nbytes: int) -> None:
        self._nbytes = nbytes
        self._state = torch.zeros(max(nbytes // 4, 1), dtype=torch.int32, device=self._dev)

    def states(self) -> Tensor:
        """The state int32 [n, R'] of the current beams (after the last ``step``)."""
        if self._dev is None or self._dev.type != "cuda":
            return self._host_state.to(torch.int32).clone()
        return self._state[: 2 * self.n * self.R_max].view(2, self.n, self.R_max)[self.s & 1, :, : max(self.rows, 1)].clone()


class _ExitSessions(DecoderStepSession):
    """n <= 8 exits of ONE utterance, a cache per exit (csrc/decoder_step.hip); ``lead`` is (n,), or () for a single exit.  A
    single exit is a group of one, as eec_decoder_step is eec_decoder_step_multi with n = 1."""

    def _begin(self, i, enc, passes):
        launch("eec_decoder_begin", self.dev, self.ps[i], *self.geo, enc, self.Tq, self.max_steps, passes, self.ptrs[i], self.nbytes)

    def _step(self, tok, par, R, log_softmax, out):
        launch("eec_decoder_step_multi", self.dev, len(self.ps), self.ps, *self.geo, self.pad_idx, tok, par, R, self.rows, self.s, self.Tq,
               self.max_steps, log_softmax, out, self.ptrs, self.nbytes)


class _BatchSession(DecoderStepSession):
    """E exits x B utterances of a padded batch, one cache for all of them (csrc/decoder_batch.hip); ``lead`` is (E, B).  The
    launches of a step do not depend on E or B.  Log-probs only."""

    E = property(lambda self: self.lead[0])
    B = property(lambda self: self.lead[1])

    def _begin(self, i, taps, passes):
        launch("eec_decoder_batch_begin", self.dev, self.ps, *self.lead, *self.geo, taps, self.Tq, self.max_steps, passes, self.ptrs[0],
               self.nbytes)

    def _step(self, tok, par, R, log_softmax, out):
        if not log_softmax:
            raise ValueError("the batch session returns log-probs only")
        launch("eec_decoder_batch_step", self.dev, self.ps, *self.lead, *self.geo, self.pad_idx, tok, par, R, self.rows, self.s, self.Tq,
               self.max_steps, out, self.ptrs[0], self.nbytes)


class _DecoderTrainFn(torch.autograd.Function):
    """Exit ``idx``'s attention decoder in train mode and its backward on the HIP training kernels (eec_decoder_train_forward /
    _backward): ``linears_2[idx](decoders[idx](positional_encoder_2(emb(trg)), enc, causal + padding masks))`` -> raw logits
    [B, S, V], differentiable with respect to every decoder parameter, the embedding table and ``enc`` (the encoder tap)."""

    @staticmethod
    def forward(ctx, model, idx, trg, enc, seed, names, *params):
        lib = capi.load()
        dev = trg.device
        cfg = model._cfg
        Bm, S = trg.shape
        Tq = enc.size(1)
        if enc.size(0) != Bm or enc.size(2) != cfg.d_model:
            raise ValueError(f"enc must be [{Bm}, T', {cfg.d_model}], got {tuple(enc.shape)}")
        tensors = dict(zip(names, params))
        for k, t in tensors.items():
            capi.require_fp32(f"parameter {k}", t, dev)
        d_ff = model.decoders[idx].layers[0].linear1.out_features
        V = model.linears_2[idx].out_features
        n_layers = len(model.decoders[idx].layers)
        with torch.cuda.device(dev):
            ps, keep = model._decoder_struct(idx, tensors, with_pe=True)
            nbytes = lib.eec_decoder_train_workspace_bytes(cfg.d_model, cfg.n_heads, d_ff, V, n_layers, Bm, S, Tq)
            if nbytes == 0:
                raise ValueError("unsupported geometry for the decoder's training step")
            ws, ws_ptr = aligned_ws(nbytes, dev)
            out = torch.empty((Bm, S, V), dtype=torch.float32, device=dev)
            geo = (cfg.d_model, cfg.n_heads, d_ff, V)
            launch("eec_decoder_train_forward", dev, C.byref(ps), *geo, int(model.trg_pad_idx), trg, enc, Bm, S, Tq,
                   int(model.decoder_passes), float(model.dropout), int(seed), int(idx), out, ws_ptr, nbytes)
        ctx.model, ctx.idx, ctx.names, ctx.seed, ctx.geo = model, idx, names, int(seed), geo
        ctx.ws, ctx.ws_ptr, ctx.nbytes, ctx.drop, ctx.passes = ws, ws_ptr, nbytes, float(model.dropout), int(model.decoder_passes)
        ctx.save_for_backward(trg, enc, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.ws is None:
            raise RuntimeError("the decoder's recorded forward was already consumed by a backward")
        model, idx, names = ctx.model, ctx.idx, ctx.names
        trg, enc, params = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
        dev = trg.device
        Bm, S = trg.shape
        Tq = enc.size(1)
        g = g.contiguous().float()
        with torch.cuda.device(dev):
            tensors = dict(zip(names, params))
            ps, keep = model._decoder_struct(idx, tensors, with_pe=True)
            grads = {k: torch.empty_like(v) for k, v in tensors.items()}
            gs, gkeep = model._decoder_struct(idx, grads, with_pe=False)
            g_enc = torch.empty_like(enc)
            launch("eec_decoder_train_backward", dev, C.byref(ps), C.byref(gs), *ctx.geo, trg, enc, Bm, S, Tq, ctx.passes, ctx.drop, ctx.seed,
                   int(idx), g, g_enc, ctx.ws_ptr, ctx.nbytes)
        ctx.ws = None
        need = ctx.needs_input_grad[6:]
        return (None, None, None, g_enc if ctx.needs_input_grad[3] else None, None, None,
                *[grads[k] if nd else None for k, nd in zip(names, need)])
