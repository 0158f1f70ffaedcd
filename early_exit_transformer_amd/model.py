"""Drop-in mirrors of the reference's model classes: ``Early_conformer`` / ``full_conformer``
(the reference's models/model/early_exit.py:565-634, :637-811, as called from train.py:148-178,37,54 and
inference.py:45-46,66), ``Splitformer`` (:227-364) and ``Early_zipformer`` (:117-224).

Same constructor keywords, ``forward`` signatures, return shapes and state_dict keys.  The encoder stack (subsampling,
positional encoding, length mask, E x L Conformer layers, per-exit Linear + log_softmax) is ONE call into libeec.so on the
caller's current HIP stream; there is no PyTorch implementation of it in this package and no CPU fallback.  The operators
around the classes live beside this module and are re-exported here: ``ctc`` (losses and decoding on log-probs),
``training`` (the training step behind autograd), ``decoding`` (the attention decoder's sessions and training step).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import capi
from .capi import launch, new_seed
from .capi import to_device as _to_device
from .conformer import Conformer
from .ctc import (CtcPrefixSession, ctc_align, ctc_beam_decode, ctc_lexicon_decode, ctc_prefix_session, encoder_lengths, exit_ctc_losses, exit_distill_losses,  # noqa: F401
                  exit_training_losses, greedy_ctc)
from .ctc import EXIT_CRITERIA, ExitStatistics, exit_route, exit_statistics, select_exits  # noqa: F401
from .ctc import MwerLists, ctc_hyp_logp, exit_mwer_losses, exit_mwer_training_losses, mwer_nbest  # noqa: F401
from .ctc import _exit_range, _exit_thresholds
from .lexicon import Lexicon, TokenTrie, apply_lex, load_dict  # noqa: F401
from .decoding import DecoderStepSession, _BatchSession, _DecoderTrainFn, _ExitSessions, beam_select  # noqa: F401
from .training import (_ExitHeadsFn, _named_tensors, _train_group, _train_head, _TrainStemFn, forward_train,  # noqa: F401
                       splitformer_sites, zipformer_sites)


class PositionalEncoding(nn.Module):
    """Holder of the sinusoid table buffer ``pe`` [max_len, 1, d_model] (reference
    models/embedding/positional_encoding.py:55-64).  The add happens inside the stem kernel."""

    def __init__(self, d_model: int, dropout: float, max_len: int):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        t = torch.arange(max_len).unsqueeze(1)
        w = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, 1, d_model)
        pe[:, 0, 0::2] = torch.sin(t * w)
        pe[:, 0, 1::2] = torch.cos(t * w)
        self.register_buffer("pe", pe)

    def forward(self, x: Tensor) -> Tensor:  # used by the AED decoder side only: [B, S, D]
        return self.dropout(x + self.pe[: x.size(1), 0].unsqueeze(0))


class Conv1dSubampling(nn.Module):
    """Parameter holder for the two Conv1d(k=3, s=2) of the stem (early_exit.py:24-48)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.sequential = nn.Sequential(
            nn.Conv1d(in_channels, out_channels, kernel_size=3, stride=2, padding=0),
            nn.Conv1d(out_channels, out_channels, kernel_size=3, stride=2, padding=0))


class AdaptiveOutput(NamedTuple):
    """What ``forward_adaptive`` returns: per utterance the log-probs [B, T', V] (and, asked for, the encoder output ``taps``
    [B, T', D]) of the exit it left at, that exit ``exit_of`` int32 [B] (0-based), and ``scores`` [E, B], the criterion's score at
    every exit the utterance reached (NaN elsewhere)."""
    logp: Tensor
    exit_of: Tensor
    scores: Tensor
    taps: Optional[Tensor]


class _HipEncoderMixin:
    """Holds the libeec encoder handle (``capi.EncoderHandle``: packed-weight cache and workspaces) and says, as data, where the
    class keeps what is packed into it."""

    _stem_keys = ("conv_subsample.sequential.0", "conv_subsample.sequential.1")  # the second is None for a one-convolution stem
    _head_key = "linears.{e}"  # exit e's Linear
    _pe_attr = "positional_encoder"
    # default operand mode: the one that keeps the north-star tolerance (|d log-prob| <= 1e-3, FLAT) on every committed fixture,
    # the peaky (trained-like) one included.  "f16f8" is the faster opt-in: 1e-3 on near-uniform outputs only
    precision = "f16x3"
    train_passes = 3     # training GEMMs: 3 = bf16 hi/lo split, three MFMA products (~fp32 results); 1 = plain bf16 operands

    def _hip_init(self, d_model, n_head, d_ff, dw_kernel, n_exits, n_layers, n_mels, vocab, max_len):
        self._cfg = capi.EecConfig(d_model, n_head, d_ff, dw_kernel, n_exits, n_layers, n_mels, vocab, max_len,
                                   capi.ARCH_CONFORMER)
        self._handle = capi.EncoderHandle(self._cfg)
        self._enc = None  # the handle itself, once a forward has packed it

    def __del__(self):
        tr = getattr(self, "_trainer", None)
        if tr is not None:
            try:
                capi.load().eec_trainer_destroy(tr)
            except Exception:
                pass

    # -- packing ------------------------------------------------------------
    def _param_tensors(self) -> List[Tensor]:
        return list(self.conv_subsample.parameters()) + list(self.conformer.parameters()) + \
            list(self.conformer.buffers()) + list(getattr(self, self._head_key.split(".")[0]).parameters()) + \
            [getattr(self, self._pe_attr).pe]

    def _params_struct(self, ptr):
        """EecParams of this model over ``ptr(state_dict name)``; returns (struct, keep-alive)."""
        return capi.params_struct(ptr, self._cfg.n_exits, self._cfg.layers_per_exit, "conformer", self._stem_keys, self._head_key,
                                  self._pe_attr + ".pe")

    def _packed(self, handle: capi.EncoderHandle, tensors: List[Tensor], device: torch.device, struct=None):
        """``handle`` on ``device`` with ``tensors`` packed (again, if one of them changed) from ``struct(ptr)``."""
        def repack(enc):
            sd = self.state_dict(keep_vars=True)
            self._pack(enc, lambda name: capi.require_fp32(f"parameter {name}", sd[name], device).data_ptr(), device,
                       struct or self._params_struct)
        return handle.ensure(device, tensors, repack)

    def _ensure_packed(self, device: torch.device) -> None:
        self._enc = self._packed(self._handle, self._param_tensors(), device)

    def _pack(self, enc, ptr, device, struct) -> None:
        params, keep = struct(ptr)
        launch("eec_encoder_pack", device, enc, C.byref(params))

    def _group(self, handle: capi.EncoderHandle, group: int, x: Tensor, key_len: Tensor) -> Tensor:
        """Group ``group`` of ``handle`` on x [B, T', D] fp32 contiguous, IN PLACE; key_len [B] int32 on the device."""
        B, Tq, _ = x.shape
        _, ws_ptr, ws_bytes = handle.workspace("group_", B, Tq, x.device)
        launch("eec_encoder_group_forward", x.device, handle.h, group, x, key_len, B, Tq, capi.PRECISIONS[self.precision], ws_ptr, ws_bytes)
        return x

    def _head(self, index: int, rows: Tensor, out: Tensor) -> Tensor:
        """Exit ``index``'s Linear + log_softmax of rows [..., D] into ``out`` [..., V]."""
        launch("eec_encoder_head_forward", rows.device, self._enc, index, rows, rows.numel() // rows.size(-1), out,
               capi.PRECISIONS[self.precision])
        return out

    # -- measurement hook -----------------------------------------------------
    def set_profiling(self, enable: bool, max_launches: int = 8192) -> None:
        if self._enc is None:
            raise RuntimeError("run one forward first (the encoder handle is created lazily)")
        capi.call("eec_encoder_set_profiling", self._enc, int(enable), max_launches)

    def read_profile(self) -> Dict[str, Tuple[float, int]]:
        """{kernel class: (total ms, launches)} of the launches recorded since set_profiling(True)."""
        n = len(capi.KERNEL_CLASSES)
        ms, cnt = (C.c_double * n)(), (C.c_longlong * n)()
        capi.call("eec_encoder_profile_read", self._enc, ms, cnt, n)
        return {k: (ms[i], cnt[i]) for i, k in enumerate(capi.KERNEL_CLASSES)}

    # -- data-parallel training (BASELINE.json configs[3]) -----------------------
    def enable_data_parallel(self, b_local: int, group=None, min_bucket_bytes: int = 4 << 20) -> None:
        """One process per GPU, every rank holding ``b_local`` utterances of the global batch: from now on the training
        backward writes the gradients into flat per-exit-group buckets (``parallel.GradBuckets``: ``p.grad`` become views
        of them) and, as ``eec_train_backward_ex`` reports each finished exit group, starts that bucket's all-reduce
        (weighted b_local / global batch: the loss is a batch mean, train.py:60-65) on the backend's stream, under the
        backward of the earlier groups.  Call ``sync_gradients()`` after ``loss.backward()`` and before clipping / the
        optimizer step.  Collective at set-up: one exchange of the shard sizes.  A no-op without an initialised process
        group of more than one rank (the buckets are still used, so the single-GPU step runs the same code)."""
        from . import parallel
        dev = next(self.parameters()).device
        named = [(n, p) for n, p in self.named_parameters()]
        self._dp = {"buckets": parallel.GradBuckets(named, self._cfg.n_exits, min_bucket_bytes=min_bucket_bytes),
                    "weight": parallel.shard_weight(b_local, dev, group), "group": group, "reduced": set(),
                    "active": parallel._active(group)}

    def sync_gradients(self) -> int:
        """Join the gradient collectives the last backward started from its progress callback and reduce EVERY other bucket
        now: buckets whose gradients the backward could not write into the flat views (gradients accumulated into existing
        ``.grad`` tensors, autograd-owned decoder gradients) and every bucket of a model whose backward does not report
        into the buckets at all (Splitformer / Early_zipformer / the heads-only step: their autograd functions know nothing
        of ``_dp``).  Call exactly once per backward, before clipping / the optimizer step.  Returns the number of
        collectives joined."""
        dp = getattr(self, "_dp", None)
        if dp is None or not dp["active"]:
            return 0
        buckets, early = dp["buckets"], dp["reduced"]
        for i in range(len(buckets.buckets)):
            if i not in early:
                buckets.allreduce_bucket(i, dp["weight"], dp["group"])
        n = buckets.wait()
        # a bucket reduced from the callback was reduced BEFORE autograd installed its views as p.grad: if autograd kept a
        # copy instead (a tensor hook, another live reference to the view), that copy was taken from an unreduced buffer
        for i in early:
            buckets.adopt_views(i)
        dp["reduced"] = set()
        return n

    def _run_encoder(self, src: Tensor, lengths: Tensor, want_out: bool = True, want_taps: bool = False,
                     stop_after: int = -1, want_x: bool = False, n_groups: Optional[int] = None, frozen: bool = False):
        """``n_groups`` (1 .. E): stop after that many exit groups (eec_encoder_forward_prefix, production launch plan);
        ``out`` / ``taps`` then hold only the exits that were run.  ``frozen``: the caller trains on top of this pass and means
        the encoder to run without autograd, in eval semantics, although the module is in train mode."""
        if not src.is_cuda:
            raise RuntimeError("the MI355X encoder runs on a HIP device only; move the model and inputs to "
                               "'cuda' (there is no CPU fallback -- the CPU reference lives in oracle/).")
        if self.training and torch.is_grad_enabled() and not frozen:
            raise NotImplementedError("this class has no training step on the HIP path (Early_conformer and full_conformer do); "
                                      "call under model.eval() / torch.no_grad()")
        if src.dim() != 3 or src.size(1) != self._cfg.n_mels:
            raise ValueError(f"src must be [B, {self._cfg.n_mels}, T], got {tuple(src.shape)}")
        dev = src.device
        with torch.cuda.device(dev):
            self._ensure_packed(dev)
            lib = capi.load()
            B, _, T = src.shape
            Tq = lib.eec_out_frames(T)
            if Tq <= 0:
                raise ValueError("T too short for two k=3 s=2 convolutions")
            src = src.contiguous().float()
            len_dev = _to_device(lengths, dev)
            E, D, V = self._cfg.n_exits, self._cfg.d_model, self._cfg.vocab
            if n_groups is not None:
                if stop_after >= 0:
                    raise ValueError("n_groups and stop_after are exclusive")
                if not 1 <= int(n_groups) <= E:
                    raise ValueError(f"n_groups must be in 1 .. {E}")
                E = int(n_groups)
            out = torch.empty((E, B, Tq, V), dtype=torch.float32, device=dev) if want_out else None
            taps = torch.empty((E, B, Tq, D), dtype=torch.float32, device=dev) if want_taps else None
            xdbg = torch.empty((B, Tq, D), dtype=torch.float32, device=dev) if want_x else None
            _, ws_ptr, ws_bytes = self._handle.workspace("", B, T, dev)
            if n_groups is not None:
                launch("eec_encoder_forward_prefix", dev, self._enc, src, len_dev, B, T, capi.PRECISIONS[self.precision], E, out, taps, xdbg,
                       ws_ptr, ws_bytes)
            else:
                launch("eec_encoder_forward", dev, self._enc, src, len_dev, B, T, capi.PRECISIONS[self.precision], out, taps, ws_ptr, ws_bytes,
                       stop_after, xdbg)
            # src/len_dev must outlive the asynchronous launches on this stream
            src.record_stream(torch.cuda.current_stream(dev))
            len_dev.record_stream(torch.cuda.current_stream(dev))
        return out, taps, xdbg

    _forward_train = forward_train  # the whole-encoder training step (Early_conformer, full_conformer)

    # -- adaptive inference ---------------------------------------------------
    @torch.no_grad()
    def forward_adaptive(self, src: Tensor, lengths: Tensor, threshold=None, criterion: str = "entropy", min_exit: int = 0,
                         max_exit: Optional[int] = None, exit_of: Optional[Tensor] = None, compact: bool = True,
                         want_taps: bool = False) -> "AdaptiveOutput":
        """Every utterance leaves the encoder at the shallowest exit that is good enough for it (extension; the reference's
        forward always runs every group): ``AdaptiveOutput(logp [B, T', V], exit_of int32 [B], scores [E, B], taps [B, T', D] or
        None)``.  ``logp[b]`` / ``taps[b]`` are the log-probs / encoder output of exit ``exit_of[b]`` (0-based) -- what ``forward``
        computes for that exit and utterance: the walk runs the stem once and then, exit by exit, the same group and head launches
        on the utterances still in flight, ``exit_statistics`` of that one exit and one ``exit_route``.
        ``criterion``: ``"entropy"`` (an utterance leaves when its average frame entropy is BELOW ``threshold``), ``"confidence"``
        (average frame confidence ABOVE) or ``"greedy_logp"`` (``greedy_logp / max(frames, 1)`` ABOVE), over the encoder's own
        frame counts ``encoder_lengths(lengths, T')``.  ``threshold``: a float or one per exit.  Exits below ``min_exit`` let
        nobody leave, ``max_exit`` (default E - 1) takes everyone left.  ``scores[e, b]`` is the score exit e gave utterance b,
        NaN for an exit the utterance never reached.
        ``exit_of`` (int [B], instead of ``threshold``): the routing is prescribed -- the "oracle exit" analysis -- and the
        scores are still recorded; ``min_exit`` / ``max_exit`` are not looked at.
        ``compact``: the rows and key lengths of the utterances that stay are gathered and the next group runs on them alone
        (T' is never trimmed: that would move the depthwise convolution's zero padding); False: the whole batch runs every
        group and only the early stop saves work.  One 8-byte device-to-host read (the route's counts) per exit evaluated but
        the last; gathers and scatters are torch index ops.  Inference only: call under ``eval()``."""
        if self._cfg.arch != capi.ARCH_CONFORMER:
            raise NotImplementedError(f"{type(self).__name__} has no adaptive forward")
        if self.training:
            raise RuntimeError("forward_adaptive is an inference pass: call it under model.eval()")
        if (threshold is None) == (exit_of is None):
            raise ValueError("forward_adaptive: give exactly one of threshold= and exit_of=")
        if criterion not in EXIT_CRITERIA:
            raise ValueError(f"forward_adaptive: criterion must be one of {sorted(EXIT_CRITERIA)}, got {criterion!r}")
        E, V = self._cfg.n_exits, self._cfg.vocab
        higher = EXIT_CRITERIA[criterion]
        if exit_of is None:
            lo, hi = _exit_range("forward_adaptive", E, min_exit, max_exit)
            thr = _exit_thresholds("forward_adaptive", threshold, E)
        else:
            planned = torch.as_tensor(exit_of).reshape(-1).cpu().to(torch.int64)
            if planned.numel() != src.size(0) or planned.numel() == 0 or int(planned.min()) < 0 or int(planned.max()) >= E:
                raise ValueError(f"forward_adaptive: exit_of must hold one exit in 0 .. {E - 1} per utterance")
            lo, hi = 0, int(planned.max())
        x = self._run_encoder(src, lengths, want_out=False, stop_after=0, want_x=True)[2]  # the stem; validates src, packs
        dev = x.device
        B, Tq, D = x.shape
        with torch.cuda.device(dev):
            key_len = encoder_lengths(_to_device(lengths, dev), Tq)
            if key_len.numel() != B:
                raise ValueError(f"forward_adaptive: lengths must have {B} entries, got {key_len.numel()}")
            planned = None if exit_of is None else planned.to(device=dev, dtype=torch.int32)
            logp = torch.empty((B, Tq, V), dtype=torch.float32, device=dev)
            taps = torch.empty((B, Tq, D), dtype=torch.float32, device=dev) if want_taps else None
            scores = torch.full((E, B), float("nan"), dtype=torch.float32, device=dev)
            chosen = torch.full((B,), hi, dtype=torch.int32, device=dev)
            idx = torch.arange(B, device=dev)              # original batch position of every row of x
            alive = torch.ones(B, dtype=torch.bool, device=dev)  # compact=False: the rows of x still in flight
            n_alive = B
            for e in range(hi + 1):
                self._group(self._handle, e, x, key_len)
                lp = self._head(e, x, torch.empty((x.size(0), Tq, V), dtype=torch.float32, device=dev))
                st = exit_statistics(lp.unsqueeze(0), key_len)
                score = {"entropy": st.entropy, "confidence": st.confidence}[criterion][0] if criterion != "greedy_logp" else \
                    st.greedy_logp[0] / key_len.clamp(min=1).to(torch.float32)
                if not compact:
                    score = torch.where(alive, score, torch.full_like(score, float("nan")))  # a NaN never leaves again
                scores[e].index_copy_(0, idx, score)
                if e == hi:  # takes everyone left: nothing to route, nothing to read
                    rows = alive.view(-1, 1, 1)
                    logp.index_copy_(0, idx, lp if compact else torch.where(rows, lp, logp))
                    if want_taps:
                        taps.index_copy_(0, idx, x if compact else torch.where(rows, x, taps))
                    break
                if e < lo:
                    continue
                if planned is None:
                    stay, leave, counts = exit_route(score, thr[e], higher)
                else:
                    due = planned[idx] == e
                    stay, leave, counts = exit_route((due if compact else due & alive).to(torch.float32), 0.5, True)
                n_stay, n_leave = counts.tolist()  # the one host read of this exit
                if n_leave:
                    rows = leave[:n_leave].long()
                    where = idx[rows]
                    logp[where] = lp[rows]
                    if want_taps:
                        taps[where] = x[rows]
                    chosen[where] = e
                    n_alive -= n_leave
                    if n_alive == 0:
                        break
                    if compact:
                        rows = stay[:n_stay].long()
                        x, key_len, idx = x[rows], key_len[rows], idx[rows]
                    else:
                        alive[rows] = False
        return AdaptiveOutput(logp, chosen, scores, taps)


class Early_conformer(_HipEncoderMixin, nn.Module):
    """CTC early-exit Conformer; ``forward(src[B,n_mels,T], lengths[B]) -> [E,B,T',V]`` log-probs."""

    def __init__(self, src_pad_idx, n_enc_exits, enc_voc_size, dec_voc_size, d_model, n_head, max_len,
                 d_feed_forward, n_enc_layers, features_length, drop_prob, depthwise_kernel_size, device=None):
        nn.Module.__init__(self)
        self.input_dim, self.num_heads, self.ffn_dim = d_model, n_head, d_feed_forward
        self.num_layers, self.depthwise_conv_kernel_size = n_enc_layers, depthwise_kernel_size
        self.n_enc_exits, self.dropout, self.device, self.src_pad_idx = n_enc_exits, drop_prob, device, src_pad_idx
        self.conv_subsample = Conv1dSubampling(features_length, d_model)
        self.positional_encoder = PositionalEncoding(d_model, drop_prob, max_len)
        self.linears = nn.ModuleList([nn.Linear(d_model, dec_voc_size) for _ in range(n_enc_exits)])
        self.conformer = nn.ModuleList([
            Conformer(input_dim=d_model, num_heads=n_head, ffn_dim=d_feed_forward, num_layers=n_enc_layers,
                      depthwise_conv_kernel_size=depthwise_kernel_size, dropout=drop_prob)
            for _ in range(n_enc_exits)])
        self._hip_init(d_model, n_head, d_feed_forward, depthwise_kernel_size, n_enc_exits, n_enc_layers,
                       features_length, dec_voc_size, max_len)

    def forward(self, src: Tensor, lengths: Tensor) -> Tensor:
        if self.training and type(self) is Early_conformer:
            # train-mode semantics (batch-statistics BatchNorm, dropout, running-statistics update) whenever the module is in
            # train mode -- with or without autograd, whatever requires_grad says, as the reference.  The one exception is an
            # explicit opt-in: ``model.frozen_encoder_eval = True`` runs a FROZEN encoder (only linears.* trainable) on the fused
            # inference path in eval semantics and trains the heads on its taps (cheaper; not what the reference computes).
            frozen = not any(p.requires_grad for n, p in self.named_parameters() if not n.startswith("linears."))
            if torch.is_grad_enabled() and frozen and getattr(self, "frozen_encoder_eval", False):
                return self._forward_heads_trainable(src, lengths)
            return self._forward_train(src, lengths)
        if self.training and torch.is_grad_enabled():
            return self._forward_heads_trainable(src, lengths)
        return self._run_encoder(src, lengths)[0]

    def _forward_heads_trainable(self, src: Tensor, lengths: Tensor) -> Tensor:
        """First slice of the training path (train.py:53-70): the exit heads ``linears.*`` are trainable on a FROZEN
        encoder.  The encoder stack runs on the HIP path without autograd, in eval semantics (running BatchNorm
        statistics, no dropout) whatever ``self.training`` says; the heads are an autograd function over its taps, so
        ``exit_ctc_losses(model(src, lengths), ...).sum().backward()`` fills ``linears.*.grad``.  With a trainable parameter
        anywhere else ``Early_conformer.forward`` takes the full training step instead (``_forward_train``); the classes that
        reuse this method (Splitformer, Early_zipformer, full_conformer) still raise for those."""
        trainable = [n for n, p in self.named_parameters() if p.requires_grad and not n.startswith("linears.")]
        if trainable:
            raise NotImplementedError("this class trains its exit heads (linears.*) only: freeze the encoder "
                                      f"(requires_grad_(False)); trainable now: {trainable[:3]}{' ...' if len(trainable) > 3 else ''}")
        taps = self._run_encoder(src, lengths, want_out=False, want_taps=True, n_groups=self._cfg.n_exits, frozen=True)[1]
        wb = [l.weight for l in self.linears] + [l.bias for l in self.linears]
        return _ExitHeadsFn.apply(self, taps, *wb)

    def forward_exits(self, src: Tensor, lengths: Tensor, n_exits: int) -> Tensor:
        """Early exit (extension; the reference's forward always runs every group): log-probs of the first
        ``n_exits`` exits only, [n_exits, B, T', V], at n_exits / E of the cost of ``forward``."""
        return self._run_encoder(src, lengths, n_groups=n_exits)[0]

    def greedy_decode(self, enc_out: Tensor, blank: int = 0, lengths: Optional[Tensor] = None) -> List[List[List[int]]]:
        """Batched GreedyCTCDecoder (util/beam_infer.py:9-24) over every exit and utterance.  ``lengths`` [B], in encoder frames
        (``encoder_lengths``; None: T' for every utterance), applies to every exit: frames at or past it are not transcribed."""
        E, B, Tq, V = enc_out.shape
        if lengths is not None:
            if lengths.numel() != B:
                raise ValueError(f"greedy_decode: lengths must have {B} entries, got {lengths.numel()}")
            lengths = lengths.reshape(B).repeat(E)  # sequence e * B + b
        tokens, counts = greedy_ctc(enc_out.reshape(E * B, Tq, V), blank, em_len=lengths)
        tokens, counts = tokens.cpu(), counts.cpu()
        return [[tokens[e * B + b, : counts[e * B + b]].tolist() for b in range(B)] for e in range(E)]


class _TimeResample(nn.Module):
    """Parameterless stand-ins that keep the reference's module tree (Downsampling / Upsampling, early_exit.py:95-114)."""

    def __init__(self, factor: int):
        super().__init__()
        self.factor = factor


class Splitformer(Early_conformer):
    """Drop-in for the reference's ``Splitformer`` (early_exit.py:227-364): Early_conformer plus,
    at the first and the last exit, a one-layer Conformer on the 2x time-down-sampled input of that exit group, added
    back (nearest-neighbour up-sampled) before the head.  Same constructor kwargs, ``forward(src, lengths)`` and
    state_dict names.  Every Conformer group and every head runs in libeec (eec_encoder_group_forward /
    eec_encoder_head_forward, the production chain-kernel plan); the strided slice, the repeat and the add that glue the
    branch in are three torch ops on [B, T', 256] tensors.  Reference quirks kept: the branch's key lengths are
    ``clamp((mel_lengths + pad) / 2, max=T'/2)`` (:324-331) and ``index // (n_enc_exits - 1)`` picks the branch."""

    factor = 2

    def __init__(self, src_pad_idx, n_enc_exits, enc_voc_size, dec_voc_size, d_model, n_head, max_len,
                 d_feed_forward, n_enc_layers, features_length, drop_prob, depthwise_kernel_size, device=None):
        if n_enc_exits < 2:
            raise ValueError("Splitformer needs n_enc_exits >= 2 (the reference divides by n_enc_exits - 1)")
        super().__init__(src_pad_idx, n_enc_exits, enc_voc_size, dec_voc_size, d_model, n_head, max_len,
                         d_feed_forward, n_enc_layers, features_length, drop_prob, depthwise_kernel_size, device)
        self.downsampling = nn.ModuleList([_TimeResample(self.factor) for _ in range(2)])
        self.upsampling = nn.ModuleList([_TimeResample(self.factor) for _ in range(2)])
        self.conformer_parallel = nn.ModuleList([
            Conformer(input_dim=d_model, num_heads=n_head, ffn_dim=d_feed_forward, num_layers=1,
                      depthwise_conv_kernel_size=depthwise_kernel_size, dropout=drop_prob) for _ in range(2)])
        # second libeec handle: the two one-layer branch groups, packed without stem and heads
        self._branch = capi.EncoderHandle(capi.EecConfig(d_model, n_head, d_feed_forward, depthwise_kernel_size, 2, 1, features_length,
                                                         dec_voc_size, max_len, capi.ARCH_CONFORMER))

    def forward_adaptive(self, *args, **kwargs):
        raise NotImplementedError("Splitformer has no adaptive forward: its walk adds the down-sampled branches at the first and last exit")

    def _walk(self, x: Tensor, lengths: Tensor, group, head, in_place: bool) -> list:
        """The reference's topology (early_exit.py:299-364) from the stem's output x [B, T', D] on, over the two operations that
        differ between the modes: ``group(which, index, x, key_len) -> x`` runs Conformer group ``index`` of ``self.<which>``,
        ``head(index, x)`` exit ``index``'s head; returns the heads' results.  ``in_place``: ``group`` overwrites its input (the
        inference entry does; the autograd functions return fresh tensors).  The strided slice, the repeat and the add that glue
        a branch in are the same torch ops in both modes."""
        B, Tq, D = x.shape
        E = self._cfg.n_exits
        mel_len = _to_device(lengths, x.device)
        base = torch.clamp(mel_len / 4, max=Tq).to(torch.int32)
        outs = []
        for index in range(E):
            branch = index in (0, E - 1)
            side = x.clone() if branch and in_place else x  # the group's INPUT feeds the branch
            x = group("conformer", index, x, base)
            if branch:
                pad = (-Tq) % self.factor
                if pad:
                    side = torch.cat((side, side.new_zeros(B, pad, D)), dim=1)
                side = side[:, :: self.factor, :].contiguous()
                side_len = torch.clamp((mel_len + pad) / self.factor, max=side.size(1)).to(torch.int32)
                side = group("conformer_parallel", index // (E - 1), side, side_len)
                x = x + torch.repeat_interleave(side, self.factor, dim=1)[:, :Tq, :]
            outs.append(head(index, x))
        return outs

    def forward(self, src: Tensor, lengths: Tensor) -> Tensor:
        E = self._cfg.n_exits
        if self.training:
            # train.py:180-208 (--model_type splitformer) in train mode: every module on the HIP training kernels behind autograd
            # functions (stem, Conformer groups -- the E main ones and the two down-sampled branches --, heads)
            if not src.is_cuda:
                raise RuntimeError("the MI355X training step runs on a HIP device only (there is no CPU fallback)")
            seed = new_seed()
            sites = splitformer_sites(E, self._cfg.layers_per_exit)
            conv = self.conv_subsample.sequential
            x = _TrainStemFn.apply(self, src.contiguous().float(), self.positional_encoder.pe, seed, sites["stem"], conv[0].weight,
                                   conv[0].bias, conv[1].weight, conv[1].bias)

            def group(which, i, t, key_len):
                site = sites["groups" if which == "conformer" else "branches"][i]
                return _train_group(self, getattr(self, which)[i], t, key_len, seed, site)
            return torch.stack(self._walk(x, lengths, group, lambda i, t: _train_head(self, self.linears[i], t), in_place=False))
        # stem (+ PE) through the monolithic entry's first sub-step; also validates src and packs the main handle
        x = self._run_encoder(src, lengths, want_out=False, stop_after=0, want_x=True)[2]
        dev = x.device
        with torch.cuda.device(dev):
            handles = {"conformer": self._handle, "conformer_parallel": self._branch}
            self._packed(self._branch, list(self.conformer_parallel.parameters()) + list(self.conformer_parallel.buffers()), dev,
                         lambda ptr: capi.params_struct(ptr, 2, 1, "conformer_parallel"))
            out = torch.empty((E, *x.shape[:2], self._cfg.vocab), dtype=torch.float32, device=dev)
            self._walk(x, lengths, lambda which, i, t, key_len: self._group(handles[which], i, t, key_len),
                       lambda i, t: self._head(i, t, out[i]), in_place=True)
        return out


class Conv1dSubampling_Zipformer(nn.Module):
    """Parameter holder for the one-convolution stem (early_exit.py:80-95)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=3, stride=2, padding=0)


class Early_zipformer(_HipEncoderMixin, nn.Module):
    """Drop-in for the reference's ``Early_zipformer`` (early_exit.py:117-224): one-convolution stem,
    two Conformer groups at full frame rate, five stacks of groups at 1/2, 1/4, 1/8, 1/4, 1/2 rate with a skip around
    each stack, one head on every second frame -> [1, B, ceil(T1/2), V].  Same kwargs, ``forward(src, lengths)`` and
    state_dict names; ``n_enc_exits`` is the number of Conformer groups and must be >= 19 (the forward indexes groups
    0 .. 18).  Stem, every group and the head run in libeec; pad / stride / repeat / add are torch ops."""

    factors = (2, 4, 8, 4, 2)
    stack = (2, 4, 5, 4, 2)
    _stem_keys = ("conv_subsample.conv", None)
    _head_key = "linear"  # one head, registered under every exit index

    def __init__(self, src_pad_idx, n_enc_exits, enc_voc_size, dec_voc_size, d_model, n_head, max_len,
                 d_feed_forward, n_enc_layers, features_length, drop_prob, depthwise_kernel_size, device=None):
        nn.Module.__init__(self)
        if n_enc_exits < 2 + sum(self.stack):
            raise ValueError(f"Early_zipformer indexes Conformer groups 0 .. {1 + sum(self.stack)}: n_enc_exits must be >= "
                             f"{2 + sum(self.stack)}")
        self.n_enc_exits, self.dropout, self.device, self.src_pad_idx = n_enc_exits, drop_prob, device, src_pad_idx
        self.downsampling = nn.ModuleList([_TimeResample(f) for f in self.factors])
        self.downsampling_output = _TimeResample(2)
        self.upsampling = nn.ModuleList([_TimeResample(f) for f in self.factors])
        self.conv_subsample = Conv1dSubampling_Zipformer(features_length, d_model)
        self.positional_encoder = PositionalEncoding(d_model, drop_prob, max_len)
        self.linear = nn.Linear(d_model, dec_voc_size)
        self.conformer = nn.ModuleList([
            Conformer(input_dim=d_model, num_heads=n_head, ffn_dim=d_feed_forward, num_layers=n_enc_layers,
                      depthwise_conv_kernel_size=depthwise_kernel_size, dropout=drop_prob)
            for _ in range(n_enc_exits)])
        self._hip_init(d_model, n_head, d_feed_forward, depthwise_kernel_size, n_enc_exits, n_enc_layers,
                       features_length, dec_voc_size, max_len)

    def forward_adaptive(self, *args, **kwargs):
        raise NotImplementedError("Early_zipformer has no adaptive forward: it has one exit, after the last stack")

    def _walk(self, enc: Tensor, lengths: Tensor, group, head):
        """The reference's topology (early_exit.py:174-224) from the stem's output enc [B, T1, D] on, over the two operations that
        differ between the modes: ``group(index, x, key_len) -> x`` (in place or not: every input that is needed again is a fresh
        tensor here) and ``head(rows)``, whose result is returned.  pad / stride / repeat / add are the same torch ops in both."""
        B, T1, D = enc.shape
        mel_len = _to_device(lengths, enc.device)
        base = torch.clamp(mel_len / 2, max=T1).to(torch.int32)
        enc = group(0, enc, base)
        enc = group(1, enc, base)
        first = 2
        for factor, count in zip(self.factors, self.stack):
            skip = enc
            n = enc.size(1)
            pad = (-n) % factor
            if pad:
                enc = torch.cat((enc, enc.new_zeros(B, pad, D)), dim=1)
            enc = enc[:, ::factor, :].contiguous()  # a fresh tensor: the groups below may run in place
            key_len = torch.clamp((mel_len + pad) / factor, max=enc.size(1)).to(torch.int32)
            for g in range(first, first + count):
                enc = group(g, enc, key_len)
            first += count
            enc = torch.repeat_interleave(enc, factor, dim=1)[:, :n, :] + skip
        return head(enc[:, ::2, :].contiguous())

    def forward(self, src: Tensor, lengths: Tensor) -> Tensor:
        if not src.is_cuda:
            raise RuntimeError("the MI355X encoder runs on a HIP device only (there is no CPU fallback -- the CPU "
                               "reference lives in oracle/).")
        if src.dim() != 3 or src.size(1) != self._cfg.n_mels or src.size(2) < 3:
            raise ValueError(f"src must be [B, {self._cfg.n_mels}, T >= 3], got {tuple(src.shape)}")
        dev = src.device
        src = src.contiguous().float()
        if self.training:
            # train.py:180-208 (--model_type zipformer) in train mode: one-convolution stem, the 19 Conformer groups at five frame
            # rates and the head on the HIP training kernels behind autograd functions
            seed = new_seed()
            sites = zipformer_sites(len(self.conformer), self._cfg.layers_per_exit)
            conv = self.conv_subsample.conv
            enc = _TrainStemFn.apply(self, src, self.positional_encoder.pe, seed, sites["stem"], conv.weight, conv.bias, None, None)
            return self._walk(enc, lengths, lambda g, x, key_len: _train_group(self, self.conformer[g], x, key_len, seed, sites["groups"][g]),
                              lambda rows: _train_head(self, self.linear, rows).unsqueeze(0))
        with torch.cuda.device(dev):
            self._ensure_packed(dev)
            B, _, T = src.shape
            enc = torch.empty((B, (T - 3) // 2 + 1, self._cfg.d_model), dtype=torch.float32, device=dev)
            launch("eec_encoder_stem1_forward", dev, self._enc, src, B, T, enc)
            src.record_stream(torch.cuda.current_stream(dev))

            def head(rows):
                return self._head(0, rows, torch.empty((1, B, rows.size(1), self._cfg.vocab), dtype=torch.float32, device=dev))
            return self._walk(enc, lengths, lambda g, x, key_len: self._group(self._handle, g, x, key_len), head)


class full_conformer(_HipEncoderMixin, nn.Module):
    """AED model: HIP encoder + the attention decoder, both on the hand-written path: inference through csrc/decoder.hip /
    decoder_step.hip, training (forward in train mode + backward, train.py:36-52) through csrc/decoder_train.hip
    behind an autograd function.  The ``nn.TransformerDecoder`` modules only hold the parameters (state_dict contract)."""

    _head_key = "linears_1.{e}"
    _pe_attr = "positional_encoder_1"

    def __init__(self, trg_pad_idx, n_enc_exits, enc_voc_size, dec_voc_size, d_model, n_head, max_len,
                 d_feed_forward, n_enc_layers, n_dec_layers, features_length, drop_prob, depthwise_kernel_size,
                 device=None):
        nn.Module.__init__(self)
        self.input_dim, self.num_heads, self.ffn_dim = d_model, n_head, d_feed_forward
        self.num_layers, self.depthwise_conv_kernel_size = n_enc_layers, depthwise_kernel_size
        self.n_enc_exits, self.dropout, self.n_dec_layers = n_enc_exits, drop_prob, n_dec_layers
        self.device, self.trg_pad_idx = device, trg_pad_idx
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-5)
        self.emb = nn.Embedding(dec_voc_size, d_model)
        self.conv_subsample = Conv1dSubampling(features_length, d_model)
        self.linears_1 = nn.ModuleList([nn.Linear(d_model, dec_voc_size) for _ in range(n_enc_exits)])
        self.linears_2 = nn.ModuleList([nn.Linear(d_model, dec_voc_size) for _ in range(n_enc_exits)])
        self.positional_encoder_1 = PositionalEncoding(d_model, drop_prob, max_len)
        self.positional_encoder_2 = PositionalEncoding(d_model, drop_prob, max_len)
        self.conformer = nn.ModuleList([
            Conformer(input_dim=d_model, num_heads=n_head, ffn_dim=d_feed_forward, num_layers=n_enc_layers,
                      depthwise_conv_kernel_size=depthwise_kernel_size, dropout=drop_prob)
            for _ in range(n_enc_exits)])
        self.decoders = nn.ModuleList([
            nn.TransformerDecoder(
                nn.TransformerDecoderLayer(d_model=d_model, nhead=n_head, dim_feedforward=d_feed_forward,
                                           dropout=drop_prob, batch_first=True, norm_first=True),
                n_dec_layers, self.layer_norm)
            for _ in range(n_enc_exits)])
        self._hip_init(d_model, n_head, d_feed_forward, depthwise_kernel_size, n_enc_exits, n_enc_layers,
                       features_length, dec_voc_size, max_len)

    def _encoder_(self, src: Tensor, lengths: Tensor, layer_n: int) -> Tensor:
        """Pre-head activations after ``layer_n`` exit groups, [B, T', D] (early_exit.py:719-737)."""
        return self._run_encoder(src, lengths, want_out=False, want_x=True, n_groups=self._exit(layer_n))[2]

    def _exit(self, layer_n) -> int:
        """The exit ``layer_n`` stands for, 1 .. n_exits: any other value runs all groups, as the reference's loop does."""
        n = int(layer_n)
        return n if 1 <= n <= self._cfg.n_exits else self._cfg.n_exits

    decoder_passes = 3  # the HIP decoder's GEMM operands: 3 = bf16 hi/lo split (~1e-5 of fp32), 1 = plain bf16

    def _decode_one(self, trg: Tensor, enc: Tensor, idx: int, log_softmax: bool = False, seed: Optional[int] = None) -> Tensor:
        if not trg.is_cuda:
            raise RuntimeError("the MI355X decoder runs on a HIP device only (there is no CPU fallback)")
        if not self.training:
            return self._hip_decoder(trg, enc, idx, log_softmax)  # inference: csrc/decoder.hip
        # train mode (train.py:36-52), with or without autograd -- the reference's modules apply their dropout in train mode
        # whatever the grad mode: forward (and backward) on the HIP training kernels (csrc/decoder_train.hip)
        if seed is None:
            seed = new_seed()
        named = self._decoder_named_params(idx)
        out = _DecoderTrainFn.apply(self, idx, trg.to(torch.int64).contiguous(), enc.contiguous().float(), seed,
                                    tuple(n for n, _ in named), *[p for _, p in named])
        return torch.log_softmax(out, dim=2) if log_softmax else out

    def _decoder_named_params(self, idx: int):
        """(name, parameter) of everything exit ``idx``'s decoder reads, under the model's state_dict names (the decoders'
        final norm is the ONE shared ``layer_norm``, early_exit.py:666,701-717)."""
        named = [("emb.weight", self.emb.weight), ("layer_norm.weight", self.layer_norm.weight), ("layer_norm.bias", self.layer_norm.bias),
                 (f"linears_2.{idx}.weight", self.linears_2[idx].weight), (f"linears_2.{idx}.bias", self.linears_2[idx].bias)]
        for l, layer in enumerate(self.decoders[idx].layers):
            sd = dict(layer.named_parameters())
            named += [(f"decoders.{idx}.layers.{l}.{suffix}", sd[suffix]) for suffix in capi.DECODER_LAYER_KEYS.values()]
        return named

    def _decoder_struct(self, idx: int, tensors: Dict[str, Tensor], with_pe: bool):
        """eec_decoder_params over ``tensors`` (name -> tensor: the parameters themselves, or gradient buffers of their shapes)."""
        n_layers = len(self.decoders[idx].layers)
        layers = (capi.EecDecoderLayerParams * n_layers)()
        for l in range(n_layers):
            for field, suffix in capi.DECODER_LAYER_KEYS.items():
                setattr(layers[l], field, tensors[f"decoders.{idx}.layers.{l}.{suffix}"].data_ptr())
        pe = self.positional_encoder_2.pe
        ps = capi.EecDecoderParams(tensors["emb.weight"].data_ptr(), pe.data_ptr() if with_pe else None, layers, n_layers, pe.size(0),
                                   tensors["layer_norm.weight"].data_ptr(), tensors["layer_norm.bias"].data_ptr(),
                                   tensors[f"linears_2.{idx}.weight"].data_ptr(), tensors[f"linears_2.{idx}.bias"].data_ptr())
        return ps, layers

    def _decoder_params(self, idx: int, dev):
        """The C-ABI view (eec_decoder_params) of exit ``idx``'s decoder: pointers into the module's own parameters, rebuilt
        when any of them moved."""
        dec = self.decoders[idx]
        tensors = [self.emb.weight, self.positional_encoder_2.pe, self.layer_norm.weight, self.layer_norm.bias,
                   self.linears_2[idx].weight, self.linears_2[idx].bias] + list(dec.layers.parameters())
        key = (dev, tuple(t.data_ptr() for t in tensors))
        cache = self.__dict__.setdefault("_dec_cache", {})
        ent = cache.get(idx)
        if ent is None or ent[0] != key:
            for t in tensors:
                capi.require_fp32("a decoder parameter", t, dev)
            ent = (key, *self._decoder_struct(idx, dict(self._decoder_named_params(idx)), with_pe=True))
            cache[idx] = ent
        return ent[1], dec.layers[0].linear1.out_features, self.linears_2[idx].out_features

    def _hip_decoder(self, trg: Tensor, enc: Tensor, idx: int, log_softmax: bool) -> Tensor:
        """``linears_2[idx](decoders[idx](positional_encoder_2(emb(trg)), enc, causal + padding masks))`` in eval semantics
        through eec_decoder_forward; trg int64 [Bm, S], enc fp32 [Bm, T', D] -> [Bm, S, V] logits or log-probs."""
        lib = capi.load()
        dev = trg.device
        cfg = self._cfg
        Bm, S = trg.shape
        Tq = enc.size(1)
        if enc.size(0) != Bm or enc.size(2) != cfg.d_model:
            raise ValueError(f"enc must be [{Bm}, T', {cfg.d_model}], got {tuple(enc.shape)}")
        ps, d_ff, V = self._decoder_params(idx, dev)
        with torch.cuda.device(dev):
            trg_c = trg.to(torch.int64).contiguous()
            shared = Bm > 1 and enc.stride(0) == 0  # beam search: one utterance expanded over the beams (util/beam_infer.py:233)
            enc_c = (enc[:1] if shared else enc).contiguous().float()
            nbytes = lib.eec_decoder_workspace_bytes(cfg.d_model, cfg.n_heads, d_ff, V, Bm, S, Tq)
            ws, ws_ptr = capi.aligned_ws(nbytes, dev)
            out = torch.empty((Bm, S, V), dtype=torch.float32, device=dev)
            launch("eec_decoder_forward", dev, C.byref(ps), cfg.d_model, cfg.n_heads, d_ff, V, int(self.trg_pad_idx), trg_c, enc_c, Bm, S, Tq,
                   int(shared), int(self.decoder_passes), int(log_softmax), out, ws_ptr, nbytes)
            for t in (ws, trg_c, enc_c):
                t.record_stream(torch.cuda.current_stream(dev))
        return out

    @torch.no_grad()
    def score_hypotheses(self, taps_or_enc, layer_n: int, tokens: Tensor, lengths: Tensor, sos: int, eos: int,
                         max_workspace_bytes: int = 2 << 30) -> Tensor:
        """Teacher-forced scores of whole hypotheses under exit ``layer_n``'s decoder, in eval mode on the HIP path
        (eec_decoder_score, csrc/decoder_score.hip): ``tokens`` int [n, R, L] and ``lengths`` int [n, R] are R hypotheses for each
        of n memories, ``taps_or_enc`` that exit's encoder output [n, T', D] (or the taps of all exits, [E, n, T', D] or a list,
        of which exit ``layer_n``'s is taken).  Returns fp32 [n, R]: ``log p(y_1 .. y_k, EOS | memory)`` of every hypothesis, the
        sum over the decoder's log-probs of the row ``SOS, y_1 .. y_k, pad ...`` -- what ``_decoder_`` yields for that row alone,
        gathered at the targets and summed; a negative length marks an absent hypothesis, which scores -inf and whose tokens
        are not read.  One decoder per call: callers loop over exits.  The C entry's workspace grows with
        n * heads * R * (L + 1) * T', so the call is split over memories to keep each part's workspace under
        ``max_workspace_bytes``; its default, 2 GiB, is a choice, not a measurement.  One memory is the smallest part: ValueError
        when the workspace of a single memory's R hypotheses is above the bound."""
        if self.training:
            raise RuntimeError("score_hypotheses is served in eval mode only")
        idx = self._exit(layer_n) - 1
        enc = taps_or_enc[idx] if isinstance(taps_or_enc, (list, tuple)) or taps_or_enc.dim() == 4 else taps_or_enc
        if not enc.is_cuda:
            raise RuntimeError("the MI355X decoder runs on a HIP device only (there is no CPU fallback)")
        cfg = self._cfg
        dev = enc.device
        if tokens.dim() != 3 or lengths.shape != tokens.shape[:2] or enc.dim() != 3 or enc.size(0) != tokens.size(0) or enc.size(2) != cfg.d_model:
            raise ValueError(f"score_hypotheses: tokens [n, R, L], lengths [n, R] and enc [n, T', {cfg.d_model}] expected, got "
                             f"{tuple(tokens.shape)}, {tuple(lengths.shape)}, {tuple(enc.shape)}")
        n, R, L = tokens.shape
        Tq = enc.size(1)
        out = torch.empty((n, R), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        lib = capi.load()
        ps, d_ff, V = self._decoder_params(idx, dev)
        tok = tokens.to(device=dev, dtype=torch.int32).contiguous()
        ln = lengths.to(device=dev, dtype=torch.int32).contiguous()
        enc_c = enc.contiguous().float()

        def need(m):
            return lib.eec_decoder_score_workspace_bytes(cfg.d_model, cfg.n_heads, d_ff, V, m, R, L, Tq)
        part = n
        while part > 1 and not 0 < need(part) <= max_workspace_bytes:  # 0: more memories than one call takes
            part = (part + 1) // 2
        nbytes = need(part)
        if nbytes == 0:
            raise ValueError("score_hypotheses: geometry not served by eec_decoder_score (include/eec.h)")
        if nbytes > max_workspace_bytes:
            raise ValueError(f"score_hypotheses: one memory's {R} hypotheses of {L} tokens need a workspace of {nbytes} bytes, above "
                             f"max_workspace_bytes = {max_workspace_bytes}")
        with torch.cuda.device(dev):
            ws, ws_ptr = capi.aligned_ws(nbytes, dev)
            for i in range(0, n, part):
                m = min(part, n - i)
                launch("eec_decoder_score", dev, C.byref(ps), cfg.d_model, cfg.n_heads, d_ff, V, int(self.trg_pad_idx), int(sos), int(eos),
                       tok[i:i + m], ln[i:i + m], enc_c[i:i + m], m, R, L, Tq, int(self.decoder_passes), out[i:i + m], ws_ptr, nbytes)
            for t in (ws, tok, ln, enc_c):
                t.record_stream(torch.cuda.current_stream(dev))
        return out

    def _steps_served(self, t: Tensor, max_steps: int) -> bool:
        return t.is_cuda and not (self.training and torch.is_grad_enabled()) and 1 <= max_steps <= self.positional_encoder_2.pe.size(0)

    def _decoders(self, layer_ns: Sequence[int], dev):
        """``([eec_decoder_params of every exit of layer_ns], d_ff, V, n_layers)``, or None unless they share one geometry."""
        idxs = [self._exit(n) - 1 for n in layer_ns]
        params = [self._decoder_params(i, dev) for i in idxs]
        geo = {(p[1], p[2], len(self.decoders[i].layers)) for p, i in zip(params, idxs)}
        return ([p[0] for p in params], *geo.pop()) if len(geo) == 1 else None

    def _exit_sessions(self, encs: Sequence[Tensor], layer_ns: Sequence[int], max_steps: int, lead) -> Optional["DecoderStepSession"]:
        if any(not self._steps_served(e, max_steps) or (e.dim() != 2 and e.size(0) != 1) for e in encs):
            return None
        encs = [e.reshape(-1, e.size(-1)) for e in encs]
        if len({(e.device, e.size(0)) for e in encs}) != 1:
            raise ValueError("the exits of a group share device and geometry")
        dec = self._decoders(layer_ns, encs[0].device)
        if dec is None:
            return None
        ps, d_ff, V, n_layers = dec
        cfg = self._cfg
        nbytes = capi.load().eec_decoder_cache_bytes(cfg.d_model, cfg.n_heads, d_ff, V, n_layers, int(max_steps), encs[0].size(0))
        if nbytes == 0:
            return None
        return _ExitSessions(self, ps, d_ff, V, encs, lead, int(max_steps), nbytes)

    def decoder_session(self, enc: Tensor, layer_n: int, max_steps: int) -> Optional["DecoderStepSession"]:
        """Step-wise decoding of ONE utterance with a key / value cache (csrc/decoder_step.hip): ``enc`` [1, T', D] or
        [T', D] is exit ``layer_n``'s encoder output, ``max_steps`` the longest prefix that will be decoded;
        ``step(tokens [R], parent [R])`` -> [R, V].  None when this geometry or device is not served (callers then use
        ``_decoder_`` on the whole prefix, as the reference does)."""
        return self._exit_sessions([enc], [layer_n], max_steps, ())

    def decoder_session_group(self, encs: Sequence[Tensor], layer_ns: Sequence[int], max_steps: int) -> Optional["DecoderStepSession"]:
        """One session for exits ``layer_ns`` of one utterance (``encs[i]``: that exit's encoder output), advanced together:
        ``step(tokens [n, R], parent [n, R])`` -> [n, R, V]; None when a session is not available or there are more than 8 exits."""
        if not 1 <= len(layer_ns) <= DecoderStepSession.MAX or len(encs) != len(layer_ns):
            return None
        return self._exit_sessions(encs, layer_ns, max_steps, (len(layer_ns),))

    def decoder_batch_session(self, taps, layer_ns: Sequence[int], max_steps: int) -> Optional["DecoderStepSession"]:
        """Step-wise decoding of exits ``layer_ns`` for every utterance of a padded batch in lockstep (csrc/decoder_batch.hip):
        ``taps`` [E, B, T', D] (or E tensors [B, T', D]) holds exit ``layer_ns[e]``'s encoder output of every utterance,
        ``max_steps`` the longest prefix that will be decoded; ``step(tokens [E, B, R], parent [E, B, R])`` -> [E, B, R, V].
        None when this geometry or device is not served."""
        if isinstance(taps, (list, tuple)):
            if not taps:
                return None
            taps = torch.stack(list(taps))
        if taps.dim() != 4 or taps.size(0) != len(layer_ns) or taps.size(3) != self._cfg.d_model or not self._steps_served(taps, max_steps):
            return None
        dec = self._decoders(layer_ns, taps.device)
        if dec is None:
            return None
        ps, d_ff, V, n_layers = dec
        cfg = self._cfg
        E, B, Tq = taps.shape[:3]
        nbytes = capi.load().eec_decoder_batch_cache_bytes(cfg.d_model, cfg.n_heads, d_ff, V, n_layers, E, B, int(max_steps), Tq)
        if nbytes == 0:
            return None
        return _BatchSession(self, ps, d_ff, V, [taps], (E, B), int(max_steps), nbytes)

    def _decoder_(self, trg: Tensor, enc: Tensor, layer_n: int) -> Tensor:
        return self._decode_one(trg, enc, self._exit(layer_n) - 1, log_softmax=True)

    def forward(self, src: Tensor, lengths: Tensor, trg: Tensor):
        if self.training:
            # train.py:36-52 (aed): encoder AND decoders forward / backward on the HIP training kernels (eec_train_*,
            # eec_decoder_train_*: _EncoderTrainFn, _DecoderTrainFn); the decoders consume the differentiable taps.  nn.TransformerDecoder
            # only holds the parameters.  Without autograd the same train-mode forward runs (dropout in both halves) and the tape is dropped
            enc_out, taps = self._forward_train(src, lengths, want_taps=True)
            seed = new_seed()  # one seed per forward: the exits share the embedding's dropout mask
            dec_out = torch.stack([self._decode_one(trg, taps[e], e, seed=seed) for e in range(self._cfg.n_exits)])
            return dec_out, enc_out
        enc_out, taps, _ = self._run_encoder(src, lengths, want_taps=True)
        dec_out = torch.stack([self._decode_one(trg, taps[e], e) for e in range(self._cfg.n_exits)])
        return dec_out, enc_out
