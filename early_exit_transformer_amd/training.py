"""The encoder's training step behind autograd: the whole ``Early_conformer`` forward / backward in one call each
(``_EncoderTrainFn``, csrc/train.hip), its building blocks for the models that glue groups together with torch ops
(``_TrainStemFn`` / ``_TrainGroupFn`` / ``_TrainHeadFn``: Splitformer, Early_zipformer), the exit heads on a frozen encoder
(``_ExitHeadsFn``), and the index of a model's tensors that the step reads instead of walking the module tree."""
from __future__ import annotations

import ctypes as C
import operator
from typing import List, Sequence

import torch
from torch import Tensor, nn

from . import capi
from .capi import aligned_ws, launch, to_device

_GROUP_FIELDS = [f for f in capi._LAYER_FIELDS if f not in ("conv_bn_rm", "conv_bn_rv")]  # the 30 trainable tensors of a ConformerLayer


def _tree_unchanged(edges, counts) -> bool:
    """True while every (parent's module dict, child name, child) edge of the index still holds, by identity, and no module
    gained or lost a submodule, parameter or buffer entry since the index was built (map() keeps the ~1200 checks of the default
    model in C: tens of microseconds against the walk's 1.7 ms)."""
    (dicts, names, children), (tables, sizes) = edges, counts
    return all(map(operator.is_, map(dict.get, dicts, names), children)) and list(map(len, tables)) == sizes


def _named_tensors(model):
    """(named parameters, state_dict entries) of ``model`` as lists of (name, tensor) -- the names and order of
    ``named_parameters()`` / ``state_dict(keep_vars=True)`` -- from an index of (name, module, key): the training step asks
    twice per forward and the walk over ~400 modules was 1.7 ms of its host time.  The tensors are read from the modules at every
    call (``.to()``, ``load_state_dict`` and in-place updates are seen); the index is built again whenever the module tree
    changed (a submodule replaced, added or removed: ``model.linears[1] = nn.Linear(...)``), which a check of its edges by
    identity finds."""
    idx = model.__dict__.get("_tensor_index")
    if idx is None or not _tree_unchanged(idx[2], idx[3]):
        pidx, sidx, seen, edges, tables = [], [], set(), [], []
        for mname, mod in model.named_modules(remove_duplicate=False):  # state_dict() lists a shared module under every path
            pre = mname + "." if mname else ""
            edges.extend((mod._modules, k, c) for k, c in mod._modules.items())
            tables += [mod._modules, mod._parameters, mod._buffers]
            for k, v in mod._parameters.items():
                if v is not None:
                    sidx.append((pre + k, mod, k, True))
                    if id(v) not in seen:  # named_parameters() lists a shared parameter once
                        seen.add(id(v))
                        pidx.append((pre + k, mod, k))
            for k, v in mod._buffers.items():
                if v is not None and k not in mod._non_persistent_buffers_set:
                    sidx.append((pre + k, mod, k, False))
        idx = model.__dict__["_tensor_index"] = (pidx, sidx, tuple(zip(*edges)) or ((), (), ()), (tables, [len(t) for t in tables]))
    pidx, sidx = idx[0], idx[1]
    return ([(n, m._parameters[k]) for n, m, k in pidx],
            [(n, (m._parameters if is_p else m._buffers)[k]) for n, m, k, is_p in sidx])


def _update_running_stats(groups, bn: Tensor, n: int) -> None:
    """What nn.BatchNorm1d does to running_mean / running_var / num_batches_tracked in train mode, for the Conformer layers of
    ``groups`` in order, from ``bn`` [layers, 2, D] (batch mean and biased variance over ``n`` rows): one multi-tensor update
    per momentum value instead of six tiny kernels per layer."""
    by_m = {}  # momentum -> [(layer index, module)]
    li = 0
    for grp in groups:
        for layer in grp.conformer_layers:
            bnm = layer.conv_module.sequential[3]
            if bnm.track_running_stats and bnm.running_mean is not None:
                by_m.setdefault(bnm.momentum if bnm.momentum is not None else 0.1, []).append((li, bnm))
            li += 1
    if not by_m:
        return
    with torch.no_grad():
        bvar = bn[:, 1] * (n / max(n - 1, 1))  # unbiased, as nn.BatchNorm1d stores it
        for m, mods in by_m.items():
            means, vars_ = [b_.running_mean for _, b_ in mods], [b_.running_var for _, b_ in mods]
            torch._foreach_mul_(means, 1 - m)
            torch._foreach_add_(means, [bn[i, 0] for i, _ in mods], alpha=m)
            torch._foreach_mul_(vars_, 1 - m)
            torch._foreach_add_(vars_, [bvar[i] for i, _ in mods], alpha=m)
            torch._foreach_add_([b_.num_batches_tracked for _, b_ in mods], 1)


# ---- dropout site numbers of one training step (include/eec.h: 7 per Conformer layer, calls of one step use disjoint ranges) ----
SITES_PER_LAYER = 7  # ffn1 activation, ffn1 residual, attention probabilities, attention residual, conv residual, ffn2 activation, ffn2 residual
STEM_SITE = 1        # the positional encoding's dropout (eec_train_forward numbers its own sites: 1, then 7 per layer from 2 on)
_GROUP_STRIDE, _BRANCH_OFFSET, _FIRST_GROUP_SITE = 128, 64, 16


def _group_sites(bases: Sequence[int], n_layers: Sequence[int], room: int) -> List[int]:
    for b, n in zip(bases, n_layers):
        if SITES_PER_LAYER * n > room:
            raise ValueError(f"{n} layers per Conformer group need {SITES_PER_LAYER * n} dropout sites; the numbering leaves {room} per group")
    return list(bases)


def splitformer_sites(n_exits: int, n_layers: int) -> dict:
    """site_base of every eec_train_group_forward call of a Splitformer step: exit group e, and the one-layer branch beside the
    first and the last group half a stride further."""
    groups = _group_sites([_FIRST_GROUP_SITE + _GROUP_STRIDE * e for e in range(n_exits)], [n_layers] * n_exits, _BRANCH_OFFSET)
    branches = _group_sites([groups[0] + _BRANCH_OFFSET, groups[-1] + _BRANCH_OFFSET], [1, 1], _GROUP_STRIDE - _BRANCH_OFFSET)
    return {"stem": STEM_SITE, "groups": groups, "branches": branches}


def zipformer_sites(n_groups: int, n_layers: int) -> dict:
    """site_base of every Conformer group of an Early_zipformer step."""
    return {"stem": STEM_SITE, "branches": [],
            "groups": _group_sites([_FIRST_GROUP_SITE + _GROUP_STRIDE * g for g in range(n_groups)], [n_layers] * n_groups, _GROUP_STRIDE)}


# ---- building blocks of the training step (Splitformer / Early_zipformer: train.py:180-208) ----------------------------------
def _group_layer_tensors(group: nn.Module) -> List[Tensor]:
    """The parameters of a Conformer group, layer-major, in _GROUP_FIELDS order."""
    out: List[Tensor] = []
    for layer in group.conformer_layers:
        sd = dict(layer.named_parameters())
        out += [sd[capi.LAYER_KEYS[f]] for f in _GROUP_FIELDS]
    return out


def _group_struct(tensors: Sequence[Tensor], n_layers: int):
    layers = (capi.EecLayerParams * n_layers)()
    k = len(_GROUP_FIELDS)
    for l in range(n_layers):
        for i, f in enumerate(_GROUP_FIELDS):
            setattr(layers[l], f, tensors[l * k + i].data_ptr())
    return layers


class _TrainGroupFn(torch.autograd.Function):
    """One Conformer group (torchaudio ``Conformer(num_layers=L)``: early_exit.py:160-172, 266-297) in train mode on rows
    x [B, T', D] with key lengths key_len [B] (int32, device), and its backward, on the HIP training kernels
    (eec_train_group_forward / _backward).  BatchNorm uses the batch statistics and updates the running ones like nn.BatchNorm1d."""

    @staticmethod
    def forward(ctx, model, group, x, key_len, seed, site_base, *params):
        lib = capi.load()
        dev = x.device
        cfg = model._cfg
        B, Tq, D = x.shape
        L = len(group.conformer_layers)
        for t in params:
            capi.require_fp32("a group parameter", t, dev)
        x = x.contiguous().float()
        with torch.cuda.device(dev):
            layers = _group_struct(params, L)
            nbytes = lib.eec_train_group_workspace_bytes(C.byref(cfg), L, B, Tq)
            if nbytes == 0:
                raise ValueError("unsupported geometry for a training group")
            ws, ws_ptr = aligned_ws(nbytes, dev)
            out = torch.empty_like(x)
            bn = torch.empty((L, 2, D), dtype=torch.float32, device=dev)
            launch("eec_train_group_forward", dev, C.byref(cfg), layers, L, x, key_len, B, Tq, int(model.train_passes), float(model.dropout),
                   int(seed), int(site_base), out, bn, ws_ptr, nbytes)
            _update_running_stats([group], bn, B * Tq)
        ctx.model, ctx.L, ctx.seed, ctx.site_base = model, L, int(seed), int(site_base)
        ctx.ws, ctx.ws_ptr, ctx.nbytes = ws, ws_ptr, nbytes
        ctx.passes, ctx.drop = int(model.train_passes), float(model.dropout)
        ctx.save_for_backward(x, key_len, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.ws is None:
            raise RuntimeError("this group's recorded forward was already consumed by a backward")
        x, key_len, params = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
        dev = x.device
        B, Tq, _ = x.shape
        g = g.contiguous().float()
        with torch.cuda.device(dev):
            layers = _group_struct(params, ctx.L)
            grads = [torch.empty_like(t) for t in params]
            glayers = _group_struct(grads, ctx.L)
            g_in = torch.empty_like(x)
            launch("eec_train_group_backward", dev, C.byref(ctx.model._cfg), layers, glayers, ctx.L, x, key_len, B, Tq, ctx.passes, ctx.drop,
                   ctx.seed, ctx.site_base, g, g_in, ctx.ws_ptr, ctx.nbytes)
        ctx.ws = None
        need = ctx.needs_input_grad[6:]
        return (None, None, g_in if ctx.needs_input_grad[2] else None, None, None, None, *[gr if nd else None for gr, nd in zip(grads, need)])


class _TrainStemFn(torch.autograd.Function):
    """Stem in train mode: Conv1d(k3, s2) [-> Conv1d(k3, s2)] -> + positional encoding -> dropout (early_exit.py:24-48 / 80-95,
    positional_encoding.py:65-73) -> [B, To, D]; no gradient with respect to the mel input."""

    @staticmethod
    def forward(ctx, model, mel, pe, seed, site, w0, b0, w1, b1):
        lib = capi.load()
        dev = mel.device
        cfg = model._cfg
        B, _, T = mel.shape
        two = w1 is not None
        T1 = (T - 3) // 2 + 1
        To = ((T1 - 3) // 2 + 1) if two else T1
        with torch.cuda.device(dev):
            nbytes = lib.eec_train_stem_workspace_bytes(C.byref(cfg), B, T, int(two))
            if nbytes == 0:
                raise ValueError("unsupported geometry for the training stem")
            ws, ws_ptr = aligned_ws(nbytes, dev)
            out = torch.empty((B, To, cfg.d_model), dtype=torch.float32, device=dev)
            launch("eec_train_stem_forward", dev, C.byref(cfg), w0, b0, w1, b1, pe, mel, B, T, int(model.train_passes), float(model.dropout),
                   int(seed), int(site), out, ws_ptr, nbytes)
        ctx.model, ctx.geo, ctx.two = model, (B, T), two
        ctx.seed, ctx.site, ctx.passes, ctx.drop = int(seed), int(site), int(model.train_passes), float(model.dropout)
        ctx.ws, ctx.ws_ptr, ctx.nbytes = ws, ws_ptr, nbytes
        ctx.save_for_backward(mel, w0, b0, *((w1, b1) if two else ()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        w0, b0 = saved[1], saved[2]
        dev = g.device
        B, T = ctx.geo
        g = g.contiguous().float()
        with torch.cuda.device(dev):
            g_w0, g_b0 = torch.empty_like(w0), torch.empty_like(b0)
            g_w1 = torch.empty_like(saved[3]) if ctx.two else None
            g_b1 = torch.empty_like(saved[4]) if ctx.two else None
            launch("eec_train_stem_backward", dev, C.byref(ctx.model._cfg), int(ctx.two), B, T, ctx.passes, ctx.drop, ctx.seed, ctx.site, g,
                   g_w0, g_b0, g_w1, g_b1, ctx.ws_ptr, ctx.nbytes)
        ctx.ws = None
        return (None, None, None, None, None, g_w0, g_b0, g_w1, g_b1)


class _TrainHeadFn(torch.autograd.Function):
    """Exit head ``log_softmax(x . W^T + b)`` (early_exit.py:629-631) and its backward on the training GEMM."""

    @staticmethod
    def forward(ctx, passes, x, W, b):
        dev = x.device
        x = x.contiguous().float()
        M, D = x.shape
        V = W.size(0)
        with torch.cuda.device(dev):
            logp = torch.empty((M, V), dtype=torch.float32, device=dev)
            scratch = torch.empty((M, V), dtype=torch.float32, device=dev)
            launch("eec_train_head_forward", dev, x, W, b, M, V, D, int(passes), logp, scratch)
            scratch.record_stream(torch.cuda.current_stream(dev))
        ctx.passes = int(passes)
        ctx.save_for_backward(x, W, logp)
        return logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, W, logp = ctx.saved_tensors
        lib = capi.load()
        dev = x.device
        M, D = x.shape
        V = W.size(0)
        g = g.contiguous().float()
        with torch.cuda.device(dev):
            dW, db = torch.empty_like(W), torch.empty((V,), dtype=torch.float32, device=dev)
            dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
            scratch = torch.empty((lib.eec_train_head_backward_scratch_floats(M, V, D),), dtype=torch.float32, device=dev)
            launch("eec_train_head_backward", dev, x, W, logp, g, M, V, D, ctx.passes, dx, dW, db, scratch)
            scratch.record_stream(torch.cuda.current_stream(dev))
        return (None, dx, dW, db)


def _train_group(model, group: nn.Module, x: Tensor, key_len: Tensor, seed: int, site_base: int) -> Tensor:
    return _TrainGroupFn.apply(model, group, x, key_len, seed, site_base, *_group_layer_tensors(group))


def _train_head(model, linear: nn.Linear, x: Tensor) -> Tensor:
    B, Tq, D = x.shape
    return _TrainHeadFn.apply(model.train_passes, x.reshape(B * Tq, D), linear.weight, linear.bias).reshape(B, Tq, -1)


class _ExitHeadsFn(torch.autograd.Function):
    """All exit heads on given encoder taps: log_softmax(taps[e] . W_e^T + b_e) (early_exit.py:629-631), forward through
    the HIP head kernel, backward = HIP log-softmax backward + the two GEMMs of a Linear's backward on the training GEMM
    (eec_train_head_backward)."""

    @staticmethod
    def forward(ctx, model, taps, *wb):
        E, B, Tq, D = taps.shape
        out = torch.empty((E, B, Tq, model._cfg.vocab), dtype=torch.float32, device=taps.device)
        with torch.cuda.device(taps.device):
            for e in range(E):
                model._head(e, taps[e], out[e])
        ctx.save_for_backward(taps, out, *wb[:E])
        ctx.need_taps = taps.requires_grad
        return out

    @staticmethod
    def backward(ctx, g):
        taps, out = ctx.saved_tensors[:2]
        ws = ctx.saved_tensors[2:]
        E, B, Tq, D = taps.shape
        V = out.size(-1)
        dev = taps.device
        g = g.contiguous().float()
        lib = capi.load()
        M = B * Tq
        dW = [torch.empty_like(w) for w in ws]
        db = [torch.empty((V,), dtype=torch.float32, device=dev) for _ in range(E)]
        dtaps = torch.empty_like(taps) if ctx.need_taps else None
        with torch.cuda.device(dev):
            scratch = torch.empty((lib.eec_train_head_backward_scratch_floats(M, V, D),), dtype=torch.float32, device=dev)
            for e in range(E):  # log-softmax backward + the two GEMMs of a Linear's backward on the training GEMM (bf16x3)
                launch("eec_train_head_backward", dev, taps[e], ws[e], out[e], g[e], M, V, D, 3, None if dtaps is None else dtaps[e], dW[e],
                       db[e], scratch)
            scratch.record_stream(torch.cuda.current_stream(dev))
        return (None, dtaps, *dW, *db)


# ---- the whole encoder in one call (Early_conformer, full_conformer) ----------------------------------------------------------
def _lenient(tensors):
    """Address of ``tensors[name]``, None (a null field) for a name it does not hold: what the trainer's structs are built with."""
    def ptr(name: str):
        t = tensors.get(name)
        return t.data_ptr() if t is not None else None
    return ptr


class _EncoderTrainFn(torch.autograd.Function):
    """``Early_conformer.forward`` in train mode and its backward on the HIP training kernels (csrc/train.hip): what
    ``enc_out = model(batch_0, valid_lengths)`` / ``loss.backward()`` do in the reference's train.py:53-68.  BatchNorm uses
    the batch statistics (and updates running_mean / running_var / num_batches_tracked like nn.BatchNorm1d), dropout
    runs at the reference's sites with probability ``model.dropout``."""

    @staticmethod
    def forward(ctx, model, src, len_dev, names, want_taps, *params):
        lib = capi.load()
        dev = src.device
        cfg = model._cfg
        B, _, T = src.shape
        Tq = lib.eec_out_frames(T)
        E, L, D, V = cfg.n_exits, cfg.layers_per_exit, cfg.d_model, cfg.vocab
        with torch.cuda.device(dev):
            if getattr(model, "_trainer", None) is None or model._trainer_device != dev:
                if getattr(model, "_trainer", None) is not None:
                    lib.eec_trainer_destroy(model._trainer)
                h = C.c_void_p()
                capi.call("eec_trainer_create", C.byref(cfg), C.byref(h))
                model._trainer, model._trainer_device = h, dev
            tensors = dict(zip(names, params))
            for k, v in _named_tensors(model)[1]:  # what model.state_dict(keep_vars=True) holds, without walking the module tree again
                tensors.setdefault(k, v)
            for k, t in tensors.items():
                if t.is_floating_point():
                    capi.require_fp32(f"parameter {k}", t, dev)
            pst, keep = model._params_struct(_lenient(tensors))
            nbytes = lib.eec_trainer_workspace_bytes(model._trainer, B, T)
            if nbytes == 0:
                raise ValueError("unsupported geometry for the training step")
            ws, ws_ptr = aligned_ws(nbytes, dev)
            out = torch.empty((E, B, Tq, V), dtype=torch.float32, device=dev)
            taps = torch.empty((E, B, Tq, D), dtype=torch.float32, device=dev) if want_taps else None
            bn = torch.empty((E * L, 2, D), dtype=torch.float32, device=dev)
            launch("eec_train_forward", dev, model._trainer, C.byref(pst), src, len_dev, B, T, int(model.train_passes), float(model.dropout),
                   capi.new_seed(), out, taps, bn, ws_ptr, nbytes)
            model._train_generation = getattr(model, "_train_generation", 0) + 1
            ctx.generation = model._train_generation
            _update_running_stats(model.conformer, bn, B * Tq)
        ctx.model, ctx.names, ctx.ws, ctx.ws_ptr, ctx.nbytes = model, names, ws, ws_ptr, nbytes
        ctx.keep = (src, len_dev)
        ctx.want_taps = bool(want_taps)
        ctx.save_for_backward(out, *params)
        return (out, taps) if want_taps else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, g_taps=None):
        model, names = ctx.model, ctx.names
        if ctx.generation != model._train_generation:
            raise RuntimeError("the trainer records one forward at a time: run backward before the next training forward")
        out, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dev = out.device
        g = torch.zeros_like(out) if g is None else g.contiguous().float()
        g_taps = g_taps.contiguous().float() if g_taps is not None else None
        with torch.cuda.device(dev):
            tensors = dict(zip(names, params))
            for k, v in _named_tensors(model)[1]:
                tensors.setdefault(k, v)
            pst, keep = model._params_struct(_lenient(tensors))
            # data-parallel mode (enable_data_parallel): gradients are written straight into the flat buckets and each exit
            # group's bucket is all-reduced as soon as the backward has passed that group.  Only while no parameter holds a
            # gradient yet (zero_grad(set_to_none=True), the torch default): autograd then installs the views as p.grad;
            # otherwise it would ADD the view to a p.grad that may alias it, so the step falls back to fresh tensors and
            # sync_gradients() reduces afterwards.
            dp = getattr(model, "_dp", None)
            use_views = dp is not None and all(p.grad is None for p in params)
            grads = {}
            for k, v in zip(names, params):
                view = dp["buckets"].view(k, v) if use_views else None
                grads[k] = view if view is not None else torch.empty_like(v)
            gst, gkeep = model._params_struct(_lenient(grads))
            cb, err = capi.GROUP_DONE_FN(0), []
            if dp is not None and dp["active"]:
                buckets, weight, group = dp["buckets"], dp["weight"], dp["group"]
                # a bucket may also hold parameters this function does not differentiate (full_conformer's decoders: their
                # gradients are autograd's own tensors): such buckets, and every bucket when the views are not in use, are
                # left to sync_gradients()
                mine = set(names)
                early = [use_views and all(n in mine for n, _ in b["params"]) for b in buckets.buckets]
                dp["reduced"] = set()

                def on_group(e, _user):
                    try:
                        for i in buckets.buckets_ready_after(e):
                            if early[i]:
                                buckets.allreduce_bucket(i, weight, group, trusted=True)
                                dp["reduced"].add(i)
                    except Exception as ex:  # never unwind through the C frames
                        err.append(ex)
                if any(early):
                    cb = capi.GROUP_DONE_FN(on_group)
            launch("eec_train_backward_ex", dev, model._trainer, C.byref(pst), C.byref(gst), out, g, g_taps, ctx.ws_ptr, ctx.nbytes,
                   cb, None)  # the stream goes in front of the callback
            if err:
                raise err[0]
        ctx.ws = None
        need = ctx.needs_input_grad[5:]
        return (None, None, None, None, None, *[grads[k] if nd else None for k, nd in zip(names, need)])


def forward_train(model, src: Tensor, lengths: Tensor, want_taps: bool = False):
    """The training step's forward (train.py:54) on the HIP training kernels; autograd reaches every parameter of the
    path (stem, Conformer groups, exit heads).  ``want_taps``: also return the group outputs [E, B, T', D] as a second
    differentiable result (what full_conformer hands to its attention decoders)."""
    if not src.is_cuda:
        raise RuntimeError("the MI355X training step runs on a HIP device only (there is no CPU fallback)")
    if src.dim() != 3 or src.size(1) != model._cfg.n_mels:
        raise ValueError(f"src must be [B, {model._cfg.n_mels}, T], got {tuple(src.shape)}")
    mine = ("conv_subsample.", "conformer.", model._head_key.split(".")[0] + ".")
    named = [(n, p) for n, p in _named_tensors(model)[0] if n.startswith(mine)]
    names = tuple(n for n, _ in named)
    return _EncoderTrainFn.apply(model, src.contiguous().float(), to_device(lengths, src.device), names, want_taps, *[p for _, p in named])
