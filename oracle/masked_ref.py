"""The oracle's train-mode forward with SUPPLIED dropout masks (the masks of csrc/eec_drop.h, restated in oracle/dropout_ref.py).

TEST INFRASTRUCTURE -- see oracle/__init__.py for who may import this.

torch's dropout streams cannot match the device's, but the device's generator is counter-based and fully specified, so the
oracle can be handed the very masks the kernels draw: the masked network is then a smooth function of the parameters and can be
compared as sharply as at drop_prob 0.  Nothing of conformer_ref's class bodies changes.  ``supplied_masks`` overrides, on ONE
model instance and for the duration of a ``with`` block, the forward of its positional encoder and of every Conformer group by
the functional restatements below; the model's own forward (the topology: exits, branches, stacks) runs unchanged around them.

``nn.MultiheadAttention`` cannot take a mask on its probabilities, so attention is written out (``explicit_attention``: in_proj,
scaled scores, padding / causal mask, softmax, mask on the probabilities, out_proj, from torch's documented definition) and held
to the module by tests/test_oracle_dropout.py.  Likewise one pre-norm decoder layer (``masked_decoder_logits``) for the AED side.

Site order (include/eec.h): per Conformer layer, from the group's base: ffn1 activation, ffn1 residual, attention probabilities,
attention residual, convolution residual, ffn2 activation, ffn2 residual.  The flat element index a mask is drawn over is the
row-major index of [B, T', D] (residual sites, positional encoding), [B, T', F] (activations), [B H, T', T'] (probabilities) and,
for the decoder, [n_tok, D] / [B S, D], [B S, F], [B H, S, S] and [B H, S, Tq].
"""
from __future__ import annotations

import contextlib
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import dropout_ref

SITES_PER_LAYER = 7


class Masks:
    """mask(site, shape) -> the multipliers (0 or 1 / (1 - p)) of site ``site`` over a tensor of ``shape``, laid out row-major as
    the device indexes it.  ``p == 0`` gives all ones: the masked path with nothing masked.  ``used`` records (site, numel)."""

    def __init__(self, seed: int, p: float, dtype=torch.float64):
        self.seed, self.p, self.dtype = int(seed), float(p), dtype
        self.used: List[Tuple[int, int]] = []

    def __call__(self, site: int, shape: Sequence[int]) -> Tensor:
        n = math.prod(shape)
        self.used.append((int(site), n))
        if self.p <= 0:
            return torch.ones(tuple(shape), dtype=self.dtype)
        keep = torch.from_numpy(dropout_ref.keep_mask(self.seed, site, self.p, n))
        return (keep.to(self.dtype) / (1.0 - self.p)).reshape(tuple(shape))


def explicit_attention(mha: nn.MultiheadAttention, query: Tensor, memory: Tensor, key_padding_mask: Optional[Tensor] = None,
                       causal: bool = False, prob_mul: Optional[Tensor] = None) -> Tensor:
    """``mha(query, memory, memory)`` written out, batch-first: query [B, Tq, D], memory [B, Tk, D], key_padding_mask [B, Tk] (True =
    masked), ``causal``: key k is masked for query q when k > q.  ``prob_mul`` [B H, Tq, Tk] multiplies the probabilities."""
    B, Tq, D = query.shape
    Tk, H = memory.size(1), mha.num_heads
    dh = D // H
    w, b = mha.in_proj_weight, mha.in_proj_bias
    q = F.linear(query, w[:D], b[:D])
    k = F.linear(memory, w[D:2 * D], b[D:2 * D])
    v = F.linear(memory, w[2 * D:], b[2 * D:])

    def heads(t):  # [B, T, D] -> [B, H, T, dh]
        return t.reshape(B, -1, H, dh).transpose(1, 2)

    s = (heads(q) / math.sqrt(dh)) @ heads(k).transpose(-1, -2)  # [B, H, Tq, Tk]
    if key_padding_mask is not None:
        s = s.masked_fill(key_padding_mask[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill(torch.ones(Tq, Tk, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    if prob_mul is not None:
        p = p * prob_mul.reshape(B, H, Tq, Tk)
    ctx = (p @ heads(v)).transpose(1, 2).reshape(B, Tq, D)
    return F.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)


def _feed_forward(ffn: nn.Module, x: Tensor, masks: Masks, site: int) -> Tensor:
    """0.5 * drop(W2 . drop(silu(W1 . LN(x)))) + x: the activation's mask at ``site``, the module output's at ``site + 1``."""
    ln, w1, act, _, w2, _ = ffn.sequential
    h = act(w1(ln(x)))
    h = h * masks(site, h.shape)
    y = w2(h)
    return 0.5 * (y * masks(site + 1, y.shape)) + x


def masked_layer(layer: nn.Module, x: Tensor, key_padding_mask: Tensor, masks: Masks, site: int) -> Tensor:
    """One ConformerLayer (conformer_ref.ConformerLayer.forward) on x [B, T', D] with the masks of sites site .. site + 6."""
    B, T, D = x.shape
    x = _feed_forward(layer.ffn1, x, masks, site)
    H = layer.self_attn.num_heads
    a = layer.self_attn_layer_norm(x)
    a = explicit_attention(layer.self_attn, a, a, key_padding_mask, prob_mul=masks(site + 2, (B * H, T, T)))
    x = a * masks(site + 3, a.shape) + x
    conv = layer.conv_module
    c = conv.layer_norm(x).transpose(1, 2)  # channel-first inside the module, as the reference runs it
    for m in list(conv.sequential)[:6]:
        c = m(c)
    c = c.transpose(1, 2)
    x = x + c * masks(site + 4, c.shape)
    x = _feed_forward(layer.ffn2, x, masks, site + 5)
    return layer.final_layer_norm(x)


def masked_group(group: nn.Module, x: Tensor, lengths: Tensor, masks: Masks, site_base: int) -> Tuple[Tensor, Tensor]:
    """conformer_ref.Conformer.forward with supplied masks: SITES_PER_LAYER sites per layer from ``site_base`` on."""
    from .conformer_ref import lengths_to_padding_mask
    kpm = lengths_to_padding_mask(lengths)
    for l, layer in enumerate(group.conformer_layers):
        x = masked_layer(layer, x, kpm, masks, site_base + SITES_PER_LAYER * l)
    return x, lengths


@contextlib.contextmanager
def supplied_masks(pe: nn.Module, pe_site: int, groups: Sequence[Tuple[nn.Module, int]], masks: Masks):
    """Within the block, positional encoder ``pe`` (conformer_ref.SinusoidPE) masks with site ``pe_site`` and every (group,
    site_base) of ``groups`` runs ``masked_group``; their nn.Dropout modules are not consulted."""
    def pe_forward(x):
        y = x + pe.pe[: x.size(1), 0].unsqueeze(0)
        return y * masks(pe_site, y.shape)

    touched = [pe]
    pe.forward = pe_forward
    for group, base in groups:
        group.forward = (lambda g, b: lambda x, lengths: masked_group(g, x, lengths, masks, b))(group, base)
        touched.append(group)
    try:
        yield masks
    finally:
        for m in touched:
            del m.forward


# --------------------------------------------------------------------------
# AED decoder (nn.TransformerDecoderLayer, norm_first, batch_first, relu)
# --------------------------------------------------------------------------
DEC_PLACES = 6  # self-attention probabilities, residual 1, cross-attention probabilities, residual 2, activation, residual 3


def masked_decoder_logits(model: nn.Module, trg: Tensor, enc: Tensor, idx: int, masks: Masks, pe_site: int, layer_sites: Sequence[int]) -> Tensor:
    """tests/conftest.ref_decoder_logits with supplied masks, over the modules that hold the parameters: embedding + positional
    encoding (mask ``pe_site`` over [n_tok, D]), the pre-norm decoder layers of ``model.decoders[idx]`` (layer l: DEC_PLACES sites
    from ``layer_sites[l]`` on), the shared final LayerNorm, ``linears_2[idx]``.  trg [B, S] int64, enc [B, Tq, D]."""
    B, S = trg.shape
    pad = trg == model.trg_pad_idx
    x = model.emb(trg) + model.positional_encoder_2.pe[:S, 0].unsqueeze(0)
    x = x * masks(pe_site, x.shape)
    dec = model.decoders[idx]
    for layer, site in zip(dec.layers, layer_sites):
        H, Tq = layer.self_attn.num_heads, enc.size(1)
        a = layer.norm1(x)
        a = explicit_attention(layer.self_attn, a, a, pad, causal=True, prob_mul=masks(site, (B * H, S, S)))
        x = x + a * masks(site + 1, a.shape)
        c = explicit_attention(layer.multihead_attn, layer.norm2(x), enc, prob_mul=masks(site + 2, (B * H, S, Tq)))
        x = x + c * masks(site + 3, c.shape)
        h = layer.activation(layer.linear1(layer.norm3(x)))  # relu (nn.TransformerDecoderLayer's default), or a caller's stand-in for it
        h = h * masks(site + 4, h.shape)
        y = layer.linear2(h)
        x = x + y * masks(site + 5, y.shape)
    return model.linears_2[idx](dec.norm(x))
