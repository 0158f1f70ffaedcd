"""CPU tests of what the GPU dropout tests (tests/test_gpu_dropout.py) stand on: the restated generator (oracle/dropout_ref.py) on
the listed seeds, the masked oracle (oracle/masked_ref.py) against the unmodified one and against torch's modules, and the site
numbering of one training step."""
import itertools
import sys

import numpy as np
import pytest
import torch

import dropout_cases as DC
from conftest import GOLDEN, ref_decoder_logits
from early_exit_transformer_amd import synth, training
from oracle import conformer_ref as R
from oracle import dropout_ref, masked_ref


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def test_generator_restatement_is_the_headers_arithmetic():
    """Hand-checkable anchors of csrc/eec_drop.h: the threshold is floor(fp32(p) 2^32), saturated; p = 0 keeps everything; the
    index enters through both of its halves; ``start`` continues the stream; the key is a function of all 64 seed bits and the site."""
    assert dropout_ref.drop_thr(0.5) == 1 << 31 and dropout_ref.drop_thr(1.0) == 0xFFFFFFFF
    assert dropout_ref.drop_thr(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32) == 429496736
    assert float(dropout_ref.inv_keep(0.5)) == 2.0 and float(dropout_ref.inv_keep(0.0)) == 1.0
    assert dropout_ref.keep_mask(5, 3, 0.0, 100).all()
    a = dropout_ref.keep_mask(7, 2, 0.3, 1000)
    assert np.array_equal(a[400:], dropout_ref.keep_mask(7, 2, 0.3, 600, start=400))
    lo, hi = dropout_ref.keep_mask(7, 2, 0.3, 512, start=0), dropout_ref.keep_mask(7, 2, 0.3, 512, start=1 << 32)
    assert not np.array_equal(lo, hi)
    keys = {dropout_ref.drop_key(s, t) for s in (1, 2 ** 32 + 1, 2 ** 63 + 1) for t in (0, 1, 2)}
    assert len(keys) == 9
    # one element by hand: h = lowbias32(i * C1 + key)
    key, i = dropout_ref.drop_key(1, 1), 12345
    h = (i * 0x9E3779B1 + key) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    assert bool(dropout_ref.keep_mask(1, 1, 0.1, 1, start=i)[0]) == (h >= dropout_ref.drop_thr(0.1))


def _assert_rate(seed, site, p, n, label):
    kept = dropout_ref.keep_mask(seed, site, p, n).mean()
    assert abs(kept - (1 - p)) <= DC.binomial_band(p, n), f"{label}: seed {seed} site {site} p {p}: kept {kept:.4f} of {n}"


def test_keep_rate_of_the_stem_cases():
    """Every (seed, site, p, size) of the element-by-element GPU test keeps a fraction within 4 sqrt(p (1 - p) / n) of 1 - p."""
    for (D, B, T), p, seed, site in itertools.product(DC.STEM_SHAPES, DC.STEM_PROBS, DC.STEM_SEEDS, DC.STEM_SITES):
        To = ((T - 3) // 2 + 1 - 3) // 2 + 1
        _assert_rate(seed, site, p, B * To * D, f"stem d_model {D}")
    a, b = (dropout_ref.keep_mask(s, 1, 0.1, 7104) for s in DC.STEM_SEEDS[:2])
    assert not np.array_equal(a, b)  # seeds 1 and 2^32 + 1 differ in the upper half only


def _sites_of_step(which, cfg, B, T, lens, p):
    """(site, numel) of every mask the masked oracle draws in one forward of the case (fp32, no autograd: only the shapes matter)."""
    ref, _ = DC.build_ref(which, DC.model_kwargs(cfg, p), seed=31)
    masks = masked_ref.Masks(DC.STEP_SEED, p, dtype=torch.float32)
    with torch.no_grad():
        DC.masked_forward(which, ref, synth.synth_mel(B, 80, T, seed=31), torch.tensor(lens), masks)
    return masks.used


@pytest.mark.parametrize("case", list(DC.all_step_cases()), ids=lambda c: c[0])
def test_keep_rate_and_independence_of_the_masks_of_a_step(case):
    """For the seed the GPU tests fix and every site of the step: the kept fraction over that site's tensor lies within
    4 sqrt(p (1 - p) / n) of 1 - p, no site is drawn twice, and every two masks agree on a fraction within the binomial band of
    p^2 + (1 - p)^2 (over the elements of the step's smallest masked tensor)."""
    cid, which, cfg, B, T, lens, p = case
    used = _sites_of_step(which, cfg, B, T, lens, p)
    sites = [s for s, _ in used]
    assert len(set(sites)) == len(sites), "a site was drawn twice in one step"
    if which == "early_conformer":
        assert len(sites) == 1 + DC.SITES_PER_LAYER * cfg["n_enc_exits"] * cfg["n_enc_layers"]
    for site, n in used:
        _assert_rate(DC.STEP_SEED, site, p, n, cid)
    n = min(n for _, n in used)
    m = np.stack([dropout_ref.keep_mask(DC.STEP_SEED, s, p, n) for s in sites]).astype(np.float64)
    agree = (m @ m.T + (1 - m) @ (1 - m).T) / n
    q = p * p + (1 - p) * (1 - p)
    off = np.abs(agree - q)[np.triu_indices(len(sites), 1)]
    assert off.max() <= DC.binomial_band(q, n), f"{cid}: two masks agree on {q:.4f} +- {off.max():.4f} of {n} (band {DC.binomial_band(q, n):.4f})"


def test_keep_rate_and_independence_of_the_decoder_masks():
    for B, S, Tq, n_dec, D, H in DC.DECODER_CASES:
        p, F = DC.DECODER_P, 192
        sizes = [B * H * S * S, B * S * D, B * H * S * Tq, B * S * D, B * S * F, B * S * D]
        used = [(0, B * S * D)] + [(DC.documented_decoder_site(e, l, k), sizes[k]) for e in range(2) for l in range(n_dec) for k in range(6)]
        for site, n in used:
            _assert_rate(DC.DECODER_SEED, site, p, n, "decoder")
        n = min(n for _, n in used)
        m = np.stack([dropout_ref.keep_mask(DC.DECODER_SEED, s, p, n) for s, _ in used]).astype(np.float64)
        agree = (m @ m.T + (1 - m) @ (1 - m).T) / n
        q = p * p + (1 - p) * (1 - p)
        assert np.abs(agree - q)[np.triu_indices(len(used), 1)].max() <= DC.binomial_band(q, n)


# ---- the site numbering -------------------------------------------------------------------------------------------------------------
def _ranges_disjoint(ranges):
    ranges = sorted(ranges)
    return all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(ranges, ranges[1:]))


@pytest.mark.parametrize("which,n_groups,n_layers", [
    ("splitformer", 2, 1), ("splitformer", 3, 1), ("splitformer", DC.LARGEST["n_exits"], DC.LARGEST["n_layers"]), ("splitformer", 2, 9),
    ("zipformer", 19, 1), ("zipformer", DC.LARGEST["zip_groups"], DC.LARGEST["n_layers"]), ("zipformer", 24, 18),
])
def test_site_ranges_of_one_step_are_disjoint(which, n_groups, n_layers):
    """The numbering Splitformer and Early_zipformer pass to the stem and group entries (training.*_sites, the functions the models
    call) is the documented one, and the ranges of the stem, every group and every branch of one step -- SITES_PER_LAYER sites per
    layer from the base on -- are pairwise disjoint.  Early_conformer's whole-model entry numbers its sites on the device (1, then 7
    per layer): there is no host function to check, the GPU step tests hold that numbering to the documented one."""
    sites = getattr(training, which + "_sites")(n_groups, n_layers)
    pe, groups, branches = DC.documented_sites(which, n_groups, n_layers)
    assert (sites["stem"], sites["groups"], sites["branches"]) == (pe, groups, branches)
    assert training.SITES_PER_LAYER == DC.SITES_PER_LAYER
    ranges = [(sites["stem"], sites["stem"] + 1)] + [(b, b + DC.SITES_PER_LAYER * n_layers) for b in sites["groups"]] + \
        [(b, b + DC.SITES_PER_LAYER) for b in sites["branches"]]
    assert _ranges_disjoint(ranges), ranges


def test_a_layer_count_that_does_not_fit_the_numbering_is_refused():
    """64 sites lie between a Splitformer group's base and its branch's, 128 between two groups: 7 sites x layers beyond that would
    share masks between two calls of one step, so the numbering raises instead."""
    training.splitformer_sites(2, 9), training.zipformer_sites(19, 18)
    with pytest.raises(ValueError):
        training.splitformer_sites(2, 10)
    with pytest.raises(ValueError):
        training.zipformer_sites(19, 19)


def test_documented_decoder_sites_are_disjoint():
    """Documentation only: the decoder trainer numbers its sites on the device (site_of in csrc/decoder_train.hip, which asserts at
    compile time that the 64 layers its entries accept fit the 1024 sites of an exit), and the GPU decoder tests hold the device to
    the statement in dropout_cases.  Here that statement is checked against itself: distinct over every exit, layer and place of
    the largest configuration, and none equal to the shared site 0."""
    E, L = DC.LARGEST["n_exits"], DC.LARGEST["n_dec_layers"]
    sites = [DC.documented_decoder_site(e, l, k) for e in range(E) for l in range(L) for k in range(6)]
    assert len(set(sites)) == len(sites) and 0 not in sites and max(sites) == DC.LARGEST_SITE
    assert DC.documented_decoder_site(0, 63, 5) < DC.documented_decoder_site(1, 0, 0)


# ---- the masked oracle against the unmodified one ----------------------------------------------------------------------------------
def test_explicit_attention_equals_multihead_attention_on_a_ragged_batch():
    """oracle.masked_ref.explicit_attention against nn.MultiheadAttention in float64: self-attention with a key-padding mask
    (ragged lengths), causal + padding (the decoder's self-attention) and cross-attention onto a memory of another length; values
    and the gradients of the input and of every parameter.  Measured 3.6e-15 .. 5.3e-15 absolute (values of order 1); bound 1e-12."""
    torch.manual_seed(0)
    B, T, Tk, D, H = 3, 11, 7, 32, 4
    mha = torch.nn.MultiheadAttention(D, H, dropout=0.0, batch_first=True).double()
    x, mem = torch.randn(B, T, D, dtype=torch.float64), torch.randn(B, Tk, D, dtype=torch.float64)
    kpm = R.lengths_to_padding_mask(torch.tensor([11, 6, 3]))
    causal = torch.triu(torch.full((T, T), float("-inf"), dtype=torch.float64), diagonal=1)
    pad_q = torch.zeros(B, T, dtype=torch.bool)
    pad_q[1, 8:] = True
    for label, kw_mod, kw_exp in [
        ("self, ragged", dict(query=x, key=x, value=x, key_padding_mask=kpm), dict(query=x, memory=x, key_padding_mask=kpm)),
        ("self, causal + padding", dict(query=x, key=x, value=x, attn_mask=causal, key_padding_mask=pad_q),
         dict(query=x, memory=x, key_padding_mask=pad_q, causal=True)),
        ("cross", dict(query=x, key=mem, value=mem), dict(query=x, memory=mem)),
    ]:
        w = torch.randn(B, T, D, dtype=torch.float64)
        res = []
        for f in (lambda: mha(need_weights=False, **kw_mod)[0], lambda: masked_ref.explicit_attention(mha, **kw_exp)):
            mha.zero_grad()
            xin = x.clone().requires_grad_(True)
            kw_mod["query"] = kw_exp["query"] = xin
            out = f()
            (out * w).sum().backward()
            res.append((out.detach(), xin.grad.clone(), [p.grad.clone() for p in mha.parameters()]))
        (o_m, gx_m, gp_m), (o_e, gx_e, gp_e) = res
        err = max((o_m - o_e).abs().max().item(), (gx_m - gx_e).abs().max().item(), *[(a - b).abs().max().item() for a, b in zip(gp_m, gp_e)])
        print(f"\n[explicit attention, {label}] max difference to nn.MultiheadAttention {err:.1e}")
        assert err < 1e-12, label


def _step(ref, forward, mel, lens, tgt, tl):
    bn0 = {n: b.clone() for n, b in ref.named_buffers()}
    ref.zero_grad()
    out = forward()
    loss = R.summed_exit_ctc_loss(out, tgt, tl)
    loss.backward()
    res = (out.detach(), loss.item(), {n: p.grad.clone() for n, p in ref.named_parameters()},
           {n: b.clone() for n, b in ref.named_buffers() if "running_" in n})
    with torch.no_grad():
        for n, b in ref.named_buffers():
            b.copy_(bn0[n])
    return res


@pytest.mark.parametrize("which,cfg,B,T,lens", [
    ("early_conformer", DC.SMALL, 2, 99, [99, 70]),
    ("early_conformer", dict(DC.SMALL, n_head=2), 2, 151, [151, 100]),
    ("splitformer", dict(DC.SMALL, n_enc_exits=2, n_enc_layers=1), 2, 151, [151, 100]),
    ("zipformer", dict(DC.SMALL, n_enc_exits=19, n_enc_layers=1, d_feed_forward=96), 2, 139, [139, 80]),
])
def test_masked_oracle_with_all_ones_masks_equals_the_plain_oracle(which, cfg, B, T, lens):
    """drop_prob 0: the unmodified oracle (its own nn.Dropout modules, nn.MultiheadAttention) and the masked path fed all-ones masks
    run the same float64 network -- train-mode log-probs, the summed CTC loss, every gradient and the BatchNorm running statistics.
    The two differ only by the rounding of float64 (torch's fused attention against the written-out one): measured at most 2.8e-14
    absolute on log-probs, 1.4e-14 on the loss and 7.2e-14 of a gradient's largest entry (the Early_zipformer and Splitformer cases);
    the bound is 1e-11 for each, some hundred times that rounding and seven orders below what the GPU tests resolve."""
    ref, _ = DC.build_ref(which, DC.model_kwargs(cfg, 0.0), seed=31)
    ref = ref.double()
    mel, lens = synth.synth_mel(B, 80, T, seed=31).double(), torch.tensor(lens)
    tgt, tl = synth.synth_targets(B, 5, 32, seed=31)
    o0, l0, g0, b0 = _step(ref, lambda: ref(mel, lens), mel, lens, tgt, tl)
    masks = masked_ref.Masks(DC.STEP_SEED, 0.0)
    o1, l1, g1, b1 = _step(ref, lambda: DC.masked_forward(which, ref, mel, lens, masks), mel, lens, tgt, tl)
    assert masks.used and "forward" not in ref.positional_encoder.__dict__ and all("forward" not in g.__dict__ for g in ref.conformer)
    e_out = (o0 - o1).abs().max().item()
    e_grad = max(((g0[n] - g1[n]).abs().max() / (g0[n].abs().max() + 1e-300)).item() for n in g0 if g0[n].abs().max() > 1e-9)
    print(f"\n[masked oracle, all-ones masks, {which}] max |dlogp| {e_out:.1e}, loss {abs(l0 - l1):.1e}, worst relative gradient difference {e_grad:.1e}")
    assert e_out < 1e-11 and abs(l0 - l1) < 1e-11 * max(1.0, abs(l0)) and e_grad < 1e-11
    assert all(torch.allclose(b0[n], b1[n], rtol=1e-12, atol=1e-14) for n in b0)


def test_masked_oracle_applies_every_mask():
    """With p > 0 every site changes the result: zeroing the masks of one site at a time (the other sites kept) moves the log-probs of
    the exits at or after it -- a site the restatement forgot to multiply in would leave them unchanged."""
    cfg = dict(DC.SMALL, n_enc_layers=1)
    ref, _ = DC.build_ref("early_conformer", DC.model_kwargs(cfg, 0.1), seed=31)
    mel, lens = synth.synth_mel(2, 80, 99, seed=31), torch.tensor([99, 70])

    class AllButOne(masked_ref.Masks):
        def __init__(self, skip):
            super().__init__(DC.STEP_SEED, 0.1, dtype=torch.float32)
            self.skip = skip

        def __call__(self, site, shape):
            m = super().__call__(site, shape)
            return torch.ones_like(m) if site == self.skip else m

    with torch.no_grad():
        full = DC.masked_forward("early_conformer", ref, mel, lens, AllButOne(-1))
        for site in range(1, 1 + 1 + 2 * 7):
            other = DC.masked_forward("early_conformer", ref, mel, lens, AllButOne(site))
            assert (other[-1] - full[-1]).abs().max().item() > 1e-4, site


# ---- the decoder layer ------------------------------------------------------------------------------------------------------------
def _aed_cpu(d_model, n_head, n_dec, p):
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    from early_exit_transformer_amd.model import full_conformer
    kw = dict(n_enc_exits=2, n_enc_layers=1, d_model=d_model, n_head=n_head, d_feed_forward=192, depthwise_kernel_size=7, dec_voc_size=64)
    common = dict(trg_pad_idx=30, enc_voc_size=64, max_len=400, features_length=80, drop_prob=p, n_dec_layers=n_dec)
    cpu = full_conformer(device="cpu", **common, **kw)
    cpu.load_state_dict(G.aed_state_dict(cpu, 13), strict=True)
    return cpu.train()


@pytest.mark.parametrize("B,S,Tq,n_dec,d_model,n_head", DC.DECODER_CASES)
def test_explicit_decoder_layer_equals_torchs_modules(B, S, Tq, n_dec, d_model, n_head):
    """masked_decoder_logits fed all-ones masks against the reference's decoder arithmetic through torch's modules
    (conftest.ref_decoder_logits: nn.TransformerDecoder, norm_first, causal + target-padding masks) in float64 at drop_prob 0, both
    exits: logits, every parameter gradient, the gradient of the encoder output.  Measured 1.1e-15 .. 1.6e-15 relative; bound 1e-12."""
    cpu = _aed_cpu(d_model, n_head, n_dec, 0.0).double()
    trg, enc, w = DC.decoder_inputs(B, S, Tq, d_model)
    enc, w = enc.double(), w.double()
    for idx in (1, 0):
        res = []
        masks = masked_ref.Masks(DC.DECODER_SEED, 0.0)
        sites = [DC.documented_decoder_site(idx, l, 0) for l in range(n_dec)]
        for f in (lambda e: ref_decoder_logits(cpu, trg, e, idx), lambda e: masked_ref.masked_decoder_logits(cpu, trg, e, idx, masks, 0, sites)):
            cpu.zero_grad()
            e = enc.clone().requires_grad_(True)
            out = f(e)
            (out * w).sum().backward()
            res.append((out.detach(), e.grad.clone(), {n: p.grad.clone() for n, p in cpu.named_parameters() if p.grad is not None}))
        (o0, ge0, g0), (o1, ge1, g1) = res
        assert set(g0) == set(g1) and len(masks.used) == 1 + 6 * n_dec
        err = max((o0 - o1).abs().max().item() / o0.abs().max().item(), (ge0 - ge1).abs().max().item() / ge0.abs().max().item(),
                  *[((g0[n] - g1[n]).abs().max() / (g0[n].abs().max() + 1e-300)).item() for n in g0])
        print(f"\n[explicit decoder layer, exit {idx}] worst relative difference to torch's modules {err:.1e}")
        assert err < 1e-12
