"""GPU tests of train-mode dropout (run with -m gpu on an MI355X) against an independent statement of the arithmetic.

The device's dropout generator is counter-based and fully specified (csrc/eec_drop.h), so the float64 oracle can be handed the very
masks the kernels draw (oracle/dropout_ref.py restates the generator, oracle/masked_ref.py runs the oracle with supplied masks at
the site numbers include/eec.h documents).  The masked network is then a smooth function, and the comparison is as sharp as at
drop_prob 0: the bounds are those of tests/test_gpu_train.py (bf16x3: log-probs 2e-4, loss 2e-4 relative, every gradient 2e-3 of
its largest entry).  What the CPU side of this rests on is checked in tests/test_oracle_dropout.py.

A site where dropout is not applied, a mask at the wrong place, a wrong scale or keep rate, two sites sharing a mask, a seed that
loses its upper half and a fused kernel that walks the mask tensor differently from its flat index all move the result by far
more than these bounds."""
import numpy as np
import pytest
import torch

import dropout_cases as DC
from conftest import base_kwargs
from early_exit_transformer_amd import capi, synth
from early_exit_transformer_amd import model as model_module
from early_exit_transformer_amd.model import Early_conformer, Early_zipformer, Splitformer, exit_ctc_losses
from early_exit_transformer_amd.training import _TrainStemFn
from oracle import conformer_ref as R
from oracle import dropout_ref, masked_ref
from test_gpu_train import bn_buffers, compare_grads, grads_of, make_aed_pair

pytestmark = pytest.mark.gpu


# ---- the generator, element by element ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,T", DC.STEM_SHAPES)
def test_device_generator_equals_the_restatement_element_by_element(D, B, T):
    """eec_train_stem_forward returns (conv(mel) + pe) * mask over [B, T', D].  Against the same call at p = 0 (no value of which
    is zero or subnormal) the mask can be read off exactly: every element is 0 or x0 * fl(1 / (1 - p)) to 1 ulp, and the kept set
    is keep_mask(seed, site, p) bit for bit -- for p 0.1 and 0.5, a seed of 32 bits, two of more (the upper half must matter), sites
    0, 1, 8 and the largest number any entry is ever passed."""
    kw = base_kwargs(**dict(DC.SMALL, d_model=D, n_enc_exits=1, n_enc_layers=1, drop_prob=0.0))
    gpu = Early_conformer(**{**kw, "device": "cuda"})
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=3, style="trained"))
    gpu = gpu.cuda().train()
    mel = synth.synth_mel(B, 80, T, seed=3).cuda()
    conv = gpu.conv_subsample.sequential

    def stem(p, seed, site):
        gpu.dropout = p
        with torch.no_grad():
            out = _TrainStemFn.apply(gpu, mel, gpu.positional_encoder.pe, seed, site, conv[0].weight, conv[0].bias, conv[1].weight, conv[1].bias)
        return out.cpu().numpy().ravel()

    x0 = stem(0.0, 1, 1)
    n = x0.size
    assert n == B * (((T - 3) // 2 + 1 - 3) // 2 + 1) * D
    assert np.isfinite(x0).all() and np.abs(x0).min() >= np.finfo(np.float32).tiny, "the p = 0 values must be normal numbers"
    kept_by = {}
    for p in DC.STEM_PROBS:
        want = x0 * dropout_ref.inv_keep(p)  # fp32 * fp32
        for seed in DC.STEM_SEEDS:
            for site in DC.STEM_SITES:
                y = stem(p, seed, site)
                kept = y != 0
                want_kept = dropout_ref.keep_mask(seed, site, p, n)
                wrong = int((kept != want_kept).sum())
                print(f"\n[generator d_model {D} p {p} seed {seed} site {site}] kept {kept.mean():.4f}, {wrong} of {n} elements differ from keep_mask")
                assert wrong == 0, (p, seed, site, wrong)
                ulps = np.abs(y[kept] - want[kept]) / np.spacing(np.abs(want[kept]))
                assert ulps.max() <= 1.0, (p, seed, site, ulps.max())
                kept_by[p, seed, site] = kept
        assert not np.array_equal(kept_by[p, DC.STEM_SEEDS[0], 1], kept_by[p, DC.STEM_SEEDS[1], 1]), "the seed's upper 32 bits are ignored"
        assert len({k.tobytes() for k in kept_by.values()}) == len(kept_by), "two (p, seed, site) drew the same mask"


# ---- the encoder's training step --------------------------------------------------------------------------------------------------
GPU_CLASSES = {"early_conformer": Early_conformer, "splitformer": Splitformer, "zipformer": Early_zipformer}


def _restore(model, buffers):
    with torch.no_grad():
        for n, b in model.named_buffers():
            if n in buffers:
                b.copy_(buffers[n].to(b.dtype))


def check_masked_step(which, cfg, B, T, lens, p, monkeypatch, label, logp_vs_dropout_off=False):
    """One training step of the product at drop_prob 0 and at ``p`` -- its dropout seed fixed to DC.STEP_SEED in both places
    new_seed is bound -- against the float64 oracle fed the masks of that seed: log-probs of every exit (2e-4), the summed CTC loss
    (2e-4 relative), every parameter gradient (2e-3, compare_grads with the float64 oracle's exact zeros) and the BatchNorm running
    statistics.  ``logp_vs_dropout_off`` (Early_zipformer only, see its test): the drop_prob 0 step keeps the log-prob bound of
    test_other_model_types_train_on_the_hip_path, 2e-4 max(1, max |logp| / 8), and the step with dropout on may exceed the error of
    the drop_prob 0 step of the same run by at most 5e-5."""
    monkeypatch.setattr(capi, "new_seed", lambda: DC.STEP_SEED)
    monkeypatch.setattr(model_module, "new_seed", lambda: DC.STEP_SEED)
    kw = DC.model_kwargs(cfg, p)
    ref, sd = DC.build_ref(which, kw, seed=31)
    ref = ref.double()
    gpu = GPU_CLASSES[which](**{**kw, "device": "cuda"})
    gpu.load_state_dict(sd, strict=True)
    gpu = gpu.cuda().train()
    mel, lens = synth.synth_mel(B, 80, T, seed=31), torch.tensor(lens)
    tgt, tl = synth.synth_targets(B, 6, kw["dec_voc_size"], seed=31)
    bn0 = bn_buffers(ref)
    outs, errs = {}, {}
    for prob in (0.0, p):
        _restore(ref, bn0), _restore(gpu, bn0)
        ref.zero_grad(set_to_none=True), gpu.zero_grad(set_to_none=True)
        masks = masked_ref.Masks(DC.STEP_SEED, prob)
        want_out = DC.masked_forward(which, ref, mel.double(), lens, masks)
        want_loss = R.summed_exit_ctc_loss(want_out, tgt, tl)
        want_loss.backward()
        gpu.dropout = prob
        out = gpu(mel.cuda(), lens)
        assert out.requires_grad and out.shape == want_out.shape
        err = (out.detach().cpu().double() - want_out.detach()).abs().max().item()
        loss = exit_ctc_losses(out, tgt, tl).sum()
        print(f"\n[{label}, drop_prob {prob}] max |dlogp| vs the masked fp64 oracle: {err:.2e} (max |logp| {want_out.abs().max().item():.1f}); "
              f"loss {loss.item():.6f} vs {want_loss.item():.6f}")
        bound = 2e-4
        if logp_vs_dropout_off:
            bound *= max(1.0, want_out.detach().abs().max().item() / 8.0)
            if prob > 0:
                bound = min(bound, errs[0.0] + 5e-5)
        errs[prob] = err
        assert err < bound, (err, bound)
        assert abs(loss.item() - want_loss.item()) < 2e-4 * max(1.0, abs(want_loss.item()))
        loss.backward()
        compare_grads(grads_of(gpu), grads_of(ref), 2e-3, f"{label}, drop_prob {prob}, bf16x3", oracle64=True)
        want_bn = bn_buffers(ref)
        for n, b in bn_buffers(gpu).items():
            assert torch.allclose(b, want_bn[n], rtol=1e-4, atol=1e-6), n
        outs[prob] = want_out.detach()
    assert (outs[p] - outs[0.0]).abs().max().item() > 1e-2, "the masks changed nothing"


@pytest.mark.parametrize("case", list(DC.ENCODER_CASES), ids=list(DC.ENCODER_CASES))
def test_training_step_with_dropout_matches_masked_fp64_oracle(case, monkeypatch):
    """Early_conformer's whole-model entry (eec_train_forward / _backward; sites: 1 = positional encoding, then 7 per layer) at the
    smallest shapes that reach each masked path: the unfused attention's softmax kernels and the GEMM epilogues (head dim 16), the
    fused attention at a ragged second key tile (head dim 32, T' = 37), the fused feed-forward launches at d_model 256 and 512 (a
    full 128-wide chunk and a 32-wide rest), p = 0.5, and d_model 256 with the feed-forward modules on the GEMM path."""
    cfg, B, T, lens, p, env = DC.ENCODER_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not env:
        for k in DC.FFN_GEMM_PATH:
            monkeypatch.delenv(k, raising=False)
    check_masked_step("early_conformer", cfg, B, T, lens, p, monkeypatch, case)


@pytest.mark.parametrize("case", list(DC.OTHER_MODEL_CASES), ids=list(DC.OTHER_MODEL_CASES))
def test_other_model_types_with_dropout_match_masked_fp64_oracle(case, monkeypatch):
    """Splitformer and Early_zipformer in train mode: the stem and every Conformer group (main groups, down-sampled branches, the
    five frame rates) go through the stem and group entries with the host's site_base numbering; the oracle draws its masks at the
    documented bases (stem 1; group g 16 + 128 g; a Splitformer branch 64 further).

    Bounds: those of the Early_conformer cases -- log-probs 2e-4, loss 2e-4 relative, every gradient 2e-3 -- with one exception,
    the log-probs of Early_zipformer.  Its head puts out log-probs down to -27 (19 layers), a bf16x3 GEMM is good to ~1e-5 of its
    result's magnitude, and the step misses 2e-4 with dropout off already: measured 2.7e-4 at drop_prob 0 and 2.1e-4 at 0.1 (max
    |logp| 27.0 / 27.5; Splitformer, max |logp| 13: 6.7e-5 / 7.5e-5).  That is the head GEMM's rounding, not the masks, and the
    project's test of this very step at drop_prob 0 (test_other_model_types_train_on_the_hip_path) bounds it by 2e-4 max(1, max
    |logp| / 8).  So the drop_prob 0 step keeps that bound, and what this test adds is held to it: the masks are integer arithmetic,
    identical on both sides, and add no rounding of their own, so the error with dropout on may exceed the error with dropout off
    of the same run by no more than 5e-5 -- a quarter of the flat bound, for the masked network being another draw of activations
    and hence of roundings.  A wrong mask moves the log-probs by 0.1 and more."""
    which, cfg, B, T, lens, p = DC.OTHER_MODEL_CASES[case]
    check_masked_step(which, cfg, B, T, lens, p, monkeypatch, case, logp_vs_dropout_off=which == "zipformer")


# ---- the AED decoder trainer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,Tq,n_dec,d_model,n_head", DC.DECODER_CASES)
def test_decoder_training_step_with_dropout_matches_masked_reference_modules(B, S, Tq, n_dec, d_model, n_head):
    """eec_decoder_train_forward / _backward at drop_prob 0.1 against the reference's decoder modules restated with supplied masks
    (oracle.masked_ref.masked_decoder_logits, float64; site 0 = positional encoding, then site_of(exit, layer, place)): logits, the
    gradient of every decoder parameter and of the encoder output, both exits, one target with trailing padding; the bounds of
    test_decoder_training_step_matches_reference_modules.  The two exits of one forward see the same embedding mask and different
    masks everywhere else: an oracle that gives exit 1 another embedding site, or exit 0's layer sites, misses the device by far
    more than the bound."""
    kw = dict(n_enc_exits=2, n_enc_layers=1, d_model=d_model, n_head=n_head, d_feed_forward=192, depthwise_kernel_size=7, dec_voc_size=64)
    common = dict(trg_pad_idx=30, enc_voc_size=64, max_len=400, features_length=80, drop_prob=DC.DECODER_P, n_dec_layers=n_dec)
    cpu, gpu, _ = make_aed_pair(kw, common, seed=13)
    cpu = cpu.double()
    trg, enc, w = DC.decoder_inputs(B, S, Tq, d_model)
    sites_of = lambda e: [DC.documented_decoder_site(e, l, 0) for l in range(n_dec)]  # noqa: E731
    got_logits = {}
    for idx in (1, 0):
        for prob in (0.0, DC.DECODER_P):
            masks = masked_ref.Masks(DC.DECODER_SEED, prob)
            e_ref = enc.double().requires_grad_(True)
            want = masked_ref.masked_decoder_logits(cpu, trg, e_ref, idx, masks, 0, sites_of(idx))
            cpu.zero_grad()
            (want * w.double()).sum().backward()
            gpu.dropout = prob
            e_gpu = enc.cuda().requires_grad_(True)
            got = gpu._decode_one(trg.cuda(), e_gpu, idx, seed=DC.DECODER_SEED)
            assert got.requires_grad and got.shape == want.shape
            err = (got.detach().cpu().double() - want.detach()).abs().max().item()
            print(f"\n[decoder exit {idx}, drop_prob {prob}] max |dlogit| vs the masked fp64 modules: {err:.2e} (max |logit| {want.abs().max().item():.1f})")
            assert err < 2e-4 * max(1.0, want.detach().abs().max().item()), err
            gpu.zero_grad()
            (got * w.cuda()).sum().backward()
            wantg = {n: p.grad.double() for n, p in cpu.named_parameters() if p.grad is not None}
            gotg = {n: p.grad.detach().cpu().double() for n, p in gpu.named_parameters() if p.grad is not None}
            assert set(wantg) == set(gotg), sorted(set(wantg) ^ set(gotg))[:5]
            compare_grads(gotg, wantg, 2e-3, f"decoder {idx}, drop_prob {prob}, bf16x3")
            ge, gw = e_gpu.grad.cpu().double(), e_ref.grad
            rel = (ge - gw).abs().max().item() / gw.abs().max().item()
            print(f"[decoder exit {idx}, drop_prob {prob}] gradient of the encoder output: {rel:.2e} of its largest entry")
            assert rel < 2e-3, "gradient of the encoder output"
        got_logits[idx] = got.detach().cpu().double()
    # what "the same embedding mask, different masks everywhere else" rules out, on exit 1
    bound = 2e-4 * max(1.0, got_logits[1].abs().max().item())
    with torch.no_grad():
        m = lambda: masked_ref.Masks(DC.DECODER_SEED, DC.DECODER_P)  # noqa: E731
        own_embedding_mask = masked_ref.masked_decoder_logits(cpu, trg, enc.double(), 1, m(), DC.documented_decoder_site(1, n_dec, 0), sites_of(1))
        exit0_layer_masks = masked_ref.masked_decoder_logits(cpu, trg, enc.double(), 1, m(), 0, sites_of(0))
    assert (own_embedding_mask - got_logits[1]).abs().max().item() > 100 * bound
    assert (exit0_layer_masks - got_logits[1]).abs().max().item() > 100 * bound
