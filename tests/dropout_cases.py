"""Cases shared by the dropout tests: tests/test_oracle_dropout.py (CPU: the generator's restatement, the masked oracle, the site
numbering) and tests/test_gpu_dropout.py (the device against them).

The seeds are listed here once.  They are ordinary numbers, but a finite mask is one draw: the CPU tests check, on the restated
generator alone, that every mask the GPU tests rely on keeps a fraction within 4 sigma of 1 - p and that the masks of one step
are pairwise independent within the same band -- a condition on these seeds, not on the device.
"""
import torch

from conftest import base_kwargs

# ---- the documented site numbers (include/eec.h), stated here independently of the package's functions -------------------------
SITES_PER_LAYER = 7  # ffn1 activation, ffn1 residual, attention probabilities, attention residual, conv residual, ffn2 activation, ffn2 residual
PE_SITE = 1


def documented_sites(which, n_groups, n_layers):
    """(pe site, site_base of every main group, site_base of the Splitformer's two branches)."""
    if which == "early_conformer":  # whole-model entry: the layers follow the positional encoding one after the other
        return PE_SITE, [2 + SITES_PER_LAYER * n_layers * e for e in range(n_groups)], []
    groups = [16 + 128 * g for g in range(n_groups)]  # group and stem entries: the host passes site_base
    if which == "splitformer":
        return PE_SITE, groups, [16 + 64, 16 + 128 * (n_groups - 1) + 64]
    assert which == "zipformer"
    return PE_SITE, groups, []


def documented_decoder_site(exit_index, layer, place):
    """place: 0 self-attention probabilities, 1 residual 1, 2 cross-attention probabilities, 3 residual 2, 4 activation, 5 residual 3;
    site 0 is the target embedding's positional encoding, shared by the exits of one forward."""
    return 1 + 1024 * exit_index + 6 * layer + place


# the largest layer counts of the project's configurations (BASELINE.json: 6 exits x 3 layers; Early_zipformer: its 19 groups; the
# reference's 6 decoder layers)
LARGEST = dict(n_exits=6, n_layers=3, zip_groups=19, n_dec_layers=6)
# ... and the largest site number the host or the decoder trainer ever passes with them
LARGEST_SITE = documented_decoder_site(LARGEST["n_exits"] - 1, LARGEST["n_dec_layers"] - 1, 5)

# ---- the device generator element by element (eec_train_stem_forward) ----------------------------------------------------------
STEM_SEEDS = (1, 2 ** 32 + 1, 2 ** 61 + 0x1234_5678_9ABC)
STEM_SITES = (0, 1, 8, LARGEST_SITE)
STEM_PROBS = (0.1, 0.5)
# (d_model, B, T): T' = 37 and 24 frames; B T' D = 7104 and 12288 elements, the first no multiple of 256.  d_model is a multiple of 64, so no
# element count here can be other than a multiple of 4: that case is not covered.  The stem's kernel draws its mask with the per-element
# mul() only; the four-at-a-time forms (mul4 / mul4s) and their tails are reached by the step tests below, not by the stem test.
STEM_SHAPES = ((64, 3, 151), (256, 2, 99))

# ---- the training step against the masked oracle -------------------------------------------------------------------------------
STEP_SEED = 2 ** 61 + 2 ** 40 + 12345  # what new_seed() is replaced by: both halves of the 64 bits in use
SMALL = dict(d_model=64, n_head=4, d_feed_forward=160, n_enc_exits=2, n_enc_layers=2, depthwise_kernel_size=7, dec_voc_size=32,
             enc_voc_size=32, max_len=200)
FFN_GEMM_PATH = {"EEC_TRAIN_FFN_FUSED": "0", "EEC_TRAIN_FFN_FUSED_BWD": "0"}
D256 = dict(SMALL, d_model=256, n_head=8, n_enc_exits=2, n_enc_layers=1)
# id -> (config, B, T, lengths, p, environment)
ENCODER_CASES = {
    # head dim 16: batched GEMMs + softmax kernels mask the probabilities; GEMM-epilogue masks; 1 + 2 x 2 x 7 = 29 sites
    "small_unfused_attention": (SMALL, 2, 99, [99, 70], 0.1, {}),
    # head dim 32: fused attention, T' = 37 = one full key tile and a ragged one
    "head_dim_32_fused_attention": (dict(SMALL, n_head=2), 2, 151, [151, 100], 0.1, {}),
    # d_model 256: one launch per feed-forward module and direction, d_ff 160 = a 128-wide chunk and a 32-wide rest
    "d256_fused_feed_forward": (D256, 2, 99, [99, 70], 0.1, {}),
    "d512_fused_feed_forward": (dict(SMALL, d_model=512, n_head=8, n_enc_exits=1, n_enc_layers=1), 2, 151, [151, 120], 0.1, {}),
    "small_p_0.5": (SMALL, 2, 99, [99, 70], 0.5, {}),
    "d256_feed_forward_on_the_gemm_path": (D256, 2, 99, [99, 70], 0.1, FFN_GEMM_PATH),
}
# the smallest configurations of test_other_model_types_train_on_the_hip_path: (class, config, B, T, lengths, p)
OTHER_MODEL_CASES = {
    "splitformer": ("splitformer", dict(SMALL, n_enc_exits=3, n_enc_layers=1), 3, 131, [131, 90, 57], 0.1),
    "zipformer": ("zipformer", dict(SMALL, n_enc_exits=19, n_enc_layers=1, d_feed_forward=96), 2, 139, [139, 80], 0.1),
}

# ---- the AED decoder trainer ---------------------------------------------------------------------------------------------------
DECODER_SEED = 2 ** 61 + 2 ** 35 + 777
DECODER_P = 0.1
DECODER_CASES = ((3, 9, 21, 2, 128, 4), (2, 19, 40, 2, 256, 8))  # B, S, Tq, n_dec, d_model, n_head


def model_kwargs(cfg, p):
    return base_kwargs(**dict(cfg, drop_prob=p))


def decoder_inputs(B, S, Tq, d_model, vocab=64, pad_idx=30):
    g = torch.Generator().manual_seed(B * 100 + S)
    trg = torch.randint(3, vocab, (B, S), generator=g)
    trg[trg == pad_idx] = pad_idx + 1
    trg[:, 0] = 1
    trg[1, S - 3:] = pad_idx  # padding at the end of one target
    return trg, torch.randn(B, Tq, d_model, generator=g), torch.randn(B, S, vocab, generator=g)


def binomial_band(q, n):
    """4 standard deviations of the mean of n draws of probability q."""
    return 4.0 * (q * (1.0 - q) / n) ** 0.5


def build_ref(which, kw, seed):
    """The oracle model of ``which`` in train mode with synthetic trained-style parameters, and its state dict."""
    from early_exit_transformer_amd import synth
    from oracle import conformer_ref as R
    cls = {"early_conformer": R.EarlyConformerRef, "splitformer": R.SplitformerRef, "zipformer": R.EarlyZipformerRef}[which]
    ref = cls(**kw)
    sd = synth.synth_state_dict(ref.state_dict(), seed=seed, style="trained")
    ref.load_state_dict(sd)
    return ref.train(), sd


def masked_forward(which, ref, src, lengths, masks):
    """``ref(src, lengths)`` with the masks of ``masks`` at the documented sites of model type ``which``."""
    from oracle import masked_ref
    pe_site, groups, branches = documented_sites(which, len(ref.conformer), len(ref.conformer[0].conformer_layers))
    pairs = list(zip(ref.conformer, groups))
    if branches:
        pairs += list(zip(ref.conformer_parallel, branches))
    with masked_ref.supplied_masks(ref.positional_encoder, pe_site, pairs, masks):
        return ref(src, lengths)


def all_step_cases():
    """(id, model type, config, B, T, lengths, p) of every masked training step of the GPU tests."""
    for cid, (cfg, B, T, lens, p, _env) in ENCODER_CASES.items():
        yield cid, "early_conformer", cfg, B, T, lens, p
    for cid, (which, cfg, B, T, lens, p) in OTHER_MODEL_CASES.items():
        yield cid, which, cfg, B, T, lens, p
