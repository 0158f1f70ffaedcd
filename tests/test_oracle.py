"""CPU tests: the oracle against what the reference's own class bodies computed (tests/golden/reference_bodies.npz), against
the committed golden fixtures, and the semantics of the callers' arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, base_kwargs, load_golden
from early_exit_transformer_amd import synth
from oracle import conformer_ref as R

# replaying a stored output on another host: 16 fp32 ulps of the output's largest magnitude (the same oracle run with one
# thread instead of eight moves it by up to 5)
REPLAY_ULPS = 16 * torch.finfo(torch.float32).eps
REF_STRIDE = 8  # tests/golden/make_golden.py: reference_bodies.npz keeps every 8th frame of an output whole


def _reference_body(tag):
    """tests/golden/reference_bodies.npz (make_golden.py reference_bodies): what the reference's own class body -- imported
    unmodified, the missing torchaudio symbol bound to the oracle's restatement -- returned, after the generator had checked that
    the oracle returns the same bits in the same process.  Here the oracle replays it on whatever host runs the suite."""
    z = np.load(os.path.join(GOLDEN, "reference_bodies.npz"))
    over = eval(str(z[f"{tag}_kwargs"]))
    cases = eval(str(z[f"{tag}_cases"]))
    return z, base_kwargs(**over), cases, int(z[f"{tag}_seed"]), z[f"{tag}_keys"].tolist(), eval(str(z[f"{tag}_shapes"]))


def _assert_reproduces(z, tag, i, got):
    """Every REF_STRIDE-th frame entry by entry, and every frame through its sum over the vocabulary."""
    want, rowsum = torch.from_numpy(z[f"{tag}_out{i}"]), torch.from_numpy(z[f"{tag}_rowsum{i}"])
    assert got.dtype == want.dtype and got.shape[:-1] == rowsum.shape
    assert got[:, :, ::REF_STRIDE].shape == want.shape
    # bit for bit against the reference in the generator's process; here the host's BLAS may order fp32 sums differently
    tol = REPLAY_ULPS * max(1.0, want.abs().max().item())
    err = (got[:, :, ::REF_STRIDE] - want).abs().max().item()
    assert err <= tol, (tag, i, err)
    err = (got.double().sum(-1) - rowsum).abs().max().item()
    assert err <= got.size(-1) * tol, (tag, i, "frame sums", err)


def test_oracle_equals_reference_class_body():
    """Pins the reference-owned half of the path: the reference's Early_conformer (early_exit.py:565-634) -- its state_dict keys
    in order and shapes, and its output -- equals the oracle."""
    z, kw, cases, seed, keys, shapes = _reference_body("conformer")
    mine = R.EarlyConformerRef(**kw).eval()
    assert list(mine.state_dict().keys()) == keys
    assert [tuple(v.shape) for v in mine.state_dict().values()] == shapes
    mine.load_state_dict(synth.synth_state_dict(mine.state_dict(), seed=seed, style="trained"), strict=True)
    for i, (B, T, lens) in enumerate(cases):
        with torch.no_grad():
            _assert_reproduces(z, "conformer", i, mine(synth.synth_mel(B, 80, T, seed=seed), torch.tensor(lens)))


def test_splitformer_oracle_equals_reference_class_body():
    """the reference's Splitformer (early_exit.py:227-364) equals oracle.SplitformerRef -- odd T' (the branch
    zero-pads one frame) and even T', ragged lengths."""
    z, kw, cases, seed, keys, shapes = _reference_body("splitformer")
    mine = R.SplitformerRef(**kw).eval()
    assert sorted(mine.state_dict().keys()) == sorted(keys)
    assert dict(zip(keys, shapes)) == {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    sd = synth.synth_state_dict({k: mine.state_dict()[k] for k in keys}, seed=seed, style="trained")
    mine.load_state_dict(sd, strict=True)
    for i, (B, T, lens) in enumerate(cases):
        with torch.no_grad():
            _assert_reproduces(z, "splitformer", i, mine(synth.synth_mel(B, 80, T, seed=seed), torch.tensor(lens)))


def test_zipformer_oracle_equals_reference_class_body():
    """the reference's Early_zipformer (early_exit.py:117-224) equals oracle.EarlyZipformerRef (632
    state_dict keys at 19 one-layer groups)."""
    z, kw, cases, seed, keys, shapes = _reference_body("zipformer")
    mine = R.EarlyZipformerRef(**kw).eval()
    assert len(keys) == 632 and sorted(mine.state_dict().keys()) == sorted(keys)
    assert dict(zip(keys, shapes)) == {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    sd = synth.synth_state_dict({k: mine.state_dict()[k] for k in keys}, seed=seed, style="trained")
    mine.load_state_dict(sd, strict=True)
    for i, (B, T, lens) in enumerate(cases):
        with torch.no_grad():
            _assert_reproduces(z, "zipformer", i, mine(synth.synth_mel(B, 80, T, seed=seed), torch.tensor(lens)))


def test_zipformer_oracle_reproduces_golden():
    z, kw = load_golden("zipformer_small")
    model = R.EarlyZipformerRef(**kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=int(z["seed"]), style="trained"), strict=True)
    for i, (B, T, lens) in enumerate(eval(str(z["cases"]))):
        with torch.no_grad():
            out = model(synth.synth_mel(B, 80, T, seed=int(z["seed"]) + i), torch.tensor(lens))
        assert torch.allclose(out, torch.from_numpy(z[f"logp{i}"]), atol=2e-5)


def test_splitformer_oracle_reproduces_golden():
    z, kw = load_golden("splitformer_small")
    model = R.SplitformerRef(**kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=int(z["seed"]), style="trained"), strict=True)
    for i, (B, T, lens) in enumerate(eval(str(z["cases"]))):
        with torch.no_grad():
            out = model(synth.synth_mel(B, 80, T, seed=int(z["seed"]) + i), torch.tensor(lens))
        assert torch.allclose(out, torch.from_numpy(z[f"logp{i}"]), atol=2e-5)


def test_reference_legacy_attention_matches_torch_sdpa():
    """the legacy models/layers attention (importable as-is) is softmax(qk^T/sqrt(d))v;
    this is the un-masked special case of what the attention kernel computes.  Its output on seeded q, k, v is stored."""
    z = np.load(os.path.join(GOLDEN, "reference_bodies.npz"))
    torch.manual_seed(0)
    q, k, v = (torch.randn(2, 4, 37, 32) for _ in range(3))
    qkv = torch.stack([q, k, v]).double()
    # the inputs the output was made from
    assert np.allclose([qkv.sum().item(), qkv.square().sum().item()], z["sdpa_qkv_checksum"], rtol=1e-12, atol=1e-9)
    out = torch.from_numpy(z["sdpa_out"])
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    assert torch.allclose(out, want, atol=1e-5)


def test_legacy_oracle_and_product_tree_equal_reference_early_encoder():
    """the legacy Early_encoder (early_exit.py:497-562) and everything below it IS in the reference
    tree; the oracle restatement equals it and the product mirror has the same state_dict keys and shapes."""
    from early_exit_transformer_amd.legacy import Early_encoder
    from oracle import legacy_ref as LR
    z, kw, cases, seed, keys, shapes = _reference_body("legacy")
    kw.pop("depthwise_kernel_size")
    mine, prod = LR.EarlyEncoderRef(**kw).eval(), Early_encoder(**kw)
    assert keys == list(mine.state_dict().keys()) == list(prod.state_dict().keys())
    assert shapes == [tuple(v.shape) for v in prod.state_dict().values()]
    mine.load_state_dict(synth.synth_state_dict(mine.state_dict(), seed=seed, style="trained"), strict=True)
    for i, (B, T, _) in enumerate(cases):
        with torch.no_grad():
            _assert_reproduces(z, "legacy", i, mine(synth.synth_mel(B, 80, T, seed=seed)))


def test_legacy_oracle_reproduces_golden():
    from oracle import legacy_ref as LR
    z, kw = load_golden("legacy_small")
    kw.pop("depthwise_kernel_size")
    m = LR.EarlyEncoderRef(**kw).eval()
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed=int(z["seed"]), style="trained"))
    with torch.no_grad():
        out = m(synth.synth_mel(int(z["B"]), 80, int(z["T"]), seed=int(z["seed"])))
    np.testing.assert_allclose(out.numpy(), z["logp"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", ["small", "small_h4_k7", "config1", "config1_peaky"])
def test_oracle_reproduces_golden(name):
    z, kw = load_golden(name)
    model = R.EarlyConformerRef(**kw).eval()
    sd = synth.synth_state_dict(model.state_dict(), seed=int(z["seed"]), style=str(z["style"]),
                                head_scale=float(z["head_scale"]))
    model.load_state_dict(sd)
    mel = synth.synth_mel(int(z["B"]), 80, int(z["T"]), seed=int(z["seed"]))
    assert abs(mel.double().sum().item() - float(z["mel_checksum"])) < 1e-6 * abs(float(z["mel_checksum"]))
    with torch.no_grad():
        out = model(mel, torch.from_numpy(z["lengths"]))
    stride = int(z["stride"])
    # 2e-5, or 16 fp32 ulps of the largest |log-prob| where that is more: the rounding of a log-softmax grows with the logit
    # scale, and on config1_peaky (max |log-prob| 59) the same oracle moves by 2.9e-5 with one thread instead of eight
    atol = max(2e-5, REPLAY_ULPS * float(np.abs(z["logp"]).max()))
    np.testing.assert_allclose(out[:, :, ::stride].numpy(), z["logp"], atol=atol, rtol=0)
    assert np.array_equal(out.argmax(-1).numpy().astype(np.int16), z["argmax"]) or \
        (out.argmax(-1).numpy() != z["argmax"]).mean() < 1e-3
    flat = [t for e in range(out.size(0)) for b in range(out.size(1)) for t in R.greedy_ctc(out[e, b])]
    if name == "config1_peaky":
        assert flat == z["greedy_flat"].tolist()


def test_state_dict_contract_default_config():
    """413 entries / 31,536,128 trainable parameters at the default ctc config."""
    from early_exit_transformer_amd.model import Early_conformer
    prod, ora = Early_conformer(**base_kwargs()), R.EarlyConformerRef(**base_kwargs())
    a, b = prod.state_dict(), ora.state_dict()
    assert len(a) == 413 and list(a.keys()) == list(b.keys())
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    assert sum(p.numel() for p in prod.parameters() if p.requires_grad) == 31_536_128
    assert torch.equal(a["positional_encoder.pe"], b["positional_encoder.pe"])


def test_encoder_lengths_truncation():
    lens = torch.tensor([1027, 1026, 1025, 1024, 7, 3, 5000])
    assert R.encoder_lengths(lens, 256).tolist() == [256, 256, 256, 256, 1, 0, 256]


def test_greedy_ctc_semantics():
    v = torch.full((9, 5), -10.0)
    for t, c in enumerate([0, 2, 2, 0, 2, 3, 3, 0, 1]):
        v[t, c] = 0.0
    assert R.greedy_ctc(v) == [2, 2, 3, 1]
    assert R.greedy_ctc(torch.zeros(4, 3)) == []  # ties -> label 0 = blank


def test_summed_exit_ctc_loss_is_sum_of_exits():
    torch.manual_seed(1)
    logp = torch.log_softmax(torch.randn(3, 4, 50, 32), -1)
    tgt, tl = synth.synth_targets(4, 12, 32, seed=2)
    total = R.summed_exit_ctc_loss(logp, tgt, tl)
    ctc = torch.nn.CTCLoss(blank=0, reduction="mean", zero_infinity=True)
    want = sum(ctc(logp[e].permute(1, 0, 2), tgt, torch.full((4,), 50), tl) for e in range(3))
    assert torch.allclose(total, want)


def test_synth_is_deterministic_and_torch_rng_independent():
    torch.manual_seed(123)
    a = synth.synth_mel(2, 80, 50, seed=7)
    torch.manual_seed(999)
    b = synth.synth_mel(2, 80, 50, seed=7)
    assert torch.equal(a, b) and float(a.min()) >= 0 and float(a.max()) <= 1e4
    assert not torch.equal(a, synth.synth_mel(2, 80, 50, seed=8))
    lens = synth.synth_lengths(16, 1027, seed=1)
    assert int(lens.max()) == 1027 and lens.tolist() == sorted(lens.tolist(), reverse=True)


def test_trace_substeps_ends_at_forward_taps():
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=1, d_feed_forward=128)
    m = R.EarlyConformerRef(**kw).eval()
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed=3, style="trained"))
    mel, lens = synth.synth_mel(2, 80, 99, seed=3), torch.tensor([99, 60])
    with torch.no_grad():
        steps = R.trace_substeps(m, mel, lens)
        _, taps = m(mel, lens, return_taps=True)
    assert len(steps) == 1 + 4 * 2 and torch.equal(steps[4], taps[0]) and torch.equal(steps[8], taps[1])


def test_oracle_conformer_layer_matches_independent_published_block():
    """The torchaudio half of the oracle has no reference-held vectors.  The only independent, offline check
    of the restated block ordering: Hugging Face's ``Wav2Vec2ConformerEncoderLayer`` (transformers, installed from the
    wheelhouse) is a separately written Conformer block with the same published structure -- macaron feed-forwards x 0.5,
    LayerNorm -> MHSA, LN -> pointwise -> GLU -> depthwise -> BatchNorm -> swish -> pointwise, final LayerNorm.  With the
    same weights (its convolutions carry no bias: the oracle's are zeroed; position embeddings off) the two must agree.
    This does not pin torchaudio itself; it pins the ordering / scaling constants the oracle restates."""
    # the stand-in torchaudio modules other tests bind for the reference import have no __spec__: transformers'
    # availability probes trip over them, so they are set aside while it imports
    stubs = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "torchaudio" or k.startswith("torchaudio.")}
    try:
        tr = pytest.importorskip("transformers")
        from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerEncoderLayer
    finally:
        sys.modules.update(stubs)
    D, H, F, K = 64, 4, 160, 7
    cfg = tr.Wav2Vec2ConformerConfig(hidden_size=D, num_attention_heads=H, intermediate_size=F, conv_depthwise_kernel_size=K,
                                     hidden_act="swish", position_embeddings_type=None, attention_dropout=0.0,
                                     activation_dropout=0.0, hidden_dropout=0.0, conformer_conv_dropout=0.0)
    hf = Wav2Vec2ConformerEncoderLayer(cfg).eval()
    mine = R.ConformerLayer(D, F, H, K, dropout=0.0).eval()
    sd = synth.synth_state_dict(mine.state_dict(), seed=77, style="trained")
    for k in ("conv_module.sequential.0.bias", "conv_module.sequential.2.bias", "conv_module.sequential.5.bias"):
        sd[k] = torch.zeros_like(sd[k])
    mine.load_state_dict(sd)
    wq, wk, wv = sd["self_attn.in_proj_weight"].chunk(3)
    bq, bk, bv = sd["self_attn.in_proj_bias"].chunk(3)
    hf_sd = {
        "ffn1_layer_norm.weight": sd["ffn1.sequential.0.weight"], "ffn1_layer_norm.bias": sd["ffn1.sequential.0.bias"],
        "ffn1.intermediate_dense.weight": sd["ffn1.sequential.1.weight"], "ffn1.intermediate_dense.bias": sd["ffn1.sequential.1.bias"],
        "ffn1.output_dense.weight": sd["ffn1.sequential.4.weight"], "ffn1.output_dense.bias": sd["ffn1.sequential.4.bias"],
        "self_attn_layer_norm.weight": sd["self_attn_layer_norm.weight"], "self_attn_layer_norm.bias": sd["self_attn_layer_norm.bias"],
        "self_attn.linear_q.weight": wq, "self_attn.linear_q.bias": bq, "self_attn.linear_k.weight": wk,
        "self_attn.linear_k.bias": bk, "self_attn.linear_v.weight": wv, "self_attn.linear_v.bias": bv,
        "self_attn.linear_out.weight": sd["self_attn.out_proj.weight"], "self_attn.linear_out.bias": sd["self_attn.out_proj.bias"],
        "conv_module.layer_norm.weight": sd["conv_module.layer_norm.weight"], "conv_module.layer_norm.bias": sd["conv_module.layer_norm.bias"],
        "conv_module.pointwise_conv1.weight": sd["conv_module.sequential.0.weight"],
        "conv_module.depthwise_conv.weight": sd["conv_module.sequential.2.weight"],
        "conv_module.batch_norm.weight": sd["conv_module.sequential.3.weight"], "conv_module.batch_norm.bias": sd["conv_module.sequential.3.bias"],
        "conv_module.batch_norm.running_mean": sd["conv_module.sequential.3.running_mean"],
        "conv_module.batch_norm.running_var": sd["conv_module.sequential.3.running_var"],
        "conv_module.batch_norm.num_batches_tracked": sd["conv_module.sequential.3.num_batches_tracked"],
        "conv_module.pointwise_conv2.weight": sd["conv_module.sequential.5.weight"],
        "ffn2_layer_norm.weight": sd["ffn2.sequential.0.weight"], "ffn2_layer_norm.bias": sd["ffn2.sequential.0.bias"],
        "ffn2.intermediate_dense.weight": sd["ffn2.sequential.1.weight"], "ffn2.intermediate_dense.bias": sd["ffn2.sequential.1.bias"],
        "ffn2.output_dense.weight": sd["ffn2.sequential.4.weight"], "ffn2.output_dense.bias": sd["ffn2.sequential.4.bias"],
        "final_layer_norm.weight": sd["final_layer_norm.weight"], "final_layer_norm.bias": sd["final_layer_norm.bias"],
    }
    missing, unexpected = hf.load_state_dict(hf_sd, strict=False)
    assert not unexpected and not [m for m in missing if "pos_bias" not in m and "linear_pos" not in m], (missing, unexpected)
    B, T = 3, 29
    x = torch.from_numpy(synth.normal(5, "x", B * T * D).astype(np.float32)).reshape(B, T, D)
    lens = torch.tensor([29, 17, 8])
    pad = R.lengths_to_padding_mask(lens)  # True = padding
    add_mask = torch.zeros(B, 1, T, T).masked_fill(pad[:, None, None, :], float("-inf"))  # keys only, like torchaudio
    with torch.no_grad():
        want = hf(x, attention_mask=add_mask)[0]
        got = mine(x.transpose(0, 1), pad).transpose(0, 1)
    assert (got - want).abs().max().item() < 2e-5


def test_frontend_oracle_properties():
    """oracle/frontend_ref.py (restated torchaudio Spectrogram + MelScale, util/data_loader.py:7-18): frame count, the
    filterbank's shape / support, a pure tone lands in the right mel bin, batch padding semantics."""
    from oracle import frontend_ref as FR
    fb = FR.melscale_fbanks(513, 0.0, 8000.0, 80, 16000)
    assert fb.shape == (513, 80) and (fb >= 0).all() and (fb.sum(0) > 0).all()
    assert (fb > 0).sum().item() < 1200  # two slopes per bin
    L = 16000
    t = torch.arange(L) / 16000.0
    wave = torch.sin(2 * torch.pi * 1000.0 * t)
    mel = FR.mel_frontend(wave)
    assert mel.shape == (80, 1 + L // 160)
    hz = 700.0 * (10.0 ** (torch.linspace(0, 2595.0 * np.log10(1 + 8000 / 700.0), 82) / 2595.0) - 1.0)
    peak = int(mel[:, 50].argmax())
    assert hz[peak] <= 1000.0 <= hz[peak + 2]
    batch = FR.mel_frontend_batch(torch.stack([wave, torch.cat([wave[:8000], torch.zeros(8000)])]), torch.tensor([16000, 8000]))
    assert batch.shape == (2, 80, 101) and torch.equal(batch[0], mel) and (batch[1, :, 51:] == 0).all()
    assert torch.allclose(batch[1, :, :51], FR.mel_frontend(wave[:8000]))


def test_ctc_beam_oracle_against_brute_force():
    """oracle/ctc_beam_ref.py: with a beam wide enough to hold every prefix the search is exact -- the most probable
    LABELLING (sum over all alignments), enumerated by brute force on tiny lattices; with blank-frame skipping off."""
    import itertools
    import math
    from collections import defaultdict
    from oracle.ctc_beam_ref import ctc_prefix_beam_search
    rng = np.random.default_rng(0)
    for T, V in ((5, 3), (6, 3), (4, 4)):
        x = rng.standard_normal((T, V)) * 1.5
        lp = x - np.log(np.exp(x).sum(-1, keepdims=True))
        tot = defaultdict(float)
        for path in itertools.product(range(V), repeat=T):
            out, prev = [], -1
            for c in path:
                if c != prev and c != 0:
                    out.append(c)
                prev = c
            tot[tuple(out)] += math.exp(sum(lp[t, c] for t, c in enumerate(path)))
        best = max(tot, key=tot.get)
        got, score = ctc_prefix_beam_search(lp, beam=200, blank_skip_threshold=1.0)
        assert tuple(got) == best and abs(score - math.log(tot[best])) < 1e-9
    # a repeated label across a skipped (blank) frame stays a repeat: "a <blank> a" -> [a, a]
    lp = np.log(np.array([[0.01, 0.98, 0.01], [0.98, 0.01, 0.01], [0.01, 0.98, 0.01]]))
    assert ctc_prefix_beam_search(lp, beam=4, blank_skip_threshold=0.95)[0] == [1, 1]


# ---------------------------------------------------------------------------------------------------------------------------
# Host checks of the inputs of tests/test_gpu_ctc.py (tests/ctc_cases.py): the reference values and the inclusion shares the GPU
# tests rely on hold for the reference / the oracle ALONE, wherever the suite runs.
# ---------------------------------------------------------------------------------------------------------------------------
def test_ctc_peaky_cases_have_the_intended_scale_and_finite_reference_losses():
    import ctc_cases as C
    cases = C.part1_cases()
    for scale, (lo, hi) in C.PEAKY_SCALES.items():
        assert lo < cases[f"scale{scale:g}"][0].abs().max().item() < hi, scale
    assert 55 < cases["fixture"][0].abs().max().item() < 65
    for name, (lp, match, mism) in cases.items():
        for e in range(lp.size(0)):
            for b in range(lp.size(1)):
                m = C.ref_nll(lp[e, b], match[0][b, : int(match[1][b])].tolist())
                x = C.ref_nll(lp[e, b], mism[0][b, : int(mism[1][b])].tolist())
                assert np.isfinite(m) and np.isfinite(x), (name, e, b)
                assert x / int(mism[1][b]) > 10.0, (name, e, b, x)  # unrelated targets: every path improbable (e^-10 per label at best)
                if e == 0:  # the greedy decode of the same log-probs: the most probable path, far likelier than any of the others
                    assert m / max(int(match[1][b]), 1) < x / int(mism[1][b]) / 3, (name, b, m, x)  # per label
    big = cases["scale16"]
    assert max(C.ref_nll(big[0][e, 0], big[2][0][0, : int(big[2][1][0])].tolist()) for e in range(2)) > 2000.0  # thousands of nats, finite


def test_ctc_range_lattices_have_the_reference_values_the_gpu_test_assumes():
    import ctc_cases as C
    cases = C.range_cases()
    assert len(cases) == len(C.RANGE_FRAMES) * len(C.RANGE_X) + 4
    for name, lp, target in cases:
        v = C.ref_nll(lp, target)
        assert np.isfinite(v) and 50.0 < v < 400.0, (name, v)
        assert lp.shape == (C.RANGE_T, C.RANGE_V)
    for fr in C.RANGE_FRAMES:  # on the named frames blank and both labels sit at -x (to 1e-6), elsewhere they are likely
        lp = C.range_lattice(fr, 60.0)
        assert (lp[list(fr)][:, [0, 3, 4]] + 60.0).abs().max().item() < 1e-6
        rest = [t for t in range(C.RANGE_T) if t not in fr]
        assert lp[rest][:, [0, 3, 4]].min().item() > -8.0
    assert C.range_lattice((5,), 95.0)[5, 0].item() < -94.0  # below the fp32 range of exp (-87.3)
    masked = dict((n, l) for n, l, _ in cases)["masked-vocabulary"]
    assert np.isneginf(masked[:, [1, 2, 5]].numpy()).all() and np.isfinite(masked[:, [0, 3, 4, 6, 7]].numpy()).all()
    for name, lp, target in C.infeasible_cases():
        assert C.ref_nll(lp, target) == float("inf"), name
        z = C.ref_ctc(lp.float().view(1, 1, *lp.shape), torch.tensor([list(target)]), torch.tensor([len(target)]))
        assert z[0].item() == 0.0 and (z[1] == 0).all()  # zero_infinity: zero loss, zero gradient


def test_ctc_beam_cases_leave_at_most_a_quarter_of_the_sequences_uncompared():
    """The GPU beam tests compare tokens only where the oracle's best prefix leads its runner-up by more than 5e-3 and require
    that on at least 3/4 of the sequences: the oracle alone meets it on the same inputs, both readings of the skip rule."""
    import ctc_cases as C
    from oracle.ctc_beam_ref import ctc_prefix_beam_search

    def share(logp, beam, **kw):
        out = []
        for drop in (False, True):
            fin = [ctc_prefix_beam_search(logp[n].double().numpy(), beam=beam, return_beams=True, skip_drops_frame=drop, **kw)[2]
                   for n in range(logp.size(0))]
            out.append(sum(C.safe_margin(f) for f in fin) / logp.size(0))
        return min(out)

    for N, T, V, beam, scale in C.BEAM_CASES:
        assert share(C.beam_logp(N, T, V, scale), beam) >= 0.75, (N, T, V, beam, scale)
    assert share(C.fixture_beam_logp(), 10) >= 0.75
    assert share(C.beam_logp(4, 30, 255, 4.0), 10) >= 0.75
    assert share(C.beam_logp(8, 40, 32, 4.0, blank=31), 10, blank=31) >= 0.75
    assert share(C.beam_logp(8, 40, 32, 6.0), 1) >= 0.75
    assert len(C.BIG_SAMPLE) == 16 and sorted(n % 4 for n in C.BIG_SAMPLE) == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    big = C.big_batch_logp()
    safe = sum(C.safe_margin(ctc_prefix_beam_search(big[n].double().numpy(), beam=10, return_beams=True)[2]) for n in C.BIG_SAMPLE)
    assert safe >= 12, safe
