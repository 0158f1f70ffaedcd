"""GPU parity tests (run with -m gpu on an MI355X): the HIP encoder, called through the drop-in
nn.Module -> ctypes -> C-ABI, against the CPU oracle and the committed golden fixtures.

Tolerances (max |delta log-prob| vs the fp32 reference path, stated per operand mode):
    f16x3  1e-3   DEFAULT.  The north_star's tolerance, FLAT, on every fixture incl. the peaky (trained-like) one; measured 3.8e-5 on the
                  12-layer model, 3.7e-4 peaky.  Every test that does not name a mode runs this one.
    f16f8  1e-3 x max(1, max|logp| / 8)   opt-in fast mode (correction products of every GEMM but the heads in block-scaled fp8):
                  1e-3 flat on near-uniform outputs (measured 4.1e-4), NOT on peaky ones (4.1e-3 at max|logp| 59) -- it does not
                  claim the north-star tolerance there and is not the default
    mixed  2.5e-3 x the same factor (measured 1.0-1.3e-3)
    f16    6e-3   x the same factor (measured 3.0e-3)
"""
import numpy as np
import pytest
import torch

from conftest import base_kwargs, load_golden, ref_decoder_logits, ref_decoder_logprobs
from early_exit_transformer_amd import synth
from early_exit_transformer_amd.model import (Early_conformer, Early_zipformer, Splitformer, exit_ctc_losses, full_conformer,
                                             greedy_ctc)
from oracle import conformer_ref as R

pytestmark = pytest.mark.gpu
TOL = {"f16f8": 1e-3, "f16x3": 1e-3, "mixed": 2.5e-3, "f16": 6e-3}
FLAT_MODES = ("f16x3",)  # modes that claim the north-star tolerance as a FLAT bound on every output, peaky ones included
DEFAULT_MODE = "f16x3"


def make_pair(kw, seed, style="trained", head_scale=1.0):
    ref = R.EarlyConformerRef(**kw).eval()
    sd = synth.synth_state_dict(ref.state_dict(), seed=seed, style=style, head_scale=head_scale)
    ref.load_state_dict(sd)
    gpu = Early_conformer(**{**kw, "device": "cuda"}).eval()
    gpu.load_state_dict(sd, strict=True)
    return ref, gpu.cuda()


def run_gpu(model, mel, lens, prec=DEFAULT_MODE):
    model.precision = prec
    with torch.no_grad():
        out = model(mel.cuda(), lens)
    torch.cuda.synchronize()
    return out.cpu()


def test_native_library_is_loaded():
    from early_exit_transformer_amd import capi
    lib = capi.load()
    assert lib.eec_abi_version() == 16
    assert any("libeec.so" in line for line in open("/proc/self/maps"))


def test_mfma16_gemm_forms_equal_the_32x32_forms():
    """Device check of the k-loops of the default (split) format: the 16x16x32 forms (re-addressed fragments of the same
    packing, quadrant accumulators restored by lane swaps; csrc/eec_device.h, csrc/eec_wave.h) against the 32x32x16 forms on the
    same LDS planes, packed weights and rings -- both orientations, 1 / 2 row tiles, 1 / 2 column tiles, ring refills, single
    k-steps -- and the training GEMM's bf16 form (csrc/eec_wave.h) against v_mfma_f32_32x32x16_bf16.  Built
    by `make` (csrc/build/mfma16_gemm_check); exits non-zero if any accumulator element differs by more than 1e-4."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "early_exit_transformer_amd", "csrc", "build", "mfma16_gemm_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(os.path.dirname(exe)), "build/mfma16_gemm_check"], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.count(" OK") >= 12 and "FAIL" not in res.stdout, res.stdout + res.stderr


def logp_tolerance(prec, want_logp):
    """The default mode (FLAT_MODES): the north-star tolerance, flat -- |dlogp| <= 1e-3 whatever the outputs look like.
    The opt-in faster modes state a weaker bound: |dlogp| <= TOL[prec] * max(1, max|logp| / LOGP_UNIT) -- their operand
    rounding is a RELATIVE error on the logits, so the absolute log-prob error grows with the logit scale; near-uniform
    outputs (|logp| <= ~8: random-init heads, log 256 = 5.5) get the flat bound, peaky ones the same bound relative to
    their scale (README / INTEGRATION.md say so where they describe the modes)."""
    if prec in FLAT_MODES:
        return TOL[prec]
    return TOL[prec] * max(1.0, float(np.abs(want_logp).max()) / LOGP_UNIT)


LOGP_UNIT = 8.0
ERR_REPORT = {}


@pytest.mark.parametrize("prec", ["f16f8", "f16x3", "mixed", "f16"])
@pytest.mark.parametrize("name", ["small", "small_h4_k7", "config1", "config1_peaky", "config3_small", "config3"])
def test_golden_logprobs(name, prec):
    """Committed fixtures made by the reference's own Early_conformer class body (make_golden.py)."""
    z, kw = load_golden(name)
    gpu = Early_conformer(**{**kw, "device": "cuda"}).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=int(z["seed"]), style=str(z["style"]),
                                               head_scale=float(z["head_scale"])))
    gpu = gpu.cuda()
    mel = synth.synth_mel(int(z["B"]), 80, int(z["T"]), seed=int(z["seed"]))
    out = run_gpu(gpu, mel, torch.from_numpy(z["lengths"]), prec)
    assert out.shape[:2] == z["logp"].shape[:2] and not torch.isnan(out).any()
    err = np.abs(out[:, :, ::int(z["stride"])].numpy() - z["logp"]).max()
    scale = float(np.abs(z["logp"]).max())
    ERR_REPORT[(name, prec)] = (err, scale)
    # the error on the entries a decoder reads (log-prob >= -10): reported next to the flat maximum, and held to the same
    # bound (it cannot exceed the maximum; on peaky outputs it is what decides a greedy / beam decision)
    top = z["logp"] >= -10.0
    err_top = np.abs(out[:, :, ::int(z["stride"])].numpy() - z["logp"])[top].max()
    print(f"\n[parity] {name:14s} {prec:6s} max|dlogp| {err:.3e}  on logp >= -10: {err_top:.3e}  max|logp| {scale:6.2f}  "
          f"err/scale {err / scale:.2e}  tolerance {logp_tolerance(prec, z['logp']):.2e}")
    assert err_top <= err
    # the mode's stated bound: FLAT 1e-3 on every fixture for the default mode (no exemption: the peaky, trained-like fixture
    # included -- Q, K and the attention probabilities keep fp16 residuals; measured 3.7e-4 at max|logp| 59); the opt-in modes'
    # own bound otherwise, which is flat as well wherever max|logp| <= 8
    assert err < logp_tolerance(prec, z["logp"]), f"{name}/{prec}: max|dlogp| {err:.3e} at max|logp| {scale:.1f}"
    if prec in FLAT_MODES:
        assert err < 1e-3, f"{name}/{prec}: the north-star tolerance: max|dlogp| {err:.3e}"
    # a checksum of checksums over the FULL tensor (fixtures keep every stride-th frame only).  A logit error on a row's
    # dominant class shifts the whole row's log-probs together, so the errors of a row do not average out: the bound is
    # a quarter of "every element off by the tolerance"
    assert np.allclose([out[e].double().sum().item() for e in range(out.size(0))], z["checksum"],
                       rtol=0, atol=logp_tolerance(prec, z["logp"]) * out[0].numel() * 0.25)


def test_golden_greedy_decode_exact():
    """Greedy CTC (util/beam_infer.py:9-24) on peaky heads, in the DEFAULT mode: token sequences identical to the reference's
    for every (exit, utterance) whose frames all have a top-2 margin above twice the bound that mode is held to on this very
    fixture (test_golden_logprobs: flat 1e-3, measured 3.7e-4) -- two log-probs off by less than the bound each cannot swap."""
    z, kw = load_golden("config1_peaky")
    gpu = Early_conformer(**{**kw, "device": "cuda"}).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=int(z["seed"]), style=str(z["style"]),
                                               head_scale=float(z["head_scale"])))
    gpu = gpu.cuda()
    mel = synth.synth_mel(int(z["B"]), 80, int(z["T"]), seed=int(z["seed"]))
    assert gpu.precision == DEFAULT_MODE  # the class default: nothing selects a mode here
    bound = logp_tolerance(gpu.precision, z["logp"])
    with torch.no_grad():
        out = gpu(mel.cuda(), torch.from_numpy(z["lengths"]))
        got = gpu.greedy_decode(out)
    assert np.abs(out[:, :, ::int(z["stride"])].cpu().numpy() - z["logp"]).max() < bound  # the bound the margin filter relies on
    E, B = z["greedy_counts"].shape
    flat, pos, compared = z["greedy_flat"].tolist(), 0, 0
    safe = (z["margin"] > 2 * bound).all(axis=-1)  # [E,B]
    frame_ok = z["margin"] > 2 * bound
    am = out.argmax(-1).cpu().numpy()
    assert (am[frame_ok] == z["argmax"][frame_ok]).all(), "argmax differs on a frame with a safe margin"
    for e in range(E):
        for b in range(B):
            n = int(z["greedy_counts"][e, b])
            want = flat[pos:pos + n]
            pos += n
            if safe[e, b]:
                assert got[e][b] == want, f"exit {e} utt {b}"
                compared += 1
    assert compared >= E * B // 2, f"only {compared}/{E*B} sequences had safe margins"


def test_ctc_skip_rule_readings_differ_exactly_where_expected():
    """'a _ a' with the middle frame above blank_skip_threshold: taken as a blank frame the repeat survives ('aa'); dropped, it
    collapses ('a').  Through BeamInference.ctc_cuda_predict the hypotheses carry .tokens like torchaudio's (train.py:82)."""
    from early_exit_transformer_amd.beam import BeamInference
    from early_exit_transformer_amd.model import ctc_beam_decode
    V = 8
    p = torch.full((1, 3, V), 1e-4)
    p[0, 0, 3] = 0.9
    p[0, 1, 0] = 0.99   # blank-dominated: above the 0.95 threshold
    p[0, 2, 3] = 0.9
    logp = torch.log(p / p.sum(-1, keepdim=True)).cuda()
    tok, cnt, _ = ctc_beam_decode(logp, beam_size=4)
    assert tok[0, : int(cnt[0])].tolist() == [3, 3]
    tok, cnt, _ = ctc_beam_decode(logp, beam_size=4, skip_drops_frame=True)
    assert tok[0, : int(cnt[0])].tolist() == [3]
    hyp = BeamInference().ctc_cuda_predict(logp, beam_size=4)
    assert hyp[0][0].tokens == [3, 3] and isinstance(hyp[0][0].score, float)


def test_greedy_kernel_bit_exact_on_same_logprobs():
    """Integer path: the decode kernel vs the oracle decoder on the SAME log-probs, incl. ties and ragged T'."""
    torch.manual_seed(0)
    for n, t, v in [(5, 1, 32), (3, 64, 256), (4, 65, 64), (2, 333, 256), (7, 128, 32)]:
        lp = torch.log_softmax(torch.randn(n, t, v) * 3, -1)
        lp[0, : t // 2] = lp[0, :1]  # long runs of repeats
        lp[-1, :, 0] = 1.0  # all blank
        if t > 3:
            lp[1, 2, 5] = lp[1, 2].max()  # an exact tie -> lowest index wins, as torch.argmax
        tokens, counts = greedy_ctc(lp.cuda())
        tokens, counts = tokens.cpu(), counts.cpu()
        for i in range(n):
            assert tokens[i, : counts[i]].tolist() == R.greedy_ctc(lp[i])


@pytest.mark.parametrize("prec", ["f16f8", "f16x3", "f16"])
def test_every_substep_against_oracle(prec):
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=2, d_feed_forward=512)
    ref, gpu = make_pair(kw, seed=4)
    mel, lens = synth.synth_mel(3, 80, 203, seed=4), torch.tensor([203, 150, 99])
    with torch.no_grad():
        steps = R.trace_substeps(ref, mel, lens)
    gpu.precision = prec
    for k, want in enumerate(steps):
        with torch.no_grad():
            x = gpu._run_encoder(mel.cuda(), lens, want_out=False, stop_after=k, want_x=True)[2].cpu()
        scale = want.abs().max().item()
        err = (x - want).abs().max().item()
        assert err < {"f16x3": 2e-4, "f16f8": 4e-4, "f16": 2e-3}[prec] * max(scale, 1.0), f"sub-step {k}: {err:.3e} (scale {scale:.2f})"


@pytest.mark.parametrize("prec", ["f16f8", "f16x3", "mixed", "f16"])
def test_fused_plan_equals_substep_plan(prec):
    """The production plan (3 launches per layer, fused chain kernel) and the sub-step plan (one launch per step,
    the one test_every_substep_against_oracle walks) run the same arithmetic: their final residual streams differ
    only by fp32 summation order (the exchange-tile row pass vs accumulator epilogues)."""
    kw = base_kwargs(n_enc_exits=3, n_enc_layers=2, d_feed_forward=640)  # 5 chunks of 128: odd chunk count
    _, gpu = make_pair(kw, seed=12)
    mel, lens = synth.synth_mel(5, 80, 403, seed=12), torch.tensor([403, 402, 300, 77, 5])  # M = 495: ragged last tile
    gpu.precision = prec
    with torch.no_grad():
        out_f, _, x_f = gpu._run_encoder(mel.cuda(), lens, want_x=True)
        n_sub = 1 + 4 * 6
        out_s, _, x_s = gpu._run_encoder(mel.cuda(), lens, stop_after=n_sub, want_x=True)
    out_f, x_f, out_s, x_s = out_f.cpu(), x_f.cpu(), out_s.cpu(), x_s.cpu()
    assert torch.isfinite(x_f).all() and torch.isfinite(out_f).all()
    assert (x_f - x_s).abs().max().item() < 2e-5 * max(x_s.abs().max().item(), 1.0)
    assert (out_f - out_s).abs().max().item() < 5e-5


@pytest.mark.parametrize("B,T,lens", [
    (1, 7, [7]),                     # T' = 1: the shortest legal input
    (1, 131, [131]),                 # single utterance, one partial row tile
    (5, 403, [403, 402, 300, 77, 5]),  # T' = 99: not a multiple of 32; M = 495 not a multiple of 64; len -> 1
    (2, 1100, [1100, 640]),          # T' = 274 > 256: two key chunks in the attention kernel
    (3, 259, [259, 259, 259]),       # no padding at all
    (4, 61, [1, 8, 61, 3]),          # lengths < 4 -> encoder length 0: every key masked (torch's safe softmax: zeros)
    # T' a multiple of 64: the attention runs inside the out_proj / GLU launch (capi.hip attn_fusable)
    (4, 515, [515, 300, 9, 2]),      # T' = 128, keys masked mid-tile, one utterance of encoder length 0
    (2, 771, [771, 400]),            # T' = 192: three row tiles per utterance
    (2, 1283, [1283, 1000]),         # T' = 320 > 256: two key chunks, the second a quarter full
])
def test_ragged_shapes(B, T, lens):
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=1, d_feed_forward=256)
    ref, gpu = make_pair(kw, seed=9)
    mel, lt = synth.synth_mel(B, 80, T, seed=9), torch.tensor(lens)
    with torch.no_grad():
        want = ref(mel, lt)
    got = run_gpu(gpu, mel, lt)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < TOL[DEFAULT_MODE]
    assert torch.allclose(got.exp().sum(-1), torch.ones(got.shape[:-1]), atol=1e-4)


@pytest.mark.parametrize("over", [dict(n_head=4), dict(depthwise_kernel_size=7), dict(depthwise_kernel_size=1),
                                  dict(d_feed_forward=128), dict(dec_voc_size=32), dict(dec_voc_size=160),
                                  dict(n_enc_exits=1, n_enc_layers=3), dict(features_length=48)])
def test_config_surface(over):
    """--n_heads / --depthwise_kernel_size / --d_feed_forward / vocab / --n_enc_exits / --n_enc_layers_per_exit / --n_mels."""
    kw = base_kwargs(**{**dict(n_enc_exits=2, n_enc_layers=1, d_feed_forward=256), **over})
    ref, gpu = make_pair(kw, seed=13)
    nm = kw["features_length"]
    mel, lens = synth.synth_mel(2, nm, 179, seed=13), torch.tensor([179, 120])
    with torch.no_grad():
        want = ref(mel, lens)
    assert (run_gpu(gpu, mel, lens) - want).abs().max().item() < TOL["f16x3"]


@pytest.mark.parametrize("case", range(40))
def test_random_configs_and_batches(case):
    """Seeded random sweep over the supported configuration surface and ragged batches (the reference's own tests
    hold no such cases; the oracle is the judge)."""
    g = np.random.default_rng(1000 + case)
    kw = base_kwargs(
        n_enc_exits=int(g.integers(1, 4)), n_enc_layers=int(g.integers(1, 3)),
        d_feed_forward=int(g.choice([96, 128, 320, 384, 512])), n_head=int(g.choice([4, 8])),
        depthwise_kernel_size=int(g.choice([3, 9, 15, 31])), dec_voc_size=int(g.choice([32, 96, 256])),
        features_length=int(g.choice([16, 48, 80])))
    B, T = int(g.integers(1, 7)), int(g.integers(7, 700))
    lens = g.integers(1, T + 1, size=B)
    lens[int(g.integers(0, B))] = T  # the reference's mask needs max(lengths) == T
    ref, gpu = make_pair(kw, seed=1000 + case)
    mel, lt = synth.synth_mel(B, kw["features_length"], T, seed=case), torch.tensor(lens)
    with torch.no_grad():
        want = ref(mel, lt)
    prec = "f16f8" if case % 4 == 3 else DEFAULT_MODE  # three quarters of the sweep in the default mode
    got = run_gpu(gpu, mel, lt, prec)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < TOL[prec], (kw, B, T, lens.tolist())


@pytest.mark.parametrize("prec", ["f16f8", "f16x3"])
def test_early_exit_prefix_equals_full_forward(prec):
    """eec_encoder_forward_prefix (run only the first n exit groups) returns bit for bit what the full forward
    returns for those exits, and its final residual stream is exit n's tap."""
    kw = base_kwargs(n_enc_exits=4, n_enc_layers=2, d_feed_forward=384)
    ref, gpu = make_pair(kw, seed=31)
    mel, lens = synth.synth_mel(3, 80, 331, seed=31), torch.tensor([331, 200, 64])
    gpu.precision = prec
    with torch.no_grad():
        full, taps, _ = gpu._run_encoder(mel.cuda(), lens, want_taps=True)
        for n in (1, 2, 4):
            out_n, taps_n, x_n = gpu._run_encoder(mel.cuda(), lens, want_taps=True, want_x=True, n_groups=n)
            assert out_n.shape[0] == n and torch.equal(out_n, full[:n]) and torch.equal(taps_n, taps[:n])
            assert torch.equal(x_n, taps[n - 1])
        assert torch.equal(gpu.forward_exits(mel.cuda(), lens, 3), full[:3])
        want = ref(mel, lens)
    assert (full.cpu() - want).abs().max().item() < TOL[prec]
    with pytest.raises(ValueError):
        gpu._run_encoder(mel.cuda(), lens, n_groups=5)


def test_more_exits_than_the_batched_head_launch_holds():
    """17 exits: above the 16 per-exit pointer slots of the batched head launch, so the heads fall back to one
    launch per exit (same kernel body)."""
    kw = base_kwargs(n_enc_exits=17, n_enc_layers=1, d_feed_forward=128, depthwise_kernel_size=7, dec_voc_size=32)
    ref, gpu = make_pair(kw, seed=71)
    mel, lens = synth.synth_mel(2, 80, 139, seed=71), torch.tensor([139, 60])
    with torch.no_grad():
        want = ref(mel, lens)
    got = run_gpu(gpu, mel, lens, "f16x3")
    assert got.shape == want.shape and got.shape[0] == 17
    assert (got - want).abs().max().item() < TOL["f16x3"]


def test_full_conformer_encoder_taps_golden():
    """config 5 substitute: full_conformer._encoder_(src, lengths, n) (early_exit.py:719-737), fixture from the
    reference's own full_conformer."""
    z, kw = load_golden("full_conformer_taps")
    kw.pop("src_pad_idx"), kw.pop("device")
    fc = full_conformer(trg_pad_idx=126, n_dec_layers=1, device="cuda", **kw).eval()
    enc_keys = {k: v for k, v in fc.state_dict().items()
                if k.split(".")[0] in ("conv_subsample", "linears_1", "positional_encoder_1", "conformer")}
    fc.load_state_dict(synth.synth_state_dict(enc_keys, seed=int(z["seed"]), style="trained"), strict=False)
    fc = fc.cuda()
    mel, lens = synth.synth_mel(1, 80, int(z["T"]), seed=int(z["seed"])), torch.tensor([int(z["T"])])
    with torch.no_grad():
        for n in (1, 2):
            tap = fc._encoder_(mel.cuda(), lens, n).cpu().numpy()
            assert np.abs(tap - z["taps"][n - 1]).max() < 1e-3
        dec, enc = fc(mel.cuda(), lens, torch.tensor([[1, 5, 9, 2]]).cuda())
    assert dec.shape == (2, 1, 4, 256) and enc.shape == (2, 1, 50, 256)


@pytest.mark.parametrize("E,B,T,V,S", [(3, 4, 50, 32, 12), (6, 5, 256, 256, 42), (2, 3, 33, 64, 1), (1, 2, 300, 256, 150), (2, 2, 10, 32, 12)])
def test_exit_ctc_losses_match_torch_ctc(E, B, T, V, S):
    """Summed per-exit CTC loss (train.py:53-65) vs the oracle's nn.CTCLoss loop on the same log-probs, incl.
    repeated labels (no skip transition), single-label targets and an infeasible utterance (zero_infinity)."""
    torch.manual_seed(E * 100 + T)
    logp = torch.log_softmax(torch.randn(E, B, T, V) * 2, -1)
    tgt, tl = synth.synth_targets(B, max(S, 3), V, seed=T) if S >= 3 else (torch.full((B, 1), 5), torch.ones(B, dtype=torch.int64))
    tgt = tgt.clone()
    if S >= 3:
        tgt[0, 2] = tgt[0, 1]  # a repeated label
    # (2, 2, 10, 32, 12): 12 labels in 10 frames is infeasible -> +inf -> zeroed by zero_infinity
    got = exit_ctc_losses(logp.cuda(), tgt, tl).cpu()
    ctc = torch.nn.CTCLoss(blank=0, reduction="mean", zero_infinity=True)
    il = torch.full((B,), T, dtype=torch.long)
    want = torch.stack([ctc(logp[e].permute(1, 0, 2), tgt, il, tl) for e in range(E)])
    assert torch.allclose(got, want, rtol=2e-5, atol=2e-5), (got, want)
    assert abs(got.sum().item() - R.summed_exit_ctc_loss(logp, tgt, tl).item()) < 1e-4 * max(1.0, want.sum().item())


@pytest.mark.parametrize("prec", ["f16f8", "f16x3", "f16"])
def test_legacy_early_encoder_golden(prec):
    """the legacy pre-norm transformer encoder on the same kernels (attention without mask,
    ReLU feed-forward, group-final LayerNorm); fixture produced by the reference's own, unmodified Early_encoder."""
    from early_exit_transformer_amd.legacy import Early_encoder
    z, kw = load_golden("legacy_small")
    kw.pop("depthwise_kernel_size")
    m = Early_encoder(**{**kw, "device": "cuda"}).eval()
    m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed=int(z["seed"]), style="trained"), strict=True)
    m = m.cuda()
    m.precision = prec
    with torch.no_grad():
        out = m(synth.synth_mel(int(z["B"]), 80, int(z["T"]), seed=int(z["seed"])).cuda()).cpu()
    assert out.shape == z["logp"].shape
    assert np.abs(out.numpy() - z["logp"]).max() < TOL[prec]


def test_legacy_early_encoder_against_oracle_other_shapes():
    from early_exit_transformer_amd.legacy import Early_encoder
    from oracle import legacy_ref as LR
    kw = base_kwargs(n_enc_exits=1, n_enc_layers=3, d_feed_forward=512, n_head=4)
    kw.pop("depthwise_kernel_size")
    ref = LR.EarlyEncoderRef(**kw).eval()
    sd = synth.synth_state_dict(ref.state_dict(), seed=8, style="trained")
    ref.load_state_dict(sd)
    m = Early_encoder(**{**kw, "device": "cuda"}).eval()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    mel = synth.synth_mel(2, 80, 403, seed=8)
    with torch.no_grad():
        assert (m(mel.cuda()).cpu() - ref(mel)).abs().max().item() < TOL["f16x3"]


def test_reload_weights_repacks():
    kw = base_kwargs(n_enc_exits=1, n_enc_layers=1, d_feed_forward=128)
    ref, gpu = make_pair(kw, seed=1)
    mel, lens = synth.synth_mel(2, 80, 99, seed=1), torch.tensor([99, 64])
    a = run_gpu(gpu, mel, lens)
    sd2 = synth.synth_state_dict(ref.state_dict(), seed=2, style="trained")
    gpu.load_state_dict(sd2)
    ref.load_state_dict(sd2)
    b = run_gpu(gpu, mel, lens)
    with torch.no_grad():
        want = ref(mel, lens)
    assert (b - want).abs().max().item() < 1e-3 and (a - b).abs().max().item() > 1e-2


def test_error_paths():
    gpu = Early_conformer(**base_kwargs(n_enc_exits=1, n_enc_layers=1, d_feed_forward=128, max_len=40, device="cuda")).eval().cuda()
    with pytest.raises(ValueError):
        gpu(torch.zeros(1, 81, 99).cuda(), torch.tensor([99]))
    with pytest.raises(RuntimeError, match="max_len"):
        gpu(torch.zeros(1, 80, 403).cuda(), torch.tensor([403]))  # T' = 99 > 40
    with pytest.raises(RuntimeError, match="HIP device only"):
        gpu(torch.zeros(1, 80, 99), torch.tensor([99]))
    with pytest.raises(RuntimeError, match="unsupported|256 or 512"):
        Early_conformer(**base_kwargs(d_model=128, n_head=4, device="cuda")).eval().cuda()(torch.zeros(1, 80, 99).cuda(), torch.tensor([99]))
    gpu.train()  # train mode with trainable parameters runs the training step (tests/test_gpu_train.py)
    assert gpu(torch.zeros(1, 80, 99).cuda(), torch.tensor([99])).requires_grad


class TestFullSize:
    """BASELINE.json configs[1] (B=64, T=1027): size-independent properties instead of a CPU run."""

    @pytest.fixture(scope="class")
    def setup(self):
        kw = base_kwargs()
        ref, gpu = make_pair(kw, seed=0, style="trained")
        mel = synth.synth_mel(64, 80, 1027, seed=0)
        lens = synth.synth_lengths(64, 1027, seed=0)
        out = run_gpu(gpu, mel, lens)
        return ref, gpu, mel, lens, out

    def test_normalised_and_finite(self, setup):
        _, _, _, _, out = setup
        assert out.shape == (6, 64, 256, 256) and torch.isfinite(out).all()
        assert torch.allclose(out.exp().sum(-1), torch.ones(6, 64, 256), atol=2e-4)

    def test_deterministic(self, setup):
        _, gpu, mel, lens, out = setup
        assert torch.equal(run_gpu(gpu, mel, lens), out)

    def test_utterances_are_independent(self, setup):
        """Batch sharding premise: an utterance's result does not depend on its batch neighbours."""
        _, gpu, mel, lens, out = setup
        sub = run_gpu(gpu, mel[40:44], lens[40:44])
        assert torch.equal(sub, out[:, 40:44])

    def test_subset_against_oracle(self, setup):
        ref, _, mel, lens, out = setup
        idx = [0, 17, 63]
        with torch.no_grad():
            # the reference mask needs max(lengths) == T inside the sub-batch: utterance 0 is full length
            want = ref(mel[idx], lens[idx])
        assert (out[:, idx] - want).abs().max().item() < TOL["f16x3"]


def test_long_utterances_two_key_chunks_default_model():
    """SURVEY 8d secondary shape: T = 2051 -> T' = 512 (two 256-key chunks per attention workgroup, two query blocks
    per (utterance, head)), ragged lengths, default 12-layer model; two utterances are checked against the oracle."""
    kw = base_kwargs()
    ref, gpu = make_pair(kw, seed=21, style="trained")
    mel = synth.synth_mel(6, 80, 2051, seed=21)
    lens = torch.tensor([2051, 1999, 1500, 1027, 640, 2051])
    out = run_gpu(gpu, mel, lens)
    assert out.shape == (6, 6, 512, 256) and torch.isfinite(out).all()
    idx = [0, 4]
    with torch.no_grad():
        want = ref(mel[idx], lens[idx])
    assert (out[:, idx] - want).abs().max().item() < TOL[DEFAULT_MODE]


@pytest.mark.parametrize("prec", ["f16f8", "f16x3"])
def test_splitformer_golden(prec):
    """the Splitformer drop-in (groups and heads through eec_encoder_group_forward /
    eec_encoder_head_forward) against the fixture produced by the reference's own Splitformer class."""
    z, kw = load_golden("splitformer_small")
    gpu = Splitformer(**{**kw, "device": "cuda"}).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=int(z["seed"]), style="trained"), strict=True)
    gpu = gpu.cuda()
    for i, (B, T, lens) in enumerate(eval(str(z["cases"]))):
        got = run_gpu(gpu, synth.synth_mel(B, 80, T, seed=int(z["seed"]) + i), torch.tensor(lens), prec)
        want = torch.from_numpy(z[f"logp{i}"])
        assert got.shape == want.shape
        assert (got - want).abs().max().item() < TOL[prec]


def test_splitformer_against_oracle_two_layer_groups():
    kw = base_kwargs(n_enc_exits=4, n_enc_layers=2, d_feed_forward=384, depthwise_kernel_size=31)
    ref = R.SplitformerRef(**kw).eval()
    sd = synth.synth_state_dict(ref.state_dict(), seed=51, style="trained")
    ref.load_state_dict(sd)
    gpu = Splitformer(**{**kw, "device": "cuda"}).eval()
    gpu.load_state_dict(sd, strict=True)
    gpu = gpu.cuda()
    mel, lens = synth.synth_mel(4, 80, 523, seed=51), torch.tensor([523, 523, 260, 40])  # T' = 130
    with torch.no_grad():
        want = ref(mel, lens)
    errs = {p: (run_gpu(gpu, mel, lens, p) - want).abs().max().item() for p in ("f16x3", "f16f8")}
    # the head input is the SUM of two LayerNormed streams (group output + up-sampled branch): with these synthetic
    # weights the logits are ~2x Early_conformer's (log-probs down to -15); the tolerance follows the stated policy
    # (logp_tolerance: the flat 1e-3 up to |logp| = 8, relative to the log-prob scale beyond)
    print(f"\n[parity] splitformer two-layer groups: max|logp| {want.abs().max().item():.1f}  errors {errs}")
    for p, e in errs.items():
        assert e < logp_tolerance(p, want.numpy()), (p, e)
    assert torch.equal(run_gpu(gpu, mel, lens), run_gpu(gpu, mel, lens))  # deterministic


@pytest.mark.parametrize("prec", ["f16f8", "f16x3"])
def test_zipformer_golden(prec):
    """the Early_zipformer drop-in (one-convolution stem, 19 groups at five frame rates, one head)
    against the fixture produced by the reference's own class; then once more against the oracle on another shape."""
    z, kw = load_golden("zipformer_small")
    gpu = Early_zipformer(**{**kw, "device": "cuda"}).eval()
    sd = synth.synth_state_dict(gpu.state_dict(), seed=int(z["seed"]), style="trained")
    gpu.load_state_dict(sd, strict=True)
    gpu = gpu.cuda()
    # Five skip additions of un-normalised streams make the head input ~6x Early_conformer's: with these synthetic
    # weights the log-probs span [-40, 0]; the tolerance follows the stated policy (logp_tolerance: relative to the
    # log-prob scale beyond |logp| = 8; measured 0.3-0.5e-4 of the scale in f16x3 / f16f8)
    def check(got, want):
        assert got.shape == want.shape
        err = (got - want).abs().max().item()
        assert err < logp_tolerance(prec, want.numpy()), (err, want.abs().max().item())

    for i, (B, T, lens) in enumerate(eval(str(z["cases"]))):
        check(run_gpu(gpu, synth.synth_mel(B, 80, T, seed=int(z["seed"]) + i), torch.tensor(lens), prec),
              torch.from_numpy(z[f"logp{i}"]))
    ref = R.EarlyZipformerRef(**kw).eval()
    ref.load_state_dict(sd)
    mel, lens = synth.synth_mel(3, 80, 523, seed=7), torch.tensor([523, 300, 31])  # T1 = 261
    with torch.no_grad():
        want = ref(mel, lens)
    check(run_gpu(gpu, mel, lens, prec), want)
    assert torch.equal(run_gpu(gpu, mel, lens, prec), run_gpu(gpu, mel, lens, prec))  # deterministic


def test_stem_dynamic_range():
    """The reference feeds UN-LOGGED power mel (util/data_loader.py:7-18): heavy-tailed, no upper bound.  The stem's
    fp16 hi/lo operands live in per-ROW power-of-two scaled domains chosen from each row's own maximum (stem.hip), so
    loud frames (1e6 - 1e7) do not saturate and neither a loud utterance nor a single outlier bin costs the quiet frames
    (1e-8) of the batch their precision."""
    kw = base_kwargs(n_enc_exits=1, n_enc_layers=1, d_feed_forward=256)
    ref, gpu = make_pair(kw, seed=17)
    B, T = 4, 259
    base = synth.synth_mel(B, 80, T, seed=17)
    mel = base.clone()
    mel[0] *= 1e3                      # up to 1e7
    mel[1] = mel[1] * 1e-6             # down to ~1e-8 and below
    mel[2, :, 100:110] = 3.0e6         # a loud burst inside an otherwise ordinary utterance
    mel[3, 5, 17] = 9.9e6              # a single outlier bin
    lens = torch.tensor([T, T, 200, 131])
    with torch.no_grad():
        want_x = ref.stem(mel)
        want = ref(mel, lens)
    for prec in ("f16f8", "f16x3"):
        gpu.precision = prec
        with torch.no_grad():
            x = gpu._run_encoder(mel.cuda(), lens, want_out=False, stop_after=0, want_x=True)[2].cpu()
        rel = ((x - want_x).abs().amax(dim=(1, 2)) / want_x.abs().amax(dim=(1, 2))).tolist()
        assert max(rel) < 2e-5, rel  # per utterance, relative to that utterance's own scale
        got = run_gpu(gpu, mel, lens, prec)
        assert torch.isfinite(got).all()
        per_utt = (got - want).abs().amax(dim=(0, 2, 3)).tolist()
        print(f"\n[stem range] {prec}: stem rel err per utterance {['%.1e' % r for r in rel]}, max|dlogp| per utterance {['%.2e' % e for e in per_utt]}")
        assert max(per_utt) < logp_tolerance(prec, want.numpy()), per_utt


def test_encoder_lengths_bit_exact():
    """clamp(lengths / 4, max=T').to(int) -- true division in fp32, then truncation
    (early_exit.py:623) -- as integers, on the device."""
    from early_exit_transformer_amd.model import encoder_lengths
    g = np.random.default_rng(3)
    for Tq in (1, 99, 256, 2000):
        lens = np.concatenate([np.arange(0, 70), g.integers(0, 4 * Tq + 50, 500), [4 * Tq - 1, 4 * Tq, 4 * Tq + 1, 2 ** 24 + 1, 2 ** 31 + 5]])
        lt = torch.from_numpy(lens.astype(np.int64))
        want = R.encoder_lengths(lt, Tq)
        got = encoder_lengths(lt.cuda(), Tq).cpu()
        assert got.dtype == torch.int32 and torch.equal(got, want.to(torch.int32))


def test_aed_greedy_tokens_golden():
    """BASELINE config 5 substitute: greedy (beam = 1) AED decode for EVERY exit, B = 1, default 6 x 2 model
    with 6 decoder layers, as inference.py:44-51 drives it: ``_encoder_`` and ``_decoder_`` both on the HIP path.  Fixture: the reference's own full_conformer run on CPU.  Tokens must be
    identical up to the first step whose top-2 margin in the fixture is below the safety margin."""
    import os
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    kw = eval(str(z["kwargs"]))
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=int(z["n_dec_layers"]), **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    fc = fc.cuda()
    fc.device = "cuda"
    SAFE = 2e-2
    compared = total = 0
    for i, (T, seed) in enumerate(eval(str(z["cases"]))):
        mel, lengths = synth.synth_mel(1, 80, T, seed=seed).cuda(), torch.tensor([T])
        for n in range(1, kw["n_enc_exits"] + 1):
            want, margin = z[f"tokens{i}"][n - 1].tolist(), z[f"margin{i}"][n - 1]
            with torch.no_grad():
                enc = fc._encoder_(mel, lengths, n)
                tokens = torch.tensor([[1]], dtype=torch.long, device="cuda")
                for _ in range(G.aed_max_length(T)):
                    nxt = fc._decoder_(tokens, enc, n)[:, -1].argmax(-1, keepdim=True)
                    tokens = torch.cat([tokens, nxt], dim=1)
            got = tokens[0].tolist()
            unsafe = np.nonzero(margin < SAFE)[0]
            upto = 1 + (int(unsafe[0]) if len(unsafe) else len(margin))  # tokens[0] is SOS; step k writes tokens[k + 1]
            assert got[:upto] == want[:upto], f"case {i} exit {n}: {got} vs {want}"
            compared += upto - 1
            total += len(margin)
    assert compared >= 0.8 * total, f"only {compared}/{total} decode steps had safe margins"


def test_hip_decoder_matches_the_reference_decoder_modules():
    """full_conformer._decoder_ on the hand-written path (eec_decoder_forward) against the same parameters run through the
    reference's own modules (nn.TransformerDecoder, norm_first, causal + padding masks) in fp32 on the CPU: log-probs within
    2e-5 of their scale (bf16x3 GEMMs), for ragged targets with PAD positions, several beams, S = 1 and odd T'."""
    import os
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    kw = dict(n_enc_exits=2, n_enc_layers=1, d_model=256, n_head=8, d_feed_forward=512, depthwise_kernel_size=31, dec_voc_size=256)
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=3, **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, 5), strict=True)
    g = torch.Generator().manual_seed(0)
    for Bm, S, Tq in ((1, 1, 17), (4, 9, 33), (10, 23, 64)):
        enc = torch.randn(Bm, Tq, 256, generator=g)
        trg = torch.randint(3, 256, (Bm, S), generator=g)
        trg[:, 0] = 1
        if S > 4:
            trg[0, S - 2:] = 126  # PAD tail on one row (masked as keys)
        fc = fc.cpu()
        with torch.no_grad():
            want = [ref_decoder_logprobs(fc, trg, enc, n) for n in (1, 2)]
            want_logits = ref_decoder_logits(fc, trg, enc, 0)
        fc = fc.cuda()
        with torch.no_grad():
            if Bm > 1:  # one memory expanded over the rows (what beam search passes): projected once, same result
                one = enc[:1].cuda()
                a = fc._decoder_(trg.cuda(), one.expand(Bm, -1, -1), 1)
                b2 = fc._decoder_(trg.cuda(), one.repeat(Bm, 1, 1), 1)
                assert (a - b2).abs().max().item() < 2e-5 * max(10.0, b2.abs().max().item())  # other tiling of the key / value GEMM
            got = [fc._decoder_(trg.cuda(), enc.cuda(), n).cpu() for n in (1, 2)]
            got_logits = fc._decode_one(trg.cuda(), enc.cuda(), 0).cpu()
        for w, gt in zip(want + [want_logits], got + [got_logits]):
            ok = torch.isfinite(w)
            assert torch.equal(ok, torch.isfinite(gt))
            # bf16x3 GEMMs are good to ~1e-5 RELATIVE: the synthetic decoder's log-probs reach -40 (measured error 2e-4 there)
            tol = 2e-5 * max(10.0, w[ok].abs().max().item())
            assert (w[ok] - gt[ok]).abs().max().item() < tol, (Bm, S, Tq, (w[ok] - gt[ok]).abs().max().item(), tol)


@pytest.mark.parametrize("d_model,n_head,d_ff,beams", [(256, 8, 512, 10), (512, 8, 2048, 16), (64, 4, 128, 3)])
def test_decoder_session_steps_match_the_reference_decoder_on_whole_prefixes(d_model, n_head, d_ff, beams):
    """Step-wise decoding over the key / value cache (eec_decoder_begin / eec_decoder_step) against what the reference's beam
    search computes at every step (util/beam_infer.py:233-240): its own decoder modules (CPU, fp32) on the WHOLE prefix of every
    live beam, last position.  The beams are re-ordered at random each step (parents with repeats and drop-outs, a changing
    beam count), prefixes contain PAD tokens (masked as self-attention keys); head dims 32, 64 and 16."""
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    kw = dict(n_enc_exits=2, n_enc_layers=1, d_model=d_model, n_head=n_head, d_feed_forward=d_ff, depthwise_kernel_size=31, dec_voc_size=256)
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=2, **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, 7), strict=True)
    g = torch.Generator().manual_seed(d_model + beams)
    Tq, steps = 37, 14
    enc = torch.randn(1, Tq, d_model, generator=g)
    ref = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cpu",
                         n_dec_layers=2, **kw).eval()
    ref.load_state_dict(fc.state_dict())
    fc = fc.cuda()
    for exit_n in (1, 2):
        sess = fc.decoder_session(enc.cuda(), exit_n, steps)
        assert sess is not None and sess.max_beams == 16
        prefixes = torch.tensor([[1]])
        parent = None
        worst = 0.0
        for s in range(steps):
            got = sess.step(prefixes[:, -1].cuda(), None if parent is None else parent.cuda()).cpu()
            with torch.no_grad():
                want = ref_decoder_logprobs(ref, prefixes, enc.expand(prefixes.size(0), -1, -1), exit_n)[:, -1]
            assert got.shape == want.shape
            tol = 2e-5 * max(10.0, want.abs().max().item())
            err = (got - want).abs().max().item()
            assert err < tol, (exit_n, s, err, tol)
            worst = max(worst, err / tol)
            # next step: a random number of beams, each extending a random row of this step with a random token (PAD now and then)
            R = beams if s % 5 != 3 else max(1, beams // 2)
            parent = torch.randint(0, prefixes.size(0), (R,), generator=g)
            tok = torch.randint(3, 256, (R,), generator=g)
            tok[torch.rand(R, generator=g) < 0.15] = 126
            prefixes = torch.cat([prefixes[parent], tok.unsqueeze(1)], dim=1)
        with pytest.raises(RuntimeError):
            sess.step(prefixes[:, -1].cuda(), parent.cuda())  # opened for `steps` positions
    assert fc.decoder_session(enc.cuda().expand(2, -1, -1), 1, steps) is None  # one utterance per session


def test_aed_beam_search_with_and_without_the_kv_cache():
    """BeamInference.beam_search through the step-wise decoder session (default) and on whole prefixes (`kv_cache=False`,
    the reference's way) return the same beams: identical tokens wherever the candidate scores are not within rounding of
    each other, final scores within 1e-3."""
    import os
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    from early_exit_transformer_amd.beam import BeamInference
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    kw = eval(str(z["kwargs"]))
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=int(z["n_dec_layers"]), **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    fc = fc.cuda()
    inf = BeamInference()
    g = torch.Generator().manual_seed(2)
    same = 0
    for case in range(3):
        enc = torch.randn(1, 40 + 13 * case, kw["d_model"], generator=g).cuda()
        for n in (1, kw["n_enc_exits"]):
            args = dict(vocab_size=256, max_length=12, SOS_token=1, EOS_token=2, PAD_token=126, beam_size=10, pen_alpha=0.6)
            ta, sa, ba = inf.beam_search(fc, enc, n, **args)
            tb, sb, bb = inf.beam_search(fc, enc, n, kv_cache=False, **args)
            sa_, sb_ = torch.stack(sa).cpu().sort().values, torch.stack(sb).cpu().sort().values
            assert (sa_ - sb_).abs().max().item() < 1e-3
            gaps = (sb_[1:] - sb_[:-1]).abs().min().item()
            if gaps > 2e-3:  # no two candidates within rounding: the beams must be the same sequences in the same order
                assert [t.tolist() for t in ta] == [t.tolist() for t in tb] and ba == bb
                same += 1
    assert same >= 3
    # EOS finalisation (min_length below the step count) removes rows mid-search: the parent indices must follow
    args = dict(vocab_size=256, max_length=10, min_length=2, SOS_token=1, EOS_token=2, PAD_token=126, beam_size=6, pen_alpha=0.6)
    first = fc._decoder_(torch.tensor([[1]], device="cuda"), enc, 1)[0, -1]
    eos = int(first.topk(3).indices[2])  # a token the head likes right after SOS: beams finish at different steps
    args["EOS_token"] = eos
    ta, sa, ba = inf.beam_search(fc, enc, 1, **args)
    tb, sb, bb = inf.beam_search(fc, enc, 1, kv_cache=False, **args)
    assert len(ta) == len(tb) == 6
    assert (torch.stack(sa).cpu().sort().values - torch.stack(sb).cpu().sort().values).abs().max().item() < 1e-3


@pytest.mark.parametrize("n,R,V,K,length", [(6, 10, 256, 10, 7), (1, 1, 256, 10, 1), (3, 16, 40, 16, 30), (2, 5, 11, 3, 4)])
def test_beam_select_matches_the_torch_bookkeeping(n, R, V, K, length):
    """eec_beam_select (top-k of score + log-prob / penalty over all beams and tokens, parent / token split, token gather:
    util/beam_infer.py:241-262 for n searches at once) against the same step written with torch.topk / gather / cat;
    ties go to the lower flat index and the output is ordered best first."""
    from early_exit_transformer_amd.model import beam_select
    g = torch.Generator().manual_seed(n * 1000 + R * V + K)
    logp = torch.log_softmax(torch.randn(n, R, V, generator=g) * 3, dim=-1).cuda()
    scores = (torch.randn(n, R, generator=g) * 2).cuda()
    steps = length + 3
    old = torch.randint(0, V, (n, max(R, K), steps), generator=g).cuda()
    new = torch.full_like(old, -1)
    penalty = 1.37
    got_s, got_p, got_t = beam_select(logp, scores, penalty, K, old, new, length)
    cand = (scores.unsqueeze(2) + logp / penalty).reshape(n, -1)
    want_s, idx = torch.topk(cand, K, dim=1)
    assert (got_s - want_s).abs().max().item() < 1e-5
    assert bool((got_s[:, :-1] >= got_s[:, 1:]).all())
    flat = got_p * V + got_t
    assert bool(((got_p >= 0) & (got_p < R) & (got_t >= 0) & (got_t < V)).all())
    assert all(len(set(row.tolist())) == K for row in flat.cpu())  # K distinct candidates
    assert (cand.gather(1, flat) - got_s).abs().max().item() < 1e-5  # the reported scores are the chosen candidates' scores
    want_tokens = torch.cat([torch.gather(old[:, :, :length], 1, got_p.unsqueeze(2).expand(-1, -1, length)), got_t.unsqueeze(2)], dim=2)
    assert torch.equal(new[:, :K, :length + 1], want_tokens)
    assert bool((new[:, :K, length + 1:] == -1).all())
    # exact ties: every beam offers the same log-probs and the same score -> the lowest flat indices, in order
    logp2 = logp[:, :1].expand(-1, R, -1).contiguous()
    s2 = torch.zeros(n, R, device="cuda")
    _, p2, t2 = beam_select(logp2, s2, 1.0, min(K, R), old, new, length)
    top_tok = logp2[:, 0].argmax(dim=1)
    assert torch.equal(t2, top_tok.unsqueeze(1).expand(-1, min(K, R)))
    assert torch.equal(p2, torch.arange(min(K, R), device="cuda").unsqueeze(0).expand(n, -1))


def test_small_host_tensors_reach_the_device_through_kernel_arguments():
    """model._to_device: up to 480 int64 values of a CPU tensor travel in a kernel's argument block (eec_upload_i64), larger
    or non-int64 tensors take the ordinary copy; values, shapes and dtypes are those of ``tensor.to(device)`` either way."""
    from early_exit_transformer_amd.model import _to_device
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    for shape in ((1,), (64,), (480,), (481,), (6, 80), (0,), (3, 5, 7)):
        for dtype in (torch.int64, torch.int32):
            t = torch.randint(-2**31, 2**31 - 1, shape, generator=g, dtype=torch.int64).to(dtype)
            got = _to_device(t, dev)
            assert got.device == dev and got.dtype == torch.int64 and got.shape == t.shape
            assert torch.equal(got.cpu(), t.to(torch.int64))
    big = torch.tensor([2**62 + 12345, -2**62 - 6789, 0])
    assert torch.equal(_to_device(big, dev).cpu(), big)
    on_dev = torch.arange(10, device=dev)
    assert _to_device(on_dev, dev).data_ptr() == on_dev.data_ptr()


def test_aed_exits_in_lockstep_match_the_exit_by_exit_search():
    """The exits of one utterance decoded together (eec_decoder_step_multi: every launch covers all sessions;
    BeamInference.beam_search_exits / decode_all_exits) against the same searches run exit by exit: a group step returns
    what the sessions return one at a time (to fp32 summation order: the tiling follows the group size), the searches return
    the same beams; the lockstep declines (None)
    when EOS could finalise beams."""
    import os
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    from early_exit_transformer_amd.beam import BeamInference
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    kw = eval(str(z["kwargs"]))
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=int(z["n_dec_layers"]), **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    fc = fc.cuda()
    E = kw["n_enc_exits"]
    g = torch.Generator().manual_seed(5)
    encs = [torch.randn(1, 45, kw["d_model"], generator=g).cuda() for _ in range(E)]
    exits = list(range(1, E + 1))
    # group step == single steps
    group = fc.decoder_session_group(encs, exits, 6)
    singles = [fc.decoder_session(encs[e], exits[e], 6) for e in range(E)]
    assert group is not None
    tok = torch.full((E, 1), 1, dtype=torch.long, device="cuda")
    parent = None
    for s in range(6):
        got = group.step(tok, parent)
        for e in range(E):
            want = singles[e].step(tok[e], None if parent is None else parent[e])
            assert (got[e] - want).abs().max().item() < 2e-6 * max(10.0, want.abs().max().item()), (s, e)  # other tiling, fp32 order
        R = 7 if s % 2 == 0 else 4
        parent = torch.randint(0, tok.size(1), (E, R), generator=g).cuda()
        tok = torch.randint(3, 256, (E, R), generator=g).cuda()
    # searches
    inf = BeamInference()
    args = dict(vocab_size=256, max_length=11, SOS_token=1, EOS_token=2, PAD_token=126, beam_size=10, pen_alpha=0.6)
    together = inf.beam_search_exits(fc, encs, exits, **args)
    assert together is not None and len(together) == E
    for e in range(E):
        ta, sa, ba = inf.beam_search(fc, encs[e], exits[e], **args)
        tb, sb, bb = together[e]
        sa_, sb_ = torch.stack(sa).cpu(), torch.stack(sb).cpu()
        assert (sa_.sort().values - sb_.sort().values).abs().max().item() < 1e-4
        gaps = (sa_.sort().values[1:] - sa_.sort().values[:-1]).abs().min().item()
        if gaps > 1e-3:
            assert [t.tolist() for t in ta] == [t.tolist() for t in tb] and ba == bb, e
    assert inf.beam_search_exits(fc, encs, exits, **dict(args, min_length=3)) is None  # EOS could finalise beams: exit by exit
    # decode_all_exits takes the lockstep by itself and agrees with the exit-by-exit path
    spec = torch.rand(80, 131, generator=g).cuda() * 3
    vlen = torch.tensor(131)
    kw2 = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=0.6, max_length=9)
    a = inf.decode_all_exits(fc, spec, vlen, beam_size=5, **kw2)
    b = inf.decode_all_exits(fc, spec, vlen, beam_size=5, kv_cache=False, **kw2)
    assert len(a) == E and sum(x == y for x, y in zip(a, b)) >= E - 1  # a near-tie may flip one search


def test_aed_beam_search_golden():
    """inference.py:18-62 (evaluate_batch_ae) end to end on the product: ONE HIP encoder run for all exits, the HIP
    decoder (eec_decoder_forward) per step, BeamInference.beam_search (beam 10) on the device.  Fixture: the reference's
    full_conformer on CPU driven by its beam-search algorithm restated with its own loops (make_golden.aed_beam_search).
    Candidates near the beam boundary can swap under 1e-3 log-prob noise, so the final scores are compared as sorted
    values, and the best token sequence wherever its score leads the runner-up by a safe margin."""
    import os
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    from early_exit_transformer_amd.beam import BeamInference
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    kw = eval(str(z["kwargs"]))
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=int(z["n_dec_layers"]), **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    fc = fc.cuda()
    inf = BeamInference()
    best_checked = 0
    for i, (T, seed) in enumerate(eval(str(z["cases"]))):
        mel, length = synth.synth_mel(1, 80, T, seed=seed)[0].cuda(), torch.tensor(T)
        taps = fc._run_encoder(mel.unsqueeze(0), length.reshape(1), want_out=False, want_taps=True, n_groups=kw["n_enc_exits"])[1]
        for n in range(1, kw["n_enc_exits"] + 1):
            ft, fs, best = inf.beam_search(fc, taps[n - 1], n, vocab_size=256, max_length=G.aed_max_length(T), SOS_token=1,
                                           EOS_token=2, PAD_token=126, beam_size=10, pen_alpha=1.0)
            got = torch.stack(fs).cpu().numpy()
            want = z[f"beam_scores{i}"][n - 1]
            assert np.abs(np.sort(got) - np.sort(want)).max() < 2e-2, (i, n)
            order = np.argsort(-want)
            if want[order[0]] - want[order[1]] > 2e-2:
                assert best == z[f"beam_best{i}"][n - 1].tolist(), (i, n)
                best_checked += 1
        all_best = inf.decode_all_exits(fc, mel, length, beam_size=10, vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=1.0)
        assert len(all_best) == kw["n_enc_exits"] and all(len(b) == 1 + G.aed_max_length(T) for b in all_best)
    assert best_checked >= 6, best_checked


def _product_rank(rank, world, port, q):
    import os
    import torch.distributed as dist
    from early_exit_transformer_amd import parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)  # both ranks share the one GPU of this box: gloo, not RCCL
    try:
        kw = base_kwargs(n_enc_exits=3, n_enc_layers=1, d_feed_forward=256)
        gpu = Early_conformer(**{**kw, "device": "cuda"}).eval()
        gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=3, style="trained"))
        gpu = gpu.cuda()
        B, T = 5, 259  # uneven shards: 3 + 2
        mel, lens = synth.synth_mel(B, 80, T, seed=3), torch.tensor([259, 200, 131, 259, 77])
        tgt, tl = synth.synth_targets(B, 12, 256, seed=3)
        lo, hi = parallel.shard_range(B, rank, world)
        with torch.no_grad():
            local = exit_ctc_losses(gpu(mel[lo:hi].cuda(), lens[lo:hi]), tgt[lo:hi], tl[lo:hi])
            combined = parallel.combine_exit_losses(local.cpu(), hi - lo)
            if rank == 0:
                full = exit_ctc_losses(gpu(mel.cuda(), lens), tgt, tl).cpu()
                q.put((combined.tolist(), full.tolist()))
    finally:
        dist.destroy_process_group()


def test_world2_product_path_sharded_exit_loss():
    """SURVEY 8e on the PRODUCT path: two ranks (sharing this box's one GPU, so the exchange runs over gloo), each the
    drop-in module + exit_ctc_losses on its utterance shard, combined by parallel.combine_exit_losses, against the
    single-process full batch."""
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_product_rank, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    combined, full = q.get(timeout=300)
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert combined == pytest.approx(full, rel=1e-5, abs=1e-5)


# ---------------------------------------------------------------------------
# d_model = 512 (BASELINE.json configs[2]: 18 layers, 8 heads -> head dim 64): the 32-row tile geometry
# ---------------------------------------------------------------------------
D512 = dict(d_model=512, n_head=8)


@pytest.mark.parametrize("prec", ["f16f8", "f16x3", "f16"])
def test_d512_every_substep_against_oracle(prec):
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=2, d_feed_forward=512, **D512)
    ref, gpu = make_pair(kw, seed=41)
    mel, lens = synth.synth_mel(3, 80, 203, seed=41), torch.tensor([203, 150, 99])
    with torch.no_grad():
        steps = R.trace_substeps(ref, mel, lens)
    gpu.precision = prec
    for k, want in enumerate(steps):
        with torch.no_grad():
            x = gpu._run_encoder(mel.cuda(), lens, want_out=False, stop_after=k, want_x=True)[2].cpu()
        scale = want.abs().max().item()
        err = (x - want).abs().max().item()
        assert err < {"f16x3": 2e-4, "f16f8": 4e-4, "f16": 2e-3}[prec] * max(scale, 1.0), f"sub-step {k}: {err:.3e} (scale {scale:.2f})"


@pytest.mark.parametrize("prec", ["f16f8", "f16x3", "mixed", "f16"])
def test_d512_fused_plan_equals_substep_plan(prec):
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=3, d_feed_forward=640, **D512)  # 5 chunks of 128
    _, gpu = make_pair(kw, seed=42)
    mel, lens = synth.synth_mel(5, 80, 403, seed=42), torch.tensor([403, 402, 300, 77, 5])  # M = 495: ragged last tile
    gpu.precision = prec
    with torch.no_grad():
        out_f, _, x_f = gpu._run_encoder(mel.cuda(), lens, want_x=True)
        out_s, _, x_s = gpu._run_encoder(mel.cuda(), lens, stop_after=1 + 4 * 6, want_x=True)
    out_f, x_f, out_s, x_s = out_f.cpu(), x_f.cpu(), out_s.cpu(), x_s.cpu()
    assert torch.isfinite(x_f).all() and torch.isfinite(out_f).all()
    assert (x_f - x_s).abs().max().item() < 2e-5 * max(x_s.abs().max().item(), 1.0)
    assert (out_f - out_s).abs().max().item() < 5e-5


@pytest.mark.parametrize("B,T,lens", [(1, 7, [7]), (1, 131, [131]), (5, 403, [403, 402, 300, 77, 5]), (2, 1100, [1100, 640]),
                                      (4, 61, [1, 8, 61, 3])])
def test_d512_ragged_shapes(B, T, lens):
    kw = base_kwargs(n_enc_exits=2, n_enc_layers=1, d_feed_forward=256, **D512)
    ref, gpu = make_pair(kw, seed=43)
    mel, lt = synth.synth_mel(B, 80, T, seed=43), torch.tensor(lens)
    with torch.no_grad():
        want = ref(mel, lt)
    for prec in ("f16f8", "f16x3"):
        got = run_gpu(gpu, mel, lt, prec)
        assert got.shape == want.shape
        assert (got - want).abs().max().item() < TOL[prec], prec
        assert torch.allclose(got.exp().sum(-1), torch.ones(got.shape[:-1]), atol=1e-4)


@pytest.mark.parametrize("over", [dict(n_head=16), dict(depthwise_kernel_size=7), dict(d_feed_forward=96), dict(dec_voc_size=96),
                                  dict(features_length=48)])
def test_d512_config_surface(over):
    kw = base_kwargs(**{**dict(n_enc_exits=2, n_enc_layers=1, d_feed_forward=256, **D512), **over})
    ref, gpu = make_pair(kw, seed=44)
    nm = kw["features_length"]
    mel, lens = synth.synth_mel(2, nm, 179, seed=44), torch.tensor([179, 120])
    with torch.no_grad():
        want = ref(mel, lens)
    assert (run_gpu(gpu, mel, lens, "f16x3") - want).abs().max().item() < TOL["f16x3"]


class TestConfig3FullSize:
    """BASELINE.json configs[2] geometry at full size: 6 exits x 3 layers, d_model 512, B = 64, T = 1027 -> T' = 256
    (forward + fused per-exit CTC losses on HIP); size-independent properties + a subset against the oracle."""

    @pytest.fixture(scope="class")
    def setup(self):
        kw = base_kwargs(n_enc_layers=3, **D512)
        ref, gpu = make_pair(kw, seed=5, style="trained")
        mel = synth.synth_mel(64, 80, 1027, seed=5)
        lens = synth.synth_lengths(64, 1027, seed=5)
        out = run_gpu(gpu, mel, lens)
        return ref, gpu, mel, lens, out

    def test_normalised_finite_deterministic(self, setup):
        _, gpu, mel, lens, out = setup
        assert out.shape == (6, 64, 256, 256) and torch.isfinite(out).all()
        assert torch.allclose(out.exp().sum(-1), torch.ones(6, 64, 256), atol=2e-4)
        assert torch.equal(run_gpu(gpu, mel, lens), out)

    def test_utterances_are_independent(self, setup):
        _, gpu, mel, lens, out = setup
        assert torch.equal(run_gpu(gpu, mel[40:44], lens[40:44]), out[:, 40:44])

    def test_subset_against_oracle(self, setup):
        ref, gpu, mel, lens, out = setup
        idx = [0, 17, 63]
        with torch.no_grad():
            want = ref(mel[idx], lens[idx])
        assert (out[:, idx] - want).abs().max().item() < TOL[DEFAULT_MODE]
        got3 = run_gpu(gpu, mel, lens, "f16x3")
        assert (got3[:, idx] - want).abs().max().item() < TOL["f16x3"]

    def test_fused_exit_losses(self, setup):
        _, _, _, _, out = setup
        tgt, tl = synth.synth_targets(64, 42, 256, seed=5)
        got = exit_ctc_losses(out.cuda(), tgt, tl).cpu()
        want = torch.stack([R.summed_exit_ctc_loss(out[e:e + 1], tgt, tl) for e in range(6)])
        assert torch.allclose(got, want, rtol=2e-5, atol=2e-5)


# ---------------------------------------------------------------------------
# First backward slice (BASELINE.json configs[2]-[3]; reference train.py:53-70): CTC gradient + exit-head backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("E,B,T,V,S", [(3, 4, 50, 32, 12), (6, 5, 256, 256, 42), (2, 3, 33, 64, 1), (1, 2, 300, 256, 150),
                                       (2, 2, 10, 32, 12), (2, 6, 97, 256, 70)])
def test_ctc_gradient_matches_torch_autograd(E, B, T, V, S):
    """d( sum_e w_e * loss_e ) / d logp from eec_ctc_loss_backward against torch autograd through the reference's loop of
    nn.CTCLoss(blank=0, 'mean', zero_infinity=True) calls on the SAME log-probs (train.py:60-68).  Covers repeated
    labels, single-label targets, P = 2 / 4 / 8 states per lane and an infeasible utterance (zeroed gradient)."""
    torch.manual_seed(E * 100 + T)
    logp = torch.log_softmax(torch.randn(E, B, T, V) * 2, -1)
    tgt, tl = synth.synth_targets(B, max(S, 3), V, seed=T) if S >= 3 else (torch.full((B, 1), 5), torch.ones(B, dtype=torch.int64))
    tgt = tgt.clone()
    if S >= 3:
        tgt[0, 2] = tgt[0, 1]
    w = torch.linspace(0.5, 1.5, E)
    ctc = torch.nn.CTCLoss(blank=0, reduction="mean", zero_infinity=True)
    il = torch.full((B,), T, dtype=torch.long)

    def torch_grad(dtype):
        x = logp.detach().clone().to(dtype).requires_grad_(True)
        losses = torch.stack([ctc(x[e].permute(1, 0, 2), tgt, il, tl) for e in range(E)])
        (losses * w.to(dtype)).sum().backward()
        return losses.detach(), x.grad

    want_loss, gw = torch_grad(torch.float64)   # the reference arithmetic, evaluated in fp64
    loss32, g32 = torch_grad(torch.float32)     # what the reference itself returns (fp32 log-space recursion)
    got_in = logp.detach().clone().cuda().requires_grad_(True)
    got_loss = exit_ctc_losses(got_in, tgt, tl)
    (got_loss * w.cuda()).sum().backward()
    assert torch.allclose(got_loss.detach().cpu().double(), want_loss, rtol=2e-5, atol=2e-5)
    g = got_in.grad.cpu().double()
    scale = gw.abs().max().item()
    err, err32 = (g - gw).abs().max().item(), (g32.double() - gw).abs().max().item()
    print(f"\n[ctc grad] E{E} B{B} T{T} V{V} S{S}: max|grad| {scale:.3e}  HIP err {err:.2e}  torch-fp32 err {err32:.2e} (both vs fp64)")
    assert torch.isfinite(g).all()
    # within 1e-5 of the gradient's scale of the exact (fp64) value -- measured 1e-6 .. 5e-7, i.e. 50-500x closer than the
    # reference's own fp32 log-space evaluation (err32), because p(target) and the scaled alphas are carried exactly
    assert err < 1e-5 * scale + 1e-9, (err, err32, scale)
    # the gradient with respect to log-softmax outputs sums to zero over the classes of every frame
    assert g.sum(-1).abs().max().item() < 1e-5 * max(scale, 1e-6) * V


def test_exit_heads_trainable_on_frozen_encoder():
    """train.py:53-70 with the encoder frozen: model.train(), loss = sum of the per-exit CTC losses, loss.backward()
    fills linears.*.grad through the HIP CTC backward + head backward; against the oracle's torch autograd."""
    kw = base_kwargs(n_enc_exits=3, n_enc_layers=1, d_feed_forward=256, drop_prob=0.0)
    ref, gpu = make_pair(kw, seed=23)
    mel, lens = synth.synth_mel(4, 80, 259, seed=23), torch.tensor([259, 200, 131, 77])
    tgt, tl = synth.synth_targets(4, 12, 256, seed=23)
    for m in (ref, gpu):
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith("linears."))
    ref.eval()  # the opt-in shortcut: the frozen encoder runs in eval semantics on both sides (BatchNorm running statistics, no dropout)
    want = R.summed_exit_ctc_loss(ref(mel, lens), tgt, tl)
    want.backward()
    gpu.train()
    gpu.frozen_encoder_eval = True
    out = gpu(mel.cuda(), lens)
    assert out.requires_grad
    loss = exit_ctc_losses(out, tgt, tl).sum()
    loss.backward()
    assert abs(loss.item() - want.item()) < 1e-3 * max(1.0, abs(want.item()))
    for e in range(3):
        for leaf in ("weight", "bias"):
            g = getattr(gpu.linears[e], leaf).grad.cpu()
            gw = getattr(ref.linears[e], leaf).grad
            assert (g - gw).abs().max().item() < 2e-3 * gw.abs().max().item() + 1e-7, (e, leaf)
    # an optimizer step on the heads is picked up by the next forward (the packed copies are re-made)
    with torch.no_grad():
        for lg, lr in zip(gpu.linears, ref.linears):
            lg.weight -= 0.1 * lg.weight.grad
            lg.bias -= 0.1 * lg.bias.grad
            lr.weight.copy_(lg.weight.cpu())  # the same updated heads on both sides
            lr.bias.copy_(lg.bias.cpu())
    gpu.eval()
    with torch.no_grad():
        assert (gpu(mel.cuda(), lens).cpu() - ref(mel, lens)).abs().max().item() < TOL[DEFAULT_MODE]
    # a trainable encoder parameter selects the full training step (tests/test_gpu_train.py)
    gpu.train()
    gpu.conformer[0].conformer_layers[0].ffn1.sequential[1].weight.requires_grad_(True)
    assert gpu(mel.cuda(), lens).requires_grad


def test_mel_frontend_against_oracle():
    """the device front end (exact-fp32 MFMA DFT + mel filters) against the restated torchaudio
    transforms on CPU (oracle/frontend_ref.py: torch.stft + htk filterbank), ragged batch, zero padding after each
    utterance's own frames.  Tolerance: 2e-5 of each FRAME's largest mel value (both sides are fp32 transforms: a bin
    that is 1e6 below the frame's peak is not resolved by either) and 1e-4 relative on the values that matter."""
    from early_exit_transformer_amd.frontend import MelFrontend
    from oracle import frontend_ref as FR
    g = torch.Generator().manual_seed(7)
    B, L = 5, 23457
    lens = torch.tensor([L, 16000, 9999, 513, 800])  # torch.stft (reflect) needs more than n_fft // 2 = 512 samples
    t = torch.arange(L) / 16000.0
    wave = 0.3 * torch.randn(B, L, generator=g)
    wave[0] += torch.sin(2 * torch.pi * 440.0 * t) * 3.0        # a loud tone
    wave[1] *= torch.linspace(1e-3, 1.0, L)                     # quiet -> loud
    wave[2] = torch.sign(torch.sin(2 * torch.pi * 100.0 * t))   # square wave: rich harmonics
    for b in range(B):
        wave[b, int(lens[b]):] = 123.0                          # garbage after the valid samples must not be read
    want = FR.mel_frontend_batch(wave, lens)
    fe = MelFrontend()
    got = fe(wave.cuda(), lens).cpu()
    assert got.shape == want.shape == (B, 80, 1 + L // 160)
    for b in range(B):
        Tb = 1 + int(lens[b]) // 160
        assert (got[b, :, Tb:] == 0).all()
        frame_peak = want[b, :, :Tb].amax(dim=0, keepdim=True).clamp_min(1e-30)
        assert ((got[b, :, :Tb] - want[b, :, :Tb]).abs() / frame_peak).max().item() < 2e-5, b
        big = want[b, :, :Tb] > 1e-3 * frame_peak
        assert ((got[b, :, :Tb] - want[b, :, :Tb]).abs()[big] / want[b, :, :Tb][big]).max().item() < 1e-4, b
    single = fe(wave[0].cuda()).cpu()
    assert torch.equal(single, got[0])
    # the encoder takes it as is: [B, 80, T] un-logged power mel
    kw = base_kwargs(n_enc_exits=1, n_enc_layers=1, d_feed_forward=128)
    ref, gpu = make_pair(kw, seed=2)
    mel_len = 1 + lens // 160
    with torch.no_grad():
        w2 = ref(want, mel_len)
    assert (run_gpu(gpu, got, mel_len) - w2).abs().max().item() < TOL[DEFAULT_MODE]


@pytest.mark.parametrize("N,T,V,beam,scale", [(4, 40, 16, 10, 3.0), (6, 256, 256, 10, 4.0), (3, 97, 64, 4, 2.0), (2, 300, 256, 16, 6.0),
                                              (3, 50, 32, 1, 3.0)])
def test_ctc_beam_decode_against_oracle(N, T, V, beam, scale):
    """the device prefix beam search (eec_ctc_beam_decode) against its CPU statement
    (oracle/ctc_beam_ref.py) on the same log-probs: blank-dominated frames (the skip rule), repeats, beam 1 .. 16.
    The kernel works in fp32, the oracle in fp64: the best prefix must be identical whenever the oracle's best final
    score leads its runner-up by a safe margin, and the best score must agree."""
    from early_exit_transformer_amd.model import ctc_beam_decode
    from oracle.ctc_beam_ref import ctc_prefix_beam_search
    g = torch.Generator().manual_seed(N * 1000 + T)
    x = torch.randn(N, T, V, generator=g) * scale
    x[:, :, 0] += scale * 2.0 * (torch.rand(N, T, generator=g) < 0.5)  # about half the frames are blank-dominated (> 0.95)
    x[0, 5:9] = x[0, 5:6]                                                # a run of identical frames
    logp = torch.log_softmax(x, -1)
    tok, cnt, sc = ctc_beam_decode(logp.cuda(), beam_size=beam)
    tok, cnt, sc = tok.cpu(), cnt.cpu(), sc.cpu()
    checked = 0
    for n in range(N):
        want, wscore, final = ctc_prefix_beam_search(logp[n].numpy(), beam=beam, return_beams=True)
        assert abs(float(sc[n]) - wscore) < 2e-3 * max(1.0, abs(wscore)), (n, float(sc[n]), wscore)
        if len(final) < 2 or final[0][1] - final[1][1] > 5e-3:
            assert tok[n, : int(cnt[n])].tolist() == want, n
            checked += 1
    assert checked >= (N + 1) // 2
    # the other reading of the third-party decoder's skip rule (frames above the threshold are dropped), same comparison
    tok2, cnt2, sc2 = ctc_beam_decode(logp.cuda(), beam_size=beam, skip_drops_frame=True)
    tok2, cnt2, sc2 = tok2.cpu(), cnt2.cpu(), sc2.cpu()
    checked2 = 0
    for n in range(N):
        want, wscore, final = ctc_prefix_beam_search(logp[n].numpy(), beam=beam, return_beams=True, skip_drops_frame=True)
        assert abs(float(sc2[n]) - wscore) < 2e-3 * max(1.0, abs(wscore)), (n, float(sc2[n]), wscore)
        if len(final) < 2 or final[0][1] - final[1][1] > 5e-3:
            assert tok2[n, : int(cnt2[n])].tolist() == want, n
            checked2 += 1
    assert checked2 >= (N + 1) // 2
    # greedy is the beam-1 search without merging: on peaky frames both agree with the arg-max path
    if beam == 1:
        g_tok, g_cnt = greedy_ctc(torch.log_softmax(x * 10, -1).cuda())
        b_tok, b_cnt, _ = ctc_beam_decode(torch.log_softmax(x * 10, -1).cuda(), beam_size=4, blank_skip_threshold=1.0)
        for n in range(N):
            assert g_tok[n, : int(g_cnt[n])].tolist() == b_tok[n, : int(b_cnt[n])].tolist()
