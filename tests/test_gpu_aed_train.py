"""The AED decoder's training step (csrc/decoder_train.hip, eec_decoder_train_forward / _backward, behind model._decode_one in train
mode) against an fp64 oracle at the kernel paths the benchmark's geometry runs (cases, oracle and the restated path rules:
tests/aed_train_cases.py; what this rests on: tests/test_host_aed_train.py).  Run with -m gpu on an MI355X.

Bounds: those of the project (header of tests/test_gpu_train.py).  decoder_passes = 3 (bf16x3): logits 2e-4 max(1, max |logit|),
every parameter gradient 2e-3 of its largest entry (compare_grads), the gradient of the encoder output 2e-3 of its largest entry;
decoder_passes = 1 (plain bf16): 5e-2 and 0.15.  The peaky cases multiply every attention score by 4 (16): a bf16x3 product is
relative, so a score's absolute error -- and with it the error of the probabilities -- grows with the score; their bounds are the
plain ones x 4 (x 16).  The dropout cases keep the bounds of test_decoder_training_step_with_dropout_matches_masked_reference_modules.

EEC_TRAIN_NO_SIDE is read by the encoder's training step alone (csrc/train.hip); the decoder's step runs on one stream and never
reads it, so the same-bits test runs with it unset only.

relu' at the kink (aed_train_cases, "the oracle at the kink of the ReLU"): the device's pre-activations of every feed-forward are
read from the workspace of a direct forward and held to the oracle's within 2e-4 max(1, max |pre|); for the few units the device
put on the other side of zero the oracle's backward takes the device's relu'.  Without that the gradient is compared across a
discontinuity: bracketed below is the parameter-gradient figure against the plain oracle and the number of such units (both exits).

Measured on an MI355X, worst error as a fraction of the asserted bound (logits / parameter gradients / grad_enc), worse exit:
  bench_paths  0.042 / 0.008 / 0.009  (plain oracle 9.3; 4 + 5 of 4.3 M units)     long       0.062 / 0.012 / 0.009  (4.8; 1 + 0 of 52 k)
  edges_S1     0.060 / 0.014 / 0.006  (the same; 0)                                edges_S2   0.039 / 0.008 / 0.006  (the same; 0)
  edges_S33    0.044 / 0.014 / 0.007  (the same; 0)                                edges_S64  0.051 / 0.010 / 0.006  (the same; 0)
  edges_S65    0.048 / 0.008 / 0.008  (the same; 0)                                one_key    0.060 / 0.007 / 0.005  (the same; 0), zeros exact
  deep_wide    0.071 / 0.013 / 0.007  (29.8; 1 + 2 of 258 k)                       max_geo    0.046 / 0.006 / 0.006  (the same; 0)
  odd_D        0.042 / 0.006 / 0.007  (the same; 0)                                max_len    0.040 / 0.010 / 0.006  (the same; 0)
  wgrad_128    0.044 / 0.009 / 0.007  (4.9; 1 + 6 of 2.1 M)
  peaky_x1     0.050 / 0.009 / 0.007  (33.5; 1 + 0 of 97 k)
  peaky_x4     0.017 / 0.004 / 0.003 of the x 4 bounds = 0.068 / 0.016 / 0.012 of the plain ones  (1.4 of x 4; 1 + 0)
  peaky_x16    0.025 / 0.016 / 0.020 of the x 16 bounds = 0.40 / 0.26 / 0.32 of the plain ones  (1.5 of x 16; 1 + 1)
  The peaky cases stay inside the PLAIN bounds: the error does grow with the score (x 6 on logits, x 30 on gradients from scale 1
  to 16), by less than the factor the bounds allow.
  plain bf16 (5e-2 / 0.15, plain oracle)   bench_paths 0.085 / 0.449 / 0.120   long 0.138 / 0.757 / 0.303
  drop_prob 0.1                            bench_paths 0.040 / 0.008 / 0.005 (8 + 10 units)   long 0.050 / 0.009 / 0.009 (1 + 0)
Same bits, direct calls (NaN-filled gradients, guard bands, tape unchanged by a second forward) and the refusals: passed as written.
"""
import copy
import ctypes as C

import pytest
import torch

import aed_train_cases as A
import dropout_cases as DC
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.model import full_conformer
from oracle import masked_ref
from test_gpu_train import compare_grads

pytestmark = pytest.mark.gpu


def _gpu_model(case, passes=3, drop=0.0):
    gpu = full_conformer(**A.model_kwargs(case, "cuda", drop))
    gpu.load_state_dict(A.state_dict(case), strict=True)
    gpu = gpu.cuda().train()
    gpu.decoder_passes = passes
    return gpu


def _device_step(gpu, case, idx, seed=None, keep_on_device=False):
    """One forward + backward of exit ``idx`` through the autograd path -> A.Step (float64 on the host unless ``keep_on_device``)."""
    trg, enc, w = A.inputs(case)
    e = enc.cuda().requires_grad_(True)
    gpu.zero_grad(set_to_none=True)
    got = gpu._decode_one(trg.cuda(), e, idx, seed=seed)
    assert got.requires_grad and tuple(got.shape) == tuple(w.shape)
    (got * w.cuda()).sum().backward()
    conv = (lambda t: t.detach().clone()) if keep_on_device else (lambda t: t.detach().cpu().double())
    return A.Step(conv(got), {n: conv(p.grad) for n, p in gpu.named_parameters() if p.grad is not None}, conv(e.grad))


def _check(case, got, want, label, factor=1.0, tol_logit=2e-4, tol_grad=2e-3):
    """Prints the fractions of the three bounds, then asserts them (x ``factor``); returns the fractions."""
    assert set(got.grads) == set(want.grads), sorted(set(got.grads) ^ set(want.grads))[:5]
    assert torch.isfinite(got.logits).all() and torch.isfinite(got.grad_enc).all()
    fl, fg, fe = A.fractions(got, want, factor, tol_logit, tol_grad)
    print(f"\n[{label}] error / bound: logits {fl:.3f}, parameter gradients {fg:.3f}, grad_enc {fe:.3f} "
          f"(max |logit| {want.logits.abs().max().item():.1f}, bounds x {factor:g})")
    assert fl < 1.0, (label, "logits", fl)
    compare_grads(got.grads, want.grads, tol_grad * factor, label)
    assert fe < 1.0, (label, "gradient of the encoder output", fe)
    # tokens that do not occur contribute nothing: their embedding rows get an exact zero, not an unwritten value
    used = torch.zeros(case.geo[7], dtype=torch.bool)
    used[A.inputs(case)[0].unique()] = True
    assert not got.grads["emb.weight"][~used].any(), (label, "embedding rows of absent tokens")
    return fl, fg, fe


# ---- the C ABI directly: every output inside guard bands, the workspace readable -------------------------------------------------
GUARD = 1 << 16  # bytes in front of and behind every output
SENTINEL = -1234.5


def _guarded(n, fill, dev):
    """A float tensor of n elements inside a larger allocation whose bands hold SENTINEL: (inner view, whole buffer)."""
    g = GUARD // 4
    buf = torch.full((g + n + g,), SENTINEL, dtype=torch.float32, device=dev)
    buf[g:g + n] = fill
    return buf[g:g + n], buf


def _bands_intact(buf, n):
    g = GUARD // 4
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[g + n:] == SENTINEL).all())


class _Direct:
    """Exit ``idx`` of ``gpu`` through eec_decoder_train_forward / _backward, every output inside guard bands."""

    def __init__(self, gpu, case, idx=1, seed=7):
        self.lib, self.gpu, self.case, self.idx = capi.load(), gpu, case, idx
        self.settings = dict(passes=int(gpu.decoder_passes), drop_prob=float(gpu.dropout), seed=int(seed))
        B, S, Tq, L, D, H, F, V, pad = case.geo
        self.dev = torch.device("cuda", torch.cuda.current_device())
        trg, enc, w = A.inputs(case)
        self.trg, self.enc, self.w = trg.cuda(), enc.cuda(), w.cuda()
        self.tensors = dict(gpu._decoder_named_params(idx))
        self.ps, self._keep = gpu._decoder_struct(idx, self.tensors, with_pe=True)
        self.nbytes = self.lib.eec_decoder_train_workspace_bytes(D, H, F, V, L, B, S, Tq)
        assert self.nbytes > 0
        self.ws_buf = torch.full((GUARD + self.nbytes + 256 + GUARD,), 0xA5, dtype=torch.uint8, device=self.dev)
        self.ws_ptr = (self.ws_buf.data_ptr() + GUARD + 255) // 256 * 256
        self.ws_off = self.ws_ptr - self.ws_buf.data_ptr()
        self.out, self.out_buf = _guarded(B * S * V, float("nan"), self.dev)
        self.g_enc, self.g_enc_buf = _guarded(B * Tq * D, float("nan"), self.dev)
        self.grads = {k: torch.full_like(v, float("nan")) for k, v in self.tensors.items()}
        self.gs, self._gkeep = gpu._decoder_struct(idx, self.grads, with_pe=False)

    def workspace(self):
        return self.ws_buf[self.ws_off: self.ws_off + self.nbytes]

    def forward_args(self, **over):
        B, S, Tq, L, D, H, F, V, pad = self.case.geo
        a = dict(p=C.byref(self.ps), d_model=D, n_heads=H, d_ff=F, vocab=V, pad_idx=pad, trg=self.trg, enc=self.enc, Bm=B, S=S, Tq=Tq,
                 **self.settings, exit_index=self.idx, out=self.out, ws=self.ws_ptr, ws_bytes=self.nbytes)
        a.update(over)
        return list(a.values())

    def backward_args(self, **over):
        B, S, Tq, L, D, H, F, V, pad = self.case.geo
        a = dict(p=C.byref(self.ps), grads=C.byref(self.gs), d_model=D, n_heads=H, d_ff=F, vocab=V, trg=self.trg, enc=self.enc, Bm=B, S=S, Tq=Tq,
                 **self.settings, exit_index=self.idx, grad_out=self.w, grad_enc=self.g_enc, ws=self.ws_ptr, ws_bytes=self.nbytes)
        a.update(over)
        return list(a.values())

    def forward(self):
        capi.launch("eec_decoder_train_forward", self.dev, *self.forward_args())

    def backward(self):
        capi.launch("eec_decoder_train_backward", self.dev, *self.backward_args())

    def bands_intact(self):
        torch.cuda.synchronize()
        ws_ok = bool((self.ws_buf[: self.ws_off] == 0xA5).all()) and bool((self.ws_buf[self.ws_off + self.nbytes:] == 0xA5).all())
        return ws_ok and _bands_intact(self.out_buf, self.out.numel()) and _bands_intact(self.g_enc_buf, self.g_enc.numel())


def _device_relu_choice(d, pre64, label):
    """relu' as the device took it, bool [B S, d_ff] per layer: the forward of ``d`` records every layer's pre-activations in its
    workspace (256-byte aligned blocks), which are found there by their values -- the one block that equals the oracle's ``pre64``
    within A.kink_band everywhere -- so nothing of the tape's layout is restated.  That match is the forward held to the oracle
    at the feed-forward's input; it admits another sign than the oracle's only inside the band around zero."""
    rows = d.workspace().view(torch.float32).view(-1, 64)
    alive, flipped = [], 0
    for l, p in enumerate(pre64):
        band, n = A.kink_band(p), p.numel()
        assert n >= 64
        ref = p.flatten().float().cuda()
        near = ((rows - ref[:64]).abs().amax(dim=1) <= band).nonzero().flatten().tolist()
        hits = [r for r in near if r * 64 + n <= rows.numel() and bool(((rows.view(-1)[r * 64: r * 64 + n] - ref).abs() <= band).all())]
        assert len(hits) == 1, (label, l, "the layer's pre-activations, within the forward bound of the oracle's, were found this often", len(hits))
        dev = rows.view(-1)[hits[0] * 64: hits[0] * 64 + n].view(p.shape).cpu()
        alive.append(dev > 0)
        other = alive[-1] != (p > 0)
        assert bool((p[other].abs() <= band).all())
        flipped += int(other.sum())
    return alive, flipped


def _direct_forward(gpu, case, idx, pre64, label, seed=7):
    """One forward of exit ``idx`` through the C ABI: (logits, relu' as the device took it per layer, units where it is not the oracle's)."""
    d = _Direct(gpu, case, idx, seed)
    d.forward()
    assert d.bands_intact()
    alive, flipped = _device_relu_choice(d, pre64, label)
    B, S, _, _, _, _, _, V, _ = case.geo
    return d.out.clone().view(B, S, V), alive, flipped


@pytest.mark.parametrize("cid", A.IDS)
def test_decoder_training_step_against_the_fp64_oracle(cid):
    """Every case, both exits, bf16x3: logits, the gradient of every decoder parameter (embedding table and shared final LayerNorm
    included) and of the encoder output.  The device's pre-activations of every feed-forward are held to the oracle's within the
    forward bound; where the device put one on the other side of zero, the oracle's backward takes the device's relu' (see
    aed_train_cases: the oracle at the kink of the ReLU).  The error against the plain oracle is printed beside it."""
    case = A.BY_ID[cid]
    gpu = _gpu_model(case)
    worst = (0.0, 0.0, 0.0)
    for idx in (1, 0):
        label = f"{cid} exit {idx} bf16x3"
        out, alive, flipped = _direct_forward(gpu, case, idx, A.oracle_pre_activations(case, idx), label)
        got, plain = _device_step(gpu, case, idx), A.oracle(case, idx)
        assert torch.equal(out.cpu().double(), got.logits), "the C entry and the autograd path disagree"
        want = A.oracle_with_relu_choice(case, idx, alive) if flipped else plain
        assert torch.equal(want.logits, plain.logits)
        fp = A.fractions(got, plain, A.PEAKY_FACTOR.get(cid, 1.0))
        print(f"\n[{label}] {flipped} of {sum(a.numel() for a in alive)} pre-activations on the other side of zero; against the oracle's own relu': "
              f"logits {fp[0]:.3f}, parameter gradients {fp[1]:.3f}, grad_enc {fp[2]:.3f}")
        worst = tuple(max(a, b) for a, b in zip(worst, _check(case, got, want, label, A.PEAKY_FACTOR.get(cid, 1.0))))
        if cid == "one_key":  # p = 1 and g - dot = 0 exactly on the device too
            zeros = A.one_key_zero_slices(got.grads, case.geo[4])
            assert len(zeros) == 4 * case.geo[3]
            for n, g in zeros:
                assert not g.any(), (n, g.abs().max().item())
    print(f"[{cid}] worst of both exits: {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f}")


@pytest.mark.parametrize("cid", ["bench_paths", "long"])
def test_decoder_training_step_in_plain_bf16(cid):
    """decoder_passes = 1: the project's bf16 bounds, 5e-2 for logits and 0.15 for gradients."""
    case = A.BY_ID[cid]
    gpu = _gpu_model(case, passes=1)
    for idx in (1, 0):
        _check(case, _device_step(gpu, case, idx), A.oracle(case, idx), f"{cid} exit {idx} bf16", tol_logit=5e-2, tol_grad=0.15)


def test_a_second_step_returns_the_same_bits(monkeypatch):
    """No atomics and a fixed summation order: the same inputs give bit-identical logits and gradients (bench_paths: 33 and 65
    weight-gradient partials, the 128 x 128 batched tile, 2112 tokens per embedding row walk)."""
    monkeypatch.delenv("EEC_TRAIN_NO_SIDE", raising=False)
    case = A.BY_ID["bench_paths"]
    gpu = _gpu_model(case)
    first = _device_step(gpu, case, 1, keep_on_device=True)
    for rep in range(2):
        again = _device_step(gpu, case, 1, keep_on_device=True)
        assert torch.equal(again.logits, first.logits) and torch.equal(again.grad_enc, first.grad_enc), rep
        bad = [n for n in first.grads if not torch.equal(again.grads[n], first.grads[n])]
        assert not bad, (rep, bad[:4])


@pytest.mark.parametrize("cid", A.DROPOUT_IDS)
def test_decoder_training_step_with_dropout_at_the_new_paths(cid):
    """drop_prob 0.1 with DC.DECODER_SEED against oracle.masked_ref.masked_decoder_logits (float64, masks at
    documented_decoder_site), as test_decoder_training_step_with_dropout_matches_masked_reference_modules does and with its bounds:
    the epi 5 / epi 6 / residual mask indexing of the 128 x 64 tile and the probability masks of 65- to 257-key rows against
    supplied masks.  (The masked oracle of bench_paths takes 0.3 s on the CPU: both cases are kept.)  relu' at the kink as in
    test_decoder_training_step_against_the_fp64_oracle."""
    case = A.BY_ID[cid]
    L = case.geo[3]
    cpu = copy.deepcopy(A.cpu_model(case)).double()
    gpu = _gpu_model(case, drop=DC.DECODER_P)
    assert gpu.dropout == DC.DECODER_P
    trg, enc, w = A.inputs(case)
    for idx in (1, 0):
        label = f"{cid} exit {idx} drop_prob {DC.DECODER_P} bf16x3"
        sites = [DC.documented_decoder_site(idx, l, 0) for l in range(L)]

        def masked(e, record=None):
            return masked_ref.masked_decoder_logits(cpu, trg, e, idx, record or masked_ref.Masks(DC.DECODER_SEED, DC.DECODER_P), 0, sites)

        pre64 = A.pre_activations(cpu, lambda: masked(enc.double()))
        out, alive, flipped = _direct_forward(gpu, case, idx, pre64, label, seed=DC.DECODER_SEED)
        for layer, a in zip(cpu.decoders[idx].layers, alive):  # the device's relu' where it differs; relu' itself everywhere else
            layer.activation = A.relu_with_choice(a)
        e_ref = enc.double().requires_grad_(True)
        masks = masked_ref.Masks(DC.DECODER_SEED, DC.DECODER_P)
        cpu.zero_grad(set_to_none=True)
        logits = masked(e_ref, masks)
        (logits * w.double()).sum().backward()
        assert sorted(masks.used) == sorted(s for s in A.dropout_sites(case) if s[0] == 0 or (s[0] - 1) // 1024 == idx)
        want = A.Step(logits.detach(), {n: p.grad.detach().clone() for n, p in cpu.named_parameters() if p.grad is not None}, e_ref.grad)
        assert (want.logits - A.oracle(case, idx).logits).abs().max().item() > 1e-2, "the masks changed nothing"
        got = _device_step(gpu, case, idx, seed=DC.DECODER_SEED)
        assert torch.equal(out.cpu().double(), got.logits), "the C entry and the autograd path disagree"
        print(f"\n[{label}] {flipped} of {sum(a.numel() for a in alive)} pre-activations on the other side of zero")
        _check(case, got, want, label)


# ---- the C ABI directly: tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["bench_paths"] + A.EDGES_S)
def test_direct_calls_write_every_gradient_and_stay_inside_their_buffers(cid):
    """decoding._DecoderTrainFn allocates the gradient buffers with torch.empty_like: every element must be written.  Here the
    buffers and grad_enc start as NaN; after the backward none remains and the values equal the autograd path's bit for bit.  out,
    grad_enc and the workspace (eec_decoder_train_workspace_bytes) sit inside larger allocations whose bands keep their sentinel
    through two forwards and the backward, and a second backward-free forward with the same seed leaves the workspace -- the tape
    -- byte for byte as the first did."""
    case = A.BY_ID[cid]
    gpu = _gpu_model(case)
    d = _Direct(gpu, case)
    d.forward()
    assert d.bands_intact(), "the forward left its buffers"
    out1, tape1 = d.out.clone(), d.workspace().clone()
    assert not torch.isnan(out1).any()
    d.out.fill_(float("nan"))
    d.forward()
    assert d.bands_intact()
    assert torch.equal(d.out, out1) and torch.equal(d.workspace(), tape1), "a second forward with the same seed changed the tape"
    d.backward()
    assert d.bands_intact(), "the backward left its buffers"
    assert not torch.isnan(d.g_enc).any(), "grad_enc has unwritten elements"
    unwritten = [k for k, g in d.grads.items() if torch.isnan(g).any()]
    assert not unwritten, unwritten
    auto = _device_step(gpu, case, d.idx, keep_on_device=True)
    B, S, Tq, _, D, _, _, V, _ = case.geo
    assert torch.equal(auto.logits, out1.view(B, S, V)) and torch.equal(auto.grad_enc, d.g_enc.view(B, Tq, D))
    assert set(auto.grads) == set(d.grads)
    bad = [k for k in d.grads if not torch.equal(auto.grads[k], d.grads[k])]
    assert not bad, bad[:4]


def test_refusals_reach_the_error_string_without_a_launch():
    lib = capi.load()
    case = A.BY_ID["max_len"]
    B, S, Tq, L, D, H, F, V, pad = case.geo
    gpu = _gpu_model(case)
    d = _Direct(gpu, case)
    d.out.fill_(5.0), d.g_enc.fill_(5.0)
    for g in d.grads.values():
        g.fill_(5.0)
    few = (capi.EecDecoderLayerParams * (L + 1))()
    other = capi.EecDecoderParams(d.gs.emb, None, few, L + 1, d.gs.max_len, d.gs.norm_w, d.gs.norm_b, d.gs.head_w, d.gs.head_b)
    # the entries ask for tape + scratch bytes; eec_decoder_train_workspace_bytes reports 512 more
    need = d.nbytes - 512

    def refused(entry, **over):
        args = d.forward_args(**over) if entry == "forward" else d.backward_args(**over)
        with pytest.raises(RuntimeError) as err:
            capi.launch("eec_decoder_train_" + entry, d.dev, *args)
        last = lib.eec_decoder_train_last_error().decode()
        assert last and last in str(err.value), (last, str(err.value))
        return last

    for entry in ("forward", "backward"):
        assert "bad geometry" in refused(entry, S=case.max_len + 1)
        assert "bad geometry" in refused(entry, n_heads=H + 1)  # d_model % n_heads != 0
        assert "bad geometry" in refused(entry, vocab=1025)
        assert "bad geometry" in refused(entry, d_model=1088)
        assert "drop_prob in [0, 1)" in refused(entry, drop_prob=1.0)
        assert "passes: 1 (bf16) or 3 (bf16x3)" in refused(entry, passes=2)
        assert "workspace too small" in refused(entry, ws_bytes=need - 1)
        assert "256-byte aligned" in refused(entry, ws=d.ws_ptr + 8)
        assert "null argument" in refused(entry, trg=None)
    assert D % (H + 1) != 0 and 1088 % H == 0 and S == case.max_len
    assert "grads must mirror params" in refused("backward", grads=C.byref(other))
    assert d.bands_intact()  # synchronises
    assert bool((d.out == 5.0).all()) and bool((d.g_enc == 5.0).all()) and all(bool((g == 5.0).all()) for g in d.grads.values())
    assert bool((d.workspace() == 0xA5).all())  # nothing was launched
    capi.launch("eec_decoder_train_forward", d.dev, *d.forward_args(ws_bytes=need))  # exactly what the entry asks for is enough
    torch.cuda.synchronize()
    assert not bool((d.out == 5.0).all()) and torch.isfinite(d.out).all() and d.bands_intact()
