"""Cases, inputs, fp64 oracle and restated path rules shared by tests/test_host_aed_train.py and tests/test_gpu_aed_train.py: the
AED decoder's training step (csrc/decoder_train.hip, eec_decoder_train_forward / _backward, behind model._decode_one in train
mode) at the kernel paths the benchmark's geometry runs.  Everything here is seeded and runs on the CPU; no device code.

A case is (B, S, T', decoder layers, d_model, heads, d_ff, V, pad_idx) plus a padding pattern, a token pattern and, for the peaky
cases, a factor on the query / key rows of every attention.  The oracle is the reference's decoder arithmetic through torch's
modules (conftest.ref_decoder_logits) on a .double() copy of the CPU full_conformer, fed float64 ``enc``; the loss is
``(logits * w).sum()`` with a fixed random ``w`` and torch autograd gives the gradients.

The path rules below are read off the kernels and stated here, not computed from the package:
  launch_gemm (train_kernels.hip)   tile by (M, N, batch count nz), wgs(bm, bn) = ceil(M / bm) ceil(N / bn) nz:
                                    N <= 32: 128 x 32;  N > 64 and wgs(128, 128) >= 512: 128 x 128;  wgs(128, 64) >= 512 or N <= 64:
                                    128 x 64;  wgs(128, 128) >= 384: 128 x 128;  otherwise 64 x 64
  linear_bwd_weight (decoder_train.hip)   dW[N][K] over M rows: tiles = ceil(N / 128) ceil(K / 128), S = max(1, min(512 / tiles,
                                    M / 64)), chunk = ceil(M / S) rounded up to 32, S = ceil(M / chunk); S > 1: S partials of
                                    [N][K] weight gradient + [N] bias gradient (pstride = N K + N), summed by reduce_leading
  reduce_leading_kernel             S <= 32 partials: <4>, otherwise <16>; the LayerNorm backward's partials ([blocks][2][D],
                                    blocks = max(1, min(1024, ceil(M / 8)))) go through the same rule
  softmax_masked_kernel             one wave per row, lane l takes keys l, l + 64, ...: ceil(Tk / 64) trips
  embed_bwd_kernel                  one workgroup per vocabulary row walks all B S tokens; 256 columns per trip: ceil(D / 256) trips
  LayerNorm                         kLnMax = 16 elements per lane: D <= 1024; <4> up to 256, <8> up to 512, <16> beyond

Out of scope: a first token equal to the pad index (the first query row has no live key: NaN in torch as on the device), and tokens
outside [0, V) (the device clamps, nn.Embedding raises).  Every case takes trg[:, 0] = 1.
"""
import copy
import functools
import sys
from typing import NamedTuple, Tuple

import torch
from torch.nn.attention import SDPBackend, sdpa_kernel

from conftest import GOLDEN, ref_decoder_logits
from early_exit_transformer_amd.model import full_conformer

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import aed_fixture  # noqa: E402

SOS = 1
BENCH_GEO = (64, 43, 256, 6, 256, 8, 2048, 256)  # B, S, T', layers, d_model, heads, d_ff, V of bench.py's decoder step
K_LN_MAX = 16


# ---- the path rules ---------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def gemm_tile(M, N, nz=1):
    """The (rows, columns) of the output tile launch_gemm picks."""
    def wgs(bm, bn):
        return _cdiv(M, bm) * _cdiv(N, bn) * nz
    if N <= 32:
        return (128, 32)
    if N > 64 and wgs(128, 128) >= 512:
        return (128, 128)
    if wgs(128, 64) >= 512 or N <= 64:
        return (128, 64)
    if wgs(128, 128) >= 384:
        return (128, 128)
    return (64, 64)


def weight_grad_splits(M, N, K):
    """(splits, rows per split) of linear_bwd_weight for dW[N][K] summed over M rows."""
    tiles = _cdiv(N, 128) * _cdiv(K, 128)
    S = max(1, min(512 // tiles, M // 64))
    chunk = _cdiv(_cdiv(M, S), 32) * 32
    return _cdiv(M, chunk), chunk


def reduce_variant(S):
    """SL of reduce_leading_kernel<SL> for S partials."""
    return 4 if S <= 32 else 16


def ln_bwd_blocks(M):
    return max(1, min(1024, _cdiv(M, 8)))


def softmax_trips(Tk):
    return _cdiv(Tk, 64)


def embed_trips(D):
    return _cdiv(D, 256)


def ln_variant(D):
    assert D <= 64 * K_LN_MAX
    return 4 if D <= 256 else 8 if D <= 512 else 16


class Gemm(NamedTuple):
    name: str
    M: int
    N: int
    K: int
    kind: str    # "single" | "heads" (nz = B H problems) | "splits" (nz = S row chunks of one contraction)
    nz: int
    epi: str     # "none" | "bias" | "accumulate" | "resid" (epi 4) | "relu_drop" (epi 5) | "drelu" (epi 6) | "rowsum" (weight gradient)
    akc: bool    # A is contiguous along the contraction
    bkc: bool    # B is
    tile: Tuple[int, int]
    splits: int  # of a weight gradient; 0 otherwise
    cvec: bool   # the epilogue's 16-byte form: N % 4 == 0 and the row stride of C % 4 == 0

    @property
    def combo(self):
        return (self.tile, self.kind, self.epi, self.akc, self.bkc)


def launches(B, S, Tq, L, D, H, F, V):
    """Every GEMM one forward + backward of the geometry launches, in order, and the (form, SL) of every reduce_leading launch."""
    M, Mk, dh, nz = B * S, B * Tq, D // H, B * H
    gemms, reduces = [], []

    def g(name, m, n, k, kind, z, epi, akc, bkc, c_m, splits=0):
        gemms.append(Gemm(name, m, n, k, kind, z, epi, akc, bkc, gemm_tile(m, n, z), splits, n % 4 == 0 and c_m % 4 == 0))

    def linear_fwd(name, m, n, k, epi="bias"):
        g(name, m, n, k, "single", 1, epi, True, True, n)

    def bwd_data(name, m, n, k, epi="none"):  # dx[M][K] = dy[M][N] . W[N][K]
        g(name, m, k, n, "single", 1, epi, True, False, k)

    def bwd_weight(name, m, n, k):  # the GEMM is [N] x [K] over chunk rows, A = dy^T, B = x^T: neither contiguous along the contraction
        s, chunk = weight_grad_splits(m, n, k)
        if s > 1:
            g(name, n, k, chunk, "splits", s, "rowsum", False, False, k, s)
            reduces.append(("split", reduce_variant(s)))
        else:
            g(name, n, k, m, "single", 1, "rowsum", False, False, k, 1)

    def ln_bwd(m):
        reduces.append(("ln2", reduce_variant(ln_bwd_blocks(m))))

    def attn_fwd(p, Tk):
        g(p + " scores", S, Tk, dh, "heads", nz, "none", True, True, Tk)
        g(p + " ctx", S, dh, Tk, "heads", nz, "none", True, False, D)

    def attn_bwd(p, Tk, kv_m, q_m):
        g(p + " dV", Tk, dh, S, "heads", nz, "none", Tk == 1, False, kv_m)  # A = Pd^T: k stride Tk
        g(p + " dP", S, Tk, dh, "heads", nz, "none", True, True, Tk)
        g(p + " dQ", S, dh, Tk, "heads", nz, "none", True, False, q_m)
        g(p + " dK", Tk, dh, S, "heads", nz, "none", Tk == 1, False, kv_m)

    for _ in range(L):
        linear_fwd("sa in_proj", M, 3 * D, D)
        attn_fwd("sa", S)
        linear_fwd("sa out_proj", M, D, D, "resid")
        linear_fwd("ca q", M, D, D)
        linear_fwd("ca kv", Mk, 2 * D, D)
        attn_fwd("ca", Tq)
        linear_fwd("ca out_proj", M, D, D, "resid")
        linear_fwd("linear1", M, F, D, "relu_drop")
        linear_fwd("linear2", M, D, F, "resid")
    linear_fwd("head", M, V, D)
    bwd_weight("head dW", M, V, D)
    bwd_data("head dX", M, V, D)
    ln_bwd(M)
    for layer in reversed(range(L)):
        bwd_weight("linear2 dW", M, D, F)
        g("dpre", M, F, D, "single", 1, "drelu", True, False, F)
        bwd_weight("linear1 dW", M, F, D)
        bwd_data("linear1 dX", M, F, D)
        ln_bwd(M)
        bwd_weight("ca out_proj dW", M, D, D)
        bwd_data("ca out_proj dX", M, D, D)
        attn_bwd("ca", Tq, 2 * D, D)
        bwd_weight("ca q dW", M, D, D)
        bwd_weight("ca kv dW", Mk, 2 * D, D)
        bwd_data("ca q dX", M, D, D)
        bwd_data("grad_enc", Mk, 2 * D, D, "none" if layer == L - 1 else "accumulate")
        ln_bwd(M)
        bwd_weight("sa out_proj dW", M, D, D)
        bwd_data("sa out_proj dX", M, D, D)
        attn_bwd("sa", S, 3 * D, 3 * D)
        bwd_weight("sa in_proj dW", M, 3 * D, D)
        bwd_data("sa in_proj dX", M, 3 * D, D)
        ln_bwd(M)
    return gemms, reduces


# ---- the cases --------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    id: str
    geo: Tuple[int, int, int, int, int, int, int, int, int]  # B, S, T', layers, d_model, heads, d_ff, V, pad_idx
    pads: Tuple[str, ...] = ()  # "trailing" | "all_after_first" | "middle"; () = no padding at all
    tokens: str = "random"      # "random" | "repeat": the first half of the rows holds ONE token at every position after the first
    qk_scale: float = 1.0       # factor on the query and key rows of every in_proj_weight: scores x qk_scale^2
    max_len: int = 400
    seed: int = 13

    @property
    def launch_geo(self):
        return self.geo[:8]


PEAKY_GEO = (4, 42, 64, 3, 256, 8, 192, 64, 30)  # the (4, 42, 64, 3, 256, 8) case of test_decoder_training_step_matches_reference_modules
CASES = (
    Case("bench_paths", (64, 33, 65, 1, 128, 8, 2048, 64, 30), ("trailing", "all_after_first"), "repeat", seed=21),
    Case("long", (2, 129, 257, 2, 64, 4, 100, 37, 36), ("middle", "trailing"), seed=22),
    *[Case(f"edges_S{S}", (2, S, 9, 1, 64, 4, 96, 64, 30), () if S == 1 else ("all_after_first",) if S == 2 else ("trailing", "middle"),
           seed=30 + S) for S in (1, 2, 33, 64, 65)],
    Case("one_key", (3, 5, 1, 2, 64, 4, 96, 64, 30), ("trailing",), seed=24),
    Case("deep_wide", (3, 7, 31, 6, 512, 8, 2048, 256, 30), ("trailing",), seed=25),
    Case("max_geo", (2, 9, 33, 1, 1024, 16, 64, 1000, 0), ("middle",), seed=26),
    Case("odd_D", (3, 11, 13, 1, 96, 6, 160, 64, 30), (), seed=27),
    Case("max_len", (2, 12, 5, 1, 64, 4, 96, 64, 30), ("trailing",), max_len=12, seed=28),
    # not in the issue's table: the benchmark's key / value weight gradient (64 splits of [512][256]) runs on the 128 x 128 tile, which
    # needs tiles x splits = 512 exactly; the smallest geometry that gets there is 32 tiles ([2048][256]) x 16 splits of 64 rows
    Case("wgrad_128", (16, 64, 9, 1, 256, 8, 2048, 64, 30), ("trailing",), seed=29),
    Case("peaky_x1", PEAKY_GEO, ("trailing",)),
    Case("peaky_x4", PEAKY_GEO, ("trailing",), qk_scale=2.0),
    Case("peaky_x16", PEAKY_GEO, ("trailing",), qk_scale=4.0),
)
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
EDGES_S = [c.id for c in CASES if c.id.startswith("edges_S")]
DROPOUT_IDS = ("bench_paths", "long")
PEAKY_FACTOR = {"peaky_x1": 1.0, "peaky_x4": 4.0, "peaky_x16": 16.0}  # the factor on the plain bounds

# the parameters of ``one_key`` whose gradient is exactly zero: with one key P = 1 and dS = p (g - dot) = 0, so nothing flows into
# the cross-attention's queries and keys, nor through the queries into norm2.  (name suffix, rows: None = all, "qk" = the first 2 D)
ONE_KEY_ZERO = (("multihead_attn.in_proj_weight", "qk"), ("multihead_attn.in_proj_bias", "qk"), ("norm2.weight", None), ("norm2.bias", None))


def one_key_zero_slices(grads, D):
    """(name, tensor) of every slice of ``grads`` that ONE_KEY_ZERO names."""
    out = []
    for n, g in grads.items():
        for suffix, rows in ONE_KEY_ZERO:
            if n.endswith(suffix):
                out.append((n, g[:2 * D] if rows == "qk" else g))
    return out


def targets(case):
    """trg int64 [B, S]: SOS first, random tokens of [3, V) other than the pad index, then the case's padding pattern."""
    B, S, _, _, _, _, _, V, pad = case.geo
    g = torch.Generator().manual_seed(case.seed * 1000 + 1)
    trg = torch.randint(3, V, (B, S), generator=g)
    trg[trg == pad] = 3
    if case.tokens == "repeat":
        trg[: B // 2] = 7
    trg[:, 0] = SOS
    if "trailing" in case.pads:  # another length for every row; row 0 stays whole
        for r in range(1, B):
            n = 1 + (3 * r) % max(S - 2, 1)
            if n < S:
                trg[r, S - n:] = pad
    if "middle" in case.pads and S >= 5:  # padding followed by tokens again: the keys are masked wherever trg == pad
        trg[0, S // 3: S // 3 + 2] = pad
        assert trg[0, S // 3 + 2] != pad
    if "all_after_first" in case.pads:
        trg[B - 1, 1:] = pad
    return trg


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(trg [B, S] int64, enc [B, T', D] fp32, w [B, S, V] fp32).  Read-only: shared between tests."""
    B, S, Tq, _, D, _, _, V, _ = case.geo
    g = torch.Generator().manual_seed(case.seed * 1000 + 2)
    return targets(case), torch.randn(B, Tq, D, generator=g), torch.randn(B, S, V, generator=g)


def model_kwargs(case, device, drop_prob=0.0):
    _, _, _, L, D, H, F, V, pad = case.geo
    return dict(device=device, trg_pad_idx=pad, enc_voc_size=V, max_len=case.max_len, features_length=80, drop_prob=drop_prob, n_dec_layers=L,
                n_enc_exits=2, n_enc_layers=1, d_model=D, n_head=H, d_feed_forward=F, depthwise_kernel_size=7, dec_voc_size=V)


@functools.lru_cache(maxsize=2)
def _cpu_model(case):
    cpu = full_conformer(**model_kwargs(case, "cpu"))
    sd = aed_fixture.aed_state_dict(cpu, case.seed)
    if case.qk_scale != 1.0:
        D = case.geo[4]
        for k in sd:
            if k.startswith("decoders.") and k.endswith("attn.in_proj_weight"):
                sd[k] = sd[k].clone()
                sd[k][:2 * D] *= case.qk_scale
    cpu.load_state_dict(sd, strict=True)
    return cpu.train()  # drop_prob 0: train mode draws nothing


def cpu_model(case):
    """The case's full_conformer on the CPU, fp32, train mode, drop_prob 0.  Shared between calls: copy it before changing it."""
    return _cpu_model(case)


def state_dict(case):
    return {k: v.clone() for k, v in cpu_model(case).state_dict().items()}


class Step(NamedTuple):
    logits: torch.Tensor  # [B, S, V]
    grads: dict           # name -> gradient, every decoder parameter of the exit (embedding and shared layer_norm included)
    grad_enc: torch.Tensor


def reference_step(model, case, idx, dtype):
    """Logits and gradients of exit ``idx`` through the reference's modules held by ``model`` (already of ``dtype``)."""
    trg, enc, w = inputs(case)
    e = enc.to(dtype, copy=True).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    logits = ref_decoder_logits(model, trg, e, idx)
    (logits * w.to(dtype)).sum().backward()
    grads = {n: p.grad.detach().double() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return Step(logits.detach().double(), grads, e.grad.detach().double())


@functools.lru_cache(maxsize=4)
def oracle(case, idx):
    """The float64 oracle of exit ``idx``.  Read-only: shared between tests.  torch's written-out attention (the MATH backend) is
    selected: its softmax backward forms (g - sum g p) p, which is an exact zero where p = 1 (``one_key``); the fused CPU kernel
    recomputes p = exp(s - lse) and leaves 1e-16 of rounding there.  The two agree to 1e-11 of the bounds on every case."""
    with sdpa_kernel(SDPBackend.MATH):
        return reference_step(copy.deepcopy(cpu_model(case)).double(), case, idx, torch.float64)


# ---- the oracle at the kink of the ReLU ---------------------------------------------------------------------------------------------
# The decoder's feed-forward is W2 . relu(W1 . LN3(x)): the gradient is a DISCONTINUOUS function of the pre-activations.  A unit
# whose pre-activation lies within the forward rounding of zero may come out on either side, and relu' is then 0 on one side and
# 1 on the other: the whole contribution of that (row, unit) to every gradient below it appears or vanishes.  That is one row's
# share of a sum over B S rows -- 1 / sqrt(B S) of the gradient's scale, ten times the bound at B S = 2112 -- however small the
# rounding was.  Measured on an MI355X against the plain oracle: every case with B S d_ff layers >= 1e5 pre-activations exceeded
# the gradient bound (bench_paths 9.3, long 4.8, deep_wide 29.8, wgrad_128 1.3, peaky_x1 33.5 times) with logits at 0.04 .. 0.07 of
# theirs, every smaller case sat at 0.006 .. 0.014.  So the comparison is made where it is well posed: the oracle's forward is
# untouched, and its backward takes, for the units the device put on the other side of zero, the device's choice of relu' -- after
# the device's pre-activations were held to the oracle's within the project's forward bound for a bf16x3 GEMM output,
# 2e-4 max(1, max |pre|) (kink_band), which admits a different sign only where |pre| is inside that band.  The bounds on logits and
# gradients stay the project's.
class _ReluWithChoice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alive):
        ctx.save_for_backward(alive)
        return torch.relu(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def kink_band(pre):
    return 2e-4 * max(1.0, pre.abs().max().item())


def relu_with_choice(alive):
    """An ``activation`` for nn.TransformerDecoderLayer: relu forward, ``alive`` (bool, the shape of its input flattened to rows) as relu'."""
    return lambda x: _ReluWithChoice.apply(x, alive.reshape(x.shape).to(x.dtype))


def pre_activations(model, run):
    """The outputs of every layer's linear1 -- [layers of [B S, d_ff]] per decoder in ``model.decoders`` order of use -- during ``run()``."""
    seen, hooks = [], []
    for dec in model.decoders:
        for layer in dec.layers:
            hooks.append(layer.linear1.register_forward_hook(lambda _m, _i, o: seen.append(o.detach().reshape(-1, o.size(-1)))))
    try:
        with torch.no_grad():
            run()
    finally:
        for h in hooks:
            h.remove()
    return seen


@functools.lru_cache(maxsize=4)
def oracle_pre_activations(case, idx):
    """float64 [B S, d_ff] per layer of exit ``idx``, at drop_prob 0."""
    m64 = copy.deepcopy(cpu_model(case)).double()
    trg, enc, _ = inputs(case)
    return pre_activations(m64, lambda: ref_decoder_logits(m64, trg, enc.double(), idx))


def oracle_with_relu_choice(case, idx, alive):
    """``oracle`` with relu' of layer l taken from ``alive[l]`` (bool [B S, d_ff])."""
    m64 = copy.deepcopy(cpu_model(case)).double()
    for layer, a in zip(m64.decoders[idx].layers, alive):
        layer.activation = relu_with_choice(a)
    with sdpa_kernel(SDPBackend.MATH):
        return reference_step(m64, case, idx, torch.float64)


# ---- the bounds (header of tests/test_gpu_train.py) --------------------------------------------------------------------------------
def logit_bound(want, tol=2e-4):
    return tol * max(1.0, want.abs().max().item())


def grad_fraction(got, want, tol=2e-3):
    """compare_grads' measure, as a fraction of ``tol``: the worst over the parameters of err / (max |g| + 2e-3 gmax); and its name."""
    gmax = max(g.abs().max().item() for g in want.values())
    worst = (0.0, "")
    for n, gw in want.items():
        rel = (got[n] - gw).abs().max().item() / (gw.abs().max().item() + 2e-3 * gmax) / tol
        if rel > worst[0]:
            worst = (rel, n)
    return worst


def fractions(got, want, factor=1.0, tol_logit=2e-4, tol_grad=2e-3):
    """(logits, parameter gradients, grad_enc) errors of ``got`` as fractions of the bounds around ``want``, each times ``factor``."""
    fl = (got.logits - want.logits).abs().max().item() / (factor * logit_bound(want.logits, tol_logit))
    fg = grad_fraction(got.grads, want.grads, tol_grad)[0] / factor
    fe = (got.grad_enc - want.grad_enc).abs().max().item() / (factor * tol_grad * want.grad_enc.abs().max().item())
    return fl, fg, fe


def dropout_sites(case):
    """(site, elements) of every mask one forward of both exits draws, at the documented sites (dropout_cases)."""
    import dropout_cases as DC
    B, S, Tq, L, D, H, F, _, _ = case.geo
    sizes = [B * H * S * S, B * S * D, B * H * S * Tq, B * S * D, B * S * F, B * S * D]
    return [(0, B * S * D)] + [(DC.documented_decoder_site(e, l, k), sizes[k]) for e in range(2) for l in range(L) for k in range(6)]
