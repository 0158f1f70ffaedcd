"""Cases, driver and fp64 oracle shared by tests/test_host_aed_step.py and tests/test_gpu_aed_step.py: the two step-wise AED
decoders (csrc/decoder_step.hip per utterance, csrc/decoder_batch.hip for a batch) at the shapes where their kernels take
another path.  Everything here is seeded and runs on the CPU; no device code.

A case is a decoder geometry, a set of searches advanced in lockstep (``lead``: () one session, (n,) the exits of one utterance,
(E, B) a batch), a memory length, a number of steps and a beam count per step.  ``drive`` yields what the device is fed at every
step and the host-side prefixes; ``oracle`` evaluates the reference's own modules in float64 on the whole prefixes, last
position, at the case's check steps only.

The thresholds below are read off the kernels and stated here, not computed from the package:
  step_attn_kernel / batch_self_attn_kernel   the score loop's second trip needs more than 256 keys: s >= 256
  step_attn_kernel                            the P.V loop's second trip needs nk > 8 * 4 * (64 / dh) keys:
                                              32 / 64 / 128 / 256 keys at head dim 64 / 32 / 16 / 8 (self: s >= that; cross: Tq > that)
  batch_cross_attn_kernel                     chunks of 256 keys: Tq = 255, 256, 257, 513
  batch_linear_kernel                         64-row tiles: M = B * R of 5, 35 (half tiles), 64, 65 (a second tile of one row), 80
"""
import copy
import functools
from typing import NamedTuple, Optional, Tuple

import torch

from conftest import ref_decoder_logprobs
from early_exit_transformer_amd import synth
from early_exit_transformer_amd.model import full_conformer

SOS, PAD, P_PAD, MAX_LEN = 1, 30, 0.1, 400
LONG_CHECKS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 263)


class Case(NamedTuple):
    id: str
    geo: Tuple[int, int, int, int, int]  # d_model, heads, d_ff, vocab, decoder layers
    lead: Tuple[int, ...]                # () | (sessions,) | (E, B)
    Tq: int
    steps: int
    segments: Optional[Tuple[Tuple[int, int], ...]]  # (first step, beams) ... : "1 -> 3 -> 16 -> 2"
    cycle: Optional[Tuple[int, ...]]                 # beams of step s = cycle[s % len]: "5, 16"
    checks: Tuple[int, ...]
    thresholds: Tuple[int, ...] = ()  # first step s at which a loop takes its second trip: s - 1 and s are both checked
    m_values: Tuple[int, ...] = ()    # batched: the B * R that the check steps must produce
    seed: int = 0

    @property
    def batched(self):
        return len(self.lead) == 2

    @property
    def EB(self):
        """(exits, utterances per exit) of the case, whatever its lead."""
        return (1, 1) if not self.lead else (self.lead[0], 1) if len(self.lead) == 1 else self.lead

    def rows(self, s):
        if self.cycle is not None:
            return self.cycle[s % len(self.cycle)]
        return [r for first, r in self.segments if first <= s][-1]


def _short(steps, *thresholds):
    """The first three steps, the last one, and both sides (and the step after) of every threshold."""
    return tuple(sorted({0, 1, 2, steps - 1, *[t + d for t in thresholds for d in (-1, 0, 1)]}))


G_TINY, G_MID, G_WIDE, G_LN = (64, 8, 100, 37, 2), (256, 8, 512, 256, 1), (512, 8, 2048, 256, 1), (1024, 16, 64, 64, 1)

PER_UTTERANCE = (
    Case("P1", G_TINY, (), 5, 264, ((0, 1), (1, 3), (32, 16), (260, 2)), None, LONG_CHECKS, (256,), seed=101),
    Case("P2", (96, 6, 160, 64, 1), (), 131, 140, None, (5, 16), _short(140, 128), (128,), seed=102),
    Case("P3-1", G_MID, (1,), 257, 70, None, (10, 16, 5), _short(70, 64), (64,), seed=103),
    Case("P3-3", G_MID, (3,), 257, 70, None, (10, 16, 5), _short(70, 64), (64,), seed=104),
    Case("P3-6", G_MID, (6,), 257, 70, None, (10, 16, 5), _short(70, 64), (64,), seed=105),
    Case("P4", G_WIDE, (), 33, 40, None, (16,), _short(40, 32), (32,), seed=136),
    Case("P5", G_LN, (), 9, 6, None, (2,), _short(6), seed=107),
)
BATCHED = (
    Case("B1", G_TINY, (2, 5), 1, 264, ((0, 1), (1, 13), (64, 16), (260, 7)), None, LONG_CHECKS, (256,), (5, 65, 80, 35), seed=201),
    *[Case(f"B2-{Tq}", G_MID, (1, 2), Tq, 4, None, (16,), (0, 1, 2, 3), (), (32,), seed=202) for Tq in (255, 256, 257, 513)],
    Case("B3", (128, 8, 160, 64, 1), (8, 3), 40, 20, None, (7, 16), _short(20), (), (21, 48), seed=203),
    Case("B4", G_WIDE, (2, 4), 33, 40, None, (16,), _short(40, 32), (32,), (64,), seed=216),
    Case("B5", G_LN, (1, 1), 9, 6, None, (2,), _short(6), (), (2,), seed=205),
)
# the weight domain: every step is checked, under rescale(model, e) for each e
W_CASE = Case("W", (256, 8, 2048, 256, 2), (2, 2), 45, 12, None, (10,), tuple(range(12)), (), (20,), seed=301)
W_EXPONENTS = (0, 4, 8)
CASES = PER_UTTERANCE + BATCHED + (W_CASE,)
BY_ID = {c.id: c for c in CASES}


def bound(want, batched):
    """The project's bound for the per-utterance step decoder, 2e-5 * max(10, max |logp|); twice that for the batched one, which
    the suite holds to the per-utterance decoder by the same bound (two chained comparisons)."""
    ok = torch.isfinite(want)
    return (2.0 if batched else 1.0) * 2e-5 * max(10.0, want[ok].abs().max().item())


@functools.lru_cache(maxsize=None)
def _model(geo, n_exits, seed):
    D, H, F, V, L = geo
    fc = full_conformer(trg_pad_idx=PAD, n_enc_exits=n_exits, enc_voc_size=V, dec_voc_size=V, d_model=D, n_head=H, max_len=MAX_LEN,
                        d_feed_forward=F, n_enc_layers=1, n_dec_layers=L, features_length=80, drop_prob=0.1, depthwise_kernel_size=31,
                        device="cpu").eval()
    sd = synth.synth_state_dict(fc.state_dict(), seed=seed, style="trained")
    for k in list(sd):  # the decoders' final norm is the one shared LayerNorm (tests/golden/aed_fixture.py); no x 8 on the heads
        if ".norm." in k and k.startswith("decoders."):
            sd[k] = sd["layer_norm." + k.rsplit(".", 1)[1]].clone()
    fc.load_state_dict(sd, strict=True)
    return fc


def build_model(case):
    """The case's model, fp32 on the CPU, in eval mode.  Shared between calls: copy it before moving or changing it."""
    return _model(case.geo, case.EB[0], case.seed % 100)


def rescale(model, e):
    """A copy of ``model`` whose decoders compute the same function with other magnitudes inside: linear1 (weight, bias) x 2^-e and
    linear2.weight x 2^e (ReLU is positively homogeneous); the value rows of both attentions' in_proj x 2^-e and their
    out_proj.weight x 2^e.  Powers of two: exact in every binary format, short of its range."""
    m = copy.deepcopy(model)
    D = m.emb.weight.size(1)
    up, down = 2.0 ** e, 2.0 ** -e
    with torch.no_grad():
        for dec in m.decoders:
            for layer in dec.layers:
                layer.linear1.weight.mul_(down)
                layer.linear1.bias.mul_(down)
                layer.linear2.weight.mul_(up)
                for att in (layer.self_attn, layer.multihead_attn):
                    att.in_proj_weight[2 * D:].mul_(down)
                    att.in_proj_bias[2 * D:].mul_(down)
                    att.out_proj.weight.mul_(up)
    return m


def memory(case):
    """The encoder outputs the searches attend to, fp32 [E, B, Tq, D]."""
    g = torch.Generator().manual_seed(case.seed + 1000)
    return torch.randn(*case.EB, case.Tq, case.geo[0], generator=g)


def drive(case):
    """Per step s: (s, tokens [*lead, R], parent [*lead, R] or None at s = 0, prefixes [E, B, R, s + 1]).  SOS at position 0, then
    random tokens, PAD with probability 0.1; every beam extends a random row of the previous step (repeats and drop-outs)."""
    g = torch.Generator().manual_seed(case.seed)
    E, B = case.EB
    V = case.geo[3]
    prefixes = None
    for s in range(case.steps):
        R = case.rows(s)
        if s == 0:
            tok, parent = torch.full((E, B, R), SOS, dtype=torch.long), None
            prefixes = tok.unsqueeze(-1)
        else:
            parent = torch.randint(0, prefixes.size(2), (E, B, R), generator=g)
            tok = torch.randint(3, V, (E, B, R), generator=g)
            tok[torch.rand(E, B, R, generator=g) < P_PAD] = PAD
            prefixes = torch.cat([torch.gather(prefixes, 2, parent.unsqueeze(-1).expand(E, B, R, s)), tok.unsqueeze(-1)], dim=-1)
        shape = (*case.lead, R)
        yield s, tok.reshape(shape), None if parent is None else parent.reshape(shape), prefixes


@functools.lru_cache(maxsize=None)
def checked_prefixes(case):
    """{check step: prefixes [E, B, R, s + 1]}."""
    return {s: p for s, _, _, p in drive(case) if s in case.checks}


def reference(model, mem, prefixes):
    """The reference's decoder modules on whole prefixes, last position: log-probs [E, B, R, V] in the dtype of ``model`` / ``mem``;
    search (e, b) runs exit e + 1 on memory mem[e, b]."""
    E, B, R, S = prefixes.shape
    out = []
    with torch.no_grad():
        for e in range(E):
            enc = mem[e].repeat_interleave(R, dim=0)
            out.append(ref_decoder_logprobs(model, prefixes[e].reshape(B * R, S), enc, e + 1)[:, -1].reshape(B, R, -1))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def oracle(case):
    """{check step: float64 log-probs [E, B, R, V]} of the case's (unscaled) model.  Read-only: shared between tests."""
    m64 = copy.deepcopy(build_model(case)).double()
    mem = memory(case).double()
    return {s: reference(m64, mem, p) for s, p in checked_prefixes(case).items()}
