"""Host checks of per-utterance input lengths in the CTC loss and decoders: the case module's reference is what it claims to be
(tests/ctc_len_cases.py), the C entries are declared and exported, and the Python arguments are validated before any device is
touched."""
import inspect
import os
import re

import pytest
import torch

import ctc_cases as C
import ctc_len_cases as L
from early_exit_transformer_amd import beam, capi, ctc, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = 10001  # EEC_ERR_BAD_ARG of include/eec.h
NEW_EXPORTS = ("eec_ctc_loss_len", "eec_ctc_loss_forward_len", "eec_ctc_loss_backward_len", "eec_greedy_ctc_len", "eec_ctc_beam_decode_len")


def test_reference_with_full_lengths_is_the_existing_reference():
    lp = C.peaky_logp(5.0, E=2, B=3, T=24)
    tgt, tl = C.greedy_targets(lp[0])
    want, gw = C.ref_ctc(lp, tgt, tl)
    for il in ([24, 24, 24], [24, 99, 1000]):  # lengths above T' are clamped
        got, g = L.ref_ctc(lp, tgt, tl, il)
        assert torch.equal(got, want) and torch.equal(g, gw)


@pytest.mark.parametrize("scale", sorted(C.PEAKY_SCALES))
def test_reference_on_ragged_peaky_inputs_is_finite_zero_past_the_length_and_pad_independent(scale):
    """torch's CPU CTCLoss with ragged input lengths: finite losses, an exactly zero gradient at and past each length, and neither
    depends on what the padding holds (NaN included)."""
    lp, tgt, tl, il = L.ragged_case(scale, 4)
    want, gw = L.ref_ctc(lp, tgt, tl, il)
    assert torch.isfinite(want).all() and (want > 0).all()
    pad = ~L.valid_mask(il, lp.size(2))
    assert (gw[:, pad] == 0).all() and torch.isfinite(gw).all()
    assert gw[:, ~pad].abs().max() > 0
    for kind in ("nan", "random"):
        got, g = L.ref_ctc(L.overwrite_pad(lp, il, kind), tgt, tl, il)
        assert torch.equal(got, want) and torch.equal(g[:, ~pad], gw[:, ~pad]) and (g[:, pad] == 0).all()


def test_reference_gives_zero_for_no_frames():
    lp = C.peaky_logp(2.0, E=1, B=2, T=8)
    tgt = torch.tensor([[3, 4], [3, 4]])
    want, gw = L.ref_ctc(lp, tgt, torch.tensor([0, 2]), [0, 0])  # an empty and a non-empty target (infeasible: zeroed)
    assert want.tolist() == [0.0] and (gw == 0).all()


def test_feasibility_edge_of_the_reference():
    lp, tgt, tl = L.feasibility_case(2)
    want, _ = L.ref_ctc(lp, tgt, tl, [10])
    path = -sum(lp[0, 0, t, c].double() for t, c in enumerate(L.FEASIBLE_PATH)) / len(L.FEASIBLE_TARGET)
    assert abs(want[0] - path) < 1e-9
    short, g = L.ref_ctc(lp, tgt, tl, [9])
    assert short.abs().max() == 0 and (g == 0).all()


def test_ring_case_covers_every_length_and_an_empty_target():
    lp, tgt, tl, il = L.ring_case(2)
    assert il.tolist() == list(L.RING_LENS) + [L.RING_T] and tl.tolist() == [0, 1, 2] + [3] * 9 + [0]
    want, _ = L.ref_ctc(lp, tgt, tl, il)
    assert torch.isfinite(want).all()


@pytest.mark.parametrize("case", C.BEAM_CASES)
def test_sliced_beam_cases_are_margin_safe(case):
    """The share of sequences on which the beam test compares tokens is held by the oracle alone: every sliced sequence of every
    BEAM_CASES entry is margin-safe under both readings of the skip rule."""
    N = case[0]
    assert L.safe_share(*case) == {False: N, True: N}


def test_decoder_references_on_slices():
    logp = C.beam_logp(8, 64, 64, 3.0)
    lens = L.decoder_lens(8, 64)
    assert lens.tolist() == [64, 1, 2, 32, 63, 3, 21, 33]
    dec = L.ref_greedy(logp, lens)
    assert all(len(d) <= int(n) for d, n in zip(dec, lens)) and L.ref_greedy(logp, [0] * 8) == [[]] * 8
    assert L.ref_beam(logp[0], 0, 10)[:2] == ([], 0.0)


def test_new_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    lib = capi.load()
    for name in NEW_EXPORTS:
        assert name in capi.EXPORTS and hasattr(lib, name)
        proto = re.search(r"\bint " + name + r"\(([^)]*)\)", header)
        assert proto, name
        assert re.search(r"const int32_t\* (input_len|em_len)\b", proto.group(1)), name
    # one more pointer than the entry without lengths, in the position the header gives it
    for name, base, pos in (("eec_ctc_loss_len", "eec_ctc_loss", 3), ("eec_ctc_loss_forward_len", "eec_ctc_loss_forward", 3),
                            ("eec_ctc_loss_backward_len", "eec_ctc_loss_backward", 3), ("eec_greedy_ctc_len", "eec_greedy_ctc", 1),
                            ("eec_ctc_beam_decode_len", "eec_ctc_beam_decode_ex", 1)):
        a, b = list(getattr(lib, name).argtypes), list(getattr(lib, base).argtypes)
        assert a[:pos] + a[pos + 1:] == b and a[pos] is capi.I32, name  # the typed device pointer of a const int32_t*
    assert lib.eec_abi_version() == 16


def test_new_entries_check_their_arguments_before_any_launch():
    """A null tensor pointer is refused with the existing entries' error whether or not lengths are given (0x100 stands for a
    lengths pointer: it is never read)."""
    lib = capi.load()
    for il in (None, 0x100):
        assert lib.eec_ctc_loss_len(None, None, None, il, 1, 1, 1, 4, 1, 0, None, None, None) == BAD_ARG
        assert lib.eec_ctc_loss_forward_len(None, None, None, il, 1, 1, 1, 4, 1, 0, None, None, None, None) == BAD_ARG
        assert lib.eec_ctc_loss_backward_len(None, None, None, il, 1, 1, 1, 4, 1, 0, None, None, None, None, None) == BAD_ARG
        assert lib.eec_greedy_ctc_len(None, il, 1, 1, 4, 0, None, None, None) == BAD_ARG
        assert lib.eec_ctc_beam_decode_len(None, il, 1, 1, 4, 0, 10, 0.95, 0, None, None, None, None, None) == BAD_ARG


def test_python_arguments():
    assert inspect.signature(ctc.exit_ctc_losses).parameters["input_len"].default is None
    assert inspect.signature(ctc.exit_training_losses).parameters["input_len"].default is None
    assert inspect.signature(ctc.greedy_ctc).parameters["em_len"].default is None
    assert inspect.signature(ctc.ctc_beam_decode).parameters["em_len"].default is None
    assert inspect.signature(model.Early_conformer.greedy_decode).parameters["lengths"].default is None
    assert inspect.signature(beam.BeamInference.ctc_cuda_predict).parameters["lengths"].default is None
    dev = torch.device("cpu")
    assert ctc._frame_counts("f", "input_len", None, 3, dev) is None
    for src in (torch.tensor([5, 0, 9]), torch.tensor([5, 0, 9], dtype=torch.int32), [5, 0, 9]):
        out = ctc._frame_counts("f", "input_len", src, 3, dev)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.tolist() == [5, 0, 9]
    with pytest.raises(ValueError, match="3 entries"):
        ctc._frame_counts("f", "input_len", torch.tensor([1, 2]), 3, dev)
    with pytest.raises(ValueError, match="int32 or int64"):
        ctc._frame_counts("f", "em_len", torch.tensor([1.0, 2.0, 3.0]), 3, dev)
    # without a device every entry still fails loudly, lengths or not
    lp = torch.zeros(1, 2, 4, 8)
    for call in (lambda: ctc.exit_ctc_losses(lp, torch.ones(2, 1, dtype=torch.long), torch.ones(2, dtype=torch.long), input_len=torch.tensor([4, 2])),
                 lambda: ctc.greedy_ctc(lp[0], em_len=torch.tensor([4, 2])),
                 lambda: ctc.ctc_beam_decode(lp[0], em_len=torch.tensor([4, 2]))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
