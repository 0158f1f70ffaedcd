"""Batched AED beam search (csrc/decoder_batch.hip, eec_decoder_batch_*; BeamInference.beam_search_batch / decode_batch) against
the per-utterance path it replaces (decoder_session_group / beam_search_exits / decode_all_exits).  The batched linears run on
f16x3 MFMA operands (fp16 hi + lo, three products, fp32 accumulation) and the per-utterance decoder in plain fp32; log-probs are
held to the bound the repository applies to its bf16x3 decoder GEMMs, 2e-5 * max(10, max |logp|), and searches agree up to
near-ties.  Both decoders against an fp64 oracle: tests/test_gpu_aed_step.py."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from early_exit_transformer_amd import synth
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import full_conformer

pytestmark = pytest.mark.gpu

ARGS = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=0.6)


def _fixture_model(**over):
    """The model of test_aed_exits_in_lockstep_match_the_exit_by_exit_search (aed_greedy.npz + aed_fixture.aed_state_dict);
    ``over`` replaces geometry fields."""
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    n_dec_layers = over.pop("n_dec_layers", int(z["n_dec_layers"]))
    kw = {**eval(str(z["kwargs"])), **over}
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=n_dec_layers, **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    return fc.cuda(), kw


@pytest.fixture(scope="module")
def fixture_model():
    return _fixture_model()


def _batch_step_vs_groups(fc, E, B, Tq, rows, seed, V=256):
    """Steps of one batch session against one session group (decoder_session_group) per utterance, random tokens (PAD now and then) and parents
    per (exit, utterance), beam counts ``rows`` step by step.  Returns the worst error over its bound."""
    g = torch.Generator().manual_seed(seed)
    D = fc._cfg.d_model
    taps = torch.randn(E, B, Tq, D, generator=g).cuda()
    exits = list(range(1, E + 1))
    steps = len(rows)
    sess = fc.decoder_batch_session(taps, exits, steps)
    assert sess is not None
    groups = [fc.decoder_session_group([taps[e, b:b + 1] for e in range(E)], exits, steps) for b in range(B)]
    assert all(gr is not None for gr in groups)
    tok = torch.full((E, B, 1), 1, dtype=torch.long)
    parent = None
    worst = 0.0
    for s, R in enumerate(rows):
        got = sess.step(tok.cuda(), None if parent is None else parent.cuda())
        assert got.shape == (E, B, tok.size(2), V)
        for b in range(B):
            want = groups[b].step(tok[:, b].cuda(), None if parent is None else parent[:, b].cuda())
            tol = 2e-5 * max(10.0, want.abs().max().item())
            err = (got[:, b] - want).abs().max().item()
            assert err < tol, (s, b, err, tol)
            worst = max(worst, err / tol)
        parent = torch.randint(0, tok.size(2), (E, B, R), generator=g)
        tok = torch.randint(3, V, (E, B, R), generator=g)
        tok[torch.rand(E, B, R, generator=g) < 0.1] = 126
    return worst


def test_batch_step_matches_the_per_utterance_group_step(fixture_model):
    """B = 5 utterances x all 6 exits (E * B = 30 searches in one launch per kernel), 6 steps, beams 1 -> 7 -> 4."""
    fc, kw = fixture_model
    worst = _batch_step_vs_groups(fc, kw["n_enc_exits"], 5, 45, [7, 4, 7, 4, 7, 4], seed=11)
    print(f"worst error / bound: {worst:.3f}")


@pytest.mark.parametrize("B,R,Tq", [(1, 10, 45), (3, 7, 300), (2, 16, 37)])
def test_batch_step_edge_shapes(fixture_model, B, R, Tq):
    """One utterance; 3 x 7 = 21 rows per exit (not a multiple of the 64-row tile); 16 beams; a memory longer than one
    256-key chunk of the cross-attention (Tq = 300)."""
    fc, kw = fixture_model
    _batch_step_vs_groups(fc, kw["n_enc_exits"], B, Tq, [R, R, max(1, R // 2), R, R], seed=B * 100 + R)


def test_batch_step_head_dim_64_and_small_vocab():
    """d_model 512 with 8 heads (head dim 64), and a 32-token vocabulary."""
    fc, _ = _fixture_model(d_model=512, n_head=8, d_feed_forward=1024, n_enc_exits=3, n_dec_layers=2)
    _batch_step_vs_groups(fc, 3, 4, 50, [10, 6, 10, 3], seed=3)
    fc, _ = _fixture_model(dec_voc_size=32, n_enc_exits=2, n_dec_layers=2)
    _batch_step_vs_groups(fc, 2, 3, 40, [5, 5, 5, 2], seed=4, V=32)


def _scores_agree(a, b, what):
    """Sorted final scores within 1e-4; True when the per-utterance search's scores are separated by more than 1e-3 (then the
    best sequences must be identical)."""
    sa, sb = torch.stack(a).cpu().sort().values, torch.stack(b).cpu().sort().values
    assert (sa - sb).abs().max().item() < 1e-4, what
    return sa.numel() < 2 or (sa[1:] - sa[:-1]).abs().min().item() > 1e-3


@pytest.mark.parametrize("beam", [1, 7, 16])
def test_beam_search_batch_matches_the_lockstep_search_per_utterance(fixture_model, beam):
    fc, kw = fixture_model
    E, B = kw["n_enc_exits"], 3
    g = torch.Generator().manual_seed(beam)
    taps = torch.randn(E, B, 60, kw["d_model"], generator=g).cuda()
    exits = list(range(1, E + 1))
    inf = BeamInference()
    args = dict(ARGS, max_length=12, beam_size=beam)
    got = inf.beam_search_batch(fc, taps, exits, **args)
    assert got is not None and len(got) == B and all(len(row) == E for row in got)
    flips = 0
    for b in range(B):
        want = inf.beam_search_exits(fc, [taps[e, b:b + 1] for e in range(E)], exits, **args)
        for e in range(E):
            (ta, sa, ba), (tb, sb, bb) = want[e], got[b][e]
            assert len(tb) == beam and all(t.numel() == 13 for t in tb)
            if _scores_agree(sa, sb, (b, e)):
                flips += ba != bb
    assert flips <= 1, flips


def _ragged_batch(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    spec = (torch.rand(B, 80, T, generator=g) * 3).cuda()
    vlen = torch.tensor([T - 9 * b for b in range(B)])
    for b in range(B):
        spec[b, :, int(vlen[b]):] = 0
    return spec, vlen


@pytest.mark.parametrize("beam", [5, 10])
def test_decode_batch_matches_the_per_utterance_loop(fixture_model, beam):
    """A ragged batch (B = 7, T = 131, distinct valid lengths): decode_batch against evaluate_batch_ae's loop
    (decode_all_exits per utterance); final scores of beam_search_batch on the batch encoder run against beam_search_exits on
    each utterance's own encoder run."""
    fc, kw = fixture_model
    E, B, T = kw["n_enc_exits"], 7, 131
    spec, vlen = _ragged_batch(B, T, seed=beam)
    inf = BeamInference()
    L = int(30 - T * 5 / 200)
    got = inf.decode_batch(fc, spec, vlen, beam_size=beam, **ARGS)
    want = [inf.decode_all_exits(fc, spec[b], vlen[b], beam_size=beam, **ARGS) for b in range(B)]
    assert len(got) == B and all(len(row) == E and all(len(t) == L + 1 for t in row) for row in got)
    taps = fc._run_encoder(spec, vlen, want_out=False, want_taps=True, n_groups=E)[1]
    batch = inf.beam_search_batch(fc, taps, list(range(1, E + 1)), max_length=L, beam_size=beam, **ARGS)
    flips = 0
    for b in range(B):
        taps_b = fc._run_encoder(spec[b:b + 1], vlen[b:b + 1], want_out=False, want_taps=True, n_groups=E)[1]
        single = inf.beam_search_exits(fc, [taps_b[e] for e in range(E)], list(range(1, E + 1)), max_length=L, beam_size=beam, **ARGS)
        for e in range(E):
            assert batch[b][e][2] == got[b][e]
            assert single[e][2] == want[b][e]
            if _scores_agree(single[e][1], batch[b][e][1], (b, e)):
                flips += got[b][e] != want[b][e]
    assert flips <= 1, flips


def test_eos_finalising_searches_fall_back_to_the_per_utterance_path(fixture_model):
    fc, kw = fixture_model
    E, B, T = kw["n_enc_exits"], 3, 131
    spec, vlen = _ragged_batch(B, T, seed=9)
    inf = BeamInference()
    taps = fc._run_encoder(spec, vlen, want_out=False, want_taps=True, n_groups=E)[1]
    assert inf.beam_search_batch(fc, taps, list(range(1, E + 1)), max_length=9, min_length=3, beam_size=5, **ARGS) is None
    got = inf.decode_batch(fc, spec, vlen, beam_size=5, min_length=3, **ARGS)
    want = [inf.decode_all_exits(fc, spec[b], vlen[b], beam_size=5, min_length=3, **ARGS) for b in range(B)]
    assert got == want


def test_decode_batch_at_the_default_geometry():
    """The bench's AED geometry (full_conformer, 6 exits, 6 decoder layers, beam 10) at B = 64, T = 1027 (85 steps):
    every search completes with finite scores; three utterances against decode_all_exits."""
    B, T = 64, 1027
    cfg = dict(n_enc_exits=6, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000, d_feed_forward=2048,
               n_enc_layers=2, features_length=80, drop_prob=0.1, depthwise_kernel_size=31)
    fc = full_conformer(trg_pad_idx=126, n_dec_layers=6, device="cuda", **cfg).eval()
    fc.load_state_dict(synth.synth_state_dict(fc.state_dict(), seed=4, style="init"))
    fc = fc.cuda()
    mel = synth.synth_mel(B, 80, T, seed=4).cuda()
    vlen = torch.full((B,), T)
    inf = BeamInference()
    args = dict(ARGS, pen_alpha=1.0)
    taps = fc._run_encoder(mel, vlen, want_out=False, want_taps=True, n_groups=6)[1]
    res = inf.beam_search_batch(fc, taps, list(range(1, 7)), max_length=int(T / 12), beam_size=10, **args)
    del taps
    assert res is not None and len(res) == B
    assert all(torch.isfinite(torch.stack(s)).all().item() and len(best) == 1 + int(T / 12) for row in res for _, s, best in row)
    flips = 0
    for b in (0, 31, 63):
        want = inf.decode_all_exits(fc, mel[b], vlen[b], beam_size=10, **args)
        taps_b = fc._run_encoder(mel[b:b + 1], vlen[b:b + 1], want_out=False, want_taps=True, n_groups=6)[1]
        single = inf.beam_search_exits(fc, [taps_b[e] for e in range(6)], list(range(1, 7)), max_length=int(T / 12), beam_size=10, **args)
        for e in range(6):
            assert single[e][2] == want[e]
            sa, sb = torch.stack(single[e][1]).cpu().sort().values, torch.stack(res[b][e][1]).cpu().sort().values
            assert (sa - sb).abs().max().item() < 1e-4 * max(1.0, sa.abs().max().item()), (b, e)
            if (sa[1:] - sa[:-1]).abs().min().item() > 1e-3:
                flips += res[b][e][2] != want[e]
    assert flips <= 1, flips
