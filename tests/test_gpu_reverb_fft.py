"""Reverberation by FFT on the device (eec_reverb_fft, csrc/reverb_fft.hip) against the fp64 convolution of reverb_fft_cases: the
derived bound and the working tolerance measured against an independent fp32 FFT, the exact properties (copies, zeros, NaN in the
padding, the tile energies behind which the noise stage runs unchanged), determinism (two runs, a split batch, no lengths, an offset
storage, a workspace-split call), the chain replayed from one captured graph, and the direct path left as it was."""
import functools

import numpy as np
import pytest
import torch

import reverb_fft_cases as F
import waveaug_cases as W
from early_exit_transformer_amd import augment

pytestmark = pytest.mark.gpu


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


@functools.lru_cache(maxsize=None)
def _bank(which="rirs", shift=True):
    if which == "impulses":
        return augment.RirBank(F.impulses(), normalize="none", shift=False, method="fft")
    return augment.RirBank(F.rirs(), shift=shift, method="fft")


def _records(bank):
    return [bank.rir(r) for r in range(len(bank))]


@functools.lru_cache(maxsize=None)
def _wave():
    return torch.from_numpy(F.wave_batch()).cuda()


def _lens(dev="cuda"):
    return torch.tensor(F.LENGTHS, device=dev)


def _outputs(bank, rows):
    """{(r, b): the device's output [length]} for the pairs of ``rows``; zeros past the lengths and no NaN asserted on the way."""
    got = {}
    for row in rows:
        out_d = augment.reverberate(_wave(), _lens(), bank, torch.tensor(row, device="cuda"))
        out = out_d.cpu().numpy()
        assert out_d.is_cuda and out.shape == (F.B, F.L) and not np.isnan(out).any()
        for b, r in enumerate(row):
            n = F.LENGTHS[b]
            assert (_bits(out[b, n:]) == 0).all(), (r, b)
            got.setdefault((r, b), out[b, :n])
    return got


@pytest.mark.parametrize("shift", [True, False], ids=["shift", "causal"])
def test_the_kernel_is_inside_the_derived_bound_and_four_times_an_independent_fp32_fft(shift):
    """Nine RIRs of 1 .. 16384 taps against utterances of 0 .. 3 S + 907 samples with NaN past each length, 24 pairs.  Measured on an
    MI355X: see the README ("Reverberation by FFT") for the ratios this prints."""
    bank = _bank("rirs", shift)
    assert bank.method == "fft" and augment.REVERB_FFT_BLOCK == F.S
    assert [bank.rir(r)[0] for r in range(9)] == (F.RIR_PEAKS if shift else [0] * 8 + [-5])
    pairs = F.pairs_of(("rirs", shift), _records(bank), F.INDEX_ROWS)
    worst, share, _ = F.judge(pairs, _outputs(bank, F.INDEX_ROWS), f"device, shift={shift}")
    assert 0.0 < worst <= F.MARGIN and share <= 1.0


def test_unit_impulses_return_the_input_shifted():
    """Impulses at 0, 1, S - 1, S, S + 1, 2 S - 1 (stored as one tap with d = -at): y[i] = x[i - at] within the working tolerance."""
    bank = _bank("impulses")
    assert [bank.rir(r)[0] for r in range(6)] == [-at for at in F.IMPULSES]
    rows = [[(b + s) % 6 for b in range(F.B)] for s in (0, 2, 4)]
    pairs = F.pairs_of("impulses", _records(bank), rows)
    outputs = _outputs(bank, rows)
    F.judge(pairs, outputs, "device, impulses")
    x = F.wave_batch()
    for (r, b), got in outputs.items():
        n, at = F.LENGTHS[b], F.IMPULSES[r]
        want = np.zeros(n, dtype=np.float32)
        want[at:] = x[b, :max(n - at, 0)]
        e_ref = max(p.e_ref for (q, _), p in pairs.items() if q == r)
        assert np.max(np.abs(got - want), initial=0.0) <= F.MARGIN * e_ref, (r, b)


def test_copies_zeros_and_all_zero_input_are_exact():
    bank, x = _bank(), F.wave_batch()
    index = torch.tensor([7, -1, 5, 9, 8, -3, 2, 99], device="cuda")
    out = augment.reverberate(_wave(), _lens(), bank, index).cpu().numpy()
    assert not np.isnan(out).any()
    for b in (1, 3, 5, 7):  # -1 and indices outside the bank: the utterance itself
        n = F.LENGTHS[b]
        assert np.array_equal(_bits(out[b, :n]), _bits(x[b, :n])) and (_bits(out[b, n:]) == 0).all()
    for b in (0, 2, 4, 6):
        n = F.LENGTHS[b]
        assert (_bits(out[b, n:]) == 0).all() and (n == 0 or not np.array_equal(out[b, :n], x[b, :n]))
    # all-zero input: exact zeros (+0.0), whatever the RIR; the padding still NaN
    zeros = np.where(np.isnan(x), x, np.float32(0.0))
    for row in F.INDEX_ROWS:
        out = augment.reverberate(torch.from_numpy(zeros).cuda(), _lens(), bank, torch.tensor(row, device="cuda"))
        assert (_bits(out) == 0).all()


def test_the_tile_energies_feed_the_noise_stage_unchanged():
    """wave_augment with an FFT bank and a noise bank: the scale within the existing 2 ulp of the one computed on the host from the
    device's own reverberated output (so ``partials`` is augment._host_energy of that output), the mix within the existing bound."""
    bank, noises = _bank(), augment.NoiseBank(W.noises())
    rir = [2, -1, 4, 7, 3, 8, 1, 5]
    gains = [1.0, 0.5, 1.7320507764816284, 1.0, 0.125, 2.0, 0.3333333432674408, 1.25]
    y = augment.reverberate(_wave(), _lens(), bank, torch.tensor(rir, device="cuda")).cpu().numpy()
    for m, row in enumerate(W.noises()):
        start = W.starts(row.shape[0])[m % 3]
        params = torch.tensor([[rir[b], m, start, (m + b) % len(W.SNRS), W.f32_bits(gains[b])] for b in range(F.B)], dtype=torch.int32)
        out_d, back, applied_d = augment.wave_augment(_wave(), _lens(), seed=0, rirs=bank, noises=noises, snrs=W.SNRS, params=params.cuda())
        out, applied = out_d.cpu().numpy(), applied_d.cpu().numpy()
        assert torch.equal(back.cpu(), params) and not np.isnan(out).any()
        for b, n in enumerate(F.LENGTHS):
            assert (_bits(out[b, n:]) == 0).all(), (m, b)
            seg = W.noise_segment(row, start, n)
            want, scale, allow = W.mix_fp64(y[b, :n], seg, W.SNRS[(m + b) % len(W.SNRS)], gains[b])
            assert W.ulps32(applied[b, 0], scale) <= 2.0, (m, b, applied[b, 0], scale)
            assert W.share_of_bound(out[b, :n], want, allow) <= 1.0, (m, b)
            if n > 0 and m != 5:  # the scale from the stated order of the energies, bit for bit
                es, en = augment._host_energy(y[b, :n]), augment._host_energy(seg)
                gain = 10.0 ** (-W.SNRS[(m + b) % len(W.SNRS)] / 20.0)
                assert _bits(applied[b, :1])[0] == W.f32_bits(float(np.sqrt(np.float64(es) / np.float64(en)) * np.float64(gain))), (m, b)


def test_two_runs_a_split_batch_no_lengths_an_offset_storage_and_a_split_workspace_return_the_same_bits():
    bank, noises = _bank(), augment.NoiseBank(W.noises())
    x = F.wave_batch()
    kw = dict(seed=9, rirs=bank, noises=noises, snrs=W.SNRS, volume=(0.5, 2.0), p_reverb=0.75)
    whole = augment.wave_augment(_wave(), _lens(), utt_offset=70, **kw)
    again = augment.wave_augment(_wave(), _lens(), utt_offset=70, **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(whole, again))
    assert len(set(whole[1][:, 0].tolist())) > 2
    lo = augment.wave_augment(torch.from_numpy(x[:3].copy()).cuda(), _lens()[:3], utt_offset=70, **kw)
    hi = augment.wave_augment(torch.from_numpy(x[3:].copy()).cuda(), _lens()[3:], utt_offset=73, **kw)
    for k in range(3):
        assert np.array_equal(np.concatenate([_bits(lo[k]), _bits(hi[k])]), _bits(whole[k])), k
    # lengths = None against lengths all L
    full = torch.from_numpy(F.wave_batch(seed=7, pad=0.5)).cuda()
    a = augment.wave_augment(full, None, utt_offset=70, **kw)
    b = augment.wave_augment(full, torch.full((F.B,), F.L), utt_offset=70, **kw)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))
    # the same samples in a storage that starts 4 bytes off a 16-byte boundary
    store = torch.empty(x.size + 1, device="cuda")
    store[1:].copy_(_wave().flatten())
    off = store[1:].view(F.B, F.L)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous() and _wave().data_ptr() % 16 == 0
    moved = augment.wave_augment(off, _lens(), utt_offset=70, **kw)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(moved, whole))
    # a workspace of one utterance at a time: the call is split, the bits stay
    index = torch.tensor(F.INDEX_ROWS[1], device="cuda")
    one = augment.reverberate(_wave(), _lens(), bank, index)
    split = augment.reverberate(_wave(), _lens(), bank, index, max_workspace_bytes=1)
    assert np.array_equal(_bits(one), _bits(split))
    old = bank.max_workspace_bytes
    try:
        bank.max_workspace_bytes = 1
        parts = augment.wave_augment(_wave(), _lens(), utt_offset=70, **kw)
    finally:
        bank.max_workspace_bytes = old
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(parts, whole))


def test_the_chain_with_an_fft_bank_replays_from_one_captured_graph():
    from early_exit_transformer_amd.frontend import MelFrontend
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    lens = [8000, 6000, 161, 0]
    x = rng.standard_normal((4, 8000)).astype(np.float32) * 0.1
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    wave, n = torch.from_numpy(x).to(dev), torch.tensor(lens, device=dev)
    bank, noises = _bank(), augment.NoiseBank(W.noises())
    speed, frontend, specaug = augment.SpeedPerturb(seed=5).train(), MelFrontend(), augment.SpecAugment(seed=6).train()
    waveaug = augment.WaveAugment(seed=8, rirs=bank, noises=noises, snrs=W.SNRS, volume=(0.5, 2.0)).train()
    hop = frontend.hop_length

    def chain():
        w, m = speed(wave, n)
        v = waveaug(w, m)
        mel = frontend(v, m)
        return w, m, v, mel, specaug(mel, 1 + m // hop)

    states = [mod.get_state() for mod in (speed, waveaug, specaug)]
    w, m, v, mel, aug = chain()  # the first call uploads the plan, the banks and the spectral image
    rows, applied = waveaug.last_params.clone(), waveaug.last_applied.clone()
    assert (rows[:, 0] >= 0).all() and torch.isfinite(v).all() and not torch.equal(v[0], w[0]) and torch.isfinite(aug).all()
    for b in range(4):
        assert not v[b, m[b]:].any()
    for mod, state in zip((speed, waveaug, specaug), states):
        mod.set_state(state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw, gm, gv, gmel, gaug = chain()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(waveaug.last_params, rows) and np.array_equal(_bits(waveaug.last_applied), _bits(applied)) and torch.equal(gm, m)
    assert np.array_equal(_bits(gw), _bits(w)) and np.array_equal(_bits(gv), _bits(v))
    assert np.array_equal(_bits(gmel), _bits(mel)) and np.array_equal(_bits(gaug), _bits(aug))


def test_a_direct_bank_and_a_call_without_method_return_todays_bits():
    x = F.wave_batch()
    direct = augment.RirBank(F.rirs()[:6])
    assert direct.method == "direct"
    index = [5, 4, 3, 2, 1, 0, 5, 4]
    out = augment.reverberate(_wave(), _lens(), direct, torch.tensor(index, device="cuda")).cpu().numpy()
    for b, r in enumerate(index):
        n = F.LENGTHS[b]
        assert np.array_equal(_bits(out[b, :n]), _bits(augment._host_reverb(x[b, :n], *direct.rir(r)))) and (_bits(out[b, n:]) == 0).all(), b
    # the override for one call, both ways
    fft = augment.reverberate(_wave(), _lens(), direct, torch.tensor(index, device="cuda"), method="fft").cpu().numpy()
    same = augment.reverberate(_wave(), _lens(), _bank(), torch.tensor(index, device="cuda")).cpu().numpy()
    assert np.array_equal(_bits(fft), _bits(same)) and not np.array_equal(_bits(fft), _bits(out))
    back = augment.reverberate(_wave(), _lens(), _bank(), torch.tensor(index, device="cuda"), method="direct").cpu().numpy()
    assert np.array_equal(_bits(back), _bits(out))
