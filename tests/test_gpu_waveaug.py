"""GPU tests of waveform augmentation (run with -m gpu on an MI355X): the launches of csrc/waveaug.hip through ``reverberate``,
``add_noise`` and ``wave_augment`` against the restatement of tests/waveaug_cases.py -- every reverberated sample within
(K_nz + 1) * 2^-24 * sum_k |h_k| |x_k| of the fp64 value; the mix, fed the kernel's own reverberation, with scale and gain within 2 ulp
and every sample within 4 * 2^-24 * (|y| + |scale n|) * |gain| --, exact copies, zeros and switched-off stages, equality with the
NumPy host path bit for bit, the draw word for word, reproducibility, split, length and alignment independence, and the chain
SpeedPerturb -> WaveAugment -> MelFrontend -> SpecAugment, eager and replayed from one captured graph.

Shapes: B = 8, L = 3000; lengths 0, 1, 7, 1023, 1024, 1025 (a tile of 1024 less one, exactly, plus one), 2999, 3000; NaN past every
length; RIRs of 1, 2, 63, 64, 65, 1025 and 2500 taps (the last two span three and five chunks of 512 taps) and one with zero heads and
tails, each against every utterance; noise rows of 1, 5, 2999, 3000 and 4001 samples and an all-zero one, from three starts each."""
import functools

import numpy as np
import pytest
import torch

import waveaug_cases as S
from early_exit_transformer_amd import augment

pytestmark = pytest.mark.gpu


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


@functools.lru_cache(maxsize=None)
def _banks():
    return augment.RirBank(S.rirs()), augment.NoiseBank(S.noises())


@functools.lru_cache(maxsize=None)
def _waves():
    """(the shared batch, the same with utterance 5 all zero); never written."""
    x = S.wave_batch()
    z = x.copy()
    z[5, :S.LENGTHS[5]] = 0.0
    return x, z


def _lens(dev="cuda"):
    return torch.tensor(S.LENGTHS, device=dev)


def test_reverberation_equals_the_restatement_and_the_host_path():
    """Every RIR against every utterance: the bound at every valid sample, no NaN, zeros past the lengths, the host path's bits."""
    x, _ = _waves()
    rirs, _ = _banks()
    wave = torch.from_numpy(x).cuda()
    worst = 0.0
    for r in range(len(rirs)):
        d, taps = rirs.rir(r)
        out_d = augment.reverberate(wave, _lens(), rirs, r)
        out = out_d.cpu().numpy()
        assert out_d.is_cuda and out.shape == (S.B, S.L) and not np.isnan(out).any()
        for b, n in enumerate(S.LENGTHS):
            assert (_bits(out[b, n:]) == 0).all(), (r, b)
            y, mag = S.reverb_fp64(x[b], n, taps, d)
            share = S.share_of_bound(out[b, :n], y, S.reverb_bound(taps.shape[0], mag))
            assert share <= 1.0, (r, b, share)
            worst = max(worst, share)
        host = augment.reverberate(torch.from_numpy(x), _lens("cpu"), rirs, r)
        assert np.array_equal(_bits(host), _bits(out)), r
    print(f"reverb: worst output at {worst:.3f} of (K_nz + 1) 2^-24 sum |h||x|")
    assert worst > 0.0
    # a different RIR per utterance in one launch, some without: copies are exact
    index = torch.tensor([6, -1, 5, 8, 7, -3, 2, 99], device="cuda")
    mixed = augment.reverberate(wave, _lens(), rirs, index).cpu().numpy()
    host = augment.reverberate(torch.from_numpy(x), _lens("cpu"), rirs, index.cpu()).numpy()
    assert np.array_equal(_bits(mixed), _bits(host))
    for b in (1, 3, 5, 7):
        n = S.LENGTHS[b]
        assert np.array_equal(_bits(mixed[b, :n]), _bits(x[b, :n])) and (_bits(mixed[b, n:]) == 0).all()
    # shift=False: the plain causal convolution cut to the input's length (d = 0, and -5 for the RIR with five zeros in front)
    late = augment.RirBank(S.rirs(), shift=False)
    for r, d_want in ((4, 0), (5, 0), (7, -5)):
        d, taps = late.rir(r)
        out = augment.reverberate(wave, _lens(), late, r).cpu().numpy()
        assert d == d_want and not np.isnan(out).any()
        for b, n in enumerate(S.LENGTHS):
            y, mag = S.reverb_fp64(x[b], n, taps, d)
            assert S.share_of_bound(out[b, :n], y, S.reverb_bound(taps.shape[0], mag)) <= 1.0 and (_bits(out[b, n:]) == 0).all(), (r, b)
        assert np.array_equal(_bits(augment.reverberate(torch.from_numpy(x), _lens("cpu"), late, r)), _bits(out)), r


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["start0", "last", "wraps"])
def test_the_mix_equals_the_restatement_fed_the_kernels_reverberation_and_the_host_path(kind):
    """Every noise row against every utterance from one of the three starts, behind a different RIR per utterance, with a gain: scale and
    gain within 2 ulp, the samples within their bound, the host path's bits; the zero row and the zero utterance add nothing."""
    _, z = _waves()
    rirs, noises = _banks()
    rows = S.noises()
    wave = torch.from_numpy(z).cuda()
    rir = [2, -1, 4, 7, 3, 0, 1, 5]
    gains = [1.0, 0.5, 1.7320507764816284, 1.0, 0.125, 2.0, 0.3333333432674408, 1.25]
    y_d = augment.reverberate(wave, _lens(), rirs, torch.tensor(rir, device="cuda"))
    y = y_d.cpu().numpy()
    worst, worst_ulp = 0.0, 0.0
    for m, row in enumerate(rows):
        start = S.starts(row.shape[0])[kind]
        params = torch.tensor([[rir[b], m, start, (m + b) % len(S.SNRS), S.f32_bits(gains[b])] for b in range(S.B)], dtype=torch.int32)
        out_d, back, applied_d = augment.wave_augment(wave, _lens(), seed=0, rirs=rirs, noises=noises, snrs=S.SNRS, params=params.cuda())
        out, applied = out_d.cpu().numpy(), applied_d.cpu().numpy()
        assert torch.equal(back.cpu(), params) and not np.isnan(out).any() and applied.shape == (S.B, 2)
        for b, n in enumerate(S.LENGTHS):
            assert (_bits(out[b, n:]) == 0).all(), (m, b)
            want, scale, allow = S.mix_fp64(y[b, :n], S.noise_segment(row, start, n), S.SNRS[(m + b) % len(S.SNRS)], gains[b])
            assert _bits(applied[b, 1:])[0] == S.f32_bits(gains[b])
            ulp = S.ulps32(applied[b, 0], scale)
            assert ulp <= 2.0, (m, b, applied[b, 0], scale)
            if m == 5 or b == 5 or n == 0:  # the all-zero row, the all-zero utterance, the empty one: nothing is added
                assert scale == 0.0 and applied[b, 0] == 0.0
                if gains[b] == 1.0:
                    assert np.array_equal(_bits(out[b, :n]), _bits(y[b, :n]))
            else:
                assert scale > 0.0
            share = S.share_of_bound(out[b, :n], want, allow)
            assert share <= 1.0, (m, b, share)
            worst, worst_ulp = max(worst, share), max(worst_ulp, ulp)
        host = augment.wave_augment(torch.from_numpy(z), _lens("cpu"), seed=0, rirs=rirs, noises=noises, snrs=S.SNRS, params=params)
        assert np.array_equal(_bits(host[0]), _bits(out)) and np.array_equal(_bits(host[2]), _bits(applied)), m
    print(f"mix ({kind}): worst sample at {worst:.3f} of 4 2^-24 (|y| + |scale n|) |gain|, worst scale {worst_ulp:.2f} ulp")
    assert worst > 0.0


def test_add_noise_alone_and_the_switched_off_stages_are_exact():
    x, _ = _waves()
    rirs, noises = _banks()
    wave = torch.from_numpy(x).cuda()
    # add_noise without a reverberation launch: E_s comes from the energy launch; the host path's bits
    snr = [S.SNRS[b % len(S.SNRS)] for b in range(S.B)]
    index, start = torch.tensor([4, 3, 2, 1, 0, 4, 3, 2]), torch.tensor([4000, 2999, 2000, 3, 0, 1, 7000, -1])
    out = augment.add_noise(wave, _lens(), noises, index.cuda(), start.cuda(), snr)
    host = augment.add_noise(torch.from_numpy(x), _lens("cpu"), noises, index, start, snr)
    assert np.array_equal(_bits(out), _bits(host))
    for b, n in enumerate(S.LENGTHS):
        seg = S.noise_segment(S.noises()[index[b]], int(start[b]), n)
        want, scale, allow = S.mix_fp64(x[b, :n], seg, snr[b], 1.0)
        assert S.share_of_bound(out[b, :n].cpu().numpy(), want, allow) <= 1.0 and (scale > 0.0) == (n > 0)
    # every stage off, by probability and by indices outside the banks: the utterances themselves, zeros past the lengths
    off = torch.tensor([[-1, -1, 0, 0, S.ONE_BITS], [8, 6, 5, 0, S.ONE_BITS], [-5, 0, 0, 6, S.ONE_BITS], [0, 2, 0, -1, S.ONE_BITS]] * 2, dtype=torch.int32)
    off[3, 0] = off[7, 0] = 99
    for kw in (dict(p_reverb=0.0, p_noise=0.0), dict(params=off.cuda()), dict(rirs=None, noises=None)):
        kw = {**dict(rirs=rirs, noises=noises, snrs=S.SNRS), **kw}
        got, _, applied = augment.wave_augment(wave, _lens(), seed=3, **kw)
        assert torch.equal(applied.cpu(), torch.tensor([[0.0, 1.0]] * S.B))
        for b, n in enumerate(S.LENGTHS):
            assert np.array_equal(_bits(got[b, :n]), _bits(x[b, :n])) and (_bits(got[b, n:]) == 0).all()


def test_the_device_draw_is_the_restated_draw():
    """B = 257 (five workgroups of the draw launch), utt_offset + b crossing 2^32; the coins word for word at p = 0, 1 and 0.5."""
    B, seed, utt = 257, 20240917, (1 << 32) - 100
    rirs, noises = _banks()
    lens = [r.shape[0] for r in S.noises()]
    wave = torch.zeros(B, 50, device="cuda")
    for p_r, p_n, volume in ((1.0, 1.0, (0.5, 1.5)), (0.0, 0.0, None), (0.5, 0.5, (2.0, 0.25)), (1.0, 0.0, None), (0.0, 1.0, (1.0, 1.0))):
        out, params, applied = augment.wave_augment(wave, seed=seed, utt_offset=utt, rirs=rirs, noises=noises, p_reverb=p_r, p_noise=p_n, snrs=S.SNRS,
                                                    volume=volume)
        want, words = S.draw(seed, utt, B, 8, p_r, lens, p_n, len(S.SNRS), volume)
        got = params.cpu().numpy()
        assert params.dtype == torch.int32 and np.array_equal(got, want), (p_r, p_n)
        assert np.array_equal(got[:, 0] >= 0, words[:, 0] < S.threshold(p_r)) and np.array_equal(got[:, 1] >= 0, words[:, 2] < S.threshold(p_n))
        assert ((got[:, 0] >= 0).all(), (got[:, 1] >= 0).all()) == (p_r == 1.0, p_n == 1.0)
        assert ((got[:, 0] < 0).all(), (got[:, 1] < 0).all()) == (p_r == 0.0, p_n == 0.0)
        assert np.array_equal(_bits(applied[:, 1]), want[:, 4]) and not applied[:, 0].any() and not out.any()
    assert S.threshold(0.5) == 1 << 31 and S.threshold(1.0) == 1 << 32 and S.threshold(0.0) == 0


def test_two_runs_a_split_batch_no_lengths_an_offset_storage_and_prescribed_rows_return_the_same_bits():
    x, _ = _waves()
    rirs, noises = _banks()
    kw = dict(seed=9, rirs=rirs, noises=noises, snrs=S.SNRS, volume=(0.5, 2.0), p_reverb=0.75)
    wave = torch.from_numpy(x).cuda()
    whole = augment.wave_augment(wave, _lens(), utt_offset=70, **kw)
    again = augment.wave_augment(wave, _lens(), utt_offset=70, **kw)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(whole, again))
    want, _ = S.draw(9, 70, S.B, 8, 0.75, [r.shape[0] for r in S.noises()], 1.0, len(S.SNRS), (0.5, 2.0))
    assert np.array_equal(whole[1].cpu().numpy(), want) and len(set(want[:, 0].tolist())) > 2
    lo = augment.wave_augment(torch.from_numpy(x[:3].copy()).cuda(), _lens()[:3], utt_offset=70, **kw)
    hi = augment.wave_augment(torch.from_numpy(x[3:].copy()).cuda(), _lens()[3:], utt_offset=73, **kw)
    for k in range(3):
        assert np.array_equal(np.concatenate([_bits(lo[k]), _bits(hi[k])]), _bits(whole[k])), k
    # prescribed rows equal to the drawn ones
    given = augment.wave_augment(wave, _lens(), **{**kw, "seed": 1, "params": whole[1].clone()})
    assert np.array_equal(_bits(given[0]), _bits(whole[0])) and np.array_equal(_bits(given[2]), _bits(whole[2]))
    # lengths = None against lengths all L
    full = torch.from_numpy(S.wave_batch(seed=7, pad=0.5)).cuda()
    a = augment.wave_augment(full, None, utt_offset=70, **kw)
    b = augment.wave_augment(full, torch.full((S.B,), S.L), utt_offset=70, **kw)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))
    # the same samples in a storage that starts 4 bytes off a 16-byte boundary, with and without RIRs (the copy path's quads)
    store = torch.empty(x.size + 1, device="cuda")
    store[1:].copy_(wave.flatten())
    off = store[1:].view(S.B, S.L)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous() and wave.data_ptr() % 16 == 0
    moved = augment.wave_augment(off, _lens(), utt_offset=70, **kw)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(moved, whole))
    plain, shifted = augment.wave_augment(wave, _lens(), seed=9, noises=noises), augment.wave_augment(off, _lens(), seed=9, noises=noises)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(plain, shifted))
    host = augment.wave_augment(torch.from_numpy(x), _lens("cpu"), seed=9, noises=noises)
    assert np.array_equal(_bits(host[0]), _bits(plain[0])) and np.array_equal(_bits(host[2]), _bits(plain[2]))


def test_the_whole_chain_composes_and_replays_from_one_captured_graph():
    from early_exit_transformer_amd.frontend import MelFrontend
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    lens = [8000, 6000, 161, 0]
    x = rng.standard_normal((4, 8000)).astype(np.float32) * 0.1
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    wave, n = torch.from_numpy(x).to(dev), torch.tensor(lens, device=dev)
    rirs, noises = _banks()
    speed, frontend, specaug = augment.SpeedPerturb(seed=5).train(), MelFrontend(), augment.SpecAugment(seed=6).train()
    waveaug = augment.WaveAugment(seed=8, rirs=rirs, noises=noises, snrs=S.SNRS, volume=(0.5, 2.0)).train()
    hop = frontend.hop_length

    def chain():
        w, m = speed(wave, n)
        v = waveaug(w, m)
        mel = frontend(v, m)
        frames = 1 + m // hop
        return w, m, v, mel, frames, specaug(mel, frames)

    states = [mod.get_state() for mod in (speed, waveaug, specaug)]
    w, m, v, mel, frames, aug = chain()  # the first call uploads the plan and the banks
    choice, rows, applied = speed.last_choice.clone(), waveaug.last_params.clone(), waveaug.last_applied.clone()
    want, _ = S.draw(8, 0, 4, 8, 1.0, [r.shape[0] for r in S.noises()], 1.0, len(S.SNRS), (0.5, 2.0))
    assert np.array_equal(rows.cpu().numpy(), want) and waveaug.get_state()["calls"] == 1
    assert v.shape == w.shape and torch.isfinite(v).all() and not torch.equal(v[0], w[0])
    assert mel.shape == (4, 80, 1 + w.shape[1] // hop) and torch.isfinite(mel).all() and torch.isfinite(aug).all()
    for b in range(4):
        assert not v[b, m[b]:].any() and not mel[b, :, frames[b]:].any()
    for b, k in enumerate(lens):  # every utterance gets the mel of itself processed alone
        alone, alone_n, _ = augment.speed_perturb(wave[b:b + 1, :k].contiguous(), seed=0, choice=choice[b:b + 1])
        assert alone_n.tolist() == [m[b].item()]
        mine, _, mine_applied = augment.wave_augment(alone, alone_n, seed=0, rirs=rirs, noises=noises, snrs=S.SNRS, params=rows[b:b + 1])
        assert np.array_equal(_bits(mine_applied), _bits(applied[b:b + 1]))
        padded = torch.zeros(1, w.shape[1], device=dev)
        padded[:, :mine.shape[1]] = mine
        assert np.array_equal(_bits(padded), _bits(v[b:b + 1])), b
        assert torch.equal(frontend(padded, alone_n), mel[b:b + 1])

    # the four stages in one captured graph: replayed, the eager run's bits
    for mod, state in zip((speed, waveaug, specaug), states):
        mod.set_state(state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw, gm, gv, gmel, gframes, gaug = chain()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(waveaug.last_params, rows) and np.array_equal(_bits(waveaug.last_applied), _bits(applied)) and torch.equal(gm, m)
    assert np.array_equal(_bits(gw), _bits(w)) and np.array_equal(_bits(gv), _bits(v))
    assert np.array_equal(_bits(gmel), _bits(mel)) and np.array_equal(_bits(gaug), _bits(aug))
