"""GPU tests of resampling and speed perturbation (run with -m gpu on an MI355X): the launches of csrc/resample.hip through
``speed_perturb`` / ``resample`` against the restatement of tests/resample_cases.py fed the library's plan -- every valid output
sample within (K_nz + 1) * 2^-24 * sum_k |h_k| |x_k| of the fp64 value, exact zeros past the lengths, exact copies under (1, 1) --,
reproducibility, split, length and alignment independence, the draw bit for bit, equality with the NumPy host path, and the chain
SpeedPerturb -> MelFrontend -> SpecAugment, eager and replayed from one captured graph.

Shapes: B = 8, L = 3000; lengths 0, 1, 6, 7, 9, 23 (shorter than a filter), 2303, 2304, 2305 and 2816 (outputs ending one before, at
and one after 2560 = 2.5 tiles of 1024), 3000; NaN past every length; every ratio meets every length."""
import functools

import numpy as np
import pytest
import torch

import resample_cases as S
from early_exit_transformer_amd import augment, capi

pytestmark = pytest.mark.gpu
CALLS = {"speed": (S.SPEED_RATIOS, dict(factors=S.SPEED_FACTORS, sample_rate=S.SPEED_RATE)),
         "rates": (S.RATE_RATIOS, dict(factors=S.RATE_FACTORS, sample_rate=S.RATE_RATE))}


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The shared batches and their restated results, computed once and never written: (plan, [(wave, lens, choice, want)]) with
    want[b] = (y fp64, bound) or None for a copy."""
    ratios, _ = CALLS[name]
    plan = augment.resample_plan(ratios)
    tables = [None if r == (1, 1) else S.dense(*plan.table(c)) for c, r in enumerate(ratios)]
    out = []
    for k, (lens, choice) in enumerate(S.batches(len(ratios))):
        wave = S.wave_batch(40 + k, lens)
        want = []
        for b, (n, c) in enumerate(zip(lens, choice)):
            if tables[c] is None:
                want.append(None)
            else:
                y, mag = S.resample_fp64(wave[b], n, tables[c])
                want.append((y, S.bound(tables[c], mag)))
        out.append((wave, lens, choice, want))
    return plan, out


def _device(name, wave, lens, choice, **kw):
    out, out_len, back = augment.speed_perturb(torch.from_numpy(wave).cuda(), None if lens is None else torch.tensor(lens, device="cuda"), seed=0,
                                               choice=torch.tensor(choice, dtype=torch.int32, device="cuda"), **CALLS[name][1], **kw)
    assert out.is_cuda and out_len.is_cuda and out_len.dtype == torch.int64 and back.tolist() == list(choice)
    return out, out_len


@pytest.mark.parametrize("name", ["speed", "rates"])
def test_the_kernel_equals_the_restatement_and_the_host_path(name):
    """Items 1, 2 and 5: the bound at every valid sample, no NaN, zeros past out_len, out_len, the (1, 1) rows, the host path's bits."""
    plan, batches = _case(name)
    worst, copies = 0.0, 0
    for wave, lens, choice, want in batches:
        out_d, len_d = _device(name, wave, lens, choice)
        out, out_len = out_d.cpu().numpy(), len_d.cpu().numpy()
        assert out.shape == (S.B, plan.out_samples(S.L)) and not np.isnan(out).any()
        for b, (n, c) in enumerate(zip(lens, choice)):
            m = S.out_len(n, *plan.ratios[c])
            assert out_len[b] == m and (out[b, m:].view(np.int32) == 0).all(), (b, n, c)
            if want[b] is None:
                assert m == n and torch.equal(out_d[b, :n].cpu(), torch.from_numpy(wave[b, :n]))
                assert np.array_equal(out[b, :n].view(np.int32), wave[b, :n].view(np.int32))
                copies += 1
            else:
                share = S.share_of_bound(out[b, :m], *want[b])
                assert share <= 1.0, (b, n, c, share)
                worst = max(worst, share)
        host, host_len, _ = augment.speed_perturb(torch.from_numpy(wave), torch.tensor(lens), seed=0, choice=torch.tensor(choice, dtype=torch.int32),
                                                  **CALLS[name][1])
        assert torch.equal(host_len, len_d.cpu()) and np.array_equal(_bits(host), _bits(out_d))
    assert copies == sum(w is None for *_, want in batches for w in want) and (copies >= len(S.LENGTHS)) == (name == "speed")
    print(f"resample {CALLS[name][0]}: worst output at {worst:.3f} of (K_nz + 1) 2^-24 sum |h||x|")
    assert worst > 0.0


def test_two_runs_a_split_batch_no_lengths_and_an_offset_storage_return_the_same_bits():
    _, batches = _case("speed")
    wave, lens, choice, _ = batches[1]
    assert max(lens) > 2000 and len(set(choice)) > 1
    kw = dict(factors=S.SPEED_FACTORS)
    whole, whole_len, whole_c = augment.speed_perturb(torch.from_numpy(wave).cuda(), torch.tensor(lens), seed=9, utt_offset=70, **kw)
    again, again_len, again_c = augment.speed_perturb(torch.from_numpy(wave).cuda(), torch.tensor(lens), seed=9, utt_offset=70, **kw)
    assert torch.equal(whole_c, again_c) and torch.equal(whole_len, again_len) and np.array_equal(_bits(whole), _bits(again))
    assert np.array_equal(whole_c.cpu().numpy(), S.draw(9, 70, S.B, 3))
    lo = augment.speed_perturb(torch.from_numpy(wave[:3].copy()).cuda(), torch.tensor(lens[:3]), seed=9, utt_offset=70, **kw)
    hi = augment.speed_perturb(torch.from_numpy(wave[3:].copy()).cuda(), torch.tensor(lens[3:]), seed=9, utt_offset=73, **kw)
    assert torch.equal(torch.cat([lo[2], hi[2]]), whole_c) and torch.equal(torch.cat([lo[1], hi[1]]), whole_len)
    assert np.array_equal(np.concatenate([_bits(lo[0]), _bits(hi[0])]), _bits(whole))
    # lengths = None against lengths all L
    full = S.wave_batch(7, [S.L] * S.B)
    a, a_len = _device("speed", full, None, choice)
    b, b_len = _device("speed", full, [S.L] * S.B, choice)
    assert torch.equal(a_len, b_len) and np.array_equal(_bits(a), _bits(b))
    # the same samples in a storage that starts 4 bytes off a 16-byte boundary
    store = torch.empty(wave.size + 1, device="cuda")
    store[1:].copy_(torch.from_numpy(wave).cuda().flatten())
    off = store[1:].view(S.B, S.L)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    moved, moved_len, _ = augment.speed_perturb(off, torch.tensor(lens), seed=9, utt_offset=70, **kw)
    assert torch.equal(moved_len, whole_len) and np.array_equal(_bits(moved), _bits(whole))


def test_the_device_draw_is_the_restated_draw():
    """B = 257 (five workgroups of the draw launch), utt_offset + b crossing 2^32; out_len from the draw launch itself."""
    B, L, seed, utt = 257, 50, 20240917, (1 << 32) - 100
    lens = [(13 * b) % (L + 1) for b in range(B)]
    wave = torch.zeros(B, L, device="cuda")
    out, out_len, choice = augment.speed_perturb(wave, torch.tensor(lens), seed=seed, utt_offset=utt)
    want = S.draw(seed, utt, B, 3)
    assert choice.dtype == torch.int32 and np.array_equal(choice.cpu().numpy(), want) and set(want.tolist()) == {0, 1, 2}
    ratios = [(9, 10), (1, 1), (11, 10)]
    want_len = [S.out_len(n, *ratios[c]) for n, c in zip(lens, want)]
    assert out_len.tolist() == want_len and not out.any()
    lib, plan = capi.load(), augment.resample_plan(ratios).on(wave.device)
    c2, n2 = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int64, device="cuda")
    len_dev = torch.tensor(lens, device="cuda")
    capi.check(lib.eec_speed_draw(len_dev.data_ptr(), B, L, seed, utt, plan.data_ptr(), c2.data_ptr(), n2.data_ptr(), capi.stream_ptr(wave.device)), "eec_speed_draw")
    assert np.array_equal(c2.cpu().numpy(), want) and n2.tolist() == want_len
    n3 = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    capi.check(lib.eec_resample_lengths(None, c2.data_ptr(), B, L, plan.data_ptr(), n3.data_ptr(), capi.stream_ptr(wave.device)), "eec_resample_lengths")
    assert n3.tolist() == [S.out_len(L, *ratios[c]) for c in want]


def test_resample_between_sample_rates():
    """44.1 kHz -> 16 kHz through ``resample`` (the window of a tile is 7 * 441 + 475 samples, the weights 5.4 k floats: both in LDS),
    then the ratios that take the kernel's other three paths."""
    rng = np.random.default_rng(12)
    lens = [4410, 4409, 300]
    x = rng.standard_normal((3, 4410)).astype(np.float32)
    x[1, 4409:], x[2, 300:] = np.nan, np.nan
    out, n = augment.resample(torch.from_numpy(x).cuda(), torch.tensor(lens), orig_freq=44100, new_freq=16000)
    host, host_n = augment.resample(torch.from_numpy(x), torch.tensor(lens), orig_freq=44100, new_freq=16000)
    assert n.tolist() == [1600, 1600, 109] and torch.equal(n.cpu(), host_n) and np.array_equal(_bits(out), _bits(host))
    t = S.dense(*augment.resample_plan([(441, 160)]).table(0))
    for b, length in enumerate(lens):
        y, mag = S.resample_fp64(x[b], length, t)
        assert S.share_of_bound(out[b, :n[b]].cpu().numpy(), y, S.bound(t, mag)) <= 1.0
    # 640 -> 1: 8398 taps, neither the weights nor a tile's window fit the LDS; 320 -> 1: the weights fit, the window does not;
    # 639 -> 640: 640 phases of 13 taps do not fit, the window does
    long = rng.standard_normal((2, 20000)).astype(np.float32)
    for (o, k), want_n in (((640, 1), [32, 15]), ((320, 1), [63, 29]), ((639, 640), [20032, 9015])):
        out, n = augment.resample(torch.from_numpy(long).cuda(), torch.tensor([20000, 9000]), orig_freq=o, new_freq=k)
        host, host_n = augment.resample(torch.from_numpy(long), torch.tensor([20000, 9000]), orig_freq=o, new_freq=k)
        assert n.tolist() == want_n and torch.equal(n.cpu(), host_n) and np.array_equal(_bits(out), _bits(host)), (o, k)
        plan = augment.resample_plan([(o, k)])
        total, fits = int(plan.image[4 + 6]), {(640, 1): False, (320, 1): True, (639, 640): False}[(o, k)]
        assert (total <= 6144) == fits


def test_speed_perturbation_front_end_and_specaugment_compose_and_capture():
    from early_exit_transformer_amd.frontend import MelFrontend
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(6)
    lens = [8000, 6000, 161, 0]
    x = rng.standard_normal((4, 8000)).astype(np.float32) * 0.1
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    wave, n = torch.from_numpy(x).to(dev), torch.tensor(lens, device=dev)
    speed, frontend, specaug = augment.SpeedPerturb(seed=5).train(), MelFrontend(), augment.SpecAugment(seed=6).train()
    hop = frontend.hop_length

    def chain():
        w, m = speed(wave, n)
        mel = frontend(w, m)
        frames = 1 + m // hop
        return w, m, mel, frames, specaug(mel, frames)

    s0, a0 = speed.get_state(), specaug.get_state()
    w, m, mel, frames, aug = chain()
    choice = speed.last_choice.clone()
    ratios = [(9, 10), (1, 1), (11, 10)]
    assert np.array_equal(choice.cpu().numpy(), S.draw(5, 0, 4, 3)) and speed.get_state()["calls"] == 1
    assert w.shape == (4, 8889) and m.tolist() == [S.out_len(k, *ratios[c]) for k, c in zip(lens, choice.tolist())]
    assert mel.shape == (4, 80, 1 + 8889 // hop) and torch.isfinite(mel).all() and frames.tolist() == [1 + k // hop for k in m.tolist()]
    for b in range(4):  # the perturbed lengths reached the front end: nothing past an utterance's frames
        assert not mel[b, :, frames[b]:].any()
    assert aug.shape == mel.shape and torch.isfinite(aug).all() and not torch.equal(aug, mel)
    assert torch.equal(aug[2, :, frames[2]:], mel[2, :, frames[2]:])
    for b, k in enumerate(lens):  # every utterance equals itself resampled alone, zero-padded to the same width
        alone, alone_n, _ = augment.speed_perturb(wave[b:b + 1, :k].contiguous(), seed=0, choice=choice[b:b + 1])
        assert alone_n.tolist() == [m[b].item()]
        padded = torch.zeros(1, w.shape[1], device=dev)
        padded[:, :alone.shape[1]] = alone
        assert torch.equal(padded, w[b:b + 1])
        assert torch.equal(frontend(padded, alone_n), mel[b:b + 1])

    # the three stages in one captured graph (a single linear chain): replayed, the eager run's bits
    speed.set_state(s0), specaug.set_state(a0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw, gm, gmel, gframes, gaug = chain()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(speed.last_choice, choice) and torch.equal(gm, m) and torch.equal(gframes, frames)
    assert np.array_equal(_bits(gw), _bits(w)) and np.array_equal(_bits(gmel), _bits(mel)) and np.array_equal(_bits(gaug), _bits(aug))
