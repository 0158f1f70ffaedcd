"""CPU tests of SpecAugment: the restatement of tests/specaug_cases.py against ``F.interpolate`` in fp64, the draw's ranges, split
independence and statistics, the host path of ``spec_augment`` against the restatement, prescribed parameters, the module, and every
refusal of the two C entries (checked before any device work, so they run without a GPU)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import specaug_cases as S
from early_exit_transformer_amd import augment, capi
from early_exit_transformer_amd.build import LIB_PATH

W = S.W
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement's warp is F.interpolate of the two segments
# ---------------------------------------------------------------------------------------------------------------------------
def _interpolate(x, c, w, cubic):
    """``x`` [rows, n] fp64: torch's interpolation of x[:, :c] onto w frames and of x[:, c:] onto n - w frames, concatenated."""
    n = x.shape[1]
    t = torch.from_numpy(x)
    if cubic:
        one = lambda seg, size: F.interpolate(seg[None, None], size=(seg.shape[0], size), mode="bicubic", align_corners=False)[0, 0]  # noqa: E731
    else:
        one = lambda seg, size: F.interpolate(seg[None], size=size, mode="linear", align_corners=False)[0]  # noqa: E731
    return torch.cat([one(t[:, :c], w), one(t[:, c:], n - w)], dim=1).numpy()


def _warp_cases():
    out = []
    for n in (11, 12, 37, 64, 131, 257):
        for win in (5, 40, 80):
            if n <= 2 * win:
                continue
            for c in sorted({win, n - win - 1, (n // 2)}):
                for w in sorted({c - win + 1, c + win, c, c + 1}):
                    out.append((n, c, w))
    out += [(11, 5, 1), (11, 5, 10), (2 * 40 + 1, 40, 1), (2 * 40 + 1, 40, 80), (37, 36, 1), (37, 1, 36), (2, 1, 1)]
    return out


@pytest.mark.parametrize("cubic", [True, False], ids=["bicubic", "linear"])
def test_the_restated_warp_is_interpolate_of_the_two_segments(cubic):
    """Includes c = W, w = 1 (= c - W + 1), w = c + W and n = 2 W + 1, for windows of 5, 40 and 80."""
    rng = np.random.default_rng(5)
    cases = _warp_cases()
    assert (11, 5, 1) in cases and (11, 5, 10) in cases and any(c == win and n == 2 * win + 1 for n, c, _ in cases for win in (5, 40))
    worst = 0.0
    for n, c, w in cases:
        assert S.warp_valid(n, c, w)
        x = rng.standard_normal((3, n)) * 10.0 ** rng.uniform(-2, 2, (3, n))
        got, _ = S.warp(x, c, w, cubic)
        want = _interpolate(x, c, w, cubic)
        err = np.abs(got - want).max() / np.abs(x).max()
        worst = max(worst, err)
        assert err <= 1e-9, (n, c, w, err)
    print(f"restated warp vs F.interpolate, cubic={cubic}: worst error {worst:.2e} of max|x|")


def test_the_weights_sum_to_one_and_the_identity_warp_is_the_identity():
    for cubic in (True, False):
        for d, n_in, n_out in ((0, 5, 1), (3, 7, 9), (8, 7, 9), (0, 1, 4), (2, 1, 4), (6, 126, 7)):
            taps, wts = S.source(d, n_in, n_out, cubic)
            assert abs(sum(wts) - 1.0) < 1e-14 and all(0 <= j < n_in for j in taps)
        x = np.random.default_rng(0).standard_normal((2, 20))
        got, _ = S.warp(x, 8, 8, cubic)
        assert np.array_equal(got, x)  # c == w: every source position is an integer, the weights are 0 and 1 exactly


# ---------------------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------------------
T_DRAW, MELS, SEED = 200, 80, 20240917


def _draw_lengths(count):
    rng = np.random.default_rng(1)
    lens = rng.integers(0, T_DRAW + 1, count)
    lens[:7] = [0, 1, 2 * W, 2 * W + 1, T_DRAW, T_DRAW + 50, -3]  # the last two are clamped
    return lens


def test_every_drawn_parameter_is_in_its_range():
    lens = _draw_lengths(3000)
    p = S.draw(lens, MELS, T_DRAW, SEED)
    assert p.shape == (3000, 16) and p.dtype == np.int32
    n = np.clip(lens, 0, T_DRAW)
    c, w = p[:, 0], p[:, 1]
    off = n <= 2 * W
    assert ((c == 0) & (w == 0))[off].all() and off[:3].all() and not off[3:6].any() and off[6]
    on = ~off
    assert (c[on] >= W).all() and (c[on] < n[on] - W).all() and (w[on] >= c[on] - W + 1).all() and (w[on] <= c[on] + W).all()
    assert (w[on] >= 1).all() and (w[on] <= n[on] - 1).all()
    for k in range(2):
        f0, fw = p[:, 2 + 2 * k], p[:, 3 + 2 * k]
        assert (fw >= 0).all() and (fw <= 27).all() and (f0 >= 0).all() and (f0 + fw <= MELS).all()
    cap = np.floor(float(np.float32(0.05)) * n).astype(np.int64)
    for k in range(5):
        t0, tw = p[:, 6 + 2 * k], p[:, 7 + 2 * k]
        assert (tw >= 0).all() and (tw <= cap).all() and (t0 >= 0).all() and (t0 + tw <= n).all()
    # the ranges are reached at both ends
    assert (c[on] == W).any() and (c[on] == n[on] - W - 1).any() and (w[on] == c[on] - W + 1).any() and (w[on] == c[on] + W).any()
    assert p[:, 3].min() == 0 and p[:, 3].max() == 27 and (p[:, 7] == cap)[n > 40].any()
    # a cap, a narrow band, a ratio above one
    q = S.draw(lens, 23, T_DRAW, SEED, F=40, ratio=3.0, Tmax=7)
    assert q[:, 3].max() == 23 and (q[:, 2] + q[:, 3] <= 23).all() and q[:, 7].max() == 7 and (q[:, 6] + q[:, 7] <= n).all()
    q = S.draw(lens, 23, T_DRAW, SEED, ratio=3.0)
    assert (q[:, 7] <= n).all() and (q[:, 6] + q[:, 7] <= n).all() and (q[:, 7] == n)[n > 0].any()


def test_seeds_differ_and_utt_offset_reproduces_a_split_batch():
    lens = _draw_lengths(400)
    whole = S.draw(lens, MELS, T_DRAW, SEED)
    assert not np.array_equal(whole, S.draw(lens, MELS, T_DRAW, SEED + 1))
    assert np.array_equal(whole, S.draw(lens, MELS, T_DRAW, SEED))
    for a in (1, 129, 399):
        assert np.array_equal(np.concatenate([S.draw(lens[:a], MELS, T_DRAW, SEED), S.draw(lens[a:], MELS, T_DRAW, SEED, utt_offset=a)]), whole)
    big = (1 << 64) - 3  # the index wraps mod 2^64
    assert np.array_equal(S.draw(lens[:8], MELS, T_DRAW, SEED, utt_offset=big)[3:], S.draw(lens[3:8], MELS, T_DRAW, SEED, utt_offset=0))


def test_the_mean_widths_are_those_of_uniform_draws():
    """4000 utterances of 200 frames under seed 20240917: fw uniform on 0 .. 27, tw on 0 .. 10, w - c on -4 .. 5, f0 and t0 uniform
    given their widths (checked through f0 / (n_mels - fw), which has mean 1 / 2): each mean within 5 sigma."""
    N = 4000
    p = S.draw([T_DRAW] * N, MELS, T_DRAW, SEED).astype(np.float64)

    def within(x, mean, var):
        x = np.asarray(x).ravel()
        assert abs(x.mean() - mean) <= 5.0 * math.sqrt(var / x.size), (x.mean(), mean, math.sqrt(var / x.size))

    within(p[:, 3:6:2], 13.5, (28 ** 2 - 1) / 12)
    within(p[:, 7::2], 5.0, (11 ** 2 - 1) / 12)
    within(p[:, 1] - p[:, 0], 0.5, (10 ** 2 - 1) / 12)
    within(p[:, 0], (W + T_DRAW - W - 1) / 2, ((T_DRAW - 2 * W) ** 2 - 1) / 12)
    within(p[:, 2:5:2] / (MELS - p[:, 3:6:2]), 0.5, 1 / 12 + 1 / 6 / (MELS - 27))  # discrete uniform on 0 .. m: variance (m + 2) / (12 m) of the ratio
    within(p[:, 6::2] / (T_DRAW - p[:, 7::2]), 0.5, 1 / 12 + 1 / 6 / (T_DRAW - 10))


# ---------------------------------------------------------------------------------------------------------------------------
# the host path of spec_augment
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bicubic", "linear"])
@pytest.mark.parametrize("n_mels,T", S.SHAPES[:2])
def test_the_host_path_is_the_restatement(n_mels, T, mode):
    lens = S.lengths_of(T)
    mel = S.mel_batch(5, n_mels, T, seed=T, lengths=lens, pad=NAN)
    out, params = augment.spec_augment(torch.from_numpy(mel), torch.tensor(lens, dtype=torch.int32), seed=11, utt_offset=3, time_warp_mode=mode)
    want_p = S.draw(lens, n_mels, T, 11, utt_offset=3)
    assert params.dtype == torch.int32 and np.array_equal(params.numpy(), want_p)
    want, kind, mag = S.apply(mel, lens, want_p, 2, 5, mode == "bicubic")
    assert (kind[4] == S.WARPED).any() and (kind[3] == S.WARPED).any() and not (kind[:3] == S.WARPED).any()
    share = S.check_output(out.numpy(), mel, want, kind, mag)
    assert 0.0 < share <= 1.0
    # the padding: bit for bit, NaN included, and none of it in a valid frame
    for b, n in enumerate(lens):
        assert np.array_equal(out.numpy()[b, :, n:].view(np.int32), mel[b, :, n:].view(np.int32))
        assert not np.isnan(out.numpy()[b, :, :n]).any()


def test_without_a_warp_the_host_path_only_copies_and_masks():
    n_mels, T = 23, 131
    lens = [131, 77, 12, 1, 0]
    mel = S.mel_batch(5, n_mels, T, seed=2, lengths=lens, pad=NAN)
    for value in (0.0, -1.5):
        out, params = augment.spec_augment(torch.from_numpy(mel), torch.tensor(lens), seed=5, time_warp_window=0, mask_value=value, n_time_masks=3,
                                           time_mask_ratio=0.2, time_mask_width=9)
        assert np.array_equal(params.numpy(), S.draw(lens, n_mels, T, 5, window=0, n_time=3, ratio=0.2, Tmax=9))
        assert (params[:, :2] == 0).all() and (params[:, 7::2] <= 9).all()
        want, kind, mag = S.apply(mel, lens, params.numpy(), 2, 3, True, value)
        assert not (kind == S.WARPED).any() and (kind == S.MASKED).any()
        S.check_output(out.numpy(), mel, want, kind, mag, value)
    # no lengths: T everywhere
    full = S.mel_batch(5, n_mels, T, seed=2)
    a, pa = augment.spec_augment(torch.from_numpy(full), None, seed=5)
    b, pb = augment.spec_augment(torch.from_numpy(full), torch.full((5,), T), seed=5)
    assert torch.equal(pa, pb) and np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))


@pytest.mark.parametrize("mode", ["bicubic", "linear"])
def test_prescribed_parameters_are_clipped_or_ignored(mode):
    n_mels, T = 23, 37
    rows = S.prescribed(n_mels, T)
    lens = [n for n, _ in rows]
    params = np.array([r for _, r in rows], dtype=np.int32)
    mel = S.mel_batch(len(rows), n_mels, T, seed=9, lengths=lens, pad=NAN)
    out, back = augment.spec_augment(torch.from_numpy(mel), torch.tensor(lens), seed=0, params=torch.from_numpy(params), time_warp_mode=mode,
                                     n_freq_masks=2, n_time_masks=2)
    assert np.array_equal(back.numpy(), params)
    want, kind, mag = S.apply(mel, lens, params, 2, 2, mode == "bicubic")
    S.check_output(out.numpy(), mel, want, kind, mag)
    warped = [bool((kind[b] == S.WARPED).any()) for b in range(len(rows))]
    assert warped == [True] * 7 + [False] * 12 + [True]
    masked = [int((kind[b] == S.MASKED).sum()) for b in range(len(rows))]
    assert masked[12] == n_mels and masked[13] == 0 and masked[15] == 0 and masked[16] == 0
    assert masked[14] == 4 * T + 3 * (n_mels - 4) and masked[17] == n_mels * T and masked[18] == n_mels * (T - 2)
    assert np.array_equal(out.numpy()[13].view(np.int32), mel[13].view(np.int32))
    # int64 parameters beyond int32 are as far outside as the limit
    wide = torch.from_numpy(params).long()
    wide[14, 9] = 1 << 40
    again, _ = augment.spec_augment(torch.from_numpy(mel), torch.tensor(lens), seed=0, params=wide, time_warp_mode=mode, n_freq_masks=2, n_time_masks=2)
    assert np.array_equal(again.numpy().view(np.int32), out.numpy().view(np.int32))


def test_spec_augment_refuses_what_the_entries_refuse():
    mel = torch.zeros(2, 8, 20)
    bad = [dict(time_warp_mode="cubic"), dict(n_freq_masks=9), dict(n_time_masks=17), dict(n_freq_masks=-1), dict(time_warp_window=-1),
           dict(time_mask_ratio=-0.1), dict(time_mask_ratio=NAN), dict(time_mask_ratio=INF), dict(time_mask_ratio=1e39), dict(mask_value=NAN),
           dict(freq_mask_width=-2), dict(time_mask_width=-1), dict(params=torch.zeros(2, 15, dtype=torch.int32)),
           dict(params=torch.zeros(2, 16)), dict(frame_len=torch.zeros(3, dtype=torch.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            augment.spec_augment(mel, kw.pop("frame_len", None), seed=1, **kw)
    for wrong in (mel.double(), mel[0], torch.zeros(2, 0, 20), torch.zeros(2, 8, 0)):
        with pytest.raises(ValueError):
            augment.spec_augment(wrong, seed=1)
    out, params = augment.spec_augment(torch.zeros(0, 8, 20), seed=1)
    assert out.shape == (0, 8, 20) and params.shape == (0, 16)


# ---------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_module_is_the_identity_in_eval_mode_and_counts_its_calls():
    mel = torch.from_numpy(S.mel_batch(3, 23, 37, seed=4))
    lens = torch.tensor([37, 30, 11])
    aug = augment.SpecAugment(seed=77, time_mask_ratio=0.2)
    assert not list(aug.state_dict()) and not list(aug.parameters())
    assert aug.eval()(mel, lens) is mel and aug.get_state() == {"seed": 77, "calls": 0} and aug.last_params is None
    aug.train()
    first = aug(mel, lens)
    p_first = aug.last_params.clone()
    state = aug.get_state()
    second = aug(mel, lens)
    p_second = aug.last_params.clone()
    assert state == {"seed": 77, "calls": 1} and aug.get_state()["calls"] == 2
    assert not torch.equal(p_first, p_second) and first is not mel and first.shape == mel.shape
    want, _ = augment.spec_augment(mel, lens, seed=77, time_mask_ratio=0.2)
    assert np.array_equal(first.numpy().view(np.int32), want.numpy().view(np.int32))
    # resuming: a fresh module put into the recorded state repeats the step that followed
    other = augment.SpecAugment(seed=1, time_mask_ratio=0.2)
    other.set_state(state)
    again = other(mel, lens)
    assert torch.equal(other.last_params, p_second) and np.array_equal(again.numpy().view(np.int32), second.numpy().view(np.int32))
    assert other.get_state() == aug.get_state()
    torch.manual_seed(3)
    a = augment.SpecAugment().seed
    torch.manual_seed(3)
    assert augment.SpecAugment().seed == a


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries' refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


FAKE = 0x10000
BAD_ARG = 10001


def _draw(lib, **over):
    a = dict(frame_len=FAKE, B=3, n_mels=80, T=100, seed=1, utt=0, W=5, nf=2, F=27, nt=5, ratio=0.05, Tmax=100, params=FAKE)
    a.update(over)
    return lib.eec_specaug_draw(a["frame_len"], a["B"], a["n_mels"], a["T"], a["seed"], a["utt"], a["W"], a["nf"], a["F"], a["nt"], a["ratio"],
                                a["Tmax"], a["params"], None)


def _apply(lib, **over):
    a = dict(mel=FAKE, frame_len=FAKE, params=FAKE, B=3, n_mels=80, T=100, nf=2, nt=5, mode=1, value=0.0, out=2 * FAKE)
    a.update(over)
    return lib.eec_specaug_apply(a["mel"], a["frame_len"], a["params"], a["B"], a["n_mels"], a["T"], a["nf"], a["nt"], a["mode"], a["value"],
                                 a["out"], None)


SHAPE_REFUSALS = [dict(B=-1), dict(n_mels=0), dict(T=0), dict(T=-5), dict(nf=9), dict(nf=-1), dict(nt=17), dict(nt=-1)]
DRAW_REFUSALS = SHAPE_REFUSALS + [dict(W=-1), dict(F=-1), dict(Tmax=-1), dict(ratio=-0.5), dict(ratio=NAN), dict(ratio=INF), dict(ratio=-INF),
                                  dict(params=None), dict(B=0, W=-1), dict(B=0, nt=17)]
APPLY_REFUSALS = SHAPE_REFUSALS + [dict(mode=2), dict(mode=-1), dict(value=NAN), dict(mel=None), dict(params=None), dict(out=None),
                                   dict(out=FAKE), dict(B=0, mode=7), dict(B=0, value=NAN)]


def test_the_entries_refuse_bad_arguments_before_any_device_work(lib):
    """The addresses are plausible but unusable: a call that got past its checks would fault, not return."""
    for case in DRAW_REFUSALS:
        assert _draw(lib, **case) == BAD_ARG, case
        assert lib.eec_last_error().decode().startswith("specaug draw: "), case
    for case in APPLY_REFUSALS:
        assert _apply(lib, **case) == BAD_ARG, case
        assert lib.eec_last_error().decode().startswith("specaug apply: "), case
    assert b"NaN" in lib.eec_last_error()


def test_an_empty_batch_is_a_successful_no_op(lib):
    assert _draw(lib, B=0) == 0 and _draw(lib, B=0, params=None, frame_len=None) == 0
    assert _apply(lib, B=0) == 0 and _apply(lib, B=0, mel=None, params=None, out=None, frame_len=None) == 0
