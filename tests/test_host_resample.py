"""CPU tests of resampling and speed perturbation: the restatement of tests/resample_cases.py against the strided-convolution form
of torchaudio's ``functional.resample`` in fp64 and against an analytic sinusoid, the library's plan against the restated table, every
refusal (checked before any device work, so they run without a GPU), the NumPy host path against the restatement fed the library's
plan, the draw and the module."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as S
from early_exit_transformer_amd import augment, capi
from early_exit_transformer_amd.build import LIB_PATH

NAN = float("nan")
RATIOS = [(9, 10), (11, 10), (1, 2), (3, 1), (441, 160), (441, 320)]


@functools.lru_cache(maxsize=None)
def _table(o, n, lpw=6, rolloff=0.99):
    return S.plan_fp64(o, n, lpw, rolloff)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement against the strided-convolution form
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_form(x, table):
    """torchaudio's ``_apply_sinc_resample_kernel`` in fp64: pad, one strided convolution with the n phase rows, interleave, cut."""
    o, n, width, h = table["o"], table["n"], table["width"], table["h"]
    length = x.shape[0]
    wave = F.pad(torch.from_numpy(x)[None, None], (width, width + o))
    y = F.conv1d(wave, torch.from_numpy(h)[:, None, :], stride=o)  # [1, n, frames]
    y = y.transpose(1, 2).reshape(-1)
    return y[:math.ceil(n * length / o)].numpy()


@pytest.mark.parametrize("o,n", RATIOS)
def test_the_restatement_is_the_strided_convolution(o, n):
    t = _table(o, n)
    rng = np.random.default_rng(o * 1000 + n)
    worst = 0.0
    for length in (0, 1, t["width"] - 1, t["width"], o, t["K"], 1000):
        x = rng.standard_normal(length)
        got, _ = S.resample_fp64(x, length, t)
        want = _conv_form(x, t)
        assert got.shape == want.shape and got.shape[0] == S.out_len(length, o, n), (length, got.shape, want.shape)
        if length:
            err = float(np.abs(got - want).max() / np.abs(x).max())
            worst = max(worst, err)
            assert err <= 1e-12, (length, err)
    print(f"restatement vs conv1d form, {o} -> {n}: worst error {worst:.2e} of max|x|")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the filter is the right filter
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0.9, 1.1])
def test_a_sinusoid_comes_out_as_the_sinusoid_at_the_new_rate(factor):
    """1 kHz at 16 kHz, resampled by (int(f * 16000), 16000): sample i of the output sits at time i * o / (n * 16000)."""
    o, n = S.speed_ratio(factor)
    assert (o, n) == {0.9: (9, 10), 1.1: (11, 10)}[factor]
    length = 4000
    x = np.sin(2.0 * math.pi * 1000.0 * np.arange(length) / 16000.0)
    y, _ = S.resample_fp64(x, length, _table(o, n))
    i = np.arange(y.shape[0])
    want = np.sin(2.0 * math.pi * 1000.0 * i * o / (n * 16000.0))
    err = float(np.abs(y - want)[200:-200].max())
    print(f"unit 1 kHz sinusoid through {o} -> {n}: worst error {err:.2e}")
    assert err <= 2e-3


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the library's plan
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


def _arr(values):
    return (C.c_int32 * len(values))(*values)


def test_the_plan_is_the_restated_table_rounded_to_fp32(lib):
    ratios = RATIOS + [(1, 1)]
    orig, new = _arr([o for o, _ in ratios]), _arr([n for _, n in ratios])
    nbytes = lib.eec_resample_plan_bytes(len(ratios), orig, new, 6, 0.99)
    assert nbytes > 0 and nbytes % 4 == 0
    guard = 16
    img = np.full(nbytes // 4 + guard, -12345, dtype=np.int32)
    assert lib.eec_resample_plan(len(ratios), orig, new, 6, 0.99, img.ctypes.data, nbytes) == 0
    assert (img[nbytes // 4:] == -12345).all() and img[0] == augment.RESAMPLE_MAGIC and img[1] == len(ratios) and img[2] == nbytes // 4
    at = 4 + 8 * len(ratios)
    for r, (o, n) in enumerate(ratios):
        t = _table(o, n)
        ro, rn, width, K, phases, weights, total, most = (int(v) for v in img[4 + 8 * r:12 + 8 * r])
        assert (ro, rn, width, K) == (o, n, t["width"], t["K"]) and phases == at and weights == at + 3 * n
        ph = img[phases:phases + 3 * n].reshape(n, 3)
        w32 = img[weights:weights + total].view(np.float32)
        scale = min(o, n) * 0.99 / o
        cursor = 0
        for j in range(n):
            first, count, off = (int(v) for v in ph[j])
            assert off == cursor and 0 <= first and first + count <= K and count <= most
            got = np.zeros(K, dtype=np.float64)
            got[first:first + count] = w32[off:off + count]
            assert np.abs(got - t["h"][j]).max() <= 2.0 ** -23 * scale
            assert count > 0 and w32[off] != 0.0 and w32[off + count - 1] != 0.0  # compact: no zero head or tail is stored
            outside = np.ones(K, dtype=bool)  # ... and what is not stored is zero
            outside[first:first + count] = False
            assert np.abs(t["h"][j][outside]).max(initial=0.0) <= 2.0 ** -23 * scale
            cursor += count
        assert cursor == total and most == ph[:, 1].max()
        at = weights + total
    assert at == nbytes // 4
    # the Python wrapper reads the same image
    plan = augment.resample_plan(ratios)
    assert plan.ratios == ratios and np.array_equal(plan.image, img[:nbytes // 4]) and augment.resample_plan(list(ratios)) is plan
    assert plan.out_samples(3000) == 6000
    # unreduced rates give the reduced ratio's table; another width and rolloff another one
    assert np.array_equal(augment.resample_plan([(14400, 16000)]).image, augment.resample_plan([(9, 10)]).image)
    t = S.plan_fp64(3, 2, 16, 0.9)
    o, n, width, K, first, count, w = augment.resample_plan([(48000, 32000)], 16, 0.9).table(0)
    assert (o, n, width, K) == (3, 2, t["width"], t["K"])
    assert np.abs(S.dense(o, n, width, K, first, count, w)["h"] - t["h"]).max() <= 2.0 ** -23 * (2 * 0.9 / 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------
FAKE = 0x10000
BAD_ARG = 10001


def _stale(lib):
    assert lib.eec_specaug_apply(None, None, None, 1, 1, 1, 0, 0, 1, 0.0, None, None) != 0
    return lib.eec_last_error()


def test_the_plan_entries_refuse_bad_arguments(lib):
    one, two = _arr([9]), _arr([10])
    nine = _arr([9] * 9)
    buf = np.zeros(4096, dtype=np.int32)
    cases = {
        "max(o, n) = 641": (1, _arr([641]), _arr([640]), 6, 0.99),
        "n = 641": (1, _arr([1]), _arr([641]), 6, 0.99),
        "R = 9": (9, nine, nine, 6, 0.99),
        "R = 0": (0, one, two, 6, 0.99),
        "lpw = 0": (1, one, two, 0, 0.99),
        "lpw = 65": (1, one, two, 65, 0.99),
        "rolloff = 0": (1, one, two, 6, 0.0),
        "rolloff = 1.5": (1, one, two, 6, 1.5),
        "rolloff NaN": (1, one, two, 6, NAN),
        "a rate of 0": (1, _arr([0]), two, 6, 0.99),
        "null orig": (1, None, two, 6, 0.99),
        "null new": (1, one, None, 6, 0.99),
    }
    for name, args in cases.items():
        stale = _stale(lib)
        assert lib.eec_resample_plan_bytes(*args) == 0, name
        msg = lib.eec_last_error()
        assert msg.startswith(b"resample plan: ") and msg != stale, (name, msg)
        stale = _stale(lib)
        assert lib.eec_resample_plan(*args, buf.ctypes.data, buf.nbytes) == BAD_ARG, name
        assert lib.eec_last_error().startswith(b"resample plan: ") and lib.eec_last_error() != stale, name
    assert not buf.any()
    # 1282 / 1280 reduces to 641 / 640; 1280 / 1278 to 640 / 639, which is served
    assert lib.eec_resample_plan_bytes(1, _arr([1282]), _arr([1280]), 6, 0.99) == 0
    assert lib.eec_resample_plan_bytes(1, _arr([1280]), _arr([1278]), 6, 0.99) > 0
    need = lib.eec_resample_plan_bytes(1, one, two, 6, 0.99)
    assert lib.eec_resample_plan(1, one, two, 6, 0.99, None, need) == BAD_ARG and b"null image" in lib.eec_last_error()
    assert lib.eec_resample_plan(1, one, two, 6, 0.99, buf.ctypes.data, need - 1) == 10003 and not buf.any()  # EEC_ERR_WORKSPACE
    assert lib.eec_resample_plan(1, one, two, 6, 0.99, buf.ctypes.data, need) == 0 and buf[0] == augment.RESAMPLE_MAGIC


def test_the_device_entries_refuse_bad_arguments_before_any_device_work(lib):
    """The addresses are plausible but unusable: a call that got past its checks would fault, not return."""
    def draw(**over):
        a = dict(lengths=FAKE, B=3, L=100, plan=FAKE, choice=FAKE, out_len=FAKE)
        a.update(over)
        return lib.eec_speed_draw(a["lengths"], a["B"], a["L"], 1, 0, a["plan"], a["choice"], a["out_len"], None)

    def lengths(**over):
        a = dict(lengths=FAKE, choice=FAKE, B=3, L=100, plan=FAKE, out_len=FAKE)
        a.update(over)
        return lib.eec_resample_lengths(a["lengths"], a["choice"], a["B"], a["L"], a["plan"], a["out_len"], None)

    def run(**over):
        a = dict(wave=FAKE, lengths=FAKE, choice=FAKE, B=3, L=100, plan=FAKE, out=2 * FAKE, L_out=112, out_len=FAKE)
        a.update(over)
        return lib.eec_resample(a["wave"], a["lengths"], a["choice"], a["B"], a["L"], a["plan"], a["out"], a["L_out"], a["out_len"], None)

    shape = [dict(B=-1), dict(L=-1), dict(L=(1 << 30) + 1)]
    for call, who, more in ((draw, b"speed draw: ", [dict(plan=None), dict(choice=None), dict(out_len=None)]),
                            (lengths, b"resample lengths: ", [dict(plan=None), dict(choice=None), dict(out_len=None)]),
                            (run, b"resample: ", [dict(plan=None), dict(choice=None), dict(wave=None), dict(out=None), dict(out=FAKE),
                                                  dict(L_out=-1), dict(B=0, L=-1)])):
        for case in shape + more:
            stale = _stale(lib)
            assert call(**case) == BAD_ARG, (who, case)
            assert lib.eec_last_error().startswith(who) and lib.eec_last_error() != stale, (who, case)
        assert call(B=0) == 0
    assert run(B=0, wave=None, lengths=None, choice=None, plan=None, out=None, out_len=None) == 0


def test_the_python_layer_refuses_with_value_errors():
    wave = torch.zeros(2, 50)
    for bad in (wave.double(), wave.half(), torch.zeros(2, 3, 50), torch.zeros(()), "wave"):
        with pytest.raises(ValueError):
            augment.resample(bad, orig_freq=9, new_freq=10)
        with pytest.raises(ValueError):
            augment.speed_perturb(bad, seed=1)
    for kw in (dict(lengths=torch.zeros(3, dtype=torch.int64)), dict(lengths=torch.zeros(2)), dict(choice=torch.zeros(3, dtype=torch.int32)),
               dict(choice=torch.zeros(2)), dict(factors=()), dict(factors=(0.9,) * 9), dict(factors=(0.0,)), dict(factors=(-1.0,)),
               dict(factors=(NAN,)), dict(factors=(0.9, 1.0003)), dict(sample_rate=0), dict(lowpass_filter_width=0),
               dict(lowpass_filter_width=65), dict(lowpass_filter_width=6.5), dict(rolloff=0.0), dict(rolloff=1.5)):
        with pytest.raises(ValueError):
            augment.speed_perturb(wave, kw.pop("lengths", None), seed=1, **kw)
    for kw in (dict(orig_freq=641, new_freq=640), dict(orig_freq=0, new_freq=1), dict(orig_freq=16000.5, new_freq=8000),
               dict(orig_freq=2, new_freq=1, rolloff=-1.0)):
        with pytest.raises(ValueError, match="resample"):
            augment.resample(wave, **kw)
    with pytest.raises(ValueError, match="641"):
        augment.resample(wave, orig_freq=1282, new_freq=1280)
    with pytest.raises(ValueError):
        augment.SpeedPerturb(seed=1, factors=())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the NumPy host path
# ---------------------------------------------------------------------------------------------------------------------------
_CALL = {tuple(S.SPEED_RATIOS): dict(factors=S.SPEED_FACTORS, sample_rate=S.SPEED_RATE),
         tuple(S.RATE_RATIOS): dict(factors=S.RATE_FACTORS, sample_rate=S.RATE_RATE)}


def _library_table(plan, r):
    return S.dense(*plan.table(r))


def _check_batch(out, out_len, wave, lens, choice, plan):
    """``out`` [B, L_out] fp32 against ``resample_fp64`` fed the library's plan; returns the worst share of the bound used."""
    worst = 0.0
    assert out.dtype == np.float32 and out_len.dtype == np.int64 and not np.isnan(out).any()
    for b, (n, c) in enumerate(zip(lens, choice)):
        o, nn = plan.ratios[c]
        m = S.out_len(n, o, nn)
        assert out_len[b] == m and (out[b, m:].view(np.int32) == 0).all()
        if (o, nn) == (1, 1):
            assert np.array_equal(out[b, :m].view(np.int32), wave[b, :n].view(np.int32))
            continue
        t = _library_table(plan, c)
        want, mag = S.resample_fp64(wave[b], n, t)
        share = S.share_of_bound(out[b, :m], want, S.bound(t, mag))
        assert share <= 1.0, (b, n, c, share)
        worst = max(worst, share)
    return worst


@pytest.mark.parametrize("ratios", [S.SPEED_RATIOS, S.RATE_RATIOS], ids=["speed", "rates"])
def test_the_host_path_is_the_restatement_with_the_librarys_plan(ratios):
    plan = augment.resample_plan(ratios)
    worst = 0.0
    for k, (lens, choice) in enumerate(S.batches(len(ratios))):
        wave = S.wave_batch(40 + k, lens)
        out, out_len, back = augment.speed_perturb(torch.from_numpy(wave), torch.tensor(lens), seed=0, choice=torch.tensor(choice, dtype=torch.int32),
                                                   **_CALL[tuple(ratios)])
        assert out.shape == (S.B, plan.out_samples(S.L)) and back.tolist() == choice
        worst = max(worst, _check_batch(out.numpy(), out_len.numpy(), wave, lens, choice, plan))
    print(f"host path {ratios}: worst output at {worst:.3f} of (K_nz + 1) 2^-24 sum |h||x|")
    assert worst > 0.0


def test_speed_ratios_are_those_of_transforms_speed():
    assert [S.reduce(*r) for r in augment.speed_ratios((0.9, 1.0, 1.1), 16000)] == [(9, 10), (1, 1), (11, 10)]
    assert augment.speed_ratios((0.9, 1.1), 16000) == [(int(0.9 * 16000), 16000), (int(1.1 * 16000), 16000)]
    assert [S.reduce(*r) for r in augment.speed_ratios(S.RATE_FACTORS, S.RATE_RATE)] == S.RATE_RATIOS
    assert [S.reduce(*r) for r in augment.speed_ratios(S.SPEED_FACTORS, S.SPEED_RATE)] == S.SPEED_RATIOS


def test_resample_and_its_edges_on_the_host():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 700)).astype(np.float32)
    lens = [700, 333, 0]
    x[1, 333:] = NAN
    x[2, :] = NAN
    wave = torch.from_numpy(x)
    # equal rates: the input's bits, zeros past the lengths
    out, n = augment.resample(wave, torch.tensor(lens), orig_freq=16000, new_freq=16000)
    assert n.dtype == torch.int64 and n.tolist() == lens and out.shape == (3, 700)
    assert np.array_equal(out.numpy()[0].view(np.int32), x[0].view(np.int32)) and np.array_equal(out.numpy()[1, :333].view(np.int32), x[1, :333].view(np.int32))
    assert (out.numpy()[1, 333:].view(np.int32) == 0).all() and (out.numpy()[2].view(np.int32) == 0).all()
    # 44.1 kHz -> 16 kHz, int32 lengths beyond L are clamped, a 1-D wave
    out, n = augment.resample(wave, torch.tensor([900, 333, 0], dtype=torch.int32), orig_freq=44100, new_freq=16000)
    plan = augment.resample_plan([(441, 160)])
    assert out.shape == (3, S.out_len(700, 441, 160))
    _check_batch(out.numpy(), n.numpy(), x, lens, [0, 0, 0], plan)
    one, n1 = augment.resample(wave[1, :333], orig_freq=44100, new_freq=16000)
    assert one.dim() == 1 and n1.item() == n[1].item() and np.array_equal(one.numpy().view(np.int32), out.numpy()[1, :n1].view(np.int32))
    # no lengths: L everywhere; an utterance alone equals its row of the batch
    clean = torch.from_numpy(rng.standard_normal((2, 100)).astype(np.float32))
    a, na = augment.resample(clean, orig_freq=8000, new_freq=16000)
    b, nb = augment.resample(clean, torch.tensor([100, 100]), orig_freq=8000, new_freq=16000)
    assert na.tolist() == [200, 200] and torch.equal(na, nb) and np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))
    # a choice outside the factors copies
    out, n, c = augment.speed_perturb(clean, seed=0, choice=torch.tensor([7, -3]))
    assert n.tolist() == [100, 100] and torch.equal(out[:, :100], clean) and not out[:, 100:].any()
    empty, ne, ce = augment.speed_perturb(torch.zeros(0, 10), seed=0)
    assert empty.shape == (0, 12) and ne.shape == (0,) and ce.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the draw and the module
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_host_draw_is_the_restated_draw():
    wave = torch.zeros(3000, 1)
    seed = 20240917
    _, n, whole = augment.speed_perturb(wave, seed=seed, utt_offset=5)
    want = S.draw(seed, 5, 3000, 3)
    assert whole.dtype == torch.int32 and np.array_equal(whole.numpy(), want)
    counts = np.bincount(want, minlength=3)
    print(f"3000 draws among three factors: {counts.tolist()}")
    assert counts.shape == (3,) and (counts >= 900).all() and (counts <= 1100).all()
    assert n.tolist() == [S.out_len(1, *[(9, 10), (1, 1), (11, 10)][c]) for c in want]
    for a in (1, 129, 2999):
        _, _, lo = augment.speed_perturb(wave[:a], seed=seed, utt_offset=5)
        _, _, hi = augment.speed_perturb(wave[a:], seed=seed, utt_offset=5 + a)
        assert torch.equal(torch.cat([lo, hi]), whole)
    assert not np.array_equal(S.draw(seed + 1, 5, 3000, 3), want)
    big = (1 << 64) - 3  # the index wraps mod 2^64
    _, _, c = augment.speed_perturb(wave[:8], seed=seed, utt_offset=big)
    assert np.array_equal(c.numpy(), S.draw(seed, big, 8, 3)) and np.array_equal(c.numpy()[3:], S.draw(seed, 0, 5, 3))
    _, _, c = augment.speed_perturb(wave[:300], seed=seed, factors=(0.9, 0.95, 1.0, 1.05, 1.1))
    assert np.array_equal(c.numpy(), S.draw(seed, 0, 300, 5)) and set(c.tolist()) == set(range(5))


def test_the_module_is_the_identity_in_eval_mode_and_counts_its_calls():
    wave = torch.from_numpy(np.random.default_rng(4).standard_normal((6, 90)).astype(np.float32))
    lens = torch.tensor([90, 80, 50, 11, 1, 0])
    speed = augment.SpeedPerturb(seed=77)
    assert not list(speed.state_dict()) and not list(speed.parameters()) and not list(speed.buffers())
    same, same_n = speed.eval()(wave, lens)
    assert same is wave and same_n is lens and speed.get_state() == {"seed": 77, "calls": 0} and speed.last_choice is None
    speed.train()
    first, n_first = speed(wave, lens)
    c_first = speed.last_choice.clone()
    state = speed.get_state()
    second, n_second = speed(wave, lens)
    c_second = speed.last_choice.clone()
    assert state == {"seed": 77, "calls": 1} and speed.get_state()["calls"] == 2
    assert np.array_equal(c_first.numpy(), S.draw(77, 0, 6, 3))
    assert np.array_equal(c_second.numpy(), S.draw((77 + 0x9E3779B97F4A7C15) & S.M64, 0, 6, 3)) and not torch.equal(c_first, c_second)
    want, want_n, _ = augment.speed_perturb(wave, lens, seed=77)
    assert first.shape == (6, 100) and torch.equal(n_first, want_n) and np.array_equal(first.numpy().view(np.int32), want.numpy().view(np.int32))
    # resuming: a fresh module put into the recorded state repeats the step that followed
    other = augment.SpeedPerturb(seed=1)
    other.set_state(state)
    again, n_again = other(wave, lens)
    assert torch.equal(other.last_choice, c_second) and torch.equal(n_again, n_second)
    assert np.array_equal(again.numpy().view(np.int32), second.numpy().view(np.int32)) and other.get_state() == speed.get_state()
    torch.manual_seed(3)
    a = augment.SpeedPerturb().seed
    torch.manual_seed(3)
    assert augment.SpeedPerturb().seed == a
