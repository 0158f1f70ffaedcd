"""GPU tests of the mel front end (csrc/frontend.hip behind ``frontend.MelFrontend``) against the float64 oracle
(oracle/frontend_ref.py) on the shared cases of tests/frontend_cases.py: every signal, the valid lengths at the edges of a
hop and of a 32-frame workgroup, impulses that localise a frame and a reflection, the configuration surface and the wrapper.
Bounds: 2e-5 of the frame's largest mel value and 1e-4 relative on the values above 1e-3 of that peak, unless a case says
bit-exact."""
import types

import pytest
import torch

import frontend_cases as FC
from oracle import frontend_ref as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    from early_exit_transformer_amd.frontend import MelFrontend
    return MelFrontend()


def _hold(got, want, what):
    """got (fp32, CPU) against the float64 want under the two measures; prints the figures before it asserts."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    e_peak, e_rel = FC.measures(got, want)
    print(f"  {what}: err_peak {e_peak:.2e} err_rel {e_rel:.2e}")
    assert e_peak < FC.BOUND_PEAK and e_rel < FC.BOUND_REL, (what, e_peak, e_rel)


def _hold_batch(got, wave, lengths, what, **kw):
    """Every row of a ragged call: its own frames against the oracle, exact zeros at and beyond its frame count."""
    B, Lmax = wave.shape
    assert got.shape == (B, kw.get("n_mels", FC.N_MELS), FC.n_frames(Lmax)), (what, got.shape)
    for b in range(B):
        n = min(max(int(lengths[b]), 0), Lmax)
        T = FC.n_frames(n)
        assert (got[b, :, T:] == 0).all(), (what, b, n)
        if T:
            _hold(got[b, :, :T], FR.mel_frontend_fp64(wave[b, :n], **kw), f"{what} row {b} (L = {n})")


def test_every_signal_default_configuration(fe):
    """One ragged call: the seven signals, each with its own valid length, NaN past it."""
    names = FC.SIGNAL_NAMES
    lens = [5121, 4960, 4961, 5119, 513, 4959, 5120]
    wave = FC.pad_nan(torch.stack([FC.signal(n) for n in names]), lens)
    got = fe(wave.cuda(), torch.tensor(lens)).cpu()
    _hold_batch(got, wave, lens, "signals")


def test_length_list(fe):
    """Every valid length of the list in one padded batch (NaN past each row's length: a finite output proves the padding is
    not read), plus a length above Lmax (taken as Lmax) and a negative one (taken as 0).  Lengths of 512 or fewer, where
    torch raises, are held to the oracle's reflect-then-clamp."""
    lens = list(FC.LENGTHS) + [FC.LENGTH_OVER, FC.LENGTH_NEGATIVE]
    wave = FC.noise_tone(len(lens), FC.LENGTHS_LMAX, seed=11)
    padded = FC.pad_nan(wave, lens)
    got = fe(padded.cuda(), torch.tensor(lens)).cpu()
    assert torch.isfinite(got).all()
    _hold_batch(got, wave, lens, "lengths")
    for b, n in enumerate(lens):
        if n <= 0:
            assert not got[b].any(), n
    # a length above Lmax equals the full-length row, and lengths=None equals lengths = Lmax, bit for bit
    full = fe(wave.cuda(), torch.full((len(lens),), FC.LENGTHS_LMAX)).cpu()
    assert torch.equal(got[lens.index(FC.LENGTH_OVER)], full[lens.index(FC.LENGTH_OVER)])
    assert torch.equal(fe(wave.cuda(), torch.full((len(lens),), FC.LENGTH_OVER)).cpu(), full)
    assert torch.equal(fe(wave.cuda()).cpu(), full)
    assert torch.equal(fe(wave.cuda(), None).cpu(), full)


@pytest.mark.parametrize("Lmax,Tmax", FC.LMAX_TMAX)
def test_lmax_around_a_workgroup(fe, Lmax, Tmax):
    """Tmax = 1, 31, 32, 33, 33: the last 32-frame workgroup is absent, full, or holds one frame.  Shape and every column,
    the last one included; one full row, one row that ends a hop short, one short row."""
    lens = [Lmax, max(Lmax - FC.HOP, 1), min(161, Lmax)]
    wave = FC.noise_tone(3, Lmax, seed=20 + Tmax)
    got = fe(FC.pad_nan(wave, lens).cuda(), torch.tensor(lens)).cpu()
    assert got.shape == (3, FC.N_MELS, Tmax)
    assert got[0, :, Tmax - 1].abs().max().item() > 0
    _hold_batch(got, wave, lens, f"Lmax {Lmax}")
    assert torch.equal(fe(wave[:1].cuda()).cpu()[0], got[0])


def test_impulse_sweep(fe):
    """330 rows, row i a unit impulse at sample 480 + i: every window slot of the covering frames, both parities of the
    staged rows.  Frames that do not cover the impulse are exactly 0; the others are w[slot]^2 sum_k fb[k][m]."""
    got = fe(FC.impulse_sweep().cuda()).cpu()
    assert got.shape == (FC.IMPULSE_ROWS, FC.N_MELS, FC.n_frames(FC.IMPULSE_LEN))
    slots = set()
    worst = (0.0, 0.0)
    for i in range(FC.IMPULSE_ROWS):
        n0 = FC.IMPULSE_N0 + i
        want = FC.impulse_mel(FC.IMPULSE_LEN, n0)
        cover = [t for t in range(want.size(1)) if 0 < n0 - FC.HOP * t + FC.WIN // 2 < FC.WIN]
        slots.update(n0 - FC.HOP * t + FC.WIN // 2 for t in cover)
        rest = [t for t in range(want.size(1)) if t not in cover]
        assert (got[i][:, rest] == 0).all(), n0
        assert (got[i][:, cover] > 0).all(), n0
        e = FC.measures(got[i][:, cover], want[:, cover])
        worst = tuple(max(a, b) for a, b in zip(worst, e))
        assert e[0] < FC.BOUND_PEAK and e[1] < FC.BOUND_REL, (n0, e)
    print(f"  impulse sweep: err_peak {worst[0]:.2e} err_rel {worst[1]:.2e}")
    assert slots == set(range(1, FC.WIN))


def test_edge_impulses(fe):
    """Impulses at samples 0, 1, L - 2 and L - 1, for L a multiple of the hop (the last frame is centred on the first sample
    past the end) and one more: reflection without edge repeat at both ends.  Sample 0 shows once in frame 0, sample 1 twice."""
    for L, n0 in FC.edge_impulses():
        got = fe(FC.impulse(L, n0).cuda()).cpu()
        want = FR.mel_frontend_fp64(FC.impulse(L, n0))
        cover = FC.covering_frames(L, n0)
        rest = [t for t in range(want.size(1)) if t not in cover]
        assert (got[:, rest] == 0).all(), (L, n0)
        _hold(got, want, f"impulse at {n0} of {L}")
    fs = FC.filter_sums()
    _hold(fe(FC.impulse(1600, 0).cuda()).cpu()[:, :1], fs.view(-1, 1), "impulse at 0, frame 0: once")
    _hold(fe(FC.impulse(1600, 1).cuda()).cpu()[:, :1], FC.impulse_at_one_frame0().view(-1, 1), "impulse at 1, frame 0: twice, coherent")


@pytest.mark.parametrize("n", [2500, 3, 4958])
def test_nan_inside_the_valid_region(fe, n):
    """A NaN at valid sample n: only the frames whose window covers it are non-finite (at most three), every other frame
    equals the run without the NaN bit for bit."""
    L = 4960
    x = FC.signal("tone")[:L].clone()
    clean = fe(x.cuda()).cpu()
    x[n] = float("nan")
    got = fe(x.cuda()).cpu()
    cover = FC.covering_frames(L, n)
    assert 1 <= len(cover) <= 3
    bad = [t for t in range(got.size(1)) if not torch.isfinite(got[:, t]).all()]
    assert set(bad) <= set(cover) and bad, (bad, cover)
    rest = [t for t in range(got.size(1)) if t not in cover]
    assert torch.equal(got[:, rest], clean[:, rest])


def test_shift_by_one_hop(fe):
    """160 samples prepended: interior frame t + 1 of the result is interior frame t of the original bit for bit -- the pairs
    fall in different rows of a workgroup and on either side of a workgroup boundary (72 frames)."""
    L = 71 * FC.HOP + 37
    x = FC.noise_tone(1, L, seed=31)[0]
    y = torch.cat([0.3 * torch.randn(FC.HOP, generator=torch.Generator().manual_seed(32)), x])
    a, b = fe(x.cuda()).cpu(), fe(y.cuda()).cpu()
    assert a.size(1) == 72 and b.size(1) == 73
    interior = [t for t in range(a.size(1)) if FC.HOP * t - FC.WIN // 2 >= 0 and FC.HOP * t + FC.WIN // 2 <= L]
    assert len(interior) >= 69 and {31, 32, 63, 64} <= set(interior)
    for t in interior:
        assert torch.equal(b[:, t + 1], a[:, t]), t
    _hold(a, FR.mel_frontend_fp64(x), "shift: original")


def test_scale_by_powers_of_two(fe):
    """mel(c x) = c^2 mel(x) bit for bit for c = 2^-10, 2^-4, 2^8, 2^15 on noise of amplitude 0.3: a power of two scales every
    product and every partial sum exactly as long as no intermediate leaves the normal fp32 range, which the float64 oracle's
    extremes confirm first.  A case that is not bit-exact is a flushed or overflowing intermediate."""
    L = 4000
    x = 0.3 * torch.randn(L, generator=torch.Generator().manual_seed(41))
    p = FR.power_spectrum_fp64(x.numpy())
    fb = FR.melscale_fbanks(FC.N_BINS, 0.0, 8000.0, FC.N_MELS, FC.SAMPLE_RATE).double()
    w = FR.hann_fp64(FC.WIN)
    tiny, huge = 2.0 ** -126, 2.0 ** 127
    # smallest product of the DFT: |x| min * smallest non-zero window weight * the smallest non-zero basis entry, cos(pi/2)
    # as fp64 rounds it (6.1e-17); smallest filter product: the smallest non-zero weight * the smallest power
    x_min, w_min, basis_min, fb_min = x.abs()[x != 0].min().item(), w[1], 6.0e-17, fb[fb > 0].min().item()
    for c in FC.SCALES:
        assert c * x_min * w_min * basis_min > tiny and c * c * p.min() * fb_min > tiny and p.min() > 0
        assert c * c * p.max() * 513 < huge and (c * x.abs().max().item() * FC.WIN) ** 2 < huge
    base = fe(x.cuda()).cpu()
    _hold(base, FR.mel_frontend_fp64(x), "scale: c = 1")
    for c in FC.SCALES:
        got = fe((x * c).cuda()).cpu()
        assert torch.equal(got, base * (c * c)), c


def test_configuration_surface():
    """Every (sample_rate, n_mels) pair on one two-row noise-plus-tone batch: the library's C-built filter table against
    torch's, through the mel output.  Where torch's table has an empty filter the output is exactly 0.  (A table whose mel
    points are laid out as m_max * i / (n + 1) from an fp32 log10, with powf, misses these bounds at 256 bins: 2.9e-5 of the
    peak at 8 kHz, 2.5e-5 at 11.025 kHz, 1.1e-4 relative at 44.1 kHz; with torch's own layout the worst are 8.2e-6 and 4.9e-5.)"""
    from early_exit_transformer_amd.frontend import MelFrontend
    lens = [2000, 1357]
    wave = FC.noise_tone(2, 2000, seed=51)
    padded = FC.pad_nan(wave, lens).cuda()
    power = [FR.power_spectrum_fp64(wave[b, :n].numpy()) for b, n in enumerate(lens)]
    failures = []
    for sr, nm in FC.CONFIGS:
        got = MelFrontend(sample_rate=sr, n_mels=nm)(padded, torch.tensor(lens)).cpu()
        assert got.shape == (2, nm, 13) and torch.isfinite(got).all(), (sr, nm)
        empty, want = FC.empty_filters(sr, nm), FC.config_reference(power, sr, nm)
        assert bool(empty) == ((sr, nm) in FC.EMPTY_FILTER_CONFIGS)
        for b, n in enumerate(lens):
            T = FC.n_frames(n)
            assert (got[b, :, T:] == 0).all()
            assert (got[b, empty] == 0).all(), (sr, nm, empty)
            e = FC.measures(got[b, :, :T], want[b][:, :T])
            print(f"  config ({sr}, {nm}) row {b}: err_peak {e[0]:.2e} err_rel {e[1]:.2e}")
            if not (e[0] < FC.BOUND_PEAK and e[1] < FC.BOUND_REL):
                failures.append((sr, nm, b, e))
    assert not failures, failures


def test_wrapper_dtypes_layouts_and_lengths(fe):
    x = FC.noise_tone(3, 1700, seed=61)
    lens = [1700, 1601, 900]
    dev = x.cuda()
    base = fe(dev, torch.tensor(lens)).cpu()
    # float64 and float16 waves: the wrapper's .float() is the conversion
    for dt in (torch.float64, torch.float16):
        xd = x.to(dt)
        assert torch.equal(fe(xd.cuda(), torch.tensor(lens)).cpu(), fe(xd.float().contiguous().cuda(), torch.tensor(lens)).cpu()), dt
    assert torch.equal(fe(x.double().cuda(), torch.tensor(lens)).cpu(), base)  # fp32 -> fp64 -> fp32 is the identity
    # a strided view
    wide = torch.zeros(3, 3400)
    wide[:, ::2] = x
    view = wide.cuda()[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(fe(view, torch.tensor(lens)).cpu(), base)
    tview = x.t().contiguous().cuda().t()
    assert not tview.is_contiguous() and torch.equal(fe(tview, torch.tensor(lens)).cpu(), base)
    # lengths: int32, int64, on the CPU, on the device
    for l in (torch.tensor(lens, dtype=torch.int32), torch.tensor(lens, dtype=torch.int64), torch.tensor(lens, dtype=torch.int32).cuda(),
              torch.tensor(lens).cuda()):
        assert torch.equal(fe(dev, l).cpu(), base), (l.dtype, l.device)
    # a 1-D wave is row 0 of the batch call
    one = fe(dev[0]).cpu()
    assert one.shape == (FC.N_MELS, 11) and torch.equal(one, base[0])
    _hold_batch(base, x, lens, "wrapper")


def test_wrapper_refusals(fe):
    from early_exit_transformer_amd.frontend import MelFrontend
    with pytest.raises(RuntimeError, match="HIP device"):
        fe(torch.zeros(2, 1000))
    with pytest.raises(RuntimeError, match="eec_frontend_forward"):
        fe(torch.zeros(2, 0).cuda())
    # a configuration the library refuses surfaces with the library's message
    for bad in (dict(n_fft=256), dict(win_length=400), dict(hop_length=80), dict(n_mels=257), dict(n_mels=0), dict(sample_rate=0)):
        with pytest.raises(RuntimeError, match="1024-point frames, window 320, hop 160"):
            MelFrontend(**bad)(torch.zeros(1, 1000).cuda())


def test_wrapper_stream_handle_and_namespace(fe):
    from early_exit_transformer_amd.frontend import MelFrontend
    x = FC.noise_tone(2, 3000, seed=71).cuda()
    base = fe(x).cpu()
    # a caller's stream, followed by work on that stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fe(x)
        twice = out * 2.0
    s.synchronize()
    assert torch.equal(out.cpu(), base) and torch.equal(twice.cpu(), base * 2.0)
    # one object, one handle
    mine = MelFrontend()
    assert mine._fe is None
    a = mine(x)
    h = mine._fe
    assert h is not None and h.value
    b = mine(x)
    assert mine._fe is h and torch.equal(a, b) and torch.equal(a.cpu(), base)
    assert mine.frames(3000) == 19 and mine.frames(0) == 0
    # the reference's flag names from a namespace (util/conf.py: n_fft is half the transform)
    args = types.SimpleNamespace(sample_rate=8000, n_fft=512, win_length=320, hop_length=160, n_mels=40, lr=1e-3)
    ns = MelFrontend(args)
    assert (ns.sample_rate, ns.n_fft, ns.win_length, ns.hop_length, ns.n_mels) == (8000, 512, 320, 160, 40)
    got = ns(x)
    assert got.shape == (2, 40, 19) and torch.equal(got, MelFrontend(sample_rate=8000, n_mels=40)(x))
    assert not torch.equal(got, MelFrontend(n_mels=40)(x))
    partial = MelFrontend(types.SimpleNamespace(n_mels=23))
    assert (partial.sample_rate, partial.n_fft, partial.n_mels) == (16000, 512, 23)
