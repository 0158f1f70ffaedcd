"""The folded stem (csrc/stem.hip, stem_fold_kernel): the two Conv1d(k=3, stride=2) of Conv1dSubampling run as ONE
Conv1d(k=7, stride=4) whose weights are composed at pack time.  Every test compares the encoder's sub-step 0
(``_run_encoder(..., stop_after=0, want_x=True)``) with an fp64 evaluation of the two reference convolutions + PE.

Statistic and bound are those of test_stem_dynamic_range: per utterance, max|delta| / max|want| < 2e-5."""
import pytest
import torch
import torch.nn.functional as F

from conftest import base_kwargs
from early_exit_transformer_amd import synth
from early_exit_transformer_amd.model import Early_conformer

pytestmark = pytest.mark.gpu
BOUND = 2e-5


def make_model(n_mels=80, d_model=256, seed=23):
    kw = base_kwargs(n_enc_exits=1, n_enc_layers=1, d_feed_forward=256, features_length=n_mels, d_model=d_model, n_head=8,
                     device="cuda")
    gpu = Early_conformer(**kw).eval()
    gpu.load_state_dict(synth.synth_state_dict(gpu.state_dict(), seed=seed, style="trained"))
    return gpu.cuda()


@pytest.fixture(scope="module")
def model80():
    return make_model()


def stem_params64(model):
    c = model.conv_subsample.sequential
    return [p.detach().cpu().double() for p in (c[0].weight, c[0].bias, c[1].weight, c[1].bias)]


def want64(model, mel):
    """fp64: the two reference convolutions, transpose, + PE."""
    w1, b1, w2, b2 = stem_params64(model)
    y = F.conv1d(F.conv1d(mel.double(), w1, b1, stride=2), w2, b2, stride=2).permute(0, 2, 1)
    return y + model.positional_encoder.pe[: y.size(1), 0].cpu().double()


def run_stem(model, mel):
    lens = torch.full((mel.size(0),), mel.size(2), dtype=torch.long)
    with torch.no_grad():
        x = model._run_encoder(mel.cuda(), lens, want_out=False, stop_after=0, want_x=True)[2]
    torch.cuda.synchronize()
    return x.cpu()


def rel_err(x, want):
    return ((x.double() - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2))).tolist()


def check(model, mel, tag):
    x, want = run_stem(model, mel), want64(model, mel)
    assert x.shape == want.shape
    rel = rel_err(x, want)
    print(f"\n[stem fold] {tag}: rel err per utterance {['%.1e' % r for r in rel]}")
    assert torch.isfinite(x).all() and max(rel) < BOUND, rel
    return x, want


@pytest.mark.parametrize("T", [7, 10, 11, 259, 262, 263, 519])
def test_frame_geometry(model80, T):
    """T' = 1; T' = 1 with three unused trailing frames; T' = 2; exactly one tile; one tile plus unused trailing frames; one
    row into a second tile; two tiles plus one row.  Unused trailing frames may hold anything."""
    mel = synth.synth_mel(3, 80, T, seed=T)
    x, _ = check(model80, mel, f"T={T}")
    Tq = x.size(1)
    assert Tq == ((T - 3) // 2 + 1 - 3) // 2 + 1
    if T in (10, 262):
        assert 4 * (Tq - 1) + 7 < T
        bad = mel.clone()
        bad[..., 4 * (Tq - 1) + 7:] = float("nan")
        y = run_stem(model80, bad)
        assert torch.isfinite(y).all() and torch.equal(x, y)


@pytest.mark.parametrize("n_mels,d_model", [(16, 256), (128, 256), (80, 512)])
def test_shapes_of_k_and_n(n_mels, d_model):
    model = make_model(n_mels, d_model, seed=29)
    check(model, synth.synth_mel(2, n_mels, 135, seed=31), f"n_mels={n_mels} D={d_model}")


def test_bias_path():
    model = make_model(seed=37)
    conv = model.conv_subsample.sequential
    with torch.no_grad():
        conv[0].bias.mul_(100.0)
    mel = torch.zeros(2, 80, 135)
    x, want = check(model, mel, "zero mel, b1 x 100")
    w1, b1, w2, b2 = stem_params64(model)
    b_eff = b2 + torch.einsum("ocj,c->o", w2, b1)
    pe = model.positional_encoder.pe[: x.size(1), 0].cpu().double()
    assert (want - (b_eff + pe)).abs().max() < 1e-12 * want.abs().max()  # the reference itself is b_eff + PE here
    assert ((x.double() - (b_eff + pe)).abs().max() / (b_eff + pe).abs().max()).item() < BOUND
    with torch.no_grad():
        conv[0].bias.zero_()
        conv[1].bias.zero_()
    check(model, synth.synth_mel(2, 80, 135, seed=41), "b1 = b2 = 0")


def rows_touching(frame, Tq):
    return [t for t in range(Tq) if 4 * t <= frame <= 4 * t + 6]


@pytest.mark.parametrize("case", ["alternating", "loud_frame", "outlier_bin", "zeros"])
def test_domains_inside_one_window(model80, case):
    B, T = 4, 259
    mel = synth.synth_mel(B, 80, T, seed=43)
    if case == "alternating":
        mel[..., 0::2] *= 1e7
        mel[..., 1::2] *= 1e-8
    elif case == "loud_frame":
        for b in range(B):
            mel[b, :, 100 + b] = 3.0e6  # every frame phase
    elif case == "outlier_bin":
        for b in range(B):
            mel[b, 5 + b, 17 + b] = 9.9e6
    else:
        mel[0] = 0.0
        mel[1, :, 40:75] = 0.0
        mel[2, :, :9] = 0.0
        mel[3, :, 250:] = 0.0
    x, want = check(model80, mel, case)
    if case == "loud_frame":
        # a burst must not cost the rows that do not see it: those meet the bound relative to their OWN row maximum
        row_rel = (x.double() - want).abs().amax(dim=2) / want.abs().amax(dim=2)
        for b in range(B):
            keep = torch.ones(x.size(1), dtype=torch.bool)
            keep[rows_touching(100 + b, x.size(1))] = False
            assert row_rel[b][keep].max().item() < BOUND, (b, row_rel[b][keep].max().item())


def test_non_finite_input(model80):
    B, T = 2, 263
    mel = synth.synth_mel(B, 80, T, seed=47)
    want = want64(model80, mel)
    bad = mel.clone()
    bad[0, 11, 130] = float("nan")
    bad[1, 79, 258] = float("nan")  # the first frame of the second tile's first row
    x = run_stem(model80, bad)
    for b, f in ((0, 130), (1, 258)):
        hit = torch.zeros(x.size(1), dtype=torch.bool)
        hit[rows_touching(f, x.size(1))] = True
        assert hit.any() and torch.isnan(x[b][hit]).all()
        rel = ((x[b][~hit].double() - want[b][~hit]).abs().max() / want[b].abs().max()).item()
        assert rel < BOUND, (b, rel)


@pytest.mark.parametrize("which", ["weight0", "bias1"])
def test_repack_follows_the_parameters(which):
    model = make_model(seed=53)
    mel = synth.synth_mel(2, 80, 135, seed=59)
    x0, _ = check(model, mel, f"before {which}")
    conv = model.conv_subsample.sequential
    with torch.no_grad():
        (conv[0].weight if which == "weight0" else conv[1].bias).mul_(1.5)
    x1, _ = check(model, mel, f"after {which}")  # against the fp64 stem of the NEW parameters
    assert not torch.equal(x0, x1)


def test_batch_independence(model80):
    mel = synth.synth_mel(4, 80, 263, seed=61)
    mel[1] *= 1e3
    mel[2] *= 1e-6
    x = run_stem(model80, mel)
    for i in range(4):
        assert torch.equal(x[i], run_stem(model80, mel[i:i + 1].clone())[0]), i
