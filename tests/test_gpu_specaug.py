"""GPU tests of SpecAugment (run with -m gpu on an MI355X): the two launches of csrc/specaug.hip through ``spec_augment`` against the
restatement of tests/specaug_cases.py -- the drawn parameters bit for bit, copied and masked elements exactly, warped elements within
6 * 2^-24 * sum_k |w_k| |x_k| of the fp64 value --, prescribed edge parameters, reproducibility, split and length independence, and one
training step of the small model on augmented input.

Shapes: B = 5; 80 and 23 mel rows (partial groups of 32); T = 37 and 131 (not multiples of 4; one partial and two tiles of 128
frames); lengths 0, 1, 2 W, 2 W + 1 and T with W = 5, the padding full of NaN."""
import functools

import numpy as np
import pytest
import torch

import specaug_cases as S
from early_exit_transformer_amd import augment, synth

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEED = 11


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _device(mel, lens=None, **kw):
    fl = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    out, params = augment.spec_augment(torch.from_numpy(mel).cuda(), fl, **kw)
    assert out.is_cuda and params.is_cuda and params.dtype == torch.int32 and out.data_ptr() != 0
    return out.cpu().numpy(), params.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _drawn_case(n_mels, T, cubic):
    """The shared input and its restated result: (mel, lengths, params, want, kind, mag); computed once, never written."""
    lens = S.lengths_of(T)
    mel = S.mel_batch(5, n_mels, T, seed=100 + T + n_mels, lengths=lens, pad=NAN)
    params = S.draw(lens, n_mels, T, SEED, utt_offset=7)
    return (mel, lens, params) + S.apply(mel, lens, params, 2, 5, cubic)


@pytest.mark.parametrize("mode", ["bicubic", "linear"])
@pytest.mark.parametrize("n_mels,T", S.SHAPES)
def test_the_kernels_equal_the_restatement(n_mels, T, mode):
    """Drawn parameters; two runs and a batch split at every utterance return the same bits."""
    mel, lens, want_p, want, kind, mag = _drawn_case(n_mels, T, mode == "bicubic")
    kw = dict(seed=SEED, time_warp_mode=mode)
    out, params = _device(mel, lens, utt_offset=7, **kw)
    assert np.array_equal(params, want_p)
    assert (kind[3] == S.WARPED).any() and (kind[4] == S.WARPED).any() and not (kind[:3] == S.WARPED).any()
    share = S.check_output(out, mel, want, kind, mag)
    print(f"specaug [{5}, {n_mels}, {T}] {mode}: worst warped element at {share:.3f} of the bound")
    for b, n in enumerate(lens):
        assert not np.isnan(out[b, :, :n]).any()
    again, _ = _device(mel, lens, utt_offset=7, **kw)
    assert np.array_equal(again.view(np.int32), out.view(np.int32))
    for a in range(1, 5):  # the halves start at other offsets into memory: other alignments of the rows
        lo, p_lo = _device(mel[:a].copy(), lens[:a], utt_offset=7, **kw)
        hi, p_hi = _device(mel[a:].copy(), lens[a:], utt_offset=7 + a, **kw)
        assert np.array_equal(np.concatenate([p_lo, p_hi]), params)
        assert np.array_equal(np.concatenate([lo, hi]).view(np.int32), out.view(np.int32))


@pytest.mark.parametrize("mode", ["bicubic", "linear"])
def test_no_lengths_means_every_frame(mode):
    n_mels, T = 23, 131
    mel = S.mel_batch(5, n_mels, T, seed=3)
    a, pa = _device(mel, None, seed=SEED, time_warp_mode=mode)
    b, pb = _device(mel, [T] * 5, seed=SEED, time_warp_mode=mode)
    assert np.array_equal(pa, pb) and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(pa, S.draw([T] * 5, n_mels, T, SEED)) and (pa[:, 0] >= S.W).all()
    want, kind, mag = S.apply(mel, None, pa, 2, 5, mode == "bicubic")
    S.check_output(a, mel, want, kind, mag)
    # int64 lengths from the host, as the collate hands them over
    c, pc = augment.spec_augment(torch.from_numpy(mel).cuda(), torch.full((5,), T + 9), seed=SEED, time_warp_mode=mode)
    assert np.array_equal(pc.cpu().numpy(), pa) and np.array_equal(_bits(c), a.view(np.int32))


@pytest.mark.parametrize("mode", ["bicubic", "linear"])
@pytest.mark.parametrize("n_mels,T", [(23, 37), (80, 131)])
def test_prescribed_edge_parameters(n_mels, T, mode):
    """c = W with w = 1, w = c + W, the extremes, rows that are ignored or clipped, masks over everything: five rows at a time, NaN in
    the padding frames."""
    rows = S.prescribed(n_mels, T)
    for at in range(0, len(rows), 5):
        lens = [n for n, _ in rows[at:at + 5]]
        params = np.array([r for _, r in rows[at:at + 5]], dtype=np.int32)
        mel = S.mel_batch(5, n_mels, T, seed=at, lengths=lens, pad=NAN)
        out, back = augment.spec_augment(torch.from_numpy(mel).cuda(), torch.tensor(lens, device="cuda"), seed=0, params=torch.from_numpy(params).cuda(),
                                         time_warp_mode=mode, n_freq_masks=2, n_time_masks=2)
        assert np.array_equal(back.cpu().numpy(), params)
        want, kind, mag = S.apply(mel, lens, params, 2, 2, mode == "bicubic")
        share = S.check_output(out.cpu().numpy(), mel, want, kind, mag)
        print(f"specaug prescribed rows {at}..{at + 4} [{n_mels}, {T}] {mode}: {share:.3f} of the bound")
        for b, n in enumerate(lens):
            assert not np.isnan(out.cpu().numpy()[b, :, :n]).any()


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "off-16-bytes"])
def test_without_a_warp_every_element_is_copied_or_masked(misaligned):
    """The quad path, and the same rows through single floats when the input does not start on a 16-byte boundary."""
    n_mels, T = 23, 131
    lens = [131, 77, 12, 1, 0]
    mel = S.mel_batch(5, n_mels, T, seed=2, lengths=lens, pad=NAN)
    dev = torch.from_numpy(mel).cuda()
    if misaligned:
        store = torch.empty(mel.size + 1, device="cuda")
        store[1:].copy_(dev.flatten())
        dev = store[1:].view(5, n_mels, T)
        assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    kw = dict(seed=5, time_warp_window=0, mask_value=-1.5, n_time_masks=3, time_mask_ratio=0.2, time_mask_width=9)
    out, params = augment.spec_augment(dev, torch.tensor(lens, device="cuda"), **kw)
    assert np.array_equal(params.cpu().numpy(), S.draw(lens, n_mels, T, 5, window=0, n_time=3, ratio=0.2, Tmax=9))
    want, kind, mag = S.apply(mel, lens, params.cpu().numpy(), 2, 3, True, -1.5)
    assert not (kind == S.WARPED).any() and (kind == S.MASKED).any()
    S.check_output(out.cpu().numpy(), mel, want, kind, mag, -1.5)
    host, host_p = augment.spec_augment(torch.from_numpy(mel), torch.tensor(lens), **kw)
    assert torch.equal(host_p, params.cpu()) and np.array_equal(_bits(host), _bits(out))


def test_one_training_step_on_augmented_input():
    """The geometry of ``smoke()``: train-mode forward, summed exit CTC loss and backward on what the module returns."""
    from early_exit_transformer_amd.model import Early_conformer, exit_ctc_losses
    kw = dict(src_pad_idx=0, n_enc_exits=2, enc_voc_size=256, dec_voc_size=256, d_model=256, n_head=8, max_len=2000, d_feed_forward=512,
              n_enc_layers=1, features_length=80, drop_prob=0.0, depthwise_kernel_size=31, device="cuda:0")
    model = Early_conformer(**kw)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=3, style="trained"))
    model = model.to("cuda:0").train()
    mel, lens = synth.synth_mel(2, 80, 259, seed=3).to("cuda:0"), torch.tensor([259, 201])
    tgt, tl = synth.synth_targets(2, 8, 256, seed=3)
    aug = augment.SpecAugment(seed=3).train()
    x = aug(mel, lens)
    assert x is not mel and x.shape == mel.shape and not torch.equal(x, mel) and torch.isfinite(x).all()
    assert np.array_equal(aug.last_params.cpu().numpy(), S.draw([259, 201], 80, 259, 3))
    assert torch.equal(x[1, :, 201:], mel[1, :, 201:])
    loss = exit_ctc_losses(model(x, lens), tgt, tl).sum()
    loss.backward()
    assert torch.isfinite(loss).item()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    assert aug.eval()(mel, lens) is mel and aug.get_state() == {"seed": 3, "calls": 1}
