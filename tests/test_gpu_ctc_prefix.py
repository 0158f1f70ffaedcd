"""GPU tests of the CTC prefix scorer (csrc/ctc_prefix.hip) and of one-pass joint CTC / attention decoding on top of it: the
kernel against the float64 statement (tests/ctc_prefix_cases.py, pinned by brute force in tests/test_host_ctc_prefix.py) within the
derived bound ``T * (2^-22 * M + 4e-7)``, infinities in the same cells; the batched call against per-search calls bit for bit; the
EOS column against the CTC loss kernel; dead beams; argument checks; and ``decode_batch(joint_ctc_weight=w)`` on the small AED
model against the statement's search."""
import os
import sys

import numpy as np
import pytest
import torch

import align_cases as A
import ctc_cases as CC
import ctc_prefix_cases as P
from conftest import GOLDEN
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import ctc_prefix_session, encoder_lengths, full_conformer

pytestmark = pytest.mark.gpu

NINF = float("-inf")
EOS, PAD = 1, 2
LABELS = [5, 6, 7]


def small(n, T, V, seed):
    return [A.small_emission(T, V, 3.0, seed + i) for i in range(n)]


def peaky(T, V):
    return list(CC.peaky_logp(16.0, E=1, B=3, T=T, V=V)[0])


# name -> (emissions, em_len, blank, beams per step after the first, CTC weight, min_length): one case per boundary
CASES = {
    "v29-t20-r5": (lambda: small(3, 20, 29, 1), [20, 13, 7], 0, [5, 5, 5, 3], 0.3, 0),
    "v64-blank3-t63-r16": (lambda: small(3, 63, 64, 2), [63, 40, 17], 3, [16, 16, 16], 0.5, 2),
    "v256-t64-r1-peaky": (lambda: peaky(64, 256), [64, 33, 64], 0, [1, 1, 1, 1], 0.3, 0),
    "v29-t65-r5-peaky": (lambda: peaky(65, 29), [65, 64, 63], 0, [5, 4, 5], 1.0, 0),
    "t1": (lambda: small(3, 1, 29, 3), [1, 1, 1], 0, [5, 5], 0.3, 0),
    "t2": (lambda: small(3, 2, 29, 4), [2, 1, 2], 0, [5, 5, 5], 0.3, 0),
    "v64-blank3-t160": (lambda: small(3, 160, 64, 5), [160, 97, 31], 3, [1, 5, 1], 0.7, 0),
}


def device_session(xs, em_len, R_max, w, blank, min_length):
    return ctc_prefix_session(torch.stack(xs).cuda(), None if em_len is None else torch.tensor(em_len), R_max, w, EOS, PAD, blank=blank,
                              min_length=min_length)


def run_case(xs, em_len, blank, R_seq, w, min_length, script=None, seed=9):
    V = xs[0].size(1)
    script = script or P.make_script(R_seq, LABELS, EOS, PAD, seed)
    R_max = max(len(p) for p, _ in script)
    return P.scripted(lambda: device_session(xs, em_len, R_max, w, blank, min_length), xs, em_len, V, w, EOS, PAD, blank, min_length, script=script)


@pytest.mark.parametrize("name", list(CASES))
def test_scripted_steps_stay_within_the_bound_of_the_statement(name):
    make, em_len, blank, R_seq, w, min_length = CASES[name]
    res = run_case(make(), em_len, blank, R_seq, w, min_length)
    print(f"{name}: worst error / bound = {P.assert_within_bound(res):.3g}, bounds {[f'{b:.2g}' for b in res[-1][2]]}")
    assert any((want != NINF).any() for _, want, _ in res[1:])


def test_the_batched_call_equals_the_per_search_calls_bit_for_bit():
    make, em_len, blank, R_seq, w, min_length = CASES["v29-t20-r5"]
    xs = make()
    together = run_case(xs, em_len, blank, R_seq, w, min_length)
    again = run_case(xs, em_len, blank, R_seq, w, min_length)
    for i in range(3):
        # the attention scores of P.scripted are drawn for [n, R, V]: draw them alike and take row i
        sess = device_session(xs[i:i + 1], em_len[i:i + 1], 5, w, blank, min_length)
        script = P.make_script(R_seq, LABELS, EOS, PAD, 9)
        last, parent = torch.full((1, 1), 7, dtype=torch.long), None
        gi = torch.Generator().manual_seed(3)
        for s in range(len(script) + 1):
            R = last.size(1)
            att = torch.log_softmax(torch.randn(3, R, 29, generator=gi) * 2.0, -1)[i:i + 1]
            got = sess.step(att.cuda(), last.cuda(), None if parent is None else parent.cuda()).double().cpu().numpy()
            assert np.array_equal(got[0], together[s][0][i]), (i, s)
            if s < len(script):
                parent, last = torch.tensor([script[s][0]]), torch.tensor([script[s][1]])
    for (a, _, _), (b, _, _) in zip(together, again):  # and run to run
        assert np.array_equal(a, b)


def test_the_long_shape():
    xs = small(1, 1024, 29, 6)
    res = run_case(xs, None, 0, [16, 16], 0.3, 0)
    print(f"T' = 1024, R = 16: worst error / bound = {P.assert_within_bound(res):.3g}, bound {res[-1][2][0]:.3g}")


def test_the_eos_column_is_minus_the_ctc_loss_of_the_labels():
    T, V, n, labels = 40, 29, 3, [5, 5, 17, 9]
    xs = small(n, T, V, 7)
    sess = device_session(xs, None, 1, 1.0, 0, 0)
    st = P.PrefixStatement([x.double().numpy() for x in xs], None, 1.0, EOS, PAD)
    lib = capi.load()
    logp = torch.stack(xs).cuda().unsqueeze(0).contiguous()
    last = torch.full((n, 1), 7, dtype=torch.long)
    att = torch.zeros(n, 1, V)
    for s in range(len(labels) + 1):
        local = sess.step(att.cuda(), last.cuda(), None if s == 0 else torch.zeros(n, 1, dtype=torch.long).cuda())
        st.step(att.double().numpy(), last.tolist(), None if s == 0 else [[0]] * n)
        full = (local[:, 0, EOS].double() + sess.prefix_scores()[:, 0].double()).cpu()
        S = max(s, 1)
        tg = torch.tensor([labels[:s] + [0] * (S - s)] * n).cuda()
        tl = torch.full((n,), s, dtype=torch.long).cuda()
        nll, out = torch.empty(n, device="cuda"), torch.empty(1, device="cuda")
        capi.check(lib.eec_ctc_loss(logp.data_ptr(), tg.data_ptr(), tl.data_ptr(), 1, n, T, V, S, 0, nll.data_ptr(), out.data_ptr(),
                                    capi.stream_ptr(logp.device)), "eec_ctc_loss")
        nll = nll.double().cpu()
        for i in range(n):
            tol = P.bound(T, st.M[i]) + 2e-5 + 2e-5 * abs(float(nll[i]))
            assert abs(float(full[i]) + float(nll[i])) <= tol, (s, i, float(full[i]), float(nll[i]), tol)
        if s < len(labels):
            last = torch.full((n, 1), labels[s], dtype=torch.long)


def test_dead_beams_give_minus_infinity_and_never_a_nan():
    script = [([0, 0, 0], [5, 6, 5]), ([0, 1, 2], [6, 6, 5]), ([0, 1, 2], [7, 1, 5]), ([1, 0, 2], [2, 5, 5]), ([0, 1, 2], [2, 5, 5])]
    res = run_case(small(2, 8, 29, 8), [2, 2], 0, None, 0.3, 0, script=script)
    assert len(res) == 6
    P.assert_within_bound(res)
    assert (res[2][0][:, 2] == NINF).all()  # "5 5" needs three frames
    assert (res[3][0][:, 0] == NINF).all() and (res[3][0][:, 1, PAD] == 0).all()  # three labels; the beam that took EOS


def test_bad_arguments_are_refused():
    em = torch.zeros(1, 8, 16).cuda()
    with pytest.raises(RuntimeError, match="10001"):
        ctc_prefix_session(em, None, 4, 0.5, EOS, PAD, blank=16)
    with pytest.raises(RuntimeError, match="10002"):
        ctc_prefix_session(torch.zeros(1, 8, 300).cuda(), None, 4, 0.5, EOS, PAD)
    with pytest.raises(RuntimeError, match="10002"):
        ctc_prefix_session(em, None, 17, 0.5, EOS, PAD)
    att, last = torch.zeros(1, 1, 16), torch.zeros(1, 1, dtype=torch.long)
    for kw in (dict(eos=16, pad=2), dict(eos=1, pad=-1)):
        with pytest.raises(RuntimeError, match="10001"):
            ctc_prefix_session(em, None, 4, 0.5, kw["eos"], kw["pad"]).step(att.cuda(), last.cuda())
    sess = ctc_prefix_session(em, None, 4, 0.5, EOS, PAD)
    with pytest.raises(RuntimeError, match="contiguous fp32 tensor on"):
        sess.step(att, last.cuda())  # CPU tensors on the device entry
    with pytest.raises(RuntimeError, match="must be on"):
        sess.step(att.cuda(), last)
    with pytest.raises(RuntimeError, match="10001"):
        sess.step(torch.zeros(1, 5, 16).cuda(), torch.zeros(1, 5, dtype=torch.long).cuda())  # more beams than the session holds
    lib = capi.load()
    need = lib.eec_ctc_prefix_state_bytes(1, 4, 8)
    state = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    assert lib.eec_ctc_prefix_begin(em.data_ptr(), None, 1, 8, 16, 0, 4, state.data_ptr(), need - 1, None) == 10003
    none = ctc_prefix_session(torch.zeros(0, 8, 16).cuda(), None, 4, 0.5, EOS, PAD)  # no searches: a no-op
    assert none.step(torch.zeros(0, 1, 16).cuda(), torch.zeros(0, 1, dtype=torch.long).cuda()).shape == (0, 1, 16)
    torch.cuda.synchronize()


ARGS = dict(vocab_size=256, SOS_token=1, EOS_token=2, PAD_token=126, pen_alpha=0.6)


def test_decode_batch_with_a_joint_ctc_weight_is_the_statements_search():
    """The small AED model of tests/golden/aed_fixture.py, B = 3 with ragged lengths, beam 5.  T = 51 mel frames (12 / 10 / 8 CTC
    frames, 28 steps): no labelling is longer than its frames, so every search has to end its beams by EOS and the done-beam / PAD
    path runs; and the bound grows with T' * M (M is about the sum of T' blank log-probs), so that on a short utterance the
    statement's own margins clear 2 * bound on most searches -- 17 and 16 of the 18 with the decoder's torch modules on the CPU;
    at T = 131 (T' = 32, 2 * bound = 2.7e-3) only 3 and 1 of them would, whatever the kernel computes."""
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    z = np.load(os.path.join(GOLDEN, "aed_greedy.npz"))
    kw = eval(str(z["kwargs"]))
    fc = full_conformer(trg_pad_idx=126, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=int(z["n_dec_layers"]), **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, int(z["seed"])), strict=True)
    fc = fc.cuda()
    E, B, T, beam = kw["n_enc_exits"], 3, 51, 5
    g = torch.Generator().manual_seed(17)
    spec = (torch.rand(B, 80, T, generator=g) * 3).cuda()
    vlen = torch.tensor([T - 9 * b for b in range(B)])
    for b in range(B):
        spec[b, :, int(vlen[b]):] = 0
    inf = BeamInference()
    L = G.aed_max_length(T)
    sos, eos, pad = ARGS["SOS_token"], ARGS["EOS_token"], ARGS["PAD_token"]
    today = inf.decode_batch(fc, spec, vlen, beam_size=beam, **ARGS)
    assert inf.decode_batch(fc, spec, vlen, beam_size=beam, joint_ctc_weight=None, **ARGS) == today
    logp, taps = fc._run_encoder(spec, vlen, want_out=True, want_taps=True, n_groups=E)[:2]
    frames = encoder_lengths(vlen.cuda(), logp.size(2))
    exits, n = list(range(1, E + 1)), E * B
    xs = [logp[i // B, i % B].double().cpu().numpy() for i in range(n)]
    changed = 0
    for w in (0.3, 1.0):
        got = inf.decode_batch(fc, spec, vlen, beam_size=beam, joint_ctc_weight=w, **ARGS)
        found = inf.joint_search_batch(fc, taps, exits, logp, frames, w, L, beam_size=beam, **ARGS)
        second = fc.decoder_batch_session(taps, exits, L)

        def step(last, parent):
            par = None if parent is None else torch.tensor(parent).view(E, B, -1).cuda()
            return second.step(torch.tensor(last).view(E, B, -1).cuda(), par).view(n, -1, 256).double().cpu().numpy()
        want = P.joint_search(xs, frames.repeat(E).tolist(), step, n, w, sos, eos, pad, beam, ARGS["pen_alpha"], L)
        pinned = 0
        for i in range(n):
            b, e = i % B, i // B
            ft, fs, best = found[b][e]
            assert got[b][e] == best, (w, b, e)
            changed += best != today[b][e]
            for row in [t.tolist() for t in ft]:  # every row is PAD after its first EOS
                if eos in row:
                    assert all(t == pad for t in row[row.index(eos) + 1:]), row
            bd = P.bound(want[i]["T"], want[i]["M"])
            if not want[i]["margin"] > 2 * bd:
                continue
            pinned += 1
            assert best == want[i]["best"], (w, b, e, best, want[i]["best"])
            for r in range(beam):
                if want[i]["scores"][r] != NINF:
                    assert ft[r].tolist() == want[i]["tokens"][r], (w, b, e, r)
        print(f"w = {w}: {pinned} of {n} searches pinned; margins {sorted(round(x['margin'], 5) for x in want)[:4]} ...")
        assert pinned >= 0.75 * n
    print(f"best beams changed by the joint search: {changed} of {2 * n}")
    assert changed >= 1
    assert all(eos in best for row in found for _, _, best in row)  # at w = 1 every search ended its best beam
    one = inf.decode_all_exits(fc, spec[1], vlen[1], beam_size=beam, joint_ctc_weight=0.3, **ARGS)  # the single-utterance entry
    assert len(one) == E and all(len(row) == L + 1 for row in one)
