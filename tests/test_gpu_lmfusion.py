"""GPU tests of shallow fusion with a token-level n-gram model: the step kernel of the AED lockstep searches (csrc/lm_fusion.hip)
against the session's host path bit for bit; the fused compile of the CTC prefix beam search (csrc/ctc_beam_lm.hip) against the
fp64 restatement of tests/lmfusion_cases.py, neutral without a model bit for bit, run-to-run and split-batch bits; and the searches of
the small AED fixture model end to end."""
import numpy as np
import pytest
import torch

import lmfusion_cases as X
import rescore_cases as RC
from early_exit_transformer_amd.beam import BeamInference, FusedRescoredList
from early_exit_transformer_amd.lm_fusion import LMFusionSession
from early_exit_transformer_amd.model import beam_select, ctc_beam_decode, ctc_prefix_session, encoder_lengths
from test_gpu_aed_batch import ARGS, _fixture_model, _ragged_batch
from test_gpu_ctxbias import _teacher_forced

pytestmark = pytest.mark.gpu

NEG = float("-inf")
EOS, PAD, SOS = ARGS["EOS_token"], ARGS["PAD_token"], ARGS["SOS_token"]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---- the step kernel --------------------------------------------------------------------------------------------------------------
def _deep_rows(model, depth):
    """Token rows that walk the model's longest n-grams (those whose words are all ordinary pieces), so that states of every depth,
    the full order included, and states with an empty edge range occur."""
    tok = {p: v for v, p in enumerate(model.pieces)}
    rows = [[tok[w] for w in g] for g in model.grams if len(g) == depth and all(w in tok for w in g)]
    return rows[:: max(1, len(rows) // 8)][:8] or [[model.V - 1] * depth]


@pytest.mark.parametrize("V,R,order,kw", [(5, 1, 1, {}), (37, 5, 3, dict(lacking=4)), (256, 16, 5, dict(lacking=7)),
                                          (37, 16, 5, dict(bos=False, eos=False, unk=False)), (256, 5, 3, dict(pad=126))])
def test_the_step_kernel_equals_the_host_path_bit_for_bit(V, R, order, kw):
    """n = 3, R_max = 16: rows that walk the model's own n-grams to every depth, random rows, parents permuted and out of range, tokens
    out of range, -inf and -0.0 entries, skip tokens, EOS and rows past it; the states too.  Then an image whose header carries another
    V: the input comes back."""
    model = X.random_model(V + order, order, V, **kw)
    lm = X.token_lm(model)
    n, R_max, w, ts = 3, 16, 0.5, 0.25
    g = torch.Generator().manual_seed(V + R)
    deep = _deep_rows(model, order)
    host, dev = LMFusionSession(lm, n, R_max, w, ts), LMFusionSession(lm, n, R_max, w, ts)
    last, parent = torch.full((n, 1), model.sos if model.sos is not None else 0, dtype=torch.long), None
    dead = changed = 0
    for s in range(order + 4):
        R_in = last.size(1)
        local = torch.randn(n, R_in, V, generator=g) * 3
        local[torch.rand(n, R_in, V, generator=g) < 0.2] = NEG
        local[0, 0, V - 1] = -0.0
        want = host.step(local, last, parent)
        got = dev.step(local.cuda(), last.cuda(), None if parent is None else parent.cuda())
        assert torch.equal(bits(got.cpu()), bits(want)) and torch.equal(dev.states().cpu(), host.states()), s
        changed += int((want != local).sum())
        dead += int((host.states() == -1).sum())
        # search 0 walks the model's n-grams in place, search 1 permutes its parents, search 2 is random with indices out of range
        last = torch.randint(-1, V + 1, (n, R), generator=g)
        parent = torch.randint(-1, R_in + 1, (n, R), generator=g)
        if s < order:
            last[0] = torch.tensor([deep[r % len(deep)][s] for r in range(R)])
            parent[0] = torch.arange(R) if R_in == R else 0
        parent[1] = torch.randperm(R, generator=g) % R_in
        last[1] = torch.randint(0, V, (R,), generator=g)
        if model.eos is not None and s == 2:
            last[1, 0] = model.eos
        if model.pad is not None and s == 3:
            last[1, -1] = model.pad
    assert changed > 0 and (dead > 0 or model.eos is None or R == 1)
    assert order == 1 or (host.states() < lm._top).all()  # a hit at the full order leaves its suffix as the state
    other = lm.ngram._image.clone()
    other.numpy().view(np.int32)[5] = V - 1
    off = LMFusionSession(lm, n, R_max, w, ts, image=other)
    x = torch.randn(n, 2, V, generator=g).cuda()
    for s in range(2):
        assert torch.equal(bits(off.step(x, torch.ones(n, 2, dtype=torch.long).cuda())), bits(x)) and not off.states().any()


def test_the_step_does_not_depend_on_the_batch_and_zero_weights_return_the_input():
    model = X.random_model(40, 3, 37, lacking=4)
    lm = X.token_lm(model)
    g = torch.Generator().manual_seed(3)
    local = [torch.randn(4, R, 37, generator=g).cuda() for R in (1, 5)]
    last = [torch.randint(0, 37, (4, R), generator=g).cuda() for R in (1, 5)]
    parent = torch.zeros(4, 5, dtype=torch.long).cuda()

    def run(rows, w=0.5, ts=0.25):
        ses = LMFusionSession(lm, len(range(*rows.indices(4))), 16, w, ts)
        return [ses.step(local[0][rows], last[0][rows]), ses.step(local[1][rows], last[1][rows], parent[rows])]
    whole = run(slice(0, 4))
    assert same(whole, run(slice(0, 4)))
    parts = [run(slice(0, 1)), run(slice(1, 4))]
    assert same(whole, [torch.cat([p[k] for p in parts]) for k in range(2)])
    assert same(run(slice(0, 4), 0.0, 0.0), local)


# ---- the CTC prefix beam search ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctc_lm():
    return X.token_lm(X.ctc_model())


@pytest.mark.parametrize("beam", [16, 5])
def test_without_a_model_the_search_is_the_existing_one_bit_for_bit(ctc_lm, beam):
    """Zero weight with zero bonus, and an image the kernel does not trust; both ends, with and without lengths, both skip readings."""
    foreign = X.token_lm(X.ctc_model())
    foreign.ngram._image.numpy().view(np.int32)[0] = 0x54434545
    runs = 0
    for T, scale, logp, lens in X.ctc_blocks():
        x = logp.cuda()
        for with_len, skip in RC.ALL_VARIANTS:
            kw = dict(beam_size=beam, skip_drops_frame=skip, em_len=lens if with_len else None)
            for nbest in (None, 4):
                want = ctc_beam_decode(x, nbest=nbest, **kw)
                for lm, w, ts in ((ctc_lm, 0.0, 0.0), (foreign, 0.5, 0.25)):
                    got = ctc_beam_decode(x, nbest=nbest, lm=lm, lm_weight=w, token_score=ts, **kw)
                    assert len(got) == len(want) + 1 and not got[-1].any() and got[-1].shape == want[2].shape
                    if nbest is None:  # the rows of `tokens` are defined up to their count
                        cut = lambda t, c: [t[i, : int(c[i])].tolist() for i in range(t.size(0))]  # noqa: E731
                        assert cut(got[0], got[1]) == cut(want[0], want[1]) and same(got[1:3], want[1:3])
                    else:
                        assert same(got[:4], want)
                    runs += 1
    print(f"{runs} fused calls equal to the unfused ones")


@pytest.mark.parametrize("with_len,skip", RC.ALL_VARIANTS)
def test_the_fused_search_against_the_restatement(ctc_lm, with_len, skip):
    """36 sequences, T' in {1, 2, 40}, V = 37, beam 16, nbest 4, weight 0.5, bonus 0.25: n_hyp equal; scores within SCORE_RTOL at each
    rank; at every comparable rank (key gaps of the restatement above BEAM_MARGIN) the token rows equal, and fusion bit-equal to the
    fp32 chain of the row and to score_of; the best-prefix end returns rank 0; the best hypothesis moves in some sequences."""
    model, w, ts = X.ctc_model(), X.CTC_W, X.CTC_TS
    restated, plain = X.restated_beams(w, ts, with_len, skip), X.restated_beams(0.0, 0.0, with_len, skip)
    compared = present = moved = 0
    for k, (T, scale, logp, lens) in enumerate(X.ctc_blocks()):
        kw = dict(beam_size=X.BEAM, em_len=lens if with_len else None, skip_drops_frame=skip, lm=ctc_lm, lm_weight=w, token_score=ts)
        tok, cnt, score, n_hyp, fusion = (t.cpu() for t in ctc_beam_decode(logp.cuda(), nbest=X.NBEST, **kw))
        tok1, cnt1, score1, fusion1 = (t.cpu() for t in ctc_beam_decode(logp.cuda(), **kw))
        for s, final in enumerate(restated[k]):
            assert int(n_hyp[s]) == min(X.NBEST, len(final)), (k, s)
            ok = X.comparable_ranks(final)
            present += int(n_hyp[s])
            compared += len(ok)
            for r in range(int(n_hyp[s])):
                want_p, want_tot, want_fusion, _ = final[r]
                assert abs(float(score[s, r]) - want_tot) <= RC.SCORE_RTOL * max(1.0, abs(want_tot)), (k, s, r, float(score[s, r]), want_tot)
                row = tok[s, r, : int(cnt[s, r])].tolist()
                got = np.float32(fusion[s, r].item())
                assert got.view(np.int32) == np.float32(X.chain(model, row, w, ts, ctc=True)).view(np.int32), (k, s, r)
                assert float(got) == ctc_lm.score_of(row, w, ts, ctc=True)
                if r in ok:
                    assert row == want_p and float(got) == want_fusion, (k, s, r)
            assert not fusion[s, int(n_hyp[s]):].any()
            if 0 in ok:
                assert tok1[s, : int(cnt1[s])].tolist() == final[0][0] and torch.equal(bits(score1[s]), bits(score[s, 0]))
                assert torch.equal(bits(fusion1[s]), bits(fusion[s, 0]))
                moved += final[0][0] != plain[k][s][0][0]
    print(f"own lengths {with_len}, skip drops {skip}: {compared} of {present} ranks compared, the best hypothesis moved in {moved} sequences")
    assert compared >= RC.MIN_COMPARED * present
    assert moved >= 4


def test_two_runs_and_a_split_batch_return_the_same_bits(ctc_lm):
    T, scale, logp, lens = X.ctc_blocks()[-1]  # T' = 40
    x = torch.cat([logp, logp.flip(0)]).cuda()
    em_len = torch.cat([lens, torch.full_like(lens, T)])
    kw = dict(beam_size=10, nbest=4, lm=ctc_lm, lm_weight=0.5, token_score=0.25)
    whole = ctc_beam_decode(x, em_len=em_len, **kw)
    assert same(whole, ctc_beam_decode(x, em_len=em_len.cuda(), **kw)) and whole[4].any()
    halves = [ctc_beam_decode(x[a:b], em_len=em_len[a:b], **kw) for a, b in ((0, 3), (3, 8))]
    assert same(whole, [torch.cat([h[i] for h in halves]) for i in range(5)])


# ---- the AED searches on the small fixture model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_model():
    return _fixture_model()


@pytest.fixture(scope="module")
def aed_lm():
    """Order 3 over the fixture's 256 tokens (blank 0, SOS 1, EOS 2, PAD 126), with <s>, </s>, <unk> and pieces it lacks."""
    model = X.random_model(256, 3, 256, lacking=9, pad=PAD)
    return model, X.token_lm(model)


def test_zero_weights_leave_the_aed_searches_as_they_are(fixture_model, aed_lm):
    fc, kw = fixture_model
    _, lm = aed_lm
    spec, vlen = _ragged_batch(3, 131, seed=5)
    inf = BeamInference()
    zero = dict(token_lm=lm, token_lm_weight=0.0, token_score=0.0)
    E, L = kw["n_enc_exits"], int(30 - 131 * 5 / 200)
    logp, taps = fc._run_encoder(spec, vlen, want_out=True, want_taps=True, n_groups=E)[:2]
    exits = list(range(1, E + 1))
    args = dict(ARGS, max_length=L, beam_size=5)
    plain, fused = inf.beam_search_batch(fc, taps, exits, **args), inf.beam_search_batch(fc, taps, exits, **args, **zero)
    for b in range(3):  # tokens and scores exactly
        for e in range(E):
            assert same(plain[b][e][0], fused[b][e][0]) and same(plain[b][e][1], fused[b][e][1]) and plain[b][e][2] == fused[b][e][2]
    assert inf.decode_batch(fc, spec, vlen, beam_size=5, **zero, **ARGS) == inf.decode_batch(fc, spec, vlen, beam_size=5, **ARGS)
    joint = inf.decode_batch(fc, spec, vlen, beam_size=5, joint_ctc_weight=0.3, **ARGS)
    assert inf.decode_batch(fc, spec, vlen, beam_size=5, joint_ctc_weight=0.3, **zero, **ARGS) == joint
    two = dict(nbest=4, beam_size=8, SOS_token=SOS, EOS_token=EOS)
    assert inf.decode_batch_rescoring(fc, spec, vlen, **zero, **two) == inf.decode_batch_rescoring(fc, spec, vlen, **two)
    with pytest.raises(ValueError, match="lockstep"):
        inf.decode_all_exits(fc, spec[0], vlen[0], beam_size=5, token_lm=lm, kv_cache=False, **ARGS)


def test_at_alpha_zero_every_final_score_is_the_unfused_score_plus_the_fusion_score_of_its_tokens(fixture_model, aed_lm):
    """Weight 0.5, bonus 0.25, pen_alpha = 0: the plain and the joint lockstep search against a teacher-forced, unfused pass over their
    own final rows (margin: the 2e-5 * max(10, |log-prob|) per step of the model's step tests); the two-pass search against its own
    list; the predictors carry ``.fusion``."""
    fc, kw = fixture_model
    model, lm = aed_lm
    E, B, L, beam, w, ts = kw["n_enc_exits"], 2, 10, 5, 0.5, 0.25
    spec, vlen = _ragged_batch(B, 131, seed=7)
    inf = BeamInference(token_lm=lm, token_lm_weight=w, token_score=ts)
    logp, taps = fc._run_encoder(spec, vlen, want_out=True, want_taps=True, n_groups=E)[:2]
    exits = list(range(1, E + 1))
    em_len = encoder_lengths(vlen.to(logp.device), logp.size(2))
    args = dict(ARGS, pen_alpha=0.0, max_length=L, beam_size=beam)
    for joint in (False, True):
        found = inf.joint_search_batch(fc, taps, exits, logp, em_len, 0.3, **args) if joint else inf.beam_search_batch(fc, taps, exits, **args)
        tokens = torch.stack([torch.stack(found[b][e][0]) for e in range(E) for b in range(B)])  # search e * B + b
        scores = torch.stack([torch.stack(found[b][e][1]) for e in range(E) for b in range(B)]).cpu()
        prefix = ctc_prefix_session(logp.reshape(E * B, logp.size(2), 256).float(), em_len.repeat(E), beam, 0.3, EOS, PAD) if joint else None
        own, big = _teacher_forced(fc, taps, exits, tokens, prefix)
        own, tokens = own.cpu(), tokens.cpu()
        tol = L * 2e-5 * max(10.0, big)
        fused = 0
        for i in range(E * B):
            for r in range(beam):
                if scores[i, r] == NEG:
                    continue
                row = tokens[i, r].tolist()
                want = lm.score_of(row, w, ts)
                assert want == float(X.chain(model, row, w, ts))
                assert abs(float(scores[i, r]) - float(own[i, r]) - want) < tol, (joint, i, r, float(scores[i, r]), float(own[i, r]), want, tol)
                fused += want != 0
        print(f"joint {joint}: {fused} of {E * B * beam} final rows carry a fusion score; margin {tol:.3g}")
        assert fused >= E * B
    # two-pass: joint = (1 - w_ctc) * att + w_ctc * ctc + fusion over the fused first pass' list, the winner its maximum
    wc = 0.4
    found = inf.rescore_batch(fc, taps, exits, logp, em_len, 4, wc, beam_size=8, SOS_token=SOS, EOS_token=EOS)
    for b in range(B):
        for e in range(E):
            best, lst = found[b][e]
            assert isinstance(lst, FusedRescoredList) and len(lst.fusion) == len(lst.tokens)
            for toks, c, a, j, f in zip(lst.tokens, lst.ctc, lst.att, lst.joint, lst.fusion):
                assert f == lm.score_of(toks, w, ts, ctc=True)
                assert abs(j - ((1 - wc) * a + wc * c + f)) < 1e-9 * max(1.0, abs(j))
            top = max(range(len(lst.joint)), key=lambda r: (lst.joint[r], -r))
            assert best == lst.tokens[top]
    # the predictors
    em = logp[-1]
    want = [t.cpu() for t in ctc_beam_decode(em, beam_size=8, em_len=em_len, nbest=3, lm=lm, lm_weight=w, token_score=ts)]
    hyps = inf.ctc_cuda_predict(em, beam_size=8, lengths=em_len, nbest=3)
    for b, row in enumerate(hyps):
        assert len(row) == int(want[3][b])
        for r, h in enumerate(row):
            assert h.tokens == want[0][b, r, : int(want[1][b, r])].tolist() and h.score == float(want[2][b, r]) and h.fusion == float(want[4][b, r])
            assert not hasattr(h, "bias")
    assert not hasattr(BeamInference().ctc_cuda_predict(em, beam_size=8, lengths=em_len)[0][0], "fusion")
    picked = [0, 3]
    hyps, exit_of = inf.ctc_adaptive_predict(fc, spec, vlen, exit_of=picked, beam_size=8)
    assert exit_of.tolist() == picked and all(h.fusion == lm.score_of(h.tokens, w, ts, ctc=True) for row in hyps for h in row)
    taps1 = fc._run_encoder(spec[:1], vlen[:1], want_out=True, want_taps=True, n_groups=E)[1]
    one = inf.beam_search_exits(fc, [taps1[e] for e in range(E)], exits, max_length=L, beam_size=beam, **ARGS)
    assert inf.decode_all_exits(fc, spec[0], vlen[0], max_length=L, beam_size=beam, **ARGS) == [best for _, _, best in one]


def test_a_context_graph_and_a_model_compose_in_the_lockstep_searches(fixture_model, aed_lm):
    from early_exit_transformer_amd.context import ContextGraph
    fc, kw = fixture_model
    _, lm = aed_lm
    spec, vlen = _ragged_batch(2, 131, seed=7)
    inf = BeamInference()
    graph = ContextGraph([(5, 6), (7,)], 0.0, vocab_size=256, eos=EOS, pad=PAD)  # zero boosts: the bias launch runs and adds nothing
    kw_lm = dict(token_lm=lm, token_lm_weight=0.5, token_score=0.25)
    assert inf.decode_batch(fc, spec, vlen, beam_size=5, context=graph, **kw_lm, **ARGS) == inf.decode_batch(fc, spec, vlen, beam_size=5, **kw_lm, **ARGS)
    with pytest.raises(ValueError, match="not served"):
        inf.ctc_cuda_predict(torch.zeros(1, 4, 256).cuda(), beam_size=5, context=ContextGraph([], vocab_size=256), token_lm=lm)


def test_the_lockstep_loop_replays_from_one_captured_graph_to_the_eager_runs_bits(aed_lm):
    """Six steps of decoder stand-in (a fixed table of log-probs read by the last token), eec_lm_fusion_step and eec_beam_select for 4
    searches of 5 beams, captured once: nothing in the session reads the device back."""
    _, lm = aed_lm
    n, beam, L, V = 4, 5, 6, 256
    g = torch.Generator().manual_seed(12)
    table = torch.log_softmax(torch.randn(V, V, generator=g) * 2, -1).cuda()

    def loop(w=0.5, ts=0.25):
        ses = LMFusionSession(lm, n, beam, w, ts)
        scores = torch.zeros((n, 1), dtype=torch.float32, device="cuda")
        bufs = [torch.zeros((n, beam, L + 1), dtype=torch.long, device="cuda") for _ in range(2)]
        bufs[0][:, 0, 0] = SOS
        last, parent = bufs[0][:, :1, 0].contiguous(), None
        for i in range(L):
            logp = ses.step(table[last].contiguous(), last, parent)
            scores, parent, last = beam_select(logp, scores, 1.0, beam, bufs[i & 1], bufs[(i + 1) & 1], i + 1)
        return scores, bufs[L & 1], ses.states()
    eager = [t.clone() for t in loop()]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        loop()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        out = loop()
    for t in out:
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    assert same(out, eager)
    assert not torch.equal(eager[0], loop(0.0, 0.0)[0])  # the model took part
