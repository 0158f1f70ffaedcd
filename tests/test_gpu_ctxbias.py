"""GPU tests of contextual biasing: the biased compile of the CTC prefix beam search (csrc/ctc_beam_ctx.hip) -- neutral without a
graph bit for bit, against the fp64 restatement (tests/ctxbias_cases.py) with a graph, unpruned on a case small enough to enumerate,
per-sequence graphs of a bank, run-to-run and split-batch bits, a captured-graph replay -- and the AED step kernel
(csrc/ctx_graph.hip) against the host path and inside the lockstep searches of the small AED fixture model."""
import numpy as np
import pytest
import torch

import ctc_cases as K
import ctxbias_cases as X
import rescore_cases as RC
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.context import ContextBiasSession, ContextGraph
from early_exit_transformer_amd.model import ctc_beam_decode, ctc_prefix_session, encoder_lengths
from test_gpu_aed_batch import ARGS, _fixture_model, _ragged_batch

pytestmark = pytest.mark.gpu

NEG = float("-inf")


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def graph_of_block(k, b):
    return ContextGraph(X.block_phrases(k), X.block_boosts(k, b), vocab_size=X.blocks()[k][1])


@pytest.mark.parametrize("beam", [16, 10, 5])
def test_without_a_bias_the_search_is_the_existing_one_bit_for_bit(beam):
    """An empty graph, graph_of = -1 under a boosted graph, and all-zero boosts; both ends, with and without lengths, both skip readings."""
    runs = 0
    for k, (T, V, scale, logp, lens, _) in enumerate(X.blocks()):
        x = logp.cuda()
        off = torch.full((x.size(0),), -1, dtype=torch.int32)
        kinds = [(ContextGraph([], vocab_size=V), None), (graph_of_block(k, 1.5), off), (graph_of_block(k, 0.0), None)]
        for with_len, skip in RC.ALL_VARIANTS:
            kw = dict(beam_size=beam, skip_drops_frame=skip, em_len=lens if with_len else None)
            for nbest in (None, 4):
                want = ctc_beam_decode(x, nbest=nbest, **kw)
                for graph, rows in kinds:
                    got = ctc_beam_decode(x, nbest=nbest, context=graph, graph_of=rows, **kw)
                    assert len(got) == len(want) + 1 and not got[-1].any() and got[-1].shape == want[2].shape
                    if nbest is None:  # the rows of `tokens` are defined up to their count
                        cut = lambda t, c: [t[i, : int(c[i])].tolist() for i in range(t.size(0))]  # noqa: E731
                        assert cut(got[0], got[1]) == cut(want[0], want[1]) and same(got[1:3], want[1:3])
                    else:
                        assert same(got[:4], want)
                    runs += 1
    print(f"{runs} biased calls equal to the unbiased ones")


@pytest.mark.parametrize("b", [1.5, 4.0])
def test_the_biased_search_against_the_restatement(b):
    """Beam 16, nbest 4: n_hyp equal; scores within SCORE_RTOL at each rank; at every comparable rank (key gaps of the restatement above
    BEAM_MARGIN) the token rows equal, and bias bit-equal to the fp32 chain and to bias_of(tokens); the best-prefix end returns rank 0.
    Measured on the MI355X: see the printed counts."""
    for with_len in (False, True):
        compared = present = moved = 0
        restated = X.restated_beams(b, with_len)
        for k, (T, V, scale, logp, lens, plain) in enumerate(X.blocks()):
            graph, tab = graph_of_block(k, b), X.block_tables(k, b)
            kw = dict(beam_size=X.BEAM, em_len=lens if with_len else None, context=graph)
            tok, cnt, score, n_hyp, bias = (t.cpu() for t in ctc_beam_decode(logp.cuda(), nbest=X.NBEST, **kw))
            tok1, cnt1, score1, bias1 = (t.cpu() for t in ctc_beam_decode(logp.cuda(), **kw))
            for s, final in enumerate(restated[k]):
                assert int(n_hyp[s]) == min(X.NBEST, len(final)), (k, s)
                ok = X.comparable_ranks(final)
                present += int(n_hyp[s])
                compared += len(ok)
                for r in range(int(n_hyp[s])):
                    want_p, want_tot, want_bias, _ = final[r]
                    assert abs(float(score[s, r]) - want_tot) <= RC.SCORE_RTOL * max(1.0, abs(want_tot)), (k, s, r, float(score[s, r]), want_tot)
                    if r in ok:
                        row = tok[s, r, : int(cnt[s, r])].tolist()
                        assert row == want_p, (k, s, r)
                        got_bias = np.float32(bias[s, r].item())
                        assert got_bias.view(np.int32) == X.bias32(tab, row).view(np.int32) and float(got_bias) == graph.bias_of(row) == want_bias
                if 0 in ok:
                    assert tok1[s, : int(cnt1[s])].tolist() == final[0][0] and torch.equal(bits(score1[s]), bits(score[s, 0]))
                    assert torch.equal(bits(bias1[s]), bits(bias[s, 0]))
                    moved += final[0][0] != plain[s][0][0] if not with_len else 0
        print(f"b = {b}, own lengths {with_len}: {compared} of {present} ranks compared, the best hypothesis moved in {moved} sequences")
        assert compared >= RC.MIN_COMPARED * present
        assert with_len or moved >= 5


def test_nothing_is_pruned_on_the_enumerable_case():
    """rescore_cases.unpruned_case (V = 3, T' = 3) with two phrases: every label sequence three frames can spell comes back, ordered by
    the enumerated log-probability plus the closed-form bias."""
    logp, total = RC.unpruned_case()
    graph = ContextGraph([(1, 2), (2,)], [1.5, 0.75], vocab_size=3)
    tok, cnt, score, n_hyp, bias = (t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=16, nbest=16, blank_skip_threshold=1.0, context=graph))
    n = int(n_hyp[0])
    rows = [tuple(tok[0, r, : int(cnt[0, r])].tolist()) for r in range(n)]
    assert n == len(total) and set(rows) == set(total)
    keys = []
    for r, row in enumerate(rows):
        assert abs(float(score[0, r]) - total[row]) < 1e-5 and float(bias[0, r]) == graph.bias_of(row)
        keys.append(total[row] + graph.bias_of(row))
    want = sorted(total, key=lambda p: -(total[p] + graph.bias_of(p)))
    gaps = [keys[i] - keys[i + 1] for i in range(n - 1)]
    assert all(g > -1e-5 for g in gaps)
    if min(abs(total[a] + graph.bias_of(a) - total[c] - graph.bias_of(c)) for a in total for c in total if a != c) > 1e-4:
        assert rows == want
    plain = [tuple(t) for t in sorted(total, key=lambda p: -total[p])]
    assert want != plain  # the bias reorders this list


def test_a_bank_serves_every_sequence_its_own_graph_and_the_bits_do_not_depend_on_the_batch():
    k = 4  # T' = 23, V = 32
    T, V, scale, logp, lens, _ = X.blocks()[k]
    graphs = [graph_of_block(k, 4.0), graph_of_block(3, 1.5), ContextGraph([], vocab_size=V)]
    bank = ContextGraph.bank(graphs)
    x = torch.cat([logp, logp]).cuda()
    em_len = torch.cat([lens, torch.full_like(lens, T)])
    rows = torch.tensor([0, 1, 2, -1, 1, 0, 3, 2], dtype=torch.int32)
    kw = dict(beam_size=10, nbest=4, context=bank)
    whole = ctc_beam_decode(x, em_len=em_len, graph_of=rows, **kw)
    assert same(whole, ctc_beam_decode(x, em_len=em_len, graph_of=rows.cuda(), **kw))  # a second run
    halves = [ctc_beam_decode(x[a:b], em_len=em_len[a:b], graph_of=rows[a:b], **kw) for a, b in ((0, 3), (3, 8))]
    assert same(whole, [torch.cat([h[i] for h in halves]) for i in range(5)])
    differ = 0
    for s in range(8):
        g = int(rows[s])
        alone = ctc_beam_decode(x[s:s + 1], em_len=em_len[s:s + 1], beam_size=10, nbest=4, context=graphs[g] if 0 <= g < 3 else graphs[2])
        assert same([t[s:s + 1] for t in whole], alone), s
        differ += bool(whole[4][s].any())
    assert differ >= 2


@pytest.mark.parametrize("V,R", [(7, 1), (32, 10), (256, 16)])
def test_the_step_kernel_equals_the_host_path_bit_for_bit(V, R):
    """Random rows with -inf entries, five steps with random parents and tokens (some outside their range), a bank with a mixed
    graph_of; the states too."""
    rng = np.random.RandomState(V)
    phrases = [tuple(int(t) for t in rng.randint(3, V, size=rng.randint(1, 5))) for _ in range(12)]
    phrases += [phrases[0][:1] + phrases[1], phrases[2] + phrases[2]]
    graphs = [ContextGraph(phrases, [1.5 if i % 2 else 0.3 for i in range(len(phrases))], vocab_size=V, eos=1, pad=2),
              ContextGraph(phrases[:3], 4.0, vocab_size=V, eos=1, pad=2)]
    bank = ContextGraph.bank(graphs)
    n = 5
    rows = torch.tensor([0, 1, -1, 1, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(V + R)
    host, dev = ContextBiasSession(bank, n, R, rows), ContextBiasSession(bank, n, R, rows)
    last, parent = torch.ones((n, 1), dtype=torch.long), None
    for s in range(5):
        R_in = last.size(1)
        local = torch.randn(n, R_in, V, generator=g) * 3
        local[torch.rand(n, R_in, V, generator=g) < 0.2] = NEG
        want = host.step(local, last, parent)
        got = dev.step(local.cuda(), last.cuda(), None if parent is None else parent.cuda())
        assert torch.equal(bits(got.cpu()), bits(want)) and torch.equal(dev.states().cpu(), host.states()), s
        assert (want != local).any() or s == 0
        parent = torch.randint(-1, R_in + 1, (n, R), generator=g)
        last = torch.randint(-1, V + 1, (n, R), generator=g)
        last[:, : R // 2] = torch.tensor(phrases[s % 3][:1])  # some rows walk into a phrase
    assert torch.equal(bits(dev.final(last.cuda(), parent.cuda()).cpu()), bits(host.final(last, parent)))


def test_a_captured_graph_replay_of_the_biased_search_equals_the_eager_run():
    k = 4
    T, V, scale, logp, lens, _ = X.blocks()[k]
    graph = graph_of_block(k, 4.0)
    x, el = logp.cuda(), lens.cuda()
    eager = ctc_beam_decode(x, beam_size=10, nbest=4, em_len=el, context=graph)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ctc_beam_decode(x, beam_size=10, nbest=4, em_len=el, context=graph)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        out = ctc_beam_decode(x, beam_size=10, nbest=4, em_len=el, context=graph)
    for t in out:
        t.zero_()
    cg.replay()
    torch.cuda.synchronize()
    assert same(out, eager) and eager[4].any()


# ---- the AED searches on the small fixture model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_model():
    return _fixture_model()


EOS, PAD, SOS = ARGS["EOS_token"], ARGS["PAD_token"], ARGS["SOS_token"]


def _phrases_from(rows, n=6):
    """Two- and three-token pieces of decoded rows (SOS, EOS and PAD left out) and one phrase that extends another."""
    out = []
    for row in rows:
        ids = [t for t in row if t not in (SOS, EOS, PAD, 0)]
        if len(ids) >= 4:
            out += [tuple(ids[1:3]), tuple(ids[-3:])]
    out = list(dict.fromkeys(out))[:n]
    return out + [out[0] + (out[-1][0],)]


def test_zero_boosts_leave_the_aed_searches_as_they_are(fixture_model):
    fc, kw = fixture_model
    spec, vlen = _ragged_batch(3, 131, seed=5)
    inf = BeamInference()
    plain = inf.decode_batch(fc, spec, vlen, beam_size=5, **ARGS)
    phrases = _phrases_from([ids for row in plain for ids in row])
    zero = ContextGraph(phrases, 0.0, vocab_size=256, eos=EOS, pad=PAD)
    assert inf.decode_batch(fc, spec, vlen, beam_size=5, context=zero, **ARGS) == plain
    joint = inf.decode_batch(fc, spec, vlen, beam_size=5, joint_ctc_weight=0.3, **ARGS)
    assert inf.decode_batch(fc, spec, vlen, beam_size=5, joint_ctc_weight=0.3, context=zero, graph_of=torch.zeros(3, dtype=torch.int32), **ARGS) == joint
    ctc_zero = ContextGraph(phrases, 0.0, vocab_size=256)
    two = dict(nbest=4, beam_size=8, SOS_token=SOS, EOS_token=EOS)
    assert inf.decode_batch_rescoring(fc, spec, vlen, context=ctc_zero, **two) == inf.decode_batch_rescoring(fc, spec, vlen, **two)


def test_the_predictors_pass_the_context_on(fixture_model):
    """ctc_cuda_predict and ctc_adaptive_predict return ctc_beam_decode(context=)'s hypotheses with ``.bias``; decode_all_exits is
    decode_batch's row; a call that only the step-by-step search could serve refuses."""
    fc, kw = fixture_model
    spec, vlen = _ragged_batch(3, 131, seed=5)
    inf = BeamInference()
    picked = [0, 3, 1]
    out = fc.forward_adaptive(spec, vlen, exit_of=picked)
    fl = encoder_lengths(vlen.to(out.logp.device), out.logp.size(1))
    tok0, cnt0, _ = (t.cpu() for t in ctc_beam_decode(out.logp, beam_size=8, em_len=fl))
    phrases = [tuple(tok0[b, : int(cnt0[b])].tolist()[1:3]) for b in range(3) if int(cnt0[b]) >= 3] or [(5, 6)]
    bank = ContextGraph.bank([ContextGraph(phrases, 4.0, vocab_size=256), ContextGraph([], vocab_size=256)])
    rows = torch.tensor([0, 1, 0], dtype=torch.int32)
    for nbest in (None, 3):
        want = [t.cpu() for t in ctc_beam_decode(out.logp, beam_size=8, em_len=fl, nbest=nbest, context=bank, graph_of=rows)]
        for hyps in (inf.ctc_cuda_predict(out.logp, beam_size=8, lengths=fl, nbest=nbest, context=bank, graph_of=rows),
                     inf.ctc_adaptive_predict(fc, spec, vlen, exit_of=picked, beam_size=8, context=bank, graph_of=rows)[0] if nbest is None else None):
            if hyps is None:
                continue
            for b, row in enumerate(hyps):
                for r, h in enumerate(row):
                    at = (b,) if nbest is None else (b, r)
                    assert h.tokens == want[0][at][: int(want[1][at])].tolist() and h.score == float(want[2][at]) and h.bias == float(want[-1][at])
                    assert h.bias == bank.bias_of(h.tokens, graph=int(rows[b]))
    assert not hasattr(inf.ctc_cuda_predict(out.logp, beam_size=8, lengths=fl)[0][0], "bias")
    graph = ContextGraph(_phrases_from([ids for row in inf.decode_batch(fc, spec[:1], vlen[:1], beam_size=5, **ARGS) for ids in row]), 4.0,
                         vocab_size=256, eos=EOS, pad=PAD)
    E, L = kw["n_enc_exits"], int(30 - 131 * 5 / 200)
    exits = list(range(1, E + 1))
    logp, taps = fc._run_encoder(spec[:1], vlen[:1], want_out=True, want_taps=True, n_groups=E)[:2]
    one = [taps[e] for e in range(E)]
    plain = inf.beam_search_exits(fc, one, exits, max_length=L, beam_size=5, context=graph, **ARGS)
    assert inf.decode_all_exits(fc, spec[0], vlen[0], beam_size=5, context=graph, **ARGS) == [best for _, _, best in plain]
    joint = inf.joint_search_exits(fc, one, exits, logp, encoder_lengths(vlen[:1].to(logp.device), logp.size(2)), 0.3, L, beam_size=5,
                                   context=graph, **ARGS)
    assert inf.decode_all_exits(fc, spec[0], vlen[0], beam_size=5, context=graph, joint_ctc_weight=0.3, **ARGS) == [best for _, _, best in joint]
    with pytest.raises(ValueError, match="lockstep"):
        inf.decode_all_exits(fc, spec[0], vlen[0], beam_size=5, context=graph, kv_cache=False, **ARGS)
    with pytest.raises(ValueError, match="graph_of"):
        inf.decode_batch(fc, spec, vlen, beam_size=5, graph_of=rows, **ARGS)


def _teacher_forced(fc, taps, exits, tokens, prefix=None):
    """The unbiased score of every row of ``tokens`` [n, R, L + 1] (SOS first): the decoder stepped along the rows themselves, the log-prob
    of each next token summed in fp64; with ``prefix`` (a CtcPrefixSession) the joint local scores instead.  Returns (sums, the
    largest finite |log-prob| met)."""
    n, R, L1 = tokens.shape
    E, B = len(exits), n // len(exits)
    sess = fc.decoder_batch_session(taps, exits, L1 - 1)
    total = torch.zeros((n, R), dtype=torch.float64, device=tokens.device)
    ident = torch.arange(R, device=tokens.device).expand(n, R).contiguous()
    big = 0.0
    for s in range(L1 - 1):
        last = tokens[:, :1, 0].contiguous() if s == 0 else tokens[:, :, s].contiguous()
        parent = None if s == 0 else torch.zeros_like(ident) if s == 1 else ident
        logp = sess.step(last.view(E, B, -1), None if parent is None else parent.view(E, B, -1)).view(n, -1, 256)
        if prefix is not None:
            logp = prefix.step(logp, last, parent)
        step = logp.expand(n, R, 256).gather(2, tokens[:, :, s + 1].unsqueeze(2)).squeeze(2)
        big = max(big, float(step[step != NEG].abs().max()))
        total += step.double()
    return total, big


def test_at_alpha_zero_every_final_score_is_the_unbiased_score_plus_the_bias_of_its_tokens(fixture_model):
    """Boost 4.0, pen_alpha = 0: the plain and the joint lockstep search against a teacher-forced, unbiased pass over their own final
    rows (margin: the 2e-5 * max(10, |log-prob|) per step of the model's step tests); the two-pass search against its own list."""
    fc, kw = fixture_model
    E, B, L, beam = kw["n_enc_exits"], 2, 10, 5
    spec, vlen = _ragged_batch(B, 131, seed=7)
    inf = BeamInference()
    logp, taps = fc._run_encoder(spec, vlen, want_out=True, want_taps=True, n_groups=E)[:2]
    exits = list(range(1, E + 1))
    em_len = encoder_lengths(vlen.to(logp.device), logp.size(2))
    args = dict(ARGS, pen_alpha=0.0, max_length=L, beam_size=beam)
    plain = inf.beam_search_batch(fc, taps, exits, **args)
    phrases = _phrases_from([t.tolist() for row in plain for ft, _, _ in row for t in ft])
    graph = ContextGraph(phrases, [4.0 if i % 2 == 0 else 2.0 for i in range(len(phrases))], vocab_size=256, eos=EOS, pad=PAD)
    rows_of = torch.tensor([0, -1], dtype=torch.int32)  # the second utterance is decoded without a bias
    for joint in (False, True):
        if joint:
            found = inf.joint_search_batch(fc, taps, exits, logp, em_len, 0.3, context=graph, graph_of=rows_of, **args)
        else:
            found = inf.beam_search_batch(fc, taps, exits, context=graph, graph_of=rows_of, **args)
        tokens = torch.stack([torch.stack(found[b][e][0]) for e in range(E) for b in range(B)])  # search e * B + b
        scores = torch.stack([torch.stack(found[b][e][1]) for e in range(E) for b in range(B)]).cpu()
        prefix = ctc_prefix_session(logp.reshape(E * B, logp.size(2), 256).float(), em_len.repeat(E), beam, 0.3, EOS, PAD) if joint else None
        own, big = _teacher_forced(fc, taps, exits, tokens, prefix)
        own, tokens = own.cpu(), tokens.cpu()
        tol = L * 2e-5 * max(10.0, big)
        biased = 0
        for i in range(E * B):
            for r in range(beam):
                if scores[i, r] == NEG:
                    continue
                want = graph.bias_of(tokens[i, r, 1:].tolist()) if i % B == 0 else 0.0
                assert abs(float(scores[i, r]) - float(own[i, r]) - want) < tol, (joint, i, r, float(scores[i, r]), float(own[i, r]), want, tol)
                biased += want > 0
        print(f"joint {joint}: {biased} of {E * B * beam} final rows carry a bias; margin {tol:.3g}")
        assert biased >= E
    # two-pass: joint = (1 - w) * att + w * ctc + bias over the biased first pass' list
    ctc_graph = ContextGraph([p for p in phrases], 4.0, vocab_size=256)
    w = 0.4
    found = inf.rescore_batch(fc, taps, exits, logp, em_len, 4, w, beam_size=8, SOS_token=SOS, EOS_token=EOS, context=ctc_graph)
    for b in range(B):
        for e in range(E):
            best, lst = found[b][e]
            for toks, c, a, j in zip(lst.tokens, lst.ctc, lst.att, lst.joint):
                assert abs(j - ((1 - w) * a + w * c + ctc_graph.bias_of(toks))) < 1e-9 * max(1.0, abs(j))
            top = max(range(len(lst.joint)), key=lambda r: (lst.joint[r], -r))
            assert best == lst.tokens[top]
