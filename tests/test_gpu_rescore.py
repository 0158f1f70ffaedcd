"""GPU tests of two-pass decoding (run with -m gpu on an MI355X): the N-best end of the CTC prefix beam search
(csrc/ctc_beam.hip) against the existing entry, the oracle's final beam and a brute-force enumeration; the hypothesis scoring
kernel against its fp64 definition; eec_decoder_score against eec_decoder_forward on every hypothesis alone and against the
model's own modules on the CPU; and the decoding mode against the fp64 mix and pick of tests/rescore_cases.py."""
import sys

import pytest
import torch

import rescore_cases as X
from conftest import GOLDEN, ref_decoder_logprobs
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference
from early_exit_transformer_amd.model import ctc_beam_decode, encoder_lengths, full_conformer

pytestmark = pytest.mark.gpu
NEG = -float("inf")


# ---------------------------------------------------------------------------------------------------------------------------
# N-best
# ---------------------------------------------------------------------------------------------------------------------------
def _nbest(logp, lens, skip, beam, nbest, thr=0.95):
    got = ctc_beam_decode(logp.cuda(), beam_size=beam, blank_skip_threshold=thr, skip_drops_frame=skip, em_len=None if lens is None else lens.cuda(),
                          nbest=nbest)
    return [t.cpu() for t in got]


def _hyps(tok, cnt, s, n):
    return [tuple(tok[s, r, : int(cnt[s, r])].tolist()) for r in range(n)]


@pytest.mark.parametrize("with_len,skip", X.ALL_VARIANTS)
@pytest.mark.parametrize("beam,nbest", [(16, 4), (10, 10), (5, 1)])
def test_nbest_structure_and_the_existing_entry(with_len, skip, beam, nbest):
    """Every block of rescore_cases, with and without lengths (0 and T' among them), under both skip readings: hypothesis 0 is
    bit for bit what ctc_beam_decode returns; scores do not increase; present hypotheses are pairwise distinct; absent ones have
    count 0 and score -inf; nbest = 1 is the existing entry; n_hyp is the oracle's final beam size capped at nbest (beam 16: every
    block; beams 10 and 5: the blocks with V <= 32, where the oracle is quick)."""
    finals = X.oracle_beams(with_len, skip, beam, 256 if beam == X.ORACLE_BEAM else 32)
    checked = 0
    for (T, V, scale, logp, lens), rows in zip(X.nbest_blocks(), finals):
        lens = lens if with_len else None
        tok, cnt, score, n_hyp = _nbest(logp, lens, skip, beam, nbest)
        tok1, cnt1, score1 = [t.cpu() for t in ctc_beam_decode(logp.cuda(), beam_size=beam, skip_drops_frame=skip,
                                                               em_len=None if lens is None else lens.cuda())]
        assert tok.shape == (logp.size(0), nbest, T) and cnt.shape == score.shape == (logp.size(0), nbest)
        assert torch.equal(cnt[:, 0], cnt1) and torch.equal(score[:, 0], score1)
        for s in range(logp.size(0)):
            n = int(n_hyp[s])
            assert 1 <= n <= nbest
            if rows is not None:
                assert n == min(len(rows[s]), nbest), (T, V, scale, s, n, len(rows[s]))
                checked += 1
            assert torch.equal(tok[s, 0, : int(cnt1[s])], tok1[s, : int(cnt1[s])])
            hyps = _hyps(tok, cnt, s, n)
            assert len(set(hyps)) == n, (T, V, scale, s, hyps)
            sc = score[s, :n]
            assert torch.isfinite(sc).all() and (sc[1:] <= sc[:-1]).all(), (T, V, scale, s, sc)
            assert (cnt[s, n:] == 0).all() and (score[s, n:] == NEG).all()
            if lens is not None and int(lens[s]) == 0:
                assert n == 1 and hyps == [()] and float(score[s, 0]) == 0.0
    assert checked >= 36  # 9 of the 12 blocks at the least


@pytest.mark.parametrize("with_len,skip", X.ORACLE_VARIANTS)
def test_nbest_against_the_oracles_final_beam(with_len, skip):
    """Beam 16, nbest 4: n_hyp is the oracle's final beam size capped at 4; every present score is within 2e-3 * max(1, |score|)
    of the oracle's at that rank; the token sequences agree at every rank whose gaps the oracle has above BEAM_MARGIN -- at least
    3/4 of all (sequence, rank) pairs (tests/test_host_rescore.py asserts that of the inputs)."""
    compared = present = 0
    worst = 0.0
    for (T, V, scale, logp, lens), rows in zip(X.nbest_blocks(), X.oracle_beams(with_len, skip)):
        tok, cnt, score, n_hyp = _nbest(logp, lens if with_len else None, skip, X.ORACLE_BEAM, X.ORACLE_NBEST)
        for s, final in enumerate(rows):
            n = min(len(final), X.ORACLE_NBEST)
            assert int(n_hyp[s]) == n, (T, V, scale, s)
            hyps = _hyps(tok, cnt, s, n)
            for r in range(n):
                err = abs(float(score[s, r]) - final[r][1]) / max(1.0, abs(final[r][1]))
                worst = max(worst, err)
                assert err <= X.SCORE_RTOL, (T, V, scale, s, r, float(score[s, r]), final[r][1])
            for r in X.comparable_ranks(final):
                assert hyps[r] == tuple(final[r][0]), (T, V, scale, s, r)
                compared += 1
            present += n
    print(f"\n[nbest vs oracle len={with_len} skip_drops={skip}] {compared} of {present} token sequences compared, worst score error "
          f"{worst / X.SCORE_RTOL:.4f} of the bound")
    assert compared >= X.MIN_COMPARED * present


def test_nbest_unpruned_equals_the_enumeration_of_all_paths():
    """V = 3, T' = 3, beam 16, no skip threshold: nothing is pruned, so the list is every label sequence three frames can spell,
    each with the summed probability of all its paths."""
    logp, total = X.unpruned_case()
    tok, cnt, score, n_hyp = _nbest(logp, None, False, 16, 16, thr=1.0)
    n = int(n_hyp[0])
    got = dict(zip(_hyps(tok, cnt, 0, n), score[0, :n].tolist()))
    assert len(got) == n and set(got) == set(total)
    for p, want in total.items():
        assert abs(got[p] - want) <= X.SCORE_RTOL * max(1.0, abs(want)), (p, got[p], want)


def test_ctc_cuda_predict_returns_nbest_hypotheses():
    T, V, scale, logp, lens = X.nbest_blocks()[7]
    inf = BeamInference()
    one = inf.ctc_cuda_predict(logp.cuda(), beam_size=10)
    many = inf.ctc_cuda_predict(logp.cuda(), beam_size=10, nbest=3)
    tok, cnt, score, n_hyp = _nbest(logp, None, False, 10, 3)
    for b, (row1, row) in enumerate(zip(one, many)):
        assert len(row) == int(n_hyp[b]) and row[0].tokens == row1[0].tokens and row[0].score == row1[0].score
        assert [h.tokens for h in row] == [list(p) for p in _hyps(tok, cnt, b, len(row))]


# ---------------------------------------------------------------------------------------------------------------------------
# the scoring kernel alone
# ---------------------------------------------------------------------------------------------------------------------------
def _hyp_score(logits, tokens, lengths, eos):
    lib = capi.load()
    lg, tk, ln = logits.cuda().contiguous(), tokens.cuda().contiguous(), lengths.cuda().contiguous()
    out = torch.full((lengths.numel(),), float("nan"), device="cuda")
    capi.check(lib.eec_hypothesis_score(lg.data_ptr(), tk.data_ptr(), ln.data_ptr(), lengths.numel(), tokens.size(1), logits.size(1), eos,
                                        out.data_ptr(), capi.stream_ptr(out.device)), "eec_hypothesis_score")
    return out.cpu()


@pytest.mark.parametrize("V", X.SCORE_VOCABS)
def test_scoring_kernel_against_the_fp64_definition(V):
    """|score - fp64| <= (k + 1) * (2^-22 * M + 4e-7), M the largest |logit| of the hypothesis' rows (up to 60); lengths 0, 1 and L;
    absent hypotheses are exactly -inf; no NaN; two runs are bit-equal.  Measured on an MI355X: see the README."""
    logits, tokens, lengths = X.score_case(V)
    want, bound = X.score_reference(logits, tokens, lengths, X.SCORE_EOS)
    got = _hyp_score(logits, tokens, lengths, X.SCORE_EOS)
    assert not torch.isnan(got).any()
    absent = lengths < 0
    assert (got[absent] == NEG).all() and torch.isfinite(got[~absent]).all()
    frac = ((got.double() - want)[~absent].abs() / bound[~absent]).max().item()
    print(f"\n[hypothesis score V={V}] worst error: {frac:.3f} of the bound")
    assert frac <= 1.0
    assert torch.equal(_hyp_score(logits, tokens, lengths, X.SCORE_EOS), got)


def test_scoring_kernel_never_writes_a_nan():
    """A row without a finite logit (all -inf, all NaN): its term counts as -inf, and so does its hypothesis; the others are untouched."""
    logits, tokens, lengths = X.score_case(32)
    logits = logits.clone()
    logits[0] = NEG                 # hypothesis 0, length 0: its only row
    logits[2 * 7 + 1] = float("nan")  # inside hypothesis 2
    got = _hyp_score(logits, tokens, lengths, X.SCORE_EOS)
    assert not torch.isnan(got).any() and got[0] == NEG and got[2] == NEG
    want, bound = X.score_reference(logits, tokens, lengths, X.SCORE_EOS)
    rest = [h for h in range(len(X.SCORE_LENS)) if h not in (0, 2) and X.SCORE_LENS[h] >= 0]
    assert ((got.double() - want)[rest].abs() <= bound[rest]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# eec_decoder_score
# ---------------------------------------------------------------------------------------------------------------------------
def _aed_model(d_model, n_head, d_feed_forward, n_dec_layers, seed=5):
    sys.path.insert(0, GOLDEN)
    import aed_fixture as G
    kw = dict(n_enc_exits=2, n_enc_layers=1, d_model=d_model, n_head=n_head, d_feed_forward=d_feed_forward, depthwise_kernel_size=31, dec_voc_size=256)
    fc = full_conformer(trg_pad_idx=X.DEC_PAD, enc_voc_size=256, max_len=2000, features_length=80, drop_prob=0.1, device="cuda",
                        n_dec_layers=n_dec_layers, **kw).eval()
    fc.load_state_dict(G.aed_state_dict(fc, seed), strict=True)
    return fc


@pytest.mark.parametrize("geo", X.DEC_MODELS, ids=lambda g: f"d{g['d_model']}")
def test_decoder_score_against_every_hypothesis_alone(geo):
    """n = 3 memories, T' = 17, R = 4, L = 9, lengths {0, 1, 5, 9}, one absent, one hypothesis with pad_idx inside: every score
    against the same hypothesis run alone through eec_decoder_forward (log-probs gathered and summed in fp64) within
    2 * (k + 1) * 2e-5 * max(10, max |logp|), and against the model's own modules on the CPU in fp32 within half of that; a
    permutation of the hypotheses inside each memory permutes the scores; R = 1."""
    fc = _aed_model(**geo)
    enc, tokens, lengths = X.decoder_case(geo["d_model"])
    layer_n = 2
    with torch.no_grad():
        cpu = {}
        for i in range(X.DEC_N):
            for r in range(X.DEC_R):
                k = int(lengths[i, r])
                if k >= 0:
                    trg, targets = X.decoder_row(tokens[i, r], k)
                    lp = ref_decoder_logprobs(fc, trg, enc[i:i + 1], layer_n)[0]
                    cpu[i, r] = (X.gather_sum(lp.double(), targets), lp.abs().max().item())
        fc = fc.cuda()
        got = fc.score_hypotheses(enc.cuda(), layer_n, tokens.cuda(), lengths.cuda(), X.DEC_SOS, X.DEC_EOS).cpu()
        assert got.shape == (X.DEC_N, X.DEC_R) and not torch.isnan(got).any()
        worst_alone = worst_cpu = 0.0
        for i in range(X.DEC_N):
            for r in range(X.DEC_R):
                k = int(lengths[i, r])
                if k < 0:
                    assert got[i, r] == NEG
                    continue
                trg, targets = X.decoder_row(tokens[i, r], k)
                lp = fc._decoder_(trg.cuda(), enc[i:i + 1].cuda(), layer_n)[0].cpu()
                alone = X.gather_sum(lp.double(), targets)
                tol = (k + 1) * 2e-5 * max(10.0, lp.abs().max().item())
                worst_alone = max(worst_alone, abs(float(got[i, r]) - alone) / (2 * tol))
                assert abs(float(got[i, r]) - alone) <= 2 * tol, (i, r, k, float(got[i, r]), alone, tol)
                want, mag = cpu[i, r]
                tol = (k + 1) * 2e-5 * max(10.0, mag)
                worst_cpu = max(worst_cpu, abs(float(got[i, r]) - want) / tol)
                assert abs(float(got[i, r]) - want) <= tol, (i, r, k, float(got[i, r]), want, tol)
        print(f"\n[decoder score d{geo['d_model']}] worst error: {worst_alone:.3f} of the bound against the row alone, {worst_cpu:.3f} against the "
              "CPU modules")
        # a permutation inside every memory
        perm = torch.tensor([2, 0, 3, 1])
        moved = fc.score_hypotheses(enc.cuda(), layer_n, tokens[:, perm].cuda(), lengths[:, perm].cuda(), X.DEC_SOS, X.DEC_EOS).cpu()
        for i in range(X.DEC_N):
            for r in range(X.DEC_R):
                k = int(lengths[i, perm[r]])
                if k < 0:
                    assert moved[i, r] == NEG
                else:
                    tol = 2 * (k + 1) * 2e-5 * max(10.0, cpu[i, int(perm[r])][1])
                    assert abs(float(moved[i, r]) - float(got[i, perm[r]])) <= tol, (i, r)
        # R = 1, and the split over memories that max_workspace_bytes asks for
        first = fc.score_hypotheses(enc.cuda(), layer_n, tokens[:, :1].cuda(), lengths[:, :1].cuda(), X.DEC_SOS, X.DEC_EOS).cpu()
        one_memory = capi.load().eec_decoder_score_workspace_bytes(geo["d_model"], geo["n_head"], geo["d_feed_forward"], 256, 1, X.DEC_R, X.DEC_L,
                                                                   X.DEC_TQ)
        split = fc.score_hypotheses(enc.cuda(), layer_n, tokens.cuda(), lengths.cuda(), X.DEC_SOS, X.DEC_EOS, max_workspace_bytes=one_memory).cpu()
        with pytest.raises(ValueError, match="max_workspace_bytes"):  # one memory is the smallest part
            fc.score_hypotheses(enc.cuda(), layer_n, tokens.cuda(), lengths.cuda(), X.DEC_SOS, X.DEC_EOS, max_workspace_bytes=one_memory - 1)
        for i in range(X.DEC_N):
            k = int(lengths[i, 0])
            tol = 2 * (k + 1) * 2e-5 * max(10.0, cpu[i, 0][1])
            assert abs(float(first[i, 0]) - float(got[i, 0])) <= tol
            for r in range(X.DEC_R):
                if int(lengths[i, r]) >= 0:
                    assert abs(float(split[i, r]) - float(got[i, r])) <= 2 * (int(lengths[i, r]) + 1) * 2e-5 * max(10.0, cpu[i, r][1])
        assert torch.equal(fc.score_hypotheses(enc.cuda(), layer_n, tokens.cuda(), lengths.cuda(), X.DEC_SOS, X.DEC_EOS).cpu(), got)  # run to run


# ---------------------------------------------------------------------------------------------------------------------------
# the decoding mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from test_gpu_aed_batch import ARGS, _fixture_model, _ragged_batch
    fc, kw = _fixture_model(n_enc_exits=2, n_dec_layers=2)
    spec, vlen = _ragged_batch(3, 131, seed=11)
    tok = dict(SOS_token=ARGS["SOS_token"], EOS_token=ARGS["EOS_token"])
    return fc, spec, vlen, tok


def _direct_lists(fc, spec, vlen, tok, nbest, beam):
    """The reference of the mode, built here from the two public pieces and nothing of ``BeamInference``: per exit e one
    ``ctc_beam_decode(nbest=)`` over that exit's emissions and one ``score_hypotheses`` call on exit e's taps and decoder, on the
    list as the kernel returned it (absent hypotheses marked by a length of -1, rows cut to the longest hypothesis of the whole
    batch).  ``lists[b][e] = (tokens, ctc, att)`` of the present hypotheses, as Python lists."""
    logp, taps = fc._run_encoder(spec, vlen, want_out=True, want_taps=True, n_groups=2)[:2]
    fl = encoder_lengths(vlen.to(logp.device), logp.size(2))
    first = [ctc_beam_decode(logp[e], beam_size=beam, em_len=fl, nbest=nbest) for e in range(2)]
    L = max(1, max(int(cnt.max()) for _, cnt, _, _ in first))
    lists = [[None, None] for _ in range(spec.size(0))]
    for e, (tk, cnt, sc, n_hyp) in enumerate(first):
        rank = torch.arange(nbest, device=cnt.device).view(1, -1)
        lengths = torch.where(rank < n_hyp.view(-1, 1), cnt, torch.full_like(cnt, -1))
        att = fc.score_hypotheses(taps[e], e + 1, tk[:, :, :L].contiguous(), lengths, tok["SOS_token"], tok["EOS_token"]).cpu()
        tk, cnt, sc, n_hyp = tk.cpu(), cnt.cpu(), sc.cpu(), n_hyp.cpu()
        for b in range(spec.size(0)):
            n = int(n_hyp[b])
            assert (att[b, n:] == NEG).all() and torch.isfinite(att[b, :n]).all()
            lists[b][e] = ([list(p) for p in _hyps(tk, cnt, b, n)], sc[b, :n].tolist(), att[b, :n].tolist())
    return lists


def test_decode_batch_rescoring_is_the_fp64_pick_of_the_direct_lists(tiny):
    """B = 3 ragged utterances, 2 exits, nbest 4 of beam 8: out[b][e] is the hypothesis rescore_cases' fp64 mix and pick choose from
    the kernel's N-best list and score_hypotheses' scores, both obtained here by direct calls; w = 1 returns the CTC 1-best, w = 0
    the arg-max of the attention scores; and the lists rescore_batch returns hold those tokens, CTC scores and attention scores
    bit for bit (the same launches on the same inputs), with the joint score of the fp64 mix."""
    fc, spec, vlen, tok = tiny
    inf = BeamInference()
    lists = _direct_lists(fc, spec, vlen, tok, 4, 8)
    assert any(len(tokens) > 1 for row in lists for tokens, _, _ in row), "every list has one hypothesis: nothing to choose"
    assert any(X.pick(X.mix(ctc, att, 0.0)) != 0 for row in lists for _, ctc, att in row), "the attention scores never change the pick"
    for w in (0.5, 0.3, 1.0, 0.0):
        got = inf.decode_batch_rescoring(fc, spec, vlen, nbest=4, rescoring_ctc_weight=w, beam_size=8, **tok)
        assert len(got) == 3 and all(len(row) == 2 for row in got)
        for b in range(3):
            for e in range(2):
                tokens, ctc, att = lists[b][e]
                assert got[b][e] == tokens[X.pick(X.mix(ctc, att, w))], (w, b, e)
                if w == 1.0:
                    assert got[b][e] == tokens[0]
                if w == 0.0:
                    assert got[b][e] == tokens[max(range(len(att)), key=lambda r: (att[r], -r))]
    logp, taps = fc._run_encoder(spec, vlen, want_out=True, want_taps=True, n_groups=2)[:2]
    found = inf.rescore_batch(fc, taps, [1, 2], logp, encoder_lengths(vlen.to(logp.device), logp.size(2)), 4, 0.5, beam_size=8, **tok)
    for b in range(3):
        for e in range(2):
            tokens, ctc, att = lists[b][e]
            best, lst = found[b][e]
            assert lst.tokens == tokens and lst.ctc == ctc and lst.att == att, (b, e, lst.att, att)
            assert lst.joint == X.mix(ctc, att, 0.5) and best == tokens[X.pick(lst.joint)]


def test_decode_batch_adaptive_rescoring_equals_rescoring_at_the_chosen_exits(tiny):
    """A prescribed routing: out[b] is decode_batch_rescoring's out[b][exit], and the fp64 pick from the direct lists of that exit
    (the adaptive pass cuts its rows to the longest hypothesis of the B chosen lists, so its attention scores are not compared
    bitwise; its picks are)."""
    fc, spec, vlen, tok = tiny
    inf = BeamInference()
    routing = [1, 0, 1]
    lists = _direct_lists(fc, spec, vlen, tok, 4, 8)
    want = inf.decode_batch_rescoring(fc, spec, vlen, nbest=4, rescoring_ctc_weight=0.4, beam_size=8, **tok)
    got = inf.decode_batch_adaptive(fc, spec, vlen, exit_of=routing, beam_size=8, nbest=4, rescoring_ctc_weight=0.4, **tok)
    assert [e for _, e in got] == routing
    for b, (best, e) in enumerate(got):
        tokens, ctc, att = lists[b][e]
        assert best == want[b][e] and best == tokens[X.pick(X.mix(ctc, att, 0.4))], (b, e)
    with pytest.raises(ValueError):
        inf.decode_batch_adaptive(fc, spec, vlen, exit_of=routing, rescoring_ctc_weight=0.4, joint_ctc_weight=0.3, **tok)
    with pytest.raises(TypeError, match="pen_alpha"):  # a keyword of the step searches has no meaning here
        inf.decode_batch_adaptive(fc, spec, vlen, exit_of=routing, rescoring_ctc_weight=0.4, pen_alpha=0.6, **tok)
    with pytest.raises(ValueError):
        inf.decode_batch_rescoring(fc, spec, vlen, rescoring_ctc_weight=1.5, **tok)
