"""Host tests of shallow fusion with a token-level n-gram model (early_exit_transformer_amd/lm_fusion.py; include/eec.h, "Shallow
fusion"): the ARPA reader against the pieces, the closed form against the dictionary restatement of tests/lmfusion_cases.py (the fp32
chain bit for bit, the fp64 scorer within a stated bound), a normalised model's rows, the session's host path against the restated
step, the neutral settings, the image checks, the refusals, the exports, and the census of the GPU test's inputs."""
import ctypes

import numpy as np
import pytest
import torch

import lmfusion_cases as X
import rescore_cases as RC
from early_exit_transformer_amd import capi
from early_exit_transformer_amd.beam import BeamInference, CTCHypothesis, FusedRescoredList, RescoredList
from early_exit_transformer_amd.lexicon import NGramLM
from early_exit_transformer_amd.lm_fusion import DEFAULT_LM_WEIGHT, LMFusionSession, TokenLM, check_lm, image_trusted

NEG = float("-inf")

# (seed, order, V, builder keywords): orders 1, 3, 5; with and without <s>, </s>, <unk>; pieces the model lacks
MODELS = [(1, 1, 5, {}), (2, 3, 37, dict(lacking=4)), (3, 5, 256, dict(lacking=7)), (4, 3, 37, dict(bos=False, eos=False, unk=False)),
          (5, 5, 37, dict(bos=False)), (6, 3, 9, dict(eos=False, lacking=1))]


def bits(x):
    return np.float32(x).view(np.int32)


def rows_of(model, rng, n=40, L=9):
    """Token rows with skip tokens, an EOS in the middle of some, and a leading SOS."""
    out = []
    for k in range(n):
        row = [int(t) for t in rng.randint(0, model.V, size=rng.randint(0, L + 1))]
        if k % 3 == 0 and model.eos is not None and len(row) > 2:
            row[len(row) // 2] = model.eos
        out.append(([model.sos] if model.sos is not None and k % 2 else []) + row)
    return out


def test_the_new_entries_are_exported():
    lib = capi.load()
    for name in ("eec_ctc_beam_decode_lm", "eec_ctc_beam_decode_nbest_lm", "eec_lm_fusion_state_bytes", "eec_lm_fusion_step"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.eec_abi_version() == 16
    assert lib.eec_lm_fusion_state_bytes(3, 16) == 2 * 3 * 16 * 4 and lib.eec_lm_fusion_state_bytes(0, 16) == 0
    assert not hasattr(lib, "eec_lm_fusion_last_error")


def test_an_arpa_file_over_the_pieces_is_read_back(tmp_path):
    model = X.random_model(11, 3, 12, lacking=2)
    path = tmp_path / "pieces.arpa"
    path.write_text(model.arpa(), encoding="utf-8")
    lm = TokenLM.from_arpa(str(path), model.pieces, blank=0, sos=1, eos=2, pad=3)
    ref = X.token_lm(model)
    assert (lm.order, lm.n_nodes, lm.vocab) == (3, ref.n_nodes, ref.vocab) and lm.V == 12
    assert lm.word_map[4:].tolist() == ref.word_map[4:].tolist() and lm.word_map[-1] == lm.unk >= 0
    assert lm.word_map[2] == lm.eos_word >= 0 and lm.word_map[1] == lm.bos >= 0  # the CTC search scores the EOS label as </s>
    rng = np.random.RandomState(0)
    for row in rows_of(model, rng):
        for ctc in (False, True):
            labels = [t for t in row if t > 3] if ctc else row
            assert bits(lm.score_of(labels, 0.7, -0.1, ctc=ctc)) == bits(X.chain(model, labels, 0.7, -0.1, ctc=ctc))
    # without <unk>: the pieces the model lacks are counted, the special tokens are not
    bare = X.random_model(12, 2, 9, unk=False)
    path.write_text(bare.arpa(), encoding="utf-8")
    ok = TokenLM.from_arpa(str(path), bare.pieces, blank=0, sos=1, eos=2, pad=3)
    assert ok.unk == -1 and ok.word_map[0] == 0 and ok.word_map[3] == 0
    with pytest.raises(ValueError, match=r"NGramLM: .*no <unk> and lacks 4 of the lexicon's words"):
        TokenLM.from_arpa(str(path), bare.pieces, blank=None)
    with pytest.raises(ValueError, match="lacks 1 of"):
        TokenLM.from_arpa(str(path), bare.pieces[:-1] + ["q"], blank=0, sos=1, eos=2, pad=3)
    with pytest.raises(ValueError, match=r"pieces.arpa:2: "):
        path.write_text("\\data\\\nngram 1=x\n", encoding="utf-8")
        TokenLM.from_arpa(str(path), bare.pieces)


def test_the_word_level_reader_is_unchanged_for_its_callers(tmp_path):
    """``exempt`` defaults to nothing: a lexicon word the model lacks is still counted and still maps to <unk>."""
    class Words:
        words = ["a", "b", "zz"]
    path = tmp_path / "w.arpa"
    path.write_text("\\data\\\nngram 1=3\n\n\\1-grams:\n-1.0\ta\n-2.0\tb\n-3.0\t<unk>\n\n\\end\\\n", encoding="utf-8")
    lm = NGramLM.from_arpa(str(path), Words)
    assert lm.word_map.tolist() == [0, 1, 2] and lm.unk == 2
    path.write_text("\\data\\\nngram 1=2\n\n\\1-grams:\n-1.0\ta\n-2.0\tb\n\n\\end\\\n", encoding="utf-8")
    with pytest.raises(ValueError, match="the model has no <unk> and lacks 1 of the lexicon's words: 'zz'"):
        NGramLM.from_arpa(str(path), Words)


@pytest.mark.parametrize("seed,order,V,kw", MODELS)
def test_score_of_is_the_fp32_chain_and_stays_near_the_fp64_scorer(seed, order, V, kw):
    """Bit for bit against the dictionary's fp32 chain.  Against the fp64 dictionary scorer: with k numbers entering the sum (every
    w * logp, w * backoff and bonus), each of the at most 2 k fp32 operations -- k additions, and the products -- commits at most
    2^-24 of a partial result that the sum of their magnitudes bounds: (k + 1) * 2^-23 * sum |terms|, the + 1 for the second order."""
    model = X.random_model(seed, order, V, **kw)
    lm = X.token_lm(model)
    rng = np.random.RandomState(seed)
    worst = 0.0
    for w, ts in ((0.5, 0.25), (DEFAULT_LM_WEIGHT, 0.0), (1.7, -0.3)):
        for row in rows_of(model, rng):
            for ctc in (False, True):
                labels = [t for t in row if t not in (model.sos, model.eos, model.pad) and (model.word(t) != X.UNK or model.has(X.UNK))] if ctc else row
                got = lm.score_of(labels, w, ts, ctc=ctc)
                assert bits(got) == bits(X.chain(model, labels, w, ts, ctc=ctc)), (labels, ctc)
                terms = []
                want = float(X.chain(model, labels, w, ts, dtype=np.float64, ctc=ctc, terms=terms))
                bound = (len(terms) + 1) * 2.0 ** -23 * sum(terms)
                assert abs(got - want) <= bound, (labels, got, want, bound)
                worst = max(worst, abs(got - want) / bound if bound else 0.0)
    print(f"order {order}, V {V}: the largest |fp32 - fp64| is {worst:.3f} of its bound")
    assert lm.score_of([], 0.5, 0.25) == 0.0


def test_the_scatter_form_of_a_row_has_the_walks_bits():
    for seed, order, V, kw in MODELS:
        model = X.random_model(seed, order, V, **kw)
        lm = X.token_lm(model)
        states = list(range(lm.n_nodes)) if lm.n_nodes < 400 else list(np.random.RandomState(seed).randint(0, lm.n_nodes, size=60))
        for s in states:
            row = lm.acc_row(s)
            for u in range(0, lm._W, 1 if lm._W < 50 else 7):
                assert bits(row[u]) == bits(lm.walk(s, u)[0]), (seed, s, u)


def test_a_normalised_model_sums_to_one_from_every_state():
    model = X.normalised_model()
    lm = X.token_lm(model)
    assert lm.order == 3 and lm.n_nodes > 40
    worst = 0.0
    for s in range(lm._top):  # every node that can be a state
        total = float((10.0 ** lm.acc_row(s).astype(np.float64)).sum())
        worst = max(worst, abs(total - 1.0))
        assert abs(total - 1.0) < 1e-5, (s, total)
    print(f"{lm._top} states, the largest |sum - 1| is {worst:.2e}")
    for g in model.grams:  # the dictionary scorer agrees
        if len(g) < 3:
            assert abs(sum(10.0 ** float(X.backoff_score(model, g, w)[0]) for w in lm.vocab) - 1.0) < 1e-5


def _drive(model, n, R, w, ts, seed, steps=6):
    """A session's host path and the restated step over the same random steps: every depth of state, parents permuted and out of
    range, tokens out of range, -inf entries, skip tokens, EOS and rows past it."""
    lm = X.token_lm(model)
    ses = LMFusionSession(lm, n, R, w, ts)
    g = torch.Generator().manual_seed(seed)
    V = model.V
    last, parent, state, R_prev = torch.zeros((n, 1), dtype=torch.long), None, None, 0
    changed = 0
    for s in range(steps):
        R_in = last.size(1)
        local = torch.randn(n, R_in, V, generator=g) * 3
        local[torch.rand(n, R_in, V, generator=g) < 0.2] = NEG
        local[0, 0, V - 1] = -0.0
        got = ses.step(local, last, parent)
        want, state = X.aed_step(model, state, None if parent is None else parent.tolist(), last.tolist(), local.numpy(), s, R_prev, w, ts)
        assert torch.equal(got.view(torch.int32), torch.from_numpy(want).view(torch.int32)), s
        dead = [[st == X.DEAD for st in row] for row in state]
        assert (ses.states() == -1).tolist() == dead
        changed += int((got != local).sum())
        R_prev = R_in
        parent = torch.randint(-1, R_in + 1, (n, R), generator=g)
        last = torch.randint(-1, V + 1, (n, R), generator=g)
        if model.eos is not None and R > 1:
            last[:, 1] = model.eos if s == 2 else last[:, 1]
            last[:, 0] = model.pad if s == 3 else last[:, 0]
    return changed


@pytest.mark.parametrize("seed,order,V,kw", [m for m in MODELS if m[2] < 256])
def test_the_sessions_host_path_is_the_restated_step(seed, order, V, kw):
    model = X.random_model(seed, order, V, **kw)
    assert _drive(model, 3, 5, 0.5, 0.25, seed) > 0
    assert _drive(model, 2, 1, DEFAULT_LM_WEIGHT, 0.0, seed + 1) > 0


def test_zero_weight_and_zero_bonus_return_the_inputs_bits():
    model = X.random_model(2, 3, 37, lacking=4)
    assert _drive(model, 3, 5, 0.0, 0.0, 9) == 0
    lm = X.token_lm(model)
    assert lm.score_of([1, 5, 6, 2, 7], 0.0, 0.0) == 0.0 and lm.score_of([5, 6, 7], 0.0, 0.0, ctc=True) == 0.0


def test_a_foreign_image_returns_the_input():
    model = X.random_model(2, 3, 37, lacking=4)
    lm = X.token_lm(model)
    good = lm.ngram._image.clone()
    words = good.numpy().view(np.int32)
    assert image_trusted(words, 37) and not image_trusted(words, 36) and not image_trusted(words[:-1], 37)

    def damaged(at, value):
        img = good.clone()
        img.numpy().view(np.int32)[at] = value
        return img
    local = torch.randn(2, 3, 37)
    last = torch.full((2, 3), 5, dtype=torch.long)
    for img in (damaged(0, 0x54434545), damaged(5, 36), damaged(11, words.size), damaged(14, -4), damaged(2, words[2] + 1), good[:-4]):
        assert not image_trusted(img.numpy().view(np.int32), 37)
        ses = LMFusionSession(lm, 2, 3, 0.5, 0.25, image=img)
        for s in range(2):
            out = ses.step(local, last)
            assert torch.equal(out.view(torch.int32), local.view(torch.int32)) and not ses.states().any()
    ses = LMFusionSession(lm, 2, 3, 0.5, 0.25, image=good)
    assert (ses.step(local, last) != local).any()


def test_the_refusals():
    model = X.random_model(2, 3, 37, lacking=4)
    lm = X.token_lm(model)
    words, logp, backoff, vocab, word_map, bos, eos_word, unk = model.arrays()
    with pytest.raises(ValueError, match="1 to 256 tokens"):
        TokenLM(words, logp, backoff, 257)
    with pytest.raises(ValueError, match="1 to 256 tokens"):
        TokenLM.from_arpa("unread.arpa", ["p"] * 300)
    with pytest.raises(ValueError, match="orders 1 to 5"):
        TokenLM([words[0]] * 6, [logp[0]] * 6, [backoff[0]] * 6, 37, word_map)
    with pytest.raises(ValueError, match="at most 512 LM words"):
        TokenLM([np.arange(600).reshape(-1, 1)], [np.zeros(600)], [np.zeros(600)], 37, np.zeros(37))
    with pytest.raises(ValueError, match="word_map must hold 37"):
        TokenLM(words, logp, backoff, 37, word_map[:-1])
    with pytest.raises(ValueError, match="eos = 40 is no token"):
        TokenLM(words, logp, backoff, 37, word_map, eos=40)
    with pytest.raises(ValueError, match="1 .. 16 beams"):
        LMFusionSession(lm, 2, 17)
    with pytest.raises(ValueError, match="must be finite"):
        LMFusionSession(lm, 2, 4, float("nan"))
    with pytest.raises(ValueError, match="over 37 tokens, the search over 256"):
        check_lm("search", lm, 256, 10, 0.3, 0.0)
    with pytest.raises(TypeError, match="lm_fusion.TokenLM"):
        check_lm("search", lm.ngram, 37, 10, 0.3, 0.0)
    with pytest.raises(ValueError, match="a token outside"):
        lm.score_of([1, 37])
    ses = LMFusionSession(lm, 2, 4)
    assert ses.lm_weight == DEFAULT_LM_WEIGHT == 0.3 and ses.token_score == 0.0
    with pytest.raises(ValueError, match=r"local must be \[2, live beams, 37\]"):
        ses.step(torch.zeros(2, 4, 36), torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="live beams per search"):
        ses.step(torch.zeros(2, 5, 37), torch.zeros(2, 5, dtype=torch.long))
    from early_exit_transformer_amd.context import ContextGraph
    from early_exit_transformer_amd.model import ctc_beam_decode
    with pytest.raises(ValueError, match="a context graph and a language model in one CTC call are not served"):
        ctc_beam_decode(torch.zeros(1, 2, 37), lm=lm, context=ContextGraph([], vocab_size=37))
    with pytest.raises(ValueError, match="which was not given"):
        ctc_beam_decode(torch.zeros(1, 2, 37), lm_weight=0.5)
    # the C entries refuse before any device work, through the one error string
    lib = capi.load()
    rc = lib.eec_lm_fusion_step(None, 0, 1, 1, 1, 17, 37, 0, None, None, None, None, None, 0, 0.5, 0.0, -1, -1, -1, -1, None)
    assert rc != 0 and b"R_max <= 16" in lib.eec_last_error()
    rc = lib.eec_lm_fusion_step(None, 0, 1, 1, 1, 4, 300, 0, None, None, None, None, None, 0, 0.5, 0.0, -1, -1, -1, -1, None)
    assert rc != 0 and b"V <= 256" in lib.eec_last_error()
    rc = lib.eec_lm_fusion_step(None, 0, 1, 1, 1, 4, 37, 0, None, None, None, None, None, 0, float("inf"), 0.0, -1, -1, -1, -1, None)
    assert rc != 0 and b"finite" in lib.eec_last_error()
    rc = lib.eec_ctc_beam_decode_lm(None, None, 1, 2, 37, 0, 17, 0.95, 0, None, None, None, None, None, 0, 0.5, 0.0, None, None)
    assert rc != 0 and b"eec_ctc_beam_decode_lm" in lib.eec_last_error()
    assert lib.eec_lm_fusion_step(None, 0, 0, 1, 1, 4, 37, 0, None, None, None, None, None, 0, 0.5, 0.0, -1, -1, -1, -1, None) == 0  # n == 0


def test_beam_inference_resolves_the_model_and_its_weights(tmp_path):
    model = X.random_model(11, 3, 12, lacking=2)
    lm = X.token_lm(model)
    assert BeamInference()._fusion() is None
    assert BeamInference(token_lm=lm)._fusion() == (lm, 0.3, 0.0)
    assert BeamInference(token_lm=lm, token_lm_weight=0.7)._fusion(token_score=0.5) == (lm, 0.7, 0.5)
    assert BeamInference()._fusion(lm, 1.0) == (lm, 1.0, 0.0)
    with pytest.raises(ValueError, match="which was not given"):
        BeamInference()._fusion(token_lm_weight=0.4)
    arpa, tokens = tmp_path / "pieces.arpa", tmp_path / "tokens.txt"
    arpa.write_text(model.arpa(), encoding="utf-8")
    tokens.write_text("\n".join(model.pieces) + "\n", encoding="utf-8")

    class Args:
        token_lm, token_lm_weight = str(arpa), 0.6
        trg_sos_idx, trg_eos_idx, trg_pad_idx = 1, 2, 3
    Args.tokens = str(tokens)
    inf = BeamInference(Args)
    read, w, ts = inf._fusion()
    assert isinstance(read, TokenLM) and (read.V, read.sos, read.eos, read.pad, w, ts) == (12, 1, 2, 3, 0.6, 0.0)
    assert inf._fusion()[0] is read  # read once
    assert read.score_of([1, 5, 6, 2], 0.6) == X.token_lm(model).score_of([1, 5, 6, 2], 0.6)
    assert "fusion" in CTCHypothesis.__slots__ and RescoredList._fields == FusedRescoredList._fields


def test_the_joint_lockstep_loop_applies_prefix_then_bias_then_model_and_the_final_term():
    """``_joint_lockstep_search`` on CPU tensors with all three scorers -- a ``CtcPrefixSession``, a ``ContextBiasSession`` and an
    ``LMFusionSession`` -- against the same three ``step`` calls written out around ``beam_select``, in the order prefix, bias, model,
    with the ``final`` tail, the PAD rewrite and the first-best pick: tokens and scores bit for bit.  n = 2 searches, beam 3, 5 steps.
    Search 0's emission allows the blank and one label over two frames, so two of its beams take EOS in the first two steps (asserted)
    and go on by PAD, and its third row is dead (score -inf); search 1 follows a six-token phrase, which is still open when the steps
    run out, so the ``final`` term is not zero (asserted)."""
    from early_exit_transformer_amd.beam import _joint_lockstep_search, sequence_length_penalty
    from early_exit_transformer_amd.context import ContextBiasSession, ContextGraph
    from early_exit_transformer_amd.model import CtcPrefixSession, beam_select
    model = X.random_model(2, 3, 37, lacking=4)
    lm = X.token_lm(model)
    n, beam, V, steps, alpha, w = 2, 3, model.V, 5, 0.6, 0.5
    sos, eos, pad = model.sos, model.eos, model.pad
    g = torch.Generator().manual_seed(3)
    table = torch.log_softmax(torch.randn(n, steps, V, V, generator=g), -1)
    em = torch.log_softmax(torch.randn(n, 6, V, generator=g), -1)
    em[0] = NEG
    em[0, :, 0], em[0, :, 5] = float(np.log(0.7)), float(np.log(0.3))
    em_len = torch.tensor([2, 6])
    graph = ContextGraph([(8, 9, 10, 11, 12, 13), (5,)], [3.0, 0.5], vocab_size=V, eos=eos, pad=pad)

    def sessions():
        return CtcPrefixSession(em, em_len, beam, w, eos, pad, blank=0), ContextBiasSession(graph, n, beam), LMFusionSession(lm, n, beam, 0.4, 0.1)

    def _rows(k, last):  # a toy decoder: the log-probs depend on the step and the last token
        return torch.stack([table[i, k][last[i]] for i in range(n)])
    at = iter(range(steps))
    prefix, bias, fusion = sessions()
    found = _joint_lockstep_search(lambda last, parent: _rows(next(at), last), prefix, n, torch.device("cpu"), steps, sos, eos, pad, beam, alpha, [bias, fusion])

    prefix, bias, fusion = sessions()
    scores = torch.zeros((n, 1))
    bufs = [torch.zeros((n, beam, steps + 1), dtype=torch.long) for _ in range(2)]
    bufs[0][:, 0, 0] = sos
    last, parent = bufs[0][:, :1, 0].contiguous(), None
    for i in range(steps):
        local = prefix.step(_rows(i, last), last, parent)
        local = bias.step(local, last, parent)
        local = fusion.step(local, last, parent)
        scores, parent, last = beam_select(local, scores, sequence_length_penalty(i + 1, alpha), beam, bufs[i & 1], bufs[(i + 1) & 1], i + 1)
    tail = bias.final(last, parent) / sequence_length_penalty(steps, alpha)
    scores = scores + tail
    raw = bufs[steps & 1]
    tokens = raw.clone()
    for i in range(n):
        for r in range(beam):
            row = raw[i, r].tolist()
            if eos in row:
                tokens[i, r, row.index(eos) + 1:] = pad
    assert (raw[0, :2, 1:3] == eos).any(dim=1).all() and (tail != 0).any() and torch.isfinite(scores).any(dim=1).all()
    for i in range(n):
        final_tokens, final_scores, best = found[i]
        assert torch.equal(torch.stack(final_tokens), tokens[i]) and torch.equal(torch.stack(final_scores), scores[i])
        assert best == tokens[i, max(range(beam), key=lambda r: (float(scores[i, r]), -r))].tolist()


def test_the_gpu_tests_inputs_leave_enough_ranks_to_compare():
    """The restated search at the GPU test's blocks, weights and variants: at least MIN_COMPARED of the present ranks have key gaps
    above BEAM_MARGIN, and fusion moves the best hypothesis of some sequences."""
    assert sum(logp.size(0) for _, _, logp, _ in X.ctc_blocks()) == 36
    for with_len, skip in RC.ALL_VARIANTS:
        fused, plain = X.restated_beams(X.CTC_W, X.CTC_TS, with_len, skip), X.restated_beams(0.0, 0.0, with_len, skip)
        compared = present = moved = 0
        for rows, rows0 in zip(fused, plain):
            for final, final0 in zip(rows, rows0):
                present += min(X.NBEST, len(final))
                compared += len(X.comparable_ranks(final))
                moved += final[0][0] != final0[0][0]
        print(f"own lengths {with_len}, skip drops {skip}: {compared} of {present} ranks comparable, the best hypothesis moves in {moved} of 36")
        assert compared >= RC.MIN_COMPARED * present and moved >= 4
