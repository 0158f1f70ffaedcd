"""What tests/test_gpu_aed_train.py rests on, checked without a device (cases, oracle and restated path rules:
tests/aed_train_cases.py): the case table reaches every GEMM path and reduction variant the benchmark's geometry runs; the fp64
oracle is finite and the fp32 reference modules sit within 1/20 of the bounds around it, so the oracle's own error does not eat
them; the exact-zero gradients are exactly those of ``one_key``; the padding and token patterns the cases are there for are
present; and the dropout masks of the two masked cases keep a fraction inside the binomial band."""
import copy

import pytest
import torch

import aed_train_cases as A
import dropout_cases as DC
from oracle import dropout_ref

# test_training_gemm_at_size_selected_paths (tests/test_gpu_train.py) runs the single 128 x 128 GEMM with a bias through
# eec_train_gemm at M = 16384: the one path of the benchmark's decoder step (its key / value projection, [16384][512]) that no case
# here reaches -- a decoder case that did would need B T' >= 16384 rows of memory
EXEMPT = {((128, 128), "single", "bias", True, True)}


def test_the_cases_reach_every_gemm_path_and_reduction_of_the_benchmark():
    bench_gemms, bench_reduces = A.launches(*A.BENCH_GEO)
    # the restated rules on the benchmark's geometry, against the issue's own figures
    assert [A.weight_grad_splits(64 * 43, n, k)[0] for n, k in ((256, 256), (768, 256), (256, 2048), (2048, 256))] == [43, 29, 15, 15]
    assert A.weight_grad_splits(64 * 256, 512, 256)[0] == 64
    assert {g.tile for g in bench_gemms if g.name in ("ca scores", "ca dP")} == {(128, 128)}
    reached, reduces = {}, set()
    for case in A.CASES:
        gemms, red = A.launches(*case.launch_geo)
        for g in gemms:
            reached.setdefault(g.combo, set()).add(case.id)
        reduces |= set(red)
    missing = {g.combo: g.name for g in bench_gemms if g.combo not in reached}
    assert set(missing) == EXEMPT, missing
    assert set(bench_reduces) <= reduces, set(bench_reduces) - reduces
    assert {("split", 4), ("split", 16), ("ln2", 16)} <= set(bench_reduces)


def test_the_cases_reach_the_paths_they_are_there_for():
    """The table of the issue, restated as arithmetic on the launch lists."""
    by = {c.id: dict(zip(("gemms", "reduces"), A.launches(*c.launch_geo))) for c in A.CASES}
    geo = {c.id: c.geo for c in A.CASES}

    def of(cid, *names):
        found = [g for g in by[cid]["gemms"] if g.name in names]
        assert found, (cid, names)
        return found

    # bench_paths: batched 128 x 128, epi 5 / 6 on 128 x 64, 33 and 65 weight-gradient splits with the bias tail, 2112 tokens per walk
    assert geo["bench_paths"] == (64, 33, 65, 1, 128, 8, 2048, 64, 30)
    assert all(g.tile == (128, 128) and g.nz == 512 and g.N == 65 for g in of("bench_paths", "ca scores", "ca dP"))
    assert all(g.tile == (128, 64) and g.M == 2112 for g in of("bench_paths", "linear1", "dpre"))
    assert {g.splits for g in by["bench_paths"]["gemms"] if g.epi == "rowsum"} >= {33, 65}
    assert ("split", 16) in by["bench_paths"]["reduces"] and ("ln2", 16) in by["bench_paths"]["reduces"]
    # long: softmax trips, two row tiles per batch in dK / dV, the N > 64 fallback tile, no 16-byte epilogue on V and d_ff
    assert geo["long"] == (2, 129, 257, 2, 64, 4, 100, 37, 36)
    assert (A.softmax_trips(129), A.softmax_trips(257)) == (3, 5) and A.softmax_trips(64) == 1 and A.softmax_trips(65) == 2
    assert all(g.M == 257 and g.M > g.tile[0] for g in of("long", "ca dK", "ca dV"))
    assert all(g.tile == (64, 64) and g.N > 64 for g in of("long", "sa scores", "ca scores"))
    assert not of("long", "head")[0].cvec and of("bench_paths", "head")[0].cvec
    assert 100 % 32 and 37 % 4  # d_ff: a ragged k-tile in linear2 and its gradients; V: rows of 37 floats are not 16-byte aligned (head dX, dW)
    # edges_S: the three tile choices of the self-attention's scores and the lane loop's boundary
    assert [geo[c][1] for c in A.EDGES_S] == [1, 2, 33, 64, 65] and all(geo[c][:1] + geo[c][2:7] == (2, 9, 1, 64, 4, 96) for c in A.EDGES_S)
    assert [of(c, "sa scores")[0].tile for c in A.EDGES_S] == [(128, 32), (128, 32), (128, 64), (128, 64), (64, 64)]
    assert geo["one_key"][1:3] == (5, 1)
    # deep_wide: the benchmark's depth and widths, head dim 64, the embedding's second column trip
    assert geo["deep_wide"] == (3, 7, 31, 6, 512, 8, 2048, 256, 30) and A.BENCH_GEO[3] == 6 and A.embed_trips(512) == 2 and A.embed_trips(256) == 1
    assert sum(g.epi == "accumulate" for g in by["deep_wide"]["gemms"]) == 5
    # max_geo: what check_geo allows at most for LayerNorm and vocabulary
    assert geo["max_geo"] == (2, 9, 33, 1, 1024, 16, 64, 1000, 0) and A.ln_variant(1024) == 16 and 1024 == 64 * A.K_LN_MAX
    assert {A.ln_variant(geo[c][4]) for c in A.IDS} == {4, 8, 16}
    assert geo["odd_D"][4:7] == (96, 6, 160) and 96 % 64 and 160 % 64
    assert A.BY_ID["max_len"].geo[1] == A.BY_ID["max_len"].max_len
    assert geo["peaky_x4"] == geo["peaky_x16"] == geo["peaky_x1"] == (4, 42, 64, 3, 256, 8, 192, 64, 30)
    assert [A.BY_ID[c].qk_scale ** 2 for c in ("peaky_x1", "peaky_x4", "peaky_x16")] == [1.0, 4.0, 16.0]
    assert all(g.tile == (128, 128) and g.nz == 16 for g in of("wgrad_128", "linear1 dW", "linear2 dW"))


@pytest.mark.parametrize("cid", A.IDS)
def test_oracle_is_finite_and_the_fp32_modules_are_within_a_twentieth_of_the_bounds(cid):
    case = A.BY_ID[cid]
    B, S, Tq, L, D, H, F, V, pad = case.geo
    f = A.PEAKY_FACTOR.get(cid, 1.0)
    for idx in (1, 0):
        want = A.oracle(case, idx)
        assert want.logits.shape == (B, S, V) and want.grad_enc.shape == (B, Tq, D) and want.logits.dtype == torch.float64
        assert torch.isfinite(want.logits).all() and torch.isfinite(want.grad_enc).all()
        assert all(torch.isfinite(g).all() for g in want.grads.values())
        assert len(want.grads) == 5 + 18 * L, sorted(want.grads)  # embedding, shared norm, head; 18 tensors per layer
        got = A.reference_step(A.cpu_model(case), case, idx, torch.float32)
        fl, fg, fe = A.fractions(got, want, f)
        print(f"{cid} exit {idx}: fp32 modules against the fp64 oracle, fractions of the bounds: logits {fl:.4f}, gradients {fg:.4f}, grad_enc {fe:.4f}")
        assert max(fl, fg, fe) <= 1 / 20, (cid, idx, fl, fg, fe)


@pytest.mark.parametrize("cid", A.IDS)
def test_exact_zero_gradients_are_those_of_one_key_and_no_others(cid):
    case = A.BY_ID[cid]
    D = case.geo[4]
    trg = A.inputs(case)[0]
    for idx in (1, 0):
        grads = A.oracle(case, idx).grads
        zero = {n for n, g in A.one_key_zero_slices(grads, D) if not g.any()}
        if cid == "one_key":
            assert len(zero) == 4 * case.geo[3] == len(A.one_key_zero_slices(grads, D))
            for n, g in grads.items():  # the value third is alive
                if n.endswith("multihead_attn.in_proj_weight"):
                    assert g[2 * D:].any()
        else:
            assert not zero, zero
        whole = {n for n, g in grads.items() if not g.any()}
        assert whole == ({n for n in grads if n.endswith(("norm2.weight", "norm2.bias"))} if cid == "one_key" else set()), whole
        used = torch.zeros(case.geo[7], dtype=torch.bool)
        used[trg.unique()] = True
        emb = grads["emb.weight"]
        assert not emb[~used].any() and emb[used].abs().amax(dim=1).min().item() > 0


def test_padding_patterns_and_token_properties_are_present():
    seen = set()
    pads = set()
    for case in A.CASES:
        B, S, _, _, _, _, _, V, pad = case.geo
        trg = A.inputs(case)[0]
        assert trg.shape == (B, S) and trg.dtype == torch.int64 and (trg[:, 0] == A.SOS).all() and pad != A.SOS
        assert int(trg.min()) >= 0 and int(trg.max()) < V and S <= case.max_len
        is_pad = trg == pad
        pads.add("0" if pad == 0 else "V-1" if pad == V - 1 else str(pad))
        if not is_pad.any():
            seen.add("none")
        # trailing: a row's padding is a suffix; lengths differ between the rows
        n_pad = is_pad.sum(dim=1)
        suffix = torch.stack([is_pad[r, S - int(n_pad[r]):].all() for r in range(B)])
        if len({int(n) for n, ok in zip(n_pad, suffix) if ok and n > 0}) >= 2:
            seen.add("trailing")
        if any(S > 2 and int(n_pad[r]) == S - 1 for r in range(B)):
            seen.add("all_after_first")
        if any(bool(is_pad[r, :-1].any()) and not bool(suffix[r]) for r in range(B)):
            seen.add("middle")
        counts = torch.bincount(trg.flatten(), minlength=V)
        if case.tokens == "repeat":
            block = trg[: B // 2, 1:]
            tok = int(block[0, 0])
            assert B // 2 >= 2 and (block[~is_pad[: B // 2, 1:]] == tok).all() and int(counts[tok]) > 256
            seen.add("repeat")
        if int((counts == 0).sum()) > 3:
            seen.add("unused")
    assert seen == {"none", "trailing", "all_after_first", "middle", "repeat", "unused"}, seen
    assert {"0", "30", "V-1"} <= pads, pads


@pytest.mark.parametrize("cid", A.DROPOUT_IDS)
def test_keep_rate_and_independence_of_the_masks_of_the_dropout_cases(cid):
    """In the manner of tests/test_oracle_dropout.py, for the shapes of the two masked cases: every mask keeps a fraction within
    4 sqrt(p (1 - p) / n) of 1 - p, no site is drawn twice, and every two masks agree on a fraction within the band of
    p^2 + (1 - p)^2 over the step's smallest masked tensor."""
    import numpy as np
    p = DC.DECODER_P
    used = A.dropout_sites(A.BY_ID[cid])
    assert len({s for s, _ in used}) == len(used)
    for site, n in used:
        kept = dropout_ref.keep_mask(DC.DECODER_SEED, site, p, n).mean()
        assert abs(kept - (1 - p)) <= DC.binomial_band(p, n), f"{cid}: site {site}: kept {kept:.4f} of {n}"
    n = min(n for _, n in used)
    m = np.stack([dropout_ref.keep_mask(DC.DECODER_SEED, s, p, n) for s, _ in used]).astype(np.float64)
    agree = (m @ m.T + (1 - m) @ (1 - m).T) / n
    q = p * p + (1 - p) * (1 - p)
    assert np.abs(agree - q)[np.triu_indices(len(used), 1)].max() <= DC.binomial_band(q, n)


def test_peaky_scaling_multiplies_the_query_and_key_rows_only():
    base, x16 = A.cpu_model(A.BY_ID["peaky_x1"]), copy.deepcopy(A.cpu_model(A.BY_ID["peaky_x16"]))
    D = A.PEAKY_GEO[4]
    sb, sx = base.state_dict(), x16.state_dict()
    for k in sb:
        if k.startswith("decoders.") and k.endswith("attn.in_proj_weight"):
            assert torch.equal(sx[k][:2 * D], sb[k][:2 * D] * 4.0) and torch.equal(sx[k][2 * D:], sb[k][2 * D:])
        else:
            assert torch.equal(sx[k], sb[k]), k
