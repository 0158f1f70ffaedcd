"""What tests/test_gpu_aed_step.py rests on, checked on the reference alone (no device): the fp32 reference modules sit well
inside the bound around the fp64 oracle, so the oracle's own error does not eat the bound; ``rescale`` moves the decoder's
function by nothing; the driven prefixes are well formed; and every case's check steps bracket the thresholds it names."""
import copy

import pytest
import torch

import aed_step_cases as A

IDS = [c.id for c in A.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_fp32_reference_is_within_a_tenth_of_the_bound_of_the_fp64_oracle(cid):
    case = A.BY_ID[cid]
    model, mem = A.build_model(case), A.memory(case)
    worst = 0.0
    for s, prefixes in A.checked_prefixes(case).items():
        want = A.oracle(case)[s]
        assert want.shape == (*case.EB, case.rows(s), case.geo[3]) and want.dtype == torch.float64
        finite, top = bool(torch.isfinite(want).all()), want.abs().max().item()
        assert finite and top < 10.0, (cid, s, top)  # every bound sits at its floor
        got = A.reference(model, mem, prefixes)
        assert got.dtype == torch.float32
        err = (got.double() - want).abs().max().item()
        assert err <= 0.1 * A.bound(want, batched=False), (cid, s, err)
        worst = max(worst, err)
    print(f"{cid}: fp32 reference against the fp64 oracle, worst |dlogp| = {worst:.2e} (bound {A.bound(want, False):.1e})")


@pytest.mark.parametrize("e", [4, 8])
def test_rescaling_leaves_the_fp64_oracle_unchanged(e):
    case = A.W_CASE
    m64 = A.rescale(copy.deepcopy(A.build_model(case)).double(), e)
    mem = A.memory(case).double()
    D = case.geo[0]
    base = A.build_model(case).decoders[0].layers[0]
    assert torch.equal(m64.decoders[0].layers[0].linear1.weight.float() * 2.0 ** e, base.linear1.weight)  # it did rescale
    assert torch.equal(m64.decoders[1].layers[1].multihead_attn.in_proj_weight[:2 * D].float(),
                       A.build_model(case).decoders[1].layers[1].multihead_attn.in_proj_weight[:2 * D])  # queries and keys untouched
    for s, prefixes in A.checked_prefixes(case).items():
        assert (A.reference(m64, mem, prefixes) - A.oracle(case)[s]).abs().max().item() <= 1e-12, (e, s)


@pytest.mark.parametrize("cid", IDS)
def test_prefixes_are_well_formed_and_the_schedules_give_the_claimed_rows(cid):
    case = A.BY_ID[cid]
    E, B = case.EB
    V = case.geo[3]
    pads_before_last, seen_m = 0, set()
    last = None
    for s, tok, parent, prefixes in A.drive(case):
        R = case.rows(s)
        assert 1 <= R <= 16 and tok.shape == (*case.lead, R) and prefixes.shape == (E, B, R, s + 1)
        assert (parent is None) == (s == 0)
        if s:
            assert parent.shape == tok.shape and 0 <= int(parent.min()) and int(parent.max()) < last.size(2)
            # host-side prefixes: the parent's prefix plus the new token
            p4, t4 = parent.reshape(E, B, R), tok.reshape(E, B, R)
            assert torch.equal(prefixes[..., :-1], torch.gather(last, 2, p4.unsqueeze(-1).expand(E, B, R, s)))
            assert torch.equal(prefixes[..., -1], t4)
        assert int(tok.min()) >= 0 and int(tok.max()) < V
        if s in case.checks:
            assert torch.equal(prefixes, A.checked_prefixes(case)[s])
            assert (prefixes[..., 0] == A.SOS).all()          # starts with SOS,
            assert not (prefixes == A.PAD).all(dim=-1).any()  # so no prefix is all PAD
            pads_before_last += int((prefixes[..., :-1] == A.PAD).sum())
            seen_m.add(B * R)
        last = prefixes
    assert s == case.steps - 1 and case.steps <= A.MAX_LEN
    assert pads_before_last > 0  # the key-padding mask is exercised at a checked step
    if case.batched:
        assert set(case.m_values) <= seen_m, (case.m_values, seen_m)


def test_parents_repeat_and_drop_rows():
    for case in A.CASES:
        repeats = drops = 0
        prev_rows = None
        for s, tok, parent, _ in A.drive(case):
            if s:
                p = parent.reshape(-1, parent.size(-1))
                for row in p:
                    used = set(row.tolist())
                    repeats += len(used) < row.numel()
                    drops += len(used) < prev_rows
            prev_rows = tok.size(-1)
        assert repeats > 0 and drops > 0, case.id


@pytest.mark.parametrize("cid", IDS)
def test_check_steps_bracket_the_thresholds(cid):
    case = A.BY_ID[cid]
    checks = set(case.checks)
    assert checks <= set(range(case.steps)) and {0, 1, 2, case.steps - 1} <= checks
    for t in case.thresholds:
        assert {t - 1, t} <= checks and t < case.steps, (cid, t)


def test_the_cases_reach_the_paths_they_are_there_for():
    """The thresholds of the module docstring, restated as arithmetic on the cases (not computed from the package)."""
    by = A.BY_ID
    second_pv_trip = {64: 32, 32: 64, 16: 128, 8: 256}  # head dim -> keys beyond which step_attn's P.V loop takes a second trip
    for cid, dh in (("P1", 8), ("P2", 16), ("P3-1", 32), ("P3-3", 32), ("P3-6", 32), ("P4", 64)):
        c = by[cid]
        assert c.geo[0] // c.geo[1] == dh and second_pv_trip[dh] in c.thresholds and c.steps > second_pv_trip[dh]
    assert by["P2"].Tq > 128 and by["P3-1"].Tq > 256 and by["P4"].Tq > 32  # the cross-attention's second trips
    assert by["P1"].steps > 257 and by["B1"].steps > 257 and 256 in by["B1"].thresholds  # score loop beyond 256 keys
    assert (by["P2"].geo[0] // 4) == 24 and 256 % 24  # per_row does not divide 256
    assert by["P1"].geo[2] % 16 and by["P2"].geo[2] % (16 * 4) and by["P1"].geo[2] % 8 == 4  # contraction tails; K % 8 == 4
    assert by["P1"].geo[3] % 32 and by["B1"].geo[3] % 32  # V tail
    assert by["P5"].geo[0] == 1024 and by["B5"].geo[0] == 1024
    assert [by[f"B2-{t}"].Tq for t in (255, 256, 257, 513)] == [255, 256, 257, 513]
    assert by["B3"].lead[0] == 8 and by["B1"].Tq == 1
    assert [c.lead for c in (by["P3-1"], by["P3-3"], by["P3-6"])] == [(1,), (3,), (6,)]
    w = A.W_CASE
    assert w.geo == (256, 8, 2048, 256, 2) and w.lead == (2, 2) and w.cycle == (10,) and w.Tq == 45 and w.checks == tuple(range(12))
    assert A.W_EXPONENTS == (0, 4, 8)
