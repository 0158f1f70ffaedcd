"""CPU tests of error-rate scoring (early_exit_transformer_amd/scoring.py; include/eec.h, "Edit distance"): the restatement of
tests/edit_cases.py against a brute force over all alignments, the host path of ``edit_counts`` against the restatement on every
shared case, the op strings replayed, interning, the tables and their rates, the oracle picks, ``exit_tradeoff`` against a loop over
``select_exits``, and the host side of the C entry: declared, exported, every bad argument refused with its own message before
anything is launched (no device here)."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import edit_cases as X
from conftest import ROOT
from early_exit_transformer_amd import capi, ctc, scoring
from early_exit_transformer_amd.build import LIB_PATH

BAD_ARG, BAD_WS = 10001, 10003
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        from early_exit_transformer_amd.build import build_library
        build_library()
    return capi.load()


# ---------------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_brute_force_on_all_binary_pairs():
    seqs = X.binary_sequences()
    assert len(seqs) == 31
    for r, h in itertools.product(seqs, repeat=2):
        d, s, dl, ins, ops = X.restate(r, h)
        assert (d, s) == X.brute_force(r, h), (r, h)
        assert d == s + dl + ins and len(h) - len(r) == ins - dl and min(s, dl, ins) >= 0
        ok, spent = X.replay(r, h, ops)
        assert ok and spent == (s, dl, ins, len(r) - s - dl), (r, h, ops)


@pytest.mark.parametrize("name", list(X.cases()))
def test_host_path_equals_the_restatement(name):
    hyp, hl, ref, rl, of = X.cases()[name]
    got = scoring.edit_counts(hyp, hl, ref, rl, of, want_ops=True)
    X.check_against_expected(name, got, sentinel=0)
    plain = scoring.edit_counts(hyp, hl, ref, rl, of)
    assert plain.ops is None and plain.n_ops is None
    assert all(torch.equal(a, b) for a, b in zip(plain[:5], got[:5]))


@pytest.mark.parametrize("name", list(X.cases()))
def test_every_op_string_replays_the_reference_into_the_hypothesis(name):
    """Of the restatement (what the host path and the kernel are held to): the ops turn ``ref`` into ``hyp`` and spend the reported
    counts."""
    hyp, hl, ref, rl, of = X.cases()[name]
    counts, n_ops, ops = X.expected(name)
    for p, op in enumerate(ops):
        q = p if of is None else int(of[p])
        if not 0 <= q < ref.size(0):
            assert op == [] and counts[p].tolist() == [-1] * 4
            continue
        n, m = min(max(int(hl[p]), 0), hyp.size(1)), min(max(int(rl[q]), 0), ref.size(1))
        ok, spent = X.replay(ref[q, :m].tolist(), hyp[p, :n].tolist(), op)
        d, s, dl, ins = counts[p].tolist()
        assert ok and spent == (s, dl, ins, m - s - dl) and len(op) == n + dl and d == s + dl + ins, (name, p)


def test_garbage_past_the_lengths_would_change_the_result_if_read():
    """The padding of the shared cases is not inert: scoring the whole rows gives other counts."""
    hyp, hl, ref, rl, of = X.cases()["ref-of"]
    whole = scoring.edit_counts(hyp, torch.full_like(hl, hyp.size(1)), ref, torch.full_like(rl, ref.size(1)), of)
    assert not torch.equal(whole.distance, X.expected("ref-of")[0][:, 0])


def test_edit_counts_takes_int64_that_fits_and_refuses_the_rest():
    hyp, hl, ref, rl, of = X.cases()["int32-extremes"]
    got = scoring.edit_counts(hyp.long(), hl.long(), ref.long(), rl.long(), of)
    assert torch.equal(got.distance, X.expected("int32-extremes")[0][:, 0])
    big = hyp.long().clone()
    big[0, 0] = 1 << 31
    with pytest.raises(ValueError, match="do not fit int32"):
        scoring.edit_counts(big, hl, ref.long(), rl)
    with pytest.raises(ValueError, match="at most 1024"):
        scoring.edit_counts(torch.zeros((1, 1025), dtype=torch.int32), torch.tensor([3]), ref, rl, torch.tensor([0]))
    with pytest.raises(ValueError, match="one reference per pair"):
        scoring.edit_counts(hyp[:2], hl[:2], ref, rl)
    with pytest.raises(ValueError, match="int32 or int64"):
        scoring.edit_counts(hyp.float(), hl, ref, rl)
    none = scoring.edit_counts(hyp[:0], hl[:0], ref[:0], rl[:0], want_ops=True)
    assert none.distance.shape == (0,) and none.ops.shape == (0, hyp.size(1) + ref.size(1))


# ---------------------------------------------------------------------------------------------------------------------------
# texts, tables, picks
# ---------------------------------------------------------------------------------------------------------------------------
def test_interning():
    table = {}
    refs = scoring.intern(["the cat  sat", "", " on the mat "], "word", table)
    assert refs.rows.dtype == refs.lens.dtype == torch.int32 and refs.lens.tolist() == [3, 0, 3]
    assert table == {"the": 0, "cat": 1, "sat": 2, "on": 3, "mat": 4}
    assert refs.rows[0, :3].tolist() == [0, 1, 2] and refs.rows[2, :3].tolist() == [3, 0, 4]
    hyps = scoring.intern(["the dog sat", "mat"], "word", table)
    assert hyps.rows[0, :3].tolist() == [0, 5, 2] and hyps.rows[1, :1].tolist() == [4] and table["dog"] == 5
    chars = scoring.intern(["a b", "ba", ""], "char")
    assert chars.lens.tolist() == [3, 2, 0] and chars.rows[0].tolist() == [0, 1, 2] and chars.rows[1, :2].tolist() == [2, 0]
    assert scoring.intern([], "word").rows.shape == (0, 1)
    with pytest.raises(ValueError, match="unit"):
        scoring.intern(["a"], "bpe")

    class Hyp:
        tokens = [4, 5]
    rows = scoring.TokenRows.from_lists([[1, 2, 3], [], Hyp(), torch.tensor([7])])
    assert rows.lens.tolist() == [3, 0, 2, 1] and rows.rows[2, :2].tolist() == [4, 5] and rows.rows.shape == (4, 3)
    with pytest.raises(ValueError, match="int32"):
        scoring.TokenRows.from_lists([[1 << 31]])


def test_error_table_layouts_units_and_rates():
    refs = ["the cat sat", "on the mat"]
    hyps = [["the cat sat", "on mat"], ["a cat sat down", "on the mat"]]  # [E][B]
    t = scoring.error_table(hyps, refs, unit="word")
    assert t.errors.tolist() == [[0, 1], [2, 0]] and t.subs.tolist() == [[0, 0], [1, 0]]
    assert t.dels.tolist() == [[0, 1], [0, 0]] and t.ins.tolist() == [[0, 0], [1, 0]] and t.ref_len.tolist() == [3, 3]
    assert t.rate().tolist() == [1 / 6, 2 / 6] and t.rate().dtype == torch.float64
    by_utt = [[hyps[e][b] for e in range(2)] for b in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(scoring.error_table(by_utt, refs, unit="word", layout="BE"), t))
    c = scoring.error_table([["abc", ""]], ["abd", "xy"], unit="char")
    assert c.errors.tolist() == [[1, 2]] and c.dels.tolist() == [[0, 2]]
    ids = scoring.error_table([[[1, 2, 3], [4]], [[1, 3], []]], [[1, 2, 3], [4, 5]], unit="token")
    assert ids.errors.tolist() == [[0, 1], [1, 2]]
    # N-best lists, ragged: an absent entry is -1 everywhere and the rate is the first entries'
    nb = scoring.error_table([[["a b", "a c", "a"], ["x"]]], ["a c", "x y"], unit="word")
    assert nb.errors.tolist() == [[[1, 0, 1], [1, -1, -1]]] and nb.subs.tolist() == [[[1, 0, 0], [0, -1, -1]]]
    assert nb.rate().tolist() == [2 / 4]
    idx, err = scoring.nbest_oracle(nb.errors)
    assert idx.tolist() == [[1, 0]] and err.tolist() == [[0, 1]] and nb.rate(err).tolist() == [1 / 4]
    with pytest.raises(ValueError, match="one per reference"):
        scoring.error_table([["a"]], ["a", "b"])
    with pytest.raises(ValueError, match="unit"):
        scoring.error_table([["a"]], ["a"], unit="bpe")


def test_rate_on_empty_corpora():
    none = scoring.ErrorTable(*(torch.zeros((3, 0), dtype=torch.int32) for _ in range(4)), torch.zeros((0,), dtype=torch.int32))
    assert none.rate().tolist() == [0.0, 0.0, 0.0]
    t = scoring.error_table([["", ""], ["a", ""]], ["", ""], unit="word")  # references without tokens
    assert t.errors.tolist() == [[0, 0], [1, 0]] and t.rate().tolist() == [0.0, float("inf")]
    assert scoring.error_rate(torch.tensor([2, 1]), torch.tensor([4, 2])).item() == 0.5


def test_oracle_picks_break_ties_to_the_shallowest_exit_and_the_better_rank():
    errors = torch.tensor([[3, 0, 2, 5], [1, 0, 2, 5], [1, 4, 1, 5]], dtype=torch.int32)
    exit_of, best = scoring.oracle_exit(errors)
    assert exit_of.tolist() == [1, 0, 2, 0] and exit_of.dtype == torch.int32 and best.tolist() == [1, 0, 1, 5]
    idx, err = scoring.nbest_oracle(torch.tensor([[2, 1, 1], [-1, -1, -1], [0, -1, -1], [4, 4, 3]]))
    assert idx.tolist() == [1, 0, 0, 2] and err.tolist() == [1, -1, 0, 3]
    with pytest.raises(ValueError):
        scoring.oracle_exit(errors[0])


def test_exit_tradeoff_equals_a_loop_over_select_exits():
    g = torch.Generator().manual_seed(5)
    E, B = 5, 37
    errors = torch.randint(0, 9, (E, B), generator=g, dtype=torch.int32)
    ref_len = torch.randint(1, 12, (B,), generator=g, dtype=torch.int32)
    score = (torch.randint(0, 6, (E, B), generator=g) / 5.0).float()  # ties with the thresholds below
    score[torch.rand(E, B, generator=g) < 0.1] = NAN
    flat = [0.0, 0.2, 0.4, 0.6, 1.1]
    per_exit = [[0.2, 0.4, 0.6, 0.8, 1.0], [1.0, 0.0, 1.0, 0.0, 1.0]]
    for thresholds, hib, lo, hi in ((flat, False, 0, None), (flat, True, 1, 3), (per_exit, False, 0, 4), (per_exit, True, 2, None)):
        got = scoring.exit_tradeoff(errors, ref_len, score, thresholds, hib, lo, hi)
        assert got.exit_of.shape == (len(thresholds), B) and got.histogram.shape == (len(thresholds), E)
        for k, thr in enumerate(thresholds):
            want = ctc.select_exits(score, thr, hib, lo, hi)
            assert torch.equal(got.exit_of[k], want)
            total = sum(int(errors[int(e), b]) for b, e in enumerate(want.tolist()))
            assert got.rate[k].item() == total / int(ref_len.sum())
            assert got.mean_exit[k].item() == sum(want.tolist()) / B
            assert got.histogram[k].tolist() == [want.tolist().count(e) for e in range(E)]
    assert len({tuple(r) for r in scoring.exit_tradeoff(errors, ref_len, score, flat).exit_of.tolist()}) > 2  # the thresholds do differ
    with pytest.raises(ValueError, match=r"\[K\] or \[K, 5\]"):
        scoring.exit_tradeoff(errors, ref_len, score, [[0.1, 0.2]])
    with pytest.raises(ValueError, match="both be"):
        scoring.exit_tradeoff(errors, ref_len, score[:2], flat)


def test_beam_inference_error_table_reads_what_the_decoders_return():
    """Nested token lists (``decode_batch``: out[b][e]), hypothesis objects (``ctc_cuda_predict``: [B][N], and a list of them per
    exit), ``(hypotheses, exit_of)`` and ``(tokens, exit)`` rows; words after detokenize / lexicon."""
    from early_exit_transformer_amd.beam import BeamInference, CTCHypothesis, DecodedTokens
    inf = BeamInference()
    refs = [[5, 6, 7], [8, 9]]
    out = [[[5, 6, 7], [5, 7]], [[8], [8, 9]]]  # [B][E]
    t = inf.error_table(out, refs)
    assert t.errors.tolist() == [[0, 1], [1, 0]] and t.ref_len.tolist() == [3, 2]
    hyp = lambda ids: CTCHypothesis(list(ids), [], 0.0)  # noqa: E731
    one_exit = [[hyp([5, 6]), hyp([5, 6, 7])], [hyp([9])]]  # [B][N], ragged
    t = inf.error_table(one_exit, refs)
    assert t.errors.tolist() == [[[1, 0], [1, -1]]]
    assert inf.error_table([one_exit, one_exit], refs).errors.shape == (2, 2, 2)
    assert inf.error_table((one_exit, torch.tensor([0, 1])), refs).errors.tolist() == t.errors.tolist()
    assert inf.error_table([([5, 6, 7], 0), ([9], 3)], refs).errors.tolist() == [[0, 1]]
    assert inf.error_table(out, (torch.tensor([[5, 6, 7], [8, 9, 0]]), torch.tensor([3, 2]))).errors.tolist() == [[0, 1], [1, 0]]
    words = {5: "the", 6: "cat", 7: "sat", 8: "on", 9: "mat"}
    detok = lambda ids: " ".join(words[i] for i in ids)  # noqa: E731
    t = inf.error_table(out, ["the cat sat", "on a mat"], unit="word", detokenize=detok)
    assert t.errors.tolist() == [[0, 2], [1, 1]] and t.ref_len.tolist() == [3, 3]
    assert inf.error_table(out, ["the cat sat", "on a mat"], unit="char", detokenize=detok).errors[0].tolist() == [0, 6]
    snapped = [[DecodedTokens(ids) for ids in row] for row in out]
    for row in snapped:
        for ids in row:
            ids.text = "on a mat"
    assert inf.error_table(snapped, ["the cat sat", "on a mat"], unit="word", detokenize=detok, lexicon=["unused"]).errors.tolist() == [[3, 0], [3, 0]]
    with pytest.raises(ValueError, match="detokenize"):
        inf.error_table(out, ["the cat sat", "on a mat"], unit="word")


# ---------------------------------------------------------------------------------------------------------------------------
# the C entry without a device
# ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "eec.h")).read()
    for name in ("eec_edit_distance_workspace_bytes", "eec_edit_distance"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/eec.h"
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert int(re.search(r"#define\s+EEC_EDIT_MAX_LEN\s+(\d+)", header).group(1)) == scoring.EDIT_MAX_LEN == 1024
    assert lib.eec_abi_version() == 16


def _stale(lib):
    """Another entry's message on the library's error string."""
    buf = (C.c_int32 * 64)()
    assert lib.eec_lexicon_nearest(buf, 0, buf, buf, 1, 4, buf, buf, buf, 256, None) != 0
    msg = lib.eec_last_error()
    assert msg and b"edit distance" not in msg
    return msg


def _call(lib, n_pairs=3, hyp_pitch=8, ref_pitch=8, n_refs=3, null=(), ops=False, ws=0x1000, ws_bytes=None, counts=0x1000):
    """One eec_edit_distance call with made-up device addresses: every case here must be refused before anything is dereferenced."""
    fake = lambda name: None if name in null else C.c_void_p(0x1000)  # noqa: E731  (256-byte aligned, never read)
    want_ops = ops or "n_ops" in null
    nbytes = lib.eec_edit_distance_workspace_bytes(n_pairs, ref_pitch, hyp_pitch, int(want_ops)) if ws_bytes is None else ws_bytes
    return lib.eec_edit_distance(fake("hyp"), fake("hyp_len"), n_pairs, hyp_pitch, fake("ref"), fake("ref_len"), n_refs, ref_pitch, fake("ref_of"),
                                 None if "counts" in null else C.c_void_p(counts), C.c_void_p(0x2000) if want_ops else None,
                                 C.c_void_p(0x3000) if ops and "n_ops" not in null else None, None if "workspace" in null else C.c_void_p(ws),
                                 nbytes, None)


REFUSALS = [
    ("null hyp", dict(null=("hyp",)), BAD_ARG, "null argument"),
    ("null hyp_len", dict(null=("hyp_len",)), BAD_ARG, "null argument"),
    ("null ref", dict(null=("ref",)), BAD_ARG, "null argument"),
    ("null ref_len", dict(null=("ref_len",)), BAD_ARG, "null argument"),
    ("null counts", dict(null=("counts",)), BAD_ARG, "null argument"),
    ("counts misaligned", dict(counts=0x1004), BAD_ARG, "16-byte aligned"),
    ("n_pairs -1", dict(n_pairs=-1), BAD_ARG, "n_pairs must not be negative, got -1"),
    ("hyp_pitch -1", dict(hyp_pitch=-1), BAD_ARG, "hyp_pitch -1"),
    ("hyp_pitch 1025", dict(hyp_pitch=1025), BAD_ARG, "hyp_pitch 1025"),
    ("ref_pitch -1", dict(ref_pitch=-1), BAD_ARG, "ref_pitch -1"),
    ("ref_pitch 1025", dict(ref_pitch=1025), BAD_ARG, "ref_pitch 1025"),
    ("n_refs 0", dict(n_refs=0), BAD_ARG, "n_refs must be positive, got 0"),
    ("no ref_of, n_refs != n_pairs", dict(n_refs=2, null=("ref_of",)), BAD_ARG, "n_refs must equal n_pairs"),
    ("ops without n_ops", dict(null=("n_ops",)), BAD_ARG, "ops without n_ops"),
    ("null workspace with ops", dict(ops=True, null=("workspace",)), BAD_ARG, "null workspace"),
    ("short workspace", dict(ops=True, ws_bytes=16), BAD_WS, "workspace too small"),
    ("misaligned workspace", dict(ops=True, ws=0x1010), BAD_WS, "256-byte aligned"),
]


@pytest.mark.parametrize("what,kw,code,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses_bad_arguments_without_a_device(lib, what, kw, code, msg):
    stale = _stale(lib)
    assert _call(lib, **kw) == code, what
    err = lib.eec_last_error()
    assert err != stale and err.startswith(b"edit distance:") and msg in err.decode(), (what, err)


def test_entry_accepts_an_empty_call(lib):
    """n_pairs == 0 is a successful no-op whatever the pointers; a pitch of 0 needs no token pointer (refused later, for its counts)."""
    assert _call(lib, n_pairs=0, null=("hyp", "hyp_len", "ref", "ref_len", "counts", "workspace")) == 0
    assert _call(lib, n_pairs=0, n_refs=0, ops=True, null=("workspace",)) == 0
    _stale(lib)
    assert _call(lib, hyp_pitch=0, ref_pitch=0, null=("hyp", "ref", "counts")) == BAD_ARG and b"null argument" in lib.eec_last_error()


def test_workspace_size_is_monotonic_and_zero_for_nothing(lib):
    ws = lib.eec_edit_distance_workspace_bytes
    for P, M, N, ops in itertools.product((0, -1, 3), (0, -2, 5), (0, -7, 9), (0, -1, 1)):
        if min(P, M, N, ops) <= 0:
            assert ws(P, M, N, ops) == 0, (P, M, N, ops)
    assert ws(3, 5, 9, 1) == 3 * 5 * 4 and ws(1, 1, 1, 1) == 4 and ws(1, 1024, 1024, 1) == 1024 * 256
    assert ws(1 << 20, 1024, 1024, 1) == (1 << 20) * 1024 * 256  # above 2^32 bytes: size_t arithmetic
    sizes = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)
    for fixed in (1, 7):
        for a, b in zip(sizes, sizes[1:]):
            assert ws(a, fixed, fixed, 1) <= ws(b, fixed, fixed, 1)
            assert ws(fixed, a, fixed, 1) <= ws(fixed, b, fixed, 1)
            assert ws(fixed, fixed, a, 1) <= ws(fixed, fixed, b, 1)
            assert ws(a, b, b, 0) <= ws(a, b, b, 1) == ws(a, b, b, 2)
