"""Error-rate scoring: hypotheses and references into error counts, per exit and per threshold of the adaptive exit choice.

* ``edit_counts``     the batched edit distance of include/eec.h ("Edit distance"; csrc/edit_distance.hip): distance, substitutions,
  deletions, insertions and hits of many (hypothesis, reference) pairs of token rows, optionally the alignment as an op string.
  Device tensors go through the kernel; CPU tensors take a host path that is the same statement in NumPy row sweeps.
* ``intern`` / ``TokenRows``   texts (words or characters) and nested token lists as padded int32 rows.
* ``error_table``     the errors of every exit's hypothesis of every utterance (or of every entry of an N-best list) -> ``ErrorTable``;
  ``ErrorTable.rate`` is the corpus-level error rate per exit.
* ``oracle_exit`` / ``nbest_oracle``   the shallowest exit with the fewest errors; the best hypothesis of every list.
* ``exit_tradeoff``   error rate against depth for a list of thresholds, the exits chosen by ``select_exits`` itself.

Limits: rows of at most 1024 tokens; unit costs only (sclite's weights are not served); the distance is free of any convention,
the substitution / deletion / insertion split is the fewest-substitutions one (include/eec.h)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import capi
from .ctc import select_exits

EDIT_MAX_LEN = 1024  # EEC_EDIT_MAX_LEN
OP_HIT, OP_SUB, OP_DEL, OP_INS = 0, 1, 2, 3
_STEP, _SUB = 1 << 16, (1 << 16) + 1


class EditCounts(NamedTuple):
    """Per pair, int32 [P]: the Levenshtein distance and its split (``distance = subs + dels + ins``, ``hits = ref_len - subs -
    dels``); all -1 for a pair whose ``ref_of`` entry names no reference.  With ``want_ops``: ``ops`` uint8 [P, ref pitch + hyp
    pitch], the alignment of pair p in ``ops[p, :n_ops[p]]`` (0 hit, 1 substitution, 2 deletion, 3 insertion), zeros past it; else
    both None."""
    distance: Tensor
    subs: Tensor
    dels: Tensor
    ins: Tensor
    hits: Tensor
    ops: Optional[Tensor]
    n_ops: Optional[Tensor]


def _token_rows(name: str, t: Tensor, dev: torch.device) -> Tensor:
    if not isinstance(t, Tensor) or t.dim() != 2:
        raise ValueError(f"edit_counts: {name} must be a 2-D tensor of token ids, got {tuple(getattr(t, 'shape', ()))}")
    if t.device != dev:
        raise ValueError(f"edit_counts: {name} is on {t.device}, hyp on {dev}")
    if t.dtype == torch.int64:
        if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= 1 << 31):
            raise ValueError(f"edit_counts: {name} holds int64 ids that do not fit int32")
        t = t.to(torch.int32)
    if t.dtype != torch.int32:
        raise ValueError(f"edit_counts: {name} must be int32 or int64, got {t.dtype}")
    if t.size(1) > EDIT_MAX_LEN:
        raise ValueError(f"edit_counts: {name} rows of {t.size(1)} tokens, at most {EDIT_MAX_LEN} are served")
    return t.contiguous()


def _int32_vector(name: str, t: Tensor, n: int, dev: torch.device, hi: int) -> Tensor:
    """``t`` [n] as int32 on ``dev``; int64 values are first clamped to [-1, hi], which the entry treats as it would the originals."""
    if not isinstance(t, Tensor) or t.dim() != 1 or t.numel() != n or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"edit_counts: {name} must be an int32 or int64 tensor of {n} entries")
    if t.dtype == torch.int64:
        t = t.clamp(-1, hi)
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _host_counts(hyp: np.ndarray, hyp_len: np.ndarray, ref: np.ndarray, ref_len: np.ndarray, ref_of: np.ndarray, want_ops: bool):
    """The statement of include/eec.h for P pairs side by side, one NumPy sweep per reference row.  In a row the insertion
    candidate chains through the row itself; with base = min(diag, del) it is min_k<=j (base[k] + (j - k) * STEP), a running
    minimum of base[j] - j * STEP."""
    P = hyp.shape[0]
    valid = (ref_of >= 0) & (ref_of < ref.shape[0])
    rsel = np.where(valid, ref_of, 0)
    n = np.where(valid, np.clip(hyp_len, 0, hyp.shape[1]), 0).astype(np.int64)
    m = np.where(valid, np.clip(ref_len[rsel] if ref.shape[0] else 0, 0, ref.shape[1]), 0).astype(np.int64)
    M, N = int(m.max(initial=0)), int(n.max(initial=0))
    cols = np.arange(N + 1, dtype=np.int32)  # keys stay below 2^28: int32 sweeps
    K = np.broadcast_to(cols * _STEP, (P, N + 1)).copy()
    h = hyp[:, :N]
    inside = cols[None, 1:] <= n[:, None]  # columns past a length hold nothing that is read; their tokens are not compared
    dirs = np.zeros((P, M, N), dtype=np.uint8) if want_ops else None
    for i in range(1, M + 1):
        act = i <= m
        r = ref[rsel, i - 1]
        eq = (h == r[:, None]) & inside
        cd = K[:, :-1] + np.where(eq, np.int32(0), np.int32(_SUB))
        cu = K[:, 1:] + np.int32(_STEP)
        base = np.concatenate([np.full((P, 1), i * _STEP, dtype=np.int32), np.minimum(cd, cu)], axis=1)
        cur = np.minimum.accumulate(base - cols * _STEP, axis=1) + cols * _STEP
        if want_ops:
            v = cur[:, 1:]
            dirs[:, i - 1] = np.where(v == cd, np.where(eq, OP_HIT, OP_SUB), np.where(v == cu, OP_DEL, OP_INS))
        K = np.where(act[:, None], cur, K)
    kend = np.where(n > 0, K[np.arange(P), n].astype(np.int64), m * _STEP)
    dist, subs = kend >> 16, kend & 0xffff
    dels = (dist - subs - (n - m)) // 2
    ins = dels + n - m
    counts = np.stack([dist, subs, dels, ins], axis=1)
    counts[~valid] = -1
    ops = n_ops = None
    if want_ops:
        ops = np.zeros((P, ref.shape[1] + hyp.shape[1]), dtype=np.uint8)
        n_ops = np.where(valid, n + dels, 0).astype(np.int32)
        for p in np.nonzero(valid)[0]:
            i, j, pos = int(m[p]), int(n[p]), int(n_ops[p])
            while i > 0 or j > 0:
                code = OP_INS if i == 0 else OP_DEL if j == 0 else int(dirs[p, i - 1, j - 1])
                pos -= 1
                ops[p, pos] = code
                i -= code != OP_INS
                j -= code != OP_DEL
    return counts.astype(np.int32), ops, n_ops


def edit_counts(hyp: Tensor, hyp_len: Tensor, ref: Tensor, ref_len: Tensor, ref_of: Optional[Tensor] = None, want_ops: bool = False,
                max_workspace_bytes: int = 2 << 30) -> EditCounts:
    """``EditCounts`` of P pairs: hypothesis p, ``hyp[p, :hyp_len[p]]``, against reference ``ref_of[p]`` (None: reference p, and as
    many references as pairs), ``ref[r, :ref_len[r]]``.  Token ids are int32, or int64 that fit int32 (refused otherwise), compared
    by equality only; lengths are clamped to [0, row length], tokens at or past a length are never read; rows of at most 1024
    tokens.  Unit costs; among the minimum-cost alignments the one with the fewest substitutions is counted (include/eec.h).
    On the device one eec_edit_distance launch (two with ``want_ops``) per chunk of pairs whose op workspace stays inside
    ``max_workspace_bytes``; integer only, so results are bit-identical run to run and whatever the chunking.  CPU tensors take
    the host path."""
    if not isinstance(hyp, Tensor):
        raise ValueError("edit_counts: hyp must be a tensor")
    dev = hyp.device
    hyp, ref = _token_rows("hyp", hyp, dev), _token_rows("ref", ref, dev)
    P, R = hyp.size(0), ref.size(0)
    hyp_len = _int32_vector("hyp_len", hyp_len, P, dev, EDIT_MAX_LEN + 1)  # lengths are clamped to [0, pitch] anyway
    ref_len = _int32_vector("ref_len", ref_len, R, dev, EDIT_MAX_LEN + 1)
    if ref_of is None:
        if R != P:
            raise ValueError(f"edit_counts: without ref_of there must be one reference per pair, got {R} for {P}")
    else:
        ref_of = _int32_vector("ref_of", ref_of, P, dev, min(R, (1 << 31) - 1))  # R itself names no reference
    want_ops = bool(want_ops)
    Lh, Lr = hyp.size(1), ref.size(1)
    if not hyp.is_cuda:
        of = np.arange(P, dtype=np.int64) if ref_of is None else ref_of.numpy().astype(np.int64)
        step = max(1, (64 << 20) // max(Lh * Lr, 1)) if want_ops else max(P, 1)
        parts = [_host_counts(hyp.numpy()[c:c + step], hyp_len.numpy()[c:c + step], ref.numpy(), ref_len.numpy(), of[c:c + step], want_ops)
                 for c in range(0, P, step)]
        counts = torch.from_numpy(np.concatenate([q[0] for q in parts], axis=0) if parts else np.zeros((0, 4), np.int32))
        ops = torch.from_numpy(np.concatenate([q[1] for q in parts], axis=0) if parts else np.zeros((0, Lr + Lh), np.uint8)) if want_ops else None
        n_ops = torch.from_numpy(np.concatenate([q[2] for q in parts], axis=0) if parts else np.zeros((0,), np.int32)) if want_ops else None
    else:
        lib = capi.load()
        counts = torch.empty((P, 4), dtype=torch.int32, device=dev)
        ops = torch.zeros((P, Lr + Lh), dtype=torch.uint8, device=dev) if want_ops else None
        n_ops = torch.zeros((P,), dtype=torch.int32, device=dev) if want_ops else None  # rows of no tokens have no ops to ask for
        per_pair = lib.eec_edit_distance_workspace_bytes(1, Lr, Lh, int(want_ops))
        step = max(1, int(max_workspace_bytes) // per_pair) if per_pair else max(P, 1)
        rows = lambda t, c=0: None if t is None or t.numel() == 0 else t[c:]  # noqa: E731
        ws = ws_ptr = None
        for c in range(0, P, step):
            k = min(step, P - c)
            nbytes = lib.eec_edit_distance_workspace_bytes(k, Lr, Lh, int(want_ops))
            if nbytes and ws is None:
                ws, ws_ptr = capi.aligned_ws(nbytes, dev)  # the first chunk is the largest
            # without ref_of a chunk scores against its own slice of the references
            refs, ref_lens, n_refs = (rows(ref, c), rows(ref_len, c), k) if ref_of is None else (rows(ref), rows(ref_len), R)
            capi.launch("eec_edit_distance", dev, rows(hyp, c), rows(hyp_len, c), k, Lh, refs, ref_lens, n_refs, Lr, rows(ref_of, c),
                        rows(counts, c), rows(ops, c), rows(n_ops, c), ws_ptr, nbytes)
    hits = torch.where(counts[:, 0] < 0, counts[:, 0], _ref_lengths(ref_len, ref_of, Lr, P) - counts[:, 1] - counts[:, 2])
    return EditCounts(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], hits.to(torch.int32), ops, n_ops)


def _ref_lengths(ref_len: Tensor, ref_of: Optional[Tensor], pitch: int, P: int) -> Tensor:
    """The clamped reference length of every pair (0 where ``ref_of`` names none)."""
    lens = ref_len.clamp(0, pitch)
    if ref_of is None:
        return lens
    if lens.numel() == 0:
        return torch.zeros((P,), dtype=torch.int32, device=ref_len.device)
    ok = (ref_of >= 0) & (ref_of < lens.numel())
    return torch.where(ok, lens[ref_of.clamp(0, lens.numel() - 1).long()], torch.zeros_like(ref_of))


# ---------------------------------------------------------------------------------------------------------------------------
# Texts and nested token lists as padded rows
# ---------------------------------------------------------------------------------------------------------------------------
class TokenRows(NamedTuple):
    """``rows`` int32 [n, L] (L = the longest row, at least 1; padded with -1) and ``lens`` int32 [n], on the host."""
    rows: Tensor
    lens: Tensor

    @classmethod
    def from_lists(cls, seqs: Sequence[Sequence[int]]) -> "TokenRows":
        """Token-id lists -- ``decode_batch``'s ``out[b][e]``, the ``.tokens`` of ``ctc_cuda_predict``'s hypotheses, the entries of an
        N-best list, flattened by the caller -- as rows.  Tensors and objects with ``.tokens`` are taken as their ids."""
        seqs = [_ids(s) for s in seqs]
        L = max([len(s) for s in seqs] + [1])
        rows = np.full((len(seqs), L), -1, dtype=np.int64)
        for i, s in enumerate(seqs):
            rows[i, :len(s)] = s
        if rows.size and (rows.min() < -(1 << 31) or rows.max() >= 1 << 31):
            raise ValueError("TokenRows: ids that do not fit int32")
        return cls(torch.from_numpy(rows.astype(np.int32)), torch.tensor([len(s) for s in seqs], dtype=torch.int32))


def _ids(s) -> List[int]:
    s = getattr(s, "tokens", s)
    return [int(v) for v in (s.tolist() if isinstance(s, Tensor) else s)]


def intern(texts: Sequence[str], unit: str = "word", table: Optional[Dict[str, int]] = None) -> TokenRows:
    """``texts`` as id rows through one host dictionary: words are ``str.split()``'s, characters are taken as they come (spaces
    included).  ``table`` (symbol -> id) is extended in place by the symbols it has not seen, in order of appearance, so hypotheses
    and references interned through the same table compare by symbol; None: a fresh one for this call."""
    if unit not in ("word", "char"):
        raise ValueError(f"intern: unit must be 'word' or 'char', got {unit!r}")
    table = {} if table is None else table
    return TokenRows.from_lists([[table.setdefault(s, len(table)) for s in (t.split() if unit == "word" else t)] for t in texts])


# ---------------------------------------------------------------------------------------------------------------------------
# Tables per exit and utterance
# ---------------------------------------------------------------------------------------------------------------------------
def error_rate(errors: Tensor, ref_len: Tensor) -> Tensor:
    """Corpus-level error rate, fp64 [...]: the sum of ``errors`` [..., B] over the utterances by the sum of ``ref_len`` [B].  A corpus
    without reference tokens gives 0.0 where there are no errors and ``inf`` where there are."""
    e = errors.to(torch.float64).sum(dim=-1)
    n = ref_len.to(torch.float64).sum()
    if n > 0:
        return e / n
    return torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e))


class ErrorTable(NamedTuple):
    """``errors = subs + dels + ins`` and its parts, int32 [E, B] -- [E, B, N] for N-best lists, -1 where a list has no N-th entry --
    and ``ref_len`` int32 [B], on the host."""
    errors: Tensor
    subs: Tensor
    dels: Tensor
    ins: Tensor
    ref_len: Tensor

    def rate(self, errors: Optional[Tensor] = None) -> Tensor:
        """The error rate of every exit over the corpus, fp64 [E] (``error_rate``): of ``errors`` [E, B] when given (say
        ``nbest_oracle``'s), else of the table's own -- for N-best lists of every list's first entry."""
        e = self.errors if errors is None else errors
        return error_rate(e[..., 0] if errors is None and e.dim() == 3 else e, self.ref_len)


def _leaf(x, unit: str) -> bool:
    return isinstance(x, str) if unit != "token" else (hasattr(x, "tokens") or isinstance(x, Tensor) or
                                                       (isinstance(x, (list, tuple)) and all(isinstance(v, (int, np.integer)) for v in x)
                                                        and not any(isinstance(v, bool) for v in x)))


def error_table(hyps, refs, unit: str = "word", layout: str = "EB", device=None, want_nbest: Optional[bool] = None) -> ErrorTable:
    """The errors of every hypothesis against its utterance's reference.  ``hyps`` is indexed ``[E][B]`` (``layout="EB"``), ``[B][E]``
    (``layout="BE"``, what ``decode_batch`` returns) or ``[E][B][N]`` (N-best lists, ragged allowed; ``want_nbest`` says so where
    the nesting alone cannot, None: inferred from the first entry); ``refs`` is ``[B]``.  Entries are strings with ``unit="word"``
    (split by ``str.split()``) or ``"char"``, token-id lists (or tensors, or objects with ``.tokens``) with ``unit="token"``.
    ``device``: a HIP device to score on (the kernel), None: the host path."""
    if unit not in ("word", "char", "token"):
        raise ValueError(f"error_table: unit must be 'word', 'char' or 'token', got {unit!r}")
    if layout not in ("EB", "BE"):
        raise ValueError(f"error_table: layout must be 'EB' or 'BE', got {layout!r}")
    refs = list(refs)
    B = len(refs)
    hyps = [list(row) for row in hyps]
    if layout == "BE":
        if len(hyps) != B:
            raise ValueError(f"error_table: {len(hyps)} rows of hypotheses for {B} references")
        E = len(hyps[0]) if hyps else 0
        if any(len(row) != E for row in hyps):
            raise ValueError("error_table: every utterance needs one hypothesis per exit")
        hyps = [[hyps[b][e] for b in range(B)] for e in range(E)]
    E = len(hyps)
    if any(len(row) != B for row in hyps):
        raise ValueError(f"error_table: every exit needs {B} entries, one per reference")
    if want_nbest is None:
        want_nbest = E > 0 and B > 0 and not _leaf(hyps[0][0], unit)
    if want_nbest:
        lists = [[list(h) for h in row] for row in hyps]
        N = max([len(h) for row in lists for h in row] + [1])
    else:
        lists, N = [[[h] for h in row] for row in hyps], 1
    flat, ref_of = [], []
    for row in lists:
        for b, entries in enumerate(row):
            flat += entries + [entries[0] if entries else ([] if unit == "token" else "")] * (N - len(entries))
            ref_of += [b] * len(entries) + [-1] * (N - len(entries))  # an absent entry names no reference: counts -1
    if unit == "token":
        h, r = TokenRows.from_lists(flat), TokenRows.from_lists(refs)
    else:
        table: Dict[str, int] = {}
        r, h = intern(refs, unit, table), intern(flat, unit, table)
    dev = torch.device("cpu") if device is None else torch.device(device)
    c = edit_counts(h.rows.to(dev), h.lens.to(dev), r.rows.to(dev), r.lens.to(dev), torch.tensor(ref_of, dtype=torch.int32, device=dev))
    shape = (E, B, N) if want_nbest else (E, B)
    subs, dels, ins = (t.cpu().reshape(shape) for t in (c.subs, c.dels, c.ins))
    return ErrorTable(c.distance.cpu().reshape(shape), subs, dels, ins, r.lens.clone())


def oracle_exit(errors: Tensor) -> Tuple[Tensor, Tensor]:
    """``(exit_of int32 [B], errors [B])`` from ``errors`` [E, B]: the shallowest exit with the fewest errors, and that count."""
    if errors.dim() != 2 or errors.size(0) < 1:
        raise ValueError(f"oracle_exit: errors must be [E, B], got {tuple(errors.shape)}")
    E = errors.size(0)
    best = errors.min(dim=0).values
    at = torch.where(errors == best, torch.arange(E, device=errors.device).view(E, 1), E).min(dim=0).values
    return at.to(torch.int32), best


def nbest_oracle(errors: Tensor) -> Tuple[Tensor, Tensor]:
    """``(index int32 [...], errors [...])`` from ``errors`` [..., N]: the entry of every list with the fewest errors, ties to the
    better rank; negative entries (absent hypotheses) are never chosen, a list without entries gives (0, -1)."""
    if errors.dim() < 1 or errors.size(-1) < 1:
        raise ValueError(f"nbest_oracle: errors must be [..., N] with N >= 1, got {tuple(errors.shape)}")
    N = errors.size(-1)
    big = torch.iinfo(errors.dtype).max
    e = torch.where(errors < 0, torch.full_like(errors, big), errors)
    best = e.min(dim=-1, keepdim=True).values
    at = torch.where(e == best, torch.arange(N, device=errors.device), N).min(dim=-1).values
    none = (errors < 0).all(dim=-1)
    return (torch.where(none, torch.zeros_like(at), at).to(torch.int32),
            torch.where(none, torch.full_like(best[..., 0], -1), best[..., 0]))


class ExitTradeoff(NamedTuple):
    """Per threshold k: ``exit_of`` int32 [K, B], the corpus error ``rate`` fp64 [K] at those exits, ``mean_exit`` fp64 [K] (0-based)
    and ``histogram`` int64 [K, E], the utterances that left at every exit."""
    exit_of: Tensor
    rate: Tensor
    mean_exit: Tensor
    histogram: Tensor


def exit_tradeoff(errors: Tensor, ref_len: Tensor, score: Tensor, thresholds, higher_is_better: bool = False, min_exit: int = 0,
                  max_exit: Optional[int] = None) -> ExitTradeoff:
    """The accuracy-against-depth curve of an early-exit model from one full forward and one decode of every exit: for every
    threshold -- ``thresholds`` [K] (one value for all exits) or [K, E] -- the exit of every utterance is
    ``select_exits(score, threshold, higher_is_better, min_exit, max_exit)`` (``score`` [E, B]: a field of ``exit_statistics`` or any
    criterion), the error rate is that of ``errors`` [E, B] (``ErrorTable.errors``) at those exits over ``ref_len`` [B]."""
    if errors.dim() != 2 or score.shape != errors.shape:
        raise ValueError(f"exit_tradeoff: errors and score must both be [E, B], got {tuple(errors.shape)} and {tuple(score.shape)}")
    E, B = errors.shape
    thr = torch.as_tensor(thresholds, dtype=torch.float64)
    if thr.dim() not in (1, 2) or (thr.dim() == 2 and thr.size(1) != E):
        raise ValueError(f"exit_tradeoff: thresholds must be [K] or [K, {E}], got {tuple(thr.shape)}")
    errors_h = errors.cpu()
    exits = [select_exits(score, t.tolist(), higher_is_better, min_exit, max_exit).cpu() for t in thr]
    exit_of = torch.stack(exits) if exits else torch.zeros((0, B), dtype=torch.int32)
    at = errors_h.t().unsqueeze(0).expand(len(exits), B, E).gather(2, exit_of.long().unsqueeze(-1)).squeeze(-1)
    hist = torch.stack([torch.bincount(x.long(), minlength=E) for x in exits]) if exits else torch.zeros((0, E), dtype=torch.int64)
    mean = exit_of.to(torch.float64).mean(dim=1) if B else torch.zeros((len(exits),), dtype=torch.float64)
    return ExitTradeoff(exit_of, error_rate(at, ref_len.cpu()), mean, hist)
