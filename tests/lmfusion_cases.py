"""Inputs and plain-Python restatements shared by tests/test_host_lmfusion.py and tests/test_gpu_lmfusion.py (shallow fusion with a
token-level n-gram model; include/eec.h, "Shallow fusion").  A model here is a dictionary {n-gram of piece strings: (logp, backoff)};
nothing below reads the packed image.  Everything is seeded and runs on the CPU."""
import functools
import itertools
import math

import numpy as np
import torch

import ctc_cases as K
import rescore_cases as RC

NEG = -float("inf")
BOS, EOS, UNK = "<s>", "</s>", "<unk>"
BEAM, NBEST = 16, 4
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------
class Model:
    """``grams``: {tuple of words: (logp, backoff)} (fp32 values, prefix-closed, every word has a unigram); ``pieces`` [V]: the piece
    string of every token; the tokens ``blank`` / ``sos`` / ``eos`` / ``pad`` (None: none) are special."""

    def __init__(self, grams, order, pieces, blank=0, sos=None, eos=None, pad=None):
        self.grams, self.order, self.pieces = grams, order, list(pieces)
        self.blank, self.sos, self.eos, self.pad = blank, sos, eos, pad
        self.V = len(self.pieces)
        self.has = lambda w: (w,) in grams  # noqa: E731
        self.skip = {t for t in (blank, sos, pad) if t is not None}

    def word(self, token):
        """The LM word of a token: its piece, or <unk> where the model lacks it."""
        p = self.pieces[token]
        return p if self.has(p) else UNK

    def start(self):
        return (BOS,) if self.has(BOS) else ()

    def state(self, history):
        """The longest suffix of ``history`` of at most order - 1 words that is an n-gram of the model."""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        while h and h not in self.grams:
            h = h[1:]
        return h

    def arrays(self):
        """(words, logp, backoff per order, vocab, word_map, bos, eos_word, unk) as TokenLM's array constructor takes them."""
        vocab = [g[0] for g in self.grams if len(g) == 1]
        ids = {w: i for i, w in enumerate(vocab)}
        per = [[g for g in self.grams if len(g) == n + 1] for n in range(self.order)]
        words = [np.array([[ids[w] for w in g] for g in gs], dtype=np.int32).reshape(-1, n + 1) for n, gs in enumerate(per)]
        logp = [np.array([self.grams[g][0] for g in gs], dtype=np.float32) for gs in per]
        backoff = [np.array([self.grams[g][1] for g in gs], dtype=np.float32) for gs in per]
        fall = ids.get(UNK, 0)
        word_map = np.array([ids.get(p, fall) for p in self.pieces], dtype=np.int32)
        return words, logp, backoff, vocab, word_map, ids.get(BOS, -1), ids.get(EOS, -1), ids.get(UNK, -1)

    def arpa(self):
        """The model as the text of an ARPA file."""
        per = [[g for g in self.grams if len(g) == n + 1] for n in range(self.order)]
        lines = ["", "\\data\\"] + [f"ngram {n + 1}={len(gs)}" for n, gs in enumerate(per)]
        for n, gs in enumerate(per):
            lines += ["", f"\\{n + 1}-grams:"]
            for g in gs:
                lp, bo = self.grams[g]
                lines.append(f"{float(lp)!r}\t{' '.join(g)}" + (f"\t{float(bo)!r}" if n + 1 < self.order else ""))
        return "\n".join(lines + ["", "\\end\\", ""])


def token_lm(model):
    """``lm_fusion.TokenLM`` of ``model``, through the array constructor."""
    from early_exit_transformer_amd.lm_fusion import TokenLM
    words, logp, backoff, vocab, word_map, bos, eos_word, unk = model.arrays()
    return TokenLM(words, logp, backoff, model.V, word_map, bos=bos, eos_word=eos_word, unk=unk, vocab=vocab, blank=model.blank, sos=model.sos,
                   eos=model.eos, pad=model.pad)


def random_model(seed, order, V, bos=True, eos=True, unk=True, lacking=0, specials=True, density=0.35, pad=3):
    """A seeded, prefix-closed, unnormalised model: logp in [-4, 0], backoff in [-1, 0] (0 at the full order).  Pieces "p0" .. ; the
    last ``lacking`` ordinary pieces have no unigram (they score as <unk>, which ``lacking`` > 0 therefore needs).  ``specials``: token 0
    is the blank, 1 SOS, 2 EOS, ``pad`` PAD (V >= 5); else the blank alone.  Some n-grams end in </s>, some contexts have no children."""
    rng = np.random.RandomState(seed)
    pieces = [f"p{v}" for v in range(V)]
    special = dict(blank=0, sos=1, eos=2, pad=pad) if specials else dict(blank=0)
    ordinary = [pieces[v] for v in range(V) if v not in special.values()]
    known = ordinary[: len(ordinary) - lacking] if lacking else ordinary
    vocab = known + ([BOS] if bos else []) + ([EOS] if eos else []) + ([UNK] if unk else [])
    assert not lacking or unk
    val = lambda n: (F32(-4.0 * rng.rand()), F32(-rng.rand()) if n < order else F32(0.0))  # noqa: E731
    grams = {(w,): val(1) for w in vocab}
    if eos:
        grams[(EOS,)] = (grams[(EOS,)][0], F32(0.0))
    level = [g for g in grams if g != (EOS,)]
    for n in range(2, order + 1):
        nxt = []
        heads = [g for g in level if rng.rand() < 0.7] or level[:1]  # the others: contexts with an empty edge range
        for g in heads[:40]:
            for w in vocab:
                if w != BOS and rng.rand() < density:
                    grams[g + (w,)] = val(n) if w != EOS else (val(n)[0], F32(0.0))
                    if w != EOS:
                        nxt.append(g + (w,))
        level = nxt
        if not level:
            break
    return Model(grams, order, pieces, **special)


def normalised_model(seed=5, V=9, order=3):
    """A properly normalised back-off model over the pieces p1 .. and </s>, with <s> as a context: every context lists some words
    with probabilities that sum to less than one, and its back-off is computed so that the row sums to one,
    (1 - sum of the listed p(w | h)) / (1 - sum of the model's p(w | the next shorter state) over the same words), shortest contexts
    first.  A context without listed words has back-off 0 (a factor of one)."""
    rng = np.random.RandomState(seed)
    pieces = [f"p{v}" for v in range(V)]
    vocab = pieces[1:] + [EOS]  # what can be predicted; token 0 is the blank
    grams = {(w,): (F32(math.log10(p)), F32(0.0)) for w, p in zip(vocab, rng.dirichlet(np.ones(len(vocab))))}
    grams[(BOS,)] = (F32(-99.0), F32(0.0))
    contexts, listed = [g for g in grams if g != (EOS,)], {}
    for n in range(2, order + 1):
        new = []
        for h in [h for h in contexts if rng.rand() < 0.7] or contexts[:1]:
            kids = [w for w in vocab if rng.rand() < 0.4] or vocab[:1]
            mass = 0.3 + 0.6 * rng.rand()
            listed[h] = kids
            for w, p in zip(kids, rng.dirichlet(np.ones(len(kids))) * mass):
                grams[h + (w,)] = (F32(math.log10(p)), F32(0.0))
                if w != EOS and n < order:
                    new.append(h + (w,))
        contexts = new
    model = Model(grams, order, pieces, blank=0)
    for h in sorted(listed, key=len):
        kids = listed[h]
        num = 1.0 - sum(10.0 ** float(grams[h + (w,)][0]) for w in kids)
        den = 1.0 - sum(10.0 ** float(backoff_score(model, model.state(h[1:]), w)[0]) for w in kids)
        grams[h] = (grams[h][0], F32(math.log10(num / den)))
    return model


# ---------------------------------------------------------------------------------------------------------------------------
# the back-off scorers: fp64 over the dictionary, and the fp32 chain in the walk's order
# ---------------------------------------------------------------------------------------------------------------------------
def backoff_score(model, state, word, dtype=np.float64, parts=None):
    """(log10 p(word | state), the state after it): x = state + word in the model -> its logp; otherwise the state's backoff and on with
    the longest proper suffix that is in the model.  One addition per step, in that order, in ``dtype``.  ``parts``: a list that
    receives every number added."""
    acc = dtype(0.0)
    h = tuple(state)
    while True:
        x = h + (word,)
        if x in model.grams:
            acc = dtype(acc + dtype(model.grams[x][0]))
            if parts is not None:
                parts.append(float(model.grams[x][0]))
            return acc, model.state(x)
        assert h, f"{word!r} has no unigram"
        acc = dtype(acc + dtype(model.grams[h][1]))
        if parts is not None:
            parts.append(float(model.grams[h][1]))
        h = h[1:]
        while h and h not in model.grams:
            h = h[1:]


DEAD = "dead"


def increment(model, state, token, w, ts, dtype=np.float32, ctc=False, terms=None):
    """(inc, next state) of ``token`` from ``state``: fl(fl(w * acc) + ts); 0 for a skip token and in the dead state.  ``ctc``: the
    blank is the only special token.  ``terms``: a list that receives |w * each number of the walk| and |ts|."""
    if state == DEAD:
        return dtype(0.0), DEAD
    parts = []
    if not ctc and token == model.eos:
        acc, nxt = (backoff_score(model, state, EOS, dtype, parts)[0] if model.has(EOS) else dtype(0.0)), DEAD
    elif token == model.blank or (not ctc and token in model.skip):
        return dtype(0.0), state
    else:
        acc, nxt = backoff_score(model, state, model.word(token), dtype, parts)
    if terms is not None:
        terms += [abs(w * p) for p in parts] + [abs(ts)]
    return dtype(dtype(dtype(w) * acc) + dtype(ts)), nxt


def chain(model, tokens, w, ts, dtype=np.float32, ctc=False, terms=None):
    """The fusion score of a token row: fl(fusion + inc) along the row in ``dtype``; an AED row (a leading SOS is not scored) or a CTC
    row (``ctc``: </s> is paid at the end, without the bonus).  ``terms``: a list that receives the magnitude of every number that
    enters the sum: |w * logp| and |w * backoff| of every walk, and |ts| per scored token."""
    row = list(tokens)
    if not ctc and row and row[0] == model.sos:
        row = row[1:]
    total, state = dtype(0.0), model.start()
    for t in row:
        inc, state = increment(model, state, t, w, ts, dtype, ctc, terms)
        if inc != 0:
            total = dtype(total + inc)
    if ctc and model.has(EOS):
        parts = []
        fin = dtype(dtype(w) * backoff_score(model, state, EOS, dtype, parts)[0])
        total = dtype(total + fin)
        if terms is not None:
            terms += [abs(w * p) for p in parts]
    return total


# ---------------------------------------------------------------------------------------------------------------------------
# the fused prefix beam search in fp64: ctxbias_cases.biased_beam_search with the increment swapped
# ---------------------------------------------------------------------------------------------------------------------------
def _lae(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def fused_beam_search(logp, model, w, ts, beam=BEAM, blank=0, blank_skip_threshold=0.95, skip_drops_frame=False):
    """logp [T', V] -> the final beam [(prefix list, total log-probability, final fusion score, key)], best key first, ties to the
    lower beam index.  ``model`` None: no fusion.  The fusion score is carried as the fp32 chain (it is a function of the row)."""
    T, V = logp.shape
    log_thr = math.log(blank_skip_threshold) if 0.0 < blank_skip_threshold < 1.0 else 0.0
    on = model is not None and not (w == 0 and ts == 0)
    incs = {}

    def inc_of(st, c):
        if not on:
            return F32(0.0), st
        if (st, c) not in incs:
            incs[st, c] = increment(model, st, c, w, ts, np.float32, ctc=True)
        return incs[st, c]
    beams = [((), 0.0, NEG, model.start() if on else (), F32(0.0))]  # (prefix, log p_blank, log p_nonblank, LM state, fusion)
    for t in range(T):
        lp = logp[t].astype(np.float64)
        lpb = float(lp[blank])
        if blank_skip_threshold < 1.0 and lpb > log_thr:
            if not skip_drops_frame:
                beams = [(p, _lae(pb, pnb) + lpb, NEG, st, bi) for p, pb, pnb, st, bi in beams]
            continue
        index = {b[0]: i for i, b in enumerate(beams)}
        stay_pb = [_lae(pb, pnb) + lpb for _, pb, pnb, _, _ in beams]
        stay_pnb = [(pnb + float(lp[p[-1]])) if p else NEG for p, _, pnb, _, _ in beams]
        cands = []  # (key, id, prefix, pb, pnb, state, fusion)
        for i, (p, pb, pnb, st, bi) in enumerate(beams):
            tot = _lae(pb, pnb)
            for c in range(V):
                if c == blank:
                    continue
                v = (pb if (p and p[-1] == c) else tot) + float(lp[c])
                q = p + (c,)
                j = index.get(q)
                if j is not None:
                    stay_pnb[j] = _lae(stay_pnb[j], v)
                elif v > NEG:
                    inc, ns = inc_of(st, c)
                    nb = F32(bi + inc)
                    cands.append((v + float(nb), 16 + c * 16 + i, q, NEG, v, ns, nb))
        for i, (p, _, _, st, bi) in enumerate(beams):
            cands.append((_lae(stay_pb[i], stay_pnb[i]) + float(bi), i, p, stay_pb[i], stay_pnb[i], st, bi))
        cands = [c for c in cands if c[0] > NEG]
        cands.sort(key=lambda c: (-c[0], c[1]))
        beams = [c[2:] for c in cands[:beam]]
    final = []
    for p, pb, pnb, st, bi in beams:
        fb = bi
        if on and model.has(EOS):
            fb = F32(bi + F32(F32(w) * backoff_score(model, st, EOS, np.float32)[0]))
        tot = _lae(pb, pnb)
        final.append((list(p), tot, float(fb), tot + float(fb)))
    final.sort(key=lambda e: -e[3])  # stable: ties to the lower beam index
    return final


# the CTC inputs: 36 sequences, T' in {1, 2, 40}, three scales, four sequences each with the lengths 0, T', T' / 2, T' - 1; V = 37
CTC_V = 37
CTC_SHAPES = (1, 2, 40)
CTC_W, CTC_TS = 0.5, 0.25


@functools.lru_cache(maxsize=None)
def ctc_blocks():
    """[(T', scale, logp [4, T', 37] fp32, em_len int32 [4])]"""
    out = []
    for T, scale in itertools.product(CTC_SHAPES, RC.NBEST_SCALES):
        lens = torch.tensor([0, T, max(1, T // 2), max(0, T - 1)], dtype=torch.int32)
        out.append((T, scale, K.beam_logp(RC.NBEST_N, T, CTC_V, scale, seed=int(scale)).float(), lens))
    return out


@functools.lru_cache(maxsize=None)
def ctc_model():
    """The model of the CTC tests: order 3 over 37 pieces with the blank as the only special token; <s>, </s>, <unk>, three pieces lacking."""
    return random_model(37, 3, CTC_V, lacking=3, specials=False, density=0.3)


@functools.lru_cache(maxsize=None)
def restated_beams(w, ts, with_len=False, skip_drops=False):
    """Per block, per sequence: ``fused_beam_search``'s final beam; w = ts = 0: the unfused search."""
    model = ctc_model()
    out = []
    for T, scale, logp, lens in ctc_blocks():
        frames = [int(lens[s]) if with_len else T for s in range(logp.size(0))]
        out.append([fused_beam_search(logp[s, :Ts].double().numpy().reshape(Ts, CTC_V), model, w, ts, skip_drops_frame=skip_drops)
                    for s, Ts in enumerate(frames)])
    return out


def comparable_ranks(final, nbest=NBEST):
    """rescore_cases.comparable_ranks on the keys: the ranks whose consecutive key gaps up to rank k + 1 all exceed BEAM_MARGIN."""
    ok = []
    for k in range(min(nbest, len(final))):
        gaps = [final[j][3] - final[j + 1][3] for j in range(min(k + 1, len(final) - 1))]
        if all(g > K.BEAM_MARGIN for g in gaps):
            ok.append(k)
        else:
            break
    return ok


# ---------------------------------------------------------------------------------------------------------------------------
# the AED step
# ---------------------------------------------------------------------------------------------------------------------------
def aed_step(model, prev_state, parent, last, local, s, R_prev, w, ts):
    """One eec_lm_fusion_step over dictionary states: prev_state [n][R_prev] (tuples, or DEAD), parent / last [n][R] (parent None: r),
    local [n][R][V] fp32 numpy.  Returns (out, state [n][R])."""
    n, R, V = local.shape
    out = local.copy()
    state = [[model.start()] * R for _ in range(n)]
    for i in range(n):
        for r in range(R):
            st = model.start()
            if s > 0:
                p = r if parent is None else int(parent[i][r])
                c = int(last[i][r])
                if 0 <= p < R_prev and 0 <= c < V:
                    st = increment(model, prev_state[i][p], c, 1.0, 0.0)[1]
            state[i][r] = st
            for v in range(V):
                inc = increment(model, st, v, w, ts)[0] if not (w == 0 and ts == 0) else F32(0.0)
                if local[i, r, v] != NEG and inc != 0:
                    out[i, r, v] = F32(local[i, r, v] + inc)
    return out, state
