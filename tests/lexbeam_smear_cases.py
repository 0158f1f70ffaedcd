"""Test-side statement of the lexicon-constrained CTC beam search with an n-gram word model AND LM look-ahead by max trie smearing
(include/eec.h, csrc/ctc_lexbeam.hip): the search of tests/lexbeam_lm_cases.py again, in plain Python with ``np.float32``
operations in the written order, with the two child rules that smearing changes.  Also here: the smear table itself (every node
carries the maximum, over the words at or below it, of the model's score for the word from the start state), a reader of the packed
table by its documented layout, and the cases of the pruning and telescoping tests.  With ``smax=None`` ``decode`` is the statement
of lexbeam_lm_cases, which stays the judge of the unsmeared search."""
import numpy as np

import lexbeam_lm_cases as M
from lexbeam_cases import F32, MAGIC, NEG_INF, Hyp, Trie  # noqa: F401
from lexbeam_lm_cases import BOS, EOS, UNK, lm_names, lm_score, model_order  # noqa: F401

SMEAR_MAGIC = 0x53434545  # "EECS"
SMEAR_HEADER = 4


# ----------------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------------
def default_words(trie):
    return [f"w{w}" for w in range(max(trie.word) + 1)]


def word_score_from_start(lm, lm_words, w):
    """u(w): ``acc`` of the back-off walk for lm_word(w) from the start state (<s>'s unigram, or the empty n-gram)."""
    v = lm_words[w] if (lm_words[w],) in lm else UNK
    return lm_score(lm, model_order(lm), lm_names(lm, (), lm_words), v)


def smear(trie, lm, lm_words=None):
    """``smax`` as a list of np.float32 over the STATEMENT's node numbers: ``smax[0] = 0``; for n >= 1 the maximum of u(w) over the
    words that end at n or below it.  Only the word a node ends -- the first in file order with that spelling -- counts.  Children
    have higher numbers than their parent, so one descending sweep fills it."""
    lm_words = default_words(trie) if lm_words is None else lm_words
    smax = [NEG_INF] * trie.n_nodes
    for n in range(trie.n_nodes - 1, 0, -1):
        if trie.word[n] >= 0:
            smax[n] = max(smax[n], word_score_from_start(lm, lm_words, trie.word[n]))
        for y in trie.kids[n].values():
            assert y > n
            smax[n] = max(smax[n], smax[y])
        assert np.isfinite(smax[n]), "every node but the root ends a word or has children"
    smax[0] = F32(0.0)
    return smax


def brute_force_smear(spellings, lm, lm_words=None):
    """{spelling prefix: maximum of u(w) over the first words whose spelling starts with it}: the table without a trie."""
    lm_words = [f"w{w}" for w in range(len(spellings))] if lm_words is None else lm_words
    first, out = {}, {}
    for w, sp in enumerate(spellings):
        first.setdefault(tuple(sp), w)
    for sp, w in first.items():
        u = word_score_from_start(lm, lm_words, w)
        for k in range(1, len(sp) + 1):
            out[sp[:k]] = max(out.get(sp[:k], NEG_INF), u)
    return out


def statement_spellings(trie):
    """The spelling (token tuple) of every node of the statement's trie."""
    out = {0: ()}
    for n in range(trie.n_nodes):
        for t, y in trie.kids[n].items():
            out[y] = out[n] + (t,)
    return [out[n] for n in range(trie.n_nodes)]


def image_spellings(image):
    """The spelling of every node of a packed trie image, by the layout include/eec.h documents (lexbeam_cases.read_image checks it)."""
    image = np.asarray(image, dtype=np.int32)
    assert int(image[0]) == MAGIC
    n_nodes, n_edges, off_begin, off_tok = int(image[1]), int(image[2]), int(image[6]), int(image[7])
    begin = image[off_begin:off_begin + n_nodes + 1].tolist()
    tok = image[off_tok:].view(np.uint8)[:n_edges].tolist()
    out = [()] * n_nodes
    for n in range(n_nodes):
        for k in range(begin[n], begin[n + 1]):
            out[k + 1] = out[n] + (tok[k],)
    return out


def read_smear_table(table):
    """``table``: int32 array.  Returns (n_nodes, n_words, the values' bit patterns as a list) after checking the layout: header[4]
    = {magic "EECS", the trie's n_nodes, the lexicon's word count, 0}, then n_nodes fp32, padded to a multiple of 8 bytes."""
    table = np.asarray(table, dtype=np.int32)
    magic, n_nodes, n_words, zero = (int(v) for v in table[:SMEAR_HEADER])
    assert magic == SMEAR_MAGIC and n_nodes >= 1 and n_words >= 1 and zero == 0
    assert len(table) == (SMEAR_HEADER + n_nodes + 1) // 2 * 2, "8-byte granules, nothing more"
    return n_nodes, n_words, table[SMEAR_HEADER:SMEAR_HEADER + n_nodes].tolist()


def table_in_image_order(trie, smax, image):
    """The statement's table as the bit patterns the packed table must hold: ``smax`` re-indexed by the image's node numbers."""
    node_of = {sp: n for n, sp in enumerate(statement_spellings(trie))}
    return [M.bits(smax[node_of[sp]]) for sp in image_spellings(image)]


# ----------------------------------------------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------------------------------------------
def decode(e, trie, beam=10, nbest=1, word_score=0.0, sil_score=0.0, beam_threshold=50.0, length=None, lm=None, lm_weight=0.0,
           lm_words=None, stats=None, smax=None):
    """The statement for ONE sequence, as ``lexbeam_lm_cases.decode``; ``smax``: None, or the table of ``smear`` for this trie and
    model -- then, with ``pmax = smax[node]`` of the hypothesis (0 at the root),
        child, in-word (c -> y)    (score + e[c]) + lm_weight * (smax[y] - pmax)
        child, word end (y: wd)    ((score + e[c]) + word_score) + lm_weight * (acc - pmax)
    the difference rounded, the product rounded on its own, then added.  ``stats["max_candidates"]``: the largest number of
    candidates (after merging, before pruning) any frame had."""
    e = np.asarray(e)
    assert e.dtype == np.float32
    assert smax is None or lm is not None, "smearing needs a model"
    T = e.shape[0] if length is None else int(length)
    if T < 1 or T > e.shape[0]:
        return []
    blank, sil = trie.blank, trie.sil
    word_score, sil_score, lm_weight = F32(word_score), F32(sil_score), F32(lm_weight)
    if lm is not None:
        order = model_order(lm)
        if lm_words is None:
            lm_words = default_words(trie)
    hyps = [Hyp(0, -1, True, (), F32(0.0))]
    with np.errstate(all="ignore"):
        for t in range(T):
            row = e[t]
            cands = {}  # (node, tok, pb, hist) -> [score, id, parent, word]

            def offer(node, tok, pb, hist, score, c, w, i, word=-1):
                if not score > NEG_INF:  # -inf and NaN are dropped
                    return
                cid = (2 * c + w) * 16 + i
                key = (node, tok, pb, hist)
                old = cands.get(key)
                if old is None or score > old[0] or (score == old[0] and cid < old[1]):
                    cands[key] = [score, cid, hyps[i], word]

            for i, h in enumerate(hyps):
                offer(h.node, blank, True, h.hist, h.score + row[blank], blank, 0, i)
                if not h.pb and h.tok >= 0:
                    s = h.score + row[h.tok]
                    if h.tok == sil:
                        s = s + sil_score
                    offer(h.node, h.tok, False, h.hist, s, h.tok, 0, i)
                ktok = trie.ktok[h.node]
                if len(ktok):
                    inword = h.score + row[ktok]       # fp32 vector: element k is score + e[c_k]
                    ended = inword + word_score        # (score + e[c]) + word_score
                    names = None
                    pmax = None if smax is None else F32(smax[h.node])
                    for c, y, s_in, s_end in zip(ktok.tolist(), trie.knode[h.node], inword, ended):
                        if c == h.tok and not h.pb:
                            continue
                        if trie.kids[y]:
                            if smax is not None:
                                s_in = F32(s_in + F32(lm_weight * F32(F32(smax[y]) - pmax)))
                            offer(y, c, False, h.hist, s_in, c, 0, i)
                        wd = trie.word[y]
                        if wd >= 0:
                            if lm is not None:
                                if names is None:
                                    names = lm_names(lm, h.hist, lm_words)
                                v = lm_words[wd] if (lm_words[wd],) in lm else UNK
                                acc = lm_score(lm, order, names, v, stats)
                                if smax is not None:
                                    acc = F32(acc - pmax)  # the advance payment is taken back: the difference is rounded
                                s_end = F32(s_end + F32(lm_weight * acc))  # the product is rounded on its own, then added
                            offer(0, c, False, h.hist + (wd,), s_end, c, 1, i, wd)
                if h.node == 0 and sil >= 0 and (sil != h.tok or h.pb):
                    offer(0, sil, False, h.hist, (h.score + row[sil]) + sil_score, sil, 0, i)

            if not cands:
                return []
            if stats is not None:
                stats["max_candidates"] = max(stats.get("max_candidates", 0), len(cands))
            best = max(v[0] for v in cands.values())
            keep = list(cands.items())
            if np.isfinite(F32(beam_threshold)):
                thr = F32(best - F32(beam_threshold))
                keep = [kv for kv in keep if kv[1][0] >= thr]
            keep.sort(key=lambda kv: (-float(kv[1][0]), kv[1][1]))
            hyps = [Hyp(k[0], k[1], k[2], k[3], v[0], v[2], k[1], v[3]) for k, v in keep[:beam]]
            if not hyps:
                return []
        # the complete hypotheses in rank order; with a model that has </s>, its term and a new order: (final score descending, rank)
        done = [(h.score, r, h) for r, h in enumerate(hyps) if h.node == 0]
        if lm is not None and (EOS,) in lm:
            done = [(F32(s + F32(lm_weight * lm_score(lm, order, lm_names(lm, h.hist, lm_words), EOS, stats))), r, h) for s, r, h in done]
            ranked = sorted(done, key=lambda d: (-float(d[0]), d[1]))
            if stats is not None and [d[1] for d in ranked] != [d[1] for d in done]:
                stats["eos_reordered"] = stats.get("eos_reordered", 0) + 1
            done = ranked
    out = []
    for score, _, h in done[:nbest]:
        labels, words, at = [], [], h
        while at.parent is not None:
            labels.append(at.label)
            if at.word >= 0:
                words.append(at.word)
            at = at.parent
        labels.reverse()
        words.reverse()
        assert tuple(words) == h.hist and len(labels) == T
        tokens, steps = [], []
        for t, c in enumerate(labels):
            if c != blank and (t == 0 or labels[t - 1] != c):
                tokens.append(c)
                steps.append(t)
        out.append((words, tokens, steps, score))
    return out


def decode_batch(em, trie, em_len=None, **kw):
    return [decode(em[s], trie, length=None if em_len is None else em_len[s], **kw) for s in range(len(em))]


# ----------------------------------------------------------------------------------------------------------------------------
# the pruning and telescoping cases
# ----------------------------------------------------------------------------------------------------------------------------
PRUNE_V = 8
A, B_, C_, D = 1, 2, 3, 4  # the labels of "a", "b", "c", "d"; 0 is the blank


def pruning_case(extra_abd=False):
    """The lexicon {ab, cd} (``extra_abd``: and abd) over 8 labels, unigrams -1 and -5 (abd: -1), and two frames: a at -1.0, c at
    -0.875, everything else at -8; then b and d at -1.0, everything else at -8.  At beam 1 and lm_weight 1 the unsmeared search
    keeps c (acoustically ahead by 1/8) and ends with cd at -6.875; the smeared one is charged -5 for c and -1 for a in the first
    frame, keeps a and ends with ab at -3.0.  With abd below ab the in-word and the word-end candidate of b tie at -3.0: the lower
    id (in-word) takes the single slot and the sequence ends incomplete.  (spellings, words, model, emission [2, 8])"""
    spellings = [[A, B_], [C_, D]] + ([[A, B_, D]] if extra_abd else [])
    words = ["ab", "cd"] + (["abd"] if extra_abd else [])
    lm = {("ab",): (F32(-1.0), F32(0.0)), ("cd",): (F32(-5.0), F32(0.0))}
    if extra_abd:
        lm[("abd",)] = (F32(-1.0), F32(0.0))
    em = np.full((2, PRUNE_V), -8.0, dtype=np.float32)
    em[0, A], em[0, C_] = -1.0, -0.875
    em[1, B_] = em[1, D] = -1.0
    return spellings, words, lm, em


TELE_WORDS = ["ab", "cd", "a", "abd"]
TELE_SPELLINGS = [[A, B_], [C_, D], [A], [A, B_, D]]


def telescoping_case(seed, T, n=1):
    """The 4-word lexicon {ab, cd, a, abd} over 8 labels with a bigram model that has <s> and </s>; every emission and model value
    is a multiple of 1/8, so every fp32 sum is exact.  (spellings, words, model, emission [n, T, 8])"""
    rng = np.random.default_rng(seed)
    g = lambda lo, hi: F32(int(rng.integers(lo * 8, hi * 8 + 1)) / 8)  # noqa: E731
    lm = {(w,): (g(-6, -1), g(-1, 0)) for w in TELE_WORDS}
    lm[(BOS,)] = (F32(-99.0), g(-1, 0))
    lm[(EOS,)] = (g(-5, -4), F32(0.0))
    heads = TELE_WORDS + [BOS]
    tails = TELE_WORDS + [EOS]
    for _ in range(8):
        a, b = heads[int(rng.integers(len(heads)))], tails[int(rng.integers(len(tails)))]
        lm[(a, b)] = (g(-2, 0), F32(0.0))
    em = (rng.integers(-64, 0, size=(n, T, PRUNE_V)) / 8).astype(np.float32)
    return TELE_SPELLINGS, TELE_WORDS, lm, em


def as_set(hyps):
    """A hypothesis list as a set of (words, tokens, timesteps, score bits): ranks, and with them candidate ids, are left out."""
    return {(tuple(w), tuple(tk), tuple(st), M.bits(sc)) for w, tk, st, sc in hyps}
