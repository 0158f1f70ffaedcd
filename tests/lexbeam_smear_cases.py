"""Test side of LM look-ahead by max trie smearing in the lexicon-constrained CTC beam search (include/eec.h,
csrc/ctc_lexbeam.hip): the smear table itself (every node carries the maximum, over the words at or below it, of the model's score
for the word from the start state) in plain Python with ``np.float32`` operations in the written order, a reader of the packed
table by its documented layout, and the cases of the pruning and telescoping tests.  The two child rules that smearing changes are
in the statement of the search (tests/lexbeam_statement.py, ``smax=``)."""
import numpy as np

import lexbeam_lm_cases as M
from lexbeam_cases import F32, MAGIC, NEG_INF
from lexbeam_lm_cases import BOS, EOS, UNK, lm_names, lm_score, model_order

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
