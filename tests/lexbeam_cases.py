"""Test side of the lexicon-constrained CTC beam search (include/eec.h, csrc/ctc_lexbeam.hip): the trie and the hypothesis that the
plain-Python statement of the search (tests/lexbeam_statement.py) walks, a reader of the packed trie image's documented layout, the
lexica and the generators of the test cases.  The search adds ``np.float32`` scores in the written order -- nothing in it is a
reduction or a transcendental --, so comparisons against the statement are exact: scores bit for bit, words, tokens and timesteps
as integers."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "bpe256_lexicon_slice.json")
MAGIC = 0x54434545
F32 = np.float32
NEG_INF = F32(-np.inf)


# ----------------------------------------------------------------------------------------------------------------------------
# the lexicon as a trie (node 0 = root; numbering is private to the statement: only words, labels and scores are compared)
# ----------------------------------------------------------------------------------------------------------------------------
class Trie:
    def __init__(self, spellings, V, blank=0, sil=None):
        self.V, self.blank, self.sil = V, blank, -1 if sil is None else sil
        self.kids = [{}]      # node -> {token: child}
        self.word = [-1]      # node -> the FIRST word in file order that ends there
        self.shadowed = 0
        for w, sp in enumerate(spellings):
            assert len(sp) > 0 and all(0 <= t < V and t != blank and t != self.sil for t in sp)
            at = 0
            for t in sp:
                if t not in self.kids[at]:
                    self.kids[at][t] = len(self.kids)
                    self.kids.append({})
                    self.word.append(-1)
                at = self.kids[at][t]
            if self.word[at] < 0:
                self.word[at] = w
            else:
                self.shadowed += 1
        # per node: child tokens ascending (an index array for one vector addition per hypothesis), the children, their words
        self.ktok = [np.array(sorted(k), dtype=np.int64) for k in self.kids]
        self.knode = [[k[t] for t in sorted(k)] for k in self.kids]

    @property
    def n_nodes(self):
        return len(self.kids)


class Hyp:
    __slots__ = ("node", "tok", "pb", "hist", "score", "parent", "label", "word")

    def __init__(self, node, tok, pb, hist, score, parent=None, label=-1, word=-1):
        self.node, self.tok, self.pb, self.hist, self.score = node, tok, pb, hist, score
        self.parent, self.label, self.word = parent, label, word  # the back-pointer: previous hypothesis, this frame's label, completed word


# ----------------------------------------------------------------------------------------------------------------------------
# the packed image, read by the layout include/eec.h documents
# ----------------------------------------------------------------------------------------------------------------------------
def read_image(image):
    """``image``: int32 array.  Returns (header dict, {spelling tuple: word index}) after checking every structural promise of the
    layout: section offsets, ascending child tokens, the breadth-first numbering (the child of edge k is node k + 1)."""
    image = np.asarray(image, dtype=np.int32)
    magic, n_nodes, n_edges, V, blank, sil, off_begin, off_tok, off_word, total, n_words, n_shadowed = (int(v) for v in image[:12])
    assert magic == MAGIC and n_edges == n_nodes - 1 and n_nodes >= 1 and all(int(v) == 0 for v in image[12:16])
    assert off_begin == 16 and off_tok == off_begin + n_nodes + 1 and off_word == off_tok + (n_edges + 3) // 4
    assert total == off_word + n_nodes and total <= len(image)
    begin = image[off_begin:off_begin + n_nodes + 1].tolist()
    tok = image[off_tok:off_word].view(np.uint8)[:n_edges].tolist()
    word_of = image[off_word:off_word + n_nodes].tolist()
    assert begin[0] == 0 and begin[-1] == n_edges and all(a <= b for a, b in zip(begin, begin[1:]))
    spelling = {0: ()}
    words = {}
    for n in range(n_nodes):  # breadth-first: a node's spelling is known before its children are visited
        edges = tok[begin[n]:begin[n + 1]]
        assert edges == sorted(set(edges)) and all(0 <= c < V and c != blank and c != sil for c in edges)
        for k in range(begin[n], begin[n + 1]):
            assert k + 1 not in spelling
            spelling[k + 1] = spelling[n] + (tok[k],)
        if word_of[n] >= 0:
            assert n > 0 and 0 <= word_of[n] < n_words
            words[spelling[n]] = word_of[n]
        else:
            assert n == 0 or begin[n + 1] > begin[n], "a leaf ends a word"
    assert len(spelling) == n_nodes
    head = dict(n_nodes=n_nodes, n_edges=n_edges, V=V, blank=blank, sil=sil, n_words=n_words, n_shadowed=n_shadowed)
    return head, words


def first_words(spellings):
    """{spelling: the first word index with it}: what a packed image must hold."""
    out = {}
    for w, sp in enumerate(spellings):
        out.setdefault(tuple(sp), w)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# lexica
# ----------------------------------------------------------------------------------------------------------------------------
def load_fixture():
    """(tokens [256], words, spellings as id lists): the 256 tokens of librispeech-bpe-256.tok and every 45th line of
    librispeech-bpe-256.lex."""
    with open(FIXTURE, encoding="utf-8") as f:
        fx = json.load(f)
    ids = {t: i for i, t in enumerate(fx["tokens"])}
    words = [w for w, _ in fx["lexicon"]]
    spellings = [[ids[t] for t in sp.split()] for _, sp in fx["lexicon"]]
    return fx["tokens"], words, spellings


ONE_WORD = [[5, 9, 5]]                                      # V = 40
# V = 32: a word that is a prefix of another, a doubled token inside a spelling (the shape of "a ar a a f"), a duplicate
PREFIX_DOUBLED = [[3], [3, 4], [3, 4, 3, 3, 7], [4], [4, 4], [3, 4], [7, 3], [9, 9, 9]]


def wide_lexicon(V=256, blank=0, sil=126, seed=3):
    """A root with 150 children, one node with 80 children (both above 64: the child range spans waves), two-level tails."""
    rng = np.random.default_rng(seed)
    toks = [t for t in range(V) if t not in (blank, sil)]
    first = rng.permutation(toks)[:150].tolist()
    out = [[c] for c in first[:100]]                                  # one-token words
    hub = first[120]
    second = rng.permutation(toks)[:80].tolist()
    out += [[hub, c] for c in second]                                 # the 80-children node
    out += [[hub, c, d] for c in second[:20] for d in rng.permutation(toks)[:3].tolist()]
    out += [[c, int(rng.choice(toks))] for c in first[50:150]]        # words whose prefix is a word (50..99) or not (100..149)
    return out


@functools.lru_cache(maxsize=None)
def lexicon(name):
    """(spellings, V, sil or None, words) of ``fixture``, ``fixture+sil``, ``one``, ``prefix`` or ``wide``"""
    if name.startswith("fixture"):
        _, words, spellings = load_fixture()
        return spellings, 256, (126 if name == "fixture+sil" else None), words
    spellings, V, sil = {"one": (ONE_WORD, 40, None), "prefix": (PREFIX_DOUBLED, 32, None), "wide": (wide_lexicon(), 256, 126)}[name]
    return spellings, V, sil, [f"w{i}" for i in range(len(spellings))]


# ----------------------------------------------------------------------------------------------------------------------------
# emissions
# ----------------------------------------------------------------------------------------------------------------------------
def log_softmax(x):
    x = x.astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def label_path(rng, spellings, T, blank, sil=-1):
    """T frame labels that spell randomly drawn words with random repeats and blanks (a blank between equal neighbours); a word
    that no longer fits is left out and the rest is blank, so a path ends at a word boundary."""
    path = []
    for _ in range(T):
        word = []
        sp = spellings[int(rng.integers(len(spellings)))]
        for c in sp:
            if (word or path) and (word or path)[-1] == c:
                word.append(blank)
            word += [c] * int(rng.integers(1, 3))
            if rng.random() < 0.3:
                word += [blank] * int(rng.integers(1, 3))
        if sil >= 0 and rng.random() < 0.5:
            word += [sil] * int(rng.integers(1, 3))
        if len(path) + len(word) > T:
            break
        path += word
    return path + [blank] * (T - len(path))


def emissions(seed, spellings, n, T, V, blank=0, sil=-1, peaks=(0.0, 2.0, 4.0, 8.0), quantum=None):
    """[n, T, V] float32: log-softmax of unit noise plus ``peaks[s % len(peaks)]`` on a label path.  ``quantum``: the log-probs are
    rounded to its multiples afterwards, so that equal scores occur."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, T, V))
    for s in range(n):
        path = label_path(rng, spellings, T, blank, sil)
        x[s, np.arange(T), path] += peaks[s % len(peaks)]
    out = log_softmax(x)
    if quantum:
        out = (np.round(out / quantum) * quantum).astype(np.float32)
    return out


def tie_emissions(seed, spellings, n, T, V, blank=0, sil=-1):
    """Log-probs rounded to multiples of 0.25, with a block of uniform frames in the middle: equal scores occur in every frame."""
    out = emissions(seed, spellings, n, T, V, blank, sil, peaks=(1.0, 2.0), quantum=0.25)
    out[:, T // 3: T // 3 + max(T // 4, 1), :] = np.float32(-np.round(np.log(V) * 4) / 4)
    return out


def main_case():
    """The suite's largest fixture case: 70 sequences of 64 frames over the fixture's lexicon, peaks 0 / 2 / 4 / 8 in turn, ragged
    lengths that include 1, T' and values outside [1, T'].  (emission, em_len, spellings, words)"""
    tokens, words, spellings = load_fixture()
    em = emissions(11, spellings, 70, 64, 256, 0, 126)
    rng = np.random.default_rng(12)
    em_len = rng.integers(20, 65, size=70).astype(np.int32)
    em_len[[0, 1, 2, 3, 4, 5]] = [64, 1, 0, 65, -2, 64]
    em_len[40:] = 64
    return em, em_len, spellings, words
