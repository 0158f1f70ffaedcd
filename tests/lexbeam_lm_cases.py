"""Test side of the lexicon-constrained CTC beam search WITH a back-off n-gram word model (include/eec.h, csrc/ctc_lexbeam.hip):
the model's score, which the statement of the search (tests/lexbeam_statement.py) adds at every word end and as the end-of-sentence
term, in plain Python with ``np.float32`` operations in the written order.  The model is a dict ``{word tuple: (logp, backoff)}``
of np.float32 values and the LM state is the word history itself.  Also here: a generator of random models over a lexicon, a writer
of ARPA text, a reader of the packed n-gram image by its documented layout, and the emissions of the LM cases."""
import numpy as np

from lexbeam_cases import F32, load_fixture, log_softmax

LM_MAGIC = 0x4E434545
BOS, EOS, UNK = "<s>", "</s>", "<unk>"


# ----------------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------------
def model_order(lm):
    return max(len(g) for g in lm)


def lm_names(lm, hist, lm_words):
    """The word history as the model sees it: <s> in front when the model has it, a word the model lacks as <unk>."""
    names = tuple(lm_words[w] if (lm_words[w],) in lm else UNK for w in hist)
    return ((BOS,) if (BOS,) in lm else ()) + names


def lm_score(lm, order, names, v, stats=None):
    """log10 p(v | names) by back-off, fp32 additions in the walk's order: from the longest context of at most order - 1 words
    down, a context that is an n-gram of the model and does not continue with ``v`` adds its back-off; a context the model lacks
    adds nothing.  The empty context always finds v's unigram."""
    ctx = names[max(len(names) - (order - 1), 0):] if order > 1 else ()
    acc, depth = F32(0.0), 0
    while True:
        hit = lm.get(ctx + (v,))
        if hit is not None:
            acc = F32(acc + hit[0])
            break
        assert ctx, f"{v!r} has no unigram"
        if ctx in lm:
            acc = F32(acc + lm[ctx][1])
            depth += 1
        ctx = ctx[1:]
    if stats is not None:
        stats.setdefault("depth", {}).setdefault(depth, 0)
        stats["depth"][depth] += 1
        stats.setdefault("pairs", set()).add((names[max(len(names) - (order - 1), 0):] if order > 1 else (), v))
    return acc


def textbook(lm, ctx, v):
    """The same probability by the textbook recursion in float64: p(v | ctx) = p(ctx v) if present, else bo(ctx) + p(v | ctx[1:]),
    with bo = 0 for a context the model lacks."""
    hit = lm.get(ctx + (v,))
    if hit is not None:
        return float(hit[0])
    assert ctx
    return (float(lm[ctx][1]) if ctx in lm else 0.0) + textbook(lm, ctx[1:], v)


# ----------------------------------------------------------------------------------------------------------------------------
# generated models
# ----------------------------------------------------------------------------------------------------------------------------
def random_model(seed, words, order, leave_out=0.1, grid=False, positive_backoff=False, unk=True, bos=True, eos=True):
    """A model of ``order`` over ``words`` (strings; duplicates count once).  About ``leave_out`` of them get no unigram (they score
    as <unk>).  Orders above 1 are sparse: an n-gram is a present (n-1)-gram context plus a random word -- or, for a
    few, a word its suffix continues with --, so the model is prefix-closed and NOT suffix-closed: most suffix links skip an order.  Among the bigram contexts one has 300 children (more
    than 256), two have exactly 1 and two exactly 2.  ``grid``: all values are multiples of 1/8; ``positive_backoff``: a third of the
    back-offs are positive.  Returns (model dict, favoured, disfavoured): word-string sequences the model scores well (chains of its
    own high-order n-grams, their logp raised to -1/8) and badly (its rarest words, and words it lacks, in an order it has never
    seen)."""
    rng = np.random.default_rng(seed)
    uniq = list(dict.fromkeys(words))
    kept = [w for w in uniq if rng.random() >= leave_out]
    kept_set = set(kept)
    left = [w for w in uniq if w not in kept_set]

    def val(lo, hi):
        x = rng.uniform(lo, hi)
        return F32(round(x * 8) / 8 if grid else x)

    def back(n):
        if n == order:
            return F32(0.0)
        b = val(-1.0, -0.125)
        return F32(-b) if positive_backoff and rng.random() < 1 / 3 else b

    lm = {(w,): (val(-6.0, -1.0), back(1)) for w in kept}
    if unk:
        lm[(UNK,)] = (val(-3.0, -2.0), back(1))
    if bos:
        lm[(BOS,)] = (F32(-99.0), back(1))
    if eos:
        lm[(EOS,)] = (val(-5.0, -4.0), F32(0.0))
    tails = kept + ([UNK] if unk else []) + ([EOS] if eos else [])
    favoured, kids = [], {}
    for n in range(2, order + 1):
        ctxs = [g for g in lm if len(g) == n - 1 and g[-1] != EOS]
        ctxs = [ctxs[i] for i in rng.permutation(len(ctxs))[:160 if n == 2 else 220]]
        if n == 2 and bos:
            ctxs = [(BOS,)] + [g for g in ctxs if g != (BOS,)]
        degrees = ([300, 1, 1, 2, 2] if n == 2 else [1, 2]) + [int(d) for d in rng.integers(3, 10, size=len(ctxs))]
        for ctx, deg in zip(ctxs, degrees):
            for i in rng.permutation(len(tails))[:min(deg, len(tails))]:
                lm[ctx + (tails[i],)] = (val(-2.0, -0.25), back(n))
                kids.setdefault(ctx, []).append(tails[i])
            for w in kids.get(ctx[1:], [])[:2] if n > 2 and deg > 2 else []:  # ... and a few whose suffix is an n-gram as well
                if ctx + (w,) not in lm:
                    lm[ctx + (w,)] = (val(-2.0, -0.25), back(n))
                    kids.setdefault(ctx, []).append(w)
    if eos and order >= 2:  # a third of the words like to end a sentence, the others pay </s>'s rare unigram
        for w in kept:
            if rng.random() < 1 / 3:
                lm[(w, EOS)] = (val(-1.0, -0.125), F32(0.0))
    # favoured chains: follow the model from a random bigram as long as a continuation exists
    plain = [g for g in lm if len(g) >= 2 and not {BOS, EOS, UNK} & set(g)]
    plain.sort(key=lambda g: (-len(g), g))
    for g in plain[:60] + [plain[i] for i in rng.permutation(len(plain))[:60]]:
        lm[g] = (F32(-0.125), lm[g][1])
        for k in range(2, len(g)):
            lm[g[:k]] = (F32(-0.125), lm[g[:k]][1])
        favoured.append(list(g))
    if not plain:
        best = sorted(kept, key=lambda w: -float(lm[(w,)][0]))[:20]
        favoured = [[best[int(i)] for i in rng.integers(len(best), size=3)] for _ in range(30)]
    rare = sorted(kept, key=lambda w: float(lm[(w,)][0]))[:40] + left[:40]
    disfavoured = [[rare[int(i)] for i in rng.integers(len(rare), size=3)] for _ in range(60)]
    return lm, favoured, disfavoured


def write_arpa(path, lm, order=None):
    """``lm`` as ARPA text.  A value is written as the shortest decimal that reads back to the same double, so its fp32 bits
    survive; fields are separated by tabs or by spaces in turn, and a zero back-off is left out of every other line that has one."""
    order = model_order(lm) if order is None else order
    by_n = [[g for g in lm if len(g) == n] for n in range(1, order + 1)]
    with open(path, "w", encoding="utf-8") as f:
        f.write("generated\n\n\\data\\\n")
        for n, grams in enumerate(by_n, 1):
            f.write(f"ngram {n}={len(grams)}\n")
        for n, grams in enumerate(by_n, 1):
            f.write(f"\n\\{n}-grams:\n")
            for k, g in enumerate(grams):
                lp, bo = lm[g]
                sep = "\t" if k % 2 else " "
                fields = [repr(float(lp)), *g]
                if n < order and (float(bo) != 0.0 or k % 4 < 2):
                    fields.append(repr(float(bo)))
                f.write(sep.join(fields) + "\n")
        f.write("\n\\end\\\n")


# ----------------------------------------------------------------------------------------------------------------------------
# the packed image, read by the layout include/eec.h documents
# ----------------------------------------------------------------------------------------------------------------------------
def read_lm_image(image):
    """``image``: int32 array.  Returns (header dict, {n-gram as LM word ids: (node, logp bits, backoff bits)}, {n-gram: its suffix
    link's n-gram}, word_map list) after checking every structural promise of the layout: section offsets, ascending edge words,
    the breadth-first numbering (the child of edge k is node k + 1, the unigram of word v is node v + 1, depths never decrease),
    the first node of the full order, and that every suffix link is the LONGEST proper suffix that is a node."""
    image = np.asarray(image, dtype=np.int32)
    (magic, order, n_nodes, n_edges, W, lex_words, bos_node, eos_word, top_begin, off_begin, off_eword, off_logp, off_backoff, off_suffix,
     off_map, total) = (int(v) for v in image[:16])
    assert magic == LM_MAGIC and 1 <= order <= 5 and n_edges == n_nodes - 1 and W >= 1 and lex_words >= 1
    assert off_begin == 16 and off_eword == off_begin + n_nodes + 1 and off_logp == off_eword + n_edges
    assert off_backoff == off_logp + n_nodes and off_suffix == off_backoff + n_nodes and off_map == off_suffix + n_nodes
    assert total == off_map + lex_words and total <= len(image)
    assert 0 <= bos_node <= W and -1 <= eos_word < W
    begin = image[off_begin:off_begin + n_nodes + 1].tolist()
    eword = image[off_eword:off_eword + n_edges].tolist()
    logp, backoff = image[off_logp:off_logp + n_nodes].tolist(), image[off_backoff:off_backoff + n_nodes].tolist()  # bit patterns
    suffix = image[off_suffix:off_suffix + n_nodes].tolist()
    word_map = image[off_map:off_map + lex_words].tolist()
    assert begin[0] == 0 and begin[-1] == n_edges and all(a <= b for a, b in zip(begin, begin[1:]))
    assert eword[:W] == list(range(W)) and begin[1] == W, "the unigram of LM word v is node v + 1"
    assert logp[0] == 0 and backoff[0] == 0 and suffix[0] == 0
    assert all(0 <= v < W for v in word_map)
    gram = {0: ()}
    for n in range(n_nodes):  # breadth-first: a node's n-gram is known before its children are visited
        edges = eword[begin[n]:begin[n + 1]]
        assert edges == sorted(set(edges)) and all(0 <= v < W for v in edges)
        assert len(gram[n]) < order or not edges, "a node of the full order has no children"
        for k in range(begin[n], begin[n + 1]):
            assert k + 1 not in gram
            gram[k + 1] = gram[n] + (eword[k],)
    assert len(gram) == n_nodes
    depth = [len(gram[n]) for n in range(n_nodes)]
    assert depth == sorted(depth) and all((depth[n] == order) == (n >= top_begin) for n in range(n_nodes))
    node_of = {g: n for n, g in gram.items()}
    links = {}
    for n in range(1, n_nodes):
        g = gram[n]
        want = next(g[k:] for k in range(1, len(g) + 1) if g[k:] in node_of)
        assert suffix[n] == node_of[want], (g, want, gram[suffix[n]])
        links[g] = want
    grams = {g: (n, logp[n], backoff[n]) for n, g in gram.items() if n}
    head = dict(order=order, n_nodes=n_nodes, n_lm_words=W, lex_words=lex_words, bos_node=bos_node, eos_word=eos_word, top_begin=top_begin)
    return head, grams, links, word_map


def bits(x):
    return int(np.float32(x).view(np.int32))


# ----------------------------------------------------------------------------------------------------------------------------
# emissions whose label paths spell word sequences the model favours or disfavours
# ----------------------------------------------------------------------------------------------------------------------------
def sequence_path(rng, sequences, spelling_of, twins, T, blank, sil=-1):
    """As ``lexbeam_cases.label_path``, but the words are those of sequences drawn from ``sequences`` (lists of word strings), in
    their order.  Returns (path, rival): ``rival[t]`` is -1, or the label a rival word -- one of ``twins[len(spelling)]``, spelled
    with as many tokens, none doubled -- has in frame t where the path's word has another."""
    path, rival = [], []
    while True:
        words = sequences[int(rng.integers(len(sequences)))]
        full = False
        for name in words:
            sp = spelling_of[name]
            other = twins.get(len(sp), [sp])
            other = other[int(rng.integers(len(other)))]
            if any(a == b for a, b in zip(sp, sp[1:])) or (path and path[-1] in (sp[0], other[0])):
                other = sp
            word, shadow = [], []
            for c, d in zip(sp, other):
                if word and word[-1] == c:  # a doubled token needs a blank between
                    word.append(blank)
                    shadow.append(-1)
                run = int(rng.integers(1, 3))
                word += [c] * run
                shadow += [d if d != c else -1] * run
                if rng.random() < 0.3:
                    run = int(rng.integers(1, 3))
                    word += [blank] * run
                    shadow += [-1] * run
            if sil >= 0 and rng.random() < 0.5:
                run = int(rng.integers(1, 3))
                word += [sil] * run
                shadow += [-1] * run
            if path and path[-1] == word[0]:
                word, shadow = [blank] + word, [-1] + shadow
            if len(path) + len(word) > T:
                full = True
                break
            path += word
            rival += shadow
        if full:
            break
    return path + [blank] * (T - len(path)), rival + [-1] * (T - len(rival))


def lm_emissions(seed, favoured, disfavoured, words, spellings, n, T, V, blank=0, sil=-1, peaks=(0.0, 2.0, 4.0, 8.0), gap=0.5):
    """[n, T, V] float32: log-softmax of unit noise plus ``peaks[s % len(peaks)]`` on a label path; the paths of even quadruples
    of sequences spell favoured word sequences, those of odd ones disfavoured ones.  Every word of a path has a rival of the same
    token count whose labels get the peak less ``gap``: two word histories stay close, and the model decides between them."""
    rng = np.random.default_rng(seed)
    spelling_of, twins = {}, {}
    for w, sp in zip(words, spellings):
        if w not in spelling_of:
            spelling_of[w] = sp
            if all(a != b for a, b in zip(sp, sp[1:])):
                twins.setdefault(len(sp), []).append(sp)
    x = rng.standard_normal((n, T, V))
    for s in range(n):
        path, rival = sequence_path(rng, favoured if (s // len(peaks)) % 2 == 0 else disfavoured, spelling_of, twins, T, blank, sil)
        peak = peaks[s % len(peaks)]
        x[s, np.arange(T), path] += peak
        at = [t for t in range(T) if rival[t] >= 0]
        x[s, at, [rival[t] for t in at]] += max(peak - gap, 0.0)
    return log_softmax(x)


MAIN_PEAKS = (0.0, 4.0, 6.0, 8.0)


def main_lm_case(order=3, seed=40, peaks=MAIN_PEAKS, gap=0.0):
    """The LM suite's largest case: 70 sequences of 64 frames over the fixture's lexicon with sil, ragged lengths that include 1,
    T', 0 and T' + 1, and a generated model of ``order``; every word of a label path has a rival with the same peak.  The seed is
    chosen so that the statement meets the conditions tests/test_gpu_lexbeam_lm.py states, at lm_weight 1.0 and at 3.23.
    (emission, em_len, spellings, words, model)"""
    _, words, spellings = load_fixture()
    lm, favoured, disfavoured = random_model(seed, words, order)
    em = lm_emissions(seed + 1, favoured, disfavoured, words, spellings, 70, 64, 256, 0, 126, peaks=peaks, gap=gap)
    rng = np.random.default_rng(seed + 2)
    em_len = rng.integers(20, 65, size=70).astype(np.int32)
    em_len[[0, 1, 2, 3, 4, 5]] = [64, 1, 0, 65, -2, 64]
    em_len[40:] = 64
    return em, em_len, spellings, words, lm
