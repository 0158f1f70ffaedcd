"""THE test-side statement of the lexicon-constrained CTC beam search (include/eec.h, csrc/ctc_lexbeam.hip,
csrc/ctc_lexbeam_wide.hip, csrc/eec_lexbeam.h): the one function under tests/ that walks the frames, in plain Python with
``np.float32`` operations in the written order and tuples for word histories.  The n-gram model is optional, the smear table is
optional and ``log_add`` is a flag, so every entry -- plain, model, smear, log-add, wide -- is judged by this one body.  Nothing in the
arithmetic is a reduction, and ``log_add`` is a stated sequence of exactly rounded fp32 operations, so comparisons against the
statement are exact: scores bit for bit, words, tokens and timesteps as integers.  Tries, hypotheses, emissions, models, smear tables,
``log_add`` and ``fold`` are the feature modules' own (lexbeam_cases, lexbeam_lm_cases, lexbeam_smear_cases, lexbeam_logadd_cases,
lexbeam_wide_cases), imported; none of them imports this module.  The candidate id is ``(2 * c + w) * 64 + i``, unique for beams up
to 64; at beams of 16 or less it orders candidates exactly as the narrow kernels' ``(2 * c + w) * 16 + i`` does.
tests/golden/lexbeam_statement_pins.json pins what the statement returns (tests/test_host_lexbeam_wide.py)."""
import numpy as np

from lexbeam_cases import F32, NEG_INF, Hyp
from lexbeam_lm_cases import EOS, UNK, lm_names, lm_score, model_order
from lexbeam_logadd_cases import fold
from lexbeam_smear_cases import default_words
from lexbeam_wide_cases import MAX_BEAM, NARROW


def decode(e, trie, beam=10, nbest=1, word_score=0.0, sil_score=0.0, beam_threshold=50.0, length=None, lm=None, lm_weight=0.0,
           lm_words=None, stats=None, smax=None, log_add=False):
    """The statement for ONE sequence: ``e`` [T', V] float32 log-probs, ``length`` frames of it (None: all).  Returns the list
    of at most ``nbest`` complete hypotheses, best first, each ``(words, tokens, timesteps, score)``: word indices, the collapsed
    label sequence, the first frame of each label, the np.float32 score.  An empty list: no complete hypothesis, a length outside
    [1, T'], or a frame that left no candidate.

    ``lm``: None or the model dict of lexbeam_lm_cases, ``lm_words[w]`` the string of lexicon word w (None: ``"w<index>"``, the names
    ``TokenTrie.from_spellings`` gives).  ``smax``: None, or the table of ``lexbeam_smear_cases.smear`` for this trie and model --
    then, with ``pmax = smax[node]`` of the hypothesis (0 at the root),
        child, in-word (c -> y)    (score + e[c]) + lm_weight * (smax[y] - pmax)
        child, word end (y: wd)    ((score + e[c]) + word_score) + lm_weight * (acc - pmax)
    the difference rounded, the product rounded on its own, then added.  ``log_add``: True -- the survivor of a merge group scores
    the fold of its members -- or False: the Viterbi merge.

    ``stats``, when a dict, receives: from ``lm_score`` the back-off ``depth`` counts and the (context, word) ``pairs`` asked for;
    ``eos_reordered`` (the </s> term changed the order of the complete hypotheses); ``max_candidates`` (the most candidates any frame
    had after merging, before pruning); from ``fold`` ``merges`` (pairs folded) and ``equal_merges`` (of those, pairs whose
    accumulators were equal: d = 0); ``max_alive`` (the most hypotheses any frame left after the threshold); ``max_group`` (members
    of the largest merge group); ``alive`` (a list: the hypotheses in the beam after each frame, appended per frame); ``wide_ties``
    (ties decided by the id -- inside a merge, or between neighbours of the new beam's order, the first candidate cut off included
    -- where at least one of the two has a beam rank i >= 16: only the 64-wide id can decide those)."""
    e = np.asarray(e)
    assert e.dtype == np.float32 and 1 <= beam <= MAX_BEAM
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
            groups = {}  # (node, tok, pb, hist) -> [(score, id, parent, word)]

            def offer(node, tok, pb, hist, score, c, w, i, word=-1):
                if not score > NEG_INF:  # -inf and NaN are dropped, before merging
                    return
                groups.setdefault((node, tok, pb, hist), []).append((score, (2 * c + w) * 64 + i, hyps[i], word))

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

            if not groups:
                if stats is not None:
                    stats.setdefault("alive", []).append(0)
                return []
            cands = {}  # key -> [score, id, parent, word]
            for key, members in groups.items():
                members.sort(key=lambda m: m[1])
                if log_add:
                    k, merged = fold(members, stats)
                else:  # the higher score survives, the lower id on equal scores
                    k = min(range(len(members)), key=lambda j: (-float(members[j][0]), members[j][1]))
                    merged = members[k][0]
                cands[key] = [merged, members[k][1], members[k][2], members[k][3]]
                if stats is not None:
                    stats["max_group"] = max(stats.get("max_group", 0), len(members))
                    for j, mem in enumerate(members):
                        if j != k and mem[0] == members[k][0] and max(mem[1] % 64, members[k][1] % 64) >= NARROW:
                            stats["wide_ties"] = stats.get("wide_ties", 0) + 1
            if stats is not None:
                stats["max_candidates"] = max(stats.get("max_candidates", 0), len(cands))
            best = max(v[0] for v in cands.values())
            keep = list(cands.items())
            if np.isfinite(F32(beam_threshold)):
                thr = F32(best - F32(beam_threshold))
                keep = [kv for kv in keep if kv[1][0] >= thr]
            keep.sort(key=lambda kv: (-float(kv[1][0]), kv[1][1]))
            hyps = [Hyp(k[0], k[1], k[2], k[3], v[0], v[2], k[1], v[3]) for k, v in keep[:beam]]
            if stats is not None:
                stats["max_alive"] = max(stats.get("max_alive", 0), len(keep))
                stats.setdefault("alive", []).append(len(hyps))
                for (_, x), (_, y) in zip(keep[:beam], keep[1:beam + 1]):
                    if x[0] == y[0] and max(x[1] % 64, y[1] % 64) >= NARROW:
                        stats["wide_ties"] = stats.get("wide_ties", 0) + 1
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


def decode_batch(em, trie, em_len=None, stats=None, **kw):
    """``stats``: None, a dict that every sequence adds to, or a list that receives one stats dict per sequence."""
    out = []
    for s in range(len(em)):
        st = {} if isinstance(stats, list) else stats
        out.append(decode(em[s], trie, length=None if em_len is None else em_len[s], stats=st, **kw))
        if isinstance(stats, list):
            stats.append(st)
    return out
