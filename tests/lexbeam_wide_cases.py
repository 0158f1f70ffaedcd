"""Test-side statement of the lexicon-constrained CTC beam search for WIDE beams (include/eec.h, csrc/ctc_lexbeam_wide.hip,
eec_ctc_lexbeam_wide_decode): the general statement -- model optional, smear table optional, ``log_add`` a flag -- with the candidate
id ``(2 * c + w) * 64 + i``, unique for beams up to 64.  It is the body of ``lexbeam_logadd_cases.decode`` with that one line
changed; tries, hypotheses, emissions, models, smear tables, ``log_add`` and ``fold`` are those modules' own, imported.  At beams of
16 or less the id orders candidates exactly as the narrow id does, so this statement must return what the four narrow statements
return (tests/test_host_lexbeam_wide.py holds it to that).  ``stats`` also record what the GPU cases must not be vacuous about: the
largest merge group, the hypotheses alive after each frame, and the ties that only an id with a rank of 16 or more decides."""
import numpy as np

import lexbeam_cases as L  # noqa: F401
import lexbeam_lm_cases as M  # noqa: F401
import lexbeam_logadd_cases as A  # noqa: F401
import lexbeam_smear_cases as S  # noqa: F401
from lexbeam_cases import F32, NEG_INF, Hyp, Trie  # noqa: F401
from lexbeam_lm_cases import EOS, UNK, lm_names, lm_score, model_order
from lexbeam_logadd_cases import fold

MAX_BEAM = 64
NARROW = 16


def decode(e, trie, beam=10, nbest=1, word_score=0.0, sil_score=0.0, beam_threshold=50.0, length=None, lm=None, lm_weight=0.0,
           lm_words=None, stats=None, smax=None, log_add=False):
    """The statement for ONE sequence, as ``lexbeam_logadd_cases.decode`` (same arguments, same return; ``log_add`` defaults to the
    Viterbi merge here).  ``stats``, when a dict, also receives ``max_group`` (members of the largest merge group), ``alive`` (a list:
    the hypotheses in the beam after each frame, appended per frame) and ``wide_ties`` (ties decided by the id -- inside a merge, or
    between neighbours of the new beam's order, the first candidate cut off included -- where at least one of the two has a beam rank
    i >= 16: only the wide id can decide those)."""
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
            lm_words = S.default_words(trie)
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
                                    acc = F32(acc - pmax)
                                s_end = F32(s_end + F32(lm_weight * acc))
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
        done = [(h.score, r, h) for r, h in enumerate(hyps) if h.node == 0]
        if lm is not None and (EOS,) in lm:
            done = [(F32(s + F32(lm_weight * lm_score(lm, order, lm_names(lm, h.hist, lm_words), EOS, stats))), r, h) for s, r, h in done]
            done = sorted(done, key=lambda d: (-float(d[0]), d[1]))
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
    """``stats``: None, or a list that receives one stats dict per sequence."""
    out = []
    for s in range(len(em)):
        st = None if stats is None else {}
        out.append(decode(em[s], trie, length=None if em_len is None else em_len[s], stats=st, **kw))
        if stats is not None:
            stats.append(st)
    return out


def wide_share(stats):
    """Of all frames a batch decoded, the share after which the beam held more than 16 hypotheses."""
    alive = [n for st in stats for n in st.get("alive", [])]
    return sum(1 for n in alive if n > NARROW) / max(len(alive), 1)


# ----------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_lexbeam_wide.py with a beam over 16, shared with the host test that keeps them from being vacuous
# ----------------------------------------------------------------------------------------------------------------------------
INF = float("inf")
WIDE_CASES = [
    # lexicon, n_seq, T', beam, nbest, options
    ("fixture+sil", 6, 48, 64, 64, dict(beam_threshold=INF)),
    ("fixture", 3, 257, 40, 40, dict(word_score=-4.0)),
    ("fixture+sil", 70, 7, 17, 1, dict(beam_threshold=2.0, word_score=1.5, sil_score=-0.5)),
    ("wide", 3, 12, 64, 64, dict(sil_score=-0.5, word_score=1.5, beam_threshold=INF)),
    ("wide", 3, 64, 33, 33, dict()),
    ("prefix", 70, 16, 64, 10, dict()),
    ("one", 1, 1, 64, 1, dict()),
    ("one", 3, 7, 64, 64, dict()),
]
# tie_emissions at (n, T'): the sizes the issue names.  Both give id-decided ties with a rank of 16 or more (the host test asserts
# it), so the uniform block keeps the length tie_emissions gives it
TIE_CASES = [("prefix", 70, 16), ("fixture+sil", 3, 64)]
TIE_BEAMS = (17, 64)


def lexicon(name):
    """(spellings, V, sil or None, words)"""
    if name.startswith("fixture"):
        _, words, spellings = L.load_fixture()
        return spellings, 256, (126 if name == "fixture+sil" else None), words
    spellings, V, sil = {"one": (L.ONE_WORD, 40, None), "prefix": (L.PREFIX_DOUBLED, 32, None), "wide": (L.wide_lexicon(), 256, 126)}[name]
    return spellings, V, sil, [f"w{i}" for i in range(len(spellings))]


# under beam_threshold = 2.0 the default peaks (up to 8) leave the beam of 17 full in only 45 % of the frames; flat emissions fill it
PEAKS = {("fixture+sil", 70, 7): (0.0, 1.0)}


def wide_case_inputs(name, n, T):
    """(emission, em_len or None) of a WIDE_CASES row: ragged lengths with 0, 1, T' and T' + 1 where there are 70 sequences."""
    spellings, V, sil, _ = lexicon(name)
    em = L.emissions(100 + n + T, spellings, n, T, V, 0, -1 if sil is None else sil, peaks=PEAKS.get((name, n, T), (0.0, 2.0, 4.0, 8.0)))
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)
        em_len[:4] = [0, 1, T, T + 1]
    return em, em_len


def tie_case_inputs(name, n, T):
    spellings, V, sil, _ = lexicon(name)
    return L.tie_emissions(7, spellings, n, T, V, 0, -1 if sil is None else sil)
