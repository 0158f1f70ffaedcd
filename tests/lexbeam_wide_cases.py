"""Test side of the lexicon-constrained CTC beam search for WIDE beams (include/eec.h, csrc/ctc_lexbeam_wide.hip,
eec_ctc_lexbeam_wide_decode): the beam limits, the cases of tests/test_gpu_lexbeam_wide.py with a beam over 16 and what the
statistics of the statement (tests/lexbeam_statement.py: the largest merge group, the hypotheses alive after each frame, the ties
that only an id with a rank of 16 or more decides) say about them, so that the GPU cases are not vacuous."""
import numpy as np

import lexbeam_cases as L

MAX_BEAM = 64
NARROW = 16


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


# under beam_threshold = 2.0 the default peaks (up to 8) leave the beam of 17 full in only 45 % of the frames; flat emissions fill it
PEAKS = {("fixture+sil", 70, 7): (0.0, 1.0)}


def wide_case_inputs(name, n, T):
    """(emission, em_len or None) of a WIDE_CASES row: ragged lengths with 0, 1, T' and T' + 1 where there are 70 sequences."""
    spellings, V, sil, _ = L.lexicon(name)
    em = L.emissions(100 + n + T, spellings, n, T, V, 0, -1 if sil is None else sil, peaks=PEAKS.get((name, n, T), (0.0, 2.0, 4.0, 8.0)))
    em_len = None
    if n == 70:
        em_len = np.random.default_rng(T).integers(0, T + 2, size=n).astype(np.int32)
        em_len[:4] = [0, 1, T, T + 1]
    return em, em_len


def tie_case_inputs(name, n, T):
    spellings, V, sil, _ = L.lexicon(name)
    return L.tie_emissions(7, spellings, n, T, V, 0, -1 if sil is None else sil)
