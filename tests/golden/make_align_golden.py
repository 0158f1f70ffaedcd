"""Generates tests/golden/ctc_align.npz by running the REFERENCE's own ``BeamInference.get_trellis`` / ``backtrack``
(util/beam_infer.py:129-191) on the CPU, unmodified.

Build-container only (needs /root/reference).  The module imports ``torchaudio.models.decoder`` for decoders this fixture never
touches; it is stubbed in ``sys.modules`` and the object is created without running ``__init__`` (which would build them), with
an ``args`` that carries ``device="cpu"``.  The fixture is data only: per case of tests/align_cases.py the tokens, the blank
id, the trellis and the path triples the reference returned, the fp64 decision margin along the path (from the restatement in
align_cases.py, on the same inputs) and -- for the two small cases -- the emission; the peaky emissions are regenerated from
their seeds and only their fp64 sums are kept.

    python tests/golden/make_align_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import align_cases as A  # noqa: E402


def reference_aligner():
    ta, tam, tad = (types.ModuleType(n) for n in ("torchaudio", "torchaudio.models", "torchaudio.models.decoder"))
    tad.ctc_decoder = tad.cuda_ctc_decoder = None
    tam.decoder, ta.models = tad, tam
    sys.modules.update({"torchaudio": ta, "torchaudio.models": tam, "torchaudio.models.decoder": tad})
    sys.path.insert(0, "/root/reference")
    from util.beam_infer import BeamInference
    inf = object.__new__(BeamInference)
    inf.args = types.SimpleNamespace(device="cpu")
    return inf


def main():
    inf = reference_aligner()
    out = {}
    for name, (em, tok, blank) in A.fixture_cases().items():
        tokens = torch.tensor(tok, dtype=torch.long)
        trellis = inf.get_trellis(em, tokens, blank_id=blank)
        path = inf.backtrack(trellis, em, tokens, blank_id=blank)
        assert path[0].token_index == 0 and path[-1].time_index == em.size(0) - 1, name
        _, _, margin, ok = A.align_ref(em.numpy(), tok, blank)
        assert ok, name
        out[f"{name}/tok"] = np.asarray(tok, dtype=np.int64)
        out[f"{name}/blank"] = np.int64(blank)
        out[f"{name}/trellis"] = trellis.numpy().astype(np.float32)
        out[f"{name}/path"] = np.asarray([(p.token_index, p.time_index, p.score) for p in path], dtype=np.float64)
        out[f"{name}/margin"] = np.float64(margin)
        if em.size(1) == 256:
            out[f"{name}/em_sum"] = np.float64(em.double().sum())
        else:
            out[f"{name}/em"] = em.numpy()
    path = os.path.join(HERE, "ctc_align.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(A.fixture_cases())} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
