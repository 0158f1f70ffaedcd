"""Same-box timing of the lexicon-constrained CTC beam search (``eec_ctc_lexbeam_decode``, csrc/ctc_lexbeam.hip) on a synthetic
trie of the real lexicon's measured size.  librispeech-bpe-256.lex (not part of this repository) has 89 114 words, 162 621 trie
nodes, root degree 109, largest other degree 103, longest spelling 43, and never uses tokens 0, 1, 2, 126, 127; the spellings
here are drawn from a seed to land on that size (the counts reached are printed).  Emissions: T' = 256, V = 256, log-softmax of
noise plus a peak of 0 / 2 / 4 / 8 on a path that spells lexicon words (tests/lexbeam_cases.py), beam 10, sil 126.

    python tools/lexbeam_time.py [--reps 20] [--seqs 1,64,384] [--out profiles/lexbeam_time.json]          JSON lines

* launch: device time by events around one call on prepared device buffers, median of ``--reps`` after three warm-up calls, and
  per call in a train of 10 calls (the launch gap taken out).
* yardstick: ``eec_ctc_beam_decode`` (the lexicon-free prefix beam search, unchanged by this tool's subject) on the same
  emissions, in the same process, measured the same way.  It is another algorithm with other outputs: the ratio says what the
  lexicon costs a caller who switches decoders, nothing else.

    python tools/lexbeam_time.py --lm [--parent-record FILE ...] [--out profiles/lexbeam_lm_time.json]

* ``--lm``: the search with a model (``eec_ctc_lexbeam_lm_decode``) against the search without one, same process, same emissions
  (384 x 256, beam 10), lm_weight 1.  The model is synthetic and built as arrays, not as text: one unigram per lexicon word plus
  ``<unk>``, ``<s>``, ``</s>``, and ``--bigrams`` / ``--trigrams`` (2 000 000 each: millions, as a pruned LibriSpeech 3-gram cut down
  to the lexicon has) distinct random n-grams, a trigram always over a bigram that is there.  The emissions' paths spell random
  words, so most word ends miss the state's edges and back off to the unigram: the walk is at its longest.
* ``--parent-record``: records this tool wrote (``--out``) when run from a checkout of the parent commit on the same box; the
  model-free time of that run joins the record with its ratio to this run's.

    python tools/lexbeam_time.py --lm --smear [--parent-record FILE ...] [--out profiles/lexbeam_smear_time.json]

* ``--smear``: also the search with LM look-ahead (``eec_ctc_lexbeam_lm_smear_decode``, max trie smearing) on the same emissions
  with the same model, against the unsmeared LM search of the same process; the host time of building the table
  (``eec_ctc_trie_smear``) is recorded too.  ``--parent-record`` then takes the records of the parent commit's ``--lm`` run: its
  model-free and its LM time join with their ratios to this run's.

    python tools/lexbeam_time.py --log-add [--lm [--smear]] [--out profiles/lexbeam_logadd_time.json]

* ``--log-add``: the search with log-add merging (``eec_ctc_lexbeam_logadd_decode``) against the Viterbi search of the same mode --
  without a model, with ``--lm`` the model, with ``--lm --smear`` the model and smearing -- in the same process on the same
  emissions (384 x 256, beam 10), each measured twice in turn (the spread between the two blocks of one entry is the noise to read
  the ratio against).  The emissions are synthetic: how often hypotheses meet, and so how often ``log_add`` runs, is theirs.

    python tools/lexbeam_time.py --wide [--lm --smear] [--log-add] [--parent-record FILE ...] [--out profiles/lexbeam_wide_time.json]

* ``--wide``: the wide-beam kernel (``eec_ctc_lexbeam_wide_decode``, csrc/ctc_lexbeam_wide.hip) against the narrow entries, all in one
  process on the same 384 x 256 emissions: narrow at beams 10 and 16, wide at 16, 32 and 64, model-free; with ``--lm --smear`` the same
  five legs under the model with smearing, with ``--log-add`` the same under log-add merging of every mode measured.  Each record
  carries the ratio wide@16 / narrow@16, the cost per doubling of the beam (wide@32 / wide@16, wide@64 / wide@32), and whether
  wide@16 returned narrow@16's outputs byte for byte.  ``--parent-record``: records of ``lexbeam_time.py`` (the ``launch`` record of
  384 sequences) run from the parent commit on the same box; the ratio of this run's narrow@10 to it shows the narrow entries did
  not move.

    python tools/lexbeam_time.py --parent-lib PATH [--rounds 11] [--out profiles/lexbeam_one_set_time.json]

* ``--parent-lib``: a second libeec.so, built from another commit, loaded beside this tree's (a library of another ABI version is
  refused).  Every search kernel is run out of both on the standing batch (384 x 256, V 256): the narrow kernel at ``--beam`` and the
  wide kernel at beams 16, 32 and 64, each without a model, with the model, with the model and smearing, and each of those with
  log-add merging, through the entry a caller of that mode reaches.  The two libraries take turns (parent, new, parent, new, ...),
  ``--rounds`` trains each of 5 calls (narrow), 2 (wide at 16) or 1 (wide at 32 and 64), device events on the current stream after
  two warm-up calls per library.  A leg's time mark: this tree's median may exceed the parent's by no more than the parent's own
  min .. max range of that leg.  The outputs of the two libraries on the same inputs are compared byte for byte.  The exit status
  is 1 when a mark is missed or outputs differ (the record is written first).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from early_exit_transformer_amd import capi  # noqa: E402
from early_exit_transformer_amd.lexicon import NGramLM, TokenTrie  # noqa: E402
import lexbeam_cases as L  # noqa: E402  (tests/: the emission generator)

UNUSED = (0, 1, 2, 126, 127)


def synthetic_spellings(n_words=89114, seed=1, mean_len=2.3, skew=1.0):
    """Spellings over the 251 used tokens: 109 word-initial tokens, continuation tokens drawn from a skewed choice of 103, Poisson lengths
    with a few up to 43, duplicates dropped.  The skew and the mean length are set so that the trie has about 164 000 nodes."""
    rng = np.random.default_rng(seed)
    toks = np.array([t for t in range(256) if t not in UNUSED])
    first = rng.permutation(toks)[:109]
    cont = rng.permutation(toks)[:103]
    p_first = 1.0 / np.arange(1, 110) ** 0.9
    p_cont = 1.0 / np.arange(1, 104) ** skew
    draw = 2 * n_words  # duplicates are dropped (the real lexicon has none): draw more than needed
    lens = np.clip(rng.poisson(mean_len, size=draw) + 1, 1, 43)
    lens[:8] = [43, 30, 25, 21, 20, 19, 18, 17]
    heads = rng.choice(first, size=draw, p=p_first / p_first.sum())
    tails = rng.choice(cont, size=int(lens.sum()), p=p_cont / p_cont.sum())
    out, seen, at = [], set(), 0
    for n, h in zip(lens.tolist(), heads.tolist()):
        sp = (h,) + tuple(tails[at:at + n - 1].tolist())
        at += n - 1
        if sp not in seen and len(out) < n_words:
            seen.add(sp)
            out.append(list(sp))
    assert len(out) == n_words
    return out


def event_ms(fn, reps, per=1):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}


def prepared_calls(trie, em, beam, nbest, dev):
    """The bare C calls of both decoders on buffers that are already on the device."""
    lib = capi.load()
    n, T, V = em.shape
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    words, wc, toks, tc, ts, nh = i32(n, nbest, T), i32(n, nbest), i32(n, nbest, T), i32(n, nbest), i32(n, nbest, T), i32(n)
    sc = torch.empty((n, nbest), dtype=torch.float32, device=dev)
    ws_bytes = lib.eec_ctc_lexbeam_workspace_bytes(n, T, beam)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    image = trie.on(dev)
    ytok, ycnt, ysc = i32(n, T), i32(n), torch.empty((n,), dtype=torch.float32, device=dev)
    yws = torch.empty(lib.eec_ctc_beam_workspace_bytes(n, T), dtype=torch.uint8, device=dev)
    keep = (em, words, wc, toks, tc, ts, nh, sc, ws, image, ytok, ycnt, ysc, yws)

    def lexbeam():
        capi.check(lib.eec_ctc_lexbeam_decode(em.data_ptr(), n, T, V, None, image.data_ptr(), trie.blank, trie.sil, beam, nbest, 0.0, 0.0, 50.0, T,
                                              words.data_ptr(), wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(),
                                              nh.data_ptr(), ws.data_ptr(), ws_bytes, capi.stream_ptr(dev)), "eec_ctc_lexbeam_decode")
        return keep

    def yardstick():
        capi.check(lib.eec_ctc_beam_decode(em.data_ptr(), n, T, V, trie.blank, beam, 0.95, yws.data_ptr(), ytok.data_ptr(), ycnt.data_ptr(),
                                           ysc.data_ptr(), capi.stream_ptr(dev)), "eec_ctc_beam_decode")
        return keep
    return lexbeam, yardstick, nh


def synthetic_model(n_words, n_bigrams, n_trigrams, seed=2):
    """``NGramLM`` of order 3 over LM words 0 .. n_words + 2 (the lexicon's words in file order, then <unk>, <s>, </s>)."""
    rng = np.random.default_rng(seed)
    W = n_words + 3
    unk, bos, eos = n_words, n_words + 1, n_words + 2
    # contexts are skewed (a few words start many bigrams), successors are not; </s> starts nothing
    ctx = np.minimum((rng.random(2 * n_bigrams) ** 3 * (W - 1)).astype(np.int64), W - 2)
    key2 = np.unique(ctx * W + rng.integers(0, W, size=2 * n_bigrams))
    key2 = np.sort(rng.permutation(key2)[:n_bigrams])
    bi = np.stack([key2 // W, key2 % W], axis=1)
    bi = bi[bi[:, 1] != bos]
    over = bi[bi[:, 1] != eos]
    key3 = np.unique(rng.integers(0, len(over), size=2 * n_trigrams) * W + rng.integers(0, W, size=2 * n_trigrams))
    key3 = np.sort(rng.permutation(key3)[:n_trigrams])
    tri = np.concatenate([over[key3 // W], (key3 % W)[:, None]], axis=1)
    tri = tri[tri[:, 2] != bos]
    words = [np.arange(W, dtype=np.int32)[:, None], bi.astype(np.int32), tri.astype(np.int32)]
    logp = [rng.uniform(-6, -1, size=len(w)).astype(np.float32) for w in words]
    backoff = [rng.uniform(-1, 0, size=len(w)).astype(np.float32) for w in words[:2]] + [np.zeros(len(tri), dtype=np.float32)]
    return NGramLM(words, logp, backoff, np.arange(n_words, dtype=np.int32), bos, eos, unk)


def lm_leg(args, trie, spellings, dev, records):
    lib = capi.load()
    lm = synthetic_model(len(spellings), args.bigrams, args.trigrams)
    n, T, beam = 384, args.frames, args.beam
    em = torch.from_numpy(L.emissions(3, spellings, n, T, 256, 0, 126)).to(dev)
    free, _, nh = prepared_calls(trie, em, beam, 1, dev)
    keep = free()
    em_, words, wc, toks, tc, ts, nh, sc, ws, image = keep[:10]
    lm_image = lm.on(dev)

    def with_lm():
        capi.check(lib.eec_ctc_lexbeam_lm_decode(em.data_ptr(), n, T, 256, None, image.data_ptr(), trie.blank, trie.sil, beam, 1, 0.0, 0.0, 50.0, T,
                                                 words.data_ptr(), wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(),
                                                 nh.data_ptr(), ws.data_ptr(), ws.numel(), capi.stream_ptr(dev), lm_image.data_ptr(), 1.0),
                   "eec_ctc_lexbeam_lm_decode")
    calls = [("lm_free", free), ("with_lm", with_lm), ("lm_free_again", free)]
    smear_rec = {}
    if args.smear:
        t0 = time.perf_counter()
        table = lm.smear(trie)
        smear_rec = {"smear_table_bytes": table._image.numel(), "smear_table_host_build_s": round(time.perf_counter() - t0, 3)}
        smear_image = table.on(dev)

        def with_smear():
            capi.check(lib.eec_ctc_lexbeam_lm_smear_decode(em.data_ptr(), n, T, 256, None, image.data_ptr(), trie.blank, trie.sil, beam, 1, 0.0, 0.0,
                                                           50.0, T, words.data_ptr(), wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(),
                                                           sc.data_ptr(), nh.data_ptr(), ws.data_ptr(), ws.numel(), capi.stream_ptr(dev),
                                                           lm_image.data_ptr(), 1.0, smear_image.data_ptr()), "eec_ctc_lexbeam_lm_smear_decode")
        calls = [("lm_free", free), ("with_lm", with_lm), ("with_smear", with_smear), ("with_lm_again", with_lm), ("with_smear_again", with_smear),
                 ("lm_free_again", free)]
    rec = {"what": "smear" if args.smear else "lm", "n_seq": n, "frames": T, "beam": beam, "lm_weight": 1.0, "order": lm.order, "n_grams": lm.n_grams, "lm_nodes": lm.n_nodes,
           "lm_image_bytes": lm._image.numel(), "trie_image_bytes": trie._image.numel(), **smear_rec}
    for name, call in calls:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        rec[name + "_train_of_10_ms_per_call"] = event_ms(call, max(args.reps // 2, 5), per=10)
        if name in ("with_lm", "with_smear"):
            rec["sequences_with_a_hypothesis_" + name] = int((nh > 0).sum())
    rec["ratio_with_lm_over_lm_free"] = round(rec["with_lm_train_of_10_ms_per_call"]["median"] / rec["lm_free_train_of_10_ms_per_call"]["median"], 3)
    med = lambda *names: statistics.median([rec[k + "_train_of_10_ms_per_call"]["median"] for k in names])  # noqa: E731
    if args.smear:
        rec["ratio_with_smear_over_with_lm"] = round(med("with_smear", "with_smear_again") / med("with_lm", "with_lm_again"), 4)
        free_p, lm_p = [], []
        for path in args.parent_record or []:
            with open(path) as f:
                for r in json.load(f):
                    if r.get("what") == "lm" and r.get("n_seq") == n:
                        free_p += [r["lm_free_train_of_10_ms_per_call"]["median"], r["lm_free_again_train_of_10_ms_per_call"]["median"]]
                        lm_p.append(r["with_lm_train_of_10_ms_per_call"]["median"])
        if free_p:
            rec["parent_commit_lm_free_train_of_10_ms_per_call_medians"] = free_p
            rec["parent_commit_with_lm_train_of_10_ms_per_call_medians"] = lm_p
            rec["ratio_lm_free_over_parent_commit"] = round(med("lm_free", "lm_free_again") / statistics.median(free_p), 4)
            rec["ratio_with_lm_over_parent_commit"] = round(med("with_lm", "with_lm_again") / statistics.median(lm_p), 4)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        return
    parents = []
    for path in args.parent_record or []:
        with open(path) as f:
            parents += [r["lexbeam_train_of_10_ms_per_call"]["median"] for r in json.load(f) if r.get("what") == "launch" and r.get("n_seq") == n]
    if parents:
        mine = statistics.median([rec["lm_free_train_of_10_ms_per_call"]["median"], rec["lm_free_again_train_of_10_ms_per_call"]["median"]])
        rec["parent_commit_lm_free_train_of_10_ms_per_call_medians"] = parents
        rec["ratio_lm_free_over_parent_commit"] = round(mine / statistics.median(parents), 4)
    records.append(rec)
    print(json.dumps(rec), flush=True)


def logadd_leg(args, trie, spellings, dev, records):
    lib = capi.load()
    n, T, beam = 384, args.frames, args.beam
    em = torch.from_numpy(L.emissions(3, spellings, n, T, 256, 0, 126)).to(dev)
    free, _, nh = prepared_calls(trie, em, beam, 1, dev)
    words, wc, toks, tc, ts, nh, sc, ws, image = free()[1:10]
    lm = synthetic_model(len(spellings), args.bigrams, args.trigrams) if args.lm else None
    lm_ptr = lm.on(dev).data_ptr() if args.lm else None
    smear_ptr = lm.smear(trie).on(dev).data_ptr() if args.smear else None
    common = (em.data_ptr(), n, T, 256, None, image.data_ptr(), trie.blank, trie.sil, beam, 1, 0.0, 0.0, 50.0, T, words.data_ptr(), wc.data_ptr(),
              toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(), nh.data_ptr(), ws.data_ptr(), ws.numel(), capi.stream_ptr(dev))
    if args.smear:
        name, tail = "eec_ctc_lexbeam_lm_smear_decode", (lm_ptr, 1.0, smear_ptr)
    elif args.lm:
        name, tail = "eec_ctc_lexbeam_lm_decode", (lm_ptr, 1.0)
    else:
        name, tail = "eec_ctc_lexbeam_decode", ()

    def viterbi():
        capi.check(getattr(lib, name)(*common, *tail), name)

    def log_add():
        capi.check(lib.eec_ctc_lexbeam_logadd_decode(*common, lm_ptr, 1.0, smear_ptr), "eec_ctc_lexbeam_logadd_decode")
    rec = {"what": "log_add", "mode": "smear" if args.smear else "lm" if args.lm else "lm_free", "viterbi_entry": name, "n_seq": n, "frames": T,
           "beam": beam, "lm_weight": 1.0 if args.lm else None}
    best = {}
    for key, call in (("viterbi", viterbi), ("log_add", log_add), ("viterbi_again", viterbi), ("log_add_again", log_add)):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        rec[key + "_train_of_10_ms_per_call"] = event_ms(call, max(args.reps // 2, 5), per=10)
        rec["sequences_with_a_hypothesis_" + key] = int((nh > 0).sum())
        best[key] = (words[:, 0].cpu(), wc[:, 0].cpu())
    same = (best["viterbi"][1] == best["log_add"][1]) & (best["viterbi"][0] == best["log_add"][0]).all(dim=1)
    rec["sequences_whose_best_words_differ"] = int((~same).sum())
    med = lambda *names: statistics.median([rec[k + "_train_of_10_ms_per_call"]["median"] for k in names])  # noqa: E731
    rec["ratio_log_add_over_viterbi"] = round(med("log_add", "log_add_again") / med("viterbi", "viterbi_again"), 4)
    rec["spread_viterbi_blocks"] = round(rec["viterbi_again_train_of_10_ms_per_call"]["median"] / rec["viterbi_train_of_10_ms_per_call"]["median"], 4)
    rec["spread_log_add_blocks"] = round(rec["log_add_again_train_of_10_ms_per_call"]["median"] / rec["log_add_train_of_10_ms_per_call"]["median"], 4)
    records.append(rec)
    print(json.dumps(rec), flush=True)


def wide_leg(args, trie, spellings, dev, records):
    lib = capi.load()
    n, T = 384, args.frames
    em = torch.from_numpy(L.emissions(3, spellings, n, T, 256, 0, 126)).to(dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    words, wc, toks, tc, ts, nh = i32(n, 1, T), i32(n, 1), i32(n, 1, T), i32(n, 1), i32(n, 1, T), i32(n)
    sc = torch.empty((n, 1), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.eec_ctc_lexbeam_wide_workspace_bytes(n, T, 64), dtype=torch.uint8, device=dev)
    image = trie.on(dev)
    outputs = (words, wc, toks, tc, ts, sc, nh)
    modes = [("lm_free", None, None)]
    if args.lm:
        lm = synthetic_model(len(spellings), args.bigrams, args.trigrams)
        modes.append(("smear", lm.on(dev).data_ptr(), lm.smear(trie).on(dev).data_ptr()))
    parents = []
    for path in args.parent_record or []:
        with open(path) as f:
            parents += [r["lexbeam_train_of_10_ms_per_call"]["median"] for r in json.load(f) if r.get("what") == "launch" and r.get("n_seq") == n]
    for mode, lm_ptr, smear_ptr in modes:
        for log_add in ([0, 1] if args.log_add else [0]):
            def call(kind, beam):
                common = (em.data_ptr(), n, T, 256, None, image.data_ptr(), trie.blank, trie.sil, beam, 1, 0.0, 0.0, 50.0, T, words.data_ptr(),
                          wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(), nh.data_ptr(), ws.data_ptr(), ws.numel(),
                          capi.stream_ptr(dev))
                if kind == "wide":
                    capi.check(lib.eec_ctc_lexbeam_wide_decode(*common, lm_ptr, 1.0, smear_ptr, log_add), "eec_ctc_lexbeam_wide_decode")
                elif log_add:
                    capi.check(lib.eec_ctc_lexbeam_logadd_decode(*common, lm_ptr, 1.0, smear_ptr), "eec_ctc_lexbeam_logadd_decode")
                elif lm_ptr is not None:
                    capi.check(lib.eec_ctc_lexbeam_lm_smear_decode(*common, lm_ptr, 1.0, smear_ptr), "eec_ctc_lexbeam_lm_smear_decode")
                else:
                    capi.check(lib.eec_ctc_lexbeam_decode(*common), "eec_ctc_lexbeam_decode")
            rec = {"what": "wide", "mode": mode, "log_add": bool(log_add), "n_seq": n, "frames": T, "lm_weight": 1.0 if lm_ptr else None}
            kept = {}
            for kind, beam in (("narrow", 10), ("narrow", 16), ("wide", 16), ("wide", 32), ("wide", 64)):
                for _ in range(2):
                    call(kind, beam)
                torch.cuda.synchronize()
                rec[f"{kind}_beam{beam}_train_of_10_ms_per_call"] = event_ms(lambda: call(kind, beam), max(args.reps // 4, 3), per=10)
                rec[f"sequences_with_a_hypothesis_{kind}_beam{beam}"] = int((nh > 0).sum())
                kept[kind, beam] = [o.cpu().numpy().tobytes() for o in outputs]
            med = lambda kind, beam: rec[f"{kind}_beam{beam}_train_of_10_ms_per_call"]["median"]  # noqa: E731
            rec["wide16_returns_narrow16_bytes"] = kept["wide", 16] == kept["narrow", 16]
            rec["ratio_wide16_over_narrow16"] = round(med("wide", 16) / med("narrow", 16), 4)
            rec["ratio_wide32_over_wide16"] = round(med("wide", 32) / med("wide", 16), 4)
            rec["ratio_wide64_over_wide32"] = round(med("wide", 64) / med("wide", 32), 4)
            if parents and mode == "lm_free" and not log_add:
                rec["parent_commit_narrow_beam10_train_of_10_ms_per_call_medians"] = parents
                rec["ratio_narrow_beam10_over_parent_commit"] = round(med("narrow", 10) / statistics.median(parents), 4)
            records.append(rec)
            print(json.dumps(rec), flush=True)


LEXBEAM_ENTRIES = ("eec_ctc_lexbeam_decode", "eec_ctc_lexbeam_lm_decode", "eec_ctc_lexbeam_lm_smear_decode", "eec_ctc_lexbeam_logadd_decode",
                   "eec_ctc_lexbeam_wide_decode")


def parent_leg(args, trie, spellings, dev, records):
    """Every search kernel out of two libraries in one process; returns the legs that miss the time mark or differ in their outputs."""
    new = capi.load()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    if parent.eec_abi_version() != new.eec_abi_version():
        raise SystemExit(f"{args.parent_lib}: ABI v{parent.eec_abi_version()}, this tree has v{new.eec_abi_version()}")
    for name in LEXBEAM_ENTRIES:
        getattr(parent, name).argtypes = getattr(new, name).argtypes
    libs = {"parent": parent, "new": new}
    n, T = 384, args.frames
    em = torch.from_numpy(L.emissions(3, spellings, n, T, 256, 0, 126)).to(dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    words, wc, toks, tc, ts, nh = i32(n, 1, T), i32(n, 1), i32(n, 1, T), i32(n, 1), i32(n, 1, T), i32(n)
    sc = torch.empty((n, 1), dtype=torch.float32, device=dev)
    outputs = (words, wc, toks, tc, ts, sc, nh)
    ws = torch.empty(new.eec_ctc_lexbeam_wide_workspace_bytes(n, T, 64), dtype=torch.uint8, device=dev)
    image = trie.on(dev)
    lm = synthetic_model(len(spellings), args.bigrams, args.trigrams)
    lm_image, smear_image = lm.on(dev), lm.smear(trie).on(dev)
    modes = {"lm_free": (None, None), "lm": (lm_image.data_ptr(), None), "smear": (lm_image.data_ptr(), smear_image.data_ptr())}
    # (kernel, beam, calls per train): fewer calls where one lasts hundreds of milliseconds
    shapes = (("narrow", args.beam, 5), ("wide", 16, 2), ("wide", 32, 1), ("wide", 64, 1))
    missed = []
    for mode, (lm_ptr, smear_ptr) in modes.items():
        for log_add in (0, 1):
            for kind, beam, per in shapes:
                common = (em.data_ptr(), n, T, 256, None, image.data_ptr(), trie.blank, trie.sil, beam, 1, 0.0, 0.0, 50.0, T, words.data_ptr(),
                          wc.data_ptr(), toks.data_ptr(), tc.data_ptr(), ts.data_ptr(), sc.data_ptr(), nh.data_ptr(), ws.data_ptr(), ws.numel(),
                          capi.stream_ptr(dev))
                # the entry a caller of this mode reaches (early_exit_transformer_amd/ctc.py)
                if kind == "wide":
                    name, tail = "eec_ctc_lexbeam_wide_decode", (lm_ptr, 1.0, smear_ptr, log_add)
                elif log_add:
                    name, tail = "eec_ctc_lexbeam_logadd_decode", (lm_ptr, 1.0, smear_ptr)
                else:
                    name, tail = {"lm_free": ("eec_ctc_lexbeam_decode", ()), "lm": ("eec_ctc_lexbeam_lm_decode", (lm_ptr, 1.0)),
                                  "smear": ("eec_ctc_lexbeam_lm_smear_decode", (lm_ptr, 1.0, smear_ptr))}[mode]

                def call(lib):
                    rc = getattr(lib, name)(*common, *tail)
                    if rc != 0:
                        raise SystemExit(f"{name} returned {rc}: {lib.eec_last_error()}")
                got = {}
                for which, lib in libs.items():  # the comparison doubles as the warm-up
                    for o in outputs:
                        o.zero_()
                    call(lib)
                    call(lib)
                    torch.cuda.synchronize()
                    got[which] = [o.cpu().numpy().tobytes() for o in outputs]
                ms = {which: [] for which in libs}
                for _ in range(args.rounds):
                    for which, lib in libs.items():
                        ms[which].append(event_ms(lambda: call(lib), 1, per=per)["median"])  # one train of `per` calls
                p = {"median": round(statistics.median(ms["parent"]), 4), "min": min(ms["parent"]), "max": max(ms["parent"])}
                q = {"median": round(statistics.median(ms["new"]), 4), "min": min(ms["new"]), "max": max(ms["new"])}
                rec = {"what": "parent_lib", "kernel": kind, "mode": mode, "log_add": bool(log_add), "beam": beam, "entry": name, "n_seq": n, "frames": T,
                       "rounds": args.rounds, "calls_per_train": per, "parent_ms_per_call": p, "new_ms_per_call": q,
                       "new_minus_parent_median_ms": round(q["median"] - p["median"], 4), "parent_range_ms": round(p["max"] - p["min"], 4),
                       "time_mark_met": q["median"] - p["median"] <= p["max"] - p["min"], "outputs_bit_identical": got["parent"] == got["new"],
                       "sequences_with_a_hypothesis": int((nh > 0).sum())}
                if not rec["time_mark_met"]:
                    missed.append(f"{kind} {mode} log_add={log_add} beam {beam}: time")
                if not rec["outputs_bit_identical"]:
                    missed.append(f"{kind} {mode} log_add={log_add} beam {beam}: outputs differ")
                records.append(rec)
                print(json.dumps(rec), flush=True)
    return missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seqs", default="1,64,384")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    ap.add_argument("--lm", action="store_true", help="time the search with a synthetic 3-gram model against the search without one")
    ap.add_argument("--smear", action="store_true", help="with --lm: also the search with LM look-ahead (max trie smearing)")
    ap.add_argument("--log-add", action="store_true", help="time log-add merging against Viterbi merging; combines with --lm and --smear")
    ap.add_argument("--wide", action="store_true", help="time the wide-beam kernel at beams 16, 32, 64 against the narrow entries at 10 and 16")
    ap.add_argument("--bigrams", type=int, default=2000000)
    ap.add_argument("--trigrams", type=int, default=2000000)
    ap.add_argument("--parent-record", nargs="*", help="records of this tool run from the parent commit on the same box")
    ap.add_argument("--parent-lib", default=None, help="a libeec.so built from the commit to compare against (the same ABI version)")
    ap.add_argument("--rounds", type=int, default=11, help="with --parent-lib: trains per library and leg, the two libraries in turn")
    args = ap.parse_args()
    if args.smear and not args.lm:
        ap.error("--smear goes with --lm")
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: there is nothing to time on the CPU")
    dev = torch.device("cuda", 0)
    records = [{"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}]
    spellings = synthetic_spellings()
    trie = TokenTrie.from_spellings(spellings, 256, blank=0, sil=126)
    image = trie._image.numpy().view(np.int32)
    degree = np.diff(image[16:16 + trie.n_nodes + 1])
    records.append({"what": "trie", "words": len(spellings), "nodes": trie.n_nodes, "shadowed": trie.n_shadowed, "root_degree": int(degree[0]),
                    "largest_other_degree": int(degree[1:].max()), "longest_spelling": max(map(len, spellings)), "image_bytes": trie._image.numel()})
    print(json.dumps(records[-1]), flush=True)
    # the synthetic trie stands for the real one only while it has its size: nodes within 2 %, the same extreme degrees
    assert abs(trie.n_nodes - 162621) <= 0.02 * 162621 and degree[0] == 109 and degree[1:].max() == 103 and trie.n_shadowed == 0, records[-1]
    counts = [] if args.lm or args.log_add or args.wide or args.parent_lib else [int(q) for q in args.seqs.split(",")]
    missed = []
    if args.parent_lib:
        missed = parent_leg(args, trie, spellings, dev, records)
        records[0]["missed"] = missed
    elif args.wide:
        wide_leg(args, trie, spellings, dev, records)
    elif args.log_add:
        logadd_leg(args, trie, spellings, dev, records)
    elif args.lm:
        lm_leg(args, trie, spellings, dev, records)
    pool = torch.from_numpy(L.emissions(3, spellings, max(counts), args.frames, 256, 0, 126)).to(dev) if counts else None
    for n in counts:
        lexbeam, yardstick, nh = prepared_calls(trie, pool[:n].contiguous(), args.beam, 1, dev)
        rec = {"what": "launch", "n_seq": n, "frames": args.frames, "beam": args.beam}
        for name, call in (("lexbeam", lexbeam), ("ctc_beam_yardstick", yardstick)):
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            rec[name + "_one_call_ms"] = event_ms(call, args.reps)
            rec[name + "_train_of_10_ms_per_call"] = event_ms(call, max(args.reps // 4, 3), per=10)
        rec["ratio_lexbeam_over_yardstick"] = round(rec["lexbeam_train_of_10_ms_per_call"]["median"] / rec["ctc_beam_yardstick_train_of_10_ms_per_call"]["median"], 2)
        rec["sequences_with_a_hypothesis"] = int((nh > 0).sum())
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    if missed:
        print("MISSED:\n  " + "\n  ".join(missed), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
