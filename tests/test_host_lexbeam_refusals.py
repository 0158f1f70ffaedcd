"""Every refusal of the six lexicon CTC beam search entries (eec_ctc_lexbeam_decode, _lm_, _lm_smear_, _logadd_, _wide_decode with
log_add 0 and 1), pinned: return code and the full eec_last_error() text of each entry for each bad call, against the table in
tests/golden/lexbeam_refusals.txt.  The table was recorded from the library as it stood before the entries were given one shared
argument check, so that the shared check answers each entry exactly as its own copy did -- code, wording and precedence.

Every call passes a workspace size one byte short, and the size check is the last one before the launch: a call that nothing
else refuses is refused there, so nothing is ever dereferenced or launched (the addresses are plausible but unusable).

    PYTHONPATH=. python tests/test_host_lexbeam_refusals.py        rewrites the table from the library that is built
"""
import os

import pytest

from early_exit_transformer_amd import capi
from lexbeam_helpers import library

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lexbeam_refusals.txt")
FAKE = 0x10000
NAN, INF = float("nan"), float("inf")

# (name in the table, C entry, takes lm + lm_weight, takes smear, log_add argument or None)
ENTRIES = [
    ("decode", "eec_ctc_lexbeam_decode", False, False, None),
    ("lm", "eec_ctc_lexbeam_lm_decode", True, False, None),
    ("lm_smear", "eec_ctc_lexbeam_lm_smear_decode", True, True, None),
    ("logadd", "eec_ctc_lexbeam_logadd_decode", True, True, None),
    ("wide", "eec_ctc_lexbeam_wide_decode", True, True, 0),
    ("wide_logadd", "eec_ctc_lexbeam_wide_decode", True, True, 1),
]

NULLS = ("logp", "trie", "words", "wc", "tok", "tc", "sc", "nh", "ws")
CASES = [
    ("nothing else wrong: short workspace", {}),
    ("n_seq -1", dict(n=-1)), ("Tq 0", dict(T=0)), ("max_words 0", dict(max_words=0)),
    ("V 257", dict(V=257)), ("V 1", dict(V=1)),
    ("beam 0", dict(beam=0)), ("beam -3", dict(beam=-3)), ("beam 17 nbest 2", dict(beam=17)), ("beam 65", dict(beam=65)),
    ("beam 16 nbest 16", dict(beam=16, nbest=16)), ("beam 64 nbest 64", dict(beam=64, nbest=64)),
    ("nbest 0", dict(nbest=0)), ("nbest 11 of beam 10", dict(nbest=11)), ("nbest 18 of beam 17", dict(beam=17, nbest=18)),
    ("blank -1", dict(blank=-1)), ("blank V", dict(blank=40)), ("sil V", dict(sil=40)), ("sil -2", dict(sil=-2)), ("sil is the blank", dict(blank=5, sil=5)),
    ("lm_weight nan", dict(lm_weight=NAN)), ("lm_weight inf", dict(lm_weight=INF)), ("lm_weight -inf", dict(lm_weight=-INF)),
    ("lm null: smear without lm", dict(lm=None)), ("lm null, lm_weight nan", dict(lm=None, lm_weight=NAN)),
    ("smear null", dict(smear=None)), ("smear misaligned", dict(smear=FAKE + 4)), ("lm null and smear null", dict(lm=None, smear=None)),
    ("lm null and smear null, lm_weight nan", dict(lm=None, smear=None, lm_weight=NAN)),
    ("smear without lm, n_seq -1", dict(lm=None, n=-1)), ("smear without lm, beam 65", dict(lm=None, beam=65)),
    ("smear null, lm_weight nan", dict(smear=None, lm_weight=NAN)), ("smear misaligned, lm null", dict(lm=None, smear=FAKE + 4)),
    *[(f"{name} null", {name: None}) for name in NULLS],
    ("every output null", {name: None for name in NULLS}),
    ("trie misaligned", dict(trie=FAKE + 4)), ("workspace misaligned", dict(ws=FAKE + 4)), ("lm misaligned", dict(lm=FAKE + 4)),
    ("lm misaligned, smear null", dict(lm=FAKE + 4, smear=None)), ("trie misaligned, lm null and smear null", dict(trie=FAKE + 4, lm=None, smear=None)),
    ("trie null and smear misaligned", dict(trie=None, smear=FAKE + 4)), ("V 257 and blank -1", dict(V=257, blank=-1)),
    ("n_seq -1 and V 257", dict(n=-1, V=257)), ("lm_weight nan and blank -1", dict(lm_weight=NAN, blank=-1)),
    ("n_seq 0, everything null", dict(n=0, ws_bytes=0, lm=None, smear=None, **{name: None for name in NULLS})),
    ("n_seq 0, beam 65", dict(n=0, beam=65)), ("n_seq 0, lm_weight nan", dict(n=0, lm_weight=NAN)), ("n_seq 0, smear misaligned", dict(n=0, smear=FAKE + 4)),
    ("n_seq 0, trie misaligned", dict(n=0, trie=FAKE + 4)),
]


@pytest.fixture(scope="module")
def lib():
    return library()


def answer(lib, entry, case):
    """(return code, message) of one entry for one case.  A call that is not refused must be one with nothing to do (n_seq 0)."""
    _, symbol, has_lm, has_smear, log_add = entry
    a = dict(logp=FAKE, n=3, T=7, V=40, em_len=None, trie=FAKE, blank=0, sil=-1, beam=10, nbest=2, thr=50.0, max_words=7, words=FAKE, wc=FAKE,
             tok=FAKE, tc=FAKE, ts=None, sc=FAKE, nh=FAKE, ws=FAKE, ws_bytes=None, lm=FAKE, lm_weight=1.0, smear=FAKE)
    a.update(case)
    if a["ws_bytes"] is None:  # one byte short of what the entry's own size function asks for; 0 where that is 0
        size = lib.eec_ctc_lexbeam_wide_workspace_bytes if log_add is not None else lib.eec_ctc_lexbeam_workspace_bytes
        a["ws_bytes"] = max(size(a["n"], a["T"], a["beam"]) - 1, 0)
    assert min(a["n"], a["T"], a["beam"]) <= 0 or a["ws_bytes"] < a["n"] * a["T"] * a["beam"] * 8  # no case can reach the launch
    tail = ([a["lm"], a["lm_weight"]] if has_lm else []) + ([a["smear"]] if has_smear else []) + ([log_add] if log_add is not None else [])
    rc = getattr(lib, symbol)(a["logp"], a["n"], a["T"], a["V"], a["em_len"], a["trie"], a["blank"], a["sil"], a["beam"], a["nbest"], 0.0, 0.0,
                              a["thr"], a["max_words"], a["words"], a["wc"], a["tok"], a["tc"], a["ts"], a["sc"], a["nh"], a["ws"], a["ws_bytes"],
                              None, *tail)
    assert rc != 0 or a["n"] == 0, (entry[0], case)
    return rc, (lib.eec_last_error().decode() if rc else "")


def lines_of(lib, entry):
    return [f"{entry[0]}\t{name}\t{rc}\t{msg}" for name, case in CASES for rc, msg in [answer(lib, entry, case)]]


def test_the_table_covers_every_entry_and_case():
    with open(TABLE, encoding="utf-8") as f:
        rows = [line.rstrip("\n").split("\t") for line in f]
    assert [(r[0], r[1]) for r in rows] == [(e[0], name) for e in ENTRIES for name, _ in CASES]
    assert all(len(r) == 4 for r in rows)
    codes = {r[2] for r in rows}
    assert codes == {"0", "10001", "10002", "10003"}, codes  # nothing to do, bad argument, unsupported, workspace


@pytest.mark.parametrize("entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_every_refusal_is_the_recorded_one(lib, entry):
    with open(TABLE, encoding="utf-8") as f:
        want = [line.rstrip("\n") for line in f if line.split("\t")[0] == entry[0]]
    got = lines_of(lib, entry)
    assert len(got) == len(want) == len(CASES)
    for g, w in zip(got, want):
        assert g == w


if __name__ == "__main__":
    the_lib = capi.load()
    with open(TABLE, "w", encoding="utf-8") as out:
        for e in ENTRIES:
            out.write("".join(line + "\n" for line in lines_of(the_lib, e)))
    print(f"wrote {TABLE}")
