"""Generates tests/golden/apply_lex.json by running the REFERENCE's own ``load_dict`` / ``apply_lex``
(util/tokenizer.py:28-50), unmodified, on a slice of its lexicon.

Build-container only (needs /root/reference).  The module imports the third-party ``editdistance``, which is absent; it is
stubbed in ``sys.modules`` with the two-row Levenshtein of tests/lex_cases.py (``editdistance.eval`` IS the Levenshtein
distance of two sequences).  The fixture is data only: the lexicon slice (the first 20 lines, every 40th line, the 69-symbol
word) and a list of input strings with the strings the reference returned for them on that slice.

    python tests/golden/make_lex_golden.py
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]
import lex_cases as L  # noqa: E402

REFERENCE = "/root/reference"


def reference_tokenizer():
    ed = types.ModuleType("editdistance")
    ed.eval = L.levenshtein
    sys.modules["editdistance"] = ed
    sys.path.insert(0, REFERENCE)
    from util import tokenizer
    return tokenizer


def main():
    tk = reference_tokenizer()
    full = tk.load_dict(os.path.join(REFERENCE, "librispeech.lex"))
    longest = max(range(len(full)), key=lambda i: len(full[i]))
    assert len(full[longest]) == 69
    keep = sorted(set(range(20)) | set(range(0, len(full), 40)) | {longest})
    lexicon = [full[i] for i in keep]
    known = [w for w in lexicon if len(w) > 3]
    inputs = [
        "the quik brown  fox jumpd ovr teh lazy dog",  # a double space: an empty word
        "",
        " ",
        "héllo wor1d a'll",  # symbols outside the lexicon's alphabet
        ("antidisestablishmentarianism" * 3)[:70],  # a 70-symbol word
        full[longest][:-1] + "x",
        " ".join(known[i] for i in (3, 500, 1500, 77)),  # words of the lexicon only
        " leading and trailing ",
        "a b c xqz zzzzzzzzzzzz",
    ]
    outputs = [tk.apply_lex(s, lexicon) for s in inputs]
    assert outputs[6] == inputs[6]
    path = os.path.join(HERE, "apply_lex.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"lexicon": lexicon, "inputs": inputs, "outputs": outputs}, f, ensure_ascii=False, indent=0)
    print(f"wrote {path}: {len(lexicon)} words, {len(inputs)} inputs, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
