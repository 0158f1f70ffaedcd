"""Generates tests/golden/bpe256_lexicon_slice.json from two data files the REFERENCE's programs read (util/beam_infer.py:56-57
hands them to the lexicon decoder as ``args.lexicon`` / ``args.tokens``): the 256 tokens of ``librispeech-bpe-256.tok`` and every
45th line of ``librispeech-bpe-256.lex`` (``word<TAB>space-separated tokens``).  Data only, nothing else.

Build-container only (needs /root/reference).

    python tests/golden/make_lexbeam_golden.py
"""
import io
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "/root/reference/sentencepiece/build"


def main():
    with io.open(os.path.join(SOURCE, "librispeech-bpe-256.tok"), encoding="utf-8") as f:
        tokens = [line.rstrip("\n") for line in f]
    with io.open(os.path.join(SOURCE, "librispeech-bpe-256.lex"), encoding="utf-8") as f:
        lines = [line.rstrip("\n") for line in f]
    assert len(tokens) == 256 and len(set(tokens)) == 256 and len(lines) == 89114
    known = set(tokens)
    lexicon = []
    for line in lines[::45]:
        word, _, spelling = line.partition("\t")
        assert word and spelling and all(t in known for t in spelling.split())
        lexicon.append([word, " ".join(spelling.split())])
    path = os.path.join(HERE, "bpe256_lexicon_slice.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"tokens": tokens, "lexicon": lexicon}, f, ensure_ascii=False, indent=0)
    print(f"wrote {path}: {len(tokens)} tokens, {len(lexicon)} words, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
