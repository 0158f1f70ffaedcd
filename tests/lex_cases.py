"""Test-side statement of the lexicon post-processing (early_exit_transformer_amd/lexicon.py, csrc/lexicon.hip): a two-row
Levenshtein distance in plain Python, the snapping rule of the reference's ``apply_lex`` (util/tokenizer.py:35-50) in our own
words, a reader of the packed image's documented layout (include/eec.h), and the generators of the test cases.  Everything
here is integers and strings: comparisons against it are exact.  The pure-Python distance costs ~23 us per pair of real words,
so a test keeps queries x lexicon words <= 150 000."""
import json
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "apply_lex.json")
LETTERS = "abcdefghijklmnopqrstuvwxyz'"  # the 27 symbols of librispeech.lex
# word counts of librispeech.lex by length 1..25; one more word has 69 symbols (89 114 in all)
LENGTH_HISTOGRAM = [26, 190, 1296, 4183, 8210, 12502, 14923, 14430, 12117, 8854, 5747, 3384, 1811, 830, 369, 144, 59, 21, 9, 3, 1, 2, 0, 1, 1]
QUERY_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)  # both sides of every vector width and word carry


def levenshtein(a, b) -> int:
    """Edit distance (insert, delete, substitute, each 1) of two sequences, two rows of the table at a time."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def nearest_ref(word: str, lexicon):
    """(index, distance) of the first lexicon entry at the smallest distance from ``word``."""
    best, at = None, -1
    for i, w in enumerate(lexicon):
        d = levenshtein(word, w)
        if best is None or d < best:
            best, at = d, i
    return at, best


def snap(text: str, lexicon) -> str:
    """The snapping rule: cut ``text`` at every single space (so doubled, leading and trailing spaces give empty words); a word
    that is an entry of the lexicon stays, any other becomes the first entry nearest to it ("" when there is no entry)."""
    known = set(lexicon)
    out = []
    for w in text.split(" "):
        out.append(w if w in known else (lexicon[nearest_ref(w, lexicon)[0]] if lexicon else ""))
    return " ".join(out)


def load_fixture():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


def unpack_image(image, code_map):
    """The words of a packed image (a sequence of int32) by original index, and the lengths in stored (sorted) order, read by
    the layout include/eec.h documents."""
    magic, n_words, max_len, n_groups, A, off_info, off_gbase, off_sym, n_sym, total = (int(v) for v in image[:10])
    assert magic == 0x4c434545 and n_groups == (max_len + 3) // 4 and total == len(image)
    assert off_info == 16 and off_gbase == off_info + 2 * n_words and off_sym == off_gbase + n_groups and off_sym + n_sym <= total
    words, lengths = [None] * n_words, []
    for s in range(n_words):
        orig, length = int(image[off_info + 2 * s]), int(image[off_info + 2 * s + 1])
        codes = []
        for p in range(length):
            at = int(image[off_gbase + p // 4]) + s
            assert 0 <= at < n_sym
            codes.append((int(image[off_sym + at]) >> (8 * (p % 4))) & 255)
        assert all(1 <= c <= A for c in codes)
        assert words[orig] is None
        words[orig] = "".join(chr(int(code_map[c])) for c in codes)
        lengths.append((length, orig))
    return words, lengths


def random_word(rng, n, letters=LETTERS):
    return "".join(rng.choice(letters) for _ in range(n))


def random_lexicon(n, seed, lengths=range(1, 13), letters=LETTERS):
    rng = random.Random(seed)
    lengths = list(lengths)
    return [random_word(rng, rng.choice(lengths), letters) for _ in range(n)]


def boundary_lexicon(seed=5):
    """512 random words over four letters, in no order of length: lengths 0 (twice), 1, 69 and 100, six words of 127 .. 300
    symbols (near neighbours for the long queries), twenty of 30 .. 90, the rest short -- the oracle's cost is the total
    length."""
    rng = random.Random(seed)
    lens = [0, 1, 69, 100, 0, 127, 128, 200, 250, 256, 300] + [rng.choice((30, 31, 32, 33, 60, 64, 65, 90)) for _ in range(20)]
    lens += [rng.choice((2, 3, 5, 8)) for _ in range(512 - len(lens))]
    rng.shuffle(lens)
    return [random_word(rng, n, "abcd") for n in lens]


def boundary_queries(lexicon, seed=6):
    """One query per length of QUERY_LENGTHS: a lexicon-like random word over the same four letters plus one symbol the lexicon
    does not have, so that every vector word of a long query carries matches."""
    rng = random.Random(seed)
    out = []
    for m in QUERY_LENGTHS:
        w = list(random_word(rng, m, "abcd"))
        if m > 2:
            w[m // 2] = "z"
        out.append("".join(w))
    return out


def tie_lexicon(block_words, seed=7):
    """(lexicon, {query: expected index}).  4 * block_words + 3 entries: "tie" stands at index 0, in the middle and last, and
    four distinct words one substitution away from the query "qqxq" stand far apart, the alphabetically last of them first;
    everything else is random words of 3, 4 or 9 letters from another alphabet, far from both.  A stable sort by length keeps
    each family in index order but spreads it: the three-letter words alone are more than two workgroups' shares of
    ``block_words``, the four-letter words follow them."""
    rng = random.Random(seed)
    n = 4 * block_words + 3
    words = [random_word(rng, rng.choice((3, 3, 3, 4, 9)), "mnoprs") for _ in range(n)]
    words[0] = words[n // 2] = words[n - 1] = "tie"
    step = (n - n // 3) // 5
    for i, w in enumerate(["qqdq", "qqcq", "qqbq", "qqaq"]):
        words[n // 3 + step * i] = w
    return words, {"tie": 0, "tix": 0, "qqxq": n // 3, "qqaq": n // 3 + 3 * step}


def synthetic_full_lexicon(seed=1):
    """89 114 words drawn from a seed with the length histogram of librispeech.lex over 27 symbols, in random order."""
    rng = random.Random(seed)
    lens = [n for n, count in enumerate(LENGTH_HISTOGRAM, 1) for _ in range(count)] + [69]
    rng.shuffle(lens)
    return [random_word(rng, n) for n in lens]
