"""Lexicon post-processing on the device: the reference's ``load_dict`` / ``apply_lex`` (util/tokenizer.py:28-50), which
``inference.py`` applies to every hypothesis it prints.  A word of the text that is not in the lexicon is replaced by the
lexicon word with the smallest edit distance, the first such word in file order; the scan over the lexicon -- a Python loop
per word in the reference -- is one call into libeec.so for all words at once (``eec_lexicon_nearest``, csrc/lexicon.hip).
There is no CPU path: without a HIP device ``nearest`` raises, and with it everything that has a word to look up.

``TokenTrie`` is the other use of a lexicon: the spellings of its words as token sequences, packed into the trie image that the
lexicon-constrained CTC beam search walks (``ctc.ctc_lexicon_decode``, csrc/ctc_lexbeam.hip; layout in include/eec.h).
``NGramLM`` is the back-off n-gram word model that search can take along: an ARPA file read against a trie's words and packed into
the n-gram image of include/eec.h (``eec_ngram_pack``, host code); ``NGramLM.smear(trie)`` is the table of its LM look-ahead (max
trie smearing, ``eec_ctc_trie_smear``, host code)."""
from __future__ import annotations

import ctypes as C
import io
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import capi

MAX_QUERY = 256   # EEC_LEX_MAX_QUERY (include/eec.h): symbols of the longest word that can be looked up
BLOCK_WORDS = 256  # EEC_LEX_BLOCK_WORDS: lexicon words per workgroup
TILE_SWITCH = 2048  # EEC_LEX_TILE_SWITCH: queries per call from which the 32-bit kernel advances 8 queries per workgroup, not 4


def load_dict(file_path) -> List[str]:
    """util/tokenizer.py:28-33: one entry per line, the line feed stripped, blank lines kept as ``""``."""
    with io.open(file_path, encoding="utf-8") as f:
        return [line.strip("\n") for line in f]


class _Codes(dict):
    """``str.translate`` table: a code point of the lexicon's alphabet -> its byte code, any other -> 0."""

    def __missing__(self, key):
        return 0


class Lexicon:
    """A word list packed once for the device.  ``words`` in file order (duplicates and empty entries allowed: the first
    index of a word counts); ``device``: where ``nearest`` runs, None = the HIP device current at the call -- the packed image
    is uploaded once and follows a change of device like the encoder handle does.  ``launches`` counts the
    ``eec_lexicon_nearest`` calls made, ``last_stream`` is the stream handle the last of them was given."""

    def __init__(self, words: Iterable[str], device=None):
        self.words: List[str] = list(words)
        self.index: Dict[str, int] = {}
        for i, w in enumerate(self.words):
            self.index.setdefault(w, i)
        self.device = None if device is None else torch.device(device)
        self.launches = 0
        self.last_stream = None  # the stream handle the last ``eec_lexicon_nearest`` call was given
        self.alphabet = 0
        self._codes = _Codes()
        self._image = None     # host copy of the packed image (uint8 tensor)
        self._resident = None  # (device, device copy)
        if self.words:
            self._pack()

    def __len__(self) -> int:
        return len(self.words)

    def __contains__(self, word) -> bool:
        return word in self.index

    def _pack(self) -> None:
        lib = capi.load()
        lens = np.fromiter((len(w) for w in self.words), dtype=np.int64, count=len(self.words))
        offsets = np.zeros(len(self.words) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        symbols = np.frombuffer("".join(self.words).encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
        if symbols.size != offsets[-1]:
            raise ValueError("Lexicon: a word does not encode to one UTF-32 unit per character")
        if len(np.unique(symbols)) > 255:  # stated here for the message; eec_lexicon_pack refuses it as well
            raise ValueError(f"Lexicon: {len(np.unique(symbols))} distinct symbols, the packed alphabet holds at most 255")
        nbytes = lib.eec_lexicon_pack_bytes(len(self.words), int(offsets[-1]), int(lens.max()))
        if nbytes == 0:
            raise ValueError("Lexicon: the word list is too large to pack")
        image = torch.empty((nbytes,), dtype=torch.uint8)
        code_map = np.empty(256, dtype=np.int32)
        n_codes = C.c_int32()
        capi.call("eec_lexicon_pack", symbols.ctypes.data if symbols.size else None, offsets.ctypes.data, len(self.words), image, nbytes,
                  code_map.ctypes.data, C.byref(n_codes))
        self.alphabet = n_codes.value
        self._codes = _Codes({int(code_map[c]): c for c in range(1, self.alphabet + 1)})
        self._image = image

    def _packed_on(self, dev: torch.device) -> Tensor:
        if self._resident is None or self._resident[0] != dev:
            self._resident = (dev, self._image.to(dev))
        return self._resident[1]

    def encode(self, words: Sequence[str]) -> Tuple[np.ndarray, int]:
        """The query block of ``eec_lexicon_nearest`` as one host buffer: int32 offsets [Q + 1], then the encoded bytes; and the
        longest word's length.  Raises for a word over ``MAX_QUERY`` symbols."""
        longest = max((len(w) for w in words), default=0)
        if longest > MAX_QUERY:
            raise ValueError(f"Lexicon: a word of {longest} symbols; at most {MAX_QUERY} can be looked up (EEC_LEX_MAX_QUERY)")
        body = "".join(words).translate(self._codes).encode("latin-1")
        Q = len(words)
        buf = np.zeros(4 * (Q + 1) + len(body), dtype=np.uint8)
        np.cumsum(np.fromiter((len(w) for w in words), dtype=np.int32, count=Q), dtype=np.int32, out=buf[:4 * (Q + 1)].view(np.int32)[1:])
        buf[4 * (Q + 1):] = np.frombuffer(body, dtype=np.uint8)
        return buf, longest

    def nearest(self, words: Sequence[str]) -> Tuple[Tensor, Tensor]:
        """``(index, distance)``, int32 device tensors [Q]: for every word the lexicon entry with the smallest Levenshtein
        distance (the lowest index among equals) and that distance.  The host dict is not consulted: a word of the lexicon comes
        back as its first index at distance 0.  One ``eec_lexicon_nearest`` call on the current stream, no host synchronisation."""
        words = list(words)
        buf, longest = self.encode(words)
        if not self.words:
            raise ValueError("Lexicon.nearest: the lexicon is empty")
        if not torch.cuda.is_available():
            raise RuntimeError("Lexicon.nearest runs on a HIP device only")
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("Lexicon.nearest runs on a HIP device only")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        Q = len(words)
        out = torch.empty((2, Q), dtype=torch.int32, device=dev)
        if Q == 0:
            return out[0], out[1]
        lib = capi.load()
        with torch.cuda.device(dev):
            packed = self._packed_on(dev)
            query = torch.from_numpy(buf).to(dev, non_blocking=True)  # int32 offsets [Q + 1], then the bytes
            ws_bytes = lib.eec_lexicon_nearest_workspace_bytes(Q, len(self.words))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            capi.launch("eec_lexicon_nearest", dev, packed, len(self.words), query.data_ptr() + 4 * (Q + 1), query.data_ptr(), Q, longest,
                        out[0], out[1], ws, ws_bytes)
            self.launches += 1
            self.last_stream = torch.cuda.current_stream(dev).cuda_stream
        return out[0], out[1]

    def apply_batch(self, texts: Sequence[str]) -> List[str]:
        """``apply_lex`` of every text.  The words that are not in the lexicon are collected over all texts, each once, and
        resolved by one ``nearest`` call and one device-to-host copy."""
        pieces = [t.split(" ") for t in texts]
        if not self.words:  # the reference's scan over nothing leaves w_min = ""
            return [" ".join("" for _ in p) for p in pieces]
        missing = list(dict.fromkeys(w for p in pieces for w in p if w not in self.index))
        snapped = {}
        if missing:
            index = self.nearest(missing)[0].cpu().tolist()
            snapped = {w: self.words[i] for w, i in zip(missing, index)}
        return [" ".join(w if w in self.index else snapped[w] for w in p) for p in pieces]

    def apply(self, predicted: str) -> str:
        """util/tokenizer.py:35-50 for one text: split on the single character ``" "`` (the empty pieces of doubled, leading or
        trailing spaces are words too), keep a piece of the lexicon, replace any other by its first nearest word, join."""
        return self.apply_batch([predicted])[0]


class TokenTrie:
    """The token trie of a lexicon, packed once (``eec_ctc_trie_pack``, host code) and kept on the device.  ``words``: the words in
    file order -- the decoder returns indices into it --, ``n_nodes`` the trie's size, ``n_shadowed`` how many spellings repeat an
    earlier one and are therefore unreachable (the first word in file order with a spelling is the one it decodes to)."""

    def __init__(self, words: Sequence[str], spellings: Sequence[Sequence[int]], V: int, blank: int = 0, sil: Optional[int] = None):
        if len(words) != len(spellings):
            raise ValueError(f"TokenTrie: {len(words)} words but {len(spellings)} spellings")
        self.words: List[str] = list(words)
        self.V, self.blank, self.sil = int(V), int(blank), -1 if sil is None else int(sil)
        lib = capi.load()
        lens = np.fromiter((len(sp) for sp in spellings), dtype=np.int64, count=len(spellings))
        offsets = np.zeros(len(spellings) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        flat = np.fromiter((t for sp in spellings for t in sp), dtype=np.int32, count=int(offsets[-1]))
        nbytes = lib.eec_ctc_trie_pack_bytes(len(spellings), int(offsets[-1]))
        image = torch.zeros((max(nbytes, 8),), dtype=torch.uint8)
        n_nodes, n_shadowed = C.c_int32(), C.c_int32()
        capi.call("eec_ctc_trie_pack", flat.ctypes.data if flat.size else None, offsets.ctypes.data, len(spellings), self.V, self.blank,
                  self.sil, image, nbytes, C.byref(n_nodes), C.byref(n_shadowed))
        self.n_nodes, self.n_shadowed = n_nodes.value, n_shadowed.value
        self._image = image[: 4 * int(image[36:40].view(torch.int32))]  # header[9]: the dwords actually used
        self._resident = None  # (device, device copy)

    @classmethod
    def from_spellings(cls, spellings: Sequence[Sequence[int]], V: int, blank: int = 0, sil: Optional[int] = None, words=None) -> "TokenTrie":
        """``spellings``: one list of token ids per word; ``words`` (optional) their strings, else ``"w0", "w1", ...``."""
        spellings = [list(sp) for sp in spellings]
        return cls([f"w{i}" for i in range(len(spellings))] if words is None else words, spellings, V, blank, sil)

    @classmethod
    def from_files(cls, lexicon_path, tokens_path, blank_token: str = "@", sil_token: Optional[str] = None) -> "TokenTrie":
        """The reference's files (args.lexicon / args.tokens): ``word<TAB>space-separated tokens`` per line, and one token per
        line (its line number is its id)."""
        with io.open(tokens_path, encoding="utf-8") as f:
            tokens = [line.rstrip("\r\n") for line in f]
        ids = {t: i for i, t in reversed(list(enumerate(tokens)))}
        if blank_token not in ids or (sil_token is not None and sil_token not in ids):
            raise ValueError(f"TokenTrie: {tokens_path} lacks the blank token {blank_token!r} or the sil token {sil_token!r}")
        words, spellings = [], []
        with io.open(lexicon_path, encoding="utf-8") as f:
            for n, line in enumerate(f, 1):
                line = line.rstrip("\r\n")
                if not line.strip():
                    continue
                word, _, spelling = line.partition("\t")
                if not word or not spelling.split():
                    raise ValueError(f"TokenTrie: {lexicon_path}:{n}: expected word<TAB>tokens, got {line!r}")
                try:
                    spellings.append([ids[t] for t in spelling.split()])
                except KeyError as e:
                    raise ValueError(f"TokenTrie: {lexicon_path}:{n}: token {e.args[0]!r} is not in {tokens_path}") from None
                words.append(word)
        return cls(words, spellings, len(tokens), ids[blank_token], None if sil_token is None else ids[sil_token])

    def __len__(self) -> int:
        return len(self.words)

    def on(self, dev: torch.device) -> Tensor:
        """The packed image on ``dev`` (uploaded once; follows a change of device)."""
        if self._resident is None or self._resident[0] != dev:
            self._resident = (dev, self._image.to(dev))
        return self._resident[1]


class NGramLM:
    """A back-off n-gram word model over the words of one ``TokenTrie``, packed once (``eec_ngram_pack``, host code) and kept on the
    device.  ``order``; ``n_grams``: the kept n-grams per order; ``n_nodes`` = 1 + their sum; ``n_words``: the word count of the
    lexicon it was packed for (the decoder refuses another trie); ``vocab``: the LM words, their index the LM word id;
    ``word_map`` [n_words]: the LM word of every lexicon word (the ``<unk>`` word where the model lacks it); ``bos`` / ``eos`` /
    ``unk``: the LM words of ``<s>`` / ``</s>`` / ``<unk>`` or -1."""

    BOS, EOS, UNK = "<s>", "</s>", "<unk>"
    MAX_ORDER = 5  # include/eec.h

    def __init__(self, words: Sequence[np.ndarray], logp: Sequence[np.ndarray], backoff: Sequence[np.ndarray], word_map, bos: int = -1,
                 eos: int = -1, unk: int = -1, vocab: Optional[Sequence[str]] = None):
        """From arrays per order, as ``eec_ngram_pack`` takes them: ``words[n-1]`` int32 [count_n, n] LM word ids, ``logp[n-1]`` and
        ``backoff[n-1]`` fp32 [count_n]; the unigrams are a permutation of the LM words 0 .. W - 1."""
        order = len(words)
        if not 1 <= order <= self.MAX_ORDER or len(logp) != order or len(backoff) != order:
            raise ValueError(f"NGramLM: orders 1 to {self.MAX_ORDER} are served, with one array of words, logp and backoff each; got {order}")
        ids = [np.ascontiguousarray(np.asarray(w, dtype=np.int32).reshape(-1, n + 1)) for n, w in enumerate(words)]
        lps = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in logp]
        bos_ = [np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in backoff]
        if any(len(a) != len(b) or len(a) != len(c) for a, b, c in zip(ids, lps, bos_)):
            raise ValueError("NGramLM: the words, logp and backoff arrays of an order differ in length")
        self.word_map = np.ascontiguousarray(word_map, dtype=np.int32).reshape(-1)
        self.order, self.n_grams, self.n_words = order, [len(a) for a in ids], int(self.word_map.size)
        self.bos, self.eos, self.unk = int(bos), int(eos), int(unk)
        self.vocab = None if vocab is None else list(vocab)
        lib = capi.load()
        counts = np.array(self.n_grams, dtype=np.int64)
        nbytes = lib.eec_ngram_pack_bytes(order, counts.ctypes.data, self.n_words)
        image = torch.zeros((max(nbytes, 8),), dtype=torch.uint8)
        ptrs = lambda arrays: (C.c_void_p * order)(*[a.ctypes.data if a.size else None for a in arrays])  # noqa: E731
        n_nodes = C.c_int32()
        capi.call("eec_ngram_pack", order, counts.ctypes.data, ptrs(ids), ptrs(lps), ptrs(bos_), self.word_map.ctypes.data if self.n_words else None,
                  self.n_words, self.bos, self.eos, image, nbytes, C.byref(n_nodes))
        self.n_nodes = n_nodes.value
        self._image = image[: 4 * int(image[60:64].view(torch.int32))]  # header[15]: the dwords actually used
        self._resident = None  # (device, device copy)
        self._smear = None     # (the trie it was built for, its SmearTable)

    @classmethod
    def from_arpa(cls, path, trie: "TokenTrie", normalize=None, exempt: Sequence[int] = ()) -> "NGramLM":
        """The ARPA file ``path`` read against ``trie.words``: an LM word is matched exactly, after ``normalize`` (None: identity;
        ``<s>``, ``</s>`` and ``<unk>`` are matched as they stand) was applied to it; lexicon entries with the same string share an
        LM word; a lexicon word the model lacks scores as ``<unk>``.  N-grams with a word outside the lexicon and those three can
        never be asked for and are dropped.  The file's log10 values are kept as they are, rounded to fp32.  Raises a ``ValueError``
        that names file and line for a malformed file, and one that counts the missing words when the model has no ``<unk>``.
        Only ``trie.words`` is read.  ``exempt``: indices into it of entries that are never looked up (the special tokens of
        ``lm_fusion.TokenLM``); they are not counted as missing and map to ``<unk>``, or to LM word 0 when the model has none."""
        lex = set(trie.words)
        special = (cls.BOS, cls.EOS, cls.UNK)

        def bad(line_no, what):
            return ValueError(f"NGramLM: {path}:{line_no}: {what}")

        declared: Dict[int, int] = {}
        vocab: List[str] = []
        ids: Dict[str, int] = {}    # kept LM word (after normalize) -> LM word id
        outside = set()             # unigrams that were dropped
        grams: List[Dict[tuple, int]] = []  # per order: kept n-gram (ids) -> its row
        rows: List[Tuple[list, list, list]] = []
        n, seen_in_section, section_line, state = 0, 0, 0, "head"

        def close_section(line_no):
            if n and seen_in_section != declared[n]:
                raise bad(line_no, f"the {n}-gram section that began at line {section_line} holds {seen_in_section} n-grams, \\data\\ states {declared[n]}")

        line_no = 0
        with io.open(path, encoding="utf-8") as f:
            for line_no, line in enumerate(f, 1):
                line = line.strip()
                if not line:
                    continue
                if state == "head":
                    if line == "\\data\\":
                        state = "data"
                    continue
                if line.startswith("\\"):
                    close_section(line_no)
                    if line == "\\end\\":
                        state = "end"
                        break
                    try:
                        want = int(line[1:line.index("-grams:")])
                    except ValueError:
                        raise bad(line_no, f"expected \\N-grams: or \\end\\, got {line!r}") from None
                    if want != n + 1 or want not in declared:
                        raise bad(line_no, f"section {line!r} where the section of order {n + 1} {'is' if n + 1 in declared else 'is not'} expected")
                    n, seen_in_section, section_line, state = want, 0, line_no, "grams"
                    grams.append({})
                    rows.append(([], [], []))
                    continue
                if state == "data":
                    if not line.startswith("ngram ") or "=" not in line:
                        raise bad(line_no, f"expected 'ngram N=count', got {line!r}")
                    try:
                        k, count = (int(v) for v in line[6:].split("="))
                    except ValueError:
                        raise bad(line_no, f"expected 'ngram N=count', got {line!r}") from None
                    if k > cls.MAX_ORDER:
                        raise bad(line_no, f"order {k}: orders above {cls.MAX_ORDER} are not served")
                    if k != len(declared) + 1 or count < 0:
                        raise bad(line_no, f"'ngram {k}={count}' where order {len(declared) + 1} is expected")
                    declared[k] = count
                    continue
                fields = line.split()
                if len(fields) not in (n + 1, n + 2):
                    raise bad(line_no, f"a {n}-gram line holds a log-probability, {n} words and at most a back-off; got {len(fields)} fields")
                try:
                    lp = float(fields[0])
                    bo = float(fields[n + 1]) if len(fields) == n + 2 else 0.0
                except ValueError:
                    raise bad(line_no, f"not a number in {line!r}") from None
                if not (math.isfinite(lp) and math.isfinite(bo) and math.isfinite(float(np.float32(lp))) and math.isfinite(float(np.float32(bo)))):
                    raise bad(line_no, f"a non-finite number in {line!r}")
                seen_in_section += 1
                names = [w if w in special or normalize is None else normalize(w) for w in fields[1:n + 1]]
                if n == 1:
                    w = names[0]
                    if w in ids or w in outside:
                        raise bad(line_no, f"duplicate n-gram {w!r}")
                    if w not in lex and w not in special:
                        outside.add(w)
                        continue
                    ids[w] = len(vocab)
                    vocab.append(w)
                    key = (ids[w],)
                else:
                    if any(w not in ids and w not in outside for w in names):
                        raise bad(line_no, f"a word of {' '.join(names)!r} has no unigram")
                    if any(w in outside for w in names):
                        continue
                    key = tuple(ids[w] for w in names)
                    if key[:-1] not in grams[n - 2]:
                        raise bad(line_no, f"the prefix {' '.join(names[:-1])!r} of {' '.join(names)!r} is not a {n - 1}-gram of the file")
                    if key in grams[n - 1]:
                        raise bad(line_no, f"duplicate n-gram {' '.join(names)!r}")
                grams[n - 1][key] = len(rows[n - 1][1])
                rows[n - 1][0].extend(key)
                rows[n - 1][1].append(lp)
                rows[n - 1][2].append(bo)
        if state != "end":
            raise bad(line_no if state != "head" else 1, "the file ends without \\end\\" if state != "head" else "no \\data\\ section")
        if len(rows) != len(declared) or not declared:
            raise bad(line_no, f"\\data\\ states {len(declared)} orders, the file holds the sections of {len(rows)}")
        unk = ids.get(cls.UNK, -1)
        spared = {trie.words[k] for k in exempt}
        missing = [w for w in dict.fromkeys(trie.words) if w not in ids and w not in spared]
        if missing and unk < 0:
            raise ValueError(f"NGramLM: {path}: the model has no <unk> and lacks {len(missing)} of the lexicon's words: "
                             + ", ".join(repr(w) for w in missing[:5]) + (", ..." if len(missing) > 5 else ""))
        if not vocab:
            raise ValueError(f"NGramLM: {path}: no unigram of the model is a word of the lexicon")
        word_map = np.fromiter((ids.get(w, unk if unk >= 0 or w not in spared else 0) for w in trie.words), dtype=np.int32, count=len(trie.words))
        return cls([np.array(r[0], dtype=np.int32).reshape(-1, k + 1) for k, r in enumerate(rows)], [np.array(r[1], dtype=np.float32) for r in rows],
                   [np.array(r[2], dtype=np.float32) for r in rows], word_map, ids.get(cls.BOS, -1), ids.get(cls.EOS, -1), unk, vocab)

    def on(self, dev: torch.device) -> Tensor:
        """The packed image on ``dev`` (uploaded once; follows a change of device)."""
        if self._resident is None or self._resident[0] != dev:
            self._resident = (dev, self._image.to(dev))
        return self._resident[1]


    def smear(self, trie: "TokenTrie") -> "SmearTable":
        """The LM look-ahead table of ``trie`` under this model (max trie smearing: every node carries the best start-state score
        of the words at or below it; ``eec_ctc_trie_smear``, host code, from the two host images).  Built once per trie and
        cached, the table of the last trie asked for is kept; it follows the device like ``on()``."""
        if self._smear is None or self._smear[0] is not trie:
            if self.n_words != len(trie.words):
                raise ValueError(f"NGramLM.smear: the model was packed for a lexicon of {self.n_words} words, the trie has {len(trie.words)}")
            lib = capi.load()
            nbytes = lib.eec_ctc_trie_smear_bytes(trie.n_nodes)
            table = torch.zeros((max(nbytes, 8),), dtype=torch.uint8)
            capi.call("eec_ctc_trie_smear", trie._image, self._image, table, nbytes)
            self._smear = (trie, SmearTable(table))
        return self._smear[1]


class SmearTable:
    """The smear table of one (trie, model) pair (layout in include/eec.h): a host copy and, at the first use, a device copy."""

    def __init__(self, table: Tensor):
        self._image = table
        self._resident = None  # (device, device copy)

    @property
    def values(self) -> np.ndarray:
        """``smax`` [n_nodes] fp32, indexed by the trie image's node numbers."""
        head = self._image[:16].view(torch.int32)
        return self._image[16:16 + 4 * int(head[1])].view(torch.float32).numpy()

    def on(self, dev: torch.device) -> Tensor:
        """The table on ``dev`` (uploaded once; follows a change of device)."""
        if self._resident is None or self._resident[0] != dev:
            self._resident = (dev, self._image.to(dev))
        return self._resident[1]


_by_list: List[Tuple[list, Lexicon]] = []  # plain lists handed to apply_lex, by identity (the list is kept alive: its id stays its own)


def as_lexicon(lexicon: Union[Lexicon, Sequence[str]]) -> Lexicon:
    """``lexicon`` itself, or the ``Lexicon`` packed from this very list object at its first use (the last four lists are kept;
    a list whose length changed since is packed again, one whose entries were replaced in place must be passed as a new
    ``Lexicon``)."""
    if isinstance(lexicon, Lexicon):
        return lexicon
    for i, (words, lex) in enumerate(_by_list):
        if words is lexicon:
            if len(words) == len(lex):
                return lex
            del _by_list[i]  # grown or shrunk in place since it was packed: pack it again
            break
    lex = Lexicon(lexicon)
    _by_list.append((lexicon, lex))
    del _by_list[:-4]
    return lex


def apply_lex(predicted: str, lexicon: Union[Lexicon, Sequence[str]]) -> str:
    """The reference's ``apply_lex(predicted, lexicon)`` (util/tokenizer.py:35-50); ``lexicon`` is a ``Lexicon`` or the plain
    list ``load_dict`` returns."""
    return as_lexicon(lexicon).apply(predicted)
