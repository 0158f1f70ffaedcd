// Host-only packers of the three images the lexicon-constrained CTC beam search reads (layouts in include/eec.h): the token trie
// (eec_ctc_trie_pack), the back-off n-gram model (eec_ngram_pack) and the max-smearing table (eec_ctc_trie_smear), with their size
// functions.  Nothing here runs on the device; the kernels that read the images are ctc_lexbeam.hip and ctc_lexbeam_wide.hip, and
// the smear table's scores come from the very lm_view / lm_walk the kernels run (eec_lexbeam.h): one sequence of fp32 additions.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_lexbeam.h"

namespace eec {

static size_t lb_image_dwords(unsigned long long nodes) {  // nodes >= 1
  return (size_t)(kLbHeader + (nodes + 1) + (nodes - 1 + 3) / 4 + nodes + 1) & ~(size_t)1;
}

static size_t lm_image_dwords(unsigned long long nodes, unsigned long long lex_words) {  // nodes >= 1
  return (size_t)(kLmHeader + (nodes + 1) + (nodes - 1) + 3 * nodes + lex_words + 1) & ~(size_t)1;
}

}  // namespace eec

extern "C" {

size_t eec_ctc_trie_pack_bytes(int n_words, int64_t total_tokens) {
  if (n_words <= 0 || total_tokens < n_words) return 0;
  const size_t dwords = eec::lb_image_dwords((unsigned long long)total_tokens + 1);  // a trie has at most one node per token, and the root
  return dwords >= ((size_t)1 << 31) ? 0 : dwords * 4;                                // the kernel indexes the image with int32
}

int eec_ctc_trie_pack(const int32_t* spellings, const int64_t* offsets, int n_words, int V, int blank, int sil, void* image,
                      size_t image_bytes, int32_t* n_nodes, int32_t* n_shadowed) {
  using namespace eec;
  using eech::fail;
  if (!spellings || !offsets || !image) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: null argument (spellings, offsets, image)");
  if (n_words <= 0) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: n_words must be positive");
  if (V > 256) return fail(EEC_ERR_UNSUPPORTED, "eec_ctc_trie_pack: V above 256");
  if (V < 2 || blank < 0 || blank >= V || sil < -1 || sil >= V || sil == blank)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: needs V >= 2, blank in [0, V), sil -1 or in [0, V) and not the blank");
  if (offsets[0] != 0) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: offsets[0] must be 0");
  for (int i = 0; i < n_words; ++i)
    if (offsets[i + 1] <= offsets[i]) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: offsets must ascend and no spelling may be empty");
  const int64_t total = offsets[n_words];
  for (int64_t k = 0; k < total; ++k)
    if (spellings[k] < 0 || spellings[k] >= V || spellings[k] == blank || spellings[k] == sil)
      return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: a token outside [0, V), or the blank or sil token, in a spelling");
  const size_t need = eec_ctc_trie_pack_bytes(n_words, total);
  if (need == 0) return fail(EEC_ERR_UNSUPPORTED, "eec_ctc_trie_pack: the image would pass 2^31 dwords");
  if (image_bytes < need) return fail(EEC_ERR_WORKSPACE, "eec_ctc_trie_pack: image_bytes below eec_ctc_trie_pack_bytes()");

  struct Node {
    std::vector<std::pair<unsigned char, int>> kids;
    int word = -1;
  };
  std::vector<Node> tn(1);
  int shadowed = 0;
  for (int wi = 0; wi < n_words; ++wi) {
    int at = 0;
    for (int64_t k = offsets[wi]; k < offsets[wi + 1]; ++k) {
      const unsigned char tok = (unsigned char)spellings[k];
      int next = -1;
      for (const auto& kid : tn[at].kids)
        if (kid.first == tok) next = kid.second;
      if (next < 0) {
        next = (int)tn.size();
        tn[at].kids.emplace_back(tok, next);
        tn.emplace_back();
      }
      at = next;
    }
    if (tn[at].word < 0)
      tn[at].word = wi;  // the first word in file order with this spelling
    else
      ++shadowed;
  }

  // breadth-first numbering, children ascending by token: the child reached by edge k is node k + 1
  const int nodes = (int)tn.size(), edges = nodes - 1;
  int32_t* img = (int32_t*)image;
  memset(img, 0, need);
  const int off_begin = kLbHeader, off_tok = off_begin + nodes + 1, off_word = off_tok + (edges + 3) / 4;
  unsigned char* tok_bytes = (unsigned char*)(img + off_tok);
  std::vector<int> order(1, 0);
  order.reserve(nodes);
  for (int id = 0; id < nodes; ++id) {
    Node& nd = tn[order[id]];
    std::sort(nd.kids.begin(), nd.kids.end());
    img[off_begin + id] = (int32_t)order.size() - 1;
    for (const auto& kid : nd.kids) {
      tok_bytes[order.size() - 1] = kid.first;
      order.push_back(kid.second);
    }
    img[off_word + id] = nd.word;
  }
  img[off_begin + nodes] = edges;
  img[0] = kLbMagic, img[1] = nodes, img[2] = edges, img[3] = V, img[4] = blank, img[5] = sil;
  img[6] = off_begin, img[7] = off_tok, img[8] = off_word, img[9] = off_word + nodes, img[10] = n_words, img[11] = shadowed;
  if (n_nodes) *n_nodes = nodes;
  if (n_shadowed) *n_shadowed = shadowed;
  return 0;
}

size_t eec_ngram_pack_bytes(int order, const int64_t* counts, int lex_words) {
  if (order < 1 || order > eec::kLmMaxOrder || !counts || lex_words <= 0 || counts[0] <= 0) return 0;
  unsigned long long nodes = 1;
  for (int n = 0; n < order; ++n) {
    if (counts[n] < 0 || counts[n] >= ((int64_t)1 << 31)) return 0;
    nodes += (unsigned long long)counts[n];
  }
  const size_t dwords = eec::lm_image_dwords(nodes, (unsigned long long)lex_words);
  return dwords >= ((size_t)1 << 31) ? 0 : dwords * 4;  // the kernel indexes the image with int32
}

int eec_ngram_pack(int order, const int64_t* counts, const int32_t* const* words, const float* const* logp, const float* const* backoff,
                   const int32_t* word_map, int lex_words, int bos_word, int eos_word, void* image, size_t image_bytes, int32_t* n_nodes) {
  using namespace eec;
  using eech::fail;
  if (order < 1 || order > kLmMaxOrder) return fail(EEC_ERR_UNSUPPORTED, "eec_ngram_pack: the order must be 1 .. " + std::to_string(kLmMaxOrder));
  if (!counts || !words || !logp || !backoff || !word_map || !image)
    return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: null argument (counts, words, logp, backoff, word_map, image)");
  if (lex_words <= 0 || counts[0] <= 0) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: needs lex_words > 0 and at least one unigram");
  for (int n = 0; n < order; ++n) {
    if (counts[n] < 0) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: a negative count");
    if (counts[n] > 0 && (!words[n] || !logp[n] || !backoff[n])) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: null array of order " + std::to_string(n + 1));
  }
  const size_t need = eec_ngram_pack_bytes(order, counts, lex_words);
  if (need == 0) return fail(EEC_ERR_UNSUPPORTED, "eec_ngram_pack: the image would pass 2^31 dwords");
  if (image_bytes < need) return fail(EEC_ERR_WORKSPACE, "eec_ngram_pack: image_bytes below eec_ngram_pack_bytes()");
  const int W = (int)counts[0];
  if (bos_word < -1 || bos_word >= W || eos_word < -1 || eos_word >= W)
    return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: bos_word and eos_word must be -1 or an LM word");
  for (int i = 0; i < lex_words; ++i)
    if (word_map[i] < 0 || word_map[i] >= W) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: word_map[" + std::to_string(i) + "] is no LM word");
  for (int n = 0; n < order; ++n)
    for (int64_t i = 0; i < counts[n]; ++i)
      if (!std::isfinite(logp[n][i]) || !std::isfinite(backoff[n][i]))
        return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: a non-finite value in " + std::to_string(n + 1) + "-gram " + std::to_string(i));

  int level[kLmMaxOrder + 2];  // level[n]: the first node of depth n; level[order + 1]: the node count
  level[0] = 0, level[1] = 1;
  for (int n = 1; n <= order; ++n) level[n + 1] = level[n] + (int)counts[n - 1];
  const int nodes = level[order + 1], edges = nodes - 1;
  int32_t* img = (int32_t*)image;
  memset(img, 0, need);
  const int off_begin = kLmHeader, off_eword = off_begin + nodes + 1, off_logp = off_eword + edges, off_backoff = off_logp + nodes,
            off_suffix = off_backoff + nodes, off_map = off_suffix + nodes;
  int32_t *begin = img + off_begin, *eword = img + off_eword, *suffix = img + off_suffix;
  float *lp = (float*)(img + off_logp), *bo = (float*)(img + off_backoff);
  for (int x = 0; x <= nodes; ++x) begin[x] = edges;  // a node without children: an empty range at its place

  // the child of `node` labelled v, or -1; the ranges of all shallower levels are final when a level is built
  auto child = [&](int node, int v) {
    if (node == 0) return v + 1;
    int lo = begin[node], hi = begin[node + 1];
    const int end = hi;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (eword[mid] < v)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo < end && eword[lo] == v ? lo + 1 : -1;
  };
  auto find = [&](const int32_t* w, int len) {  // the node of the n-gram w[0 .. len), or -1
    int at = 0;
    for (int k = 0; k < len && at >= 0; ++k) at = child(at, w[k]);
    return at;
  };

  // unigrams: LM word v is node v + 1, edge v of the root
  begin[0] = 0;
  std::vector<char> seen(W, 0);
  for (int i = 0; i < W; ++i) {
    const int v = words[0][i];
    if (v < 0 || v >= W) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: unigram " + std::to_string(i) + " is outside [0, counts[0])");
    if (seen[v]) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: unigram " + std::to_string(i) + " is a duplicate");
    seen[v] = 1;
    eword[v] = v, lp[v + 1] = logp[0][i], bo[v + 1] = backoff[0][i];
  }
  // higher orders, breadth-first: the nodes of depth n in the order of (parent, last word)
  for (int n = 2; n <= order; ++n) {
    const int64_t cnt = counts[n - 1];
    const int32_t* w = words[n - 1];
    std::vector<std::pair<std::pair<int, int>, int64_t>> ent((size_t)cnt);  // ((parent, word), index)
    for (int64_t i = 0; i < cnt; ++i) {
      for (int k = 0; k < n; ++k)
        if (w[i * n + k] < 0 || w[i * n + k] >= W)
          return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: " + std::to_string(n) + "-gram " + std::to_string(i) + " has a word outside [0, counts[0])");
      const int parent = find(w + i * n, n - 1);
      if (parent < 0) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: the prefix of " + std::to_string(n) + "-gram " + std::to_string(i) + " is absent");
      ent[(size_t)i] = {{parent, w[i * n + n - 1]}, i};
    }
    std::sort(ent.begin(), ent.end());
    for (int64_t r = 0; r < cnt; ++r) {
      if (r > 0 && ent[(size_t)r].first == ent[(size_t)r - 1].first)
        return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: " + std::to_string(n) + "-gram " + std::to_string(ent[(size_t)r].second) + " is a duplicate");
      const int x = level[n] + (int)r;
      eword[x - 1] = ent[(size_t)r].first.second;
      lp[x] = logp[n - 1][ent[(size_t)r].second], bo[x] = backoff[n - 1][ent[(size_t)r].second];
    }
    // the parents' ranges: edges level[n] - 1 .. in parent order
    int64_t r = 0;
    for (int p = level[n - 1]; p < level[n]; ++p) {
      begin[p] = level[n] - 1 + (int)r;
      while (r < cnt && ent[(size_t)r].first.first == p) ++r;
    }
    for (int x = level[n]; x <= nodes; ++x) begin[x] = level[n] - 1 + (int)cnt;
    // suffix links of this level: the longest proper suffix that is a node; the last word's unigram at worst
    for (int64_t q = 0; q < cnt; ++q) {
      const int32_t* g = w + ent[(size_t)q].second * n;
      int to = -1;
      for (int k = 1; k < n && to < 0; ++k) to = find(g + k, n - k);
      suffix[level[n] + (int)q] = to;
    }
  }
  for (int i = 0; i < lex_words; ++i) img[off_map + i] = word_map[i];
  img[0] = kLmMagic, img[1] = order, img[2] = nodes, img[3] = edges, img[4] = W, img[5] = lex_words, img[6] = bos_word + 1, img[7] = eos_word;
  img[8] = level[order], img[9] = off_begin, img[10] = off_eword, img[11] = off_logp, img[12] = off_backoff, img[13] = off_suffix;
  img[14] = off_map, img[15] = off_map + lex_words;
  if (n_nodes) *n_nodes = nodes;
  return 0;
}

size_t eec_ctc_trie_smear_bytes(int n_nodes) {
  return n_nodes >= 1 ? (((size_t)eec::kSmHeader + (size_t)n_nodes + 1) & ~(size_t)1) * 4 : 0;
}

int eec_ctc_trie_smear(const void* trie_image, const void* lm_image, void* table, size_t table_bytes) {
  using namespace eec;
  using eech::fail;
  if (!trie_image || !lm_image || !table) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: null argument (trie_image, lm_image, table)");
  if (((uintptr_t)trie_image | (uintptr_t)lm_image | (uintptr_t)table) & 7)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: trie_image, lm_image and table must be 8-byte aligned");
  const int32_t *trie = (const int32_t*)trie_image, *lm = (const int32_t*)lm_image;
  if (trie[0] != kLbMagic || trie[1] < 1) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: trie_image is no packed trie");
  if (lm[0] != kLmMagic) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: lm_image is no packed n-gram model");
  if (lm[5] != trie[10])
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: the model was packed for a lexicon of " + std::to_string(lm[5]) + " words, the trie has " +
                                     std::to_string(trie[10]));
  const int nodes = trie[1];
  if (table_bytes < eec_ctc_trie_smear_bytes(nodes)) return fail(EEC_ERR_WORKSPACE, "eec_ctc_trie_smear: table_bytes below eec_ctc_trie_smear_bytes()");
  const int32_t *cbeg = trie + trie[6], *word_of = trie + trie[8];
  const LmView m = lm_view(lm);
  int32_t* tab = (int32_t*)table;
  memset(tab, 0, eec_ctc_trie_smear_bytes(nodes));
  float* smax = (float*)(tab + kSmHeader);
  // children have higher numbers than their parent (the child of edge k is node k + 1): one descending sweep
  for (int n = nodes - 1; n >= 1; --n) {
    float best = -INFINITY;
    const int word = word_of[n];
    if (word >= lm[5]) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: node " + std::to_string(n) + " ends a word outside the lexicon");
    if (word >= 0) {
      int next;
      best = lm_walk(m, m.bos, m.map[word], next);  // u(word): the walk from the start state
    }
    if (cbeg[n] < n || cbeg[n + 1] > nodes - 1 || cbeg[n + 1] < cbeg[n])
      return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: node " + std::to_string(n) + " has children that are not below it");
    for (int k = cbeg[n]; k < cbeg[n + 1]; ++k) best = std::max(best, smax[k + 1]);
    if (!std::isfinite(best)) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: node " + std::to_string(n) + " neither ends a word nor has children, or a model value is not finite");
    smax[n] = best;
  }
  smax[0] = 0.f;
  tab[0] = kSmMagic, tab[1] = nodes, tab[2] = trie[10], tab[3] = 0;
  return 0;
}

}  // extern "C"
