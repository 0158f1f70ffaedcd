// Stand-alone host check of the smear table (eec_ctc_trie_smear, csrc/lexpack.hip), meant to be built with the host sanitizers;
// it makes no device call.  Generates a lexicon (argv[1]: words, default 3000; duplicates and words that are prefixes of words
// included) and a prefix-closed model of order 3 with <s> from a seed, packs both, computes the table into an exactly sized heap
// buffer, and recomputes smax by brute force over the words: u(w) by a back-off walk written here against the documented image
// layout, then for every prefix of every first spelling the maximum.  Then the entry's error cases.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/lexpack.hip tools/trie_smear_check.cpp -o trie_smear_check
//   ./trie_smear_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <vector>

#include "../include/eec.h"

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      return 1;                                                             \
    }                                                                       \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

int main(int argc, char** argv) {
  const int n_words = argc > 1 ? atoi(argv[1]) : 3000, V = 64, blank = 0, sil = 63, order = 3;
  CHECK(n_words >= 100);
  // the lexicon: tokens 1 .. 20, lengths 1 .. 6; every tenth word repeats an earlier spelling (shadowed)
  typedef std::vector<int32_t> Spelling;
  std::vector<Spelling> spell(n_words);
  std::vector<int32_t> flat;
  std::vector<int64_t> offsets(1, 0);
  for (int w = 0; w < n_words; ++w) {
    if (w >= 10 && w % 10 == 0)
      spell[w] = spell[rnd((uint32_t)w)];
    else
      for (int k = 1 + (int)rnd(6); k > 0; --k) spell[w].push_back(1 + (int32_t)rnd(20));
    flat.insert(flat.end(), spell[w].begin(), spell[w].end());
    offsets.push_back((int64_t)flat.size());
  }
  const size_t trie_bytes = eec_ctc_trie_pack_bytes(n_words, offsets.back());
  CHECK(trie_bytes > 0);
  std::unique_ptr<int32_t[]> trie(new int32_t[trie_bytes / 4]);
  int32_t n_nodes = 0, n_shadowed = 0;
  CHECK(eec_ctc_trie_pack(flat.data(), offsets.data(), n_words, V, blank, sil, trie.get(), trie_bytes, &n_nodes, &n_shadowed) == 0);
  CHECK(n_shadowed > 0);

  // the model: LM words 0 .. W - 1 = the lexicon's first n_words - 7 words, then <unk>, <s>; the last seven lexicon words are unknown
  const int W = n_words - 7 + 2, unk = W - 2, bos = W - 1;
  typedef std::vector<int32_t> Gram;
  std::map<Gram, std::pair<float, float>> model;
  std::vector<std::vector<int32_t>> words(order);
  std::vector<std::vector<float>> logp(order), backoff(order);
  auto add = [&](const Gram& g) {
    if (model.count(g)) return;
    const float lp = -0.0625f * (float)(1 + rnd(90)), bo = g.size() == (size_t)order ? 0.f : 0.125f * (float)rnd(12) - 1.f;  // some back-offs positive
    model[g] = {lp, bo};
    words[g.size() - 1].insert(words[g.size() - 1].end(), g.begin(), g.end());
    logp[g.size() - 1].push_back(lp);
    backoff[g.size() - 1].push_back(bo);
  };
  for (int v = 0; v < W; ++v) add(Gram{v});
  for (int k = 0; k < n_words / 3; ++k) add(Gram{bos, (int32_t)rnd((uint32_t)W - 1)});  // what follows <s>: the walk's first step hits or backs off
  for (int k = 0; k < n_words / 3; ++k) {
    const int32_t a = (int32_t)rnd((uint32_t)W - 1), b = (int32_t)rnd((uint32_t)W - 1);
    add(Gram{a, b});
    add(Gram{a, b, (int32_t)rnd((uint32_t)W - 1)});
  }
  std::vector<int64_t> counts(order);
  const int32_t* wp[5] = {};
  const float *lp[5] = {}, *bp[5] = {};
  for (int n = 0; n < order; ++n) counts[n] = (int64_t)logp[n].size(), wp[n] = words[n].data(), lp[n] = logp[n].data(), bp[n] = backoff[n].data();
  std::vector<int32_t> word_map(n_words);
  for (int i = 0; i < n_words; ++i) word_map[i] = i < n_words - 7 ? i : unk;
  const size_t lm_bytes = eec_ngram_pack_bytes(order, counts.data(), n_words);
  CHECK(lm_bytes > 0);
  std::unique_ptr<int32_t[]> lm(new int32_t[lm_bytes / 4]);
  CHECK(eec_ngram_pack(order, counts.data(), wp, lp, bp, word_map.data(), n_words, bos, -1, lm.get(), lm_bytes, nullptr) == 0);

  // the table, into an exactly sized buffer: a write past the end is the sanitizer's to find
  const size_t need = eec_ctc_trie_smear_bytes(n_nodes);
  CHECK(need == (size_t)(4 + n_nodes + ((4 + n_nodes) & 1)) * 4 && need % 8 == 0);
  std::unique_ptr<int32_t[]> table(new int32_t[need / 4]);
  memset(table.get(), 0x5A, need);
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), table.get(), need) == 0);
  const int32_t* tab = table.get();
  CHECK(tab[0] == 0x53434545 && tab[1] == n_nodes && tab[2] == n_words && tab[3] == 0);
  if ((4 + n_nodes) & 1) CHECK(tab[4 + n_nodes] == 0);
  const float* smax = (const float*)(tab + 4);
  CHECK(smax[0] == 0.f && !signbit(smax[0]));

  // u(w) from <s> by the definition: the longest context first, a context that is an n-gram and lacks the word adds its back-off
  auto u = [&](int32_t v) {
    float acc = 0.f;
    Gram ctx{bos};
    for (;;) {
      Gram g = ctx;
      g.push_back(v);
      auto hit = model.find(g);
      if (hit != model.end()) return acc + hit->second.first;
      if (model.count(ctx)) acc = acc + model[ctx].second;
      ctx.erase(ctx.begin());
    }
  };
  std::map<Spelling, int> first;
  for (int w = 0; w < n_words; ++w) first.insert({spell[w], w});
  std::map<Spelling, float> brute;
  int backed_off = 0;
  for (const auto& kv : first) {
    const float score = u(word_map[kv.second]);
    backed_off += !model.count(Gram{bos, word_map[kv.second]});
    for (size_t k = 1; k <= kv.first.size(); ++k) {
      const Spelling prefix(kv.first.begin(), kv.first.begin() + (long)k);
      auto at = brute.find(prefix);
      if (at == brute.end())
        brute[prefix] = score;
      else if (score > at->second)
        at->second = score;
    }
  }
  CHECK(backed_off > 0 && backed_off < (int)first.size());
  CHECK((int)brute.size() == n_nodes - 1);
  const int32_t* cbeg = trie.get() + trie[6];
  const unsigned char* ctok = (const unsigned char*)(trie.get() + trie[7]);
  int inner_above_own_word = 0;
  for (const auto& kv : brute) {
    int at = 0;
    for (int32_t t : kv.first) {
      int next = -1;
      for (int e = cbeg[at]; e < cbeg[at + 1]; ++e)
        if (ctok[e] == t) next = e + 1;
      CHECK(next > at);
      at = next;
    }
    CHECK(memcmp(&smax[at], &kv.second, 4) == 0);
    const auto own = first.find(kv.first);
    if (own != first.end() && u(word_map[own->second]) < kv.second) ++inner_above_own_word;
  }
  CHECK(inner_above_own_word > 0);  // a word that is a prefix of a better word carries the better word's score

  // the error cases (include/eec.h)
  CHECK(eec_ctc_trie_smear_bytes(0) == 0 && eec_ctc_trie_smear_bytes(-1) == 0 && eec_ctc_trie_smear_bytes(1) == 24 && eec_ctc_trie_smear_bytes(2) == 24);
  CHECK(eec_ctc_trie_smear(nullptr, lm.get(), table.get(), need) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_smear(trie.get(), nullptr, table.get(), need) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), nullptr, need) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), table.get() + 1, need) == EEC_ERR_BAD_ARG);  // misaligned
  CHECK(eec_ctc_trie_smear(lm.get(), lm.get(), table.get(), need) == EEC_ERR_BAD_ARG);        // wrong magics
  CHECK(eec_ctc_trie_smear(trie.get(), trie.get(), table.get(), need) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), table.get(), need - 1) == EEC_ERR_WORKSPACE);
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), table.get(), 0) == EEC_ERR_WORKSPACE);
  lm[5] = n_words - 1;  // a model packed for another lexicon
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), table.get(), need) == EEC_ERR_BAD_ARG);
  lm[5] = n_words;
  CHECK(eec_ctc_trie_smear(trie.get(), lm.get(), table.get(), need) == 0);
  printf("trie_smear_check: %d words (%d shadowed), %d nodes, model of order %d with %lld / %lld / %lld n-grams, %d of %zu first words back off from <s>, "
         "%d inner word nodes carry a longer word's score, table %zu bytes, error cases ok\n", n_words, n_shadowed, n_nodes, order, (long long)counts[0],
         (long long)counts[1], (long long)counts[2], backed_off, first.size(), inner_above_own_word, need);
  return 0;
}
