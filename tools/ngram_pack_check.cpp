// Stand-alone host check of the n-gram packer (eec_ngram_pack, csrc/lexpack.hip), meant to be built with the host sanitizers;
// it makes no device call.  Generates a prefix-closed, not suffix-closed model of order 4 from a seed (argv[1]: words, default
// 2000), packs it into an exactly sized heap buffer, walks the image by the documented layout -- every generated n-gram must be
// found with its values, every suffix link must be the longest suffix that is a node --, and runs the packer's error cases.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/lexpack.hip tools/ngram_pack_check.cpp -o ngram_pack_check
//   ./ngram_pack_check
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
  const int W = argc > 1 ? atoi(argv[1]) : 2000, order = 4, lex_words = W + 7;
  CHECK(W >= 400);
  typedef std::vector<int32_t> Gram;
  std::map<Gram, std::pair<float, float>> model;  // every n-gram -> (logp, backoff)
  std::vector<std::vector<int32_t>> words(order);
  std::vector<std::vector<float>> logp(order), backoff(order);
  auto add = [&](const Gram& g) {
    if (model.count(g)) return;
    const float lp = -0.125f * (float)(1 + rnd(40)), bo = g.size() == (size_t)order ? 0.f : 0.125f * (float)rnd(9) - 1.f;
    model[g] = {lp, bo};
    words[g.size() - 1].insert(words[g.size() - 1].end(), g.begin(), g.end());
    logp[g.size() - 1].push_back(lp);
    backoff[g.size() - 1].push_back(bo);
  };
  for (int v = W - 1; v >= 0; --v) add(Gram{v});  // unigrams in descending order: the packer must not rely on theirs
  for (int n = 2; n <= order; ++n) {
    std::vector<Gram> ctx;
    for (const auto& kv : model)
      if ((int)kv.first.size() == n - 1) ctx.push_back(kv.first);
    for (int k = 0; k < 3 * W / 4; ++k) {
      Gram g = ctx[rnd((uint32_t)ctx.size())];
      const int deg = (n == 2 && k == 0) ? 300 : 1 + (int)rnd(4);  // one context with more than 256 children
      for (int d = 0; d < deg; ++d) {
        Gram h = g;
        h.push_back((int32_t)rnd((uint32_t)W));
        add(h);
      }
    }
  }
  std::vector<int64_t> counts(order);
  const int32_t* wp[5] = {};
  const float *lp[5] = {}, *bp[5] = {};
  for (int n = 0; n < order; ++n) counts[n] = (int64_t)logp[n].size(), wp[n] = words[n].data(), lp[n] = logp[n].data(), bp[n] = backoff[n].data();
  std::vector<int32_t> word_map(lex_words);
  for (int i = 0; i < lex_words; ++i) word_map[i] = i < W ? i : 0;  // the last seven lexicon words are unknown to the model

  const size_t need = eec_ngram_pack_bytes(order, counts.data(), lex_words);
  CHECK(need > 0 && need % 8 == 0);
  std::unique_ptr<int32_t[]> image(new int32_t[need / 4]);  // exactly sized: a write past the end is the sanitizer's to find
  int32_t nodes = 0;
  CHECK(eec_ngram_pack(order, counts.data(), wp, lp, bp, word_map.data(), lex_words, 1, 2, image.get(), need, &nodes) == 0);
  const int32_t* img = image.get();
  CHECK(img[0] == 0x4E434545 && img[1] == order && img[2] == nodes && nodes == 1 + (int)model.size() && img[3] == nodes - 1);
  CHECK(img[4] == W && img[5] == lex_words && img[6] == 2 && img[7] == 2 && (size_t)img[15] * 4 <= need);
  const int32_t *begin = img + img[9], *eword = img + img[10], *suffix = img + img[13], *map = img + img[14];
  const float *flp = (const float*)(img + img[11]), *fbo = (const float*)(img + img[12]);
  auto find = [&](const Gram& g, size_t from) {
    int at = 0;
    for (size_t k = from; k < g.size() && at >= 0; ++k) {
      int next = -1;
      for (int e = begin[at]; e < begin[at + 1]; ++e)
        if (eword[e] == g[k]) next = e + 1;
      if (at == 0) next = g[k] + 1;
      at = next;
    }
    return at;
  };
  int skipping = 0;
  for (const auto& kv : model) {
    const Gram& g = kv.first;
    const int x = find(g, 0);
    CHECK(x > 0 && x < nodes && flp[x] == kv.second.first && fbo[x] == kv.second.second);
    CHECK(((int)g.size() == order) == (x >= img[8]));
    int want = 0;
    for (size_t k = 1; k < g.size() && want <= 0; ++k) {
      want = find(g, k);
      if (want <= 0 && k + 1 < g.size()) ++skipping;
    }
    CHECK(suffix[x] == (want > 0 ? want : 0));
  }
  CHECK(skipping > 0);
  for (int x = 0; x < nodes; ++x) {
    CHECK(begin[x] <= begin[x + 1]);
    for (int e = begin[x] + 1; e < begin[x + 1]; ++e) CHECK(eword[e - 1] < eword[e]);
  }
  CHECK(begin[0] == 0 && begin[1] == W && begin[nodes] == nodes - 1);
  for (int i = 0; i < lex_words; ++i) CHECK(map[i] == word_map[i]);

  // the error cases (include/eec.h), on a model of two words
  const int64_t c2[2] = {2, 1}, neg[2] = {2, -1};
  const int32_t u[2] = {0, 1}, dup_u[2] = {1, 1}, b[2] = {0, 1}, far[2] = {0, 2};
  const float v1[2] = {-1.f, -2.f}, v2[1] = {-0.5f}, inf1[2] = {-1.f, -INFINITY};
  const int32_t wm[1] = {1}, wm_bad[1] = {2};
  const int32_t *w_ok[2] = {u, b}, *w_dup[2] = {dup_u, b}, *w_far[2] = {u, far}, *w_null[2] = {u, nullptr};
  const float *l_ok[2] = {v1, v2}, *l_inf[2] = {inf1, v2};
  const size_t sb = eec_ngram_pack_bytes(2, c2, 1);
  std::vector<int32_t> small(sb / 4);
  CHECK(sb > 0 && eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == 0);
  CHECK(eec_ngram_pack(2, nullptr, w_ok, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, nullptr, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, nullptr, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, wm, 1, -1, -1, nullptr, sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_null, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, neg, w_ok, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_dup, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_far, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_inf, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, wm_bad, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, wm, 1, 2, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, wm, 0, -1, -1, small.data(), sb, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ngram_pack(6, c2, w_ok, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb, nullptr) == EEC_ERR_UNSUPPORTED);
  CHECK(eec_ngram_pack(2, c2, w_ok, l_ok, l_ok, wm, 1, -1, -1, small.data(), sb - 1, nullptr) == EEC_ERR_WORKSPACE);
  CHECK(eec_ngram_pack_bytes(0, c2, 1) == 0 && eec_ngram_pack_bytes(2, nullptr, 1) == 0 && eec_ngram_pack_bytes(2, neg, 1) == 0);
  printf("ngram_pack_check: order %d, %d words, %d nodes (%lld / %lld / %lld / %lld n-grams), %d suffix links skip an order, image %d of %zu bytes, "
         "error cases ok\n", order, W, nodes, (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3], skipping,
         4 * img[15], need);
  return 0;
}
