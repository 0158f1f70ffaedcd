// Stand-alone host check of the trie packer (eec_ctc_trie_pack, csrc/lexpack.hip), meant to be built with the host
// sanitizers; it makes no device call.  Reads a lexicon as text -- first line "n_words V blank sil", then one spelling per line
// as token ids --, packs it into an exactly sized heap buffer, walks the image by the documented layout (every spelling must lead
// to the first word that has it), and runs the packer's error cases.  (The two kernel files are on the line for the decoder's
// workspace size function, which the program also checks.)
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/lexpack.hip early_exit_transformer_amd/csrc/ctc_lexbeam.hip \
//         early_exit_transformer_amd/csrc/ctc_lexbeam_wide.hip tools/trie_pack_check.cpp -o trie_pack_check
//   python -c "import sys; sys.path.insert(0, 'tests'); import lexbeam_cases as L; t, w, s = L.load_fixture(); \
//              print(len(s), 256, 0, 126); [print(*x) for x in s]" | ./trie_pack_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <sstream>
#include <iostream>
#include <string>
#include <vector>

#include "../include/eec.h"

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      return 1;                                                             \
    }                                                                       \
  } while (0)

int main() {
  int n_words = 0, V = 0, blank = 0, sil = -1;
  std::string line;
  CHECK(std::getline(std::cin, line));
  CHECK(sscanf(line.c_str(), "%d %d %d %d", &n_words, &V, &blank, &sil) == 4 && n_words > 0);
  std::vector<int32_t> flat;
  std::vector<int64_t> off(1, 0);
  while ((int)off.size() <= n_words && std::getline(std::cin, line)) {
    std::istringstream in(line);
    for (int t; in >> t;) flat.push_back(t);
    off.push_back((int64_t)flat.size());
  }
  CHECK((int)off.size() == n_words + 1);

  const size_t need = eec_ctc_trie_pack_bytes(n_words, off.back());
  CHECK(need > 0 && need % 8 == 0);
  std::vector<int32_t>* image = new std::vector<int32_t>(need / 4);  // exactly sized: a write past the end is caught
  int32_t nodes = -1, shadowed = -1;
  CHECK(eec_ctc_trie_pack(flat.data(), off.data(), n_words, V, blank, sil, image->data(), need, &nodes, &shadowed) == 0);
  const int32_t* img = image->data();
  CHECK(img[1] == nodes && img[2] == nodes - 1 && img[3] == V && img[4] == blank && img[5] == sil && img[9] * 4 <= (int64_t)need);
  const int32_t* begin = img + img[6];
  const unsigned char* tok = (const unsigned char*)(img + img[7]);
  const int32_t* word_of = img + img[8];
  std::map<std::vector<int32_t>, int> first;
  int dup = 0;
  for (int w = 0; w < n_words; ++w) {
    std::vector<int32_t> sp(flat.begin() + off[w], flat.begin() + off[w + 1]);
    if (!first.emplace(sp, w).second) ++dup;
    int node = 0;
    for (int32_t t : sp) {
      int k = begin[node];
      while (k < begin[node + 1] && tok[k] != t) ++k;
      CHECK(k < begin[node + 1]);
      node = k + 1;  // breadth-first numbering
      CHECK(node < nodes);
    }
    CHECK(word_of[node] == first[sp]);
  }
  CHECK(dup == shadowed);

  // the error cases
  int32_t three[] = {1, 2, 3}, with_blank[] = {1, 0, 3}, too_big[] = {1, 300, 3};
  int64_t o2[] = {0, 1, 3}, empty[] = {0, 0, 3}, down[] = {0, 3, 2}, late[] = {1, 2, 3};
  std::vector<int32_t> small(eec_ctc_trie_pack_bytes(2, 3) / 4);
  const size_t sb = small.size() * 4;
  CHECK(eec_ctc_trie_pack(three, o2, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == 0);
  CHECK(eec_ctc_trie_pack(nullptr, o2, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, nullptr, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, o2, 2, 8, 0, -1, nullptr, sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, o2, 0, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, empty, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, down, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, late, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(with_blank, o2, 2, 8, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, o2, 2, 8, 0, 3, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(three, o2, 2, 3, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_ctc_trie_pack(too_big, o2, 2, 301, 0, -1, small.data(), sb, nullptr, nullptr) == EEC_ERR_UNSUPPORTED);
  CHECK(eec_ctc_trie_pack(three, o2, 2, 8, 0, -1, small.data(), sb - 1, nullptr, nullptr) == EEC_ERR_WORKSPACE);
  CHECK(eec_ctc_lexbeam_workspace_bytes(3, 7, 10) == 3 * 7 * 10 * 8);
  printf("trie_pack_check: %d words, %d nodes, %d shadowed, image %d of %zu bytes, error cases ok\n", n_words, nodes, shadowed, 4 * img[9], need);
  delete image;
  return 0;
}
