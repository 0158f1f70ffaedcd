// Stand-alone host check of the context-graph builder (eec_context_graph, csrc/ctx_graph.hip), meant to be built with the host
// sanitizers; it makes no device call.  Builds images into exactly sized heap buffers (a write past the end is caught), walks each by
// the documented layout -- header, records, offsets in sequence -- and checks the tables against a naive restatement that knows no
// trie: the state after a token row is the longest suffix of the row that is a prefix of a phrase, node_score the sum of the largest
// boosts over the phrases sharing each of its prefixes, and what a transition pays is the change of the open bonus plus every phrase
// that ends at the new position.  Then the refusals.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         early_exit_transformer_amd/csrc/ctx_graph.hip tools/context_graph_check.cpp -o context_graph_check && ./context_graph_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../include/eec.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

typedef std::vector<int> Row;

static uint32_t g_state = 2024u;
static int draw(int m) {  // a small generator of its own: [0, m)
  g_state = g_state * 1664525u + 1013904223u;
  return (int)((g_state >> 8) % (uint32_t)m);
}

struct Graph {
  std::vector<Row> phrases;
  std::vector<double> boosts;
};

static bool is_prefix(const Row& p, const Row& of) { return p.size() <= of.size() && std::equal(p.begin(), p.end(), of.begin()); }

// node_score of the trie node spelled by `path` (which is a prefix of a phrase): per prefix the largest boost among the phrases through it
static double node_score(const Graph& g, const Row& path) {
  double total = 0.0;
  for (size_t k = 1; k <= path.size(); ++k) {
    const Row head(path.begin(), path.begin() + k);
    double best = 0.0;
    for (size_t p = 0; p < g.phrases.size(); ++p)
      if (is_prefix(head, g.phrases[p]) && g.boosts[p] > best) best = g.boosts[p];
    total = total + best;
  }
  return total;
}

// the longest suffix of `row` that is a prefix of a phrase
static Row open_match(const Graph& g, const Row& row) {
  for (size_t cut = 0; cut <= row.size(); ++cut) {
    const Row tail(row.begin() + cut, row.end());
    for (const Row& p : g.phrases)
      if (is_prefix(tail, p)) return tail;
  }
  return Row();
}

// the sum of node_score over the phrases that end where `row` ends (a phrase given twice counts once), added from the shortest up:
// the order of out(n) = (end(n) ? node_score(n) : 0) + out(fail(n))
static double ending_here(const Graph& g, const Row& row) {
  double total = 0.0;
  for (size_t len = 1; len <= row.size(); ++len) {
    const Row tail(row.end() - len, row.end());
    if (std::find(g.phrases.begin(), g.phrases.end(), tail) != g.phrases.end()) total = node_score(g, tail) + total;
  }
  return total;
}

static int walk(const std::vector<Graph>& graphs, int V, int blank, int eos, int pad, size_t* bytes_out, long long* states_out) {
  const int G = (int)graphs.size();
  std::vector<int32_t> n_phrases, lens, toks;
  std::vector<double> boosts;
  for (const Graph& g : graphs) {
    n_phrases.push_back((int32_t)g.phrases.size());
    for (size_t p = 0; p < g.phrases.size(); ++p) {
      lens.push_back((int32_t)g.phrases[p].size());
      toks.insert(toks.end(), g.phrases[p].begin(), g.phrases[p].end());
      boosts.push_back(g.boosts[p]);
    }
  }
  const size_t need = eec_context_graph_bytes(G, n_phrases.data(), lens.data(), toks.data(), boosts.data(), V, blank, eos, pad);
  CHECK(need > 0 && need % 4 == 0);
  std::vector<int32_t>* image = new std::vector<int32_t>(need / 4);  // exactly sized
  CHECK(eec_context_graph(G, n_phrases.data(), lens.data(), toks.data(), boosts.data(), V, blank, eos, pad, image->data(), need) == 0);
  const int32_t* img = image->data();
  CHECK(img[0] == EEC_CTX_MAGIC && img[1] == G && (size_t)img[2] == need / 4 && img[3] == V);
  const bool closing = eos >= 0 || pad >= 0;
  size_t at = 4 + 4 * (size_t)G;
  for (int gi = 0; gi < G; ++gi) {
    const Graph& g = graphs[gi];
    const int32_t* rec = img + 4 + 4 * gi;
    const int S = rec[0], N = S - (closing ? 1 : 0);
    CHECK(S >= 1 && (size_t)rec[1] == at && (size_t)rec[2] == at + (size_t)S * V && (size_t)rec[3] == at + 2 * (size_t)S * V);
    const float* delta = (const float*)(img + rec[1]);
    const int32_t* next = img + rec[2];
    const float* fin = (const float*)(img + rec[3]);
    // the path of every state, breadth first from the root along the tree edges (an edge grows the path by its token)
    std::map<Row, int> id;
    std::vector<Row> path(N);
    std::vector<char> known(N, 0);
    id[Row()] = 0, known[0] = 1;
    std::vector<int> order(1, 0);
    for (size_t q = 0; q < order.size(); ++q) {
      const int s = order[q];
      for (int t = 0; t < V; ++t) {
        if (t == blank || t == eos || t == pad) continue;
        Row grown = path[s];
        grown.push_back(t);
        const int d = next[(size_t)s * V + t];
        CHECK(d >= 0 && d < N);
        if (open_match(g, grown) == grown) {  // a tree edge
          CHECK(!known[d]);
          known[d] = 1, path[d] = grown, id[grown] = d;
          order.push_back(d);
        }
      }
    }
    CHECK((int)order.size() == N);  // every state is a prefix of a phrase, each one once
    for (int s = 0; s < N; ++s) {
      const double here = node_score(g, path[s]);
      CHECK(fin[s] == (float)(0.0 - here));
      for (int t = 0; t < V; ++t) {
        const size_t k = (size_t)s * V + t;
        if (t == blank) {
          CHECK(next[k] == s && delta[k] == 0.0f);
        } else if (t == eos || t == pad) {
          CHECK(next[k] == N && delta[k] == (float)(0.0 - here));
        } else {
          Row grown = path[s];
          grown.push_back(t);
          const Row open = open_match(g, grown);
          CHECK(id.count(open) && next[k] == id[open]);
          CHECK(delta[k] == (float)((node_score(g, open) - here) + ending_here(g, grown)));
        }
      }
    }
    if (closing) {
      CHECK(fin[N] == 0.0f);
      for (int t = 0; t < V; ++t) CHECK(next[(size_t)N * V + t] == N && delta[(size_t)N * V + t] == 0.0f);
    }
    at += (size_t)S * (2 * V + 1);
    *states_out += S;
  }
  CHECK(at == need / 4);
  // one byte short: refused, nothing written
  std::vector<int32_t>* small = new std::vector<int32_t>(need / 4, 0x5a5a5a5a);
  CHECK(eec_context_graph(G, n_phrases.data(), lens.data(), toks.data(), boosts.data(), V, blank, eos, pad, small->data(), need - 1) == EEC_ERR_WORKSPACE);
  for (int32_t v : *small) CHECK(v == 0x5a5a5a5a);
  delete small;
  delete image;
  *bytes_out = need;
  return 0;
}

static Graph random_graph(int P, int V, int lo, int max_len, bool dyadic) {
  Graph g;
  for (int p = 0; p < P; ++p) {
    Row row(1 + draw(max_len));
    for (int& t : row) t = lo + draw(V - lo);
    g.phrases.push_back(row);
    g.boosts.push_back(dyadic ? 0.25 * draw(17) : 0.1 * (1 + draw(40)));
  }
  return g;
}

int main() {
  size_t bytes[8] = {0};
  long long states = 0;
  int at = 0;
  // a small alphabet: nested and overlapping phrases, shared prefixes, duplicates
  Graph hand;
  hand.phrases = {{1, 2, 1}, {2, 1}, {1, 2, 1, 3}, {3, 3}, {1}, {2, 1, 3, 3, 2}, {1, 2, 1}, {3, 1, 2}};
  hand.boosts = {1.5, 0.75, 4.0, 2.0, 0.5, 1.25, 0.1, 0.3};
  if (walk({hand}, 5, 0, -1, -1, &bytes[at++], &states)) return 1;
  if (walk({hand}, 7, 0, 5, 6, &bytes[at++], &states)) return 1;
  if (walk({hand}, 6, 4, 5, -1, &bytes[at++], &states)) return 1;
  // random graphs over 4, 32 and 256 tokens, an empty graph among them, as one bank each
  if (walk({random_graph(12, 4, 1, 5, true), Graph(), random_graph(30, 4, 1, 6, false)}, 4, 0, -1, -1, &bytes[at++], &states)) return 1;
  if (walk({random_graph(40, 32, 3, 5, false), random_graph(5, 32, 3, 8, true)}, 32, 0, 1, 2, &bytes[at++], &states)) return 1;
  if (walk({random_graph(60, 256, 3, 4, false)}, 256, 0, 1, 2, &bytes[at++], &states)) return 1;
  Graph longest;
  longest.phrases = {Row(EEC_CTX_MAX_PHRASE, 3)};  // the limit of the length: 64 equal tokens (every suffix is a prefix)
  longest.boosts = {0.7};
  if (walk({longest}, 5, 0, -1, 4, &bytes[at++], &states)) return 1;
  if (walk(std::vector<Graph>(EEC_CTX_MAX_GRAPHS), 3, 0, -1, -1, &bytes[at++], &states)) return 1;  // the limit of the count: empty graphs

  // the refusals (their messages are the tests' business: the error string's accessor lives in another file of the library)
  int32_t buf[512];
  const int32_t one[1] = {1}, three[1] = {3}, none[1] = {0}, over[1] = {EEC_CTX_MAX_PHRASE + 1}, neg[1] = {-1};
  const int32_t ok[3] = {3, 4, 5}, with_blank[3] = {3, 0, 5}, outside[3] = {3, 8, 5}, below[3] = {-1, 4, 5};
  int32_t longrow[EEC_CTX_MAX_PHRASE + 1];
  for (int& t : longrow) t = 2;
  const double b[1] = {1.5}, nan_[1] = {NAN}, inf_[1] = {INFINITY}, minus[1] = {-0.5}, huge[1] = {1e300};
  struct {
    int G;
    const int32_t *n, *len, *tok;
    const double* boost;
    int V, blank, eos, pad;
  } bad[] = {{0, one, three, ok, b, 8, 0, -1, -1},        {EEC_CTX_MAX_GRAPHS + 1, one, three, ok, b, 8, 0, -1, -1},
             {1, nullptr, three, ok, b, 8, 0, -1, -1},    {1, one, nullptr, ok, b, 8, 0, -1, -1},
             {1, one, three, nullptr, b, 8, 0, -1, -1},   {1, one, three, ok, nullptr, 8, 0, -1, -1},
             {1, neg, three, ok, b, 8, 0, -1, -1},        {1, one, none, ok, b, 8, 0, -1, -1},
             {1, one, over, longrow, b, 8, 0, -1, -1},    {1, one, three, with_blank, b, 8, 0, -1, -1},
             {1, one, three, outside, b, 8, 0, -1, -1},   {1, one, three, below, b, 8, 0, -1, -1},
             {1, one, three, ok, nan_, 8, 0, -1, -1},     {1, one, three, ok, inf_, 8, 0, -1, -1},
             {1, one, three, ok, minus, 8, 0, -1, -1},    {1, one, three, ok, huge, 8, 0, -1, -1},
             {1, one, three, ok, b, 0, 0, -1, -1},        {1, one, three, ok, b, 257, 0, -1, -1},
             {1, one, three, ok, b, 8, 8, -1, -1},        {1, one, three, ok, b, 8, 0, 4, -1},
             {1, one, three, ok, b, 8, 0, -1, 5},         {1, one, three, ok, b, 8, 0, 0, -1},
             {1, one, three, ok, b, 8, 0, 8, -1},         {1, one, three, ok, b, 8, 0, -1, -2}};
  for (const auto& k : bad) {
    CHECK(eec_context_graph_bytes(k.G, k.n, k.len, k.tok, k.boost, k.V, k.blank, k.eos, k.pad) == 0);
    CHECK(eec_context_graph(k.G, k.n, k.len, k.tok, k.boost, k.V, k.blank, k.eos, k.pad, buf, sizeof buf) == EEC_ERR_BAD_ARG);
  }
  CHECK(eec_context_graph(1, one, three, ok, b, 8, 0, -1, -1, nullptr, 4096) == EEC_ERR_BAD_ARG);
  // more states than the limit: 1000 phrases of 40 tokens that share nothing
  {
    std::vector<int32_t> n(1, 1000), len(1000, 40), tok(40000);
    std::vector<double> boost(1000, 1.0);
    for (int p = 0; p < 1000; ++p)
      for (int k = 0; k < 40; ++k) tok[p * 40 + k] = 1 + (k == 0 ? p % 200 : k == 1 ? p / 200 : (p + k) % 200);
    CHECK(eec_context_graph_bytes(1, n.data(), len.data(), tok.data(), boost.data(), 256, 0, -1, -1) == 0);
  }
  // the device entries refuse before any device work
  CHECK(eec_context_bias_step(nullptr, 0, nullptr, 1, 1, 1, 4, 7, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_context_bias_step(nullptr, 0, nullptr, 1, 5, 1, 4, 7, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == EEC_ERR_BAD_ARG);
  CHECK(eec_context_bias_step(nullptr, 0, nullptr, 0, 1, 1, 4, 7, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0);
  CHECK(eec_context_bias_state_bytes(3, 16) == 2 * 3 * 16 * sizeof(int32_t));
  printf("context_graph_check: images of %zu .. %zu bytes (%lld states) walked against the naive restatement, refusals ok\n", bytes[0], bytes[5],
         states);
  return 0;
}
