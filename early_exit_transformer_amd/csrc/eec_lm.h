// Shallow fusion with a token-level n-gram model (include/eec.h, "Shallow fusion"): how a kernel reads a packed n-gram image it does
// not trust, and the one statement of the per-token increment.  Shared by the fused compile of ctc_beam.hip (ctc_beam_lm.hip) and by
// the AED step kernel of lm_fusion.hip.  The walk is lm_walk of eec_lexbeam.h -- the same loads, the same fp32 additions in the same
// order -- with every index it takes from the image brought back into its section first, so that a damaged image is never used as
// an address outside itself.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/eec.h"
#include "eec_lexbeam.h"

namespace eec {

constexpr int kTlmMaxWords = 512;  // LM words of a token-level model: the pieces and <s>, </s>, <unk> (V <= 256)
constexpr int kTlmDead = -1;       // the state of a row after its EOS
constexpr int kTlmChain = kLmMaxOrder + 1;

struct TlmView {
  LmView m;
  int n_nodes, n_edges, W;  // on == false: fusion is off for the call
  bool on;
};

// The model behind `lm`, an array of `words` int32 words, for a vocabulary of V tokens; off when there is no image, the magic is
// wrong, header word 5 is not V or a section does not lie inside the image.  Uniform loads: every work-item gets the same answer.
__device__ __forceinline__ TlmView tlm_view(const int* __restrict__ lm, long long words, int V) {
  TlmView t;
  t.on = false;
  t.n_nodes = 1, t.n_edges = 0, t.W = 0;
  t.m = LmView{};
  if (!lm || words < kLmHeader) return t;
  if (lm[0] != kLmMagic || lm[5] != V) return t;
  const long long order = lm[1], n_nodes = lm[2], n_edges = lm[3], W = lm[4], total = lm[15];
  if (order < 1 || order > kLmMaxOrder || n_nodes < 2 || n_edges != n_nodes - 1 || W < 1 || W > kTlmMaxWords || W > n_edges) return t;
  if (total > words || lm[6] < 0 || lm[6] >= n_nodes || lm[7] < -1 || lm[7] >= W) return t;
  const long long len[6] = {n_nodes + 1, n_edges, n_nodes, n_nodes, n_nodes, (long long)V};
  for (int k = 0; k < 6; ++k) {
    const long long at = lm[9 + k];
    if (at < kLmHeader || at + len[k] > words) return t;
  }
  t.m = lm_view(lm);
  t.n_nodes = (int)n_nodes, t.n_edges = (int)n_edges, t.W = (int)W;
  t.on = true;
  return t;
}

__device__ __forceinline__ int tlm_node(const TlmView& t, int s) { return (unsigned)s < (unsigned)t.n_nodes ? s : 0; }  // outside: the root
__device__ __forceinline__ int tlm_word(const TlmView& t, int token) {  // word_map[token], an entry outside [0, W) read as word 0
  const int u = t.m.map[token];
  return (unsigned)u < (unsigned)t.W ? u : 0;
}
__device__ __forceinline__ int tlm_edge(const TlmView& t, int e) { return e < 0 ? 0 : (e > t.n_edges ? t.n_edges : e); }

// lm_walk(t.m, s, u, next) for a node s and an LM word u of the model, indices clamped as said above
__device__ __forceinline__ float tlm_walk(const TlmView& t, int s, int u, int& next) {
  const LmView& m = t.m;
  float acc = 0.f;
  for (int d = 0; d <= kLmMaxOrder; ++d) {
    int x = u + 1;
    if (s != 0 && d < kLmMaxOrder) {  // the sixth node of a chain is read as the root: a valid image reaches it within five
      int lo = tlm_edge(t, m.begin[s]);
      const int end = tlm_edge(t, m.begin[s + 1]);
      int hi = end;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m.eword[mid] < u)
          lo = mid + 1;
        else
          hi = mid;
      }
      x = (lo < end && m.eword[lo] == u) ? lo + 1 : -1;
    }
    if (x >= 0) {
      acc = acc + m.logp[x];
      next = x < m.top_begin ? x : tlm_node(t, m.suffix[x]);
      return acc;
    }
    acc = acc + m.backoff[s];
    s = tlm_node(t, m.suffix[s]);
  }
  next = 0;
  return acc;
}

// inc = fl(fl(lm_weight * acc) + token_score): the product rounded on its own (lm_add's rule)
__device__ __forceinline__ float tlm_inc(float lm_weight, float acc, float token_score) {
#pragma clang fp contract(off)
  const float term = lm_weight * acc;
  return term + token_score;
}

}  // namespace eec
