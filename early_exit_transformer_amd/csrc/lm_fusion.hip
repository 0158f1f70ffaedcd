// Shallow fusion with a token-level n-gram model in the AED lockstep searches: the step kernel (include/eec.h, "Shallow fusion";
// tests/lmfusion_cases.py is the plain-Python restatement).  The fused CTC prefix beam search is ctc_beam_lm.hip.
//
// One workgroup per (search, beam) row, work-item v owns token v.  Every work-item derives the row's new state from uniform loads
// (parent, last token, the parent's state, one walk); work-item 0 stores it.  The V increments of the row are NOT V binary searches:
// the row's suffix chain state, suffix[state], .., root is walked once, with the running back-off sum in front of each node formed
// in the walk's order; then the root's unigrams and each chain node's edge range are scattered into one LDS row over the LM words,
// shallowest first and the deepest node last (a barrier between two levels), so that a word ends with the entry lm_walk stops
// at: acc = fl(sum of the back-offs passed + logp), the same additions.  One gather through word_map and two rounded operations per
// token follow.  States are double-buffered as in ctx_graph.hip: step s reads half s & 1 and writes the other.  Vector stores only,
// no atomics, nothing read back.
#include <math.h>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_lm.h"

namespace eec {

__global__ __launch_bounds__(256) void lm_fusion_step_kernel(const int* __restrict__ lm, long long words, int R, int R_prev, int R_max, int V,
                                                             int s, const long long* __restrict__ parent, const long long* __restrict__ last,
                                                             const float* local, float* out, const int* __restrict__ src,
                                                             int* __restrict__ dst, float lm_weight, float token_score, int eos, int skip0,
                                                             int skip1, int skip2) {
  __shared__ float accw[kTlmMaxWords];
  const int i = blockIdx.x / R, r = blockIdx.x % R, v = threadIdx.x, nt = blockDim.x;
  const size_t at = ((size_t)i * R + r) * V + v;
  const TlmView T = tlm_view(lm, words, V);
  if (!T.on) {  // fusion is off: the input as it is
    if (v == 0) dst[(size_t)i * R_max + r] = 0;
    if (v < V) out[at] = local[at];
    return;
  }
  int st = tlm_node(T, T.m.bos);
  if (s > 0) {
    const long long pl = parent ? parent[(size_t)i * R + r] : (long long)r;
    const long long cl = last[(size_t)i * R + r];
    if (pl >= 0 && pl < R_prev && cl >= 0 && cl < V) {  // an index outside its range is never used as an address: the start state
      const int ps = src[(size_t)i * R_max + pl];
      if (ps == kTlmDead || cl == eos)
        st = kTlmDead;
      else if (cl == skip0 || cl == skip1 || cl == skip2)
        st = tlm_node(T, ps);
      else
        tlm_walk(T, tlm_node(T, ps), tlm_word(T, (int)cl), st);
    }
  }
  if (v == 0) dst[(size_t)i * R_max + r] = st;
  if (st == kTlmDead || (lm_weight == 0.f && token_score == 0.f)) {  // uniform: every increment of the row is 0
    if (v < V) out[at] = local[at];
    return;
  }
  // the suffix chain, and in front of every node the back-offs passed on the way to it
  int chain[kTlmChain];
  float passed[kTlmChain];
  int L = 0;
  {
    int node = st;
    float b = 0.f;
    for (int k = 0; k < kTlmChain; ++k) {
      if (k == kTlmChain - 1) node = 0;
      chain[k] = node, passed[k] = b, L = k + 1;
      if (node == 0) break;
      b = b + T.m.backoff[node];
      node = tlm_node(T, T.m.suffix[node]);
    }
  }
#pragma unroll
  for (int k = kTlmChain - 1; k >= 0; --k) {
    if (k >= L) continue;  // uniform
    if (k == L - 1) {      // the root: the unigram of word u is node u + 1
      for (int u = v; u < T.W; u += nt) accw[u] = passed[k] + T.m.logp[u + 1];
    } else {
      const int lo = tlm_edge(T, T.m.begin[chain[k]]), end = tlm_edge(T, T.m.begin[chain[k] + 1]);
      for (int e = lo + v; e < end; e += nt) {
        const int u = T.m.eword[e];
        if ((unsigned)u < (unsigned)T.W) accw[u] = passed[k] + T.m.logp[e + 1];
      }
    }
    __syncthreads();
  }
  if (v >= V) return;
  const float x = local[at];
  float inc = 0.f;
  if (v == eos)
    inc = tlm_inc(lm_weight, T.m.eos >= 0 ? accw[T.m.eos] : 0.f, token_score);
  else if (v != skip0 && v != skip1 && v != skip2)
    inc = tlm_inc(lm_weight, accw[tlm_word(T, v)], token_score);
  out[at] = (x == -INFINITY || inc == 0.f) ? x : x + inc;
}

}  // namespace eec

extern "C" {

size_t eec_lm_fusion_state_bytes(int n, int R_max) {
  return n > 0 && R_max > 0 ? 2 * (size_t)n * R_max * sizeof(int32_t) : 0;
}

int eec_lm_fusion_step(const void* lm, size_t lm_bytes, int n, int R, int R_prev, int R_max, int V, int s, const int64_t* parent,
                       const int64_t* last, const float* local, float* out, void* state, size_t state_bytes, float lm_weight,
                       float token_score, int eos, int skip0, int skip1, int skip2, void* stream) {
  const char* refused = isfinite(lm_weight) && isfinite(token_score) ? nullptr : "lm_weight and token_score must be finite";
  eech::StepHalves h;
  const int rc = eech::step_head("eec_lm_fusion_step", "lm", refused, lm, n, R, R_prev, R_max, V, s, last, local, out, state, state_bytes, &h);
  if (rc != 0 || !h.src) return rc;
  hipLaunchKernelGGL(eec::lm_fusion_step_kernel, dim3(n * R), dim3((V + 63) / 64 * 64), 0, (hipStream_t)stream, (const int*)lm,
                     (long long)(lm_bytes / 4), R, R_prev, R_max, V, s, (const long long*)parent, (const long long*)last, local, out,
                     h.src, h.dst, lm_weight, token_score, eos, skip0, skip1, skip2);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_lm_fusion_step launch");
}

}  // extern "C"
