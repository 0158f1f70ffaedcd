// Keyword and phrase spotting on CTC emissions (include/eec.h, "Keyword spotting on CTC emissions"): for every (emission,
// keyword) pair the best-scoring segment of the emission whose frames CTC-collapse to the keyword, and optionally that score for
// every end frame.  Max-over-paths (Viterbi) only; the frame term is the emission minus the frame's maximum, so a segment that
// greedy decoding spells scores exactly 0.  The statement -- states, candidate order, tie rules -- is the header's; this file is
// its layout on the device.
//
// Two launches, both without atomics, barriers or LDS:
//   kw_frame_max_kernel: m[n][t] = max_v x[n][t][v] for t < T_n, one wave per frame.  A row is read as float4 from its first
//     16-byte boundary on, the up to three floats in front of it and behind the last whole float4 as scalars: V need not be a
//     multiple of 4 and the storage may begin anywhere on a 4-byte boundary.  A maximum is exact in any order.
//   kw_lattice_kernel: one wave per (emission, keyword); the four waves of a workgroup are four keywords of ONE emission, and
//     consecutive workgroups stay on that emission, so its rows are fetched from memory once and served to the other keywords by
//     the caches.  The 2L - 1 states live in registers, state s in lane s / C: C = 1 for L <= 32 (lane s: even lanes the labels, odd
//     lanes the blanks between them), C = 2 up to L = 64 (lane l: label state 2l and the blank state 2l + 1 behind it).  C is chosen
//     per wave from the keyword's own length.  What crosses a lane boundary (the values and starts of states s - 1 and s - 2) comes
//     by DPP wave shifts, so a frame is a short chain of shifts, compares, selects and one add, with no memory round trip.  The
//     frame's loads -- the gather x[t][lab(s)], the blank's x[t][blank] for C = 2, and m[t] -- are issued kKwAhead frames before
//     their use, off that chain.  Every lane keeps the running best of its own label state; the last state's lane writes it.  The
//     trace leaves in words of 64 frames: lane f & 63 picks frame f's value up from the last state's lane, and a word is one
//     coalesced store.
// A keyword the device cannot serve (a length outside [1, tok_stride], a token outside [0, V) or equal to the blank) gets the fill
// values and none of its tokens becomes an address.  em_len is clamped to [0, T']; frames from the length on are never read.
#include <limits.h>
#include <math.h>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"

namespace eec {

constexpr int kKwAhead = 8;             // frames of look-ahead held in registers (divides 64)
constexpr int kKwWaves = 4;             // keywords of one emission per workgroup
constexpr int kKwMaxTokens = 64;        // L: 2L - 1 states in 64 lanes, two per lane
constexpr int kKwMaxKeywords = 65536;   // K
constexpr int kKwMaxFrames = 1 << 20;   // T'

__device__ __forceinline__ int kw_frames(const int* __restrict__ em_len, int n, int Tq) { return em_len ? min(max(em_len[n], 0), Tq) : Tq; }

__device__ __forceinline__ float kw_lane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

// m[row] = max_v x[row][v], row = n * Tq + t, for the frames t < T_n; the others are left alone (nothing reads them)
__global__ __launch_bounds__(64 * kKwWaves) void kw_frame_max_kernel(const float* __restrict__ x, const int* __restrict__ em_len, int Tq, int V,
                                                                     int n_rows, float* __restrict__ m) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int row = blockIdx.x * kKwWaves + w;
  if (row >= n_rows) return;  // wave-uniform; the kernel has no barrier
  const int n = row / Tq, t = row - n * Tq;
  if (t >= kw_frames(em_len, n, Tq)) return;  // a frame past the length: nothing is read
  const float* p = x + (size_t)row * V;
  const int head = min((int)((16 - ((uintptr_t)p & 15)) & 15) >> 2, V);  // floats in front of the first 16-byte boundary
  const int nvec = (V - head) >> 2, tail = head + 4 * nvec;              // whole float4s, first float behind them
  float v = -INFINITY;
  if (lane < head) v = p[lane];
  if (lane < V - tail) v = fmaxf(v, p[tail + lane]);
  const float4* q = (const float4*)(p + head);
  for (int i = lane; i < nvec; i += 64) {
    const float4 r = q[i];
    v = fmaxf(v, fmaxf(fmaxf(r.x, r.y), fmaxf(r.z, r.w)));
  }
  v = wave_max(v);
  if (lane == 0) m[row] = v;
}

// One (emission, keyword) lattice on one wave, C states per lane.  d[0] / st[0]: this lane's label state (s = 2 * j), for C == 2
// d[1] / st[1]: the blank state behind it; for C == 1 the odd lanes' d[0] is a blank state.
template <int C, bool TRACE>
__device__ __forceinline__ void kw_walk(const float* __restrict__ em, const float* __restrict__ mr, int T, int Tq, int V, int blank, int L,
                                        int id, bool skip, int lane, float* __restrict__ score, int* __restrict__ start,
                                        int* __restrict__ end, float* __restrict__ ts_out, int* __restrict__ tb_out) {
  const int last = (2 * L - 2) / C;  // the last state's lane (its d[0]): wave-uniform
  float d[C], best = -INFINITY;
  int st[C], best_start = -1, best_end = -1;
#pragma unroll
  for (int k = 0; k < C; ++k) d[k] = -INFINITY, st[k] = -1;

  float rg[kKwAhead], rb[kKwAhead], rm[kKwAhead];  // x[t][lab], x[t][blank] (C == 2), m[t] of the frames ahead
#pragma unroll
  for (int u = 0; u < kKwAhead; ++u) {
    rg[u] = rb[u] = rm[u] = 0.f;
    if (T > 0) {
      const int f = min(u, T - 1);
      const float* row = em + (size_t)f * V;
      rg[u] = row[id];
      if (C == 2) rb[u] = row[blank];
      rm[u] = mr[f];
    }
  }
  const int t_end = TRACE ? Tq : T;
  for (int t0 = 0; t0 < t_end; t0 += 64) {
    float word_score = -INFINITY;  // the trace of frame t0 + lane
    int word_start = -1;
    for (int tt = 0; tt < 64 && t0 + tt < T; tt += kKwAhead) {
#pragma unroll
      for (int u = 0; u < kKwAhead; ++u) {
        const int t = t0 + tt + u;
        const float g = rg[u], xb = rb[u], mt = rm[u];
        {  // refill the slot with frame t + kKwAhead (past the end: the last frame again, unused)
          const int f = min(t + kKwAhead, T - 1);
          const float* row = em + (size_t)f * V;
          rg[u] = row[id];
          if (C == 2) rb[u] = row[blank];
          rm[u] = mr[f];
        }
        if (t >= T) continue;
        const bool finite = fabsf(mt) < INFINITY;  // false for a NaN as well
        const float e0 = finite ? g - mt : -INFINITY;
        // the candidates of the label state, in the statement's order; a later one replaces only if strictly greater
        float c = d[0];
        int cs = st[0];
        const float p1 = from_left(d[C - 1], -INFINITY);  // state s - 1
        const int s1 = from_left(st[C - 1], -1);
        const float p2 = C == 1 ? from_left(p1, -INFINITY) : from_left(d[0], -INFINITY);  // state s - 2
        const int s2 = C == 1 ? from_left(s1, -1) : from_left(st[0], -1);
        if (p1 > c) c = p1, cs = s1;
        if (skip && p2 > c) c = p2, cs = s2;
        if (lane == 0 && 0.f > c) c = 0.f, cs = t;  // the fresh start, state 0 only
        if (C == 2) {  // the blank state behind the label: itself, then the label's previous value
          const float e1 = finite ? xb - mt : -INFINITY;
          float cb = d[1];
          int cbs = st[1];
          if (d[0] > cb) cb = d[0], cbs = st[0];
          d[1] = cb + e1;
          st[1] = d[1] == -INFINITY ? -1 : cbs;
        }
        d[0] = c + e0;
        st[0] = d[0] == -INFINITY ? -1 : cs;
        if (d[0] > best) best = d[0], best_start = st[0], best_end = t;  // strict: the first frame that attains the maximum
        if (TRACE) {
          const float fv = kw_lane(d[0], last);
          const int fs = __builtin_amdgcn_readlane(st[0], last);
          if (lane == tt + u) word_score = fv, word_start = fs;
        }
      }
    }
    if (TRACE && t0 + lane < Tq) {
      ts_out[t0 + lane] = word_score;
      tb_out[t0 + lane] = word_start;
    }
  }
  if (lane == last) *score = best, *start = best_start, *end = best_end;
}

template <bool TRACE>
__global__ __launch_bounds__(64 * kKwWaves) void kw_lattice_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                                   const int* __restrict__ em_len, const int* __restrict__ tokens,
                                                                   const int* __restrict__ tok_len, int K, int tok_stride, int kb, int Tq,
                                                                   int V, int blank, float* __restrict__ score, int* __restrict__ start,
                                                                   int* __restrict__ end, float* __restrict__ trace_score,
                                                                   int* __restrict__ trace_start) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int n = blockIdx.x / kb, k = (blockIdx.x - n * kb) * kKwWaves + w;
  if (k >= K) return;  // wave-uniform; the kernel has no barrier
  const size_t o = (size_t)n * K + k;
  const int T = __builtin_amdgcn_readfirstlane(kw_frames(em_len, n, Tq));
  const int L = __builtin_amdgcn_readfirstlane(tok_len[k]);
  float* ts_out = TRACE ? trace_score + o * Tq : nullptr;
  int* tb_out = TRACE ? trace_start + o * Tq : nullptr;

  const bool one = L <= 32;                                   // C == 1
  const int j = one ? lane >> 1 : lane;                       // the token of this lane's label state
  const bool label = !(one && (lane & 1)) && j < L;           // ... if it has one (odd lanes of C == 1 are blanks)
  bool ok = L >= 1 && L <= tok_stride;
  int tk = blank, prev = blank;
  if (ok) {
    const int* row = tokens + (size_t)k * tok_stride;
    if (label) tk = row[j];
    if (label && j >= 1) prev = row[j - 1];
    ok = __ballot(label && (tk < 0 || tk >= V || tk == blank)) == 0;
  }
  if (!ok) {  // not a keyword: defined fill values, none of its tokens is used
    if (lane == 0) score[o] = -INFINITY, start[o] = -1, end[o] = -1;
    if (TRACE)
      for (int f = lane; f < Tq; f += 64) ts_out[f] = -INFINITY, tb_out[f] = -1;
    return;
  }
  const int id = label ? tk : blank;                    // lanes past the last state compute on the blank and feed nothing
  const bool skip = label && j >= 1 && tk != prev;      // state s - 2 is a candidate: lab(s) != lab(s - 2)
  const float* em = x + (size_t)n * Tq * V;
  const float* mr = m + (size_t)n * Tq;
  if (one)
    kw_walk<1, TRACE>(em, mr, T, Tq, V, blank, L, id, skip, lane, score + o, start + o, end + o, ts_out, tb_out);
  else
    kw_walk<2, TRACE>(em, mr, T, Tq, V, blank, L, id, skip, lane, score + o, start + o, end + o, ts_out, tb_out);
}

}  // namespace eec

extern "C" {

size_t eec_keyword_search_workspace_bytes(int n_em, int Tq) {
  if (n_em < 1 || Tq < 1) return 0;
  return eech::up256((size_t)n_em * Tq * sizeof(float));  // the frame maxima
}

int eec_keyword_search(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                       int K, int tok_stride, int blank, float* score, int32_t* start, int32_t* end, float* trace_score,
                       int32_t* trace_start, void* workspace, size_t workspace_bytes, void* stream) {
  using eech::fail;
  using std::to_string;
  if (K < 1 || K > eec::kKwMaxKeywords)
    return fail(EEC_ERR_BAD_ARG, "eec_keyword_search: K must be in 1.." + to_string(eec::kKwMaxKeywords) + ", got " + to_string(K));
  if (tok_stride < 1 || tok_stride > eec::kKwMaxTokens)
    return fail(EEC_ERR_BAD_ARG, "eec_keyword_search: a keyword has 1.." + to_string(eec::kKwMaxTokens) + " tokens, got tok_stride " +
                                     to_string(tok_stride));
  if (Tq < 1 || Tq > eec::kKwMaxFrames)
    return fail(EEC_ERR_BAD_ARG, "eec_keyword_search: Tq must be in 1..2^20, got " + to_string(Tq));
  if (n_em < 1 || V < 2 || blank < 0 || blank >= V)
    return fail(EEC_ERR_BAD_ARG, "eec_keyword_search: needs n_em >= 1, V >= 2 and blank in [0, V)");
  if (!logp || !tokens || !tok_len || !score || !start || !end) return fail(EEC_ERR_BAD_ARG, "eec_keyword_search: null argument");
  if ((trace_score == nullptr) != (trace_start == nullptr))
    return fail(EEC_ERR_BAD_ARG, "eec_keyword_search: trace_score and trace_start are given together or not at all");
  const int kb = (K + eec::kKwWaves - 1) / eec::kKwWaves;
  if ((long long)n_em * Tq > INT_MAX || (long long)n_em * kb > INT_MAX)
    return fail(EEC_ERR_UNSUPPORTED, "eec_keyword_search: n_em * Tq and n_em * ceil(K / 4) must stay below 2^31");
  if (!workspace) return fail(EEC_ERR_WORKSPACE, "eec_keyword_search: null workspace");
  if (int rc = eech::check_workspace(workspace, workspace_bytes, eec_keyword_search_workspace_bytes(n_em, Tq))) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* m = (float*)workspace;
  const int n_rows = n_em * Tq;
  hipLaunchKernelGGL(eec::kw_frame_max_kernel, dim3((n_rows + eec::kKwWaves - 1) / eec::kKwWaves), dim3(64 * eec::kKwWaves), 0, st, logp,
                     em_len, Tq, V, n_rows, m);
  EEC_HIP(hipGetLastError());
  const dim3 grid(n_em * kb), block(64 * eec::kKwWaves);
  if (trace_score)
    hipLaunchKernelGGL(eec::kw_lattice_kernel<true>, grid, block, 0, st, logp, m, em_len, tokens, tok_len, K, tok_stride, kb, Tq, V, blank,
                       score, start, end, trace_score, trace_start);
  else
    hipLaunchKernelGGL(eec::kw_lattice_kernel<false>, grid, block, 0, st, logp, m, em_len, tokens, tok_len, K, tok_stride, kb, Tq, V, blank,
                       score, start, end, trace_score, trace_start);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
