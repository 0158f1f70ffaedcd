// CTC forced alignment in the standard topology (include/eec.h, "CTC forced alignment, standard topology"): the Viterbi path of a
// token row through the 2N + 1 states blank, y_0, blank, y_1, ..., blank of one emission, and what a caller reads off it: the label
// of every frame, the first and last frame of every token, the token's summed emission, the path's score.  The statement -- the
// candidates, their order, the tie rule, the end rule, the status -- is the header's; this file is its layout on the device.
//
// One launch, no atomics, no barrier, nothing read back.  One wave per hypothesis on the state strips of eec_ctc_strip.h, which
// also holds the row checks, the strip's labels, frame 0 and the end read.
//   Forward.  A frame is a short chain of shifts, compares, selects and one add per state.  The frame's loads -- the gathers
//     x[t][lab(s)] of the strip's labels and x[t][blank] -- are issued kFaAhead frames before their use, off that chain.
//   Decisions.  Two bits per (frame, state), the strip's 2 * C bits packed per lane, 16 / C frames to a dword; a dword per lane is
//     one coalesced 256-byte store, so a row of T frames costs ceil(T * C / 16) such stores.  They go to the WORKSPACE, not to the
//     LDS: at the benchmarked shape (T' = 256, 200 tokens) a row has 32 KiB of them, and four waves' worth would hold a compute
//     unit to one workgroup.  eec_ctc_forced_align_workspace_bytes is n_hyp * ceil(T' * C(tok_stride) / 16) * 256 bytes.
//   Backtrack.  Blocks of 64 frames, last block first.  Every lane loads the block's dwords of its OWN states back (coalesced, all
//     in flight at once, and a lane reads only what it stored itself); the walk is then wave-uniform scalar work on registers --
//     one v_readlane of the state's lane, a shift, a mask, a subtract per frame -- with no memory round trip per step.  Lane
//     t & 63 keeps state[t], so frame_token leaves as whole 256-byte lines, and a lane whose frame opens or closes a run of a label
//     state 2j + 1 writes tok_start[j] / tok_end[j]: the index is the token index, nothing is compacted.  tok_score is then summed
//     by lane j over its own frames, in frame order.
// A row the device cannot serve (the header's status 1) gets the fill values.
#include "../../include/eec.h"
#include "eec_ctc_strip.h"
#include "eec_kernels.h"

namespace eec {

constexpr int kFaAhead = 8;  // frames of look-ahead held in registers

// decision dwords per lane of one hypothesis: 16 / C frames to a dword
__host__ __device__ inline size_t fa_words(int Tq, int C) { return ((size_t)Tq * C + 15) / 16; }

struct FaOut {
  int* tok_start;     // [tok_stride]
  int* tok_end;       // [tok_stride]
  float* tok_score;   // [tok_stride]
  int* frame_token;   // [Tq]
  float* path_score;  // [1]
  int* status;        // [1]
};

// the fill values of a row that is not alignable
__device__ __forceinline__ void fa_fill(const FaOut& o, int Tq, int tok_stride, int lane) {
  for (int f = lane; f < Tq; f += 64) o.frame_token[f] = -2;
  for (int j = lane; j < tok_stride; j += 64) o.tok_start[j] = -1, o.tok_end[j] = -1, o.tok_score[j] = -INFINITY;
  if (lane == 0) *o.path_score = -INFINITY, *o.status = 1;
}

// One alignable-looking row (1 <= N <= tok_stride tokens, all of them labels of [0, V); N + R <= T <= Tq) on one wave, C states
// per lane.  dec: the row's decision dwords, [fa_words(T, C)][64]; spans: the wave's own [2][256] ints of LDS.
template <int C>
__device__ __forceinline__ void fa_row(const float* __restrict__ em, int T, int Tq, int V, int blank, int N, int tok_stride,
                                       const int* __restrict__ tk, int lane, unsigned* __restrict__ dec, int* __restrict__ spans,
                                       const FaOut& o) {
  constexpr int NL = strip_labels(C), LOGC = strip_log2(C);
  constexpr int G = 16 / C;  // frames per decision dword
  int id[NL];     // the strip's labels
  bool skip[NL];  // ... and whether state s - 2 is a candidate of the label slot
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const StripLabel l = strip_label<C>(tk, N, blank, lane, i);
    id[i] = l.id, skip[i] = l.skip;
  }

  float a[C];
  strip_frame0<C>(a, em, blank, id[0], lane);
  float rg[kFaAhead][NL], rb[kFaAhead];  // x[t][label] and (C >= 2) x[t][blank] of the frames ahead; slot u: frame t0 + u
#pragma unroll
  for (int u = 0; u < kFaAhead; ++u) {
    const float* row = em + (size_t)min(u, T - 1) * V;
#pragma unroll
    for (int i = 0; i < NL; ++i) rg[u][i] = row[id[i]];
    rb[u] = C >= 2 ? row[blank] : 0.f;
  }
  unsigned word = 0;
  for (int t0 = 0; t0 < T; t0 += kFaAhead) {
#pragma unroll
    for (int u = 0; u < kFaAhead; ++u) {
      const int t = t0 + u;
      float g[NL];
#pragma unroll
      for (int i = 0; i < NL; ++i) g[i] = rg[u][i];
      const float xb = rb[u];
      {  // refill the slot with frame t + kFaAhead (past the end: the last frame again, unused)
        const float* row = em + (size_t)min(t + kFaAhead, T - 1) * V;
#pragma unroll
        for (int i = 0; i < NL; ++i) rg[u][i] = row[id[i]];
        if (C >= 2) rb[u] = row[blank];
      }
      if (t == 0 || t >= T) continue;
      // the candidates in the statement's order; a later one replaces only if strictly greater
      unsigned dd = 0;
      if (C == 1) {
        const float p1 = from_left(a[0], -INFINITY), p2 = from_left(p1, -INFINITY);
        float best = a[0];
        if (p1 > best) best = p1, dd = 1;  // lane 0 receives -inf, which is greater than nothing: state 0 only stays
        if (skip[0] && p2 > best) best = p2, dd = 2;
        a[0] = best + g[0];
      } else {
        const float left = from_left(a[C - 1], -INFINITY);
        static_range<0, C>([&](auto tag) {  // descending: a[k - 1] and a[k - 2] are still the previous frame's
          constexpr int k = C - 1 - decltype(tag)::value;
          float best = a[k];
          unsigned d = 0;
          const float step = k >= 1 ? a[k >= 1 ? k - 1 : 0] : left;
          if (step > best) best = step, d = 1;
          if (k & 1) {
            const float two = k >= 2 ? a[k >= 2 ? k - 2 : 0] : left;
            if (skip[k >> 1] && two > best) best = two, d = 2;
          }
          a[k] = best + ((k & 1) ? g[k >> 1] : xb);
          dd |= d << (2 * k);
        });
      }
      word |= dd << ((t & (G - 1)) * 2 * C);
      if ((t & (G - 1)) == G - 1) {
        dec[(size_t)(t / G) * 64 + lane] = word;
        word = 0;
      }
    }
  }
  if (T & (G - 1)) dec[(size_t)((T - 1) / G) * 64 + lane] = word;

  const int sN = 2 * N;
  float hi, lo;
  strip_end<C>(a, N, hi, lo);
  const bool at_blank = hi > lo;
  const float ps = at_blank ? hi : lo;
  if (!(ps > -INFINITY)) {  // no path (or a NaN on it)
    fa_fill(o, Tq, tok_stride, lane);
    return;
  }
  for (int j = N + lane; j < tok_stride; j += 64) o.tok_start[j] = -1, o.tok_end[j] = -1, o.tok_score[j] = -INFINITY;

  // the walk back, a block of 64 frames at a time; s is wave-uniform and stays in [0, 2N]
  constexpr int NW = 64 / G;  // dwords per lane and block
  int s = __builtin_amdgcn_readfirstlane(at_blank ? sN : sN - 1);
  int above = -1;  // state[t0 + 64] (-1: there is no such frame)
  int *sp_start = spans, *sp_end = spans + 256;
  const int last_word = (T - 1) / G;
  for (int b = (Tq - 1) / 64; b >= 0; --b) {
    const int t0 = b * 64;
    int st = -1;  // state[t0 + lane]
    if (t0 < T) {
      unsigned w[NW];
      static_range<0, NW>([&](auto tag) {
        constexpr int i = decltype(tag)::value;
        const int wi = t0 / G + i;
        w[i] = wi <= last_word ? dec[(size_t)wi * 64 + lane] : 0u;  // this lane's own stores
      });
      unsigned long long m0 = 0, m1 = 0;  // the moves of frames t0 .. t0 + 31 and t0 + 32 .. t0 + 63, two bits each (scalars)
      static_range<0, 64>([&](auto tag) {  // u = 63 .. 0, a compile-time constant: w stays in registers
        constexpr int u = 63 - decltype(tag)::value;
        const int t = t0 + u;
        if (t < T && t >= 1) {
          const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)w[u / G], s >> LOGC);
          const int ns = max(s - ((int)(v >> (((u & (G - 1)) * C + (s & (C - 1))) * 2)) & 3), 0);
          if (u >= 32)
            m1 |= (unsigned long long)(s - ns) << (2 * (u & 31));
          else
            m0 |= (unsigned long long)(s - ns) << (2 * (u & 31));
          s = ns;
        }
      });
      // state[t] = state[t - 1] + move[t]: the walk stands at state[t0 - 1] (at state[0] in the first block, whose frame 0 has
      // no move), and lane u adds the moves of frames t0 .. t0 + u
      const unsigned long long odd = 0xaaaaaaaaaaaaaaaaull;
      const int n0 = min(lane, 31) + 1, n1 = lane - 31;
      const unsigned long long x0 = m0 & (n0 == 32 ? ~0ull : (1ull << (2 * n0)) - 1);
      const unsigned long long x1 = n1 <= 0 ? 0ull : m1 & (n1 == 32 ? ~0ull : (1ull << (2 * n1)) - 1);
      st = s + __popcll(x0 & ~odd) + 2 * __popcll(x0 & odd) + __popcll(x1 & ~odd) + 2 * __popcll(x1 & odd);
    }
    const int t = t0 + lane;
    const int prev = from_left(st, s);  // lane 0: state[t0 - 1], where the walk now stands
    int next = __shfl_down(st, 1);
    if (lane == 63) next = above;
    above = __builtin_amdgcn_readfirstlane(st);
    if (t < Tq) o.frame_token[t] = t < T ? ((st & 1) ? st >> 1 : -1) : -2;
    if (t < T && (st & 1)) {
      const int j = min(st >> 1, N - 1);
      if (t == 0 || prev != st) o.tok_start[j] = t, sp_start[j] = t;
      if (t == T - 1 || next != st) o.tok_end[j] = t + 1, sp_end[j] = t + 1;
    }
  }
  if (s > 1) {  // state[0]: the walk was left short of the first two states
    fa_fill(o, Tq, tok_stride, lane);
    return;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // token j's emissions over its own frames, in frame order, beginning with the first frame's value
  for (int j = lane; j < N; j += 64) {
    const int y = tk[j], f0 = min(max(sp_start[j], 0), T - 1), f1 = min(sp_end[j], T);
    float acc = em[(size_t)f0 * V + y];
    for (int f = f0 + 1; f < f1; f += 4) {
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = em[(size_t)min(f + q, f1 - 1) * V + y];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (f + q < f1) acc += v[q];
    }
    o.tok_score[j] = acc;
  }
  if (lane == 0) *o.path_score = ps, *o.status = 0;
}

__global__ __launch_bounds__(64 * kStripWaves) void ctc_forced_align_kernel(
    const float* __restrict__ logp, int n_em, int Tq, int V, const int* __restrict__ em_len, const int* __restrict__ tokens,
    const int* __restrict__ tok_len, const int* __restrict__ em_index, int n_hyp, int tok_stride, int blank, int* __restrict__ tok_start,
    int* __restrict__ tok_end, float* __restrict__ tok_score, int* __restrict__ frame_token, float* __restrict__ path_score,
    int* __restrict__ status, unsigned* __restrict__ ws, size_t hyp_words) {
  __shared__ int spans[kStripWaves][2 * 256];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int h = blockIdx.x * kStripWaves + w;
  if (h >= n_hyp) return;  // wave-uniform; the kernel has no barrier
  const FaOut o{tok_start + (size_t)h * tok_stride, tok_end + (size_t)h * tok_stride, tok_score + (size_t)h * tok_stride,
                frame_token + (size_t)h * Tq,       path_score + h,                   status + h};
  const int* tk = tokens + (size_t)h * tok_stride;
  const auto [N, T, ei, ok] = strip_row(tk, tok_len, em_index, em_len, h, n_em, Tq, V, tok_stride, blank, lane);
  if (!ok) {  // not alignable: the fill values
    fa_fill(o, Tq, tok_stride, lane);
    return;
  }
  const float* em = logp + (size_t)ei * Tq * V;
  unsigned* dec = ws + (size_t)h * hyp_words * 64;
  switch (strip_states(N)) {
    case 1: fa_row<1>(em, T, Tq, V, blank, N, tok_stride, tk, lane, dec, spans[w], o); break;
    case 2: fa_row<2>(em, T, Tq, V, blank, N, tok_stride, tk, lane, dec, spans[w], o); break;
    case 4: fa_row<4>(em, T, Tq, V, blank, N, tok_stride, tk, lane, dec, spans[w], o); break;
    default: fa_row<8>(em, T, Tq, V, blank, N, tok_stride, tk, lane, dec, spans[w], o); break;
  }
}

}  // namespace eec

extern "C" {

size_t eec_ctc_forced_align_workspace_bytes(int n_hyp, int Tq, int tok_stride) {
  if (n_hyp < 1 || Tq < 1 || tok_stride < 1) return 0;
  return (size_t)n_hyp * eec::fa_words(Tq, eec::strip_states(tok_stride)) * 64 * sizeof(uint32_t);  // the decisions
}

int eec_ctc_forced_align(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                         const int32_t* em_index, int n_hyp, int tok_stride, int blank, int32_t* tok_start, int32_t* tok_end,
                         float* tok_score, int32_t* frame_token, float* path_score, int32_t* status, void* workspace, size_t workspace_bytes,
                         void* stream) {
  const int rc = eech::strip_entry_head("eec_ctc_forced_align", {logp, tokens, tok_len, tok_start, tok_end, tok_score, frame_token, path_score, status},
                                        n_em, Tq, V, n_hyp, tok_stride, blank, workspace, workspace_bytes,
                                        eec_ctc_forced_align_workspace_bytes(n_hyp, Tq, tok_stride));
  if (rc || n_hyp == 0) return rc;
  const size_t hyp_words = eec::fa_words(Tq, eec::strip_states(tok_stride));
  hipLaunchKernelGGL(eec::ctc_forced_align_kernel, dim3((n_hyp + eec::kStripWaves - 1) / eec::kStripWaves), dim3(64 * eec::kStripWaves), 0,
                     (hipStream_t)stream, logp, n_em, Tq, V, em_len, tokens, tok_len, em_index, n_hyp, tok_stride, blank, tok_start, tok_end,
                     tok_score, frame_token, path_score, status, (unsigned*)workspace, hyp_words);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
