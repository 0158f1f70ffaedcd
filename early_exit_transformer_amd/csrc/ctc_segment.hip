// CTC segmentation (include/eec.h, "CTC segmentation: long rows, free ends"): eec_ctc_forced_align's statement for rows of up to
// EEC_SEG_MAX_TOKENS tokens, with the two flags that make the audio before the first and after the last token free.  The statement
// is the header's; this file is its layout on the device.
//
// One workgroup per row, W = ceil((2 * tok_stride + 1) / 512) waves of it, chosen per launch.  Wave w holds the states 512 w ..
// 512 w + 511 as the eight-states-per-lane strip of eec_ctc_strip.h (lane l, slot k: state 512 w + 8 l + k, label slot i: token
// 256 w + 4 l + i).  One launch, no atomics, no spinning on memory, nothing between workgroups, nothing read back.
//   Forward.  A frame is fa_row<8>'s frame.  The one value that crosses a wave boundary is the left wave's last state of the frame
//     before: lane 63 of wave w leaves its a[7] of frame t in edge[t & 1][w + 1], and lane 0 of wave w + 1 takes it at frame t + 1 as
//     the step candidate of its slot 0 and the skip candidate of its slot 1 (wave 0 reads edge[.][0], which stays -inf).  ONE
//     barrier per frame: the slot written at frame t + 1 was last read at frame t, before the barrier of frame t.  The gathers are
//     issued kSegAhead frames before their use; the barrier does not wait for them, nor for the decision stores.
//   Control flow.  Every barrier is executed by every wave: the row checks, T, N, the end values and the state the walk ends in go
//     through the LDS before anything branches on them, no wave returns before the last barrier, and a wave whose states all lie
//     past 2N runs the loop like the others.  The number of barriers is T + 3 for a row that passes the checks and 3 otherwise.
//   Decisions.  Two bits per (frame, state), a lane's 16 bits of a frame packed two frames to a dword; a frame pair is W lines of
//     256 bytes, [pair][wave][lane], so the dword of "global lane" g = state >> 3 of pair p is dec[p * 64 W + g].
//   Walk back, by wave 0 after every wave's stores have completed (vmcnt(0)) and a barrier.  Blocks of 64 frames, last first.  A
//     state falls by at most 2 a frame, so a block's walk stays within 127 states, 17 global lanes, below the state it enters at:
//     the 32 global lanes that end at the entry state's, for the block's 32 frame pairs, are 16 loads per lane (two pairs a load,
//     128 contiguous bytes each), all in flight at once.  The walk is then wave-uniform scalar work on those registers, as in
//     fa_row; frame_token leaves as whole 256-byte lines, tok_start / tok_end are written by the lane whose frame opens or closes a
//     run.  tok_score is summed by thread j, of all waves, over token j's own frames in frame order.
// A row that is not alignable (the header's status 1) gets the fill values; none of its values becomes an address.
#include "../../include/eec.h"
#include "eec_ctc_strip.h"
#include "eec_kernels.h"

namespace eec {

constexpr int kSegAhead = 8;       // frames of look-ahead held in registers (ctc_forced_align.hip's kFaAhead)
constexpr int kSegMaxWaves = 16;   // 2 * 4095 + 1 = 8191 states, 512 a wave
static_assert(2 * EEC_SEG_MAX_TOKENS + 1 <= 512 * kSegMaxWaves, "the states of the longest row fit the workgroup");

__host__ __device__ inline int seg_waves(int tok_stride) { return (2 * tok_stride + 1 + 511) / 512; }
__host__ __device__ inline size_t seg_pairs(int Tq) { return ((size_t)Tq + 1) / 2; }  // decision dwords per global lane

// the label slot i of lane `lane` of wave w: strip_label<8>'s token index 4 l + i, moved by the wave's 256 tokens
__device__ __forceinline__ StripLabel seg_label(const int* __restrict__ tk, int N, int blank, int w, int lane, int i) {
  return strip_label<8>(tk, N, blank, 64 * w + lane, i);
}

struct SegOut {
  int* tok_start;     // [tok_stride]
  int* tok_end;       // [tok_stride]
  float* tok_score;   // [tok_stride]
  int* frame_token;   // [Tq]
  float* path_score;  // [1]
  int* status;        // [1]
};

// the fill values of a row that is not alignable, by the whole workgroup
__device__ __forceinline__ void seg_fill(const SegOut& o, int Tq, int tok_stride, int tid, int nt) {
  for (int f = tid; f < Tq; f += nt) o.frame_token[f] = -2;
  for (int j = tid; j < tok_stride; j += nt) o.tok_start[j] = -1, o.tok_end[j] = -1, o.tok_score[j] = -INFINITY;
  if (tid == 0) *o.path_score = -INFINITY, *o.status = 1;
}

// The forward sweep of a row that passed the row checks, on every wave of the workgroup: T barriers.  Leaves the decisions in dec
// and the states 2N and 2N - 1 of the last frame in end[0] and end[1].
__device__ __forceinline__ void seg_forward(const float* __restrict__ em, int T, int V, int blank, int flags, int N, const int* __restrict__ tk,
                                            int w, int W, int lane, unsigned* __restrict__ dec, float (*edge)[kSegMaxWaves + 1], float* end) {
  constexpr int C = 8, NL = 4;
  const int s0 = 512 * w + 8 * lane;  // the strip's first state
  int id[NL];      // the strip's labels
  bool skip[NL];   // ... and whether state s - 2 is a candidate of the label slot
  bool zero[NL];   // the emission term of the blank slot 2 i is 0.0f: state 0 under FREE_START, state 2N under FREE_END
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const StripLabel l = seg_label(tk, N, blank, w, lane, i);
    id[i] = l.id, skip[i] = l.skip;
    zero[i] = ((flags & EEC_SEG_FREE_START) && s0 + 2 * i == 0) || ((flags & EEC_SEG_FREE_END) && s0 + 2 * i == 2 * N);
  }

  float a[C];
  {  // frame 0: states 0 and 1 only
    const float xb = em[blank], x0 = em[id[0]];
#pragma unroll
    for (int k = 0; k < C; ++k) a[k] = -INFINITY;
    if (s0 == 0) a[0] = zero[0] ? 0.0f : xb, a[1] = x0;
  }
  if (lane == 63) edge[0][w + 1] = a[C - 1];
  float rg[kSegAhead][NL], rb[kSegAhead];  // x[t][label] and x[t][blank] of the frames ahead; slot u: frame t0 + u
#pragma unroll
  for (int u = 0; u < kSegAhead; ++u) {
    const float* row = em + (size_t)min(u, T - 1) * V;
#pragma unroll
    for (int i = 0; i < NL; ++i) rg[u][i] = row[id[i]];
    rb[u] = row[blank];
  }
  __syncthreads();  // frame 0's edge values

  const size_t line = (size_t)W * 64;
  unsigned word = 0;
  for (int t0 = 0; t0 < T; t0 += kSegAhead) {
#pragma unroll
    for (int u = 0; u < kSegAhead; ++u) {
      const int t = t0 + u;
      float g[NL];
#pragma unroll
      for (int i = 0; i < NL; ++i) g[i] = rg[u][i];
      const float xb = rb[u];
      {  // refill the slot with frame t + kSegAhead (past the end: the last frame again, unused)
        const float* row = em + (size_t)min(t + kSegAhead, T - 1) * V;
#pragma unroll
        for (int i = 0; i < NL; ++i) rg[u][i] = row[id[i]];
        rb[u] = row[blank];
      }
      if (t == 0 || t >= T) continue;  // t and T are the same in every wave
      // the candidates in the statement's order; a later one replaces only if strictly greater.  Lane 0 takes the left wave's
      // last state of frame t - 1; in wave 0 that is -inf, which is greater than nothing: state 0 only stays
      const float left = from_left(a[C - 1], edge[(t - 1) & 1][w]);
      unsigned dd = 0;
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
        a[k] = best + ((k & 1) ? g[k >> 1] : (zero[k >> 1] ? 0.0f : xb));
        dd |= d << (2 * k);
      });
      if (lane == 63) edge[t & 1][w + 1] = a[C - 1];
      word |= dd << ((t & 1) * 16);
      if (t & 1) {
        dec[(size_t)(t >> 1) * line + 64 * w + lane] = word;
        word = 0;
      }
      __syncthreads();  // frame t's edge values; the slot it will overwrite at t + 1 was read before this barrier
    }
  }
  if (T & 1) dec[(size_t)((T - 1) >> 1) * line + 64 * w + lane] = word;

  static_range<0, C>([&](auto tag) {  // one lane of one wave holds each
    constexpr int k = decltype(tag)::value;
    if (s0 + k == 2 * N) end[0] = a[k];
    if (s0 + k == 2 * N - 1) end[1] = a[k];
  });
}

// The walk back from state s (wave-uniform, in [0, 2N]) on ONE wave, after the decisions of all waves have arrived: frame_token,
// tok_start, tok_end and the spans in the LDS.  Returns state[0].
__device__ __forceinline__ int seg_walk(int s, int T, int Tq, int N, int W, int lane, const unsigned* __restrict__ dec, int* __restrict__ sp_start,
                                        int* __restrict__ sp_end, const SegOut& o) {
  const size_t line = (size_t)W * 64;
  const int last_word = (T - 1) >> 1;
  int above = -1;  // state[t0 + 64] (-1: there is no such frame)
  for (int b = (Tq - 1) / 64; b >= 0; --b) {
    const int t0 = b * 64;
    int st = -1;  // state[t0 + lane]
    if (t0 < T) {
      // the window: the 32 global lanes up to the entry state's (from 0 where there are fewer below it; 32 <= 64 W).  Register i,
      // lanes 32 q .. 32 q + 31: frame pair t0 / 2 + 2 i + q
      const int g0 = __builtin_amdgcn_readfirstlane(max((s >> 3) - 31, 0));
      unsigned wd[16];
      static_range<0, 16>([&](auto tag) {
        constexpr int i = decltype(tag)::value;
        const int wi = (t0 >> 1) + 2 * i + (lane >> 5);
        wd[i] = wi <= last_word ? dec[(size_t)wi * line + g0 + (lane & 31)] : 0u;
      });
      unsigned long long m0 = 0, m1 = 0;  // the moves of frames t0 .. t0 + 31 and t0 + 32 .. t0 + 63, two bits each (scalars)
      static_range<0, 64>([&](auto tag) {  // u = 63 .. 0, a compile-time constant: wd stays in registers
        constexpr int u = 63 - decltype(tag)::value;
        const int t = t0 + u;
        if (t < T && t >= 1) {
          const int col = min(max((s >> 3) - g0, 0), 31);  // in [0, 31] by the window's construction
          const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)wd[u >> 2], ((u >> 1) & 1) * 32 + col);
          const int ns = max(s - ((int)(v >> (((u & 1) * 8 + (s & 7)) * 2)) & 3), 0);
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
  return s;
}

__global__ __launch_bounds__(64 * kSegMaxWaves) void ctc_segment_kernel(
    const float* __restrict__ logp, int n_em, int Tq, int V, const int* __restrict__ em_len, const int* __restrict__ tokens,
    const int* __restrict__ tok_len, const int* __restrict__ em_index, int tok_stride, int blank, int flags, int* __restrict__ tok_start,
    int* __restrict__ tok_end, float* __restrict__ tok_score, int* __restrict__ frame_token, float* __restrict__ path_score,
    int* __restrict__ status, unsigned* __restrict__ ws) {
  extern __shared__ int seg_spans[];  // [2][tok_stride]: tok_start and tok_end of the row
  __shared__ float edge[2][kSegMaxWaves + 1];
  __shared__ int row_bc[4];   // N, T, ei, ok
  __shared__ float end_bc[2];  // a[T - 1][2N], a[T - 1][2N - 1]
  __shared__ int walk_bc;     // state[0]
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), W = nt >> 6;
  const int h = blockIdx.x;
  const SegOut o{tok_start + (size_t)h * tok_stride, tok_end + (size_t)h * tok_stride, tok_score + (size_t)h * tok_stride,
                 frame_token + (size_t)h * Tq,       path_score + h,                   status + h};
  const int* tk = tokens + (size_t)h * tok_stride;
  unsigned* dec = ws + (size_t)h * seg_pairs(Tq) * W * 64;
  int *sp_start = seg_spans, *sp_end = seg_spans + tok_stride;

  if (w == 0) {  // the row checks, once, and to every wave through the LDS
    const StripRow r = strip_row(tk, tok_len, em_index, em_len, h, n_em, Tq, V, tok_stride, blank, lane, EEC_SEG_MAX_TOKENS);
    if (lane == 0) row_bc[0] = r.N, row_bc[1] = r.T, row_bc[2] = r.ei, row_bc[3] = r.ok ? 1 : 0;
  }
  if (tid < 2) edge[tid][0] = -INFINITY;  // what wave 0 takes from its left
  if (tid == 0) end_bc[0] = -INFINITY, end_bc[1] = -INFINITY, walk_bc = 2;
  __syncthreads();
  const int N = __builtin_amdgcn_readfirstlane(row_bc[0]), T = __builtin_amdgcn_readfirstlane(row_bc[1]);
  const int ei = __builtin_amdgcn_readfirstlane(row_bc[2]);
  const bool ok = __builtin_amdgcn_readfirstlane(row_bc[3]) != 0;
  const float* em = logp + (size_t)(ok ? ei : 0) * Tq * V;

  if (ok) seg_forward(em, T, V, blank, flags, N, tk, w, W, lane, dec, edge, end_bc);  // T barriers, in every wave alike
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's decisions have arrived before any wave reads them back
  __syncthreads();
  const float hi = end_bc[0], lo = end_bc[1];
  const bool at_blank = hi > lo;
  const float ps = at_blank ? hi : lo;
  const bool path = ok && ps > -INFINITY;  // false for a NaN; the same in every wave

  if (path && w == 0) {
    const int s0 = seg_walk(__builtin_amdgcn_readfirstlane(at_blank ? 2 * N : 2 * N - 1), T, Tq, N, W, lane, dec, sp_start, sp_end, o);
    if (lane == 0) walk_bc = s0;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the walk's stores have arrived before another wave may write the fill over them
  __syncthreads();  // the last barrier
  if (!path || walk_bc > 1) {  // not alignable: the checks, no path, or a walk left short of the first two states
    seg_fill(o, Tq, tok_stride, tid, nt);
  } else {
    for (int j = N + tid; j < tok_stride; j += nt) o.tok_start[j] = -1, o.tok_end[j] = -1, o.tok_score[j] = -INFINITY;
    // token j's emissions over its own frames, in frame order, beginning with the first frame's value
    for (int j = tid; j < N; j += nt) {
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
    if (tid == 0) *o.path_score = ps, *o.status = 0;
  }
}

}  // namespace eec

extern "C" {

size_t eec_ctc_segment_workspace_bytes(int n_hyp, int Tq, int tok_stride) {
  if (n_hyp < 1 || Tq < 1 || tok_stride < 1) return 0;
  const size_t waves = ((size_t)2 * (size_t)tok_stride + 1 + 511) / 512;  // in size_t: no limit on tok_stride here
  return (size_t)n_hyp * eec::seg_pairs(Tq) * waves * 64 * sizeof(uint32_t);
}

int eec_ctc_segment(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                    const int32_t* em_index, int n_hyp, int tok_stride, int blank, int flags, int32_t* tok_start, int32_t* tok_end,
                    float* tok_score, int32_t* frame_token, float* path_score, int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (flags & ~(EEC_SEG_FREE_START | EEC_SEG_FREE_END))
    return eech::fail(EEC_ERR_BAD_ARG, "eec_ctc_segment: flags holds a bit other than EEC_SEG_FREE_START | EEC_SEG_FREE_END");
  const int rc = eech::strip_entry_head("eec_ctc_segment", {logp, tokens, tok_len, tok_start, tok_end, tok_score, frame_token, path_score, status},
                                        n_em, Tq, V, n_hyp, tok_stride, blank, workspace, workspace_bytes,
                                        eec_ctc_segment_workspace_bytes(n_hyp, Tq, tok_stride), EEC_SEG_MAX_TOKENS);
  if (rc || n_hyp == 0) return rc;
  const int W = eec::seg_waves(tok_stride);
  hipLaunchKernelGGL(eec::ctc_segment_kernel, dim3(n_hyp), dim3(64 * W), 2 * (size_t)tok_stride * sizeof(int), (hipStream_t)stream, logp, n_em,
                     Tq, V, em_len, tokens, tok_len, em_index, tok_stride, blank, flags, tok_start, tok_end, tok_score, frame_token,
                     path_score, status, (unsigned*)workspace);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
