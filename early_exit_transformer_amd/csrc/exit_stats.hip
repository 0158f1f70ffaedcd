// Exit statistics and exit routing (include/eec.h, "Adaptive inference"): what an early-exit model chooses its exit by.
//   lp_v = x_v - lse(x),  p_v = exp(lp_v)   for every row x[e, b, t, :] with t < len_b (logits or log-probs: normalised here)
//   entropy[e, b]     = (1 / max(len_b, 1)) sum_t -sum_v p_v lp_v        (nats; a term with p_v = 0 is 0)
//   confidence[e, b]  = (1 / max(len_b, 1)) sum_t max_v p_v
//   greedy_logp[e, b] = sum_t max_v lp_v                                  (the greedy CTC path, not divided by the length)
// The layout is distill.hip's: ONE WAVE PER FRAME (b, t), a float4 per lane (V <= 256, lanes past V idle); the wave walks the
// exits four at a time -- the four loads are in flight before the first reduction waits -- and keeps a row as
//   s_v = x_v - max  and  lse = log sum_v exp(s_v),     lp_v = s_v - lse,     max_v lp_v = -lse  (the maximum's s is 0),
// so every logit is read once.  The frame's three terms go to a [3, E, B, T] workspace; exit_stats_reduce_kernel adds an
// utterance's frames in index order (one wave per (statistic, e, b): 64 frames per load, added up out of registers).  No
// floating-point atomics: the statistics are bit-reproducible from run to run, and a call on a slice of the exits or of the batch
// gives the bits of the whole call.  Memory-bound (no LDS, no MFMA): [6, 64, 256, 256] reads 100 MB.  exp / log are the exact forms.
// A masked frame (t >= len_b) is neither read nor written nor added.  A NaN logit makes its row's log-sum-exp NaN, hence the
// three statistics of that (e, b) and nothing else.
//
// exit_route_kernel: the stable partition of 0 .. n-1 by "row i leaves" (score[i] < threshold, or > with higher_is_better; a
// NaN compares false and stays; force_all: every row leaves).  One workgroup walks the rows 256 at a time: a wave's ballot
// gives a row's rank among the wave's leavers, the waves' counts meet in LDS, the running total is carried in a register that
// every thread holds alike.  Row i is leaver number r(i) = #{j < i : j leaves} or stayer number i - r(i): both lists ascend.
#include <limits.h>

#include "eec_kernels.h"

namespace eec {

__device__ __forceinline__ int exit_frame_len(const int* __restrict__ frame_len, int b, int T) {
  return frame_len ? min(max(frame_len[b], 0), T) : T;
}

// ws[k][e][b][t], k = 0 entropy term, 1 max_v p_v, 2 max_v lp_v of frame (b, t) of exit e; frames t >= len_b are left alone
__global__ __launch_bounds__(256) void exit_stats_frame_kernel(const float* __restrict__ x, const int* __restrict__ frame_len, int E, int B,
                                                               int T, int V, int n_rows, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int row = blockIdx.x * 4 + w;
  if (row >= n_rows) return;  // wave-uniform; the kernel has no barrier
  const int b = row / T, t = row - b * T, c0 = lane * 4;
  if (t >= exit_frame_len(frame_len, b, T)) return;  // a masked frame: nothing is read
  const size_t plane = (size_t)E * B * T;
  for (int e0 = 0; e0 < E; e0 += 4) {
    float4 s[4];
    static_range<0, 4>([&](auto J) {
      constexpr int j = decltype(J)::value;
      s[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);  // idle lanes: neutral for the maximum, exp(s) = 0
      if (e0 + j < E && c0 < V) s[j] = *(const float4*)(x + (((size_t)(e0 + j) * B + b) * T + t) * V + c0);
    });
    static_range<0, 4>([&](auto J) {
      constexpr int j = decltype(J)::value;
      if (e0 + j < E) {  // wave-uniform
        float4 r = s[j];
        // fmaxf drops a NaN: the maximum is that of the row's numbers, the NaN comes back through exp below
        const float m = wave_max(fmaxf(fmaxf(r.x, r.y), fmaxf(r.z, r.w)));
        r.x -= m, r.y -= m, r.z -= m, r.w -= m;
        const float lse = logf(wave_sum((expf(r.x) + expf(r.y)) + (expf(r.z) + expf(r.w))));
        auto term = [&](float sv) {
          const float lp = sv - lse, p = expf(lp);
          return p == 0.f ? 0.f : p * lp;
        };
        const float plogp = wave_sum((term(r.x) + term(r.y)) + (term(r.z) + term(r.w)));
        const float top = 0.f - lse;  // max_v lp_v: the maximum's s is 0 (NaN with the row's lse)
        const float out = lane == 0 ? 0.f - plogp : lane == 1 ? expf(top) : top;
        if (lane < 3) ws[lane * plane + ((size_t)(e0 + j) * B + b) * T + t] = out;
      }
    });
  }
}

// stats[k][e][b]: the frames t < len_b of ws[k][e][b] added in index order; k = 0, 1 divided by max(len_b, 1).  One wave per (k, e, b).
__global__ __launch_bounds__(256) void exit_stats_reduce_kernel(const float* __restrict__ ws, const int* __restrict__ frame_len, int E, int B,
                                                                int T, int n_out, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int o = blockIdx.x * 4 + w;  // (k * E + e) * B + b
  if (o >= n_out) return;            // wave-uniform; the kernel has no barrier
  const int b = o % B, k = o / (E * B);
  const int len = exit_frame_len(frame_len, b, T);
  const float* p = ws + (size_t)o * T;
  float s = 0.f;
  for (int t0 = 0; t0 < len; t0 += 64) {
    const float term = t0 + lane < len ? p[t0 + lane] : 0.f;
    const int n = min(64, len - t0);
    if (n == 64) {
#pragma unroll
      for (int i = 0; i < 64; ++i) s += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, term), i));
    } else {
      for (int i = 0; i < n; ++i) s += __shfl(term, i, 64);
    }
  }
  if (lane == 0) stats[o] = k < 2 ? s / (float)(len > 0 ? len : 1) : s;
}

constexpr int kRouteThreads = 256;

__global__ __launch_bounds__(kRouteThreads) void exit_route_kernel(const float* __restrict__ score, int n, float threshold, int higher,
                                                                   int force_all, int* __restrict__ stay_idx, int* __restrict__ leave_idx,
                                                                   int* __restrict__ counts) {
  __shared__ int wave_leavers[2][kRouteThreads / 64];  // double-buffered: one barrier per 256 rows
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  int left = 0;  // leavers among the rows before this round's: the same number in every thread
  int round = 0;
  for (int i0 = 0; i0 < n; i0 += kRouteThreads, round ^= 1) {
    const int i = i0 + (int)threadIdx.x;
    bool leaves = false;
    if (i < n) {
      const float s = score[i];
      leaves = force_all || (higher ? s > threshold : s < threshold);  // a NaN compares false: it stays
    }
    const unsigned long long mask = __ballot(leaves);
    if (lane == 0) wave_leavers[round][w] = __popcll(mask);
    __syncthreads();
    int before = left, total = left;
#pragma unroll
    for (int j = 0; j < kRouteThreads / 64; ++j) {
      const int c = wave_leavers[round][j];
      before += j < w ? c : 0;
      total += c;
    }
    if (i < n) {
      const int r = before + __popcll(mask & ((1ull << lane) - 1ull));  // leavers before row i
      if (leaves) {
        leave_idx[r] = i;
      } else {
        stay_idx[i - r] = i;
      }
    }
    left = total;
  }
  if (threadIdx.x == 0) counts[0] = n - left, counts[1] = left;
}

// sizes are validated by the entry point (eec_exit_stats, capi.hip)
hipError_t launch_exit_stats(const float* x, const int* frame_len, int E, int B, int T, int V, float* stats, float* ws, hipStream_t st) {
  if (E < 1 || E > kExitStatsMaxExits || V > 256 || V % 4 || (long long)B * T > INT_MAX || (long long)3 * E * B > INT_MAX)
    return hipErrorInvalidValue;
  const int n_rows = B * T, n_out = 3 * E * B;
  hipLaunchKernelGGL(exit_stats_frame_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, x, frame_len, E, B, T, V, n_rows, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(exit_stats_reduce_kernel, dim3((n_out + 3) / 4), dim3(256), 0, st, ws, frame_len, E, B, T, n_out, stats);
  return hipGetLastError();
}

hipError_t launch_exit_route(const float* score, int n, float threshold, int higher_is_better, int force_all, int* stay_idx,
                             int* leave_idx, int* counts, hipStream_t st) {
  if (n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exit_route_kernel, dim3(1), dim3(kRouteThreads), 0, st, score, n, threshold, higher_is_better, force_all, stay_idx,
                     leave_idx, counts);
  return hipGetLastError();
}

}  // namespace eec
