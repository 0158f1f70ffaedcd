// Self-distillation between exits (include/eec.h, "Self-distillation between exits"; the reference declares the flag
// `--distill` and leaves it unimplemented, util/conf.py:48-57): the temperature-softened KL term that pulls a student exit's
// frame posteriors towards its teacher exit's, and its gradient with respect to the student's rows.
//   p = softmax(x[k, b, t, :] / tau),  q = softmax(x[e, b, t, :] / tau),  k = teacher[e]
//   kl[e, b] = sum_{t < len_b} sum_v p_v (log p_v - log q_v),   loss[e] = tau^2 mean_b( kl[e, b] / max(len_b, 1) )
//   d loss[e] / d x[e, b, t, v] = tau (q_v - p_v) / (B max(len_b, 1))            (the teacher is a constant)
// Both directions walk the frames: ONE WAVE PER FRAME (b, t) loads that frame's row of every exit that is a student or a
// teacher -- a float4 per lane, V <= 256, lanes past V idle (the layout of logsoftmax_bwd_kernel, ctc.hip) -- and takes each
// row's maximum and log-sum-exp ONCE, whatever the number of students it teaches.  A row is kept as
//   s_v = (x_v - max) / tau  and  lse = log sum_v exp(s_v),     log softmax(x / tau)_v = s_v - lse,
// so every logit is read once per direction, and the backward writes every gradient element once.  The teacher of a student
// is a run-time index into rows that live in registers: it is resolved by a chain of selects on a wave-uniform condition
// (EC^2 v_cndmask per component at most), never by indexing (which would put the rows into scratch memory).
// The forward leaves the frame's term of every exit in a [E, B, T] workspace (0 on masked frames and for exits without a
// teacher); distill_reduce_kernel adds an utterance's frames in index order and then the batch in index order, as
// ctc_reduce_kernel does.  No floating-point atomics: losses and gradients are bit-reproducible from run to run.
// Memory-bound (no LDS, no MFMA): at [6, 64, 256, 256] the forward reads 100 MB; the backward reads 100 MB and, accumulating
// into the CTC gradient, reads and writes 84 MB.  exp / log are the exact forms.
// NaN logits make the row's log-sum-exp NaN, hence the terms of the exits that read the row (itself as a student, its
// students) and nothing else; a masked frame is not read at all.  p_v = 0 (an exact -inf teacher logit) contributes 0.
#include <limits.h>

#include "eec_kernels.h"

namespace eec {

struct DistillMap {
  int teacher[kDistillMaxExits];  // teacher[e] in [-1, E), != e; -1: exit e is no student
};

// the row k of `rows` / entry k of `vals`, k wave-uniform: selects over compile-time indices
template <int EC>
__device__ __forceinline__ float4 distill_row(const float4 (&rows)[EC], int k) {
  float4 r = rows[0];
  static_range<1, EC>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const bool hit = k == j;
    r.x = hit ? rows[j].x : r.x, r.y = hit ? rows[j].y : r.y, r.z = hit ? rows[j].z : r.z, r.w = hit ? rows[j].w : r.w;
  });
  return r;
}
template <int EC>
__device__ __forceinline__ float distill_val(const float (&vals)[EC], int k) {
  float r = vals[0];
  static_range<1, EC>([&](auto J) {
    constexpr int j = decltype(J)::value;
    r = k == j ? vals[j] : r;
  });
  return r;
}

// One frame's rows: s[j] = (x[j] - max_j) / tau per lane and lse[j] (wave-uniform), for the exits of `used` below E.  Idle lanes
// (c0 >= V) hold s = -inf: the neutral element of the maximum, exp(s) = 0 for the sums.
template <int EC>
__device__ __forceinline__ void distill_load_rows(const float* __restrict__ x, int E, int B, int T, int V, int b, int t, int c0,
                                                  float inv_tau, unsigned used, float4 (&s)[EC], float (&lse)[EC]) {
  static_range<0, EC>([&](auto J) {
    constexpr int j = decltype(J)::value;
    s[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    lse[j] = 0.f;
    if (j < E && ((used >> j) & 1u)) {  // wave-uniform
      if (c0 < V) s[j] = *(const float4*)(x + (((size_t)j * B + b) * T + t) * V + c0);
    }
  });
  // the loads above are independent of each other: all of them are in flight before the first reduction waits
  static_range<0, EC>([&](auto J) {
    constexpr int j = decltype(J)::value;
    if (j < E && ((used >> j) & 1u)) {
      // fmaxf drops a NaN: the maximum is that of the row's numbers, the NaN comes back through exp below
      const float m = wave_max(fmaxf(fmaxf(s[j].x, s[j].y), fmaxf(s[j].z, s[j].w)));
      s[j].x = (s[j].x - m) * inv_tau, s[j].y = (s[j].y - m) * inv_tau, s[j].z = (s[j].z - m) * inv_tau, s[j].w = (s[j].w - m) * inv_tau;
      lse[j] = logf(wave_sum((expf(s[j].x) + expf(s[j].y)) + (expf(s[j].z) + expf(s[j].w))));
    }
  });
}

__device__ __forceinline__ int distill_frame_len(const int* __restrict__ frame_len, int b, int T) {
  return frame_len ? min(max(frame_len[b], 0), T) : T;
}

// ws[e][b][t] = sum_v p_v (log p_v - log q_v) of frame (b, t) for student e; 0 for t >= len_b and for an exit without a teacher
template <int EC>
__global__ __launch_bounds__(256) void distill_fwd_kernel(const float* __restrict__ x, const int* __restrict__ frame_len, DistillMap map,
                                                          int E, int B, int T, int V, float inv_tau, unsigned used, int n_rows,
                                                          float* __restrict__ ws) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int row = blockIdx.x * 4 + w;
  if (row >= n_rows) return;  // wave-uniform; the kernel has no barrier
  const int b = row / T, t = row - b * T, c0 = lane * 4;
  float out = 0.f;  // lane e keeps exit e's term
  if (t < distill_frame_len(frame_len, b, T)) {
    float4 s[EC];
    float lse[EC];
    distill_load_rows<EC>(x, E, B, T, V, b, t, c0, inv_tau, used, s, lse);
    static_range<0, EC>([&](auto Ei) {
      constexpr int e = decltype(Ei)::value;
      const int k = e < E ? map.teacher[e] : -1;
      if (k >= 0) {  // wave-uniform
        const float4 tk = distill_row<EC>(s, k);
        const float lk = distill_val<EC>(lse, k), dl = lse[e] - lk;
        // log p_v - log q_v = (s_k - lse_k) - (s_e - lse_e), grouped so that rows that agree give small differences
        auto term = [&](float sk, float se) {
          const float p = expf(sk - lk);
          return p == 0.f ? 0.f : p * ((sk - se) + dl);
        };
        const float kl = wave_sum((term(tk.x, s[e].x) + term(tk.y, s[e].y)) + (term(tk.z, s[e].z) + term(tk.w, s[e].w)));
        out = lane == e ? kl : out;
      }
    });
  }
  if (lane < E) ws[((size_t)lane * B + b) * T + t] = out;
}

// kl[e][b] = the frames of ws[e][b] added in index order; loss[e] = tau^2 * (sum_b in index order of kl[e][b] / max(len_b, 1)) / B.
// One workgroup per exit: its waves take the utterances in turn (64 frames per load, added up out of registers), then wave 0
// walks the batch as ctc_reduce_kernel does.
__global__ __launch_bounds__(1024) void distill_reduce_kernel(const float* __restrict__ ws, const int* __restrict__ frame_len, int B, int T,
                                                              float tau2, float* kl, float* __restrict__ out) {
  const int e = blockIdx.x, lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int nw = (int)blockDim.x >> 6;
  for (int b = w; b < B; b += nw) {
    const float* p = ws + ((size_t)e * B + b) * T;
    float s = 0.f;
    for (int t0 = 0; t0 < T; t0 += 64) {
      const float term = t0 + lane < T ? p[t0 + lane] : 0.f;
      const int n = min(64, T - t0);
      if (n == 64) {
#pragma unroll
        for (int i = 0; i < 64; ++i) s += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, term), i));
      } else {
        for (int i = 0; i < n; ++i) s += __shfl(term, i, 64);
      }
    }
    if (lane == 0) kl[(size_t)e * B + b] = s;
  }
  __syncthreads();  // the kl written above, by this workgroup, are read below
  if (w != 0) return;
  float s = 0.f;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    float term = 0.f;
    if (b < B) {
      const int len = distill_frame_len(frame_len, b, T);
      term = kl[(size_t)e * B + b] / (float)(len > 0 ? len : 1);
    }
    const int n = min(64, B - b0);
    for (int i = 0; i < n; ++i) s += __shfl(term, i, 64);
  }
  if (lane == 0) out[e] = tau2 * (s / (float)B);
}

// dx[e][b][t][:] (+)= scale * (q - p), scale = grad_loss[e] * tau / (B max(len_b, 1)), for every student e with a non-zero
// grad_loss[e] and t < len_b.  accumulate == 0: every other element of dx is written as 0; accumulate != 0: it is left alone.
template <int EC>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const float* __restrict__ x, const int* __restrict__ frame_len, DistillMap map,
                                                          int E, int B, int T, int V, float inv_tau, float tau, unsigned used,
                                                          const float* __restrict__ grad_loss, int accumulate, int n_rows,
                                                          float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int row = blockIdx.x * 4 + w;
  if (row >= n_rows) return;  // wave-uniform; the kernel has no barrier
  const int b = row / T, t = row - b * T, c0 = lane * 4;
  const int len = distill_frame_len(frame_len, b, T);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  auto at = [&](int e) { return dx + (((size_t)e * B + b) * T + t) * V + c0; };
  if (t >= len) {  // a masked frame: nothing is read
    if (!accumulate && c0 < V)
      for (int e = 0; e < E; ++e) *(float4*)at(e) = zero;
    return;
  }
  float4 s[EC];
  float lse[EC];
  distill_load_rows<EC>(x, E, B, T, V, b, t, c0, inv_tau, used, s, lse);
  const float per_frame = tau / ((float)B * (float)(len > 0 ? len : 1));
  static_range<0, EC>([&](auto Ei) {
    constexpr int e = decltype(Ei)::value;
    if (e < E) {
      const int k = map.teacher[e];
      const float gl = k >= 0 ? grad_loss[e] : 0.f;
      if (gl != 0.f) {  // wave-uniform (a NaN weight counts: it propagates)
        const float4 tk = distill_row<EC>(s, k);
        const float lk = distill_val<EC>(lse, k), le = lse[e], scale = gl * per_frame;
        float4 g;
        g.x = scale * (expf(s[e].x - le) - expf(tk.x - lk)), g.y = scale * (expf(s[e].y - le) - expf(tk.y - lk));
        g.z = scale * (expf(s[e].z - le) - expf(tk.z - lk)), g.w = scale * (expf(s[e].w - le) - expf(tk.w - lk));
        if (c0 < V) {
          if (accumulate) {
            const float4 o = *(const float4*)at(e);
            g.x += o.x, g.y += o.y, g.z += o.z, g.w += o.w;
          }
          *(float4*)at(e) = g;
        }
      } else if (!accumulate && c0 < V) {
        *(float4*)at(e) = zero;
      }
    }
  });
}

// rows a frame's wave has to load: the students and their teachers
static unsigned distill_used(const int* teacher, int E) {
  unsigned used = 0;
  for (int e = 0; e < E; ++e)
    if (teacher[e] >= 0) used |= (1u << e) | (1u << teacher[e]);
  return used;
}

static DistillMap distill_map(const int* teacher, int E) {
  DistillMap m;
  for (int e = 0; e < kDistillMaxExits; ++e) m.teacher[e] = e < E ? teacher[e] : -1;
  return m;
}

// `teacher` is a HOST array the entry point has validated (eec_exit_distill_forward, capi.hip); sizes likewise
hipError_t launch_distill_forward(const float* x, const int* frame_len, const int* teacher, int E, int B, int T, int V, float tau,
                                  float* kl, float* out, float* ws, hipStream_t st) {
  if (E < 1 || E > kDistillMaxExits || V > 256 || V % 4 || (long long)B * T > INT_MAX) return hipErrorInvalidValue;
  const int n_rows = B * T;
  const DistillMap map = distill_map(teacher, E);
  const unsigned used = distill_used(teacher, E);
  const float inv_tau = 1.0f / tau;
#define EEC_DISTILL_FWD(EC_) \
  hipLaunchKernelGGL(distill_fwd_kernel<EC_>, dim3((n_rows + 3) / 4), dim3(256), 0, st, x, frame_len, map, E, B, T, V, inv_tau, used, n_rows, ws)
  if (E <= 4) {
    EEC_DISTILL_FWD(4);
  } else if (E <= 8) {
    EEC_DISTILL_FWD(8);
  } else {
    EEC_DISTILL_FWD(kDistillMaxExits);
  }
#undef EEC_DISTILL_FWD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int waves = B < 16 ? B : 16;
  hipLaunchKernelGGL(distill_reduce_kernel, dim3(E), dim3(64 * waves), 0, st, ws, frame_len, B, T, tau * tau, kl, out);
  return hipGetLastError();
}

hipError_t launch_distill_backward(const float* x, const int* frame_len, const int* teacher, int E, int B, int T, int V, float tau,
                                   const float* grad_loss, int accumulate, float* dx, hipStream_t st) {
  if (E < 1 || E > kDistillMaxExits || V > 256 || V % 4 || (long long)B * T > INT_MAX) return hipErrorInvalidValue;
  const int n_rows = B * T;
  const DistillMap map = distill_map(teacher, E);
  const unsigned used = distill_used(teacher, E);
  const float inv_tau = 1.0f / tau;
#define EEC_DISTILL_BWD(EC_)                                                                                                    \
  hipLaunchKernelGGL(distill_bwd_kernel<EC_>, dim3((n_rows + 3) / 4), dim3(256), 0, st, x, frame_len, map, E, B, T, V, inv_tau, \
                     tau, used, grad_loss, accumulate, n_rows, dx)
  if (E <= 4) {
    EEC_DISTILL_BWD(4);
  } else if (E <= 8) {
    EEC_DISTILL_BWD(8);
  } else {
    EEC_DISTILL_BWD(kDistillMaxExits);
  }
#undef EEC_DISTILL_BWD
  return hipGetLastError();
}

}  // namespace eec
