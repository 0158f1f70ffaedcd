// SpecAugment on the device: time warp, frequency and time masks of a mel batch [B, n_mels, T].  The statement -- the draw, the warp's
// integer source positions and fp64 weights, the clipping of untrusted parameters -- is in include/eec.h ("SpecAugment").
//
// eec_specaug_draw: one work-item per (utterance, slot group): group 0 the warp's (c, w), then one group per frequency mask and per
// time mask; each draws its two integers from the dropout generator (eec_drop.h) indexed (utt_offset + b) * 64 + slot and writes them.
//
// eec_specaug_apply: one workgroup of 128 work-items per (time tile, group of 32 mel rows, utterance).  The utterance's parameter row
// is read once through wave-uniform addresses and its clipped mask ranges are kept in registers; which rows of the group and which
// frames of a work-item are masked are bit sets worked out once.  An utterance either has a warp or not, so the choice below is
// uniform per workgroup:
//   * with a warp, work-item j owns output frame 128 * tile + j: segment, tap indices and the fp64 weights (rounded once to fp32)
//     are computed once and reused down the rows; the lanes of a wave store consecutive addresses and load nearly consecutive ones
//     (the source position grows by n_in / n_out per frame).  The taps of four rows (eight in linear mode) are loaded before any of
//     them is stored.  Frames past the length are copied, masked frames and rows store mask_value without loading.
//   * without one, the rows move as 16-byte quads aligned in MEMORY: row r starts (b * n_mels + r) * T floats into the tensor, which
//     is rarely a multiple of four, so quad q of a row covers the frames 4 q - a .. 4 q - a + 3 with a = that offset mod 4.  The 128
//     work-items are four groups of 32: a group takes every fourth row, its lanes the 32 quads of the tile (512 contiguous bytes),
//     four rows loaded before they are stored.  A quad hanging over a row's head or tail, and every quad when a pointer is off a
//     16-byte boundary, moves as single floats.  The seven frames 4 q - 3 .. 4 q + 3 a work-item can touch have their mask bits
//     worked out once; a row shifts them by its a.
#include "../../include/eec.h"
#include "eec_drop.h"
#include "eec_host.h"

#include <cmath>

namespace eec {

constexpr int kSaTile = 128;  // output frames per workgroup; 32 quads per row in the copy path
constexpr int kSaRows = 32;   // mel rows per workgroup

__device__ __forceinline__ int sa_len(const int* __restrict__ frame_len, int b, int T) {
  const int n = frame_len ? frame_len[b] : T;
  return n < 0 ? 0 : n > T ? T : n;
}

// the `count` <= N ranges (start, width) at m, clipped to [0, limit] (the sums in 64 bits; a width below 1 leaves hi <= lo: empty), held
// in registers: the loads are unconditional (index min(k, count - 1)) so that they issue together, entries past count are emptied
template <int N>
__device__ __forceinline__ void sa_ranges(const int* __restrict__ m, int count, int limit, int (&lo)[N], int (&hi)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    lo[k] = hi[k] = 0;
    if (count > 0) {
      const int kk = k < count ? k : count - 1;
      const long long s = m[2 * kk], e = s + (long long)m[2 * kk + 1];
      const int l = (int)(s < 0 ? 0 : s > limit ? limit : s), h = (int)(e < 0 ? 0 : e > limit ? limit : e);
      lo[k] = k < count ? l : 0, hi[k] = k < count ? h : 0;
    }
  }
}
// bit j (j < width <= 32): base + j lies inside one of the ranges
template <int N>
__device__ __forceinline__ unsigned sa_bits(const int (&lo)[N], const int (&hi)[N], int base, int width) {
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int a = min(max(lo[k] - base, 0), width), b = min(max(hi[k] - base, 0), width);
    bits |= b > a ? (unsigned)(((1ull << b) - 1ull) & ~((1ull << a) - 1ull)) : 0u;
  }
  return bits;
}

// taps (absolute frame indices) and weights of output frame d of a segment: n_in source frames from `base` on, n_out output frames
template <bool CUBIC>
__device__ __forceinline__ void sa_taps(int d, int n_in, int n_out, int base, int (&idx)[4], float (&wt)[4]) {
#pragma clang fp contract(off)  // the weights are the stated fp64 expressions, operation by operation
  long long num = (2LL * d + 1) * n_in - n_out;
  const long long den = 2LL * n_out;
  if (!CUBIC && num < 0) num = 0;
  const long long i = num < 0 ? -1 : (long long)((unsigned long long)num / (unsigned long long)den);  // floor: num >= -n_out > -den
  const double f = (double)(num - i * den) / (double)den;
  const int last = n_in - 1, i0 = (int)i;
  if (CUBIC) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = i0 - 1 + k;
      idx[k] = base + (j < 0 ? 0 : j > last ? last : j);
    }
    double x = f + 1.0;
    wt[0] = (float)(((-0.75 * x + 3.75) * x - 6.0) * x + 3.0);
    x = f;
    wt[1] = (float)((1.25 * x - 2.25) * x * x + 1.0);
    x = 1.0 - f;
    wt[2] = (float)((1.25 * x - 2.25) * x * x + 1.0);
    x = 2.0 - f;
    wt[3] = (float)(((-0.75 * x + 3.75) * x - 6.0) * x + 3.0);
  } else {
    idx[0] = base + i0;
    idx[1] = base + (i0 + 1 > last ? last : i0 + 1);
    idx[2] = idx[3] = idx[0];
    wt[0] = (float)(1.0 - f);
    wt[1] = (float)f;
    wt[2] = wt[3] = 0.0f;
  }
}

template <bool CUBIC>
__global__ __launch_bounds__(kSaTile) void specaug_apply_kernel(const float* __restrict__ mel, const int* __restrict__ frame_len,
                                                                 const int* __restrict__ params, int B, int n_mels, int T, int n_freq, int n_time,
                                                                 float mask_value, int vec_ok, float* __restrict__ out) {
  constexpr int K = CUBIC ? 4 : 2;  // taps
  const int r0 = blockIdx.y * kSaRows, r1 = min(r0 + kSaRows, n_mels);
  const int P = 2 + 2 * n_freq + 2 * n_time;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {  // one pass unless B exceeds the grid's z limit
    const int* __restrict__ p = params + (size_t)b * P;
    const int n = sa_len(frame_len, b, T);
    const int c = p[0], w = p[1];
    const bool warped = c >= 1 && c <= n - 1 && w >= 1 && w <= n - 1;
    int flo[EEC_SPECAUG_MAX_FREQ_MASKS], fhi[EEC_SPECAUG_MAX_FREQ_MASKS], tlo[EEC_SPECAUG_MAX_TIME_MASKS], thi[EEC_SPECAUG_MAX_TIME_MASKS];
    sa_ranges(p + 2, n_freq, n_mels, flo, fhi);
    sa_ranges(p + 2 + 2 * n_freq, n_time, n, tlo, thi);
    const unsigned frows = sa_bits(flo, fhi, r0, kSaRows);  // bit r - r0: row r is inside a frequency mask
    const size_t row0 = (size_t)b * n_mels * T;

    if (warped) {
      const int t = blockIdx.x * kSaTile + threadIdx.x;
      if (t >= T) continue;
      const bool valid = t < n;
      const bool tmasked = sa_bits(tlo, thi, t, 1) != 0;  // the ranges lie inside [0, n)
      int idx[4] = {t, t, t, t};  // a frame past the length copies itself: one tap of weight 1 is not a copy (NaN payloads), so v below is src[t]
      float wt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (valid && !tmasked) {
        if (t < w) sa_taps<CUBIC>(t, c, w, 0, idx, wt);
        else sa_taps<CUBIC>(t - w, n - c, n - w, c, idx, wt);
      }
      // 16 taps at a time (four rows, eight in linear mode): loaded before anything is stored
      constexpr int R = 16 / K;
      for (int rr = r0; rr < r1; rr += R) {
        float x[R][K];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const bool load = rr + i < r1 && !(valid && (tmasked || (frows >> (rr + i - r0) & 1u)));
          const float* __restrict__ src = mel + row0 + (size_t)(rr + i) * T;
#pragma unroll
          for (int k = 0; k < K; ++k) x[i][k] = load && (valid || k == 0) ? src[idx[k]] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
          if (rr + i >= r1) break;
          float v;
          if (!valid) v = x[i][0];
          else if (tmasked || (frows >> (rr + i - r0) & 1u)) v = mask_value;
          else if (CUBIC) v = ((wt[0] * x[i][0] + wt[1] * x[i][1]) + wt[2] * x[i][2]) + wt[3] * x[i][3];
          else v = wt[0] * x[i][0] + wt[1] * x[i][1];
          out[row0 + (size_t)(rr + i) * T + t] = v;
        }
      }
    } else {
      const int sub = threadIdx.x >> 5, q = blockIdx.x * (kSaTile / 4) + (threadIdx.x & 31);
      const int tb = 4 * q - 3;  // the seven frames a quad of this work-item can touch: tb .. tb + 6
      if (tb >= T) continue;
      const unsigned tmasked7 = sa_bits(tlo, thi, tb, 7);
      const int one_lo[1] = {0}, one_hi[1] = {n};
      const unsigned valid7 = sa_bits(one_lo, one_hi, tb, 7);
      // this work-item's rows, four at a time: whole quads are loaded first and stored after; quads over a row's end go as floats
      for (int rb = r0 + sub; rb < r1; rb += 16) {
      float4 v[4];
      unsigned masks[4];
      int at[4];
      int kind[4];  // 0 nothing, 1 a whole aligned quad, 2 a quad over the row's head or tail (or an unaligned tensor): single floats
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = rb + 4 * i;
        kind[i] = 0;
        if (r >= r1) continue;
        const size_t off = row0 + (size_t)r * T;
        const int a = vec_ok ? (int)(off & 3) : 0;
        const int e0 = 4 * q - a;
        if (e0 >= T) continue;
        masks[i] = ((frows >> (r - r0) & 1u) ? valid7 : tmasked7) >> (3 - a) & 15u;  // bit k: frame e0 + k becomes mask_value
        at[i] = e0;
        const float* __restrict__ src = mel + off;
        if (vec_ok && e0 >= 0 && e0 + 4 <= T) {
          kind[i] = 1;
          if (masks[i] != 15u) v[i] = *(const float4*)(src + e0);
        } else {  // frames outside the row are read at its nearest end and not stored
          kind[i] = 2;
          v[i].x = src[min(max(e0, 0), T - 1)], v[i].y = src[min(max(e0 + 1, 0), T - 1)];
          v[i].z = src[min(max(e0 + 2, 0), T - 1)], v[i].w = src[min(max(e0 + 3, 0), T - 1)];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (kind[i] == 0) continue;
        const unsigned m = masks[i];
        float4 u = v[i];
        u.x = (m & 1u) ? mask_value : u.x, u.y = (m & 2u) ? mask_value : u.y, u.z = (m & 4u) ? mask_value : u.z, u.w = (m & 8u) ? mask_value : u.w;
        float* __restrict__ dst = out + row0 + (size_t)(rb + 4 * i) * T;
        const int e0 = at[i];
        if (kind[i] == 1) {
          *(float4*)(dst + e0) = u;
        } else {
          if (e0 >= 0) dst[e0] = u.x;  // e0 < T
          if (e0 + 1 >= 0 && e0 + 1 < T) dst[e0 + 1] = u.y;
          if (e0 + 2 >= 0 && e0 + 2 < T) dst[e0 + 2] = u.z;
          if (e0 + 3 >= 0 && e0 + 3 < T) dst[e0 + 3] = u.w;
        }
      }
      }
    }
  }
}

__global__ __launch_bounds__(64) void specaug_draw_kernel(const int* __restrict__ frame_len, int B, int n_mels, int T, uint64_t seed,
                                                          uint64_t utt_offset, int W, int n_freq, int F, int n_time, double ratio, int Tmax,
                                                          int* __restrict__ params) {
  const int G = 1 + n_freq + n_time;
  const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
  if (id >= (long long)B * G) return;
  const int b = (int)(id / G), g = (int)(id % G);
  const int n = sa_len(frame_len, b, T);
  const uint32_t key = eect::drop_key(eect::Drop{0.0f, seed, EEC_SPECAUG_SITE});
  const uint64_t at = (utt_offset + (uint64_t)b) * 64u;
  auto below = [&](int slot, uint32_t m) { return (int)(((uint64_t)eect::drop_word(key, at + (uint64_t)slot) * m) >> 32); };
  int* __restrict__ p = params + (size_t)b * (2 * G);
  if (g == 0) {
    int c = 0, w = 0;
    if (W > 0 && (long long)n > 2LL * W) {
      c = W + below(0, (uint32_t)(n - 2 * W));
      w = c - W + 1 + below(1, (uint32_t)(2 * W));
    }
    p[0] = c, p[1] = w;
  } else if (g <= n_freq) {
    const int k = g - 1;
    const int fw = below(2 + 2 * k, (uint32_t)min(F, n_mels) + 1u);
    p[2 + 2 * k] = below(3 + 2 * k, (uint32_t)(n_mels - fw) + 1u);
    p[3 + 2 * k] = fw;
  } else {
    const int slot = 2 + 2 * n_freq + 2 * (g - 1 - n_freq);
    const double cap = floor(ratio * (double)n);
    const int most = min(Tmax, cap >= (double)n ? n : (int)cap);
    const int tw = below(slot, (uint32_t)most + 1u);
    p[slot] = below(slot + 1, (uint32_t)(n - tw) + 1u);
    p[slot + 1] = tw;
  }
}

static int specaug_check_shape(const char* who, int B, int n_mels, int T, int n_freq, int n_time) {
  using eech::fail;
  const std::string w(who);
  if (B < 0) return fail(EEC_ERR_BAD_ARG, w + ": B must not be negative, got " + std::to_string(B));
  if (n_mels < 1 || T < 1) return fail(EEC_ERR_BAD_ARG, w + ": n_mels and T must be positive, got " + std::to_string(n_mels) + " and " + std::to_string(T));
  if (n_freq < 0 || n_freq > EEC_SPECAUG_MAX_FREQ_MASKS)
    return fail(EEC_ERR_BAD_ARG, w + ": n_freq_masks must lie in [0, " + std::to_string(EEC_SPECAUG_MAX_FREQ_MASKS) + "], got " + std::to_string(n_freq));
  if (n_time < 0 || n_time > EEC_SPECAUG_MAX_TIME_MASKS)
    return fail(EEC_ERR_BAD_ARG, w + ": n_time_masks must lie in [0, " + std::to_string(EEC_SPECAUG_MAX_TIME_MASKS) + "], got " + std::to_string(n_time));
  return 0;
}

}  // namespace eec

extern "C" {

int eec_specaug_draw(const int32_t* frame_len, int B, int n_mels, int T, uint64_t seed, uint64_t utt_offset, int time_warp_window, int n_freq_masks,
                     int freq_mask_width, int n_time_masks, float time_mask_ratio, int time_mask_width, int32_t* params, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = specaug_check_shape("specaug draw", B, n_mels, T, n_freq_masks, n_time_masks)) return rc;
  if (time_warp_window < 0 || freq_mask_width < 0 || time_mask_width < 0)
    return fail(EEC_ERR_BAD_ARG, "specaug draw: time_warp_window, freq_mask_width and time_mask_width must not be negative, got " +
                                     std::to_string(time_warp_window) + ", " + std::to_string(freq_mask_width) + ", " + std::to_string(time_mask_width));
  if (!(time_mask_ratio >= 0.0f) || std::isinf(time_mask_ratio))
    return fail(EEC_ERR_BAD_ARG, "specaug draw: time_mask_ratio must be finite and not negative");
  if (B == 0) return 0;
  if (!params) return fail(EEC_ERR_BAD_ARG, "specaug draw: null params");
  const long long items = (long long)B * (1 + n_freq_masks + n_time_masks);
  hipLaunchKernelGGL(specaug_draw_kernel, dim3((unsigned)((items + 63) / 64)), dim3(64), 0, (hipStream_t)stream, frame_len, B, n_mels, T, seed,
                     utt_offset, time_warp_window, n_freq_masks, freq_mask_width, n_time_masks, (double)time_mask_ratio, time_mask_width, params);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_specaug_draw launch");
}

int eec_specaug_apply(const float* mel, const int32_t* frame_len, const int32_t* params, int B, int n_mels, int T, int n_freq_masks, int n_time_masks,
                      int mode, float mask_value, float* out, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = specaug_check_shape("specaug apply", B, n_mels, T, n_freq_masks, n_time_masks)) return rc;
  if (mode != EEC_SPECAUG_LINEAR && mode != EEC_SPECAUG_BICUBIC)
    return fail(EEC_ERR_BAD_ARG, "specaug apply: mode must be EEC_SPECAUG_LINEAR or EEC_SPECAUG_BICUBIC, got " + std::to_string(mode));
  if (std::isnan(mask_value)) return fail(EEC_ERR_BAD_ARG, "specaug apply: mask_value is NaN");
  if (B == 0) return 0;
  if (!mel || !params || !out) return fail(EEC_ERR_BAD_ARG, "specaug apply: null argument (mel, params, out)");
  if (mel == out) return fail(EEC_ERR_BAD_ARG, "specaug apply: out must not be mel (the warp reads frames other work-items write)");
  const int vec_ok = (((uintptr_t)mel | (uintptr_t)out) & 15) == 0;
  const long long quads = ((long long)T + 6) / 4;  // the most aligned quads a row can span
  const dim3 grid((unsigned)((quads + kSaTile / 4 - 1) / (kSaTile / 4)), (unsigned)((n_mels + kSaRows - 1) / kSaRows), (unsigned)(B < 65535 ? B : 65535));
  if (grid.y > 65535u) return fail(EEC_ERR_BAD_ARG, "specaug apply: n_mels above " + std::to_string(65535 * kSaRows) + " is not served");
  if (mode == EEC_SPECAUG_BICUBIC)
    hipLaunchKernelGGL((specaug_apply_kernel<true>), grid, dim3(kSaTile), 0, (hipStream_t)stream, mel, frame_len, params, B, n_mels, T, n_freq_masks,
                       n_time_masks, mask_value, vec_ok, out);
  else
    hipLaunchKernelGGL((specaug_apply_kernel<false>), grid, dim3(kSaTile), 0, (hipStream_t)stream, mel, frame_len, params, B, n_mels, T, n_freq_masks,
                       n_time_masks, mask_value, vec_ok, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_specaug_apply launch");
}

}  // extern "C"
