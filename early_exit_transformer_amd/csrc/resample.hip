// Batched polyphase sinc resampling of a waveform batch [B, L]: sample-rate conversion and speed perturbation.  The statement -- the
// filter, the order of the fp32 sum, the lengths, the draw and the layout of the plan image -- is in include/eec.h ("Resampling /
// speed perturbation").
//
// eec_resample_plan (host only): the phase tables of up to eight ratios in fp64, each weight rounded once to fp32, zero heads and tails
// dropped, as one image of int32 words the caller uploads once.
//
// eec_speed_draw / eec_resample_lengths: one work-item per utterance: the choice (drawn from the dropout generator of eec_drop.h, or
// prescribed) and ceil(n * len / o).
//
// eec_resample: one workgroup of 256 work-items per (tile of 1024 output samples, utterance); the utterance's ratio, and with it every
// choice below, is uniform per workgroup:
//   * a tile at or past out_len stores zeros; the ratio (1, 1) and a choice outside the plan copy (zeros past the length), a 16-byte
//     quad per work-item where both rows are 16-byte aligned, single floats otherwise and at the utterance's end;
//   * otherwise output i = q * n + j reads the input from q * o - width + first(j) on, count(j) taps.  The tile's input window is
//     staged in LDS with zeros outside [0, len) when it fits kWin floats, the ratio's weights when they fit kWts floats; what does not
//     fit is read through the caches (long filters: a large o against n = 1, a wide lowpass_filter_width).  Work-item t owns the
//     outputs tile + t, + 256, + 512, + 768: a wave stores 256 consecutive bytes, whatever the alignment of the row.
#include "../../include/eec.h"
#include "eec_drop.h"
#include "eec_host.h"

#include <cmath>
#include <numeric>
#include <vector>

namespace eec {

constexpr int kRsThreads = 256;
constexpr int kRsTile = 1024;  // output samples per workgroup
static_assert(kRsTile == 4 * kRsThreads, "the copy path moves one quad per work-item");
constexpr int kRsWin = 4096;   // floats of LDS for the input window
constexpr int kRsWts = 6144;   // floats of LDS for a ratio's weights
constexpr int kRsHead = 4, kRsRec = 8;  // words of the image's header and of a ratio's record

// ---------------------------------------------------------------------------------------------------------------------------
// the plan (host)
// ---------------------------------------------------------------------------------------------------------------------------
struct RsPhase {
  int first, count;
  std::vector<float> w;
};
struct RsRatio {
  int o, n, width, K, most;
  long long total;
  std::vector<RsPhase> phases;
};

static int rs_check_plan_args(int R, const int32_t* orig, const int32_t* new_, int lpw, double rolloff) {
  using eech::fail;
  if (R < 1 || R > EEC_RESAMPLE_MAX_RATIOS)
    return fail(EEC_ERR_BAD_ARG, "resample plan: the number of ratios must lie in [1, " + std::to_string(EEC_RESAMPLE_MAX_RATIOS) + "], got " + std::to_string(R));
  if (!orig || !new_) return fail(EEC_ERR_BAD_ARG, "resample plan: null argument (orig, new)");
  if (lpw < 1 || lpw > EEC_RESAMPLE_MAX_LPW)
    return fail(EEC_ERR_BAD_ARG, "resample plan: lowpass_filter_width must lie in [1, " + std::to_string(EEC_RESAMPLE_MAX_LPW) + "], got " + std::to_string(lpw));
  if (!(rolloff > 0.0) || !(rolloff <= 1.0)) return fail(EEC_ERR_BAD_ARG, "resample plan: rolloff must lie in (0, 1], got " + std::to_string(rolloff));
  for (int r = 0; r < R; ++r) {
    if (orig[r] < 1 || new_[r] < 1)
      return fail(EEC_ERR_BAD_ARG, "resample plan: rates must be positive, got " + std::to_string(orig[r]) + " and " + std::to_string(new_[r]));
    const int g = std::gcd(orig[r], new_[r]);
    if (orig[r] / g > EEC_RESAMPLE_MAX_RATE || new_[r] / g > EEC_RESAMPLE_MAX_RATE)
      return fail(EEC_ERR_BAD_ARG, "resample plan: ratio " + std::to_string(orig[r] / g) + " / " + std::to_string(new_[r] / g) + " exceeds " +
                                       std::to_string(EEC_RESAMPLE_MAX_RATE) + " after reduction");
  }
  return 0;
}

static RsRatio rs_ratio(int orig, int new_, int lpw, double rolloff) {
#pragma clang fp contract(off)  // the table is the stated fp64 expression, operation by operation
  const double pi = 3.14159265358979323846;
  RsRatio q;
  const int g = std::gcd(orig, new_);
  q.o = orig / g, q.n = new_ / g;
  const double base = (double)(q.o < q.n ? q.o : q.n) * rolloff;
  q.width = (int)std::ceil((double)(lpw * q.o) / base);
  q.K = 2 * q.width + q.o;
  q.most = 0, q.total = 0;
  q.phases.resize(q.n);
  const double scale = base / (double)q.o;
  std::vector<float> row(q.K);
  for (int j = 0; j < q.n; ++j) {
    for (int k = 0; k < q.K; ++k) {
      double t = ((double)(-j) / (double)q.n + (double)(k - q.width) / (double)q.o) * base;
      t = t < -(double)lpw ? -(double)lpw : t > (double)lpw ? (double)lpw : t;
      const double c = std::cos(t * pi / (double)lpw / 2.0);
      const double a = t * pi;
      const double s = a == 0.0 ? 1.0 : std::sin(a) / a;
      row[k] = (float)(s * (c * c * scale));
    }
    int lo = 0, hi = q.K;
    while (lo < hi && row[lo] == 0.0f) ++lo;
    while (hi > lo && row[hi - 1] == 0.0f) --hi;
    RsPhase& p = q.phases[j];
    p.first = lo, p.count = hi - lo;
    p.w.assign(row.begin() + lo, row.begin() + hi);
    q.total += p.count;
    if (p.count > q.most) q.most = p.count;
  }
  return q;
}

static size_t rs_words(const std::vector<RsRatio>& qs) {
  size_t words = kRsHead + kRsRec * qs.size();
  for (const RsRatio& q : qs) words += 3 * (size_t)q.n + (size_t)q.total;
  return words;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the kernels
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long rs_len(const int64_t* __restrict__ lengths, int b, int L) {
  const long long n = lengths ? (long long)lengths[b] : (long long)L;
  return n < 0 ? 0 : n > L ? L : n;
}
// record of the ratio utterance b takes, or nullptr: a copy (a choice outside the plan, or o == n == 1)
__device__ __forceinline__ const int* rs_record(const int* __restrict__ plan, int c) {
  const int R = plan[1];
  if (c < 0 || c >= R || R > EEC_RESAMPLE_MAX_RATIOS) return nullptr;
  const int* rec = plan + kRsHead + kRsRec * c;
  return rec[0] == 1 && rec[1] == 1 ? nullptr : rec;
}
__device__ __forceinline__ long long rs_out_len(const int* rec, long long len) {
  return rec ? ((long long)rec[1] * len + rec[0] - 1) / rec[0] : len;
}

__global__ __launch_bounds__(64) void resample_lengths_kernel(const int64_t* __restrict__ lengths, const int* __restrict__ choice_in, int B, int L,
                                                              int draw, uint64_t seed, uint64_t utt_offset, const int* __restrict__ plan,
                                                              int* __restrict__ choice_out, int64_t* __restrict__ out_len) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int c;
  if (draw) {
    const uint32_t key = eect::drop_key(eect::Drop{0.0f, seed, EEC_SPEED_SITE});
    const int R = plan[1];
    c = (int)(((uint64_t)eect::drop_word(key, (utt_offset + (uint64_t)b) * 64u) * (uint32_t)(R < 0 ? 0 : R)) >> 32);
    choice_out[b] = c;
  } else {
    c = choice_in[b];
  }
  out_len[b] = rs_out_len(rs_record(plan, c), rs_len(lengths, b, L));
}

template <bool XLDS, bool WLDS>
__device__ __forceinline__ void rs_tile(const float* __restrict__ x, long long len, const int* __restrict__ ph, const float* __restrict__ wg,
                                        const float* xs, const float* ws, int o, int n, int width, long long in0, long long i0, long long i1,
                                        float* __restrict__ y) {
#pragma clang fp contract(off)  // one rounded multiply and one rounded add per tap
  for (long long i = i0 + threadIdx.x; i < i1; i += kRsThreads) {
    const unsigned q32 = (unsigned)i / (unsigned)n;  // i < L_out < 2^31
    const int j = (int)((unsigned)i - q32 * (unsigned)n);
    const long long q = q32;
    const int first = ph[3 * j], count = ph[3 * j + 1], at = ph[3 * j + 2];
    const long long g0 = q * o - width + first;  // the input sample of the first stored tap
    const float* __restrict__ w = WLDS ? ws + at : wg + at;
    float acc = 0.0f;
    if (XLDS) {
      const float* __restrict__ s = xs + (int)(g0 - in0);
#pragma unroll 4  // four taps a trip: their weights and samples come as two-dword LDS reads, the sum still adds them one by one in order
      for (int k = 0; k < count; ++k) acc = acc + w[k] * s[k];
    } else {
      for (int k = 0; k < count; ++k) {
        const long long g = g0 + k;
        acc = acc + w[k] * (g >= 0 && g < len ? x[g] : 0.0f);
      }
    }
    y[i] = acc;
  }
}

__global__ __launch_bounds__(kRsThreads) void resample_kernel(const float* __restrict__ wave, const int64_t* __restrict__ lengths,
                                                              const int* __restrict__ choice, int B, int L, const int* __restrict__ plan,
                                                              float* __restrict__ out, int L_out, int64_t* __restrict__ out_len) {
  __shared__ float xs[kRsWin];
  __shared__ float ws[kRsWts];
  const long long i0 = (long long)blockIdx.x * kRsTile;
  const long long i1 = i0 + kRsTile < L_out ? i0 + kRsTile : L_out;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // one pass unless B exceeds the grid's y limit
    const long long len = rs_len(lengths, b, L);
    const int* rec = rs_record(plan, choice[b]);
    long long n_out = rs_out_len(rec, len);
    if (n_out > L_out) n_out = L_out;
    if (blockIdx.x == 0 && threadIdx.x == 0 && out_len) out_len[b] = n_out;
    const float* __restrict__ x = wave + (size_t)b * L;
    float* __restrict__ y = out + (size_t)b * L_out;
    const long long v1 = i1 < n_out ? i1 : n_out;  // outputs [i0, v1) are computed, [max(i0, v1), i1) are zeros
    for (long long i = (v1 > i0 ? v1 : i0) + threadIdx.x; i < i1; i += kRsThreads) y[i] = 0.0f;
    if (v1 <= i0) continue;
    if (!rec) {  // n_out == len <= L.  A 16-byte quad per work-item where both rows are aligned (the tile starts a multiple of 4 in)
      const long long i = i0 + 4 * threadIdx.x;
      if (i + 4 <= v1 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
        *(float4*)(y + i) = *(const float4*)(x + i);
      } else {
        for (int k = 0; k < 4; ++k)
          if (i + k < v1) y[i + k] = x[i + k];
      }
      continue;
    }
    const int o = rec[0], n = rec[1], width = rec[2], K = rec[3], total = rec[6];
    const int* __restrict__ ph = plan + rec[4];
    const float* __restrict__ wg = (const float*)(plan + rec[5]);
    const long long q0 = i0 / n, q1 = (v1 - 1) / n;
    const long long in0 = q0 * o - width, span = (q1 - q0) * o + K;  // every tap of the tile lies in [in0, in0 + span)
    const bool xl = span <= kRsWin, wl = total <= kRsWts;
    __syncthreads();  // the previous utterance's readers are done with the LDS
    if (xl)
      for (int t = threadIdx.x; t < (int)span; t += kRsThreads) {
        const long long g = in0 + t;
        xs[t] = g >= 0 && g < len ? x[g] : 0.0f;
      }
    if (wl)
      for (int t = threadIdx.x; t < total; t += kRsThreads) ws[t] = wg[t];
    __syncthreads();
    if (xl && wl) rs_tile<true, true>(x, len, ph, wg, xs, ws, o, n, width, in0, i0, v1, y);
    else if (xl) rs_tile<true, false>(x, len, ph, wg, xs, ws, o, n, width, in0, i0, v1, y);
    else if (wl) rs_tile<false, true>(x, len, ph, wg, xs, ws, o, n, width, in0, i0, v1, y);
    else rs_tile<false, false>(x, len, ph, wg, xs, ws, o, n, width, in0, i0, v1, y);
  }
}

static int rs_check_batch(const char* who, int B, int L) {
  using eech::fail;
  const std::string w(who);
  if (B < 0) return fail(EEC_ERR_BAD_ARG, w + ": B must not be negative, got " + std::to_string(B));
  if (L < 0 || L > (1 << 30)) return fail(EEC_ERR_BAD_ARG, w + ": L must lie in [0, 2^30], got " + std::to_string(L));
  return 0;
}

static int rs_lengths_launch(const char* who, const int64_t* lengths, const int32_t* choice_in, int B, int L, int draw, uint64_t seed,
                             uint64_t utt_offset, const void* plan, int32_t* choice_out, int64_t* out_len, void* stream) {
  hipLaunchKernelGGL(resample_lengths_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, lengths, choice_in, B, L, draw, seed,
                     utt_offset, (const int*)plan, choice_out, out_len);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, who);
}

}  // namespace eec

extern "C" {

size_t eec_resample_plan_bytes(int R, const int32_t* orig, const int32_t* new_, int lowpass_filter_width, double rolloff) {
  using namespace eec;
  if (rs_check_plan_args(R, orig, new_, lowpass_filter_width, rolloff)) return 0;
  std::vector<RsRatio> qs;
  for (int r = 0; r < R; ++r) qs.push_back(rs_ratio(orig[r], new_[r], lowpass_filter_width, rolloff));
  return 4 * rs_words(qs);
}

int eec_resample_plan(int R, const int32_t* orig, const int32_t* new_, int lowpass_filter_width, double rolloff, void* image, size_t image_bytes) {
  using namespace eec;
  using eech::fail;
  if (int rc = rs_check_plan_args(R, orig, new_, lowpass_filter_width, rolloff)) return rc;
  if (!image) return fail(EEC_ERR_BAD_ARG, "resample plan: null image");
  std::vector<RsRatio> qs;
  for (int r = 0; r < R; ++r) qs.push_back(rs_ratio(orig[r], new_[r], lowpass_filter_width, rolloff));
  const size_t words = rs_words(qs);
  if (image_bytes < 4 * words)
    return fail(EEC_ERR_WORKSPACE, "resample plan: the image needs " + std::to_string(4 * words) + " bytes, got " + std::to_string(image_bytes));
  int32_t* img = (int32_t*)image;
  img[0] = EEC_RESAMPLE_MAGIC, img[1] = R, img[2] = (int32_t)words, img[3] = lowpass_filter_width;
  size_t at = kRsHead + kRsRec * (size_t)R;
  for (int r = 0; r < R; ++r) {
    const RsRatio& q = qs[r];
    int32_t* rec = img + kRsHead + kRsRec * r;
    const size_t phases = at, weights = at + 3 * (size_t)q.n;
    rec[0] = q.o, rec[1] = q.n, rec[2] = q.width, rec[3] = q.K, rec[4] = (int32_t)phases, rec[5] = (int32_t)weights, rec[6] = (int32_t)q.total,
    rec[7] = q.most;
    int32_t off = 0;
    for (int j = 0; j < q.n; ++j) {
      const RsPhase& p = q.phases[j];
      img[phases + 3 * j] = p.first, img[phases + 3 * j + 1] = p.count, img[phases + 3 * j + 2] = off;
      float* w = (float*)(img + weights + off);
      for (int k = 0; k < p.count; ++k) w[k] = p.w[k];
      off += p.count;
    }
    at = weights + (size_t)q.total;
  }
  return 0;
}

int eec_speed_draw(const int64_t* lengths, int B, int L, uint64_t seed, uint64_t utt_offset, const void* plan, int32_t* choice, int64_t* out_len,
                   void* stream) {
  using namespace eec;
  if (int rc = rs_check_batch("speed draw", B, L)) return rc;
  if (B == 0) return 0;
  if (!plan || !choice || !out_len) return eech::fail(EEC_ERR_BAD_ARG, "speed draw: null argument (plan, choice, out_len)");
  return rs_lengths_launch("eec_speed_draw launch", lengths, nullptr, B, L, 1, seed, utt_offset, plan, choice, out_len, stream);
}

int eec_resample_lengths(const int64_t* lengths, const int32_t* choice, int B, int L, const void* plan, int64_t* out_len, void* stream) {
  using namespace eec;
  if (int rc = rs_check_batch("resample lengths", B, L)) return rc;
  if (B == 0) return 0;
  if (!plan || !choice || !out_len) return eech::fail(EEC_ERR_BAD_ARG, "resample lengths: null argument (plan, choice, out_len)");
  return rs_lengths_launch("eec_resample_lengths launch", lengths, choice, B, L, 0, 0, 0, plan, nullptr, out_len, stream);
}

int eec_resample(const float* wave, const int64_t* lengths, const int32_t* choice, int B, int L, const void* plan, float* out, int L_out,
                 int64_t* out_len, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = rs_check_batch("resample", B, L)) return rc;
  if (L_out < 0) return fail(EEC_ERR_BAD_ARG, "resample: L_out must not be negative, got " + std::to_string(L_out));
  if (B == 0) return 0;
  if (!choice || !plan || (L > 0 && !wave) || (L_out > 0 && !out)) return fail(EEC_ERR_BAD_ARG, "resample: null argument (wave, choice, plan, out)");
  if (wave && wave == out) return fail(EEC_ERR_BAD_ARG, "resample: out must not be wave (an output reads samples other work-items overwrite)");
  const unsigned tiles = L_out > 0 ? (unsigned)(((long long)L_out + kRsTile - 1) / kRsTile) : 1u;  // one workgroup still writes out_len
  hipLaunchKernelGGL(resample_kernel, dim3(tiles, (unsigned)(B < 65535 ? B : 65535)), dim3(kRsThreads), 0, (hipStream_t)stream, wave, lengths, choice, B,
                     L, (const int*)plan, out, L_out, out_len);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_resample launch");
}

}  // extern "C"
