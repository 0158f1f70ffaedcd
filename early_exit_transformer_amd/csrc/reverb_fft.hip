// Reverberation by FFT: the convolution of waveaug.hip's eec_reverb, y[i] = sum_k h[k] x[i + d - k], evaluated by uniformly partitioned
// overlap-save in output coordinates.  The statement, the layout of the spectral image and the error bound are in include/eec.h
// ("Reverberation by FFT").
//
// S = EEC_REVERB_FFT_BLOCK outputs per block, N = 2 S points per transform.  A real sequence of N points is transformed as the complex
// sequence z[n] = x[2 n] + i x[2 n + 1] of M = N / 2 points followed by the split X[k] = E[k] + W_N^k O[k]; its spectrum is stored as M
// complex words, the real Nyquist bin beside DC in word 0.
//
// eec_rir_spectra (host only): the RIRs of a tap image cut into partitions of S taps, each transformed in fp64 and rounded once, and
// the fp32 twiddles W_N^u, u < N / 2, the kernels read (no sincos on the device).
//
// reverb_fft_windows_kernel: one workgroup of 256 work-items per (input window, utterance).  Window j is x[(j - 1) S + d, (j + 1) S + d),
// zeros outside [0, len).  The M-point transform runs in LDS as four Stockham passes (radix 8, 8, 8, 4) with the butterflies in
// registers; LDS word i sits at i + i / 8 so that the strided stores of a pass spread over the banks.  The split writes the spectrum
// to the workspace.  Windows without a valid sample, or that no block of the utterance meets, are skipped.
//
// reverb_fft_blocks_kernel: one workgroup per (output block, utterance).  Work-item t accumulates Y[k] = sum_p X_{m-p}[k] H_p[k], p in
// order, for k = t + 256 r and its mirror M - k (r < 4; the mirror of 0 is M / 2) in 16 registers, merges them to the complex
// sequence, transforms back in LDS (the forward passes on the conjugate) and keeps the last S of the N samples.  The block leaves
// through LDS, so a wave stores 256 consecutive bytes whatever the row's alignment; the energies of its two tiles come from the stored
// values in the stated order (eec_waveaug.h).
#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_waveaug.h"

#include <cmath>
#include <vector>

namespace eec {

constexpr int kRfS = EEC_REVERB_FFT_BLOCK;
constexpr int kRfN = 2 * kRfS;
constexpr int kRfM = kRfN / 2;  // complex points per transform, complex words per spectrum
constexpr int kRfThreads = 256;
constexpr int kRfMaxP = EEC_REVERB_MAX_TAPS / kRfS;
constexpr int kRfHead = 8, kRfRec = 2;  // words of the spectral image's header and of a record
constexpr int kRfLds = kRfM + kRfM / 8;
static_assert(kRfS == 2048 && kRfM == 8 * 8 * 8 * 4, "the passes below are radix 8, 8, 8, 4");
static_assert(kRfS % kWaTile == 0 && kRfS == kRfThreads * kWaPer, "a work-item owns eight consecutive outputs; tiles never straddle blocks");
static_assert(kRfMaxP * kRfS == EEC_REVERB_MAX_TAPS, "partitions of the longest RIR");

// ---------------------------------------------------------------------------------------------------------------------------
// the spectral image (host)
// ---------------------------------------------------------------------------------------------------------------------------
// exp(-2 pi i u / n) in fp64, u in [0, n), n a multiple of 8: evaluated in the first octant and reflected, so exact on the axes
static void rf_unit(int u, int n, double& re, double& im) {
  const double kTwoPi = 6.283185307179586476925286766559;
  const int quarter = n / 4, q = u / quarter, r = u % quarter;
  double c, s;
  if (2 * r <= quarter) c = std::cos(kTwoPi * r / n), s = std::sin(kTwoPi * r / n);
  else c = std::sin(kTwoPi * (quarter - r) / n), s = std::cos(kTwoPi * (quarter - r) / n);
  const double cq = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
  const double sq = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
  re = cq, im = -sq;
}

// in-place radix-2 decimation in time of n = 2^k complex points in fp64; w[u] = exp(-2 pi i u / n), u < n / 2
static void rf_host_fft(std::vector<double>& re, std::vector<double>& im, const std::vector<double>& wr, const std::vector<double>& wi) {
  const int n = (int)re.size();
  for (int i = 1, j = 0; i < n; ++i) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(re[i], re[j]), std::swap(im[i], im[j]);
  }
  for (int half = 1; half < n; half <<= 1) {
    const int step = n / (2 * half);
    for (int base = 0; base < n; base += 2 * half)
      for (int k = 0; k < half; ++k) {
        const double cr = wr[k * step], ci = wi[k * step];
        const int a = base + k, b = a + half;
        const double tr = re[b] * cr - im[b] * ci, ti = re[b] * ci + im[b] * cr;
        re[b] = re[a] - tr, im[b] = im[a] - ti;
        re[a] = re[a] + tr, im[a] = im[a] + ti;
      }
  }
}

static size_t rf_round4(size_t words) { return (words + 3) & ~(size_t)3; }

// checks the tap image and returns the words of its spectral image
static int rf_spectra_words(const void* rir_bank_image, size_t& words) {
  using eech::fail;
  if (!rir_bank_image) return fail(EEC_ERR_BAD_ARG, "rir spectra: null tap image");
  const int32_t* bank = (const int32_t*)rir_bank_image;
  const int R = bank[1];
  if (bank[0] != EEC_RIR_MAGIC || R < 1 || R > EEC_WAVEAUG_MAX_BANK || bank[2] < kWaHead + kWaRirRec * R)
    return fail(EEC_ERR_BAD_ARG, "rir spectra: the tap image is not one eec_rir_bank wrote");
  words = rf_round4(kRfHead + kRfRec * (size_t)R) + kRfN;
  for (int r = 0; r < R; ++r) {
    const int32_t* rec = bank + kWaHead + kWaRirRec * r;
    if (rec[0] < 1 || rec[0] > EEC_REVERB_MAX_TAPS || rec[2] < 0 || (long long)rec[2] + rec[0] > bank[2])
      return fail(EEC_ERR_BAD_ARG, "rir spectra: RIR " + std::to_string(r) + " of the tap image is out of range");
    words += (size_t)((rec[0] + kRfS - 1) / kRfS) * kRfN;
  }
  if (words >= (1ull << 31)) return fail(EEC_ERR_BAD_ARG, "rir spectra: the image would have 2^31 words or more");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the kernels
// ---------------------------------------------------------------------------------------------------------------------------
struct RfRir {
  int P, d;
  const float2* H;   // P spectra of M complex words
  const float2* tw;  // W_N^u, u < N / 2
};

// RIR `at` of the bank with its spectra, or false: the utterance is copied (no bank, no spectra, an index outside the bank, a spectral
// image that is not the bank's)
__device__ __forceinline__ bool rf_rir(const int* __restrict__ bank, const int* __restrict__ spec, int at, RfRir& q) {
  const int* rec = wa_record(bank, at, kWaRirRec);
  if (!rec || !spec || spec[0] != EEC_RIR_SPECTRA_MAGIC || spec[1] != bank[1] || spec[3] != kRfS) return false;
  const int* srec = spec + kRfHead + kRfRec * at;
  q.P = srec[0], q.d = rec[1];
  if (q.P < 1 || q.P > kRfMaxP) return false;
  q.H = (const float2*)(spec + srec[1]);
  q.tw = (const float2*)(spec + spec[4]);
  return true;
}

// does window j hold a sample of [0, len)?
__device__ __forceinline__ bool rf_window_live(int j, int d, long long len) {
  const long long g0 = (long long)(j - 1) * kRfS + d;
  return g0 < len && g0 + kRfN > 0;
}

__device__ __forceinline__ int rf_at(int i) { return i + (i >> 3); }
__device__ __forceinline__ float2 rf_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 rf_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 rf_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 rf_mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)
// W_M^t, t in [0, M), from the table of W_N^u, u < N / 2: W_N^(u + N / 2) = -W_N^u
__device__ __forceinline__ float2 rf_wm(const float2* __restrict__ tw, int t) {
  const float2 w = tw[(2 * t) & (kRfM - 1)];
  return 2 * t >= kRfM ? make_float2(-w.x, -w.y) : w;
}

__device__ __forceinline__ void rf_dft4(float2& a, float2& b, float2& c, float2& e) {
  const float2 t0 = rf_add(a, c), t1 = rf_sub(a, c), t2 = rf_add(b, e), t3 = rf_mul_mi(rf_sub(b, e));
  a = rf_add(t0, t2), b = rf_add(t1, t3), c = rf_sub(t0, t2), e = rf_sub(t1, t3);
}
template <int R>
__device__ __forceinline__ void rf_dft(float2 (&v)[R]) {
  if constexpr (R == 4) {
    rf_dft4(v[0], v[1], v[2], v[3]);
  } else {
    static_assert(R == 8, "radix 4 or 8");
    constexpr float h = 0.70710678118654752440f;
    rf_dft4(v[0], v[2], v[4], v[6]);
    rf_dft4(v[1], v[3], v[5], v[7]);
    const float2 o1 = make_float2(h * (v[3].x + v[3].y), h * (v[3].y - v[3].x));   // * (1 - i) / sqrt 2
    const float2 o2 = rf_mul_mi(v[5]);
    const float2 o3 = make_float2(h * (v[7].y - v[7].x), -h * (v[7].x + v[7].y));  // * (-1 - i) / sqrt 2
    const float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1];
    v[0] = rf_add(e0, o0), v[4] = rf_sub(e0, o0);
    v[1] = rf_add(e1, o1), v[5] = rf_sub(e1, o1);
    v[2] = rf_add(e2, o2), v[6] = rf_sub(e2, o2);
    v[3] = rf_add(e3, o3), v[7] = rf_sub(e3, o3);
  }
}

// one Stockham pass of radix R over the M points in LDS; Ns is the product of the radices before it.  Ends synchronised.
template <int R, int Ns>
__device__ __forceinline__ void rf_pass(float2* z, const float2* __restrict__ tw, int tid) {
  constexpr int J = kRfM / R, per = J / kRfThreads;
  float2 v[per][R];
#pragma unroll
  for (int q = 0; q < per; ++q)
#pragma unroll
    for (int r = 0; r < R; ++r) v[q][r] = z[rf_at(tid + q * kRfThreads + r * J)];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < per; ++q) {
    const int j = tid + q * kRfThreads, k = j & (Ns - 1);
    if constexpr (Ns > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) v[q][r] = rf_mul(v[q][r], rf_wm(tw, r * k * (kRfM / (Ns * R))));
    }
    rf_dft<R>(v[q]);
    const int j0 = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) z[rf_at(j0 + r * Ns)] = v[q][r];
  }
  __syncthreads();
}

// Z[k] = sum_n z[n] exp(-2 pi i n k / M) in place, in natural order.  Expects the LDS synchronised and leaves it so.
__device__ __forceinline__ void rf_fft(float2* z, const float2* __restrict__ tw, int tid) {
  rf_pass<8, 1>(z, tw, tid);
  rf_pass<8, 8>(z, tw, tid);
  rf_pass<8, 64>(z, tw, tid);
  rf_pass<4, 512>(z, tw, tid);
}

__global__ __launch_bounds__(kRfThreads) void reverb_fft_windows_kernel(const float* __restrict__ wave, const int64_t* __restrict__ lengths,
                                                                        const int* __restrict__ params, int B, int L,
                                                                        const int* __restrict__ bank, const int* __restrict__ spec,
                                                                        float2* __restrict__ ws, int n_slots) {
  __shared__ __attribute__((aligned(16))) float2 z[kRfLds];
  const int tid = threadIdx.x;
  const int j = (int)blockIdx.x - (kRfMaxP - 1);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // one pass unless B exceeds the grid's y limit
    const long long len = wa_len(lengths, b, L);
    RfRir q;
    if (!rf_rir(bank, spec, params[(size_t)b * kWaP], q)) continue;  // uniform per workgroup, as every skip below
    const long long blocks = (len + kRfS - 1) / kRfS;
    if (j + q.P - 1 < 0 || j >= blocks || !rf_window_live(j, q.d, len)) continue;
    const float* __restrict__ x = wave + (size_t)b * L;
    const long long g0 = (long long)(j - 1) * kRfS + q.d;
    __syncthreads();  // the previous utterance's readers are done with the LDS
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int n = tid + r * kRfThreads;
      const long long g = g0 + 2 * n;
      z[rf_at(n)] = make_float2(g >= 0 && g < len ? x[g] : 0.0f, g + 1 >= 0 && g + 1 < len ? x[g + 1] : 0.0f);
    }
    __syncthreads();
    rf_fft(z, q.tw, tid);
    float2* __restrict__ X = ws + ((size_t)b * n_slots + blockIdx.x) * kRfM;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = tid + r * kRfThreads;
      if (k == 0) {
        const float2 a = z[rf_at(0)], c = z[rf_at(kRfM / 2)];
        X[0] = make_float2(a.x + a.y, a.x - a.y);  // DC, Nyquist
        X[kRfM / 2] = make_float2(c.x, -c.y);
      } else {
        const float2 a = z[rf_at(k)], c = z[rf_at(kRfM - k)];
        const float2 e = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));  // E[k] = (Z[k] + conj Z[M - k]) / 2
        const float2 o = make_float2(0.5f * (a.y + c.y), 0.5f * (c.x - a.x));  // O[k] = (Z[k] - conj Z[M - k]) / (2 i)
        const float2 t = rf_mul(q.tw[k], o);
        X[k] = rf_add(e, t);
        X[kRfM - k] = make_float2(e.x - t.x, t.y - e.y);  // conj (E[k] - W_N^k O[k])
      }
    }
  }
}

__global__ __launch_bounds__(kRfThreads) void reverb_fft_blocks_kernel(const float* __restrict__ wave, const int64_t* __restrict__ lengths,
                                                                       const int* __restrict__ params, int B, int L,
                                                                       const int* __restrict__ bank, const int* __restrict__ spec,
                                                                       const float2* __restrict__ ws, int n_slots, float* __restrict__ out,
                                                                       double* __restrict__ partials, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float2 z[kRfLds];
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  const int m = (int)blockIdx.x;
  const long long i0 = (long long)m * kRfS;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long len = wa_len(lengths, b, L);
    const float* __restrict__ x = wave + (size_t)b * L;
    float* __restrict__ y = out + (size_t)b * L;
    const long long left = len - (i0 + kWaPer * tid);  // of the work-item's eight samples, min(left, 8) lie below len
    const int valid = left < 0 ? 0 : left > kWaPer ? kWaPer : (int)left;
    if (len <= i0) {  // past the utterance: zeros (and zero partials, which eec_noise_mix never adds)
      for (long long i = i0 + tid; i < i0 + kRfS && i < L; i += kRfThreads) y[i] = 0.0f;
      if (partials && tid < 2 && 2 * m + tid < n_tiles) partials[((size_t)b * n_tiles + 2 * m + tid) * 2] = 0.0;
      continue;
    }
    RfRir q;
    const bool on = rf_rir(bank, spec, params[(size_t)b * kWaP], q);
    float acc[kWaPer];
#pragma unroll
    for (int j = 0; j < kWaPer; ++j) acc[j] = 0.0f;
    __syncthreads();  // the previous utterance's readers are done with the LDS
    if (!on) {  // a copy, as eec_reverb makes it
      const long long i = i0 + kWaPer * tid;
      if (valid == kWaPer && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
        const float4 a = *(const float4*)(x + i), c = *(const float4*)(x + i + 4);
        *(float4*)(y + i) = a, *(float4*)(y + i + 4) = c;
        acc[0] = a.x, acc[1] = a.y, acc[2] = a.z, acc[3] = a.w, acc[4] = c.x, acc[5] = c.y, acc[6] = c.z, acc[7] = c.w;
      } else {
#pragma unroll
        for (int j = 0; j < kWaPer; ++j) {
          if (j < valid) acc[j] = x[i + j];
          if (i + j < L) y[i + j] = acc[j];
        }
      }
    } else {
      float2 lo[4], hi[4];  // Y[k] and Y[M - k], k = tid + 256 r (Y[0] = DC, Nyquist; its mirror is Y[M / 2])
#pragma unroll
      for (int r = 0; r < 4; ++r) lo[r] = hi[r] = make_float2(0.0f, 0.0f);
      bool any = false;
      for (int p = 0; p < q.P; ++p) {
        if (!rf_window_live(m - p, q.d, len)) continue;
        any = true;
        const float2* __restrict__ X = ws + ((size_t)b * n_slots + (m - p + kRfMaxP - 1)) * kRfM;
        const float2* __restrict__ H = q.H + (size_t)p * kRfM;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = tid + r * kRfThreads, km = k ? kRfM - k : kRfM / 2;
          const float2 xa = X[k], ha = H[k], xc = X[km], hc = H[km];
          if (k == 0) lo[r].x += xa.x * ha.x, lo[r].y += xa.y * ha.y;
          else lo[r] = rf_add(lo[r], rf_mul(xa, ha));
          hi[r] = rf_add(hi[r], rf_mul(xc, hc));
        }
      }
      float* zf = (float*)z;
      if (any) {
        // 2 Z[k] = (Y[k] + conj Y[M - k]) + i conj(W_N^k) (Y[k] - conj Y[M - k]); its conjugate goes through the forward passes
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = tid + r * kRfThreads;
          if (k == 0) {
            z[rf_at(0)] = make_float2(lo[r].x + lo[r].y, lo[r].y - lo[r].x);
            z[rf_at(kRfM / 2)] = make_float2(2.0f * hi[r].x, 2.0f * hi[r].y);
          } else {
            const float2 w = q.tw[k];
            const float2 e = make_float2(lo[r].x + hi[r].x, lo[r].y - hi[r].y);
            const float2 f = make_float2(lo[r].x - hi[r].x, lo[r].y + hi[r].y);
            const float2 o = rf_mul(f, make_float2(w.x, -w.y));
            z[rf_at(k)] = make_float2(e.x - o.y, -(e.y + o.x));
            z[rf_at(kRfM - k)] = make_float2(e.x + o.y, e.y - o.x);
          }
        }
        __syncthreads();
        rf_fft(z, q.tw, tid);
        constexpr float scale = 1.0f / kRfN;  // a power of two: exact
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float2 v = z[rf_at(kRfM / 2 + 4 * tid + u)];
          acc[2 * u] = 2 * u < valid ? v.x * scale + 0.0f : 0.0f;  // + 0.0f: a zero leaves as +0.0
          acc[2 * u + 1] = 2 * u + 1 < valid ? 0.0f - v.y * scale : 0.0f;
        }
        __syncthreads();  // every work-item has its outputs: the block leaves through the same LDS
      }
#pragma unroll
      for (int j = 0; j < kWaPer; ++j) zf[kWaPer * tid + j] = acc[j];
      __syncthreads();
      for (int o = tid; o < kRfS && i0 + o < L; o += kRfThreads) y[i0 + o] = i0 + o < len ? zf[o] : 0.0f;
    }
    if (partials) {  // uniform per launch: the stated order of a tile, two tiles per block
      double e = wa_own_energy(acc, valid);
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) e = e + __shfl_down(e, s, 64);
      if ((tid & 63) == 0) wsum[tid >> 6] = e;
      __syncthreads();
      if (tid < 2 && 2 * m + tid < n_tiles) partials[((size_t)b * n_tiles + 2 * m + tid) * 2] = wsum[2 * tid] + wsum[2 * tid + 1];
    }
  }
}

static int rf_blocks(int L) { return (L + kRfS - 1) / kRfS; }

}  // namespace eec

extern "C" {

size_t eec_rir_spectra_bytes(const void* rir_bank_image) {
  size_t words = 0;
  return eec::rf_spectra_words(rir_bank_image, words) ? 0 : 4 * words;
}

int eec_rir_spectra(const void* rir_bank_image, void* image, size_t image_bytes) {
  using namespace eec;
  using eech::fail;
  size_t words = 0;
  if (int rc = rf_spectra_words(rir_bank_image, words)) return rc;
  if (!image) return fail(EEC_ERR_BAD_ARG, "rir spectra: null image");
  if (image_bytes < 4 * words)
    return fail(EEC_ERR_WORKSPACE, "rir spectra: the image needs " + std::to_string(4 * words) + " bytes, got " + std::to_string(image_bytes));
  const int32_t* bank = (const int32_t*)rir_bank_image;
  const int R = bank[1];
  int32_t* img = (int32_t*)image;
  size_t at = rf_round4(kRfHead + kRfRec * (size_t)R);
  for (size_t i = 0; i < at; ++i) img[i] = 0;
  img[0] = EEC_RIR_SPECTRA_MAGIC, img[1] = R, img[2] = (int32_t)words, img[3] = kRfS, img[4] = (int32_t)at;
  std::vector<double> wr(kRfN / 2), wi(kRfN / 2), re(kRfN), im(kRfN);
  float* tw = (float*)(img + at);
  for (int u = 0; u < kRfN / 2; ++u) {
    rf_unit(u, kRfN, wr[u], wi[u]);
    tw[2 * u] = (float)wr[u], tw[2 * u + 1] = (float)wi[u];
  }
  at += kRfN;
  for (int r = 0; r < R; ++r) {
    const int32_t* rec = bank + kWaHead + kWaRirRec * r;
    const int K = rec[0], P = (K + kRfS - 1) / kRfS;
    const float* h = (const float*)(bank + rec[2]);
    img[kRfHead + kRfRec * r] = P, img[kRfHead + kRfRec * r + 1] = (int32_t)at;
    for (int p = 0; p < P; ++p, at += kRfN) {
      for (int n = 0; n < kRfN; ++n) re[n] = n < kRfS && p * kRfS + n < K ? (double)h[p * kRfS + n] : 0.0, im[n] = 0.0;
      rf_host_fft(re, im, wr, wi);
      float* H = (float*)(img + at);
      H[0] = (float)re[0], H[1] = (float)re[kRfM];
      for (int k = 1; k < kRfM; ++k) H[2 * k] = (float)re[k], H[2 * k + 1] = (float)im[k];
    }
  }
  return 0;
}

size_t eec_reverb_fft_workspace_bytes(int B, int L) {
  if (eec::wa_check_batch("reverb fft workspace", B, L)) return 0;
  return (size_t)(B > 0 ? B : 1) * (size_t)(eec::rf_blocks(L) + eec::kRfMaxP - 1) * eec::kRfN * sizeof(float);
}

int eec_reverb_fft_stage(const float* wave, const int64_t* lengths, const int32_t* params, int B, int L, const void* rir_bank,
                         const void* rir_spectra, float* out, double* partials, void* workspace, size_t workspace_bytes, int stages,
                         void* stream) {
  using namespace eec;
  using eech::fail;
  if (stages < 1 || stages > 3) return fail(EEC_ERR_BAD_ARG, "reverb fft: stages must be 1 (windows), 2 (blocks) or 3, got " + std::to_string(stages));
  if (int rc = wa_check_batch("reverb fft", B, L)) return rc;
  if (B == 0) return 0;
  if (!params || (L > 0 && (!wave || !out))) return fail(EEC_ERR_BAD_ARG, "reverb fft: null argument (wave, params, out)");
  if (wave && wave == out) return fail(EEC_ERR_BAD_ARG, "reverb fft: out must not be wave");
  if (((uintptr_t)partials & 7) != 0) return fail(EEC_ERR_BAD_ARG, "reverb fft: partials must be 8-byte aligned");
  const bool banks = rir_bank && rir_spectra;  // without either every utterance is copied and no workspace is touched
  if (banks) {
    const size_t need = eec_reverb_fft_workspace_bytes(B, L);
    if (!workspace || ((uintptr_t)workspace & 15) != 0) return fail(EEC_ERR_WORKSPACE, "reverb fft: the workspace must be 16-byte aligned and not null");
    if (workspace_bytes < need)
      return fail(EEC_ERR_WORKSPACE, "reverb fft: the workspace needs " + std::to_string(need) + " bytes, got " + std::to_string(workspace_bytes));
  }
  const int tiles = wa_tiles(L), blocks = rf_blocks(L), slots = blocks + kRfMaxP - 1;
  const unsigned by = (unsigned)(B < 65535 ? B : 65535);
  if (blocks == 0) {  // L == 0: nothing to write but the partial of the one tile a caller may add
    if (partials) EEC_HIP(hipMemsetAsync(partials, 0, (size_t)B * 2 * sizeof(double), (hipStream_t)stream));
    return 0;
  }
  if (banks && (stages & 1)) {
    hipLaunchKernelGGL(reverb_fft_windows_kernel, dim3((unsigned)slots, by), dim3(kRfThreads), 0, (hipStream_t)stream, wave, lengths, params, B, L,
                       (const int*)rir_bank, (const int*)rir_spectra, (float2*)workspace, slots);
    if (int rc = wa_launched("eec_reverb_fft launch (windows)")) return rc;
  }
  if (!(stages & 2)) return 0;
  hipLaunchKernelGGL(reverb_fft_blocks_kernel, dim3((unsigned)blocks, by), dim3(kRfThreads), 0, (hipStream_t)stream, wave, lengths, params, B, L,
                     banks ? (const int*)rir_bank : nullptr, banks ? (const int*)rir_spectra : nullptr, (const float2*)workspace, slots, out,
                     partials, tiles);
  return wa_launched("eec_reverb_fft launch (blocks)");
}

int eec_reverb_fft(const float* wave, const int64_t* lengths, const int32_t* params, int B, int L, const void* rir_bank,
                   const void* rir_spectra, float* out, double* partials, void* workspace, size_t workspace_bytes, void* stream) {
  return eec_reverb_fft_stage(wave, lengths, params, B, L, rir_bank, rir_spectra, out, partials, workspace, workspace_bytes, 3, stream);
}

}  // extern "C"
