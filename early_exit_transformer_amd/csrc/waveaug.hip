// Waveform augmentation of a batch [B, L]: reverberation with room impulse responses, additive noise at a chosen signal-to-noise ratio,
// volume.  The statement -- the fp32 tap order, the order of the fp64 energy sums, the draw and the layout of the bank images -- is in
// include/eec.h ("Waveform augmentation: reverberation, noise, volume").
//
// eec_rir_bank / eec_noise_bank (host only): the normalised, trimmed RIRs and the noise rows as one image of int32 words each.
//
// eec_waveaug_draw: one work-item per utterance, one row rir, noise, start, snr_idx, gain_bits from the dropout generator of eec_drop.h.
//
// eec_reverb: one workgroup of 128 work-items per (tile of 1024 outputs, utterance); work-item t holds the outputs 8 t .. 8 t + 7 of
// the tile in registers.  The taps stream through LDS 512 at a time.  For a chunk of taps k0 .. k0 + 511 the LDS holds the 1536
// samples x[i0 + d - k0 - 512 + s], s = 0 .. 1535 (zeros outside [0, len)), so that output 8 t + j and tap k0 + q meet the slot
// 8 t + j - q + 512: eight taps meet 16 consecutive slots from a multiple of 8, of which the upper eight are the lower eight of the
// eight taps before, so a work-item reads eight new slots (two 16-byte reads) and eight taps (two 16-byte broadcast reads) for 64
// multiplies and 64 adds.  The finished tile goes through the same LDS, so a wave stores 256
// consecutive bytes whatever the row's alignment.
//
// The tile's partial energy is taken from the registers in the stated order (tile_energy); eec_noise_energy walks the tiled noise
// segment in the same geometry; eec_noise_mix adds the partials in tile order, forms the scale and writes the output.
#include "../../include/eec.h"
#include "eec_drop.h"
#include "eec_host.h"
#include "eec_waveaug.h"

#include <cmath>
#include <vector>

namespace eec {

constexpr int kWaChunk = 512;             // taps per LDS stage
constexpr int kWaWin = kWaTile + kWaChunk;
constexpr int kWaMixThreads = 256, kWaMixTile = 2048;

struct WaSnr {
  double g[EEC_WAVEAUG_MAX_SNRS];
};

// ---------------------------------------------------------------------------------------------------------------------------
// the banks (host)
// ---------------------------------------------------------------------------------------------------------------------------
struct WaRir {
  int d, peak;
  std::vector<float> h;
};

static int wa_check_counts(const char* who, int n, const void* data, const int32_t* counts, long long most) {
  using eech::fail;
  const std::string w(who);
  if (n < 1 || n > EEC_WAVEAUG_MAX_BANK)
    return fail(EEC_ERR_BAD_ARG, w + ": the number of rows must lie in [1, " + std::to_string(EEC_WAVEAUG_MAX_BANK) + "], got " + std::to_string(n));
  if (!data || !counts) return fail(EEC_ERR_BAD_ARG, w + ": null argument");
  for (int r = 0; r < n; ++r)
    if (counts[r] < 1 || counts[r] > most)
      return fail(EEC_ERR_BAD_ARG, w + ": row " + std::to_string(r) + " must have between 1 and " + std::to_string(most) + " values, got " + std::to_string(counts[r]));
  return 0;
}

static int wa_rirs(int R, const float* taps, const int32_t* n_taps, int normalize, int shift, std::vector<WaRir>& out, size_t& words) {
#pragma clang fp contract(off)  // the normalisation is the stated fp64 expression, operation by operation
  using eech::fail;
  if (int rc = wa_check_counts("rir bank", R, taps, n_taps, EEC_REVERB_MAX_TAPS)) return rc;
  if (normalize != EEC_RIR_NORM_NONE && normalize != EEC_RIR_NORM_L2 && normalize != EEC_RIR_NORM_PEAK)
    return fail(EEC_ERR_BAD_ARG, "rir bank: normalize must be EEC_RIR_NORM_NONE, _L2 or _PEAK, got " + std::to_string(normalize));
  words = kWaHead + kWaRirRec * (size_t)R;
  const float* h = taps;
  for (int r = 0; r < R; h += n_taps[r], ++r) {
    const int K = n_taps[r];
    int p = 0;
    double energy = 0.0;
    for (int k = 0; k < K; ++k) {
      if (!std::isfinite(h[k])) return fail(EEC_ERR_BAD_ARG, "rir bank: RIR " + std::to_string(r) + " holds a value that is not finite");
      if (std::fabs(h[k]) > std::fabs(h[p])) p = k;
      energy += (double)h[k] * (double)h[k];
    }
    const double div = normalize == EEC_RIR_NORM_L2 ? std::sqrt(energy) : normalize == EEC_RIR_NORM_PEAK ? std::fabs((double)h[p]) : 1.0;
    std::vector<float> v(K);
    for (int k = 0; k < K; ++k) v[k] = div > 0.0 ? (float)((double)h[k] / div) : 0.0f;
    int lo = 0, hi = K;
    while (lo < hi && v[lo] == 0.0f) ++lo;
    while (hi > lo && v[hi - 1] == 0.0f) --hi;
    if (lo == hi) return fail(EEC_ERR_BAD_ARG, "rir bank: RIR " + std::to_string(r) + " has no non-zero tap");
    WaRir q;
    q.peak = p - lo, q.d = shift ? p - lo : -lo;
    q.h.assign(v.begin() + lo, v.begin() + hi);
    words += q.h.size();
    out.push_back(std::move(q));
  }
  return 0;
}

static int wa_noise_words(int M, const float* samples, const int32_t* n_samples, size_t& words) {
  using eech::fail;
  if (int rc = wa_check_counts("noise bank", M, samples, n_samples, 1ll << 30)) return rc;
  words = kWaHead + kWaNoiseRec * (size_t)M;
  const float* x = samples;
  for (int m = 0; m < M; x += n_samples[m], ++m) {
    for (int i = 0; i < n_samples[m]; ++i)
      if (!std::isfinite(x[i])) return fail(EEC_ERR_BAD_ARG, "noise bank: row " + std::to_string(m) + " holds a value that is not finite");
    words += (size_t)n_samples[m];
  }
  if (words >= (1ull << 31)) return fail(EEC_ERR_BAD_ARG, "noise bank: the image would have 2^31 words or more");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the kernels
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void waveaug_draw_kernel(int B, uint64_t seed, uint64_t utt_offset, const int* __restrict__ rir_bank, uint64_t thr_reverb,
                                                          const int* __restrict__ noise_bank, uint64_t thr_noise, int n_snrs, int volume, double lo,
                                                          double hi, int* __restrict__ params) {
#pragma clang fp contract(off)  // the gain is the stated fp64 expression, operation by operation
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const uint32_t key = eect::drop_key(eect::Drop{0.0f, seed, EEC_WAVEAUG_SITE});
  const uint64_t at = (utt_offset + (uint64_t)b) * 64u;
  auto word = [&](int slot) { return (uint64_t)eect::drop_word(key, at + (uint64_t)slot); };
  int R = rir_bank ? rir_bank[1] : 0, M = noise_bank ? noise_bank[1] : 0;
  R = R < 0 || R > EEC_WAVEAUG_MAX_BANK ? 0 : R, M = M < 0 || M > EEC_WAVEAUG_MAX_BANK ? 0 : M;
  int rir = -1, noise = -1, start = 0, snr = 0;
  if (R > 0 && word(0) < thr_reverb) rir = (int)((word(1) * (uint32_t)R) >> 32);
  if (M > 0 && n_snrs > 0 && word(2) < thr_noise) {
    noise = (int)((word(3) * (uint32_t)M) >> 32);
    const int len_m = noise_bank[kWaHead + kWaNoiseRec * noise];
    start = (int)((word(4) * (uint32_t)(len_m < 0 ? 0 : len_m)) >> 32);
    snr = (int)((word(5) * (uint32_t)n_snrs) >> 32);
  }
  float gain = 1.0f;
  if (volume) gain = (float)(lo + (hi - lo) * ((double)word(6) * 0x1p-32));
  int* p = params + (size_t)b * kWaP;
  p[0] = rir, p[1] = noise, p[2] = start, p[3] = snr, p[4] = __float_as_int(gain);
}

__global__ __launch_bounds__(kWaThreads) void reverb_kernel(const float* __restrict__ wave, const int64_t* __restrict__ lengths,
                                                            const int* __restrict__ params, int B, int L, const int* __restrict__ bank,
                                                            float* __restrict__ out, double* __restrict__ partials, int n_tiles) {
#pragma clang fp contract(off)  // one rounded multiply and one rounded add per tap
  __shared__ __attribute__((aligned(16))) float xs[kWaWin];
  __shared__ __attribute__((aligned(16))) float hs[kWaChunk];
  __shared__ double wsum[2];
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * kWaTile;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // one pass unless B exceeds the grid's y limit
    const long long len = wa_len(lengths, b, L);
    const float* __restrict__ x = wave + (size_t)b * L;
    float* __restrict__ y = out + (size_t)b * L;
    const long long left = len - (i0 + kWaPer * tid);  // of the work-item's eight samples, min(left, 8) lie below len
    const int valid = left < 0 ? 0 : left > kWaPer ? kWaPer : (int)left;
    if (len <= i0) {  // past the utterance: zeros (and a zero partial, which eec_noise_mix never adds)
      for (long long i = i0 + tid; i < i0 + kWaTile && i < L; i += kWaThreads) y[i] = 0.0f;
      if (partials && tid == 0) partials[((size_t)b * n_tiles + blockIdx.x) * 2] = 0.0;
      continue;
    }
    const int* rec = wa_record(bank, params[(size_t)b * kWaP], kWaRirRec);
    float acc[kWaPer];
#pragma unroll
    for (int j = 0; j < kWaPer; ++j) acc[j] = 0.0f;
    __syncthreads();  // the previous utterance's readers are done with the LDS
    if (!rec) {  // a copy: quads where both rows are aligned and the eight samples are valid, single floats otherwise; zeros past len
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
      const int K = rec[0], d = rec[1];
      const float* __restrict__ h = (const float*)(bank + rec[2]);
      for (int k0 = 0; k0 < K; k0 += kWaChunk) {
        const long long g0 = i0 + d - k0 - kWaChunk;  // the sample of slot 0
        if (g0 >= len || g0 + kWaWin <= 0) continue;  // every product of the chunk has a zero sample
        __syncthreads();
        for (int s = tid; s < kWaWin; s += kWaThreads) {
          const long long g = g0 + s;
          xs[s] = g >= 0 && g < len ? x[g] : 0.0f;
        }
        for (int q = tid; q < kWaChunk; q += kWaThreads) hs[q] = k0 + q < K ? h[k0 + q] : 0.0f;
        __syncthreads();
        const int taps = K - k0 < kWaChunk ? K - k0 : kWaChunk;
        float w[16], t[8];  // w[i] = slot 8 t - q0 + 504 + i: the upper eight are the lower eight of the taps before
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const float4 a = ((const float4*)(xs + kWaPer * tid + kWaChunk))[v];
          w[8 + 4 * v] = a.x, w[9 + 4 * v] = a.y, w[10 + 4 * v] = a.z, w[11 + 4 * v] = a.w;
        }
#pragma unroll 2
        for (int q0 = 0; q0 < taps; q0 += 8) {
          if (q0 > 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) w[8 + i] = w[i];
          }
          const float4* ws = (const float4*)(xs + kWaPer * tid - q0 + kWaChunk - 8);
          const float4* ts = (const float4*)(hs + q0);
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const float4 a = ws[v];
            w[4 * v] = a.x, w[4 * v + 1] = a.y, w[4 * v + 2] = a.z, w[4 * v + 3] = a.w;
          }
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const float4 a = ts[v];
            t[4 * v] = a.x, t[4 * v + 1] = a.y, t[4 * v + 2] = a.z, t[4 * v + 3] = a.w;
          }
#pragma unroll
          for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int j = 0; j < kWaPer; ++j) acc[j] = acc[j] + t[q] * w[8 + j - q];
        }
      }
      __syncthreads();  // the last chunk's readers are done: the tile leaves through the window's LDS
#pragma unroll
      for (int j = 0; j < kWaPer; ++j) xs[kWaPer * tid + j] = acc[j];
      __syncthreads();
      for (int o = tid; o < kWaTile && i0 + o < L; o += kWaThreads) y[i0 + o] = i0 + o < len ? xs[o] : 0.0f;
    }
    if (partials) {  // uniform per launch
      const double e = wa_tile_energy(wa_own_energy(acc, valid), wsum);
      if (tid == 0) partials[((size_t)b * n_tiles + blockIdx.x) * 2] = e;
    }
  }
}

__global__ __launch_bounds__(kWaThreads) void noise_energy_kernel(const float* __restrict__ signal, const int64_t* __restrict__ lengths,
                                                                  const int* __restrict__ params, int B, int L, const int* __restrict__ bank,
                                                                  double* __restrict__ partials, int n_tiles) {
  __shared__ double wsum[2];
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * kWaTile;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long len = wa_len(lengths, b, L);
    const long long left = len - (i0 + kWaPer * tid);
    const int valid = left < 0 ? 0 : left > kWaPer ? kWaPer : (int)left;
    double* part = partials + ((size_t)b * n_tiles + blockIdx.x) * 2;
    const int* rec = wa_record(bank, params[(size_t)b * kWaP + 1], kWaNoiseRec);
    const int len_m = rec ? rec[0] : 0;
    float v[kWaPer];
    __syncthreads();  // wsum of the previous pass
    if (signal) {
      const float* __restrict__ x = signal + (size_t)b * L + i0 + kWaPer * tid;
#pragma unroll
      for (int j = 0; j < kWaPer; ++j) v[j] = j < valid ? x[j] : 0.0f;
      const double e = wa_tile_energy(wa_own_energy(v, valid), wsum);
      if (tid == 0) part[0] = e;
      __syncthreads();
    }
    if (len_m < 1 || len <= i0) {  // uniform per workgroup
      if (tid == 0) part[1] = 0.0;
      continue;
    }
    const float* __restrict__ nz = (const float*)(bank + rec[1]);
    int s = params[(size_t)b * kWaP + 2] % len_m;
    s = s < 0 ? s + len_m : s;
    unsigned p = (unsigned)(((unsigned long long)s + (unsigned long long)(i0 + kWaPer * tid)) % (unsigned)len_m);
#pragma unroll
    for (int j = 0; j < kWaPer; ++j) {
      v[j] = j < valid ? nz[p] : 0.0f;
      p = p + 1 == (unsigned)len_m ? 0u : p + 1;
    }
    const double e = wa_tile_energy(wa_own_energy(v, valid), wsum);
    if (tid == 0) part[1] = e;
  }
}

__global__ __launch_bounds__(kWaMixThreads) void noise_mix_kernel(const float* y, const int64_t* __restrict__ lengths, const int* __restrict__ params,
                                                                  int B, int L, const int* __restrict__ bank, WaSnr snr, int n_snrs,
                                                                  const double* __restrict__ partials, int n_tiles, float* out,
                                                                  float* __restrict__ applied) {
#pragma clang fp contract(off)  // a rounded multiply, a rounded add, a rounded multiply
  const int tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * kWaMixTile;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long len = wa_len(lengths, b, L);
    const int* row = params + (size_t)b * kWaP;
    const float gain = __int_as_float(row[4]);
    const int* rec = wa_record(bank, row[1], kWaNoiseRec);
    const int len_m = rec ? rec[0] : 0, snr_idx = row[3];
    float scale = 0.0f;
    if (len_m >= 1 && snr_idx >= 0 && snr_idx < n_snrs && partials && len > 0) {
      const double* part = partials + (size_t)b * n_tiles * 2;
      const int used = (int)((len + kWaTile - 1) / kWaTile);
      double es = 0.0, en = 0.0;
      for (int t = 0; t < used; ++t) es = es + part[2 * t], en = en + part[2 * t + 1];
      if (es > 0.0 && en > 0.0) scale = (float)(__builtin_sqrt(es / en) * snr.g[snr_idx]);
    }
    if (applied && blockIdx.x == 0 && tid == 0) applied[2 * (size_t)b] = scale, applied[2 * (size_t)b + 1] = gain;
    const float* yb = y + (size_t)b * L;
    float* ob = out + (size_t)b * L;
    const long long i1 = i0 + kWaMixTile < L ? i0 + kWaMixTile : L;
    if (scale != 0.0f) {  // uniform per workgroup
      const float* __restrict__ nz = (const float*)(bank + rec[1]);
      int s = row[2] % len_m;
      s = s < 0 ? s + len_m : s;
      unsigned p = (unsigned)(((unsigned long long)s + (unsigned long long)(i0 + tid)) % (unsigned)len_m);
      const unsigned step = (unsigned)kWaMixThreads % (unsigned)len_m;
      for (long long i = i0 + tid; i < i1; i += kWaMixThreads) {
        float z = 0.0f;
        if (i < len) {
          z = yb[i] + scale * nz[p];
          z = z * gain;
        }
        ob[i] = z;
        p += step;
        p = p >= (unsigned)len_m ? p - (unsigned)len_m : p;
      }
    } else {
      for (long long i = i0 + tid; i < i1; i += kWaMixThreads) ob[i] = i < len ? yb[i] * gain : 0.0f;
    }
  }
}

}  // namespace eec

extern "C" {

size_t eec_rir_bank_bytes(int R, const float* taps, const int32_t* n_taps, int normalize, int shift) {
  std::vector<eec::WaRir> qs;
  size_t words = 0;
  return eec::wa_rirs(R, taps, n_taps, normalize, shift, qs, words) ? 0 : 4 * words;
}

int eec_rir_bank(int R, const float* taps, const int32_t* n_taps, int normalize, int shift, void* image, size_t image_bytes) {
  using namespace eec;
  using eech::fail;
  std::vector<WaRir> qs;
  size_t words = 0;
  if (int rc = wa_rirs(R, taps, n_taps, normalize, shift, qs, words)) return rc;
  if (!image) return fail(EEC_ERR_BAD_ARG, "rir bank: null image");
  if (image_bytes < 4 * words)
    return fail(EEC_ERR_WORKSPACE, "rir bank: the image needs " + std::to_string(4 * words) + " bytes, got " + std::to_string(image_bytes));
  int32_t* img = (int32_t*)image;
  img[0] = EEC_RIR_MAGIC, img[1] = R, img[2] = (int32_t)words, img[3] = normalize | (shift ? 1 : 0) << 8;
  size_t at = kWaHead + kWaRirRec * (size_t)R;
  for (int r = 0; r < R; ++r) {
    int32_t* rec = img + kWaHead + kWaRirRec * r;
    rec[0] = (int32_t)qs[r].h.size(), rec[1] = qs[r].d, rec[2] = (int32_t)at, rec[3] = qs[r].peak;
    float* w = (float*)(img + at);
    for (size_t k = 0; k < qs[r].h.size(); ++k) w[k] = qs[r].h[k];
    at += qs[r].h.size();
  }
  return 0;
}

size_t eec_noise_bank_bytes(int M, const float* samples, const int32_t* n_samples) {
  size_t words = 0;
  return eec::wa_noise_words(M, samples, n_samples, words) ? 0 : 4 * words;
}

int eec_noise_bank(int M, const float* samples, const int32_t* n_samples, void* image, size_t image_bytes) {
  using namespace eec;
  using eech::fail;
  size_t words = 0;
  if (int rc = wa_noise_words(M, samples, n_samples, words)) return rc;
  if (!image) return fail(EEC_ERR_BAD_ARG, "noise bank: null image");
  if (image_bytes < 4 * words)
    return fail(EEC_ERR_WORKSPACE, "noise bank: the image needs " + std::to_string(4 * words) + " bytes, got " + std::to_string(image_bytes));
  int32_t* img = (int32_t*)image;
  img[0] = EEC_NOISE_MAGIC, img[1] = M, img[2] = (int32_t)words, img[3] = 0;
  size_t at = kWaHead + kWaNoiseRec * (size_t)M;
  const float* x = samples;
  for (int m = 0; m < M; x += n_samples[m], ++m) {
    img[kWaHead + kWaNoiseRec * m] = n_samples[m], img[kWaHead + kWaNoiseRec * m + 1] = (int32_t)at;
    float* w = (float*)(img + at);
    for (int i = 0; i < n_samples[m]; ++i) w[i] = x[i];
    at += (size_t)n_samples[m];
  }
  return 0;
}

size_t eec_waveaug_partials_bytes(int B, int L) {
  if (eec::wa_check_batch("waveaug partials", B, L)) return 0;
  return (size_t)B * (size_t)eec::wa_tiles(L) * 2 * sizeof(double);
}

int eec_waveaug_draw(int B, uint64_t seed, uint64_t utt_offset, const void* rir_bank, uint64_t thr_reverb, const void* noise_bank,
                     uint64_t thr_noise, int n_snrs, int volume, double lo, double hi, int32_t* params, void* stream) {
  using namespace eec;
  using eech::fail;
  if (B < 0) return fail(EEC_ERR_BAD_ARG, "waveaug draw: B must not be negative, got " + std::to_string(B));
  if (thr_reverb > (1ull << 32) || thr_noise > (1ull << 32)) return fail(EEC_ERR_BAD_ARG, "waveaug draw: a threshold must not exceed 2^32");
  if (n_snrs < 0 || n_snrs > EEC_WAVEAUG_MAX_SNRS)
    return fail(EEC_ERR_BAD_ARG, "waveaug draw: n_snrs must lie in [0, " + std::to_string(EEC_WAVEAUG_MAX_SNRS) + "], got " + std::to_string(n_snrs));
  if (volume && (!std::isfinite(lo) || !std::isfinite(hi))) return fail(EEC_ERR_BAD_ARG, "waveaug draw: the volume range must be finite");
  if (B == 0) return 0;
  if (!params) return fail(EEC_ERR_BAD_ARG, "waveaug draw: null argument (params)");
  hipLaunchKernelGGL(waveaug_draw_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, B, seed, utt_offset, (const int*)rir_bank,
                     thr_reverb, (const int*)noise_bank, thr_noise, n_snrs, volume, lo, hi, params);
  return wa_launched("eec_waveaug_draw launch");
}

int eec_reverb(const float* wave, const int64_t* lengths, const int32_t* params, int B, int L, const void* rir_bank, float* out,
               double* partials, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = wa_check_batch("reverb", B, L)) return rc;
  if (B == 0) return 0;
  if (!params || (L > 0 && (!wave || !out))) return fail(EEC_ERR_BAD_ARG, "reverb: null argument (wave, params, out)");
  if (wave && wave == out) return fail(EEC_ERR_BAD_ARG, "reverb: out must not be wave (an output reads samples other work-items overwrite)");
  if (((uintptr_t)partials & 7) != 0) return fail(EEC_ERR_BAD_ARG, "reverb: partials must be 8-byte aligned");
  const int tiles = wa_tiles(L);
  hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)tiles, (unsigned)(B < 65535 ? B : 65535)), dim3(kWaThreads), 0, (hipStream_t)stream, wave, lengths,
                     params, B, L, (const int*)rir_bank, out, partials, tiles);
  return wa_launched("eec_reverb launch");
}

int eec_noise_energy(const float* signal, const int64_t* lengths, const int32_t* params, int B, int L, const void* noise_bank,
                     double* partials, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = wa_check_batch("noise energy", B, L)) return rc;
  if (B == 0) return 0;
  if (!params || !partials) return fail(EEC_ERR_BAD_ARG, "noise energy: null argument (params, partials)");
  if (((uintptr_t)partials & 7) != 0) return fail(EEC_ERR_BAD_ARG, "noise energy: partials must be 8-byte aligned");
  const int tiles = wa_tiles(L);
  hipLaunchKernelGGL(noise_energy_kernel, dim3((unsigned)tiles, (unsigned)(B < 65535 ? B : 65535)), dim3(kWaThreads), 0, (hipStream_t)stream, signal,
                     lengths, params, B, L, (const int*)noise_bank, partials, tiles);
  return wa_launched("eec_noise_energy launch");
}

int eec_noise_mix(const float* y, const int64_t* lengths, const int32_t* params, int B, int L, const void* noise_bank,
                  const double* snr_gain, int n_snrs, const double* partials, float* out, float* applied, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = wa_check_batch("noise mix", B, L)) return rc;
  if (n_snrs < 0 || n_snrs > EEC_WAVEAUG_MAX_SNRS)
    return fail(EEC_ERR_BAD_ARG, "noise mix: n_snrs must lie in [0, " + std::to_string(EEC_WAVEAUG_MAX_SNRS) + "], got " + std::to_string(n_snrs));
  if (n_snrs > 0 && !snr_gain) return fail(EEC_ERR_BAD_ARG, "noise mix: null argument (snr_gain)");
  WaSnr snr = {};
  for (int k = 0; k < n_snrs; ++k) {
    if (!std::isfinite(snr_gain[k])) return fail(EEC_ERR_BAD_ARG, "noise mix: snr_gain holds a value that is not finite");
    snr.g[k] = snr_gain[k];
  }
  if (B == 0) return 0;
  if (!params || (L > 0 && (!y || !out))) return fail(EEC_ERR_BAD_ARG, "noise mix: null argument (y, params, out)");
  if (((uintptr_t)partials & 7) != 0) return fail(EEC_ERR_BAD_ARG, "noise mix: partials must be 8-byte aligned");
  const unsigned tiles = L > 0 ? (unsigned)((L + kWaMixTile - 1) / kWaMixTile) : 1u;  // one workgroup still writes applied
  hipLaunchKernelGGL(noise_mix_kernel, dim3(tiles, (unsigned)(B < 65535 ? B : 65535)), dim3(kWaMixThreads), 0, (hipStream_t)stream, y, lengths, params, B,
                     L, noise_bank && partials ? (const int*)noise_bank : nullptr, snr, n_snrs, partials, wa_tiles(L), out, applied);
  return wa_launched("eec_noise_mix launch");
}

}  // extern "C"
