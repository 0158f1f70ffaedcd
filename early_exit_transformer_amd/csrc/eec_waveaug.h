// What the waveform-augmentation launch families share (waveaug.hip: the direct reverberation, noise, volume; reverb_fft.hip: the
// reverberation by FFT): the geometry of an energy tile, the layout constants of the bank images, the clamped length, the record of
// a bank row that is never trusted, the stated order of a tile's energy, and the host checks of a batch.  The statement is in
// include/eec.h ("Waveform augmentation: reverberation, noise, volume").
#pragma once

#include "../../include/eec.h"
#include "eec_host.h"

#include <string>

namespace eec {

constexpr int kWaThreads = 128;
constexpr int kWaPer = 8;                 // consecutive outputs per work-item
constexpr int kWaTile = EEC_WAVEAUG_TILE;
static_assert(kWaTile == kWaThreads * kWaPer, "a work-item owns eight consecutive samples of the tile");
constexpr int kWaHead = 4, kWaRirRec = 4, kWaNoiseRec = 2;  // words of an image's header and of a record
constexpr int kWaP = EEC_WAVEAUG_PARAMS;

__device__ __forceinline__ long long wa_len(const int64_t* __restrict__ lengths, int b, int L) {
  const long long n = lengths ? (long long)lengths[b] : (long long)L;
  return n < 0 ? 0 : n > L ? L : n;
}
// record of RIR / noise row `at`, or nullptr: the stage is off (no bank, an index outside it)
__device__ __forceinline__ const int* wa_record(const int* __restrict__ bank, int at, int rec_words) {
  if (!bank) return nullptr;
  const int n = bank[1];
  if (at < 0 || at >= n || n > EEC_WAVEAUG_MAX_BANK) return nullptr;
  return bank + kWaHead + rec_words * at;
}

// the stated order inside a tile: the work-item's own sum, 64 lanes by halving, block 0 + block 1.  Valid in work-item 0.
__device__ __forceinline__ double wa_tile_energy(double e, double* wsum) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) e = e + __shfl_down(e, s, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = e;
  __syncthreads();
  return wsum[0] + wsum[1];
}
__device__ __forceinline__ double wa_own_energy(const float (&v)[kWaPer], int valid) {
#pragma clang fp contract(off)
  double e = 0.0;
#pragma unroll
  for (int j = 0; j < kWaPer; ++j)
    if (j < valid) e = e + (double)v[j] * (double)v[j];
  return e;
}

static int wa_check_batch(const char* who, int B, int L) {
  using eech::fail;
  const std::string w(who);
  if (B < 0) return fail(EEC_ERR_BAD_ARG, w + ": B must not be negative, got " + std::to_string(B));
  if (L < 0 || L > (1 << 30)) return fail(EEC_ERR_BAD_ARG, w + ": L must lie in [0, 2^30], got " + std::to_string(L));
  return 0;
}
static int wa_tiles(int L) { return L > 0 ? (L + kWaTile - 1) / kWaTile : 1; }
static int wa_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, who);
}

}  // namespace eec
