// Device check of the 16x16x32 GEMM forms (eec_device.h) against the 32x32x16 forms on the same LDS planes, packed
// weights and rings: both orientations, one / two row tiles, one / two column tiles, ring refills, and the layout conversions;
// and of the training GEMM's form (bf16 hi / lo fragments of one 32-deep LDS tile, quad_mac16 + accs_q_to_std of eec_wave.h)
// against v_mfma_f32_32x32x16_bf16 on the same LDS image.  The single k-step cases (KS2, K = 32) put the last MFMA directly in
// front of the lane swaps: the case in which a stale quadrant was once read.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I early_exit_transformer_amd/csrc tools/mfma16_gemm_check.hip -o tools/mfma16_gemm_check
#include <stdio.h>
#include <stdlib.h>
#include "eec_device.h"
using namespace eec;
template <bool SW, int MT, int NT, int KS, int PF>
__global__ void k(const half_t* act_hi, const half_t* act_lo, const uint4* wp, float* out32, float* out16) {
  constexpr int K = KS * 16, LD = (K + 8) * 2, PLANE = 64 * LD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  for (int i = threadIdx.x; i < 64 * K; i += 64) {
    const int r = i / K, c = i % K;
    *(half_t*)(smem + r * LD + c * 2) = act_hi[i];
    *(half_t*)(smem + PLANE + r * LD + c * 2) = act_lo[i];
  }
  __syncthreads();
  const int lane = threadIdx.x, hh = lane >> 5;
  const char* a_lane = smem + (lane & 31) * LD + hh * 16;
  f32x16 a32[MT][NT], a16[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) a32[mt][nt][i] = a16[mt][nt][i] = 0.01f * i + mt + 3 * nt;
  WRing<3, PF, NT> r;
  const size_t nts = (size_t)KS * 128;
  ring_fill_32<3, PF, NT>(r, wp + lane, nts, KS);
  gemm_ring_32<3, KS, NT, SW, PF, NoSide, 0, MT>(a32, a_lane, LD, PLANE, wp + lane, nts, r);
  ring_fill_16<3, PF, NT>(r, wp + lane, nts, KS);
  gemm_ring_16<3, KS, NT, SW, PF, NoSide, 0, MT, true, true>(a16, a_lane, LD, PLANE, wp + lane, nts, r);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        out32[((mt * NT + nt) * 16 + i) * 64 + lane] = a32[mt][nt][i];
        out16[((mt * NT + nt) * 16 + i) * 64 + lane] = a16[mt][nt][i];
      }
}
// The training form: A [32 MT][32] and B [32 NT][32] as bf16 hi / lo planes in LDS (row stride 40 elements, as the training GEMM's
// k-contiguous tiles).  16x16x32 fragment of row block rb: lane 16 g + c holds row 16 rb + c, k = 8 g .. 8 g + 7; the 32x32x16
// fragment of k-step s: lane 32 h + r holds row r, k = 16 s + 8 h .. + 7.  Same products (lo.hi, hi.lo, hi.hi), same quadrant
// order as the training k-tile.
template <int MT, int NT>
__global__ void kt(const bf16* a_hi, const bf16* a_lo, const bf16* b_hi, const bf16* b_lo, float* out32, float* out16) {
  constexpr int LD = 40;
  __shared__ __attribute__((aligned(16))) bf16 t[4][64 * LD];  // a_hi, a_lo, b_hi, b_lo
  const bf16* src[4] = {a_hi, a_lo, b_hi, b_lo};
  for (int p = 0; p < 4; ++p)
    for (int i = threadIdx.x; i < 64 * 32; i += 64) t[p][(i / 32) * LD + i % 32] = src[p][i];
  __syncthreads();
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4, r = lane & 31, h = lane >> 5;
  auto f16 = [&](int p, int tile, int rb) { return *(const bf16x8*)(&t[p][(32 * tile + 16 * rb + c) * LD + 8 * g]); };
  auto f32 = [&](int p, int tile, int s) { return *(const bf16x8*)(&t[p][(32 * tile + r) * LD + 16 * s + 8 * h]); };
  f32x16 a32[MT][NT], a16[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) a32[mt][nt][i] = a16[mt][nt][i] = 0.0f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        a32[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f32(1, mt, s), f32(2, nt, s), a32[mt][nt], 0, 0, 0);
        a32[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f32(0, mt, s), f32(3, nt, s), a32[mt][nt], 0, 0, 0);
        a32[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f32(0, mt, s), f32(2, nt, s), a32[mt][nt], 0, 0, 0);
      }
    }
  constexpr int order[4][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 0}};
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int ra = order[o][0], cb = order[o][1];
        quad_mac16(a16[mt][nt], ra, cb, f16(1, mt, ra), f16(2, nt, cb));
        quad_mac16(a16[mt][nt], ra, cb, f16(0, mt, ra), f16(3, nt, cb));
        quad_mac16(a16[mt][nt], ra, cb, f16(0, mt, ra), f16(2, nt, cb));
      }
  accs_q_to_std<MT, NT>(a16);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        out32[((mt * NT + nt) * 16 + i) * 64 + lane] = a32[mt][nt][i];
        out16[((mt * NT + nt) * 16 + i) * 64 + lane] = a16[mt][nt][i];
      }
}
static half_t *ah, *al; static uint4* wp; static float *o32, *o16;
static bf16* tb[4];  // a_hi, a_lo, b_hi, b_lo of the training form: [64][32] each
static int compare(const char* name, int tiles) {
  if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); return 1; }
  double worst = 0; int bad = 0;
  for (int i = 0; i < tiles * 16 * 64; ++i) { const double d = fabs(o32[i] - o16[i]); if (d > worst) worst = d; if (d > 1e-4) ++bad; }
  printf("%-36s max |32x32x16 - 16x16x32| = %.3e, %d of %d differ  %s\n", name, worst, bad, tiles * 1024, bad ? "FAIL" : "OK");
  return bad != 0;
}
template <int MT, int NT>
static int run_train(const char* name) {
  hipLaunchKernelGGL((kt<MT, NT>), dim3(1), dim3(64), 0, 0, tb[0], tb[1], tb[2], tb[3], o32, o16);
  return compare(name, MT * NT);
}
template <bool SW, int MT, int NT, int KS, int PF>
static int run(const char* name) {
  hipLaunchKernelGGL((k<SW, MT, NT, KS, PF>), dim3(1), dim3(64), 2 * 64 * (KS * 16 + 8) * 2, 0, ah, al, wp, o32, o16);
  return compare(name, MT * NT);
}
int main() {
  const int KMAX = 512;
  (void)hipMallocManaged(&ah, 64 * KMAX * 2); (void)hipMallocManaged(&al, 64 * KMAX * 2); (void)hipMallocManaged(&wp, 2 * (KMAX / 16) * 2 * 64 * 16);
  (void)hipMallocManaged(&o32, 4 * 16 * 64 * 4); (void)hipMallocManaged(&o16, 4 * 16 * 64 * 4);
  srand(1);
  for (int i = 0; i < 64 * KMAX; ++i) { ah[i] = (half_t)((rand() % 200 - 100) / 64.0f); al[i] = (half_t)((rand() % 200 - 100) / 65536.0f); }
  half_t* w = (half_t*)wp;
  for (int i = 0; i < 2 * (KMAX / 16) * 2 * 64 * 8; ++i) w[i] = (half_t)((rand() % 200 - 100) / 128.0f);
  for (int p = 0; p < 4; ++p) {  // hi planes n / 64, lo planes n / 65536, |n| <= 100: exact in bf16
    (void)hipMallocManaged(&tb[p], 64 * 32 * sizeof(bf16));
    for (int i = 0; i < 64 * 32; ++i) tb[p][i] = (bf16)((rand() % 200 - 100) / ((p & 1) ? 65536.0f : 64.0f));
  }
  int fails = 0;
  fails += run<false, 2, 1, 4, 4>("normal  MT2 NT1 KS4  PF4");
  fails += run<true, 2, 1, 4, 4>("swapped MT2 NT1 KS4  PF4");
  fails += run<true, 1, 1, 4, 4>("swapped MT1 NT1 KS4  PF4");
  fails += run<true, 1, 1, 16, 4>("swapped MT1 NT1 KS16 PF4");
  fails += run<true, 2, 1, 16, 8>("swapped MT2 NT1 KS16 PF8");
  fails += run<true, 1, 2, 32, 4>("swapped MT1 NT2 KS32 PF4");
  fails += run<false, 2, 2, 8, 4>("normal  MT2 NT2 KS8  PF4");
  fails += run<false, 1, 2, 8, 2>("normal  MT1 NT2 KS8  PF2");
  fails += run<false, 1, 1, 2, 2>("normal  MT1 NT1 KS2  PF2");
  fails += run<true, 1, 1, 2, 2>("swapped MT1 NT1 KS2  PF2");
  fails += run_train<1, 1>("train bf16x3 TM1 TN1 K32");
  fails += run_train<2, 2>("train bf16x3 TM2 TN2 K32");
  return fails;
}
