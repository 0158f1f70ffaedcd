// Wave-level building blocks of every kernel in this directory (gfx950, wave64), device code only: vector types, lane
// indices, wave reductions, the compile-time loop, and the 16x16x32 MFMA accumulate with the lane swaps that restore the
// 32x32x16 accumulator layout.  No kernels, no tile geometry, no LDS layouts: those are in eec_device.h (inference) and in the
// training files, which all get this header (through eec_device.h, eec_drop.h or eec_decoder_step.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eec {

typedef _Float16 half_t;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16;
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float kNegBig = -1.0e30f;  // "minus infinity" of the online softmaxes: exp2 of it is 0, differences of it stay finite

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
// row of accumulator register i for this lane, within a 32x32 tile in the 32x32x16 MFMA's layout (col = lane & 31)
__device__ __forceinline__ int acc_row(int i, int lane) { return (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); }

// ---------------------------------------------------------------------------------------------------------------------
// Wave-wide reductions on the DPP crossbar (no LDS traffic, unlike __shfl_xor = ds_bpermute): xor-1 / xor-2
// inside each quad, half-row and row mirrors -> every lane of a 16-lane row holds the row total; row_bcast15
// into rows 1,3 and row_bcast31 into rows 2,3 -> lane 63 holds the wave total, returned wave-uniform.
// ---------------------------------------------------------------------------------------------------------------------
#define EEC_DPP_ADD(v, ctrl, rmask) \
  ((v) + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), ctrl, rmask, 0xf, false)))
#define EEC_DPP_MAX(v, ctrl, rmask) \
  fmaxf((v), __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, (v)), __builtin_bit_cast(int, (v)), ctrl, rmask, 0xf, false)))
// sum over the 16 lanes of a DPP row, left in every lane of the row
__device__ __forceinline__ float row16_sum(float v) {
  v = EEC_DPP_ADD(v, 0xB1, 0xf);   // quad_perm [1,0,3,2]
  v = EEC_DPP_ADD(v, 0x4E, 0xf);   // quad_perm [2,3,0,1]
  v = EEC_DPP_ADD(v, 0x141, 0xf);  // row_half_mirror
  v = EEC_DPP_ADD(v, 0x140, 0xf);  // row_mirror
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  v = EEC_DPP_ADD(v, 0x142, 0xa);  // row_bcast15 -> rows 1, 3
  v = EEC_DPP_ADD(v, 0x143, 0xc);  // row_bcast31 -> rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  v = EEC_DPP_MAX(v, 0xB1, 0xf);
  v = EEC_DPP_MAX(v, 0x4E, 0xf);
  v = EEC_DPP_MAX(v, 0x141, 0xf);
  v = EEC_DPP_MAX(v, 0x140, 0xf);
  v = EEC_DPP_MAX(v, 0x142, 0xa);
  v = EEC_DPP_MAX(v, 0x143, 0xc);
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// The butterfly forms (__shfl_xor): over the 2 * from lanes of a group, the result left in EVERY lane of it; the whole wave by
// default.  For per-lane follow-up work, and for the groups (8, 16 lanes of a head or a row) the DPP forms do not serve.
__device__ __forceinline__ float wave_all_sum(float v, int from = 32) {
#pragma unroll
  for (int m = from; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_all_max(float v, int from = 32) {
#pragma unroll
  for (int m = from; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_all_max(int v, int from = 32) {
#pragma unroll
  for (int m = from; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

// One-lane shifts on the DPP crossbar.  from_left: lane l receives lane l - 1's v (wave_shr:1), lane 0 receives `first`;
// from_right: lane l receives lane l + 1's v (wave_shl:1), lane 63 receives `last`.
__device__ __forceinline__ int from_left(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float from_left(float v, float first) {
  return __builtin_bit_cast(float, from_left(__builtin_bit_cast(int, v), __builtin_bit_cast(int, first)));
}
__device__ __forceinline__ float from_right(float v, float last) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, last), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// f(IntTag<K0>{}), ..., f(IntTag<K1-1>{}): a loop whose index is a compile-time constant in the body (register arrays
// indexed by it never fall back to scratch memory, whatever the unroller decides)
template <int I>
struct IntTag {
  static constexpr int value = I;
};
template <int K0, int K1, typename F>
__device__ __forceinline__ void static_range(F&& f) {
  if constexpr (K0 < K1) {
    f(IntTag<K0>{});
    static_range<K0 + 1, K1>(f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// v_mfma_f32_16x16x32_{f16, bf16} into the quadrants of a 32 x 32 accumulator tile.  Lane l = 16 g + c holds, of an operand
// fragment of 16 rows x 32 k, row c, k = 8 g .. 8 g + 7.  The tile is four 16 x 16 quadrants (ra, cb) in registers
// 4 (2 ra + cb) + i: m = 16 ra + 4 g + i, n = 16 cb + c ("quadrant layout").  The standard layout every epilogue expects
// (the 32x32x16 MFMA's: n = lane & 31, m = acc_row(reg, lane)) is restored with v_permlane16_swap + v_permlane32_swap on the
// register pairs (4 (2 ra) + i, 4 (2 ra + 1) + i): 32 cross-lane instructions per tile, once per accumulation.
// ---------------------------------------------------------------------------------------------------------------------
// EEC_OPERAND_BF16 (a translation-unit switch; only the training step's fused feed-forward BACKWARD sets it, ffn.hip): the split
// operands of the inference-path forms are bf16 hi / lo pairs (2^-16 per product, the fp32 exponent range: gradients) on
// v_mfma_*_bf16 instead of fp16 pairs.  Fragments keep their h8 / h2 storage types -- only the conversions and the MFMA
// builtins differ.  The training GEMM passes bf16x8 fragments and gets the bf16 form whatever the switch says.
#ifndef EEC_OPERAND_BF16
#define EEC_OPERAND_BF16 0
#endif
__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma32(h8 a, h8 b, f32x4 c) {
#if EEC_OPERAND_BF16
  return mfma32(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c);
#else
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#endif
}
// quadrant (ra, cb) of a tile += a . b^T  (ra, cb constants after unrolling; V = h8 or bf16x8)
template <typename V>
__device__ __forceinline__ void quad_mac16(f32x16& acc, int ra, int cb, V a, V b) {
  const int q = 4 * (2 * ra + cb);
  f32x4 t = {acc[q], acc[q + 1], acc[q + 2], acc[q + 3]};
  t = mfma32(a, b, t);
  acc[q] = t[0], acc[q + 1] = t[1], acc[q + 2] = t[2], acc[q + 3] = t[3];
}

// The lane exchanges are inline asm, and THIS is the one place that has to get their hazards right: hipcc pads nothing inside
// or in front of an asm statement, and a v_permlane*_swap that reads a register of an MFMA still in flight reads it stale (seen
// once: a single tile, the last MFMA's quadrant).  The compiler's own __builtin_amdgcn_permlane{16,32}_swap would be padded,
// but a chain of them loses its second result in hipcc 7.2 (after two MFMAs, permlane16_swap followed by permlane32_swap stores
// the first result register twice), so they are not used.  Instead:
//   * one tile's exchanges are ONE asm block on the tile's 16 registers, each an in-place "+v" operand (a swap reads and writes
//     both of its registers).  The eight pairs of a SWAP8 are independent, so inside the block no swap reads a register written
//     fewer than seven instructions earlier; the leading s_nop 1 covers a VALU write right in front of the block.
//   * accs_q_to_std -- the only way from quadrant accumulators to an epilogue -- first passes every tile through an EMPTY asm
//     block (the anchor), then waits 19 states (a 16-pass MFMA's result latency), then swaps.  The anchor reads the tile's
//     registers, so every MFMA that writes them is issued before it (a data dependency); asm volatile statements keep their
//     order, so the wait follows all anchors and all swaps follow the wait.  Hence no MFMA that writes a swapped register can
//     be issued after the wait that covers it, whatever the scheduler does with the surrounding code.  The anchors emit nothing.
// tools/mfma16_gemm_check.hip runs both operand formats through this, including single k-steps (last MFMA right in front).
#define EEC_SWAP8(OP)                                                                                                        \
  "v_permlane" OP "_swap_b32 %0, %4\n\tv_permlane" OP "_swap_b32 %1, %5\n\tv_permlane" OP "_swap_b32 %2, %6\n\t"            \
  "v_permlane" OP "_swap_b32 %3, %7\n\tv_permlane" OP "_swap_b32 %8, %12\n\tv_permlane" OP "_swap_b32 %9, %13\n\t"          \
  "v_permlane" OP "_swap_b32 %10, %14\n\tv_permlane" OP "_swap_b32 %11, %15\n\t"
// ASM on the 16 registers of a tile as operands %0 .. %15 (vector elements cannot be asm operands: through scalars)
#define EEC_TILE_ASM(acc, ASM)                                                                                                          \
  do {                                                                                                                                  \
    float r0 = acc[0], r1 = acc[1], r2 = acc[2], r3 = acc[3], r4 = acc[4], r5 = acc[5], r6 = acc[6], r7 = acc[7];                       \
    float r8 = acc[8], r9 = acc[9], r10 = acc[10], r11 = acc[11], r12 = acc[12], r13 = acc[13], r14 = acc[14], r15 = acc[15];           \
    asm volatile(ASM                                                                                                                    \
                 : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7), "+v"(r8), "+v"(r9), "+v"(r10),      \
                   "+v"(r11), "+v"(r12), "+v"(r13), "+v"(r14), "+v"(r15));                                                             \
    acc = (f32x16){r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15};                                               \
  } while (0)
// one tile, WITHOUT the wait for MFMAs in flight: kernels call accs_q_to_std
__device__ __forceinline__ void acc_q_to_std(f32x16& acc) { EEC_TILE_ASM(acc, "s_nop 1\n\t" EEC_SWAP8("16") EEC_SWAP8("32") "s_nop 1"); }
// standard -> quadrant layout, in front of an accumulation (the tile comes from VALU code or from memory, not from an MFMA)
__device__ __forceinline__ void acc_std_to_q(f32x16& acc) { EEC_TILE_ASM(acc, "s_nop 1\n\t" EEC_SWAP8("32") EEC_SWAP8("16") "s_nop 1"); }
// the anchor: an empty statement that READS the tile, so every MFMA that writes the tile is issued before it
__device__ __forceinline__ void acc_anchor(const f32x16& acc) {
  asm volatile("" ::"v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]), "v"(acc[4]), "v"(acc[5]), "v"(acc[6]), "v"(acc[7]), "v"(acc[8]),
               "v"(acc[9]), "v"(acc[10]), "v"(acc[11]), "v"(acc[12]), "v"(acc[13]), "v"(acc[14]), "v"(acc[15]));
}
template <int MT, int NT>
__device__ __forceinline__ void accs_q_to_std(f32x16 (&acc)[MT][NT]) {
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc_anchor(acc[a][b]);
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 2" ::: "memory");
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc_q_to_std(acc[a][b]);
}
template <int MT, int NT>
__device__ __forceinline__ void accs_std_to_q(f32x16 (&acc)[MT][NT]) {
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc_std_to_q(acc[a][b]);
}

}  // namespace eec
