// The row-tile chain kernel.  Its core is the fused Conformer feed-forward half-step (SURVEY 8a row a5,
// torchaudio _FeedForwardModule + the 0.5*y + x residual of ConformerLayer; a8 for the optional final LayerNorm):
//
//     x <- [LN_final]( 0.5 * ( W2 . silu( W1 . LN(x) + b1 ) + b2 ) + x )
//
// of which one launch runs one or two, optionally preceded by the conv-module tail (depthwise + pointwise-2, a7) and
// followed by the next half-layer's attention in_proj (a6) -- everything between two cross-tile dependencies of the
// layer stack (see ffn_chain_kernel below and DESIGN.md section 5).
//
// One 512-thread workgroup owns 64 rows of x; the [64, F] hidden activation never leaves the CU.
// F is walked in chunks of 128 hidden units.  The 8 waves are specialised (one wave of each kind
// per SIMD):
//   producers (waves 0-3): GEMM1 in the swapped orientation (lane = frame, register quad = 4
//       consecutive hidden units; wave wl makes hidden [32wl, 32wl+32) of the chunk for all 64
//       rows; accumulators start at the bias), SiLU in the exp2 domain (log2 e folded into W1/b1,
//       1/log2 e into W2), hi/lo split, ds_write_b64 into H[c & 1][frame][hidden];
//   consumers (waves 4-7): GEMM2 (normal orientation) of chunk c-1 from H[(c-1) & 1], wave wl
//       accumulating output columns [64wl, 64wl+64) in registers that live across all chunks.
// In slot s the producers multiply chunk s and, inside that k-loop (two values per k-step, in the
// shadow of the step's MFMAs), SiLU chunk s-1 into H[(s-1) & 1]; the consumers eat chunk s-2.  Both
// waves of a SIMD therefore run continuous MFMA streams of 32*NP MFMAs per slot, with ONE workgroup
// barrier per slot.  (A stand-alone SiLU phase halves the partner wave's MFMA rate and is pure
// critical path: measured 9.8k cycles per slot against 6.1k of MFMA work.)
// Each wave streams its own, disjoint weight fragments from L2 straight into a register ring
// (1 KiB per load) that runs PF k-steps ahead, across chunk boundaries.
//
// Algorithmic work: 4*D*F flop per row (2.097 MFLOP at D=256, F=2048); bound: MFMA.
// Executed MFMA work is NP x that.  HBM/L2 traffic per launch: x read+write 2 KiB/row; each
// workgroup streams all 2*D*F*2 B (x2 planes when NP=3) of weights once from L2.
#ifdef EEC_FFN_TRAIN_BWD  // fourth object of this source: the backward variants, on bf16 operands (see eec_device.h)
#define EEC_OPERAND_BF16 1
#endif
#if defined(EEC_FFN_TRAIN) || defined(EEC_FFN_TRAIN_BWD)
// the training variants' single-product form runs on the 16x16x32 shape as well: its accumulator layout stores 16 rows x 64 B per
// instruction to the tape; the 32x32 layout's 32 rows x 32 B make the same launch 417 instead of 88 us (profiles/r04_micro_ffn_train_fwd.txt)
#define EEC_MFMA16_NP1 1
#endif
#include "eec_blocks.h"
#include "eec_drop.h"

namespace eec {

constexpr int kFfnThreads = 512;
constexpr int kFC = 128;                          // hidden units per chunk (4 waves x 32)
constexpr int kHLd = (kFC + 8) * 2;               // 272
template <int D>
struct FfnGeo {
  using G = Geo<D>;
  static constexpr int kHPlane = G::kRows * kHLd;                 // 17408 / 8704
  static constexpr int kNT2 = D / 128;                            // output column tiles per consumer wave: 2 / 4
  // A hi/lo planes + two H buffers of two planes each; the fp32 exchange tile of the row passes aliases the H buffers
  // (D = 256: it fits inside them; D = 512: it is the larger of the two)
  static constexpr int kLds = 2 * G::kAPlane + (4 * kHPlane > G::kETile ? 4 * kHPlane : G::kETile);  // 137216 / 132608
};
#ifndef EEC_TR_NT
#define EEC_TR_NT 1  // TR variants: tape stores with the non-temporal hint
#endif
// k-steps of W1 / W2 fragments a producer / consumer wave keeps in flight.  The shared weight stream
// out of L2 is latency x concurrency bound (tools/l2bw.hip: 64 KiB in flight per CU -> 18 TB/s,
// 128 KiB -> 28 TB/s), so the rings are as deep as the register budget allows.
#if defined(EEC_FFN_TRAIN_BWD) && !defined(EEC_PF1_NP3)
// the backward variants' producers hold 32 more values across a slot (the requested pre-activations): paid for with two k-steps of the ring
#define EEC_PF1_NP3 6
#define EEC_PF2_NP3 2
#define EEC_PF1_NP1 12
#define EEC_PF2_NP1 8
#endif
#ifndef EEC_PF1_NP3
#define EEC_PF1_NP3 8
// (the 16x16x32 consumer loop of the split format needs a few registers more than a 32x32x16 one, and with four steps in flight
// it spilled 35 of them into the chunk loop: same-box A/B 217.3 us per chain launch with 4, 214.3 us with 2)
#define EEC_PF2_NP3 2
#define EEC_PF1_NP1 12
#define EEC_PF2_NP1 8
#endif
// (D = 512: a consumer's ring holds 4 column tiles per k-step instead of 2, so it is half as deep)
template <int D, int NP> struct FfnPf { static constexpr int P1 = EEC_PF1_NP3, P2 = (D == 512 && EEC_PF2_NP3 > 2) ? EEC_PF2_NP3 / 2 : EEC_PF2_NP3; };
template <int D> struct FfnPf<D, 1> { static constexpr int P1 = EEC_PF1_NP1, P2 = D == 512 ? EEC_PF2_NP1 / 2 : EEC_PF2_NP1; };
#ifndef EEC_PF1_NP8
#define EEC_PF1_NP8 6
#define EEC_PF2_NP8 3
#endif
template <int D> struct FfnPf<D, 8> { static constexpr int P1 = EEC_PF1_NP8, P2 = D == 512 ? 2 : EEC_PF2_NP8; };  // D = 512: continued stream, PF | k-steps  // hi fragments only ride the ring in the f8 stream
#ifndef EEC_SIDE_VALU_NP8
#define EEC_SIDE_VALU_NP8 5  // VALU instructions of the SiLU side work pinned behind each MFMA of GEMM1 (f8 stream)
#endif
#ifndef EEC_SIDE_VALU_NP3
#define EEC_SIDE_VALU_NP3 3  // VALU instructions of the SiLU side work pinned behind each MFMA pair of GEMM1 (split format)
#endif
#ifndef EEC_NW1
#define EEC_NW1 4
#endif
constexpr int kNW1 = EEC_NW1;
#ifndef EEC_NW2
#define EEC_NW2 1
#endif
constexpr int kNW2 = EEC_NW2;  // lo8 group buffers of the consumers' GEMM2 (2 = whole stage resident)  // lo8 group buffers of the producers' GEMM1 (4 = whole stage resident)
constexpr int kH8Ld = kFC + 16;  // 144: H lo8 byte plane row stride (NP == 8)

#if defined(EEC_TIMELINE) && (!defined(EEC_FFN_D) || EEC_FFN_D == 256)
// Diagnostic build only: s_memtime stamps of wave 0 (consumer slot of the buffer) and wave 4 of the first
// 8 workgroups, written to a buffer nothing else reads.  Layout: [block][role][stamp], 128 stamps.
__device__ unsigned long long* g_timeline = nullptr;
__device__ __forceinline__ void tl_stamp(int& idx) {
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0 && (w == 0 || w == 4) && blockIdx.x < 8 && g_timeline && idx < 128)
    g_timeline[(blockIdx.x * 2 + (w >> 2)) * 128 + idx] = __builtin_amdgcn_s_memtime();
  ++idx;
}
#ifndef EEC_TL_NS
#define EEC_TL_NS 0  // 0: stamp every launch; 1 / 2: only the variants with that many stages
#endif
#define TL_STAMP()                                  \
  do {                                              \
    if (EEC_TL_NS == 0 || EEC_TL_NS == NS) tl_stamp(tl_idx); \
  } while (0)
#ifdef EEC_KSTEP_STAMPS
__device__ int g_ks_idx;  // stamps of consumer wave 0, block 0 only, slots 3..5
__device__ unsigned long long g_ks[256];
__device__ void eec_kstep_stamp() {
  if (threadIdx.x == 0 && blockIdx.x == 0 && g_ks_idx < 256) g_ks[g_ks_idx++] = __builtin_amdgcn_s_memtime();
}
extern "C" int eec_debug_ksteps(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  int zero = 0;
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ks), 256 * 8);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_ks_idx), &zero, 4);
  return (int)e;
}
#endif
#else
#define TL_STAMP()
#endif

// L2 warm-up: one dword per 128-byte line; the value only feeds a sink that keeps the load alive.
// instruction j (0 or 1) of this wave's part of the workgroup's 1/32 share of an array (the workgroups of an
// XCD -- blockIdx % 8 -- share one L2; a share is at most 2 x 64 lines per wave for the matrices used here)
__device__ __forceinline__ unsigned touch_share(const void* base, size_t bytes, int wl, int j, int lane = lane_id()) {
  const size_t n_lines = bytes / 128, per_wg = (n_lines + 31) / 32, per_wave = (per_wg + 3) / 4;
  const size_t k = (size_t)j * 64 + lane;
  const size_t ln = ((blockIdx.x >> 3) & 31) * per_wg + wl * per_wave + k;
  return (k < per_wave && ln < n_lines) ? *(const unsigned*)((const char*)base + ln * 128) : 0u;
}
// 16-byte store to the training tape.  Non-temporal: 268 MB of [M, F] tensors per launch written through the L2 as ordinary lines push
// the weight stream -- 6.5 MB per stage against 4 MB of L2 per XCD -- out of it (same-box A/B: 172.6 us per launch with plain stores,
// 135.4 us with the hint, 99.7 us without any tape stores; profiles/r04_micro_ffn_train_fwd.txt)
__device__ __forceinline__ void tape_store4(float* p, float x, float y, float z, float w) {
  const f32x4 v = {x, y, z, w};
#if EEC_TR_NT
  __builtin_nontemporal_store(v, (f32x4*)p);
#else
  *(f32x4*)p = v;
#endif
}
template <bool B>
struct BoolTag {
  static constexpr bool value = B;
};
// One FFN stage's packed weight streams.
struct WPtrs {
  const uint4 *w1p, *w2p, *w1f8, *w2f8;
};

// Row pass between two GEMM stages of the chain: the fp32 exchange tile `lds_e` (this stage's product, bias
// included) is scaled and - HAS_RES - added to the residual rows `xr` (wave w owns local rows 8w .. 8w+7, one float4 per lane), the
// optional final LayerNorm is applied, the rows are stored to x (and to `tap`), and - NPN != 0 - the rows are
// LayerNormed with (nln_g, nln_b) and written as the NEXT stage's activation planes (NPN format) at `smem`.
template <int D, int NPN, bool HAS_RES>
__device__ __forceinline__ void chain_rowpass(char* smem, const char* lds_e, float* __restrict__ x, RowV<Geo<D>::kQ> (&xr)[Geo<D>::kRPW],
                                              int row0, int M, float scale, const float* __restrict__ fin_g,
                                              const float* __restrict__ fin_b, float* __restrict__ tap,
                                              const float* __restrict__ nln_g, const float* __restrict__ nln_b,
                                              int lane = lane_id(), int w = wave_id()) {
  using G = Geo<D>;
  constexpr int RPW = G::kRPW, Q = G::kQ;
  RowV<Q> v[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    v[i] = HAS_RES ? xr[i] : zero_row<Q>();  // !HAS_RES: the residual went in as the accumulator init
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float4 e = *(const float4*)(lds_e + (w * RPW + i) * G::kELd + (q * 256 + lane * 4) * 4);
      v[i].p[q].x += scale * e.x;
      v[i].p[q].y += scale * e.y;
      v[i].p[q].z += scale * e.z;
      v[i].p[q].w += scale * e.w;
    }
  }
  if (fin_g) layer_norm_rows<D, RPW>(v, load_row<D>(fin_g, lane), load_row<D>(fin_b, lane));
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int row = row0 + w * RPW + i;
    if (row < M) {
      store_row<D>(x + (size_t)row * D, v[i], lane);
      if (tap) store_row<D>(tap + (size_t)row * D, v[i], lane);
    }
  }
  if constexpr (NPN != 0) {
    layer_norm_rows<D, RPW>(v, load_row<D>(nln_g, lane), load_row<D>(nln_b, lane));
    rows_to_planes<D, NPN, RPW>(smem, v, w * RPW, row0, M, true, lane);
  }
}

// The chain kernel: [conv-module tail ->] FFN stage(s) [-> QKV], one 64-row tile per workgroup, x rows touched
// in HBM only for the residual stream.
//   NP   FFN product format (1, 3, 8);  ACT 0: SiLU in the exp2 domain (Conformer; log2 e folded into the packed
//        weights), 1: ReLU (legacy pre-norm layer, models/layers/position_wise_feed_forward.py:9-23, plain weights)
//   FNP  0: stage 0 reads x;  else: the depthwise + pointwise-2 front (format FNP) produces x first
//   QNP  0: none;  else: the attention in_proj of the NEXT half-layer (format QNP) runs on the final rows
//   NS   number of FFN stages (1 or 2)
//   TR   the feed-forward module of the TRAINING step's forward (train.hip ffn_fwd; train.py:54 in train mode): one stage, no front
//        or tail, ACT = 2 (SiLU in the plain domain: the weights are this step's parameters, packed with scale 1), dropout after
//        the activation and on the module's output (a.tr sites), output rows to a.tr.y, and everything the backward reads --
//        LN(x) and its statistics, W1 . LN(x) + b1, drop(silu(.)) -- recorded on the way: the [M, F] tensors are written once
//        and never read back by the forward.
//        TR = 2: the data path of that module's BACKWARD with the same machinery (x = dh, W1 slot = W2^T, W2 slot = W1^T, bf16 operands):
//        GEMM1 gives dh . W2 per chunk, the activation step is * mask * silu'(pre) with `pre` read back from the tape (requested one
//        slot ahead) and the result d(pre) stored for the weight-gradient GEMM, GEMM2 accumulates d(pre) . W1 = d(LN(x)); no LayerNorm,
//        bias, residual or output dropout
template <int D, int NP, int ACT, int FNP, int QNP, int NS, int TR = 0>
#ifndef EEC_FFN_MINWAVES
#define EEC_FFN_MINWAVES 2
#endif
__global__ __launch_bounds__(kFfnThreads, EEC_FFN_MINWAVES) void ffn_chain_kernel(ChainArgs a) {
  static_assert(!TR || (FNP == 0 && QNP == 0 && NS == 1 && ACT == 2 && NP != 8), "TR: one plain stage");
  static_assert(TR || ACT != 2, "ACT = 2 is the training variant's");
  static_assert((TR == 2) == (EEC_OPERAND_BF16 != 0), "the backward variant (and only it) runs on bf16 operands");
  using G = Geo<D>;
  using FG = FfnGeo<D>;
  constexpr int MT = G::kMT, NW = G::kNW, KS = G::kKS, RPW = G::kRPW, NT2 = FG::kNT2;
  constexpr int kALd = G::kALd, kAPlane = G::kAPlane, kA8Ld = G::kA8Ld, kHPlane = FG::kHPlane;
  constexpr size_t nts = (size_t)KS * 128;  // uint4 between adjacent n-tiles of a K = D matrix
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int kPF1 = FfnPf<D, NP>::P1, kPF2 = FfnPf<D, NP>::P2;
  // A consumer wave owns NT2 output column tiles.  In the f8 stream more than two tiles per k-step do not fit the register
  // file (ring + lo8 buffers + e5m2 copies per tile), so at D = 512 a chunk's GEMM2 runs as NH = 2 column passes of
  // NTP = 2 tiles over the same H chunk, each pass's weight stream continuing into the next (gemm_ring_f8 CONT).
  constexpr int NH = (NP == 8 && NT2 > 2) ? NT2 / 2 : 1, NTP = NT2 / NH;
  const int lane = lane_id(), w = wave_id();
  const int hh = lane >> 5, wl = w & 3;  // index inside the role (0 .. 3)
  const int w_s = wave_id_sgpr();
  const int wl_s = w_s & 3;  // the same index from the SGPR copy
  // wave-uniform.  The producers are the OLDER waves (0-3): issue arbitration between the two waves of a SIMD goes by
  // priority, then age, and the producers are the critical path of the chunk pipeline (measured -2.3 % forward against
  // the opposite assignment; raising their priority with s_setprio instead makes it slower)
  const bool is_producer = w < 4;
  const int row0 = row_tile_index() * G::kRows;
  const int M = a.M, F = a.F;
  float* __restrict__ x = a.x;
  char* lds_h = smem + 2 * kAPlane;  // H[buf][plane][rows][136]
  char* lds_e = lds_h;               // fp32 exchange tile: aliases the H buffers (dead outside the chunk loops), not the planes
  const char* a_lane = smem + (lane & 31) * kALd + hh * 16;

  const int nft = F / 32;  // 32-wide hidden tiles
  const int nchunk = (nft + 3) / 4;
  const int ks2_total = F / 16;
#ifndef EEC_SKEW
#define EEC_SKEW 56
#endif
#ifndef EEC_WARM_SLOTS
#define EEC_WARM_SLOTS 4  // slots before the end of a stage at which the consumers start the L2 warm-up
#endif
  // chunk index wrapped into [0, nchunk): the identity for every index the loops below pass
  auto phys = [&](int c) { return c >= nchunk ? c - nchunk : c; };
  const size_t w2_nt_stride = (size_t)ks2_total * 128;

#ifdef EEC_TIMELINE
  int tl_idx = 0;
#endif
  TL_STAMP();  // 0: kernel entry
#if EEC_SKEW > 0
  // De-phase the workgroups that share an XCD (blockIdx % 8) by up to 3 x EEC_SKEW x 64 cycles (~5 us): all 32 CUs of
  // an XCD otherwise walk the same weight stream in lockstep and hit the same L2 channels at the same time.  It changes
  // no arithmetic.  Measured: neutral on boxes that run the forward in
  // 2.8 ms, -9 % on a box that ran it in 3.3 ms.
  for (int i = 0; i < (int)((blockIdx.x >> 3) & 3); ++i) __builtin_amdgcn_s_sleep(EEC_SKEW);
#endif
  constexpr int RNP = NP == 8 ? 1 : NP;  // the f8 stream keeps only the hi fragments in the ring
  // split format (NP = 3): the products run on the 16x16x32 shape and the accumulators live in the quadrant layout inside
  // the chunk loops (eec_device.h); NP = 1 and the f8 stream keep the 32x32 shapes and the standard layout
  constexpr bool Q16 = kMfma16For<NP>;
  // Everything below is instantiated ONCE PER ROLE (the tag is a compile-time bool) and the role split is the
  // outermost branch: each role then carries only its own rings and accumulators through the stage loop
  // (with the split inside the loop the register allocator keeps both roles' state live: ~600 spilled VGPRs).
  auto run = [&](auto prod_tag) {
  constexpr bool producer = decltype(prod_tag)::value;
  [[maybe_unused]] const eect::DropState ds_act(eect::Drop{TR ? a.tr.p : 0.0f, a.tr.seed, a.tr.site_act});
  WRing<RNP, kPF1, 1> r1;
  WRing<RNP, kPF2, NTP> r2;
  WGroupF8<1> wg1[kNW1];    // NP == 8: lo8 + scales of GEMM1 (K = D = D/64 groups), rolling through kNW1 buffers
  WGroupF8<NTP> wg2[kNW2];  //          ... of a whole GEMM2 stage (128 hidden = 2 groups, NTP n-tiles)
  const size_t w2f8_nt = (size_t)(F / 64) * kF8Rec;
  auto w1f8_lane = [&](const WPtrs& W, int ft) { return W.w1f8 + (size_t)ft * (D / 64) * kF8Rec + lane; };
  auto w2f8_lane = [&](const WPtrs& W, int c, int h = 0) {  // column pass h of chunk c
    return W.w2f8 + ((size_t)(NT2 * wl + NTP * h) * (F / 64) + 2 * c) * kF8Rec + lane;
  };
  auto fill1 = [&](const WPtrs& W, int ft) {  // start the W1 stream of hidden tile ft
    if constexpr (NP == 8) {
      ring_fill_f8<kPF1, 1>(r1, w1f8_lane(W, ft), 0);
#pragma unroll
      for (int g = 0; g < kNW1; ++g) f8_group_load<1>(wg1[g], w1f8_lane(W, ft) + (size_t)g * kF8Rec, 0);
    } else {
      ring_fill<RNP, kPF1, 1>(r1, W.w1p + (size_t)ft * nts + lane, 0, KS);
    }
  };
  auto fill2 = [&](const WPtrs& W, int c) {  // start the W2 stream of chunk c
    if constexpr (NP == 8) {
      ring_fill_f8<kPF2, NTP>(r2, w2f8_lane(W, c), w2f8_nt);
#pragma unroll
      for (int g = 0; g < kNW2; ++g) f8_group_load<NTP>(wg2[g], w2f8_lane(W, c) + (size_t)g * kF8Rec, w2f8_nt);
    } else {
      ring_fill<RNP, kPF2, NTP>(r2, W.w2p + ((size_t)(NT2 * wl) * ks2_total + c * (kFC / 16)) * 128 + lane, w2_nt_stride,
                             min(kFC / 16, ks2_total - c * (kFC / 16)));
    }
  };
  // both weight streams of a stage start one phase ahead: inside the prologue / the previous stage's row pass
  auto start_streams = [&](const WPtrs& W) {
    if constexpr (producer) {
      if (wl < nft) fill1(W, phys(0) * 4 + wl);
    } else {
      fill2(W, phys(0));
    }
  };
  // stage parameters by SELECT, never by a runtime index into the by-value argument block (which would force
  // the whole block into scratch memory)
#define EEC_STAGE_FIELD(si, f) ((si) == 0 ? a.st[0].f : a.st[1].f)
  auto wptrs = [&](int si) {
    return WPtrs{EEC_STAGE_FIELD(si, w1p), EEC_STAGE_FIELD(si, w2p), EEC_STAGE_FIELD(si, w1f8), EEC_STAGE_FIELD(si, w2f8)};
  };

  unsigned sink_front = 0;
  // ---- planes of stage 0 ----
  if constexpr (FNP != 0) {
    ProjStream<FNP, kDPF, NW> rp;
    proj_fill<D, FNP, kDPF, NW>(rp, WMat{a.pw2.wp, a.pw2.wf8}, NW * w);
#if EEC_WARM_SLOTS > 0
    {  // stage 0's weights are cold in this XCD's L2: fetch this workgroup's share while the conv front runs
      const WPtrs W0 = wptrs(0);
      const size_t wbytes = NP == 8 ? (size_t)(F / 32) * (D / 64) * kF8Rec * 16 : (size_t)F * D * 2 * (NP == 3 ? 2 : 1);
      unsigned t = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        t ^= touch_share(NP == 8 ? (const void*)W0.w1f8 : (const void*)W0.w1p, wbytes, wl, j);
        t ^= touch_share(NP == 8 ? (const void*)W0.w2f8 : (const void*)W0.w2p, wbytes, wl, j);
      }
      sink_front = t;
    }
#endif
    TL_STAMP();  // front: weight requests issued
    dw_front<D, FNP>(smem, a.dw, M, row0);
    TL_STAMP();  // front: depthwise planes written
    RowV<G::kQ> xr[RPW];  // residual rows: requested now, consumed after the pointwise-2 GEMM
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int row = row0 + w * RPW + i;
      xr[i] = zero_row<G::kQ>();
      if (row < M) xr[i] = load_row<D>(x + (size_t)row * D, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // conv planes complete; the staged GLU rows / taps are dead
    TL_STAMP();  // front: barrier
    f32x16 accp[MT][NW];
    pw2_gemm<D, FNP>(accp, smem, a.pw2, rp);
    TL_STAMP();  // front: pointwise-2 done
    start_streams(wptrs(0));
    acc_swapped_to_etile<MT, NW>(lds_e, G::kELd, accp, 32 * NW * w);
    __syncthreads();  // tile complete; every wave is done reading the conv planes
    TL_STAMP();  // front: exchange tile complete
    chain_rowpass<D, NP, true>(smem, lds_e, x, xr, row0, M, 1.0f, nullptr, nullptr, nullptr, a.st[0].ln_g, a.st[0].ln_b);
  } else {
    const WPtrs W0 = wptrs(0);
    if constexpr (TR == 2) {
      // x = the gradient of the module's output; dh = res_scale * dropmask_res(x) are the rows this launch multiplies -- and, stored to
      // a.tr.ln, the operand of the W2 / b2 gradient
      const eect::DropState ds_res(eect::Drop{a.tr.p, a.tr.seed, a.tr.site_res});
      const float rsc = a.st[0].res_scale;
      RowV<G::kQ> v[RPW];
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int row = row0 + w * RPW + i;
        v[i] = zero_row<G::kQ>();
        if (row < M) v[i] = load_row<D>(x + (size_t)row * D, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      start_streams(W0);
      if (a.tr.pl_x) {
        // A LayerNorm backward in front of the module (the layer-final LayerNorm when this is the second feed-forward module): the rows
        // of x are the gradient of that LayerNorm's OUTPUT; they become -- in place, and for everything below -- the gradient of its
        // input, LN'(g) = rstd (t - mean_c(t) - xh mean_c(t xh)) with t = g gamma, xh = (x_ln - mean) rstd.  The weight / bias gradient
        // leaves as one partial row per WAVE (a.tr.pl_part[8 block + wave][2][D]: no LDS is free here), summed by the host's reduce launch.
        constexpr int Q = G::kQ;
        const RowV<Q> gam = load_row<D>(a.tr.pl_g, lane);
        RowV<Q> xh[RPW];
        float rsd[RPW], c1[RPW], c2[RPW];
        RowV<Q> dgs = zero_row<Q>(), dbs = zero_row<Q>();
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          const int row = row0 + w * RPW + i;
          const bool ok = row < M;
          const float mu = ok ? a.tr.pl_mean[row] : 0.0f;
          rsd[i] = ok ? a.tr.pl_rstd[row] : 0.0f;
          xh[i] = ok ? load_row<D>(a.tr.pl_x + (size_t)row * D, lane) : zero_row<Q>();
          c1[i] = 0.0f, c2[i] = 0.0f;
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            float4& h = xh[i].p[q];
            h.x = (h.x - mu) * rsd[i], h.y = (h.y - mu) * rsd[i], h.z = (h.z - mu) * rsd[i], h.w = (h.w - mu) * rsd[i];
            const float4 ev = v[i].p[q], gq = gam.p[q];
            const float tx = ev.x * gq.x, ty = ev.y * gq.y, tz = ev.z * gq.z, tw = ev.w * gq.w;
            c1[i] += tx + ty + tz + tw;
            c2[i] += tx * h.x + ty * h.y + tz * h.z + tw * h.w;
            dgs.p[q].x += ev.x * h.x, dgs.p[q].y += ev.y * h.y, dgs.p[q].z += ev.z * h.z, dgs.p[q].w += ev.w * h.w;
            dbs.p[q].x += ev.x, dbs.p[q].y += ev.y, dbs.p[q].z += ev.z, dbs.p[q].w += ev.w;
          }
        }
        wave_sum_n<RPW>(c1);
        wave_sum_n<RPW>(c2);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          const int row = row0 + w * RPW + i;
          const float m1 = c1[i] * (1.0f / D), m2 = c2[i] * (1.0f / D);
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const float4 ev = v[i].p[q], gq = gam.p[q], h = xh[i].p[q];
            v[i].p[q].x = rsd[i] * (ev.x * gq.x - m1 - h.x * m2);
            v[i].p[q].y = rsd[i] * (ev.y * gq.y - m1 - h.y * m2);
            v[i].p[q].z = rsd[i] * (ev.z * gq.z - m1 - h.z * m2);
            v[i].p[q].w = rsd[i] * (ev.w * gq.w - m1 - h.w * m2);
          }
          if (row < M) store_row<D>(x + (size_t)row * D, v[i], lane);  // read again (by this same wave) as the residual gradient in the epilogue
        }
        float* pw = a.tr.pl_part + ((size_t)blockIdx.x * 8 + w) * 2 * D;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          *(float4*)(pw + q * 256 + lane * 4) = dgs.p[q];
          *(float4*)(pw + D + q * 256 + lane * 4) = dbs.p[q];
        }
      }
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int row = row0 + w * RPW + i;
#pragma unroll
        for (int q = 0; q < G::kQ; ++q) {
          float m[4];
          ds_res.mul4((size_t)row * D + q * 256 + lane * 4, m);
          v[i].p[q].x *= rsc * m[0], v[i].p[q].y *= rsc * m[1], v[i].p[q].z *= rsc * m[2], v[i].p[q].w *= rsc * m[3];
        }
        if (row < M) store_row<D>(a.tr.ln + (size_t)row * D, v[i], lane);
      }
      rows_to_planes<D, NP, RPW>(smem, v, w * RPW, row0, M, false);
    } else if constexpr (TR == 1) {  // as rows_f32_to_planes, and the LayerNormed rows and their statistics go to the tape
      const RowV<G::kQ> lg = load_row<D>(a.st[0].ln_g, lane), lb = load_row<D>(a.st[0].ln_b, lane);
      RowV<G::kQ> v[RPW];
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int row = row0 + w * RPW + i;
        v[i] = zero_row<G::kQ>();
        if (row < M) v[i] = load_row<D>(x + (size_t)row * D, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      start_streams(W0);
      float mu[RPW], rs[RPW];
      layer_norm_rows<D, RPW>(v, lg, lb, mu, rs);
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int row = row0 + w * RPW + i;
        if (row < M) {
          store_row<D>(a.tr.ln + (size_t)row * D, v[i], lane);
          if (lane == 0) a.tr.mean[row] = mu[i], a.tr.rstd[row] = rs[i];
        }
      }
      rows_to_planes<D, NP, RPW>(smem, v, w * RPW, row0, M, true);
    } else {
      rows_f32_to_planes<D, NP, true>(smem, x, row0, M, a.st[0].ln_g, a.st[0].ln_b, [&]() { start_streams(W0); });
    }
  }
  TL_STAMP();  // 1: prologue done
  __syncthreads();
  TL_STAMP();  // 2: after prologue barrier

  [[maybe_unused]] ProjStream<(QNP ? QNP : 1), kLPF, NW> rq;  // tail: first k-steps of this wave's Q weight tiles
  unsigned sink = 0;  // keeps the L2 warm-up loads alive
  const int nslots = nchunk + 2;
  f32x16 acc2c[NH][MT][NTP];  // consumers' [rows x D/4] output accumulators (unused by producers)
  static_range<0, NS>([&](auto si_tag) {
    constexpr int si = decltype(si_tag)::value;  // NS is a template parameter and the loop is unrolled: as a runtime loop it makes
                                     // every ring and accumulator loop-carried (~250 spilled VGPRs in the hot loops)
    const WPtrs W = wptrs(si);
    const float* __restrict__ b1s = EEC_STAGE_FIELD(si, b1);
    // The two roles run separate loops (so neither carries the other's registers); both execute
    // exactly nslots workgroup barriers.  Pipeline: chunk c is multiplied (GEMM1) in slot c, SiLU'd
    // and written to H[c & 1] in slot c+1 -- inside the k-loop of GEMM1(c+1), two values per k-step in
    // the shadow of that step's MFMAs -- and consumed (GEMM2) in slot c+2.
    if constexpr (producer) {
      // SiLU + hi/lo split + ds_write of values [2q, 2q+1] of tile mt of a finished accumulator.  Standard layout: register quad
      // g = q >> 1 of lane (hh, r32) is hidden units 8 g + 4 hh .. + 3 of frame r32.  Quadrant layout (Q16): quad g = 2 ra + cb is
      // hidden units 16 ra + 8 hh + 4 u .. + 3 of frame 16 cb + (lane & 15) -- either way four consecutive halves of one H row.
      // TR = 2: the pre-activations of the chunk this wave multiplied last, in the accumulator's element order
      [[maybe_unused]] f32x16 preq[TR == 2 ? MT : 1];
      [[maybe_unused]] auto request_pre = [&](int hcol0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int frame = Q16 ? mt * 32 + 16 * (g & 1) + (lane & 15) : mt * 32 + (lane & 31);
            const int hid = Q16 ? wl * 32 + 16 * (g >> 1) + 8 * hh + 4 * ((lane >> 4) & 1) : wl * 32 + 4 * hh + g * 8;
            const int row = min(row0 + frame, M - 1);  // clamped, not branched: rows past the end are never stored
            const f32x4 v = __builtin_nontemporal_load((const f32x4*)(a.tr.pre + (size_t)row * F + hcol0 + hid));
            preq[mt][4 * g] = v[0], preq[mt][4 * g + 1] = v[1], preq[mt][4 * g + 2] = v[2], preq[mt][4 * g + 3] = v[3];
          }
      };
      auto silu_pair = [&](const f32x16 (&acc)[MT][1], char* hb, int step, h2& keep_hi, h2& keep_lo, [[maybe_unused]] int hcol0 = 0) {
        const int mt = step >> 3, q = step & 7;
        const float u0 = acc[mt][0][2 * q], u1 = acc[mt][0][2 * q + 1];
        if constexpr (TR == 2) {
          // u0, u1 are (dh . W2) of two hidden units; their pre-activations wait in preq (requested at the end of the previous slot)
          const float x0 = preq[mt][2 * q], x1 = preq[mt][2 * q + 1];
          const float sg0 = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-kLog2e * x0));
          const float sg1 = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-kLog2e * x1));
          const float t0 = u0 * sg0 * (1.0f + x0 * (1.0f - sg0)), t1 = u1 * sg1 * (1.0f + x1 * (1.0f - sg1));
          if ((q & 1) == 0) {
            keep_hi = __builtin_bit_cast(h2, t0);
            keep_lo = __builtin_bit_cast(h2, t1);
            return;
          }
          const int g = q >> 1;
          const int frame = Q16 ? mt * 32 + 16 * (g & 1) + (lane & 15) : mt * 32 + (lane & 31);
          const int hid = Q16 ? wl * 32 + 16 * (g >> 1) + 8 * hh + 4 * ((lane >> 4) & 1) : wl * 32 + 4 * hh + g * 8;
          const int row = row0 + frame;
          const size_t idx = (size_t)row * F + hcol0 + hid;
          float m[4];
          ds_act.mul4(idx, m);
          const float d0 = __builtin_bit_cast(float, keep_hi) * m[0], d1 = __builtin_bit_cast(float, keep_lo) * m[1], d2 = t0 * m[2], d3 = t1 * m[3];
          if (row < M) tape_store4(a.tr.act + idx, d0, d1, d2, d3);
          constexpr int SNPT = NP == 1 ? 1 : 3;
          const hl2_t sa = split2<SNPT>(d0, d1), sb = split2<SNPT>(d2, d3);
          char* dst = hb + frame * kHLd + hid * 2;
          h4 hi, lo;
          hi.xy = sa.hi, hi.zw = sb.hi, lo.xy = sa.lo, lo.zw = sb.lo;
          *(h4*)dst = hi;
          if (NP == 3) *(h4*)(dst + kHPlane) = lo;
          return;
        }
        if constexpr (TR == 1) {
          // even q: the two SiLU values wait in (keep_hi, keep_lo) as floats; odd q: the quad's four pre-activations and its four
          // dropped activations go to the tape (one float4 each: the (hh, u) lanes of a frame cover 64 contiguous bytes), and the
          // dropped activations, split, into the H tile
          const float s0 = silu_f(u0), s1 = silu_f(u1);
          if ((q & 1) == 0) {
            keep_hi = __builtin_bit_cast(h2, s0);
            keep_lo = __builtin_bit_cast(h2, s1);
            return;
          }
          const int g = q >> 1;
          const int frame = Q16 ? mt * 32 + 16 * (g & 1) + (lane & 15) : mt * 32 + (lane & 31);
          const int hid = Q16 ? wl * 32 + 16 * (g >> 1) + 8 * hh + 4 * ((lane >> 4) & 1) : wl * 32 + 4 * hh + g * 8;
          const int row = row0 + frame;
          const size_t idx = (size_t)row * F + hcol0 + hid;
          float m[4];
          ds_act.mul4(idx, m);
          const float h0 = __builtin_bit_cast(float, keep_hi) * m[0], h1 = __builtin_bit_cast(float, keep_lo) * m[1], h2v = s0 * m[2], h3 = s1 * m[3];
          if (row < M) {
            tape_store4(a.tr.pre + idx, acc[mt][0][2 * q - 2], acc[mt][0][2 * q - 1], u0, u1);
            tape_store4(a.tr.act + idx, h0, h1, h2v, h3);
          }
          constexpr int SNPT = NP == 1 ? 1 : 3;
          const hl2_t sa = split2<SNPT>(h0, h1), sb = split2<SNPT>(h2v, h3);
          char* dst = hb + frame * kHLd + hid * 2;
          h4 hi, lo;
          hi.xy = sa.hi, hi.zw = sb.hi, lo.xy = sa.lo, lo.zw = sb.lo;
          *(h4*)dst = hi;
          if (NP == 3) *(h4*)(dst + kHPlane) = lo;
          return;
        }
        constexpr int SNP = NP == 1 ? 1 : 3;
        const hl2_t sp = ACT == 0 ? split2<SNP>(silu_exp2(u0), silu_exp2(u1)) : split2<SNP>(fmaxf(u0, 0.f), fmaxf(u1, 0.f));
        if ((q & 1) == 0) {
          keep_hi = sp.hi;
          keep_lo = sp.lo;
        } else {
          const int g = q >> 1;
          const int frame = Q16 ? mt * 32 + 16 * (g & 1) + (lane & 15) : mt * 32 + (lane & 31);
          const int hid = Q16 ? wl * 32 + 16 * (g >> 1) + 8 * hh + 4 * ((lane >> 4) & 1) : wl * 32 + 4 * hh + g * 8;
          char* dst = hb + frame * kHLd + hid * 2;
          h4 hi, lo;
          hi.xy = keep_hi, hi.zw = sp.hi, lo.xy = keep_lo, lo.zw = sp.lo;
          *(h4*)dst = hi;
          if (NP == 3) *(h4*)(dst + kHPlane) = lo;
          if (NP == 8) {
            h4 lg;
            lg.xy = lo8_gain(keep_lo), lg.zw = lo8_gain(sp.lo);
            const uint2 lb = __builtin_bit_cast(uint2, lg);
            *(unsigned*)(hb + kHPlane + (mt * 32 + (lane & 31)) * kH8Ld + lo8_pos(wl * 32 + 4 * hh + (q >> 1) * 8)) =
                __builtin_amdgcn_perm(lb.y, lb.x, 0x07050301u);
          }
        }
      };
      auto init_bias = [&](f32x16 (&acc)[MT][1], int ft) {
        if constexpr (TR == 2) {
          zero_acc(acc);
          return;
        }
        if constexpr (Q16) {  // quadrant layout: register 4 (2 ra + cb) + i <-> hidden unit 16 ra + 8 hh + 4 u + i
          const int u = (lane >> 4) & 1;
#pragma unroll
          for (int ra = 0; ra < 2; ++ra) {
            const float4 bb = *(const float4*)(b1s + ft * 32 + 16 * ra + 8 * hh + 4 * u);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) {
                acc[mt][0][4 * (2 * ra + cb) + 0] = bb.x;
                acc[mt][0][4 * (2 * ra + cb) + 1] = bb.y;
                acc[mt][0][4 * (2 * ra + cb) + 2] = bb.z;
                acc[mt][0][4 * (2 * ra + cb) + 3] = bb.w;
              }
          }
          return;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 bb = *(const float4*)(b1s + ft * 32 + 8 * g + 4 * hh);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[mt][0][4 * g + 0] = bb.x;
            acc[mt][0][4 * g + 1] = bb.y;
            acc[mt][0][4 * g + 2] = bb.z;
            acc[mt][0][4 * g + 3] = bb.w;
          }
        }
      };
      // one slot: GEMM1 of chunk s into `cur` while the SiLU of chunk s-1 (held in `prev`) rides along
      // the SiLU side work of one chunk = 8 MT value pairs, spread over the KS k-steps of the next chunk's GEMM1
      constexpr int kSideEvery = KS / (8 * MT);  // 1 (D = 256) / 4 (D = 512)
      auto slot = [&](int s, f32x16 (&cur)[MT][1], f32x16 (&prev)[MT][1]) {
        const int ft = (s < nchunk ? phys(s) : s) * 4 + wl;  // s >= nchunk: no GEMM1 (ft is out of range)
        const bool do_gemm = s < nchunk && ft < nft;
        const bool do_silu = s >= 1 && s - 1 < nchunk && phys(s - 1) * 4 + wl < nft;
        char* hb_prev = lds_h + ((s - 1) & 1) * 2 * kHPlane;
        [[maybe_unused]] const int hcol_prev = do_silu ? phys(s - 1) * kFC : 0;  // TR: hidden column of the chunk being activated
        h2 khi, klo;
        if (do_gemm) {
          init_bias(cur, ft);
          const uint4* w1_lane = W.w1p + (size_t)ft * nts + lane;
          const char* a8_lane = smem + kAPlane + (lane & 31) * kA8Ld + hh * 32;
          if (do_silu) {
            auto side = [&](int st) {
              if (st % kSideEvery == 0) silu_pair(prev, hb_prev, st / kSideEvery, khi, klo, hcol_prev);
            };
            if constexpr (NP == 8)
              gemm_ring_f8<D / 64, 1, true, kPF1, decltype(side), EEC_SIDE_VALU_NP8, kNW1, MT>(
                  cur, a_lane, kALd, a8_lane, kA8Ld, w1f8_lane(W, ft), 0, r1, wg1, side);
            else
              gemm_ring<RNP, KS, 1, true, kPF1, decltype(side), (NP == 3 ? EEC_SIDE_VALU_NP3 : 7), MT, !Q16, !Q16>(cur, a_lane, kALd, kAPlane, w1_lane,
                                                                                                  0, r1, side);
          } else {
            if constexpr (NP == 8)
              gemm_ring_f8<D / 64, 1, true, kPF1, NoSide, 0, kNW1, MT>(cur, a_lane, kALd, a8_lane, kA8Ld,
                                                                                                                    w1f8_lane(W, ft), 0, r1, wg1);
            else
              gemm_ring<RNP, KS, 1, true, kPF1, NoSide, 0, MT, !Q16, !Q16>(cur, a_lane, kALd, kAPlane, w1_lane, 0, r1);
          }
          if (s + 1 < nchunk && phys(s + 1) * 4 + wl < nft) fill1(W, phys(s + 1) * 4 + wl);  // next chunk's W1 stream
          if constexpr (TR == 2) request_pre(phys(s) * kFC);  // consumed by the next slot's side work
        } else if (do_silu) {  // the last chunk's SiLU has no GEMM1 to hide under
#pragma unroll
          for (int st = 0; st < 8 * MT; ++st) silu_pair(prev, hb_prev, st, khi, klo, hcol_prev);
        }
        TL_STAMP();  // producer: slot work done
        __syncthreads();
        TL_STAMP();  // producer: barrier passed
      };
      f32x16 accA[MT][1], accB[MT][1];
      for (int s = 0; s < nslots; s += 2) {
        slot(s, accA, accB);
        if (s + 1 < nslots) slot(s + 1, accB, accA);
      }
    } else {
#pragma unroll
      for (int h = 0; h < NH; ++h) zero_acc(acc2c[h]);
#if EEC_WARM_SLOTS > 0
      unsigned warm[4] = {0u, 0u, 0u, 0u};
#endif
      for (int s = 0; s < nslots; ++s) {
#if EEC_WARM_SLOTS > 0
        if (s == nslots - EEC_WARM_SLOTS) {
          // L2 warm-up for the stage boundary, in the consumers' slack: this workgroup's 1/32 share of what the next
          // phase streams (the next stage's weights, or the in_proj weights of the tail).  Without it the boundary
          // starts with a burst of cold misses (each XCD fetches its own copy: ~26 MB at once).
          const int lane_t = fresh_lane();
          if constexpr (si + 1 < NS) {
            const WPtrs Wn = wptrs(si + 1);
            const size_t wbytes = NP == 8 ? (size_t)(F / 32) * (D / 64) * kF8Rec * 16 : (size_t)F * D * 2 * (NP == 3 ? 2 : 1);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              warm[j] = touch_share(NP == 8 ? (const void*)Wn.w1f8 : (const void*)Wn.w1p, wbytes, wl_s, j, lane_t);
              warm[2 + j] = touch_share(NP == 8 ? (const void*)Wn.w2f8 : (const void*)Wn.w2p, wbytes, wl_s, j, lane_t);
            }
          } else if constexpr (QNP != 0) {
            warm[0] = QNP == 8 ? touch_share(a.qkv.wf8, (size_t)(3 * D / 32) * (D / 64) * kF8Rec * 16, wl_s, 0, lane_t)
                               : touch_share(a.qkv.wp, (size_t)3 * D * D * 2 * (QNP == 3 ? 2 : 1), wl_s, 0, lane_t);
          }
        }
#endif
        if (s >= 2) {
          const int cl = s - 2, c = phys(cl);  // slot chunk (picks the H buffer) / hidden chunk
          const char* h_lane = lds_h + (cl & 1) * 2 * kHPlane + (lane & 31) * kHLd + hh * 16;
          const int ks2 = min(kFC / 16, ks2_total - c * (kFC / 16));
          const uint4* w2_lane = W.w2p + ((size_t)(NT2 * wl) * ks2_total + c * (kFC / 16)) * 128 + lane;
          if constexpr (NP == 8) {  // the launcher guarantees F % 128 == 0 for this stream
            const char* h8_lane = lds_h + (cl & 1) * 2 * kHPlane + kHPlane + (lane & 31) * kH8Ld + hh * 32;
            if constexpr (NH == 1) {
              gemm_ring_f8<2, NTP, false, kPF2, NoSide, 0, kNW2, MT>(acc2c[0], h_lane, kHLd, h8_lane, kH8Ld, w2f8_lane(W, c), w2f8_nt, r2, wg2);
            } else {
#pragma unroll
              for (int h = 0; h < NH; ++h) {
                const uint4* next = h + 1 < NH ? w2f8_lane(W, c, h + 1) : (cl + 1 < nchunk ? w2f8_lane(W, phys(cl + 1), 0) : nullptr);
                gemm_ring_f8<2, NTP, false, kPF2, NoSide, 0, kNW2, MT, true>(acc2c[h], h_lane, kHLd, h8_lane, kH8Ld, w2f8_lane(W, c, h), w2f8_nt, r2, wg2, NoSide(), next);
              }
            }
          } else if (ks2 == kFC / 16) {
            gemm_ring<RNP, kFC / 16, NTP, false, kPF2, NoSide, 0, MT, !Q16, !Q16>(acc2c[0], h_lane, kHLd, kHPlane, w2_lane, w2_nt_stride, r2);
          } else {
            gemm_plain<RNP, NTP, false, MT, !Q16, !Q16>(acc2c[0], h_lane, kHLd, kHPlane, w2_lane, w2_nt_stride, ks2);
          }
          if (NH == 1 && cl + 1 < nchunk) fill2(W, phys(cl + 1));  // next chunk's W2 stream: in flight across the barrier
        }
        TL_STAMP();  // consumer: slot work done
        __syncthreads();
        TL_STAMP();  // consumer: barrier passed
      }
#if EEC_WARM_SLOTS > 0
      sink ^= warm[0] ^ warm[1] ^ warm[2] ^ warm[3];
#endif
    }
    // ---- stage epilogue ----
    // residual rows of this wave: issued now, consumed after the tile exchange below (for a second stage
    // they are the rows this very thread stored in the previous row pass)
    const int lane_e = fresh_lane(), w_e = w_s;  // see fresh_lane(): nothing index-like stays live across the chunk loops
    RowV<G::kQ> xr[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int row = row0 + w_e * RPW + i;
      xr[i] = zero_row<G::kQ>();
      if (TR != 2 && row < M) xr[i] = load_row<D>(x + (size_t)row * D, lane_e);
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr bool more = si + 1 < NS;
    // the consumers hold the [64, 256] result: stage it through the fp32 tile (the last barrier of the
    // loops guarantees that nobody still reads the H buffers it aliases)
    TL_STAMP();  // residual loads issued
    if constexpr (!producer) {
      if constexpr (Q16) {  // the chunk loops kept the accumulators in the quadrant layout: back to the standard one, once
#pragma unroll
        for (int h = 0; h < NH; ++h) accs_q_to_std<MT, NTP>(acc2c[h]);
      }
#pragma unroll
      for (int h = 0; h < NH; ++h)
        acc_to_etile<MT, NTP>(lds_e, G::kELd, acc2c[h], wl_s * 32 * NT2 + h * 32 * NTP, EEC_STAGE_FIELD(si, b2), lane_e);
    }
    TL_STAMP();  // exchange tile written
    // the next phase's weight streams start only now, when the accumulators are dead (issued earlier, their
    // registers push the allocator into spilling, and scratch reloads queue behind these cold loads); the
    // warm-up above has already brought this data into the XCD's L2
    if constexpr (more) {
      start_streams(wptrs(1));
    } else if constexpr (QNP != 0) {
      proj_fill<D, QNP, kLPF, NW>(rq, WMat{a.qkv.wp, a.qkv.wf8}, NW * w);
    }
    __syncthreads();
    TL_STAMP();  // barrier
    const float res_scale = EEC_STAGE_FIELD(si, res_scale);
    const float *fin_g = EEC_STAGE_FIELD(si, fin_g), *fin_b = EEC_STAGE_FIELD(si, fin_b);
    float* tap = EEC_STAGE_FIELD(si, tap);
    if constexpr (TR == 2) {
      if (a.tr.x_in) {
        // the module's LayerNorm backward in the same row pass (train_kernels.hip ln_bwd_kernel's arithmetic): with e = d(LN(x)),
        // xh = (x - mean) rstd, t = e gamma:  dx <- dx + rstd (t - mean_c(t) - xh mean_c(t xh)),  dgamma += e xh,  dbeta += e
        // (column sums over this workgroup's rows -> a.tr.ln_part[block][2][D], summed by the host's reduce launch)
        constexpr int Q = G::kQ;
        const RowV<Q> gam = load_row<D>(a.st[0].ln_g, lane_e);
        RowV<Q> e[RPW], xh[RPW], dres[RPW];
        float rsd[RPW], c1[RPW], c2[RPW];
        RowV<Q> dgs = zero_row<Q>(), dbs = zero_row<Q>();
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          const int rl = w_e * RPW + i, row = row0 + rl;
          const bool ok = row < M;
          const float mu = ok ? a.tr.mean[row] : 0.0f;
          rsd[i] = ok ? a.tr.rstd[row] : 0.0f;
          xh[i] = ok ? load_row<D>(a.tr.x_in + (size_t)row * D, lane_e) : zero_row<Q>();
          dres[i] = ok ? load_row<D>(x + (size_t)row * D, lane_e) : zero_row<Q>();
          c1[i] = 0.0f, c2[i] = 0.0f;
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            e[i].p[q] = *(const float4*)(lds_e + rl * G::kELd + (q * 256 + lane_e * 4) * 4);
            float4& h = xh[i].p[q];
            h.x = (h.x - mu) * rsd[i], h.y = (h.y - mu) * rsd[i], h.z = (h.z - mu) * rsd[i], h.w = (h.w - mu) * rsd[i];
            const float4 ev = e[i].p[q], gq = gam.p[q];
            const float tx = ev.x * gq.x, ty = ev.y * gq.y, tz = ev.z * gq.z, tw = ev.w * gq.w;
            c1[i] += tx + ty + tz + tw;
            c2[i] += tx * h.x + ty * h.y + tz * h.z + tw * h.w;
            dgs.p[q].x += ev.x * h.x, dgs.p[q].y += ev.y * h.y, dgs.p[q].z += ev.z * h.z, dgs.p[q].w += ev.w * h.w;
            dbs.p[q].x += ev.x, dbs.p[q].y += ev.y, dbs.p[q].z += ev.z, dbs.p[q].w += ev.w;
          }
        }
        wave_sum_n<RPW>(c1);
        wave_sum_n<RPW>(c2);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          const int row = row0 + w_e * RPW + i;
          const float m1 = c1[i] * (1.0f / D), m2 = c2[i] * (1.0f / D);
          RowV<Q> o;
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const float4 ev = e[i].p[q], gq = gam.p[q], h = xh[i].p[q], dr = dres[i].p[q];
            o.p[q].x = rsd[i] * (ev.x * gq.x - m1 - h.x * m2) + dr.x;
            o.p[q].y = rsd[i] * (ev.y * gq.y - m1 - h.y * m2) + dr.y;
            o.p[q].z = rsd[i] * (ev.z * gq.z - m1 - h.z * m2) + dr.z;
            o.p[q].w = rsd[i] * (ev.w * gq.w - m1 - h.w * m2) + dr.w;
          }
          if (row < M) store_row<D>(x + (size_t)row * D, o, lane_e);
        }
        // column sums of the tile: per wave in LDS (over the activation planes, dead since the chunk loops), then 2 D threads add the 8 waves
        float* red = (float*)smem;  // [8 waves][2][D]
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          *(float4*)(red + (w_e * 2 + 0) * D + q * 256 + lane_e * 4) = dgs.p[q];
          *(float4*)(red + (w_e * 2 + 1) * D + q * 256 + lane_e * 4) = dbs.p[q];
        }
        __syncthreads();
        for (int c = threadIdx.x; c < 2 * D; c += kFfnThreads) {
          float t = 0.0f;
#pragma unroll
          for (int ww = 0; ww < 8; ++ww) t += red[ww * 2 * D + c];
          a.tr.ln_part[(size_t)blockIdx.x * 2 * D + c] = t;
        }
      } else {  // d(LN(x)) rows, as they are
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          const int row = row0 + w_e * RPW + i;
          RowV<G::kQ> v;
#pragma unroll
          for (int q = 0; q < G::kQ; ++q) v.p[q] = *(const float4*)(lds_e + (w_e * RPW + i) * G::kELd + (q * 256 + lane_e * 4) * 4);
          if (row < M) store_row<D>(a.tr.y + (size_t)row * D, v, lane_e);
        }
      }
    } else if constexpr (TR == 1) {
      // y = x + res_scale * drop(W2 . h + b2): the row pass with the output dropout of the module, rows to a.tr.y
      const eect::DropState ds_res(eect::Drop{a.tr.p, a.tr.seed, a.tr.site_res});
      RowV<G::kQ> v[RPW];
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int row = row0 + w_e * RPW + i;
        v[i] = xr[i];
#pragma unroll
        for (int q = 0; q < G::kQ; ++q) {
          const float4 e = *(const float4*)(lds_e + (w_e * RPW + i) * G::kELd + (q * 256 + lane_e * 4) * 4);
          float m[4];
          ds_res.mul4((size_t)row * D + q * 256 + lane_e * 4, m);
          v[i].p[q].x += res_scale * m[0] * e.x;
          v[i].p[q].y += res_scale * m[1] * e.y;
          v[i].p[q].z += res_scale * m[2] * e.z;
          v[i].p[q].w += res_scale * m[3] * e.w;
        }
        if (row < M) store_row<D>(a.tr.y + (size_t)row * D, v[i], lane_e);
      }
      if (a.tr.ln2) {  // the LayerNorm that reads these rows next (the attention module's, or the layer's final one): rows and statistics
        float mu[RPW], rs[RPW];
        layer_norm_rows<D, RPW>(v, load_row<D>(a.tr.ln2_g, lane_e), load_row<D>(a.tr.ln2_b, lane_e), mu, rs);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
          const int row = row0 + w_e * RPW + i;
          if (row < M) {
            store_row<D>(a.tr.ln2 + (size_t)row * D, v[i], lane_e);
            if (lane_e == 0) a.tr.mean2[row] = mu[i], a.tr.rstd2[row] = rs[i];
          }
        }
      }
    } else if constexpr (more) {  // only stage 0 can have a successor
      chain_rowpass<D, NP, true>(smem, lds_e, x, xr, row0, M, res_scale, fin_g, fin_b, tap, a.st[1].ln_g, a.st[1].ln_b, lane_e, w_e);
    } else if constexpr (QNP != 0) {
      chain_rowpass<D, QNP, true>(smem, lds_e, x, xr, row0, M, res_scale, fin_g, fin_b, tap, a.qkv.ln_g, a.qkv.ln_b, lane_e, w_e);
    } else {
      chain_rowpass<D, 0, true>(smem, lds_e, x, xr, row0, M, res_scale, fin_g, fin_b, tap, nullptr, nullptr, lane_e, w_e);
    }
    TL_STAMP();  // row pass done
    if (more || QNP != 0) __syncthreads();  // next planes complete; the exchange tile is free again
    TL_STAMP();  // stage epilogue + row pass done
  });
  // (the H buffers are dead by now: 8 x 5 KB of them stage the tail's whole-line Q / K / V^T stores)
  static_assert(QNP == 0 || 8 * kQkvStageBytes <= 4 * FG::kHPlane || D != 256, "qkv staging fits the H buffers");
  if constexpr (QNP != 0) qkv_body<D, QNP>(smem, a.qkv, row0, rq, D == 256 ? lds_h : nullptr);
  if ((sink ^ sink_front) == 0x9e3779b9u && M == -7) x[0] = 0.f;  // never true: the warm-up loads must not be optimised away
  TL_STAMP();  // last: epilogue done
  };
  if (is_producer)
    run(BoolTag<true>{});
  else
    run(BoolTag<false>{});
}

#if defined(EEC_TIMELINE) && (!defined(EEC_FFN_D) || EEC_FFN_D == 256)
extern "C" int eec_debug_timeline(unsigned long long* host_out, int n) {
  static unsigned long long* dev = nullptr;
  if (!dev) {
    if (hipMalloc(&dev, 8 * 2 * 128 * 8) != hipSuccess) return 1;
    (void)hipMemset(dev, 0, 8 * 2 * 128 * 8);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &dev, sizeof(dev));
    return 0;
  }
  (void)hipDeviceSynchronize();
  return (int)hipMemcpy(host_out, dev, (size_t)n * 8, hipMemcpyDeviceToHost);
}
#endif

template <int D, int NP, int ACT, int FNP, int QNP, int NS, int TR = 0>
static hipError_t launch_chain_t(const ChainArgs& a, hipStream_t st) {
  auto k = ffn_chain_kernel<D, NP, ACT, FNP, QNP, NS, TR>;
  constexpr int lds = FNP != 0 ? (DwGeo<D>::kLds > FfnGeo<D>::kLds ? DwGeo<D>::kLds : FfnGeo<D>::kLds) : FfnGeo<D>::kLds;
  if (hipError_t e = ensure_max_lds((const void*)k, lds); e != hipSuccess) return e;
  const int grid = (a.M + Geo<D>::kRows - 1) / Geo<D>::kRows;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kFfnThreads), lds, st, a);
  return hipGetLastError();
}

#if defined(EEC_FFN_TRAIN_BWD)
// Fourth object of this source (build/ffn_train_bwd.o, bf16 operands): the training step's backward variants.
hipError_t launch_ffn_train_bwd(const ChainArgs& a, int np, hipStream_t st) {
  if (a.nstage != 1 || a.F < 32 || a.F % 32 != 0 || (np != 1 && np != 3)) return hipErrorInvalidValue;
  if (!a.tr.pre || !a.tr.act || !a.tr.ln) return hipErrorInvalidValue;
  if (a.tr.x_in ? (!a.tr.mean || !a.tr.rstd || !a.tr.ln_part || !a.st[0].ln_g) : !a.tr.y) return hipErrorInvalidValue;
  if (a.tr.pl_x && (!a.tr.pl_mean || !a.tr.pl_rstd || !a.tr.pl_g || !a.tr.pl_part)) return hipErrorInvalidValue;
  if (a.D == 256) return np == 3 ? launch_chain_t<256, 3, 2, 0, 0, 1, 2>(a, st) : launch_chain_t<256, 1, 2, 0, 0, 1, 2>(a, st);
  if (a.D == 512) return np == 3 ? launch_chain_t<512, 3, 2, 0, 0, 1, 2>(a, st) : launch_chain_t<512, 1, 2, 0, 0, 1, 2>(a, st);
  return hipErrorInvalidValue;
}
}  // namespace eec
#elif defined(EEC_FFN_TRAIN)
// Third object of this source (build/ffn_train.o): only the training step's forward variants.
hipError_t launch_ffn_train_fwd(const ChainArgs& a, int np, hipStream_t st) {
  if (a.nstage != 1 || a.F < 32 || a.F % 32 != 0 || (np != 1 && np != 3)) return hipErrorInvalidValue;
  if (!a.tr.y || !a.tr.ln || !a.tr.mean || !a.tr.rstd || !a.tr.pre || !a.tr.act) return hipErrorInvalidValue;
  if (a.D == 256) return np == 3 ? launch_chain_t<256, 3, 2, 0, 0, 1, 1>(a, st) : launch_chain_t<256, 1, 2, 0, 0, 1, 1>(a, st);
  if (a.D == 512) return np == 3 ? launch_chain_t<512, 3, 2, 0, 0, 1, 1>(a, st) : launch_chain_t<512, 1, 2, 0, 0, 1, 1>(a, st);
  return hipErrorInvalidValue;
}
}  // namespace eec
#else
// This file is compiled once per d_model (-DEEC_FFN_D=256 / 512: two objects, so the two sets of chain-kernel variants
// build in parallel); each object defines launch_ffn_chain_d<EEC_FFN_D>, the D = 256 object also the dispatchers.
#ifndef EEC_FFN_D
#define EEC_FFN_D 256
#endif
template <int D>
hipError_t launch_ffn_chain_d(const ChainArgs& a_in, int np, int np_front, int np_tail, bool front, bool tail, bool relu, hipStream_t st);

// np: FFN format (1, 3, 8); np_o: format of the optional front / tail (1 or 3)
template <>
hipError_t launch_ffn_chain_d<EEC_FFN_D>(const ChainArgs& a_in, int np, int np_front, int np_tail, bool front, bool tail, bool relu, hipStream_t st) {
  constexpr int D = EEC_FFN_D;
  ChainArgs a = a_in;
  if (a.nstage < 1 || a.nstage > 2) return hipErrorInvalidValue;
  for (int i = 0; i < a.nstage; ++i)
    if (np == 8 && (a.F % kFC != 0 || !a.st[i].w1f8 || !a.st[i].w2f8)) np = 3;  // the f8 stream needs whole 128-wide chunks
#ifndef EEC_CHAIN_MINIMAL
  if (relu) {
    if (front || tail || a.nstage != 1) return hipErrorInvalidValue;
    if (np == 8) return launch_chain_t<D, 8, 1, 0, 0, 1>(a, st);
    if (np == 3) return launch_chain_t<D, 3, 1, 0, 0, 1>(a, st);
    return launch_chain_t<D, 1, 1, 0, 0, 1>(a, st);
  }
#endif
  const int f = front ? np_front : 0, q = tail ? np_tail : 0;
#ifdef EEC_CHAIN_MINIMAL  // tuning builds: only the three launches of the production plan in the default (f16x3) and the f16f8 mode
  if (np == 3 && f == 0 && q == 3 && a.nstage == 1) return launch_chain_t<D, 3, 0, 0, 3, 1>(a, st);
  if (np == 3 && f == 3 && q == 3 && a.nstage == 2) return launch_chain_t<D, 3, 0, 3, 3, 2>(a, st);
  if (np == 3 && f == 3 && q == 0 && a.nstage == 1) return launch_chain_t<D, 3, 0, 3, 0, 1>(a, st);
#ifdef EEC_CHAIN_MINIMAL_F8
  if (np == 8 && f == 0 && q == 8 && a.nstage == 1) return launch_chain_t<D, 8, 0, 0, 8, 1>(a, st);
  if (np == 8 && f == 8 && q == 8 && a.nstage == 2) return launch_chain_t<D, 8, 0, 8, 8, 2>(a, st);
  if (np == 8 && f == 8 && q == 0 && a.nstage == 1) return launch_chain_t<D, 8, 0, 8, 0, 1>(a, st);
#endif
  return hipErrorInvalidValue;
#else
#define EEC_CHAIN_CASE(NP_, F_, Q_)                                                                      \
  if (np == NP_ && f == F_ && q == Q_)                                                                   \
    return a.nstage == 2 ? launch_chain_t<D, NP_, 0, F_, Q_, 2>(a, st) : launch_chain_t<D, NP_, 0, F_, Q_, 1>(a, st);
  if constexpr (D == 256) {  // f16f8 at d_model 256: conv front and in_proj tail on the f8 stream too
    EEC_CHAIN_CASE(8, 0, 0) EEC_CHAIN_CASE(8, 8, 0) EEC_CHAIN_CASE(8, 0, 8) EEC_CHAIN_CASE(8, 8, 8)
  } else {  // ... at d_model 512 they keep the fragment formats
    EEC_CHAIN_CASE(8, 0, 0) EEC_CHAIN_CASE(8, 3, 0) EEC_CHAIN_CASE(8, 0, 3) EEC_CHAIN_CASE(8, 3, 3)
  }
  EEC_CHAIN_CASE(3, 0, 0) EEC_CHAIN_CASE(3, 3, 0) EEC_CHAIN_CASE(3, 0, 3) EEC_CHAIN_CASE(3, 3, 3)
  EEC_CHAIN_CASE(1, 0, 0) EEC_CHAIN_CASE(1, 3, 0) EEC_CHAIN_CASE(1, 0, 3) EEC_CHAIN_CASE(1, 3, 3)
  EEC_CHAIN_CASE(1, 1, 0) EEC_CHAIN_CASE(1, 0, 1) EEC_CHAIN_CASE(1, 1, 1)
#undef EEC_CHAIN_CASE
  return hipErrorInvalidValue;
#endif
}

#if EEC_FFN_D == 256
template <>
hipError_t launch_ffn_chain_d<512>(const ChainArgs& a_in, int np, int np_front, int np_tail, bool front, bool tail, bool relu, hipStream_t st);  // ffn512.o

hipError_t launch_ffn_chain(const ChainArgs& a, int np, int np_front, int np_tail, bool front, bool tail, bool relu, hipStream_t st) {
  if (a.D == 512) return launch_ffn_chain_d<512>(a, np, np_front, np_tail, front, tail, relu, st);
  if (a.D == 256) return launch_ffn_chain_d<256>(a, np, np_front, np_tail, front, tail, relu, st);
  return hipErrorInvalidValue;
}

// single stand-alone stage (the unfused plan and the legacy encoder)
hipError_t launch_ffn(const FfnArgs& f, int np, hipStream_t st) {
  ChainArgs a{};
  a.x = f.x, a.M = f.M, a.F = f.F, a.D = f.D, a.nstage = 1;
  a.st[0] = FfnStage{f.ln_g, f.ln_b, f.w1p, f.b1, f.w2p, f.b2, f.fin_g, f.fin_b, f.w1f8, f.w2f8, f.res_scale, nullptr};
  return launch_ffn_chain(a, np, 3, 3, false, false, f.relu, st);
}
#endif

}  // namespace eec
#endif  // EEC_FFN_TRAIN
