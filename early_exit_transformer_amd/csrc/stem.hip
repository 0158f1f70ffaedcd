// Conv1dSubampling + positional encoding (reference early_exit.py:24-48,620-621):
// two Conv1d(k=3, stride=2, pad=0) back to back (no activation between), transpose to
// [utterance][frame][channel], + sinusoid PE.  Two linear maps with nothing between them are one: a
// Conv1d(n_mels -> D, k=7, stride=4, pad=0) whose weights W_eff / b_eff are composed once, in fp64, when the model is packed
// (pack.hip, launch_stem_fold).  The stem is ONE launch, an MFMA GEMM on hi/lo-split fp16 operands with no intermediate tensor:
//   rows = (b, t'), K = 7 * n_mels as seven K = n_mels passes k = 0..6,
//   A_k[row][ci] = mel[b][ci][4 t' + k]   (4 R + 3 staged mel frames per R-row tile, lane row stride 4 frames)
// The input is un-logged power mel (util/data_loader.py:7-18: heavy-tailed, no upper bound, 5+ decades between the loud
// and the quiet frames of one utterance).  fp16 operands need a bounded domain, so every staged mel FRAME gets its own
// power-of-two scale (exact): the frame is multiplied by 2^-e, e = exponent(max over channels) - 15, and split into hi/lo
// planes; the accumulators (lane = output frame) sit in the domain of the frame of the running pass and move to the next
// frame's domain by 2^(e_k - e_(k+1)) between the passes.  One outlier bin or one loud frame therefore costs no other frame
// its precision, nothing saturates up to fp32's own range, and an utterance's result does not depend on its batch position.
// The one-convolution stem of Early_zipformer keeps a kernel of its own (stem_conv1_kernel, a row = one 3-frame window).
#include "eec_kernels.h"
#include <algorithm>

#include "eec_blocks.h"

namespace eec {

constexpr int kStemThreads = 512;
constexpr int kStemRows1 = 64;  // conv1 row tile: (utterance, frame) rows of the half-rate sequence
constexpr int kSPF = 4;

// exponent e such that |m| * 2^-e < 2^15 (m = a row's maximum magnitude); 0 for an all-zero / non-finite row
__device__ __forceinline__ int row_exponent(float m) {
  if (!(m > 0.f) || !(m < INFINITY)) return 0;
  int ex;
  (void)frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
  return ex - 15;
}

// ---------------------------------------------------------------------------
// The one-convolution stem of Early_zipformer (Conv1dSubampling_Zipformer, early_exit.py:80-95):
// x[b][t1][:] = conv + bias + pe[t1].  rows = (b, t1), K1 = n_mels * 3 in the weight tensor's own [ci][j] order
// (multiple of 16, <= 384), A[row][3ci + j] = mel[b][ci][2 t1 + j]; plane row stride (K1 + 8) halves.  A row (the 3-frame
// window of one half-rate frame) is multiplied by 2^-e, e = exponent(max |window|) - 15, and its accumulators by 2^e.
template <int D, int NP>
__global__ __launch_bounds__(kStemThreads, 2) void stem_conv1_kernel(SubsampleArgs a) {
  constexpr int NW = Geo<D>::kNW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), w = wave_id(), hh = lane >> 5;
  const int K1 = a.n_mels * 3, ks = K1 / 16;
  const int ld = (K1 + 8) * 2, plane = kStemRows1 * ld;
  const int M1 = a.B * a.T1;
  const int row0 = blockIdx.x * kStemRows1;

  WRing<NP, kSPF, NW> r;
  const uint4* w_lane = a.w1p + (size_t)(NW * w) * ks * 128 + lane;
  const size_t nts = (size_t)ks * 128;
  ring_fill_32<NP, kSPF, NW>(r, w_lane, nts, ks);  // consumed by gemm_plain_ring (32x32x16 fragments)
  unsigned* row_max = (unsigned*)(smem + 2 * plane);  // [64] input rows: |max| as fp32 bit patterns
  if (threadIdx.x < kStemRows1) row_max[threadIdx.x] = 0u;
  // stage A: thread = (row rr, channel group cg); 3 taps per (row, ci); the row's scale comes from its own maximum
  {
    const int rr = threadIdx.x & 63, cg = threadIdx.x >> 6;
    const int row = row0 + rr;
    const bool ok = row < M1;
    const int b = ok ? row / a.T1 : 0, t1 = ok ? row - b * a.T1 : 0;
    const float* src = a.mel + (size_t)b * a.n_mels * a.T + 2 * t1;
    constexpr int CI = 16;  // channels per thread: n_mels <= 128
    float v[CI][3];
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < CI; ++i) {
      const int ci = cg + 8 * i;
      v[i][0] = v[i][1] = v[i][2] = 0.f;
      if (ok && ci < a.n_mels) {
        const float* p = src + (size_t)ci * a.T;
        v[i][0] = p[0], v[i][1] = p[1], v[i][2] = p[2];
      }
      m = fmaxf(m, fmaxf(fabsf(v[i][0]), fmaxf(fabsf(v[i][1]), fabsf(v[i][2]))));
    }
    __syncthreads();  // row_max zeroed
    atomicMax(&row_max[rr], __builtin_bit_cast(unsigned, m));  // non-negative floats order like their bit patterns
    __syncthreads();
    const float sc = ldexpf(1.0f, -row_exponent(__builtin_bit_cast(float, row_max[rr])));
#pragma unroll
    for (int i = 0; i < CI; ++i) {
      const int ci = cg + 8 * i;
      if (ci < a.n_mels) {
        const hl2_t s01 = split2<NP>(v[i][0] * sc, v[i][1] * sc), s2 = split2<NP>(v[i][2] * sc, 0.f);
        half_t* dh = (half_t*)(smem + rr * ld) + ci * 3;
        dh[0] = s01.hi[0], dh[1] = s01.hi[1], dh[2] = s2.hi[0];
        if (NP == 3) {
          half_t* dl = (half_t*)(smem + plane + rr * ld) + ci * 3;
          dl[0] = s01.lo[0], dl[1] = s01.lo[1], dl[2] = s2.lo[0];
        }
      }
    }
  }
  __syncthreads();
  // this lane's two rows and the exponents of their scaled input domains
  int rowl[2], el[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    rowl[mt] = row0 + mt * 32 + (lane & 31);
    el[mt] = row_exponent(__builtin_bit_cast(float, row_max[mt * 32 + (lane & 31)]));
  }
  f32x16 acc[2][NW];
  // accumulators start at bias * 2^-e (the row's scaled domain)
#pragma unroll
  for (int nt = 0; nt < NW; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bb = *(const float4*)(a.b1 + 32 * (NW * w + nt) + 8 * g + 4 * hh);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const float sc = ldexpf(1.0f, -el[mt]);
        acc[mt][nt][4 * g + 0] = bb.x * sc;
        acc[mt][nt][4 * g + 1] = bb.y * sc;
        acc[mt][nt][4 * g + 2] = bb.z * sc;
        acc[mt][nt][4 * g + 3] = bb.w * sc;
      }
    }
  const char* a_lane = smem + (lane & 31) * ld + hh * 16;
  gemm_plain_ring<NP, kSPF, NW>(acc, a_lane, ld, plane, w_lane, nts, ks, r);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int row = rowl[mt];
    if (row < M1) {
      const int t1 = row % a.T1;
      const float up = ldexpf(1.0f, el[mt]);
#pragma unroll
      for (int nt = 0; nt < NW; ++nt) {
        const int c0 = 32 * (NW * w + nt) + 4 * hh;
        float* dst = a.x + (size_t)row * D + c0;
        const float* pe = a.pe + (size_t)t1 * D + c0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 p = *(const float4*)(pe + 8 * g);
          *(float4*)(dst + 8 * g) = make_float4(acc[mt][nt][4 * g + 0] * up + p.x, acc[mt][nt][4 * g + 1] * up + p.y,
                                                acc[mt][nt][4 * g + 2] * up + p.z, acc[mt][nt][4 * g + 3] * up + p.w);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The folded two-convolution stem + PE.  One workgroup = Geo<D>::kRows consecutive output frames of one utterance.
//
// Staged image.  Output row r of a tile reads mel frames 4 r + k, k = 0..6: in a plain [frame][n_mels] image the lane row
// stride would be four frames, and with 16-byte-aligned frames (ds_read_b128 off its alignment is replayed) four frames are a
// multiple of 64 B -- the 16 lanes that share an LDS cycle would land on 4 of the 16 sixteen-byte slots of the bank row, a
// 4-way conflict.  So the image is split by frame phase: frame f lies at [f & 3][f >> 2][n_mels].  Pass k then reads phase
// k & 3 at index r + (k >> 2): the lane row stride is ONE frame, ld = 2 n_mels + 16 bytes = an odd number of slots
// (n_mels % 16 == 0), which is conflict-free for the same reason Geo<D>::kALd is.
template <int D>
struct StemGeo {
  static constexpr int kR = Geo<D>::kRows;
  static constexpr int kFrames = 4 * kR + 3;                   // 259 / 131 staged mel frames
  static constexpr int kNQ = kR + 1;                           // frames per phase
  static constexpr int kChunk = 128;                           // frames staged per sweep: thread = (frame, 1 of 4 channel groups)
  static constexpr int kNCh = (kFrames + kChunk - 1) / kChunk;  // 3 / 2
  static constexpr int kAux = 4 * kNQ * 4 + kNCh * 4 * kChunk * 4;  // frame exponents, partial maxima (behind the planes)
  static constexpr int kOut = kR * (D * 4 + 16);               // the fp32 tile that leaves through LDS
  __host__ __device__ static constexpr int ld(int n_mels) { return n_mels * 2 + 16; }
  __host__ __device__ static constexpr int plane(int n_mels) { return 4 * kNQ * ld(n_mels); }
  // 80 mels: 92560 (planes) + aux; 128 mels: 141440 + aux; 16 mels: the output tile (66560) sets the size
  __host__ __device__ static constexpr int lds(int n_mels) { return 2 * plane(n_mels) + kAux > kOut ? 2 * plane(n_mels) + kAux : kOut; }
};
// A frame's exponent is kept above this: the accumulators of a pass hold (true partial sum) * 2^(kStemWShift - e), and a loud
// frame's partial sum must still fit fp32 in the domain of a (nearly) silent neighbour.  Frames whose maximum is below
// 2^(kStemMinExp + 1) ~ 1.6e-24 keep less than the full hi/lo precision.
constexpr int kStemMinExp = -80;

template <int D, int NP>
__global__ __launch_bounds__(kStemThreads, 2) void stem_fold_kernel(SubsampleArgs a) {
  using G = Geo<D>;
  using S = StemGeo<D>;
  constexpr int MT = G::kMT, NW = G::kNW;
  constexpr int LO = (NP == 3) ? 1 : 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), w = wave_id(), hh = lane >> 5;
  const int b = blockIdx.y, t0 = blockIdx.x * G::kRows;
  const int ks1 = a.n_mels >> 4, ks_total = 7 * ks1;  // k-steps per pass / per n-tile, ordered (k, ci)
  const int ld = S::ld(a.n_mels), plane = S::plane(a.n_mels);
  const size_t nts = (size_t)ks_total * 128;
  WRing<NP, kSPF, NW> r;
  const uint4* w_lane = a.wfp + (size_t)(NW * w) * ks_total * 128 + lane;
  ring_fill_32<NP, kSPF, NW>(r, w_lane, nts, ks_total);
  int* const fe = (int*)(smem + 2 * plane);      // [4 kNQ]: exponent of every staged frame's domain
  float* const pm = (float*)(fe + 4 * S::kNQ);   // [kNCh][4][kChunk]: a channel group's maximum of a frame
  // Stage mel frames 4 t0 .. 4 t0 + 4 R + 2 of utterance b.  thread = (frame fl of a 128-frame chunk, channel group cg);
  // a thread holds quads of consecutive channels (quad cg + 4 i), a wave reads 64 consecutive frames of one channel.
  // Frames behind the last one that a valid output row uses (4 T' + 3 <= T) are zero and are not read.
  {
    const int fl = threadIdx.x & (S::kChunk - 1), cg = threadIdx.x >> 7;
    const int nquad = a.n_mels >> 2, f_end = 4 * a.Tq + 3;
    const float* src = a.mel + (size_t)b * a.n_mels * a.T + 4 * t0;
    constexpr int QI = 8;  // quads per thread: n_mels <= 128
    float v[2][QI][4];
    auto load = [&](int c, float(&d)[QI][4]) {
      const int f = c * S::kChunk + fl;
      const bool ok = f < S::kFrames && 4 * t0 + f < f_end;
#pragma unroll
      for (int i = 0; i < QI; ++i)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          d[i][cc] = 0.f;
          if (ok && cg + 4 * i < nquad) d[i][cc] = src[(size_t)(4 * (cg + 4 * i) + cc) * a.T + f];
        }
    };
    load(0, v[0]);
#pragma unroll
    for (int c = 0; c < S::kNCh; ++c) {
      float(&cur)[QI][4] = v[c & 1];
      if (c + 1 < S::kNCh) load(c + 1, v[(c + 1) & 1]);  // the next chunk's loads fly during this chunk's reduction
      const int f = c * S::kChunk + fl;
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < QI; ++i) m = fmaxf(m, fmaxf(fmaxf(fabsf(cur[i][0]), fabsf(cur[i][1])), fmaxf(fabsf(cur[i][2]), fabsf(cur[i][3]))));
      pm[(c * 4 + cg) * S::kChunk + fl] = m;
      __syncthreads();
      m = fmaxf(fmaxf(pm[(c * 4 + 0) * S::kChunk + fl], pm[(c * 4 + 1) * S::kChunk + fl]),
                fmaxf(pm[(c * 4 + 2) * S::kChunk + fl], pm[(c * 4 + 3) * S::kChunk + fl]));
      const int e = max(row_exponent(m), kStemMinExp);
      if (f < 4 * S::kNQ) {
        if (cg == 0) fe[f] = e;
        char* const dst = smem + ((f & 3) * S::kNQ + (f >> 2)) * ld;
#pragma unroll
        for (int i = 0; i < QI; ++i)
          if (cg + 4 * i < nquad) {
            const hl2_t s0 = split2<NP>(ldexpf(cur[i][0], -e), ldexpf(cur[i][1], -e));
            const hl2_t s1 = split2<NP>(ldexpf(cur[i][2], -e), ldexpf(cur[i][3], -e));
            h4 hi, lo;
            hi.xy = s0.hi, hi.zw = s1.hi, lo.xy = s0.lo, lo.zw = s1.lo;
            *(h4*)(dst + (cg + 4 * i) * 8) = hi;
            if (NP == 3) *(h4*)(dst + plane + (cg + 4 * i) * 8) = lo;
          }
      }
    }
  }
  __syncthreads();
  // the accumulators start at b_eff in the domain of the row's first frame (the packed weights carry 2^kStemWShift)
  const int* const fe_lane = fe + 4 * (lane & 31);  // frame 4 r + k of row tile mt: fe_lane[128 mt + k]
  f32x16 acc[MT][NW];
#pragma unroll
  for (int nt = 0; nt < NW; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bb = *(const float4*)(a.bf + 32 * (NW * w + nt) + 8 * g + 4 * hh);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int sh = kStemWShift - fe_lane[128 * mt];
        acc[mt][nt][4 * g + 0] = ldexpf(bb.x, sh);
        acc[mt][nt][4 * g + 1] = ldexpf(bb.y, sh);
        acc[mt][nt][4 * g + 2] = ldexpf(bb.z, sh);
        acc[mt][nt][4 * g + 3] = ldexpf(bb.w, sh);
      }
    }
  // Seven passes as ONE ring-pipelined k-loop (32x32x16 fragments, runtime k-step count, swapped orientation: frames on lanes):
  // the weight ring and the one-step-ahead reads of the activation fragments run across the pass boundaries, where the
  // accumulators move into the next frame's domain (exact: powers of two; the clamp keeps the shift inside ldexp's exact range).
  {
    const char* const a_base = smem + (lane & 31) * ld + hh * 16;
    int k = 0, sl = 0;  // pass and k-step inside it (wave-uniform)
    h8 ah[MT], al[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ah[mt] = *(const h8*)(a_base + mt * 32 * ld);
      al[mt] = ah[mt];
      if (NP == 3) al[mt] = *(const h8*)(a_base + plane + mt * 32 * ld);
    }
    for (int s0 = 0; s0 < ks_total; s0 += kSPF) {
#pragma unroll
      for (int p = 0; p < kSPF; ++p) {
        const int s = s0 + p;
        if (s < ks_total) {
          int k2 = k, sl2 = sl + 1;
          if (sl2 == ks1) sl2 = 0, ++k2;
          h8 nh[MT], nl[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) nh[mt] = ah[mt], nl[mt] = al[mt];
          if (s + 1 < ks_total) {
            const char* an = a_base + ((k2 & 3) * S::kNQ + (k2 >> 2)) * ld + sl2 * 32;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              nh[mt] = *(const h8*)(an + mt * 32 * ld);
              if (NP == 3) nl[mt] = *(const h8*)(an + plane + mt * 32 * ld);
            }
          }
          __builtin_amdgcn_sched_barrier(0);  // issue the next step's LDS reads BEFORE this step's MFMAs
          if (sl == 0 && k > 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const int d = max(-120, min(120, fe_lane[128 * mt + k - 1] - fe_lane[128 * mt + k]));
#pragma unroll
              for (int nt = 0; nt < NW; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][nt][i] = ldexpf(acc[mt][nt][i], d);
            }
          }
#pragma unroll
          for (int nt = 0; nt < NW; ++nt) {
            const h8 bh = __builtin_bit_cast(h8, r.q[p][nt][0]);
            const h8 bl = __builtin_bit_cast(h8, r.q[p][nt][LO]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              if (NP == 3) {
                acc[mt][nt] = mfma16(bh, al[mt], acc[mt][nt]);
                acc[mt][nt] = mfma16(bl, ah[mt], acc[mt][nt]);
              }
              acc[mt][nt] = mfma16(bh, ah[mt], acc[mt][nt]);
            }
            if (s + kSPF < ks_total) {
              r.q[p][nt][0] = w_lane[nt * nts + (size_t)(s + kSPF) * 128];
              if (NP == 3) r.q[p][nt][LO] = w_lane[nt * nts + (size_t)(s + kSPF) * 128 + 64];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) ah[mt] = nh[mt], al[mt] = nl[mt];
          k = k2, sl = sl2;
        }
      }
    }
  }
  // The fp32 tile leaves through LDS (the staged frames are dead once every wave is past its seven passes): a wave then adds the
  // positional encoding to, and stores, whole rows (1 KiB per instruction) -- from the accumulators a store instruction and a load of
  // the encoding are 32 rows x 32 B each.  The tile may cover the frame exponents: the last frame's is read before the barrier.
  constexpr int kSLd2 = D * 4 + 16;
  int up[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) up[mt] = fe_lane[128 * mt + 6] - kStemWShift;
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int nt = 0; nt < NW; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(float4*)(smem + (mt * 32 + (lane & 31)) * kSLd2 + (32 * (NW * w + nt) + 8 * g + 4 * hh) * 4) =
            make_float4(ldexpf(acc[mt][nt][4 * g + 0], up[mt]), ldexpf(acc[mt][nt][4 * g + 1], up[mt]),
                        ldexpf(acc[mt][nt][4 * g + 2], up[mt]), ldexpf(acc[mt][nt][4 * g + 3], up[mt]));
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < G::kRPW; ++i) {
    const int rl = w * G::kRPW + i, t = t0 + rl;
    if (t < a.Tq) {
      RowV<G::kQ> v = load_row<D>((const float*)(smem + rl * kSLd2), lane);
      const RowV<G::kQ> p = load_row<D>(a.pe + (size_t)t * D, lane);
#pragma unroll
      for (int q = 0; q < G::kQ; ++q) v.p[q].x += p.p[q].x, v.p[q].y += p.p[q].y, v.p[q].z += p.p[q].z, v.p[q].w += p.p[q].w;
      store_row<D>(a.x + ((size_t)b * a.Tq + t) * D, v, lane);
    }
  }
}

template <int D>
static hipError_t launch_subsample_d(const SubsampleArgs& a, int np, hipStream_t st) {
  auto kf = np == 3 ? stem_fold_kernel<D, 3> : stem_fold_kernel<D, 1>;
  if (hipError_t e = ensure_max_lds((const void*)kf, StemGeo<D>::lds(128)); e != hipSuccess) return e;
  hipLaunchKernelGGL(kf, dim3((a.Tq + Geo<D>::kRows - 1) / Geo<D>::kRows, a.B), dim3(kStemThreads), StemGeo<D>::lds(a.n_mels), st, a);
  return hipGetLastError();
}
hipError_t launch_subsample(const SubsampleArgs& a, int np, hipStream_t st) {
  if (a.n_mels % 16 || a.n_mels > 128 || !a.wfp || !a.bf) return hipErrorInvalidValue;
  return a.D == 512 ? launch_subsample_d<512>(a, np, st) : launch_subsample_d<256>(a, np, st);
}

// one Conv1d(k=3, s=2) + PE: x [B][T1][D] fp32 (the Early_zipformer stem); hi/lo split operands
template <int D>
static hipError_t launch_subsample_single_d(const SubsampleArgs& a, hipStream_t st) {
  const int K1 = a.n_mels * 3;
  auto k1 = stem_conv1_kernel<D, 3>;
  if (hipError_t e = ensure_max_lds((const void*)k1, 2 * kStemRows1 * (384 + 8) * 2 + kStemRows1 * 4); e != hipSuccess) return e;
  const int M1 = a.B * a.T1;
  hipLaunchKernelGGL(k1, dim3((M1 + kStemRows1 - 1) / kStemRows1), dim3(kStemThreads), 2 * kStemRows1 * (K1 + 8) * 2 + kStemRows1 * 4, st, a);
  return hipGetLastError();
}
hipError_t launch_subsample_single(const SubsampleArgs& a, hipStream_t st) {
  const int K1 = a.n_mels * 3;
  if (K1 % 16 || K1 > 384) return hipErrorInvalidValue;
  return a.D == 512 ? launch_subsample_single_d<512>(a, st) : launch_subsample_single_d<256>(a, st);
}

}  // namespace eec
