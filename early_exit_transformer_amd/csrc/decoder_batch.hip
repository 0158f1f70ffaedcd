// Step-wise AED decoding of a whole batch: every exit and every utterance of a padded batch advanced by the same launches
// (include/eec.h, eec_decoder_batch_begin / eec_decoder_batch_step).  Same arithmetic as eec_decoder_step_multi
// (decoder_step.hip): norm_first nn.TransformerDecoderLayer in eval mode, causal + target-padding key mask over each beam's
// ancestry, the shared final LayerNorm, the exit Linear and log_softmax.  What differs is the shape of a step: one exit's
// decoder sees B utterances x R beams = B * R rows that share one set of weights, so every linear is a small GEMM over those
// rows (a weight tile is read once per 64-row tile, not once per utterance), with the exit as a grid dimension.
//
// Launches per step do not depend on B or E: embed, then per decoder layer
//   batch_linear (LN1 -> in_proj)  batch_self_attn   batch_linear (out_proj, += x)
//   batch_linear (LN2 -> q)        batch_cross_attn  batch_linear (out_proj, += x)
//   batch_linear (LN3 -> linear1 -> ReLU)            batch_linear (linear2, += x)
// then batch_linear (final LN -> head) and the log_softmax.  The beam bookkeeping is eec_beam_select with n = E * B groups.
//
// One cache for all of them: the layout of eec_decoder_step.h (carve()) with u = e * B + b the (exit, utterance) index; the
// memory keys | values are projected by _begin with one training GEMM per (exit, layer).
#include "eec_decoder_step.h"

using namespace eec;  // eec_wave.h
using namespace eect;
using namespace eecs;

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Y[e][m][n] (+)= act( LN_e?(X[e][m]) . W_e[n] + bias_e[n] ),  m < M = B * R, on v_mfma_f32_32x32x16_f16 with f16x3 operands:
// x = hi + lo, hi = fp16(x) (saturated at the fp16 maximum, as the inference path's split in eec_device.h), lo = fp16(x - hi);
// hi.hi + hi.lo + lo.hi with fp32 accumulation, ~2^-21 relative per product WHILE lo is a normal fp16 number: below 2^-14 it
// keeps absolute, not relative, precision (the device does not flush fp16 subnormals; their spacing is 2^-24).  Unscaled, that
// already holds for |x| < 2^-3, and a decoder whose feed-forward or value weights are of the order 1e-4 .. 1e-3 lost the
// precision of the split: tests/test_gpu_aed_step.py (weight domain) measured 0.017 / 0.077 / 1.30 of its bound -- twice
// 2e-5 * max(10, max |logp|) -- on weights scaled by 2^0 / 2^-4 / 2^-8.  So the WEIGHT fragments are multiplied by kWScale = 2^8
// before the split (exact; the factor the stem's packed weights carry, DESIGN.md "Stem domains") and the summed accumulators by
// 2^-8 in the epilogue: weights keep the full split down to |w| ~ 2^-11 and saturate beyond |w| = 255 (the decoders of the AED
// tests stay below 1; rescaled by 2^8, below 16).  With it the same test reads 0.014 / 0.017 / 0.112.  The ACTIVATIONS are split
// as they are, which is what is left at 2^-8 (hidden rows of the order 4e-3): a row whose entries fall far below 2^-3 keeps
// fewer bits, and a per-row exponent would be the next step if a checkpoint needed it.  (The bf16x3 form, 2^-16, moved the final
// scores of a 12-step search by 1.5e-4 against the fp32 step decoder; this one keeps them within 1e-4.)
// Workgroup = 64 rows x 32 columns of one exit (grid: column tiles, row tiles, exit).  The 4 waves split the contraction
// (wave w takes the 16-deep k-steps w, w + 4, ...), each with 4 k-steps of loads in flight: at B = 1 a call is a chain of
// dependent memory round trips, and the split cuts it 4-fold; the partial tiles are summed through LDS in the epilogue.
// Operand fragments come straight from global memory (lane l = 32 h + r holds row r, k = 8 h .. 8 h + 7 of both operands:
// two float4 each) and are split in registers.  LayerNorm (over K = d_model, eps 1e-5) in the prologue: row statistics into
// LDS, the normalisation applied as the fragments are loaded.  Bias, ReLU and the residual add in the epilogue.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kTM = 64, kTN = 32, kKB = 4;  // rows, columns of a workgroup; k-steps in flight per wave
constexpr float kHalfMax = 65504.0f;
constexpr float kWScale = 256.0f;  // on the weight fragments before the split, undone on the accumulator sum

struct ExitLinear {
  const float *W, *bias;     // [N][K], [N]
  const float *ln_g, *ln_b;  // [K] or null
};
struct BatchLinearArgs {
  const float* X;  // row m of exit e at X + e * x_e + m * ldx
  long ldx, x_e;
  float* Y;
  long ldy, y_e;
  int M, N, K, relu, accumulate;
  ExitLinear ex[kGroup];
};

// 8 consecutive fp32 of a row from k (a multiple of 8; K a multiple of 4), zero past K
__device__ __forceinline__ f32x8 load8(const float* p, int k, int K) {
  f32x8 v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < K) {
    const float4 a = *reinterpret_cast<const float4*>(p + k);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  }
  if (k + 4 < K) {
    const float4 b = *reinterpret_cast<const float4*>(p + k + 4);
    v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  return v;
}
__device__ __forceinline__ void split8(f32x8 x, h8& hi, h8& lo) {
  const f32x8 top = {kHalfMax, kHalfMax, kHalfMax, kHalfMax, kHalfMax, kHalfMax, kHalfMax, kHalfMax};
  hi = __builtin_convertvector(__builtin_elementwise_min(__builtin_elementwise_max(x, -top), top), h8);
  lo = __builtin_convertvector(x - __builtin_convertvector(hi, f32x8), h8);
}
__device__ __forceinline__ f32x16 mac3(f32x16 acc, h8 ah, h8 al, h8 bh, h8 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);  // small terms first
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

__global__ __launch_bounds__(256) void batch_linear_kernel(BatchLinearArgs a) {
  const ExitLinear& ex = a.ex[blockIdx.z];
  __shared__ float mu[kTM], rs[kTM];
  __shared__ float part[4][kTM][kTN + 1];  // the 4 waves' partial tiles
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5, K = a.K;
  const int m0 = blockIdx.y * kTM, n0 = blockIdx.x * kTN, n = n0 + r;
  const float* X = a.X + blockIdx.z * a.x_e;
  const bool ln = ex.ln_g != nullptr;
  if (ln) {  // wave w: statistics of rows m0 + 16 w .. + 16, a row per 16-lane group, the row held in registers (K <= 1024)
    const int g = lane >> 4, l16 = lane & 15;
    for (int it = 0; it < kTM / 16; ++it) {
      const int ml = 16 * w + 4 * it + g, m = m0 + ml;
      const float* xr = X + (long)(m < a.M ? m : 0) * a.ldx;
      float4 v[16];
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = 4 * l16 + 64 * j;
        v[j] = k < K ? *reinterpret_cast<const float4*>(xr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
      }
      const float mean = wave_all_sum(s, 8) / K;
      float q = 0.0f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (4 * l16 + 64 * j < K) {
          const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
          q += dx * dx + dy * dy + dz * dz + dw * dw;
        }
      }
      const float rstd = rsqrtf(wave_all_sum(q, 8) / K + 1e-5f);
      if (l16 == 0) mu[ml] = mean, rs[ml] = rstd;
    }
    __syncthreads();
  }
  const int ma = m0 + r, mb = m0 + 32 + r;
  const bool va = ma < a.M, vb = mb < a.M, vn = n < a.N;
  const float* xa = X + (long)(va ? ma : 0) * a.ldx;
  const float* xb = X + (long)(vb ? mb : 0) * a.ldx;
  const float* wr = ex.W + (long)(vn ? n : 0) * K;
  const float mua = ln ? mu[r] : 0.0f, rsa = ln ? rs[r] : 1.0f, mub = ln ? mu[32 + r] : 0.0f, rsb = ln ? rs[32 + r] : 1.0f;
  f32x16 acc0 = {}, acc1 = {};
  for (int kb = 16 * w; kb < K; kb += 64 * kKB) {
    f32x8 wv[kKB], av[kKB], bv[kKB];
#pragma unroll
    for (int i = 0; i < kKB; ++i) {  // all loads of the kKB k-steps first
      const int k = kb + 64 * i + 8 * h;
      wv[i] = vn ? load8(wr, k, K) : f32x8{};
      av[i] = va ? load8(xa, k, K) : f32x8{};
      bv[i] = vb ? load8(xb, k, K) : f32x8{};
    }
#pragma unroll
    for (int i = 0; i < kKB; ++i) {
      if (ln) {
        const int k = kb + 64 * i + 8 * h;
        const f32x8 g = load8(ex.ln_g, k, K), be = load8(ex.ln_b, k, K);  // zero past K: the padded k stay 0
        av[i] = (av[i] - mua) * rsa * g + be;
        bv[i] = (bv[i] - mub) * rsb * g + be;
      }
      h8 wh, wl, ah, al, bh, bl;
      split8(wv[i] * kWScale, wh, wl);
      split8(av[i], ah, al);
      split8(bv[i], bh, bl);
      acc0 = mac3(acc0, ah, al, wh, wl);
      acc1 = mac3(acc1, bh, bl, wh, wl);
    }
  }
  // accumulator register i of a 32 x 32 tile: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 h
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
    part[w][row][r] = acc0[i];
    part[w][32 + row][r] = acc1[i];
  }
  __syncthreads();
  const int c = tid & 31, nc = n0 + c;
  if (nc >= a.N) return;
  const float bias = ex.bias ? ex.bias[nc] : 0.0f;
  float* Y = a.Y + blockIdx.z * a.y_e + nc;
  for (int row = tid >> 5; row < kTM && m0 + row < a.M; row += 8) {
    float v = ((part[0][row][c] + part[1][row][c]) + (part[2][row][c] + part[3][row][c])) * (1.0f / kWScale) + bias;
    if (a.relu) v = fmaxf(v, 0.0f);
    float* yp = Y + (long)(m0 + row) * a.ldy;
    *yp = a.accumulate ? *yp + v : v;
  }
}

hipError_t batch_linear(const BatchLinearArgs& a, int E, hipStream_t st) {
  hipLaunchKernelGGL(batch_linear_kernel, dim3((a.N + kTN - 1) / kTN, (a.M + kTM - 1) / kTM, E), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// New position s of every live beam of every (exit, utterance) u: x = emb[token] + pe[s]; pad flag of (s, r); ancestry of
// beam r = ancestry of its parent in the previous step + its own slot r at position s.  Grid (R, E * B).
// ---------------------------------------------------------------------------------------------------------------------
struct BatchEmbedArgs {
  const long long *tok, *parent;  // [E*B][R]
  const float* emb[kGroup];
  const float* pe[kGroup];
  float* x;  // [E*B*R][D]
  unsigned char* pad;
  int* anc;
  long anc_u;
  int B, R, R_prev, s, S_max, D, V, pad_idx;
};
__global__ __launch_bounds__(256) void batch_embed_kernel(BatchEmbedArgs a) {
  const int r = blockIdx.x, u = blockIdx.y, e = u / a.B, s = a.s, S_max = a.S_max;
  const long row = (long)u * a.R + r;
  const long long t = a.tok[row];
  const long long tc = t < 0 ? 0 : (t >= a.V ? a.V - 1 : t);  // nn.Embedding would raise; stay in bounds
  const float *emb = a.emb[e], *pe = a.pe[e];
  for (int c = threadIdx.x; c < a.D; c += 256) a.x[row * a.D + c] = emb[tc * a.D + c] + pe[(long)s * a.D + c];
  if (threadIdx.x == 0) a.pad[(long)u * S_max * kRows + s * kRows + r] = t == a.pad_idx;
  int p = 0;
  if (s > 0) {
    const long long pp = a.parent ? a.parent[row] : r;
    p = (int)(pp < 0 ? 0 : (pp >= a.R_prev ? a.R_prev - 1 : pp));
  }
  const int* anc_old = a.anc + u * a.anc_u + (long)((s + 1) & 1) * kRows * S_max;
  int* anc_new = a.anc + u * a.anc_u + (long)(s & 1) * kRows * S_max;
  for (int i = threadIdx.x; i <= s; i += 256) anc_new[r * S_max + i] = i < s ? anc_old[p * S_max + i] : r;
}

// log_softmax of the exit heads' logits, a wave per row of E * B * R
__global__ __launch_bounds__(64) void batch_logsoftmax_kernel(const float* __restrict__ logits, float* __restrict__ out, int V) {
  log_softmax_row(logits + (long)blockIdx.x * V, out + (long)blockIdx.x * V, V, threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------------
// Self-attention: one query row per (row of exit e, head h) workgroup of 4 waves, keys 0 .. s of the beam's ancestry
// (position s itself comes from this step's in_proj output and is appended to the cache here), keys whose token is the
// padding index masked.  Grid (B * R, H, E).
// ---------------------------------------------------------------------------------------------------------------------
struct SelfAttnArgs {
  const float* qkv;  // [E][B*R][3D]
  float* kv;         // layer l of (exit, utterance) u: kv + u * kv_u, [S_max][16][2D]
  long kv_u;
  const int* anc;  // u: anc + u * anc_u, this step's half [16][S_max]
  long anc_u;
  const unsigned char* pad;  // u: pad + u * S_max * 16
  float* ctx;                // [E][B*R][D]
  int B, R, s, S_max, D, dh;
  float scale;
};
__global__ __launch_bounds__(256) void batch_self_attn_kernel(SelfAttnArgs a) {
  extern __shared__ float lds[];
  __shared__ float red[4][64];
  __shared__ float stat[2][4];
  const int gr = blockIdx.x, h = blockIdx.y, e = blockIdx.z, b = gr / a.R, r = gr - b * a.R;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int dh = a.dh, D = a.D, nk = a.s + 1, S_max = a.S_max;
  const long u = (long)e * a.B + b, row = (long)e * a.B * a.R + gr;
  float* sc = lds;               // [nk] scores, then probabilities
  int* slot = (int*)(lds + nk);  // [nk] cache slot of key t
  const float* q = a.qkv + row * 3 * D + h * dh;
  const float *kn = q + D, *vn = q + 2 * D;
  float* kv = a.kv + u * a.kv_u;
  const int* anc = a.anc + u * a.anc_u;
  const unsigned char* pad = a.pad + u * S_max * kRows;
  if (tid < dh) {  // append the new position: cache row (s, r)
    float* dst = kv + ((long)a.s * kRows + r) * 2 * D + h * dh;
    dst[tid] = kn[tid];
    dst[D + tid] = vn[tid];
  }
  float mx = -INFINITY;
  for (int t = tid; t < nk; t += 256) {
    const int sl = t == a.s ? r : anc[r * S_max + t];
    slot[t] = sl;
    const bool live = !pad[t * kRows + sl];
    const float* kp = t == a.s ? kn : kv + ((long)t * kRows + sl) * 2 * D + h * dh;
    float d = 0.0f;
    for (int i = 0; i < dh; i += 4) {
      const float4 k4 = *reinterpret_cast<const float4*>(kp + i);
      const float4 qv = *reinterpret_cast<const float4*>(q + i);
      d += qv.x * k4.x + qv.y * k4.y + qv.z * k4.z + qv.w * k4.w;
    }
    d = live ? d * a.scale : -INFINITY;
    sc[t] = d;
    mx = fmaxf(mx, d);
  }
  mx = wave_all_max(mx);
  if (lane == 0) stat[0][w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(stat[0][0], stat[0][1]), fmaxf(stat[0][2], stat[0][3]));
  float sum = 0.0f;
  for (int t = tid; t < nk; t += 256) {
    const float p = sc[t] == -INFINITY ? 0.0f : __expf(sc[t] - mx);
    sc[t] = p;
    sum += p;
  }
  sum = wave_all_sum(sum);
  if (lane == 0) stat[1][w] = sum;
  __syncthreads();
  const float inv = 1.0f / (stat[1][0] + stat[1][1] + stat[1][2] + stat[1][3]);  // no live key: nan, as torch
  // probabilities . V: lane = (feature d, part); the 4 * (64 / dh) (wave, part) pairs interleave the keys
  const int parts = 64 / dh, d = lane % dh, part = lane / dh, stride = 4 * parts;
  float acc = 0.0f;
  for (int t = w * parts + part; t < nk; t += stride) {
    const float* vp = t == a.s ? vn : kv + ((long)t * kRows + slot[t]) * 2 * D + D + h * dh;
    acc += sc[t] * vp[d];
  }
  for (int m = dh; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
  red[w][lane] = acc;
  __syncthreads();
  if (tid < dh) a.ctx[row * D + h * dh + tid] = (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) * inv;
}

// ---------------------------------------------------------------------------------------------------------------------
// Cross-attention: one workgroup per (head h, utterance b, exit e) owns all R beam queries of it, so the utterance's memory
// keys / values are read once per step, not once per beam.  Keys in chunks of 256 (one per thread): scores of all R queries
// -> LDS; per query, an online softmax (running max and sum: any Tq in one pass); probabilities . V with lane = (feature d,
// part), R accumulators per lane, rescaled as the running max moves.  No mask: the memory is the full padded tap.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kChunk = 256;
struct CrossAttnArgs {
  const float* q;    // [E][B*R][D]
  const float* mem;  // layer l of exit e, utterance b: mem + e * mem_e + b * Tq * 2D, [Tq][2D]
  long mem_e;
  float* ctx;  // [E][B*R][D]
  int B, R, Tq, D, dh;
  float scale;
};
__global__ __launch_bounds__(256) void batch_cross_attn_kernel(CrossAttnArgs a) {
  __shared__ float qs[kRows * 64];   // the R queries of this head, scaled
  __shared__ float ps[kRows][kChunk];  // scores, then probabilities, of a chunk; at the end the partial outputs
  __shared__ float alpha[kRows], lsum[kRows];
  const int h = blockIdx.x, b = blockIdx.y, e = blockIdx.z, tid = threadIdx.x;
  const int R = a.R, dh = a.dh, D = a.D, Tq = a.Tq;
  const long row0 = (long)e * a.B * R + (long)b * R;
  for (int i = tid; i < R * dh; i += 256) qs[i] = a.q[(row0 + i / dh) * D + h * dh + i % dh] * a.scale;
  const float* kvp = a.mem + e * a.mem_e + (long)b * Tq * 2 * D + h * dh;  // key t at kvp + t * 2D, value at + D
  const int rr = tid >> 4, l16 = tid & 15;  // softmax lanes: 16 per query row
  float m_run = -INFINITY, l_run = 0.0f;
  const int parts = 256 / dh, d = tid % dh, part = tid / dh;  // P . V lanes
  float acc[kRows];
#pragma unroll
  for (int i = 0; i < kRows; ++i) acc[i] = 0.0f;
  __syncthreads();
  for (int t0 = 0; t0 < Tq; t0 += kChunk) {
    {
      const int t = t0 + tid;
      float sc[kRows];
#pragma unroll
      for (int i = 0; i < kRows; ++i) sc[i] = t < Tq ? 0.0f : -INFINITY;
      if (t < Tq) {
        const float* kp = kvp + (long)t * 2 * D;
        for (int k = 0; k < dh; k += 4) {
          const float4 k4 = *reinterpret_cast<const float4*>(kp + k);
#pragma unroll
          for (int i = 0; i < kRows; ++i)
            if (i < R) sc[i] += qs[i * dh + k] * k4.x + qs[i * dh + k + 1] * k4.y + qs[i * dh + k + 2] * k4.z + qs[i * dh + k + 3] * k4.w;
        }
      }
#pragma unroll
      for (int i = 0; i < kRows; ++i)
        if (i < R) ps[i][tid] = sc[i];
    }
    __syncthreads();
    if (rr < R) {
      float mx = -INFINITY;
      for (int j = l16; j < kChunk; j += 16) mx = fmaxf(mx, ps[rr][j]);
      const float m_new = fmaxf(m_run, wave_all_max(mx, 8));  // finite: the chunk holds at least one key
      float sum = 0.0f;
      for (int j = l16; j < kChunk; j += 16) {
        const float p = __expf(ps[rr][j] - m_new);
        ps[rr][j] = p;
        sum += p;
      }
      const float al = __expf(m_run - m_new);
      l_run = l_run * al + wave_all_sum(sum, 8);
      m_run = m_new;
      if (l16 == 0) alpha[rr] = al;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRows; ++i)
      if (i < R) acc[i] *= alpha[i];
    const int nj = min(kChunk, Tq - t0);
    for (int j = part; j < nj; j += parts) {
      const float v = kvp[(long)(t0 + j) * 2 * D + D + d];
#pragma unroll
      for (int i = 0; i < kRows; ++i)
        if (i < R) acc[i] += ps[i][j] * v;
    }
    __syncthreads();
  }
  float* red = &ps[0][0];  // [parts][16][dh] = 256 * 16 floats
#pragma unroll
  for (int i = 0; i < kRows; ++i)
    if (i < R) red[(part * kRows + i) * dh + d] = acc[i];
  if (rr < R && l16 == 0) lsum[rr] = l_run;
  __syncthreads();
  for (int i = tid; i < R * dh; i += 256) {
    const int r = i / dh, dd = i - r * dh;
    float s = 0.0f;
    for (int p = 0; p < parts; ++p) s += red[(p * kRows + r) * dh + dd];
    a.ctx[(row0 + r) * D + h * dh + dd] = s / lsum[r];
  }
}

}  // namespace

extern "C" {

size_t eec_decoder_batch_cache_bytes(int d_model, int n_heads, int d_ff, int vocab, int n_layers, int E, int B, int S_max, int Tq) {
  const Geo g{d_model, n_heads, d_ff, vocab, n_layers, S_max, Tq, E, B};
  return geometry_ok(g) ? carve(nullptr, g).bytes : 0;
}

int eec_decoder_batch_begin(const eec_decoder_params* const* ps, int E, int B, int d_model, int n_heads, int d_ff, int vocab, const float* taps,
                            int Tq, int S_max, int passes, void* cache, size_t cache_bytes, void* stream) {
  Geo g{d_model, n_heads, d_ff, vocab, 0, S_max, Tq, E, B};
  Cache c;
  if (int rc = check_call(taps != nullptr, ps, E, g, nullptr, &cache, 1, cache_bytes, &c)) return rc;
  if (int rc = eech::check_passes(passes)) return rc;
  const int L = g.L;
  hipStream_t st = (hipStream_t)stream;
  const int D = d_model;
  const size_t rows = (size_t)B * Tq;
  for (int e = 0; e < E; ++e)
    for (int l = 0; l < L; ++l) {  // memory keys | values of every (exit, layer) over the B * Tq rows: taps[e] . W[D:3D]^T + b[D:3D]
      const eec_decoder_layer_params& P = ps[e]->layers[l];
      GemmArgs a = gemm_args(taps + (size_t)e * rows * D, D, 1, P.ca_in_w + (size_t)D * D, D, 1, c.mem + ((size_t)e * L + l) * rows * 2 * D, 2 * D,
                             (int)rows, 2 * D, D);
      a.bias = P.ca_in_b + D;
      EEC_HIP(launch_gemm(a, passes, st));
    }
  return 0;
}

int eec_decoder_batch_step(const eec_decoder_params* const* ps, int E, int B, int d_model, int n_heads, int d_ff, int vocab, int pad_idx,
                           const int64_t* last_tokens, const int64_t* parent, int R, int R_prev, int s, int Tq, int S_max, float* out, void* cache,
                           size_t cache_bytes, void* stream) {
  Geo g{d_model, n_heads, d_ff, vocab, 0, S_max, Tq, E, B};
  const Step step{R, R_prev, s};
  Cache c;
  if (int rc = check_call(last_tokens && out, ps, E, g, &step, &cache, 1, cache_bytes, &c)) return rc;
  const int L = g.L;
  hipStream_t st = (hipStream_t)stream;
  const int D = d_model, H = n_heads, dh = D / H, F = d_ff, M = B * R;
  const float scale = 1.0f / sqrtf((float)dh);
  const long U = (long)E * B;
  const long kv_u = (long)L * S_max * kRows * 2 * D, anc_u = 2L * kRows * S_max;
  {
    BatchEmbedArgs a{};
    a.tok = (const long long*)last_tokens, a.parent = (const long long*)parent;
    for (int e = 0; e < E; ++e) a.emb[e] = ps[e]->emb, a.pe[e] = ps[e]->pe;
    a.x = c.x, a.pad = c.pad, a.anc = c.anc, a.anc_u = anc_u;
    a.B = B, a.R = R, a.R_prev = R_prev, a.s = s, a.S_max = S_max, a.D = D, a.V = vocab, a.pad_idx = pad_idx;
    hipLaunchKernelGGL(batch_embed_kernel, dim3(R, (unsigned)U), dim3(256), 0, st, a);
    EEC_HIP(hipGetLastError());
  }
  // one batch_linear launch for all exits: exit e's weights through f(e)
  auto linear = [&](const float* X, long ldx, float* Y, long ldy, int N, int K, int relu, int accumulate, auto f) {
    BatchLinearArgs a{};
    a.X = X, a.ldx = ldx, a.x_e = (long)M * ldx, a.Y = Y, a.ldy = ldy, a.y_e = (long)M * ldy;
    a.M = M, a.N = N, a.K = K, a.relu = relu, a.accumulate = accumulate;
    for (int e = 0; e < E; ++e) a.ex[e] = f(e);
    return batch_linear(a, E, st);
  };
  const size_t self_lds = (size_t)(s + 1) * 8;
  EEC_HIP(eec::ensure_max_lds((const void*)batch_self_attn_kernel, (int)self_lds));
  for (int l = 0; l < L; ++l) {
    auto P = [&](int e) -> const eec_decoder_layer_params& { return ps[e]->layers[l]; };
    // self-attention over each beam's own prefix
    EEC_HIP(linear(c.x, D, c.qkv, 3L * D, 3 * D, D, 0, 0, [&](int e) { return ExitLinear{P(e).sa_in_w, P(e).sa_in_b, P(e).norm1_w, P(e).norm1_b}; }));
    {
      SelfAttnArgs a{c.qkv, c.kv + (size_t)l * S_max * kRows * 2 * D, kv_u, c.anc + (size_t)(s & 1) * kRows * S_max, anc_u, c.pad, c.ctx,
                     B, R, s, S_max, D, dh, scale};
      hipLaunchKernelGGL(batch_self_attn_kernel, dim3(M, H, E), dim3(256), self_lds, st, a);
      EEC_HIP(hipGetLastError());
    }
    EEC_HIP(linear(c.ctx, D, c.x, D, D, D, 0, 1, [&](int e) { return ExitLinear{P(e).sa_out_w, P(e).sa_out_b, nullptr, nullptr}; }));
    // cross-attention over the utterance's memory
    EEC_HIP(linear(c.x, D, c.q, D, D, D, 0, 0, [&](int e) { return ExitLinear{P(e).ca_in_w, P(e).ca_in_b, P(e).norm2_w, P(e).norm2_b}; }));
    {
      CrossAttnArgs a{c.q, c.mem + (size_t)l * B * Tq * 2 * D, (long)L * B * Tq * 2 * D, c.ctx, B, R, Tq, D, dh, scale};
      hipLaunchKernelGGL(batch_cross_attn_kernel, dim3(H, B, E), dim3(256), 0, st, a);
      EEC_HIP(hipGetLastError());
    }
    EEC_HIP(linear(c.ctx, D, c.x, D, D, D, 0, 1, [&](int e) { return ExitLinear{P(e).ca_out_w, P(e).ca_out_b, nullptr, nullptr}; }));
    // feed-forward, ReLU
    EEC_HIP(linear(c.x, D, c.h, F, F, D, 1, 0, [&](int e) { return ExitLinear{P(e).w1, P(e).b1, P(e).norm3_w, P(e).norm3_b}; }));
    EEC_HIP(linear(c.h, F, c.x, D, D, F, 0, 1, [&](int e) { return ExitLinear{P(e).w2, P(e).b2, nullptr, nullptr}; }));
  }
  EEC_HIP(linear(c.x, D, c.logits, vocab, vocab, D, 0, 0, [&](int e) { return ExitLinear{ps[e]->head_w, ps[e]->head_b, ps[e]->norm_w, ps[e]->norm_b}; }));
  hipLaunchKernelGGL(batch_logsoftmax_kernel, dim3((unsigned)(U * R)), dim3(64), 0, st, c.logits, out, vocab);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
