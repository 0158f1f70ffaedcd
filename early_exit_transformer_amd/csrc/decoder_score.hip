// Teacher-forced scoring of whole hypotheses under one AED decoder (include/eec.h, eec_decoder_score): R hypotheses for each
// of n memories in ONE pass -- the second pass of two-pass decoding, where the CTC head proposes an N-best list and the
// attention decoder scores it.  The arithmetic per row is eec_decoder_forward's (decoder.hip: the same embed, LayerNorm, GEMM
// and masked-softmax launches, the same masks), laid out so that
//   * self-attention and every row-wise GEMM run over all M = n * R * S rows at once (S = L + 1),
//   * the memory keys | values are projected once per memory, and the cross-attention is the batched GEMM with batch n * H and
//     R * S query rows: the R hypotheses of a memory are contiguous,
//   * the head's [M][V] logits are reduced to one number per hypothesis by hyp_score_kernel; no [M][V] log-probs are written.
#include <algorithm>
#include <string>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_train.h"
#include "eec_wave.h"

using namespace eect;
using namespace eech;

namespace {

// decoder input rows: hypothesis h of length k = min(len, L) (absent, len < 0: as k = 0, its tokens never read) becomes
// SOS, y_1 .. y_k, pad ... over S = L + 1 positions, as int64 for launch_embed_pe
__global__ __launch_bounds__(256) void hyp_rows_kernel(const int* __restrict__ tok, const int* __restrict__ len, long long* __restrict__ trg, long n_hyp,
                                                       int L, int sos, int pad_idx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, S = L + 1;
  if (i >= n_hyp * S) return;
  const long h = i / S;
  const int pos = (int)(i - h * S), k = min(len[h], L);
  trg[i] = pos == 0 ? sos : (pos <= k ? tok[h * L + pos - 1] : pad_idx);
}
hipError_t launch_hyp_rows(const int* tok, const int* len, long long* trg, long n_hyp, int L, int sos, int pad_idx, hipStream_t st) {
  hipLaunchKernelGGL(hyp_rows_kernel, dim3((unsigned)((n_hyp * (L + 1) + 255) / 256)), dim3(256), 0, st, tok, len, trg, n_hyp, L, sos, pad_idx);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// score[h] = sum_{t = 0 .. k} log_softmax(logits[h * S + t])[target_t], targets y_1 .. y_k, EOS (ids clamped into [0, V) as the
// embedding clamps them); -inf for an absent hypothesis.  One workgroup per hypothesis, one wave per row (wave w: rows w, w + 4,
// ...): the row is read once, a float4 per lane and step (V a multiple of 4, at most 1024: 4 steps, held in registers), its
// maximum by wave_max, the exp-sum pairwise inside a float4, then over the lane's steps, then the DPP tree -- log2(V) + 2 levels
// of rounding -- and the term is (x[target] - max) - log(sum).  The k + 1 terms meet in LDS and one work-item adds them in index
// order in fp64, rounded once: no atomics, the same bits every run.  A term that is not a number (a row without a finite
// logit) counts as -inf: no NaN leaves.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kScoreMaxV = 1024;
__global__ __launch_bounds__(256) void hyp_score_kernel(const float* __restrict__ logits, const int* __restrict__ tok, const int* __restrict__ len,
                                                        float* __restrict__ score, int L, int V, int eos) {
  extern __shared__ float term[];  // [S]
  const long h = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, S = L + 1;
  const int k_raw = len[h];
  if (k_raw < 0) {  // absent (uniform over the workgroup)
    if (threadIdx.x == 0) score[h] = -INFINITY;
    return;
  }
  const int k = min(k_raw, L);
  for (int t = w; t <= k; t += 4) {
    const float* xr = logits + (h * S + t) * V;
    float mx = -INFINITY, sum;
    if ((V & 3) == 0) {
      const int n4 = V >> 2;
      float4 v[kScoreMaxV / 256];
#pragma unroll
      for (int j = 0; j < kScoreMaxV / 256; ++j) {
        const int q = lane + 64 * j;
        v[j] = q < n4 ? reinterpret_cast<const float4*>(xr)[q] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        mx = fmaxf(mx, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
      }
      mx = eec::wave_max(mx);
      float s[kScoreMaxV / 256];
#pragma unroll
      for (int j = 0; j < kScoreMaxV / 256; ++j)  // exp(-inf) = 0 past the row's end
        s[j] = (expf(v[j].x - mx) + expf(v[j].y - mx)) + (expf(v[j].z - mx) + expf(v[j].w - mx));
      sum = (s[0] + s[1]) + (s[2] + s[3]);
    } else {  // any other V: scalar loads, two passes, pairs of lane steps
      for (int c = lane; c < V; c += 64) mx = fmaxf(mx, xr[c]);
      mx = eec::wave_max(mx);
      float s0 = 0.0f, s1 = 0.0f;
      for (int c = lane; c < V; c += 128) {
        s0 += expf(xr[c] - mx);
        if (c + 64 < V) s1 += expf(xr[c + 64] - mx);
      }
      sum = s0 + s1;
    }
    sum = eec::wave_sum(sum);
    if (lane == 0) {
      int y = t < k ? tok[h * L + t] : eos;
      y = y < 0 ? 0 : (y >= V ? V - 1 : y);
      const float lp = (xr[y] - mx) - logf(sum);
      term[t] = lp == lp ? lp : -INFINITY;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int t = 0; t <= k; ++t) acc += (double)term[t];
    score[h] = (float)acc;
  }
}

hipError_t launch_hyp_score(const float* logits, const int* tok, const int* len, float* score, long n_hyp, int L, int V, int eos, hipStream_t st) {
  hipLaunchKernelGGL(hyp_score_kernel, dim3((unsigned)n_hyp), dim3(256), (size_t)(L + 1) * sizeof(float), st, logits, tok, len, score, L, V, eos);
  return hipGetLastError();
}

constexpr int kScoreMaxS = 8192;  // the terms of a hypothesis in LDS: 32 KiB
// one call: the self-attention's GEMM batches n * R * H and the 32-row tiles of the M = n * R * S rows are grid dimensions
constexpr long kMaxBatches = 65535, kMaxRows = 32L * 65535;

struct Geo {
  int D, H, F, V, n, R, S, Tq, dh;
};
struct Bufs {
  float *x, *ln, *qkv, *kv, *P, *ctx, *h, *o, *logits;
  unsigned char* pad;
  long long* trg;
};
Bufs carve(Bump& c, const Geo& g) {
  Bufs b{};
  const size_t M = (size_t)g.n * g.R * g.S, Mk = (size_t)g.n * g.Tq;
  b.x = c.f(M * g.D), b.ln = c.f(M * g.D), b.qkv = c.f(M * 3 * g.D), b.kv = c.f(Mk * 2 * g.D);
  b.P = c.f((size_t)g.n * g.R * g.H * g.S * std::max(g.S, g.Tq));  // self: [n*R*H][S][S]; cross: [n*H][R*S][Tq]
  b.ctx = c.f(M * g.D), b.h = c.f(M * std::max(g.F, 2)), b.o = c.f(M * g.D), b.logits = c.f(M * g.V);
  b.pad = c.take<unsigned char>(M);
  b.trg = c.take<long long>(M);
  return b;
}
bool sizes_ok(int d_model, int n_heads, int d_ff, int vocab, int n, int R, int L, int Tq) {
  return d_model > 0 && d_model <= 1024 && n_heads > 0 && d_model % n_heads == 0 && d_ff > 0 && vocab > 0 && vocab <= kScoreMaxV && n >= 0 && R > 0 &&
         L >= 0 && L < kScoreMaxS && Tq > 0 && (long)n * R * n_heads <= kMaxBatches && (long)n * R * (L + 1) <= kMaxRows;
}

}  // namespace

extern "C" {

int eec_hypothesis_score(const float* logits, const int32_t* hyp_tokens, const int32_t* hyp_len, int n_hyp, int L, int vocab, int eos,
                         float* att_score, void* stream) {
  if (n_hyp < 0 || L < 0 || L >= kScoreMaxS || vocab < 1 || vocab > kScoreMaxV || eos < 0 || eos >= vocab)
    return fail(EEC_ERR_BAD_ARG, "eec_hypothesis_score: needs n_hyp >= 0, 0 <= L < " + std::to_string(kScoreMaxS) + ", 1 <= vocab <= " +
                                     std::to_string(kScoreMaxV) + ", eos in [0, vocab)");
  if (n_hyp == 0) return 0;
  if (!logits || !hyp_tokens || !hyp_len || !att_score) return fail(EEC_ERR_BAD_ARG, "eec_hypothesis_score: null argument");
  if (vocab % 4 == 0 && ((uintptr_t)logits & 15) != 0)  // rows are read a float4 at a time
    return fail(EEC_ERR_BAD_ARG, "eec_hypothesis_score: logits must be 16-byte aligned when vocab is a multiple of 4");
  EEC_HIP(launch_hyp_score(logits, hyp_tokens, hyp_len, att_score, n_hyp, L, vocab, eos, (hipStream_t)stream));
  return 0;
}

size_t eec_decoder_score_workspace_bytes(int d_model, int n_heads, int d_ff, int vocab, int n, int R, int L, int Tq) {
  if (!sizes_ok(d_model, n_heads, d_ff, vocab, n, R, L, Tq) || n == 0) return 0;
  Bump c;
  carve(c, Geo{d_model, n_heads, d_ff, vocab, n, R, L + 1, Tq, d_model / n_heads});
  return up256(c.off);
}

int eec_decoder_score(const eec_decoder_params* p, int d_model, int n_heads, int d_ff, int vocab, int pad_idx, int sos, int eos,
                      const int32_t* hyp_tokens, const int32_t* hyp_len, const float* enc, int n, int R, int L, int Tq, int passes, float* att_score,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!p || !p->layers) return fail(EEC_ERR_BAD_ARG, "eec_decoder_score: null argument");
  if (int rc = check_passes(passes)) return rc;
  if (!sizes_ok(d_model, n_heads, d_ff, vocab, n, R, L, Tq) || p->n_layers <= 0 || L + 1 > p->max_len)
    return fail(EEC_ERR_BAD_ARG, "eec_decoder_score: bad geometry");
  if (pad_idx < 0 || pad_idx >= vocab || sos < 0 || sos >= vocab || eos < 0 || eos >= vocab)
    return fail(EEC_ERR_BAD_ARG, "eec_decoder_score: pad_idx, sos and eos must lie in [0, vocab)");
  if (n == 0) return 0;
  if (!hyp_tokens || !hyp_len || !enc || !att_score || !workspace) return fail(EEC_ERR_BAD_ARG, "eec_decoder_score: null argument");
  const int S = L + 1;
  const Geo g{d_model, n_heads, d_ff, vocab, n, R, S, Tq, d_model / n_heads};
  Bump c;
  c.base = (char*)workspace, c.cap = workspace_bytes;
  const Bufs b = carve(c, g);
  if (int rc = check_workspace(workspace, workspace_bytes, up256(c.off))) return rc;  // eec_decoder_score_workspace_bytes
  hipStream_t st = (hipStream_t)stream;
  const int D = g.D, H = g.H, dh = g.dh, Bm = n * R, M = Bm * S, RS = R * S, Mk = n * Tq;
  const float scale = 1.0f / sqrtf((float)dh);
  float* stats = b.h;  // LayerNorm statistics are not kept: [2][M] scratch in the h buffer, which is free whenever a LayerNorm runs
  auto linear = [&](const float* x, const float* W, const float* bias, float* y, int m, int nn, int k, int epi, bool accumulate) {
    GemmArgs a = gemm_args(x, k, 1, W, k, 1, y, nn, m, nn, k);
    a.bias = bias, a.epi = epi, a.accumulate = accumulate ? 1 : 0;
    return launch_gemm(a, passes, st);
  };
  // nb batches of Sq query rows (row stride q_m, batch stride q_b) against Tk keys / values (row stride kv_m, batch stride kv_b)
  auto attention = [&](int nb, int Sq, const float* q, long q_m, long q_b, const float* k, const float* v, long kv_m, long kv_b, int Tk, int causal,
                       const unsigned char* pad) -> hipError_t {
    {  // scores[z][tq][tk] = Q . K^T
      GemmArgs a = gemm_args(q, q_m, 1, k, kv_m, 1, b.P, Tk, Sq, Tk, dh);
      a.nz = nb * H, a.zdiv = H, a.a_z0 = q_b, a.a_z1 = dh, a.b_z0 = kv_b, a.b_z1 = dh, a.c_z0 = (long)H * Sq * Tk, a.c_z1 = (long)Sq * Tk;
      if (hipError_t e = launch_gemm(a, passes, st); e != hipSuccess) return e;
    }
    if (hipError_t e = launch_softmax_masked(b.P, nb, H, Sq, Tk, scale, causal, pad, st); e != hipSuccess) return e;
    GemmArgs a = gemm_args(b.P, Tk, 1, v, 1, kv_m, b.ctx, D, Sq, dh, Tk);
    a.nz = nb * H, a.zdiv = H, a.a_z0 = (long)H * Sq * Tk, a.a_z1 = (long)Sq * Tk, a.b_z0 = kv_b, a.b_z1 = dh, a.c_z0 = (long)Sq * D, a.c_z1 = dh;
    return launch_gemm(a, passes, st);
  };
  EEC_HIP(launch_hyp_rows(hyp_tokens, hyp_len, b.trg, (long)Bm, L, sos, pad_idx, st));
  EEC_HIP(launch_embed_pe(b.trg, p->emb, p->pe, b.x, b.pad, (long)M, S, D, vocab, pad_idx, st));
  for (int l = 0; l < p->n_layers; ++l) {
    const eec_decoder_layer_params& P = p->layers[l];
    // self-attention of every hypothesis over its own row: causal + target key padding
    EEC_HIP(launch_ln_fwd(b.x, P.norm1_w, P.norm1_b, b.ln, stats, stats + M, M, D, st));
    EEC_HIP(linear(b.ln, P.sa_in_w, P.sa_in_b, b.qkv, M, 3 * D, D, 0, false));
    EEC_HIP(attention(Bm, S, b.qkv, 3 * D, (long)S * 3 * D, b.qkv + D, b.qkv + 2 * D, 3 * D, (long)S * 3 * D, S, 1, b.pad));
    EEC_HIP(linear(b.ctx, P.sa_out_w, P.sa_out_b, b.x, M, D, D, 0, true));
    // cross-attention: the R * S rows of a memory's hypotheses against its keys | values, projected once per memory
    EEC_HIP(launch_ln_fwd(b.x, P.norm2_w, P.norm2_b, b.ln, stats, stats + M, M, D, st));
    EEC_HIP(linear(b.ln, P.ca_in_w, P.ca_in_b, b.o, M, D, D, 0, false));
    EEC_HIP(linear(enc, P.ca_in_w + (size_t)D * D, P.ca_in_b + D, b.kv, Mk, 2 * D, D, 0, false));
    EEC_HIP(attention(n, RS, b.o, D, (long)RS * D, b.kv, b.kv + D, 2 * D, (long)Tq * 2 * D, Tq, 0, nullptr));
    EEC_HIP(linear(b.ctx, P.ca_out_w, P.ca_out_b, b.x, M, D, D, 0, true));
    // feed-forward, ReLU
    EEC_HIP(launch_ln_fwd(b.x, P.norm3_w, P.norm3_b, b.ln, stats, stats + M, M, D, st));
    EEC_HIP(linear(b.ln, P.w1, P.b1, b.h, M, g.F, D, 3, false));
    EEC_HIP(linear(b.h, P.w2, P.b2, b.x, M, D, g.F, 0, true));
  }
  EEC_HIP(launch_ln_fwd(b.x, p->norm_w, p->norm_b, b.ln, stats, stats + M, M, D, st));
  EEC_HIP(linear(b.ln, p->head_w, p->head_b, b.logits, M, vocab, D, 0, false));
  EEC_HIP(launch_hyp_score(b.logits, hyp_tokens, hyp_len, att_score, Bm, L, vocab, eos, st));
  return 0;
}

}  // extern "C"
