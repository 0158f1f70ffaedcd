// CTC forced alignment on the device: BeamInference.get_trellis + backtrack (util/beam_infer.py:129-191), the Viterbi
// alignment of a token sequence against one exit's CTC log-probs, for many hypotheses in one launch.  It is the CTC half
// of the reference's joint AED + CTC beam choice (the dormant branch util/beam_infer.py:309-383).
//
// Semantics: the reference's, quirks included (stated, not repaired).  em [T, V] fp32 log-probs, tok N ids, tr [T+1, N+1]:
//   tr[0,0] = 0;  tr[t+1,0] = tr[t,0] + em[t,0]  (column 0 of the emission, NOT `blank`);  tr[0,1:] = -inf;
//   tr[T+1-N:, 0] = +inf, applied after the cumulative sum;
//   tr[t+1,j] = max(tr[t,j] + em[t,blank], tr[t,j-1] + em[t,tok[j-1]])  for j >= 1: a token occupies exactly ONE frame,
//   staying costs the blank, repeated tokens get no special treatment.
//   The +inf cells occupy rows >= T+1-N+j; they feed only each other and the backtrack never reads them.
//   Backtrack from (t, j) = (T, N):  stayed = tr[t-1,j] + em[t-1,blank], changed = tr[t-1,j-1] + em[t-1,tok[j-1]]; the change
//   is taken only if changed > stayed (a tie stays);  prob += em[t-1, changed ? tok[j-1] : 0]  (the literal 0, not `blank`);
//   Point(j-1, t-1, prob); after a change --j, stop at j == 0.  The path is returned reversed, so path[0].score is the sum over
//   the whole path, from the first token's frame to the last frame.
// Stated divergence: for N > T or N = 0 the reference prints "Failed to align" and returns a fragment; here the hypothesis
// gets status 1 and its outputs the fill values (-1, -inf).  The same holds for a token id outside [0, V), an em_index
// outside [0, n_em), an em_len outside [1, Tq], a tok_len above tok_stride (none is ever used as an address), and for
// non-finite emissions that leave the backtrack short of the first token.
//
// One wavefront per hypothesis.  The recurrence is a serial chain over t of width N + 1: lane l owns the C = ceil((tok_stride
// + 1) / 64) contiguous columns l*C .. l*C + C - 1 in registers, and the one value that crosses a lane boundary (the left
// neighbour's last column of the previous row) comes by a DPP wave shift, so a frame costs C add / compare / select groups
// and no memory round trip.  The backtrack's comparison at (t, j) is the very comparison that produced tr[t,j], so the forward
// pass keeps its outcome: one ballot per frame and column slot k (bit l = column l*C + k), T * C 64-bit words in LDS; no
// trellis goes to memory unless the caller asks for it.  A frame's loads (the two broadcasts em[t,0] / em[t,blank] as one
// two-address vector load, and one 4-byte gather per column, V floats apart from the next frame's) are issued kAlAhead frames
// before their use, off the chain.  The walk back over the decision words is wave-uniform register work on words fetched
// eight frames at a time; the emissions on the path are then gathered by all lanes at once and summed in the reference's
// order (last frame first), so with equal trellis bits the Point scores equal the reference's bit for bit.
#include <math.h>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"

namespace eec {

constexpr int kAlMaxC = 4;               // columns per lane: tok_stride + 1 <= 256
constexpr int kAlAhead = 8;              // frames of look-ahead held in registers
constexpr size_t kAlMaxLds = 64 * 1024;  // decision words + path emissions + path columns of one hypothesis

__host__ __device__ inline size_t al_lds_bytes(int Tq, int C) { return ((size_t)Tq * (C * 8 + 4 + 2) + 15) & ~(size_t)15; }

template <int C, bool TRELLIS>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ logp, int n_em, int Tq, int V, const int* __restrict__ em_len,
                                                       const long long* __restrict__ tokens, const int* __restrict__ tok_len,
                                                       const int* __restrict__ em_index, int tok_stride, int blank,
                                                       int* __restrict__ point_token, float* __restrict__ point_score,
                                                       float* __restrict__ path_score, float* __restrict__ final_score,
                                                       int* __restrict__ status, float* __restrict__ trellis) {
  extern __shared__ __attribute__((aligned(16))) unsigned char al_smem[];
  unsigned long long* bits = (unsigned long long*)al_smem;                // [Tq][C]: bit l of word (f, k) = decision of column l*C + k at frame f
  float* vals = (float*)(al_smem + (size_t)Tq * C * 8);                   // [Tq]: the path's emission at frame f, then its cumulative score
  unsigned short* jrow = (unsigned short*)(al_smem + (size_t)Tq * (C * 8 + 4));  // [Tq]: the path's column at frame f | changed << 15
  const int h = blockIdx.x, lane = threadIdx.x;
  const int W = tok_stride + 1;
  int* pt_out = point_token + (size_t)h * Tq;
  float* ps_out = point_score + (size_t)h * Tq;
  float* tr_out = TRELLIS ? trellis + (size_t)h * (Tq + 1) * W : nullptr;

  const int N = tok_len[h];
  const int ei = em_index ? em_index[h] : h;
  int T = Tq;
  bool ok = ei >= 0 && ei < n_em;
  if (ok && em_len) T = em_len[ei];
  ok = ok && T >= 1 && T <= Tq && N >= 1 && N <= T && N <= tok_stride;
  const long long* tk = tokens + (size_t)h * tok_stride;
  int id[C];  // the label of column l*C + k (its token is tok[column - 1]); 0 for column 0 and the columns past N
  if (ok) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const int j = lane * C + k;
      const long long v = (j >= 1 && j <= N) ? tk[j - 1] : 0;
      bad = bad || v < 0 || v >= V;
      id[k] = bad ? 0 : (int)v;
    }
    ok = __ballot(bad) == 0;
  }
  if (!ok) {  // not alignable: defined fill values, nothing else is read
    for (int f = lane; f < Tq; f += 64) {
      pt_out[f] = -1;
      ps_out[f] = -INFINITY;
    }
    if (TRELLIS)
      for (size_t i = lane; i < (size_t)(Tq + 1) * W; i += 64) tr_out[i] = -INFINITY;
    if (lane == 0) {
      path_score[h] = -INFINITY;
      final_score[h] = -INFINITY;
      status[h] = 1;
    }
    return;
  }

  float tr[C];
#pragma unroll
  for (int k = 0; k < C; ++k) tr[k] = (lane * C + k == 0) ? 0.f : -INFINITY;
  if (TRELLIS) {
#pragma unroll
    for (int k = 0; k < C; ++k)
      if (lane * C + k < W) tr_out[lane * C + k] = tr[k];
  }
  const float* em = logp + (size_t)ei * Tq * V;
  const int inf_from = T + 1 - N;  // column 0 is +inf from this row on

  // the frame's two broadcasts travel as ONE vector load (even lanes em[t,0], odd lanes em[t,blank]): wave-uniform scalar
  // loads return out of order, so waiting for one of them would wait for the whole look-ahead
  const int bsel = (lane & 1) ? blank : 0;
  float rb[kAlAhead], rg[kAlAhead][C];
#pragma unroll
  for (int u = 0; u < kAlAhead; ++u) {
    const float* row = em + (size_t)min(u, T - 1) * V;
    rb[u] = row[bsel];
#pragma unroll
    for (int k = 0; k < C; ++k) rg[u][k] = row[id[k]];
  }
  for (int t0 = 0; t0 < T; t0 += kAlAhead) {
#pragma unroll
    for (int u = 0; u < kAlAhead; ++u) {
      const int t = t0 + u;
      const float e0 = rb[u];  // lane 0's own: em[t,0]
      const float eb = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rb[u]), 1));
      float g[C];
#pragma unroll
      for (int k = 0; k < C; ++k) g[k] = rg[u][k];
      {  // refill the slot with frame t + kAlAhead (past the end: the last frame again, unused)
        const float* row = em + (size_t)min(t + kAlAhead, T - 1) * V;
        rb[u] = row[bsel];
#pragma unroll
        for (int k = 0; k < C; ++k) rg[u][k] = row[id[k]];
      }
      if (t >= T) continue;
      const float left = from_left(tr[C - 1], 0.f);
      unsigned long long m[C];
#pragma unroll
      for (int k = C - 1; k >= 0; --k) {  // descending: tr[k - 1] is still the previous row's
        const float stayed = tr[k] + eb, changed = (k > 0 ? tr[k - 1] : left) + g[k];
        const bool bit = changed > stayed;
        float nv = (bit || changed != changed) ? changed : stayed;  // torch.maximum: a NaN on either side wins
        if (k == 0 && lane == 0) nv = (t + 1 >= inf_from) ? INFINITY : tr[0] + e0;
        m[k] = __ballot(bit);
        tr[k] = nv;
      }
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < C; ++k) bits[(size_t)t * C + k] = m[k];
      }
      if (TRELLIS) {
        float* dst = tr_out + (size_t)(t + 1) * W;
#pragma unroll
        for (int k = 0; k < C; ++k)
          if (lane * C + k < W) dst[lane * C + k] = (lane * C + k <= N) ? tr[k] : -INFINITY;
      }
    }
  }
  if (TRELLIS)  // the rows past this emission's length
    for (size_t i = (size_t)(T + 1) * W + lane; i < (size_t)(Tq + 1) * W; i += 64) tr_out[i] = -INFINITY;
  {
    float fv = tr[0];
#pragma unroll
    for (int k = 1; k < C; ++k)
      if (N % C == k) fv = tr[k];
    if (lane == N / C) final_score[h] = fv;
  }
  __syncthreads();

  // the walk back over the decision words: wave-uniform, eight frames' words per fetch
  int j = N, f0 = -1;
  for (int f = T - 1; f >= 0 && j > 0; f -= 8) {
    unsigned long long w[8][C];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int k = 0; k < C; ++k) w[u][k] = bits[(size_t)max(f - u, 0) * C + k];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int fu = f - u;
      if (fu < 0 || j <= 0) continue;
      const int k = j % C, l = j / C;
      unsigned long long word = w[u][0];
#pragma unroll
      for (int kk = 1; kk < C; ++kk)
        if (k == kk) word = w[u][kk];
      const int bit = (int)(word >> l) & 1;
      if (lane == 0) jrow[fu] = (unsigned short)(j | bit << 15);
      j -= bit;
      if (j == 0) f0 = fu;
    }
  }
  __syncthreads();
  if (f0 < 0) {  // non-finite emissions: the first token was never reached
    for (int f = lane; f < Tq; f += 64) {
      pt_out[f] = -1;
      ps_out[f] = -INFINITY;
    }
    if (lane == 0) {
      path_score[h] = -INFINITY;
      status[h] = 1;
    }
    return;
  }
  // the path's emissions, all lanes at once
  for (int f = lane; f < Tq; f += 64) {
    int pt = -1;
    if (f >= f0 && f < T) {
      const int e = jrow[f], jj = e & 0x7fff;
      pt = jj - 1;
      vals[f] = em[(size_t)f * V + ((e >> 15) ? (int)tk[jj - 1] : 0)];
    }
    pt_out[f] = pt;
  }
  __syncthreads();
  // cumulative scores in the reference's order: from the last frame towards the first token's
  if (lane == 0) {
    float acc = 0.f;
    for (int f = T - 1; f >= f0; f -= 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = vals[max(f - u, f0)];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (f - u >= f0) {
          acc += v[u];
          vals[f - u] = acc;
        }
    }
    path_score[h] = acc;
    status[h] = 0;
  }
  __syncthreads();
  for (int f = lane; f < Tq; f += 64) ps_out[f] = (f >= f0 && f < T) ? vals[f] : -INFINITY;
}

template <int C>
static hipError_t launch_ctc_align_c(bool want_trellis, dim3 grid, size_t lds, hipStream_t st, const float* logp, int n_em, int Tq, int V,
                                     const int* em_len, const long long* tokens, const int* tok_len, const int* em_index, int tok_stride,
                                     int blank, int* point_token, float* point_score, float* path_score, float* final_score, int* status,
                                     float* trellis) {
  if (want_trellis)
    hipLaunchKernelGGL((ctc_align_kernel<C, true>), grid, dim3(64), lds, st, logp, n_em, Tq, V, em_len, tokens, tok_len, em_index, tok_stride,
                       blank, point_token, point_score, path_score, final_score, status, trellis);
  else
    hipLaunchKernelGGL((ctc_align_kernel<C, false>), grid, dim3(64), lds, st, logp, n_em, Tq, V, em_len, tokens, tok_len, em_index, tok_stride,
                       blank, point_token, point_score, path_score, final_score, status, trellis);
  return hipGetLastError();
}

}  // namespace eec

extern "C" {

size_t eec_ctc_align_workspace_bytes(int n_hyp, int Tq, int max_tokens) {
  (void)n_hyp, (void)Tq, (void)max_tokens;
  return 0;  // decisions and path live in LDS
}

int eec_ctc_align(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int64_t* tokens, const int32_t* tok_len,
                  const int32_t* em_index, int n_hyp, int tok_stride, int blank, int32_t* point_token, float* point_score, float* path_score,
                  float* final_score, int32_t* status, float* trellis_opt, void* workspace, void* stream) {
  (void)workspace;
  using eech::fail;
  if (n_hyp < 0 || Tq < 1 || tok_stride < 1 || n_em < 1 || V < 1 || blank < 0 || blank >= V)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_align: needs n_hyp >= 0, Tq, tok_stride, n_em, V >= 1 and blank in [0, V)");
  if (n_hyp == 0) return 0;
  if (!logp || !tokens || !tok_len || !point_token || !point_score || !path_score || !final_score || !status)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_align: null argument");
  const int C = (tok_stride + 1 + 63) / 64;
  if (V < 2 || C > eec::kAlMaxC || eec::al_lds_bytes(Tq, C) > eec::kAlMaxLds)
    return fail(EEC_ERR_UNSUPPORTED, "eec_ctc_align: needs V >= 2, tok_stride <= " + std::to_string(64 * eec::kAlMaxC - 1) +
                                         " and a Tq x tok_stride lattice that fits the LDS");
  const size_t lds = eec::al_lds_bytes(Tq, C);
  const dim3 grid(n_hyp);
  hipStream_t st = (hipStream_t)stream;
#define EEC_AL_LAUNCH(c)                                                                                                                  \
  eec::launch_ctc_align_c<c>(trellis_opt != nullptr, grid, lds, st, logp, n_em, Tq, V, em_len, (const long long*)tokens, tok_len, em_index, \
                             tok_stride, blank, point_token, point_score, path_score, final_score, status, trellis_opt)
  hipError_t e = C == 1 ? EEC_AL_LAUNCH(1) : C == 2 ? EEC_AL_LAUNCH(2) : C == 3 ? EEC_AL_LAUNCH(3) : EEC_AL_LAUNCH(4);
#undef EEC_AL_LAUNCH
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_ctc_align launch");
}

}  // extern "C"
