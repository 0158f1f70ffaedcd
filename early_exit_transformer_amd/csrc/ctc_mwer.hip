// MWER training of the CTC exits (include/eec.h, "Minimum word error rate training"): the exact CTC log-likelihood of every
// hypothesis of an N-best list against the emission the list was decoded from, the expected-risk loss over the list, and its
// gradient with respect to the log-probs -- N CTC lattices that share one emission, their posteriors folded into ONE gradient row.
//
// Every recursion runs in log space with lb_log_add, the exactly stated fp32 sequence of include/eec.h: no scaling, no exponent
// bookkeeping, no range limit, and -inf is an ordinary value (an infeasible lattice ends at -inf by itself).  A lattice of a
// hypothesis of `len` tokens has S = 2 len + 1 states; lane l of the lattice's wave keeps the P states l P .. l P + P - 1 in
// registers, P = 2, 4 or 8 by the pitch L of the list (2 min(L, 255) + 1 <= 64 P).  P is even, so the odd registers are the label
// states and the even ones the blank states; the state to the left of a lane's first one comes by a one-lane shift.  States at or
// past S are held at -inf by their emission, which is never read.
//
// Forward (mwer_alpha_kernel): one wave per lattice.  alpha_t[s] includes the emission of frame t; with STORE every frame's
// registers go to the workspace as they are ([lattice][t][lane][P]: a lane reads its states back with one or two vector loads).
// ll = log_add(alpha[S - 2], alpha[S - 1]) after the last frame.  mwer_coef_kernel then forms, per (e, b), the softmax over the
// list, the loss and the coefficients c_i (one thread per list: N <= 16 terms in index order), and mwer_reduce_kernel the batch
// mean in index order.
//
// Backward (mwer_beta_kernel): one workgroup owns an (e, b), wave i its lattice i.  All waves walk the frames downwards together.
// bx_t[s] is the backward variable WITHOUT the emission of frame t, so the state posterior is exp(alpha_t[s] + bx_t[s] - ll) and
// no emission is ever subtracted (an exact -inf log-prob stays harmless).  A wave scatters c_i * posterior into ITS row of V
// floats in LDS: the blank states as one DPP sum, the label states in rounds by the occurrence rank of their label in the
// hypothesis (rank r = r earlier tokens are the same label), so no two work-items of a round meet on an address and a label's
// occurrences are added in position order.  After the frame's barrier wave 0 adds the N rows in index order and stores the
// gradient row as one float4 per lane.  Rows are double-buffered by frame parity: one barrier per frame.  Nothing is atomic and
// no [N, T', V] intermediate exists; a list whose coefficients are all zero (equal risks, N = 1, nothing feasible) walks nothing.
#include <limits.h>
#include <math.h>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"
#include "eec_lexbeam.h"

namespace eec {

constexpr int kMwerMaxN = EEC_MWER_MAX_NBEST;
constexpr int kMwerMaxLen = 255;

__host__ __device__ inline int mwer_states_per_lane(int L) {
  const int len = L < kMwerMaxLen ? L : kMwerMaxLen;
  return 2 * len + 1 <= 128 ? 2 : 2 * len + 1 <= 256 ? 4 : 8;
}

// log(exp(a) + exp(b)) of two values that are no NaN (the kernels keep NaNs out of the recursions: mw_emissions)
__device__ __forceinline__ float mw_la(float a, float b) { return lb_log_add(a, b); }

// A lattice as its wave sees it: the P / 2 tokens of this lane, and which of its label states may be entered from / left to the
// label state two away (the neighbouring token differs).  tok is clamped into [0, V) so that every read it indexes is in bounds.
template <int P>
struct MwLattice {
  int tok[P / 2];
  bool skip_in[P / 2], skip_out[P / 2];
  int len;   // tokens; -1: absent
  bool bad;  // wave-uniform: a length or a label the statement refuses
};

template <int P>
__device__ __forceinline__ MwLattice<P> mw_lattice(const int* __restrict__ hyp_row, int len_raw, int L, int V, int blank, int lane) {
  MwLattice<P> lt;
  const int max_len = L < kMwerMaxLen ? L : kMwerMaxLen;
  lt.bad = len_raw < -1 || len_raw > max_len;
  lt.len = lt.bad ? -1 : len_raw;
  bool wrong = false;
#pragma unroll
  for (int kk = 0; kk < P / 2; ++kk) {
    const int j = lane * (P / 2) + kk;
    int v = j < lt.len ? hyp_row[j] : 0;
    if (j < lt.len && (v < 0 || v >= V || v == blank)) wrong = true, v = 0;
    lt.tok[kk] = v;
  }
  if (__any(wrong)) lt.bad = true, lt.len = -1;
  const int left = __shfl_up(lt.tok[P / 2 - 1], 1, 64), right = __shfl_down(lt.tok[0], 1, 64);
#pragma unroll
  for (int kk = 0; kk < P / 2; ++kk) {
    const int j = lane * (P / 2) + kk;
    const int before = kk > 0 ? lt.tok[kk > 0 ? kk - 1 : 0] : left, after = kk + 1 < P / 2 ? lt.tok[kk + 1 < P / 2 ? kk + 1 : 0] : right;
    lt.skip_in[kk] = j >= 1 && j < lt.len && lt.tok[kk] != before;
    lt.skip_out[kk] = j + 1 < lt.len && lt.tok[kk] != after;
  }
  return lt;
}

// the emissions of one frame for this lane's states: em[k] = logp[t][label of state lane P + k], -inf at and past state S.
// Returns whether one of the values read is a NaN; a NaN is replaced by -inf, so the recursions never see one.
template <int P>
__device__ __forceinline__ bool mw_emissions(const float* __restrict__ row, const MwLattice<P>& lt, int blank, int lane, float (&em)[P]) {
  const int S = 2 * lt.len + 1;
  const float lb = row[blank];
  bool nan = false;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int s = lane * P + k;
    float v = -INFINITY;
    if (s < S) v = (k & 1) ? row[lt.tok[k / 2]] : lb;
    if (v != v) nan = true, v = -INFINITY;
    em[k] = v;
  }
  return nan;
}

__device__ __forceinline__ int mwer_frames(const int* __restrict__ input_len, int b, int Tq) {
  return input_len ? min(max(input_len[b], 0), Tq) : Tq;
}

// register k (wave-uniform) of lane `src`
template <int P>
__device__ __forceinline__ float mw_pick(const float (&a)[P], int k, int src) {
  float r = a[0];
#pragma unroll
  for (int c = 1; c < P; ++c) r = c == k ? a[c] : r;
  return __shfl(r, src, 64);
}

// One wave per lattice g = (e * nb + bb) * N + i of the chunk (utterances b0 .. b0 + nb - 1 of a batch of B).  ll_out is indexed by
// the lattice's place in the WHOLE batch; ws_ll / ws_status / alpha (STORE only) by its place in the chunk.
// status: 0 present, 1 absent, 2 refused (bad length or label; ll = NaN)
template <int P, bool STORE>
__global__ __launch_bounds__(256) void mwer_alpha_kernel(const float* __restrict__ logp, const int* __restrict__ input_len,
                                                         const int* __restrict__ hyp, const int* __restrict__ hyp_len, int B, int b0, int nb,
                                                         int Tq, int V, int N, int L, int blank, int n_lat, float* __restrict__ ll_out,
                                                         float* __restrict__ ws_ll, int* __restrict__ ws_status, float* __restrict__ alpha) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int g = blockIdx.x * 4 + w;
  if (g >= n_lat) return;  // wave-uniform; the kernel has no barrier
  const int i = g % N, eb = g / N, bb = eb % nb, e = eb / nb, b = b0 + bb;
  const size_t gf = ((size_t)e * B + b) * N + i;
  const MwLattice<P> lt = mw_lattice<P>(hyp + gf * L, hyp_len[gf], L, V, blank, lane);
  const int Tb = mwer_frames(input_len, b, Tq);
  float ll = -INFINITY;
  int status = lt.bad ? 2 : lt.len < 0 ? 1 : 0;
  if (status == 0) {
    const int S = 2 * lt.len + 1;
    const float* base = logp + ((size_t)e * B + b) * Tq * V;
    float a[P], em[P], nx[P];
    bool nan = false;
    if (Tb > 0) nan = mw_emissions<P>(base, lt, blank, lane, em);
    for (int t = 0; t < Tb; ++t) {
      if (t + 1 < Tb) nan |= mw_emissions<P>(base + (size_t)(t + 1) * V, lt, blank, lane, nx);  // in flight under this frame's work
      if (t == 0) {
#pragma unroll
        for (int k = 0; k < P; ++k) a[k] = (lane == 0 && k < 2) ? em[k] : -INFINITY;
      } else {
        float left = __shfl_up(a[P - 1], 1, 64);
        left = lane == 0 ? -INFINITY : left;
#pragma unroll
        for (int k = P - 1; k >= 0; --k) {  // downwards: a[k - 1], a[k - 2] are still the previous frame's
          const float l1 = k >= 1 ? a[k >= 1 ? k - 1 : 0] : left;
          float x = mw_la(a[k], l1);
          if (k & 1) {
            const float l2 = k >= 2 ? a[k >= 2 ? k - 2 : 0] : left;
            x = mw_la(x, lt.skip_in[k / 2] ? l2 : -INFINITY);
          }
          a[k] = x + em[k];
        }
      }
      if (STORE) {
        float* at = alpha + (((size_t)g * Tq + t) * 64 + lane) * P;
        if (P == 2) {
          *(float2*)at = make_float2(a[0], a[1]);
        } else {
#pragma unroll
          for (int c = 0; c < P; c += 4) *(float4*)(at + c) = make_float4(a[c], a[c + 1], a[c + 2 < P ? c + 2 : 0], a[c + 3 < P ? c + 3 : 0]);
        }
      }
#pragma unroll
      for (int k = 0; k < P; ++k) em[k] = nx[k];
    }
    if (Tb == 0) {
      ll = lt.len == 0 ? 0.f : -INFINITY;
    } else {
      const float last = mw_pick<P>(a, (S - 1) % P, (S - 1) / P);
      ll = last;
      if (lt.len > 0) ll = mw_la(mw_pick<P>(a, (S - 2) % P, (S - 2) / P), last);
    }
    if (__any(nan)) ll = NAN;
  } else if (status == 2) {
    ll = NAN;
  }
  if (lane == 0) {
    ll_out[gf] = ll;
    if (STORE) ws_ll[g] = ll, ws_status[g] = status;
  }
}

// One work-item per list (e, bb) of the chunk: the softmax over the present, feasible entries, the loss and the coefficients.
__global__ __launch_bounds__(64) void mwer_coef_kernel(const float* __restrict__ ws_ll, const int* __restrict__ ws_status,
                                                       const float* __restrict__ risk, int B, int b0, int nb, int N, int n_lists,
                                                       float* __restrict__ loss_eb, float* __restrict__ ws_c) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_lists) return;
  const int bb = q % nb, e = q / nb;
  const size_t ebf = (size_t)e * B + b0 + bb;
  const float* ll = ws_ll + (size_t)q * N;
  const int* st = ws_status + (size_t)q * N;
  const float* rk = risk + ebf * N;
  float* c = ws_c + (size_t)q * N;
  bool bad = false, nan = false;
  int cnt = 0;
  float m = -INFINITY, rsum = 0.f, rmin = INFINITY, rmax = -INFINITY;
  for (int i = 0; i < N; ++i) {
    const float l = ll[i];
    if (st[i] == 2) bad = true;
    else if (st[i] == 0 && l != l) nan = true;
    else if (st[i] == 0 && l > -INFINITY) {
      const float r = rk[i];
      m = fmaxf(m, l), rsum += r, rmin = fminf(rmin, r), rmax = fmaxf(rmax, r), ++cnt;
    }
  }
  float loss = 0.f;
  if (bad || nan || cnt == 0) {
    // refused input: the NaN stays in the loss; NaN log-probs: the coefficients carry it into the gradient rows of this (e, b)
    loss = (bad || nan) ? NAN : 0.f;
    const float v = (!bad && nan) ? NAN : 0.f;
    for (int i = 0; i < N; ++i) c[i] = v;
  } else {
    const float rbar = rmin == rmax ? rmin : rsum / (float)cnt;  // equal risks: every r_i exactly 0
    float z = 0.f;
    for (int i = 0; i < N; ++i)
      if (st[i] == 0 && ll[i] > -INFINITY) z += expf(ll[i] - m);
    for (int i = 0; i < N; ++i)
      if (st[i] == 0 && ll[i] > -INFINITY) loss += (expf(ll[i] - m) / z) * (rk[i] - rbar);
    // c_i = phat_i (r_i - loss) as phat_i sum_j phat_j (risk_i - risk_j): the same number, without the cancellation that leaves
    // nothing of it when one hypothesis holds nearly all the mass
    for (int i = 0; i < N; ++i) {
      float ci = 0.f;
      if (st[i] == 0 && ll[i] > -INFINITY) {
        for (int j = 0; j < N; ++j)
          if (st[j] == 0 && ll[j] > -INFINITY) ci += (expf(ll[j] - m) / z) * (rk[i] - rk[j]);
        ci *= expf(ll[i] - m) / z;
      }
      c[i] = ci;
    }
  }
  loss_eb[ebf] = loss;
}

// loss[e] = (sum over b in index order of loss_eb[e][b]) / B: one wave per exit
__global__ __launch_bounds__(64) void mwer_reduce_kernel(const float* __restrict__ loss_eb, int B, float* __restrict__ out) {
  const int e = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const float term = b0 + lane < B ? loss_eb[(size_t)e * B + b0 + lane] : 0.f;
    const int n = min(64, B - b0);
    for (int i = 0; i < n; ++i) s += __shfl(term, i, 64);
  }
  if (lane == 0) out[e] = s / (float)B;
}

// dlogp[e][b0 + bb][t][:] (+)= (grad_loss[e] / B) * sum_i c_i * gamma_i[t][:].  Workgroup (e, bb), wave i = lattice i, 64 N threads.
// LDS: rows[2][N][V] floats (dynamic).
template <int P>
__global__ __launch_bounds__(1024) void mwer_beta_kernel(const float* __restrict__ logp, const int* __restrict__ input_len,
                                                         const int* __restrict__ hyp, const int* __restrict__ hyp_len, int B, int b0, int nb,
                                                         int Tq, int V, int N, int L, int blank, const float* __restrict__ alpha,
                                                         const float* __restrict__ ws_ll, const float* __restrict__ ws_c,
                                                         const float* __restrict__ grad_loss, int accumulate, float* __restrict__ dlogp) {
  extern __shared__ float4 mw_rows4[];
  float* rows = (float*)mw_rows4;
  const int lane = threadIdx.x & 63, i = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int q = blockIdx.x, bb = q % nb, e = q / nb, b = b0 + bb;
  const int Tb = mwer_frames(input_len, b, Tq);
  const float wgt = grad_loss[e] / (float)B;
  const int g = q * N + i;
  float* out = dlogp + ((size_t)e * B + b) * Tq * V;
  const int V4 = V / 4, n_thr = 64 * N;

  // what the list asks for: nothing (every weighted coefficient 0), NaN rows, or the walk
  bool any = false, nan = false;
  for (int k = 0; k < N; ++k) {
    const float ck = ws_c[(size_t)q * N + k] * wgt;
    nan |= ck != ck, any |= ck != 0.f;
  }
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const int t_fill = (any || nan) ? Tb : 0;  // rows at and past it are zero rows: written, or left alone when accumulating
  if (!accumulate)
    for (int x = t_fill * V4 + (int)threadIdx.x; x < Tq * V4; x += n_thr) ((float4*)out)[x] = zero;
  if (!(any || nan)) return;  // block-uniform
  if (nan) {
    const float4 f = make_float4(NAN, NAN, NAN, NAN);
    for (int x = threadIdx.x; x < Tb * V4; x += n_thr) ((float4*)out)[x] = f;
    return;
  }

  const float c = ws_c[g] * wgt;  // wave-uniform
  const bool active = c != 0.f;   // then the entry is present and its ll finite
  const size_t gf = ((size_t)e * B + b) * N + i;
  MwLattice<P> lt;
  int rank[P / 2], max_rank = 0;
  float ll = 0.f;
  if (active) {
    lt = mw_lattice<P>(hyp + gf * L, hyp_len[gf], L, V, blank, lane);
    ll = ws_ll[g];
    // rank[kk]: how many earlier tokens of the hypothesis are this token
#pragma unroll
    for (int kk = 0; kk < P / 2; ++kk) rank[kk] = 0;
    const int lanes_used = (lt.len + P / 2 - 1) / (P / 2);
    for (int src = 0; src < lanes_used; ++src) {
#pragma unroll
      for (int k2 = 0; k2 < P / 2; ++k2) {
        const int tk = __shfl(lt.tok[k2], src, 64), jp = src * (P / 2) + k2;
#pragma unroll
        for (int kk = 0; kk < P / 2; ++kk) {
          const int j = lane * (P / 2) + kk;
          if (jp < j && j < lt.len && tk == lt.tok[kk]) ++rank[kk];
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < P / 2; ++kk) max_rank = max(max_rank, rank[kk]);
    max_rank = __builtin_amdgcn_readfirstlane(wave_all_max(max_rank));
  }
  // this wave's two rows start as zeros; an inactive wave never writes them again
  for (int x = lane; x < V4; x += 64) {
    ((float4*)(rows + (size_t)(0 * N + i) * V))[x] = zero;
    ((float4*)(rows + (size_t)(1 * N + i) * V))[x] = zero;
  }

  const float* base = logp + ((size_t)e * B + b) * Tq * V;
  const int S = active ? 2 * lt.len + 1 : 1;
  float bi[P], bx[P], em[P];  // bi: the backward variable of frame t + 1 with its emission
  for (int t = Tb - 1; t >= 0; --t) {
    if (active) {
      float* row = rows + (size_t)((t & 1) * N + i) * V;
      if (t == Tb - 1) {
#pragma unroll
        for (int k = 0; k < P; ++k) {
          const int s = lane * P + k;
          bx[k] = (s == S - 1 || (s == S - 2 && s >= 0)) ? 0.f : -INFINITY;
        }
      } else {
        float r1 = __shfl_down(bi[0], 1, 64), r2 = __shfl_down(bi[1], 1, 64);
        r1 = lane == 63 ? -INFINITY : r1, r2 = lane == 63 ? -INFINITY : r2;
#pragma unroll
        for (int k = 0; k < P; ++k) {
          const float n1 = k + 1 < P ? bi[k + 1 < P ? k + 1 : 0] : r1;
          float x = mw_la(bi[k], n1);
          if (k & 1) {
            const float n2 = k + 2 < P ? bi[k + 2 < P ? k + 2 : 0] : r2;
            x = mw_la(x, lt.skip_out[k / 2] ? n2 : -INFINITY);
          }
          bx[k] = x;
        }
      }
      // the frame's alphas, as the forward left them
      float a[P];
      const float* at = alpha + (((size_t)g * Tq + t) * 64 + lane) * P;
      if (P == 2) {
        const float2 v = *(const float2*)at;
        a[0] = v.x, a[1] = v.y;
      } else {
#pragma unroll
        for (int k = 0; k < P; k += 4) {
          const float4 v = *(const float4*)(at + k);
          a[k] = v.x, a[k + 1] = v.y, a[k + 2 < P ? k + 2 : 0] = v.z, a[k + 3 < P ? k + 3 : 0] = v.w;
        }
      }
      if (t > 0) mw_emissions<P>(base + (size_t)t * V, lt, blank, lane, em);  // for frame t - 1; the forward has seen any NaN
      float val[P], blank_sum = 0.f;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        val[k] = c * expf((a[k] + bx[k]) - ll);
        if (!(k & 1)) blank_sum += val[k];
      }
      blank_sum = wave_sum(blank_sum);
      // the row of frame t: zeros, the blank, then the labels by occurrence rank (scalar accesses throughout: one wave's LDS
      // operations complete in order, and the compiler sees every one of them as a float)
      for (int x = lane; x < V; x += 64) row[x] = 0.f;
      if (lane == 0) row[blank] = blank_sum;
      for (int r = 0; r <= max_rank; ++r) {
#pragma unroll
        for (int kk = 0; kk < P / 2; ++kk) {
          const int j = lane * (P / 2) + kk;
          if (rank[kk] == r && j < lt.len) row[lt.tok[kk]] += val[2 * kk + 1];
        }
      }
      if (t > 0) {
#pragma unroll
        for (int k = 0; k < P; ++k) bi[k] = bx[k] + em[k];
      }
    }
    __syncthreads();  // the N rows of this frame's parity are complete; the other parity is free again
    if (i == 0 && lane < V4) {
      float4 s = ((const float4*)(rows + (size_t)((t & 1) * N) * V))[lane];
      for (int k = 1; k < N; ++k) {
        const float4 v = ((const float4*)(rows + (size_t)((t & 1) * N + k) * V))[lane];
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
      }
      float4* dst = (float4*)(out + (size_t)t * V) + lane;
      if (accumulate) {
        const float4 o = *dst;
        s.x += o.x, s.y += o.y, s.z += o.z, s.w += o.w;
      }
      *dst = s;
    }
  }
}

struct MwerShape {
  int E, B, b0, nb, Tq, V, N, L, blank;
};

static size_t mwer_head_bytes(size_t n_lat) { return eech::up256(n_lat * sizeof(float)); }
static size_t mwer_ws_bytes(int E, int nb, int Tq, int N, int L) {
  if (E <= 0 || nb <= 0 || Tq <= 0 || N <= 0 || L <= 0) return 0;
  const size_t n_lat = (size_t)E * nb * N;
  return 3 * mwer_head_bytes(n_lat) + n_lat * (size_t)Tq * 64 * mwer_states_per_lane(L) * sizeof(float);
}

template <bool STORE>
static hipError_t launch_mwer_alpha(const float* logp, const int* input_len, const int* hyp, const int* hyp_len, const MwerShape& s, float* ll,
                                    float* ws_ll, int* ws_status, float* alpha, hipStream_t st) {
  const int n_lat = s.E * s.nb * s.N;
  const dim3 grid((n_lat + 3) / 4), block(256);
#define EEC_MWER_ALPHA(P_)                                                                                                                  \
  hipLaunchKernelGGL((mwer_alpha_kernel<P_, STORE>), grid, block, 0, st, logp, input_len, hyp, hyp_len, s.B, s.b0, s.nb, s.Tq, s.V, s.N, s.L, \
                     s.blank, n_lat, ll, ws_ll, ws_status, alpha)
  const int P = mwer_states_per_lane(s.L);
  if (P == 2) EEC_MWER_ALPHA(2);
  else if (P == 4) EEC_MWER_ALPHA(4);
  else EEC_MWER_ALPHA(8);
#undef EEC_MWER_ALPHA
  return hipGetLastError();
}

// the checks the three entries share; `what` names the entry
static int mwer_check(const char* what, const void* logp, const void* hyp, const void* hyp_len, int E, int B, int b0, int nb, int Tq, int V,
                      int N, int L, int blank) {
  using eech::fail;
  const std::string w = std::string(what) + ": ";
  if (E < 1 || B < 1 || Tq < 1 || V < 1 || L < 1 || nb < 1)
    return fail(EEC_ERR_BAD_ARG, w + "E, B, nb, T', V and L must be positive, got E " + std::to_string(E) + ", B " + std::to_string(B) + ", nb " +
                                     std::to_string(nb) + ", T' " + std::to_string(Tq) + ", V " + std::to_string(V) + ", L " + std::to_string(L));
  if (N < 1 || N > kMwerMaxN)
    return fail(EEC_ERR_BAD_ARG, w + "N must lie in [1, EEC_MWER_MAX_NBEST = " + std::to_string(kMwerMaxN) + "], got " + std::to_string(N));
  if (b0 < 0 || (long long)b0 + nb > B)
    return fail(EEC_ERR_BAD_ARG, w + "the chunk b0 .. b0 + nb - 1 must lie inside the batch, got b0 " + std::to_string(b0) + ", nb " +
                                     std::to_string(nb) + ", B " + std::to_string(B));
  if (blank < 0 || blank >= V) return fail(EEC_ERR_BAD_ARG, w + "blank must lie in [0, V), got " + std::to_string(blank));
  if (!logp || !hyp || !hyp_len) return fail(EEC_ERR_BAD_ARG, w + "null argument (logp, hyp, hyp_len)");
  if ((long long)E * B * N > INT_MAX / 4 || (long long)E * B * N * L > INT_MAX)
    return fail(EEC_ERR_BAD_ARG, w + "E * B * N * L must stay below 2^31");
  return 0;
}

}  // namespace eec

extern "C" {

size_t eec_ctc_mwer_workspace_bytes(int E, int B, int Tq, int N, int L) { return eec::mwer_ws_bytes(E, B, Tq, N, L); }

int eec_ctc_hyp_logp(const float* logp, const int32_t* input_len, const int32_t* hyp, const int32_t* hyp_len, int E, int B, int Tq, int V, int N,
                     int L, int blank, float* ll, void* stream) {
  using namespace eec;
  if (int rc = mwer_check("eec_ctc_hyp_logp", logp, hyp, hyp_len, E, B, 0, B, Tq, V, N, L, blank)) return rc;
  if (!ll) return eech::fail(EEC_ERR_BAD_ARG, "eec_ctc_hyp_logp: null argument (ll)");
  const MwerShape s{E, B, 0, B, Tq, V, N, L, blank};
  const hipError_t e = launch_mwer_alpha<false>(logp, input_len, hyp, hyp_len, s, ll, nullptr, nullptr, nullptr, (hipStream_t)stream);
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_ctc_hyp_logp launch");
}

int eec_ctc_mwer_forward(const float* logp, const int32_t* input_len, const int32_t* hyp, const int32_t* hyp_len, const float* risk, int E, int B,
                         int b0, int nb, int Tq, int V, int N, int L, int blank, float* ll, float* loss_eb, float* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = mwer_check("eec_ctc_mwer_forward", logp, hyp, hyp_len, E, B, b0, nb, Tq, V, N, L, blank)) return rc;
  if (!risk || !ll || !loss_eb || !loss || !workspace) return fail(EEC_ERR_BAD_ARG, "eec_ctc_mwer_forward: null argument (risk, ll, loss_eb, loss, workspace)");
  if (eech::check_workspace(workspace, workspace_bytes, mwer_ws_bytes(E, nb, Tq, N, L)) != 0)
    return fail(EEC_ERR_WORKSPACE, "eec_ctc_mwer_forward: " + eech::g_err + " (eec_ctc_mwer_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const size_t n_lat = (size_t)E * nb * N, head = mwer_head_bytes(n_lat);
  char* ws = (char*)workspace;
  float *ws_ll = (float*)ws, *ws_c = (float*)(ws + head), *alpha = (float*)(ws + 3 * head);
  int* ws_status = (int*)(ws + 2 * head);
  const MwerShape s{E, B, b0, nb, Tq, V, N, L, blank};
  hipError_t e = launch_mwer_alpha<true>(logp, input_len, hyp, hyp_len, s, ll, ws_ll, ws_status, alpha, st);
  if (e != hipSuccess) return eech::hip_fail(e, "eec_ctc_mwer_forward launch (alpha)");
  const int n_lists = E * nb;
  hipLaunchKernelGGL(mwer_coef_kernel, dim3((n_lists + 63) / 64), dim3(64), 0, st, ws_ll, ws_status, risk, B, b0, nb, N, n_lists, loss_eb, ws_c);
  if ((e = hipGetLastError()) != hipSuccess) return eech::hip_fail(e, "eec_ctc_mwer_forward launch (coefficients)");
  if (b0 + nb == B) {  // the chunk that completes the batch: the means over all of loss_eb
    hipLaunchKernelGGL(mwer_reduce_kernel, dim3(E), dim3(64), 0, st, loss_eb, B, loss);
    if ((e = hipGetLastError()) != hipSuccess) return eech::hip_fail(e, "eec_ctc_mwer_forward launch (reduce)");
  }
  return 0;
}

int eec_ctc_mwer_backward(const float* logp, const int32_t* input_len, const int32_t* hyp, const int32_t* hyp_len, int E, int B, int b0, int nb,
                          int Tq, int V, int N, int L, int blank, const void* workspace, size_t workspace_bytes, const float* grad_loss,
                          int accumulate, float* dlogp, void* stream) {
  using namespace eec;
  using eech::fail;
  if (int rc = mwer_check("eec_ctc_mwer_backward", logp, hyp, hyp_len, E, B, b0, nb, Tq, V, N, L, blank)) return rc;
  if (V > 256 || V % 4)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_mwer_backward: V must be a multiple of 4, <= 256 (a gradient row is one float4 per lane), got " + std::to_string(V));
  if (!workspace || !grad_loss || !dlogp) return fail(EEC_ERR_BAD_ARG, "eec_ctc_mwer_backward: null argument (workspace, grad_loss, dlogp)");
  if ((uintptr_t)dlogp & 15) return fail(EEC_ERR_BAD_ARG, "eec_ctc_mwer_backward: dlogp must be 16-byte aligned (rows leave as float4)");
  if (eech::check_workspace(workspace, workspace_bytes, mwer_ws_bytes(E, nb, Tq, N, L)) != 0)
    return fail(EEC_ERR_WORKSPACE, "eec_ctc_mwer_backward: " + eech::g_err + " (eec_ctc_mwer_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const size_t n_lat = (size_t)E * nb * N, head = mwer_head_bytes(n_lat);
  const char* ws = (const char*)workspace;
  const float *ws_ll = (const float*)ws, *ws_c = (const float*)(ws + head), *alpha = (const float*)(ws + 3 * head);
  const dim3 grid(E * nb), block(64 * N);
  const size_t lds = (size_t)2 * N * V * sizeof(float);
#define EEC_MWER_BETA(P_)                                                                                                                 \
  hipLaunchKernelGGL(mwer_beta_kernel<P_>, grid, block, lds, st, logp, input_len, hyp, hyp_len, B, b0, nb, Tq, V, N, L, blank, alpha, ws_ll, \
                     ws_c, grad_loss, accumulate, dlogp)
  const int P = mwer_states_per_lane(L);
  if (P == 2) EEC_MWER_BETA(2);
  else if (P == 4) EEC_MWER_BETA(4);
  else EEC_MWER_BETA(8);
#undef EEC_MWER_BETA
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_ctc_mwer_backward launch");
}

}  // extern "C"
