// CTC prefix scores for one-pass joint CTC / attention beam search (Watanabe et al. 2017): at every step of the lockstep AED
// search each candidate extension of each live beam is scored by the CTC prefix probability of the extended label sequence, the
// EOS candidate by the full-sequence CTC likelihood.  The semantics -- state, extension, local scores, what happens after the
// selection -- are stated in include/eec.h; tests/ctc_prefix_cases.py is the float64 restatement.
//
// State of a beam slot (floats): [pfx, last, done, 0][psi of every token, 256][rn, T'][rb, T'][u = log_add(rn, rb), T'].  Two
// buffers of n * R_max slots: step s reads the parents from buffer s & 1 and writes the R current beams to the other one, so no
// workgroup reads what another one writes.  Per-candidate states are never stored: psi(g.v) does not depend on the candidate's own
// (nn, nb) -- it is the log-sum over t of phi[t] + x[t][v], and phi[t] is rb[t-1] for v == last, u[t-1] otherwise: two vectors
// of the BEAM.  The psi of every token is kept (V floats), so the chosen candidate's prefix score is the very number that was
// ranked.
//
// One workgroup per (beam, search), one work-item per token.
//   advance: the chosen (parent, token) is extended once: phi / x[t][c] / x[t][blank] of all frames are gathered into LDS by all
//     work-items (off the chain), one work-item walks the T frames (two independent log_adds per frame), all of them then form u
//     and write the slot.  A done parent, EOS and a dead beam copy or fill instead: no chain.
//   score: work-item v walks psi over the frames: {rb, u}[t-1] is one LDS broadcast, x[t][v] a whole row per frame, loaded eight
//     frames ahead of its use.
// Both chains are T dependent log_adds (the exactly stated fp32 sequence of include/eec.h, lb_log_add); nothing else is serial.
// Vector stores only; no atomics; the order of every sum is fixed, so results are bit-identical run to run and independent of n.
#include <math.h>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_lexbeam.h"

namespace eec {

constexpr int kPxMaxR = 16;    // beams per search, as eec_beam_select
constexpr int kPxMaxV = 256;   // one work-item per token
constexpr int kPxMaxT = 2048;  // 24 bytes of LDS per frame: 48 KiB
constexpr int kPxHdr = 4;      // pfx, last, done, 0
constexpr int kPxAhead = 8;    // frames of look-ahead held in registers

__host__ __device__ inline size_t px_slot_floats(int Tq) { return ((size_t)kPxHdr + kPxMaxV + 3 * (size_t)Tq + 3) & ~(size_t)3; }
inline size_t px_state_bytes(int n, int R_max, int Tq) { return 2 * (size_t)n * R_max * px_slot_floats(Tq) * sizeof(float); }

__device__ __forceinline__ int px_frames(const int* em_len, int i, int Tq) {
  const int T = em_len ? em_len[i] : Tq;
  return T < 1 ? 1 : T > Tq ? Tq : T;
}

// the empty hypothesis into slot 0 of buffer 0 of every search
__global__ __launch_bounds__(256) void ctc_prefix_begin_kernel(const float* __restrict__ logp, const int* __restrict__ em_len, int Tq, int V, int blank,
                                                               int R_max, float* __restrict__ state, size_t slot) {
  extern __shared__ __attribute__((aligned(16))) float px_xs[];  // [Tq]
  const int i = blockIdx.x, tid = threadIdx.x;
  const int T = px_frames(em_len, i, Tq);
  const float* em = logp + (size_t)i * Tq * V;
  for (int t = tid; t < T; t += 256) px_xs[t] = em[(size_t)t * V + blank];
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
      acc = t == 0 ? px_xs[0] : acc + px_xs[t];
      px_xs[t] = acc;
    }
  }
  __syncthreads();
  float* sl = state + (size_t)i * R_max * slot;
  float* rn = sl + kPxHdr + kPxMaxV;
  float* rb = rn + Tq;
  float* u = rb + Tq;
  for (int t = tid; t < Tq; t += 256) {
    const float v = t < T ? px_xs[t] : -INFINITY;
    rn[t] = -INFINITY;
    rb[t] = v;
    u[t] = v;  // log_add(-inf, rb)
  }
  sl[kPxHdr + tid] = -INFINITY;
  if (tid == 0) {
    sl[0] = 0.f;
    sl[1] = __int_as_float(-1);
    sl[2] = __int_as_float(0);
    sl[3] = 0.f;
  }
}

enum { kPxCopy = 0, kPxFinish = 1, kPxDead = 2, kPxExtend = 3 };

__global__ __launch_bounds__(256) void ctc_prefix_step_kernel(const float* __restrict__ logp, const int* __restrict__ em_len, int Tq, int V, int blank,
                                                              int R_max, const long long* __restrict__ parent,
                                                              const long long* __restrict__ last_tokens, int R, int R_prev, int s,
                                                              const float* __restrict__ att, float w, int eos, int pad, int min_length,
                                                              float* __restrict__ local_out, const float* __restrict__ src,
                                                              float* __restrict__ dst, size_t slot) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float px_smem[];
  float4* a4 = (float4*)px_smem;               // [Tq]: phi[t], x[t][c], x[t][blank] of the advance
  float2* nb2 = (float2*)(px_smem + 4 * (size_t)Tq);  // [Tq]: (nn, nb) of the advance, then (rb, u) of the current beam
  const int r = blockIdx.x, i = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int T = px_frames(em_len, i, Tq);
  const float* em = logp + (size_t)i * Tq * V;

  int p = 0, c = -1;
  if (s > 0) {
    const long long pl = parent ? parent[(size_t)i * R + r] : (long long)r;
    const long long cl = last_tokens[(size_t)i * R + r];
    p = (pl < 0 || pl >= R_prev) ? -1 : (int)pl;
    c = (cl < 0 || cl >= V) ? -1 : (int)cl;
  }
  const float* ps = src + ((size_t)i * R_max + (p < 0 ? 0 : p)) * slot;
  float* ds = dst + ((size_t)i * R_max + r) * slot;
  const float p_pfx = ps[0];
  const int p_last = __float_as_int(ps[1]), p_done = __float_as_int(ps[2]);
  const float* p_rn = ps + kPxHdr + kPxMaxV;
  const float* p_rb = p_rn + Tq;
  const float* p_u = p_rb + Tq;
  float* d_rn = ds + kPxHdr + kPxMaxV;
  float* d_rb = d_rn + Tq;
  float* d_u = d_rb + Tq;

  int mode;
  float pfx = p_pfx;
  int last = p_last, done = p_done;
  if (p < 0 || (s > 0 && !p_done && c < 0)) {  // an index outside its range is never used as an address: the beam is dead
    mode = kPxDead, pfx = -INFINITY, last = -1, done = 0;
  } else if (s == 0 || p_done) {
    mode = kPxCopy;
  } else if (c == eos) {
    mode = kPxFinish, pfx = p_u[T - 1], done = 1;
  } else {
    pfx = c == blank ? -INFINITY : ps[kPxHdr + c];
    last = c;
    mode = pfx == -INFINITY ? kPxDead : kPxExtend;
  }

  if (mode == kPxExtend) {
    const bool same = c == p_last;
    for (int t = tid; t < T; t += nt) {
      const float phi = t == 0 ? -INFINITY : same ? p_rb[t - 1] : p_u[t - 1];
      a4[t] = make_float4(phi, em[(size_t)t * V + c], em[(size_t)t * V + blank], 0.f);
    }
    __syncthreads();
    if (tid == 0) {
      float nn = p_last < 0 ? a4[0].y : -INFINITY, nb = -INFINITY;
      nb2[0] = make_float2(nn, nb);
      for (int t0 = 1; t0 < T; t0 += kPxAhead) {
        float4 f[kPxAhead];
#pragma unroll
        for (int k = 0; k < kPxAhead; ++k) f[k] = a4[min(t0 + k, T - 1)];
#pragma unroll
        for (int k = 0; k < kPxAhead; ++k) {
          if (t0 + k >= T) break;
          const float n1 = lb_log_add(nn, f[k].x) + f[k].y;
          const float b1 = lb_log_add(nn, nb) + f[k].z;
          nn = n1, nb = b1;
          nb2[t0 + k] = make_float2(nn, nb);
        }
      }
    }
    __syncthreads();
    for (int t = tid; t < Tq; t += nt) {
      float n1 = -INFINITY, b1 = -INFINITY, u1 = -INFINITY;
      if (t < T) {
        const float2 v = nb2[t];
        n1 = v.x, b1 = v.y, u1 = lb_log_add(n1, b1);
      }
      d_rn[t] = n1, d_rb[t] = b1, d_u[t] = u1;
      nb2[t] = make_float2(b1, u1);
    }
  } else if (mode == kPxDead) {
    for (int t = tid; t < Tq; t += nt) {
      d_rn[t] = -INFINITY, d_rb[t] = -INFINITY, d_u[t] = -INFINITY;
      nb2[t] = make_float2(-INFINITY, -INFINITY);
    }
  } else {
    for (int t = tid; t < Tq; t += nt) {
      const float b1 = p_rb[t], u1 = p_u[t];
      d_rn[t] = p_rn[t], d_rb[t] = b1, d_u[t] = u1;
      nb2[t] = make_float2(b1, u1);
    }
  }
  if (tid == 0) {
    ds[0] = pfx;
    ds[1] = __int_as_float(last);
    ds[2] = __int_as_float(done);
    ds[3] = 0.f;
  }
  __syncthreads();

  // the local scores of the current beam: work-item v scores token v
  const int v = tid;
  if (v >= V) return;
  const size_t at = ((size_t)i * R + r) * V + v;
  if (done || pfx == -INFINITY) {
    ds[kPxHdr + v] = -INFINITY;
    local_out[at] = (done && v == pad) ? 0.f : -INFINITY;
    return;
  }
  const bool same = v == last;
  float psi = last < 0 ? em[v] : -INFINITY;
  float x[kPxAhead];
#pragma unroll
  for (int k = 0; k < kPxAhead; ++k) x[k] = em[(size_t)min(1 + k, T - 1) * V + v];
  for (int t0 = 1; t0 < T; t0 += kPxAhead) {
#pragma unroll
    for (int k = 0; k < kPxAhead; ++k) {
      const int t = t0 + k;
      const float xv = x[k];
      x[k] = em[(size_t)min(t + kPxAhead, T - 1) * V + v];
      if (t < T) {
        const float2 f = nb2[t - 1];
        psi = lb_log_add(psi, (same ? f.x : f.y) + xv);
      }
    }
  }
  ds[kPxHdr + v] = psi;
  float ctc = psi - pfx;
  if (v == eos) ctc = s < min_length ? -INFINITY : nb2[T - 1].y - pfx;
  if (v == blank) ctc = -INFINITY;
  float out = -INFINITY;
  if (ctc != -INFINITY) {
    const float a = (1.f - w) * att[at];
    const float b = w * ctc;
    out = a + b;
    if (!(out == out)) out = -INFINITY;  // a non-finite attention score: never a NaN
  }
  local_out[at] = out;
}

static int px_check(const char* who, const float* logp, int n, int Tq, int V, int blank, int R_max, const void* state, size_t state_bytes) {
  using eech::fail;
  const std::string me(who);
  if (n < 0 || Tq < 1 || V < 2 || blank < 0 || blank >= V || R_max < 1)
    return fail(EEC_ERR_BAD_ARG, me + ": needs n >= 0, T' >= 1, V >= 2, blank in [0, V) and R_max >= 1");
  if (V > kPxMaxV || R_max > kPxMaxR || Tq > kPxMaxT)
    return fail(EEC_ERR_UNSUPPORTED, me + ": V <= " + std::to_string(kPxMaxV) + ", R_max <= " + std::to_string(kPxMaxR) + " and T' <= " +
                                         std::to_string(kPxMaxT));
  if (n == 0) return 0;
  if (!logp || !state) return fail(EEC_ERR_BAD_ARG, me + ": null argument (logp, state)");
  if (((uintptr_t)state & 15) != 0) return fail(EEC_ERR_WORKSPACE, me + ": state must be 16-byte aligned");
  if (state_bytes < px_state_bytes(n, R_max, Tq)) return fail(EEC_ERR_WORKSPACE, me + ": state buffer too small (eec_ctc_prefix_state_bytes)");
  return 0;
}

}  // namespace eec

extern "C" {

size_t eec_ctc_prefix_state_bytes(int n, int R_max, int Tq) {
  if (n <= 0 || R_max <= 0 || Tq <= 0) return 0;
  return eec::px_state_bytes(n, R_max, Tq);
}

int eec_ctc_prefix_begin(const float* logp, const int32_t* em_len, int n, int Tq, int V, int blank, int R_max, void* state, size_t state_bytes,
                         void* stream) {
  if (int rc = eec::px_check("eec_ctc_prefix_begin", logp, n, Tq, V, blank, R_max, state, state_bytes)) return rc;
  if (n == 0) return 0;
  hipLaunchKernelGGL(eec::ctc_prefix_begin_kernel, dim3(n), dim3(256), (size_t)Tq * sizeof(float), (hipStream_t)stream, logp, em_len, Tq, V, blank,
                     R_max, (float*)state, eec::px_slot_floats(Tq));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_ctc_prefix_begin launch");
}

int eec_ctc_prefix_step(const float* logp, const int32_t* em_len, int n, int Tq, int V, int blank, int R_max, const int64_t* parent,
                        const int64_t* last_tokens, int R, int R_prev, int s, const float* att, float w, int eos, int pad, int min_length,
                        float* local_out, void* state, size_t state_bytes, void* stream) {
  using eech::fail;
  if (int rc = eec::px_check("eec_ctc_prefix_step", logp, n, Tq, V, blank, R_max, state, state_bytes)) return rc;
  if (eos < 0 || eos >= V || pad < 0 || pad >= V || eos == pad || eos == blank || pad == blank)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_prefix_step: eos and pad in [0, V); blank, eos and pad pairwise distinct");
  if (R < 1 || R > R_max || s < 0 || (s > 0 && (R_prev < 1 || R_prev > R_max)))
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_prefix_step: 1 <= R, R_prev <= R_max and s >= 0");
  if (!(w > 0.f && w <= 1.f)) return fail(EEC_ERR_BAD_ARG, "eec_ctc_prefix_step: the CTC weight must be in (0, 1]");
  if (n == 0) return 0;
  if (!last_tokens || !att || !local_out) return fail(EEC_ERR_BAD_ARG, "eec_ctc_prefix_step: null argument (last_tokens, att, local_out)");
  const size_t slot = eec::px_slot_floats(Tq);
  float* base = (float*)state;
  const size_t half = (size_t)n * R_max * slot;
  const float* src = base + (size_t)(s & 1) * half;
  float* dst = base + (size_t)((s + 1) & 1) * half;
  const int threads = (V + 63) / 64 * 64;
  hipLaunchKernelGGL(eec::ctc_prefix_step_kernel, dim3(R, n), dim3(threads), (size_t)Tq * 24, (hipStream_t)stream, logp, em_len, Tq, V, blank, R_max,
                     (const long long*)parent, (const long long*)last_tokens, R, R_prev, s, att, w, eos, pad, min_length, local_out, src, dst, slot);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_ctc_prefix_step launch");
}

}  // extern "C"
