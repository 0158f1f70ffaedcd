// CTC posteriors in the standard topology (include/eec.h, "CTC posteriors, standard topology"): the forward-backward occupancy of
// the 2N + 1 states blank, y_0, blank, y_1, ..., blank of a token row over one emission, and what a caller reads off it per token:
// the expected number of frames, the posterior-weighted emission, the expected first and last frame with their variances, the
// occupancy itself, and the row's sum-over-paths log-likelihood.  The statement -- the recursions, the fold order of log_add, the
// order of every fp32 operation, the status -- is the header's; this file is its layout on the device.
//
// One launch, no atomics, no barrier, no LDS, nothing read back.  One wave per row on the state strips of eec_ctc_strip.h, which
// also holds the row checks, the strip's labels, frame 0 and the end read.
//   Forward.  alpha in registers.  Every frame's strip goes to the WORKSPACE as C coalesced 256-byte lines (line t * C + k holds
//     slot k of all 64 lanes), so a row of T frames costs T * C lines and eec_ctc_posteriors_workspace_bytes is
//     n_hyp * T' * C(tok_stride) * 256.  A lane later reads only what it stored itself.
//   Backward.  beta in registers; what crosses a lane boundary are the right neighbour's slots 0 and 1 (s + 1 and s + 2 of the last
//     slot), two DPP wave shifts.  At frame t the lane has beta_t of its strip, reads alpha_t (carried: it was alpha_{t-1} one
//     step earlier; at T - 1 it is still in the forward's registers) and alpha_{t-1} (its own lines), and adds the frame's terms to
//     the six fp64 sums of each of its label states: at most four label states per lane, 48 registers.  No value is reduced across
//     lanes: a state's sums live where the state lives and leave once, rounded to fp32.
//   Loads.  The gathers x[t][lab(s)] of the strip's labels, x[t][blank] and, backward, the lines of alpha_{t-1} are issued
//     kPoAheadF / kPoAheadB frames before their use into a register queue that advances by one frame per frame; the frame loop is
//     not unrolled over the queue (a frame is 12 to 20 inlined log_adds at C = 8: unrolled copies would not fit the instruction
//     cache).
// A row the device cannot serve (the header's status 1) gets the fill values.
#include "../../include/eec.h"
#include "eec_ctc_strip.h"
#include "eec_kernels.h"
#include "eec_lexbeam.h"

namespace eec {

constexpr int kPoAheadF = 8;  // frames of look-ahead held in registers, forward (NL + 1 values each)
constexpr int kPoAheadB = 4;  // ... and backward (NL + 1 + C values each)

struct PoOut {
  float* row_logp;  // [1]
  float* frames;    // [tok_stride] each, down to end_var
  float* score;
  float* start;
  float* end;
  float* start_var;
  float* end_var;
  float* gamma;     // [Tq][tok_stride], or null
  int* status;      // [1]
};

// the fill values of a row with status 1 or 2
__device__ __forceinline__ void po_fill(const PoOut& o, int Tq, int tok_stride, int lane, int code) {
  for (int j = lane; j < tok_stride; j += 64)
    o.frames[j] = -1.f, o.score[j] = -1.f, o.start[j] = -1.f, o.end[j] = -1.f, o.start_var[j] = -1.f, o.end_var[j] = -1.f;
  if (o.gamma)
    for (size_t k = lane; k < (size_t)Tq * tok_stride; k += 64) o.gamma[k] = 0.f;
  if (lane == 0) *o.row_logp = -INFINITY, *o.status = code;
}

// One row that passed the row checks (1 <= N <= tok_stride tokens, all of them labels of [0, V); N + R <= T <= Tq) on one wave, C
// states per lane.  al: the row's alpha lines, [T * C][64] floats.
template <int C>
__device__ __forceinline__ void po_row(const float* __restrict__ em, int T, int Tq, int V, int blank, int N, int tok_stride,
                                       const int* __restrict__ tk, int lane, float* __restrict__ al, const PoOut& o) {
  constexpr int NL = strip_labels(C);
  constexpr float NEG = -INFINITY;
  int id[NL];                      // the strip's labels; the states past 2N are held at -inf backward
  bool own[NL], skip[NL], skipn[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const StripLabel l = strip_label<C>(tk, N, blank, lane, i);
    id[i] = l.id, own[i] = l.own, skip[i] = l.skip, skipn[i] = l.skipn;
  }

  // ---- forward ---------------------------------------------------------------------------------------------------------------------
  float a[C];
  strip_frame0<C>(a, em, blank, id[0], lane);
#pragma unroll
  for (int k = 0; k < C; ++k) al[(size_t)k * 64 + lane] = a[k];
  {
    float rg[kPoAheadF][NL], rb[kPoAheadF];  // x[t][label] and (C >= 2) x[t][blank]; slot u: frame t + u
#pragma unroll
    for (int u = 0; u < kPoAheadF; ++u) {
      const float* row = em + (size_t)min(1 + u, T - 1) * V;
#pragma unroll
      for (int i = 0; i < NL; ++i) rg[u][i] = row[id[i]];
      rb[u] = C >= 2 ? row[blank] : 0.f;
    }
    for (int t = 1; t < T; ++t) {
      float g[NL];
#pragma unroll
      for (int i = 0; i < NL; ++i) g[i] = rg[0][i];
      const float xb = rb[0];
#pragma unroll
      for (int u = 0; u + 1 < kPoAheadF; ++u) {
#pragma unroll
        for (int i = 0; i < NL; ++i) rg[u][i] = rg[u + 1][i];
        rb[u] = rb[u + 1];
      }
      {  // the queue's last slot: frame t + kPoAheadF (past the end: the last frame again, unused)
        const float* row = em + (size_t)min(t + kPoAheadF, T - 1) * V;
#pragma unroll
        for (int i = 0; i < NL; ++i) rg[kPoAheadF - 1][i] = row[id[i]];
        if (C >= 2) rb[kPoAheadF - 1] = row[blank];
      }
      // the fold in the statement's order: stay, step, skip
      if (C == 1) {
        const float p1 = from_left(a[0], NEG), p2 = from_left(p1, NEG);
        float v = lb_log_add(a[0], p1);
        v = lb_log_add(v, skip[0] ? p2 : NEG);
        a[0] = v + g[0];
      } else {
        const float left = from_left(a[C - 1], NEG);
        static_range<0, C>([&](auto tag) {  // descending: a[k - 1] and a[k - 2] are still the previous frame's
          constexpr int k = C - 1 - decltype(tag)::value;
          float v = lb_log_add(a[k], k >= 1 ? a[k >= 1 ? k - 1 : 0] : left);
          if (k & 1) {
            const float two = k >= 2 ? a[k >= 2 ? k - 2 : 0] : left;
            v = lb_log_add(v, skip[k >> 1] ? two : NEG);
          }
          a[k] = v + ((k & 1) ? g[k >> 1] : xb);
        });
      }
#pragma unroll
      for (int k = 0; k < C; ++k) al[((size_t)t * C + k) * 64 + lane] = a[k];
    }
  }

  const int sN = 2 * N;
  float hi, lo;
  strip_end<C>(a, N, hi, lo);
  const float ll = lb_log_add(hi, lo);
  if (!(fabsf(ll) < INFINITY)) {  // no path of finite mass (or a NaN)
    po_fill(o, Tq, tok_stride, lane, 2);
    return;
  }

  // ---- backward --------------------------------------------------------------------------------------------------------------------
  // gamma: the strip's stores below cover tokens 0 .. covered - 1 of the frames 0 .. T - 1; the rest is zero
  const int covered = min(C == 1 ? 32 : 64 * NL, tok_stride);
  const bool vec = NL >= 2 && o.gamma && tok_stride % NL == 0 && ((uintptr_t)o.gamma & 15) == 0;  // a lane's NL floats as one store
  if (o.gamma) {
    for (int t = 0; t < T; ++t)
      for (int j = covered + lane; j < tok_stride; j += 64) o.gamma[(size_t)t * tok_stride + j] = 0.f;
    for (size_t k = (size_t)T * tok_stride + lane; k < (size_t)Tq * tok_stride; k += 64) o.gamma[k] = 0.f;
  }

  float b[C];
  bool valid[C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int s = lane * C + k;
    valid[k] = s <= sN;
    b[k] = (s == sN || s == sN - 1) ? 0.f : NEG;
  }
  float lq[NL];       // log_add(c_{t+1}(s + 1), [skip(s + 2)] c_{t+1}(s + 2)) of the label slot: what leaves it after frame t
  double acc[NL][6];  // frames, score, sum t f, sum t^2 f, sum (t + 1) l, sum (t + 1)^2 l
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    lq[i] = NEG;
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[i][q] = 0.0;
  }
  float rg[kPoAheadB][NL], rb[kPoAheadB], rp[kPoAheadB][C];  // x[t][label], x[t][blank], alpha_{t-1}; slot u: frame t - u
#pragma unroll
  for (int u = 0; u < kPoAheadB; ++u) {
    const int tt = max(T - 1 - u, 0);
    const float* row = em + (size_t)tt * V;
#pragma unroll
    for (int i = 0; i < NL; ++i) rg[u][i] = row[id[i]];
    rb[u] = C >= 2 ? row[blank] : 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) rp[u][k] = al[((size_t)max(tt - 1, 0) * C + k) * 64 + lane];
  }
  for (int t = T - 1; t >= 0; --t) {
    float g[NL], ap[C];
#pragma unroll
    for (int i = 0; i < NL; ++i) g[i] = rg[0][i];
    const float xb = rb[0];
#pragma unroll
    for (int k = 0; k < C; ++k) ap[k] = rp[0][k];
#pragma unroll
    for (int u = 0; u + 1 < kPoAheadB; ++u) {
#pragma unroll
      for (int i = 0; i < NL; ++i) rg[u][i] = rg[u + 1][i];
      rb[u] = rb[u + 1];
#pragma unroll
      for (int k = 0; k < C; ++k) rp[u][k] = rp[u + 1][k];
    }
    {  // the queue's last slot: frame t - kPoAheadB (before the start: frame 0 again, unused)
      const int tt = max(t - kPoAheadB, 0);
      const float* row = em + (size_t)tt * V;
#pragma unroll
      for (int i = 0; i < NL; ++i) rg[kPoAheadB - 1][i] = row[id[i]];
      if (C >= 2) rb[kPoAheadB - 1] = row[blank];
#pragma unroll
      for (int k = 0; k < C; ++k) rp[kPoAheadB - 1][k] = al[((size_t)max(tt - 1, 0) * C + k) * 64 + lane];
    }

    // the frame's posteriors of the label slots
    const float pl1 = from_left(ap[C - 1], NEG);                // alpha_{t-1}: C >= 2: s - 2 of slot 1; C == 1: s - 1
    const float pl2 = C == 1 ? from_left(pl1, NEG) : NEG;       // C == 1: s - 2
    const double td = (double)t, te = (double)(t + 1);
    float gam[NL];
    static_range<0, NL>([&](auto tag) {
      constexpr int i = decltype(tag)::value;
      constexpr int k = C == 1 ? 0 : 2 * i + 1;
      gam[i] = expf((a[k] + b[k]) - ll);
      float fv, lv;
      if (t >= 1) {
        const float one = C == 1 ? pl1 : ap[k >= 1 ? k - 1 : 0];
        const float two = C == 1 ? pl2 : k >= 2 ? ap[k >= 2 ? k - 2 : 0] : pl1;
        const float pre = lb_log_add(one, skip[i] ? two : NEG);
        fv = expf(((pre + g[i]) + b[k]) - ll);
      } else {
        fv = (C == 1 ? lane == 1 : lane == 0 && i == 0) ? gam[i] : 0.f;
      }
      lv = t < T - 1 ? expf((a[k] + lq[i]) - ll) : gam[i];
      const double dg = (double)gam[i], df = (double)fv, dl = (double)lv;
      acc[i][0] += dg;
      acc[i][1] += gam[i] > 0.f ? dg * (double)g[i] : 0.0;
      acc[i][2] += td * df;
      acc[i][3] += td * td * df;
      acc[i][4] += te * dl;
      acc[i][5] += te * te * dl;
      if (!own[i]) gam[i] = 0.f;
    });
    if (o.gamma) {
      float* row = o.gamma + (size_t)t * tok_stride;
      if (C == 1) {
        if ((lane & 1) && (lane >> 1) < covered) row[lane >> 1] = gam[0];
      } else {
        bool stored = false;
        if constexpr (NL >= 2) {
          if (vec) {  // covered is a multiple of NL here: a lane's floats are all inside or all outside
            if (lane * NL < covered) {
              typedef float vec_t __attribute__((ext_vector_type(NL)));
              vec_t v;
#pragma unroll
              for (int i = 0; i < NL; ++i) v[i] = gam[i];
              *(vec_t*)(row + lane * NL) = v;
            }
            stored = true;
          }
        }
        if (!stored) {
#pragma unroll
          for (int i = 0; i < NL; ++i)
            if (lane * NL + i < covered) row[lane * NL + i] = gam[i];
        }
      }
    }
    if (t == 0) break;

    // beta_{t-1} from c(s) = x_t(lab(s)) + beta_t(s), in the statement's order: stay, step, skip
    float c[C];
#pragma unroll
    for (int k = 0; k < C; ++k) c[k] = valid[k] ? ((C == 1 || (k & 1)) ? g[k >> 1] : xb) + b[k] : NEG;
    const float r1 = from_right(c[0], NEG);                           // s + 1 of the last slot
    const float r2 = C == 1 ? from_right(r1, NEG) : from_right(c[C > 1 ? 1 : 0], NEG);  // s + 2 of the last slot
    if (C == 1) {
      const float two = skipn[0] ? r2 : NEG;
      b[0] = lb_log_add(lb_log_add(c[0], r1), two);
      lq[0] = lb_log_add(r1, two);
    } else {
      static_range<0, C>([&](auto tag) {
        constexpr int k = decltype(tag)::value;
        const float step = k + 1 < C ? c[k + 1 < C ? k + 1 : 0] : r1;
        float v = lb_log_add(c[k], step);
        if (k & 1) {
          const float far = k + 2 < C ? c[k + 2 < C ? k + 2 : 0] : r2;
          const float two = skipn[k >> 1] ? far : NEG;
          v = lb_log_add(v, two);
          lq[k >> 1] = lb_log_add(step, two);
        }
        b[k] = v;
      });
    }
#pragma unroll
    for (int k = 0; k < C; ++k) a[k] = ap[k];
  }

  // the sums leave, rounded once
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int j = C == 1 ? lane >> 1 : lane * NL + i;
    if (own[i]) {
      o.frames[j] = (float)acc[i][0];
      o.score[j] = (float)acc[i][1];
      o.start[j] = (float)acc[i][2];
      o.end[j] = (float)acc[i][4];
      o.start_var[j] = (float)(acc[i][3] - acc[i][2] * acc[i][2]);
      o.end_var[j] = (float)(acc[i][5] - acc[i][4] * acc[i][4]);
    }
  }
  for (int j = N + lane; j < tok_stride; j += 64)
    o.frames[j] = -1.f, o.score[j] = -1.f, o.start[j] = -1.f, o.end[j] = -1.f, o.start_var[j] = -1.f, o.end_var[j] = -1.f;
  if (lane == 0) *o.row_logp = ll, *o.status = 0;
}

__global__ __launch_bounds__(64 * kStripWaves) void ctc_posterior_kernel(
    const float* __restrict__ logp, int n_em, int Tq, int V, const int* __restrict__ em_len, const int* __restrict__ tokens,
    const int* __restrict__ tok_len, const int* __restrict__ em_index, int n_hyp, int tok_stride, int blank, float* __restrict__ row_logp,
    float* __restrict__ tok_frames, float* __restrict__ tok_score, float* __restrict__ tok_start, float* __restrict__ tok_end,
    float* __restrict__ tok_start_var, float* __restrict__ tok_end_var, float* __restrict__ gamma, int* __restrict__ status,
    float* __restrict__ ws, size_t hyp_floats) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int h = blockIdx.x * kStripWaves + w;
  if (h >= n_hyp) return;  // wave-uniform; the kernel has no barrier
  const size_t at = (size_t)h * tok_stride;
  const PoOut o{row_logp + h,       tok_frames + at,  tok_score + at,
                tok_start + at,     tok_end + at,     tok_start_var + at,
                tok_end_var + at,   gamma ? gamma + (size_t)h * Tq * tok_stride : nullptr,
                status + h};
  const int* tk = tokens + at;
  const auto [N, T, ei, ok] = strip_row(tk, tok_len, em_index, em_len, h, n_em, Tq, V, tok_stride, blank, lane);
  if (!ok) {  // the fill values
    po_fill(o, Tq, tok_stride, lane, 1);
    return;
  }
  const float* em = logp + (size_t)ei * Tq * V;
  float* al = ws + (size_t)h * hyp_floats;
  switch (strip_states(N)) {
    case 1: po_row<1>(em, T, Tq, V, blank, N, tok_stride, tk, lane, al, o); break;
    case 2: po_row<2>(em, T, Tq, V, blank, N, tok_stride, tk, lane, al, o); break;
    case 4: po_row<4>(em, T, Tq, V, blank, N, tok_stride, tk, lane, al, o); break;
    default: po_row<8>(em, T, Tq, V, blank, N, tok_stride, tk, lane, al, o); break;
  }
}

}  // namespace eec

extern "C" {

size_t eec_ctc_posteriors_workspace_bytes(int n_hyp, int Tq, int tok_stride) {
  if (n_hyp < 1 || Tq < 1 || tok_stride < 1) return 0;
  return (size_t)n_hyp * Tq * eec::strip_states(tok_stride) * 64 * sizeof(float);  // the alpha lines
}

int eec_ctc_posteriors(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                       const int32_t* em_index, int n_hyp, int tok_stride, int blank, float* row_logp, float* tok_frames, float* tok_score,
                       float* tok_start, float* tok_end, float* tok_start_var, float* tok_end_var, float* gamma, int32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = eech::strip_entry_head(
      "eec_ctc_posteriors", {logp, tokens, tok_len, row_logp, tok_frames, tok_score, tok_start, tok_end, tok_start_var, tok_end_var, status},
      n_em, Tq, V, n_hyp, tok_stride, blank, workspace, workspace_bytes, eec_ctc_posteriors_workspace_bytes(n_hyp, Tq, tok_stride));
  if (rc || n_hyp == 0) return rc;
  const size_t hyp_floats = (size_t)Tq * eec::strip_states(tok_stride) * 64;
  hipLaunchKernelGGL(eec::ctc_posterior_kernel, dim3((n_hyp + eec::kStripWaves - 1) / eec::kStripWaves), dim3(64 * eec::kStripWaves), 0,
                     (hipStream_t)stream, logp, n_em, Tq, V, em_len, tokens, tok_len, em_index, n_hyp, tok_stride, blank, row_logp, tok_frames,
                     tok_score, tok_start, tok_end, tok_start_var, tok_end_var, gamma, status, (float*)workspace, hyp_floats);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
