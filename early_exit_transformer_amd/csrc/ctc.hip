// Summed per-exit CTC loss, forward (reference train.py:53-65,259):
//   loss_e = mean_b( CTC(logp[e, b], targets[b, :len_b]) / max(len_b, 1) ),  blank = 0,
//   input length = T' for every utterance, zero_infinity=True;  train.py sums loss_e over exits.
// All E*B lattices run in ONE launch, the extended label sequence (2*len+1 states, <= 8 per lane) in registers.  Two entries:
//   the loss alone (eec_ctc_loss, the benchmarked step): ctc_loss_kernel, then ctc_reduce_kernel.  Two waves per lattice walk
//     it from both ends in the WIDE format (one exponent per state: no range limit) and meet in the middle; see the kernel.
//   the training forward (eec_ctc_loss_forward): ctc_alpha_kernel, which stores what the backward pass needs, then
//     ctc_loss_kernel on the lattices it marked (RANGE below), then ctc_reduce_kernel.
// ctc_alpha_kernel: one wave per lattice.  The time recursion is latency-bound (T' serial
// steps), so it runs in a BLOCK-FLOATING linear domain instead of log space:
//   a_t[s] = ( a_{t-1}[s] + a_{t-1}[s-1] + [a_{t-1}[s-2]] ) * p_t(l'_s),   p = exp(logp)
// Each lane keeps its states as fp32 mantissas times a lane-private power of two 2^e (renormalised
// every 2 steps from the lane's own maximum: exact, no log); the two states taken from the previous
// lane arrive with that lane's exponent and both sides are brought to the larger one.  Dynamic range
// ACROSS lanes is therefore unbounded -- necessary, because dead-end prefixes (e.g. "all blank so
// far") can be 1e60 times more probable than the states that will reach the end -- while the
// dependent chain per step is 3 DPP lane shifts, a few ldexp, 2 adds and 1 multiply.  The emission
// log-probs are gathered kCtcAhead steps ahead (their exp is independent of the alpha chain).
//
// RANGE.  A lane's states share one exponent and a lane is renormalised every second step, so a state more than 2^-126 below
// its lane's scale -- two emissions below e^-44 between two renormalisations, an emission below the range of exp, a state far
// behind its lane's maximum, a lane far below the one it receives from -- leaves the fp32 range and its mass is lost.  Whether
// that mass mattered cannot be told where it is lost (it does whenever the flushed states carry the only, or the best, way to
// the end: peaky log-probs with long or improbable targets), so both recursions WATCH for it: a value that is non-zero
// before a product or an alignment and below kCtcTiny after it is an EVENT at the step's common scale 2^ec, i.e. at most
// kCtcTiny * 2^ec of probability mass is gone.  Log-probs are <= 0, so what a state's mass can still add to p(target) (its
// beta') and what a beta' can still meet (its alpha) are probabilities <= 1: all events together take at most
// N * kCtcTiny * 2^(largest ec) from p(target), N = number of (state, step) pairs.  Where that is below 2^-26 of p(target)
// the events are harmless (trailing states of a peaky lattice; the usual case); otherwise the lattice is MARKED and run again
// in the wide format, the same recursion with one exponent per STATE (no range limit, a renormalisation per step): its loss by
// ctc_loss_kernel, its posteriors by ctc_wide_kernel.  The fast path's own arithmetic is unchanged: the watch is compares only.
// The bound is sufficient, not sharp: random log-probs with |log-prob| of 10 and more over 256 frames mark most lattices, which
// is why the loss alone does not take this path at all.
//
// INPUT LENGTHS (eec_len.h: this file is compiled a second time, with EEC_CTC_LEN, by ctc_len.hip, for eec_ctc_loss_len and its
// forward / backward pair).  Every lattice of utterance b then has Tb = clamp(input_len[b], 0, T') frames: the recursions cover
// t < Tb, their look-ahead is clamped to Tb - 1, so no frame at or past Tb is ever read, and ctc_grad_kernel writes zeros to the
// rows t >= Tb.  Tb = 0: nll is 0 for an empty target and +inf for any other (zeroed by the reduction).  Strides and the `astore`
// layout stay on T', and so does ctc_watch_slack(T'): N of RANGE only shrinks with Tb.
#include <limits.h>

#include "eec_kernels.h"
#include "eec_len.h"

namespace eec {

constexpr int kCtcPerLane = 8;  // up to 512 states = target length <= 255
constexpr int kCtcEmpty = -(1 << 20);  // exponent of a lane that holds no probability mass yet
constexpr float kCtcTiny = 7.52316385e-37f;  // 2^-120: a non-zero value that falls below it may have lost bits (fp32 normals end at 2^-126)
// markers of a lattice the fast path gave up on: nll = -inf after ctc_alpha_kernel (replaced by ctc_loss_kernel before the
// reduction), p(target) slot < 0 for the backward pass
constexpr float kCtcRedo = -1.f;
// events at scale 2^ec are harmless when ec <= exponent(p(target)) + ctc_watch_slack: -120 (kCtcTiny) + log2 N + 26 <= 0
__host__ __device__ inline int ctc_watch_slack(int Tq) {
  int lg = 0;
  while (((long long)Tq * 2048) >> lg) ++lg;  // N < Tq * 2048 >= Tq * 4 * 512 states
  return 120 - 26 - lg;
}

#define EEC_DPP_F(old, src, ctrl) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, (float)(old)), __builtin_bit_cast(int, (float)(src)), ctrl, 0xf, 0xf, false))
#define EEC_DPP_I(old, src, ctrl) __builtin_amdgcn_update_dpp((int)(old), (int)(src), ctrl, 0xf, 0xf, false)

// The training forward (ctc_alpha_kernel): every step's scaled alphas and lane exponents are written to `astore` (layout
// ctc_store_index below); the backward pass multiplies them with the betas it recomputes (ctc_beta_kernel).
__device__ __forceinline__ size_t ctc_store_index(int lat, int Tq, int P, int t, int k, int lane) {
  return (((size_t)lat * Tq + t) * (P + 1) + k) * 64 + lane;  // k < P: state lane*P + k; k == P: the lane's exponent
}

template <int P>
__global__ __launch_bounds__(64) void ctc_alpha_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                       const long long* __restrict__ target_len,
                                                       EEC_LEN_PARAM(const int* __restrict__ input_len) int B, int Tq, int V,
                                                       int S, int blank, float* __restrict__ nll, float* __restrict__ astore) {
  const int lat = blockIdx.x, b = lat % B, lane = threadIdx.x;
  const float* lp = logp + (size_t)lat * Tq * V;
  const int Tb = EEC_LEN_FRAMES(input_len, b, Tq);
  // inputs nn.CTCLoss validates on the host: a length outside [0, S] or a label outside [0, V) would index out of
  // bounds.  Such a lattice is not run on the caller's data: its nll becomes NaN (ctc_reduce_kernel propagates it).
  const long long len_raw = target_len[b];
  bool bad = len_raw < 0 || len_raw > (long long)S;
  const int len = bad ? 0 : (int)len_raw;
  const int L = 2 * len + 1;
  int label[P];
  bool skip_ok[P], live[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    label[i] = blank;
    skip_ok[i] = false;
    live[i] = s < L;
    if (s < L && (s & 1)) {
      const int k = s >> 1;
      const long long lab = targets[(size_t)b * S + k];
      if (lab < 0 || lab >= (long long)V) bad = true;
      label[i] = (lab < 0 || lab >= (long long)V) ? blank : (int)lab;
      skip_ok[i] = k > 0 && lab != targets[(size_t)b * S + k - 1];
    }
  }
  bad = __any((int)bad) != 0;  // wave-uniform
  if (kLen && Tb == 0) {  // no frame (wave-uniform): only the empty target is feasible; frame 0 is padding and is not read
    if (lane == 0) {
      float* pinfo = astore + ctc_store_index(gridDim.x, Tq, P, 0, 0, 0) + 2 * (size_t)lat;
      nll[lat] = bad ? __builtin_nanf("") : len == 0 ? 0.f : INFINITY;
      pinfo[0] = bad ? __builtin_nanf("") : len == 0 ? 1.f : 0.f;
      pinfo[1] = __builtin_bit_cast(float, 0);
    }
    return;
  }
  float livef[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    livef[i] = live[i] ? 1.f : 0.f;
    // keep every label in a VGPR: a label the compiler can prove wave-uniform (the blanks) would turn
    // its gather into s_load + s_waitcnt lgkmcnt(0), which serialises the prefetch ring
    asm volatile("" : "+v"(label[i]));
  }
  float alpha[P], lim[P];
  int ex = kCtcEmpty;  // this lane's states are alpha[i] * 2^ex
  static_assert(P % 2 == 0, "a lane's first state must be a blank");
  int eloss = kCtcEmpty;  // largest scale at which a non-zero value left the fp32 range (see RANGE above)
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    const float l0 = lp[label[i]];
    alpha[i] = (s < 2 && s < L) ? __expf(l0) : 0.f;
    eloss = ((s < 2 && s < L) & (l0 > -INFINITY) & (alpha[i] < kCtcTiny)) ? 0 : eloss;
    lim[i] = live[i] ? -INFINITY : INFINITY;  // an emission above lim is a finite log-prob of a live state
  }
  if (lane == 0) ex = 0;
  auto store = [&](int t) {
#pragma unroll
    for (int i = 0; i < P; ++i) astore[ctc_store_index(lat, Tq, P, t, i, lane)] = alpha[i];
    astore[ctc_store_index(lat, Tq, P, t, P, lane)] = __builtin_bit_cast(float, ex);
  };
  store(0);
  // emission log-probs are gathered kCtcAhead steps ahead of their use (exponentiated when used)
  constexpr int kCtcAhead = P <= 4 ? 16 : 8;
  float emit[kCtcAhead][P];
#pragma unroll
  for (int d = 0; d < kCtcAhead; ++d)
#pragma unroll
    for (int i = 0; i < P; ++i) emit[d][i] = lp[(size_t)min(1 + d, Tb - 1) * V + label[i]];
  // one time step, branch-free (selects only) so that the unrolled group below is a single basic
  // block and the emission loads keep their kCtcAhead-step lead (s_waitcnt vmcnt(N), not vmcnt(0))
  auto step = [&](const float (&em)[P], bool renorm) {
    // the previous lane's last two states and its exponent (lane 0 receives 0 / its own exponent)
    float up1 = EEC_DPP_F(0.f, alpha[P - 1], 0x138);  // wave_shr:1
    float up2 = EEC_DPP_F(0.f, alpha[P - 2], 0x138);
    const int ex_up = EEC_DPP_I(ex, ex, 0x138);
    const int ec = max(ex, ex_up);  // common scale of this step
    const int d_own = max(ex - ec, -200), d_up = max(ex_up - ec, -200);
    const float up1s = ldexpf(up1, d_up), up2s = ldexpf(up2, d_up);
    bool lost = (up1 > 0.f) & (up1s < kCtcTiny);  // up2 is never taken: a lane's first state is a blank (P is even)
    up1 = up1s;
    up2 = up2s;
    float cur[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      cur[i] = ldexpf(alpha[i], d_own);
      lost |= (alpha[i] > 0.f) & (cur[i] < kCtcTiny);
    }
    ex = ec;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float p1 = i >= 1 ? cur[i - 1] : up1;
      const float p2 = i >= 2 ? cur[i - 2] : (i == 1 ? up1 : up2);
      // exp(em) * livef is independent of the alpha chain; states beyond 2*len+1 are zeroed by livef
      const float sum = cur[i] + p1 + (skip_ok[i] ? p2 : 0.f);
      alpha[i] = sum * (__expf(em[i]) * livef[i]);
      lost |= (sum > 0.f) & (alpha[i] < kCtcTiny) & (em[i] > lim[i]);
    }
    eloss = lost ? max(eloss, ec) : eloss;
    if (renorm) {  // compile-time: renormalise this lane every second step
      float m = alpha[0];
#pragma unroll
      for (int i = 1; i < P; ++i) m = fmaxf(m, alpha[i]);
      const bool any = m > 0.f;
      const int e = any ? (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu) - 127 : 0;
#pragma unroll
      for (int i = 0; i < P; ++i) alpha[i] = ldexpf(alpha[i], -e);
      ex = any ? ex + e : kCtcEmpty;
    }
  };
  int t0 = 1;
  for (; t0 + kCtcAhead <= Tb; t0 += kCtcAhead) {  // full groups
#pragma unroll
    for (int d = 0; d < kCtcAhead; ++d) {
      step(emit[d], (d & 1) != 0);
      store(t0 + d);
      const int tn = min(t0 + d + kCtcAhead, Tb - 1);  // clamped: a harmless re-read near the end
#pragma unroll
      for (int i = 0; i < P; ++i) emit[d][i] = lp[(size_t)tn * V + label[i]];  // raw: exp at use
    }
  }
#pragma unroll
  for (int d = 0; d < kCtcAhead; ++d)  // ragged tail (wave-uniform guard); its emissions are already in the ring
    if (t0 + d < Tb) {
      step(emit[d], (d & 1) != 0);
      store(t0 + d);
    }
  // p(target) = a[L-1] + a[L-2]: at most two lanes contribute, each with its own exponent
  float tail = 0.f;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    if (s == L - 1 || s == L - 2) tail += alpha[i];
  }
  bad = bad || __any((int)(tail != tail)) != 0;  // NaN log-probs that reach the final states (fmaxf / > drop NaNs silently)
  const int e_lane = tail > 0.f ? ex : kCtcEmpty;
  const int e_max = (int)wave_max((float)e_lane);  // exponents are small integers: exact in fp32
  const float total = wave_sum(tail > 0.f ? ldexpf(tail, max(e_lane - e_max, -200)) : 0.f);
  // the events are harmless where they cannot have taken 2^-26 of p(target) = total * 2^e_max
  const int e_tot = total > 0.f ? e_max + (int)((__builtin_bit_cast(unsigned, total) >> 23) & 0xffu) - 127 : 2 * kCtcEmpty;
  const bool redo = __any((int)(eloss > kCtcEmpty && eloss > e_tot + ctc_watch_slack(Tq))) != 0;
  // a NaN emission makes `total` NaN: (NaN > 0) is false, so test it explicitly instead of reporting "infeasible"
  if (lane == 0)
    nll[lat] = (bad || total != total) ? __builtin_nanf("")
               : redo                  ? -INFINITY
               : (total > 0.f)         ? -(logf(total) + (float)e_max * 0.6931471805599453f)
                                       : INFINITY;
  if (lane == 0) {  // p(target) = total * 2^e_max, kept exactly for the backward pass (nll alone rounds it to ~1e-4 relative)
    float* pinfo = astore + ctc_store_index(gridDim.x, Tq, P, 0, 0, 0) + 2 * (size_t)lat;
    pinfo[0] = (bad || total != total) ? __builtin_nanf("") : redo ? kCtcRedo : total;
    pinfo[1] = __builtin_bit_cast(float, e_max);
  }
}

// ---------------------------------------------------------------------------
// Backward (gradient of the summed per-exit loss with respect to the log-probs; reference: loss.backward() through
// nn.CTCLoss, train.py:60-68).  torch's CTC backward returns, for a lattice with upstream gradient g,
//     dlogp[t][c] = g * ( exp(logp[t][c]) - gamma_t(c) ),    gamma_t(c) = sum_{s: l'_s = c} alpha_t(s) beta'_t(s) / p(target)
// (the gradient with respect to the logits of a log-softmax: it sums to zero over c), with
//     beta'_{T-1}(s) = [s is one of the last two states],
//     beta'_{t-1}(s) = sum_{s' in {s, s+1, s+2 if allowed}} beta'_t(s') * p_t(l'_{s'}).
// ctc_beta_kernel walks t downwards with the same block-floating representation as the forward pass (one wave per
// lattice, neighbour states of the NEXT lane through a DPP wave shift) and overwrites the stored alphas with the state
// posteriors gamma_t(s); ctc_grad_kernel then turns them into the dense gradient, one wave per (lattice, frame).
template <int P>
__global__ __launch_bounds__(64) void ctc_beta_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                      const long long* __restrict__ target_len,
                                                      EEC_LEN_PARAM(const int* __restrict__ input_len) int B, int Tq, int V,
                                                      int S, int blank, const float* __restrict__ nll, float* __restrict__ astore) {
  const int lat = blockIdx.x, b = lat % B, lane = threadIdx.x;
  const float* lp = logp + (size_t)lat * Tq * V;
  float* pinfo = astore + ctc_store_index(gridDim.x, Tq, P, 0, 0, 0) + 2 * (size_t)lat;
  if (pinfo[0] < 0.f) return;  // the forward pass left this lattice to the wide format (wave-uniform)
  const int Tb = EEC_LEN_FRAMES(input_len, b, Tq);
  if (kLen && Tb == 0) return;  // no frame, no posteriors (wave-uniform)
  const long long len_raw = target_len[b];
  const int len = (len_raw < 0 || len_raw > (long long)S) ? 0 : (int)len_raw;
  const int L = 2 * len + 1;
  int label[P];
  bool skip_ok[P];
  float livef[P], lim[P];
  bool redo = false;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    label[i] = blank;
    skip_ok[i] = false;
    livef[i] = s < L ? 1.f : 0.f;
    lim[i] = s < L ? -INFINITY : INFINITY;
    if (s < L && (s & 1)) {
      const int k = s >> 1;
      const long long lab = targets[(size_t)b * S + k];
      label[i] = (lab < 0 || lab >= (long long)V) ? blank : (int)lab;
      skip_ok[i] = k > 0 && lab != targets[(size_t)b * S + k - 1];
    }
    asm volatile("" : "+v"(label[i]));
  }
  // transition s -> s + 2 is allowed when state s + 2 may be entered by a skip; states s + 1, s + 2 of the last slots of a
  // lane live in the next lane
  bool skip_dn[P];
  {
    const int n0 = EEC_DPP_I(0, (int)skip_ok[0], 0x130), n1 = EEC_DPP_I(0, (int)skip_ok[1], 0x130);  // wave_shl:1
#pragma unroll
    for (int i = 0; i < P; ++i) skip_dn[i] = i + 2 < P ? skip_ok[i + 2] : ((i + 2 - P == 0 ? n0 : n1) != 0);
  }
  // p(target) = total * 2^e_max exactly as the forward pass left it: gamma = alpha beta' 2^(ea + eb - e_max) / total
  const float ptot = pinfo[0];
  const bool usable = ptot > 0.f && ptot < INFINITY;  // false for an infeasible (0) or invalid (NaN) lattice
  const int ishift = usable ? -__builtin_bit_cast(int, pinfo[1]) : 0;
  const float fscale = usable ? 1.0f / ptot : 0.f;
  // events above this scale may have taken 2^-26 of p(target) (see RANGE at the top)
  const int e_ptot = (int)((__builtin_bit_cast(unsigned, ptot) >> 23) & 0xffu) - 127;  // p(target) = ptot * 2^-ishift
  const int e_harm = usable ? -ishift + e_ptot + ctc_watch_slack(Tq) : INT_MAX;
  const int sh_harm = 120 - 26 - 2 + e_ptot;  // a product below kCtcTiny shifted by more than this: a posterior of 2^-26 or more
  float beta[P];
  int eb = kCtcEmpty;
  bool any0 = false;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    beta[i] = (s < L && (s == L - 1 || s == L - 2)) ? 1.f : 0.f;
    any0 = any0 || beta[i] != 0.f;
  }
  if (any0) eb = 0;
  constexpr int kAhead = P <= 4 ? 8 : 4;
  float emit[kAhead][P], al[kAhead][P + 1];
  auto fetch = [&](int slot, int t) {  // emissions and stored alphas of time t (clamped: harmless re-reads below t = 0)
    const int tc = max(t, 0);
#pragma unroll
    for (int i = 0; i < P; ++i) emit[slot][i] = lp[(size_t)tc * V + label[i]];
#pragma unroll
    for (int k = 0; k <= P; ++k) al[slot][k] = astore[ctc_store_index(lat, Tq, P, tc, k, lane)];
  };
#pragma unroll
  for (int d = 0; d < kAhead; ++d) fetch(d, Tb - 1 - d);
  auto step = [&](int slot, int t, bool renorm) {
    // posteriors of time t, in place of the stored alphas
    const int ea = __builtin_bit_cast(int, al[slot][P]);
    const int sh = max(min(ea + eb + ishift, 126), -300);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float ab = al[slot][i] * beta[i];
      redo |= (al[slot][i] > 0.f) & (beta[i] > 0.f) & (ab < kCtcTiny) & (sh > sh_harm);
      astore[ctc_store_index(lat, Tq, P, t, i, lane)] = ldexpf(ab * fscale, sh) * livef[i];
    }
    // beta'_{t-1}
    float bw[P];
    bool lost = false;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      bw[i] = beta[i] * (__expf(emit[slot][i]) * livef[i]);
      lost |= (beta[i] > 0.f) & (bw[i] < kCtcTiny) & (emit[slot][i] > lim[i]);
    }
    float dn1 = EEC_DPP_F(0.f, bw[0], 0x130);  // next lane's first two weighted betas and its exponent
    float dn2 = EEC_DPP_F(0.f, bw[1], 0x130);
    const int eb_dn = EEC_DPP_I(kCtcEmpty, eb, 0x130);
    const int ec = max(eb, eb_dn);
    const int d_own = max(eb - ec, -200), d_dn = max(eb_dn - ec, -200);
    const float dn1s = ldexpf(dn1, d_dn), dn2s = ldexpf(dn2, d_dn);
    lost |= ((dn1 > 0.f) & (dn1s < kCtcTiny)) | ((dn2 > 0.f) & (dn2s < kCtcTiny));
    dn1 = dn1s;
    dn2 = dn2s;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float sh_own = ldexpf(bw[i], d_own);
      lost |= (bw[i] > 0.f) & (sh_own < kCtcTiny);
      bw[i] = sh_own;
    }
    eb = ec;
    redo |= lost & (ec > e_harm);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float n1 = i + 1 < P ? bw[i + 1 < P ? i + 1 : 0] : dn1;
      const float n2 = i + 2 < P ? bw[i + 2 < P ? i + 2 : 0] : (i + 2 - P == 0 ? dn1 : dn2);
      beta[i] = bw[i] + n1 + (skip_dn[i] ? n2 : 0.f);
    }
    if (renorm) {
      float m = beta[0];
#pragma unroll
      for (int i = 1; i < P; ++i) m = fmaxf(m, beta[i]);
      const bool any = m > 0.f;
      const int e = any ? (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xffu) - 127 : 0;
#pragma unroll
      for (int i = 0; i < P; ++i) beta[i] = ldexpf(beta[i], -e);
      eb = any ? eb + e : kCtcEmpty;
    }
  };
  int t = Tb - 1;
  for (; t - kAhead + 1 >= 0; t -= kAhead) {
#pragma unroll
    for (int d = 0; d < kAhead; ++d) {
      step(d, t - d, (d & 1) != 0);
      fetch(d, t - d - kAhead);
    }
  }
#pragma unroll
  for (int d = 0; d < kAhead; ++d)
    if (t - d >= 0) step(d, t - d, (d & 1) != 0);
  if (usable && __any((int)redo) != 0 && lane == 0) pinfo[0] = kCtcRedo;  // an unusable lattice has no posteriors to lose
}

// dlogp[lat][t][c] = gs * (exp(logp) - sum of the posteriors of the states labelled c), gs = grad_loss[e] / (B max(len, 1))
// (0 for an infeasible lattice: zero_infinity; NaN for a lattice whose loss is NaN).  One wave per (lattice, frame).
// With input lengths a row t >= Tb is written as zeros, without a read of its log-probs or of its slots of `astore` (never stored).
template <int P>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                       const long long* __restrict__ target_len,
                                                       EEC_LEN_PARAM(const int* __restrict__ input_len) int B, int Tq, int V, int S,
                                                       int blank, const float* __restrict__ nll, const float* __restrict__ astore,
                                                       const float* __restrict__ grad_loss, int n_rows, float* __restrict__ dlogp) {
  __shared__ float bins_all[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  float* bins = bins_all[w];
  const bool row_ok = row < n_rows;
  const int lat = row_ok ? row / Tq : 0, t = row_ok ? row - lat * Tq : 0, b = lat % B, e = lat / B;
  *(float4*)(bins + lane * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const long long len_raw = target_len[b];
  const int len = (len_raw < 0 || len_raw > (long long)S) ? 0 : (int)len_raw;
  const int L = 2 * len + 1;
  const bool pad = kLen && t >= EEC_LEN_FRAMES(input_len, b, Tq);  // wave-uniform
  if (row_ok && !pad) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int s = lane * P + i;
      if (s < L) {
        int lab = blank;
        if (s & 1) {
          const long long lr = targets[(size_t)b * S + (s >> 1)];
          lab = (lr < 0 || lr >= (long long)V) ? blank : (int)lr;
        }
        atomicAdd(&bins[lab], astore[ctc_store_index(lat, Tq, P, t, i, lane)]);
      }
    }
  }
  __syncthreads();
  if (!row_ok) return;
  if (pad) {
    if (lane * 4 < V) *(float4*)(dlogp + ((size_t)lat * Tq + t) * V + lane * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float nl = nll[lat];
  float gs = grad_loss[e] / ((float)B * (float)(len > 0 ? len : 1));
  if (nl != nl) gs = nl;            // NaN loss: NaN gradient
  else if (!(nl < INFINITY)) gs = 0.f;  // zero_infinity
  const int c0 = lane * 4;
  if (c0 < V) {
    const size_t off = ((size_t)lat * Tq + t) * V + c0;
    const float4 l = *(const float4*)(logp + off);
    const float4 g = *(const float4*)(bins + c0);
    float4 o;
    o.x = gs * (__expf(l.x) - g.x), o.y = gs * (__expf(l.y) - g.y), o.z = gs * (__expf(l.z) - g.z), o.w = gs * (__expf(l.w) - g.w);
    if (gs == 0.f) o = make_float4(0.f, 0.f, 0.f, 0.f);  // an infeasible lattice may hold inf / NaN posteriors
    *(float4*)(dlogp + off) = o;
  }
}

// ---------------------------------------------------------------------------
// The wide path: the lattices the block-floating kernels marked (see RANGE at the top).  Same linear-domain recursions, but
// every state carries its own exponent -- value = m * 2^e, m in [1, 2) or 0 -- and is renormalised at every step, and an
// emission enters as exp(l) = pm * 2^k with the product l * log2(e) split exactly, so nothing can leave the range whatever the
// log-probs are (below -3e4 they count as -inf: impossible).  ctc_wide_kernel (after ctc_beta_kernel; one wave per marked lattice,
// a 4-step look-ahead ring; the waves of unmarked lattices return at once): the forward recursion again, its states kept
// (mantissas in the alpha slots of `astore`, exponents in the region behind it), then the beta recursion, which overwrites the
// mantissas with the state posteriors for ctc_grad_kernel.  ctc_loss_kernel (further down) is the same format's loss.
constexpr int kCtcWideEmpty = -(1 << 30);

__device__ __forceinline__ void ctc_wide_exp(float l, float& pm, int& k) {
  const float hi = l * 1.44269502f;
  const float lo = fmaf(l, 1.44269502f, -hi) + l * 1.92596299e-8f;  // log2(e) = 1.44269502 + 1.92596299e-8
  const float kf = floorf(hi);
  const bool zero = !(l > -3.0e4f);
  pm = zero ? 0.f : exp2f((hi - kf) + lo);
  k = zero ? 0 : (int)kf;
}
__device__ __forceinline__ void ctc_wide_norm(float v, int base, float& m, int& e) {  // v: 0 or a normal number
  const int ex = (int)((__builtin_bit_cast(unsigned, v) >> 23) & 0xffu) - 127;
  const bool any = v > 0.f;
  m = any ? ldexpf(v, -ex) : 0.f;
  e = any ? base + ex : kCtcWideEmpty;
}
__device__ __forceinline__ float ctc_wide_add3(float m0, int e0, float m1, int e1, float m2, int e2, int& ec) {
  ec = max(e0, max(e1, e2));  // a term more than 2^-64 below the largest is below the fp32 sum's last bit
  return ldexpf(m0, max(e0 - ec, -64)) + ldexpf(m1, max(e1 - ec, -64)) + ldexpf(m2, max(e2 - ec, -64));
}

template <int P>
__global__ __launch_bounds__(64) void ctc_wide_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                      const long long* __restrict__ target_len,
                                                      EEC_LEN_PARAM(const int* __restrict__ input_len) int B, int Tq, int V, int S,
                                                      int blank, float* __restrict__ nll, float* __restrict__ astore) {
  const int lat = blockIdx.x, b = lat % B, lane = threadIdx.x;
  if (!(astore[ctc_store_index(gridDim.x, Tq, P, 0, 0, 0) + 2 * (size_t)lat] < 0.f)) return;
  const int Tb = EEC_LEN_FRAMES(input_len, b, Tq);  // a marked lattice has a frame: Tb >= 1
  const float* lp = logp + (size_t)lat * Tq * V;
  int* estore = (int*)(astore + ctc_store_index(gridDim.x, Tq, P, 0, 0, 0) + 2 * (size_t)gridDim.x);  // [lat][t][P][64]
  const long long len_raw = target_len[b];  // a marked lattice passed ctc_alpha_kernel's input checks
  const int len = (len_raw < 0 || len_raw > (long long)S) ? 0 : (int)len_raw;
  const int L = 2 * len + 1;
  int label[P];
  bool skip_ok[P], live[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    label[i] = blank;
    skip_ok[i] = false;
    live[i] = s < L;
    if (s < L && (s & 1)) {
      const int k = s >> 1;
      const long long lab = targets[(size_t)b * S + k];
      label[i] = (lab < 0 || lab >= (long long)V) ? blank : (int)lab;
      skip_ok[i] = k > 0 && lab != targets[(size_t)b * S + k - 1];
    }
  }
  float am[P];
  int ae[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    float pm;
    int k;
    ctc_wide_exp(lp[label[i]], pm, k);
    ctc_wide_norm((s < 2 && s < L) ? pm : 0.f, k, am[i], ae[i]);
  }
  auto store = [&](int t) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      astore[ctc_store_index(lat, Tq, P, t, i, lane)] = am[i];
      estore[(((size_t)lat * Tq + t) * P + i) * 64 + lane] = ae[i];
    }
  };
  store(0);
  // the emission log-probs are gathered kAhead steps ahead of their use, as in the fast path
  constexpr int kAhead = 4;
  float emit[kAhead][P];
#pragma unroll
  for (int d = 0; d < kAhead; ++d)
#pragma unroll
    for (int i = 0; i < P; ++i) emit[d][i] = lp[(size_t)min(1 + d, Tb - 1) * V + label[i]];
  for (int t0 = 1; t0 < Tb; t0 += kAhead)
#pragma unroll
  for (int d = 0; d < kAhead; ++d) {
    const int t = t0 + d;
    if (t >= Tb) break;  // wave-uniform
    // the previous lane's last two states (wave_shr:1; lane 0 receives an empty state)
    const float u1m = EEC_DPP_F(0.f, am[P - 1], 0x138), u2m = EEC_DPP_F(0.f, am[P - 2], 0x138);
    const int u1e = EEC_DPP_I(kCtcWideEmpty, ae[P - 1], 0x138), u2e = EEC_DPP_I(kCtcWideEmpty, ae[P - 2], 0x138);
    float nm[P];
    int ne[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float p1m = i >= 1 ? am[i >= 1 ? i - 1 : 0] : u1m;
      const int p1e = i >= 1 ? ae[i >= 1 ? i - 1 : 0] : u1e;
      float p2m = i >= 2 ? am[i >= 2 ? i - 2 : 0] : (i == 1 ? u1m : u2m);
      int p2e = i >= 2 ? ae[i >= 2 ? i - 2 : 0] : (i == 1 ? u1e : u2e);
      if (!skip_ok[i]) p2m = 0.f, p2e = kCtcWideEmpty;
      float pm;
      int k, ec;
      ctc_wide_exp(emit[d][i], pm, k);
      const float sum = ctc_wide_add3(am[i], ae[i], p1m, p1e, p2m, p2e, ec);
      ctc_wide_norm(live[i] ? sum * pm : 0.f, ec + k, nm[i], ne[i]);
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
      am[i] = nm[i], ae[i] = ne[i];
      emit[d][i] = lp[(size_t)min(t + kAhead, Tb - 1) * V + label[i]];  // clamped: a harmless re-read near the end
    }
    store(t);
  }
  // p(target) = a[L-1] + a[L-2] = mt * 2^et
  float tm = 0.f;
  int te = kCtcWideEmpty;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    if (s == L - 1 || s == L - 2) {
      int ec;
      tm = ctc_wide_add3(tm, te, am[i], ae[i], 0.f, kCtcWideEmpty, ec);
      te = tm > 0.f ? ec : kCtcWideEmpty;
    }
  }
  const int e_max = wave_all_max(te);
  float total = ldexpf(tm, max(te - e_max, -64));
  total = wave_all_sum(total);
  float mt;
  int et;
  ctc_wide_norm(total, e_max, mt, et);
  if (!(total > 0.f)) return;  // infeasible: nll is +inf and ctc_grad_kernel writes zeros
  bool skip_dn[P];
  {
    int n0 = __shfl_down((int)skip_ok[0], 1, 64), n1 = __shfl_down((int)skip_ok[1], 1, 64);
    if (lane == 63) n0 = n1 = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) skip_dn[i] = i + 2 < P ? skip_ok[i + 2 < P ? i + 2 : 0] : ((i + 2 - P == 0 ? n0 : n1) != 0);
  }
  const float inv = 1.0f / mt;
  float bm[P];
  int be[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    const bool last = s < L && (s == L - 1 || s == L - 2);
    bm[i] = last ? 1.f : 0.f;
    be[i] = last ? 0 : kCtcWideEmpty;
  }
  for (int t = Tb - 1; t >= 0; --t) {
    float wm[P];
    int we[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const size_t ia = ctc_store_index(lat, Tq, P, t, i, lane);
      const float a_m = astore[ia];
      const int a_e = estore[(((size_t)lat * Tq + t) * P + i) * 64 + lane];
      const bool nz = a_m > 0.f && bm[i] > 0.f;
      const int sh = nz ? min(max(a_e + be[i] - et, -200), 126) : 0;
      astore[ia] = nz ? ldexpf(a_m * bm[i] * inv, sh) : 0.f;  // the posterior of state lane * P + i at time t
      float pm;
      int k;
      ctc_wide_exp(lp[(size_t)t * V + label[i]], pm, k);
      ctc_wide_norm(live[i] ? bm[i] * pm : 0.f, be[i] + k, wm[i], we[i]);
    }
    float d1m = __shfl_down(wm[0], 1, 64), d2m = __shfl_down(wm[1], 1, 64);
    int d1e = __shfl_down(we[0], 1, 64), d2e = __shfl_down(we[1], 1, 64);
    if (lane == 63) d1m = d2m = 0.f, d1e = d2e = kCtcWideEmpty;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const float n1m = i + 1 < P ? wm[i + 1 < P ? i + 1 : 0] : d1m;
      const int n1e = i + 1 < P ? we[i + 1 < P ? i + 1 : 0] : d1e;
      float n2m = i + 2 < P ? wm[i + 2 < P ? i + 2 : 0] : (i + 2 - P == 0 ? d1m : d2m);
      int n2e = i + 2 < P ? we[i + 2 < P ? i + 2 : 0] : (i + 2 - P == 0 ? d1e : d2e);
      if (!skip_dn[i]) n2m = 0.f, n2e = kCtcWideEmpty;
      int ec;
      const float sum = ctc_wide_add3(wm[i], we[i], n1m, n1e, n2m, n2e, ec);
      ctc_wide_norm(sum, ec, bm[i], be[i]);
    }
  }
}

// ---------------------------------------------------------------------------
// The loss alone (eec_ctc_loss, and the marked lattices of the training forward): the wide format on EVERY lattice -- no range
// limit, so no watch, no marking and no second pass -- with the T' - 1 dependent steps shared by two waves.  At any frame m
//     p(target) = sum_s alpha_m(s) * beta'_m(s),     beta' as defined above ctc_beta_kernel,
// so wave 0 of a workgroup walks alpha from frame 0 up to m = (T' - 1) / 2 while wave 1 walks from frame T' - 1 down to m + 1;
// both keep state lane * P + i in slot i, share nothing until wave 1 hands beta'_m over through LDS (one barrier), and wave 0
// forms the sum.  Both halves run ONE recursion, X_t(s) = p_t(l'_s) * (X_u(s) + X_u(s -+ 1) + [X_u(s -+ 2)]), u = t -+ 1:
// upwards X = alpha (neighbours in the previous lane); downwards X_t(s) = beta'_t(s) p_t(l'_s) (neighbours in the next lane),
// and beta'_m is one more neighbour sum without an emission.  T' = 1 .. 3: m = 0, 0, 1, wave 0 takes 0, 0, 1 steps, wave 1
// none (T' = 1: beta'_0 is the indicator of the last two states, no emission; T' = 2, 3: its start and the closing sum).
// NaN log-probs: a NaN emission makes its state's mantissa NaN and travels with it (ctc_loss_norm keeps it).  As in torch and
// ctc_alpha_kernel, a NaN emission of a live state counts whether or not any mass has reached the state (upwards 0 * NaN = NaN;
// a NaN beta'_m makes its term NaN even where alpha_m is 0): reachability from the START is never asked for.  What is asked
// for is a way on to the END with non-zero probability: the downward half multiplies an emission in only where the sum behind
// it is non-zero, and the closing sum drops a NaN alpha_m where beta'_m is 0.  So the loss is NaN when a live state's NaN
// emission has such a way to the final states, and is not disturbed by one that has none (torch asks for a way by the
// transitions alone: the two differ only where exact -inf log-probs close every way that the transitions leave open).
__device__ __forceinline__ void ctc_loss_exp(float l, float& pm, int& k) {  // ctc_wide_exp that keeps a NaN
  const float hi = l * 1.44269502f;
  const float lo = fmaf(l, 1.44269502f, -hi) + l * 1.92596299e-8f;
  const float kf = floorf(hi);
  pm = l <= -3.0e4f ? 0.f : __builtin_amdgcn_exp2f((hi - kf) + lo);  // the argument is in [0, 1]: exp2f's range fix-up is idle
  k = l > -3.0e4f ? (int)kf : 0;
}
__device__ __forceinline__ void ctc_loss_norm(float v, int base, float& m, int& e) {  // v: 0, a normal number or NaN
  const int ex = (int)((__builtin_bit_cast(unsigned, v) >> 23) & 0xffu) - 127;
  m = ldexpf(v, -ex);  // 0 stays 0
  e = v != 0.f ? base + ex : kCtcWideEmpty;
}

// sum[i] * 2^ec[i] = X(s) + X(s -+ 1) + [X(s -+ 2) where the skip is allowed], s = lane * P + i
template <int P, bool DOWN>
__device__ __forceinline__ void ctc_loss_sums(const float (&xm)[P], const int (&xe)[P], const bool (&skip)[P], float (&sum)[P],
                                              int (&ec)[P]) {
  // the two states next to this lane's: the previous lane's last two (wave_shr:1) or the next lane's first two (wave_shl:1);
  // the lane at the end of the wave receives empty states
  constexpr int ctrl = DOWN ? 0x130 : 0x138;
  const float u1m = EEC_DPP_F(0.f, xm[DOWN ? 0 : P - 1], ctrl), u2m = EEC_DPP_F(0.f, xm[DOWN ? 1 : P - 2], ctrl);
  const int u1e = EEC_DPP_I(kCtcWideEmpty, xe[DOWN ? 0 : P - 1], ctrl), u2e = EEC_DPP_I(kCtcWideEmpty, xe[DOWN ? 1 : P - 2], ctrl);
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int d1 = DOWN ? i + 1 : i - 1, d2 = DOWN ? i + 2 : i - 2;  // slots of the neighbours; outside [0, P): the other lane's
    const bool in1 = d1 >= 0 && d1 < P, in2 = d2 >= 0 && d2 < P;
    const bool far2 = DOWN ? d2 == P + 1 : d2 == -2;
    const float n1m = in1 ? xm[in1 ? d1 : 0] : u1m;
    const int n1e = in1 ? xe[in1 ? d1 : 0] : u1e;
    float n2m = in2 ? xm[in2 ? d2 : 0] : (far2 ? u2m : u1m);
    int n2e = in2 ? xe[in2 ? d2 : 0] : (far2 ? u2e : u1e);
    if (!skip[i]) n2m = 0.f, n2e = kCtcWideEmpty;
    sum[i] = ctc_wide_add3(xm[i], xe[i], n1m, n1e, n2m, n2e, ec[i]);
  }
}

// n steps of the recursion over the frames t_first, t_first +- 1, ...; the emission log-probs are gathered kAhead steps ahead of
// their use (raw; split into mantissa and exponent when used), never from a frame beyond the walk's last one
template <int P, bool DOWN>
__device__ __forceinline__ void ctc_loss_walk(const float* __restrict__ lp, int V, const int (&label)[P], const bool (&skip)[P],
                                              const bool (&live)[P], int t_first, int n, float (&xm)[P], int (&xe)[P]) {
  // label: byte offsets of the states' classes in a row of log-probs (32 bits beside the row's wave-uniform address)
  if (n <= 0) return;  // wave-uniform
  constexpr int kAhead = P <= 4 ? 16 : 8;  // 78 / 144 / 148 VGPRs at P = 2 / 4 / 8, no scratch; at P = 2, 8 measures the same, 32 is 3 us slower
  float emit[kAhead][P];
  auto gather = [&](float (&em)[P], int j) {
    const float* row = lp + (size_t)(DOWN ? t_first - min(j, n - 1) : t_first + min(j, n - 1)) * V;  // wave-uniform
#pragma unroll
    for (int i = 0; i < P; ++i) em[i] = *(const float*)((const char*)row + (unsigned)label[i]);
  };
#pragma unroll
  for (int d = 0; d < kAhead; ++d) gather(emit[d], d);
  auto step = [&](const float (&em)[P]) {
    float sum[P];
    int ec[P];
    ctc_loss_sums<P, DOWN>(xm, xe, skip, sum, ec);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      float pm;
      int k;
      ctc_loss_exp(em[i], pm, k);
      // upwards: states beyond 2 len + 1 stay empty (`live`).  Downwards `live` is not needed: those states receive from
      // higher ones only and are empty anyway, and an emission (NaN included) counts only where the end can be reached from
      const bool keep = DOWN ? sum[i] != 0.f : live[i];
      ctc_loss_norm(keep ? sum[i] * pm : 0.f, ec[i] + k, xm[i], xe[i]);
    }
  };
  int j0 = 0;
  for (; j0 + kAhead <= n; j0 += kAhead) {  // full groups
#pragma unroll
    for (int d = 0; d < kAhead; ++d) {
      step(emit[d]);
      gather(emit[d], j0 + d + kAhead);  // clamped to the last frame of the walk: a harmless re-read near its end
    }
  }
#pragma unroll
  for (int d = 0; d < kAhead; ++d)  // ragged tail (wave-uniform guard); its emissions are already in the ring
    if (j0 + d < n) step(emit[d]);
}

// only_marked: the training forward's follow-up launch -- lattices ctc_alpha_kernel marked (nll == -inf) are run, the others keep
// their nll.  With input lengths T' in the account above is Tb: the waves meet at m = (Tb - 1) / 2 and wave 1 starts at Tb - 1.
template <int P>
__global__ __launch_bounds__(128) void ctc_loss_kernel(const float* __restrict__ logp, const long long* __restrict__ targets,
                                                       const long long* __restrict__ target_len,
                                                       EEC_LEN_PARAM(const int* __restrict__ input_len) int B, int Tq, int V, int S,
                                                       int blank, int only_marked, float* __restrict__ nll) {
  __shared__ float beta_m[P][64];
  __shared__ int beta_e[P][64];
  const int lat = blockIdx.x, b = lat % B, lane = threadIdx.x & 63;
  const bool down = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) != 0;  // wave 1
  // read by both waves before the barrier; written by wave 0 behind it
  if (only_marked && !(nll[lat] == -INFINITY)) return;
  const float* lp = logp + (size_t)lat * Tq * V;
  // inputs nn.CTCLoss validates on the host, as in ctc_alpha_kernel: such a lattice is not run, its nll becomes NaN
  const long long len_raw = target_len[b];
  bool bad = len_raw < 0 || len_raw > (long long)S;
  const int len = bad ? 0 : (int)len_raw;
  const int L = 2 * len + 1;
  int label[P];
  bool skip_ok[P], live[P], last[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int s = lane * P + i;
    label[i] = blank;
    skip_ok[i] = false;
    live[i] = s < L;
    last[i] = s < L && (s == L - 1 || s == L - 2);
    if (s < L && (s & 1)) {
      const int k = s >> 1;
      const long long lab = targets[(size_t)b * S + k];
      if (lab < 0 || lab >= (long long)V) bad = true;
      label[i] = (lab < 0 || lab >= (long long)V) ? blank : (int)lab;
      skip_ok[i] = k > 0 && lab != targets[(size_t)b * S + k - 1];
    }
  }
  bad = __any((int)bad) != 0;  // wave-uniform, and the same in both waves (they hold the same states)
  if (bad) {
    if (threadIdx.x == 0) nll[lat] = __builtin_nanf("");
    return;
  }
  const int Tb = EEC_LEN_FRAMES(input_len, b, Tq);
  if (kLen && Tb == 0) {  // no frame (the same in both waves): only the empty target is feasible
    if (threadIdx.x == 0) nll[lat] = len == 0 ? 0.f : INFINITY;
    return;
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    // keep every label in a VGPR: a label the compiler can prove wave-uniform (the blanks) would turn its gather into
    // s_load + s_waitcnt lgkmcnt(0), which serialises the look-ahead ring
    label[i] *= (int)sizeof(float);  // from here on: the class's byte offset in a row
    asm volatile("" : "+v"(label[i]));
  }
  static_assert(P % 2 == 0, "a lane's first state must be a blank");
  auto at = [&](int t, int i) { return *(const float*)((const char*)(lp + (size_t)t * V) + (unsigned)label[i]); };
  const int m = (Tb - 1) / 2;
  float xm[P];
  int xe[P];
  if (!down) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int s = lane * P + i;
      float pm;
      int k;
      ctc_loss_exp(at(0, i), pm, k);
      ctc_loss_norm((s < 2 && s < L) ? pm : 0.f, k, xm[i], xe[i]);
    }
    ctc_loss_walk<P, false>(lp, V, label, skip_ok, live, 1, m, xm, xe);
  } else {
    if (Tb - 1 > m) {
      // the transition s -> s + 2 is allowed when state s + 2 may be entered by a skip
      bool skip_dn[P];
      const int n0 = EEC_DPP_I(0, (int)skip_ok[0], 0x130), n1 = EEC_DPP_I(0, (int)skip_ok[1], 0x130);
#pragma unroll
      for (int i = 0; i < P; ++i) skip_dn[i] = i + 2 < P ? skip_ok[i + 2 < P ? i + 2 : 0] : ((i + 2 - P == 0 ? n0 : n1) != 0);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        float pm;
        int k;
        ctc_loss_exp(at(Tb - 1, i), pm, k);
        ctc_loss_norm(last[i] ? pm : 0.f, k, xm[i], xe[i]);
      }
      ctc_loss_walk<P, true>(lp, V, label, skip_dn, live, Tb - 2, Tb - 2 - m, xm, xe);
      float sum[P];
      int ec[P];
      ctc_loss_sums<P, true>(xm, xe, skip_dn, sum, ec);
#pragma unroll
      for (int i = 0; i < P; ++i) ctc_loss_norm(sum[i], ec[i], xm[i], xe[i]);
    } else {  // T' = 1: beta'_0
#pragma unroll
      for (int i = 0; i < P; ++i) xm[i] = last[i] ? 1.f : 0.f, xe[i] = last[i] ? 0 : kCtcWideEmpty;
    }
#pragma unroll
    for (int i = 0; i < P; ++i) beta_m[i][lane] = xm[i], beta_e[i][lane] = xe[i];
  }
  __syncthreads();
  if (down) return;
  // p(target) = sum_s alpha_m(s) beta'_m(s) = mt * 2^et; the terms are brought to the lane's, then the wave's largest exponent
  float tm[P];
  int te[P], e_lane = kCtcWideEmpty;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const float bm = beta_m[i][lane];
    tm[i] = bm == 0.f ? 0.f : xm[i] * bm;  // 0, in [1, 4), or NaN
    te[i] = tm[i] != 0.f ? max(xe[i], kCtcWideEmpty / 2) + max(beta_e[i][lane], kCtcWideEmpty / 2) : kCtcWideEmpty;
    e_lane = max(e_lane, te[i]);
  }
  float tl = 0.f;
#pragma unroll
  for (int i = 0; i < P; ++i) tl += ldexpf(tm[i], max(te[i] - e_lane, -64));
  int e_max = e_lane;  // (written out: through wave_all_max / wave_all_sum this kernel's registers are allocated differently)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) e_max = max(e_max, __shfl_xor(e_max, off, 64));
  float total = ldexpf(tl, max(e_lane - e_max, -64));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off, 64);
  float mt;
  int et;
  ctc_loss_norm(total, e_max, mt, et);
  // a NaN total stays NaN (ctc_reduce_kernel propagates it); no common state of the two halves, or none at all: infeasible
  if (lane == 0) nll[lat] = total != 0.f ? -(logf(mt) + (float)et * 0.6931471805599453f) : INFINITY;
}

#ifndef EEC_CTC_LEN  // one copy of what takes no lengths: ctc_len.hip calls these
int ctc_states_per_lane(int S) {
  if (2 * S + 1 <= 64 * 2) return 2;
  if (2 * S + 1 <= 64 * 4) return 4;
  if (2 * S + 1 <= 64 * kCtcPerLane) return kCtcPerLane;
  return 0;
}

size_t ctc_store_floats(int E, int B, int Tq, int S) {
  const int P = ctc_states_per_lane(S);
  // the fast path's states and lane exponents, p(target) per lattice, the wide path's state exponents
  return P ? (size_t)E * B * Tq * (P + 1) * 64 + 2 * (size_t)E * B + (size_t)E * B * Tq * P * 64 : 0;
}
#endif

hipError_t launch_ctc_backward(const float* logp, const long long* targets, const long long* target_len,
                               EEC_LEN_PARAM(const int* input_len) int E, int B, int Tq, int V, int S, int blank, const float* nll, float* astore, const float* grad_loss, float* dlogp,
                               hipStream_t st) {
  const int P = ctc_states_per_lane(S), n_rows = E * B * Tq;
  if (!P || V > 256 || V % 4) return hipErrorInvalidValue;
#define EEC_CTC_BWD(P_)                                                                                                      \
  hipLaunchKernelGGL(ctc_beta_kernel<P_>, dim3(E * B), dim3(64), 0, st, logp, targets, target_len,                           \
                     EEC_LEN_PARAM(input_len) B, Tq, V, S, blank, nll, astore);                                              \
  hipLaunchKernelGGL(ctc_wide_kernel<P_>, dim3(E * B), dim3(64), 0, st, logp, targets, target_len,                           \
                     EEC_LEN_PARAM(input_len) B, Tq, V, S, blank, (float*)nullptr, astore);                                  \
  hipLaunchKernelGGL(ctc_grad_kernel<P_>, dim3((n_rows + 3) / 4), dim3(256), 0, st, logp, targets, target_len,               \
                     EEC_LEN_PARAM(input_len) B, Tq, V, S, blank, nll, astore, grad_loss, n_rows, dlogp);
  if (P == 2) {
    EEC_CTC_BWD(2)
  } else if (P == 4) {
    EEC_CTC_BWD(4)
  } else {
    EEC_CTC_BWD(kCtcPerLane)
  }
#undef EEC_CTC_BWD
  return hipGetLastError();
}

#ifndef EEC_CTC_LEN
// loss_e = mean_b( zero_inf(nll[e][b]) / max(len_b, 1) ): fixed summation order (bitwise reproducible).  The 64 lanes fetch 64
// utterances' terms at once; lane order is then added up sequentially out of registers (one thread walking the batch with two
// dependent loads per utterance took 10.7 us per launch: 0.4 % of the headline step).
__global__ void ctc_reduce_kernel(const float* nll, const long long* target_len, int B, float* out) {
  const int e = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    float term = 0.f;
    if (b < B) {
      float v = nll[e * B + b];
      if (isinf(v)) v = 0.f;  // zero_infinity=True zeroes infinite losses only: NaN (bad input) propagates
      const long long l = target_len[b] > 0 ? target_len[b] : 1;
      term = v / (float)l;
    }
    const int n = min(64, B - b0);
    for (int i = 0; i < n; ++i) s += __shfl(term, i, 64);
  }
  if (lane == 0) out[e] = s / (float)B;
}

hipError_t launch_ctc_reduce(const float* nll, const long long* target_len, int E, int B, float* out, hipStream_t st) {
  hipLaunchKernelGGL(ctc_reduce_kernel, dim3(E), dim3(64), 0, st, nll, target_len, B, out);
  return hipGetLastError();
}
#endif

hipError_t launch_ctc_loss(const float* logp, const long long* targets, const long long* target_len,
                           EEC_LEN_PARAM(const int* input_len) int E, int B, int Tq, int V, int S, int blank, float* nll, float* out, float* astore, hipStream_t st) {
  // state count 2*S+1 must fit 64 lanes x P
  const int P = ctc_states_per_lane(S);
  if (!P) return hipErrorInvalidValue;
  // the training forward keeps the block-floating recursion (the backward pass needs its stored alphas) and leaves the
  // lattices it marked to the loss kernel; the loss alone is the loss kernel on every lattice
#define EEC_CTC_FWD(P_)                                                                                                      \
  if (astore)                                                                                                                \
    hipLaunchKernelGGL(ctc_alpha_kernel<P_>, dim3(E * B), dim3(64), 0, st, logp, targets, target_len,                        \
                       EEC_LEN_PARAM(input_len) B, Tq, V, S, blank, nll, astore);                                            \
  hipLaunchKernelGGL(ctc_loss_kernel<P_>, dim3(E * B), dim3(128), 0, st, logp, targets, target_len,                          \
                     EEC_LEN_PARAM(input_len) B, Tq, V, S, blank, astore ? 1 : 0, nll);
  if (P == 2) {
    EEC_CTC_FWD(2)
  } else if (P == 4) {
    EEC_CTC_FWD(4)
  } else {
    EEC_CTC_FWD(kCtcPerLane)
  }
#undef EEC_CTC_FWD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_ctc_reduce(nll, target_len, E, B, out, st);
}

#ifndef EEC_CTC_LEN
// dlogits = g - exp(logp) * sum_c g  (backward of log_softmax over the last axis); one wave per row, V <= 256, V % 4 == 0
__global__ __launch_bounds__(256) void logsoftmax_bwd_kernel(const float* __restrict__ logp, const float* __restrict__ g, int M, int V,
                                                             float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int c0 = lane * 4;
  float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), lv = gv;
  if (c0 < V) {
    gv = *(const float4*)(g + (size_t)row * V + c0);
    lv = *(const float4*)(logp + (size_t)row * V + c0);
  }
  const float sum = wave_sum(gv.x + gv.y + gv.z + gv.w);
  if (c0 < V)
    *(float4*)(dlogits + (size_t)row * V + c0) = make_float4(gv.x - __expf(lv.x) * sum, gv.y - __expf(lv.y) * sum,
                                                             gv.z - __expf(lv.z) * sum, gv.w - __expf(lv.w) * sum);
}

hipError_t launch_logsoftmax_backward(const float* logp, const float* g, int M, int V, float* dlogits, hipStream_t st) {
  if (V > 256 || V % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(logsoftmax_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, st, logp, g, M, V, dlogits);
  return hipGetLastError();
}
#endif

}  // namespace eec
