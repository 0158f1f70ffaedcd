// CTC prefix beam search on the device: what the reference's CTC inference calls through
// torchaudio's cuda_ctc_decoder(nbest=1, beam_size=10, blank_skip_threshold=0.95) (util/beam_infer.py:79-80,102-112,
// inference.py:65-77).  That decoder is third-party CUDA code outside the reference tree: the algorithm restated here is
// the published prefix beam search without a language model (oracle/ctc_beam_ref.py is its CPU statement, and the judge
// of this kernel) -- per frame every prefix stays or is extended by a label, extensions that spell an existing prefix
// merge into it, the `beam` most probable prefixes survive; frames whose blank probability exceeds the threshold are taken
// as blank frames without expansion.
//
// One 256-thread workgroup per sequence; thread c owns label c (V <= 256): its log-prob and its `beam` extension scores
// live in registers, the beam (<= 16 prefixes: two log-probabilities, last label, length, 64-bit prefix hash) in LDS.
// Survivors are picked by `beam` rounds of a block-wide arg-max (DPP wave maximum + ballot, 4 wave winners through LDS);
// ties go to the lower candidate id.  Prefixes are not copied: every frame records (parent beam, appended label) per
// survivor in a back-pointer table and the best prefix is read off backwards at the end.  Latency-bound integer / scalar
// work (T' serial frames): it is sized to keep all E*B sequences of a batch in flight at once, not for the roofline.
// Input lengths: `em_len` [n_seq] is a device array of frame counts, or nullptr for T' frames everywhere.  Sequence s is its
// first Ts = ctc_frames(em_len, s, T') = clamp(em_len[s], 0, T') frames (eec_kernels.h) and the back-trace starts at Ts - 1;
// Ts = 0 leaves the empty prefix: count 0, score 0.  The rows of `tokens` and of the back-pointer table stay T' apart.
// One kernel, two ENDS, chosen by `n_hyp` (block-uniform).  nullptr (eec_ctc_beam_decode and its _ex / _len forms): the best
// prefix, traced back by one work-item.  Otherwise (eec_ctc_beam_decode_nbest) the final beam is ranked by
// total log-probability (ties to the lower beam index) and the first min(nbest, live beams) prefixes are traced back, one
// work-item per hypothesis, into tokens [n_seq][nbest][T'], counts / scores [n_seq][nbest] and n_hyp [n_seq].  The first end is
// NOT the second with nbest = 1: when no prefix is live (nb_s == 0: every candidate of a frame was -inf) the N-best end reports
// count 0 and n_hyp = 0, the best-prefix end the length of slot 0 and score -inf.
// Contextual biasing: EEC_CTC_CTX compiles this file a second time (ctc_beam_ctx.hip) into ctc_beam_ctx_kernel and the _ctx entries,
// the same search ranked by key = fl(total + bias) (include/eec.h, "Contextual biasing").  A beam grows by `int state; float bias`;
// work-item c reads delta[state_i][c] of every live beam i (one coalesced row per beam), the owner of a chosen extension reads its one
// `next` entry and recomputes the extension's CTC mass from lpc, since the number that was ranked is the key.  Without the switch
// every line of it is compiled out: the object of this file is the one it was.
// Shallow fusion: EEC_CTC_LM compiles it a third time (ctc_beam_lm.hip) into ctc_beam_lm_kernel and the _lm entries (include/eec.h,
// "Shallow fusion").  The same two fields and the same ranking by key -- the lines both switches share stand under EEC_CTC_BIAS --;
// the per-label increment is a back-off walk instead of a table row, so a beam's V increments are kept in LDS (work-item c owns
// column c of every row: no barrier of their own) and follow the beam through stays and skipped frames; only a new extension walks.
#include <limits.h>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"
#if defined(EEC_CTC_CTX) && defined(EEC_CTC_LM)
#error "a context graph and a language model in one CTC search are not served"
#endif
#ifdef EEC_CTC_CTX
#include "eec_ctx.h"
#define EEC_CTC_BIAS 1
#define CbBeam CbBeamCtx
#define ctc_beam_kernel ctc_beam_ctx_kernel
#define launch_ctc_beam launch_ctc_beam_ctx
#define CB_CTX_ARGS(...) , __VA_ARGS__
#define CB_LM_ARGS(...)
#elif defined(EEC_CTC_LM)
#include "eec_lm.h"
#define EEC_CTC_BIAS 1
#define CbBeam CbBeamLm
#define ctc_beam_kernel ctc_beam_lm_kernel
#define launch_ctc_beam launch_ctc_beam_lm
#define CB_CTX_ARGS(...)
#define CB_LM_ARGS(...) , __VA_ARGS__
#else
#define CB_CTX_ARGS(...)
#define CB_LM_ARGS(...)
#endif
#ifdef EEC_CTC_BIAS
#define CB_CTX(...) , __VA_ARGS__  // the two fields a beam grows by, at the end of its initialiser
#else
#define CB_CTX(...)
#endif

namespace eec {

constexpr int kCbMaxBeam = 16;
constexpr int kCbThreads = 256;

struct CbBeam {
  float pb, pnb;
  int last, len;
  unsigned long long hash;
#ifdef EEC_CTC_BIAS
  int state;
  float bias;
#endif
};

__device__ __forceinline__ float cb_lae(float a, float b) {  // log(exp a + exp b), -inf safe
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1pf(__expf(-fabsf(a - b)));
}
__device__ __forceinline__ unsigned long long cb_mix(unsigned long long h, int c) {
  unsigned long long z = h ^ ((unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kCbThreads) void ctc_beam_kernel(const float* __restrict__ logp, const int* __restrict__ em_len,
                                                              int Tq, int V, int blank, int beam,
                                                              float log_thr, int skip_drops, int* __restrict__ backptr, int* __restrict__ tokens,
                                                              int* __restrict__ counts, float* __restrict__ scores,
                                                              int nbest, int* __restrict__ n_hyp
                                                              CB_CTX_ARGS(const int* __restrict__ image, long long image_words,
                                                                          const int* __restrict__ graph_of, float* __restrict__ bias_out)
                                                              CB_LM_ARGS(const int* __restrict__ image, long long image_words,
                                                                         float lm_weight, float token_score, float* __restrict__ bias_out)) {
  __shared__ CbBeam bufs[2][kCbMaxBeam];
  __shared__ float tot[kCbMaxBeam], stay_pb[kCbMaxBeam], stay_pnb[kCbMaxBeam], row[256];
  __shared__ unsigned merge_mask[kCbMaxBeam];  // bit i of word j: extension of beam i by last[j] spells beam j
  __shared__ float red_v[4];
  __shared__ int red_id[4];
  __shared__ int nb_s;
  const int seq = blockIdx.x, c = threadIdx.x, lane = c & 63, w = c >> 6;
  const float* lp_seq = logp + (size_t)seq * Tq * V;
  int* bp = backptr + (size_t)seq * Tq * kCbMaxBeam;
  const int Ts = ctc_frames(em_len, seq, Tq);
#ifdef EEC_CTC_BIAS
  __shared__ float fin_key[kCbMaxBeam], fin_bias[kCbMaxBeam];
#endif
#ifdef EEC_CTC_CTX
  const CtxTables G = ctx_tables(image, image_words, graph_of, seq, V);  // all-null: biasing is off for this sequence
  const int start = 0;
#endif
#ifdef EEC_CTC_LM
  __shared__ float inc_s[2][kCbMaxBeam][kCbThreads];  // inc(state of beam i, label c), of the beams of the frame and of the next one
  __shared__ int chosen[kCbMaxBeam];                  // the candidate id behind every new beam
  const TlmView G = tlm_view(image, image_words, V);
  const bool fused = G.on && !(lm_weight == 0.f && token_score == 0.f);  // off: every increment is 0
  const int start = G.on ? tlm_node(G, G.m.bos) : 0;
  // the increment of label c from `state`; the blank is never an extension
  auto inc_of = [&](int state) -> float {
    if (!fused || c >= V || c == blank) return 0.f;
    int next;
    return tlm_inc(lm_weight, tlm_walk(G, tlm_node(G, state), tlm_word(G, c), next), token_score);
  };
  int icur = 0;
  inc_s[0][0][c] = inc_of(start);
#endif
  int cur = 0;
  if (c == 0) {
    bufs[0][0] = CbBeam{0.f, -INFINITY, -1, 0, 0x243F6A8885A308D3ull CB_CTX(start, 0.f)};
    nb_s = 1;
  }
  __syncthreads();
  for (int t = 0; t < Ts; ++t) {
    const CbBeam* B = bufs[cur];
    CbBeam* N = bufs[cur ^ 1];
    const int nb = nb_s;
    const float lpc = c < V ? lp_seq[(size_t)t * V + c] : -INFINITY;
    row[c] = lpc;
    __syncthreads();
    const float lpb = row[blank];
    if (lpb > log_thr) {  // blank-dominated frame, not expanded
      if (c < nb) {
        // skip_drops == 0: the frame counts as a blank frame (all mass ends in blank: a label repeated across it stays a repeat)
        // skip_drops != 0: the frame is DROPPED, as if the sequence were one frame shorter (the repeat collapses)
        N[c] = skip_drops ? B[c] : CbBeam{cb_lae(B[c].pb, B[c].pnb) + lpb, -INFINITY, B[c].last, B[c].len, B[c].hash CB_CTX(B[c].state, B[c].bias)};
        bp[t * kCbMaxBeam + c] = c << 16;
      }
      __syncthreads();
      cur ^= 1;
      continue;
    }
    if (c < nb) {
      const float tt = cb_lae(B[c].pb, B[c].pnb);
      tot[c] = tt;
      stay_pb[c] = tt + lpb;
      stay_pnb[c] = B[c].last >= 0 ? B[c].pnb + row[B[c].last] : -INFINITY;
      // which beams i, extended by this beam's last label, spell this beam?
      unsigned m = 0;
      if (B[c].last >= 0)
        for (int i = 0; i < nb; ++i)
          if (i != c && B[i].len + 1 == B[c].len && cb_mix(B[i].hash, B[c].last) == B[c].hash) m |= 1u << i;
      merge_mask[c] = m;
    }
    __syncthreads();
    if (c < nb && merge_mask[c]) {  // fold those extensions into this beam's "stay" candidate (ascending i: fixed order)
      float acc = stay_pnb[c];
      for (int i = 0; i < nb; ++i)
        if (merge_mask[c] >> i & 1) acc = cb_lae(acc, (B[i].last == B[c].last ? B[i].pb : tot[i]) + row[B[c].last]);
      stay_pnb[c] = acc;
    }
    __syncthreads();
    // this label's extension of every beam (killed where it merged into an existing prefix), and the stays
    float ext[kCbMaxBeam];
#pragma unroll
    for (int i = 0; i < kCbMaxBeam; ++i) {
      float v = -INFINITY;
      if (i < nb && c != blank && c < V) {
        v = (B[i].last == c ? B[i].pb : tot[i]) + lpc;
        for (int j = 0; j < nb; ++j)
          if (B[j].last == c && (merge_mask[j] >> i & 1)) v = -INFINITY;
#ifdef EEC_CTC_CTX
        v = v + (B[i].bias + (G.delta ? G.delta[(size_t)B[i].state * V + c] : 0.f));  // the key; -inf stays -inf
#endif
#ifdef EEC_CTC_LM
        v = v + (B[i].bias + inc_s[icur][i][c]);  // the key; -inf stays -inf
#endif
      }
      ext[i] = v;
    }
#ifdef EEC_CTC_BIAS
    float stay = c < nb ? cb_lae(stay_pb[c], stay_pnb[c]) + B[c].bias : -INFINITY;
#else
    float stay = c < nb ? cb_lae(stay_pb[c], stay_pnb[c]) : -INFINITY;
#endif
    // `beam` rounds of block-wide arg-max; candidate id: stays = beam index (0 .. 15), extensions = 16 + 16 c + i
    int n_new = 0;
    for (int r = 0; r < beam; ++r) {
      float bv = stay;
      int bid = c < nb ? c : INT_MAX;
#pragma unroll
      for (int i = 0; i < kCbMaxBeam; ++i)
        if (ext[i] > bv || (ext[i] == bv && ext[i] > -INFINITY && 16 + 16 * c + i < bid)) {
          bv = ext[i];
          bid = 16 + 16 * c + i;
        }
      if (bv == -INFINITY) bid = INT_MAX;
      const float wm = wave_max(bv);
      int cand = (bv == wm && wm > -INFINITY) ? bid : INT_MAX;
      // lowest id among the lanes that hold the wave maximum (written out: as a shared eec_wave.h function its last exchange is scheduled elsewhere)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) cand = min(cand, __shfl_xor(cand, off, 64));
      if (lane == 0) {
        red_v[w] = wm;
        red_id[w] = cand;
      }
      __syncthreads();
      float gv = red_v[0];
      int gid = red_id[0];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (red_v[k] > gv || (red_v[k] == gv && red_id[k] < gid)) {
          gv = red_v[k];
          gid = red_id[k];
        }
      if (gv == -INFINITY || gid == INT_MAX) {
        __syncthreads();
        break;
      }
      if (gid < 16) {  // a stay: its owner is thread gid
        if (c == gid) {
          N[r] = CbBeam{stay_pb[c], stay_pnb[c], B[c].last, B[c].len, B[c].hash CB_CTX(B[c].state, B[c].bias)};
          bp[t * kCbMaxBeam + r] = c << 16;
          stay = -INFINITY;
#ifdef EEC_CTC_LM
          chosen[r] = gid;
#endif
        }
      } else {
        const int cc = (gid - 16) >> 4, ii = (gid - 16) & 15;
        if (c == cc) {
#ifdef EEC_CTC_CTX
          const size_t at = (size_t)B[ii].state * V + cc;
          N[r] = CbBeam{-INFINITY, (B[ii].last == cc ? B[ii].pb : tot[ii]) + lpc, cc, B[ii].len + 1, cb_mix(B[ii].hash, cc),
                        G.delta ? ctx_state(G.next[at], G.S) : 0, B[ii].bias + (G.delta ? G.delta[at] : 0.f)};
#elif defined(EEC_CTC_LM)
          int next = start;
          if (fused) tlm_walk(G, tlm_node(G, B[ii].state), tlm_word(G, cc), next);
          N[r] = CbBeam{-INFINITY, (B[ii].last == cc ? B[ii].pb : tot[ii]) + lpc, cc, B[ii].len + 1, cb_mix(B[ii].hash, cc), next,
                        B[ii].bias + inc_s[icur][ii][cc]};
          chosen[r] = gid;
#else
          N[r] = CbBeam{-INFINITY, gv, cc, B[ii].len + 1, cb_mix(B[ii].hash, cc)};
#endif
          bp[t * kCbMaxBeam + r] = (ii << 16) | (cc + 1);
#pragma unroll
          for (int i = 0; i < kCbMaxBeam; ++i)
            if (i == ii) ext[i] = -INFINITY;
        }
      }
      n_new = r + 1;
      __syncthreads();
    }
    if (c == 0) nb_s = n_new;
    __syncthreads();
#ifdef EEC_CTC_LM
    // the new beams' increments: a stay takes its row along, an extension walks from its new state (column c only: no barrier)
    for (int r = 0; r < n_new; ++r) inc_s[icur ^ 1][r][c] = chosen[r] < 16 ? inc_s[icur][chosen[r]][c] : inc_of(N[r].state);
    icur ^= 1;
#endif
    cur ^= 1;
  }
#ifdef EEC_CTC_LM
  // the end of the sentence: fl(lm_weight * acc(</s>)) from a prefix's state, when the model has </s>
  auto fin_of = [&](int state) -> float {
#pragma clang fp contract(off)
    if (!fused || G.m.eos < 0) return 0.f;
    int next;
    const float term = lm_weight * tlm_walk(G, tlm_node(G, state), G.m.eos, next);
    return term;
  };
#endif
  if (n_hyp) {  // block-uniform
    // N-best: thread i < live beams ranks prefix i (the number of prefixes ahead of it: a higher total, or the same total and a
    // lower index) and, if it is among the first nbest, reads its labels off the back-pointers into row `rank` of the sequence
    if (c < kCbMaxBeam) tot[c] = c < nb_s ? cb_lae(bufs[cur][c].pb, bufs[cur][c].pnb) : -INFINITY;
#ifdef EEC_CTC_BIAS
    // the open bonus is taken back (the model's </s> is paid), and the ranking is by the key: total + that final bias
    if (c < kCbMaxBeam) {
#ifdef EEC_CTC_CTX
      const float b = c < nb_s ? bufs[cur][c].bias + (G.delta ? G.fin[ctx_state(bufs[cur][c].state, G.S)] : 0.f) : 0.f;
#else
      const float b = c < nb_s ? bufs[cur][c].bias + fin_of(bufs[cur][c].state) : 0.f;
#endif
      fin_bias[c] = b;
      fin_key[c] = tot[c] + b;
    }
    const float* rank_by = fin_key;
#else
    const float* rank_by = tot;
#endif
    __syncthreads();
    const int live = nb_s, n_out = min(live, nbest);
    if (c < live) {
      const CbBeam* B = bufs[cur];
      const float s = rank_by[c];
      int rank = 0;
      for (int j = 0; j < live; ++j) rank += (rank_by[j] > s || (rank_by[j] == s && j < c)) ? 1 : 0;
      if (rank < nbest) {
        int n = B[c].len, k = c;
        int* out = tokens + ((size_t)seq * nbest + rank) * Tq;
        counts[(size_t)seq * nbest + rank] = n;
        scores[(size_t)seq * nbest + rank] = tot[c];
#ifdef EEC_CTC_BIAS
        bias_out[(size_t)seq * nbest + rank] = fin_bias[c];
#endif
        for (int t = Ts - 1; t >= 0 && n > 0; --t) {
          const int e = bp[t * kCbMaxBeam + k];
          if (e & 0xffff) out[--n] = (e & 0xffff) - 1;
          k = e >> 16;
        }
      }
    }
    if (c >= n_out && c < nbest) {  // absent hypotheses
      counts[(size_t)seq * nbest + c] = 0;
      scores[(size_t)seq * nbest + c] = -INFINITY;
#ifdef EEC_CTC_BIAS
      bias_out[(size_t)seq * nbest + c] = 0.f;
#endif
    }
    if (c == 0) n_hyp[seq] = n_out;
  } else if (c == 0) {
    // best prefix: highest total, ties to the lower beam index; read the labels off the back-pointers
    const CbBeam* B = bufs[cur];
    int best = 0;
    float bs = -INFINITY;
#ifdef EEC_CTC_BIAS
    float best_key = -INFINITY, best_bias = 0.f;
    for (int i = 0; i < nb_s; ++i) {
      const float s = cb_lae(B[i].pb, B[i].pnb);
#ifdef EEC_CTC_CTX
      const float b = B[i].bias + (G.delta ? G.fin[ctx_state(B[i].state, G.S)] : 0.f);
#else
      const float b = B[i].bias + fin_of(B[i].state);
#endif
      if (s + b > best_key) {
        best_key = s + b;
        bs = s;
        best_bias = b;
        best = i;
      }
    }
    bias_out[seq] = best_bias;
#else
    for (int i = 0; i < nb_s; ++i) {
      const float s = cb_lae(B[i].pb, B[i].pnb);
      if (s > bs) {
        bs = s;
        best = i;
      }
    }
#endif
    int n = B[best].len, k = best;
    int* out = tokens + (size_t)seq * Tq;
    counts[seq] = n;
    scores[seq] = bs;
    for (int t = Ts - 1; t >= 0 && n > 0; --t) {
      const int e = bp[t * kCbMaxBeam + k];
      if (e & 0xffff) out[--n] = (e & 0xffff) - 1;
      k = e >> 16;
    }
  }
}

// n_hyp != nullptr: the N-best end, into `nbest` rows per sequence; nullptr: the best prefix (nbest is not read)
hipError_t launch_ctc_beam(const float* logp, const int* em_len, int n_seq, int Tq, int V, int blank, int beam, float blank_skip_threshold,
                           int skip_drops, int* backptr, int* tokens, int* counts, float* scores, int nbest, int* n_hyp, hipStream_t st
                           CB_CTX_ARGS(const int* image, long long image_words, const int* graph_of, float* bias)
                           CB_LM_ARGS(const int* image, long long image_words, float lm_weight, float token_score, float* bias)) {
  if (V < 1 || V > 256 || beam < 1 || beam > kCbMaxBeam || blank < 0 || blank >= V) return hipErrorInvalidValue;
  if (n_hyp && (nbest < 1 || nbest > beam)) return hipErrorInvalidValue;
  const float log_thr = (blank_skip_threshold > 0.f && blank_skip_threshold < 1.f) ? logf(blank_skip_threshold) : INFINITY;
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(n_seq), dim3(kCbThreads), 0, st, logp, em_len, Tq, V, blank, beam, log_thr, skip_drops, backptr, tokens,
                     counts, scores, nbest, n_hyp CB_CTX_ARGS(image, image_words, graph_of, bias)
                     CB_LM_ARGS(image, image_words, lm_weight, token_score, bias));
  return hipGetLastError();
}

}  // namespace eec

extern "C" {

#ifndef EEC_CTC_BIAS
size_t eec_ctc_beam_workspace_bytes(int n_seq, int Tq) {
  return n_seq > 0 && Tq > 0 ? (size_t)n_seq * Tq * eec::kCbMaxBeam * sizeof(int) : 0;
}
#endif

// what the beam entries ask of their arguments; `entry` is the name their messages carry
static int check_ctc_beam_args(const char* entry, bool have_pointers, int n_seq, int Tq, int V, int blank, int beam_size) {
  using eech::fail;
  const std::string name = entry;
  if (!have_pointers) return fail(EEC_ERR_BAD_ARG, name + ": null argument");
  if (n_seq <= 0 || Tq <= 0) return fail(EEC_ERR_BAD_ARG, name + ": n_seq and Tq must be positive");
  if (V < 1 || V > 256 || beam_size < 1 || beam_size > eec::kCbMaxBeam || blank < 0 || blank >= V)
    return fail(EEC_ERR_UNSUPPORTED, name + ": needs 1 <= V <= 256, 1 <= beam_size <= " + std::to_string(eec::kCbMaxBeam) + ", blank in [0, V)");
  return 0;
}

#ifndef EEC_CTC_BIAS
int eec_ctc_beam_decode(const float* logp, int n_seq, int Tq, int V, int blank, int beam_size, float blank_skip_threshold,
                        void* workspace, int32_t* tokens, int32_t* counts, float* scores, void* stream) {
  return eec_ctc_beam_decode_len(logp, NULL, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, 0, workspace, tokens, counts, scores, stream);
}

int eec_ctc_beam_decode_ex(const float* logp, int n_seq, int Tq, int V, int blank, int beam_size, float blank_skip_threshold,
                           int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts, float* scores, void* stream) {
  return eec_ctc_beam_decode_len(logp, NULL, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame, workspace, tokens, counts,
                                 scores, stream);
}

int eec_ctc_beam_decode_len(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                            float blank_skip_threshold, int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts,
                            float* scores, void* stream) {
  if (int rc = check_ctc_beam_args("eec_ctc_beam_decode", logp && workspace && tokens && counts && scores, n_seq, Tq, V, blank, beam_size)) return rc;
  EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                               counts, scores, 1, nullptr, (hipStream_t)stream));
  return 0;
}

int eec_ctc_beam_decode_nbest(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                              float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens, int32_t* counts,
                              float* scores, int32_t* n_hyp, void* stream) {
  if (int rc = check_ctc_beam_args("eec_ctc_beam_decode_nbest", logp && workspace && tokens && counts && scores && n_hyp, n_seq, Tq, V, blank,
                                   beam_size))
    return rc;
  if (nbest < 1 || nbest > beam_size) return eech::fail(EEC_ERR_BAD_ARG, "eec_ctc_beam_decode_nbest: needs 1 <= nbest <= beam_size");
  EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                               counts, scores, nbest, n_hyp, (hipStream_t)stream));
  return 0;
}
#elif defined(EEC_CTC_CTX)
// the _len / _nbest entries with a graph image (a device pointer, or NULL: no biasing), graph_of [n_seq] (NULL: graph 0) and `bias`
static int check_ctx_image(const char* entry, const void* image, size_t image_bytes) {
  if (image && (((uintptr_t)image & 3) != 0 || image_bytes < 16)) return eech::fail(EEC_ERR_BAD_ARG, std::string(entry) + ": image must be 4-byte aligned, image_bytes its size");
  return 0;
}

int eec_ctc_beam_decode_ctx(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                            float blank_skip_threshold, int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts,
                            float* scores, const void* image, size_t image_bytes, const int32_t* graph_of, float* bias, void* stream) {
  if (int rc = check_ctc_beam_args("eec_ctc_beam_decode_ctx", logp && workspace && tokens && counts && scores && bias, n_seq, Tq, V, blank, beam_size))
    return rc;
  if (int rc = check_ctx_image("eec_ctc_beam_decode_ctx", image, image_bytes)) return rc;
  EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                               counts, scores, 1, nullptr, (hipStream_t)stream, (const int*)image, (long long)(image_bytes / 4), graph_of, bias));
  return 0;
}

int eec_ctc_beam_decode_nbest_ctx(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                                  float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens,
                                  int32_t* counts, float* scores, int32_t* n_hyp, const void* image, size_t image_bytes,
                                  const int32_t* graph_of, float* bias, void* stream) {
  if (int rc = check_ctc_beam_args("eec_ctc_beam_decode_nbest_ctx", logp && workspace && tokens && counts && scores && n_hyp && bias, n_seq, Tq, V,
                                   blank, beam_size))
    return rc;
  if (nbest < 1 || nbest > beam_size) return eech::fail(EEC_ERR_BAD_ARG, "eec_ctc_beam_decode_nbest_ctx: needs 1 <= nbest <= beam_size");
  if (int rc = check_ctx_image("eec_ctc_beam_decode_nbest_ctx", image, image_bytes)) return rc;
  EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                               counts, scores, nbest, n_hyp, (hipStream_t)stream, (const int*)image, (long long)(image_bytes / 4), graph_of, bias));
  return 0;
}
#else
// the _len / _nbest entries with a model image (a device pointer, or NULL: no fusion), its weight, the per-token bonus and `fusion`
static int check_lm_args(const char* entry, const void* lm, size_t lm_bytes, float lm_weight, float token_score) {
  const std::string name = entry;
  if (lm && (((uintptr_t)lm & 3) != 0 || lm_bytes < 64)) return eech::fail(EEC_ERR_BAD_ARG, name + ": lm must be 4-byte aligned, lm_bytes its size");
  if (!isfinite(lm_weight) || !isfinite(token_score)) return eech::fail(EEC_ERR_BAD_ARG, name + ": lm_weight and token_score must be finite");
  return 0;
}

int eec_ctc_beam_decode_lm(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                           float blank_skip_threshold, int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts,
                           float* scores, const void* lm, size_t lm_bytes, float lm_weight, float token_score, float* fusion, void* stream) {
  if (int rc = check_ctc_beam_args("eec_ctc_beam_decode_lm", logp && workspace && tokens && counts && scores && fusion, n_seq, Tq, V, blank, beam_size))
    return rc;
  if (int rc = check_lm_args("eec_ctc_beam_decode_lm", lm, lm_bytes, lm_weight, token_score)) return rc;
  EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                               counts, scores, 1, nullptr, (hipStream_t)stream, (const int*)lm, (long long)(lm_bytes / 4), lm_weight, token_score,
                               fusion));
  return 0;
}

int eec_ctc_beam_decode_nbest_lm(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                                 float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens,
                                 int32_t* counts, float* scores, int32_t* n_hyp, const void* lm, size_t lm_bytes, float lm_weight,
                                 float token_score, float* fusion, void* stream) {
  if (int rc = check_ctc_beam_args("eec_ctc_beam_decode_nbest_lm", logp && workspace && tokens && counts && scores && n_hyp && fusion, n_seq, Tq, V,
                                   blank, beam_size))
    return rc;
  if (nbest < 1 || nbest > beam_size) return eech::fail(EEC_ERR_BAD_ARG, "eec_ctc_beam_decode_nbest_lm: needs 1 <= nbest <= beam_size");
  if (int rc = check_lm_args("eec_ctc_beam_decode_nbest_lm", lm, lm_bytes, lm_weight, token_score)) return rc;
  EEC_HIP(eec::launch_ctc_beam(logp, em_len, n_seq, Tq, V, blank, beam_size, blank_skip_threshold, skip_drops_frame != 0, (int*)workspace, tokens,
                               counts, scores, nbest, n_hyp, (hipStream_t)stream, (const int*)lm, (long long)(lm_bytes / 4), lm_weight,
                               token_score, fusion));
  return 0;
}
#endif

}  // extern "C"
