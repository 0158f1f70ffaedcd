// Lexicon-constrained CTC beam search on the device, with N-best: what the reference's ctc_predict / ctc_predict_ / beam_predict
// call through torchaudio's ctc_decoder(lexicon=..., tokens=..., nbest=N_BEST, log_add=False, word_score=w_ins, sil_token="<pad>",
// blank_token="@", lm=..., lm_weight=LM_WEIGHT) (util/beam_infer.py:39-78, 85-126), without a language model
// (eec_ctc_lexbeam_decode) or with a back-off n-gram model read from an ARPA file (eec_ctc_lexbeam_lm_decode).  That decoder
// (flashlight-text) is third-party code outside the reference tree and not installed: what is built is the published algorithm --
// token-trie beam search under CTC, Viterbi merging (log_add=False), the word model's score at every word end and its end-of-sentence
// term -- stated completely in include/eec.h; tests/lexbeam_cases.py and tests/lexbeam_lm_cases.py are its plain-Python statement
// and the judge of this kernel.  Parity with the third-party decoder is unpinned.
// log_add=True, the reference's character-lexicon branch (util/beam_infer.py:66-75), is eec_ctc_lexbeam_logadd_decode: the same
// search with the merged hypotheses' probabilities summed (the LA instantiations, at the end of this comment).
// Out of scope: unknown-word scores other than through the model's <unk>, binary KenLM files, beams over 64 (17 to 64: ctc_lexbeam_wide.hip).
//
// What is here and what is not.  Here: this kernel's own strategy -- a thread's candidates in registers, the pairwise merge, the
// arg-max rounds -- and the host path of ALL six entries, the wide one included (lb_decode: one copy of the argument checks, one
// ladder over the instantiations).  In eec_lexbeam.h, shared with the wide kernel: the set-up before the first frame (lb_context,
// lb_start), the child-lookup table (lb_fill_slots), the candidate rules (lb_expand: the only device statement of them), a
// survivor's beam entry and back-pointer (lb_survive) and the epilogue (lb_epilogue).  In lexpack.hip: the host packers of the
// three images.
//
// One 256-thread workgroup per sequence, one launch for the batch; thread c owns frame label c (V <= 256).  All candidates that
// can merge share their frame label, so every merge is local to one thread.  Per frame:
//   * the beam (<= 16 hypotheses: trie node with its child range, last label, 64-bit history hash, score, token and word counts)
//     lives in LDS, double-buffered;
//   * child lookup is a scatter instead of a search (lb_fill_slots): for beam entry i the first deg(node_i) threads read the node's
//     child bytes (one coalesced load) and write "edge offset" into a byte table slot[i][label] in LDS; thread c then reads
//     slot[i][c].  The breadth-first node numbering makes the child of edge k node k + 1, so the table needs no target;
//   * thread c holds, per beam entry, what lb_expand gives its label -- at most one in-place / in-word candidate (blank, repeat,
//     child, sil: w = 0) and one word-end candidate (w = 1) -- in registers at the unrolled index, merges equal (node, history) keys among its <= 32 candidates (the higher score survives, the
//     lower id on a tie), and `beam` rounds of a block-wide arg-max on (score, id) pick the survivors; a thread rescans its own
//     candidates only after it won a round.  The first round's winner gives the beam threshold;
//   * every survivor leaves (parent rank, label, completed word + 1) in a back-pointer table, 8 bytes per (frame, rank).
// At the end the complete hypotheses (node 0) are already in rank order; up to nbest threads walk their back-pointers, one each.
// In the three Viterbi entries scores are fp32 additions in the order include/eec.h writes them, no reductions, no log / exp: the
// result is bit-identical to the statement.  Latency-bound integer / scalar work over T' serial frames: it is sized to keep all E * B = 384 sequences of a
// batch in flight at once (5.4 KB of LDS, well under two workgroups per CU), not for the roofline.  The real lexicon's image
// (89 114 words, 162 621 nodes, 1.5 MB) is read-only and shared by all workgroups: it sits in L2.
//
// With a model (ctc_lexbeam_kernel<LM = true, ..>; LM = false is the search without one) a hypothesis also carries an LM state, a node
// of the packed n-gram image (layout in include/eec.h).  The back-off walk -- a binary search over the state's edge range, then the
// suffix link -- runs where a word-end candidate is formed; only the candidate's score is kept, and the at most `beam` word-end
// candidates that win a round redo their walk for the state they continue from.  After the last frame one thread adds the </s>
// term to the complete hypotheses and orders the at most 16 of them by insertion.
//
// With LM look-ahead (ctc_lexbeam_kernel<true, SM = true, ..>, eec_ctc_lexbeam_lm_smear_decode) the trie is smeared with the MAX mode, as
// the third-party decoder always does: a host-built table (eec_ctc_trie_smear) gives every node the best start-state score of the
// words at or below it, a step into a node is charged the increase of that maximum, and a word end takes the advance payment back.
// smax[y] is loaded beside cbeg[y] / word_of[y]; the payment outstanding at a hypothesis' node rides in its beam entry in LDS and is
// written by the round's winner.  The instantiations without it do not see any of it: their beam entry is the plain one, and of
// the one argument struct they never read the table's pointer.
//
// With log-add merging (LA = true on any of the three, eec_ctc_lexbeam_logadd_decode) a thread keeps, beside the raw score of each of
// its <= 32 candidates, an accumulator that starts as the raw score (32 KB of LDS per workgroup, a column per thread, touched only by
// threads with two or more live candidates: as registers they pushed the kernel past 256 and the CU down to one workgroup).  The pairwise merge loop is the Viterbi one -- the raw scores
// decide who is eliminated, in the same pair order --, and at every elimination the winner's accumulator takes log_add(winner's,
// loser's): that pair order IS the fold order include/eec.h states.  After the loop the accumulators replace the scores, so the
// rounds, the threshold and the beam work on merged scores.  log_add is the fixed fp32 sequence stated in include/eec.h (lb_log_add
// in eec_lexbeam.h: add, subtract, multiply, compare, rintf, ldexpf; no libm transcendental, no division), the same function on the
// host: the LA entries are bit-identical to the statement, whose log_add is that sequence.  It is called out of line
// (lb_log_add_call: merges are rare per thread and frame; 496 inlined copies would not be).
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"
#include "eec_lexbeam.h"

namespace eec {

__global__ void ctc_log_add_kernel(const float* a, const float* b, float* out, int n) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) out[k] = lb_log_add(a[k], b[k]);
}

// SM (with LM only): LM look-ahead by the smear table.  LA: log-add merging instead of Viterbi merging
template <bool LM, bool SM, bool LA>
__global__ __launch_bounds__(kLbThreads) void ctc_lexbeam_kernel(const LbArgs a) {
  static_assert(LM || !SM, "smearing needs a model");
  using Beam = LbBeamOf<SM>;
  __shared__ Beam bufs[2][kLbMaxBeam];
  __shared__ __attribute__((aligned(16))) unsigned char slot[kLbMaxBeam][256];  // edge offset of label c below beam i's node
  __shared__ float red_v[4];
  __shared__ int red_id[4];
  __shared__ int fin_rank[kLbMaxBeam], fin_ntok[kLbMaxBeam], fin_nw[kLbMaxBeam], fin_n;
  __shared__ float fin_score[LM ? kLbMaxBeam : 1];  // with a model: the final scores, </s> term included
  const int c = threadIdx.x, lane = c & 63, w = c >> 6;
  const int V = a.V, beam = a.beam;
  const LbCtx cx = lb_context<LM, SM>(a, blockIdx.x);
  const int L = cx.L;

  int cur = 0, nb = 1;
  float lp_next = lb_start<LM, SM>(a, cx, &bufs[0][0], c);
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const Beam* B = bufs[cur];
    Beam* N = bufs[cur ^ 1];
    const float lpc = lp_next;
    if (t + 1 < L && c < V) lp_next = cx.lp_seq[(size_t)(t + 1) * V + c];  // one frame ahead of its use

    lb_fill_slots(slot, B, nb, cx.ctok, c);

    // this label's candidates from every beam entry: s0 = blank / repeat / in-word child / sil, s1 = word end
    float s0[kLbMaxBeam], s1[kLbMaxBeam];
    int nd0[kLbMaxBeam], beg0[kLbMaxBeam], deg0[kLbMaxBeam], wd[kLbMaxBeam];
    unsigned long long h0[kLbMaxBeam], h1[kLbMaxBeam];
    int live = 0;
    // i < nb, compared afresh at every use: as one common expression the sixteen comparisons become sixteen lane masks in scalar
    // registers that stay live across the frame and push others out
    auto in_beam = [&](int i) {
      int n = nb;
      asm volatile("" : "+s"(n));
      return i < n;
    };
#pragma unroll
    for (int i = 0; i < kLbMaxBeam; ++i) {
      s0[i] = s1[i] = -INFINITY;
      nd0[i] = beg0[i] = deg0[i] = 0;
      wd[i] = -1;
      h0[i] = h1[i] = 0;
      if (in_beam(i) && c < V) {
        const Beam b = B[i];
        const LbCand x = lb_expand<LM, SM>(a, cx, b, c, lpc, slot[i][c]);
        s0[i] = x.s0, s1[i] = x.s1;
        nd0[i] = x.node, beg0[i] = x.beg, deg0[i] = x.deg, wd[i] = x.word;
        h0[i] = b.hash, h1[i] = x.h1;
        live += (s0[i] > -INFINITY) + (s1[i] > -INFINITY);
      }
    }

    // merge equal (node, history) among this thread's candidates, in id order (w = 0 before w = 1, then the beam rank)
    if (live >= 2) {
      // log-add: the accumulators, the raw scores to begin with.  They live in LDS, candidate-major (column c is this thread's:
      // constant offsets, no bank conflict, no barrier): 32 more registers would cost the second workgroup of a CU
      float* acc = nullptr;
      if constexpr (LA) {
        __shared__ float la_acc[2 * kLbMaxBeam * kLbThreads];
        acc = la_acc + c;
#pragma unroll
        for (int i = 0; i < kLbMaxBeam; ++i) acc[i * kLbThreads] = s0[i], acc[(16 + i) * kLbThreads] = s1[i];
      }
#pragma unroll
      for (int p = 0; p < 2 * kLbMaxBeam; ++p) {
        if (!in_beam(p & 15)) continue;
#pragma unroll
        for (int q = p + 1; q < 2 * kLbMaxBeam; ++q) {
          if (!in_beam(q & 15)) continue;
          const int np_ = p < 16 ? nd0[p & 15] : 0, nq_ = q < 16 ? nd0[q & 15] : 0;
          const unsigned long long hp = p < 16 ? h0[p & 15] : h1[p & 15], hq = q < 16 ? h0[q & 15] : h1[q & 15];
          float& sp = p < 16 ? s0[p & 15] : s1[p & 15];
          float& sq = q < 16 ? s0[q & 15] : s1[q & 15];
          if constexpr (LA) {
            // the raw scores decide as above; the winner's accumulator takes the sum.  Dead candidates take no part
            if (np_ == nq_ && hp == hq && sp > -INFINITY && sq > -INFINITY) {
              const float sum = lb_log_add_call(acc[p * kLbThreads], acc[q * kLbThreads]);
              if (sq > sp)
                acc[q * kLbThreads] = sum, sp = -INFINITY;
              else
                acc[p * kLbThreads] = sum, sq = -INFINITY;
            }
          } else if (np_ == nq_ && hp == hq) {
            if (sq > sp)
              sp = -INFINITY;
            else
              sq = -INFINITY;
          }
        }
      }
      // from here on a survivor's score is its merged score
      if constexpr (LA) {
#pragma unroll
        for (int i = 0; i < kLbMaxBeam; ++i) {
          if (s0[i] > -INFINITY) s0[i] = acc[i * kLbThreads];
          if (s1[i] > -INFINITY) s1[i] = acc[(16 + i) * kLbThreads];
        }
      }
    }

    // `beam` rounds of block-wide arg-max on (score, id), id = (2 c + w) * 16 + i
    int n_new = 0;
    float thr = -INFINITY, bv = -INFINITY;
    int bid = INT_MAX;
    bool rescan = true;
    for (int r = 0; r < beam; ++r) {
      if (rescan) {
        bv = -INFINITY, bid = INT_MAX;
#pragma unroll
        for (int i = 0; i < kLbMaxBeam; ++i)
          if (s0[i] > bv) bv = s0[i], bid = 32 * c + i;
#pragma unroll
        for (int i = 0; i < kLbMaxBeam; ++i)
          if (s1[i] > bv) bv = s1[i], bid = 32 * c + 16 + i;
        rescan = false;
      }
      const float wm = wave_max(bv);
      int cand = (bv == wm && wm > -INFINITY) ? bid : INT_MAX;
      // lowest id among the lanes that hold the wave maximum (written out, as in ctc_beam.hip)
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
      if (r == 0 && a.use_thr) thr = gv - a.beam_threshold;
      if (!(gv > -INFINITY) || gid == INT_MAX || gv < thr) {
        __syncthreads();
        break;
      }
      if (c == (gid >> 5)) {
        const int ii = gid & 15;
        const bool end = (gid >> 4) & 1;
        const Beam par = B[ii];
        // where the winner stands, from this thread's registers: a word end at the root with the new history, else the candidate's node
        int node = 0, beg = 0, deg = cx.root_deg, word = -1;
        unsigned long long hash = par.hash;
#pragma unroll
        for (int i = 0; i < kLbMaxBeam; ++i)
          if (i == ii) {
            if (end) {
              hash = h1[i], word = wd[i];
              s1[i] = -INFINITY;
            } else {
              node = nd0[i], beg = beg0[i], deg = deg0[i];
              s0[i] = -INFINITY;
            }
          }
        lb_survive<LM, SM>(a, cx, N, t, par, ii, c, end, node, beg, deg, hash, word, gv, r);
        rescan = true;
      }
      n_new = r + 1;
      __syncthreads();
    }
    nb = n_new;
    cur ^= 1;
    if (nb == 0) break;  // no candidate survived the frame: the sequence ends without a hypothesis
  }

  lb_epilogue<LM, SM>(a, cx, bufs[cur], nb, c, fin_rank, fin_ntok, fin_nw, fin_score, fin_n);
}

template <bool LM, bool SM, bool LA>
static void lb_launch(bool wide, const LbArgs& a, int n_seq, hipStream_t stream) {
  if (wide)
    lexbeam_wide_launch<LM, SM, LA>(a, n_seq, stream);
  else
    hipLaunchKernelGGL((ctc_lexbeam_kernel<LM, SM, LA>), dim3(n_seq), dim3(kLbThreads), 0, stream, a);
}

// The checks and the launch of all six entries, narrow (beams up to 16) and wide (up to 64).  An entry that cannot be called
// without a model or without a table says so with with_lm / with_smear = true and is refused a null one; the entries where lm and
// smear choose the mode (log-add, wide) pass lm != NULL / smear != NULL.  What the wide entry has always done differently stays the
// wide entry's: it names lm in the alignment message whatever the mode, it names its own size function, and it hands the kernel
// lm_weight 0 when there is no model (no kernel without a model reads it)
static int lb_decode(const char* who, bool wide, const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank,
                     int sil, int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words, int32_t* words,
                     int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores, int32_t* n_hyp, void* workspace,
                     size_t workspace_bytes, void* stream, bool with_lm, const void* lm, float lm_weight, bool with_smear, const void* smear,
                     bool log_add) {
  using eech::fail;
  const std::string me(who);
  const int max_beam = wide ? kLwMaxBeam : kLbMaxBeam;
  if (with_smear && !with_lm) return fail(EEC_ERR_BAD_ARG, me + ": smear without lm: it is the model's scores that are smeared");
  if (n_seq < 0 || Tq < 1 || max_words < 1) return fail(EEC_ERR_BAD_ARG, me + ": needs n_seq >= 0, Tq >= 1, max_words >= 1");
  if (V > 256 || V < 2 || beam_size < 1 || beam_size > max_beam || nbest < 1 || nbest > beam_size)
    return fail(EEC_ERR_UNSUPPORTED, me + ": needs 2 <= V <= 256, 1 <= beam_size <= " + std::to_string(max_beam) + ", 1 <= nbest <= beam_size");
  if (blank < 0 || blank >= V || sil < -1 || sil >= V || sil == blank)
    return fail(EEC_ERR_BAD_ARG, me + ": needs blank in [0, V), sil -1 or in [0, V) and not the blank");
  if (with_lm && !std::isfinite(lm_weight)) return fail(EEC_ERR_BAD_ARG, me + ": lm_weight must be finite");
  if (with_lm && !lm) return fail(EEC_ERR_BAD_ARG, me + ": null argument (lm)");
  if (with_smear && !smear) return fail(EEC_ERR_BAD_ARG, me + ": null argument (smear)");
  if (with_smear && ((uintptr_t)smear & 7)) return fail(EEC_ERR_BAD_ARG, me + ": smear must be 8-byte aligned");
  if (n_seq == 0) return 0;
  if (!logp || !trie || !words || !word_count || !tokens || !token_count || !scores || !n_hyp || !workspace)
    return fail(EEC_ERR_BAD_ARG, me + ": null argument");
  if (((uintptr_t)trie | (uintptr_t)workspace | (uintptr_t)lm) & 7)
    return fail(EEC_ERR_BAD_ARG, me + (with_lm || wide ? ": trie, lm and workspace must be 8-byte aligned" : ": trie and workspace must be 8-byte aligned"));
  if (workspace_bytes < eec_ctc_lexbeam_workspace_bytes(n_seq, Tq, beam_size))
    return fail(EEC_ERR_WORKSPACE, me + ": workspace below " + (wide ? "eec_ctc_lexbeam_wide_workspace_bytes()" : "eec_ctc_lexbeam_workspace_bytes()"));
  LbArgs a;
  a.logp = logp, a.em_len = em_len, a.trie = (const int*)trie;
  a.Tq = Tq, a.V = V, a.blank = blank, a.sil = sil, a.beam = beam_size, a.nbest = nbest, a.max_words = max_words;
  a.use_thr = std::isfinite(beam_threshold) ? 1 : 0;
  a.word_score = word_score, a.sil_score = sil_score, a.beam_threshold = beam_threshold;
  a.words = words, a.word_count = word_count, a.tokens = tokens, a.token_count = token_count, a.timesteps = timesteps, a.n_hyp = n_hyp;
  a.scores = scores, a.backptr = (int2*)workspace;
  a.lm = (const int*)lm, a.lm_weight = wide && !with_lm ? 0.f : lm_weight, a.smear = (const int*)smear;
  hipStream_t st = (hipStream_t)stream;
  if (log_add && with_smear)
    lb_launch<true, true, true>(wide, a, n_seq, st);
  else if (log_add && with_lm)
    lb_launch<true, false, true>(wide, a, n_seq, st);
  else if (log_add)
    lb_launch<false, false, true>(wide, a, n_seq, st);
  else if (with_smear)
    lb_launch<true, true, false>(wide, a, n_seq, st);
  else if (with_lm)
    lb_launch<true, false, false>(wide, a, n_seq, st);
  else
    lb_launch<false, false, false>(wide, a, n_seq, st);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // namespace eec

extern "C" {

size_t eec_ctc_lexbeam_workspace_bytes(int n_seq, int Tq, int beam_size) {
  return n_seq > 0 && Tq > 0 && beam_size > 0 ? (size_t)n_seq * Tq * beam_size * sizeof(int2) : 0;
}

size_t eec_ctc_lexbeam_wide_workspace_bytes(int n_seq, int Tq, int beam_size) { return eec_ctc_lexbeam_workspace_bytes(n_seq, Tq, beam_size); }

int eec_ctc_lexbeam_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                           int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                           int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                           int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream) {
  return eec::lb_decode("eec_ctc_lexbeam_decode", false, logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score, sil_score,
                        beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace, workspace_bytes,
                        stream, false, nullptr, 0.f, false, nullptr, false);
}

int eec_ctc_lexbeam_lm_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                              int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                              int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                              int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm, float lm_weight) {
  return eec::lb_decode("eec_ctc_lexbeam_lm_decode", false, logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score,
                        sil_score, beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace,
                        workspace_bytes, stream, true, lm, lm_weight, false, nullptr, false);
}

int eec_ctc_lexbeam_lm_smear_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                    int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                    int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps,
                                    float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm,
                                    float lm_weight, const void* smear) {
  return eec::lb_decode("eec_ctc_lexbeam_lm_smear_decode", false, logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score,
                        sil_score, beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace,
                        workspace_bytes, stream, true, lm, lm_weight, true, smear, false);
}

int eec_ctc_lexbeam_logadd_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                  int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                  int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps,
                                  float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm,
                                  float lm_weight, const void* smear) {
  return eec::lb_decode("eec_ctc_lexbeam_logadd_decode", false, logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score,
                        sil_score, beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace,
                        workspace_bytes, stream, lm != nullptr, lm, lm_weight, smear != nullptr, smear, true);
}

int eec_ctc_lexbeam_wide_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                                int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm, float lm_weight,
                                const void* smear, int log_add) {
  return eec::lb_decode("eec_ctc_lexbeam_wide_decode", true, logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score, sil_score,
                        beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace, workspace_bytes,
                        stream, lm != nullptr, lm, lm_weight, smear != nullptr, smear, log_add != 0);
}

float eec_ctc_log_add_host(float a, float b) { return eec::lb_log_add(a, b); }

int eec_ctc_log_add(const float* a, const float* b, float* out, int n, void* stream) {
  using eech::fail;
  if (n < 0) return fail(EEC_ERR_BAD_ARG, "eec_ctc_log_add: n must not be negative");
  if (n == 0) return 0;
  if (!a || !b || !out) return fail(EEC_ERR_BAD_ARG, "eec_ctc_log_add: null argument (a, b, out)");
  const int blocks = std::min((n + 255) / 256, 1024);
  hipLaunchKernelGGL(eec::ctc_log_add_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
