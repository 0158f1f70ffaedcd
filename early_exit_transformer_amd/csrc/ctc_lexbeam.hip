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
// One 256-thread workgroup per sequence, one launch for the batch; thread c owns frame label c (V <= 256).  All candidates that
// can merge share their frame label, so every merge is local to one thread.  Per frame:
//   * the beam (<= 16 hypotheses: trie node with its child range, last label, 64-bit history hash, score, token and word counts)
//     lives in LDS, double-buffered;
//   * child lookup is a scatter instead of a search: for beam entry i the first deg(node_i) threads read the node's child bytes
//     (one coalesced load) and write "edge offset" into a byte table slot[i][label] in LDS; thread c then reads slot[i][c].  The
//     breadth-first node numbering makes the child of edge k node k + 1, so the table needs no target;
//   * thread c holds, per beam entry, at most one in-place / in-word candidate (blank, repeat, child, sil: w = 0) and one word-end
//     candidate (w = 1) in registers, merges equal (node, history) keys among its <= 32 candidates (the higher score survives, the
//     lower id on a tie), and `beam` rounds of a block-wide arg-max on (score, id) pick the survivors; a thread rescans its own
//     candidates only after it won a round.  The first round's winner gives the beam threshold;
//   * every survivor leaves (parent rank, label, completed word + 1) in a back-pointer table, 8 bytes per (frame, rank).
// At the end the complete hypotheses (node 0) are already in rank order; up to nbest threads walk their back-pointers, one each.
// In the three Viterbi entries scores are fp32 additions in the order include/eec.h writes them, no reductions, no log / exp: the
// result is bit-identical to the statement.  Latency-bound integer / scalar work over T' serial frames: it is sized to keep all E * B = 384 sequences of a
// batch in flight at once (5.4 KB of LDS, well under two workgroups per CU), not for the roofline.  The real lexicon's image
// (89 114 words, 162 621 nodes, 1.5 MB) is read-only and shared by all workgroups: it sits in L2.
//
// With a model (ctc_lexbeam_kernel<true>; <false> is the search without one) a hypothesis also carries an LM state, a node
// of the packed n-gram image (layout in include/eec.h).  The back-off walk -- a binary search over the state's edge range, then the
// suffix link -- runs where a word-end candidate is formed; only the candidate's score is kept, and the at most `beam` word-end
// candidates that win a round redo their walk for the state they continue from.  After the last frame one thread adds the </s>
// term to the complete hypotheses and orders the at most 16 of them by insertion.
//
// With LM look-ahead (ctc_lexbeam_kernel<true, true>, eec_ctc_lexbeam_lm_smear_decode) the trie is smeared with the MAX mode, as
// the third-party decoder always does: a host-built table (eec_ctc_trie_smear) gives every node the best start-state score of the
// words at or below it, a step into a node is charged the increase of that maximum, and a word end takes the advance payment back.
// smax[y] is loaded beside cbeg[y] / word_of[y]; the payment outstanding at a hypothesis' node rides in its beam entry in LDS and is
// written by the round's winner.  The two other instantiations do not see any of it: their beam entry and arguments are unchanged.
//
// With log-add merging (LA = true on any of the three, eec_ctc_lexbeam_logadd_decode) a thread keeps, beside the raw score of each of
// its <= 32 candidates, an accumulator that starts as the raw score (32 KB of LDS per workgroup, a column per thread, touched only by
// threads with two or more live candidates: as registers they pushed the kernel past 256 and the CU down to one workgroup).  The pairwise merge loop is the Viterbi one -- the raw scores
// decide who is eliminated, in the same pair order --, and at every elimination the winner's accumulator takes log_add(winner's,
// loser's): that pair order IS the fold order include/eec.h states.  After the loop the accumulators replace the scores, so the
// rounds, the threshold and the beam work on merged scores.  log_add is the fixed fp32 sequence stated in include/eec.h (lb_log_add
// below: add, subtract, multiply, compare, rintf, ldexpf; no libm transcendental, no division), the same function on the host: the
// LA entries are bit-identical to the statement, whose log_add is that sequence.  It is called out of line (merges are rare per
// thread and frame; 496 inlined copies would not be).  The LA = false instantiations compile to what they were.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"
#include "eec_lexbeam.h"

namespace eec {

// the merge loop's call: one copy of the sequence for its 496 pairs
__device__ __noinline__ float lb_log_add_call(float a, float b) { return lb_log_add(a, b); }

__global__ void ctc_log_add_kernel(const float* a, const float* b, float* out, int n) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) out[k] = lb_log_add(a[k], b[k]);
}

// SM (with LM only): LM look-ahead by the smear table.  LA: log-add merging instead of Viterbi merging
template <bool LM, bool SM = false, bool LA = false>
__global__ __launch_bounds__(kLbThreads) void ctc_lexbeam_kernel(const std::conditional_t<SM, LbSmArgs, std::conditional_t<LM, LbLmArgs, LbArgs>> a) {
  static_assert(LM || !SM, "smearing needs a model");
  using Beam = std::conditional_t<SM, LbBeamSm, LbBeam>;
  __shared__ Beam bufs[2][kLbMaxBeam];
  __shared__ __attribute__((aligned(16))) unsigned char slot[kLbMaxBeam][256];  // edge offset of label c below beam i's node
  __shared__ float red_v[4];
  __shared__ int red_id[4];
  __shared__ int fin_rank[kLbMaxBeam], fin_ntok[kLbMaxBeam], fin_nw[kLbMaxBeam], fin_n;
  __shared__ float fin_score[LM ? kLbMaxBeam : 1];  // with a model: the final scores, </s> term included
  const int seq = blockIdx.x, c = threadIdx.x, lane = c & 63, w = c >> 6;
  const int V = a.V, blank = a.blank, sil = a.sil, beam = a.beam, Tq = a.Tq;

  // a trie that is not the one the call describes is not read past its header: every sequence ends without a hypothesis
  // ... and so is a model that is none, or was packed for another lexicon, or a smear table that is none or another trie's
  const bool ok = a.trie[0] == kLbMagic && a.trie[1] >= 1 && a.trie[3] == V && a.trie[4] == blank && a.trie[5] == sil && lm_fits<LM, SM>(a);
  int L = a.em_len ? a.em_len[seq] : Tq;
  if (!ok || L < 1 || L > Tq) L = 0;
  const int* cbeg = a.trie + (ok ? a.trie[6] : 0);
  const unsigned char* ctok = (const unsigned char*)(a.trie + (ok ? a.trie[7] : 0));
  const int* word_of = a.trie + (ok ? a.trie[8] : 0);
  const int root_deg = L > 0 ? cbeg[1] : 0;
  const float* smax = nullptr;
  if constexpr (SM) smax = (const float*)(a.smear + (ok ? kSmHeader : 0));
  LmView m = {};
  if constexpr (LM) {
    const int* lm = a.lm;
    if (ok) {
      m.begin = lm + lm[9], m.eword = lm + lm[10], m.suffix = lm + lm[13], m.map = lm + lm[14];
      m.logp = (const float*)(lm + lm[11]), m.backoff = (const float*)(lm + lm[12]);
      m.top_begin = lm[8], m.bos = lm[6], m.eos = lm[7];
    }
  }

  const float* lp_seq = a.logp + (size_t)seq * Tq * V;
  int2* bp = a.backptr + (size_t)seq * Tq * beam;
  int cur = 0, nb = 1;
  if (c == 0) bufs[0][0] = lb_entry<Beam>(LbBeam{0x243F6A8885A308D3ull, 0.f, 0, 0, root_deg, -1, 0, 0, LM ? m.bos : 0}, 0.f);
  float lp_next = (L > 0 && c < V) ? lp_seq[c] : -INFINITY;
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const Beam* B = bufs[cur];
    Beam* N = bufs[cur ^ 1];
    const float lpc = lp_next;
    if (t + 1 < L && c < V) lp_next = lp_seq[(size_t)(t + 1) * V + c];  // one frame ahead of its use

    for (int k = c; k < nb * 64; k += kLbThreads) ((unsigned*)slot)[k] = ~0u;  // rows 0 .. nb - 1 <- kLbNoChild
    __syncthreads();
    for (int i = 0; i < nb; ++i)
      if (c < B[i].deg) slot[i][ctok[B[i].beg + c]] = (unsigned char)c;
    __syncthreads();

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
        const float base = b.score + lpc;
        h0[i] = b.hash;
        if (c == blank || c == b.tok) {  // blank, or the repeat of a non-blank label: the state stays
          s0[i] = (c == sil) ? base + a.sil_score : base;
          nd0[i] = b.node, beg0[i] = b.beg, deg0[i] = b.deg;
        } else if (c == sil) {
          if (b.node == 0) {
            s0[i] = base + a.sil_score;
            deg0[i] = root_deg;
          }
        } else {
          const int j = slot[i][c];
          if (j != kLbNoChild) {
            const int y = b.beg + j + 1;
            const int yb = cbeg[y], ye = cbeg[y + 1], word = word_of[y];
            float sy = 0.f;
            if constexpr (SM) sy = smax[y];
            if (ye > yb) {
              s0[i] = base;
              if constexpr (SM) s0[i] = lm_add(base, a.lm_weight, sy - b.pmax);  // the increase of the maximum, paid in advance
              nd0[i] = y, beg0[i] = yb, deg0[i] = ye - yb;
            }
            if (word >= 0) {
              s1[i] = base + a.word_score;
              if constexpr (LM) {
                int next;
                float acc = lm_walk(m, b.pad, m.map[word], next);
                if constexpr (SM) acc = acc - b.pmax;  // the true score replaces what was paid
                s1[i] = lm_add(s1[i], a.lm_weight, acc);
              }
              wd[i] = word;
              h1[i] = lb_mix(b.hash, word);
            }
          }
        }
        if (!(s0[i] > -INFINITY)) s0[i] = -INFINITY;  // -inf and NaN are dropped
        if (!(s1[i] > -INFINITY)) s1[i] = -INFINITY;
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
        LbBeam e = LbBeam{par.hash, gv, 0, 0, root_deg, c, par.ntok + (c != blank && c != par.tok), par.nw + end, LM ? par.pad : 0};
        int word = 0;
#pragma unroll
        for (int i = 0; i < kLbMaxBeam; ++i)
          if (i == ii) {
            if (end) {
              e.hash = h1[i];
              word = wd[i] + 1;
              s1[i] = -INFINITY;
            } else {
              e.node = nd0[i], e.beg = beg0[i], e.deg = deg0[i];
              s0[i] = -INFINITY;
            }
          }
        if constexpr (LM)
          if (end) lm_walk(m, par.pad, m.map[word - 1], e.pad);  // the walk again, for the state this time
        float pmax = 0.f;  // nothing is outstanding at the root
        if constexpr (SM)
          if (!end) pmax = e.node == par.node ? par.pmax : smax[e.node];
        N[r] = lb_entry<Beam>(e, pmax);
        bp[(size_t)t * beam + r] = make_int2((ii << 16) | c, word);
        rescan = true;
      }
      n_new = r + 1;
      __syncthreads();
    }
    nb = n_new;
    cur ^= 1;
    if (nb == 0) break;  // no candidate survived the frame: the sequence ends without a hypothesis
  }

#include "eec_lexbeam_epilogue.inc"
}

static size_t lb_image_dwords(unsigned long long nodes) {  // nodes >= 1
  return (size_t)(kLbHeader + (nodes + 1) + (nodes - 1 + 3) / 4 + nodes + 1) & ~(size_t)1;
}

static size_t lm_image_dwords(unsigned long long nodes, unsigned long long lex_words) {  // nodes >= 1
  return (size_t)(kLmHeader + (nodes + 1) + (nodes - 1) + 3 * nodes + lex_words + 1) & ~(size_t)1;
}

// the checks and the launch of the four entries
static int lb_decode(const char* who, const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                     int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words, int32_t* words,
                     int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores, int32_t* n_hyp, void* workspace,
                     size_t workspace_bytes, void* stream, bool with_lm, const void* lm, float lm_weight, bool with_smear = false,
                     const void* smear = nullptr, bool log_add = false) {
  using eech::fail;
  const std::string me(who);
  if (n_seq < 0 || Tq < 1 || max_words < 1) return fail(EEC_ERR_BAD_ARG, me + ": needs n_seq >= 0, Tq >= 1, max_words >= 1");
  if (V > 256 || V < 2 || beam_size < 1 || beam_size > kLbMaxBeam || nbest < 1 || nbest > beam_size)
    return fail(EEC_ERR_UNSUPPORTED, me + ": needs 2 <= V <= 256, 1 <= beam_size <= " + std::to_string(kLbMaxBeam) + ", 1 <= nbest <= beam_size");
  if (blank < 0 || blank >= V || sil < -1 || sil >= V || sil == blank)
    return fail(EEC_ERR_BAD_ARG, me + ": needs blank in [0, V), sil -1 or in [0, V) and not the blank");
  if (with_lm && !std::isfinite(lm_weight)) return fail(EEC_ERR_BAD_ARG, me + ": lm_weight must be finite");
  if (with_lm && !lm) return fail(EEC_ERR_BAD_ARG, me + ": null argument (lm)");
  if (with_smear && !smear) return fail(EEC_ERR_BAD_ARG, me + ": null argument (smear)");
  if (with_smear && ((uintptr_t)smear & 7)) return fail(EEC_ERR_BAD_ARG, me + ": smear must be 8-byte aligned");
  if (n_seq == 0) return 0;
  if (!logp || !trie || !words || !word_count || !tokens || !token_count || !scores || !n_hyp || !workspace)
    return fail(EEC_ERR_BAD_ARG, me + ": null argument");
  if (((uintptr_t)trie | (uintptr_t)workspace | (uintptr_t)lm) & 7) return fail(EEC_ERR_BAD_ARG, me + (with_lm ? ": trie, lm and workspace must be 8-byte aligned" : ": trie and workspace must be 8-byte aligned"));
  if (workspace_bytes < eec_ctc_lexbeam_workspace_bytes(n_seq, Tq, beam_size))
    return fail(EEC_ERR_WORKSPACE, me + ": workspace below eec_ctc_lexbeam_workspace_bytes()");
  LbSmArgs a;
  a.logp = logp, a.em_len = em_len, a.trie = (const int*)trie;
  a.Tq = Tq, a.V = V, a.blank = blank, a.sil = sil, a.beam = beam_size, a.nbest = nbest, a.max_words = max_words;
  a.use_thr = std::isfinite(beam_threshold) ? 1 : 0;
  a.word_score = word_score, a.sil_score = sil_score, a.beam_threshold = beam_threshold;
  a.words = words, a.word_count = word_count, a.tokens = tokens, a.token_count = token_count, a.timesteps = timesteps, a.n_hyp = n_hyp;
  a.scores = scores, a.backptr = (int2*)workspace;
  a.lm = (const int*)lm, a.lm_weight = lm_weight, a.smear = (const int*)smear;
  if (log_add && with_smear)
    hipLaunchKernelGGL((ctc_lexbeam_kernel<true, true, true>), dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, a);
  else if (log_add && with_lm)
    hipLaunchKernelGGL((ctc_lexbeam_kernel<true, false, true>), dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, (const LbLmArgs&)a);
  else if (log_add)
    hipLaunchKernelGGL((ctc_lexbeam_kernel<false, false, true>), dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, (const LbArgs&)a);
  else if (with_smear)
    hipLaunchKernelGGL((ctc_lexbeam_kernel<true, true>), dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, a);
  else if (with_lm)
    hipLaunchKernelGGL(ctc_lexbeam_kernel<true>, dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, (const LbLmArgs&)a);
  else
    hipLaunchKernelGGL(ctc_lexbeam_kernel<false>, dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, (const LbArgs&)a);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // namespace eec

extern "C" {

size_t eec_ctc_trie_pack_bytes(int n_words, int64_t total_tokens) {
  if (n_words <= 0 || total_tokens < n_words) return 0;
  const size_t dwords = eec::lb_image_dwords((unsigned long long)total_tokens + 1);  // a trie has at most one node per token, and the root
  return dwords >= ((size_t)1 << 31) ? 0 : dwords * 4;                                // the kernel indexes the image with int32
}

int eec_ctc_trie_pack(const int32_t* spellings, const int64_t* offsets, int n_words, int V, int blank, int sil, void* image,
                      size_t image_bytes, int32_t* n_nodes, int32_t* n_shadowed) {
  using namespace eec;
  using eech::fail;
  if (!spellings || !offsets || !image) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: null argument (spellings, offsets, image)");
  if (n_words <= 0) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: n_words must be positive");
  if (V > 256) return fail(EEC_ERR_UNSUPPORTED, "eec_ctc_trie_pack: V above 256");
  if (V < 2 || blank < 0 || blank >= V || sil < -1 || sil >= V || sil == blank)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: needs V >= 2, blank in [0, V), sil -1 or in [0, V) and not the blank");
  if (offsets[0] != 0) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: offsets[0] must be 0");
  for (int i = 0; i < n_words; ++i)
    if (offsets[i + 1] <= offsets[i]) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: offsets must ascend and no spelling may be empty");
  const int64_t total = offsets[n_words];
  for (int64_t k = 0; k < total; ++k)
    if (spellings[k] < 0 || spellings[k] >= V || spellings[k] == blank || spellings[k] == sil)
      return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_pack: a token outside [0, V), or the blank or sil token, in a spelling");
  const size_t need = eec_ctc_trie_pack_bytes(n_words, total);
  if (need == 0) return fail(EEC_ERR_UNSUPPORTED, "eec_ctc_trie_pack: the image would pass 2^31 dwords");
  if (image_bytes < need) return fail(EEC_ERR_WORKSPACE, "eec_ctc_trie_pack: image_bytes below eec_ctc_trie_pack_bytes()");

  struct Node {
    std::vector<std::pair<unsigned char, int>> kids;
    int word = -1;
  };
  std::vector<Node> tn(1);
  int shadowed = 0;
  for (int wi = 0; wi < n_words; ++wi) {
    int at = 0;
    for (int64_t k = offsets[wi]; k < offsets[wi + 1]; ++k) {
      const unsigned char tok = (unsigned char)spellings[k];
      int next = -1;
      for (const auto& kid : tn[at].kids)
        if (kid.first == tok) next = kid.second;
      if (next < 0) {
        next = (int)tn.size();
        tn[at].kids.emplace_back(tok, next);
        tn.emplace_back();
      }
      at = next;
    }
    if (tn[at].word < 0)
      tn[at].word = wi;  // the first word in file order with this spelling
    else
      ++shadowed;
  }

  // breadth-first numbering, children ascending by token: the child reached by edge k is node k + 1
  const int nodes = (int)tn.size(), edges = nodes - 1;
  int32_t* img = (int32_t*)image;
  memset(img, 0, need);
  const int off_begin = kLbHeader, off_tok = off_begin + nodes + 1, off_word = off_tok + (edges + 3) / 4;
  unsigned char* tok_bytes = (unsigned char*)(img + off_tok);
  std::vector<int> order(1, 0);
  order.reserve(nodes);
  for (int id = 0; id < nodes; ++id) {
    Node& nd = tn[order[id]];
    std::sort(nd.kids.begin(), nd.kids.end());
    img[off_begin + id] = (int32_t)order.size() - 1;
    for (const auto& kid : nd.kids) {
      tok_bytes[order.size() - 1] = kid.first;
      order.push_back(kid.second);
    }
    img[off_word + id] = nd.word;
  }
  img[off_begin + nodes] = edges;
  img[0] = kLbMagic, img[1] = nodes, img[2] = edges, img[3] = V, img[4] = blank, img[5] = sil;
  img[6] = off_begin, img[7] = off_tok, img[8] = off_word, img[9] = off_word + nodes, img[10] = n_words, img[11] = shadowed;
  if (n_nodes) *n_nodes = nodes;
  if (n_shadowed) *n_shadowed = shadowed;
  return 0;
}

size_t eec_ngram_pack_bytes(int order, const int64_t* counts, int lex_words) {
  if (order < 1 || order > eec::kLmMaxOrder || !counts || lex_words <= 0 || counts[0] <= 0) return 0;
  unsigned long long nodes = 1;
  for (int n = 0; n < order; ++n) {
    if (counts[n] < 0 || counts[n] >= ((int64_t)1 << 31)) return 0;
    nodes += (unsigned long long)counts[n];
  }
  const size_t dwords = eec::lm_image_dwords(nodes, (unsigned long long)lex_words);
  return dwords >= ((size_t)1 << 31) ? 0 : dwords * 4;  // the kernel indexes the image with int32
}

int eec_ngram_pack(int order, const int64_t* counts, const int32_t* const* words, const float* const* logp, const float* const* backoff,
                   const int32_t* word_map, int lex_words, int bos_word, int eos_word, void* image, size_t image_bytes, int32_t* n_nodes) {
  using namespace eec;
  using eech::fail;
  if (order < 1 || order > kLmMaxOrder) return fail(EEC_ERR_UNSUPPORTED, "eec_ngram_pack: the order must be 1 .. " + std::to_string(kLmMaxOrder));
  if (!counts || !words || !logp || !backoff || !word_map || !image)
    return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: null argument (counts, words, logp, backoff, word_map, image)");
  if (lex_words <= 0 || counts[0] <= 0) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: needs lex_words > 0 and at least one unigram");
  for (int n = 0; n < order; ++n) {
    if (counts[n] < 0) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: a negative count");
    if (counts[n] > 0 && (!words[n] || !logp[n] || !backoff[n])) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: null array of order " + std::to_string(n + 1));
  }
  const size_t need = eec_ngram_pack_bytes(order, counts, lex_words);
  if (need == 0) return fail(EEC_ERR_UNSUPPORTED, "eec_ngram_pack: the image would pass 2^31 dwords");
  if (image_bytes < need) return fail(EEC_ERR_WORKSPACE, "eec_ngram_pack: image_bytes below eec_ngram_pack_bytes()");
  const int W = (int)counts[0];
  if (bos_word < -1 || bos_word >= W || eos_word < -1 || eos_word >= W)
    return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: bos_word and eos_word must be -1 or an LM word");
  for (int i = 0; i < lex_words; ++i)
    if (word_map[i] < 0 || word_map[i] >= W) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: word_map[" + std::to_string(i) + "] is no LM word");
  for (int n = 0; n < order; ++n)
    for (int64_t i = 0; i < counts[n]; ++i)
      if (!std::isfinite(logp[n][i]) || !std::isfinite(backoff[n][i]))
        return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: a non-finite value in " + std::to_string(n + 1) + "-gram " + std::to_string(i));

  int level[kLmMaxOrder + 2];  // level[n]: the first node of depth n; level[order + 1]: the node count
  level[0] = 0, level[1] = 1;
  for (int n = 1; n <= order; ++n) level[n + 1] = level[n] + (int)counts[n - 1];
  const int nodes = level[order + 1], edges = nodes - 1;
  int32_t* img = (int32_t*)image;
  memset(img, 0, need);
  const int off_begin = kLmHeader, off_eword = off_begin + nodes + 1, off_logp = off_eword + edges, off_backoff = off_logp + nodes,
            off_suffix = off_backoff + nodes, off_map = off_suffix + nodes;
  int32_t *begin = img + off_begin, *eword = img + off_eword, *suffix = img + off_suffix;
  float *lp = (float*)(img + off_logp), *bo = (float*)(img + off_backoff);
  for (int x = 0; x <= nodes; ++x) begin[x] = edges;  // a node without children: an empty range at its place

  // the child of `node` labelled v, or -1; the ranges of all shallower levels are final when a level is built
  auto child = [&](int node, int v) {
    if (node == 0) return v + 1;
    int lo = begin[node], hi = begin[node + 1];
    const int end = hi;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (eword[mid] < v)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo < end && eword[lo] == v ? lo + 1 : -1;
  };
  auto find = [&](const int32_t* w, int len) {  // the node of the n-gram w[0 .. len), or -1
    int at = 0;
    for (int k = 0; k < len && at >= 0; ++k) at = child(at, w[k]);
    return at;
  };

  // unigrams: LM word v is node v + 1, edge v of the root
  begin[0] = 0;
  std::vector<char> seen(W, 0);
  for (int i = 0; i < W; ++i) {
    const int v = words[0][i];
    if (v < 0 || v >= W) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: unigram " + std::to_string(i) + " is outside [0, counts[0])");
    if (seen[v]) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: unigram " + std::to_string(i) + " is a duplicate");
    seen[v] = 1;
    eword[v] = v, lp[v + 1] = logp[0][i], bo[v + 1] = backoff[0][i];
  }
  // higher orders, breadth-first: the nodes of depth n in the order of (parent, last word)
  for (int n = 2; n <= order; ++n) {
    const int64_t cnt = counts[n - 1];
    const int32_t* w = words[n - 1];
    std::vector<std::pair<std::pair<int, int>, int64_t>> ent((size_t)cnt);  // ((parent, word), index)
    for (int64_t i = 0; i < cnt; ++i) {
      for (int k = 0; k < n; ++k)
        if (w[i * n + k] < 0 || w[i * n + k] >= W)
          return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: " + std::to_string(n) + "-gram " + std::to_string(i) + " has a word outside [0, counts[0])");
      const int parent = find(w + i * n, n - 1);
      if (parent < 0) return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: the prefix of " + std::to_string(n) + "-gram " + std::to_string(i) + " is absent");
      ent[(size_t)i] = {{parent, w[i * n + n - 1]}, i};
    }
    std::sort(ent.begin(), ent.end());
    for (int64_t r = 0; r < cnt; ++r) {
      if (r > 0 && ent[(size_t)r].first == ent[(size_t)r - 1].first)
        return fail(EEC_ERR_BAD_ARG, "eec_ngram_pack: " + std::to_string(n) + "-gram " + std::to_string(ent[(size_t)r].second) + " is a duplicate");
      const int x = level[n] + (int)r;
      eword[x - 1] = ent[(size_t)r].first.second;
      lp[x] = logp[n - 1][ent[(size_t)r].second], bo[x] = backoff[n - 1][ent[(size_t)r].second];
    }
    // the parents' ranges: edges level[n] - 1 .. in parent order
    int64_t r = 0;
    for (int p = level[n - 1]; p < level[n]; ++p) {
      begin[p] = level[n] - 1 + (int)r;
      while (r < cnt && ent[(size_t)r].first.first == p) ++r;
    }
    for (int x = level[n]; x <= nodes; ++x) begin[x] = level[n] - 1 + (int)cnt;
    // suffix links of this level: the longest proper suffix that is a node; the last word's unigram at worst
    for (int64_t q = 0; q < cnt; ++q) {
      const int32_t* g = w + ent[(size_t)q].second * n;
      int to = -1;
      for (int k = 1; k < n && to < 0; ++k) to = find(g + k, n - k);
      suffix[level[n] + (int)q] = to;
    }
  }
  for (int i = 0; i < lex_words; ++i) img[off_map + i] = word_map[i];
  img[0] = kLmMagic, img[1] = order, img[2] = nodes, img[3] = edges, img[4] = W, img[5] = lex_words, img[6] = bos_word + 1, img[7] = eos_word;
  img[8] = level[order], img[9] = off_begin, img[10] = off_eword, img[11] = off_logp, img[12] = off_backoff, img[13] = off_suffix;
  img[14] = off_map, img[15] = off_map + lex_words;
  if (n_nodes) *n_nodes = nodes;
  return 0;
}

size_t eec_ctc_trie_smear_bytes(int n_nodes) {
  return n_nodes >= 1 ? (((size_t)eec::kSmHeader + (size_t)n_nodes + 1) & ~(size_t)1) * 4 : 0;
}

int eec_ctc_trie_smear(const void* trie_image, const void* lm_image, void* table, size_t table_bytes) {
  using namespace eec;
  using eech::fail;
  if (!trie_image || !lm_image || !table) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: null argument (trie_image, lm_image, table)");
  if (((uintptr_t)trie_image | (uintptr_t)lm_image | (uintptr_t)table) & 7)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: trie_image, lm_image and table must be 8-byte aligned");
  const int32_t *trie = (const int32_t*)trie_image, *lm = (const int32_t*)lm_image;
  if (trie[0] != kLbMagic || trie[1] < 1) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: trie_image is no packed trie");
  if (lm[0] != kLmMagic) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: lm_image is no packed n-gram model");
  if (lm[5] != trie[10])
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: the model was packed for a lexicon of " + std::to_string(lm[5]) + " words, the trie has " +
                                     std::to_string(trie[10]));
  const int nodes = trie[1];
  if (table_bytes < eec_ctc_trie_smear_bytes(nodes)) return fail(EEC_ERR_WORKSPACE, "eec_ctc_trie_smear: table_bytes below eec_ctc_trie_smear_bytes()");
  const int32_t *cbeg = trie + trie[6], *word_of = trie + trie[8];
  LmView m;
  m.begin = lm + lm[9], m.eword = lm + lm[10], m.suffix = lm + lm[13], m.map = lm + lm[14];
  m.logp = (const float*)(lm + lm[11]), m.backoff = (const float*)(lm + lm[12]);
  m.top_begin = lm[8], m.bos = lm[6], m.eos = lm[7];
  int32_t* tab = (int32_t*)table;
  memset(tab, 0, eec_ctc_trie_smear_bytes(nodes));
  float* smax = (float*)(tab + kSmHeader);
  // children have higher numbers than their parent (the child of edge k is node k + 1): one descending sweep
  for (int n = nodes - 1; n >= 1; --n) {
    float best = -INFINITY;
    const int word = word_of[n];
    if (word >= lm[5]) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: node " + std::to_string(n) + " ends a word outside the lexicon");
    if (word >= 0) {
      int next;
      best = lm_walk(m, m.bos, m.map[word], next);  // u(word): the walk from the start state
    }
    if (cbeg[n] < n || cbeg[n + 1] > nodes - 1 || cbeg[n + 1] < cbeg[n])
      return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: node " + std::to_string(n) + " has children that are not below it");
    for (int k = cbeg[n]; k < cbeg[n + 1]; ++k) best = std::max(best, smax[k + 1]);
    if (!std::isfinite(best)) return fail(EEC_ERR_BAD_ARG, "eec_ctc_trie_smear: node " + std::to_string(n) + " neither ends a word nor has children, or a model value is not finite");
    smax[n] = best;
  }
  smax[0] = 0.f;
  tab[0] = kSmMagic, tab[1] = nodes, tab[2] = trie[10], tab[3] = 0;
  return 0;
}

size_t eec_ctc_lexbeam_workspace_bytes(int n_seq, int Tq, int beam_size) {
  return n_seq > 0 && Tq > 0 && beam_size > 0 ? (size_t)n_seq * Tq * beam_size * sizeof(int2) : 0;
}

int eec_ctc_lexbeam_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                           int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                           int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                           int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream) {
  return eec::lb_decode("eec_ctc_lexbeam_decode", logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score, sil_score,
                        beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace, workspace_bytes,
                        stream, false, nullptr, 0.f);
}

int eec_ctc_lexbeam_lm_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                              int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                              int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                              int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm, float lm_weight) {
  return eec::lb_decode("eec_ctc_lexbeam_lm_decode", logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score, sil_score,
                        beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace, workspace_bytes,
                        stream, true, lm, lm_weight);
}

int eec_ctc_lexbeam_lm_smear_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                    int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                    int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps,
                                    float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm,
                                    float lm_weight, const void* smear) {
  return eec::lb_decode("eec_ctc_lexbeam_lm_smear_decode", logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score,
                        sil_score, beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace,
                        workspace_bytes, stream, true, lm, lm_weight, true, smear);
}

int eec_ctc_lexbeam_logadd_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                  int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                  int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps,
                                  float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm,
                                  float lm_weight, const void* smear) {
  if (smear && !lm) return eech::fail(EEC_ERR_BAD_ARG, "eec_ctc_lexbeam_logadd_decode: smear without lm: it is the model's scores that are smeared");
  return eec::lb_decode("eec_ctc_lexbeam_logadd_decode", logp, n_seq, Tq, V, em_len, trie, blank, sil, beam_size, nbest, word_score,
                        sil_score, beam_threshold, max_words, words, word_count, tokens, token_count, timesteps, scores, n_hyp, workspace,
                        workspace_bytes, stream, lm != nullptr, lm, lm_weight, smear != nullptr, smear, true);
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
