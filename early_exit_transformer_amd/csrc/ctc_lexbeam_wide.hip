// Lexicon-constrained CTC beam search for beams up to 64 (eec_ctc_lexbeam_wide_decode): the search of ctc_lexbeam.hip -- stated in
// include/eec.h, model, smearing and log-add merging included -- where a thread's candidates no longer fit registers.  The candidate
// id is (2 c + w) * 64 + i; nothing else of the statement differs, so for beams of 16 or less the results are those of the narrow
// entries bit for bit.  tests/lexbeam_wide_cases.py is the plain-Python statement and the judge.  Out of scope: beams over 64.
//
// One 256-thread workgroup per sequence, thread c owns frame label c, as in the narrow kernel: candidates that can merge share their
// label, so every merge is still local to one thread.  What changes is where candidates live and how survivors are picked.  Per frame:
//   * the child-lookup byte table slot[i][label] is built as in the narrow kernel (64 rows);
//   * thread c walks the beam in rank order and OFFERS each live candidate to a list of merged candidates ("groups") in LDS.  A group
//     is found through an open-addressing hash table on (c, node, history): a slot holds (c, list index), claimed with an LDS integer
//     compare-and-swap; only thread c ever inserts or matches keys of label c, so the arrival order of other threads decides where a
//     group sits, never what it holds.  A thread generates its candidates in ascending id order (the one w = 0 candidate that can
//     meet w = 1 candidates -- the repeat of a word's last label at the root -- goes first), and the stated pair loop over a group in
//     id order is a running fold: the group keeps the best raw score with its id (the lower id on a tie) and, with log-add, the
//     accumulator acc = log_add(acc, raw of the newcomer).  No floating-point atomics; nothing sized by the beam in registers;
//   * the list holds 1024 groups.  A frame that offers more (the bound is beam * (2 * degree + 3): 12 928 were seen) is redone
//     exactly: every thread counts its live candidates, a prefix sum cuts the labels into chunks of at most 1023 candidates, and the
//     chunks are processed one after the other, each selecting the best `beam` of (its groups + the survivors carried so far).  The
//     best `beam` of a union is the best `beam` of the parts' best `beam`, and a group never spans two labels: no heuristic cut;
//   * selection is an MSB-first radix select (8 bits a round, an LDS histogram with integer atomics) on the 48-bit key
//     (score as an ordered integer, -0 as +0; 0xffff - id): (score descending, id ascending) is a total order and ids are unique, so
//     exactly min(beam, groups) keys lie at or above the cut.  The survivors rank themselves by counting, the best one gives the beam
//     threshold (score >= best - beam_threshold stays), and each builds its beam entry and back-pointer from its id.
// The epilogue is the narrow kernel's (eec_lexbeam_epilogue.inc).
//
// Resources (tools/kernel_resources.py on build/ctc_lexbeam_wide.o, gfx950): 62 VGPRs (65 with smearing), 106 SGPRs, no scratch, no
// vector spills (45 to 80 scalars parked in VGPR lanes); 50 736 B of LDS without a model, 50 992 B with one, 52 016 B with smearing,
// and 4 096 B more with log-add (54 832 / 55 088 / 56 112 B) -- static, under the 64 KB that need no function attribute.  By LDS a
// CU (160 KB) holds two workgroups (three of the Viterbi instantiations), so the standing batch of 384 sequences is resident at once
// on 256 CUs, in one pass, as with the narrow kernel.
// Latency-bound integer and LDS work over T' serial frames, and slower than the narrow kernel where both serve: measured on the
// 384 x 256-frame batch, 57.4 ms at beam 16 against the narrow kernel's 12.7 ms, 157 ms at 32, 446 ms at 64 (DESIGN.md,
// profiles/lexbeam_wide_time.json).  Beams of 16 or less therefore stay with the narrow kernels.
#include <limits.h>
#include <math.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"
#include "eec_lexbeam.h"

namespace eec {

constexpr int kLwMaxBeam = 64;
constexpr int kLwCap = 1024;                     // groups of one pass
constexpr int kLwList = kLwMaxBeam + kLwCap;     // list slots: [0, 64) the survivors carried between chunks, then the pass's groups
constexpr int kLwTable = 2048;                   // hash slots (a power of two, twice the groups)
constexpr int kLwChunk = kLwCap - 2 * kLwMaxBeam;  // candidates at which a chunk closes; a thread adds at most 2 * 64 - 1 more

__device__ __noinline__ float lw_log_add_call(float a, float b) { return lb_log_add(a, b); }

template <bool LM, bool SM, bool LA>
__global__ __launch_bounds__(kLbThreads) void ctc_lexbeam_wide_kernel(const LbSmArgs a) {
  static_assert(LM || !SM, "smearing needs a model");
  using Beam = std::conditional_t<SM, LbBeamSm, LbBeam>;
  __shared__ Beam bufs[2][kLwMaxBeam];
  __shared__ __attribute__((aligned(16))) unsigned char slot[kLwMaxBeam][256];  // edge offset of label c below beam i's node
  __shared__ unsigned long long g_hash[kLwCap];  // a group's key: (label of its id, node, history)
  __shared__ int g_node[kLwCap];
  __shared__ float g_raw[LA ? kLwCap : 1];  // log-add: the best raw score of the members (g_score is the accumulator)
  __shared__ float g_score[kLwList];        // merged score
  __shared__ unsigned short g_id[kLwList];  // id of the member that survives
  __shared__ unsigned table[kLwTable];      // 0: empty, else (c << 16) | (group + 1)
  __shared__ int hist[256];
  __shared__ int wave_tot[4];
  __shared__ float t_score[kLwMaxBeam];
  __shared__ unsigned short t_id[kLwMaxBeam];
  __shared__ int sh_ng, sh_sel, sh_need, sh_nsurv, sh_nnew, sh_nchunks;
  __shared__ float sh_best;
  __shared__ int fin_rank[kLwMaxBeam], fin_ntok[kLwMaxBeam], fin_nw[kLwMaxBeam], fin_n;
  __shared__ float fin_score[LM ? kLwMaxBeam : 1];
  const int seq = blockIdx.x, c = threadIdx.x, lane = c & 63, w = c >> 6;
  const int V = a.V, blank = a.blank, sil = a.sil, beam = a.beam, Tq = a.Tq;

  // a foreign trie, model or smear table: as in the narrow kernel, nothing past the headers is read and no hypothesis is returned
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
  float* const raw = LA ? g_raw : g_score + kLwMaxBeam;  // Viterbi: the merged score is the best raw score
  int cur = 0, nb = 1;
  if (c == 0) bufs[0][0] = lb_entry<Beam>(LbBeam{0x243F6A8885A308D3ull, 0.f, 0, 0, root_deg, -1, 0, 0, LM ? m.bos : 0}, 0.f);
  float lp_next = (L > 0 && c < V) ? lp_seq[c] : -INFINITY;
  __syncthreads();

  // inclusive prefix sum of v over the workgroup's threads; a barrier must follow before the next call
  auto block_scan = [&](int v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(v, off, 64);
      if (lane >= off) v += up;
    }
    if (lane == 63) wave_tot[w] = v;
    __syncthreads();
    for (int k = 0; k < w; ++k) v += wave_tot[k];
    return v;
  };

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

    // a live candidate of this thread meets its group, or founds one.  Called in ascending id order within a group
    auto offer = [&](int node, unsigned long long h, float s, int id) {
      unsigned x = (unsigned)h ^ (unsigned)(h >> 32) ^ ((unsigned)node * 0x9E3779B1u) ^ ((unsigned)c * 0x85EBCA6Bu);
      x ^= x >> 15;
      unsigned p = x & (kLwTable - 1);
      int mine = -1;
      for (;;) {
        unsigned v = *(volatile unsigned*)&table[p];
        if (v == 0) {
          if (mine < 0) {
            mine = atomicAdd(&sh_ng, 1);
            if (mine >= kLwCap) return;  // the list is full: the frame is redone in chunks
            g_hash[mine] = h, g_node[mine] = node, g_score[kLwMaxBeam + mine] = s, g_id[kLwMaxBeam + mine] = (unsigned short)id;
            if constexpr (LA) g_raw[mine] = s;
          }
          v = atomicCAS(&table[p], 0u, ((unsigned)c << 16) | (unsigned)(mine + 1));
          if (v == 0) return;  // founded; otherwise another label's group took the slot first
        }
        if ((int)(v >> 16) == c) {
          const int g = (int)(v & 0xffff) - 1;
          if (g_node[g] == node && g_hash[g] == h) {
            if constexpr (LA) g_score[kLwMaxBeam + g] = lw_log_add_call(g_score[kLwMaxBeam + g], s);
            if (s > raw[g]) raw[g] = s, g_id[kLwMaxBeam + g] = (unsigned short)id;  // the lower id stays on a tie
            return;
          }
        }
        p = (p + 1) & (kLwTable - 1);
      }
    };

    // this label's candidates from every beam entry, by the rules and in the fp32 order of the narrow kernel; returns how many live
    auto emit = [&](bool insert) {
      int live = 0;
      if (c >= V) return live;
      auto put = [&](int node, unsigned long long h, float s, int id) {
        if (!(s > -INFINITY)) return;  // -inf and NaN are dropped
        ++live;
        if (insert) offer(node, h, s, id);
      };
      // the repeat of a word's last label at the root: the only w = 0 candidate that can meet word-end candidates, and the lowest id
      if (c != blank && c != sil)
        for (int i = 0; i < nb; ++i)
          if (B[i].tok == c && B[i].node == 0) put(0, B[i].hash, B[i].score + lpc, 128 * c + i);
      for (int i = 0; i < nb; ++i) {
        const int tok = B[i].tok, node = B[i].node;
        const float base = B[i].score + lpc;
        if (c == blank || c == tok) {  // blank, or the repeat of a non-blank label: the state stays
          if (c != blank && c != sil && node == 0) continue;  // went first
          put(node, B[i].hash, (c == sil) ? base + a.sil_score : base, 128 * c + i);
        } else if (c == sil) {
          if (node == 0) put(0, B[i].hash, base + a.sil_score, 128 * c + i);
        } else {
          const int j = slot[i][c];
          if (j != kLbNoChild) {
            const int y = B[i].beg + j + 1;
            const int yb = cbeg[y], ye = cbeg[y + 1], word = word_of[y];
            float pmax = 0.f;
            if constexpr (SM) pmax = B[i].pmax;
            if (ye > yb) {
              float s0 = base;
              if constexpr (SM) s0 = lm_add(base, a.lm_weight, smax[y] - pmax);  // the increase of the maximum, paid in advance
              put(y, B[i].hash, s0, 128 * c + i);
            }
            if (word >= 0) {
              float s1 = base + a.word_score;
              if constexpr (LM) {
                int next;
                float acc = lm_walk(m, B[i].pad, m.map[word], next);
                if constexpr (SM) acc = acc - pmax;  // the true score replaces what was paid
                s1 = lm_add(s1, a.lm_weight, acc);
              }
              put(0, lb_mix(B[i].hash, word), s1, 128 * c + 64 + i);
            }
          }
        }
      }
      return live;
    };

    // (score descending, id ascending) as one descending 48-bit integer
    auto key_of = [&](int g) {
      const float s = g_score[g];
      unsigned u = s == 0.f ? 0u : __float_as_uint(s);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      return ((unsigned long long)u << 16) | (unsigned long long)(0xffffu - g_id[g]);
    };

    int my_chunk = 0, nchunks = 1, ntop = 0;
    bool counted = false;
    for (int k = 0; k < nchunks;) {
      for (int x = c; x < kLwTable; x += kLbThreads) table[x] = 0;
      if (c == 0) sh_ng = 0, sh_nsurv = 0, sh_nnew = 0;
      __syncthreads();
      if (my_chunk == k) emit(true);
      __syncthreads();
      const int ng = min(sh_ng, kLwCap);
      if (sh_ng > kLwCap && !counted) {  // only the first, optimistic pass can overflow: cut the labels into chunks and start again
        const int cnt = emit(false);
        const int excl = block_scan(cnt) - cnt;
        my_chunk = excl / kLwChunk;
        if (c == kLbThreads - 1) sh_nchunks = my_chunk + 1;
        __syncthreads();
        nchunks = sh_nchunks, counted = true, k = 0, ntop = 0;
        continue;
      }
      const bool last = k == nchunks - 1;
      const int end = kLwMaxBeam + ng;  // list indices [0, ntop) and [64, end)

      // the cut: the beam-th largest key, or 0 when everything fits
      unsigned long long cut = 0;
      if (ntop + ng > beam) {
        int need = beam;
        for (int shift = 40; shift >= 0; shift -= 8) {
          hist[c] = 0;
          __syncthreads();
          for (int g = c; g < end; g += kLbThreads)
            if (g < ntop || g >= kLwMaxBeam) {
              const unsigned long long key = key_of(g);
              if ((key >> (shift + 8)) == cut) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
            }
          __syncthreads();
          // thread c owns digit 255 - c: its inclusive prefix counts the keys with that digit or a higher one
          const int own = hist[255 - c];
          const int incl = block_scan(own);
          if (incl - own < need && incl >= need) sh_sel = 255 - c, sh_need = need - (incl - own);
          __syncthreads();
          cut = (cut << 8) | (unsigned)sh_sel, need = sh_need;
        }
      }
      for (int g = c; g < end; g += kLbThreads)
        if ((g < ntop || g >= kLwMaxBeam) && key_of(g) >= cut) {
          const int j = atomicAdd(&sh_nsurv, 1);  // exactly min(beam, candidates) keys pass; the bound only guards the arrays
          if (j < kLwMaxBeam) t_score[j] = g_score[g], t_id[j] = g_id[g];
        }
      __syncthreads();
      const int nsurv = min(sh_nsurv, beam);  // min(beam, ntop + ng)
      if (!last) {
        if (c < nsurv) g_score[c] = t_score[c], g_id[c] = t_id[c];
        ntop = nsurv;
        ++k;
        __syncthreads();
        continue;
      }

      // the last chunk: the survivors rank themselves, the best gives the threshold, each builds its entry from its id
      int rank = -1, id = 0;
      float s = -INFINITY;
      if (c < nsurv) {
        s = t_score[c], id = t_id[c];
        rank = 0;
        for (int j = 0; j < nsurv; ++j) rank += (t_score[j] > s || (t_score[j] == s && t_id[j] < id)) ? 1 : 0;
        if (rank == 0) sh_best = s;
      }
      __syncthreads();
      if (rank >= 0) {
        const float thr = a.use_thr ? sh_best - a.beam_threshold : -INFINITY;
        if (!(s < thr)) {
          atomicMax(&sh_nnew, rank + 1);  // the survivors above the threshold are a prefix of the rank order
          const int lab = id >> 7, ii = id & 63;
          const bool end_w = (id >> 6) & 1;
          const Beam par = B[ii];
          LbBeam e = LbBeam{par.hash, s, 0, 0, root_deg, lab, par.ntok + (lab != blank && lab != par.tok), par.nw + end_w, LM ? par.pad : 0};
          int word = 0;
          if (end_w) {
            const int wd = word_of[par.beg + slot[ii][lab] + 1];
            e.hash = lb_mix(par.hash, wd);
            word = wd + 1;
            if constexpr (LM) lm_walk(m, par.pad, m.map[wd], e.pad);  // the walk again, for the state this time
          } else if (lab == blank || lab == par.tok) {
            e.node = par.node, e.beg = par.beg, e.deg = par.deg;
          } else if (lab != sil) {
            const int y = par.beg + slot[ii][lab] + 1;
            e.node = y, e.beg = cbeg[y], e.deg = cbeg[y + 1] - cbeg[y];
          }
          float pmax = 0.f;  // nothing is outstanding at the root
          if constexpr (SM)
            if (!end_w) pmax = e.node == par.node ? par.pmax : smax[e.node];
          N[rank] = lb_entry<Beam>(e, pmax);
          bp[(size_t)t * beam + rank] = make_int2((ii << 16) | lab, word);
        }
      }
      __syncthreads();
      ++k;
    }
    nb = sh_nnew;
    cur ^= 1;
    __syncthreads();  // sh_nnew is cleared at the top of the next frame
    if (nb == 0) break;  // no candidate survived the frame: the sequence ends without a hypothesis
  }

#include "eec_lexbeam_epilogue.inc"
}

}  // namespace eec

extern "C" {

size_t eec_ctc_lexbeam_wide_workspace_bytes(int n_seq, int Tq, int beam_size) {
  return n_seq > 0 && Tq > 0 && beam_size > 0 ? (size_t)n_seq * Tq * beam_size * sizeof(int2) : 0;
}

int eec_ctc_lexbeam_wide_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                                int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm, float lm_weight,
                                const void* smear, int log_add) {
  using namespace eec;
  using eech::fail;
  const std::string me("eec_ctc_lexbeam_wide_decode");
  const bool with_lm = lm != nullptr, with_smear = smear != nullptr;
  if (smear && !lm) return fail(EEC_ERR_BAD_ARG, me + ": smear without lm: it is the model's scores that are smeared");
  if (n_seq < 0 || Tq < 1 || max_words < 1) return fail(EEC_ERR_BAD_ARG, me + ": needs n_seq >= 0, Tq >= 1, max_words >= 1");
  if (V > 256 || V < 2 || beam_size < 1 || beam_size > kLwMaxBeam || nbest < 1 || nbest > beam_size)
    return fail(EEC_ERR_UNSUPPORTED, me + ": needs 2 <= V <= 256, 1 <= beam_size <= " + std::to_string(kLwMaxBeam) + ", 1 <= nbest <= beam_size");
  if (blank < 0 || blank >= V || sil < -1 || sil >= V || sil == blank)
    return fail(EEC_ERR_BAD_ARG, me + ": needs blank in [0, V), sil -1 or in [0, V) and not the blank");
  if (with_lm && !std::isfinite(lm_weight)) return fail(EEC_ERR_BAD_ARG, me + ": lm_weight must be finite");
  if (with_smear && ((uintptr_t)smear & 7)) return fail(EEC_ERR_BAD_ARG, me + ": smear must be 8-byte aligned");
  if (n_seq == 0) return 0;
  if (!logp || !trie || !words || !word_count || !tokens || !token_count || !scores || !n_hyp || !workspace)
    return fail(EEC_ERR_BAD_ARG, me + ": null argument");
  if (((uintptr_t)trie | (uintptr_t)workspace | (uintptr_t)lm) & 7) return fail(EEC_ERR_BAD_ARG, me + ": trie, lm and workspace must be 8-byte aligned");
  if (workspace_bytes < eec_ctc_lexbeam_wide_workspace_bytes(n_seq, Tq, beam_size))
    return fail(EEC_ERR_WORKSPACE, me + ": workspace below eec_ctc_lexbeam_wide_workspace_bytes()");
  LbSmArgs a;
  a.logp = logp, a.em_len = em_len, a.trie = (const int*)trie;
  a.Tq = Tq, a.V = V, a.blank = blank, a.sil = sil, a.beam = beam_size, a.nbest = nbest, a.max_words = max_words;
  a.use_thr = std::isfinite(beam_threshold) ? 1 : 0;
  a.word_score = word_score, a.sil_score = sil_score, a.beam_threshold = beam_threshold;
  a.words = words, a.word_count = word_count, a.tokens = tokens, a.token_count = token_count, a.timesteps = timesteps, a.n_hyp = n_hyp;
  a.scores = scores, a.backptr = (int2*)workspace;
  a.lm = (const int*)lm, a.lm_weight = with_lm ? lm_weight : 0.f, a.smear = (const int*)smear;
  const dim3 grid(n_seq), block(kLbThreads);
  hipStream_t st = (hipStream_t)stream;
  if (log_add && with_smear)
    hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<true, true, true>), grid, block, 0, st, a);
  else if (log_add && with_lm)
    hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<true, false, true>), grid, block, 0, st, a);
  else if (log_add)
    hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<false, false, true>), grid, block, 0, st, a);
  else if (with_smear)
    hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<true, true, false>), grid, block, 0, st, a);
  else if (with_lm)
    hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<true, false, false>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<false, false, false>), grid, block, 0, st, a);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
