// Lexicon-constrained CTC beam search for beams up to 64 (eec_ctc_lexbeam_wide_decode): the search of ctc_lexbeam.hip -- stated in
// include/eec.h, model, smearing and log-add merging included -- where a thread's candidates no longer fit registers.  The candidate
// id is (2 c + w) * 64 + i; nothing else of the statement differs, so for beams of 16 or less the results are those of the narrow
// entries bit for bit.  tests/lexbeam_wide_cases.py is the plain-Python statement and the judge.  Out of scope: beams over 64.
//
// This file holds the wide strategy alone: where the merged candidates live and how the survivors are picked.  Everything that is
// the narrow kernel's statement too is called from eec_lexbeam.h -- lb_context and lb_start before the first frame, lb_fill_slots,
// the candidate rules (lb_expand), a survivor's entry and back-pointer (lb_survive), the epilogue (lb_epilogue), log_add's one
// out-of-line wrapper -- and the host path (the argument checks, the choice of the instantiation, eec_ctc_lexbeam_wide_decode
// itself) is lb_decode in ctc_lexbeam.hip, which reaches the kernels here through lexbeam_wide_launch.
//
// One 256-thread workgroup per sequence, thread c owns frame label c, as in the narrow kernel: candidates that can merge share their
// label, so every merge is still local to one thread.  What changes is where candidates live and how survivors are picked.  Per frame:
//   * the child-lookup byte table slot[i][label] is built by the narrow kernel's lb_fill_slots (64 rows here);
//   * thread c walks the beam in rank order and OFFERS each live candidate lb_expand returns to a list of merged candidates ("groups") in LDS.  A group
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
//     threshold (score >= best - beam_threshold stays), and each works out from its id where it stands and hands that to lb_survive.
// The epilogue is the narrow kernel's (lb_epilogue).
//
// Resources (tools/kernel_resources.py on build/ctc_lexbeam_wide.o, gfx950): 63 VGPRs (69 with the model, 65 with smearing), 106
// SGPRs, no scratch, no vector spills (42 to 84 scalars parked in VGPR lanes); 50 736 B of LDS without a model, 50 992 B with one, 52 016 B with smearing,
// and 4 096 B more with log-add (54 832 / 55 088 / 56 112 B) -- static, under the 64 KB that need no function attribute.  By LDS a
// CU (160 KB) holds two workgroups (three of the Viterbi instantiations), so the standing batch of 384 sequences is resident at once
// on 256 CUs, in one pass, as with the narrow kernel.
// Latency-bound integer and LDS work over T' serial frames, and slower than the narrow kernel where both serve: measured on the
// 384 x 256-frame batch, 57.4 ms at beam 16 against the narrow kernel's 12.7 ms, 157 ms at 32, 446 ms at 64 (DESIGN.md,
// profiles/lexbeam_wide_time.json).  Beams of 16 or less therefore stay with the narrow kernels.
#include <limits.h>
#include <math.h>

#include "eec_kernels.h"
#include "eec_lexbeam.h"

namespace eec {

constexpr int kLwCap = 1024;                    // groups of one pass
constexpr int kLwList = kLwMaxBeam + kLwCap;     // list slots: [0, 64) the survivors carried between chunks, then the pass's groups
constexpr int kLwTable = 2048;                   // hash slots (a power of two, twice the groups)
constexpr int kLwChunk = kLwCap - 2 * kLwMaxBeam;  // candidates at which a chunk closes; a thread adds at most 2 * 64 - 1 more

template <bool LM, bool SM, bool LA>
__global__ __launch_bounds__(kLbThreads) void ctc_lexbeam_wide_kernel(const LbArgs a) {
  static_assert(LM || !SM, "smearing needs a model");
  using Beam = LbBeamOf<SM>;
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
  const int c = threadIdx.x, lane = c & 63, w = c >> 6;
  const int V = a.V, blank = a.blank, sil = a.sil, beam = a.beam;
  const LbCtx cx = lb_context<LM, SM>(a, blockIdx.x);
  const int L = cx.L;

  float* const raw = LA ? g_raw : g_score + kLwMaxBeam;  // Viterbi: the merged score is the best raw score
  int cur = 0, nb = 1;
  float lp_next = lb_start<LM, SM>(a, cx, &bufs[0][0], c);
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
    if (t + 1 < L && c < V) lp_next = cx.lp_seq[(size_t)(t + 1) * V + c];  // one frame ahead of its use

    lb_fill_slots(slot, B, nb, cx.ctok, c);

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
            if constexpr (LA) g_score[kLwMaxBeam + g] = lb_log_add_call(g_score[kLwMaxBeam + g], s);
            if (s > raw[g]) raw[g] = s, g_id[kLwMaxBeam + g] = (unsigned short)id;  // the lower id stays on a tie
            return;
          }
        }
        p = (p + 1) & (kLwTable - 1);
      }
    };

    // this label's candidates from every beam entry, by lb_expand's rules; returns how many live
    auto emit = [&](bool insert) {
      int live = 0;
      if (c >= V) return live;
      auto put = [&](int node, unsigned long long h, float s, int id) {
        if (!(s > -INFINITY)) return;  // lb_expand left -inf where there is no candidate
        ++live;
        if (insert) offer(node, h, s, id);
      };
      // The order is this kernel's concern, not the rules': offer() folds a group in id order.  The repeat of a word's last label at
      // the root is the only w = 0 candidate that can meet word-end candidates (both stand at the root), and the lowest id: it goes first
      auto root_repeat = [&](int i) { return c != blank && c != sil && B[i].tok == c && B[i].node == 0; };
      for (int i = 0; i < nb; ++i)
        if (root_repeat(i)) put(0, B[i].hash, lb_expand<LM, SM>(a, cx, B[i], c, lpc, slot[i][c]).s0, 128 * c + i);
      for (int i = 0; i < nb; ++i) {
        if (root_repeat(i)) continue;  // went first
        const LbCand x = lb_expand<LM, SM>(a, cx, B[i], c, lpc, slot[i][c]);
        put(x.node, B[i].hash, x.s0, 128 * c + i);
        put(0, x.h1, x.s1, 128 * c + 64 + i);
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
          // where the survivor stands, worked out again from its id and slot: a word end at the root with the new history, sil at the
          // root, blank or a repeat where the parent stands, else the child
          int node = 0, beg = 0, deg = cx.root_deg, word = -1;
          unsigned long long hash = par.hash;
          if (end_w) {
            word = cx.word_of[par.beg + slot[ii][lab] + 1];
            hash = lb_mix(par.hash, word);
          } else if (lab == blank || lab == par.tok) {
            node = par.node, beg = par.beg, deg = par.deg;
          } else if (lab != sil) {
            node = par.beg + slot[ii][lab] + 1;
            beg = cx.cbeg[node], deg = cx.cbeg[node + 1] - beg;
          }
          lb_survive<LM, SM>(a, cx, N, t, par, ii, lab, end_w, node, beg, deg, hash, word, s, rank);
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

  lb_epilogue<LM, SM>(a, cx, bufs[cur], nb, c, fin_rank, fin_ntok, fin_nw, fin_score, fin_n);
}

// the host path -- checks, the choice of the instantiation, eec_ctc_lexbeam_wide_decode itself -- is lb_decode in ctc_lexbeam.hip
template <bool LM, bool SM, bool LA>
void lexbeam_wide_launch(const LbArgs& a, int n_seq, hipStream_t stream) {
  hipLaunchKernelGGL((ctc_lexbeam_wide_kernel<LM, SM, LA>), dim3(n_seq), dim3(kLbThreads), 0, stream, a);
}
template void lexbeam_wide_launch<false, false, false>(const LbArgs&, int, hipStream_t);
template void lexbeam_wide_launch<true, false, false>(const LbArgs&, int, hipStream_t);
template void lexbeam_wide_launch<true, true, false>(const LbArgs&, int, hipStream_t);
template void lexbeam_wide_launch<false, false, true>(const LbArgs&, int, hipStream_t);
template void lexbeam_wide_launch<true, false, true>(const LbArgs&, int, hipStream_t);
template void lexbeam_wide_launch<true, true, true>(const LbArgs&, int, hipStream_t);

}  // namespace eec
