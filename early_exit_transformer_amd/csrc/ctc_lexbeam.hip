// Lexicon-constrained CTC beam search on the device, with N-best: what the reference's ctc_predict / ctc_predict_ / beam_predict
// call through torchaudio's ctc_decoder(lexicon=..., tokens=..., nbest=N_BEST, log_add=False, word_score=w_ins, sil_token="<pad>",
// blank_token="@") without a language model (util/beam_infer.py:51-65, 85-126).  That decoder (flashlight-text) is third-party code
// outside the reference tree and not installed: what is built is the published algorithm -- token-trie beam search under CTC,
// Viterbi merging (log_add=False), no language model -- stated completely in include/eec.h; tests/lexbeam_cases.py is its
// plain-Python statement and the judge of this kernel.  Parity with the third-party decoder is unpinned.
// Out of scope: a language model, log_add=True (the reference's character-lexicon branch), unknown-word scores, beams over 16.
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
// Scores are fp32 additions in the order include/eec.h writes them, no reductions, no log / exp: the result is bit-identical to
// the statement.  Latency-bound integer / scalar work over T' serial frames: it is sized to keep all E * B = 384 sequences of a
// batch in flight at once (5.4 KB of LDS, well under two workgroups per CU), not for the roofline.  The real lexicon's image
// (89 114 words, 162 621 nodes, 1.5 MB) is read-only and shared by all workgroups: it sits in L2.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"

namespace eec {

constexpr int kLbMagic = 0x54434545;  // "EECT"
constexpr int kLbHeader = 16;
constexpr int kLbMaxBeam = 16;
constexpr int kLbThreads = 256;
constexpr int kLbNoChild = 255;  // a node has at most 255 children (V <= 256, no blank edge): offsets 0 .. 254

struct LbBeam {
  unsigned long long hash;  // identity of the word history
  float score;
  int node, beg, deg;  // trie node, its first edge, its child count
  int tok;             // label of the last frame; -1 at the start.  "previous frame was blank" is tok == blank || tok < 0
  int ntok, nw;        // collapsed labels and words so far
  int pad;
};

// the history hash's step, as cb_mix in ctc_beam.hip
__device__ __forceinline__ unsigned long long lb_mix(unsigned long long h, int c) {
  unsigned long long z = h ^ ((unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct LbArgs {
  const float* logp;
  const int* em_len;
  const int* trie;
  int Tq, V, blank, sil, beam, nbest, max_words, use_thr;
  float word_score, sil_score, beam_threshold;
  int *words, *word_count, *tokens, *token_count, *timesteps, *n_hyp;
  float* scores;
  int2* backptr;
};

__global__ __launch_bounds__(kLbThreads) void ctc_lexbeam_kernel(const LbArgs a) {
  __shared__ LbBeam bufs[2][kLbMaxBeam];
  __shared__ __attribute__((aligned(16))) unsigned char slot[kLbMaxBeam][256];  // edge offset of label c below beam i's node
  __shared__ float red_v[4];
  __shared__ int red_id[4];
  __shared__ int fin_rank[kLbMaxBeam], fin_ntok[kLbMaxBeam], fin_nw[kLbMaxBeam], fin_n;
  const int seq = blockIdx.x, c = threadIdx.x, lane = c & 63, w = c >> 6;
  const int V = a.V, blank = a.blank, sil = a.sil, beam = a.beam, Tq = a.Tq;

  // a trie that is not the one the call describes is not read past its header: every sequence ends without a hypothesis
  const bool ok = a.trie[0] == kLbMagic && a.trie[1] >= 1 && a.trie[3] == V && a.trie[4] == blank && a.trie[5] == sil;
  int L = a.em_len ? a.em_len[seq] : Tq;
  if (!ok || L < 1 || L > Tq) L = 0;
  const int* cbeg = a.trie + (ok ? a.trie[6] : 0);
  const unsigned char* ctok = (const unsigned char*)(a.trie + (ok ? a.trie[7] : 0));
  const int* word_of = a.trie + (ok ? a.trie[8] : 0);
  const int root_deg = L > 0 ? cbeg[1] : 0;

  const float* lp_seq = a.logp + (size_t)seq * Tq * V;
  int2* bp = a.backptr + (size_t)seq * Tq * beam;
  int cur = 0, nb = 1;
  if (c == 0) bufs[0][0] = LbBeam{0x243F6A8885A308D3ull, 0.f, 0, 0, root_deg, -1, 0, 0, 0};
  float lp_next = (L > 0 && c < V) ? lp_seq[c] : -INFINITY;
  __syncthreads();

  for (int t = 0; t < L; ++t) {
    const LbBeam* B = bufs[cur];
    LbBeam* N = bufs[cur ^ 1];
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
        const LbBeam b = B[i];
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
            if (ye > yb) {
              s0[i] = base;
              nd0[i] = y, beg0[i] = yb, deg0[i] = ye - yb;
            }
            if (word >= 0) {
              s1[i] = base + a.word_score;
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
          if (np_ == nq_ && hp == hq) {
            if (sq > sp)
              sp = -INFINITY;
            else
              sq = -INFINITY;
          }
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
        const LbBeam par = B[ii];
        LbBeam e = LbBeam{par.hash, gv, 0, 0, root_deg, c, par.ntok + (c != blank && c != par.tok), par.nw + end, 0};
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
        N[r] = e;
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

  // the complete hypotheses (node 0) in rank order are best first; one thread walks each one's back-pointers
  if (c == 0) {
    int n = 0;
    if (L > 0)
      for (int i = 0; i < nb; ++i)
        if (bufs[cur][i].node == 0 && n < a.nbest) fin_rank[n++] = i;
    fin_n = n;
    a.n_hyp[seq] = n;
  }
  __syncthreads();
  if (c < a.nbest) {
    const size_t o = (size_t)seq * a.nbest + c;
    int n = 0, nw = 0;
    float score = -INFINITY;
    if (c < fin_n) {
      int k = fin_rank[c];
      const LbBeam e = bufs[cur][k];
      n = e.ntok, nw = e.nw, score = e.score;
      int* tok_out = a.tokens + o * Tq;
      int* ts_out = a.timesteps ? a.timesteps + o * Tq : nullptr;
      int* w_out = a.words + o * a.max_words;
      int nt = n, nwd = nw;
      int2 at = bp[(size_t)(L - 1) * beam + k];
      for (int t = L - 1; t >= 0; --t) {
        const int lab = at.x & 0xffff;
        const int2 prev = t > 0 ? bp[(size_t)(t - 1) * beam + (at.x >> 16)] : make_int2(0xffff, 0);
        if (lab != blank && lab != (prev.x & 0xffff) && nt > 0) {  // the first frame of a run of one label
          tok_out[--nt] = lab;
          if (ts_out) ts_out[nt] = t;
        }
        if (at.y && nwd > 0 && --nwd < a.max_words) w_out[nwd] = at.y - 1;
        at = prev;
      }
    }
    a.scores[o] = score;
    a.token_count[o] = n;
    a.word_count[o] = nw;
    fin_ntok[c] = n;
    fin_nw[c] = min(nw, a.max_words);
  }
  __syncthreads();
  // what lies past a hypothesis' counts is -1
  for (int k = c; k < a.nbest * Tq; k += kLbThreads) {
    const int j = k / Tq;
    if (k - j * Tq >= fin_ntok[j]) {
      const size_t o = ((size_t)seq * a.nbest + j) * Tq + (k - j * Tq);
      a.tokens[o] = -1;
      if (a.timesteps) a.timesteps[o] = -1;
    }
  }
  for (int k = c; k < a.nbest * a.max_words; k += kLbThreads) {
    const int j = k / a.max_words;
    if (k - j * a.max_words >= fin_nw[j]) a.words[((size_t)seq * a.nbest + j) * a.max_words + (k - j * a.max_words)] = -1;
  }
}

static size_t lb_image_dwords(unsigned long long nodes) {  // nodes >= 1
  return (size_t)(kLbHeader + (nodes + 1) + (nodes - 1 + 3) / 4 + nodes + 1) & ~(size_t)1;
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

size_t eec_ctc_lexbeam_workspace_bytes(int n_seq, int Tq, int beam_size) {
  return n_seq > 0 && Tq > 0 && beam_size > 0 ? (size_t)n_seq * Tq * beam_size * sizeof(int2) : 0;
}

int eec_ctc_lexbeam_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                           int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                           int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                           int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace eec;
  using eech::fail;
  if (n_seq < 0 || Tq < 1 || max_words < 1) return fail(EEC_ERR_BAD_ARG, "eec_ctc_lexbeam_decode: needs n_seq >= 0, Tq >= 1, max_words >= 1");
  if (V > 256 || V < 2 || beam_size < 1 || beam_size > kLbMaxBeam || nbest < 1 || nbest > beam_size)
    return fail(EEC_ERR_UNSUPPORTED, "eec_ctc_lexbeam_decode: needs 2 <= V <= 256, 1 <= beam_size <= " + std::to_string(kLbMaxBeam) +
                                         ", 1 <= nbest <= beam_size");
  if (blank < 0 || blank >= V || sil < -1 || sil >= V || sil == blank)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_lexbeam_decode: needs blank in [0, V), sil -1 or in [0, V) and not the blank");
  if (n_seq == 0) return 0;
  if (!logp || !trie || !words || !word_count || !tokens || !token_count || !scores || !n_hyp || !workspace)
    return fail(EEC_ERR_BAD_ARG, "eec_ctc_lexbeam_decode: null argument");
  if (((uintptr_t)trie | (uintptr_t)workspace) & 7) return fail(EEC_ERR_BAD_ARG, "eec_ctc_lexbeam_decode: trie and workspace must be 8-byte aligned");
  if (workspace_bytes < eec_ctc_lexbeam_workspace_bytes(n_seq, Tq, beam_size))
    return fail(EEC_ERR_WORKSPACE, "eec_ctc_lexbeam_decode: workspace below eec_ctc_lexbeam_workspace_bytes()");
  LbArgs a;
  a.logp = logp, a.em_len = em_len, a.trie = (const int*)trie;
  a.Tq = Tq, a.V = V, a.blank = blank, a.sil = sil, a.beam = beam_size, a.nbest = nbest, a.max_words = max_words;
  a.use_thr = std::isfinite(beam_threshold) ? 1 : 0;
  a.word_score = word_score, a.sil_score = sil_score, a.beam_threshold = beam_threshold;
  a.words = words, a.word_count = word_count, a.tokens = tokens, a.token_count = token_count, a.timesteps = timesteps, a.n_hyp = n_hyp;
  a.scores = scores, a.backptr = (int2*)workspace;
  hipLaunchKernelGGL(ctc_lexbeam_kernel, dim3(n_seq), dim3(kLbThreads), 0, (hipStream_t)stream, a);
  EEC_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
