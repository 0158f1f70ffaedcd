// What the two lexicon-constrained CTC beam search kernels share (ctc_lexbeam.hip: beams up to 16, a thread's candidates in
// registers; ctc_lexbeam_wide.hip: beams up to 64, the frame's merged candidates in LDS).  The two differ in where candidates live
// and how survivors are picked, and in nothing else; everything that is the same statement is here, once: the images' magic
// numbers, the beam entry, the one argument struct, LmView with lm_view (the host's smear table builder in lexpack.hip reads the
// model through it too), the n-gram walk, lm_add, log_add; then, in the order a kernel calls them, lb_context, lb_start,
// lb_fill_slots, lb_expand -- THE device statement of the candidate rules -- lb_survive and lb_epilogue.  All of it is
// __forceinline__: each kernel compiles it into its own body.  The search itself is stated in include/eec.h.
#pragma once
#include <limits.h>
#include <math.h>

#include <type_traits>

#include "eec_kernels.h"

namespace eec {

constexpr int kLbMagic = 0x54434545;  // "EECT"
constexpr int kLbHeader = 16;
constexpr int kLbMaxBeam = 16;  // the narrow kernel's largest beam
constexpr int kLwMaxBeam = 64;  // the wide kernel's
constexpr int kLbThreads = 256;
constexpr int kLbNoChild = 255;  // a node has at most 255 children (V <= 256, no blank edge): offsets 0 .. 254

struct LbBeam {
  unsigned long long hash;  // identity of the word history
  float score;
  int node, beg, deg;  // trie node, its first edge, its child count
  int tok;             // label of the last frame; -1 at the start.  "previous frame was blank" is tok == blank || tok < 0
  int ntok, nw;        // collapsed labels and words so far
  int pad;             // with a model: the LM state, a node of the n-gram image
};

// the history hash's step, as cb_mix in ctc_beam.hip
__device__ __forceinline__ unsigned long long lb_mix(unsigned long long h, int c) {
  unsigned long long z = h ^ ((unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ... with smearing also the advance payment outstanding at its node, smax[node] (0 at the root)
struct LbBeamSm : LbBeam {
  float pmax;
  int pad2;
};

template <bool SM>
using LbBeamOf = std::conditional_t<SM, LbBeamSm, LbBeam>;

template <typename Beam>
__device__ __forceinline__ Beam lb_entry(const LbBeam& b, float pmax) {
  if constexpr (std::is_same_v<Beam, LbBeamSm>)
    return LbBeamSm{b, pmax, 0};
  else
    return b;
}

// one argument struct for every mode of both kernels; lm / lm_weight are read with a model only, smear with smearing only
struct LbArgs {
  const float* logp;
  const int* em_len;
  const int* trie;
  int Tq, V, blank, sil, beam, nbest, max_words, use_thr;
  float word_score, sil_score, beam_threshold;
  int *words, *word_count, *tokens, *token_count, *timesteps, *n_hyp;
  float* scores;
  int2* backptr;
  const int* lm;
  float lm_weight;
  const int* smear;
};

constexpr int kSmMagic = 0x53434545;  // "EECS"
constexpr int kSmHeader = 4;

constexpr int kLmMagic = 0x4E434545;  // "EECN"
constexpr int kLmHeader = 16;
constexpr int kLmMaxOrder = 5;

// the n-gram image's sections (include/eec.h)
struct LmView {
  const int *begin, *eword, *suffix, *map;
  const float *logp, *backoff;
  int top_begin, bos, eos;
};

// the one place that maps the header words of a packed n-gram image (include/eec.h) to its sections
__host__ __device__ __forceinline__ LmView lm_view(const int* lm) {
  LmView m;
  m.begin = lm + lm[9], m.eword = lm + lm[10], m.suffix = lm + lm[13], m.map = lm + lm[14];
  m.logp = (const float*)(lm + lm[11]), m.backoff = (const float*)(lm + lm[12]);
  m.top_begin = lm[8], m.bos = lm[6], m.eos = lm[7];
  return m;
}

// log10 p(v | state s) by the back-off walk of include/eec.h, fp32 additions in the walk's order; `next`: the state after v.
// The root finds every word without a search (the unigram of word v is node v + 1), so the walk ends after at most `order` steps;
// the bound keeps a damaged image from looping.  The smear table's host code runs this very function: one sequence of additions.
__host__ __device__ __forceinline__ float lm_walk(const LmView& m, int s, int v, int& next) {
  float acc = 0.f;
  for (int d = 0; d <= kLmMaxOrder; ++d) {
    int x = v + 1;
    if (s != 0) {
      int lo = m.begin[s];
      const int end = m.begin[s + 1];
      int hi = end;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m.eword[mid] < v)
          lo = mid + 1;
        else
          hi = mid;
      }
      x = (lo < end && m.eword[lo] == v) ? lo + 1 : -1;
    }
    if (x >= 0) {
      acc = acc + m.logp[x];
      next = x < m.top_begin ? x : m.suffix[x];
      return acc;
    }
    acc = acc + m.backoff[s];
    s = m.suffix[s];
  }
  next = 0;
  return acc;
}

// LM = false is the model-free search; LM = true adds the model's score at word ends and at the end of the sentence
// s + lm_weight * acc, the product rounded on its own: the two operations must not contract into a fused multiply-add
// (__fmul_rn / __fadd_rn are plain operators to this compiler and do contract)
__device__ __forceinline__ float lm_add(float s, float lm_weight, float acc) {
#pragma clang fp contract(off)
  const float term = lm_weight * acc;
  return s + term;
}

// log_add(a, b) = log(exp(a) + exp(b)) as the fixed sequence of fp32 operations include/eec.h states (constants, order, cutoff):
// every step is an IEEE-exact operation and nothing contracts, so device, host and a numpy float32 restatement agree bit for bit
constexpr float kLaCutoff = -17.34375f;  // exp(d) < 2^-25 at and below it: the sum would round back to hi
__host__ __device__ __forceinline__ float lb_log_add(float a, float b) {
#pragma clang fp contract(off)
  const bool a_hi = a > b;
  const float hi = a_hi ? a : b, lo = a_hi ? b : a;
  const float d = lo - hi;
  if (!(d > kLaCutoff)) return hi;
  // x = exp(d): d = n ln 2 + r, |r| <= ln 2 / 2; exp(r) by its Taylor polynomial of degree 7
  const float n = rintf(d * 1.44269502f);
  float r = d - n * 0.693145751953125f;
  r = r - n * 1.42860677e-06f;
  float p = 1.98412701e-04f;
  p = p * r + 1.38888892e-03f;
  p = p * r + 8.33333377e-03f;
  p = p * r + 4.16666679e-02f;
  p = p * r + 0.166666672f;
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  const float x = ldexpf(p, (int)n);
  // log(1 + x): u = 1 + x in [1, 2], halved above sqrt 2; log u = m P(m), m = u - 1 (exact), P of degree 10
  float u = 1.0f + x;
  const bool halved = u > 1.41421354f;
  if (halved) u = u * 0.5f;
  const float m = u - 1.0f;
  float q = 0.0657233745f;
  q = q * m + -0.116206668f;
  q = q * m + 0.119458839f;
  q = q * m + -0.12420819f;
  q = q * m + 0.142122895f;
  q = q * m + -0.166665554f;
  q = q * m + 0.20002535f;
  q = q * m + -0.250000626f;
  q = q * m + 0.333333015f;
  q = q * m + -0.5f;
  q = q * m + 1.0f;
  float s = m * q;
  if (halved) s = s + 0.693147182f;
  return hi + s;
}

// the merge's call in both kernels: one copy of the sequence per kernel (merges are rare per thread and frame)
__device__ __noinline__ inline float lb_log_add_call(float a, float b) { return lb_log_add(a, b); }

// What a workgroup knows of its sequence and of the three images before the first frame
struct LbCtx {
  bool ok;   // the images are the ones the call describes
  int seq;   // the sequence of this workgroup
  int L;     // its frames; 0: nothing to decode, the sequence ends without a hypothesis
  const int* cbeg;            // trie sections (include/eec.h)
  const unsigned char* ctok;
  const int* word_of;
  int root_deg;
  const float* smax;  // with smearing: the table's values, else null
  LmView m;           // with a model, else zeros
  const float* lp_seq;
  int2* bp;
};

// A trie that is not the one the call describes is not read past its header: every sequence ends without a hypothesis
// ... and so is a model that is none, or was packed for another lexicon, or a smear table that is none or another trie's
template <bool LM, bool SM>
__device__ __forceinline__ LbCtx lb_context(const LbArgs& a, int seq) {
  LbCtx cx;
  bool fits = true;
  if constexpr (LM) fits = a.lm[0] == kLmMagic && a.lm[5] == a.trie[10];
  if constexpr (SM) fits = fits && a.smear[0] == kSmMagic && a.smear[1] == a.trie[1];
  const bool ok = a.trie[0] == kLbMagic && a.trie[1] >= 1 && a.trie[3] == a.V && a.trie[4] == a.blank && a.trie[5] == a.sil && fits;
  int L = a.em_len ? a.em_len[seq] : a.Tq;
  if (!ok || L < 1 || L > a.Tq) L = 0;
  cx.ok = ok, cx.seq = seq, cx.L = L;
  cx.cbeg = a.trie + (ok ? a.trie[6] : 0);
  cx.ctok = (const unsigned char*)(a.trie + (ok ? a.trie[7] : 0));
  cx.word_of = a.trie + (ok ? a.trie[8] : 0);
  cx.root_deg = L > 0 ? cx.cbeg[1] : 0;
  cx.smax = nullptr;
  if constexpr (SM) cx.smax = (const float*)(a.smear + (ok ? kSmHeader : 0));
  cx.m = {};
  if constexpr (LM)
    if (ok) cx.m = lm_view(a.lm);
  cx.lp_seq = a.logp + (size_t)seq * a.Tq * a.V;
  cx.bp = a.backptr + (size_t)seq * a.Tq * a.beam;
  return cx;
}

// Thread 0 writes the first beam entry (the root, no label yet, the model's start state); every thread gets its label's log-prob
// of frame 0, one frame ahead of its use as in the frame loop.  The caller's barrier follows
template <bool LM, bool SM>
__device__ __forceinline__ float lb_start(const LbArgs& a, const LbCtx& cx, LbBeamOf<SM>* first, int c) {
  if (c == 0) *first = lb_entry<LbBeamOf<SM>>(LbBeam{0x243F6A8885A308D3ull, 0.f, 0, 0, cx.root_deg, -1, 0, 0, LM ? cx.m.bos : 0}, 0.f);
  return (cx.L > 0 && c < a.V) ? cx.lp_seq[c] : -INFINITY;
}

// Child lookup as a scatter instead of a search: rows 0 .. nb - 1 of slot <- kLbNoChild, then for beam entry i the first deg(node_i)
// threads read the node's child bytes (one coalesced load) and write their edge offset to slot[i][label].  The breadth-first node
// numbering makes the child of edge k node k + 1, so the table needs no target.  The row count is the caller's (its largest beam)
template <typename Beam>
__device__ __forceinline__ void lb_fill_slots(unsigned char (*slot)[256], const Beam* B, int nb, const unsigned char* ctok, int c) {
  for (int k = c; k < nb * 64; k += kLbThreads) ((unsigned*)slot)[k] = ~0u;
  __syncthreads();
  for (int i = 0; i < nb; ++i)
    if (c < B[i].deg) slot[i][ctok[B[i].beg + c]] = (unsigned char)c;
  __syncthreads();
}

// What one beam entry gives one label: at most one in-place / in-word candidate (w = 0) and one word-end candidate (w = 1)
struct LbCand {
  float s0, s1;           // their scores; -inf: there is none
  int node, beg, deg;     // w = 0: the trie node it stands at, with its child range (w = 1 stands at the root)
  int word;               // w = 1: the word that ends, else -1
  unsigned long long h1;  // w = 1: the history with that word (w = 0 keeps the entry's)
};

// THE candidate rules of include/eec.h for beam entry b and label c (c < V), lpc the label's log-prob in this frame:
//   * blank, or the repeat of a non-blank label: the state stays (sil pays sil_score also when it repeats);
//   * sil otherwise only at the root;
//   * any other label needs a child of b's node, found through slot_c = slot[i][c], the byte lb_fill_slots left for (entry, label)
//     (a reference: it is read on this path only).  The child is an in-word candidate if it has children itself -- with smearing
//     charged the increase of the maximum, smax[y] - pmax, in advance -- and a word-end candidate if it ends a word: word_score,
//     with a model the walk's score, with smearing the advance payment taken back (acc - pmax before the weight);
//   * -inf and NaN are dropped.
// fp32 operations in the stated order: base = score + lpc first, lm_add (uncontracted) as it is.
template <bool LM, bool SM>
__device__ __forceinline__ LbCand lb_expand(const LbArgs& a, const LbCtx& cx, const LbBeamOf<SM>& b, int c, float lpc, const unsigned char& slot_c) {
  LbCand r = {-INFINITY, -INFINITY, 0, 0, 0, -1, 0};
  const float base = b.score + lpc;
  if (c == a.blank || c == b.tok) {
    r.s0 = (c == a.sil) ? base + a.sil_score : base;
    r.node = b.node, r.beg = b.beg, r.deg = b.deg;
  } else if (c == a.sil) {
    if (b.node == 0) {
      r.s0 = base + a.sil_score;
      r.deg = cx.root_deg;
    }
  } else {
    const int j = slot_c;
    if (j != kLbNoChild) {
      const int y = b.beg + j + 1;
      const int yb = cx.cbeg[y], ye = cx.cbeg[y + 1], word = cx.word_of[y];
      float sy = 0.f, pmax = 0.f;
      if constexpr (SM) sy = cx.smax[y], pmax = b.pmax;
      if (ye > yb) {
        r.s0 = base;
        if constexpr (SM) r.s0 = lm_add(base, a.lm_weight, sy - pmax);  // the increase of the maximum, paid in advance
        r.node = y, r.beg = yb, r.deg = ye - yb;
      }
      if (word >= 0) {
        r.s1 = base + a.word_score;
        if constexpr (LM) {
          int next;
          float acc = lm_walk(cx.m, b.pad, cx.m.map[word], next);
          if constexpr (SM) acc = acc - pmax;  // the true score replaces what was paid
          r.s1 = lm_add(r.s1, a.lm_weight, acc);
        }
        r.word = word;
        r.h1 = lb_mix(b.hash, word);
      }
    }
  }
  if (!(r.s0 > -INFINITY)) r.s0 = -INFINITY;  // -inf and NaN are dropped
  if (!(r.s1 > -INFINITY)) r.s1 = -INFINITY;
  return r;
}

// The survivor of rank `rank` in frame t: its beam entry N[rank] and its back-pointer (parent rank, label, completed word + 1).
// par = B[ii] is its parent, lab its label, end_w says whether it ends `word`; (node, beg, deg, hash) is where it stands and its
// history -- for a word end the root (0, 0, root_deg) and the history with the word, else the w = 0 candidate's node and the
// parent's history.  The narrow kernel has the five in registers, the wide kernel works them out again from slot.  With a model a
// word end redoes its walk, for the state this time; with smearing the payment outstanding at the node rides in the entry
template <bool LM, bool SM>
__device__ __forceinline__ void lb_survive(const LbArgs& a, const LbCtx& cx, LbBeamOf<SM>* N, int t, const LbBeamOf<SM>& par, int ii, int lab,
                                           bool end_w, int node, int beg, int deg, unsigned long long hash, int word, float score, int rank) {
  LbBeam e = LbBeam{hash, score, node, beg, deg, lab, par.ntok + (lab != a.blank && lab != par.tok), par.nw + end_w, LM ? par.pad : 0};
  if constexpr (LM)
    if (end_w) lm_walk(cx.m, par.pad, cx.m.map[word], e.pad);
  float pmax = 0.f;  // nothing is outstanding at the root
  if constexpr (SM)
    if (!end_w) pmax = e.node == par.node ? par.pmax : cx.smax[e.node];
  N[rank] = lb_entry<LbBeamOf<SM>>(e, pmax);
  cx.bp[(size_t)t * a.beam + rank] = make_int2((ii << 16) | lab, end_w ? word + 1 : 0);
}

// The end of both kernels, after a barrier that made the last frame's beam B[0 .. nb) visible.  The complete hypotheses (node 0) in
// rank order are best first; one thread walks each one's back-pointers.  fin_rank, fin_ntok, fin_nw (and with a model fin_score)
// are LDS arrays of the caller with at least max(beam, nbest) entries, fin_n one LDS word
template <bool LM, bool SM>
__device__ __forceinline__ void lb_epilogue(const LbArgs& a, const LbCtx& cx, const LbBeamOf<SM>* B, int nb, int c, int* fin_rank, int* fin_ntok,
                                            int* fin_nw, float* fin_score, int& fin_n) {
  const int seq = cx.seq, L = cx.L, Tq = a.Tq, beam = a.beam, blank = a.blank;
  const int2* bp = cx.bp;
  if (c == 0) {
    int n = 0;
    if constexpr (LM) {
      // ... after the </s> term they no longer are: ordered by (final score descending, rank ascending), one thread's insertion
      if (L > 0)
        for (int i = 0; i < nb; ++i) {
          const LbBeam e = B[i];
          if (e.node != 0) continue;
          float f = e.score;
          if (cx.m.eos >= 0) {
            int next;
            f = lm_add(f, a.lm_weight, lm_walk(cx.m, e.pad, cx.m.eos, next));
          }
          int k = n++;
          for (; k > 0 && f > fin_score[k - 1]; --k) fin_score[k] = fin_score[k - 1], fin_rank[k] = fin_rank[k - 1];
          fin_score[k] = f, fin_rank[k] = i;
        }
      n = min(n, a.nbest);
    } else {
      if (L > 0)
        for (int i = 0; i < nb; ++i)
          if (B[i].node == 0 && n < a.nbest) fin_rank[n++] = i;
    }
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
      const LbBeam e = B[k];
      n = e.ntok, nw = e.nw, score = LM ? fin_score[c] : e.score;
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

// The launch of the wide-beam kernel's instantiation (ctc_lexbeam_wide.hip), for the one host path in ctc_lexbeam.hip
template <bool LM, bool SM, bool LA>
void lexbeam_wide_launch(const LbArgs& a, int n_seq, hipStream_t stream);

}  // namespace eec

