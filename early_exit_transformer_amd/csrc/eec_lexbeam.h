// What the two lexicon-constrained CTC beam search kernels share (ctc_lexbeam.hip: beams up to 16, a thread's candidates in
// registers; ctc_lexbeam_wide.hip: beams up to 64, the frame's merged candidates in LDS): the magic numbers of the three images, the
// beam entry, the argument structs, the n-gram walk, lm_add and log_add.  The epilogue that walks the back-pointers and writes the
// outputs is eec_lexbeam_epilogue.inc, included as text by both kernels.  The search itself is stated in include/eec.h.
#pragma once
#include <limits.h>
#include <math.h>

#include <type_traits>

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

template <typename Beam>
__device__ __forceinline__ Beam lb_entry(const LbBeam& b, float pmax) {
  if constexpr (std::is_same_v<Beam, LbBeamSm>)
    return LbBeamSm{b, pmax, 0};
  else
    return b;
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

struct LbLmArgs : LbArgs {
  const int* lm;
  float lm_weight;
};

struct LbSmArgs : LbLmArgs {
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

template <bool LM, bool SM, typename Args>
__device__ __forceinline__ bool lm_fits(const Args& a) {
  bool fits = true;
  if constexpr (LM) fits = a.lm[0] == kLmMagic && a.lm[5] == a.trie[10];
  if constexpr (SM) fits = fits && a.smear[0] == kSmMagic && a.smear[1] == a.trie[1];
  return fits;
}

}  // namespace eec
