// The standard-topology CTC lattice on one wave, stated once for its consumers (ctc_forced_align.hip: the best path;
// ctc_posterior.hip: forward-backward): the 2N + 1 states blank, y_0, blank, y_1, ..., blank of a token row of N <= 255 tokens live
// in registers as a strip of C = 1, 2, 4 or 8 consecutive states per lane (lane l: states l * C .. l * C + C - 1), C chosen per wave
// from the row's own N.  For C >= 2 the even slots of a strip are blanks and the odd ones labels, so a lane has NL = C / 2 label
// slots (slot 2 i + 1 is token l * NL + i); for C = 1 the odd lanes are the labels (lane l: token l >> 1, NL = 1).  The one value
// that crosses a lane boundary forward -- the left neighbour's last state, s - 1 of slot 0 and s - 2 of slot 1 -- comes by one
// from_left (C = 1: two).  One wave serves one row, kStripWaves rows a workgroup: row h is wave h & 3 of workgroup h >> 2, so rows
// that follow each other and share an emission fetch its lines from memory once.  The frame loops are the consumers' own.
// ctc_segment.hip lays a row of up to 4095 tokens over several waves of one workgroup, each a C = 8 strip of 512 states: it takes
// the row checks and the entry head with its own limit (max_tokens) and strip_label<8> with the lane index moved by the wave's.
#pragma once
#include <math.h>

#include <initializer_list>
#include <string>

#include "eec_host.h"
#include "eec_wave.h"

namespace eec {

constexpr int kStripWaves = 4;        // rows per workgroup
constexpr int kStripMaxTokens = 255;  // N: 2N + 1 = 511 states in 64 lanes, eight per lane

// states per lane for a row of N tokens: 2N + 1 <= 64 * C
__host__ __device__ inline int strip_states(int N) { return N <= 31 ? 1 : N <= 63 ? 2 : N <= 127 ? 4 : 8; }
constexpr int strip_labels(int C) { return C >= 2 ? C / 2 : 1; }                  // NL: label slots of a strip
constexpr int strip_log2(int C) { return C == 1 ? 0 : C == 2 ? 1 : C == 4 ? 2 : 3; }  // state s: lane s >> log2 C, slot s & (C - 1)

// The row checks of row h, wave-uniform: N tokens, T frames (em_len clamped to [0, Tq]; frames from T on are never read) of
// emission ei.  ok: 0 <= ei < n_em, 1 <= N <= min(tok_stride, max_tokens), every token a label of [0, V) other than the blank, and
// T >= N + R.
// None of the row's values becomes an address unless ok: N bounds the token reads only once it is known to be within tok_stride,
// ei indexes em_len only once it is known to be an emission, and the caller forms no emission address and runs no strip before
// it has seen ok (a row that is not ok gets the caller's fill values).
struct StripRow {
  int N, T, ei;
  bool ok;
};
__device__ __forceinline__ StripRow strip_row(const int* __restrict__ tk, const int* __restrict__ tok_len, const int* __restrict__ em_index,
                                              const int* __restrict__ em_len, int h, int n_em, int Tq, int V, int tok_stride, int blank,
                                              int lane, int max_tokens = kStripMaxTokens) {
  const int N = __builtin_amdgcn_readfirstlane(tok_len[h]);
  const int ei = __builtin_amdgcn_readfirstlane(em_index ? em_index[h] : h);
  bool ok = ei >= 0 && ei < n_em && N >= 1 && N <= tok_stride && N <= max_tokens;
  int T = 0;
  if (ok) {
    T = __builtin_amdgcn_readfirstlane(em_len ? min(max(em_len[ei], 0), Tq) : Tq);
    bool bad = false;
    int R = 0;  // adjacent equal pairs: each needs a blank frame between its two tokens
    for (int j0 = 0; j0 < N; j0 += 64) {
      const int j = j0 + lane;
      const bool in = j < N;
      const int y = in ? tk[j] : 0, p = (in && j >= 1) ? tk[j - 1] : -1;
      bad = bad || (in && (y < 0 || y >= V || y == blank));
      R += __popcll(__ballot(in && j >= 1 && y == p));
    }
    ok = __ballot(bad) == 0 && T >= N + R;
  }
  return {N, T, ei, ok};
}

// The label slot i of a lane's strip, for a row that passed the row checks.  The states past 2N compute on the blank: forward they
// feed nothing.  A consumer that reads only some of the members pays for those alone.
struct StripLabel {
  int id;      // the token of the label slot; else the blank
  bool own;    // the slot is a label state of the row
  bool skip;   // state s - 2 feeds it
  bool skipn;  // it feeds state s + 2
};
template <int C>
__device__ __forceinline__ StripLabel strip_label(const int* __restrict__ tk, int N, int blank, int lane, int i) {
  const int j = C == 1 ? lane >> 1 : lane * strip_labels(C) + i;
  const bool label = (C == 1 ? (lane & 1) != 0 : true) && j < N;
  const int y = label ? tk[j] : blank, p = (label && j >= 1) ? tk[j - 1] : blank, nx = (label && j + 1 < N) ? tk[j + 1] : blank;
  return {y, label, label && j >= 1 && y != p, label && j + 1 < N && nx != y};
}

// frame 0 of a strip: states 0 and 1 only (em: the emission's first frame; id0: the strip's first label)
template <int C>
__device__ __forceinline__ void strip_frame0(float (&a)[C], const float* __restrict__ em, int blank, int id0, int lane) {
  const float xb = em[blank], x0 = em[id0];
#pragma unroll
  for (int k = 0; k < C; ++k) a[k] = -INFINITY;
  if (C == 1) {
    if (lane == 0) a[0] = xb;
    if (lane == 1) a[0] = x0;
  } else if (lane == 0) {
    a[0] = xb;
    a[C > 1 ? 1 : 0] = x0;
  }
}

// states 2N (hi) and 2N - 1 (lo) out of a strip, wave-uniform: the slot is wave-uniform, the lane is read
template <int C>
__device__ __forceinline__ void strip_end(const float (&a)[C], int N, float& hi, float& lo) {
  const int sN = 2 * N;
  hi = a[0], lo = a[0];
  static_range<1, C>([&](auto tag) {
    constexpr int k = decltype(tag)::value;
    if ((sN & (C - 1)) == k) hi = a[k];
    if (((sN - 1) & (C - 1)) == k) lo = a[k];
  });
  hi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hi), sN >> strip_log2(C)));
  lo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lo), (sN - 1) >> strip_log2(C)));
}

}  // namespace eec

namespace eech {

// The head of an entry over lattice rows (`me`: its name): the argument, limit and workspace refusals, `required` the pointers
// that may not be null, `need` the entry's workspace size and `max_tokens` its limit on tok_stride.  Returns the entry's return code; 0 with n_hyp == 0 means there is
// nothing to launch.
inline int strip_entry_head(const char* me, std::initializer_list<const void*> required, int n_em, int Tq, int V, int n_hyp,
                            int tok_stride, int blank, const void* workspace, size_t workspace_bytes, size_t need,
                            int max_tokens = eec::kStripMaxTokens) {
  const std::string m = std::string(me) + ": ";
  if (n_hyp < 0 || Tq < 1 || tok_stride < 1 || n_em < 1 || V < 1 || blank < 0 || blank >= V)
    return fail(EEC_ERR_BAD_ARG, m + "needs n_hyp >= 0, Tq, tok_stride, n_em, V >= 1 and blank in [0, V)");
  if (n_hyp == 0) return 0;
  for (const void* p : required)
    if (!p) return fail(EEC_ERR_BAD_ARG, m + "null argument");
  if (V < 2 || tok_stride > max_tokens)
    return fail(EEC_ERR_UNSUPPORTED, m + "needs V >= 2 and tok_stride <= " + std::to_string(max_tokens));
  if (!workspace) return fail(EEC_ERR_WORKSPACE, m + "null workspace");
  return check_workspace(workspace, workspace_bytes, need);
}

}  // namespace eech
