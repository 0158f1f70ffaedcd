// Lexicon post-processing on the device: apply_lex (util/tokenizer.py:35-50), the step inference.py puts every printed
// hypothesis through.  A word that is not in the lexicon is replaced by the lexicon word with the smallest edit distance, the
// FIRST such word in file order (the reference scans with a strict <).  Here: for Q query words at once,
//   argmin_i levenshtein(query, lexicon[i]),  ties to the lowest original index,  as (index, distance) int32 pairs.
//
// Symbols are Unicode code points, mapped by the packer to byte codes 1..A (A <= 255, the lexicon's distinct code points in
// ascending order); a query symbol the lexicon never uses is code 0, which matches nothing.
//
// Algorithm: Myers / Hyyro bit-parallel edit distance, the query as the pattern (vertical), the lexicon word as the text.  A
// column of the DP table is two bit vectors of m bits (the +1 and -1 vertical differences); one text symbol advances it with
// ~17 integer operations and one lookup of the query's match mask Peq[symbol].  Information only moves towards higher bits
// (an addition's carry, two shifts), so a vector wider than the query needs no masking, and a vector of W 32-bit words is the
// same code with the three carries handed from word to word.  Three instantiations by query length: W = 1 (m <= 32, every
// operation one VALU instruction), W = 2 (m <= 64), W = 8 (m <= EEC_LEX_MAX_QUERY = 256).
//
// Work distribution: a workgroup of 256 work-items takes a tile of QT queries (W = 1: 4, or 8 from EEC_LEX_TILE_SWITCH queries
// on; W = 2: 4; W = 8: 1) and every `splits`-th chunk of EEC_LEX_BLOCK_WORDS = 256 lexicon words; a work-item owns one word
// of the chunk, loads its symbols once (a dword = 4 symbols, one group ahead of its use) and advances the QT columns of the
// tile side by side, so a (query, word) pair is one work-item's work and a word's symbols are read once per tile.  The tile's
// match masks are built once per workgroup in LDS, [query][code][W] with a fixed stride of 256 codes: lanes look up by text
// symbol, and the codes of a real lexicon (A = 27) fall on distinct banks.  The lexicon is sorted by length (stable), so the
// lanes of a wave run the same number of symbols; chunks are dealt round-robin, so every workgroup gets short and long words
// alike.  `splits` (lex_splits below) follows the query count: at Q = 1 the lexicon is split over one workgroup per chunk, with
// more queries a workgroup owns several chunks.
//
// Packed image (int32 units; written once by eec_lexicon_pack on the host, resident on the device: 1.6 MB for the 89 114 words of
// librispeech.lex, half of it symbols, inside one XCD's 4 MB L2):
//   header[16]: magic, n_words, max_len, n_groups = ceil(max_len / 4), A, info offset, gbase offset, sym offset, sym dwords,
//               total dwords, 0...
//   info [n_words][2]: (original index, length) of the word at sorted position s
//   gbase[n_groups]:   the dword of word s's symbols 4g .. 4g+3 is sym[gbase[g] + s].  Only the words longer than 4g have one;
//                      after the length sort they are a suffix of the order, so row g stores that suffix alone and gbase[g] =
//                      (start of row g) - (first sorted position with length > 4g).  Position-major: adjacent lanes read
//                      adjacent dwords.
//   sym:               the rows, symbol 4g+k in byte k, unused bytes 0
// Reduction: key = distance << 32 | original index, min.  In a wave on the DPP crossbar, across the four waves through LDS,
// across workgroups through a partials buffer [splits][Q] that a second kernel reduces with one wave per query -- integer
// min, so the result does not depend on any order, and the outputs are written with ordinary vector stores.  Lanes past the
// last word contribute the all-ones key and read nothing.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"

namespace eec {

typedef unsigned long long lex_key_t;

constexpr int kLexMagic = 0x4c434545;  // "EECL"
constexpr int kLexHeader = 16;
constexpr int kLexThreads = EEC_LEX_BLOCK_WORDS;
constexpr int kLexCodes = 256;         // stride of a query's match-mask table
// The grid (measured on the MI355X, tools/lexicon_time.py): a workgroup's fixed cost -- header, offsets,
// query bytes, the mask table: a chain of dependent loads -- is about that of two chunks, so with few queries a workgroup
// should own several chunks, while with many queries more, shorter workgroups even out the tail.
#ifndef EEC_LEX_TARGET_BLOCKS
#define EEC_LEX_TARGET_BLOCKS 4096  // workgroups asked for when there is work for them: 2 rounds of 8 x 256 CUs
#endif
#ifndef EEC_LEX_MIN_BLOCKS
#define EEC_LEX_MIN_BLOCKS 512      // ... and the count not to fall below for the sake of longer workgroups
#endif
#ifndef EEC_LEX_MIN_CHUNKS
#define EEC_LEX_MIN_CHUNKS 6        // chunks a workgroup should own if that leaves EEC_LEX_MIN_BLOCKS of them
#endif
// EEC_LEX_TILE_SWITCH (include/eec.h): the 32-bit kernel takes tiles of 8 queries from this many queries on, of 4 below
static_assert(kLexThreads == 256, "four waves per workgroup");

// queries per workgroup tile: the columns a work-item advances side by side (2 W + 1 registers each)
__host__ inline int lex_tile_queries(int W, int Q) { return W == 1 ? (Q >= EEC_LEX_TILE_SWITCH ? 8 : 4) : W == 2 ? 4 : 1; }
__host__ inline int lex_tiles(int Q, int qt) { return (Q + qt - 1) / qt; }
__host__ inline int lex_chunks(int n_words) { return (n_words + kLexThreads - 1) / kLexThreads; }
// lexicon shares: every workgroup of a tile owns `per` chunks (the last share may be short), dealt round-robin
__host__ inline int lex_splits(int Q, int n_words, int qt) {
  const long long units = (long long)lex_chunks(n_words) * lex_tiles(Q, qt);  // (tile, chunk) pairs
  long long per = std::max(1LL, (units + EEC_LEX_TARGET_BLOCKS - 1) / EEC_LEX_TARGET_BLOCKS);
  if (per < EEC_LEX_MIN_CHUNKS) per = std::max(per, std::min((long long)EEC_LEX_MIN_CHUNKS, units / EEC_LEX_MIN_BLOCKS));
  per = std::max(per, (long long)(lex_chunks(n_words) + 65534) / 65535);  // gridDim.y
  return (int)((lex_chunks(n_words) + per - 1) / per);
}

template <int CTRL, int RMASK>
__device__ __forceinline__ lex_key_t lex_dpp_min(lex_key_t v) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, RMASK, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, RMASK, 0xf, false);
  const lex_key_t o = (lex_key_t)ohi << 32 | olo;
  return o < v ? o : v;
}
// the wave's minimum, wave-uniform (the steps of wave_max, eec_device.h)
__device__ __forceinline__ lex_key_t lex_wave_min(lex_key_t v) {
  v = lex_dpp_min<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v = lex_dpp_min<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v = lex_dpp_min<0x141, 0xf>(v);  // row_half_mirror
  v = lex_dpp_min<0x140, 0xf>(v);  // row_mirror
  v = lex_dpp_min<0x142, 0xa>(v);  // row_bcast15 -> rows 1, 3
  v = lex_dpp_min<0x143, 0xc>(v);  // row_bcast31 -> rows 2, 3
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return (lex_key_t)hi << 32 | lo;
}

// One text symbol: the column (pv, mv: +1 / -1 vertical differences, bit i = row i + 1) moves one to the right; eq = the
// rows whose pattern symbol equals the text symbol.  The horizontal difference entering row 0 is +1 (global distance: the
// top row of the table counts the text), the score follows the horizontal difference of the pattern's last row.
template <int W>
__device__ __forceinline__ void lex_step(unsigned (&pv)[W], unsigned (&mv)[W], int& score, const unsigned (&eq)[W], int topw, unsigned topbit) {
  unsigned carry = 0, phc = 1, mhc = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const unsigned e = eq[w], p = pv[w], m = mv[w];
    const unsigned xv = e | m, a = e & p;
    const unsigned s1 = a + p, s = s1 + carry;
    carry = (unsigned)(s1 < a) | (unsigned)(s < s1);
    const unsigned xh = (s ^ p) | e;
    const unsigned ph = m | ~(xh | p), mh = p & xh;
    if (W == 1 || w == topw) score += (int)((ph & topbit) != 0) - (int)((mh & topbit) != 0);
    const unsigned phs = ph << 1 | phc, mhs = mh << 1 | mhc;
    phc = ph >> 31;
    mhc = mh >> 31;
    pv[w] = mhs | ~(xv | phs);
    mv[w] = phs & xv;
  }
}

template <int W, int QT>
__global__ __launch_bounds__(kLexThreads) void lexicon_nearest_kernel(const int* __restrict__ img, int n_words, const unsigned char* __restrict__ qsym,
                                                                      const int* __restrict__ qoff, int Q, int cap, int splits,
                                                                      lex_key_t* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) unsigned peq[QT * kLexCodes * W];
  __shared__ lex_key_t red[kLexThreads / 64][QT];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id_sgpr();
  const int tile = blockIdx.x, split = blockIdx.y;

  // an image that is not the one the caller described is not searched: every key stays all ones
  const int L = (img[0] == kLexMagic && img[1] == n_words) ? n_words : 0;
  const int A = min(max(img[4], 0), kLexCodes - 1);
  const int* info = img + img[5];
  const int* gbase = img + img[6];
  const unsigned* sym = (const unsigned*)img + img[7];

  const int nq = min(QT, Q - tile * QT);  // the last tile may be short: its unused columns are not advanced
  int m[QT], q0[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    const int qi = tile * QT + q;
    m[q] = 0, q0[q] = 0;
    if (qi < Q) {
      const int a = qoff[qi], b = qoff[qi + 1];
      if (a >= 0 && b >= a && b - a <= cap) m[q] = b - a, q0[q] = a;  // else: no symbol is read, the second kernel writes -1
    }
  }
  for (int i = tid; i < QT * (A + 1) * W; i += kLexThreads) peq[(i / ((A + 1) * W)) * kLexCodes * W + i % ((A + 1) * W)] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < QT; ++q)
    for (int j = tid; j < m[q]; j += kLexThreads) {
      const int c = qsym[(size_t)q0[q] + j];
      if (c >= 1 && c <= A) atomicOr(&peq[(q * kLexCodes + c) * W + (j >> 5)], 1u << (j & 31));
    }
  __syncthreads();

  lex_key_t best[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) best[q] = ~(lex_key_t)0;

  const int n_chunks = (L + kLexThreads - 1) / kLexThreads;
  for (int chunk = split; chunk < n_chunks; chunk += splits) {
    const int wave0 = chunk * kLexThreads + wave * 64;  // wave-uniform
    if (wave0 >= L) break;                              // this wave's lanes are all past the last word, here and in later chunks
    const int s = wave0 + lane;
    const bool valid = s < L;
    int orig = -1, len = 0;
    if (valid) {
      const int2 io = ((const int2*)info)[s];
      orig = io.x, len = io.y;
    }
    const int wlen = info[2 * min(wave0 + 63, L - 1) + 1];  // sorted by length: the wave's longest word is its last
    unsigned pv[QT][W], mv[QT][W];
    int score[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      score[q] = m[q];
#pragma unroll
      for (int w = 0; w < W; ++w) pv[q][w] = ~0u, mv[q][w] = 0;
    }
    unsigned next = 0;  // the word's next four symbols, loaded one group ahead of their use
    if (0 < len) next = sym[gbase[0] + s];
    for (int g = 0; 4 * g < wlen; ++g) {
      const unsigned d = next;
      if (4 * (g + 1) < wlen) {
        const int base = gbase[g + 1];
        if (4 * (g + 1) < len) next = sym[base + s];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (4 * g + k < len) {
          const int c = (d >> (8 * k)) & 255;
#pragma unroll
          for (int q = 0; q < QT; ++q) {
            if (q >= nq) break;  // wave-uniform
            unsigned eq[W];
#pragma unroll
            for (int w = 0; w < W; ++w) eq[w] = peq[(q * kLexCodes + c) * W + w];
            lex_step<W>(pv[q], mv[q], score[q], eq, (m[q] - 1) >> 5, m[q] ? 1u << ((m[q] - 1) & 31) : 0u);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const int dist = m[q] ? score[q] : len;
      const lex_key_t key = valid ? ((lex_key_t)(unsigned)dist << 32 | (unsigned)orig) : ~(lex_key_t)0;
      best[q] = key < best[q] ? key : best[q];
    }
  }

#pragma unroll
  for (int q = 0; q < QT; ++q) {
    const lex_key_t k = lex_wave_min(best[q]);
    if (lane == 0) red[wave][q] = k;
  }
  __syncthreads();
  if (tid < QT && tile * QT + tid < Q) {
    lex_key_t k = red[0][tid];
#pragma unroll
    for (int w = 1; w < kLexThreads / 64; ++w) k = red[w][tid] < k ? red[w][tid] : k;
    partial[(size_t)split * Q + tile * QT + tid] = k;
  }
}

// the partial minima of the `splits` lexicon shares -> (index, distance), one wave per query; a query the search refused
// (offsets out of order, longer than `cap`) and a search over an image that did not match give (-1, -1)
__global__ __launch_bounds__(256) void lexicon_finalize_kernel(const lex_key_t* __restrict__ partial, int splits, const int* __restrict__ qoff,
                                                               int Q, int cap, int* __restrict__ out_index, int* __restrict__ out_distance) {
  const int q = blockIdx.x * 4 + wave_id_sgpr(), lane = threadIdx.x & 63;
  if (q >= Q) return;
  const int a = qoff[q], b = qoff[q + 1];
  lex_key_t k = ~(lex_key_t)0;
  if (a >= 0 && b >= a && b - a <= cap)
    for (int s = lane; s < splits; s += 64) {
      const lex_key_t p = partial[(size_t)s * Q + q];
      k = p < k ? p : k;
    }
  k = lex_wave_min(k);
  if (lane == 0) {
    out_index[q] = (int)(unsigned)k;
    out_distance[q] = (int)(unsigned)(k >> 32);
  }
}

template <int W, int QT>
static hipError_t launch_lexicon_nearest(const int* img, int n_words, const unsigned char* qsym, const int* qoff, int Q, int cap, lex_key_t* partial,
                                         int* out_index, int* out_distance, hipStream_t st) {
  const int splits = lex_splits(Q, n_words, QT);
  hipLaunchKernelGGL((lexicon_nearest_kernel<W, QT>), dim3(lex_tiles(Q, QT), splits), dim3(kLexThreads), 0, st, img, n_words, qsym, qoff, Q, cap,
                     splits, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lexicon_finalize_kernel, dim3((Q + 3) / 4), dim3(256), 0, st, partial, splits, qoff, Q, cap, out_index, out_distance);
  return hipGetLastError();
}

static size_t lex_image_dwords(long long n_words, long long total_symbols, long long max_len) {
  const long long groups = (max_len + 3) / 4;
  const long long sym = std::min((total_symbols + 3 * n_words) / 4, n_words * groups);  // sum of ceil(len / 4) is at most either
  return (size_t)(kLexHeader + 2 * n_words + groups + sym + 3) & ~(size_t)3;
}

}  // namespace eec

extern "C" {

size_t eec_lexicon_pack_bytes(int n_words, int64_t total_symbols, int max_len) {
  if (n_words <= 0 || total_symbols < 0 || max_len < 0 || total_symbols > (int64_t)n_words * max_len) return 0;
  const size_t dwords = eec::lex_image_dwords(n_words, total_symbols, max_len);
  return dwords >= ((size_t)1 << 31) ? 0 : dwords * 4;  // the kernel indexes the image with int32
}

int eec_lexicon_pack(const uint32_t* symbols, const int64_t* offsets, int n_words, void* image, size_t image_bytes, int32_t* code_map,
                     int32_t* n_codes) {
  using namespace eec;
  using eech::fail;
  if (!offsets || !image || !code_map) return fail(EEC_ERR_BAD_ARG, "eec_lexicon_pack: null argument (offsets, image, code_map)");
  if (n_words <= 0) return fail(EEC_ERR_BAD_ARG, "eec_lexicon_pack: n_words must be positive");
  if (offsets[0] != 0) return fail(EEC_ERR_BAD_ARG, "eec_lexicon_pack: offsets[0] must be 0");
  int64_t max_len = 0;
  for (int i = 0; i < n_words; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(EEC_ERR_BAD_ARG, "eec_lexicon_pack: offsets must not decrease");
    max_len = std::max(max_len, offsets[i + 1] - offsets[i]);
  }
  const int64_t total = offsets[n_words];
  if (total > 0 && !symbols) return fail(EEC_ERR_BAD_ARG, "eec_lexicon_pack: null symbols");
  if (max_len > 0x7fffffff) return fail(EEC_ERR_UNSUPPORTED, "eec_lexicon_pack: a word longer than 2^31 - 1 symbols");
  const size_t need = eec_lexicon_pack_bytes(n_words, total, (int)max_len);
  if (need == 0) return fail(EEC_ERR_UNSUPPORTED, "eec_lexicon_pack: the image would pass 2^31 dwords");
  if (image_bytes < need) return fail(EEC_ERR_WORKSPACE, "eec_lexicon_pack: image_bytes below eec_lexicon_pack_bytes()");

  // the alphabet: distinct code points in ascending order -> codes 1..A
  std::vector<uint32_t> alpha(symbols, symbols + total);
  std::sort(alpha.begin(), alpha.end());
  alpha.erase(std::unique(alpha.begin(), alpha.end()), alpha.end());
  if (alpha.size() > 255) return fail(EEC_ERR_UNSUPPORTED, "eec_lexicon_pack: more than 255 distinct symbols");
  const int A = (int)alpha.size();
  for (int c = 0; c < 256; ++c) code_map[c] = (c >= 1 && c <= A) ? (int32_t)alpha[c - 1] : -1;
  if (n_codes) *n_codes = A;
  auto code_of = [&](uint32_t cp) { return (unsigned)(std::lower_bound(alpha.begin(), alpha.end(), cp) - alpha.begin()) + 1u; };

  std::vector<int> order(n_words);
  for (int i = 0; i < n_words; ++i) order[i] = i;
  auto len_of = [&](int i) { return (int)(offsets[i + 1] - offsets[i]); };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len_of(a) < len_of(b); });

  const int groups = (int)((max_len + 3) / 4);
  int32_t* img = (int32_t*)image;
  memset(img, 0, need);
  const int off_info = kLexHeader, off_gbase = off_info + 2 * n_words, off_sym = off_gbase + groups;
  for (int s = 0; s < n_words; ++s) {
    img[off_info + 2 * s] = order[s];
    img[off_info + 2 * s + 1] = len_of(order[s]);
  }
  int64_t row = 0;
  int first = 0;  // first sorted position with length > 4g
  for (int g = 0; g < groups; ++g) {
    while (first < n_words && len_of(order[first]) <= 4 * g) ++first;
    img[off_gbase + g] = (int32_t)(row - first);
    for (int s = first; s < n_words; ++s) {
      const int i = order[s], len = len_of(i);
      uint32_t d = 0;
      for (int k = 0; k < 4 && 4 * g + k < len; ++k) d |= code_of(symbols[offsets[i] + 4 * g + k]) << (8 * k);
      img[off_sym + row + (s - first)] = (int32_t)d;
    }
    row += n_words - first;
  }
  img[0] = kLexMagic, img[1] = n_words, img[2] = (int32_t)max_len, img[3] = groups, img[4] = A;
  img[5] = off_info, img[6] = off_gbase, img[7] = off_sym, img[8] = (int32_t)row, img[9] = (int32_t)(need / 4);
  return 0;
}

size_t eec_lexicon_nearest_workspace_bytes(int n_queries, int n_words) {
  using namespace eec;
  if (n_queries <= 0 || n_words <= 0) return 0;
  int splits = 1;  // whichever kernel the longest query selects
  for (int W : {1, 2, 8}) splits = std::max(splits, lex_splits(n_queries, n_words, lex_tile_queries(W, n_queries)));
  return (size_t)n_queries * splits * sizeof(lex_key_t);
}

int eec_lexicon_nearest(const void* packed, int n_words, const uint8_t* queries, const int32_t* query_offsets, int n_queries, int max_query_len,
                        int32_t* out_index, int32_t* out_distance, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace eec;
  using eech::fail;
  if (n_queries < 0 || n_words <= 0 || max_query_len < 0)
    return fail(EEC_ERR_BAD_ARG, "eec_lexicon_nearest: needs n_queries >= 0, n_words >= 1, max_query_len >= 0");
  if (max_query_len > EEC_LEX_MAX_QUERY) return fail(EEC_ERR_UNSUPPORTED, "eec_lexicon_nearest: max_query_len above EEC_LEX_MAX_QUERY");
  if (n_queries == 0) return 0;
  if (!packed || !queries || !query_offsets || !out_index || !out_distance || !workspace)
    return fail(EEC_ERR_BAD_ARG, "eec_lexicon_nearest: null argument");
  if (((uintptr_t)packed | (uintptr_t)workspace) & 7) return fail(EEC_ERR_BAD_ARG, "eec_lexicon_nearest: packed and workspace must be 8-byte aligned");
  if (workspace_bytes < eec_lexicon_nearest_workspace_bytes(n_queries, n_words))
    return fail(EEC_ERR_WORKSPACE, "eec_lexicon_nearest: workspace below eec_lexicon_nearest_workspace_bytes()");
  const int* img = (const int*)packed;
  lex_key_t* partial = (lex_key_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
#define EEC_LEX_LAUNCH(w, qt) \
  launch_lexicon_nearest<w, qt>(img, n_words, queries, query_offsets, n_queries, max_query_len, partial, out_index, out_distance, st)
  static_assert(EEC_LEX_MAX_QUERY == 8 * 32, "the widest kernel");
  hipError_t e = max_query_len > 64 ? EEC_LEX_LAUNCH(8, 1) : max_query_len > 32 ? EEC_LEX_LAUNCH(2, 4)
                 : lex_tile_queries(1, n_queries) == 8 ? EEC_LEX_LAUNCH(1, 8) : EEC_LEX_LAUNCH(1, 4);
#undef EEC_LEX_LAUNCH
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_lexicon_nearest launch");
}

}  // extern "C"
