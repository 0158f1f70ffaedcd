// Error-rate scoring on the device: the edit distance of many (hypothesis, reference) pairs of int32 token rows at once, with the
// substitution / deletion / insertion split and, on request, the alignment as an op string.  The statement is in include/eec.h
// ("Edit distance"): unit costs, a packed key K = distance << 16 | substitutions under min, so among all minimum-cost alignments the
// one with the fewest substitutions is counted, and dir = the FIRST of (diag, del, ins) that attains K.
//
// Work distribution: one wave per pair, four pairs per workgroup.  The table's columns (hypothesis tokens) are dealt over the lanes
// in strips of S = 4, 8 or 16 columns -- the entry picks S from hyp_pitch (<= 256, <= 512, above), so 64 lanes always cover the
// pitch --; a lane keeps the K values of its strip and the strip's tokens in registers.  The rows (reference tokens) run as a
// systolic wavefront: at step t lane l works on row t - l + 1, one step behind lane l - 1, whose last column of that row it
// receives by a one-lane shift (__shfl_up: one ds_bpermute per step).  The value received one step earlier is the diagonal
// neighbour.  A pair of m x n tokens takes m + ceil(n / S) - 1 steps; lanes whose strip starts past n idle.  The reference row is
// staged once in LDS (4 KiB per wave), where lane l reads token t - l: consecutive addresses, no bank conflict.  Nothing is
// reduced, nothing is atomic: lane (n - 1) / S holds K[m][n] at the end and lane 0 writes the four counts with one vector store.
//
// Op strings: the same kernel, instantiated with OPS, also writes the op code of every cell -- two bits: 0 diag on equal tokens,
// 1 diag on different ones, 2 del, 3 ins, i.e. the op code itself -- into the workspace: a row of the table is ceil(hyp_pitch /
// 16) dwords, the 2 S bits of a lane's strip are S / 4 bytes at byte l * S / 4 (one byte, short or dword store per lane and row).
// A second kernel walks back from (m, n) with one work-item per pair.  The length of the op string is known before the walk
// (n + dels), so the ops are written back to front into their final places and no byte past n_ops is touched.
#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_kernels.h"

namespace eec {

constexpr int kEditWaves = 4;  // pairs per workgroup
constexpr unsigned kEditStep = 1u << 16;         // one deletion or insertion
constexpr unsigned kEditSub = (1u << 16) + 1u;   // one substitution: a unit of cost, and one in the tie-break field

__host__ __device__ inline int edit_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// strip width for a hypothesis pitch: 64 strips cover EEC_EDIT_MAX_LEN at 16
__host__ inline int edit_strip(int hyp_pitch) { return hyp_pitch <= 256 ? 4 : hyp_pitch <= 512 ? 8 : 16; }
// bytes of one table row of op codes: two bits per column, whole dwords
__host__ __device__ inline size_t edit_row_bytes(int hyp_pitch) { return (size_t)((hyp_pitch + 15) / 16) * 4; }

// the reference of pair p, or -1 (then nothing of the pair is read)
__device__ __forceinline__ int edit_ref_index(const int* __restrict__ ref_of, int p, int n_refs) {
  const int r = ref_of ? ref_of[p] : p;
  return (r >= 0 && r < n_refs) ? r : -1;
}

template <int S, bool OPS>
__global__ __launch_bounds__(kEditWaves * 64) void edit_distance_kernel(const int* __restrict__ hyp, const int* __restrict__ hyp_len, int n_pairs,
                                                                        int hyp_pitch, const int* __restrict__ ref, const int* __restrict__ ref_len,
                                                                        int n_refs, int ref_pitch, const int* __restrict__ ref_of,
                                                                        int* __restrict__ counts, int* __restrict__ n_ops,
                                                                        unsigned char* __restrict__ dirs) {
  __shared__ int sref[kEditWaves][EEC_EDIT_MAX_LEN];
  const int lane = threadIdx.x & 63, wave = wave_id_sgpr();
  const int p = blockIdx.x * kEditWaves + wave;  // wave-uniform
  int ridx = -1, m = 0, n = 0;
  if (p < n_pairs) {
    ridx = edit_ref_index(ref_of, p, n_refs);
    if (ridx >= 0) {
      m = edit_clamp(ref_len[ridx], ref_pitch);
      n = edit_clamp(hyp_len[p], hyp_pitch);
    }
  }
  ridx = __builtin_amdgcn_readfirstlane(ridx), m = __builtin_amdgcn_readfirstlane(m), n = __builtin_amdgcn_readfirstlane(n);
  for (int k = lane; k < m; k += 64) sref[wave][k] = ref[(size_t)ridx * ref_pitch + k];
  __syncthreads();
  if (p >= n_pairs) return;
  if (ridx < 0) {
    if (lane == 0) {
      ((int4*)counts)[p] = make_int4(-1, -1, -1, -1);
      if (OPS) n_ops[p] = 0;
    }
    return;
  }

  // the strip: columns j = lane * S + c + 1, row 0 of the table; tokens past n are not read (their columns feed nothing that is)
  unsigned K[S];
  int h[S];
#pragma unroll
  for (int c = 0; c < S; ++c) {
    const int j0 = lane * S + c;
    K[c] = (unsigned)(j0 + 1) << 16;
    h[c] = j0 < n ? hyp[(size_t)p * hyp_pitch + j0] : 0;
  }
  const int L = (n + S - 1) / S;  // lanes with a column of the pair
  unsigned klast = K[S - 1];      // K[row this lane did last][last column of the strip]
  unsigned left_prev = (unsigned)(lane * S) << 16;  // K[row - 1][column left of the strip]
  const int steps = (m > 0 && L > 0) ? m + L - 1 : 0;
  unsigned char* dir_row = OPS ? dirs + (size_t)p * ref_pitch * edit_row_bytes(hyp_pitch) + (size_t)lane * (S / 4) : nullptr;
  for (int t = 0; t < steps; ++t) {
    const int i = t - lane + 1;  // this lane's row, 1-based
    const unsigned recv = (unsigned)__shfl_up((int)klast, 1, 64);
    if (lane < L && i >= 1 && i <= m) {
      const unsigned left = lane == 0 ? (unsigned)i << 16 : recv;
      const int rt = sref[wave][i - 1];
      unsigned diag = left_prev, lft = left, bits = 0;
#pragma unroll
      for (int c = 0; c < S; ++c) {
        const unsigned up = K[c];
        const bool eq = rt == h[c];
        const unsigned cd = diag + (eq ? 0u : kEditSub), cu = up + kEditStep, cl = lft + kEditStep;
        const unsigned v = min(cd, min(cu, cl));
        if (OPS) bits |= (v == cd ? (eq ? 0u : 1u) : v == cu ? 2u : 3u) << (2 * c);
        diag = up, lft = v, K[c] = v;
      }
      left_prev = left;
      klast = lft;
      if (OPS) {
        unsigned char* at = dir_row + (size_t)(i - 1) * edit_row_bytes(hyp_pitch);
        if (S == 4) *at = (unsigned char)bits;
        else if (S == 8) *(unsigned short*)at = (unsigned short)bits;
        else *(unsigned*)at = bits;
      }
    }
  }

  // K[m][n]: column n of lane (n - 1) / S; without hypothesis tokens the left border, m << 16
  const int cn = n > 0 ? (n - 1) % S : 0;
  unsigned kend = K[0];
#pragma unroll
  for (int c = 1; c < S; ++c) kend = c == cn ? K[c] : kend;
  kend = (unsigned)__shfl((int)kend, n > 0 ? (n - 1) / S : 0, 64);
  if (n == 0) kend = (unsigned)m << 16;
  if (lane == 0) {
    const int dist = (int)(kend >> 16), subs = (int)(kend & 0xffffu);
    const int dels = (dist - subs - (n - m)) / 2, ins = dels + n - m;
    ((int4*)counts)[p] = make_int4(dist, subs, dels, ins);
    if (OPS) n_ops[p] = n + dels;
  }
}

// the walk back from (m, n) over the op codes the kernel above left: one work-item per pair, ops written back to front
__global__ __launch_bounds__(64) void edit_traceback_kernel(const int* __restrict__ hyp_len, int n_pairs, int hyp_pitch, const int* __restrict__ ref_len,
                                                            int n_refs, int ref_pitch, const int* __restrict__ ref_of, const int* __restrict__ counts,
                                                            const unsigned char* __restrict__ dirs, unsigned char* __restrict__ ops) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_pairs) return;
  const int ridx = edit_ref_index(ref_of, p, n_refs);
  if (ridx < 0) return;
  int i = edit_clamp(ref_len[ridx], ref_pitch), j = edit_clamp(hyp_len[p], hyp_pitch);
  const size_t row = edit_row_bytes(hyp_pitch);
  const unsigned char* d = dirs + (size_t)p * ref_pitch * row;
  unsigned char* out = ops + (size_t)p * ((size_t)ref_pitch + hyp_pitch);
  int pos = min(j + counts[4 * p + 2], i + j);  // n + dels: every hypothesis token and every deleted reference token is one op
  while ((i > 0 || j > 0) && pos > 0) {
    const int code = i == 0 ? 3 : j == 0 ? 2 : (d[(size_t)(i - 1) * row + ((j - 1) >> 2)] >> (2 * ((j - 1) & 3))) & 3;
    out[--pos] = (unsigned char)code;
    i -= code != 3;
    j -= code != 2;
  }
}

template <int S>
static hipError_t launch_edit(bool want_ops, const int* hyp, const int* hyp_len, int n_pairs, int hyp_pitch, const int* ref, const int* ref_len,
                              int n_refs, int ref_pitch, const int* ref_of, int* counts, unsigned char* ops, int* n_ops, unsigned char* dirs,
                              hipStream_t st) {
  const dim3 grid((n_pairs + kEditWaves - 1) / kEditWaves), block(kEditWaves * 64);
  if (!want_ops) {
    hipLaunchKernelGGL((edit_distance_kernel<S, false>), grid, block, 0, st, hyp, hyp_len, n_pairs, hyp_pitch, ref, ref_len, n_refs, ref_pitch, ref_of,
                       counts, n_ops, dirs);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((edit_distance_kernel<S, true>), grid, block, 0, st, hyp, hyp_len, n_pairs, hyp_pitch, ref, ref_len, n_refs, ref_pitch, ref_of,
                     counts, n_ops, dirs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(edit_traceback_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, hyp_len, n_pairs, hyp_pitch, ref_len, n_refs, ref_pitch, ref_of,
                     counts, dirs, ops);
  return hipGetLastError();
}

}  // namespace eec

extern "C" {

size_t eec_edit_distance_workspace_bytes(int n_pairs, int max_ref_len, int max_hyp_len, int want_ops) {
  if (n_pairs <= 0 || max_ref_len <= 0 || max_hyp_len <= 0 || want_ops <= 0) return 0;
  return (size_t)n_pairs * (size_t)max_ref_len * eec::edit_row_bytes(max_hyp_len);
}

int eec_edit_distance(const int32_t* hyp, const int32_t* hyp_len, int n_pairs, int hyp_pitch, const int32_t* ref, const int32_t* ref_len, int n_refs,
                      int ref_pitch, const int32_t* ref_of, int32_t* counts, uint8_t* ops, int32_t* n_ops, void* workspace, size_t workspace_bytes,
                      void* stream) {
  using namespace eec;
  using eech::fail;
  if (n_pairs < 0) return fail(EEC_ERR_BAD_ARG, "edit distance: n_pairs must not be negative, got " + std::to_string(n_pairs));
  if (hyp_pitch < 0 || hyp_pitch > EEC_EDIT_MAX_LEN || ref_pitch < 0 || ref_pitch > EEC_EDIT_MAX_LEN)
    return fail(EEC_ERR_BAD_ARG, "edit distance: pitches must lie in [0, EEC_EDIT_MAX_LEN = " + std::to_string(EEC_EDIT_MAX_LEN) + "], got hyp_pitch " +
                                     std::to_string(hyp_pitch) + ", ref_pitch " + std::to_string(ref_pitch));
  if (n_pairs == 0) return 0;
  if (n_refs < 1) return fail(EEC_ERR_BAD_ARG, "edit distance: n_refs must be positive, got " + std::to_string(n_refs));
  if (!ref_of && n_refs != n_pairs)
    return fail(EEC_ERR_BAD_ARG, "edit distance: without ref_of pair p scores against reference p, so n_refs must equal n_pairs");
  if (!hyp_len || !ref_len || !counts || (!hyp && hyp_pitch > 0) || (!ref && ref_pitch > 0))
    return fail(EEC_ERR_BAD_ARG, "edit distance: null argument (hyp, hyp_len, ref, ref_len, counts)");
  if ((uintptr_t)counts & 15) return fail(EEC_ERR_BAD_ARG, "edit distance: counts must be 16-byte aligned (one vector store per pair)");
  if (ops && !n_ops) return fail(EEC_ERR_BAD_ARG, "edit distance: ops without n_ops");
  const bool want_ops = ops != nullptr;
  const size_t need = eec_edit_distance_workspace_bytes(n_pairs, ref_pitch, hyp_pitch, want_ops);
  if (need > 0) {
    if (!workspace) return fail(EEC_ERR_BAD_ARG, "edit distance: null workspace");
    if (eech::check_workspace(workspace, workspace_bytes, need) != 0)
      return fail(EEC_ERR_WORKSPACE, "edit distance: " + eech::g_err + " (eec_edit_distance_workspace_bytes)");
  }
  hipStream_t st = (hipStream_t)stream;
#define EEC_EDIT_LAUNCH(s) \
  launch_edit<s>(want_ops, hyp, hyp_len, n_pairs, hyp_pitch, ref, ref_len, n_refs, ref_pitch, ref_of, counts, ops, n_ops, (unsigned char*)workspace, st)
  const int S = edit_strip(hyp_pitch);
  static_assert(EEC_EDIT_MAX_LEN == 64 * 16, "the widest strip");
  const hipError_t e = S == 4 ? EEC_EDIT_LAUNCH(4) : S == 8 ? EEC_EDIT_LAUNCH(8) : EEC_EDIT_LAUNCH(16);
#undef EEC_EDIT_LAUNCH
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_edit_distance launch");
}

}  // extern "C"
