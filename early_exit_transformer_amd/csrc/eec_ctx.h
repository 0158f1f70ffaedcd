// Contextual biasing (include/eec.h, "Contextual biasing"): how a kernel finds one graph's tables in a device image it does not
// trust.  Shared by the biased compile of ctc_beam.hip (ctc_beam_ctx.hip) and by the AED step kernel of ctx_graph.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/eec.h"

namespace eec {

struct CtxTables {
  const float* delta;  // [S][V]; nullptr: biasing is off for this sequence
  const int* next;     // [S][V]
  const float* fin;    // [S]
  int S;
};

// Graph graph_of[seq] (graph 0 without graph_of) of `image`, an array of `words` int32 words, or all-null when there is no image, the
// index is outside [0, G) or the header does not describe tables that lie inside the image.  Every work-item of a workgroup gets
// the same answer (the loads are uniform).
__device__ __forceinline__ CtxTables ctx_tables(const int* __restrict__ image, long long words, const int* __restrict__ graph_of, int seq, int V) {
  CtxTables off{nullptr, nullptr, nullptr, 1};
  if (!image || words < 4) return off;
  const long long G = image[1];
  if (image[0] != EEC_CTX_MAGIC || image[3] != V || G < 0 || G > EEC_CTX_MAX_GRAPHS || 4 + 4 * G > words) return off;
  const long long g = graph_of ? graph_of[seq] : 0;
  if (g < 0 || g >= G) return off;
  const int* rec = image + 4 + 4 * g;
  const long long S = rec[0], od = rec[1], on = rec[2], of = rec[3], SV = S * (long long)V, lo = 4 + 4 * G;
  if (S < 1 || S > EEC_CTX_MAX_STATES || od < lo || on < lo || of < lo || od + SV > words || on + SV > words || of + S > words) return off;
  return CtxTables{(const float*)(image + od), image + on, (const float*)(image + of), (int)S};
}

// a `next` entry as a state: anything outside [0, S) is the root
__device__ __forceinline__ int ctx_state(int s, int S) { return (unsigned)s < (unsigned)S ? s : 0; }

}  // namespace eec
