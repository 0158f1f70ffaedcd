// What the two step-wise AED decoders share (decoder_step.hip: the exits of one utterance; decoder_batch.hip: every exit and
// utterance of a padded batch): the cache layout, the argument checks of their entry points and the log-softmax of a
// row.  Their embed, attention and linear kernels differ by design and stay in their own files.
#pragma once
#include <algorithm>
#include <string>

#include "../../include/eec.h"
#include "eec_host.h"
#include "eec_train.h"
#include "eec_wave.h"

namespace eecs {

constexpr int kRows = 16;  // live beams per search and step (rows of every activation of a step)
constexpr int kGroup = 8;  // decoders (exits) per call: their pointers travel in the kernel arguments

// out[0 .. V) = log_softmax(xr[0 .. V)), by one wave
__device__ __forceinline__ void log_softmax_row(const float* xr, float* out, int V, int lane) {
  float mx = -INFINITY;
  for (int k = lane; k < V; k += 64) mx = fmaxf(mx, xr[k]);
  mx = eec::wave_all_max(mx);
  float sum = 0.0f;
  for (int k = lane; k < V; k += 64) sum += expf(xr[k] - mx);
  const float lse = mx + logf(eec::wave_all_sum(sum));
  for (int k = lane; k < V; k += 64) out[k] = xr[k] - lse;
}

// ---------------------------------------------------------------------------------------------------------------------
using eech::fail;

// E exits x B utterances in one cache: the per-utterance path has E = B = 1 per cache
struct Geo {
  int D, H, F, V, L, S_max, Tq, E, B;
};
struct Step {
  int R, R_prev, s;
};

// One caller-owned buffer, u = e * B + b is the (exit, utterance) index:
//   mem [E][L][B][Tq][2D]        memory keys | values, projected once by _begin
//   kv  [E*B][L][S_max][16][2D]  self-attention keys | values of every (position, beam slot)
//   anc [E*B][2][16][S_max]      each beam's ancestry slots (double-buffered by step parity); pad [E*B][S_max][16]
//   activations [E][B*16][...]   rows of exit e at e * B * R + b * R + r (dense for the step's R)
struct Cache {
  float *mem, *kv, *x, *qkv, *q, *ctx, *h, *logits;
  int* anc;
  unsigned char* pad;
  size_t bytes;
};
inline Cache carve(char* base, const Geo& g) {
  eech::Bump a;
  a.base = base;
  Cache c{};
  const size_t U = (size_t)g.E * g.B, rows = U * kRows;
  c.mem = a.f(U * g.L * g.Tq * 2 * g.D);
  c.kv = a.f(U * g.L * g.S_max * kRows * 2 * g.D);
  c.x = a.f(rows * g.D);
  c.qkv = a.f(rows * 3 * g.D);
  c.q = a.f(rows * g.D);
  c.ctx = a.f(rows * g.D);
  c.h = a.f(rows * g.F);
  c.logits = a.f(rows * g.V);
  c.anc = a.take<int>(U * 2 * kRows * g.S_max);
  c.pad = a.take<unsigned char>(U * g.S_max * kRows);
  c.bytes = a.off + 256;
  return c;
}

inline bool geometry_ok(const Geo& g) {
  if (g.D <= 0 || g.H <= 0 || g.D % g.H || g.F <= 0 || g.V <= 0 || g.L <= 0 || g.S_max <= 0 || g.Tq <= 0) return false;
  const int dh = g.D / g.H;
  if (dh != 8 && dh != 16 && dh != 32 && dh != 64) return false;  // a head's features on a power-of-two fraction of a wave
  if (g.D % 4 || g.F % 4) return false;                             // float4 weight rows
  if (g.D > 1024 || g.F > 2048) return false;                       // LayerNorm rows in registers; 16 rows of d_ff in LDS (128 KB)
  if ((size_t)std::max(g.S_max, g.Tq) * 8 > 60000) return false;    // scores + slots of one query row in LDS
  return g.E > 0 && g.E <= kGroup && g.B > 0 && (long)g.E * g.B <= 65535;  // E * B within a grid's y extent
}

// The argument checks of the four begin / step entry points, before any HIP call: ``ptrs`` says that the caller's own
// pointers are there, ``ps`` are the n decoders of the call (g.L comes from them), ``step`` is null for a begin; then the
// ``n_caches`` caches, each of ``cache_bytes``, are carved into c[].  0, or the code of the error left in g_err.
inline int check_call(bool ptrs, const eec_decoder_params* const* ps, int n, Geo& g, const Step* step, void* const* caches, int n_caches,
                      size_t cache_bytes, Cache* c) {
  if (!ptrs || !ps || !caches) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (n <= 0 || n > kGroup) return fail(EEC_ERR_BAD_ARG, "1 .. 8 decoders (exits, sessions) per call");
  for (int i = 0; i < n; ++i) {
    if (!ps[i] || !ps[i]->layers) return fail(EEC_ERR_BAD_ARG, "null argument");
    if (ps[i]->n_layers != ps[0]->n_layers) return fail(EEC_ERR_BAD_ARG, "the decoders of a call share one geometry");
    if (g.S_max > ps[i]->max_len) return fail(EEC_ERR_UNSUPPORTED, "S_max beyond the positional-encoding table");
  }
  g.L = ps[0]->n_layers;
  if (!geometry_ok(g)) return fail(EEC_ERR_UNSUPPORTED, "geometry not served by the step-wise decoder (use eec_decoder_forward)");
  if (step) {
    if (step->R <= 0 || step->R > kRows) return fail(EEC_ERR_BAD_ARG, "1 .. 16 live beams per search and step");
    if (step->s < 0 || step->s >= g.S_max) return fail(EEC_ERR_BAD_ARG, "step index outside the cache (S_max)");
    if (step->s > 0 && (step->R_prev <= 0 || step->R_prev > kRows)) return fail(EEC_ERR_BAD_ARG, "R_prev: the previous step's beam count");
  }
  for (int i = 0; i < n_caches; ++i) {
    if (!caches[i]) return fail(EEC_ERR_BAD_ARG, "null argument");
    c[i] = carve((char*)caches[i], g);
    if (c[i].bytes > cache_bytes) return fail(EEC_ERR_WORKSPACE, "cache too small");
  }
  return 0;
}

}  // namespace eecs
