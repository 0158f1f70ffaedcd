// What every host-side entry point of libeec.so shares (host code only): the calling thread's error string behind all
// eec_*_last_error() symbols, the return-on-error and deferred-error idioms, the bump allocator that lays buffers over a
// caller's workspace (or sizes them), and the argument checks that several families repeat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/eec.h"

namespace eec {
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, DEVICE): the attribute is per device, so a
// process-wide flag would leave the > 64 KiB launches of a second device failing.  Thread-safe.  (pack.hip)
hipError_t ensure_max_lds(const void* kernel, int bytes);
}  // namespace eec

namespace eech {

// One message per thread for the whole library: every non-zero return of an extern "C" entry leaves its reason here.
inline thread_local std::string g_err;
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
inline int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return (int)e;
}
// return from the enclosing entry point when a HIP call (or a launch wrapper) fails
#define EEC_HIP(expr)                                      \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return eech::hip_fail(_e, #expr); \
  } while (0)

// Deferred errors, for code that carves and launches in one pass and may run dry (sizes only): the first failing call is
// kept, later ones still run their carves, and finish() turns the outcome into the entry point's return code.
struct Deferred {
  bool dry = false;
  hipError_t err = hipSuccess;
  const char* where = "";
  void ok(hipError_t e, const char* w) {
    if (e != hipSuccess && err == hipSuccess) err = e, where = w;
  }
};
#define RUN(expr)                    \
  do {                               \
    if (!r.dry) r.ok((expr), #expr); \
  } while (0)
inline int finish(const Deferred& r, bool overflow) {
  if (overflow) return fail(EEC_ERR_WORKSPACE, "internal: workspace carve exceeded its size");
  if (r.err != hipSuccess) return hip_fail(r.err, r.where);
  return 0;
}

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// Bump allocator over one buffer, every take aligned to 256 bytes; base == nullptr: sizes only (takes return nullptr).
struct Bump {
  char* base = nullptr;
  size_t off = 0, peak = 0, cap = ~(size_t)0;
  bool overflow = false;  // a take went past cap: checked by the entry points before anything is reported as done
  template <typename T>
  T* take(size_t n) {
    off = up256(off);
    T* p = (T*)(base ? base + off : nullptr);
    off += n * sizeof(T);
    if (off > peak) peak = off;
    if (off > cap) overflow = true;
    return p;
  }
  float* f(size_t n) { return take<float>(n); }
  void reset(size_t to = 0) { off = to; }
};

inline int check_workspace(const void* ws, size_t have, size_t need) {
  if (((uintptr_t)ws & 255) != 0) return fail(EEC_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  if (have < need) return fail(EEC_ERR_WORKSPACE, "workspace too small");
  return 0;
}
inline int check_precision(int precision) {
  if (precision < EEC_PREC_F16X3 || precision > EEC_PREC_F16F8) return fail(EEC_ERR_BAD_ARG, "unknown precision");
  return 0;
}
inline int check_passes(int passes) {
  if (passes != 1 && passes != 3) return fail(EEC_ERR_BAD_ARG, "passes: 1 (bf16) or 3 (bf16x3)");
  return 0;
}

// The head of a step entry over one int32 state per beam, double-buffered [2, n, R_max] (eec_context_bias_step,
// eec_lm_fusion_step): the refusals under the entry's name `me` (`image_arg` names its image argument; `refused`: a refusal of
// the entry's own, or nullptr, reported after the range checks), then the half step s reads and the one it writes.  Returns the
// entry's return code; src stays nullptr where there is nothing to launch (a refusal, or n == 0).  `me` ends in "step", the
// name of its size function in "state_bytes".
struct StepHalves {
  int *src = nullptr, *dst = nullptr;
};
inline int step_head(const char* me, const char* image_arg, const char* refused, const void* image, int n, int R, int R_prev, int R_max,
                     int V, int s, const void* last, const void* local, const void* out, void* state, size_t state_bytes,
                     StepHalves* h) {
  const std::string m = std::string(me) + ": ";
  if (n < 0 || V < 1 || V > 256 || R_max < 1 || R_max > 16)
    return fail(EEC_ERR_BAD_ARG, m + "needs n >= 0, 1 <= V <= 256 and 1 <= R_max <= 16");
  if (R < 1 || R > R_max || s < 0 || (s > 0 && (R_prev < 1 || R_prev > R_max)))
    return fail(EEC_ERR_BAD_ARG, m + "1 <= R, R_prev <= R_max and s >= 0");
  if (refused) return fail(EEC_ERR_BAD_ARG, m + refused);
  if (n == 0) return 0;
  if ((long long)n * R > 0x7fffffffLL) return fail(EEC_ERR_UNSUPPORTED, m + "n * R must stay below 2^31");
  if (!local || !out || !state || (s > 0 && !last)) return fail(EEC_ERR_BAD_ARG, m + "null argument (local, out, state, last)");
  if (((uintptr_t)state & 3) != 0 || ((uintptr_t)image & 3) != 0)
    return fail(EEC_ERR_WORKSPACE, m + image_arg + " and state must be 4-byte aligned");
  const size_t half = (size_t)n * R_max;
  if (state_bytes < 2 * half * sizeof(int32_t))
    return fail(EEC_ERR_WORKSPACE, m + "state buffer too small (" + std::string(me, strlen(me) - 4) + "state_bytes)");
  h->src = (int*)state + (size_t)(s & 1) * half;
  h->dst = (int*)state + (size_t)((s + 1) & 1) * half;
  return 0;
}

}  // namespace eech
