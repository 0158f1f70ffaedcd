// Contextual biasing (hot phrases): the host builder of the graph image and the step kernel of the AED lockstep searches.  The
// semantics -- trie, failure links, what a transition pays -- are stated in include/eec.h ("Contextual biasing");
// tests/ctxbias_cases.py is the plain-Python restatement.  The biased CTC prefix beam search is ctc_beam_ctx.hip.
//
// Builder (host only): per graph the trie of its phrases in insertion order (node ids are the order of creation), then one
// breadth-first pass that resolves the failure links into a dense next[S][V] / delta[S][V]: the device never follows a link.
// Step kernel: one workgroup per (search, beam) row, work-item v owns token v.  Every work-item derives the row's new state from
// uniform loads (parent, last token, the parent's state, one `next` entry); work-item 0 stores it; then one coalesced read of
// delta[state][.] and one add per element.  States are double-buffered: step s reads buffer s & 1 and writes the other one, so no
// workgroup reads what another one writes.  Vector stores only, no atomics, nothing read back.
#include <float.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/eec.h"
#include "eec_ctx.h"
#include "eec_host.h"

namespace eec {

__global__ __launch_bounds__(256) void context_bias_step_kernel(const int* __restrict__ image, long long words, const int* __restrict__ graph_of,
                                                                int R, int R_prev, int R_max, int V, int s,
                                                                const long long* __restrict__ parent, const long long* __restrict__ last,
                                                                const float* local, float* out, const int* __restrict__ src,
                                                                int* __restrict__ dst) {
  const int i = blockIdx.x / R, r = blockIdx.x % R, v = threadIdx.x;
  const CtxTables T = ctx_tables(image, words, graph_of, i, V);
  int st = 0;
  if (s > 0 && T.delta) {
    const long long pl = parent ? parent[(size_t)i * R + r] : (long long)r;
    const long long cl = last[(size_t)i * R + r];
    if (pl >= 0 && pl < R_prev && cl >= 0 && cl < V) {  // an index outside its range is never used as an address: back to the root
      const int ps = ctx_state(src[(size_t)i * R_max + pl], T.S);
      st = ctx_state(T.next[(size_t)ps * V + cl], T.S);
    }
  }
  if (v == 0) dst[(size_t)i * R_max + r] = st;
  if (v >= V) return;
  const size_t at = ((size_t)i * R + r) * V + v;
  const float x = local[at];
  out[at] = (T.delta && x != -INFINITY) ? x + T.delta[(size_t)st * V + v] : x;
}

// ---- the builder ----------------------------------------------------------------------------------------------------------------
struct CtxGraphArgs {
  int G;
  const int32_t *n_phrases, *phrase_len, *tokens;
  const double* boost;
  int V, blank, eos, pad;
};

// The image of `a` into `img` (sized here), or a refusal: its code, the message left behind eec_last_error().
static int ctx_build(const char* who, const CtxGraphArgs& a, std::vector<int32_t>& img) {
  using eech::fail;
  const std::string me(who);
  const int V = a.V;
  if (a.G < 1 || a.G > EEC_CTX_MAX_GRAPHS) return fail(EEC_ERR_BAD_ARG, me + ": 1 .. " + std::to_string(EEC_CTX_MAX_GRAPHS) + " graphs");
  if (V < 1 || V > 256 || a.blank < 0 || a.blank >= V) return fail(EEC_ERR_BAD_ARG, me + ": needs 1 <= V <= 256 and blank in [0, V)");
  if (a.eos < -1 || a.eos >= V || a.pad < -1 || a.pad >= V || a.eos == a.blank || a.pad == a.blank)
    return fail(EEC_ERR_BAD_ARG, me + ": eos and pad are -1 (none) or tokens of [0, V) other than blank");
  if (!a.n_phrases) return fail(EEC_ERR_BAD_ARG, me + ": null argument (n_phrases)");
  long long P = 0;
  for (int g = 0; g < a.G; ++g) {
    if (a.n_phrases[g] < 0) return fail(EEC_ERR_BAD_ARG, me + ": a negative phrase count");
    P += a.n_phrases[g];
  }
  if (P > 0 && (!a.phrase_len || !a.tokens || !a.boost)) return fail(EEC_ERR_BAD_ARG, me + ": null argument (phrase_len, tokens, boost)");
  long long n_tok = 0;
  for (long long p = 0; p < P; ++p) {
    const int L = a.phrase_len[p];
    if (L < 1) return fail(EEC_ERR_BAD_ARG, me + ": an empty phrase");
    if (L > EEC_CTX_MAX_PHRASE) return fail(EEC_ERR_BAD_ARG, me + ": a phrase of more than " + std::to_string(EEC_CTX_MAX_PHRASE) + " tokens");
    if (!(a.boost[p] >= 0.0) || !(a.boost[p] <= (double)FLT_MAX))
      return fail(EEC_ERR_BAD_ARG, me + ": a boost must be finite and >= 0");
    for (int k = 0; k < L; ++k) {
      const int t = a.tokens[n_tok + k];
      if (t < 0 || t >= V) return fail(EEC_ERR_BAD_ARG, me + ": a token outside [0, V)");
      if (t == a.blank) return fail(EEC_ERR_BAD_ARG, me + ": blank inside a phrase");
      if (t == a.eos || t == a.pad) return fail(EEC_ERR_BAD_ARG, me + ": eos or pad inside a phrase");
    }
    n_tok += L;
  }
  const bool closing = a.eos >= 0 || a.pad >= 0;  // one more state, the dead one, behind the trie's

  img.assign(4 + 4 * (size_t)a.G, 0);
  long long states = 0;
  size_t p0 = 0, t0 = 0;
  std::vector<int> go, fail_, order;
  std::vector<double> tscore, nscore, out;
  std::vector<char> endf;
  for (int g = 0; g < a.G; ++g) {
    // the trie, node ids in the order of creation
    go.assign(V, -1);
    tscore.assign(1, 0.0);
    endf.assign(1, 0);
    for (int p = 0; p < a.n_phrases[g]; ++p) {
      int n = 0;
      const int L = a.phrase_len[p0 + p];
      const double b = a.boost[p0 + p];
      for (int k = 0; k < L; ++k) {
        const int t = a.tokens[t0 + k];
        if (go[(size_t)n * V + t] < 0) {
          if (states + (long long)tscore.size() + (closing ? 2 : 1) > EEC_CTX_MAX_STATES)
            return fail(EEC_ERR_BAD_ARG, me + ": more than " + std::to_string(EEC_CTX_MAX_STATES) + " states over all graphs");
          go[(size_t)n * V + t] = (int)tscore.size();
          go.insert(go.end(), V, -1);
          tscore.push_back(0.0);
          endf.push_back(0);
        }
        n = go[(size_t)n * V + t];
        if (b > tscore[n]) tscore[n] = b;
      }
      endf[n] = 1;
      t0 += L;
    }
    p0 += a.n_phrases[g];
    const int N = (int)tscore.size(), S = N + (closing ? 1 : 0);
    states += S;
    if (states > EEC_CTX_MAX_STATES) return fail(EEC_ERR_BAD_ARG, me + ": more than " + std::to_string(EEC_CTX_MAX_STATES) + " states over all graphs");
    // breadth first: scores, failure links, the sum over the end nodes of a failure chain, and goto completed in place
    nscore.assign(N, 0.0);
    out.assign(N, 0.0);
    fail_.assign(N, 0);
    order.assign(1, 0);
    for (size_t q = 0; q < order.size(); ++q) {
      const int n = order[q];
      for (int t = 0; t < V; ++t) {
        const int c = go[(size_t)n * V + t];
        const int via = n == 0 ? 0 : go[(size_t)fail_[n] * V + t];
        if (c < 0) {
          go[(size_t)n * V + t] = via;
          continue;
        }
        fail_[c] = via;
        nscore[c] = nscore[n] + tscore[c];
        if (!(nscore[c] <= (double)FLT_MAX)) return fail(EEC_ERR_BAD_ARG, me + ": the boosts of a phrase add up beyond the fp32 range");
        out[c] = (endf[c] ? nscore[c] : 0.0) + out[via];
        order.push_back(c);
      }
    }
    const size_t od = img.size(), on = od + (size_t)S * V, of = on + (size_t)S * V;
    img.resize(of + S, 0);
    int32_t* rec = img.data() + 4 + 4 * (size_t)g;
    rec[0] = S, rec[1] = (int32_t)od, rec[2] = (int32_t)on, rec[3] = (int32_t)of;
    float* delta = (float*)(img.data() + od);
    int32_t* next = img.data() + on;
    float* fin = (float*)(img.data() + of);
    for (int s = 0; s < N; ++s) {
      for (int t = 0; t < V; ++t) {
        const size_t at = (size_t)s * V + t;
        if (t == a.blank) {
          next[at] = s, delta[at] = 0.0f;
        } else if (t == a.eos || t == a.pad) {
          next[at] = N, delta[at] = (float)(0.0 - nscore[s]);
        } else {
          const int d = go[at];
          next[at] = d, delta[at] = (float)((nscore[d] - nscore[s]) + out[d]);
        }
      }
      fin[s] = (float)(0.0 - nscore[s]);
    }
    if (closing) {
      for (int t = 0; t < V; ++t) next[(size_t)N * V + t] = N, delta[(size_t)N * V + t] = 0.0f;
      fin[N] = 0.0f;
    }
  }
  img[0] = EEC_CTX_MAGIC, img[1] = a.G, img[2] = (int32_t)img.size(), img[3] = V;
  return 0;
}

}  // namespace eec

extern "C" {

size_t eec_context_graph_bytes(int G, const int32_t* n_phrases, const int32_t* phrase_len, const int32_t* tokens, const double* boost, int V,
                               int blank, int eos, int pad) {
  std::vector<int32_t> img;
  if (eec::ctx_build("eec_context_graph_bytes", eec::CtxGraphArgs{G, n_phrases, phrase_len, tokens, boost, V, blank, eos, pad}, img)) return 0;
  return img.size() * sizeof(int32_t);
}

int eec_context_graph(int G, const int32_t* n_phrases, const int32_t* phrase_len, const int32_t* tokens, const double* boost, int V, int blank,
                      int eos, int pad, void* image, size_t image_bytes) {
  std::vector<int32_t> img;
  if (int rc = eec::ctx_build("eec_context_graph", eec::CtxGraphArgs{G, n_phrases, phrase_len, tokens, boost, V, blank, eos, pad}, img)) return rc;
  if (!image) return eech::fail(EEC_ERR_BAD_ARG, "eec_context_graph: null argument (image)");
  if (image_bytes < img.size() * sizeof(int32_t)) return eech::fail(EEC_ERR_WORKSPACE, "eec_context_graph: image too small (eec_context_graph_bytes)");
  memcpy(image, img.data(), img.size() * sizeof(int32_t));
  return 0;
}

size_t eec_context_bias_state_bytes(int n, int R_max) {
  return n > 0 && R_max > 0 ? 2 * (size_t)n * R_max * sizeof(int32_t) : 0;
}

int eec_context_bias_step(const void* image, size_t image_bytes, const int32_t* graph_of, int n, int R, int R_prev, int R_max, int V, int s,
                          const int64_t* parent, const int64_t* last, const float* local, float* out, void* state, size_t state_bytes,
                          void* stream) {
  eech::StepHalves h;
  const int rc = eech::step_head("eec_context_bias_step", "image", nullptr, image, n, R, R_prev, R_max, V, s, last, local, out, state, state_bytes, &h);
  if (rc != 0 || !h.src) return rc;
  hipLaunchKernelGGL(eec::context_bias_step_kernel, dim3(n * R), dim3((V + 63) / 64 * 64), 0, (hipStream_t)stream, (const int*)image,
                     (long long)(image_bytes / 4), graph_of, R, R_prev, R_max, V, s, (const long long*)parent, (const long long*)last, local, out,
                     h.src, h.dst);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : eech::hip_fail(e, "eec_context_bias_step launch");
}

}  // extern "C"
