// C-ABI of libeec.so (include/eec.h): parameter packing, workspace carving and the
// launch plan of one encoder forward.  Host code only; kernels live in the other .hip files.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/eec.h"
#include <cstdlib>
#include <cstring>

#include "eec_host.h"
#include "eec_kernels.h"

using namespace eec;
using namespace eech;

namespace {

struct PackedLayer {
  // device pointers into the encoder's arena
  float *ffn1_ln_w, *ffn1_ln_b, *ffn1_b1, *ffn1_b2;
  uint4 *ffn1_w1p, *ffn1_w2p, *ffn1_w1f8, *ffn1_w2f8;
  float *attn_ln_w, *attn_ln_b, *attn_in_b, *attn_out_b;
  uint4 *attn_in_p, *attn_out_p, *attn_in_f8, *attn_out_f8;
  float *conv_ln_w, *conv_ln_b, *conv_pw1_b, *conv_pw2_b, *dw_wfold, *dw_bfold;
  uint4 *conv_pw1_p, *conv_pw2_p, *conv_pw1_f8, *conv_pw2_f8;
  float *ffn2_ln_w, *ffn2_ln_b, *ffn2_b1, *ffn2_b2;
  uint4 *ffn2_w1p, *ffn2_w2p, *ffn2_w1f8, *ffn2_w2f8;
  float *final_ln_w, *final_ln_b;
};

size_t frag_u4(int N, int K) { return (size_t)((N + 31) / 32) * (K / 16) * 128; }
size_t f8_u4(int N, int K) { return (size_t)((N + 31) / 32) * ((K + 63) / 64) * kF8Rec; }

// The packed tensors of one layer, in arena order: where each comes from in eec_layer_params, where it goes in PackedLayer,
// its extent as a function of (D, F), what packing makes it and with which scale.  eec_encoder::carve() sizes the arena
// from this table and eec_encoder_pack fills it from the same rows.
// Kinds: fp32 copy; fp32 copy times scale; MFMA fragment image of a [rows][cols] weight (fp16 hi / lo pairs); its f8 image; the
// same for a feed-forward weight (made only when F % 128 == 0); made by the depthwise / BatchNorm fold from several sources.
enum PackKind { PK_COPY, PK_SCALE, PK_FRAG, PK_F8, PK_F8_FFN, PK_FOLD };
struct Ext {  // d * D + f * F + c
  int d, f, c;
  int of(int D, int F) const { return d * D + f * F + c; }
};
constexpr Ext kD{1, 0, 0}, k2D{2, 0, 0}, k3D{3, 0, 0}, kF{0, 1, 0}, kOne{0, 0, 1}, kTaps{0, 0, 31};
struct LayerTensor {
  const float* eec_layer_params::*src;
  float* PackedLayer::*f32;  // destination of the fp32 kinds, else nullptr
  uint4* PackedLayer::*img;  // destination of the image kinds, else nullptr
  Ext rows, cols;
  PackKind kind;
  float scale;
  size_t count(int D, int F) const {  // elements of the destination's type
    const int N = rows.of(D, F), K = cols.of(D, F);
    return f32 ? (size_t)N * K : kind == PK_FRAG ? frag_u4(N, K) : f8_u4(N, K);
  }
};
using LP = eec_layer_params;
using PL = PackedLayer;
constexpr LayerTensor vec(const float* LP::*src, float* PL::*dst, Ext n, PackKind kind = PK_COPY, float scale = 1.0f) { return {src, dst, nullptr, n, kOne, kind, scale}; }
constexpr LayerTensor img(const float* LP::*src, uint4* PL::*dst, Ext rows, Ext cols, PackKind kind, float scale = 1.0f) { return {src, nullptr, dst, rows, cols, kind, scale}; }
const LayerTensor kLayerTensors[] = {  // the feed-forward modules are stored with W1 and b1 times log2(e) and W2 divided by it
    vec(&LP::ffn1_ln_w, &PL::ffn1_ln_w, kD),
    vec(&LP::ffn1_ln_b, &PL::ffn1_ln_b, kD),
    vec(&LP::ffn1_b1, &PL::ffn1_b1, kF, PK_SCALE, kLog2e),
    vec(&LP::ffn1_b2, &PL::ffn1_b2, kD),
    img(&LP::ffn1_w1, &PL::ffn1_w1p, kF, kD, PK_FRAG, kLog2e),
    img(&LP::ffn1_w2, &PL::ffn1_w2p, kD, kF, PK_FRAG, 1.0f / kLog2e),
    img(&LP::ffn1_w1, &PL::ffn1_w1f8, kF, kD, PK_F8_FFN, kLog2e),
    img(&LP::ffn1_w2, &PL::ffn1_w2f8, kD, kF, PK_F8_FFN, 1.0f / kLog2e),
    vec(&LP::attn_ln_w, &PL::attn_ln_w, kD),
    vec(&LP::attn_ln_b, &PL::attn_ln_b, kD),
    vec(&LP::attn_in_b, &PL::attn_in_b, k3D),
    vec(&LP::attn_out_b, &PL::attn_out_b, kD),
    img(&LP::attn_in_w, &PL::attn_in_p, k3D, kD, PK_FRAG),
    img(&LP::attn_out_w, &PL::attn_out_p, kD, kD, PK_FRAG),
    img(&LP::attn_in_w, &PL::attn_in_f8, k3D, kD, PK_F8),
    img(&LP::attn_out_w, &PL::attn_out_f8, kD, kD, PK_F8),
    vec(&LP::conv_ln_w, &PL::conv_ln_w, kD),
    vec(&LP::conv_ln_b, &PL::conv_ln_b, kD),
    vec(&LP::conv_pw1_b, &PL::conv_pw1_b, k2D),
    vec(&LP::conv_pw2_b, &PL::conv_pw2_b, kD),
    LayerTensor{&LP::conv_dw_w, &PL::dw_wfold, nullptr, kTaps, kD, PK_FOLD, 1.0f},
    vec(&LP::conv_dw_b, &PL::dw_bfold, kD, PK_FOLD),
    img(&LP::conv_pw1_w, &PL::conv_pw1_p, k2D, kD, PK_FRAG),
    img(&LP::conv_pw2_w, &PL::conv_pw2_p, kD, kD, PK_FRAG),
    img(&LP::conv_pw1_w, &PL::conv_pw1_f8, k2D, kD, PK_F8),
    img(&LP::conv_pw2_w, &PL::conv_pw2_f8, kD, kD, PK_F8),
    vec(&LP::ffn2_ln_w, &PL::ffn2_ln_w, kD),
    vec(&LP::ffn2_ln_b, &PL::ffn2_ln_b, kD),
    vec(&LP::ffn2_b1, &PL::ffn2_b1, kF, PK_SCALE, kLog2e),
    vec(&LP::ffn2_b2, &PL::ffn2_b2, kD),
    img(&LP::ffn2_w1, &PL::ffn2_w1p, kF, kD, PK_FRAG, kLog2e),
    img(&LP::ffn2_w2, &PL::ffn2_w2p, kD, kF, PK_FRAG, 1.0f / kLog2e),
    img(&LP::ffn2_w1, &PL::ffn2_w1f8, kF, kD, PK_F8_FFN, kLog2e),
    img(&LP::ffn2_w2, &PL::ffn2_w2f8, kD, kF, PK_F8_FFN, 1.0f / kLog2e),
    vec(&LP::final_ln_w, &PL::final_ln_w, kD),
    vec(&LP::final_ln_b, &PL::final_ln_b, kD),
};

}  // namespace

enum KernelClass { KC_STEM = 0, KC_FFN, KC_QKV, KC_ATTN, KC_PROJ_GLU, KC_PROJ, KC_DW_PW2, KC_HEAD, KC_CHAIN, KC_COUNT };

struct eec_encoder {
  eec_config cfg;
  int device = -1;  // the HIP device the packed-weight arena lives on: every entry point must run with it current
  Bump arena;
  bool packed = false;
  bool has_stem = false, has_stem1 = false, has_heads = false;  // eec_encoder_pack may be given layers only (building-block use)
  // optional per-kernel-class timing with HIP events on the launch stream (bench/roofline only)
  bool profiling = false;
  std::vector<hipEvent_t> ev;       // pairs: start, stop
  std::vector<int> ev_class;        // class of each recorded pair
  size_t ev_used = 0;
  double prof_ms[KC_COUNT] = {0};
  long long prof_n[KC_COUNT] = {0};
  std::vector<PackedLayer> layers;
  uint4 *sub_w1p, *sub_wfp;          // the first convolution alone (one-convolution stem); both convolutions folded into one
  float *sub_b1, *sub_bf, *sub_weff, *pe;  // sub_weff: the folded weight in fp32, [D][7 n_mels], as composed at pack time
  std::vector<uint4*> head_p, head_f8;
  std::vector<float*> head_b;

  void carve() {
    const int D = cfg.d_model, F = cfg.d_ff, nl = cfg.n_exits * cfg.layers_per_exit;
    layers.assign(nl, PackedLayer());
    for (auto& L : layers)
      for (const LayerTensor& t : kLayerTensors) {
        if (t.f32) L.*t.f32 = arena.take<float>(t.count(D, F));
        else L.*t.img = arena.take<uint4>(t.count(D, F));
      }
    sub_w1p = arena.take<uint4>(frag_u4(D, cfg.n_mels * 3));
    sub_b1 = arena.take<float>(D);
    sub_wfp = arena.take<uint4>(frag_u4(D, 7 * cfg.n_mels));
    sub_bf = arena.take<float>(D);
    sub_weff = arena.take<float>((size_t)D * 7 * cfg.n_mels);
    pe = arena.take<float>((size_t)cfg.max_len * D);
    head_p.assign(cfg.n_exits, nullptr);
    head_f8.assign(cfg.n_exits, nullptr);
    head_b.assign(cfg.n_exits, nullptr);
    for (int e = 0; e < cfg.n_exits; ++e) {
      head_p[e] = arena.take<uint4>(frag_u4(cfg.vocab, D));
      head_f8[e] = arena.take<uint4>(f8_u4(cfg.vocab, D));
      head_b[e] = arena.take<float>(cfg.vocab);
    }
    arena.off = up256(arena.off);
  }
};

namespace {

// the six planes a run of layers works in (eec_encoder_group_forward's whole workspace)
struct GroupWs {
  half_t *q, *k, *vt, *p_hi, *p_lo, *g;
  size_t bytes;
};
void carve_group_planes(Bump& a, GroupWs& w, const eec_config& c, int B, int Tq) {
  const int Tp = (Tq + 31) / 32 * 32;
  const size_t M = (size_t)B * Tq, D = c.d_model;
  w.q = a.take<half_t>((size_t)2 * B * Tp * D);   // hi plane, then the residual plane (exact mode f16x3 only)
  w.k = a.take<half_t>((size_t)2 * B * Tp * D);
  w.vt = a.take<half_t>((size_t)2 * B * Tp * D);  // hi plane, then the residual plane
  w.p_hi = a.take<half_t>(M * D);
  w.p_lo = a.take<half_t>(M * D);
  w.g = a.take<half_t>(M * D);
}
GroupWs carve_group_ws(const eec_config& c, int B, int Tq, char* base) {
  Bump a;
  a.base = base;
  GroupWs w;
  carve_group_planes(a, w, c, B, Tq);
  w.bytes = up256(a.off);
  return w;
}

struct Workspace {
  float* x;
  float* y;  // [(E-1)][M][256]: exit rows for the batched head launch when the caller passes no tap buffer
  GroupWs gw;
  int* enc_len;
  size_t bytes;
};

Workspace carve_ws(const eec_config& c, int B, int T, char* base) {
  const int T1 = (T - 3) / 2 + 1, Tq = (T1 - 3) / 2 + 1;
  const size_t M = (size_t)B * Tq, D = c.d_model;
  Bump a;
  a.base = base;
  Workspace w;
  w.x = a.take<float>(M * D);
  w.y = a.take<float>((size_t)(c.n_exits > 1 ? c.n_exits - 1 : 0) * M * D);
  carve_group_planes(a, w.gw, c, B, Tq);
  w.enc_len = a.take<int>(B);
  w.bytes = up256(a.off);
  return w;
}

// One device per encoder handle: the arena (and the caller's workspace) are plain device allocations, never peer-mapped.
int check_device(const eec_encoder* enc) {
  int dev = -1;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return hip_fail(e, "hipGetDevice");
  if (dev != enc->device)
    return fail(EEC_ERR_BAD_ARG, "encoder was created on device " + std::to_string(enc->device) + " but device " +
                                     std::to_string(dev) + " is current (one handle per device; re-create it after a move)");
  return 0;
}

int check_cfg(const eec_config& c) {
  if (c.arch != EEC_ARCH_CONFORMER && c.arch != EEC_ARCH_LEGACY) return fail(EEC_ERR_BAD_ARG, "unknown arch");
  if (c.d_model != 256 && c.d_model != 512) return fail(EEC_ERR_UNSUPPORTED, "d_model must be 256 or 512 in this build");
  if (c.n_heads <= 0 || c.d_model % c.n_heads) return fail(EEC_ERR_BAD_ARG, "n_heads must divide d_model");
  const int dh = c.d_model / c.n_heads;
  if (dh != 32 && dh != 64) return fail(EEC_ERR_UNSUPPORTED, "head dim must be 32 or 64");
  if (c.d_ff <= 0 || c.d_ff % 32) return fail(EEC_ERR_UNSUPPORTED, "d_ff must be a positive multiple of 32");
  if (c.arch == EEC_ARCH_CONFORMER && (c.dw_kernel < 1 || c.dw_kernel > 31 || !(c.dw_kernel & 1)))
    return fail(EEC_ERR_UNSUPPORTED, "depthwise kernel must be odd and <= 31");
  if (c.vocab <= 0 || c.vocab > 256 || c.vocab % 32) return fail(EEC_ERR_UNSUPPORTED, "vocab must be a multiple of 32, <= 256");
  if ((c.n_mels * 3) % 16 || c.n_mels * 3 > 384)
    return fail(EEC_ERR_UNSUPPORTED, "n_mels*3 must be a multiple of 16 and <= 384 (n_mels in {16,32,48,64,80,96,112,128})");
  if (c.n_exits <= 0 || c.layers_per_exit <= 0 || c.n_mels <= 0 || c.max_len <= 0)
    return fail(EEC_ERR_BAD_ARG, "n_exits, layers_per_exit, n_mels, max_len must be positive");
  return 0;
}

}  // namespace

// TIMED(class, launch-expression): brackets the launch with events when profiling is on (uses `enc` and `st` of the caller)
#define TIMED(cls, expr)                                                        \
  do {                                                                          \
    const bool _p = enc->profiling && (enc->ev_used + 1) * 2 <= enc->ev.size(); \
    if (_p) EEC_HIP(hipEventRecord(enc->ev[enc->ev_used * 2], st));             \
    EEC_HIP(expr);                                                              \
    if (_p) {                                                                   \
      EEC_HIP(hipEventRecord(enc->ev[enc->ev_used * 2 + 1], st));               \
      enc->ev_class[enc->ev_used++] = (cls);                                    \
    }                                                                           \
  } while (0)

// The production launch plan of Conformer layers [l0, l1) on rows x (in place): 3 launches per layer.  Everything that
// is local to a 64-row tile runs in ONE chain kernel per layer boundary,
//   [depthwise + pointwise-2 of layer l] -> ffn2(l) + final LN (+ tap) -> ffn1(l+1) -> in_proj(l+1),
// and only the two steps with cross-tile dependencies keep their own launch: attention (all keys of the utterance) and
// out_proj + LN + pointwise-1 + GLU (whose output the depthwise conv reads with a +-15 frame halo).  tap_of(li) says
// where layer li's output is stored besides x (nullptr: nowhere; x itself moves on to ffn1 of layer li + 1).
struct LayerBufs {
  float* x;
  half_t *q, *k, *vt, *vt_lo, *p_hi, *p_lo, *g;
  const int* key_len;
  half_t *q_lo = nullptr, *k_lo = nullptr;  // exact mode (f16x3): Q and K keep their fp16 residuals, attention runs as its own launch
};
struct LayerFormats {
  int ffn, front, qkv, att, glu;  // operand formats of the GEMM groups (1, 3 or 8)
};
// What a precision means for the launch plans: the operand format of every GEMM group and which residual planes exist.
struct Formats {
  LayerFormats layer;  // the production plan's groups
  int o, p, head;      // fragment formats (1 or 3) of the legacy plan and the attention; the projections' format; the exit heads'
  bool v_res, qk_res;  // V keeps its fp16 residual plane; Q and K keep theirs (exact mode)
};
static Formats formats_of(const eec_config& c, int precision) {
  const int np_ffn = precision == EEC_PREC_F16X3 ? 3 : (precision == EEC_PREC_F16F8 ? 8 : 1);
  const int np_o = precision == EEC_PREC_F16 ? 1 : 3;
  // f16f8 (default): besides the feed-forward, out_proj + pointwise-1, pointwise-2 and (round 3) in_proj run on the f8
  // stream (fp16 + two fp8 correction products); the exit heads (their error is the logit error) keep the exact 3-pass
  // split.  Measured on the default model, 3 weight / input seeds (profiles/r02_np_budget.txt): max |dlogp| 3.6e-4 (2.5e-4
  // with in_proj on the 3-pass split: its error is amplified by the softmax, but the chain kernel's in_proj tail is
  // MFMA-bound at three passes: -8 us of 169 per launch, profiles/r03_ab_chain_knobs.txt), heads too 4.0e-4
  // (d_model 512 keeps the fragment formats there: its f8 projection kernels do not fit the register file yet)
  const bool conformer = c.arch == EEC_ARCH_CONFORMER;
  const int np_p = (precision == EEC_PREC_F16F8 && conformer && c.d_model == 256 && c.d_ff % 128 == 0) ? 8 : np_o;
  Formats f;
  f.layer = LayerFormats{np_ffn, np_p, np_p, np_o, np_p};
  f.o = np_o, f.p = np_p, f.head = np_o;
  f.v_res = np_o == 3;  // V keeps its fp16 residual in the split modes
  // exact parity mode (f16x3): Q, K and the attention probabilities keep their fp16 residuals as well (three MFMA products per
  // attention product, attention as its own launch): what remains of the log-prob error is the GLU output's fp16 rounding
  f.qk_res = precision == EEC_PREC_F16X3 && conformer;
  return f;
}
// the buffers of a run of layers on rows x: the residual planes are the second halves of the q / k / vt planes
static LayerBufs layer_bufs(float* x, const GroupWs& w, const int* key_len, const Formats& f, int B, int Tq, int D) {
  const size_t plane = (size_t)B * ((Tq + 31) / 32 * 32) * D;
  LayerBufs b{x, w.q, w.k, w.vt, f.v_res ? w.vt + plane : nullptr, w.p_hi, w.p_lo, w.g, key_len};
  if (f.qk_res) b.q_lo = w.q + plane, b.k_lo = w.k + plane;
  return b;
}
template <typename TapFn>
static int run_layer_plan(eec_encoder* enc, int l0, int l1, const LayerBufs& b, int B, int Tq, const LayerFormats& np,
                          TapFn tap_of, hipStream_t st) {
  const eec_config& c = enc->cfg;
  const int Tp = (Tq + 31) / 32 * 32, M = B * Tq, D = c.d_model, H = c.n_heads;
  // the attention of a row tile runs in the prologue of the out_proj / GLU launch when the shape allows it -- a property of the
  // call, not of the layer (exact mode: Q / K residual planes present -> its three-product form, which needs glu format 3); the
  // chain tail then writes V^T fragment-major for it
  AttnArgs at_shape{b.q, b.k, b.vt, b.key_len, B, H, Tq, Tp, D / H, b.p_hi, b.p_lo, b.vt_lo};
  const bool fused_attn = attn_fusable(at_shape, D) && (np.att != 1) == (np.glu != 1) && (!b.q_lo || np.glu == 3);
  auto qkv_args = [&](const PackedLayer& L) {
    QkvArgs q{b.x, M, B, Tq, Tp, H, D, L.attn_ln_w, L.attn_ln_b, L.attn_in_p, L.attn_in_b, b.q, b.k, b.vt, b.vt_lo, L.attn_in_f8};
    q.q_lo = b.q_lo, q.k_lo = b.k_lo;
    q.vt_frag = fused_attn && D == 256 && Tq % 64 == 0 ? 1 : 0;  // qkv_body's whole-line store path is taken for exactly these shapes
    return q;
  };
  auto stage1 = [&](const PackedLayer& L) {
    return FfnStage{L.ffn1_ln_w, L.ffn1_ln_b, L.ffn1_w1p, L.ffn1_b1, L.ffn1_w2p, L.ffn1_b2, nullptr, nullptr,
                    L.ffn1_w1f8, L.ffn1_w2f8, 0.5f, nullptr};
  };
  {
    ChainArgs ca{};
    ca.x = b.x, ca.M = M, ca.F = c.d_ff, ca.D = D, ca.nstage = 1, ca.Tq = Tq;
    ca.st[0] = stage1(enc->layers[l0]);
    ca.qkv = qkv_args(enc->layers[l0]);
    TIMED(KC_CHAIN, launch_ffn_chain(ca, np.ffn, np.front, np.qkv, false, true, false, st));
  }
  for (int li = l0; li < l1; ++li) {
    const PackedLayer& L = enc->layers[li];
    const bool last = li + 1 == l1;
    AttnArgs at{b.q, b.k, b.vt, b.key_len, B, H, Tq, Tp, D / H, b.p_hi, b.p_lo, b.vt_lo};
    at.q_lo = b.q_lo, at.k_lo = b.k_lo;
    at.vt_frag = fused_attn && D == 256 && Tq % 64 == 0 ? 1 : 0;
    ProjResArgs pr{b.x, M, D, b.p_hi, b.p_lo, L.attn_out_p, L.attn_out_b, L.attn_out_f8};
    GluArgs ga{b.x, M, L.conv_ln_w, L.conv_ln_b, L.conv_pw1_p, L.conv_pw1_b, b.g, L.conv_pw1_f8};
    if (fused_attn) {
      // two launches per layer: the attention of a row tile runs in the prologue of the out_proj / GLU kernel
      TIMED(KC_PROJ_GLU, launch_attn_proj_glu(at, pr, ga, np.glu, st));
    } else {
      TIMED(KC_ATTN, launch_attention(at, np.att == 1 ? 1 : 3, st));
      TIMED(KC_PROJ_GLU, launch_proj_glu(pr, ga, np.glu, st));
    }
    ChainArgs ca{};
    ca.x = b.x, ca.M = M, ca.F = c.d_ff, ca.D = D, ca.nstage = last ? 1 : 2, ca.Tq = Tq;
    ca.dw = DwArgs{b.g, B, Tq, L.dw_wfold, L.dw_bfold, b.p_hi, b.p_lo};
    ca.pw2 = ProjResArgs{b.x, M, D, nullptr, nullptr, L.conv_pw2_p, L.conv_pw2_b, L.conv_pw2_f8};
    ca.st[0] = FfnStage{L.ffn2_ln_w, L.ffn2_ln_b, L.ffn2_w1p, L.ffn2_b1, L.ffn2_w2p, L.ffn2_b2, L.final_ln_w, L.final_ln_b,
                        L.ffn2_w1f8, L.ffn2_w2f8, 0.5f, tap_of(li)};
    if (!last) {
      ca.st[1] = stage1(enc->layers[li + 1]);
      ca.qkv = qkv_args(enc->layers[li + 1]);
    }
    TIMED(KC_CHAIN, launch_ffn_chain(ca, np.ffn, np.front, np.qkv, true, !last, false, st));
  }
  return 0;
}


extern "C" {

const char* eec_last_error(void) { return g_err.c_str(); }
int eec_abi_version(void) { return EEC_ABI_VERSION; }

int eec_out_frames(int T) {
  if (T < 7) return 0;
  const int T1 = (T - 3) / 2 + 1;
  return (T1 - 3) / 2 + 1;
}

int eec_encoder_lengths(const int64_t* lengths, int B, int Tq, int32_t* enc_len, void* stream) {
  if (!lengths || !enc_len || B <= 0 || Tq <= 0) return fail(EEC_ERR_BAD_ARG, "bad argument");
  EEC_HIP(launch_enc_lengths((const long long*)lengths, B, Tq, enc_len, (hipStream_t)stream));
  return 0;
}

int eec_upload_i64_max(void) { return kUploadMax; }

int eec_upload_i64(const int64_t* host, int n, int64_t* dev, void* stream) {
  if (!host || !dev || n <= 0 || n > kUploadMax) return fail(EEC_ERR_BAD_ARG, "eec_upload_i64: 1 .. 480 values");
  EEC_HIP(launch_upload_i64((const long long*)host, n, (long long*)dev, (hipStream_t)stream));
  return 0;
}

int eec_encoder_create(const eec_config* cfg, eec_encoder** out) {
  if (!cfg || !out) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_cfg(*cfg)) return rc;
  eec_encoder* enc = new eec_encoder();
  enc->cfg = *cfg;
  if (hipError_t e = hipGetDevice(&enc->device); e != hipSuccess) {
    delete enc;
    return hip_fail(e, "hipGetDevice");
  }
  enc->carve();  // dry run: sizes only
  const size_t need = enc->arena.off;
  void* mem = nullptr;
  hipError_t e = hipMalloc(&mem, need);
  if (e != hipSuccess) {
    delete enc;
    return hip_fail(e, "hipMalloc(packed weights)");
  }
  enc->arena = Bump();
  enc->arena.base = (char*)mem;
  enc->arena.cap = need;
  enc->carve();
  *out = enc;
  return 0;
}

void eec_encoder_destroy(eec_encoder* enc) {
  if (!enc) return;
  for (hipEvent_t e : enc->ev) (void)hipEventDestroy(e);
  if (enc->arena.base) (void)hipFree(enc->arena.base);
  delete enc;
}

// The stem and the exit heads, for both pack entries; marks the encoder packed.  A stem may be given whole (two
// convolutions), as its first convolution only (enough for eec_encoder_stem1_forward) or not at all; the heads likewise.
static int pack_stem_and_heads(eec_encoder* enc, const float* sub0_w, const float* sub0_b, const float* sub1_w, const float* sub1_b,
                               const float* pe, const float* const* head_w, const float* const* head_b, hipStream_t st) {
  const eec_config& c = enc->cfg;
  const int D = c.d_model;
  auto cp = [&](float* dst, const float* src, size_t n) {
    return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
  };
  enc->has_stem1 = sub0_w && sub0_b && pe;
  enc->has_stem = enc->has_stem1 && sub1_w && sub1_b;
  if (enc->has_stem1) {
    EEC_HIP(launch_pack_frags(sub0_w, D, c.n_mels * 3, enc->sub_w1p, 1.0f, st));
    EEC_HIP(cp(enc->sub_b1, sub0_b, D));
  }
  if (enc->has_stem) {
    // the two convolutions compose into one (k = 7, stride 4): here, once per pack, and nowhere else
    EEC_HIP(launch_stem_fold(sub0_w, sub0_b, sub1_w, sub1_b, D, c.n_mels, enc->sub_weff, enc->sub_bf, st));
    EEC_HIP(launch_pack_frags(enc->sub_weff, D, 7 * c.n_mels, enc->sub_wfp, (float)(1 << kStemWShift), st));
  }
  if (enc->has_stem1) EEC_HIP(cp(enc->pe, pe, (size_t)c.max_len * D));
  enc->has_heads = head_w != nullptr;
  if (enc->has_heads)
    for (int e = 0; e < c.n_exits; ++e) {
      if (!head_w[e] || !head_b[e]) return fail(EEC_ERR_BAD_ARG, "null head parameter");
      EEC_HIP(launch_pack_frags(head_w[e], c.vocab, D, enc->head_p[e], 1.0f, st));
      EEC_HIP(launch_pack_frags_f8(head_w[e], c.vocab, D, enc->head_f8[e], 1.0f, st));
      EEC_HIP(cp(enc->head_b[e], head_b[e], c.vocab));
    }
  enc->packed = true;
  return 0;
}

int eec_encoder_pack(eec_encoder* enc, const eec_params* p, void* stream) {
  if (!enc || !p || !p->layers) return fail(EEC_ERR_BAD_ARG, "null argument");
  if ((p->head_w == nullptr) != (p->head_b == nullptr)) return fail(EEC_ERR_BAD_ARG, "head_w and head_b go together");
  if (enc->cfg.arch != EEC_ARCH_CONFORMER) return fail(EEC_ERR_BAD_ARG, "use eec_encoder_pack_legacy for EEC_ARCH_LEGACY");
  if (int rc = check_device(enc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const eec_config& c = enc->cfg;
  const int D = c.d_model, F = c.d_ff;
  auto cp = [&](float* dst, const float* src, size_t n) {
    return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
  };
  for (size_t i = 0; i < enc->layers.size(); ++i) {
    const eec_layer_params& s = p->layers[i];
    PackedLayer& L = enc->layers[i];
    for (const LayerTensor& t : kLayerTensors) {
      const int N = t.rows.of(D, F), K = t.cols.of(D, F);
      if (t.kind == PK_COPY) EEC_HIP(cp(L.*t.f32, s.*t.src, t.count(D, F)));
      if (t.kind == PK_SCALE) EEC_HIP(launch_scale_copy(s.*t.src, L.*t.f32, N * K, t.scale, st));
      if (t.kind == PK_FRAG) EEC_HIP(launch_pack_frags(s.*t.src, N, K, L.*t.img, t.scale, st));
      if (t.kind == PK_F8 || (t.kind == PK_F8_FFN && F % 128 == 0)) EEC_HIP(launch_pack_frags_f8(s.*t.src, N, K, L.*t.img, t.scale, st));
    }
    EEC_HIP(launch_fold_dw(s.conv_dw_w, s.conv_dw_b, s.conv_bn_w, s.conv_bn_b, s.conv_bn_rm, s.conv_bn_rv,
                           c.dw_kernel, D, L.dw_wfold, L.dw_bfold, st));
  }
  return pack_stem_and_heads(enc, p->sub0_w, p->sub0_b, p->sub1_w, p->sub1_b, p->pe, p->head_w, p->head_b, st);
}

int eec_encoder_pack_legacy(eec_encoder* enc, const eec_legacy_params* p, void* stream) {
  if (!enc || !p || !p->layers || !p->group_ln_w || !p->group_ln_b || !p->head_w || !p->head_b)
    return fail(EEC_ERR_BAD_ARG, "null argument");
  if (enc->cfg.arch != EEC_ARCH_LEGACY) return fail(EEC_ERR_BAD_ARG, "encoder was not created with EEC_ARCH_LEGACY");
  if (int rc = check_device(enc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const eec_config& c = enc->cfg;
  const int D = c.d_model, F = c.d_ff;
  auto cp = [&](float* dst, const float* src, size_t n) {
    return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
  };
  const size_t tile8 = frag_u4(D, D);  // the D/32 n-tiles (D output columns) of one of w_q / w_k / w_v
  for (size_t i = 0; i < enc->layers.size(); ++i) {
    const eec_legacy_layer_params& s = p->layers[i];
    PackedLayer& L = enc->layers[i];
    const int e = (int)i / c.layers_per_exit;
    EEC_HIP(cp(L.attn_ln_w, s.norm1_w, D));
    EEC_HIP(cp(L.attn_ln_b, s.norm1_b, D));
    // w_q / w_k / w_v become one [768][256] in_proj
    EEC_HIP(launch_pack_frags(s.wq, D, D, L.attn_in_p, 1.0f, st));
    EEC_HIP(launch_pack_frags(s.wk, D, D, L.attn_in_p + tile8, 1.0f, st));
    EEC_HIP(launch_pack_frags(s.wv, D, D, L.attn_in_p + 2 * tile8, 1.0f, st));
    EEC_HIP(cp(L.attn_in_b, s.bq, D));
    EEC_HIP(cp(L.attn_in_b + D, s.bk, D));
    EEC_HIP(cp(L.attn_in_b + 2 * D, s.bv, D));
    EEC_HIP(launch_pack_frags(s.wo, D, D, L.attn_out_p, 1.0f, st));
    EEC_HIP(cp(L.attn_out_b, s.bo, D));
    EEC_HIP(cp(L.ffn2_ln_w, s.norm2_w, D));
    EEC_HIP(cp(L.ffn2_ln_b, s.norm2_b, D));
    EEC_HIP(launch_pack_frags(s.w1, F, D, L.ffn2_w1p, 1.0f, st));
    EEC_HIP(cp(L.ffn2_b1, s.b1, F));
    EEC_HIP(launch_pack_frags(s.w2, D, F, L.ffn2_w2p, 1.0f, st));
    if (F % 128 == 0) {
      EEC_HIP(launch_pack_frags_f8(s.w1, F, D, L.ffn2_w1f8, 1.0f, st));
      EEC_HIP(launch_pack_frags_f8(s.w2, D, F, L.ffn2_w2f8, 1.0f, st));
    }
    EEC_HIP(cp(L.ffn2_b2, s.b2, D));
    EEC_HIP(cp(L.final_ln_w, p->group_ln_w[e], D));
    EEC_HIP(cp(L.final_ln_b, p->group_ln_b[e], D));
  }
  return pack_stem_and_heads(enc, p->sub0_w, p->sub0_b, p->sub1_w, p->sub1_b, p->pe, p->head_w, p->head_b, st);
}

size_t eec_encoder_workspace_bytes(const eec_encoder* enc, int B, int T) {
  if (!enc || B <= 0 || T < 7) return 0;
  return carve_ws(enc->cfg, B, T, nullptr).bytes;
}

// n_groups: exit groups to run (1 .. E); the production plan then ends after the last layer of group n_groups
static int forward_impl(eec_encoder* enc, const float* mel, const int64_t* lengths, int B, int T, int precision,
                        float* out, float* taps_opt, void* workspace, size_t workspace_bytes, int stop_after,
                        float* x_dbg_opt, int n_groups, void* stream) {
  if (!enc || !mel || !lengths || !workspace) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (!out && !taps_opt && !x_dbg_opt && stop_after < 0) return fail(EEC_ERR_BAD_ARG, "no output buffer given");
  if (n_groups < 1 || n_groups > enc->cfg.n_exits) return fail(EEC_ERR_BAD_ARG, "n_groups must be in 1 .. n_exits");
  if (enc->packed && enc->cfg.arch == EEC_ARCH_CONFORMER && (!enc->has_stem || (out && !enc->has_heads)))
    return fail(EEC_ERR_NOT_PACKED, "this encoder was packed without stem / head parameters");
  if (!enc->packed) return fail(EEC_ERR_NOT_PACKED, "eec_encoder_pack has not been called");
  if (int rc = check_device(enc)) return rc;
  if (B <= 0 || T < 7) return fail(EEC_ERR_BAD_ARG, "need B > 0 and T >= 7 (two k=3 s=2 convs)");
  if (int rc = check_precision(precision)) return rc;
  const eec_config& c = enc->cfg;
  const int T1 = (T - 3) / 2 + 1, Tq = (T1 - 3) / 2 + 1, Tp = (Tq + 31) / 32 * 32;
  if (Tq > c.max_len) return fail(EEC_ERR_BAD_ARG, "T' exceeds the positional-encoding table (max_len)");
  const Workspace ws = carve_ws(c, B, T, (char*)workspace);
  if (int rc = check_workspace(workspace, workspace_bytes, ws.bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Formats fm = formats_of(c, precision);
  const int np_ffn = fm.layer.ffn, np_o = fm.o, np_p = fm.p;
  const LayerBufs bufs = layer_bufs(ws.x, ws.gw, ws.enc_len, fm, B, Tq, c.d_model);
  half_t *const vt_lo = bufs.vt_lo, *const q_lo = bufs.q_lo, *const k_lo = bufs.k_lo;
  const int M = B * Tq, D = c.d_model, H = c.n_heads;
  int step = 0;
  auto done = [&](void) -> bool { return stop_after >= 0 && step > stop_after; };
  auto finish_dbg = [&]() -> int {
    if (x_dbg_opt) EEC_HIP(hipMemcpyAsync(x_dbg_opt, ws.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
    return 0;
  };


  EEC_HIP(launch_enc_lengths((const long long*)lengths, B, Tq, ws.enc_len, st));
  if (Tp != Tq) EEC_HIP(hipMemsetAsync(ws.gw.vt, 0, (size_t)2 * B * Tp * D * sizeof(half_t), st));
  {
    SubsampleArgs a{mel, B, c.n_mels, T, T1, Tq, D, nullptr, nullptr, enc->sub_wfp, enc->sub_bf, enc->pe, ws.x};
    TIMED(KC_STEM, launch_subsample(a, 3, st));  // raw power mel: always hi/lo split (1 % of the flops)
  }
  ++step;
  if (done()) return finish_dbg();

  if (c.arch == EEC_ARCH_LEGACY) {
    // Early_encoder: every key is valid (mask=None): overwrite the clamp(lengths/4) result with T'
    EEC_HIP(launch_fill_int(ws.enc_len, B, Tq, st));
    for (int e = 0; e < n_groups; ++e) {
      for (int l = 0; l < c.layers_per_exit; ++l) {
        const PackedLayer& L = enc->layers[e * c.layers_per_exit + l];
        {
          QkvArgs a{ws.x, M, B, Tq, Tp, H, D, L.attn_ln_w, L.attn_ln_b, L.attn_in_p, L.attn_in_b, ws.gw.q, ws.gw.k, ws.gw.vt, vt_lo};
          TIMED(KC_QKV, launch_qkv(a, np_o, st));
          AttnArgs at{ws.gw.q, ws.gw.k, ws.gw.vt, ws.enc_len, B, H, Tq, Tp, D / H, ws.gw.p_hi, ws.gw.p_lo, vt_lo};
          TIMED(KC_ATTN, launch_attention(at, np_o, st));
          ProjResArgs pr{ws.x, M, D, ws.gw.p_hi, ws.gw.p_lo, L.attn_out_p, L.attn_out_b};
          TIMED(KC_PROJ, launch_proj_residual(pr, np_o, st));
        }
        ++step;
        if (done()) return finish_dbg();
        {
          const bool last = l == c.layers_per_exit - 1;  // Encoder.layer_norm closes the group
          FfnArgs a{ws.x, M, c.d_ff, D, L.ffn2_ln_w, L.ffn2_ln_b, L.ffn2_w1p, L.ffn2_b1, L.ffn2_w2p, L.ffn2_b2,
                    last ? L.final_ln_w : nullptr, last ? L.final_ln_b : nullptr, 1.0f, true};
          a.w1f8 = L.ffn2_w1f8, a.w2f8 = L.ffn2_w2f8;
          TIMED(KC_FFN, launch_ffn(a, np_ffn, st));
        }
        ++step;
        if (done()) return finish_dbg();
      }
      if (out) {
        HeadArgs h{ws.x, M, c.vocab, D, enc->head_p[e], enc->head_b[e], out + (size_t)e * M * c.vocab};
        TIMED(KC_HEAD, launch_head(h, np_o, st));
      }
      if (taps_opt)
        EEC_HIP(hipMemcpyAsync(taps_opt + (size_t)e * M * D, ws.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
    }
    return finish_dbg();
  }

  if (stop_after < 0) {
    // production plan (run_layer_plan); the sub-step hook (stop_after >= 0) uses the unfused plan below; both are parity-tested
    const int n_layers = n_groups * c.layers_per_exit;
    const bool batch_heads = out && n_groups <= kMaxHeadExits;  // all exit heads in ONE launch after the last layer
    // where exit e's encoder output goes besides x: the caller's tap buffer, else (if a head needs it later) workspace rows
    auto tap_of = [&](int li) -> float* {
      if ((li + 1) % c.layers_per_exit != 0) return nullptr;
      const int e = li / c.layers_per_exit;
      if (taps_opt) return taps_opt + (size_t)e * M * D;
      return (out && li + 1 != n_layers) ? ws.y + (size_t)e * M * D : nullptr;
    };
    if (int rc = run_layer_plan(enc, 0, n_layers, bufs, B, Tq, fm.layer, tap_of, st)) return rc;
    if (out) {
      HeadBatchArgs hb{};
      hb.out = out, hb.M = M, hb.V = c.vocab, hb.E = n_groups, hb.D = D;
      for (int e = 0; e < n_groups; ++e) {
        const int li = (e + 1) * c.layers_per_exit - 1;
        const float* rows = li + 1 == n_layers ? ws.x : tap_of(li);
        if (batch_heads) {
          hb.x[e] = rows, hb.wp[e] = enc->head_p[e], hb.wf8[e] = enc->head_f8[e], hb.bias[e] = enc->head_b[e];
        } else {
          HeadArgs h{rows, M, c.vocab, D, enc->head_p[e], enc->head_b[e], out + (size_t)e * M * c.vocab, enc->head_f8[e]};
          TIMED(KC_HEAD, launch_head(h, fm.head, st));
        }
      }
      if (batch_heads) TIMED(KC_HEAD, launch_head_batch(hb, fm.head, st));
    }
    return finish_dbg();
  }

  for (int e = 0; e < n_groups; ++e) {
    for (int l = 0; l < c.layers_per_exit; ++l) {
      const PackedLayer& L = enc->layers[e * c.layers_per_exit + l];
      {
        FfnArgs a{ws.x, M, c.d_ff, D, L.ffn1_ln_w, L.ffn1_ln_b, L.ffn1_w1p, L.ffn1_b1, L.ffn1_w2p, L.ffn1_b2, nullptr, nullptr};
        a.w1f8 = L.ffn1_w1f8, a.w2f8 = L.ffn1_w2f8;
        TIMED(KC_FFN, launch_ffn(a, np_ffn, st));
      }
      ++step;
      if (done()) return finish_dbg();
      {
        QkvArgs a{ws.x, M, B, Tq, Tp, H, D, L.attn_ln_w, L.attn_ln_b, L.attn_in_p, L.attn_in_b, ws.gw.q, ws.gw.k, ws.gw.vt, vt_lo, L.attn_in_f8};
        a.q_lo = q_lo, a.k_lo = k_lo;
        TIMED(KC_QKV, launch_qkv(a, np_p, st));
        AttnArgs at{ws.gw.q, ws.gw.k, ws.gw.vt, ws.enc_len, B, H, Tq, Tp, D / H, ws.gw.p_hi, ws.gw.p_lo, vt_lo};
        at.q_lo = q_lo, at.k_lo = k_lo;
        TIMED(KC_ATTN, launch_attention(at, np_o, st));
        ProjResArgs pr{ws.x, M, D, ws.gw.p_hi, ws.gw.p_lo, L.attn_out_p, L.attn_out_b, L.attn_out_f8};
        GluArgs ga{ws.x, M, L.conv_ln_w, L.conv_ln_b, L.conv_pw1_p, L.conv_pw1_b, ws.gw.g, L.conv_pw1_f8};
        // out-proj + residual and the conv module's LN -> pointwise-1 -> GLU share one launch
        // (the sub-step hook stops between them, so it falls back to the two separate kernels)
        const bool split_here = stop_after >= 0 && step + 1 > stop_after;
        if (split_here) {
          TIMED(KC_PROJ, launch_proj_residual(pr, np_o, st));
        } else {
          TIMED(KC_PROJ_GLU, launch_proj_glu(pr, ga, np_p, st));
        }
        ++step;
        if (done()) return finish_dbg();
      }
      {
        DwArgs da{ws.gw.g, B, Tq, L.dw_wfold, L.dw_bfold, ws.gw.p_hi, ws.gw.p_lo};
        ProjResArgs pr{ws.x, M, D, nullptr, nullptr, L.conv_pw2_p, L.conv_pw2_b, L.conv_pw2_f8};
        TIMED(KC_DW_PW2, launch_dw_pw2(da, pr, np_p, st));
      }
      ++step;
      if (done()) return finish_dbg();
      {
        FfnArgs a{ws.x, M, c.d_ff, D, L.ffn2_ln_w, L.ffn2_ln_b, L.ffn2_w1p, L.ffn2_b1, L.ffn2_w2p, L.ffn2_b2, L.final_ln_w, L.final_ln_b};
        a.w1f8 = L.ffn2_w1f8, a.w2f8 = L.ffn2_w2f8;
        TIMED(KC_FFN, launch_ffn(a, np_ffn, st));
      }
      ++step;
      if (done()) return finish_dbg();
    }
    if (out) {
      HeadArgs h{ws.x, M, c.vocab, D, enc->head_p[e], enc->head_b[e], out + (size_t)e * M * c.vocab, enc->head_f8[e]};
      TIMED(KC_HEAD, launch_head(h, np_o, st));
    }
    if (taps_opt)
      EEC_HIP(hipMemcpyAsync(taps_opt + (size_t)e * M * D, ws.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
  }
  return finish_dbg();
}

int eec_encoder_forward(eec_encoder* enc, const float* mel, const int64_t* lengths, int B, int T, int precision,
                        float* out, float* taps_opt, void* workspace, size_t workspace_bytes, int stop_after,
                        float* x_dbg_opt, void* stream) {
  if (!enc) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (!out && stop_after < 0) return fail(EEC_ERR_BAD_ARG, "out is null");
  return forward_impl(enc, mel, lengths, B, T, precision, out, taps_opt, workspace, workspace_bytes, stop_after, x_dbg_opt,
                      enc->cfg.n_exits, stream);
}

int eec_encoder_forward_prefix(eec_encoder* enc, const float* mel, const int64_t* lengths, int B, int T, int precision,
                               int n_groups, float* out_opt, float* taps_opt, float* x_out_opt, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!enc) return fail(EEC_ERR_BAD_ARG, "null argument");
  return forward_impl(enc, mel, lengths, B, T, precision, out_opt, taps_opt, workspace, workspace_bytes, -1, x_out_opt,
                      n_groups, stream);
}

// ---------------------------------------------------------------------------
// Building blocks: one exit group / one head on caller-owned rows.  They let a host compose the reference's
// other encoder topologies (Splitformer early_exit.py:227-364: parallel down-sampled branches) out of the same
// kernels; Early_conformer itself goes through eec_encoder_forward.
size_t eec_encoder_group_workspace_bytes(const eec_encoder* enc, int B, int Tq) {
  if (!enc || B <= 0 || Tq <= 0) return 0;
  return carve_group_ws(enc->cfg, B, Tq, nullptr).bytes;
}

int eec_encoder_group_forward(eec_encoder* enc, int group, float* x, const int32_t* key_len, int B, int Tq, int precision,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!enc || !x || !key_len || !workspace) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (!enc->packed) return fail(EEC_ERR_NOT_PACKED, "eec_encoder_pack has not been called");
  if (int rc = check_device(enc)) return rc;
  const eec_config& c = enc->cfg;
  if (c.arch != EEC_ARCH_CONFORMER) return fail(EEC_ERR_UNSUPPORTED, "group forward is built for EEC_ARCH_CONFORMER");
  if (group < 0 || group >= c.n_exits) return fail(EEC_ERR_BAD_ARG, "group out of range");
  if (B <= 0 || Tq <= 0) return fail(EEC_ERR_BAD_ARG, "need B > 0 and T' > 0");
  if (int rc = check_precision(precision)) return rc;
  const GroupWs ws = carve_group_ws(c, B, Tq, (char*)workspace);
  if (int rc = check_workspace(workspace, workspace_bytes, ws.bytes)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Formats fm = formats_of(c, precision);
  const int Tp = (Tq + 31) / 32 * 32, D = c.d_model;
  if (Tp != Tq) EEC_HIP(hipMemsetAsync(ws.vt, 0, (size_t)2 * B * Tp * D * sizeof(half_t), st));
  const LayerBufs bufs = layer_bufs(x, ws, key_len, fm, B, Tq, D);
  const int l0 = group * c.layers_per_exit;
  return run_layer_plan(enc, l0, l0 + c.layers_per_exit, bufs, B, Tq, fm.layer, [](int) -> float* { return nullptr; }, st);
}

int eec_encoder_stem1_forward(eec_encoder* enc, const float* mel, int B, int T, float* x, void* stream) {
  if (!enc || !mel || !x) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (!enc->packed || !enc->has_stem1) return fail(EEC_ERR_NOT_PACKED, "no packed stem parameters");
  if (int rc = check_device(enc)) return rc;
  if (B <= 0 || T < 3) return fail(EEC_ERR_BAD_ARG, "need B > 0 and T >= 3");
  const eec_config& c = enc->cfg;
  const int T1 = (T - 3) / 2 + 1;
  if (T1 > c.max_len) return fail(EEC_ERR_BAD_ARG, "T1 exceeds the positional-encoding table (max_len)");
  hipStream_t st = (hipStream_t)stream;
  SubsampleArgs a{mel, B, c.n_mels, T, T1, T1, c.d_model, enc->sub_w1p, enc->sub_b1, nullptr, nullptr, enc->pe, x};
  TIMED(KC_STEM, launch_subsample_single(a, st));
  return 0;
}

int eec_encoder_head_forward(eec_encoder* enc, int exit, const float* x, int M, float* out, int precision, void* stream) {
  if (!enc || !x || !out) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (!enc->packed || !enc->has_heads) return fail(EEC_ERR_NOT_PACKED, "no packed head parameters");
  if (int rc = check_device(enc)) return rc;
  if (exit < 0 || exit >= enc->cfg.n_exits || M <= 0) return fail(EEC_ERR_BAD_ARG, "exit / M out of range");
  if (int rc = check_precision(precision)) return rc;
  HeadArgs h{x, M, enc->cfg.vocab, enc->cfg.d_model, enc->head_p[exit], enc->head_b[exit], out, enc->head_f8[exit]};
  hipStream_t st = (hipStream_t)stream;
  TIMED(KC_HEAD, launch_head(h, precision == EEC_PREC_F16 ? 1 : 3, st));
  return 0;
}

// what the three CTC loss entries ask of their sizes (each checks its own pointers first); the two forward entries take any
// vocabulary and check the blank label, the backward holds a vocabulary row in one wave and does not read `blank`
static int check_ctc_args(int E, int B, int Tq, int V, int S, int blank, bool backward) {
  if (E <= 0 || B <= 0 || Tq <= 0 || V <= 0 || S <= 0) return fail(EEC_ERR_BAD_ARG, "bad size");
  if (!backward && (blank < 0 || blank >= V)) return fail(EEC_ERR_BAD_ARG, "blank must be a label in [0, V)");
  if (backward && (V > 256 || V % 4)) return fail(EEC_ERR_UNSUPPORTED, "vocab must be a multiple of 4, <= 256");
  if (2 * S + 1 > 512) return fail(EEC_ERR_UNSUPPORTED, "target length above 255");
  return 0;
}

int eec_ctc_loss(const float* logp, const int64_t* targets, const int64_t* target_len, int E, int B, int Tq, int V, int S,
                 int blank, float* nll_scratch, float* loss_per_exit, void* stream) {
  if (!logp || !targets || !target_len || !nll_scratch || !loss_per_exit) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_ctc_args(E, B, Tq, V, S, blank, false)) return rc;
  EEC_HIP(launch_ctc_loss(logp, (const long long*)targets, (const long long*)target_len, E, B, Tq, V, S, blank, nll_scratch,
                          loss_per_exit, nullptr, (hipStream_t)stream));
  return 0;
}

size_t eec_ctc_backward_workspace_bytes(int E, int B, int Tq, int S) {
  if (E <= 0 || B <= 0 || Tq <= 0 || S <= 0) return 0;
  return ctc_store_floats(E, B, Tq, S) * sizeof(float);
}

int eec_ctc_loss_forward(const float* logp, const int64_t* targets, const int64_t* target_len, int E, int B, int Tq, int V, int S,
                         int blank, float* nll, float* loss_per_exit, void* bwd_workspace, void* stream) {
  if (!logp || !targets || !target_len || !nll || !loss_per_exit || !bwd_workspace) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_ctc_args(E, B, Tq, V, S, blank, false)) return rc;
  EEC_HIP(launch_ctc_loss(logp, (const long long*)targets, (const long long*)target_len, E, B, Tq, V, S, blank, nll,
                          loss_per_exit, (float*)bwd_workspace, (hipStream_t)stream));
  return 0;
}

int eec_ctc_loss_backward(const float* logp, const int64_t* targets, const int64_t* target_len, int E, int B, int Tq, int V, int S,
                          int blank, const float* nll, void* bwd_workspace, const float* grad_loss, float* dlogp, void* stream) {
  if (!logp || !targets || !target_len || !nll || !bwd_workspace || !grad_loss || !dlogp) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_ctc_args(E, B, Tq, V, S, blank, true)) return rc;
  EEC_HIP(launch_ctc_backward(logp, (const long long*)targets, (const long long*)target_len, E, B, Tq, V, S, blank, nll,
                              (float*)bwd_workspace, grad_loss, dlogp, (hipStream_t)stream));
  return 0;
}

// the three with per-utterance input lengths: NULL lengths are the entries above, launch for launch
int eec_ctc_loss_len(const float* logp, const int64_t* targets, const int64_t* target_len, const int32_t* input_len, int E, int B,
                     int Tq, int V, int S, int blank, float* nll_scratch, float* loss_per_exit, void* stream) {
  if (!input_len) return eec_ctc_loss(logp, targets, target_len, E, B, Tq, V, S, blank, nll_scratch, loss_per_exit, stream);
  if (!logp || !targets || !target_len || !nll_scratch || !loss_per_exit) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_ctc_args(E, B, Tq, V, S, blank, false)) return rc;
  EEC_HIP(launch_ctc_loss(logp, (const long long*)targets, (const long long*)target_len, input_len, E, B, Tq, V, S, blank,
                          nll_scratch, loss_per_exit, nullptr, (hipStream_t)stream));
  return 0;
}

int eec_ctc_loss_forward_len(const float* logp, const int64_t* targets, const int64_t* target_len, const int32_t* input_len, int E,
                             int B, int Tq, int V, int S, int blank, float* nll, float* loss_per_exit, void* bwd_workspace,
                             void* stream) {
  if (!input_len)
    return eec_ctc_loss_forward(logp, targets, target_len, E, B, Tq, V, S, blank, nll, loss_per_exit, bwd_workspace, stream);
  if (!logp || !targets || !target_len || !nll || !loss_per_exit || !bwd_workspace) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_ctc_args(E, B, Tq, V, S, blank, false)) return rc;
  EEC_HIP(launch_ctc_loss(logp, (const long long*)targets, (const long long*)target_len, input_len, E, B, Tq, V, S, blank, nll,
                          loss_per_exit, (float*)bwd_workspace, (hipStream_t)stream));
  return 0;
}

int eec_ctc_loss_backward_len(const float* logp, const int64_t* targets, const int64_t* target_len, const int32_t* input_len, int E,
                              int B, int Tq, int V, int S, int blank, const float* nll, void* bwd_workspace, const float* grad_loss,
                              float* dlogp, void* stream) {
  if (!input_len)
    return eec_ctc_loss_backward(logp, targets, target_len, E, B, Tq, V, S, blank, nll, bwd_workspace, grad_loss, dlogp, stream);
  if (!logp || !targets || !target_len || !nll || !bwd_workspace || !grad_loss || !dlogp) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_ctc_args(E, B, Tq, V, S, blank, true)) return rc;
  EEC_HIP(launch_ctc_backward(logp, (const long long*)targets, (const long long*)target_len, input_len, E, B, Tq, V, S, blank, nll,
                              (float*)bwd_workspace, grad_loss, dlogp, (hipStream_t)stream));
  return 0;
}

int eec_logsoftmax_backward(const float* logp, const float* grad_logp, int M, int V, float* grad_logits, void* stream) {
  if (!logp || !grad_logp || !grad_logits || M <= 0 || V <= 0) return fail(EEC_ERR_BAD_ARG, "bad argument");
  if (V > 256 || V % 4) return fail(EEC_ERR_UNSUPPORTED, "vocab must be a multiple of 4, <= 256");
  EEC_HIP(launch_logsoftmax_backward(logp, grad_logp, M, V, grad_logits, (hipStream_t)stream));
  return 0;
}

// what the two distillation entries ask of their sizes, the temperature and the teacher map (each checks its own pointers first)
static int check_distill_args(const int32_t* teacher, int E, int B, int T, int V, float tau) {
  if (E <= 0 || B <= 0 || T <= 0 || V <= 0) return fail(EEC_ERR_BAD_ARG, "exit distillation: E, B, T and V must be positive");
  if (E > EEC_DISTILL_MAX_EXITS)
    return fail(EEC_ERR_BAD_ARG, "exit distillation: at most " + std::to_string(EEC_DISTILL_MAX_EXITS) + " exits, got " + std::to_string(E));
  if (V > 256 || V % 4) return fail(EEC_ERR_BAD_ARG, "exit distillation: vocab must be a multiple of 4, <= 256");
  if ((long long)B * T > 0x7fffffffLL) return fail(EEC_ERR_BAD_ARG, "exit distillation: B * T above 2^31 - 1");
  if (!(tau > 0.f) || !(tau < INFINITY)) return fail(EEC_ERR_BAD_ARG, "exit distillation: the temperature must be a finite number above 0");
  for (int e = 0; e < E; ++e) {
    if (teacher[e] < -1 || teacher[e] >= E)
      return fail(EEC_ERR_BAD_ARG, "exit distillation: teacher[" + std::to_string(e) + "] = " + std::to_string(teacher[e]) + " is outside [-1, E)");
    if (teacher[e] == e) return fail(EEC_ERR_BAD_ARG, "exit distillation: exit " + std::to_string(e) + " cannot be its own teacher");
  }
  return 0;
}

size_t eec_exit_distill_workspace_bytes(int E, int B, int T) {
  if (E <= 0 || B <= 0 || T <= 0) return 0;
  return (size_t)E * B * T * sizeof(float);
}

int eec_exit_distill_forward(const float* x, const int32_t* frame_len, const int32_t* teacher, int E, int B, int T, int V, float tau,
                             float* kl, float* loss_per_exit, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !teacher || !kl || !loss_per_exit || !workspace) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_distill_args(teacher, E, B, T, V, tau)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, eec_exit_distill_workspace_bytes(E, B, T))) return rc;
  EEC_HIP(launch_distill_forward(x, frame_len, teacher, E, B, T, V, tau, kl, loss_per_exit, (float*)workspace, (hipStream_t)stream));
  return 0;
}

int eec_exit_distill_backward(const float* x, const int32_t* frame_len, const int32_t* teacher, int E, int B, int T, int V, float tau,
                              const float* grad_loss, int accumulate, float* dx, void* stream) {
  if (!x || !teacher || !grad_loss || !dx) return fail(EEC_ERR_BAD_ARG, "null argument");
  if (int rc = check_distill_args(teacher, E, B, T, V, tau)) return rc;
  EEC_HIP(launch_distill_backward(x, frame_len, teacher, E, B, T, V, tau, grad_loss, accumulate, dx, (hipStream_t)stream));
  return 0;
}

size_t eec_exit_stats_workspace_bytes(int E, int B, int T) {
  if (E <= 0 || B <= 0 || T <= 0) return 0;
  return (size_t)3 * E * B * T * sizeof(float);
}

int eec_exit_stats(const float* x, const int32_t* frame_len, int E, int B, int T, int V, float* stats, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (!x || !stats || !workspace) return fail(EEC_ERR_BAD_ARG, "exit statistics: null argument");
  if (E <= 0 || B <= 0 || T <= 0 || V <= 0) return fail(EEC_ERR_BAD_ARG, "exit statistics: E, B, T and V must be positive");
  if (E > EEC_EXIT_STATS_MAX_EXITS)
    return fail(EEC_ERR_BAD_ARG, "exit statistics: at most " + std::to_string(EEC_EXIT_STATS_MAX_EXITS) + " exits, got " + std::to_string(E));
  if (V > 256 || V % 4) return fail(EEC_ERR_BAD_ARG, "exit statistics: vocab must be a multiple of 4, <= 256");
  if ((long long)B * T > 0x7fffffffLL) return fail(EEC_ERR_BAD_ARG, "exit statistics: B * T above 2^31 - 1");
  if ((long long)3 * E * B > 0x7fffffffLL) return fail(EEC_ERR_BAD_ARG, "exit statistics: 3 * E * B above 2^31 - 1");
  if (int rc = check_workspace(workspace, workspace_bytes, eec_exit_stats_workspace_bytes(E, B, T))) return rc;
  EEC_HIP(launch_exit_stats(x, frame_len, E, B, T, V, stats, (float*)workspace, (hipStream_t)stream));
  return 0;
}

int eec_exit_route(const float* score, int n, float threshold, int higher_is_better, int force_all, int32_t* stay_idx,
                   int32_t* leave_idx, int32_t* counts, void* stream) {
  if (!score || !stay_idx || !leave_idx || !counts) return fail(EEC_ERR_BAD_ARG, "exit route: null argument");
  if (n <= 0) return fail(EEC_ERR_BAD_ARG, "exit route: n must be positive, got " + std::to_string(n));
  if (threshold != threshold && !force_all) return fail(EEC_ERR_BAD_ARG, "exit route: the threshold is NaN");
  EEC_HIP(launch_exit_route(score, n, threshold, higher_is_better != 0, force_all != 0, stay_idx, leave_idx, counts, (hipStream_t)stream));
  return 0;
}

int eec_encoder_set_profiling(eec_encoder* enc, int enable, int max_launches) {
  if (!enc) return fail(EEC_ERR_BAD_ARG, "null argument");
  for (hipEvent_t e : enc->ev) (void)hipEventDestroy(e);
  enc->ev.clear();
  enc->ev_class.clear();
  enc->ev_used = 0;
  for (int i = 0; i < KC_COUNT; ++i) enc->prof_ms[i] = 0, enc->prof_n[i] = 0;
  enc->profiling = enable != 0;
  if (enc->profiling) {
    if (max_launches <= 0) max_launches = 4096;
    enc->ev.resize((size_t)max_launches * 2);
    enc->ev_class.assign(max_launches, 0);
    for (auto& e : enc->ev) EEC_HIP(hipEventCreate(&e));
  }
  return 0;
}

int eec_encoder_profile_read(eec_encoder* enc, double* ms_by_class, long long* launches_by_class, int n_classes) {
  if (!enc || !ms_by_class || !launches_by_class) return fail(EEC_ERR_BAD_ARG, "null argument");
  for (size_t i = 0; i < enc->ev_used; ++i) {
    EEC_HIP(hipEventSynchronize(enc->ev[2 * i + 1]));
    float ms = 0.f;
    EEC_HIP(hipEventElapsedTime(&ms, enc->ev[2 * i], enc->ev[2 * i + 1]));
    enc->prof_ms[enc->ev_class[i]] += ms;
    enc->prof_n[enc->ev_class[i]] += 1;
  }
  enc->ev_used = 0;
  for (int i = 0; i < n_classes && i < KC_COUNT; ++i) {
    ms_by_class[i] = enc->prof_ms[i];
    launches_by_class[i] = enc->prof_n[i];
  }
  return 0;
}

int eec_greedy_ctc(const float* logp, int n_seq, int Tq, int V, int blank, int32_t* tokens, int32_t* counts,
                   void* stream) {
  return eec_greedy_ctc_len(logp, NULL, n_seq, Tq, V, blank, tokens, counts, stream);
}

int eec_greedy_ctc_len(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int32_t* tokens,
                       int32_t* counts, void* stream) {
  if (!logp || !tokens || !counts || n_seq <= 0 || Tq <= 0 || V <= 0) return fail(EEC_ERR_BAD_ARG, "bad argument");
  EEC_HIP(launch_greedy_ctc(logp, em_len, n_seq, Tq, V, blank, tokens, counts, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
