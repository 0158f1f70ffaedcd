/* eec.h -- C ABI of the MI355X-native early-exit Conformer encoder (libeec.so).
 *
 * The reference (augustgw/early-exit-transformer) has no FFI / plugin registry: its
 * drop-in boundary is the Python class `Early_conformer` / `full_conformer`
 * (models/model/early_exit.py:565-634, 637-800) as called from train.py:54,37 and
 * inference.py:66,45.  This library sits behind this repo's own nn.Module mirror of
 * that class (early_exit_transformer_amd/model.py); every entry point below states the
 * reference code it replaces.  Plain pointers and sizes only: all `const float*`,
 * `void* workspace` etc. are DEVICE pointers (HIP), `stream` is a hipStream_t passed as
 * void*.  Every function returns 0 on success, a non-zero hipError_t / EEC_ERR_* code
 * otherwise, and every non-zero return leaves its reason in one thread-local message.
 * eec_last_error() and the eec_*_last_error() of the other families all return that one
 * string: the calling thread's most recent message, whichever family the failing call
 * belonged to.  No entry point allocates, frees or synchronises the device except
 * create/destroy/pack.
 *
 * Devices: an eec_encoder handle belongs to the HIP device that was current in eec_encoder_create (its packed-weight
 * arena is a plain allocation on that device).  Every later call on the handle must be made with the same device
 * current and with parameters / inputs / workspace on it, else EEC_ERR_BAD_ARG.  The intended deployment is one
 * process per GPU (torch.distributed over RCCL); a process that does drive several devices creates one handle per
 * device (launch attributes are tracked per device).  Handles are not thread-safe; use one per thread or lock.
 */
#ifndef EEC_H_
#define EEC_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EEC_ABI_VERSION 16
#define EEC_ERR_BAD_ARG 10001
#define EEC_ERR_UNSUPPORTED 10002
#define EEC_ERR_WORKSPACE 10003
#define EEC_ERR_NOT_PACKED 10004

/* Operand precision of the MFMA products (accumulation, residual stream, LayerNorm,
 * softmax and log-softmax are always fp32).  The reference computes everything in fp32. */
enum {
  EEC_PREC_F16X3 = 0, /* hi/lo-split fp16, 3 MFMA passes per GEMM: |dlogp| ~2e-4, parity mode   */
  EEC_PREC_MIXED = 1, /* feed-forward GEMMs single-pass fp16, all others split: |dlogp| ~1e-3  */
  EEC_PREC_F16 = 2,   /* every GEMM single-pass fp16: |dlogp| ~3e-3                            */
  EEC_PREC_F16F8 = 3  /* as F16X3, but the feed-forward GEMMs compute the two hi/lo correction products
                         with block-scaled fp8 (e5m2) MFMAs at twice the fp16 rate: |dlogp| ~3e-4 */
};

/* Constructor kwargs of Early_conformer that shape the encoder (early_exit.py:567-615;
 * flags util/conf.py --d_model --n_heads --d_feed_forward --depthwise_kernel_size
 * --n_enc_exits --n_enc_layers_per_exit --n_mels, dec_voc_size, --max_len). */
typedef struct eec_config {
  int32_t d_model;         /* 256 or 512 (64-row / 32-row tile geometry) */
  int32_t n_heads;         /* d_model / n_heads in {32, 64} */
  int32_t d_ff;            /* multiple of 32 */
  int32_t dw_kernel;       /* odd, <= 31 */
  int32_t n_exits;         /* E */
  int32_t layers_per_exit; /* L */
  int32_t n_mels;          /* features_length: 3*n_mels a multiple of 16, <= 384 (80 -> 240) */
  int32_t vocab;           /* dec_voc_size: multiple of 32, <= 256 */
  int32_t max_len;         /* rows of the positional-encoding table */
  int32_t arch;            /* EEC_ARCH_CONFORMER (Early_conformer / full_conformer) or EEC_ARCH_LEGACY (Early_encoder) */
} eec_config;

#define EEC_ARCH_CONFORMER 0
#define EEC_ARCH_LEGACY 1

/* fp32 parameters of one torchaudio ConformerLayer, by state_dict key suffix. */
typedef struct eec_layer_params {
  const float *ffn1_ln_w, *ffn1_ln_b;   /* ffn1.sequential.0.{weight,bias}          [D]      */
  const float *ffn1_w1, *ffn1_b1;       /* ffn1.sequential.1.{weight,bias}          [F,D],[F]*/
  const float *ffn1_w2, *ffn1_b2;       /* ffn1.sequential.4.{weight,bias}          [D,F],[D]*/
  const float *attn_ln_w, *attn_ln_b;   /* self_attn_layer_norm.{weight,bias}                */
  const float *attn_in_w, *attn_in_b;   /* self_attn.in_proj_{weight,bias}          [3D,D]   */
  const float *attn_out_w, *attn_out_b; /* self_attn.out_proj.{weight,bias}         [D,D]    */
  const float *conv_ln_w, *conv_ln_b;   /* conv_module.layer_norm.{weight,bias}              */
  const float *conv_pw1_w, *conv_pw1_b; /* conv_module.sequential.0.{weight,bias}   [2D,D,1] */
  const float *conv_dw_w, *conv_dw_b;   /* conv_module.sequential.2.{weight,bias}   [D,1,K]  */
  const float *conv_bn_w, *conv_bn_b;   /* conv_module.sequential.3.{weight,bias}            */
  const float *conv_bn_rm, *conv_bn_rv; /* conv_module.sequential.3.running_{mean,var}       */
  const float *conv_pw2_w, *conv_pw2_b; /* conv_module.sequential.5.{weight,bias}   [D,D,1]  */
  const float *ffn2_ln_w, *ffn2_ln_b, *ffn2_w1, *ffn2_b1, *ffn2_w2, *ffn2_b2; /* ffn2.sequential.* */
  const float *final_ln_w, *final_ln_b; /* final_layer_norm.{weight,bias}                    */
} eec_layer_params;

typedef struct eec_params {
  const float *sub0_w, *sub0_b; /* conv_subsample.sequential.0  [D, n_mels, 3], [D] */
  const float *sub1_w, *sub1_b; /* conv_subsample.sequential.1  [D, D, 3], [D]      */
  const float* pe;              /* positional_encoder.pe        [max_len, 1, D]     */
  const eec_layer_params* layers; /* HOST array of n_exits*layers_per_exit entries, exit-major */
  const float* const* head_w;   /* HOST array of n_exits device pointers: linears.e.weight [V, D] */
  const float* const* head_b;   /* HOST array of n_exits device pointers: linears.e.bias   [V]    */
} eec_params;

/* fp32 parameters of one legacy pre-norm transformer layer, models/blocks/encoder_layer.py:14-44 with
 * models/layers/multi_head_attention.py:11-29 (separate w_q/w_k/w_v/w_concat Linears) and
 * models/layers/position_wise_feed_forward.py:9-23 (Linear -> ReLU -> Linear); SURVEY.md 8a row a14. */
typedef struct eec_legacy_layer_params {
  const float *norm1_w, *norm1_b;                     /* norm1.{weight,bias}                 */
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo; /* attention.w_{q,k,v,concat}.{weight,bias} [D,D],[D] */
  const float *norm2_w, *norm2_b;                     /* norm2.{weight,bias}                 */
  const float *w1, *b1, *w2, *b2;                     /* ffn.linear{1,2}.{weight,bias} [F,D],[F],[D,F],[D] */
} eec_legacy_layer_params;

/* Early_encoder (models/model/early_exit.py:497-562): stem, PE, E x Encoder(L layers + layer_norm), E heads. */
typedef struct eec_legacy_params {
  const float *sub0_w, *sub0_b, *sub1_w, *sub1_b, *pe;
  const eec_legacy_layer_params* layers; /* HOST array, n_exits*layers_per_exit, exit-major: encoders.e.layers.l */
  const float* const* group_ln_w;        /* HOST arrays of n_exits device pointers: encoders.e.layer_norm.{weight,bias} */
  const float* const* group_ln_b;
  const float* const* head_w;            /* linears.e.{weight,bias} */
  const float* const* head_b;
} eec_legacy_params;

typedef struct eec_encoder eec_encoder;

const char* eec_last_error(void);
int eec_abi_version(void);

/* T' = ((T-3)/2+1 - 3)/2 + 1 : frames after the two stride-2 convs (early_exit.py:24-48). */
int eec_out_frames(int T);

/* The length -> key-mask arithmetic of Early_conformer.forward (early_exit.py:623) on its own:
 *   enc_len[b] = int32( min( float(lengths[b]) / 4, float(T') ) )      (true division in fp32, clamp, truncation)
 * keys t >= enc_len[b] are masked in every attention of the stack (torchaudio _lengths_to_padding_mask).  The forward
 * entry points compute it internally; this entry exposes the integers (tests compare them bit for bit). */
int eec_encoder_lengths(const int64_t* lengths, int B, int Tq, int32_t* enc_len, void* stream);
/* A small HOST int64 array (the `lengths` the reference's collate hands to forward() as a CPU tensor, train.py:34,54) -> device
 * memory through a kernel's argument block: stream-ordered like a copy, but no DMA and no cross-queue dependency in front of the
 * forward.  n <= eec_upload_i64_max() (480); the host array is read before the call returns. */
int eec_upload_i64_max(void);
int eec_upload_i64(const int64_t* host, int n, int64_t* dev, void* stream);


/* Replaces Early_conformer.__init__ (early_exit.py:567-615) for the encoder stack. */
int eec_encoder_create(const eec_config* cfg, eec_encoder** out);
void eec_encoder_destroy(eec_encoder* enc);

/* Re-packs the fp32 parameters (fp16 hi/lo MFMA fragments, BatchNorm folded into the depthwise
 * taps, conv weights transposed).  Call after load_state_dict / an optimizer step; eval-mode
 * BatchNorm semantics (running statistics).  Asynchronous on `stream`. */
int eec_encoder_pack(eec_encoder* enc, const eec_params* params, void* stream);

/* Same for an EEC_ARCH_LEGACY encoder (no mask, no convolution module; `lengths` of eec_encoder_forward is ignored:
 * Early_encoder.forward(src) passes mask=None, early_exit.py:549-554). */
int eec_encoder_pack_legacy(eec_encoder* enc, const eec_legacy_params* params, void* stream);

size_t eec_encoder_workspace_bytes(const eec_encoder* enc, int B, int T);

/* Replaces Early_conformer.forward(src, lengths) (early_exit.py:617-634) in eval mode:
 *   mel      [B, n_mels, T] fp32        lengths [B] int64 (device copy of the caller's tensor)
 *   out      [E, B, T', V] fp32 log-probabilities (written in place, no torch.cat)
 *   taps_opt [E, B, T', D] fp32 or NULL: pre-head activations after each exit group
 *            (what full_conformer._encoder_(src, lengths, n) returns, early_exit.py:719-737)
 *   stop_after: <0 = run everything with the production launch plan (Conformer: 3 launches per layer, the
 *            row-tile-local steps fused into one "chain" kernel); otherwise stop after that many
 *            sub-steps (0 = stem, then per layer: ffn1, attention, conv, ffn2; legacy: attention, ffn), each sub-step
 *            its own launch -- test hook; the current residual stream is then left in x_dbg_opt [B*T', D] if given. */
int eec_encoder_forward(eec_encoder* enc, const float* mel, const int64_t* lengths, int B, int T,
                        int precision, float* out, float* taps_opt, void* workspace, size_t workspace_bytes,
                        int stop_after, float* x_dbg_opt, void* stream);

/* Early exit: the same forward, stopped after the first n_groups exit groups (1 .. E) -- what the reference does with
 * full_conformer._encoder_(src, lengths, layer_n) (early_exit.py:719-737: the loop breaks after layer_n groups) and what
 * an early-exit deployment runs when it decodes from exit n_groups.  Production launch plan; cost is n_groups / E of a
 * full forward.
 *   out_opt   [n_groups, B, T', V] log-probs of the exits that were run, or NULL
 *   taps_opt  [n_groups, B, T', D] or NULL          x_out_opt [B, T', D]: encoder output after group n_groups, or NULL
 * At least one of the three must be given. */
int eec_encoder_forward_prefix(eec_encoder* enc, const float* mel, const int64_t* lengths, int B, int T, int precision,
                               int n_groups, float* out_opt, float* taps_opt, float* x_out_opt, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Building blocks for the reference's other encoder topologies built from the same Conformer groups (Splitformer,
 * early_exit.py:227-364: down-sampled parallel branches added to the main path at the first and last exit).
 * eec_encoder_pack may be called with the stem (sub0_w .. pe) and / or the heads (head_w, head_b) left NULL for an
 * encoder that is used through these entry points only.
 *   eec_encoder_group_forward: x [B, T', D] fp32, in place, through the layers_per_exit Conformer layers of `group`
 *       (= one torchaudio Conformer.forward(x, lengths), early_exit.py:603-615,627); key_len [B] int32 on the device:
 *       keys >= key_len[b] are masked (the caller applies the reference's length rule); production launch plan.
 *   eec_encoder_head_forward:  out [M, V] = log_softmax(x [M, D] . W_exit^T + b_exit)   (early_exit.py:629-631).
 *   eec_encoder_stem1_forward: x [B, T1, D] = Conv1d(k=3, s=2)(mel) + bias + pe[t1], T1 = (T - 3) / 2 + 1: the
 *       one-convolution stem of Early_zipformer (Conv1dSubampling_Zipformer, early_exit.py:80-95, 175-176); needs
 *       sub0_w, sub0_b and pe at pack time (sub1_* may be NULL). */
size_t eec_encoder_group_workspace_bytes(const eec_encoder* enc, int B, int Tq);
int eec_encoder_stem1_forward(eec_encoder* enc, const float* mel, int B, int T, float* x, void* stream);
int eec_encoder_group_forward(eec_encoder* enc, int group, float* x, const int32_t* key_len, int B, int Tq, int precision,
                              void* workspace, size_t workspace_bytes, void* stream);
int eec_encoder_head_forward(eec_encoder* enc, int exit, const float* x, int M, float* out, int precision, void* stream);

/* Measurement hook (no reference counterpart; the reference has no profiler hooks):
 * when enabled, every kernel launch of eec_encoder_forward is bracketed by hipEventRecord on the
 * launch stream; eec_encoder_profile_read synchronises the recorded events and returns the summed
 * milliseconds and launch counts per kernel class, index = EEC_KC_* (EEC_KC_CHAIN: the fused chain kernel of the
 * production plan; EEC_KC_FFN / _QKV / _DW_PW2 / _PROJ: the same steps as separate launches of the sub-step plan). */
enum { EEC_KC_STEM = 0, EEC_KC_FFN, EEC_KC_QKV, EEC_KC_ATTN, EEC_KC_PROJ_GLU, EEC_KC_PROJ, EEC_KC_DW_PW2, EEC_KC_HEAD, EEC_KC_CHAIN, EEC_KC_COUNT };
int eec_encoder_set_profiling(eec_encoder* enc, int enable, int max_launches);
int eec_encoder_profile_read(eec_encoder* enc, double* ms_by_class, long long* launches_by_class, int n_classes);

/* Replaces GreedyCTCDecoder.forward (util/beam_infer.py:9-24), batched over n_seq sequences:
 *   logp [n_seq, Tq, V] fp32 -> tokens [n_seq, Tq] int32 (first counts[s] entries valid), counts [n_seq]. */
int eec_greedy_ctc(const float* logp, int n_seq, int Tq, int V, int blank, int32_t* tokens, int32_t* counts,
                   void* stream);

/* Replaces the per-exit loss loop of the CTC training/eval step (train.py:53-65 with
 * nn.CTCLoss(blank, reduction='mean', zero_infinity=True), train.py:259), all exits and utterances in one launch:
 *   logp [E, B, T', V] fp32 log-probs (the encoder output as is; input length = T' for every utterance)
 *   targets [B, S] int64, target_len [B] int64 (device copies of the caller's tensors; len <= 255)
 *   nll_scratch [E*B] fp32, loss_per_exit [E] fp32 = batch mean of nll / max(len, 1); train.py's loss = their sum.
 * Input checking (nn.CTCLoss raises on these; a kernel cannot): a target_len outside [0, S] or a label outside [0, V)
 * among an utterance's first target_len labels makes that utterance's nll -- and the exit's loss -- NaN; NaN log-probs
 * propagate as NaN; only +inf (an infeasible alignment) is zeroed, as zero_infinity=True does. */
int eec_ctc_loss(const float* logp, const int64_t* targets, const int64_t* target_len, int E, int B, int Tq, int V, int S,
                 int blank, float* nll_scratch, float* loss_per_exit, void* stream);

/* Backward of the per-exit loss loop (train.py:60-68: loss.backward() through E nn.CTCLoss calls), first slice of the
 * training path: gradient with respect to the encoder's log-prob output.
 *   eec_ctc_loss_forward: as eec_ctc_loss, and additionally keeps every step's forward variables in `bwd_workspace`
 *       (eec_ctc_backward_workspace_bytes(E, B, T', S) bytes, 256-byte aligned device memory; nll [E*B] is an output
 *       the backward needs again).
 *   eec_ctc_loss_backward: dlogp [E, B, T', V] = d( sum_e grad_loss[e] * loss_e ) / d logp, what torch autograd returns
 *       for the same loop (for each lattice grad * (exp(logp) - state posteriors), zero for an infeasible lattice);
 *       consumes bwd_workspace (call once per forward).
 *   eec_logsoftmax_backward: grad_logits = grad_logp - exp(logp) * sum_c grad_logp  (rows of V <= 256 entries): the
 *       log-softmax half of the exit heads' backward (early_exit.py:629-631); the two plain GEMMs of the Linear's
 *       backward (dW = grad_logits^T . x, dx = grad_logits . W) are library GEMMs on the caller's side. */
size_t eec_ctc_backward_workspace_bytes(int E, int B, int Tq, int S);
int eec_ctc_loss_forward(const float* logp, const int64_t* targets, const int64_t* target_len, int E, int B, int Tq, int V, int S,
                         int blank, float* nll, float* loss_per_exit, void* bwd_workspace, void* stream);
int eec_ctc_loss_backward(const float* logp, const int64_t* targets, const int64_t* target_len, int E, int B, int Tq, int V, int S,
                          int blank, const float* nll, void* bwd_workspace, const float* grad_loss, float* dlogp, void* stream);
int eec_logsoftmax_backward(const float* logp, const float* grad_logp, int M, int V, float* grad_logits, void* stream);

/* The three CTC loss entries with per-utterance input lengths, what nn.CTCLoss takes as `input_lengths` (the reference fills them
 * with T': train.py:57-58).  Every argument the entries above share keeps its meaning; the new one:
 *   input_len [B] int32 on the device, in encoder frames (eec_encoder_lengths), shared by the E exits of an utterance and clamped:
 *       Tb = clamp(input_len[b], 0, T').  NULL: T' for every utterance -- the call IS the entry above, launch for launch.
 * Utterance b's lattices cover the frames t < Tb.  Frames at or past Tb are never read: no loss, no gradient and no zero depends
 * on what they hold, NaN included.  Tb = 0: nll is 0 for an empty target and +inf (infeasible: zeroed) for any other.  A target
 * that needs more than Tb frames is infeasible like one that needs more than T'.  The normalisation does not change:
 * loss_e = batch mean of nll / max(target_len, 1); like torch, nothing is divided by the input length.
 *   eec_ctc_loss_backward_len: dlogp is written in full -- the rows t >= Tb of every lattice as ZEROS, so a buffer that was never
 *       initialised is a complete gradient afterwards (eec_exit_distill_backward with accumulate != 0 may then add into it).
 * The forward / backward pair must be given the same input_len.  The workspace is still eec_ctc_backward_workspace_bytes(E, B, T', S)
 * bytes.  Sizes, the limits (target length <= 255; V <= 256 and V % 4 == 0 for the backward) and the errors are the entries' above. */
int eec_ctc_loss_len(const float* logp, const int64_t* targets, const int64_t* target_len, const int32_t* input_len, int E, int B,
                     int Tq, int V, int S, int blank, float* nll_scratch, float* loss_per_exit, void* stream);
int eec_ctc_loss_forward_len(const float* logp, const int64_t* targets, const int64_t* target_len, const int32_t* input_len, int E,
                             int B, int Tq, int V, int S, int blank, float* nll, float* loss_per_exit, void* bwd_workspace,
                             void* stream);
int eec_ctc_loss_backward_len(const float* logp, const int64_t* targets, const int64_t* target_len, const int32_t* input_len, int E,
                              int B, int Tq, int V, int S, int blank, const float* nll, void* bwd_workspace, const float* grad_loss,
                              float* dlogp, void* stream);

/* Self-distillation between exits: the second training recipe of a multi-exit network (the reference declares the flag
 * `--distill`, "whether to use knowledge distillation", and leaves it unimplemented: util/conf.py:48-57).  A student exit's frame
 * posteriors are pulled towards its teacher exit's by a temperature-softened KL term that is added to the per-exit CTC loss; it
 * is a second producer of the gradient with respect to the encoder output, next to eec_ctc_loss_backward.
 *   x [E, B, T, V] fp32: logits or log-probs; every row is normalised inside, so the result does not depend on a per-row shift
 *   frame_len [B] int32 on the device, or NULL for T everywhere (the reference's CTC input-length convention); clamped to [0, T]
 *   teacher [E] int32, a HOST array: teacher[e] = k makes exit k the teacher of exit e; -1: exit e is no student (loss 0).  A
 *       teacher may be shallower than its student and may itself be a student of another exit.
 *   tau > 0, the temperature
 * With p = softmax(x[k, b, t, :] / tau) and q = softmax(x[e, b, t, :] / tau), k = teacher[e]:
 *   kl[e, b] = sum_{t < len_b} sum_v p_v (log p_v - log q_v)
 *   loss[e]  = tau^2 * mean_b( kl[e, b] / max(len_b, 1) )
 *   d loss[e] / d x[e, b, t, v] = tau * (q_v - p_v) / (B * max(len_b, 1))    for t < len_b, else 0
 * The teacher is a constant: no gradient flows into x[k] from its students (mutual distillation is not offered).  A term with
 * p_v = 0 (an exact -inf teacher logit) is 0.  NaN logits propagate to the losses (and gradient rows) of the exits that read them
 * -- the row's own exit as a student, and its students -- and to nothing else; frames at or past len_b are not read.
 *   eec_exit_distill_forward: kl [E * B] and loss_per_exit [E]; workspace: eec_exit_distill_workspace_bytes(E, B, T) bytes of
 *       256-byte aligned device memory (the per-frame terms; 0 for a non-positive size).  Frames, then utterances, are added in
 *       index order without atomics: the losses are bit-reproducible from run to run.
 *   eec_exit_distill_backward: dx [E, B, T, V] = d( sum_e grad_loss[e] * loss[e] ) / dx, grad_loss [E] on the device.
 *       accumulate == 0: every element of dx is written (zeros on rows of exits that are no students or whose grad_loss is 0,
 *       and on frames at or past len_b).  accumulate != 0: the gradient is ADDED into dx -- eec_ctc_loss_backward's dlogp, so the
 *       two losses share one gradient buffer -- and those rows and frames are left untouched.
 * EEC_ERR_BAD_ARG, with a message, before anything is launched: a null pointer (frame_len may be NULL), a size below 1,
 * E > EEC_DISTILL_MAX_EXITS (a frame's rows of all exits are held in one wave's registers), V > 256 or V % 4 != 0 (a row is one
 * float4 per lane, as in the CTC gradient kernel), tau not a finite number above 0, teacher[e] == e or outside [-1, E).
 * EEC_ERR_WORKSPACE: a misaligned or short workspace. */
#define EEC_DISTILL_MAX_EXITS 16
size_t eec_exit_distill_workspace_bytes(int E, int B, int T);
int eec_exit_distill_forward(const float* x, const int32_t* frame_len, const int32_t* teacher, int E, int B, int T, int V, float tau,
                             float* kl, float* loss_per_exit, void* workspace, size_t workspace_bytes, void* stream);
int eec_exit_distill_backward(const float* x, const int32_t* frame_len, const int32_t* teacher, int E, int B, int T, int V, float tau,
                              const float* grad_loss, int accumulate, float* dx, void* stream);

/* Minimum word error rate (MWER) training of the CTC exits: the expected risk over an N-best list (Prabhavalkar et al. 2018), the
 * usual second stage after CTC training.  Every exit has its own list and its own error counts.  The reference has nothing like
 * it.  A third producer of the gradient with respect to the encoder output, next to eec_ctc_loss_backward and
 * eec_exit_distill_backward: N CTC lattices share one emission and their posteriors are folded into one gradient row.
 *   logp [E, B, T', V] fp32 log-probs (rows are log_softmax outputs)
 *   input_len [B] int32 on the device, or NULL for T' everywhere; Tb = clamp(input_len[b], 0, T'); frames at or past Tb are never read
 *   hyp [E, B, N, L] int32 tokens, hyp_len [E, B, N] int32 (-1: the entry is absent), risk [E, B, N] fp32: the caller's error count of
 *       that hypothesis (tokens, words, anything), `blank`
 * For lattice (e, b, i) with len = hyp_len[e, b, i] >= 0:
 *   ll[e, b, i] = log p_ctc(hyp[e, b, i, :len] | logp[e, b, :Tb]), the exact forward log-likelihood, divided by nothing: -inf when
 *       infeasible (too few frames, repeats included; Tb == 0 with len > 0), 0 for the empty hypothesis on zero frames; -inf for an
 *       absent entry.  The recursions run in log space with the log_add stated under eec_ctc_log_add: there is no range limit.
 *   gamma_i[t, v] = the posterior probability that an alignment of hypothesis i emits label v at frame t = d ll_i / d logp[e, b, t, v]
 * P = the present entries with a finite ll.  |P| == 0: loss_eb = 0 and the gradient rows are 0.  Otherwise
 *   phat_i = softmax over P of ll_i (the maximum subtracted; 0 outside P),  rbar = mean over P of risk (the common value itself
 *   when all risks of P are equal),  r_i = risk_i - rbar,
 *   loss_eb = sum_i phat_i r_i,   c_i = phat_i (r_i - loss_eb)      (sum_i c_i = 0; equal risks: loss and every c_i exactly 0)
 *       c_i is evaluated as phat_i sum_j phat_j (risk_i - risk_j): the same number, without the cancellation that leaves nothing
 *       of it when one hypothesis holds nearly all the mass
 *   d loss_eb / d logp[e, b, t, v] = sum_i c_i gamma_i[t, v] for t < Tb, 0 for t >= Tb
 * which, because the c_i add up to 0, is what torch autograd returns through F.ctc_loss (whose gradient folds the softmax in): it
 * adds into the buffer eec_ctc_loss_backward wrote.  loss[e] = mean_b loss_eb; dlogp = d( sum_e grad_loss[e] loss[e] ) / d logp.
 * Input only the device can see: a hyp_len outside [-1, min(L, 255)], or a label outside [0, V) or equal to blank among the first
 * len tokens, makes that entry's ll, its loss_eb and loss[e] NaN and nothing else (its list's gradient rows are zero rows).  NaN
 * log-probs a lattice reads make its ll NaN, and with it loss_eb, loss[e] and the gradient rows t < Tb of that (e, b), and reach no
 * other (e, b).  No input makes a kernel read out of bounds.
 * A call serves the utterances b0 .. b0 + nb - 1 of the batch (b0 = 0, nb = B: all of it), so that a caller can bound the
 * workspace -- the alphas of every lattice: eec_ctc_mwer_workspace_bytes(E, nb, T', N, L) bytes of 256-byte aligned device memory,
 * 64 P floats per lattice and frame, P = 2 / 4 / 8 for min(L, 255) <= 63 / 127 / 255.  All arrays are those of the whole batch.
 *   eec_ctc_hyp_logp: ll [E, B, N] alone -- the exact CTC score of an N-best list; no workspace.
 *   eec_ctc_mwer_forward: ll and loss_eb [E * B] of the chunk; loss [E] is written by the call whose chunk ends the batch
 *       (b0 + nb == B), from loss_eb of the whole batch in index order; leaves what the backward needs in the workspace.
 *   eec_ctc_mwer_backward: the rows of dlogp [E, B, T', V] of the chunk's utterances, from the workspace its forward left (read
 *       only); grad_loss [E] on the device.  accumulate == 0: every element of those rows is written; accumulate != 0: the
 *       gradient is ADDED into dlogp, and rows that would be written as zeros are left untouched, as in eec_exit_distill_backward.
 * Reproducibility: no floating-point atomics; the hypotheses of a list are folded in index order, the occurrences of a label in a
 * hypothesis in position order; two runs return the same bits, a call on a slice of the exits returns the bits of the whole call,
 * and so does, for ll and loss_eb, a call on a slice of the batch or on a chunk (loss and dlogp carry 1 / B).
 * EEC_ERR_BAD_ARG, with a message, before anything is launched: N outside [1, EEC_MWER_MAX_NBEST]; a null pointer (input_len may
 * be NULL); E, B, nb, T', V or L below 1; a chunk outside the batch; blank outside [0, V); for the backward V > 256 or V % 4 != 0
 * (a gradient row is one float4 per lane) or a dlogp that is not 16-byte aligned.  EEC_ERR_WORKSPACE: a short or misaligned
 * workspace. */
#define EEC_MWER_MAX_NBEST 16
size_t eec_ctc_mwer_workspace_bytes(int E, int B, int Tq, int N, int L);
int eec_ctc_hyp_logp(const float* logp, const int32_t* input_len, const int32_t* hyp, const int32_t* hyp_len, int E, int B, int Tq, int V,
                     int N, int L, int blank, float* ll, void* stream);
int eec_ctc_mwer_forward(const float* logp, const int32_t* input_len, const int32_t* hyp, const int32_t* hyp_len, const float* risk, int E,
                         int B, int b0, int nb, int Tq, int V, int N, int L, int blank, float* ll, float* loss_eb, float* loss,
                         void* workspace, size_t workspace_bytes, void* stream);
int eec_ctc_mwer_backward(const float* logp, const int32_t* input_len, const int32_t* hyp, const int32_t* hyp_len, int E, int B, int b0,
                          int nb, int Tq, int V, int N, int L, int blank, const void* workspace, size_t workspace_bytes,
                          const float* grad_loss, int accumulate, float* dlogp, void* stream);

/* Adaptive inference: the statistics an early-exit model chooses an utterance's exit by (average frame entropy, average frame
 * confidence, log-probability of the greedy CTC path), and the routing of a batch by one of them.
 *   x [E, B, T, V] fp32: logits or log-probs; every row is normalised inside: lp_v = x_v - lse(x), p_v = exp(lp_v)
 *   frame_len [B] int32 on the device, or NULL for T everywhere; len_b = clamp(frame_len[b], 0, T), n_b = max(len_b, 1)
 *   stats [3, E, B] fp32:
 *     stats[0][e][b] = entropy     = (1 / n_b) sum_{t < len_b} -sum_v p_v lp_v     in nats; a term with p_v = 0 is 0
 *     stats[1][e][b] = confidence  = (1 / n_b) sum_{t < len_b} max_v p_v
 *     stats[2][e][b] = greedy_logp = sum_{t < len_b} max_v lp_v                     NOT divided by the length
 * An utterance without frames gives 0 / 0 / 0.  Frames at or past len_b are never read: a NaN there reaches nothing.  A NaN inside
 * the valid frames reaches the three statistics of that (e, b) and nothing else.  The per-frame terms go to the workspace
 * (eec_exit_stats_workspace_bytes(E, B, T) bytes of 256-byte aligned device memory; 0 for a non-positive size) and an utterance's
 * frames are added in index order without atomics: the statistics are bit-reproducible from run to run, and a call on a slice of
 * the exits or of the batch returns the bits of the whole call.
 * EEC_ERR_BAD_ARG, with a message, before anything is launched: a null pointer (frame_len may be NULL), a size below 1,
 * E > EEC_EXIT_STATS_MAX_EXITS, V > 256 or V % 4 != 0 (a row is one float4 per lane), B * T or 3 * E * B above 2^31 - 1.
 * EEC_ERR_WORKSPACE: a misaligned or short workspace.
 *
 * eec_exit_route: row i of score [n] LEAVES when score[i] < threshold (higher_is_better != 0: when score[i] > threshold); a tie
 * stays, a NaN score never leaves; force_all != 0: every row leaves, whatever it scores.  leave_idx and stay_idx [n] int32 receive
 * the stable partition of 0 .. n-1 -- the leavers, and the stayers, each in ascending order; only the first counts[1] entries of
 * leave_idx and the first counts[0] of stay_idx are written -- and counts [2] int32 = {stayers, leavers}.  One launch for any
 * n >= 1.  EEC_ERR_BAD_ARG: a null pointer, n < 1, a NaN threshold (without force_all). */
#define EEC_EXIT_STATS_MAX_EXITS 16
size_t eec_exit_stats_workspace_bytes(int E, int B, int T);
int eec_exit_stats(const float* x, const int32_t* frame_len, int E, int B, int T, int V, float* stats, void* workspace,
                   size_t workspace_bytes, void* stream);
int eec_exit_route(const float* score, int n, float threshold, int higher_is_better, int force_all, int32_t* stay_idx,
                   int32_t* leave_idx, int32_t* counts, void* stream);

/* CTC prefix beam search: replaces BeamInference.ctc_cuda_predict (util/beam_infer.py:79-80,102-112:
 * torchaudio cuda_ctc_decoder(tokens, nbest=1, beam_size=10, blank_skip_threshold=0.95) on the log-probs of one exit,
 * input length T' for every utterance), batched over n_seq sequences.  That decoder is third-party CUDA code outside the
 * reference tree: this is the published algorithm (prefix beam search without a language model; oracle/ctc_beam_ref.py),
 * parity with torchaudio's tie-breaking is unpinned.
 *   logp [n_seq, T', V] fp32 log-probs, blank label `blank` (0 in the reference), V <= 256, beam_size <= 16
 *   blank_skip_threshold in (0, 1): a frame with p(blank) above it is taken as a blank frame without expansion; >= 1 disables
 *   workspace: eec_ctc_beam_workspace_bytes(n_seq, T') bytes (back-pointers)
 *   tokens [n_seq, T'] int32 (first counts[s] valid), counts [n_seq], scores [n_seq] = log p of the best prefix. */
size_t eec_ctc_beam_workspace_bytes(int n_seq, int Tq);
int eec_ctc_beam_decode(const float* logp, int n_seq, int Tq, int V, int blank, int beam_size, float blank_skip_threshold,
                        void* workspace, int32_t* tokens, int32_t* counts, float* scores, void* stream);
/* What torchaudio's CUDA decoder does with a frame above blank_skip_threshold is not visible from the reference (third-party,
 * absent): eec_ctc_beam_decode takes the frame as a BLANK frame (every prefix's mass moves to "ending in blank": a label
 * repeated across the frame stays a repeat, "a _ a" -> "aa").  skip_drops_frame != 0 selects the other reading: the frame is
 * DROPPED, as if the sequence were one frame shorter (the repeat collapses, "a _ a" -> "a"; scores exclude the frame).  Both
 * are tested against the CPU statement (oracle/ctc_beam_ref.py); the default stays the first until a torchaudio vector pins it. */
int eec_ctc_beam_decode_ex(const float* logp, int n_seq, int Tq, int V, int blank, int beam_size, float blank_skip_threshold,
                           int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts, float* scores, void* stream);

/* The greedy decoder and the prefix beam search with per-sequence input lengths (torchaudio's cuda_ctc_decoder takes them as
 * `encoder_out_lens`; the reference fills them with T': util/beam_infer.py:106-107):
 *   em_len [n_seq] int32 on the device, clamped: sequence s is its first Ts = clamp(em_len[s], 0, T') frames, exactly as if
 *       logp[s, :Ts] had been decoded alone; frames at or past Ts are never read.  NULL: T' for every sequence -- what
 *       eec_greedy_ctc / eec_ctc_beam_decode / eec_ctc_beam_decode_ex pass: they are these with NULL.
 * Ts = 0 gives counts[s] = 0, and scores[s] = 0 (the empty prefix, log 1).  The rows of `tokens` stay T' apart and the workspace
 * is still eec_ctc_beam_workspace_bytes(n_seq, T') bytes.  skip_drops_frame as in eec_ctc_beam_decode_ex; errors as the entries above. */
int eec_greedy_ctc_len(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int32_t* tokens,
                       int32_t* counts, void* stream);
int eec_ctc_beam_decode_len(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                            float blank_skip_threshold, int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts,
                            float* scores, void* stream);

/* N-best from the prefix beam search (csrc/ctc_beam.hip: the kernel of eec_ctc_beam_decode_len, which has a second end for this
 * entry).  The search is exactly that of eec_ctc_beam_decode_len -- the same kernel body, candidate ids and
 * tie rules, em_len (may be NULL), blank_skip_threshold and skip_drops_frame as there -- and the final beam, which that entry
 * drops after its best prefix, is returned: its prefixes are ranked by total log-probability log_add(p_blank, p_non_blank),
 * ties to the lower beam index (the order oracle/ctc_beam_ref.py returns with return_beams=True), and the first
 * n_hyp[s] = min(nbest, live beams) of them are traced back.  1 <= nbest <= beam_size <= 16.
 *   tokens [n_seq][nbest][T'] int32 (first counts[s][r] valid), counts [n_seq][nbest], scores [n_seq][nbest], n_hyp [n_seq]
 *   hypothesis 0 is what eec_ctc_beam_decode_len returns; present hypotheses are distinct prefixes with non-increasing scores;
 *   absent ones (r >= n_hyp[s]) have count 0 and score -inf; Ts = 0 gives one hypothesis, the empty prefix with score 0.
 *   workspace: eec_ctc_beam_workspace_bytes(n_seq, T') bytes.
 * The list is the beam the search ends with, not the N most probable label sequences: a prefix pruned on the way is gone.
 * EEC_ERR_BAD_ARG: a null pointer (em_len may be NULL), n_seq or T' below 1, nbest outside [1, beam_size];
 * EEC_ERR_UNSUPPORTED: V, beam_size or blank outside the limits above. */
int eec_ctc_beam_decode_nbest(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                              float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens,
                              int32_t* counts, float* scores, int32_t* n_hyp, void* stream);

/* Lexicon-constrained CTC beam search with N-best: replaces the decoder behind BeamInference.ctc_predict / ctc_predict_ /
 * beam_predict (util/beam_infer.py:51-65, 85-126): torchaudio ctc_decoder(lexicon, tokens, nbest=N_BEST, log_add=False, beam_size,
 * word_score=w_ins, blank_token="@", sil_token="<pad>") with lm=None, unk_score=-inf, for n_seq sequences in one launch
 * (csrc/ctc_lexbeam.hip: one workgroup per sequence).  That decoder (flashlight-text) is third-party code outside the reference
 * tree and is not installed: this is the published algorithm -- token-trie beam search under CTC, Viterbi merging, no language
 * model -- as stated here; tests/lexbeam_cases.py is its plain-Python statement.  PARITY WITH THE THIRD-PARTY DECODER IS UNPINNED.
 * A back-off n-gram word model joins through eec_ctc_lexbeam_lm_decode, stated after this entry; without one nothing below changes.
 * LM look-ahead (max trie smearing) joins through eec_ctc_lexbeam_lm_smear_decode, stated after that one.
 * log_add=True (the reference's character-lexicon branch, util/beam_infer.py:66-75) is eec_ctc_lexbeam_logadd_decode, stated last:
 * only the Merging rule below changes.
 * Out of scope: unknown-word scores other than through the model's <unk>, binary KenLM files, beams over 64 (beams of 17 to 64: eec_ctc_lexbeam_wide_decode, stated after the log-add entry).
 *
 * Lexicon: n_words spellings, each a non-empty sequence of token ids in [0, V), none of them `blank` or (when given) `sil`.  The
 *   trie's root is node 0.  A node "ends word w" when w is the FIRST word in file order with that spelling (later duplicates are
 *   unreachable; the packer counts them in n_shadowed).  A node may both end a word and have children.
 * Hypothesis: (node, tok, pb, hist, score) -- tok the label of the last frame, pb whether that frame was blank, hist the word
 *   sequence so far, score fp32.  The start is (0, -1, true, (), 0.0f).
 * Frame t, log-probs e[0..V), the beam in rank order i = 0..n-1.  Hypothesis i generates these candidates; every score is
 *   computed in fp32 in exactly the order written:
 *     blank            always                                       (node, blank, true, hist)   score + e[blank]           c = blank, w = 0
 *     repeat           !pb and tok >= 0                             (node, tok, false, hist)    score + e[tok], and when tok == sil
 *                                                                                               then + sil_score           c = tok,   w = 0
 *     child, in-word   every child edge (c -> y) of node with
 *                      c != tok or pb; y has children               (y, c, false, hist)         score + e[c]               w = 0
 *     child, word end  the same edge; y ends word wd                (0, c, false, hist + wd)    (score + e[c]) + word_score  w = 1
 *     sil              node == 0, sil >= 0, and sil != tok or pb    (0, sil, false, hist)       (score + e[sil]) + sil_score  c = sil, w = 0
 *   An edge whose node both has children and ends a word emits both child candidates.  After a word ends, its last token may
 *   repeat across frames through the repeat rule (ordinary CTC; a stated choice, the third-party code cannot be consulted).
 *   Candidate id = (2 * c + w) * 16 + i: unique within a frame.
 *   Merging: candidates with the same (node, tok, pb, hist) merge; the higher score survives, on equal scores the lower id; the
 *   survivor keeps its own id and back-pointer.  (All members of a merge share the frame label c.)
 *   Dropping: a candidate whose score is not > -inf is dropped (-inf and NaN).
 *   Pruning: with best the highest score and beam_threshold finite, only candidates with score >= (float)(best - beam_threshold)
 *   stay.  The new beam is the first beam_size candidates by descending score, then ascending id; that order is the next frame's
 *   rank.  If nothing survives, the sequence ends with no hypothesis.
 * End, after frame em_len[s] - 1: the complete hypotheses are those with node == 0 (an empty hist is a legal, empty transcript),
 *   returned best first -- by score, then rank -- up to nbest; n_hyp[s] is how many.  It is 0 when none is complete, when em_len[s]
 *   is outside [1, T'], or when a frame left no candidate.
 * Per hypothesis: its words; its collapsed label sequence (blank frames dropped, runs collapsed, sil included: torchaudio's
 *   CTCHypothesis.tokens); the first frame of each such label (timesteps); its score.
 * hist identity on the device is a chained 64-bit hash (a collision is not handled).  In this entry and the two that follow there
 * are no reductions and no log / exp in the arithmetic: scores are bit-identical to a statement that keeps fp32 and the written
 * order of additions.  (eec_ctc_lexbeam_logadd_decode adds one function, log_add, itself a stated sequence of fp32 operations.)
 *
 * eec_ctc_trie_pack is HOST code and needs no device:
 *   spellings [offsets[n_words]] int32 token ids, flat; offsets [n_words + 1] int64, offsets[0] = 0, strictly ascending
 *   sil: -1 = none.  image: image_bytes >= eec_ctc_trie_pack_bytes(n_words, offsets[n_words]) bytes of host memory, 8-byte
 *       aligned; the caller copies it to the device (8-byte aligned) and passes it as `trie`.
 *   n_nodes, n_shadowed: NULL or where the node count and the number of unreachable duplicate spellings are written
 *   image layout, int32 units: header[16] = {magic, n_nodes, n_edges = n_nodes - 1, V, blank, sil, child_begin offset, child token
 *       offset, word_of offset, total dwords, n_words, n_shadowed, 0..};  child_begin [n_nodes + 1]: the edges of node n are
 *       child_begin[n] .. child_begin[n + 1];  child tokens: one BYTE per edge (padded to a dword), ascending within a node;
 *       word_of [n_nodes]: the word a node ends, or -1.  Nodes are numbered breadth-first, children in token order, so that the
 *       child reached by edge k is node k + 1: an edge needs no target.
 *   eec_ctc_trie_pack_bytes is non-decreasing in each argument (it sizes the worst case, one node per token); 0 for n_words <= 0,
 *       total_tokens < n_words, or an image of 2^31 dwords or more.
 *   EEC_ERR_BAD_ARG: a null pointer (spellings, offsets, image), n_words <= 0, V < 2, blank / sil outside their ranges or equal,
 *   offsets not ascending from 0, an empty spelling, a token outside [0, V) or equal to blank / sil.  EEC_ERR_UNSUPPORTED: V > 256.
 *   EEC_ERR_WORKSPACE: image_bytes too small.
 *
 * eec_ctc_lexbeam_decode:
 *   logp [n_seq, T', V] fp32 log-probs; em_len [n_seq] int32 frames of every sequence, or NULL = T' for all
 *   trie: the image on the device; blank, sil (-1 none): must be the values it was packed with, as must V
 *   beam_size 1..16, nbest 1..beam_size; word_score, sil_score; beam_threshold: +inf (any non-finite value) disables
 *   words [n_seq][nbest][max_words] int32 word indices (file order); word_count [n_seq][nbest] the TRUE count, even above
 *       max_words (the first max_words words are written; max_words = T' is always enough)
 *   tokens, timesteps [n_seq][nbest][T'] int32 (timesteps may be NULL); token_count, scores [n_seq][nbest]; n_hyp [n_seq]
 *   Absent hypotheses have score -inf and counts 0; entries past a hypothesis' counts are -1.
 *   workspace: eec_ctc_lexbeam_workspace_bytes(n_seq, T', beam_size) bytes, 8-byte aligned: the back-pointers.
 * EEC_ERR_BAD_ARG: a null required pointer, n_seq < 0, T' < 1, max_words < 1, blank / sil outside their ranges or equal, a
 * misaligned image or workspace; n_seq == 0 is a successful no-op.  EEC_ERR_UNSUPPORTED: V > 256, V < 2, beam_size outside 1..16,
 * nbest outside 1..beam_size.  EEC_ERR_WORKSPACE: workspace_bytes too small.  All checked before any device work.  A trie whose
 * header does not carry the call's V, blank and sil gives n_hyp = 0 for every sequence and nothing else of it is read.
 * One kernel on `stream`; no allocation, no synchronisation; graph-capturable; results are bit-identical run to run. */
size_t eec_ctc_trie_pack_bytes(int n_words, int64_t total_tokens);
int eec_ctc_trie_pack(const int32_t* spellings, const int64_t* offsets, int n_words, int V, int blank, int sil, void* image,
                      size_t image_bytes, int32_t* n_nodes, int32_t* n_shadowed);
size_t eec_ctc_lexbeam_workspace_bytes(int n_seq, int Tq, int beam_size);
int eec_ctc_lexbeam_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                           int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                           int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                           int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream);

/* The same search with a back-off n-gram word model: the reference's ctc_decoder(lexicon=..., lm="4gram_small.arpa.lm" / "lm.bin",
 * lm_weight=LM_WEIGHT) (util/beam_infer.py:39-78).  The model is what an ARPA file states, its log10 values kept as they are (what
 * KenLM's query interface returns, so the reference's LM_WEIGHT constants carry over); tests/lexbeam_lm_cases.py is the plain-Python
 * statement.  PARITY WITH THE THIRD-PARTY DECODER IS UNPINNED, as above.
 *
 * Model: n-grams (w1 .. wn), n <= order <= 5, over LM words 0 .. W - 1, each with logp and backoff (fp32).  Every LM word has a
 *   unigram; the prefix (w1 .. wn-1) of every n-gram is an (n-1)-gram of the model (prefix-closed; a suffix may be absent).
 *   lm_word(w): the LM word of lexicon word w -- the model's <unk> where the model lacks w.
 * LM state: an n-gram of the model (a node of the image), the empty one included.  A hypothesis carries one; the start hypothesis
 *   carries <s>'s unigram, or the empty n-gram when the model has no <s>.
 * Scoring LM word v from state s, fp32 in the written order:
 *     acc = 0
 *     loop:  x = the n-gram s + v
 *            x is in the model  -> acc = acc + logp[x]; stop
 *            otherwise          -> acc = acc + backoff[s]; s = suffix[s]
 *   suffix[s] is the longest proper suffix of s that is in the model.  The empty n-gram always finds v's unigram.  The state after
 *   the hit is x when x is shorter than `order`, else suffix[x].
 * Word-end candidate: ((score + e[c]) + word_score) + lm_weight * acc with acc for lm_word(wd) from the hypothesis' state; the
 *   product is rounded on its own and then added (no fused multiply-add).  The new hypothesis carries the state after the hit;
 *   every other candidate keeps its parent's.  Merging is still on (node, tok, pb, hist): the history determines the state.
 *   Dropping, pruning, candidate ids and the other candidates are as above.
 * End: when the model has </s>, every complete hypothesis' final score is score + lm_weight * acc with acc for </s> from its state
 *   (formed the same way); otherwise its score.  The complete hypotheses are ordered by (final score descending, beam rank
 *   ascending); the first nbest are returned, `scores` holds the final scores.
 *
 * eec_ngram_pack is HOST code and needs no device:
 *   order 1..5; counts [order] int64: n-grams per order, counts[0] = W > 0
 *   words [order] pointers: words[n-1] is [counts[n-1] * n] int32 LM word ids, n per n-gram; the unigrams are a permutation of
 *       0 .. W - 1.  logp, backoff [order] pointers to [counts[n-1]] fp32 each (0 where the file has no back-off).
 *   word_map [lex_words] int32: lm_word of every lexicon word (file order of the trie's lexicon)
 *   bos_word, eos_word: the LM words of <s> and </s>, or -1
 *   image: image_bytes >= eec_ngram_pack_bytes(order, counts, lex_words) bytes of host memory, 8-byte aligned; n_nodes: NULL or
 *       where the node count (1 + all n-grams) is written
 *   image layout, int32 units: header[16] = {magic "EECN", order, n_nodes, n_edges = n_nodes - 1, W, lex_words, <s> node (0: the
 *       root), </s> word (-1: none), first node of depth `order`, child_begin offset, edge word offset, logp offset, backoff offset,
 *       suffix offset, word_map offset, total dwords};  child_begin [n_nodes + 1]: the edges of node n are child_begin[n] ..
 *       child_begin[n + 1];  edge words [n_edges] int32, ascending within a node;  logp, backoff [n_nodes] fp32 (0 for the root);
 *       suffix [n_nodes] int32;  word_map [lex_words].  Node 0 is the empty n-gram.  Nodes are numbered breadth-first, children in
 *       word order, so that the child reached by edge k is node k + 1 and the unigram of LM word v is node v + 1; a lookup below any
 *       other node is a binary search over its edge range.  A node at or past header[8] has the full order.
 *   eec_ngram_pack_bytes: 0 for an order outside 1..5, counts NULL or negative, counts[0] <= 0, lex_words <= 0, or an image of
 *       2^31 dwords or more.
 *   EEC_ERR_BAD_ARG: a null pointer, lex_words <= 0, no unigram, a word id outside [0, W), unigrams that are no permutation, an
 *   n-gram whose prefix is absent, a duplicate n-gram, a non-finite value, bos_word / eos_word / a word_map entry that is no LM word.
 *   EEC_ERR_UNSUPPORTED: an order outside 1..5, an image past 2^31 dwords.  EEC_ERR_WORKSPACE: image_bytes too small.
 *
 * eec_ctc_lexbeam_lm_decode: eec_ctc_lexbeam_decode's arguments, then lm: the model image on the device (8-byte aligned), and
 *   lm_weight.  The same workspace.  EEC_ERR_BAD_ARG also for a null lm or a non-finite lm_weight, checked before any device work.
 *   A model whose header does not carry the magic and the trie's n_words gives n_hyp = 0 for every sequence, as a foreign trie does.
 * One kernel on `stream`; no allocation, no synchronisation; graph-capturable; results are bit-identical run to run. */
size_t eec_ngram_pack_bytes(int order, const int64_t* counts, int lex_words);
int eec_ngram_pack(int order, const int64_t* counts, const int32_t* const* words, const float* const* logp, const float* const* backoff,
                   const int32_t* word_map, int lex_words, int bos_word, int eos_word, void* image, size_t image_bytes, int32_t* n_nodes);
int eec_ctc_lexbeam_lm_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                              int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                              int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                              int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm, float lm_weight);

/* The same search with the model AND LM look-ahead by max trie smearing.  eec_ctc_lexbeam_lm_decode asks the model only where a
 * word ends; between word ends the beam is ordered by acoustic score alone.  The published lexicon decoder inserts every lexicon
 * word into the token trie with the model's score for it from the start state and smears the trie (torchaudio's ctc_decoder builds
 * its trie this way and smears it with the MAX mode, always): every node carries the maximum of those scores over the words at or
 * below it, a step into a node is charged the increase of that maximum, a word end replaces the advance payment by the true
 * conditional score.  For a complete hypothesis the payments telescope to exactly the word scores paid without smearing, so only
 * pruning changes.  tests/lexbeam_smear_cases.py is the plain-Python statement.  PARITY WITH THE THIRD-PARTY DECODER IS UNPINNED.
 *
 * Word score: for a lexicon word w that ends a trie node (the first word in file order with that spelling; shadowed duplicates do
 *   not count), u(w) is `acc` of the walk above for lm_word(w) from the start state (<s>'s unigram, or the empty n-gram when the
 *   model has no <s>): fp32, the additions in the walk's order.
 * Smear table: smax[n], n >= 1, is the maximum of u(w) over the words that end at node n or at any node below it; smax[0] = 0.  A
 *   maximum involves no rounding.  Every node but the root ends a word or has children and the packer refuses non-finite model
 *   values, so every entry is finite.
 * Search: eec_ctc_lexbeam_lm_decode's with two candidate rules changed; pmax = smax[node] of the hypothesis (0 at the root):
 *     child, in-word   (edge c -> y, y has children)   (score + e[c]) + lm_weight * (smax[y] - pmax)
 *     child, word end  (y ends wd)                     ((score + e[c]) + word_score) + lm_weight * (acc - pmax)
 *   fp32 in the written order: the difference is rounded, the product is rounded on its own, then added (no fused multiply-add).
 *   A node that ends a word and has children emits both.  Nothing else differs: blank, repeat, sil, ids, merging keys, dropping,
 *   the threshold, the </s> term and its re-ordering, the outputs.  A complete hypothesis sits at the root: no payment is
 *   outstanding at the end.  With lm_weight = 0, or a model whose word scores are all equal, every term is a zero and the results
 *   equal eec_ctc_lexbeam_lm_decode's bitwise.
 *
 * eec_ctc_trie_smear is HOST code and needs no device:
 *   trie_image, lm_image: HOST copies of the two packed images (8-byte aligned), the model packed for this trie's lexicon
 *   table: table_bytes >= eec_ctc_trie_smear_bytes(the trie's n_nodes) bytes of host memory, 8-byte aligned; the caller copies it
 *       to the device (8-byte aligned) and passes it as `smear`
 *   table layout, int32 units: header[4] = {magic "EECS", the trie's n_nodes, the lexicon's word count, 0}, then smax [n_nodes] fp32,
 *       padded to a multiple of 8 bytes.  One descending sweep over the nodes fills it (children have higher numbers than their
 *       parent); the walk is the function the kernel runs, compiled for the host: the same sequence of fp32 additions.
 *   eec_ctc_trie_smear_bytes: 0 for n_nodes < 1.
 *   EEC_ERR_BAD_ARG: a null or misaligned pointer, an image without its magic, a model packed for another lexicon (its header's
 *   lex_words is not the trie's n_words), a trie image whose nodes are not what the packer writes.  EEC_ERR_WORKSPACE: table_bytes
 *   too small.
 *
 * eec_ctc_lexbeam_lm_smear_decode: eec_ctc_lexbeam_lm_decode's arguments, then smear: the table on the device.  The same workspace.
 *   EEC_ERR_BAD_ARG also for a null or misaligned smear, checked before any device work.  A table whose header does not carry its
 *   magic and the trie's n_nodes gives n_hyp = 0 for every sequence, as a foreign trie or model does.
 * One kernel on `stream`; no allocation, no synchronisation; graph-capturable; results are bit-identical run to run. */
size_t eec_ctc_trie_smear_bytes(int n_nodes);
int eec_ctc_trie_smear(const void* trie_image, const void* lm_image, void* table, size_t table_bytes);
int eec_ctc_lexbeam_lm_smear_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                    int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                    int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps,
                                    float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm,
                                    float lm_weight, const void* smear);

/* The same search with LOG-ADD merging: torchaudio's ctc_decoder(..., log_add=True), which the reference switches on for its
 * character-lexicon decoder behind beam_predict (util/beam_infer.py:66-75, 85-90).  A hypothesis then scores the sum over the
 * alignments merged into it, not the best single one.  It works without a model (lm == NULL: eec_ctc_lexbeam_decode's search), with
 * the model (smear == NULL: eec_ctc_lexbeam_lm_decode's) and with the model plus max smearing (eec_ctc_lexbeam_lm_smear_decode's);
 * of those statements only the Merging rule changes.  tests/lexbeam_logadd_cases.py is the plain-Python statement.  PARITY WITH THE
 * THIRD-PARTY DECODER IS UNPINNED, as above.
 *
 * Merging (log-add): the candidates of a frame with the same (node, tok, pb, hist) form a group (dropped candidates -- score not
 *   > -inf -- are no members: Dropping comes first).  Every member carries its raw score and an accumulator acc, acc = raw at first.
 *   With the members in ascending id order m_0 .. m_{k-1}, all alive:
 *       for p = 0 .. k-1:  for q = p+1 .. k-1:  if m_p and m_q are both alive:
 *           sum = log_add(acc_p, acc_q)
 *           if raw_q > raw_p:  acc_q = sum, m_p is eliminated      (m_p takes no part in any later pair)
 *           else:              acc_p = sum, m_q is eliminated
 *   This fixes the fold order (fp32 log_add is not associative).  The raw scores alone decide who wins a pair, so the survivor is
 *   the member with the highest raw score, the lowest id among equals -- the Viterbi survivor --, and it keeps its own id and
 *   back-pointer; its score becomes its acc, the log of the sum of the members' probabilities.  A group of one keeps its score.
 *   The LM and smearing terms enter every member's raw score before the merge, exactly where they enter without log-add.
 *   Pruning, the beam order, the next frame's scores, the </s> term and the final order all work on merged scores.
 *
 * log_add(a, b), fp32, every operation rounded on its own (no fused multiply-add), in this order:
 *     hi = a if a > b else b;  lo = the other;  d = lo - hi
 *     if not d > -17.34375:  return hi                        (the cutoff: exp(d) < 2^-25; also taken when d is NaN)
 *     n = rint(d * 1.44269502)                                 (round to nearest, ties to even; n in -25 .. 0)
 *     r = d - n * 0.693145751953125;  r = r - n * 1.42860677e-06
 *     p = 1.98412701e-04;  then p = p * r + c for c = 1.38888892e-03, 8.33333377e-03, 4.16666679e-02, 0.166666672, 0.5, 1, 1
 *     x = ldexp(p, n)                                          (exp(d); exact scaling)
 *     u = 1 + x;  halved = u > 1.41421354;  if halved: u = u * 0.5
 *     m = u - 1
 *     q = 0.0657233745;  then q = q * m + c for c = -0.116206668, 0.119458839, -0.12420819, 0.142122895, -0.166665554,
 *         0.20002535, -0.250000626, 0.333333015, -0.5, 1
 *     s = m * q;  if halved: s = s + 0.693147182
 *     return hi + s
 *   Each decimal constant is the fp32 value nearest to it.  No libm transcendental, no division, no reciprocal: add, subtract,
 *   multiply, compare, rint, ldexp are exact IEEE operations, so the device, the host and a numpy float32 restatement give the same
 *   bits.  The function is symmetric in its arguments bit for bit.  a == b: d = 0, n = 0, x = 1, u = 2 is halved, m = 0, the result
 *   is hi + 0.693147182.  -inf and NaN never reach it from the search (they are dropped first).
 *   Accuracy: s against float64 log1p(exp(d)) over 6 000 001 equally spaced d in [-17.34375, 0], both ends included (at the cutoff
 *   itself s = 0): the maximum absolute deviation measured is 9.9e-8; the bound the tests assert is 1.2e-7, well below 1e-6 -- half
 *   an fp32 ulp of a score of magnitude 16 --, so the function's error stays below the rounding of the addition that follows it.
 *
 * eec_ctc_lexbeam_logadd_decode: eec_ctc_lexbeam_lm_smear_decode's arguments in the same order.  lm == NULL: no model (lm_weight
 *   and smear unused; smear != NULL without lm is EEC_ERR_BAD_ARG); lm != NULL, smear == NULL: the model; both: the model and
 *   smearing.  Everything else is as the three entries: the same checks before any device work, the same workspace, one kernel on
 *   `stream`, no allocation, no synchronisation, graph-capturable, results bit-identical run to run.
 * eec_ctc_log_add_host is HOST code and needs no device: log_add(a, b), the very function the kernel calls.
 * eec_ctc_log_add: out[k] = log_add(a[k], b[k]) for k < n on the device (a, b, out: n fp32 each; out may alias a or b), one kernel on
 *   `stream` -- for holding the function to its statement, and for combining scores (an N-best list's posterior mass, say).
 *   EEC_ERR_BAD_ARG: n < 0, or a null pointer with n > 0; n == 0 is a successful no-op. */
int eec_ctc_lexbeam_logadd_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                  int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                  int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps,
                                  float* scores, int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm,
                                  float lm_weight, const void* smear);
float eec_ctc_log_add_host(float a, float b);
int eec_ctc_log_add(const float* a, const float* b, float* out, int n, void* stream);

/* The same search for WIDE beams, 17 to 64 (any beam of 1 to 64 is served): what a word-level n-gram search over the full lexicon is
 * normally run with (torchaudio's default for this decoder is 50).  One entry covers every mode, as eec_ctc_lexbeam_logadd_decode
 * does, and log_add is an argument.  csrc/ctc_lexbeam_wide.hip; tests/lexbeam_wide_cases.py is the plain-Python statement.  PARITY
 * WITH THE THIRD-PARTY DECODER IS UNPINNED, as above.
 *
 * Search: the one stated for eec_ctc_lexbeam_decode and its three successors, word for word -- candidates, the order of the fp32
 *   operations, dropping, merging, pruning, the LM walk, lm_weight * acc without contraction, smearing, the stated log_add and its
 *   fold order, the </s> term and the final order -- with one line changed:
 *     Candidate id = (2 * c + w) * 64 + i: unique within a frame for i < 64.
 *   That is the same lexicographic order on (label, word-end flag, beam rank) as the narrow id, so for every beam_size of 16 or less
 *   this entry returns exactly what the narrow entries return, bit for bit.
 *   beam_size 1..64, nbest 1..beam_size.
 *
 * eec_ctc_lexbeam_wide_decode: eec_ctc_lexbeam_decode's arguments in order, then lm, lm_weight, smear, log_add.
 *   lm == NULL: the model-free search (lm_weight is ignored; smear must be NULL: smear != NULL without lm is EEC_ERR_BAD_ARG);
 *   lm != NULL, smear == NULL: the model; both: the model and max smearing.  log_add != 0: log-add merging, else Viterbi merging.
 *   workspace: eec_ctc_lexbeam_wide_workspace_bytes(n_seq, T', beam_size) = n_seq * T' * beam_size * 8 bytes, 8-byte aligned: the
 *       back-pointers, 8 bytes per (frame, rank); the kernel uses no other global scratch (0 for an argument <= 0; non-decreasing in
 *       each argument).
 *   Checks, codes and their order are the narrow entries', all before any device work: EEC_ERR_UNSUPPORTED for beam_size outside
 *   1..64, nbest outside 1..beam_size, V outside 2..256; EEC_ERR_BAD_ARG for a null required pointer, a misaligned trie / lm / smear /
 *   workspace, a non-finite lm_weight with a model, smear without lm, n_seq < 0, T' < 1, max_words < 1, blank / sil outside their
 *   ranges or equal; EEC_ERR_WORKSPACE for a short workspace; n_seq == 0 is a successful no-op.  Foreign images give n_hyp = 0.
 * One kernel on `stream`; no allocation, no synchronisation; graph-capturable; results are bit-identical run to run (the kernel's
 * LDS integer atomics decide where a candidate is stored, never what is computed; there are no floating-point atomics).
 * Out of scope: beams over 64. */
size_t eec_ctc_lexbeam_wide_workspace_bytes(int n_seq, int Tq, int beam_size);
int eec_ctc_lexbeam_wide_decode(const float* logp, int n_seq, int Tq, int V, const int32_t* em_len, const void* trie, int blank, int sil,
                                int beam_size, int nbest, float word_score, float sil_score, float beam_threshold, int max_words,
                                int32_t* words, int32_t* word_count, int32_t* tokens, int32_t* token_count, int32_t* timesteps, float* scores,
                                int32_t* n_hyp, void* workspace, size_t workspace_bytes, void* stream, const void* lm, float lm_weight,
                                const void* smear, int log_add);

/* CTC forced alignment: replaces BeamInference.get_trellis / backtrack (util/beam_infer.py:129-150, 153-191), the Viterbi
 * alignment of a token sequence against one exit's CTC log-probs -- the CTC half of the reference's joint AED + CTC beam
 * choice (util/beam_infer.py:309-383) --, for n_hyp hypotheses in one launch (one wavefront each; csrc/ctc_align.hip).
 * The reference's semantics, quirks included.  With em [T, V] the emission of a hypothesis, tok its N ids, tr [T+1, N+1]:
 *   tr[0,0] = 0;  tr[t+1,0] = tr[t,0] + em[t,0] (column 0 of the emission, not `blank`);  tr[0,1:] = -inf;
 *   tr[T+1-N:,0] = +inf (after the cumulative sum);  tr[t+1,j] = max(tr[t,j] + em[t,blank], tr[t,j-1] + em[t,tok[j-1]]):
 *   a token occupies exactly one frame, staying costs the blank, repeated tokens get no special treatment.  The +inf cells
 *   (rows >= T+1-N+j) feed only each other and are never read by the backtrack.
 *   Backtrack from (t, j) = (T, N): stayed = tr[t-1,j] + em[t-1,blank], changed = tr[t-1,j-1] + em[t-1,tok[j-1]]; the change is
 *   taken only if changed > stayed (a tie stays); prob += em[t-1, changed ? tok[j-1] : 0] (the literal 0, not `blank`);
 *   Point(j-1, t-1, prob); after a change --j, stop at j == 0.  path[0].score is the sum over the whole path.
 *   logp [n_em, T', V] fp32; em_len [n_em] int32 frames T of every emission, or NULL = T' for all
 *   tokens [n_hyp, tok_stride] int64, tok_len [n_hyp] int32 (N); em_index [n_hyp] int32 the emission of every hypothesis, or
 *   NULL = its own index h (then n_em >= n_hyp)
 *   point_token [n_hyp, T'] int32: the Point's token_index at frame t; -1 before the first token's frame and from T on
 *   point_score [n_hyp, T'] fp32: the Point's cumulative score (summed from the last frame, as the reference does); -inf there
 *   path_score [n_hyp] = path[0].score, final_score [n_hyp] = tr[T, N]
 *   status [n_hyp] int32: 0 aligned; 1 not alignable -- N = 0, N > T (the reference prints "Failed to align" and returns a
 *       fragment: a stated divergence), N > tok_stride, a token id outside [0, V), an em_index outside [0, n_em), an em_len
 *       outside [1, T'], or non-finite emissions that leave the backtrack short of the first token.  None of these is used as
 *       an address; the row's outputs are the fill values (-1, -inf).
 *   trellis_opt: NULL, or [n_hyp, T' + 1, tok_stride + 1] fp32: the full trellis, +-inf cells included, rows past T and columns
 *       past N (and every cell of a status-1 row) -inf.
 *   workspace: eec_ctc_align_workspace_bytes(n_hyp, T', max tokens) bytes -- 0 today (decisions live in LDS), NULL is accepted.
 * EEC_ERR_BAD_ARG: a null required pointer, blank outside [0, V), tok_stride < 1, n_hyp < 0, T' < 1, n_em < 1; n_hyp == 0 is a
 * successful no-op.  EEC_ERR_UNSUPPORTED: tok_stride > 255, V < 2, or T' * (8 * ceil((tok_stride + 1) / 64) + 6) > 65536 bytes
 * of LDS (T' <= 1724 at tok_stride 255, T' <= 2978 below 128).  No allocation, no synchronisation; graph-capturable. */
size_t eec_ctc_align_workspace_bytes(int n_hyp, int Tq, int max_tokens);
int eec_ctc_align(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int64_t* tokens, const int32_t* tok_len,
                  const int32_t* em_index, int n_hyp, int tok_stride, int blank, int32_t* point_token, float* point_score,
                  float* path_score, float* final_score, int32_t* status, float* trellis_opt, void* workspace, void* stream);

/* Lexicon post-processing: replaces the scan of apply_lex (util/tokenizer.py:35-50), which inference.py applies to every
 * hypothesis it prints -- a word that is not in the lexicon becomes the lexicon word with the smallest Levenshtein distance,
 * the first such word in file order (strict <) --, for n_queries words against the whole lexicon in one call
 * (csrc/lexicon.hip: Myers / Hyyro bit-parallel edit distance, one work-item per (query, lexicon word) pair).
 * Symbols are Unicode code points.  The packer maps the lexicon's distinct code points, in ascending order, to the byte codes
 * 1..A (A <= 255); a query symbol outside that alphabet is encoded as 0, which matches nothing.
 *
 * eec_lexicon_pack is HOST code and needs no device:
 *   symbols [offsets[n_words]] UTF-32 code points of all words, flat; offsets [n_words + 1] int64, offsets[0] = 0, ascending
 *       (word i = symbols[offsets[i] .. offsets[i+1]); empty words are legal and keep their index)
 *   image: image_bytes >= eec_lexicon_pack_bytes(n_words, offsets[n_words], longest word) bytes of host memory, 8-byte aligned;
 *       the caller copies exactly that many bytes to the device (8-byte aligned) and passes them as `packed`
 *   code_map [256] int32: code -> code point for 1..A, -1 elsewhere;  n_codes: NULL or where A is written
 *   image layout, int32 units: header[16] = {magic, n_words, max_len, n_groups = ceil(max_len / 4), A, info offset, gbase
 *       offset, sym offset, sym dwords, total dwords, 0..};  info [n_words][2] = (original index, length) of the word at sorted
 *       position s -- the words are stably sorted by length, a speed choice only --;  gbase [n_groups]: the dword holding symbols
 *       4g .. 4g+3 of sorted word s (symbol 4g+k in byte k, unused bytes 0) is sym[gbase[g] + s], stored for the words longer
 *       than 4g only (a suffix of the sorted order), position-major.
 *   eec_lexicon_pack_bytes is non-decreasing in each argument; 0 for n_words <= 0, negative sizes, total_symbols >
 *       n_words * max_len, or an image of 2^31 dwords or more.
 *   EEC_ERR_BAD_ARG: a null pointer, n_words <= 0, offsets not ascending from 0.  EEC_ERR_UNSUPPORTED: more than 255 distinct
 *   code points.  EEC_ERR_WORKSPACE: image_bytes too small.
 *
 * eec_lexicon_nearest:
 *   packed: the image on the device; n_words must be the count it was packed with
 *   queries: encoded query bytes, flat, on the device; query_offsets [n_queries + 1] int32 on the device (query q =
 *       queries[query_offsets[q] .. query_offsets[q+1]))
 *   max_query_len: the longest query of the call, stated by the caller (the offsets are device memory): it selects the kernel
 *       (32-bit vectors up to 32 symbols, 64-bit up to 64, 8 x 32-bit with carries up to EEC_LEX_MAX_QUERY)
 *   out_index, out_distance [n_queries] int32: argmin_i levenshtein(query, word i) with ties to the LOWEST original index, and
 *       that distance.  A query of no symbols gets the first shortest word.  (-1, -1) for a query whose offsets are negative,
 *       descending or more than max_query_len apart (none of its bytes is read), and for every query when the image's header does
 *       not carry n_words.
 *   workspace: eec_lexicon_nearest_workspace_bytes(n_queries, n_words) bytes, 8-byte aligned: the per-share minima.
 * The 32-bit kernel has two forms: a workgroup advances 4 queries side by side below EEC_LEX_TILE_SWITCH queries per call and 8
 * from there on (same results; the wider tile reads the lexicon half as often).
 * A workgroup is EEC_LEX_BLOCK_WORDS work-items, one lexicon word each; with few queries the lexicon is dealt over up to one
 * workgroup per EEC_LEX_BLOCK_WORDS words.  Two kernels on `stream` (the search, then the reduction of the shares, one wave
 * per query); integer keys (distance << 32 | index) under min, so results are bit-identical run to run.
 * EEC_ERR_BAD_ARG: a null pointer, n_words <= 0, n_queries < 0, max_query_len < 0, a misaligned image or workspace;
 * n_queries == 0 is a successful no-op.  EEC_ERR_UNSUPPORTED: max_query_len > EEC_LEX_MAX_QUERY.  EEC_ERR_WORKSPACE:
 * workspace_bytes too small.  All checked before any device work.  No allocation, no synchronisation; graph-capturable. */
#define EEC_LEX_MAX_QUERY 256
#define EEC_LEX_BLOCK_WORDS 256
#define EEC_LEX_TILE_SWITCH 2048
size_t eec_lexicon_pack_bytes(int n_words, int64_t total_symbols, int max_len);
int eec_lexicon_pack(const uint32_t* symbols, const int64_t* offsets, int n_words, void* image, size_t image_bytes, int32_t* code_map,
                     int32_t* n_codes);
size_t eec_lexicon_nearest_workspace_bytes(int n_queries, int n_words);
int eec_lexicon_nearest(const void* packed, int n_words, const uint8_t* queries, const int32_t* query_offsets, int n_queries,
                        int max_query_len, int32_t* out_index, int32_t* out_distance, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- Edit distance: error-rate scoring of hypotheses against references (csrc/edit_distance.hip) ---------------------------------
 * For a reference r of m tokens and a hypothesis h of n tokens, int32 each and compared by equality only, with the unit costs of
 * Kaldi's compute-wer, jiwer and torchaudio's edit_distance (sclite's 4 / 3 / 3 weights are not served):
 *     K[0][0] = 0;   K[i][0] = i << 16;   K[0][j] = j << 16
 *     K[i][j] = min( K[i-1][j-1] + (r_i == h_j ? 0 : (1 << 16) + 1),     diag
 *                    K[i-1][j]   + (1 << 16),                            del: a reference token unmatched
 *                    K[i][j-1]   + (1 << 16) )                           ins: a hypothesis token unmatched
 *     distance = K[m][n] >> 16        subs = K[m][n] & 0xffff
 *     dels = (distance - subs - (n - m)) / 2      ins = dels + n - m      hits = m - subs - dels
 * distance is the Levenshtein distance and depends on no convention.  The S / D / I split does: among all minimum-cost
 * alignments this is the one with the FEWEST SUBSTITUTIONS (the key is minimised lexicographically; an additive pair under
 * lexicographic min is a valid dynamic programme, so no evaluation order enters).  n - m = ins - dels, so (distance, subs) fixes
 * all four counts.  Other tools may split the same distance differently.
 * The op string, written only when asked for, is the canonical alignment: dir[i][j] is the FIRST of (diag, del, ins) whose
 * candidate equals K[i][j]; del on the border j = 0, ins on the border i = 0; walked back from (m, n), emitted in forward order as
 *     0 hit, 1 substitution, 2 deletion, 3 insertion.
 * Its counts are the reported ones, and it has n + dels ops.
 *
 *   hyp [n_pairs][hyp_pitch], hyp_len [n_pairs]; ref [n_refs][ref_pitch], ref_len [n_refs]: int32 on the device.  Lengths are
 *       clamped to [0, pitch]; tokens at or past a length are never read.  hyp / ref may be NULL when their pitch is 0.
 *   ref_of [n_pairs] int32 or NULL: the reference of pair p; NULL: pair p scores against reference p and n_refs == n_pairs.
 *       An entry outside [0, n_refs) gives counts (-1, -1, -1, -1) and n_ops 0 for that pair, and nothing of the pair is read.
 *   counts [n_pairs][4] int32, 16-byte aligned: distance, subs, dels, ins.
 *   ops [n_pairs][ref_pitch + hyp_pitch] uint8 or NULL; n_ops [n_pairs] int32 (needed with ops): the op string of pair p is
 *       ops[p][0 .. n_ops[p]); bytes past it are not written.
 *   workspace: eec_edit_distance_workspace_bytes(n_pairs, ref_pitch, hyp_pitch, ops != NULL) bytes, 256-byte aligned: two bits per
 *       table cell when ops are wanted, nothing otherwise (then it may be NULL).  The size is non-decreasing in each argument and
 *       0 for a non-positive one.
 * One wave per pair, four pairs per workgroup, the hypothesis dealt over the lanes in strips of 4, 8 or 16 columns (by hyp_pitch),
 * the rows as a systolic wavefront; with ops a second kernel of one work-item per pair walks back.  Integer only: two runs are
 * bit-identical, and a call on a slice of the pairs returns the rows of the whole call.
 * EEC_ERR_BAD_ARG: a null pointer where one is needed, a misaligned counts, n_pairs < 0, a pitch below 0 or above
 * EEC_EDIT_MAX_LEN, n_refs < 1 or (without ref_of) != n_pairs with n_pairs > 0, ops without n_ops.  EEC_ERR_WORKSPACE: a short or
 * misaligned workspace.  n_pairs == 0 is a successful no-op.  All checked before any device work.  No allocation, no
 * synchronisation; graph-capturable. */
#define EEC_EDIT_MAX_LEN 1024
size_t eec_edit_distance_workspace_bytes(int n_pairs, int max_ref_len, int max_hyp_len, int want_ops);
int eec_edit_distance(const int32_t* hyp, const int32_t* hyp_len, int n_pairs, int hyp_pitch, const int32_t* ref,
                      const int32_t* ref_len, int n_refs, int ref_pitch, const int32_t* ref_of, int32_t* counts, uint8_t* ops,
                      int32_t* n_ops, void* workspace, size_t workspace_bytes, void* stream);

/* ---- SpecAugment: time warp, frequency and time masks of a mel batch (csrc/specaug.hip) -------------------------------------------
 * The stage between the mel front end and the encoder in training; the reference has none (its collate hands the mel over as it
 * is).  Two launches: eec_specaug_draw writes one row of integer parameters per utterance, eec_specaug_apply reads such rows --
 * drawn or prescribed by the caller alike -- and writes the augmented copy.
 *
 *   mel, out [B][n_mels][T] fp32, T contiguous (what eec_frontend_forward writes and the encoder entries read); out != mel.
 *   frame_len [B] int32 or NULL: valid mel frames per utterance, clamped to [0, T]; NULL: T everywhere.  n = the clamped length.
 *       Frames t >= n are copied through bit for bit and are never read for a frame t < n: a NaN there reaches nothing.
 *   params [B][P] int32, P = 2 + 2 * n_freq_masks + 2 * n_time_masks (n_freq_masks <= EEC_SPECAUG_MAX_FREQ_MASKS, n_time_masks <=
 *       EEC_SPECAUG_MAX_TIME_MASKS):   c, w,   f0, fw per frequency mask,   t0, tw per time mask.   (c, w) = (0, 0): no warp.
 *
 * The draw is a pure function of (seed, utt_offset + b, slot) through the dropout generator (csrc/eec_drop.h, the contract above at
 * eec_train_forward): u(slot) = lowbias32(lo(i) * C1 + hi(i) * C2 + key(seed, EEC_SPECAUG_SITE)) with i = (utt_offset + b) * 64 + slot
 * in 64-bit wrap-around arithmetic, and a uniform integer in [0, m) is (uint64) u * m >> 32.  Slots, W = time_warp_window,
 * F = freq_mask_width, Tmax = time_mask_width, ratio = time_mask_ratio:
 *   0, 1          if W > 0 and n > 2 W:  c = W + [0, n - 2 W),  then  w = c - W + 1 + [0, 2 W);  otherwise c = w = 0
 *   2 + 2 k, + 1  frequency mask k:  fw = [0, min(F, n_mels) + 1),  then  f0 = [0, n_mels - fw + 1)
 *   2 + 2 n_freq_masks + 2 k, + 1   time mask k:  tw = [0, min(Tmax, n, floor((double) ratio * n)) + 1),  then  t0 = [0, n - tw + 1)
 * so c lies in [W, n - W), w in [c - W + 1, c + W], every mask inside its axis, and -- utt_offset entering the index -- a call on a
 * slice of the batch with utt_offset advanced by the slice's start returns the rows of the whole call.
 *
 * The warp (applied when 1 <= c <= n - 1 and 1 <= w <= n - 1, ignored otherwise) maps the source frames [0, c) onto the output
 * frames [0, w) and the source frames [c, n) onto the output frames [w, n): torch.nn.functional.interpolate(align_corners=False) of
 * the two segments separately, as ESPnet's and lhotse's time_warp do.  For output frame d of a segment of n_in source and n_out output
 * frames, in exact integers:
 *     num = (2 d + 1) * n_in - n_out   (EEC_SPECAUG_LINEAR: clamped at 0)      den = 2 * n_out
 *     i = floor(num / den)             fraction f = (num - i * den) / den  in [0, 1)
 *   EEC_SPECAUG_LINEAR:   taps i, min(i + 1, n_in - 1);  weights 1 - f, f
 *   EEC_SPECAUG_BICUBIC:  taps i - 1, i, i + 1, i + 2, each clamped to [0, n_in - 1];  cubic convolution with A = -0.75:
 *       weights k2(f + 1), k1(f), k1(1 - f), k2(2 - f),   k1(x) = ((A + 2) x - (A + 3)) x x + 1,   k2(x) = ((A x - 5 A) x + 8 A) x - 4 A
 * Tap indices are relative to the segment and never cross c.  f and the weights are evaluated in fp64, each weight is rounded once to
 * fp32, and the taps are combined in fp32 in index order (the compiler may fuse the multiply-adds):
 *     |out - exact| <= 6 * 2^-24 * sum_k |w_k| |x_k|     (one rounding per weight, one per product, three additions).
 *
 * The masks are applied after the warp, to frames t < n only: an element whose mel row lies in some [f0, f0 + fw) or whose frame lies
 * in some [t0, t0 + tw) becomes mask_value.  Parameters are never trusted: mask ranges are clipped to [0, n_mels) and [0, n) (sums in
 * 64 bits; an empty or negative width masks nothing), a warp outside the range above is ignored, so nothing outside an utterance's
 * valid frames is ever read, whatever params holds.
 *
 * eec_specaug_draw: one work-item per (utterance, slot group).  eec_specaug_apply: one workgroup per (tile of 128 output frames, group
 * of 32 mel rows, utterance); with a warp one work-item per output frame computes segment, taps and weights once and walks down the
 * rows; without one the rows move as aligned 16-byte quads (row heads and tails, and pointers off a 16-byte boundary, as single
 * floats).  Masked elements are not loaded.  No atomics, no LDS, no scratch: two runs are bit-identical.
 * EEC_ERR_BAD_ARG, before any device work: B < 0, n_mels < 1, T < 1, a mask count below 0 or over its limit; draw: W < 0, F < 0,
 * Tmax < 0, a negative, NaN or infinite ratio, null params; apply: a mode other than the two, a NaN mask_value, null mel, params or
 * out, out == mel.  B == 0 is a successful no-op.  Errors through eec_last_error().  No allocation, no synchronisation;
 * graph-capturable. */
#define EEC_SPECAUG_MAX_FREQ_MASKS 8
#define EEC_SPECAUG_MAX_TIME_MASKS 16
#define EEC_SPECAUG_SITE 0x53504341u
#define EEC_SPECAUG_LINEAR 0
#define EEC_SPECAUG_BICUBIC 1
int eec_specaug_draw(const int32_t* frame_len, int B, int n_mels, int T, uint64_t seed, uint64_t utt_offset, int time_warp_window,
                     int n_freq_masks, int freq_mask_width, int n_time_masks, float time_mask_ratio, int time_mask_width,
                     int32_t* params, void* stream);
int eec_specaug_apply(const float* mel, const int32_t* frame_len, const int32_t* params, int B, int n_mels, int T, int n_freq_masks,
                      int n_time_masks, int mode, float mask_value, float* out, void* stream);

/* ---- Resampling / speed perturbation: batched polyphase sinc resampling of a waveform batch (csrc/resample.hip) -------------------
 * The waveform-level stage in front of the mel front end: speed perturbation by the customary factors 0.9 / 1.0 / 1.1 (Ko et al. 2015)
 * and sample-rate conversion.  The reference has neither; the definition is torchaudio's functional.resample / transforms.Speed with
 * resampling_method "sinc_interp_hann".
 *
 * A ratio is (orig, new) in positive integers, reduced by their gcd to (o, n); a speed factor f at sample rate sr is the ratio
 * (int(f * sr), sr), as transforms.Speed computes it (16 kHz: 0.9 -> (9, 10), 1.1 -> (11, 10)).  With lpw = lowpass_filter_width
 * (default 6), rolloff (default 0.99) and a Hann window:
 *     base  = min(o, n) * rolloff            width = ceil(lpw * o / base)            K = 2 * width + o
 *     t(j, k) = clamp((-j / n + (k - width) / o) * base, -lpw, +lpw)                  j = 0 .. n - 1 (phase), k = 0 .. K - 1 (tap)
 *     h(j, k) = sinc(pi * t) * cos(pi * t / (2 * lpw))^2 * base / o                   sinc(0) = 1
 *               evaluated in fp64 on the host, rounded once to fp32
 *     y[i]    = sum_{k = 0 .. K - 1} h(i % n, k) * x[(i / n) * o + k - width]         x outside [0, len) is 0
 *     out_len = ceil(n * len / o) = (n * len + o - 1) / o                             int64 arithmetic
 * The sum is fp32: each tap is one rounded multiply and one rounded add (no fused multiply-add), the taps run in the order
 * k = 0, 1, ... from +0.  Taps whose fp32 weight is exactly zero may be skipped: the clamp makes every tap outside the window round to
 * zero, and skipping them cannot change the bits for finite input.  The ratio (1, 1) is a bit-for-bit copy (torchaudio returns its
 * input; the formula would low-pass it).  Samples at or past an utterance's length are never read, so a NaN there reaches nothing;
 * output positions at or past out_len[b] are written as 0.0, the collate's padding value; the result for utterance b equals
 * resampling that utterance alone and padding afterwards.  A non-finite sample inside the valid region is unspecified.
 *
 * The plan (host only, no device call): eec_resample_plan writes one image of int32 words for R <= EEC_RESAMPLE_MAX_RATIOS ratios;
 * eec_resample_plan_bytes returns its size (0 with a message when the arguments are refused).  The caller uploads it once.
 *     word 0 EEC_RESAMPLE_MAGIC, 1 R, 2 the image's size in words, 3 lpw
 *     ratio r, words 4 + 8 r ..:  o, n, width, K, phases, weights, total, most
 *         phases: word offset of n triples (first, count, at): phase j's non-zero fp32 weights are the taps first .. first + count - 1,
 *                 stored at words weights + at ..;  zero heads and tails are not stored (zeros between two non-zero taps are)
 *         weights: word offset of the ratio's `total` fp32 weights, phase after phase;  most: the largest count
 * A call carries one plan; choice [B] int32 says which of its ratios each utterance takes.  A choice outside [0, R) is treated as a
 * copy, and the kernel never indexes the plan with it.
 *
 * The draw: choice[b] = (uint64) word(key(seed, EEC_SPEED_SITE), (utt_offset + b) * 64 + 0) * R >> 32, word and key being those of
 * the dropout generator (csrc/eec_drop.h; the contract at eec_train_forward), exactly as eec_specaug_draw uses them; the same launch
 * writes out_len[b].  utt_offset enters the index, so a call on a slice of the batch with utt_offset advanced returns the rows of
 * the whole call.  eec_resample_lengths writes out_len for prescribed choices.
 *
 *   wave [B][L] fp32, out [B][L_out] fp32, both contiguous in time, out != wave.  L_out is the caller's: max_r ceil(n_r * L / o_r) of
 *       the plan's ratios holds every utterance; an out_len beyond L_out is cut to it.
 *   lengths [B] int64 or NULL: valid samples per utterance, clamped to [0, L]; NULL: L everywhere.
 *   choice [B] int32; out_len [B] int64 (eec_resample: written too, may be NULL).
 * eec_resample: one workgroup of 256 work-items per (tile of 1024 output samples, utterance).  The tile's input window --
 * (1024 / n) * o + K samples -- is staged in LDS with zeros outside [0, len) when it fits 4096 floats, and the ratio's weights when
 * they fit 6144 floats; otherwise they are read through the caches.  One work-item per output sample, four rounds per tile, so a
 * wave stores 256 consecutive bytes; a copy moves 16-byte quads where both rows are 16-byte aligned.  Workgroups past an utterance's
 * out_len only write zeros.  No atomics, every output a pure
 * function of its utterance: two runs, a split batch and lengths = NULL against lengths all L return the same bits.
 * EEC_ERR_BAD_ARG, before any device work, through eec_last_error(): plan -- R outside [1, EEC_RESAMPLE_MAX_RATIOS], a rate below 1,
 * max(o, n) > EEC_RESAMPLE_MAX_RATE after reduction, lpw outside [1, EEC_RESAMPLE_MAX_LPW], rolloff outside (0, 1], a null pointer,
 * (EEC_ERR_WORKSPACE) a short image; device entries -- B < 0, L outside [0, 2^30], L_out < 0, a null pointer where one is needed,
 * out == wave.  B == 0 is a successful no-op.  No allocation, no synchronisation, nothing read back; graph-capturable.
 * Not served: sinc_interp_kaiser, a backward (the input is data), tempo change without pitch change. */
#define EEC_RESAMPLE_MAX_RATIOS 8
#define EEC_RESAMPLE_MAX_RATE 640
#define EEC_RESAMPLE_MAX_LPW 64
#define EEC_RESAMPLE_MAGIC 0x52534D50
#define EEC_SPEED_SITE 0x53504545u
size_t eec_resample_plan_bytes(int R, const int32_t* orig, const int32_t* new_, int lowpass_filter_width, double rolloff);
int eec_resample_plan(int R, const int32_t* orig, const int32_t* new_, int lowpass_filter_width, double rolloff, void* image,
                      size_t image_bytes);
int eec_speed_draw(const int64_t* lengths, int B, int L, uint64_t seed, uint64_t utt_offset, const void* plan, int32_t* choice,
                   int64_t* out_len, void* stream);
int eec_resample_lengths(const int64_t* lengths, const int32_t* choice, int B, int L, const void* plan, int64_t* out_len,
                         void* stream);
int eec_resample(const float* wave, const int64_t* lengths, const int32_t* choice, int B, int L, const void* plan, float* out,
                 int L_out, int64_t* out_len, void* stream);

/* ---- Waveform augmentation: reverberation, noise, volume (csrc/waveaug.hip) --------------------------------------------------------
 * The waveform-level stages between speed perturbation and the mel front end, in the order of Kaldi's wav-reverberate: convolution
 * with a room impulse response (RIR), additive noise at a chosen signal-to-noise ratio, a volume gain.  The reference has none of
 * them.  Each stage is switched per utterance by a row of parameters, drawn (eec_waveaug_draw) or prescribed by the caller.
 *
 *   wave, out [B][L] fp32, contiguous in time; lengths [B] int64 or NULL: valid samples per utterance, clamped to [0, L]; NULL: L.
 *       len = the clamped length.  Samples at or past len are never read (a NaN there reaches nothing), outputs at or past len are
 *       0.0, and every utterance comes out as if it had been processed alone.
 *   params [B][EEC_WAVEAUG_PARAMS] int32:  rir, noise, start, snr_idx, gain_bits (the fp32 gain as its bits).
 *
 * 1. Reverberation.  RIR r of the bank has K stored taps h[0 .. K) and a shift d (below).  For 0 <= i < len
 *         y[i] = sum_{k = 0 .. K - 1} h[k] * x[i + d - k]                  x outside [0, len) is 0
 *    in fp32, the taps in the order k = 0, 1, ... from +0, each one rounded multiply and one rounded add (no fused multiply-add), as
 *    eec_resample states its sum; products with a sample outside [0, len) may be skipped, which cannot change the bits for finite
 *    input.  The output is as long as the input.  rir outside [0, R) (-1 by convention), or no bank: y = x bit for bit.
 * 2. Noise.  Noise row m has len_m >= 1 samples; s = start reduced into [0, len_m) (the non-negative remainder);
 *         n[i] = noise[m][(s + i) mod len_m]                               the row is tiled, as Kaldi repeats it
 *         E_s = sum_{i < len} y[i]^2      E_n = sum_{i < len} n[i]^2       in fp64 (the square of an fp32 value is exact there)
 *         scale = (float) (sqrt(E_s / E_n) * g[snr_idx])                   fp64, IEEE division and square root, rounded once
 *         z[i] = y[i] + scale * n[i]                                       one rounded multiply, one rounded add
 *    g is the caller's table of n_snrs <= EEC_WAVEAUG_MAX_SNRS fp64 factors, g = 10^(-snr / 20) for an SNR in dB, evaluated on the host
 *    (it travels in the launch's argument block; no transcendental is evaluated on the device).  noise outside [0, M), snr_idx
 *    outside [0, n_snrs), no bank, E_s == 0 or E_n == 0: z = y bit for bit.
 *    The order of the two energy sums is fixed.  The samples are cut into tiles of EEC_WAVEAUG_TILE = 1024.  Inside a tile, group t
 *    (t = 0 .. 127) adds the squares of its samples 8 t .. 8 t + 7 that lie below len, in that order, from 0.0; the 128 group sums are
 *    combined as two blocks of 64, inside a block by v[t] += v[t + s] for t < s, s = 32, 16, 8, 4, 2, 1 in turn, and the tile's partial
 *    is block 0 + block 1.  The partials of the tiles 0 .. ceil(len / 1024) - 1 are added in tile order from 0.0.  Nothing else of
 *    the launch geometry enters, and no atomics are used.
 * 3. Volume.  out[i] = z[i] * gain, gain = the float of gain_bits; 1.0f leaves z as it is.
 *
 * The banks (host only, no device call) follow eec_resample_plan: *_bytes returns the image's size (0 with a message when the
 * arguments are refused), the builder writes one image of int32 words the caller uploads once per device.
 *   eec_rir_bank: R <= EEC_WAVEAUG_MAX_BANK RIRs, `taps` their fp32 taps one RIR after the other, n_taps [R] in
 *       [1, EEC_REVERB_MAX_TAPS].  The peak p is the first index of max |h| of the taps as given.  Normalisation in fp64, each tap
 *       rounded once to fp32: EEC_RIR_NORM_L2 divides by sqrt(sum h^2) (unit energy), EEC_RIR_NORM_PEAK by |h[p]|, EEC_RIR_NORM_NONE
 *       keeps the taps.  The lo leading and the trailing taps that are exactly zero afterwards are not stored.  shift != 0 (Kaldi's
 *       --shift-output): d = p - lo, the direct path stays where it was, so frame counts and CTC targets are untouched; shift == 0:
 *       d = -lo, the plain causal convolution cut to the input's length.
 *           word 0 EEC_RIR_MAGIC, 1 R, 2 the image's size in words, 3 normalize | shift << 8
 *           RIR r, words 4 + 4 r ..:  K, d, taps (word offset of the K fp32 taps), p - lo
 *   eec_noise_bank: M <= EEC_WAVEAUG_MAX_BANK rows, `samples` one row after the other, n_samples [M] in [1, 2^30].
 *           word 0 EEC_NOISE_MAGIC, 1 M, 2 the image's size in words, 3 0
 *           row m, words 4 + 2 m ..:  len_m, samples (word offset of the len_m fp32 samples)
 *   Refused (EEC_ERR_BAD_ARG): a count outside its range, a null pointer, an unknown normalize, a value that is not finite, a RIR
 *   without a non-zero tap (also one whose taps all round to zero), an image of 2^31 words or more; (EEC_ERR_WORKSPACE) a short image.
 *
 * The draw, one work-item per utterance, from the dropout generator exactly as eec_specaug_draw and eec_speed_draw use it:
 * u(slot) = word(key(seed, EEC_WAVEAUG_SITE), (utt_offset + b) * 64 + slot); a coin fires when u < thr, thr = floor(p * 2^32) computed
 * by the caller (2^32 always fires, 0 never); a uniform integer in [0, m) is (uint64) u * m >> 32.
 *     slot 0  reverb coin (thr_reverb)         slot 1  rir = [0, R)              no coin, or no bank: rir = -1
 *     slot 2  noise coin (thr_noise)           slot 3  noise = [0, M)            slot 4  start = [0, len_noise)
 *     slot 5  snr_idx = [0, n_snrs)            no coin, no bank or n_snrs == 0: noise = -1, start = snr_idx = 0
 *     slot 6  gain = (float) (lo + (hi - lo) * (u * 2^-32)) in fp64, operation by operation;  volume == 0: gain = 1.0f
 * utt_offset enters the index, so a call on a slice of the batch with utt_offset advanced returns the rows of the whole call.
 *
 * The launches take such rows and never trust them: an index outside a bank switches its stage off, a start is reduced mod len_m.
 *   eec_reverb        one workgroup of 128 work-items per (tile of 1024 outputs, utterance); a work-item holds 8 consecutive outputs in
 *       registers.  The taps stream through LDS in chunks of 512 together with the 1536 input samples they meet (zeros outside
 *       [0, len)); chunks whose samples all lie outside the utterance are skipped.  The tile leaves through LDS, so a wave stores 256
 *       consecutive bytes whatever the row's alignment.  Without a RIR the tile moves as 16-byte quads where both rows are 16-byte
 *       aligned.  Workgroups past len only write zeros.  partials (may be NULL) receives the tile's partial E_s.
 *   eec_noise_energy  the same geometry: the partial E_n of the tiled noise segment per tile, and, when `signal` is not NULL, the
 *       partial E_s of that buffer (for a caller that did not run eec_reverb).
 *   eec_noise_mix     one workgroup of 256 work-items per (2048 samples, utterance): adds the partials in the stated order, forms
 *       scale, writes out (out == y is allowed: every element is read and written by one work-item) and, from the first workgroup
 *       of an utterance, applied[b] = (scale, gain) when applied is not NULL; scale is written as 0.0 where no noise was added.
 *   partials: double [B][ceil(max(L, 1) / 1024)][2] (E_s, E_n), eec_waveaug_partials_bytes(B, L) bytes, 8-byte aligned.
 * No atomics, nothing read back, no allocation, no synchronisation; graph-capturable.  Two runs, a split batch with utt_offset
 * advanced, lengths = NULL against lengths all L and a storage off a 16-byte boundary return the same bits.
 * EEC_ERR_BAD_ARG, before any device work, through eec_last_error(): B < 0, L outside [0, 2^30], n_snrs outside [0, 64], a threshold
 * above 2^32, lo or hi not finite, a null pointer where one is needed, out == wave in eec_reverb.  B == 0 is a successful no-op.
 * Not served: reverberated point-source noises, babble, codec and clipping effects, a backward (the input is data). */
#define EEC_WAVEAUG_SITE 0x57415547u
#define EEC_WAVEAUG_PARAMS 5
#define EEC_WAVEAUG_TILE 1024
#define EEC_WAVEAUG_MAX_BANK 4096
#define EEC_WAVEAUG_MAX_SNRS 64
#define EEC_REVERB_MAX_TAPS 16384
#define EEC_RIR_MAGIC 0x52495242
#define EEC_NOISE_MAGIC 0x4E4F4953
#define EEC_RIR_NORM_NONE 0
#define EEC_RIR_NORM_L2 1
#define EEC_RIR_NORM_PEAK 2
size_t eec_rir_bank_bytes(int R, const float* taps, const int32_t* n_taps, int normalize, int shift);
int eec_rir_bank(int R, const float* taps, const int32_t* n_taps, int normalize, int shift, void* image, size_t image_bytes);
size_t eec_noise_bank_bytes(int M, const float* samples, const int32_t* n_samples);
int eec_noise_bank(int M, const float* samples, const int32_t* n_samples, void* image, size_t image_bytes);
size_t eec_waveaug_partials_bytes(int B, int L);
int eec_waveaug_draw(int B, uint64_t seed, uint64_t utt_offset, const void* rir_bank, uint64_t thr_reverb, const void* noise_bank,
                     uint64_t thr_noise, int n_snrs, int volume, double lo, double hi, int32_t* params, void* stream);
int eec_reverb(const float* wave, const int64_t* lengths, const int32_t* params, int B, int L, const void* rir_bank, float* out,
               double* partials, void* stream);
int eec_noise_energy(const float* signal, const int64_t* lengths, const int32_t* params, int B, int L, const void* noise_bank,
                     double* partials, void* stream);
int eec_noise_mix(const float* y, const int64_t* lengths, const int32_t* params, int B, int L, const void* noise_bank,
                  const double* snr_gain, int n_snrs, const double* partials, float* out, float* applied, void* stream);

/* ---- Reverberation by FFT (csrc/reverb_fft.hip) -------------------------------------------------------------------------------------
 * A second evaluation of stage 1 above, y[i] = sum_k h[k] x[i + d - k] over the stored taps with x = 0 outside [0, len), for RIRs of
 * thousands of taps, where the direct sum's cost grows with K.  Uniformly partitioned overlap-save in output coordinates, with
 * S = EEC_REVERB_FFT_BLOCK and N = 2 S: RIR r of K taps has P = ceil(K / S) partitions, partition p the taps [p S, (p + 1) S) padded
 * with zeros to N; output block m is y[m S, (m + 1) S); input window j of an utterance is x[(j - 1) S + d, (j + 1) S + d); and
 *         Y_m = sum_{p = 0 .. P - 1} X_{m - p} * H_p          in that order, X and H the N-point DFTs, * bin by bin
 * of whose inverse transform the last S samples are the block.  The block grid starts at the utterance's own sample 0, so every
 * utterance comes out as if processed alone.  Multiply-adds may be fused.
 *
 * What this path keeps: rows are never trusted (an index outside the bank, or a spectral image that is not the bank's, copies the
 * utterance bit for bit, as eec_reverb does); samples at or past len are never read; outputs there are 0.0; all-zero input gives exact
 * zeros; two runs, a split batch, lengths = NULL against lengths all L and a storage off a 16-byte boundary return the same bits;
 * `partials` receives the tile energies E_s of the fp32 output in the layout and order stated above, so eec_noise_energy and
 * eec_noise_mix run unchanged behind it.  What it does not keep: it is not bit-identical to eec_reverb or to any host path, and a
 * one-tap RIR is no longer an exact scaled copy.
 *
 * The bound.  u = 2^-24.  The transforms are Cooley-Tukey factorisations of log2 N radix-2 stages (the radix-8 and radix-4 butterflies
 * are three and two of them with fewer twiddle products, the real split is the last) with fp32 twiddles rounded from fp64, so by
 * Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, a computed transform is off by at most log2 N * eta in the 2-norm
 * relative to its result, eta = mu + gamma_4 (sqrt 2 + mu) < 7 u with mu <= u the twiddles' error.  Per term X_{m-p} H_p: 7 u log2 N
 * from the window's transform, u from the one rounding of H_p, 3 u from the complex product; P - 1 additions add (P - 1) u of the
 * sum of the terms' norms; the inverse transform adds 7 u log2 N; the scalings by 1/2 and 1/N are exact.  With
 * ||X H_p||_2 <= ||H_p||_inf ||X||_2 <= ||h_p||_1 ||X||_2, Parseval, sum_p ||h_p||_1 = ||h||_1 and max |e| <= ||e||_2, for every
 * output block
 *         max |y_fft - y| <= (14 log2 N + P + 8) * 2^-24 * ||h||_1 * max_j ||x_j||_2        x_j the N-sample windows
 * where 8 covers the 1 + 3 - 1 above and the second-order terms.  It catches gross faults only; the kernels use at most 5e-3 of it in the tests.
 *
 *   eec_rir_spectra (host only, *_bytes as for the banks): the spectral image of a tap image eec_rir_bank wrote, so both methods see
 *       the same normalised, trimmed taps and the same d.  Every partition's N-point DFT is evaluated in fp64 by a radix-2 transform
 *       in that file and every component rounded once to fp32.  A spectrum is N floats: word pair 0 = (X[0], X[N/2]), both real;
 *       word pair k = (Re X[k], Im X[k]), 0 < k < N/2.
 *           word 0 EEC_RIR_SPECTRA_MAGIC, 1 R, 2 the image's size in words, 3 S, 4 the word offset of the twiddles, 5 .. 7 0
 *           RIR r, words 8 + 2 r ..:  P, the word offset of its P spectra (partition after partition)
 *           twiddles: N/2 pairs (cos, -sin)(2 pi u / N), u < N/2, evaluated in fp64 and rounded once; the device computes no sincos
 *       Every offset is a multiple of 4 words.  Refused (EEC_ERR_BAD_ARG): a null pointer, a tap image whose header or records are
 *       not eec_rir_bank's, an image of 2^31 words or more; (EEC_ERR_WORKSPACE) a short image.
 *   eec_reverb_fft: eec_reverb's contract argument for argument, plus the spectral image (device copy) and a workspace of
 *       eec_reverb_fft_workspace_bytes(B, L) = max(B, 1) * (ceil(L / S) + EEC_REVERB_MAX_TAPS / S - 1) * N * 4 bytes, 16-byte aligned:
 *       the spectra of the windows j = -(EEC_REVERB_MAX_TAPS / S - 1) .. ceil(L / S) - 1 of every utterance.  Two launches of 256
 *       work-items per workgroup: one workgroup per (window, utterance) transforms the windows that hold a valid sample and that a
 *       block of the utterance meets; one per (block, utterance) accumulates the products over the live windows, transforms back,
 *       writes the block through LDS and the two tile energies.  rir_bank or rir_spectra NULL: every utterance is copied and the
 *       workspace is not touched.  No atomics, nothing read back, no allocation, no synchronisation; graph-capturable.
 * Refused as eec_reverb refuses, and (EEC_ERR_WORKSPACE) a null, misaligned or short workspace when both images are given. */
#define EEC_REVERB_FFT_BLOCK 2048
#define EEC_REVERB_FFT_MIN_TAPS 256 /* from this many taps on eec_reverb_fft measured faster than eec_reverb (profiles/waveaug_fft_time.json) */
#define EEC_RIR_SPECTRA_MAGIC 0x52495246
size_t eec_rir_spectra_bytes(const void* rir_bank_image);
int eec_rir_spectra(const void* rir_bank_image, void* image, size_t image_bytes);
size_t eec_reverb_fft_workspace_bytes(int B, int L);
int eec_reverb_fft(const float* wave, const int64_t* lengths, const int32_t* params, int B, int L, const void* rir_bank,
                   const void* rir_spectra, float* out, double* partials, void* workspace, size_t workspace_bytes, void* stream);
/* for the timing tool: stages = 1 the windows' launch alone, 2 the blocks' launch alone (it reads the workspace as it finds it: run
 * the windows' launch on the same arguments first), 3 both, which is eec_reverb_fft */
int eec_reverb_fft_stage(const float* wave, const int64_t* lengths, const int32_t* params, int B, int L, const void* rir_bank,
                         const void* rir_spectra, float* out, double* partials, void* workspace, size_t workspace_bytes, int stages,
                         void* stream);

/* Mel front end(SURVEY 8f row f3): replaces util/data_loader.py:7-18 -- torchaudio Spectrogram(n_fft = 2 * args.n_fft = 1024,
 * hop_length 160, win_length 320; hann window, power 2, centred frames with reflect padding) followed by MelScale(sample_rate,
 * n_mels, n_stft = 513; htk scale, no normalisation), NO log -- on the device, as an exact-fp32 MFMA transform.
 *   wave [B, Lmax] fp32; lengths_opt [B] int64 valid samples per utterance or NULL (all Lmax)
 *   mel  [B, n_mels, 1 + Lmax / 160] fp32: utterance b fills its first 1 + lengths[b] / 160 frames (torch.stft, center=True),
 *        the rest is zero -- what the reference's collate (pad_sequence with 0) hands to the model.
 * The tables (window, DFT basis, filterbank) are built in eec_frontend_create; only the reference's geometry is served. */
typedef struct eec_frontend eec_frontend;
const char* eec_frontend_last_error(void);
int eec_frontend_create(int sample_rate, int n_fft, int win_length, int hop_length, int n_mels, eec_frontend** out);
void eec_frontend_destroy(eec_frontend* fe);
int eec_frontend_frames(int n_samples, int hop_length);
int eec_frontend_forward(eec_frontend* fe, const float* wave, const int64_t* lengths_opt, int B, int Lmax, float* mel, void* stream);

/* ---- Training step of the Early_conformer path (train.py:53-70) -------------------------------------------------
 * `enc_out = model(batch_0, valid_lengths)` in train mode and `loss.backward()` through it.  Parameters are read in place
 * as fp32 (eec_params: the nn.Parameter storages themselves, no packing); activations stay fp32 in HBM; GEMM operands are
 * split into bf16 hi / lo planes on the fly (`passes` 3: three MFMA products per GEMM, ~1e-5 relative; 1: plain bf16).
 * Semantics of the reference's train mode: BatchNorm1d normalises with the statistics of the batch (all B*T' frames,
 * padded ones included) -- `bn_batch_stats` [E*L][2][D] returns (mean, biased variance) per layer so the caller can update
 * running_mean / running_var (momentum 0.1, unbiased variance) --, dropout with probability `drop_prob` at the reference's
 * sites (after the positional encoding, inside and after each feed-forward module, on the attention probabilities, after
 * out_proj, after the convolution module) from a counter-based generator keyed by `seed` and a site number.
 * Dropout contract (csrc/eec_drop.h; restated in oracle/dropout_ref.py): element i of the tensor a site masks is kept when
 * lowbias32(lo(i) * C1 + hi(i) * C2 + key(seed, site)) >= floor(drop_prob * 2^32) and then scaled by 1 / (1 - drop_prob); i is the
 * flat row-major index of [B][T'][D] (positional encoding, the residual sites), [B][T'][F] (feed-forward activations) and
 * [B*H][T'][T'] (attention probabilities), whichever kernel applies the mask.  Site numbers of eec_train_forward: 1 = positional
 * encoding; then 7 per ConformerLayer in the order they run (layer l of exit e: from 2 + 7 * (e * L + l)) -- ffn1 activation, ffn1
 * residual (the module's output), attention probabilities, attention residual (after out_proj), convolution residual (the
 * module's output), ffn2 activation, ffn2 residual.  torch's own dropout streams cannot match these, but an oracle handed the
 * masks of this generator can: parity with the reference's arithmetic holds at drop_prob 0 and, fed the same masks, at
 * drop_prob > 0, at the same bounds (tests/test_gpu_dropout.py).
 * eec_train_forward records the activations the backward needs in `workspace` (eec_trainer_workspace_bytes; the caller
 * keeps it untouched until eec_train_backward); one recorded forward per trainer at a time.
 * eec_train_backward: `out` = the log-probs eec_train_forward returned, `grad_out` = dLoss/d out [E,B,T',V]; `grads` is
 * an eec_params whose pointers are WRITTEN (overwritten, not accumulated) with the gradient of the parameter at the same
 * position (pe / running_mean / running_var entries are ignored).  Gradient with respect to `mel` is not produced.
 * `taps` (optional, [E][B*T'][D]) returns the group outputs the heads read -- what full_conformer feeds its attention decoders
 * (early_exit.py:764-800); `grad_taps` (optional, same shape) is the gradient that arrived at them from outside the path.
 * A trainer is bound to the device that is current in its first eec_train_forward (eec_trainer_workspace_bytes is host
 * arithmetic and needs none), is not thread-safe, and holds ONE recorded forward at a time. */
typedef struct eec_trainer eec_trainer;
const char* eec_trainer_last_error(void);
int eec_trainer_create(const eec_config* cfg, eec_trainer** out);
void eec_trainer_destroy(eec_trainer* tr);
size_t eec_trainer_workspace_bytes(const eec_trainer* tr, int B, int T);
int eec_train_forward(eec_trainer* tr, const eec_params* params, const float* mel, const int64_t* lengths, int B, int T, int passes,
                      float drop_prob, uint64_t seed, float* out, float* taps, float* bn_batch_stats, void* workspace,
                      size_t workspace_bytes, void* stream);
int eec_train_backward(eec_trainer* tr, const eec_params* params, const eec_params* grads, const float* out, const float* grad_out,
                       const float* grad_taps, void* workspace, size_t workspace_bytes, void* stream);
/* The same backward, reporting its progress: the exit groups are differentiated last to first (train.py:60-68 sums the exit
 * losses, so the gradient of group e's parameters is final once the backward has passed group e), and `on_group(e, user)` is
 * called on the host right after the last launch that writes a gradient of exit group e (its layers and its head; e = E-1 ... 0),
 * then once with e = -1 after the stem.  Everything the callback enqueues on `stream` -- or on a stream that waits for it, as
 * torch.distributed's collectives do -- therefore runs behind those gradients and beside the backward of the earlier groups:
 * the hook that lets data-parallel training (BASELINE.json configs[3]) all-reduce bucket e under the backward of group e - 1.
 * The callback must not call into this library. */
typedef void (*eec_group_done_fn)(int group, void* user);
int eec_train_backward_ex(eec_trainer* tr, const eec_params* params, const eec_params* grads, const float* out, const float* grad_out,
                          const float* grad_taps, void* workspace, size_t workspace_bytes, void* stream, eec_group_done_fn on_group,
                          void* user);
/* ---- Building blocks of the training step: what `--model_type splitformer / zipformer` need (train.py:180-208) --------------
 * The same modules as eec_train_forward / _backward, cut where those models put their own glue (strided slices, repeats, adds
 * between Conformer groups: early_exit.py:117-224, 227-364).  Stateless: the activations a backward needs are recorded in the
 * caller's `workspace` (256-byte aligned, *_workspace_bytes; untouched until the matching backward, which takes the same
 * geometry, seed, drop_prob and site numbers).  A GROUP = n_layers ConformerLayers (torchaudio Conformer(num_layers=n_layers))
 * on rows x [B][T'][D] with key lengths key_len [B] (int32, device): x_out [B][T'][D], bn_batch_stats [n_layers][2][D] as in
 * eec_train_forward; the backward writes the gradient of every layer parameter (grads mirrors layers) and grad_in = dLoss/dx_in.
 * site_base numbers the group's dropout sites: layer l of the group uses site_base + 7 * l ... + 6 in the order given at
 * eec_train_forward, the stem the one number `site`; calls of one step must use disjoint ranges (the models' numbering:
 * training.splitformer_sites / zipformer_sites -- stem 1, group g from 16 + 128 * g, a Splitformer branch 64 further).  The STEM =
 * Conv1d(k3, s2) [-> Conv1d(k3, s2) when sub1_* are given] -> + positional encoding -> dropout: x_out [B][To][D], To = T1 or T';
 * no gradient with respect to mel.  The HEAD = log_softmax(x . W^T + b) and the backward of exactly that. */
size_t eec_train_group_workspace_bytes(const eec_config* cfg, int n_layers, int B, int Tq);
int eec_train_group_forward(const eec_config* cfg, const eec_layer_params* layers, int n_layers, const float* x_in, const int32_t* key_len, int B,
                            int Tq, int passes, float drop_prob, uint64_t seed, uint32_t site_base, float* x_out, float* bn_batch_stats,
                            void* workspace, size_t workspace_bytes, void* stream);
int eec_train_group_backward(const eec_config* cfg, const eec_layer_params* layers, const eec_layer_params* grads, int n_layers, const float* x_in,
                             const int32_t* key_len, int B, int Tq, int passes, float drop_prob, uint64_t seed, uint32_t site_base,
                             const float* grad_out, float* grad_in, void* workspace, size_t workspace_bytes, void* stream);
size_t eec_train_stem_workspace_bytes(const eec_config* cfg, int B, int T, int two_convs);
int eec_train_stem_forward(const eec_config* cfg, const float* sub0_w, const float* sub0_b, const float* sub1_w, const float* sub1_b,
                           const float* pe, const float* mel, int B, int T, int passes, float drop_prob, uint64_t seed, uint32_t site, float* x_out,
                           void* workspace, size_t workspace_bytes, void* stream);
int eec_train_stem_backward(const eec_config* cfg, int two_convs, int B, int T, int passes, float drop_prob, uint64_t seed, uint32_t site,
                            const float* grad_x, float* g_sub0_w, float* g_sub0_b, float* g_sub1_w, float* g_sub1_b, void* workspace,
                            size_t workspace_bytes, void* stream);
int eec_train_head_forward(const float* x, const float* W, const float* b, int M, int V, int D, int passes, float* logp, float* scratch /* M*V */,
                           void* stream);
size_t eec_train_head_backward_scratch_floats(int M, int V, int D);
int eec_train_head_backward(const float* x, const float* W, const float* logp, const float* grad_logp, int M, int V, int D, int passes, float* dx,
                            float* dW, float* db, float* scratch, void* stream);
/* C = alpha * A . B^T (+ bias) on the training GEMM (test hook): A [M][K], B [N][K], C [M][N] fp32 row-major on the device */
int eec_train_gemm(const float* A, const float* B, const float* bias, float* C, int M, int N, int K, int passes, int a_transposed,
                   int b_transposed, void* stream);

/* ---- AED decoder forward (full_conformer._decoder_, early_exit.py:739-762; util/beam_infer.py:236-240) ----------------
 * out[Bm][S][V] = (log_softmax of) linears_2[e]( TransformerDecoder_e( positional_encoder_2(emb(trg)), memory = enc ) ) in eval
 * mode: n_layers x nn.TransformerDecoderLayer(batch_first, norm_first: causal + target-padding self-attention,
 * cross-attention over enc [Bm][Tq][D], ReLU feed-forward) and the shared final LayerNorm.  fp32 parameters are read in
 * place (state_dict tensors); arithmetic as the training GEMM (passes 3: bf16 hi/lo split, ~1e-5 of fp32).  trg: int64
 * [Bm][S]; positions equal to pad_idx are masked as keys.  The caller's beam search (util/beam_infer.py:198-307) stays
 * above this call: one call per decoding step on the whole prefix, as the reference (the step-wise form with a key / value
 * cache is eec_decoder_begin / eec_decoder_step below).  enc_shared != 0: every one of the Bm rows attends
 * to the SAME memory enc [1][Tq][D] (beam search expands one utterance over its beams): its keys / values are projected once. */
typedef struct eec_decoder_layer_params {
  const float *sa_in_w, *sa_in_b;   /* self_attn.in_proj_{weight,bias}      [3D,D],[3D] */
  const float *sa_out_w, *sa_out_b; /* self_attn.out_proj.{weight,bias}     [D,D],[D]   */
  const float *ca_in_w, *ca_in_b;   /* multihead_attn.in_proj_{weight,bias}             */
  const float *ca_out_w, *ca_out_b; /* multihead_attn.out_proj.{weight,bias}            */
  const float *w1, *b1, *w2, *b2;   /* linear1 [F,D],[F]; linear2 [D,F],[D]             */
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b, *norm3_w, *norm3_b;
} eec_decoder_layer_params;
typedef struct eec_decoder_params {
  const float* emb;                       /* emb.weight [V,D]                                   */
  const float* pe;                        /* positional_encoder_2.pe [max_len,1,D]              */
  const eec_decoder_layer_params* layers; /* HOST array of n_layers: decoders.e.layers.l        */
  int32_t n_layers, max_len;
  const float *norm_w, *norm_b;           /* layer_norm.{weight,bias} (shared final norm)       */
  const float *head_w, *head_b;           /* linears_2.e.{weight,bias} [V,D],[V]                */
} eec_decoder_params;
const char* eec_decoder_last_error(void);
size_t eec_decoder_workspace_bytes(int d_model, int n_heads, int d_ff, int vocab, int Bm, int S, int Tq);
int eec_decoder_forward(const eec_decoder_params* p, int d_model, int n_heads, int d_ff, int vocab, int pad_idx, const int64_t* trg,
                        const float* enc, int Bm, int S, int Tq, int enc_shared, int passes, int log_softmax, float* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- Teacher-forced scoring of whole hypotheses (csrc/decoder_score.hip): the second pass of two-pass decoding ------------------
 * eec_decoder_score: att_score [n][R] = log p(y, EOS | memory) of R hypotheses for each of n memories under ONE decoder, in one
 * pass.  hyp_tokens [n][R][L] int32, hyp_len [n][R] int32, enc [n][Tq][D]; S = L + 1 <= p->max_len.  Hypothesis y of length
 * k = min(hyp_len, L) has the decoder input row SOS, y_1 .. y_k, then pad_idx up to S positions, and
 *     att_score = sum_{t = 0 .. k} logp[t][target_t],   targets y_1 .. y_k, EOS,
 * where logp is what eec_decoder_forward(..., log_softmax = 1) yields for that row alone against enc[i]: the same masks (causal;
 * keys equal to pad_idx masked -- the reference's rule, so a pad_idx INSIDE a hypothesis is masked as a key too), the same
 * arithmetic (`passes`).  k = 0 scores log p(EOS | SOS).  hyp_len < 0 marks an ABSENT hypothesis: its score is -inf and its
 * tokens are never read.  Token ids outside [0, vocab) are clamped, as the embedding clamps them.  A term that is not a number
 * counts as -inf: no NaN is written.
 * Self-attention and every row-wise GEMM run over the M = n * R * S rows at once; the memory's keys | values are projected once
 * per memory and the cross-attention is one batched GEMM with batch n * H and R * S query rows; the head's [M][V] logits are
 * reduced by eec_hypothesis_score's kernel, and no [M][V] log-probs are written.  No allocation, no synchronisation; results are
 * bit-identical from run to run (no atomics).
 * All checks come before the first launch.  EEC_ERR_BAD_ARG: a null pointer; `passes` not 1 or 3; d_model outside [1, 1024] or
 * not divisible by n_heads; vocab outside [1, 1024]; d_ff, R or Tq below 1; n or L below 0; L >= 8192; S > p->max_len;
 * n * R * n_heads > 65535 or n * R * S > 32 * 65535 (grid dimensions of one call: callers split over memories); pad_idx, sos
 * or eos outside [0, vocab).  EEC_ERR_WORKSPACE: a workspace that is not 256-byte aligned or shorter than
 * eec_decoder_score_workspace_bytes (0 for a geometry the entry rejects, and for n = 0).  n = 0 succeeds and launches nothing.
 * The workspace grows with n * H * R * S * max(S, Tq) (attention probabilities) and M * d_ff floats: callers bound it by
 * splitting over memories.
 *
 * eec_hypothesis_score: the reduction alone, on given logits [n_hyp * (L + 1)][vocab] (16-byte aligned where
 * vocab is a multiple of 4: such rows are read a float4 at a time): one wave per row takes
 * the maximum, the log-sum-exp and (x[target] - max) - log(sum); the k + 1 terms of a hypothesis are added in index order in
 * fp64 and rounded once.  Error of a hypothesis against the exact sum: within (k + 1) * (2^-22 * max|logit| + 4e-7). */
size_t eec_decoder_score_workspace_bytes(int d_model, int n_heads, int d_ff, int vocab, int n, int R, int L, int Tq);
int eec_decoder_score(const eec_decoder_params* p, int d_model, int n_heads, int d_ff, int vocab, int pad_idx, int sos, int eos,
                      const int32_t* hyp_tokens, const int32_t* hyp_len, const float* enc, int n, int R, int L, int Tq, int passes,
                      float* att_score, void* workspace, size_t workspace_bytes, void* stream);
int eec_hypothesis_score(const float* logits, const int32_t* hyp_tokens, const int32_t* hyp_len, int n_hyp, int L, int vocab, int eos,
                         float* att_score, void* stream);


/* ---- Training step of the AED decoder (csrc/decoder_train.hip): what autograd does through the decoder half of
 * full_conformer.forward in train mode (early_exit.py:764-800; train.py:36-52, --decoder_mode aed) -----------------------------
 * eec_decoder_train_forward: out [Bm][S][V] = RAW logits (the reference comments the log_softmax out, early_exit.py:790) of exit
 * `exit_index`'s decoder on targets trg [Bm][S] (int64; pad_idx positions masked as keys) over the memory enc [Bm][Tq][D], with
 * dropout of probability drop_prob at the reference's sites (after the positional encoding -- site shared by the exits of a
 * forward, the reference embeds the targets once --, on both attention-probability tensors, after the three sub-modules, inside
 * the feed-forward), from the counter-based generator keyed by (seed, exit_index).  It records what the backward needs in
 * `workspace` (eec_decoder_train_workspace_bytes; 256-byte aligned; keep it untouched until the backward).
 * eec_decoder_train_backward (same geometry, trg, enc, seed, drop_prob, exit_index): grad_out = dLoss / d out; `grads` mirrors
 * `p` with pointers that are WRITTEN with the gradient of the parameter in the same position (emb [V][D]; pe ignored; layers a
 * host array); grad_enc [Bm][Tq][D] is written with the gradient of the memory (what flows on into the encoder's backward as
 * eec_train_backward's grad_taps).  The shared final LayerNorm and the embedding receive one such gradient per exit: the caller
 * sums them (autograd does).  Dropout sites (generator and index convention as at eec_train_forward): 0 = positional encoding
 * over [Bm*S][D], the same for every exit; layer l of exit e uses 1 + 1024 * e + 6 * l + place, place = 0 self-attention
 * probabilities [Bm*H][S][S], 1 residual 1, 2 cross-attention probabilities [Bm*H][S][Tq], 3 residual 2, 4 feed-forward activation
 * [Bm*S][F], 5 residual 3 ([Bm*S][D]).  Parity with the reference's modules holds at drop_prob 0 and, with the modules fed these
 * masks, at drop_prob > 0 (tests/test_gpu_dropout.py). */
const char* eec_decoder_train_last_error(void);
size_t eec_decoder_train_workspace_bytes(int d_model, int n_heads, int d_ff, int vocab, int n_layers, int Bm, int S, int Tq);
int eec_decoder_train_forward(const eec_decoder_params* p, int d_model, int n_heads, int d_ff, int vocab, int pad_idx, const int64_t* trg,
                              const float* enc, int Bm, int S, int Tq, int passes, float drop_prob, uint64_t seed, int exit_index, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int eec_decoder_train_backward(const eec_decoder_params* p, const eec_decoder_params* grads, int d_model, int n_heads, int d_ff, int vocab,
                               const int64_t* trg, const float* enc, int Bm, int S, int Tq, int passes, float drop_prob, uint64_t seed,
                               int exit_index, const float* grad_out, float* grad_enc, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Step-wise AED decoding with a key / value cache (csrc/decoder_step.hip) ----------------------------------------------------
 * What util/beam_infer.py:233-240 needs from `_decoder_` is the LAST position's log-probs of every live beam; the reference gets
 * them by re-running the decoder over the whole prefix at every step.  A session here is a caller-owned device buffer `cache`
 * (eec_decoder_cache_bytes) holding the memory keys / values of ONE utterance's encoder output (projected once by
 * eec_decoder_begin), the self-attention keys / values of every (position, beam slot) decoded so far and each beam's ancestry.
 *   eec_decoder_begin(p, ..., enc [Tq][D], Tq, S_max, passes, cache, bytes, stream)
 *   eec_decoder_step (p, ..., pad_idx, last_tokens [R], parent [R] | NULL, R, R_prev, s, Tq, S_max, log_softmax, out [R][V], ...)
 * step s = 0, 1, 2, ... in order (s < S_max <= p->max_len): last_tokens[r] is beam r's token at position s, parent[r] the row of the
 * PREVIOUS step that beam r extends (NULL: r itself; ignored at s = 0), R_prev that step's beam count; 1 <= R <=
 * eec_decoder_step_max_beams() (16).  out[r] = log_softmax (or the raw logits) of the exit head at position s -- what
 * `_decoder_(prefix_r, enc, exit)[:, -1]` returns.  Plain fp32 arithmetic; the memory projection of _begin runs on the training
 * GEMM (`passes` as eec_decoder_forward).  EEC_ERR_UNSUPPORTED for geometries outside head dim 8 / 16 / 32 / 64, d_model <= 1024
 * and d_ff <= 2048 (multiples of 4): callers then stay on eec_decoder_forward. */
const char* eec_decoder_step_last_error(void);
int eec_decoder_step_max_beams(void);
size_t eec_decoder_cache_bytes(int d_model, int n_heads, int d_ff, int vocab, int n_layers, int S_max, int Tq);
int eec_decoder_begin(const eec_decoder_params* p, int d_model, int n_heads, int d_ff, int vocab, const float* enc, int Tq, int S_max,
                      int passes, void* cache, size_t cache_bytes, void* stream);
int eec_decoder_step(const eec_decoder_params* p, int d_model, int n_heads, int d_ff, int vocab, int pad_idx, const int64_t* last_tokens,
                     const int64_t* parent, int R, int R_prev, int s, int Tq, int S_max, int log_softmax, float* out, void* cache,
                     size_t cache_bytes, void* stream);
/* The same step for n <= 8 sessions at once -- the E exits of one utterance, which inference.py:44-51 decodes one after the other:
 * every launch of the step covers all sessions (one more grid dimension), so E searches cost the launches of one.  ps / caches: HOST
 * arrays of n pointers (sessions of one decoder geometry, each begun with eec_decoder_begin); last_tokens [n][R], parent [n][R] | NULL,
 * out [n][R][V]; R, R_prev and s are common to the sessions (they advance in lockstep). */
int eec_decoder_step_multi(int n, const eec_decoder_params* const* ps, int d_model, int n_heads, int d_ff, int vocab, int pad_idx,
                           const int64_t* last_tokens, const int64_t* parent, int R, int R_prev, int s, int Tq, int S_max, int log_softmax,
                           float* out, void* const* caches, size_t cache_bytes, void* stream);
/* ---- Batched step-wise AED decoding (csrc/decoder_batch.hip) ----------------------------------------------------------------
 * The step above for every exit AND every utterance of a padded batch at once: E <= 8 exits x B utterances, R <= 16 live beams per
 * utterance, one cache (eec_decoder_batch_cache_bytes) for all of them.  The launches of a step do not depend on E or B: each linear
 * is one GEMM over the B * R rows of every exit (f16x3 MFMA operands, ~2^-21 relative per product; the weights are split after an
 * exact factor 2^8, so that holds for 2^-11 <= |w| <= 255 -- measured against an fp64 oracle at 0.014 / 0.017 / 0.112 of
 * 4e-5 * max(10, max |logp|) with the feed-forward and value weights scaled by 2^0 / 2^-4 / 2^-8, 1.30 at 2^-8 without the factor),
 * the cross-attention reads an utterance's memory once for all of its beams.  The search's bookkeeping is eec_beam_select with
 * n = E * B.
 *   eec_decoder_batch_begin(ps, E, B, ..., taps [E][B][Tq][D], Tq, S_max, passes, cache, bytes, stream)
 *   eec_decoder_batch_step (ps, E, B, ..., pad_idx, last_tokens [E][B][R], parent [E][B][R] | NULL, R, R_prev, s, Tq, S_max,
 *                           out [E][B][R][V], cache, bytes, stream)
 * ps: HOST array of E pointers (exit e's decoder; one geometry).  Every utterance has the full padded Tq memory frames (no memory
 * mask, as the reference's per-utterance search).  Step semantics as eec_decoder_step; out holds log-probs.  The cache size is
 * host arithmetic: 0 for geometries eec_decoder_cache_bytes does not serve, or E outside 1 .. 8.  Errors through
 * eec_decoder_step_last_error(); arguments are checked before any device call. */
size_t eec_decoder_batch_cache_bytes(int d_model, int n_heads, int d_ff, int vocab, int n_layers, int E, int B, int S_max, int Tq);
int eec_decoder_batch_begin(const eec_decoder_params* const* ps, int E, int B, int d_model, int n_heads, int d_ff, int vocab, const float* taps,
                            int Tq, int S_max, int passes, void* cache, size_t cache_bytes, void* stream);
int eec_decoder_batch_step(const eec_decoder_params* const* ps, int E, int B, int d_model, int n_heads, int d_ff, int vocab, int pad_idx,
                           const int64_t* last_tokens, const int64_t* parent, int R, int R_prev, int s, int Tq, int S_max, float* out, void* cache,
                           size_t cache_bytes, void* stream);
/* The bookkeeping of one beam-search step (util/beam_infer.py:241-262) for n searches in lockstep, one launch: over the R live beams'
 * V next-token log-probs, cand = scores_in[r] + logp[r][v] / penalty; the K best, best first (ties: the lower r * V + v) ->
 * scores_out [n][K], parent [n][K] (= index / V), tok [n][K] (= index % V); tokens_new[i][b][0 .. len] = tokens_old[i][parent][0 .. len)
 * followed by tok.  Token buffers: [n][rows_ld][ld] int64, len tokens per beam so far.  R, K <= 16. */
int eec_beam_select(int n, int R, int V, int K, const float* logp, const float* scores_in, float penalty, float* scores_out, int64_t* parent,
                    int64_t* tok, const int64_t* tokens_old, int64_t* tokens_new, int len, int ld, int rows_ld, void* stream);

/* ---- CTC prefix scores for one-pass joint CTC / attention decoding (csrc/ctc_prefix.hip) --------------------------------------
 * The model is trained on 0.7 * CE + 0.3 * CTC at every exit; one-pass joint decoding (Watanabe et al. 2017) lets the two heads
 * meet INSIDE the search: at every step each candidate extension of each live beam is scored by the decoder and by the CTC prefix
 * probability of the extended label sequence, an EOS candidate by the full-sequence CTC likelihood -- which gives the search a
 * principled way to stop.  The reference has no such search; the semantics are stated here, restated in float64 in
 * tests/ctc_prefix_cases.py and pinned by a brute-force enumeration of all V^T paths.
 *
 * One search: x[t][v] the emission (CTC log-probs) for t < T (T = em_len clamped to [1, T'], T' without em_len), `blank` the blank id.
 * A hypothesis is SOS followed by labels g; SOS is not a CTC label.  All arithmetic is fp32 in the written order; log_add is the
 * sequence stated for eec_ctc_log_add, and log_add(-inf, a) = a.
 *   State of a hypothesis: rn[t], rb[t] (t < T) and pfx.  rn[t]: log-probability of all paths over frames 0..t that collapse to g and
 *     end in a non-blank; rb[t]: the same for paths that end in blank; pfx: the log prefix probability of g.  It also carries its
 *     last label `last` (none for empty g) and a flag `done`.
 *   Begin (empty g): rn[t] = -inf; rb[t] = x[0][blank] + ... + x[t][blank] (summed in that order); pfx = 0.
 *   Extending g (state rn, rb) by a label c != blank:
 *     nn[0] = x[0][c] if g is empty, else -inf;  nb[0] = -inf;  psi = nn[0];
 *     for t = 1 .. T-1:  phi = rb[t-1] if c == last, else log_add(rn[t-1], rb[t-1]);
 *                        nn[t] = log_add(nn[t-1], phi) + x[t][c];  nb[t] = log_add(nn[t-1], nb[t-1]) + x[t][blank];
 *                        psi = log_add(psi, phi + x[t][c]).
 *     psi is the prefix log-probability of g.c, (nn, nb) its state.  A sequence that contains the blank has probability zero:
 *     extending by c == blank gives psi = -inf and a state of -inf.  Full-sequence score of g: full = log_add(rn[T-1], rb[T-1]).
 *   Joint local score of live beam r, token v, weight w in (0, 1]:
 *     done beam:  local[r][pad] = 0, every other token -inf.
 *     open beam:  ctc[r][v] = -inf for v == blank;  -inf for every v when pfx_r == -inf;  full_r - pfx_r for v == eos (-inf while
 *                 s < min_length);  psi(g_r.v) - pfx_r otherwise.
 *                 local[r][v] = -inf if ctc[r][v] is -inf, else (1 - w) * att[r][v] + w * ctc[r][v]; a result that is a NaN (a
 *                 non-finite att) becomes -inf.  No NaN ever leaves the kernel.
 *   Selection is eec_beam_select on `local`, unchanged (the reference's division by the length penalty, its tie rule).
 *   After the selection, beam b with parent p and token v:  parent done: the parent's state is copied and b stays done;  else
 *     v == eos: done = 1 and pfx = full_p;  else: pfx = psi(g_p.v), last = v, and the state is the extended one.
 *   End of the search: after max_length steps every row is final as it stands; after EOS a row holds only PAD.  The best beam is
 *   the one with the highest score, ties to the lower index.
 *
 * eec_ctc_prefix_state_bytes(n, R_max, T'): the session's state, caller-owned device memory, 16-byte aligned: two buffers of
 *   n * R_max slots of 4 + 256 + 3 * T' floats (rounded up to 4) -- O(n * R * T'); states of candidates are never stored.  0 for an
 *   argument <= 0.
 * eec_ctc_prefix_begin(logp [n][T'][V], em_len [n] | NULL, n, T', V, blank, R_max, state, bytes, stream): the empty hypothesis.
 * eec_ctc_prefix_step(logp, em_len, n, T', V, blank, R_max, parent [n][R] | NULL, last_tokens [n][R], R, R_prev, s, att [n][R][V], w,
 *                     eos, pad, min_length, local_out [n][R][V], state, bytes, stream):  step s = 0, 1, 2, ... in order, with the
 *   arguments of eec_decoder_batch_step: last_tokens[i][r] is beam r's newest token (SOS at s = 0, where it is not read), parent[i][r]
 *   the row of the previous step it extends (NULL: r itself; not read at s = 0), R_prev that step's beam count.  The call first
 *   advances the state to the R current beams (the "after the selection" rule for the previous step's choice), then writes `local`
 *   for all V tokens of every beam.  The whole vocabulary is scored; there is no attention pre-pruning.  A parent outside [0, R_prev)
 *   or a token outside [0, V) is never used as an address: that beam's prefix probability becomes zero (pfx = -inf).
 *   n = E * B searches (search e * B + b), R <= R_max <= 16, 2 <= V <= 256 (the decoder's vocabulary is the CTC vocabulary),
 *   T' <= 2048; blank, eos and pad pairwise distinct.
 * Checks, all before any device call, errors through eec_last_error(): EEC_ERR_BAD_ARG for n < 0, T' < 1, V < 2, R_max < 1, blank /
 *   eos / pad outside [0, V) or not distinct, R or R_prev outside 1 .. R_max, s < 0, w outside (0, 1], a null required pointer;
 *   EEC_ERR_UNSUPPORTED for V > 256, R_max > 16, T' > 2048; EEC_ERR_WORKSPACE for a misaligned or short state; n == 0 is a successful
 *   no-op.  One launch per call on `stream` (one workgroup per (beam, search), one work-item per token; two dependent chains of T
 *   log_adds); no allocation, no synchronisation; graph-capturable; no atomics, vector stores only; results are bit-identical run to
 *   run and do not depend on n. */
size_t eec_ctc_prefix_state_bytes(int n, int R_max, int Tq);
int eec_ctc_prefix_begin(const float* logp, const int32_t* em_len, int n, int Tq, int V, int blank, int R_max, void* state, size_t state_bytes,
                         void* stream);
int eec_ctc_prefix_step(const float* logp, const int32_t* em_len, int n, int Tq, int V, int blank, int R_max, const int64_t* parent,
                        const int64_t* last_tokens, int R, int R_prev, int s, const float* att, float w, int eos, int pad, int min_length,
                        float* local_out, void* state, size_t state_bytes, void* stream);

/* ---- Contextual biasing: hot phrases in the CTC and AED beam searches (csrc/ctx_graph.hip, csrc/ctc_beam_ctx.hip) -------------------
 * Telling a search which phrases to expect: WeNet's "context graph", icefall / sherpa's ContextGraph.  The reference has nothing of the
 * kind (its cuda_ctc_decoder is third-party and takes no context): an addition, not a parity item.  tests/ctxbias_cases.py restates
 * everything below in fp64 and Python integers.
 *
 * Graph.  P >= 0 phrases over a vocabulary of V <= 256 tokens; a phrase is a non-empty row of tokens of [0, V), none of them blank, eos
 * or pad, with a finite per-token boost b_p >= 0.  The trie of the phrases has node 0 as its root; nodes are numbered in the order in
 * which inserting the phrases one after the other creates them.
 *     token_score(n)  the largest b_p over the phrases through n
 *     node_score(n)   node_score(parent) + token_score(n), node_score(0) = 0
 *     end(n)          a phrase ends at n
 *     fail(n)         the longest proper suffix of n's path that is a trie node (the Aho-Corasick failure link); fail of a child of the
 *                     root is the root
 *     out(n)          (end(n) ? node_score(n) : 0) + out(fail(n)), out(0) = 0: the end nodes on the chain n, fail(n), fail(fail(n)), ...
 *     goto(s, v)      child v of the first node on s's failure chain that has one, else the root
 *     delta(s, v)     (node_score(goto) - node_score(s)) + out(goto)        final(s) = 0 - node_score(s)
 * all in fp64 in the order written.  The open bonus node_score(s) is provisional: leaving a partial match pays it back, final(s) takes
 * it back at the end of a hypothesis, and a completed phrase pays node_score of its end node once more, for good.  So the bias of a
 * finished hypothesis y is the sum, over every occurrence of every phrase in y (overlapping and nested ones count), of node_score of
 * that phrase's end node.  Special tokens: blank keeps the state and pays 0 (the CTC search never takes it; it is a row of the
 * tables all the same).  With eos and / or pad given (-1: none) there is one more state behind the trie's, the dead one:
 * goto(s, eos) = dead and delta(s, eos) = final(s), pad alike; every token leaves the dead state at 0 into itself and final(dead) = 0.
 * The bias is accumulated in fp32 along the prefix, one rounded add per token, bias(y . v) = fl(bias(y) + delta): a function of the
 * token row alone.
 *
 * Image (host only, no device call; the size-query-then-fill form of eec_resample_plan).  G graphs in one image of int32 words:
 *     word 0 EEC_CTX_MAGIC, 1 G, 2 the image's size in words, 3 V
 *     graph g, words 4 + 4 g ..:  S (states), then the word offsets of delta [S][V] fp32 (the fp64 value rounded once), of
 *     next [S][V] int32 and of final [S] fp32
 * n_phrases [G] phrases per graph (0: a graph that biases nothing), phrase_len / boost one entry per phrase, graph after graph,
 * `tokens` the phrases' tokens one after the other.  Failure links are resolved here; the device never follows one.  Refused with a
 * message (EEC_ERR_BAD_ARG, before anything is written; *_bytes returns 0): G outside [1, EEC_CTX_MAX_GRAPHS], more than
 * EEC_CTX_MAX_STATES states over all graphs (64 MB of tables at V = 256), a phrase of more than EEC_CTX_MAX_PHRASE tokens or of none,
 * a token outside [0, V), blank, eos or pad inside a phrase, a boost that is negative or not finite (or a phrase whose boosts add up
 * beyond the fp32 range), V outside [1, 256], blank outside [0, V), a null pointer; (EEC_ERR_WORKSPACE) a short image.  The limits are
 * choices, not measurements.
 * A sequence chooses its graph by graph_of [n_seq] int32 on the device; NULL: graph 0 for all; an index outside [0, G) switches biasing
 * off for that sequence, as does image == NULL.  The kernels never trust an image: a header that does not describe tables inside
 * image_bytes switches biasing off, a `next` value outside [0, S) is taken as the root.
 *
 * CTC prefix beam search: eec_ctc_beam_decode_ctx (the best-prefix end) and eec_ctc_beam_decode_nbest_ctx (the N-best end) take the
 * arguments of eec_ctc_beam_decode_len / _nbest and image, image_bytes, graph_of and bias ([n_seq], [n_seq][nbest]).  It is that search
 * (csrc/ctc_beam.hip compiled with EEC_CTC_CTX) with one change: every ranking compares key = fl(total log-probability + bias).  A stay
 * keeps its prefix's state and bias; an extension of beam i by label c has bias fl(bias_i + delta[state_i][c]) and state
 * next[state_i][c], its key is fl(mass + that bias); an extension that spells an existing prefix merges into it as before (that
 * prefix's bias is the same number by construction).  A blank-skipped frame changes nothing; candidate ids and tie rules are unchanged.
 * At the end each prefix's bias becomes fl(bias + final[state]) and both ends rank by fl(total + that).  scores stays the CTC
 * log-probability alone, so downstream mixing keeps its meaning; bias is returned beside it (0 for an absent hypothesis).  An empty
 * graph, graph_of = -1, no image and all-zero boosts return the tokens, counts and scores of the entries without context bit for
 * bit, with bias 0.  Nothing is read back and there are no atomics: graph-capturable; two runs and a split batch (graph_of sliced to
 * match) return the same bits.
 *
 * AED lockstep search: eec_context_bias_step, with the place eec_ctc_prefix_step has in the loop.  One launch, one workgroup per
 * (search, beam) row.  state: int32 [2][n][R_max], eec_context_bias_state_bytes(n, R_max) bytes; step s reads half s & 1 and writes
 * the other.  Row (i, r): state = root at s == 0 (the token there is SOS and is not read), else
 * next[state_prev[parent[i][r]]][last[i][r]] (parent == NULL: r; a parent outside [0, R_prev) or a token outside [0, V): the root);
 * then out[i][r][v] = local[i][r][v] + delta[state][v], one fp32 add per element, an entry at -inf stays -inf; out == local is
 * allowed.  The bonus is part of the step's log-prob and therefore shares the step's length penalty: the closed form above holds for
 * pen_alpha = 0.  The graph for these searches is built with eos and pad, so a beam's bias stops at its EOS with the open bonus taken
 * back.  A search that declares its rows final without an EOS (the lockstep searches do, after max_length steps) adds
 * final[next[state][last token]] to each row's score itself, at the last step's penalty: one gather on the image, once per search
 * (ContextBiasSession.final), so that every final score carries the closed form.  EEC_ERR_BAD_ARG: a null pointer, R or R_prev outside [1, R_max], R_max outside [1, 16], V outside [1, 256]; n == 0 is a
 * successful no-op. */
#define EEC_CTX_MAGIC 0x43545847
#define EEC_CTX_MAX_GRAPHS 1024
#define EEC_CTX_MAX_STATES 32768
#define EEC_CTX_MAX_PHRASE 64
size_t eec_context_graph_bytes(int G, const int32_t* n_phrases, const int32_t* phrase_len, const int32_t* tokens, const double* boost, int V,
                               int blank, int eos, int pad);
int eec_context_graph(int G, const int32_t* n_phrases, const int32_t* phrase_len, const int32_t* tokens, const double* boost, int V, int blank,
                      int eos, int pad, void* image, size_t image_bytes);
int eec_ctc_beam_decode_ctx(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                            float blank_skip_threshold, int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts,
                            float* scores, const void* image, size_t image_bytes, const int32_t* graph_of, float* bias, void* stream);
int eec_ctc_beam_decode_nbest_ctx(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                                  float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens,
                                  int32_t* counts, float* scores, int32_t* n_hyp, const void* image, size_t image_bytes,
                                  const int32_t* graph_of, float* bias, void* stream);
size_t eec_context_bias_state_bytes(int n, int R_max);
int eec_context_bias_step(const void* image, size_t image_bytes, const int32_t* graph_of, int n, int R, int R_prev, int R_max, int V, int s,
                          const int64_t* parent, const int64_t* last, const float* local, float* out, void* state, size_t state_bytes,
                          void* stream);

/* ---- Shallow fusion: token-level n-gram model (csrc/lm_fusion.hip, csrc/ctc_beam_lm.hip, csrc/eec_lm.h) -----------------------------
 * A back-off n-gram over the model's own tokens (sentencepiece pieces), added to the scores of the lexicon-free searches: the CTC
 * prefix beam search and the AED lockstep searches.  WeNet, ESPnet and icefall offer the same; the reference's cuda_ctc_decoder and
 * its AED beam search take no LM: an addition, not a parity item.  tests/lmfusion_cases.py restates everything below in plain
 * Python and NumPy fp32 / fp64.
 *
 * Model.  A packed n-gram image as eec_ngram_pack makes it (above), with lex_words = V and word_map[v] the LM word of token v: ARPA
 * words are piece strings, a piece the model lacks maps to <unk> (refused on the host when the model has none).  Values stay the
 * file's log10 numbers; the weight absorbs ln 10.  At most 512 LM words (V <= 256 pieces and the three special words).
 * Special tokens are arguments of the kernels and never looked up: `skip` tokens (blank, SOS, PAD; -1: none) pay 0 and keep the state;
 * `eos` (-1: none) is tested before the skip tokens and scores as </s> when the model has one (header word 7), else with acc = 0;
 * after `eos` a row is in the dead state, -1, where every token pays 0 and the state stays dead.  The start state is header word 6:
 * <s>'s unigram, or the root.
 * Increment of token v from state s:  acc = lm_walk(view, s, word_map[v], next) -- the walk stated above, in its addition order,
 * beginning at acc = 0 --, inc = fl(fl(lm_weight * acc) + token_score): the product is rounded on its own, no fused multiply-add.
 * token_score is the per-token insertion bonus; skip tokens and dead rows do not receive it (their inc is 0).  The state after v
 * is `next`.  An entry whose inc is 0 keeps its bits.
 * Fusion score of a row: fusion(y . v) = fl(fusion(y) + inc) in fp32 along the prefix, fusion() = 0: a function of the token row alone.
 * Never trust the image: fusion is off for the call and the input is returned bit for bit when the image pointer is NULL, the magic
 * is wrong, header word 5 is not V, the counts of the header contradict each other or the sections do not lie inside the image's
 * bytes.  A state outside [0, n_nodes) is taken as the root, an edge bound or a suffix outside its section is brought back into it,
 * a word_map entry outside the LM words reads as word 0, and the sixth node of a suffix chain is read as the root (a packed image
 * reaches it within five): no value of the image is ever an address outside it.
 *
 * AED lockstep search: eec_lm_fusion_step, with the place and the argument order of eec_context_bias_step (no graph_of), then
 * lm_weight, token_score, eos and three skip tokens.  state: int32 [2][n][R_max], eec_lm_fusion_state_bytes(n, R_max) bytes; step s
 * reads half s & 1 and writes the other.  Row (i, r): the start state at s == 0 (the token there is SOS and is not read), else the
 * state after last[i][r] from state_prev[parent[i][r]] (parent == NULL: r; a parent outside [0, R_prev) or a token outside [0, V):
 * the start state); then out[i][r][v] = fl(local[i][r][v] + inc(state, v)); -inf stays -inf; out == local is allowed.  The increment
 * is part of the step's log-prob and shares its length penalty: the closed form holds for pen_alpha = 0.  One launch, one workgroup
 * per row, one work-item per token; the row's suffix chain is walked once and each chain node's edges are scattered into one LDS
 * row, deepest node last, which leaves lm_walk's bits.  With lm_weight == 0 and token_score == 0 the states advance and out is
 * local's bits.  EEC_ERR_BAD_ARG: a null pointer, R or R_prev outside [1, R_max], R_max outside [1, 16], V outside [1, 256], a weight
 * or bonus that is not finite; n == 0 is a successful no-op.  No atomics, nothing read back, graph-capturable, bit-identical run to
 * run and independent of n.
 *
 * CTC prefix beam search: eec_ctc_beam_decode_lm (the best-prefix end) and eec_ctc_beam_decode_nbest_lm (the N-best end) take the
 * arguments of eec_ctc_beam_decode_len / _nbest and lm, lm_bytes, lm_weight, token_score and fusion ([n_seq], [n_seq][nbest]).  It is
 * that search (csrc/ctc_beam.hip compiled with EEC_CTC_LM) under the change contextual biasing makes: a beam grows by a state and a
 * bias, every ranking compares key = fl(total log-probability + bias).  The blank is this search's one skip token and it has no eos:
 * every other label is scored through word_map.  An extension of beam i by label c has bias fl(bias_i + inc(state_i, c)) and the
 * state after c; stays, merges, blank-skipped frames, candidate ids and tie rules are unchanged.  At the end, when the model has
 * </s>, each prefix's bias becomes fl(bias + fl(lm_weight * acc(</s>))) from its state, and both ends rank by fl(total + that).
 * scores stays the CTC log-probability alone; fusion is returned beside it (0 for an absent hypothesis).  lm == NULL, an image that
 * is not trusted, or lm_weight == 0 with token_score == 0 return the tokens, counts and scores of the entries without a model bit
 * for bit, with fusion 0.  EEC_ERR_BAD_ARG also for a weight or bonus that is not finite.  A context graph and a model in one CTC
 * call are not served.  Graph-capturable; two runs and a split batch return the same bits. */
int eec_ctc_beam_decode_lm(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                           float blank_skip_threshold, int skip_drops_frame, void* workspace, int32_t* tokens, int32_t* counts,
                           float* scores, const void* lm, size_t lm_bytes, float lm_weight, float token_score, float* fusion, void* stream);
int eec_ctc_beam_decode_nbest_lm(const float* logp, const int32_t* em_len, int n_seq, int Tq, int V, int blank, int beam_size,
                                 float blank_skip_threshold, int skip_drops_frame, int nbest, void* workspace, int32_t* tokens,
                                 int32_t* counts, float* scores, int32_t* n_hyp, const void* lm, size_t lm_bytes, float lm_weight,
                                 float token_score, float* fusion, void* stream);
size_t eec_lm_fusion_state_bytes(int n, int R_max);
int eec_lm_fusion_step(const void* lm, size_t lm_bytes, int n, int R, int R_prev, int R_max, int V, int s, const int64_t* parent,
                       const int64_t* last, const float* local, float* out, void* state, size_t state_bytes, float lm_weight,
                       float token_score, int eos, int skip0, int skip1, int skip2, void* stream);

/* ---- Keyword spotting on CTC emissions (csrc/keyword.hip) ------------------------------------------------------------------------------
 * "Does this emission contain one of these phrases, and where": for every (emission, keyword) pair the best segment of the emission
 * whose frames CTC-collapse to the keyword, without decoding the utterance.  Max over paths only (no log-add).  The reference has
 * nothing of the kind: an addition, not a parity item.  tests/kws_cases.py restates everything below in scalar fp32 loops and checks
 * it against a brute force over all segments and label paths.
 *
 * Inputs.  Emission x [T', V] fp32 -- log-probs or logits: the score is invariant to a per-frame shift --, T = clamp(em_len, 0, T').
 * Keyword y_1 .. y_L, no y_j equal to `blank`.  States s = 0 .. 2L - 2: lab(s) = y_{s/2 + 1} for even s, `blank` for odd s.  A match
 * starts on a frame of y_1 and ends on a frame of y_L: there are no boundary blanks.
 * Frame term.  m[t] = max_v x[t][v];  e[t][s] = fl(x[t][lab(s)] - m[t]), and -inf for every s when m[t] is not finite.  Every term is
 * at most 0; a path scores 0 exactly when greedy decoding spells it.
 * Recurrence.  Before frame 0 every d is -inf and every start -1.  At frame t state s takes a candidate (c, start) from these sources,
 * in this order, a later one replacing an earlier one only if it is strictly greater:
 *   1. d[t-1][s];  2. d[t-1][s-1] for s >= 1;  3. d[t-1][s-2] for even s >= 2 with lab(s) != lab(s-2);  4. for s = 0 only, the fresh
 *   start (0, t).
 * Then d[t][s] = fl(c + e[t][s]); the start travels with the candidate and becomes -1 again when d[t][s] is -inf.
 * Outputs.  trace_score[t] = d[t][2L-2] and trace_start[t] its start for t < T; -inf and -1 for T <= t < T'.  score = the maximum of
 * the trace over t, end = the first t that attains it, start = that frame's start; -inf, -1, -1 with no reachable end.  The tie
 * rules are local: only the score is a global maximum, and [start, end] is a segment that attains it.
 * Frames at or past a length are never read: a NaN there reaches nothing.  A NaN inside a valid frame gives unspecified scores and
 * never an address out of range.  fp32 subtract, add and compare only: the kernel and a host restatement agree bit for bit.
 *
 *   logp [n_em, T', V] fp32, from any 4-byte boundary; V need not be a multiple of 4.  em_len [n_em] int32, or NULL = T' for all.
 *   tokens [K, tok_stride] int32, tok_len [K] int32 (L), both on the device; blank in [0, V)
 *   score fp32, start, end int32: [n_em, K]
 *   trace_score fp32, trace_start int32: [n_em, K, T'], or both NULL
 *   workspace: eec_keyword_search_workspace_bytes(n_em, T') bytes (the frame maxima), 256-byte aligned
 * Refused before any device work.  EEC_ERR_BAD_ARG: K outside [1, 65536], tok_stride -- the table's width, hence the longest keyword --
 * outside [1, 64], T' outside [1, 2^20], n_em < 1, V < 2, blank outside [0, V), a null required pointer, one trace pointer without the
 * other.  EEC_ERR_UNSUPPORTED: n_em * T' or n_em * ceil(K / 4) at or above 2^31.  EEC_ERR_WORKSPACE: a null, misaligned or too small
 * workspace.  The entry never reads device memory, so what only the table's contents show is the owner's to refuse: the package's
 * KeywordSet is the one maker of token tables and raises for a length outside [1, 64] and for a token equal to `blank` or outside
 * [0, V).  The device trusts neither: em_len is clamped, and a keyword with a length outside [1, tok_stride] or with such a token gets
 * the fill values (-inf, -1, -1, the trace likewise) without any of its tokens becoming an address.
 * Two launches (frame maxima; one wavefront per (emission, keyword)), no atomics, nothing read back, no allocation, no
 * synchronisation; graph-capturable; two runs, a split over keywords and a split over emissions return the same bits. */
size_t eec_keyword_search_workspace_bytes(int n_em, int Tq);
int eec_keyword_search(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                       int K, int tok_stride, int blank, float* score, int32_t* start, int32_t* end, float* trace_score,
                       int32_t* trace_start, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC forced alignment, standard topology (csrc/ctc_forced_align.hip) -----------------------------------------------------------------
 * "When was each token said, for how long, and how surely": the Viterbi path of a token row through the real CTC topology of one
 * emission -- 2N + 1 states, optional blanks, a blank forced between equal neighbours -- and the spans and scores read off it.  Max
 * over paths only.  eec_ctc_align above is the reference's trellis (one frame per token, kept quirk for quirk) and stays what it is;
 * the reference has nothing like this entry: an addition, not a parity item.  tests/forced_align_cases.py restates everything below in
 * scalar fp32 and checks it against a brute force over all frame labellings.
 *
 * Inputs, per hypothesis h.  x = logp[em_index[h]] ([T', V] fp32, log-probs or logits), T = clamp(em_len[em_index[h]], 0, T') (em_len
 * NULL: T'), y the N = tok_len[h] labels of tokens[h].  States s = 0 .. 2N: lab(s) = blank for even s, y[(s-1)/2] for odd s.
 * Recursion.  a[0][0] = x[0][blank], a[0][1] = x[0][y_0], all others -inf.  For t >= 1 the candidates of state s are, in this order:
 *   stay a[t-1][s];  step a[t-1][s-1] for s >= 1;  skip a[t-1][s-2] for odd s >= 3 with y[(s-1)/2] != y[(s-3)/2].
 * best starts as stay and is replaced only by a strictly greater (>) later candidate, so ties go stay, then step, then skip.  d[t][s]
 * in {0, 1, 2} is the move taken and a[t][s] = best + x[t][lab(s)], one fp32 add.  -inf is an ordinary value, and a decision is only
 * ever one of the moves the state has.
 * End and backtrack.  s_end = 2N if a[T-1][2N] > a[T-1][2N-1], else 2N - 1;  path_score = a[T-1][s_end].  s = s_end; for t = T-1 down
 * to 1: state[t] = s, s -= d[t][s]; then state[0] = s.  The walk is exactly T - 1 steps, never loops on data and never leaves
 * [0, 2N].
 * Status.  0 iff path_score > -inf, path_score is not NaN and state[0] <= 1.  1 (not alignable) for N = 0; for T < N + R, R the
 * number of adjacent equal pairs of y; for a bad row -- N > tok_stride, a token outside [0, V) or equal to blank, an em_index outside
 * [0, n_em) --; and for a NaN in the valid frames that leaves the walk short.  None of these values is ever used as an address; a
 * status-1 row gets the fill values.
 * Outputs.  frame_token[t]: j at a frame in state 2j + 1, -1 at a blank frame, -2 for t >= T and in status-1 rows.  Per token j < N:
 * tok_start[j] the first frame in state 2j + 1, tok_end[j] the last such frame plus 1, tok_score[j] the sum of x[t][y_j] over those
 * frames in frame order, fp32, beginning with the first frame's value; -1, -1, -inf for j >= N and in status-1 rows.
 * Frames at or past a length are never read: a NaN there reaches nothing.  Only fp32 adds and compares occur, so the kernel, the
 * package's host path and a scalar restatement agree bit for bit.
 *
 *   logp [n_em, T', V] fp32, from any 4-byte boundary; em_len [n_em] int32, or NULL = T' for all
 *   tokens [n_hyp, tok_stride] int32, tok_len [n_hyp] int32 (N); em_index [n_hyp] int32, or NULL = the row's own index h
 *   tok_start, tok_end int32 and tok_score fp32: [n_hyp, tok_stride];  frame_token [n_hyp, T'] int32;  path_score fp32 and status
 *   int32: [n_hyp]
 *   workspace: eec_ctc_forced_align_workspace_bytes(n_hyp, T', tok_stride) bytes, 256-byte aligned: the decisions, two bits per
 *   (frame, state), n_hyp * ceil(T' * C / 16) * 256 bytes with C = 1, 2, 4, 8 states per lane for tok_stride <= 31, 63, 127, 255.
 *   The size is a multiple of 8, does not decrease in any argument and is 0 when an argument is <= 0.
 * All checks come before any device work, in the codes and order of eec_ctc_align.  EEC_ERR_BAD_ARG: a null required pointer, blank
 * outside [0, V), tok_stride < 1, n_hyp < 0, T' < 1, n_em < 1; n_hyp == 0 is a successful no-op.  EEC_ERR_UNSUPPORTED: tok_stride >
 * 255, V < 2.  EEC_ERR_WORKSPACE: a null, short or misaligned workspace.
 * One launch (one wavefront per hypothesis, four to a workgroup: rows that follow each other and share an emission share its cache
 * lines), no atomics, nothing read back, no allocation, no synchronisation; graph-capturable; two runs and any split of the
 * hypotheses return the same bits. */
size_t eec_ctc_forced_align_workspace_bytes(int n_hyp, int Tq, int tok_stride);
int eec_ctc_forced_align(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                         const int32_t* em_index, int n_hyp, int tok_stride, int blank, int32_t* tok_start, int32_t* tok_end,
                         float* tok_score, int32_t* frame_token, float* path_score, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- CTC posteriors, standard topology (csrc/ctc_posterior.hip) ---------------------------------------------------------------------------
 * "How sure is the model of this token, summed over every way of aligning it, and where does it begin and end in expectation": the
 * forward-backward occupancy of the lattice eec_ctc_forced_align walks -- the same 2N + 1 states, the same inputs, the same row
 * checks -- and the per-token sums read off it.  Sum over paths where eec_ctc_forced_align takes the best path; per state where
 * eec_ctc_hyp_logp keeps only the total.  The reference has nothing like this entry: an addition, not a parity item.
 * tests/posterior_cases.py restates everything below in fp64 and checks it against a brute force over all frame labellings.
 *
 * Inputs, per row h: exactly eec_ctc_forced_align's.  x = logp[em_index[h]] ([T', V] fp32 log-probs), T = clamp(em_len[em_index[h]],
 * 0, T') (em_len NULL: T'), y the N = tok_len[h] labels of tokens[h].  States s = 0 .. 2N: lab(s) = blank for even s, y[(s-1)/2] for
 * odd s; skip(s) holds for odd s >= 3 with y[(s-1)/2] != y[(s-3)/2].  x_t(v) = x[t][v].
 * Recursions, fp32, in log space.  log_add(a, b) is the sequence stated under eec_ctc_log_add; log_add(a, b, c) = log_add(log_add(a,
 * b), c), and a candidate a state does not have (s - 1 of state 0, a skip that does not hold, a state past 2N) is -inf, for which
 * log_add returns its other argument unchanged.  The fold order is stay, step, skip.  -inf is an ordinary value; there is no range
 * limit and no scaling.
 *   alpha_0(0) = x_0(blank), alpha_0(1) = x_0(y_0), every other state -inf;
 *   alpha_t(s) = log_add(alpha_{t-1}(s), alpha_{t-1}(s-1), [skip(s)] alpha_{t-1}(s-2)) + x_t(lab(s))            one add
 *   beta_{T-1}(2N) = beta_{T-1}(2N-1) = 0, every other state -inf;  c_t(s) = x_t(lab(s)) + beta_t(s)             one add
 *   beta_t(s) = log_add(c_{t+1}(s), c_{t+1}(s+1), [skip(s+2)] c_{t+1}(s+2))      (beta_t does not hold frame t's own emission)
 *   ll = log_add(alpha_{T-1}(2N), alpha_{T-1}(2N-1))
 *   gamma_t(s) = exp((alpha_t(s) + beta_t(s)) - ll)
 * and for token j, s = 2j + 1, the posterior of t being its first and its last frame, written without cancellation:
 *   f_t(j) = exp(((log_add(alpha_{t-1}(s-1), [skip(s)] alpha_{t-1}(s-2)) + x_t(y_j)) + beta_t(s)) - ll) for t >= 1;
 *   f_0(0) = gamma_0(1), f_0(j) = 0 for j >= 1
 *   l_t(j) = exp((alpha_t(s) + log_add(c_{t+1}(s+1), [skip(s+2)] c_{t+1}(s+2))) - ll) for t < T - 1;  l_{T-1}(j) = gamma_{T-1}(s)
 * Additions and subtractions are single fp32 operations in the written order; exp is the fp32 library exponential (it is not one of
 * the exactly stated operations: the device's results are its own, reproducible bit for bit on the device, and other
 * implementations of this statement agree with it within the bound below).
 * Per-token sums, each accumulated in fp64 over t = T-1 down to 0 -- the order of the backward sweep, which is where the terms come
 * to exist -- from the fp32 terms above and rounded ONCE to fp32:
 *   tok_frames[j] = sum_t gamma_t(s)                      the expected number of frames the token holds
 *   tok_score[j]  = sum_t gamma_t(s) * x_t(y_j)           (a frame with gamma_t(s) = 0 adds 0, whatever x_t(y_j) is);
 *                                                         exp(tok_score / tok_frames) is the token's confidence
 *   tok_start[j]  = sum_t t f_t(j)                        tok_start_var[j] = sum_t t^2 f_t(j) - (sum_t t f_t(j))^2
 *   tok_end[j]    = sum_t (t + 1) l_t(j)                  tok_end_var[j]   = sum_t (t+1)^2 l_t(j) - (sum_t (t+1) l_t(j))^2
 * with the subtraction and the square in fp64 on the unrounded sums.  A token's frames are contiguous on every path, so in exact
 * arithmetic sum_t f_t(j) = sum_t l_t(j) = 1, tok_end - tok_start = tok_frames and the variances are >= 0; in fp32 these hold within
 * the bound below and a variance near 0 may come out slightly negative.
 * row_logp[h] = ll.  gamma (optional) [n_hyp, T', tok_stride] fp32: gamma[h][t][j] = gamma_t(2j + 1); 0 for j >= N and for t >= T.
 * The blank's share of a frame is one minus the row's sum.
 * Status.  1: the row fails eec_ctc_forced_align's row checks -- N = 0; T < N + R, R the number of adjacent equal pairs of y; N >
 * tok_stride, a token outside [0, V) or equal to blank, an em_index outside [0, n_em) --; none of these values is ever used as an
 * address.  2: the row passes them and ll is not finite (-inf emissions on every path; a NaN that reaches ll.  log_add drops a NaN
 * argument in favour of the other one, so a NaN emission inside the length gives status 0 or 2 and unspecified values, never an
 * address out of range).  0 otherwise.  Status 1 and 2 write the fill values: row_logp = -inf, the six token outputs -1.0 over the
 * whole tok_stride, the row's gamma 0.  A status-0 row has -1.0 in the six token outputs for j >= N.
 * Frames at or past a length are never read: a NaN there reaches nothing.
 * Accuracy.  With bound(T, M) = T * (2^-22 * M + 4e-7) the model every log_add lattice of this library is held to (M the largest
 * finite magnitude of alpha and beta), |row_logp - ll| <= bound, every posterior is within a factor exp(+-3 bound) * (1 +- 2^-22)
 * of its exact value, and so every sum above is within (expm1(3 bound) + 2^-22) times the sum of the absolute values of its terms,
 * plus its one rounding.  tests/test_gpu_posterior.py holds the device to that against the fp64 restatement.
 *
 *   logp [n_em, T', V] fp32, from any 4-byte boundary; em_len [n_em] int32, or NULL = T' for all
 *   tokens [n_hyp, tok_stride] int32, tok_len [n_hyp] int32 (N); em_index [n_hyp] int32, or NULL = the row's own index h
 *   row_logp fp32 and status int32: [n_hyp];  tok_frames, tok_score, tok_start, tok_end, tok_start_var, tok_end_var fp32:
 *   [n_hyp, tok_stride];  gamma fp32 [n_hyp, T', tok_stride], or NULL: not wanted
 *   workspace: eec_ctc_posteriors_workspace_bytes(n_hyp, T', tok_stride) bytes, 256-byte aligned: alpha, one 256-byte line per
 *   (frame, slot of the state strip), n_hyp * T' * C * 256 bytes with C = 1, 2, 4, 8 states per lane for tok_stride <= 31, 63, 127,
 *   255.  The size is a multiple of 8, does not decrease in any argument and is 0 when an argument is <= 0.
 * All checks come before any device work, in the codes and order of eec_ctc_forced_align.  EEC_ERR_BAD_ARG: a null required pointer,
 * blank outside [0, V), tok_stride < 1, n_hyp < 0, T' < 1, n_em < 1; n_hyp == 0 is a successful no-op.  EEC_ERR_UNSUPPORTED:
 * tok_stride > 255, V < 2.  EEC_ERR_WORKSPACE: a null, short or misaligned workspace.  Errors through eec_last_error().
 * One launch (one wavefront per row, four to a workgroup), no atomics, nothing read back, no allocation, no synchronisation;
 * graph-capturable; two runs and any split of the rows return the same bits. */
size_t eec_ctc_posteriors_workspace_bytes(int n_hyp, int Tq, int tok_stride);
int eec_ctc_posteriors(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                       const int32_t* em_index, int n_hyp, int tok_stride, int blank, float* row_logp, float* tok_frames, float* tok_score,
                       float* tok_start, float* tok_end, float* tok_start_var, float* tok_end_var, float* gamma, int32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC segmentation: long rows, free ends (csrc/ctc_segment.hip) -------------------------------------------------------------------------
 * "Where in this recording is this transcript": eec_ctc_forced_align for rows of up to EEC_SEG_MAX_TOKENS = 4095 tokens -- a
 * character-level utterance, or the concatenated transcript of a talk aligned against the whole recording as in CTC segmentation
 * (Kuerzinger et al. 2020) -- with two flags that make the audio before the first and after the last token cost nothing.  The
 * reference has nothing like this entry: an addition, not a parity item.  tests/segment_cases.py restates it in scalar fp32 and
 * checks it against a brute force over all frame labellings.
 *
 * Arguments: eec_ctc_forced_align's, in its order, with `flags` after `blank`; the outputs are the same.
 * Semantics: eec_ctc_forced_align's statement word for word -- states, candidates, their order stay / step / skip, the strict > tie
 * rule, the end rule, the walk back, the row checks, status 0 / 1, the fill values, "frames at or past a length are never read" --
 * with one term changed per flag:
 *   EEC_SEG_FREE_START (bit 0): the emission term of state 0 is 0.0f at every frame: a[0][0] = 0, and a[t][0] = best + 0.0f.
 *   EEC_SEG_FREE_END   (bit 1): the emission term of state 2N is 0.0f at every frame t >= 1.
 * Any other bit set is EEC_ERR_BAD_ARG.  Everything else is unchanged, tok_score included, which sums label frames only.  With
 * flags = 0 the statement IS eec_ctc_forced_align's.  Adding 0.0f is exact in fp32, so the kernel, the package's host path and a
 * scalar restatement still agree bit for bit.
 * Accumulation.  A path score is a plain fp32 sum over as many frames as the emission has, tens of thousands for a recording.  The
 * statement stays exact -- every implementation performs the same adds -- but the precision of the SCORE shrinks with its magnitude:
 * at |score| around 2^16 one add rounds to 2^-8.  Nothing is rescaled; a decision between two candidates closer than that rounding
 * goes by the tie rule.
 * Limits.  tok_stride <= EEC_SEG_MAX_TOKENS (the 2N + 1 <= 8191 states lie on up to 16 wavefronts of one workgroup, 512 states
 * each), V >= 2.  A row with tok_len > tok_stride has status 1 like every bad row.
 *
 *   workspace: eec_ctc_segment_workspace_bytes(n_hyp, T', tok_stride) bytes, 256-byte aligned: the decisions, two bits per (frame,
 *   state): n_hyp * ceil(T' / 2) * W * 256 bytes with W = ceil((2 * tok_stride + 1) / 512) wavefronts per row.  The size does not
 *   decrease in any argument and is 0 when an argument is <= 0.
 * All checks come before any device work, through eec_last_error().  EEC_ERR_BAD_ARG: a flags bit other than the two; then, in the
 * codes and order of eec_ctc_forced_align, a null required pointer, blank outside [0, V), tok_stride < 1, n_hyp < 0, T' < 1, n_em <
 * 1; n_hyp == 0 is a successful no-op.  EEC_ERR_UNSUPPORTED: tok_stride > 4095 (the message names the limit), V < 2.
 * EEC_ERR_WORKSPACE: a null, short or misaligned workspace.
 * One launch, one workgroup per row -- the best path is sequential in time, so a recording is one workgroup however long it is --,
 * no atomics, nothing read back, no allocation, no synchronisation; graph-capturable; two runs and any split of the rows return the
 * same bits.  Rows of at most 255 tokens are served faster by eec_ctc_forced_align, which needs no barrier. */
#define EEC_SEG_MAX_TOKENS 4095
#define EEC_SEG_FREE_START 1
#define EEC_SEG_FREE_END 2
size_t eec_ctc_segment_workspace_bytes(int n_hyp, int Tq, int tok_stride);
int eec_ctc_segment(const float* logp, int n_em, int Tq, int V, const int32_t* em_len, const int32_t* tokens, const int32_t* tok_len,
                    const int32_t* em_index, int n_hyp, int tok_stride, int blank, int flags, int32_t* tok_start, int32_t* tok_end,
                    float* tok_score, int32_t* frame_token, float* path_score, int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EEC_H_ */
