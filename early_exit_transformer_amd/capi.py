"""ctypes binding of libeec.so (include/eec.h).  There is no CPU fallback: if the
library is missing, loading raises and every product entry point fails loudly."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from .build import LIB_PATH

PREC_F16X3, PREC_MIXED, PREC_F16, PREC_F16F8 = 0, 1, 2, 3
ARCH_CONFORMER, ARCH_LEGACY = 0, 1
PRECISIONS = {"f16x3": PREC_F16X3, "mixed": PREC_MIXED, "f16": PREC_F16, "f16f8": PREC_F16F8}

_LAYER_FIELDS = [
    "ffn1_ln_w", "ffn1_ln_b", "ffn1_w1", "ffn1_b1", "ffn1_w2", "ffn1_b2",
    "attn_ln_w", "attn_ln_b", "attn_in_w", "attn_in_b", "attn_out_w", "attn_out_b",
    "conv_ln_w", "conv_ln_b", "conv_pw1_w", "conv_pw1_b", "conv_dw_w", "conv_dw_b",
    "conv_bn_w", "conv_bn_b", "conv_bn_rm", "conv_bn_rv", "conv_pw2_w", "conv_pw2_b",
    "ffn2_ln_w", "ffn2_ln_b", "ffn2_w1", "ffn2_b1", "ffn2_w2", "ffn2_b2",
    "final_ln_w", "final_ln_b",
]

# state_dict key suffix (inside conformer.{e}.conformer_layers.{l}.) of every eec_layer_params field
LAYER_KEYS = {
    "ffn1_ln_w": "ffn1.sequential.0.weight", "ffn1_ln_b": "ffn1.sequential.0.bias",
    "ffn1_w1": "ffn1.sequential.1.weight", "ffn1_b1": "ffn1.sequential.1.bias",
    "ffn1_w2": "ffn1.sequential.4.weight", "ffn1_b2": "ffn1.sequential.4.bias",
    "attn_ln_w": "self_attn_layer_norm.weight", "attn_ln_b": "self_attn_layer_norm.bias",
    "attn_in_w": "self_attn.in_proj_weight", "attn_in_b": "self_attn.in_proj_bias",
    "attn_out_w": "self_attn.out_proj.weight", "attn_out_b": "self_attn.out_proj.bias",
    "conv_ln_w": "conv_module.layer_norm.weight", "conv_ln_b": "conv_module.layer_norm.bias",
    "conv_pw1_w": "conv_module.sequential.0.weight", "conv_pw1_b": "conv_module.sequential.0.bias",
    "conv_dw_w": "conv_module.sequential.2.weight", "conv_dw_b": "conv_module.sequential.2.bias",
    "conv_bn_w": "conv_module.sequential.3.weight", "conv_bn_b": "conv_module.sequential.3.bias",
    "conv_bn_rm": "conv_module.sequential.3.running_mean", "conv_bn_rv": "conv_module.sequential.3.running_var",
    "conv_pw2_w": "conv_module.sequential.5.weight", "conv_pw2_b": "conv_module.sequential.5.bias",
    "ffn2_ln_w": "ffn2.sequential.0.weight", "ffn2_ln_b": "ffn2.sequential.0.bias",
    "ffn2_w1": "ffn2.sequential.1.weight", "ffn2_b1": "ffn2.sequential.1.bias",
    "ffn2_w2": "ffn2.sequential.4.weight", "ffn2_b2": "ffn2.sequential.4.bias",
    "final_ln_w": "final_layer_norm.weight", "final_ln_b": "final_layer_norm.bias",
}


class EecConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "n_heads", "d_ff", "dw_kernel", "n_exits",
                                         "layers_per_exit", "n_mels", "vocab", "max_len", "arch")]


class EecLayerParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _LAYER_FIELDS]


class EecParams(C.Structure):
    _fields_ = [("sub0_w", C.c_void_p), ("sub0_b", C.c_void_p), ("sub1_w", C.c_void_p), ("sub1_b", C.c_void_p),
                ("pe", C.c_void_p), ("layers", C.POINTER(EecLayerParams)),
                ("head_w", C.POINTER(C.c_void_p)), ("head_b", C.POINTER(C.c_void_p))]


class EecDecoderLayerParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ca_in_w", "ca_in_b", "ca_out_w", "ca_out_b",
                                          "w1", "b1", "w2", "b2", "norm1_w", "norm1_b", "norm2_w", "norm2_b", "norm3_w", "norm3_b")]


# field -> state_dict key suffix below ``decoders.{e}.layers.{l}.``
DECODER_LAYER_KEYS = {"sa_in_w": "self_attn.in_proj_weight", "sa_in_b": "self_attn.in_proj_bias",
                      "sa_out_w": "self_attn.out_proj.weight", "sa_out_b": "self_attn.out_proj.bias",
                      "ca_in_w": "multihead_attn.in_proj_weight", "ca_in_b": "multihead_attn.in_proj_bias",
                      "ca_out_w": "multihead_attn.out_proj.weight", "ca_out_b": "multihead_attn.out_proj.bias",
                      "w1": "linear1.weight", "b1": "linear1.bias", "w2": "linear2.weight", "b2": "linear2.bias",
                      "norm1_w": "norm1.weight", "norm1_b": "norm1.bias", "norm2_w": "norm2.weight", "norm2_b": "norm2.bias",
                      "norm3_w": "norm3.weight", "norm3_b": "norm3.bias"}


class EecDecoderParams(C.Structure):
    _fields_ = [("emb", C.c_void_p), ("pe", C.c_void_p), ("layers", C.POINTER(EecDecoderLayerParams)), ("n_layers", C.c_int32),
                ("max_len", C.c_int32), ("norm_w", C.c_void_p), ("norm_b", C.c_void_p), ("head_w", C.c_void_p), ("head_b", C.c_void_p)]


# host callback of eec_train_backward_ex: (exit group just finished, or -1 after the stem; user pointer)
GROUP_DONE_FN = C.CFUNCTYPE(None, C.c_int, C.c_void_p)

EXPORTS = ["eec_last_error", "eec_abi_version", "eec_out_frames", "eec_encoder_create", "eec_encoder_destroy",
           "eec_encoder_pack", "eec_encoder_workspace_bytes", "eec_encoder_forward", "eec_greedy_ctc",
           "eec_encoder_set_profiling", "eec_encoder_profile_read", "eec_ctc_loss", "eec_encoder_pack_legacy",
           "eec_encoder_forward_prefix", "eec_encoder_group_workspace_bytes", "eec_encoder_group_forward",
           "eec_encoder_head_forward", "eec_encoder_stem1_forward", "eec_encoder_lengths",
           "eec_ctc_backward_workspace_bytes", "eec_ctc_loss_forward", "eec_ctc_loss_backward", "eec_logsoftmax_backward",
           "eec_exit_distill_workspace_bytes", "eec_exit_distill_forward", "eec_exit_distill_backward",
           "eec_ctc_mwer_workspace_bytes", "eec_ctc_hyp_logp", "eec_ctc_mwer_forward", "eec_ctc_mwer_backward",
           "eec_exit_stats_workspace_bytes", "eec_exit_stats", "eec_exit_route",
           "eec_ctc_beam_workspace_bytes", "eec_ctc_beam_decode", "eec_ctc_beam_decode_ex",
           "eec_ctc_loss_len", "eec_ctc_loss_forward_len", "eec_ctc_loss_backward_len", "eec_greedy_ctc_len", "eec_ctc_beam_decode_len",
           "eec_ctc_beam_decode_nbest",
           "eec_ctc_align_workspace_bytes", "eec_ctc_align",
           "eec_ctc_trie_pack_bytes", "eec_ctc_trie_pack", "eec_ctc_lexbeam_workspace_bytes", "eec_ctc_lexbeam_decode",
           "eec_ngram_pack_bytes", "eec_ngram_pack", "eec_ctc_lexbeam_lm_decode",
           "eec_ctc_trie_smear_bytes", "eec_ctc_trie_smear", "eec_ctc_lexbeam_lm_smear_decode",
           "eec_ctc_lexbeam_logadd_decode", "eec_ctc_log_add_host", "eec_ctc_log_add",
           "eec_ctc_lexbeam_wide_workspace_bytes", "eec_ctc_lexbeam_wide_decode",
           "eec_lexicon_pack_bytes", "eec_lexicon_pack", "eec_lexicon_nearest_workspace_bytes", "eec_lexicon_nearest",
           "eec_edit_distance_workspace_bytes", "eec_edit_distance",
           "eec_specaug_draw", "eec_specaug_apply",
           "eec_resample_plan_bytes", "eec_resample_plan", "eec_speed_draw", "eec_resample_lengths", "eec_resample",
           "eec_rir_bank_bytes", "eec_rir_bank", "eec_noise_bank_bytes", "eec_noise_bank", "eec_waveaug_partials_bytes", "eec_waveaug_draw",
           "eec_reverb", "eec_noise_energy", "eec_noise_mix",
           "eec_rir_spectra_bytes", "eec_rir_spectra", "eec_reverb_fft_workspace_bytes", "eec_reverb_fft", "eec_reverb_fft_stage",
           "eec_frontend_last_error", "eec_frontend_create", "eec_frontend_destroy", "eec_frontend_frames", "eec_frontend_forward",
           "eec_trainer_last_error", "eec_trainer_create", "eec_trainer_destroy", "eec_trainer_workspace_bytes",
           "eec_train_forward", "eec_train_backward", "eec_train_backward_ex", "eec_train_gemm",
           "eec_train_group_workspace_bytes", "eec_train_group_forward", "eec_train_group_backward", "eec_train_stem_workspace_bytes",
           "eec_train_stem_forward", "eec_train_stem_backward", "eec_train_head_forward", "eec_train_head_backward_scratch_floats",
           "eec_train_head_backward",
           "eec_decoder_last_error", "eec_decoder_workspace_bytes", "eec_decoder_forward",
           "eec_decoder_score_workspace_bytes", "eec_decoder_score", "eec_hypothesis_score",
           "eec_decoder_train_last_error", "eec_decoder_train_workspace_bytes", "eec_decoder_train_forward", "eec_decoder_train_backward",
           "eec_decoder_step_last_error", "eec_decoder_step_max_beams", "eec_decoder_cache_bytes", "eec_decoder_begin", "eec_decoder_step", "eec_decoder_step_multi", "eec_upload_i64_max", "eec_upload_i64", "eec_beam_select",
           "eec_decoder_batch_cache_bytes", "eec_decoder_batch_begin", "eec_decoder_batch_step",
           "eec_ctc_prefix_state_bytes", "eec_ctc_prefix_begin", "eec_ctc_prefix_step",
           "eec_context_graph_bytes", "eec_context_graph", "eec_ctc_beam_decode_ctx", "eec_ctc_beam_decode_nbest_ctx",
           "eec_context_bias_state_bytes", "eec_context_bias_step"]
KERNEL_CLASSES = ["stem", "ffn", "qkv", "attn", "proj_glu", "proj", "dw_pw2", "head", "chain"]

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen libeec.so and declare the prototypes; raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP library is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or early_exit_transformer_amd.build.build_library()). There is no CPU fallback.")
    # torch is imported first (top of this module): its bundled libamdhip64.so carries the soname libeec.so asks for
    # (libamdhip64.so.7), so the loader reuses it.  Loaded the other way round, /opt/rocm's copy comes in as well and one
    # process holds two HIP runtimes (the second to initialise then reports "no ROCm-capable device").
    lib = C.CDLL(LIB_PATH)
    lib.eec_last_error.restype = C.c_char_p
    lib.eec_abi_version.restype = C.c_int
    lib.eec_out_frames.argtypes = [C.c_int]
    lib.eec_encoder_create.argtypes = [C.POINTER(EecConfig), C.POINTER(C.c_void_p)]
    lib.eec_encoder_destroy.argtypes = [C.c_void_p]
    lib.eec_encoder_destroy.restype = None
    lib.eec_encoder_pack.argtypes = [C.c_void_p, C.POINTER(EecParams), C.c_void_p]
    lib.eec_encoder_pack_legacy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_encoder_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.eec_encoder_workspace_bytes.restype = C.c_size_t
    lib.eec_encoder_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_encoder_forward_prefix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_encoder_group_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.eec_encoder_group_workspace_bytes.restype = C.c_size_t
    lib.eec_encoder_group_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_encoder_head_forward.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.eec_encoder_stem1_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_encoder_lengths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_greedy_ctc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p]
    lib.eec_ctc_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_ctc_backward_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.eec_ctc_backward_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_loss_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_ctc_loss_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # the _len entries: the lengths pointer follows the arguments it qualifies (NULL = T' everywhere = the entry without lengths)
    lib.eec_ctc_loss_len.argtypes = lib.eec_ctc_loss.argtypes[:3] + [C.c_void_p] + lib.eec_ctc_loss.argtypes[3:]
    lib.eec_ctc_loss_forward_len.argtypes = lib.eec_ctc_loss_forward.argtypes[:3] + [C.c_void_p] + lib.eec_ctc_loss_forward.argtypes[3:]
    lib.eec_ctc_loss_backward_len.argtypes = lib.eec_ctc_loss_backward.argtypes[:3] + [C.c_void_p] + lib.eec_ctc_loss_backward.argtypes[3:]
    lib.eec_greedy_ctc_len.argtypes = lib.eec_greedy_ctc.argtypes[:1] + [C.c_void_p] + lib.eec_greedy_ctc.argtypes[1:]
    lib.eec_logsoftmax_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_exit_distill_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_exit_distill_workspace_bytes.restype = C.c_size_t
    lib.eec_exit_distill_forward.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_exit_distill_backward.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_ctc_mwer_workspace_bytes.argtypes = [C.c_int] * 5
    lib.eec_ctc_mwer_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_hyp_logp.argtypes = [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]
    # logp, input_len, hyp, hyp_len, risk; E, B, b0, nb, T', V, N, L, blank; ll, loss_eb, loss, workspace, its bytes, stream
    lib.eec_ctc_mwer_forward.argtypes = [C.c_void_p] * 5 + [C.c_int] * 9 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
    # logp, input_len, hyp, hyp_len; E, B, b0, nb, T', V, N, L, blank; workspace, its bytes, grad_loss, accumulate, dlogp, stream
    lib.eec_ctc_mwer_backward.argtypes = [C.c_void_p] * 4 + [C.c_int] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_exit_stats_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_exit_stats_workspace_bytes.restype = C.c_size_t
    lib.eec_exit_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_exit_route.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_ctc_beam_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.eec_ctc_beam_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_beam_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_ctc_beam_decode_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_ctc_beam_decode_len.argtypes = lib.eec_ctc_beam_decode_ex.argtypes[:1] + [C.c_void_p] + lib.eec_ctc_beam_decode_ex.argtypes[1:]
    # N-best: nbest follows skip_drops_frame, n_hyp follows scores
    lib.eec_ctc_beam_decode_nbest.argtypes = lib.eec_ctc_beam_decode_len.argtypes[:9] + [C.c_int] + lib.eec_ctc_beam_decode_len.argtypes[9:13] + \
        [C.c_void_p, C.c_void_p]
    lib.eec_ctc_align_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_ctc_align_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_align.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_ctc_trie_pack_bytes.argtypes = [C.c_int, C.c_int64]
    lib.eec_ctc_trie_pack_bytes.restype = C.c_size_t
    lib.eec_ctc_trie_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.eec_ctc_lexbeam_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_ctc_lexbeam_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_lexbeam_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_float, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 8 + [C.c_size_t, C.c_void_p]
    lib.eec_ctc_lexbeam_lm_decode.argtypes = lib.eec_ctc_lexbeam_decode.argtypes + [C.c_void_p, C.c_float]
    lib.eec_ctc_lexbeam_lm_smear_decode.argtypes = lib.eec_ctc_lexbeam_lm_decode.argtypes + [C.c_void_p]
    lib.eec_ctc_lexbeam_logadd_decode.argtypes = lib.eec_ctc_lexbeam_lm_smear_decode.argtypes
    lib.eec_ctc_lexbeam_wide_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_ctc_lexbeam_wide_workspace_bytes.restype = C.c_size_t
    lib.eec_ctc_lexbeam_wide_decode.argtypes = lib.eec_ctc_lexbeam_lm_smear_decode.argtypes + [C.c_int]
    lib.eec_ctc_log_add_host.argtypes = [C.c_float, C.c_float]
    lib.eec_ctc_log_add_host.restype = C.c_float
    lib.eec_ctc_log_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.eec_ctc_trie_smear_bytes.argtypes = [C.c_int]
    lib.eec_ctc_trie_smear_bytes.restype = C.c_size_t
    lib.eec_ctc_trie_smear.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.eec_ngram_pack_bytes.argtypes = [C.c_int, C.c_void_p, C.c_int]
    lib.eec_ngram_pack_bytes.restype = C.c_size_t
    lib.eec_ngram_pack.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_size_t, C.c_void_p]
    lib.eec_lexicon_pack_bytes.argtypes = [C.c_int, C.c_int64, C.c_int]
    lib.eec_lexicon_pack_bytes.restype = C.c_size_t
    lib.eec_lexicon_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.eec_lexicon_nearest_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.eec_lexicon_nearest_workspace_bytes.restype = C.c_size_t
    lib.eec_lexicon_nearest.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    lib.eec_edit_distance_workspace_bytes.argtypes = [C.c_int] * 4
    lib.eec_edit_distance_workspace_bytes.restype = C.c_size_t
    lib.eec_edit_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    # frame_len; B, n_mels, T; seed, utt_offset; W, n_freq_masks, F, n_time_masks, ratio, Tmax; params, stream
    lib.eec_specaug_draw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                     C.c_int, C.c_void_p, C.c_void_p]
    # mel, frame_len, params; B, n_mels, T, n_freq_masks, n_time_masks, mode; mask_value; out, stream
    lib.eec_specaug_apply.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float, C.c_void_p, C.c_void_p]
    # R, orig, new, lowpass_filter_width, rolloff (; image, its bytes)
    lib.eec_resample_plan_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    lib.eec_resample_plan_bytes.restype = C.c_size_t
    lib.eec_resample_plan.argtypes = lib.eec_resample_plan_bytes.argtypes + [C.c_void_p, C.c_size_t]
    # lengths; B, L; seed, utt_offset; plan, choice, out_len, stream
    lib.eec_speed_draw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # lengths, choice; B, L; plan, out_len, stream
    lib.eec_resample_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    # wave, lengths, choice; B, L; plan, out; L_out; out_len, stream
    lib.eec_resample.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    # R, taps, n_taps, normalize, shift (; image, its bytes);  M, samples, n_samples (; image, its bytes)
    lib.eec_rir_bank_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.eec_rir_bank_bytes.restype = C.c_size_t
    lib.eec_rir_bank.argtypes = lib.eec_rir_bank_bytes.argtypes + [C.c_void_p, C.c_size_t]
    lib.eec_noise_bank_bytes.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_noise_bank_bytes.restype = C.c_size_t
    lib.eec_noise_bank.argtypes = lib.eec_noise_bank_bytes.argtypes + [C.c_void_p, C.c_size_t]
    lib.eec_waveaug_partials_bytes.argtypes = [C.c_int, C.c_int]
    lib.eec_waveaug_partials_bytes.restype = C.c_size_t
    # B; seed, utt_offset; rir_bank, thr_reverb; noise_bank, thr_noise; n_snrs, volume, lo, hi; params, stream
    lib.eec_waveaug_draw.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_double,
                                     C.c_double, C.c_void_p, C.c_void_p]
    # wave, lengths, params; B, L; rir_bank, out, partials, stream
    lib.eec_reverb.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.eec_rir_spectra_bytes.argtypes = [C.c_void_p]
    lib.eec_rir_spectra_bytes.restype = C.c_size_t
    lib.eec_rir_spectra.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.eec_reverb_fft_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.eec_reverb_fft_workspace_bytes.restype = C.c_size_t
    # wave, lengths, params; B, L; rir_bank, rir_spectra, out, partials, workspace; workspace_bytes; stream
    lib.eec_reverb_fft.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
    lib.eec_reverb_fft_stage.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_size_t, C.c_int, C.c_void_p]
    # signal, lengths, params; B, L; noise_bank, partials, stream
    lib.eec_noise_energy.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    # y, lengths, params; B, L; noise_bank, snr_gain; n_snrs; partials, out, applied, stream
    lib.eec_noise_mix.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    lib.eec_frontend_last_error.restype = C.c_char_p
    lib.eec_frontend_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.eec_frontend_destroy.argtypes = [C.c_void_p]
    lib.eec_frontend_destroy.restype = None
    lib.eec_frontend_frames.argtypes = [C.c_int, C.c_int]
    lib.eec_frontend_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_trainer_last_error.restype = C.c_char_p
    lib.eec_trainer_create.argtypes = [C.POINTER(EecConfig), C.POINTER(C.c_void_p)]
    lib.eec_trainer_destroy.argtypes = [C.c_void_p]
    lib.eec_trainer_destroy.restype = None
    lib.eec_trainer_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.eec_trainer_workspace_bytes.restype = C.c_size_t
    lib.eec_train_forward.argtypes = [C.c_void_p, C.POINTER(EecParams), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_train_backward.argtypes = [C.c_void_p, C.POINTER(EecParams), C.POINTER(EecParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_train_backward_ex.argtypes = [C.c_void_p, C.POINTER(EecParams), C.POINTER(EecParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p, GROUP_DONE_FN, C.c_void_p]
    lib.eec_train_group_workspace_bytes.argtypes = [C.POINTER(EecConfig), C.c_int, C.c_int, C.c_int]
    lib.eec_train_group_workspace_bytes.restype = C.c_size_t
    lib.eec_train_group_forward.argtypes = [C.POINTER(EecConfig), C.POINTER(EecLayerParams), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                            C.c_int, C.c_float, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_train_group_backward.argtypes = [C.POINTER(EecConfig), C.POINTER(EecLayerParams), C.POINTER(EecLayerParams), C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_train_stem_workspace_bytes.argtypes = [C.POINTER(EecConfig), C.c_int, C.c_int, C.c_int]
    lib.eec_train_stem_workspace_bytes.restype = C.c_size_t
    lib.eec_train_stem_forward.argtypes = [C.POINTER(EecConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_train_stem_backward.argtypes = [C.POINTER(EecConfig), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_train_head_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_train_head_backward_scratch_floats.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_train_head_backward_scratch_floats.restype = C.c_size_t
    lib.eec_train_head_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.eec_train_gemm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p]
    lib.eec_decoder_last_error.restype = C.c_char_p
    lib.eec_decoder_workspace_bytes.argtypes = [C.c_int] * 7
    lib.eec_decoder_workspace_bytes.restype = C.c_size_t
    lib.eec_decoder_forward.argtypes = [C.POINTER(EecDecoderParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_decoder_score_workspace_bytes.argtypes = [C.c_int] * 8
    lib.eec_decoder_score_workspace_bytes.restype = C.c_size_t
    lib.eec_decoder_score.argtypes = [C.POINTER(EecDecoderParams)] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_hypothesis_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_decoder_train_last_error.restype = C.c_char_p
    lib.eec_decoder_train_workspace_bytes.argtypes = [C.c_int] * 8
    lib.eec_decoder_train_workspace_bytes.restype = C.c_size_t
    lib.eec_decoder_train_forward.argtypes = [C.POINTER(EecDecoderParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]
    lib.eec_decoder_train_backward.argtypes = [C.POINTER(EecDecoderParams), C.POINTER(EecDecoderParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_decoder_step_last_error.restype = C.c_char_p
    lib.eec_decoder_cache_bytes.argtypes = [C.c_int] * 7
    lib.eec_decoder_cache_bytes.restype = C.c_size_t
    lib.eec_decoder_begin.argtypes = [C.POINTER(EecDecoderParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_decoder_step.argtypes = [C.POINTER(EecDecoderParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_decoder_step_multi.argtypes = [C.c_int, C.POINTER(C.POINTER(EecDecoderParams)), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p]
    lib.eec_decoder_batch_cache_bytes.argtypes = [C.c_int] * 9
    lib.eec_decoder_batch_cache_bytes.restype = C.c_size_t
    lib.eec_decoder_batch_begin.argtypes = [C.POINTER(C.POINTER(EecDecoderParams)), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_decoder_batch_step.argtypes = [C.POINTER(C.POINTER(EecDecoderParams)), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]
    lib.eec_beam_select.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.eec_upload_i64.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.eec_ctc_prefix_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.eec_ctc_prefix_state_bytes.restype = C.c_size_t
    lib.eec_ctc_prefix_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.eec_ctc_prefix_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p]
    # G, n_phrases, phrase_len, tokens, boost; V, blank, eos, pad (; image, its bytes)
    lib.eec_context_graph_bytes.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 4
    lib.eec_context_graph_bytes.restype = C.c_size_t
    lib.eec_context_graph.argtypes = lib.eec_context_graph_bytes.argtypes + [C.c_void_p, C.c_size_t]
    # the _len / _nbest entries, then image, its bytes, graph_of, bias in front of the stream
    ctx = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.eec_ctc_beam_decode_ctx.argtypes = lib.eec_ctc_beam_decode_len.argtypes[:-1] + ctx + [C.c_void_p]
    lib.eec_ctc_beam_decode_nbest_ctx.argtypes = lib.eec_ctc_beam_decode_nbest.argtypes[:-1] + ctx + [C.c_void_p]
    lib.eec_context_bias_state_bytes.argtypes = [C.c_int, C.c_int]
    lib.eec_context_bias_state_bytes.restype = C.c_size_t
    # image, its bytes, graph_of; n, R, R_prev, R_max, V, s; parent, last, local, out, state, its bytes, stream
    lib.eec_context_bias_step.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
    lib.eec_encoder_set_profiling.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.eec_encoder_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    """Raise on a non-zero return code with the library's message (one per thread, whichever family the entry belongs to)."""
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {load().eec_last_error().decode(errors='replace')}")


def stream_ptr(dev) -> C.c_void_p:
    """The current HIP stream of ``dev``, as the C entries take it."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def aligned_ws(nbytes: int, dev):
    """A device workspace of ``nbytes`` usable bytes from a 256-byte boundary on: (tensor that owns it, aligned address)."""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def require_fp32(name: str, t, dev):
    """``t``, which a kernel is about to read through its raw pointer."""
    if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous fp32 tensor on {dev}")
    return t


def new_seed() -> int:
    """A dropout seed from torch's CPU generator (so ``torch.manual_seed`` fixes the masks)."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def to_device(t, dev: torch.device, dtype: torch.dtype = torch.int64):
    """``t.to(dev, dtype).contiguous()``; a small CPU int64 tensor (the collate's ``lengths`` are CPU tensors in the
    reference, train.py:34,54) travels in a kernel's argument block instead (eec_upload_i64): a host-to-device copy in front
    of the forward drains the host's launch queue and leaves a hole on the stream once per step."""
    if t.is_cuda or dev.type != "cuda" or dtype != torch.int64 or t.numel() == 0:
        return t.to(device=dev, dtype=dtype).contiguous()
    lib = load()
    if t.numel() > lib.eec_upload_i64_max():
        return t.to(device=dev, dtype=dtype).contiguous()
    dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
    host = t.to(torch.int64).contiguous()
    out = torch.empty(host.shape, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.eec_upload_i64(host.data_ptr(), host.numel(), out.data_ptr(), stream_ptr(dev)), "eec_upload_i64")
    return out


def layer_params(ptr, prefix: str, n_groups: int, n_layers: int):
    """HOST array of EecLayerParams for ``{prefix}.{g}.conformer_layers.{l}.*`` (group-major)."""
    layers = (EecLayerParams * (n_groups * n_layers))()
    for g in range(n_groups):
        for l in range(n_layers):
            lp = layers[g * n_layers + l]
            for field, suffix in LAYER_KEYS.items():
                setattr(lp, field, ptr(f"{prefix}.{g}.conformer_layers.{l}.{suffix}"))
    return layers


def params_struct(ptr, n_groups: int, n_layers: int, layers: str, stem=(None, None), head: Optional[str] = None,
                  pe: Optional[str] = None):
    """The one map from state_dict names to EecParams.  ``ptr(name)`` gives a tensor's address (or None: a null field);
    ``layers`` is the prefix of the Conformer groups, ``stem`` the key prefixes of the one or two stem convolutions, ``head``
    the key prefix of exit ``{e}``'s Linear, ``pe`` the key of the sinusoid table -- None for what is not packed.  Returns
    (struct, the host arrays it points into: keep them alive as long as the struct)."""
    at = lambda key: ptr(key) if key else None  # noqa: E731
    lay = layer_params(ptr, layers, n_groups, n_layers)
    hw = (C.c_void_p * n_groups)(*[ptr(head.format(e=e) + ".weight") for e in range(n_groups)]) if head else None
    hb = (C.c_void_p * n_groups)(*[ptr(head.format(e=e) + ".bias") for e in range(n_groups)]) if head else None
    st = EecParams(at(stem[0] and stem[0] + ".weight"), at(stem[0] and stem[0] + ".bias"),
                   at(stem[1] and stem[1] + ".weight"), at(stem[1] and stem[1] + ".bias"), at(pe), lay, hw, hb)
    return st, (lay, hw, hb)


class EncoderHandle:
    """Owner of one libeec encoder handle: its device, the key of what is packed into it, and the bounded caches of the
    workspaces its entry points take.  One handle lives on one device (include/eec.h); the owner destroys it when the
    model moved to another one, and when the owner goes."""

    def __init__(self, cfg: EecConfig):
        self.cfg, self.h, self.device, self.key = cfg, None, None, None
        self._ws = {"": {}, "group_": {}}  # eec_encoder_workspace_bytes / eec_encoder_group_workspace_bytes

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def destroy(self) -> None:
        if self.h is not None:
            load().eec_encoder_destroy(self.h)
            self.h = self.key = None
            for cache in self._ws.values():
                cache.clear()

    def ensure(self, device, tensors, pack):
        """The handle on ``device`` with ``tensors`` packed: ``pack(handle)`` runs when a tensor of the list was written,
        moved or replaced since the last packing (``_version``, ``data_ptr``) and on a fresh handle."""
        key = (device, tuple(t._version for t in tensors), tuple(t.data_ptr() for t in tensors))
        if self.h is None or key != self.key:
            if self.h is not None and self.device != device:
                self.destroy()  # model.to(another device): the packed-weight arena lives on the old one
            if self.h is None:
                h = C.c_void_p()
                check(load().eec_encoder_create(C.byref(self.cfg), C.byref(h)), "eec_encoder_create")
                self.h, self.device = h, device
            pack(self.h)
            self.key = key
        return self.h

    def workspace(self, kind: str, B: int, T: int, device):
        """(tensor, aligned address, bytes from there on) for ``eec_encoder_{kind}workspace_bytes(handle, B, T)``: at most
        five geometries are kept."""
        cache = self._ws[kind]
        k = (B, T, device.index or 0)
        ent = cache.get(k)
        if ent is None:
            if len(cache) > 4:
                cache.clear()
            ws, ptr = aligned_ws(getattr(load(), f"eec_encoder_{kind}workspace_bytes")(self.h, B, T), device)
            ent = cache[k] = (ws, ptr, ws.numel() - (ptr - ws.data_ptr()))
        return ent
