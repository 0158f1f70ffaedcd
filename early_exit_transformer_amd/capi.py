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

_as_address = C.c_void_p.from_param  # None -> NULL; an int, a c_void_p, a ctypes array / pointer / byref: taken as they are


class TensorPtr:
    """A pointer parameter of include/eec.h as an ``argtypes`` entry: ctypes hands every argument to ``from_param``.  A tensor
    becomes its address after its element type (``dtypes``; None: any), its layout (contiguous) and where it lives (``host``: the
    entry dereferences the pointer on the host; else on the device) were checked; anything else is an address already.  A refused
    tensor surfaces as ``ctypes.ArgumentError`` naming the argument's position, before the entry is called."""
    elem, dtypes, host = "void", None, False

    @classmethod
    def from_param(cls, v):
        if not isinstance(v, torch.Tensor):
            return _as_address(v)
        if cls.dtypes is not None and v.dtype not in cls.dtypes:
            raise TypeError(f"expected a {cls.elem} tensor, got {v.dtype}")
        if not v.is_contiguous():
            raise TypeError(f"expected a contiguous tensor, got strides {tuple(v.stride())} for shape {tuple(v.shape)}")
        if v.is_cuda == cls.host:
            raise TypeError(f"expected a {'host (CPU)' if cls.host else 'device'} tensor, got one on {v.device}")
        return _as_address(v.data_ptr())


def _ptr_types(elem: str, *dtypes):
    """(device, host) pointer types of element type ``elem``."""
    return tuple(type(("Host" if host else "Device") + "Ptr_" + elem, (TensorPtr,),
                      {"elem": elem, "dtypes": dtypes or None, "host": host}) for host in (False, True))


class STREAM:
    """The hipStream_t parameter of an entry: ``call`` puts the device's current stream where the table has this marker."""
    from_param = _as_address


F32, hF32 = _ptr_types("float", torch.float32)
F64, hF64 = _ptr_types("double", torch.float64)
I32, hI32 = _ptr_types("int32_t", torch.int32)
I64, hI64 = _ptr_types("int64_t", torch.int64)
U8, hU8 = _ptr_types("uint8_t", torch.uint8)
W32, hW32 = _ptr_types("uint32_t", torch.int32, torch.uint32)  # 32-bit words
VOID, hVOID = _ptr_types("void")
i, f, d, z, i64, u32, u64, H = C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_int64, C.c_uint32, C.c_uint64, C.c_void_p  # H: handle
CFG, PRM, LAY, DEC = C.POINTER(EecConfig), C.POINTER(EecParams), C.POINTER(EecLayerParams), C.POINTER(EecDecoderParams)
DECS = C.POINTER(DEC)  # HOST array of decoder parameter structs, one per session / exit

# eec_ctc_lexbeam_decode; its _lm / _lm_smear / _logadd / _wide variants append to it (the stream stays where it is)
_LEXBEAM = [F32, i, i, i, I32, VOID, i, i, i, i, f, f, f, i, I32, I32, I32, I32, I32, F32, I32, VOID, z, STREAM]

# Every export of libeec.so, parameter for parameter as include/eec.h declares it (tests/test_host.py compares the two):
# name -> argtypes, or (restype, argtypes) where the entry does not return int.  h*: the pointer is host memory.
PROTOTYPES = {
    "eec_last_error": (C.c_char_p, []),
    "eec_abi_version": [],
    "eec_out_frames": [i],
    "eec_encoder_lengths": [I64, i, i, I32, STREAM],
    "eec_upload_i64_max": [],
    "eec_upload_i64": [hI64, i, I64, STREAM],
    "eec_encoder_create": [CFG, C.POINTER(H)],
    "eec_encoder_destroy": (None, [H]),
    "eec_encoder_pack": [H, PRM, STREAM],
    "eec_encoder_pack_legacy": [H, H, STREAM],
    "eec_encoder_workspace_bytes": (z, [H, i, i]),
    "eec_encoder_forward": [H, F32, I64, i, i, i, F32, F32, VOID, z, i, F32, STREAM],
    "eec_encoder_forward_prefix": [H, F32, I64, i, i, i, i, F32, F32, F32, VOID, z, STREAM],
    "eec_encoder_group_workspace_bytes": (z, [H, i, i]),
    "eec_encoder_stem1_forward": [H, F32, i, i, F32, STREAM],
    "eec_encoder_group_forward": [H, i, F32, I32, i, i, i, VOID, z, STREAM],
    "eec_encoder_head_forward": [H, i, F32, i, F32, i, STREAM],
    "eec_encoder_set_profiling": [H, i, i],
    "eec_encoder_profile_read": [H, hF64, hI64, i],
    "eec_greedy_ctc": [F32, i, i, i, i, I32, I32, STREAM],
    "eec_ctc_loss": [F32, I64, I64, i, i, i, i, i, i, F32, F32, STREAM],
    "eec_ctc_backward_workspace_bytes": (z, [i, i, i, i]),
    "eec_ctc_loss_forward": [F32, I64, I64, i, i, i, i, i, i, F32, F32, VOID, STREAM],
    "eec_ctc_loss_backward": [F32, I64, I64, i, i, i, i, i, i, F32, VOID, F32, F32, STREAM],
    "eec_logsoftmax_backward": [F32, F32, i, i, F32, STREAM],
    "eec_ctc_loss_len": [F32, I64, I64, I32, i, i, i, i, i, i, F32, F32, STREAM],
    "eec_ctc_loss_forward_len": [F32, I64, I64, I32, i, i, i, i, i, i, F32, F32, VOID, STREAM],
    "eec_ctc_loss_backward_len": [F32, I64, I64, I32, i, i, i, i, i, i, F32, VOID, F32, F32, STREAM],
    "eec_exit_distill_workspace_bytes": (z, [i, i, i]),
    "eec_exit_distill_forward": [F32, I32, hI32, i, i, i, i, f, F32, F32, VOID, z, STREAM],
    "eec_exit_distill_backward": [F32, I32, hI32, i, i, i, i, f, F32, i, F32, STREAM],
    "eec_ctc_mwer_workspace_bytes": (z, [i, i, i, i, i]),
    "eec_ctc_hyp_logp": [F32, I32, I32, I32, i, i, i, i, i, i, i, F32, STREAM],
    "eec_ctc_mwer_forward": [F32, I32, I32, I32, F32, i, i, i, i, i, i, i, i, i, F32, F32, F32, VOID, z, STREAM],
    "eec_ctc_mwer_backward": [F32, I32, I32, I32, i, i, i, i, i, i, i, i, i, VOID, z, F32, i, F32, STREAM],
    "eec_exit_stats_workspace_bytes": (z, [i, i, i]),
    "eec_exit_stats": [F32, I32, i, i, i, i, F32, VOID, z, STREAM],
    "eec_exit_route": [F32, i, f, i, i, I32, I32, I32, STREAM],
    "eec_ctc_beam_workspace_bytes": (z, [i, i]),
    "eec_ctc_beam_decode": [F32, i, i, i, i, i, f, VOID, I32, I32, F32, STREAM],
    "eec_ctc_beam_decode_ex": [F32, i, i, i, i, i, f, i, VOID, I32, I32, F32, STREAM],
    "eec_greedy_ctc_len": [F32, I32, i, i, i, i, I32, I32, STREAM],
    "eec_ctc_beam_decode_len": [F32, I32, i, i, i, i, i, f, i, VOID, I32, I32, F32, STREAM],
    "eec_ctc_beam_decode_nbest": [F32, I32, i, i, i, i, i, f, i, i, VOID, I32, I32, F32, I32, STREAM],
    "eec_ctc_trie_pack_bytes": (z, [i, i64]),
    "eec_ctc_trie_pack": [hI32, hI64, i, i, i, i, hVOID, z, hI32, hI32],
    "eec_ctc_lexbeam_workspace_bytes": (z, [i, i, i]),
    "eec_ctc_lexbeam_decode": _LEXBEAM,
    "eec_ngram_pack_bytes": (z, [i, hI64, i]),
    "eec_ngram_pack": [i, hI64, H, H, H, hI32, i, i, i, hVOID, z, hI32],  # words, logp, backoff: HOST arrays of host pointers
    "eec_ctc_lexbeam_lm_decode": _LEXBEAM + [VOID, f],
    "eec_ctc_trie_smear_bytes": (z, [i]),
    "eec_ctc_trie_smear": [hVOID, hVOID, hVOID, z],
    "eec_ctc_lexbeam_lm_smear_decode": _LEXBEAM + [VOID, f, VOID],
    "eec_ctc_lexbeam_logadd_decode": _LEXBEAM + [VOID, f, VOID],
    "eec_ctc_log_add_host": (f, [f, f]),
    "eec_ctc_log_add": [F32, F32, F32, i, STREAM],
    "eec_ctc_lexbeam_wide_workspace_bytes": (z, [i, i, i]),
    "eec_ctc_lexbeam_wide_decode": _LEXBEAM + [VOID, f, VOID, i],
    "eec_ctc_align_workspace_bytes": (z, [i, i, i]),
    "eec_ctc_align": [F32, i, i, i, I32, I64, I32, I32, i, i, i, I32, F32, F32, F32, I32, F32, VOID, STREAM],
    "eec_lexicon_pack_bytes": (z, [i, i64, i]),
    "eec_lexicon_pack": [hW32, hI64, i, hVOID, z, hI32, hI32],
    "eec_lexicon_nearest_workspace_bytes": (z, [i, i]),
    "eec_lexicon_nearest": [VOID, i, U8, I32, i, i, I32, I32, VOID, z, STREAM],
    "eec_edit_distance_workspace_bytes": (z, [i, i, i, i]),
    "eec_edit_distance": [I32, I32, i, i, I32, I32, i, i, I32, I32, U8, I32, VOID, z, STREAM],
    "eec_specaug_draw": [I32, i, i, i, u64, u64, i, i, i, i, f, i, I32, STREAM],
    "eec_specaug_apply": [F32, I32, I32, i, i, i, i, i, i, f, F32, STREAM],
    "eec_resample_plan_bytes": (z, [i, hI32, hI32, i, d]),
    "eec_resample_plan": [i, hI32, hI32, i, d, hVOID, z],
    "eec_speed_draw": [I64, i, i, u64, u64, VOID, I32, I64, STREAM],
    "eec_resample_lengths": [I64, I32, i, i, VOID, I64, STREAM],
    "eec_resample": [F32, I64, I32, i, i, VOID, F32, i, I64, STREAM],
    "eec_rir_bank_bytes": (z, [i, hF32, hI32, i, i]),
    "eec_rir_bank": [i, hF32, hI32, i, i, hVOID, z],
    "eec_noise_bank_bytes": (z, [i, hF32, hI32]),
    "eec_noise_bank": [i, hF32, hI32, hVOID, z],
    "eec_waveaug_partials_bytes": (z, [i, i]),
    "eec_waveaug_draw": [i, u64, u64, VOID, u64, VOID, u64, i, i, d, d, I32, STREAM],
    "eec_reverb": [F32, I64, I32, i, i, VOID, F32, F64, STREAM],
    "eec_noise_energy": [F32, I64, I32, i, i, VOID, F64, STREAM],
    "eec_noise_mix": [F32, I64, I32, i, i, VOID, hF64, i, F64, F32, F32, STREAM],  # snr_gain travels in the argument block
    "eec_rir_spectra_bytes": (z, [hVOID]),
    "eec_rir_spectra": [hVOID, hVOID, z],
    "eec_reverb_fft_workspace_bytes": (z, [i, i]),
    "eec_reverb_fft": [F32, I64, I32, i, i, VOID, VOID, F32, F64, VOID, z, STREAM],
    "eec_reverb_fft_stage": [F32, I64, I32, i, i, VOID, VOID, F32, F64, VOID, z, i, STREAM],
    "eec_frontend_last_error": (C.c_char_p, []),
    "eec_frontend_create": [i, i, i, i, i, C.POINTER(H)],
    "eec_frontend_destroy": (None, [H]),
    "eec_frontend_frames": [i, i],
    "eec_frontend_forward": [H, F32, I64, i, i, F32, STREAM],
    "eec_trainer_last_error": (C.c_char_p, []),
    "eec_trainer_create": [CFG, C.POINTER(H)],
    "eec_trainer_destroy": (None, [H]),
    "eec_trainer_workspace_bytes": (z, [H, i, i]),
    "eec_train_forward": [H, PRM, F32, I64, i, i, i, f, u64, F32, F32, F32, VOID, z, STREAM],
    "eec_train_backward": [H, PRM, PRM, F32, F32, F32, VOID, z, STREAM],
    "eec_train_backward_ex": [H, PRM, PRM, F32, F32, F32, VOID, z, STREAM, GROUP_DONE_FN, H],
    "eec_train_group_workspace_bytes": (z, [CFG, i, i, i]),
    "eec_train_group_forward": [CFG, LAY, i, F32, I32, i, i, i, f, u64, u32, F32, F32, VOID, z, STREAM],
    "eec_train_group_backward": [CFG, LAY, LAY, i, F32, I32, i, i, i, f, u64, u32, F32, F32, VOID, z, STREAM],
    "eec_train_stem_workspace_bytes": (z, [CFG, i, i, i]),
    "eec_train_stem_forward": [CFG, F32, F32, F32, F32, F32, F32, i, i, i, f, u64, u32, F32, VOID, z, STREAM],
    "eec_train_stem_backward": [CFG, i, i, i, i, f, u64, u32, F32, F32, F32, F32, F32, VOID, z, STREAM],
    "eec_train_head_forward": [F32, F32, F32, i, i, i, i, F32, F32, STREAM],
    "eec_train_head_backward_scratch_floats": (z, [i, i, i]),
    "eec_train_head_backward": [F32, F32, F32, F32, i, i, i, i, F32, F32, F32, F32, STREAM],
    "eec_train_gemm": [F32, F32, F32, F32, i, i, i, i, i, i, STREAM],
    "eec_decoder_last_error": (C.c_char_p, []),
    "eec_decoder_workspace_bytes": (z, [i] * 7),
    "eec_decoder_forward": [DEC, i, i, i, i, i, I64, F32, i, i, i, i, i, i, F32, VOID, z, STREAM],
    "eec_decoder_score_workspace_bytes": (z, [i] * 8),
    "eec_decoder_score": [DEC, i, i, i, i, i, i, i, I32, I32, F32, i, i, i, i, i, F32, VOID, z, STREAM],
    "eec_hypothesis_score": [F32, I32, I32, i, i, i, i, F32, STREAM],
    "eec_decoder_train_last_error": (C.c_char_p, []),
    "eec_decoder_train_workspace_bytes": (z, [i] * 8),
    "eec_decoder_train_forward": [DEC, i, i, i, i, i, I64, F32, i, i, i, i, f, u64, i, F32, VOID, z, STREAM],
    "eec_decoder_train_backward": [DEC, DEC, i, i, i, i, I64, F32, i, i, i, i, f, u64, i, F32, F32, VOID, z, STREAM],
    "eec_decoder_step_last_error": (C.c_char_p, []),
    "eec_decoder_step_max_beams": [],
    "eec_decoder_cache_bytes": (z, [i] * 7),
    "eec_decoder_begin": [DEC, i, i, i, i, F32, i, i, i, VOID, z, STREAM],
    "eec_decoder_step": [DEC, i, i, i, i, i, I64, I64, i, i, i, i, i, i, F32, VOID, z, STREAM],
    "eec_decoder_step_multi": [i, DECS, i, i, i, i, i, I64, I64, i, i, i, i, i, i, F32, C.POINTER(H), z, STREAM],
    "eec_decoder_batch_cache_bytes": (z, [i] * 9),
    "eec_decoder_batch_begin": [DECS, i, i, i, i, i, i, F32, i, i, i, VOID, z, STREAM],
    "eec_decoder_batch_step": [DECS, i, i, i, i, i, i, i, I64, I64, i, i, i, i, i, F32, VOID, z, STREAM],
    "eec_beam_select": [i, i, i, i, F32, F32, f, F32, I64, I64, I64, I64, i, i, i, STREAM],
    "eec_ctc_prefix_state_bytes": (z, [i, i, i]),
    "eec_ctc_prefix_begin": [F32, I32, i, i, i, i, i, VOID, z, STREAM],
    "eec_ctc_prefix_step": [F32, I32, i, i, i, i, i, I64, I64, i, i, i, F32, f, i, i, i, F32, VOID, z, STREAM],
    "eec_context_graph_bytes": (z, [i, hI32, hI32, hI32, hF64, i, i, i, i]),
    "eec_context_graph": [i, hI32, hI32, hI32, hF64, i, i, i, i, hVOID, z],
    "eec_ctc_beam_decode_ctx": [F32, I32, i, i, i, i, i, f, i, VOID, I32, I32, F32, VOID, z, I32, F32, STREAM],
    "eec_ctc_beam_decode_nbest_ctx": [F32, I32, i, i, i, i, i, f, i, i, VOID, I32, I32, F32, I32, VOID, z, I32, F32, STREAM],
    "eec_context_bias_state_bytes": (z, [i, i]),
    "eec_context_bias_step": [VOID, z, I32, i, i, i, i, i, i, I64, I64, F32, F32, VOID, z, STREAM],
    "eec_ctc_beam_decode_lm": [F32, I32, i, i, i, i, i, f, i, VOID, I32, I32, F32, VOID, z, f, f, F32, STREAM],
    "eec_ctc_beam_decode_nbest_lm": [F32, I32, i, i, i, i, i, f, i, i, VOID, I32, I32, F32, I32, VOID, z, f, f, F32, STREAM],
    "eec_lm_fusion_state_bytes": (z, [i, i]),
    "eec_lm_fusion_step": [VOID, z, i, i, i, i, i, i, I64, I64, F32, F32, VOID, z, f, f, i, i, i, i, STREAM],
    "eec_keyword_search_workspace_bytes": (z, [i, i]),
    "eec_keyword_search": [F32, i, i, i, I32, I32, I32, i, i, i, F32, I32, I32, F32, I32, VOID, z, STREAM],
    "eec_ctc_forced_align_workspace_bytes": (z, [i, i, i]),
    "eec_ctc_forced_align": [F32, i, i, i, I32, I32, I32, I32, i, i, i, I32, I32, F32, I32, F32, I32, VOID, z, STREAM],
    "eec_ctc_posteriors_workspace_bytes": (z, [i, i, i]),
    "eec_ctc_posteriors": [F32, i, i, i, I32, I32, I32, I32, i, i, i, F32, F32, F32, F32, F32, F32, F32, F32, I32, VOID, z, STREAM],
    "eec_ctc_segment_workspace_bytes": (z, [i, i, i]),
    "eec_ctc_segment": [F32, i, i, i, I32, I32, I32, I32, i, i, i, i, I32, I32, F32, I32, F32, I32, VOID, z, STREAM],
}
EXPORTS = list(PROTOTYPES)
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
    for name, proto in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = proto if isinstance(proto, tuple) else (C.c_int, proto)
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    """Raise on a non-zero return code with the library's message (one per thread, whichever family the entry belongs to)."""
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {load().eec_last_error().decode(errors='replace')}")


def call(name: str, *args) -> None:
    """Entry ``name``, which has no stream parameter (a packer, create / destroy, a setter): raises unless it returns 0."""
    check(getattr(load(), name)(*args), name)


def stream_ptr(dev) -> C.c_void_p:
    """The current HIP stream of ``dev``, as the C entries take it (``launch`` supplies it itself)."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_stream_slot = {}  # entry -> position of its STREAM parameter


def launch(name: str, dev, *args) -> None:
    """Entry ``name`` on ``dev``: the device is made current for the call, its current stream goes into the entry's stream slot
    (``args`` are the other arguments in order: the slot is not always the last), and a non-zero return code raises under the
    entry's own name.  A ``dev`` that is no HIP device gets a NULL stream: the pointer types keep every CPU tensor out of a device
    slot, so such a call ends in the entry's own refusal of its arguments, which is what the host tests ask of it."""
    fn = getattr(load(), name)
    k = _stream_slot.get(name)
    if k is None:
        k = _stream_slot[name] = fn.argtypes.index(STREAM)
    if torch.device(dev).type != "cuda":
        rc = fn(*args[:k], None, *args[k:])
    else:
        with torch.cuda.device(dev):
            rc = fn(*args[:k], torch.cuda.current_stream(dev).cuda_stream, *args[k:])
    check(rc, name)


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
    launch("eec_upload_i64", dev, host, host.numel(), out)
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
