"""ctypes binding of libfat5.so (the C ABI declared in include/fat5.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing the
ops raises -- a GPU box must never silently run something else.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FAT5_LIB_VARIANT selects a developer A/B build (lib/libfat5_<name>.so); unset = the product library
_VAR = os.environ.get("FAT5_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, "lib", "libfat5" + ("_" + _VAR if _VAR else "") + ".so")

FAT5_F32, FAT5_F16, FAT5_BF16 = 0, 1, 2
FAT5_FORCED_BOS, FAT5_FORCED_EOS = 1, 2  # fat5_logits_params.forced_tokens
BIAS_NONE, BIAS_DENSE, BIAS_RPE1D = 0, 1, 2
KV_NATIVE, KV_FP8_E4M3 = 0, 1  # fat5_kv_cache_dtype
MAX_RPE_RADIUS = 1024  # forward alone takes 2048; the backward's per-wave diagonal accumulators must fit LDS (include/fat5.h)

_DT = {torch.float32: FAT5_F32, torch.float16: FAT5_F16, torch.bfloat16: FAT5_BF16}

c_i64x3 = ctypes.c_int64 * 3


class AttnParams(ctypes.Structure):
    """Mirror of `fat5_attn_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("M", ctypes.c_int32), ("N", ctypes.c_int32),
        ("D", ctypes.c_int32), ("dtype", ctypes.c_int32), ("causal", ctypes.c_int32),
        ("bias_mode", ctypes.c_int32), ("sm_scale", ctypes.c_float), ("rpe_radius", ctypes.c_int32),
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("o", ctypes.c_void_p),
        ("lse", ctypes.c_void_p),
        ("q_stride", c_i64x3), ("k_stride", c_i64x3), ("v_stride", c_i64x3), ("o_stride", c_i64x3),
        ("bias", ctypes.c_void_p), ("bias_stride", c_i64x3), ("rpe1d", ctypes.c_void_p),
        ("cu_seqlens_q", ctypes.c_void_p), ("cu_seqlens_k", ctypes.c_void_p),
        ("total_q", ctypes.c_int32), ("total_k", ctypes.c_int32),
        ("dout", ctypes.c_void_p), ("dq", ctypes.c_void_p), ("dk", ctypes.c_void_p), ("dv", ctypes.c_void_p),
        ("do_stride", c_i64x3), ("dq_stride", c_i64x3), ("dk_stride", c_i64x3), ("dv_stride", c_i64x3),
        ("dbias", ctypes.c_void_p), ("dbias_batch", ctypes.c_int32), ("dbias_heads", ctypes.c_int32),
        ("drpe1d", ctypes.c_void_p), ("rpe_bucket", ctypes.c_void_p), ("drpe_table", ctypes.c_void_p),
        ("rpe_num_buckets", ctypes.c_int32), ("unit_begin", ctypes.c_int32), ("unit_count", ctypes.c_int32),
        ("variant", ctypes.c_int32),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
        ("rpe_bucket_host", ctypes.c_void_p),
    ]


c_i64x3x3 = c_i64x3 * 3


class RopeParams(ctypes.Structure):
    """Mirror of `fat5_rope_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("S", ctypes.c_int32), ("S_k", ctypes.c_int32), ("H", ctypes.c_int32), ("D", ctypes.c_int32),
        ("rd", ctypes.c_int32), ("dtype", ctypes.c_int32), ("interleaved", ctypes.c_int32), ("conjugate", ctypes.c_int32),
        ("n_tensors", ctypes.c_int32), ("n_q", ctypes.c_int32), ("table_rows", ctypes.c_int32),
        ("cos", ctypes.c_void_p), ("sin", ctypes.c_void_p), ("cos_k", ctypes.c_void_p), ("sin_k", ctypes.c_void_p),
        ("x", ctypes.c_void_p * 3), ("y", ctypes.c_void_p * 3), ("x_stride", c_i64x3x3), ("y_stride", c_i64x3x3),
        ("cu_seqlens", ctypes.c_void_p), ("cu_seqlens_k", ctypes.c_void_p),
    ]

class FireParams(ctypes.Structure):
    """Mirror of `fat5_fire_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("eps", ctypes.c_float),
        ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
        ("c", ctypes.c_void_p), ("L_multiplier", ctypes.c_void_p), ("init_L", ctypes.c_void_p),
        ("bias", ctypes.c_void_p), ("dbias", ctypes.c_void_p), ("bias_stride", ctypes.c_int64 * 2),
        ("dw1", ctypes.c_void_p), ("db1", ctypes.c_void_p), ("dw2", ctypes.c_void_p), ("db2", ctypes.c_void_p),
        ("dc", ctypes.c_void_p), ("dL_multiplier", ctypes.c_void_p),
    ]


class DecodeParams(ctypes.Structure):
    """Mirror of `fat5_decode_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("D", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("capacity", ctypes.c_int32), ("N", ctypes.c_int32), ("cache_seqlens", ctypes.c_void_p), ("sm_scale", ctypes.c_float),
        ("bias_mode", ctypes.c_int32), ("rpe_radius", ctypes.c_int32), ("rpe1d", ctypes.c_void_p),
        ("q", ctypes.c_void_p), ("k_cache", ctypes.c_void_p), ("v_cache", ctypes.c_void_p), ("k_new", ctypes.c_void_p),
        ("v_new", ctypes.c_void_p), ("o", ctypes.c_void_p), ("lse", ctypes.c_void_p),
        ("q_stride", ctypes.c_int64 * 2), ("k_cache_stride", c_i64x3), ("v_cache_stride", c_i64x3),
        ("k_new_stride", ctypes.c_int64 * 2), ("v_new_stride", ctypes.c_int64 * 2), ("o_stride", ctypes.c_int64 * 2),
        ("num_splits", ctypes.c_int32), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
        ("cache_batch_idx", ctypes.c_void_p), ("cache_row_batch", ctypes.c_void_p), ("cache_B", ctypes.c_int32),
    ]


class DecodeKV8Params(ctypes.Structure):
    """Mirror of `fat5_decode_kv8_params` (include/fat5.h): `fat5_decode_params` followed by the FP8-cache fields.  The fields of
    `base` are reachable on the instance itself (`p.B` is `p.base.B`)."""
    _anonymous_ = ("base",)
    _fields_ = [
        ("base", DecodeParams),
        ("cache_dtype", ctypes.c_int32), ("k_scale", ctypes.c_void_p), ("v_scale", ctypes.c_void_p),
        ("k_scale_stride", c_i64x3), ("v_scale_stride", c_i64x3),
    ]


class DecodeChunkParams(ctypes.Structure):
    """Mirror of `fat5_decode_chunk_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("H", ctypes.c_int32), ("M", ctypes.c_int32), ("D", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("capacity", ctypes.c_int32), ("N", ctypes.c_int32), ("causal", ctypes.c_int32), ("cache_seqlens", ctypes.c_void_p),
        ("sm_scale", ctypes.c_float), ("bias_mode", ctypes.c_int32), ("rpe_radius", ctypes.c_int32), ("rpe1d", ctypes.c_void_p),
        ("q", ctypes.c_void_p), ("k_cache", ctypes.c_void_p), ("v_cache", ctypes.c_void_p), ("k_new", ctypes.c_void_p),
        ("v_new", ctypes.c_void_p), ("o", ctypes.c_void_p), ("lse", ctypes.c_void_p),
        ("q_stride", c_i64x3), ("k_cache_stride", c_i64x3), ("v_cache_stride", c_i64x3),
        ("k_new_stride", c_i64x3), ("v_new_stride", c_i64x3), ("o_stride", c_i64x3),
        ("num_splits", ctypes.c_int32), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
        ("chunk_seqlens", ctypes.c_void_p),
        ("cache_dtype", ctypes.c_int32), ("k_scale", ctypes.c_void_p), ("v_scale", ctypes.c_void_p),
        ("k_scale_stride", c_i64x3), ("v_scale_stride", c_i64x3),
    ]


class KvQuantParams(ctypes.Structure):
    """Mirror of `fat5_kv_quant_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("L", ctypes.c_int32), ("H", ctypes.c_int32), ("D", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("out", ctypes.c_void_p), ("scale", ctypes.c_void_p),
        ("x_stride", c_i64x3), ("out_stride", c_i64x3), ("scale_stride", c_i64x3),
    ]


class SampleParams(ctypes.Structure):
    """Mirror of `fat5_sample_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("V", ctypes.c_int32), ("dtype", ctypes.c_int32), ("top_k", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("temperature", ctypes.c_float), ("top_p", ctypes.c_float),
        ("seed", ctypes.c_uint64), ("offset", ctypes.c_int64), ("offsets", ctypes.c_void_p), ("uniforms", ctypes.c_void_p),
        ("tokens", ctypes.c_void_p), ("aux", ctypes.c_void_p),
    ]


class BeamParams(ctypes.Structure):
    """Mirror of `fat5_beam_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("k", ctypes.c_int32), ("V", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("running_scores", ctypes.c_void_p),
        ("running_seqs", ctypes.c_void_p), ("cache_row_batch", ctypes.c_void_p), ("finished_seqs", ctypes.c_void_p),
        ("finished_scores", ctypes.c_void_p), ("finished_flags", ctypes.c_void_p), ("finished_lens", ctypes.c_void_p),
        ("heuristic", ctypes.c_void_p), ("status", ctypes.c_void_p), ("tokens", ctypes.c_void_p), ("step", ctypes.c_void_p),
        ("seq_len", ctypes.c_int32), ("capacity", ctypes.c_int32), ("max_length", ctypes.c_int32), ("early_stopping", ctypes.c_int32),
        ("length_penalty", ctypes.c_float), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
        ("logits_normalized", ctypes.c_int32),
    ]


class LogitsParams(ctypes.Structure):
    """Mirror of `fat5_logits_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("rows", ctypes.c_int32), ("V", ctypes.c_int32), ("dtype", ctypes.c_int32), ("log_softmax", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64),
        ("sequences", ctypes.c_void_p), ("seq_stride", ctypes.c_int64), ("lengths", ctypes.c_void_p), ("seq_len", ctypes.c_int32),
        ("repetition_penalty", ctypes.c_float), ("no_repeat_ngram_size", ctypes.c_int32), ("min_length", ctypes.c_int32),
        ("eos_token_id", ctypes.c_int32), ("n_suppress", ctypes.c_int32), ("suppress_tokens", ctypes.c_void_p),
        # appended: all zero / None is the call as it was
        ("encoder_repetition_penalty", ctypes.c_double), ("encoder_input_ids", ctypes.c_void_p), ("encoder_stride", ctypes.c_int64),
        ("encoder_lengths", ctypes.c_void_p), ("encoder_rows", ctypes.c_int32), ("encoder_len", ctypes.c_int32),
        ("rows_per_encoder_row", ctypes.c_int32), ("encoder_no_repeat_ngram_size", ctypes.c_int32),
        ("bad_words_ids", ctypes.c_void_p), ("bad_words_offsets", ctypes.c_void_p), ("bad_words_offsets_host", ctypes.c_void_p),
        ("n_bad_words", ctypes.c_int32), ("n_bad_word_ids", ctypes.c_int32), ("min_new_tokens", ctypes.c_int32),
        ("prompt_length", ctypes.c_int32), ("prompt_lengths", ctypes.c_void_p), ("max_new_tokens", ctypes.c_int32),
        ("forced_tokens", ctypes.c_int32), ("forced_bos_token_id", ctypes.c_int32), ("forced_eos_token_id", ctypes.c_int32),
    ]


class SpecParams(ctypes.Structure):
    """Mirror of `fat5_spec_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("M", ctypes.c_int32), ("V", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("batch_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64),
        ("draft", ctypes.c_void_p), ("draft_stride", ctypes.c_int64), ("cache_seqlens", ctypes.c_void_p),
        ("draft_seqlens", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("labels_stride", ctypes.c_int64),
        ("ncols", ctypes.c_int32), ("eos_token_id", ctypes.c_int32), ("tok", ctypes.c_void_p), ("seen_eos", ctypes.c_void_p),
        ("limit", ctypes.c_void_p), ("limit_scalar", ctypes.c_int32), ("n_accepted", ctypes.c_void_p), ("n_new", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class SpecSampleParams(ctypes.Structure):
    """Mirror of `fat5_spec_sample_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("spec", SpecParams), ("draft_logits", ctypes.c_void_p), ("draft_batch_stride", ctypes.c_int64),
        ("draft_row_stride", ctypes.c_int64), ("temperature", ctypes.c_float), ("top_p", ctypes.c_float),
        ("top_k", ctypes.c_int32), ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64), ("offset", ctypes.c_int64),
        ("uniforms", ctypes.c_void_p), ("sampled", ctypes.c_void_p), ("aux", ctypes.c_void_p),
    ]


class LookupParams(ctypes.Structure):
    """Mirror of `fat5_lookup_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("L_src", ctypes.c_int32), ("ncols", ctypes.c_int32), ("gamma", ctypes.c_int32),
        ("max_ngram", ctypes.c_int32), ("V", ctypes.c_int32),
        ("source", ctypes.c_void_p), ("source_stride", ctypes.c_int64), ("src_seqlens", ctypes.c_void_p),
        ("labels", ctypes.c_void_p), ("labels_stride", ctypes.c_int64), ("cache_seqlens", ctypes.c_void_p),
        ("tok", ctypes.c_void_p), ("seen_eos", ctypes.c_void_p), ("draft", ctypes.c_void_p), ("draft_stride", ctypes.c_int64),
        ("n_proposed", ctypes.c_void_p),
    ]


class PackParams(ctypes.Structure):
    """Mirror of `fat5_pack_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("L", ctypes.c_int32), ("seg_cap", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("seg", ctypes.c_void_p), ("cu_seqlens", ctypes.c_void_p), ("index", ctypes.c_void_p), ("seg_count", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
    ]


class Ul2Params(ctypes.Structure):
    """Mirror of `fat5_ul2_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("B", ctypes.c_int32), ("L", ctypes.c_int32), ("max_length", ctypes.c_int32), ("max_labels_length", ctypes.c_int32),
        ("num_denoisers", ctypes.c_int32), ("num_sentinels", ctypes.c_int32), ("random_chunk", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("sentinel_first_id", ctypes.c_int64), ("eos_token_id", ctypes.c_int64), ("pad_token_id", ctypes.c_int64), ("seed", ctypes.c_uint64),
        ("tokens", ctypes.c_void_p), ("tokens_stride", ctypes.c_int64), ("lengths", ctypes.c_void_p), ("step", ctypes.c_void_p),
        ("mu", ctypes.c_void_p), ("r", ctypes.c_void_p), ("max_spans", ctypes.c_void_p), ("tokens_len", ctypes.c_void_p),
        ("prefix_off", ctypes.c_void_p), ("prefix_ids", ctypes.c_void_p), ("cum_prop", ctypes.c_void_p),
        ("noise_mask", ctypes.c_void_p), ("noise_mask_stride", ctypes.c_int64), ("denoiser_in", ctypes.c_void_p),
        ("input_ids", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("attention_mask", ctypes.c_void_p),
        ("decoder_attention_mask", ctypes.c_void_p), ("enc_len", ctypes.c_void_p), ("dec_len", ctypes.c_void_p),
        ("denoiser", ctypes.c_void_p), ("status", ctypes.c_void_p),
    ]


class W8QuantParams(ctypes.Structure):
    """Mirror of `fat5_w8_quant_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("N", ctypes.c_int64), ("K", ctypes.c_int32), ("dtype", ctypes.c_int32), ("w", ctypes.c_void_p), ("w_stride", ctypes.c_int64),
        ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64), ("scale", ctypes.c_void_p),
    ]


class W8LinearParams(ctypes.Structure):
    """Mirror of `fat5_w8_linear_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("R", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("x_stride", ctypes.c_int64), ("w8", ctypes.c_void_p), ("w_stride", ctypes.c_int64),
        ("scale", ctypes.c_void_p), ("norm_weight", ctypes.c_void_p), ("eps", ctypes.c_float), ("reserved", ctypes.c_int32),
        ("residual", ctypes.c_void_p), ("residual_stride", ctypes.c_int64), ("y", ctypes.c_void_p), ("y_stride", ctypes.c_int64),
    ]


POOL_EOS, POOL_FIRST, POOL_LAST, POOL_MEAN = 0, 1, 2, 3  # fat5_pool_mode


class SeqPoolParams(ctypes.Structure):
    """Mirror of `fat5_seq_pool_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("mode", ctypes.c_int32), ("dtype", ctypes.c_int32), ("nseq", ctypes.c_int32), ("L", ctypes.c_int32),
        ("total", ctypes.c_int64), ("d", ctypes.c_int64), ("eos_token_id", ctypes.c_int64),
        ("hidden", ctypes.c_void_p), ("hidden_row_stride", ctypes.c_int64), ("hidden_batch_stride", ctypes.c_int64),
        ("cu_seqlens", ctypes.c_void_p), ("seqlens", ctypes.c_void_p), ("input_ids", ctypes.c_void_p),
        ("ids_batch_stride", ctypes.c_int64), ("pooled", ctypes.c_void_p), ("pooled_stride", ctypes.c_int64),
        ("position", ctypes.c_void_p), ("found", ctypes.c_void_p), ("dpooled", ctypes.c_void_p), ("dpooled_stride", ctypes.c_int64),
        ("dhidden", ctypes.c_void_p), ("dhidden_row_stride", ctypes.c_int64), ("dhidden_batch_stride", ctypes.c_int64),
    ]


class KdParams(ctypes.Structure):
    """Mirror of `fat5_kd_params` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32), ("rows", ctypes.c_int64), ("n_cols", ctypes.c_int64),
        ("logits", ctypes.c_void_p), ("row_stride", ctypes.c_int64), ("teacher_logits", ctypes.c_void_p),
        ("teacher_row_stride", ctypes.c_int64), ("labels", ctypes.c_void_p), ("dlosses", ctypes.c_void_p), ("dloss_stride", ctypes.c_int64),
        ("losses", ctypes.c_void_p), ("kd_losses", ctypes.c_void_p), ("z_losses", ctypes.c_void_p), ("ce_losses", ctypes.c_void_p),
        ("lse", ctypes.c_void_p), ("lse_student_t", ctypes.c_void_p), ("lse_teacher_t", ctypes.c_void_p),
        ("dlogits", ctypes.c_void_p), ("dlogits_row_stride", ctypes.c_int64), ("ignore_index", ctypes.c_int64),
        ("alpha", ctypes.c_float), ("temperature", ctypes.c_float), ("label_smoothing", ctypes.c_float), ("logit_scale", ctypes.c_float),
        ("lse_square_scale", ctypes.c_float), ("reserved2", ctypes.c_int32),
    ]


class DropoutDesc(ctypes.Structure):
    """Mirror of `fat5_dropout_desc` (include/fat5.h) -- field order must match exactly."""
    _fields_ = [
        ("seed", ctypes.c_uint64), ("step", ctypes.c_void_p), ("elem_offset", ctypes.c_uint64), ("site", ctypes.c_uint32),
        ("p", ctypes.c_float),
    ]


EXPORTS = (
    "fat5_version", "fat5_chip_cus", "fat5_last_error", "fat5_sizeof_attn_params", "fat5_attn_fwd", "fat5_attn_bwd_workspace_bytes", "fat5_attn_bwd", "fat5_attn_bwd_launches", "fat5_attn_bwd_kvres",
    "fat5_attn_bwd_stages", "fat5_attn_describe", "fat5_rpe1d_from_table",
    "fat5_rmsnorm_fwd", "fat5_rmsnorm_bwd_workspace_bytes", "fat5_rmsnorm_bwd", "fat5_add_rmsnorm_fwd", "fat5_add_rmsnorm_bwd",
    "fat5_ce_fwd", "fat5_ce_bwd", "fat5_ce_fwd_bwd", "fat5_fold_weights", "fat5_fold_weights_bwd", "fat5_fold_weights_bwd_scratch_bytes", "fat5_rmsnorm_unit_bwd", "fat5_gated_act_fwd", "fat5_gated_act_bwd",
    "fat5_adamw_scale_step", "fat5_adamw_scale_step_clipped", "fat5_adamw_scale_step_dev", "fat5_adamw_grad_sumsq", "fat5_sizeof_adamw_tensor",
    "fat5_rope_apply", "fat5_sizeof_rope_params",
    "fat5_fire_fwd", "fat5_fire_bwd", "fat5_fire_bwd_workspace_bytes", "fat5_sizeof_fire_params",
    "fat5_attn_decode", "fat5_attn_decode_workspace_bytes", "fat5_sizeof_decode_params",
    "fat5_attn_decode_kv8", "fat5_sizeof_decode_kv8_params",
    "fat5_attn_decode_chunk", "fat5_attn_decode_chunk_workspace_bytes", "fat5_sizeof_decode_chunk_params",
    "fat5_sample_logits", "fat5_sizeof_sample_params",
    "fat5_beam_step", "fat5_beam_step_workspace_bytes", "fat5_sizeof_beam_params",
    "fat5_process_logits", "fat5_sizeof_logits_params",
    "fat5_spec_accept", "fat5_spec_accept_workspace_bytes", "fat5_sizeof_spec_params",
    "fat5_spec_accept_sampled", "fat5_spec_accept_sampled_workspace_bytes", "fat5_sizeof_spec_sample_params",
    "fat5_kv_quantize", "fat5_sizeof_kv_quant_params",
    "fat5_lookup_draft", "fat5_sizeof_lookup_params",
    "fat5_pack_plan", "fat5_sizeof_pack_params",
    "fat5_ul2_collate", "fat5_sizeof_ul2_params",
    "fat5_w8_quantize", "fat5_sizeof_w8_quant_params", "fat5_w8_linear", "fat5_sizeof_w8_linear_params",
    "fat5_dropout", "fat5_dropout_add_rmsnorm_fwd", "fat5_dropout_add_rmsnorm_bwd", "fat5_sizeof_dropout_desc",
    "fat5_seq_pool_fwd", "fat5_seq_pool_bwd", "fat5_sizeof_seq_pool_params",
    "fat5_kd_fwd", "fat5_kd_bwd", "fat5_kd_fwd_bwd", "fat5_sizeof_kd_params",
)

_lib = None


def load():
    """Load libfat5.so once; raise loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python flasht5_amd/build.py` (hipcc, gfx950). "
            "flasht5_amd has no non-HIP fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.fat5_version.restype = ctypes.c_int
    lib.fat5_last_error.restype = ctypes.c_char_p
    lib.fat5_attn_fwd.restype = ctypes.c_int
    lib.fat5_attn_fwd.argtypes = [ctypes.POINTER(AttnParams), ctypes.c_void_p]
    lib.fat5_attn_bwd.restype = ctypes.c_int
    lib.fat5_attn_bwd.argtypes = [ctypes.POINTER(AttnParams), ctypes.c_void_p]
    lib.fat5_attn_bwd_stages.restype = ctypes.c_int
    lib.fat5_attn_bwd_stages.argtypes = [ctypes.POINTER(AttnParams), ctypes.c_int, ctypes.c_void_p]
    lib.fat5_attn_bwd_launches.restype = ctypes.c_int
    lib.fat5_attn_bwd_launches.argtypes = [ctypes.POINTER(AttnParams)]
    lib.fat5_attn_bwd_kvres.restype = ctypes.c_int
    lib.fat5_attn_bwd_kvres.argtypes = [ctypes.POINTER(AttnParams)]
    lib.fat5_attn_describe.restype = ctypes.c_int
    lib.fat5_attn_describe.argtypes = [ctypes.POINTER(AttnParams), ctypes.c_char_p, ctypes.c_size_t]
    lib.fat5_attn_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_attn_bwd_workspace_bytes.argtypes = [ctypes.POINTER(AttnParams)]
    lib.fat5_rpe1d_from_table.restype = ctypes.c_int
    lib.fat5_rpe1d_from_table.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_void_p]
    i64, f32, vp, i32 = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int
    lib.fat5_rmsnorm_fwd.restype = ctypes.c_int
    lib.fat5_rmsnorm_fwd.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, f32, i32, i32, vp]
    lib.fat5_rmsnorm_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_rmsnorm_bwd_workspace_bytes.argtypes = [i64, i64]
    lib.fat5_rmsnorm_bwd.restype = ctypes.c_int
    lib.fat5_rmsnorm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, i32, vp, ctypes.c_size_t, vp]
    lib.fat5_add_rmsnorm_fwd.restype = ctypes.c_int
    lib.fat5_add_rmsnorm_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, f32, i32, i32, vp]
    lib.fat5_add_rmsnorm_bwd.restype = ctypes.c_int
    lib.fat5_add_rmsnorm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, i32, i32, vp, ctypes.c_size_t, vp]
    lib.fat5_ce_fwd.restype = ctypes.c_int
    lib.fat5_ce_fwd.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, f32, f32, f32, i64, i32, i32, vp]
    lib.fat5_fold_weights_bwd.restype = ctypes.c_int
    lib.fat5_fold_weights_bwd.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, i64, i32, vp, ctypes.c_size_t, vp]
    lib.fat5_fold_weights_bwd_scratch_bytes.restype = ctypes.c_size_t
    lib.fat5_gated_act_fwd.restype = ctypes.c_int
    lib.fat5_gated_act_fwd.argtypes = [vp, vp, vp, i64, i64, i64, i64, i64, i32, i32, vp]
    lib.fat5_gated_act_bwd.restype = ctypes.c_int
    lib.fat5_gated_act_bwd.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, i32, i32, vp]
    lib.fat5_fold_weights_bwd_scratch_bytes.argtypes = [i64, i64]
    lib.fat5_rmsnorm_unit_bwd.restype = ctypes.c_int
    lib.fat5_rmsnorm_unit_bwd.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, i64, i32, vp]
    lib.fat5_fold_weights.restype = ctypes.c_int
    lib.fat5_fold_weights.argtypes = [vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, i64, i32, vp]
    lib.fat5_ce_bwd.restype = ctypes.c_int
    lib.fat5_ce_bwd.argtypes = [vp, i64, vp, vp, vp, vp, i64, i64, i64, i64, f32, f32, f32, i64, i32, vp]
    lib.fat5_ce_fwd_bwd.restype = ctypes.c_int
    lib.fat5_ce_fwd_bwd.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, i64, i64, i64, i64, f32, f32, f32, i64, i32, vp]
    lib.fat5_adamw_scale_step.restype = ctypes.c_int
    f64 = ctypes.c_double
    lib.fat5_adamw_scale_step.argtypes = [vp, i32, i32, vp, f64, f64, f64, f64, f64, i32, i32, i32, vp]
    lib.fat5_adamw_scale_step_clipped.restype = ctypes.c_int
    lib.fat5_adamw_scale_step_dev.restype = ctypes.c_int
    lib.fat5_adamw_scale_step_dev.argtypes = [vp, i32, i32, vp, vp, f64, f64, f64, i32, i32, i32, vp, vp]
    lib.fat5_adamw_scale_step_clipped.argtypes = [vp, i32, i32, vp, f64, f64, f64, f64, f64, i32, i32, i32, vp, vp]
    lib.fat5_adamw_grad_sumsq.restype = ctypes.c_int
    lib.fat5_adamw_grad_sumsq.argtypes = [vp, i32, i32, vp, i32, vp]
    lib.fat5_sizeof_adamw_tensor.restype = ctypes.c_size_t
    lib.fat5_rope_apply.restype = ctypes.c_int
    lib.fat5_rope_apply.argtypes = [ctypes.POINTER(RopeParams), ctypes.c_void_p]
    lib.fat5_sizeof_rope_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_rope_params() != ctypes.sizeof(RopeParams):
        raise ImportError(f"fat5_rope_params layout mismatch: library {lib.fat5_sizeof_rope_params()} B, "
                          f"binding {ctypes.sizeof(RopeParams)} B")
    lib.fat5_fire_fwd.restype = ctypes.c_int
    lib.fat5_fire_fwd.argtypes = [ctypes.POINTER(FireParams), ctypes.c_void_p]
    lib.fat5_fire_bwd.restype = ctypes.c_int
    lib.fat5_fire_bwd.argtypes = [ctypes.POINTER(FireParams), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fat5_fire_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_fire_bwd_workspace_bytes.argtypes = [ctypes.POINTER(FireParams)]
    lib.fat5_sizeof_fire_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_fire_params() != ctypes.sizeof(FireParams):
        raise ImportError(f"fat5_fire_params layout mismatch: library {lib.fat5_sizeof_fire_params()} B, "
                          f"binding {ctypes.sizeof(FireParams)} B")
    lib.fat5_attn_decode.restype = ctypes.c_int
    lib.fat5_attn_decode.argtypes = [ctypes.POINTER(DecodeParams), ctypes.c_void_p]
    lib.fat5_attn_decode_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_attn_decode_workspace_bytes.argtypes = [ctypes.POINTER(DecodeParams)]
    lib.fat5_sizeof_decode_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_decode_params() != ctypes.sizeof(DecodeParams):
        raise ImportError(f"fat5_decode_params layout mismatch: library {lib.fat5_sizeof_decode_params()} B, "
                          f"binding {ctypes.sizeof(DecodeParams)} B")
    lib.fat5_attn_decode_kv8.restype = ctypes.c_int
    lib.fat5_attn_decode_kv8.argtypes = [ctypes.POINTER(DecodeKV8Params), ctypes.c_void_p]
    lib.fat5_sizeof_decode_kv8_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_decode_kv8_params() != ctypes.sizeof(DecodeKV8Params):
        raise ImportError(f"fat5_decode_kv8_params layout mismatch: library {lib.fat5_sizeof_decode_kv8_params()} B, "
                          f"binding {ctypes.sizeof(DecodeKV8Params)} B")
    lib.fat5_attn_decode_chunk.restype = ctypes.c_int
    lib.fat5_attn_decode_chunk.argtypes = [ctypes.POINTER(DecodeChunkParams), ctypes.c_void_p]
    lib.fat5_attn_decode_chunk_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_attn_decode_chunk_workspace_bytes.argtypes = [ctypes.POINTER(DecodeChunkParams)]
    lib.fat5_sizeof_decode_chunk_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_decode_chunk_params() != ctypes.sizeof(DecodeChunkParams):
        raise ImportError(f"fat5_decode_chunk_params layout mismatch: library {lib.fat5_sizeof_decode_chunk_params()} B, "
                          f"binding {ctypes.sizeof(DecodeChunkParams)} B")
    lib.fat5_sample_logits.restype = ctypes.c_int
    lib.fat5_sample_logits.argtypes = [ctypes.POINTER(SampleParams), ctypes.c_void_p]
    lib.fat5_sizeof_sample_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_sample_params() != ctypes.sizeof(SampleParams):
        raise ImportError(f"fat5_sample_params layout mismatch: library {lib.fat5_sizeof_sample_params()} B, "
                          f"binding {ctypes.sizeof(SampleParams)} B")
    lib.fat5_beam_step.restype = ctypes.c_int
    lib.fat5_beam_step.argtypes = [ctypes.POINTER(BeamParams), ctypes.c_void_p]
    lib.fat5_beam_step_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_beam_step_workspace_bytes.argtypes = [ctypes.POINTER(BeamParams)]
    lib.fat5_sizeof_beam_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_beam_params() != ctypes.sizeof(BeamParams):
        raise ImportError(f"fat5_beam_params layout mismatch: library {lib.fat5_sizeof_beam_params()} B, "
                          f"binding {ctypes.sizeof(BeamParams)} B")
    lib.fat5_process_logits.restype = ctypes.c_int
    lib.fat5_process_logits.argtypes = [ctypes.POINTER(LogitsParams), ctypes.c_void_p]
    lib.fat5_sizeof_logits_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_logits_params() != ctypes.sizeof(LogitsParams):
        raise ImportError(f"fat5_logits_params layout mismatch: library {lib.fat5_sizeof_logits_params()} B, "
                          f"binding {ctypes.sizeof(LogitsParams)} B")
    lib.fat5_spec_accept.restype = ctypes.c_int
    lib.fat5_spec_accept.argtypes = [ctypes.POINTER(SpecParams), ctypes.c_void_p]
    lib.fat5_spec_accept_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_spec_accept_workspace_bytes.argtypes = [ctypes.POINTER(SpecParams)]
    lib.fat5_sizeof_spec_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_spec_params() != ctypes.sizeof(SpecParams):
        raise ImportError(f"fat5_spec_params layout mismatch: library {lib.fat5_sizeof_spec_params()} B, "
                          f"binding {ctypes.sizeof(SpecParams)} B")
    lib.fat5_spec_accept_sampled.restype = ctypes.c_int
    lib.fat5_spec_accept_sampled.argtypes = [ctypes.POINTER(SpecSampleParams), ctypes.c_void_p]
    lib.fat5_spec_accept_sampled_workspace_bytes.restype = ctypes.c_size_t
    lib.fat5_spec_accept_sampled_workspace_bytes.argtypes = [ctypes.POINTER(SpecSampleParams)]
    lib.fat5_sizeof_spec_sample_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_spec_sample_params() != ctypes.sizeof(SpecSampleParams):
        raise ImportError(f"fat5_spec_sample_params layout mismatch: library {lib.fat5_sizeof_spec_sample_params()} B, "
                          f"binding {ctypes.sizeof(SpecSampleParams)} B")
    lib.fat5_kv_quantize.restype = ctypes.c_int
    lib.fat5_kv_quantize.argtypes = [ctypes.POINTER(KvQuantParams), ctypes.c_void_p]
    lib.fat5_sizeof_kv_quant_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_kv_quant_params() != ctypes.sizeof(KvQuantParams):
        raise ImportError(f"fat5_kv_quant_params layout mismatch: library {lib.fat5_sizeof_kv_quant_params()} B, "
                          f"binding {ctypes.sizeof(KvQuantParams)} B")
    lib.fat5_lookup_draft.restype = ctypes.c_int
    lib.fat5_lookup_draft.argtypes = [ctypes.POINTER(LookupParams), ctypes.c_void_p]
    lib.fat5_sizeof_lookup_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_lookup_params() != ctypes.sizeof(LookupParams):
        raise ImportError(f"fat5_lookup_params layout mismatch: library {lib.fat5_sizeof_lookup_params()} B, "
                          f"binding {ctypes.sizeof(LookupParams)} B")
    lib.fat5_pack_plan.restype = ctypes.c_int
    lib.fat5_pack_plan.argtypes = [ctypes.POINTER(PackParams), ctypes.c_void_p]
    lib.fat5_sizeof_pack_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_pack_params() != ctypes.sizeof(PackParams):
        raise ImportError(f"fat5_pack_params layout mismatch: library {lib.fat5_sizeof_pack_params()} B, "
                          f"binding {ctypes.sizeof(PackParams)} B")
    lib.fat5_ul2_collate.restype = ctypes.c_int
    lib.fat5_ul2_collate.argtypes = [ctypes.POINTER(Ul2Params), ctypes.c_void_p]
    lib.fat5_sizeof_ul2_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_ul2_params() != ctypes.sizeof(Ul2Params):
        raise ImportError(f"fat5_ul2_params layout mismatch: library {lib.fat5_sizeof_ul2_params()} B, "
                          f"binding {ctypes.sizeof(Ul2Params)} B")
    for fn, size_fn, struct, name in ((lib.fat5_w8_quantize, lib.fat5_sizeof_w8_quant_params, W8QuantParams, "fat5_w8_quant_params"),
                                      (lib.fat5_w8_linear, lib.fat5_sizeof_w8_linear_params, W8LinearParams, "fat5_w8_linear_params")):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(struct), ctypes.c_void_p]
        size_fn.restype = ctypes.c_size_t
        if size_fn() != ctypes.sizeof(struct):
            raise ImportError(f"{name} layout mismatch: library {size_fn()} B, binding {ctypes.sizeof(struct)} B")
    for fn in (lib.fat5_seq_pool_fwd, lib.fat5_seq_pool_bwd):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(SeqPoolParams), ctypes.c_void_p]
    lib.fat5_sizeof_seq_pool_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_seq_pool_params() != ctypes.sizeof(SeqPoolParams):
        raise ImportError(f"fat5_seq_pool_params layout mismatch: library {lib.fat5_sizeof_seq_pool_params()} B, "
                          f"binding {ctypes.sizeof(SeqPoolParams)} B")
    for fn in (lib.fat5_kd_fwd, lib.fat5_kd_bwd, lib.fat5_kd_fwd_bwd):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(KdParams), ctypes.c_void_p]
    lib.fat5_sizeof_kd_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_kd_params() != ctypes.sizeof(KdParams):
        raise ImportError(f"fat5_kd_params layout mismatch: library {lib.fat5_sizeof_kd_params()} B, "
                          f"binding {ctypes.sizeof(KdParams)} B")
    dd = ctypes.POINTER(DropoutDesc)
    lib.fat5_dropout.restype = ctypes.c_int
    lib.fat5_dropout.argtypes = [vp, vp, vp, i64, i64, i64, i64, i64, dd, i32, vp]
    lib.fat5_dropout_add_rmsnorm_fwd.restype = ctypes.c_int
    lib.fat5_dropout_add_rmsnorm_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, f32, dd, i32, i32, vp]
    lib.fat5_dropout_add_rmsnorm_bwd.restype = ctypes.c_int
    lib.fat5_dropout_add_rmsnorm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, dd, i32, i32, vp,
                                                 ctypes.c_size_t, vp]
    lib.fat5_sizeof_dropout_desc.restype = ctypes.c_size_t
    if lib.fat5_sizeof_dropout_desc() != ctypes.sizeof(DropoutDesc):
        raise ImportError(f"fat5_dropout_desc layout mismatch: library {lib.fat5_sizeof_dropout_desc()} B, "
                          f"binding {ctypes.sizeof(DropoutDesc)} B")
    lib.fat5_sizeof_attn_params.restype = ctypes.c_size_t
    if lib.fat5_sizeof_attn_params() != ctypes.sizeof(AttnParams):
        raise ImportError(f"fat5_attn_params layout mismatch: library {lib.fat5_sizeof_attn_params()} B, "
                          f"binding {ctypes.sizeof(AttnParams)} B")
    _lib = lib
    return lib


# fat5_attn_params.variant bits (include/fat5.h `enum fat5_variant`): tests and profilers force / forbid a kernel body per call
V_FWD64_ON, V_FWD64_OFF, V_KV64_ON, V_KV64_OFF, V_Q64_ON, V_Q64_OFF = 1, 2, 4, 8, 16, 32
V_DBIAS_STAGED, V_DBIAS_INKERNEL, V_NO_FUSE, V_NO_SPLIT = 64, 128, 256, 512
V_FWD64_KSPLIT_ON, V_FWD64_KSPLIT_OFF = 1024, 2048
V_KV64_HALF_ON, V_KV64_HALF_OFF = 4096, 8192
V_KV64_MIX_ON, V_KV64_MIX_OFF = 16384, 32768
V_FWD64_MIX_ON, V_FWD64_MIX_OFF = 524288, 1048576
V_FUSED64_ON, V_FUSED64_OFF = 65536, 131072
V_DBIAS_NOSPLIT = 262144
V_QDB64_ON, V_QDB64_OFF = 2097152, 4194304
V_KVRES_ON, V_KVRES_OFF = 134217728, 268435456  # 64-row dQ body, at most 512 keys: the head's K / V resident in LDS (no ring) wherever legal / never
V_QDIAG_ON, V_QDIAG_OFF = 8388608, 16777216  # T5 bias, one-launch backward: the per-diagonal sums of the table gradient in the dQ workgroups always / never
V_DTABLE_RUNS_ON, V_DTABLE_RUNS_OFF = 33554432, 67108864  # T5 table gradient: the per-bucket-run reduction wherever legal (the default) / never
_variant = 0  # what the host mirror writes into every descriptor it builds; 0 = the library's own choice (production)


def set_variant(bits):
    """Test / profiling hook: OR of V_* bits carried by every subsequent attention call of this process (ctypes path and the
    C++ binding alike); returns the previous value.  Production code never calls this."""
    global _variant
    prev, _variant = _variant, int(bits)
    nat = native()
    if nat is not None:
        nat.set_variant(int(bits))
    return prev


class variant:
    """`with _lib.variant(_lib.V_FWD64_ON | _lib.V_KV64_ON): ...`"""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        self.prev = set_variant(self.bits)

    def __exit__(self, *exc):
        set_variant(self.prev)
        return False


_native = False  # (False: not looked up yet; None: unavailable / disabled)


def native():
    """The C++ host path (csrc/torch_binding.cpp -> lib/_fat5_torch.so: at::Tensor in / out, C++ autograd functions on the C ABI),
    or None when it is not built or FAT5_TORCH_BINDING=0 -- the ctypes path below is then used for eager calls as well (same
    kernels, ~10x the host time per call)."""
    global _native
    if _native is False:
        _native = None
        if os.environ.get("FAT5_TORCH_BINDING", "1") != "0" and not _VAR:
            path = os.path.join(_HERE, "lib", "_fat5_torch.so")
            if os.path.exists(path):
                import importlib.util
                load()  # (libfat5.so first: same image for both paths)
                spec = importlib.util.spec_from_file_location("_fat5_torch", path)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                if mod.sizeof_attn_params() != ctypes.sizeof(AttnParams):
                    raise ImportError("lib/_fat5_torch.so was built against another include/fat5.h: rebuild (python flasht5_amd/build.py)")
                _native = mod
    return _native


def check(rc, what):
    if rc != 0:
        msg = load().fat5_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (fat5 status {rc}): {msg}")


def dtype_code(dt):
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f"unsupported dtype {dt}") from None


def stream_ptr(device):
    """raw hipStream_t of torch's current stream on `device` (the C ABI launches there, asynchronously)"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


class on_device:
    """`with on_device(t.device):` -- make the tensor's device current for the C-ABI call (the reference wraps its launches
    the same way, flash_attention_v2_bias.py:61,:128); a no-op, without touching the runtime, when it already is."""
    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index if device.index is not None else -1
        self.prev = -1

    def __enter__(self):
        if self.idx >= 0:
            cur = torch.cuda.current_device()
            if cur != self.idx:
                self.prev = cur
                torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def strides3(t):
    """(b, h, s) element strides of a 4-D (B,H,S,D) tensor as a ctypes array."""
    return c_i64x3(t.stride(0), t.stride(1), t.stride(2))


def kernel_ready(t):
    """The kernels need last-dim stride 1, 16-byte aligned base and strides that are multiples of 8."""
    return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:-1]))


def describe(B, H, M, N, D=64, dtype=FAT5_BF16, causal=False, bias_mode=0, radius=0, need_dbias=False, variant=0, sm_scale=None,
             bucket=None, num_buckets=32, packed=False, total_q=0, total_k=None):
    """Which kernel bodies the library would run for a problem -- {"fwd": "64row-ksplit", "dq": "32row", "dkdv": "64key-mixed:4",
    "fused": "0", "dbias": "direct"} -- from shapes alone (fat5_attn_describe: host-only, works without a GPU).
    packed: a cu_seqlens batch of B sequences, M / N its max_seqlen_q / max_seqlen_k, total_q / total_k its token counts (total_k
    defaults to total_q)."""
    p = AttnParams()
    p.B, p.H, p.M, p.N, p.D = B, H, M, N, D
    p.dtype, p.causal, p.bias_mode, p.rpe_radius, p.variant = dtype, int(causal), bias_mode, radius, variant
    p.sm_scale = float(D) ** -0.5 if sm_scale is None else float(sm_scale)  # (a zero scale keeps the dense bias off the matrix pipe)
    if packed:
        p.cu_seqlens_q = p.cu_seqlens_k = 16  # (never followed: the policy reads only whether they are null)
        p.total_q, p.total_k = int(total_q), int(total_q if total_k is None else total_k)
    if bias_mode == BIAS_DENSE:
        p.bias = 16  # (never followed)
        p.bias_stride[0], p.bias_stride[1], p.bias_stride[2] = 0, M * N, N  # the model's (1, H, M, N) bias, shared by the batch
        if need_dbias:
            p.dbias, p.dbias_batch, p.dbias_heads = 16, 1, H
    elif bias_mode == BIAS_RPE1D:
        p.rpe1d = 16
        if need_dbias and bucket is not None:  # the (num_buckets, H) table gradient; `bucket`: the host bucket map (2R+1 ids)
            host = (ctypes.c_int32 * len(bucket))(*[int(x) for x in bucket])
            p.rpe_bucket, p.drpe_table, p.rpe_num_buckets = 16, 16, int(num_buckets)
            p.rpe_bucket_host = ctypes.addressof(host)
        elif need_dbias:
            p.drpe1d = 16
    buf = ctypes.create_string_buffer(256)
    check(load().fat5_attn_describe(ctypes.byref(p), buf, 256), "fat5_attn_describe")
    d = dict(kv.split("=") for kv in buf.value.decode().split())
    d["kvres"] = str(load().fat5_attn_bwd_kvres(ctypes.byref(p)))  # (fat5_attn_bwd_kvres: not a field of the text)
    return d
