"""flasht5_amd -- MI355X-native (gfx950) FlashAttention-2 with T5 relative-position bias, T5 RMSNorm and
cross-entropy + z-loss, as drop-in replacements of the reference's three operator callables
(modeling_flash_t5.py:15-28):

    from flasht5_amd import flash_attention_v2_bias, fast_rms_layernorm, cross_entropy_loss

Everything runs in hand-written HIP kernels behind the C ABI of `lib/libfat5.so` (include/fat5.h); there is
no CPU / PyTorch fallback -- importing raises if the library has not been built.
"""
from . import _lib

_lib.load()  # fail loudly at import time when the HIP library is missing

from .flash_attention_v2_bias import (flash_attention_v2_bias, FlashAttentionAdditiveBias,  # noqa: E402
                                      flash_attention_v2_rpe, FlashAttentionRPE, flash_attention_v2_rpe1d, FlashAttentionRPE1D,
                                      flash_attn_varlen_fwd, flash_attn_varlen_bwd,
                                      flash_attn_varlen_func, FlashAttentionVarlen)
from .rms_norm import fast_rms_layernorm, Fast_RMS_Layernorm, fused_add_rms_layernorm, FusedAddRMSLayernorm  # noqa: E402
from .cross_entropy_loss import cross_entropy_loss, CrossEntropyLoss  # noqa: E402
from .lm_head_cross_entropy import lm_head_cross_entropy, LMHeadCrossEntropy  # noqa: E402
from .distillation import distillation_loss, lm_head_distillation  # noqa: E402
from .fused_linear import rmsnorm_linear, linear_residual, RMSNormLinear, LinearResidual  # noqa: E402
from .gated_act import gated_act, gated_act_packed  # noqa: E402
from .dropout import dropout, dropout_add, dropout_add_rms_layernorm  # noqa: E402
from .fire import fire_bias, FIRE  # noqa: E402
from .rotary import (apply_rotary_emb, apply_rotary_emb_qkv, apply_rotary_emb_packed, rotary_tables,  # noqa: E402
                     RotaryPositionalEncoding)
from .positional_encoding import (relative_position_bucket, compute_bias, rpe1d_from_table,  # noqa: E402
                                  RelativePositionalEncoding)

from .decode import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk, quantize_kv  # noqa: E402
from .w8 import quantize_weight, w8_linear  # noqa: E402
from .sampling import sample_logits  # noqa: E402
from .logits_process import process_logits, pack_bad_words  # noqa: E402
from .speculative import speculative_accept, speculative_round, draft_tokens  # noqa: E402
from .prompt_lookup import prompt_lookup_draft  # noqa: E402
from .packing import pack_plan, plan_pair, PackPlan  # noqa: E402
from .ul2 import ul2_lengths, ul2_tables, ul2_collate, UL2Collator, UL2Tables  # noqa: E402
from .attention_module import FlashT5Attention  # noqa: E402
from .modules import FlashT5LayerNorm, FlashT5CrossEntropyLoss  # noqa: E402
from .adamw_scaled import AdamWScale  # noqa: E402
from .fat5_step import FAT5Config, FAT5ForConditionalGeneration, allreduce_gradients, train_step, GraphedTrainStep  # noqa: E402
from .distill import DistilledFAT5  # noqa: E402
from .pooling import sequence_pool  # noqa: E402
from .heads import (FAT5EncoderModel, FAT5ForTokenClassification, FAT5ForSequenceClassification,  # noqa: E402
                    FAT5ForQuestionAnswering)

__version__ = "0.1.0"
