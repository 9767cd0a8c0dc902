"""Config 5 of BASELINE.json: a FAT5-base UL2 training step (seq 1024, data parallel) built from the path's three operators.

A minimal encoder-decoder with the reference's structure (src/model/modeling_flash_t5.py: `FlashT5LayerFF` :148-164,
`FlashT5LayerSelfAttention` / `FlashT5LayerCrossAttention` :297-349, `FlashT5Block` :352-392, `FlashT5Stack` :394-464,
`FlashT5ForConditionalGeneration` :604-736) and its parameter names, so a reference checkpoint's state dict loads:

  * RMSNorm        -> `FlashT5LayerNorm`        (fast_rms_layernorm, HIP)
  * attention      -> `FlashT5Attention`        (flash_attention_v2_rpe1d / flash_attention_v2_bias, HIP); the T5 relative-position
                      bias is produced by block 0 of each stack and handed to the following blocks (:403-405, :452-455);
                      cross-attention has no bias (`bias=None`, :207,:324)
  * loss           -> `FlashT5CrossEntropyLoss` (cross_entropy_loss with z-loss and label smoothing, HIP)
  * everything else is plain torch-ROCm: `nn.Linear` (hipBLASLt), `nn.Embedding`, tanh-GELU gating, residual adds.

Generation: `generate` (greedy -- the reference's algorithm and return value --, sampled, or beam search) and `decode_step` run one new token per step through
the decoder against per-layer KV caches (flasht5_amd/generation.py, the split-KV decode kernel), optionally replayed from a HIP graph.

Dropout (`dropout_rate`, 0 in every reference pre-training config, 0.1 in fine-tuning recipes) is applied at the reference's six
kinds of places with Philox masks recomputed inside HIP kernels (flasht5_amd/dropout.py): nothing is stored, and a
captured `GraphedTrainStep` draws new masks at every replay because the step counter lives in device memory.

This is the step DRIVER of the hot path, not a model zoo: no HF plumbing or checkpoint conversion (the encoder-only models and
their fine-tuning heads are built on `FAT5Stack` in heads.py).  Data parallelism = one process per GPU; `allreduce_gradients` is the step's one
exchange (RCCL over xGMI): a single flat fp32 all-reduce that carries the two `(32, H)` relative-position tables first.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.distributed as dist
from torch import nn

from .attention_module import FlashT5Attention
from .modules import FlashT5LayerNorm, FlashT5CrossEntropyLoss


@dataclass
class FAT5Config:
    """model_args of configs/flan/fat5-flan-base.yaml (vocabulary: the 32768-entry tokenizer of examples/minipile)"""
    vocab_size: int = 32768
    d_model: int = 768
    d_kv: int = 64
    d_ff: int = 2048
    num_heads: int = 12
    num_layers: int = 12
    num_decoder_layers: int = 12
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    max_sequence_length: int = 1024
    layer_norm_epsilon: float = 1e-6
    z_loss: float = 1e-4
    label_smoothing: float = 0.1
    attention_scale: float = 1.0
    attention_type: str = "fat5_rpe"      # "fat5_rpe": O(S) bias memory; "triton": the reference's dense-bias operator
    position_encoding_type: str = "t5"      # "t5", "RoPE" (rotary, in every attention layer; no bias) or "FIRE" (needs "triton")
    fire_mlp_width: int = 32               # FIRE: width of the bias MLP
    rotary_emb_fraction: float = 1.0       # RoPE: rotated share of d_kv
    rotary_base: float = 10000.0
    rotary_interleaved: bool = False
    rotary_scale_base: Optional[float] = None  # xPos when set
    use_glu_mlp: bool = True
    use_gelu_act: bool = True
    decoder_start_token_id: int = 0
    pad_token_id: int = 0
    crossentropy_inplace_backward: bool = True
    fuse_lm_head_ce: bool = False          # lm_head + loss in row chunks: the (B*T, vocab) logits are never materialised
    fuse_add_norm: bool = False            # every residual add runs inside the next pre-norm (fused_add_rms_layernorm): same bits, fewer passes
    fuse_norm_linear: bool = False         # stacked projections (q | k | v, wi_0 | wi_1: one library GEMM each, packed gradients), the residual add in the
                                           # output projection's GEMM epilogue, fused backward passes around them (fused_linear.py)
    fuse_gated_act: bool = True            # act(wi_0 x) * wi_1 x in one kernel forward, one backward (gated_act.py / fat5_gated_act_*)
    dropout_rate: float = 0.0              # the reference's six dropout sites (modeling_flash_t5.py :124/:143, :163, :316, :342, :440, :460), training only
    dropout_seed: Optional[int] = None     # the Philox key of the masks; None: drawn from torch's default CPU generator when the model is built
    is_decoder: bool = False
    num_labels: int = 2                    # the encoder-only heads (heads.py): classes of the classifiers; the QA head needs 2
    classifier_dropout: float = 0.0        # the heads' own dropout sites (training only)
    eos_token_id: int = 1                  # FAT5ForSequenceClassification pools the row of the last <eos>

    def __post_init__(self):
        if self.position_encoding_type == "FIRE" and self.attention_type == "fat5_rpe":
            raise ValueError("position_encoding_type='FIRE' needs attention_type='triton' (dense bias): FIRE's bias is not "
                             "Toeplitz once a row passes the threshold T, so fat5_rpe cannot carry it")
        if not 0.0 <= float(self.dropout_rate) < 1.0:
            raise ValueError(f"dropout_rate = {self.dropout_rate} outside [0, 1)")
        if not 0.0 <= float(self.classifier_dropout) < 1.0:
            raise ValueError(f"classifier_dropout = {self.classifier_dropout} outside [0, 1)")
        if int(self.num_labels) < 1:
            raise ValueError(f"num_labels = {self.num_labels} must be at least 1")
        if self.dropout_rate > 0 and self.fuse_norm_linear:
            raise ValueError("dropout_rate > 0 with fuse_norm_linear: that path's residual add is a GEMM epilogue, which cannot carry "
                             "a dropout mask (use fuse_add_norm, whose pre-norm kernel applies it, or the plain path)")


class FAT5GatedAct(nn.Module):  # reference FlashT5DenseGatedAct / FlashT5DenseAct (:114-146)
    def __init__(self, c):
        super().__init__()
        self.glu = c.use_glu_mlp
        if self.glu:
            self.wi_0 = nn.Linear(c.d_model, c.d_ff, bias=False)
            self.wi_1 = nn.Linear(c.d_model, c.d_ff, bias=False)
        else:
            self.wi = nn.Linear(c.d_model, c.d_ff, bias=False)
        self.act = nn.GELU(approximate="tanh") if c.use_gelu_act else nn.ReLU()
        self.act_name = "gelu_tanh" if c.use_gelu_act else "relu"
        self.fuse = bool(getattr(c, "fuse_gated_act", True))

    def fused_ok(self, x):
        return self.fuse and x.is_cuda and x.dtype in (torch.float32, torch.float16, torch.bfloat16)

    def forward(self, x):
        if self.glu:
            if self.fused_ok(x) and self.wi_0.weight.shape[0] % 8 == 0:
                from .gated_act import gated_act
                return gated_act(self.wi_0(x), self.wi_1(x), self.act_name)
            return self.act(self.wi_0(x)) * self.wi_1(x)
        return self.act(self.wi(x))


def _self_kw(packing):
    """the packed-row keyword arguments of a self-attention layer (none without a packing.Packed: today's call)"""
    return {} if packing is None else dict(cu_seqlens=packing.cu_seqlens, max_seqlen=packing.max_seqlen)


def _cross_kw(packing):
    if packing is None:
        return {}
    return dict(cu_seqlens=packing.cu_seqlens, max_seqlen=packing.max_seqlen, kv_cu_seqlens=packing.kv_cu_seqlens,
                kv_max_seqlen=packing.kv_max_seqlen)


class _Drop:
    """what the dropout sites of ONE training forward share: the rate, this rank's Philox key and the forward's own copy of the step
    counter (an int64 device tensor the kernels read, forward and backward)"""
    __slots__ = ("p", "key", "step")

    def __init__(self, p, key, step):
        self.p, self.key, self.step = p, key, step

    def __call__(self, x, site):
        from .dropout import dropout
        return dropout(x, self.p, self.key, self.step, site)

    def add(self, h, delta, site):
        """h + dropout(delta): the residual add of a sub-layer whose output is dropped out at `site`"""
        from .dropout import dropout_add
        return dropout_add(delta, h, self.p, self.key, self.step, site)


def _pre_norm(ln, h, pending, drop=None, pending_site=0):
    """pre-norm of a sub-layer with the previous sub-layer's residual add folded in: (h + pending, layer_norm(h + pending));
    with `drop` the pending output is dropped out (at the site of the sub-layer that produced it) inside the same kernel"""
    if pending is None:
        return h, ln(h)
    if drop is not None:
        from .dropout import dropout_add_rms_layernorm
        return dropout_add_rms_layernorm(h, pending, ln.weight, ln.variance_epsilon, drop.p, drop.key, drop.step, pending_site)
    from .rms_norm import fused_add_rms_layernorm
    return fused_add_rms_layernorm(h, pending, ln.weight, ln.variance_epsilon)


class FAT5LayerFF(nn.Module):  # :148-164
    def __init__(self, c):
        super().__init__()
        self.act = FAT5GatedAct(c)
        self.layer_norm = FlashT5LayerNorm(c.d_model, eps=c.layer_norm_epsilon)
        self.wo = nn.Linear(c.d_ff, c.d_model, bias=False)

    site_act = site = 0  # dropout sites: after the activation (in front of wo) and on the sub-layer's output (FAT5Stack numbers them)

    def forward(self, h, drop=None):
        if drop is not None:
            return drop.add(h, self.wo(drop(self.act(self.layer_norm(h)), self.site_act)), self.site)
        return h + self.wo(self.act(self.layer_norm(h)))

    def forward_fused(self, h):
        """the same sub-layer with the norm inside the wi GEMM and the residual add as wo's epilogue"""
        from .fused_linear import rmsnorm_linear, linear_residual
        a = self.act
        if a.glu:
            g, h = rmsnorm_linear(h, self.layer_norm.weight, (a.wi_0.weight, a.wi_1.weight), self.layer_norm.variance_epsilon, return_residual=True)
            if a.fused_ok(g) and a.wi_0.weight.shape[0] % 8 == 0:
                from .gated_act import gated_act_packed
                t = gated_act_packed(g, a.act_name)  # (its gradient is ONE (…, 2 d_ff) tensor: no concatenation in front of the backward GEMMs)
            else:
                g0, g1 = g.split(a.wi_0.weight.shape[0], dim=-1)
                t = a.act(g0) * g1
        else:
            t, h = rmsnorm_linear(h, self.layer_norm.weight, a.wi.weight, self.layer_norm.variance_epsilon, return_residual=True)
            t = a.act(t)
        return linear_residual(t, self.wo.weight, h)

    def forward_deferred(self, h, pending, drop=None, pending_site=0):
        """(h, delta): the residual stream after the pending add, and this sub-layer's output whose add is left to the next pre-norm"""
        h, n = _pre_norm(self.layer_norm, h, pending, drop, pending_site)
        t = self.act(n)
        return h, self.wo(t if drop is None else drop(t, self.site_act))


class FAT5LayerSelfAttention(nn.Module):  # :297-318
    def __init__(self, c, has_positional_encoding):
        super().__init__()
        self.self_attention = FlashT5Attention(c, has_positional_encoding=has_positional_encoding, is_causal=c.is_decoder)
        self.layer_norm = FlashT5LayerNorm(c.d_model, eps=c.layer_norm_epsilon)

    site = 0  # dropout site of the sub-layer's output

    def forward(self, h, position_bias=None, packing=None, drop=None):
        a, position_bias = self.self_attention(self.layer_norm(h), position_bias=position_bias, **_self_kw(packing))
        return (h + a if drop is None else drop.add(h, a, self.site)), position_bias

    def forward_fused(self, h, position_bias=None, packing=None):
        return self.self_attention.forward_fused(h, self.layer_norm.weight, self.layer_norm.variance_epsilon, position_bias=position_bias,
                                                 **_self_kw(packing))

    def forward_deferred(self, h, pending, position_bias=None, packing=None, drop=None, pending_site=0):
        h, n = _pre_norm(self.layer_norm, h, pending, drop, pending_site)
        a, position_bias = self.self_attention(n, position_bias=position_bias, **_self_kw(packing))
        return h, a, position_bias


class FAT5LayerCrossAttention(nn.Module):  # :321-349
    def __init__(self, c):
        super().__init__()
        self.cross_attention = FlashT5Attention(c, has_positional_encoding=False)
        self.layer_norm = FlashT5LayerNorm(c.d_model, eps=c.layer_norm_epsilon)

    site = 0  # dropout site of the sub-layer's output

    def forward(self, h, key_value_states, packing=None, drop=None):
        a, _ = self.cross_attention(self.layer_norm(h), key_value_states=key_value_states, **_cross_kw(packing))
        return h + a if drop is None else drop.add(h, a, self.site)

    def forward_fused(self, h, key_value_states, packing=None):
        return self.cross_attention.forward_fused(h, self.layer_norm.weight, self.layer_norm.variance_epsilon, key_value_states=key_value_states,
                                                  **_cross_kw(packing))[0]

    def forward_deferred(self, h, pending, key_value_states, packing=None, drop=None, pending_site=0):
        h, n = _pre_norm(self.layer_norm, h, pending, drop, pending_site)
        a, _ = self.cross_attention(n, key_value_states=key_value_states, **_cross_kw(packing))
        return h, a


class FAT5Block(nn.Module):  # :352-392
    def __init__(self, c, has_positional_encoding):
        super().__init__()
        self.is_decoder = c.is_decoder
        self.self_attention_layer = FAT5LayerSelfAttention(c, has_positional_encoding)
        if self.is_decoder:
            self.cross_attention_layer = FAT5LayerCrossAttention(c)
        self.ff_layer = FAT5LayerFF(c)

    def assign_sites(self, site):
        """number this block's dropout sites in forward order from `site`; returns the next free number"""
        self.self_attention_layer.site = site
        site += 1
        if self.is_decoder:
            self.cross_attention_layer.site = site
            site += 1
        self.ff_layer.site_act, self.ff_layer.site = site, site + 1
        return site + 2

    def forward(self, h, position_bias=None, encoder_hidden_states=None, packing=None, drop=None):
        h, position_bias = self.self_attention_layer(h, position_bias, packing, drop)
        if self.is_decoder and encoder_hidden_states is not None:
            h = self.cross_attention_layer(h, encoder_hidden_states, packing, drop)
        return self.ff_layer(h, drop), position_bias

    def forward_fused(self, h, position_bias=None, encoder_hidden_states=None, packing=None):
        h, position_bias = self.self_attention_layer.forward_fused(h, position_bias, packing)
        if self.is_decoder and encoder_hidden_states is not None:
            h = self.cross_attention_layer.forward_fused(h, encoder_hidden_states, packing)
        return self.ff_layer.forward_fused(h), position_bias

    def forward_deferred(self, h, pending, position_bias=None, encoder_hidden_states=None, packing=None, drop=None, pending_site=0):
        """pending_site: the dropout site of the sub-layer that produced `pending` (the previous block's feed-forward)"""
        h, pending, position_bias = self.self_attention_layer.forward_deferred(h, pending, position_bias, packing, drop, pending_site)
        pending_site = self.self_attention_layer.site
        if self.is_decoder and encoder_hidden_states is not None:
            h, pending = self.cross_attention_layer.forward_deferred(h, pending, encoder_hidden_states, packing, drop, pending_site)
            pending_site = self.cross_attention_layer.site
        h, pending = self.ff_layer.forward_deferred(h, pending, drop, pending_site)
        return h, pending, position_bias


class FAT5Stack(nn.Module):  # :394-464
    def __init__(self, c, embed_tokens, n_layers, first_site=0):
        super().__init__()
        self.embed_tokens = embed_tokens
        self.block = nn.ModuleList([FAT5Block(c, has_positional_encoding=(i == 0)) for i in range(n_layers)])
        self.final_layer_norm = FlashT5LayerNorm(c.d_model, eps=c.layer_norm_epsilon)
        self.fuse_add_norm = c.fuse_add_norm
        self.fuse_norm_linear = c.fuse_norm_linear
        # dropout sites in forward order: the embeddings, every block's sub-layers, the final norm's output
        self.site_embed = first_site
        site = first_site + 1
        for blk in self.block:
            site = blk.assign_sites(site)
        self.site_final = site
        self.next_site = site + 1

    def forward(self, input_ids, encoder_hidden_states=None, packing=None, drop=None):
        """packing (packing.Packed): input_ids are the (1, total) valid tokens of a padded or packed batch, every attention layer
        runs over cu_seqlens, and the output stays (1, total, d_model).  drop (_Drop): a training forward with dropout; None (what
        every caller but the training loss passes) runs the code below as it always ran"""
        h = self.embed_tokens(input_ids)
        if torch.is_autocast_enabled() and h.is_cuda:  # :424-425
            h = h.to(torch.get_autocast_gpu_dtype())
        position_bias = None  # produced by block 0, shared by the others (:452-455)
        if drop is not None:
            h = drop(h, self.site_embed)  # :440
            if self.fuse_add_norm:
                pending, pending_site = None, 0
                for blk in self.block:
                    h, pending, position_bias = blk.forward_deferred(h, pending, position_bias, encoder_hidden_states, packing, drop, pending_site)
                    pending_site = blk.ff_layer.site
                h = _pre_norm(self.final_layer_norm, h, pending, drop, pending_site)[1]
            else:
                for blk in self.block:
                    h, position_bias = blk(h, position_bias, encoder_hidden_states, packing, drop)
                h = self.final_layer_norm(h)
            return drop(h, self.site_final)  # :460
        if self.fuse_norm_linear and h.dtype in (torch.float16, torch.bfloat16):
            for blk in self.block:
                h, position_bias = blk.forward_fused(h, position_bias, encoder_hidden_states, packing)
            return self.final_layer_norm(h)
        if self.fuse_add_norm:
            pending = None  # the last sub-layer's output: its residual add happens inside the next pre-norm
            for blk in self.block:
                h, pending, position_bias = blk.forward_deferred(h, pending, position_bias, encoder_hidden_states, packing)
            return _pre_norm(self.final_layer_norm, h, pending)[1]
        for blk in self.block:
            h, position_bias = blk(h, position_bias, encoder_hidden_states, packing)
        return self.final_layer_norm(h)


@torch.no_grad()
def init_stack_weights(root, c):
    """the reference's `_init_weights` (:482-517, Mesh-TF style, factor 1.0) for every norm, feed-forward and attention module under
    `root`, in module order (the random draws of a model are taken in that order)"""
    for m in root.modules():
        if isinstance(m, FlashT5LayerNorm):
            m.weight.fill_(1.0)
        elif isinstance(m, FAT5GatedAct):
            for w in ((m.wi_0, m.wi_1) if m.glu else (m.wi,)):
                w.weight.normal_(0.0, c.d_model ** -0.5)
        elif isinstance(m, FAT5LayerFF):
            m.wo.weight.normal_(0.0, c.d_ff ** -0.5)
        elif isinstance(m, FlashT5Attention):
            m.Wq.weight.normal_(0.0, (c.d_model * c.d_kv) ** -0.5)
            m.Wk.weight.normal_(0.0, c.d_model ** -0.5)
            m.Wv.weight.normal_(0.0, c.d_model ** -0.5)
            m.o.weight.normal_(0.0, (c.num_heads * c.d_kv) ** -0.5)
            # (RoPE has no table; FIRE keeps its own initialisation, which the reference's _init_weights does not touch)
            if m.pe_encoding is not None and hasattr(m.pe_encoding, "relative_attention_bias"):
                m.pe_encoding.relative_attention_bias.weight.normal_(0.0, c.d_model ** -0.5)


class FAT5ForConditionalGeneration(nn.Module):  # :604-736 (training forward; cached greedy / sampled generation in generation.py)
    def __init__(self, config: FAT5Config):
        super().__init__()
        import copy
        self.config = config
        self.shared = nn.Embedding(config.vocab_size, config.d_model)
        enc = copy.copy(config)
        enc.is_decoder = False
        dec = copy.copy(config)
        dec.is_decoder = True
        self.encoder = FAT5Stack(enc, self.shared, config.num_layers)
        self.decoder = FAT5Stack(dec, self.shared, config.num_decoder_layers, first_site=self.encoder.next_site)
        self.lm_head = nn.Linear(config.d_model, config.vocab_size, bias=False)
        self.loss_fct = FlashT5CrossEntropyLoss(z_loss_factor=config.z_loss, label_smoothing=config.label_smoothing,
                                                inplace_backward=config.crossentropy_inplace_backward)
        self.reset_parameters()
        # dropout: the step counter is a buffer outside the state dict (reference checkpoints load strictly); a
        # dropout_rate of 0 builds nothing and draws nothing
        self.dropout_seed = config.dropout_seed
        if config.dropout_rate > 0:
            if self.dropout_seed is None:
                self.dropout_seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64))
            self.register_buffer("dropout_step", torch.zeros(1, dtype=torch.int64), persistent=False)

    def _drop(self):
        """the dropout context of this forward, or None (eval, or dropout_rate 0: no new launch, today's code path).  The sites of
        the forward and of its backward read a COPY of the step counter; the counter itself is advanced on the device right away,
        so a captured step holds both and every replay draws new masks."""
        c = self.config
        if not (self.training and c.dropout_rate > 0):
            return None
        from .dropout import rank_key
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        step = self.dropout_step.clone()
        self.dropout_step.add_(1)
        return _Drop(float(c.dropout_rate), rank_key(self.dropout_seed, rank), step)

    @torch.no_grad()
    def reset_parameters(self):
        """the reference's `_init_weights` (:482-517): Mesh-TF style, factor 1.0"""
        c = self.config
        self.shared.weight.normal_(0.0, 1.0)
        self.lm_head.weight.normal_(0.0, c.d_model ** -0.5)
        init_stack_weights(self, c)

    def _shift_right(self, labels):  # HF T5 convention used by the reference (:713-714)
        c = self.config
        shifted = labels.new_zeros(labels.shape)
        shifted[..., 1:] = labels[..., :-1]
        shifted[..., 0] = c.decoder_start_token_id
        return shifted.masked_fill(shifted == -100, c.pad_token_id)

    def rpe_tables(self):
        """the two (num_buckets, H) relative-position tables (encoder, decoder): the bias gradients of the step; none with RoPE or
        FIRE (FIRE's parameters are ordinary parameters of block 0's self-attention)"""
        if self.config.position_encoding_type != "t5":
            return []
        return [self.encoder.block[0].self_attention_layer.self_attention.pe_encoding.relative_attention_bias.weight,
                self.decoder.block[0].self_attention_layer.self_attention.pe_encoding.relative_attention_bias.weight]

    def forward(self, input_ids, labels, attention_mask=None, decoder_attention_mask=None, segment_ids=None, decoder_segment_ids=None):
        """the training loss.  attention_mask / decoder_attention_mask: (B, L) bool or integer, non-zero = valid, right-padded;
        segment_ids / decoder_segment_ids: (B, L) integer, several examples per row (0 = padding, then runs of 1, 2, ...; a row
        holds as many decoder as encoder segments).  With any of them the model runs over the valid tokens only:
        attention stays inside each example with positions of its own, and the mean runs over the non-ignored labels of valid
        positions.  Without a decoder-side argument, row b's decoder length is max(1, 1 + the last index with labels != -100)."""
        return self._loss(*self._decoder_states(self._plan(input_ids, labels, attention_mask, decoder_attention_mask, segment_ids,
                                                           decoder_segment_ids), input_ids, labels))

    def _plan(self, input_ids, labels, attention_mask=None, decoder_attention_mask=None, segment_ids=None, decoder_segment_ids=None):
        """`_pack`'s plan for a batch with padding masks or segment ids; None without them, or when they describe a batch in which
        nothing is padded and no row holds two examples (the dense path, bit for bit)"""
        if attention_mask is None and decoder_attention_mask is None and segment_ids is None and decoder_segment_ids is None:
            return None
        return self._pack(input_ids, labels, attention_mask, decoder_attention_mask, segment_ids, decoder_segment_ids)

    def _decoder_states(self, packed, input_ids, labels):
        """the forward up to the lm_head -> (decoder hidden states, the labels the loss sees): over the valid tokens of `packed`
        (a `_plan` result; any model with this vocabulary can run over another's plan), or over the whole batch when it is None"""
        if packed is not None:
            return self._packed_states(*packed)
        drop = self._drop()
        enc = self.encoder(input_ids, drop=drop)
        dec = self.decoder(self._shift_right(labels), encoder_hidden_states=enc, drop=drop)
        return dec, labels

    def _loss(self, dec, labels):
        if self.config.fuse_lm_head_ce:
            from .lm_head_cross_entropy import lm_head_cross_entropy
            c = self.config
            return lm_head_cross_entropy(dec, self.lm_head.weight, labels, label_smoothing=c.label_smoothing,
                                         lse_square_scale=c.z_loss, reduction="mean")[0]
        return self.loss_fct(self.lm_head(dec), labels)

    def packed_supported(self):
        """raise NotImplementedError when this model cannot train on padded / packed batches (FlashT5Attention.packed_supported)"""
        for stack in (self.encoder, self.decoder):
            stack.block[0].self_attention_layer.self_attention.packed_supported()

    def _pack(self, input_ids, labels, attention_mask, decoder_attention_mask, segment_ids, decoder_segment_ids):
        """check the padding / segment arguments on the host, plan both sides on the device (packing.plan_pair: ONE host read) ->
        (encoder PackPlan, decoder PackPlan, input_ids, labels), or None when the batch is neither padded nor packed"""
        from .packing import plan_pair
        for side, mask, seg in (("encoder", attention_mask, segment_ids), ("decoder", decoder_attention_mask, decoder_segment_ids)):
            if mask is not None and seg is not None:
                raise ValueError(f"forward: a padding mask and segment ids for the {side} side: segment ids already say what is "
                                 "padding (0), pass one of them")
        if segment_ids is not None and decoder_segment_ids is None:
            raise ValueError("forward: segment_ids needs decoder_segment_ids (example i of a row's input belongs to example i of its "
                             "labels, which the labels alone do not delimit)")
        for name, t, like in (("attention_mask", attention_mask, input_ids), ("segment_ids", segment_ids, input_ids),
                              ("decoder_attention_mask", decoder_attention_mask, labels),
                              ("decoder_segment_ids", decoder_segment_ids, labels)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dim() != 2 or tuple(t.shape) != tuple(like.shape):
                raise ValueError(f"forward: {name} must be a (B, L) = {tuple(like.shape)} tensor like the ids it describes, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype.is_floating_point or t.dtype.is_complex or (name.endswith("segment_ids") and t.dtype == torch.bool):
                raise ValueError(f"forward: {name} must be {'an integer' if name.endswith('segment_ids') else 'a bool or integer'} "
                                 f"tensor, got {t.dtype}")
        if input_ids.dim() != 2 or labels.dim() != 2 or input_ids.shape[0] != labels.shape[0]:
            raise ValueError(f"forward: input_ids (B, L_enc) and labels (B, L_dec), got {tuple(input_ids.shape)} / {tuple(labels.shape)}")
        self.packed_supported()
        dev = input_ids.device
        if segment_ids is not None:
            enc_in = segment_ids.to(dev)
        elif attention_mask is not None:
            enc_in = attention_mask.to(dev) != 0
        else:
            enc_in = torch.ones(input_ids.shape, dtype=torch.bool, device=dev)
        if decoder_segment_ids is not None:
            dec_in = decoder_segment_ids.to(dev)
        elif decoder_attention_mask is not None:
            dec_in = decoder_attention_mask.to(dev) != 0
        else:   # the labels delimit the row: everything up to the last label that is not ignored
            cols = torch.arange(1, labels.shape[1] + 1, device=dev)
            lens = ((labels != -100) * cols).amax(1, keepdim=True).clamp_(min=1)
            dec_in = cols.unsqueeze(0) <= lens
        ep, dp = plan_pair(enc_in, dec_in, names=("attention_mask / segment_ids", "decoder_attention_mask / decoder_segment_ids"))
        B = input_ids.shape[0]
        if ep.nseq == B and dp.nseq == B and ep.total == input_ids.numel() and dp.total == labels.numel():
            return None
        return ep, dp, input_ids, labels

    def _forward_packed(self, ep, dp, input_ids, labels):
        """the loss over the valid tokens only: the loss on the packed rows of `_packed_states`"""
        return self._loss(*self._packed_states(ep, dp, input_ids, labels))

    def _packed_states(self, ep, dp, input_ids, labels):
        """ids and labels gathered through the plans' indices, both stacks over cu_seqlens, the encoder output left packed for
        the cross-attention -> (decoder hidden states (1, total_dec, d_model), labels (1, total_dec))"""
        from .packing import Packed
        c = self.config
        ids = input_ids.reshape(-1).index_select(0, ep.index).unsqueeze(0)      # (1, total_enc)
        lab = labels.reshape(-1).index_select(0, dp.index)                      # (total_dec,)
        # _shift_right per segment: a segment's first position gets the start token, the others the label before them
        shifted = torch.cat([lab.new_full((1,), c.decoder_start_token_id), lab[:-1]])
        shifted.index_fill_(0, dp.cu_seqlens[:-1].long(), c.decoder_start_token_id)
        shifted = shifted.masked_fill(shifted == -100, c.pad_token_id).unsqueeze(0)
        drop = self._drop()   # (the masks index the packed (total, d_model) rows)
        enc = self.encoder(ids, packing=Packed(ep.cu_seqlens, ep.max_seqlen), drop=drop)
        dec = self.decoder(shifted, encoder_hidden_states=enc,
                           packing=Packed(dp.cu_seqlens, dp.max_seqlen, ep.cu_seqlens, ep.max_seqlen), drop=drop)
        return dec, lab.unsqueeze(0)

    def init_decode_state(self, input_ids, max_length=32, attention_mask=None, prompt_length=1, kv_cache_dtype=None, weight_dtype=None):
        """encoder output, cross K / V and empty self-attention caches of capacity max_length + prompt_length (generation.DecodeState);
        kv_cache_dtype="fp8": the caches as e4m3fn bytes plus one fp32 scale per row and head; weight_dtype="fp8": the state's steps
        read the FP8 decoder weights of `quantize_decoder_weights`"""
        from .generation import init_decode_state
        return init_decode_state(self, input_ids, max_length, attention_mask, prompt_length=prompt_length, kv_cache_dtype=kv_cache_dtype,
                                 weight_dtype=weight_dtype)

    def quantize_decoder_weights(self):
        """the FP8 (e4m3fn bytes + one fp32 scale per output row) copies of the decoder weights a cached step reads, built once and
        kept on the model; rebuilt when a source weight changed (w8.quantize_decoder_weights)"""
        from .w8 import quantize_decoder_weights
        return quantize_decoder_weights(self)

    def decode_chunk(self, state, token_ids, logits="all", chunk_seqlens=None):
        """M tokens per row (B, M) through the cached decoder in one step -> logits (B, M, vocab) ("all"), (B, vocab) ("last") or
        None ("none"); the caches and cache_seqlens advance by M, or per row by chunk_seqlens (generation.decode_chunk)"""
        from .generation import decode_chunk
        return decode_chunk(self, state, token_ids, logits, chunk_seqlens)

    def decode_step(self, state, token_ids):
        """one token per row through the cached decoder -> logits (B, vocab) of the next position (generation.decode_step)"""
        from .generation import decode_step
        return decode_step(self, state, token_ids)

    def generate(self, input_ids, attention_mask=None, max_length=32, graph=False, *, do_sample=False, temperature=1.0, top_k=50,
                 top_p=1.0, seed=None, num_beams=1, num_return_sequences=1, length_penalty=1.0, early_stopping=False,
                 return_scores=False, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None,
                 decoder_input_ids=None, assistant_model=None, num_assistant_tokens=4, return_stats=False,
                 decoder_attention_mask=None, kv_cache_dtype=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=2,
                 encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
                 forced_bos_token_id=None, forced_eos_token_id=None, weight_dtype=None):
        """greedy (or, with do_sample=True, temperature / top-k / top-p sampled) decoding with a KV cache; returns what the
        reference's generate returns; num_beams > 1: HF's beam search; repetition_penalty / no_repeat_ngram_size / min_length /
        suppress_tokens / encoder_repetition_penalty / encoder_no_repeat_ngram_size / bad_words_ids / min_new_tokens /
        forced_bos_token_id / forced_eos_token_id: HF's logits processors in one HIP launch per step; decoder_input_ids (B, P): a decoder prompt, prefilled
        in one chunk step; assistant_model: speculative greedy decoding, num_assistant_tokens drafted per round and verified in one
        chunk step; attention_mask / decoder_attention_mask: right-padded inputs and ragged decoder prompts; kv_cache_dtype="fp8": the K / V
        caches as e4m3fn bytes plus per-row scales, in every mode; prompt_lookup_num_tokens / max_matching_ngram_size: speculative greedy
        decoding drafted by an n-gram search of the input and the output so far, one launch per round; weight_dtype="fp8": the decoder
        weights of a step as e4m3fn bytes plus per-row scales, every projection one fused HIP launch (generation.generate)"""
        from .generation import generate
        return generate(self, input_ids, attention_mask, max_length, graph, do_sample=do_sample, temperature=temperature,
                        top_k=top_k, top_p=top_p, seed=seed, num_beams=num_beams, num_return_sequences=num_return_sequences,
                        length_penalty=length_penalty, early_stopping=early_stopping, return_scores=return_scores,
                        repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                        suppress_tokens=suppress_tokens, decoder_input_ids=decoder_input_ids, assistant_model=assistant_model,
                        num_assistant_tokens=num_assistant_tokens, return_stats=return_stats,
                        decoder_attention_mask=decoder_attention_mask, kv_cache_dtype=kv_cache_dtype,
                        prompt_lookup_num_tokens=prompt_lookup_num_tokens, max_matching_ngram_size=max_matching_ngram_size,
                        encoder_repetition_penalty=encoder_repetition_penalty,
                        encoder_no_repeat_ngram_size=encoder_no_repeat_ngram_size, bad_words_ids=bad_words_ids,
                        min_new_tokens=min_new_tokens, forced_bos_token_id=forced_bos_token_id,
                        forced_eos_token_id=forced_eos_token_id, weight_dtype=weight_dtype)


def allreduce_gradients(model: nn.Module, group=None, average=True):
    """The data-parallel exchange of one step: ONE flat fp32 all-reduce (SUM, then 1/world) of every parameter gradient,
    the `(32, H)` bias tables at the front of the buffer (what DDP's first bucket carries in the reference's runs,
    SURVEY 2 #14a).  In place; returns the flat reduced buffer (tests look at its head)."""
    params = [p for p in model.parameters() if p.grad is not None]
    if hasattr(model, "rpe_tables"):
        head = [p for p in model.rpe_tables() if p.grad is not None]
        ids = {id(p) for p in head}
        params = head + [p for p in params if id(p) not in ids]
    if not params:
        return None
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return None  # one rank: nothing to exchange (and no 1 GB flat copy of a FAT5-base gradient set)
    flat = torch.cat([p.grad.detach().reshape(-1).float() for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    if average:
        flat /= dist.get_world_size(group)
    off = 0
    for p in params:
        n = p.numel()
        p.grad.copy_(flat[off:off + n].view_as(p.grad))
        off += n
    return flat


def train_step(model, input_ids, labels, optimizer=None, group=None, max_grad_norm=1.0, attention_mask=None,
               decoder_attention_mask=None, segment_ids=None, decoder_segment_ids=None):
    """forward + backward (+ gradient all-reduce, clip like the reference's `max_grad_norm: 1.0`, optimizer step); the padding masks
    / segment ids of `FAT5ForConditionalGeneration.forward` are handed on (none given: the call of before, whatever `model` is)"""
    pad = dict(attention_mask=attention_mask, decoder_attention_mask=decoder_attention_mask, segment_ids=segment_ids,
               decoder_segment_ids=decoder_segment_ids)
    pad = {k: v for k, v in pad.items() if v is not None}
    loss = model(input_ids, labels, **pad)
    loss.backward()
    allreduce_gradients(model, group)
    if optimizer is not None:
        if max_grad_norm and getattr(optimizer, "max_grad_norm", None) is None:  # (AdamWScale(max_grad_norm=...) clips inside its step)
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    return loss.detach()



class GraphedTrainStep:
    """`train_step` captured ONCE in HIP graphs and replayed per batch: forward, backward, global-norm clipping and the fused
    AdamWScale step of a fixed-shape batch are ~3,400 kernel launches whose enqueue time (24-29 ms of Python, dispatcher and
    hipLaunchKernel for FAT5-base at B = 4) exceeds their 17 ms of kernel time; a replay enqueues them in well under a millisecond.

        step = GraphedTrainStep(model, AdamWScale(model.parameters(), ..., max_grad_norm=1.0))
        for input_ids, labels in loader:       # every batch of ONE shape
            loss = step(input_ids, labels)     # (a static tensor, overwritten by the next call: .item() / .clone() to keep it)

    The first `warmup` calls run the eager `train_step` (they also create the optimizer state), the next call captures and replays, every later call only replays.  What changes from step to step reaches the graph
    through device memory: the batch (copied into static buffers), and the optimizer's step-dependent scalars (learning rate,
    bias correction: `AdamWScale.graph_advance`, so LR schedulers keep working -- they set `param_group["lr"]` as always).
    Gradients stay allocated between steps (the graph owns them): `p.grad` holds the last step's unclipped gradients.

    Data parallel (`group` with more than one rank; `split=True` forces this form): two graphs -- forward + backward, then the
    optimizer step -- with the flat gradient all-reduce (RCCL, `allreduce_gradients`) between them, outside any graph.

    What a captured step fixes (checked before every replay where it can be): `betas` and `eps` of every parameter group are launch
    arguments of the captured kernels -- changing them afterwards raises; the gradient tensors belong to the graph -- a
    `zero_grad(set_to_none=True)` / re-assignment of `p.grad` between replays raises (the graph would keep writing the old buffers
    while `allreduce_gradients` skipped the parameter); clipping happens only if the optimizer was built with `max_grad_norm`
    (the eager warm-up steps behave the same: `train_step(..., max_grad_norm=None)`); one captured step per optimizer
    (`close()` -- also run when this object is destroyed -- releases it: `AdamWScale.release_captured_step()`)."""

    def __init__(self, model, optimizer, group=None, warmup=2, split=None):
        from .adamw_scaled import AdamWScale
        if not isinstance(optimizer, AdamWScale):
            raise TypeError("GraphedTrainStep needs flasht5_amd.AdamWScale (its captured step reads lr / bias correction from device memory)")
        self.model, self.optimizer, self.group = model, optimizer, group
        self.warmup = int(warmup)
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        self.split = multi if split is None else (bool(split) or multi)
        self.calls = 0
        self.graphs = None
        self.ids = self.labels = self.loss = None

    def _eager(self, input_ids, labels):
        # (on the CURRENT stream.  Warming up on a side stream, as the PyTorch recipe has it, made the first replay after a
        #  device-wide synchronize fault on this ROCm stack -- HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION, full-size model only;
        #  tools/graph_step_debug.py -- and buys nothing here: no DDP hooks, one autograd stream)
        return train_step(self.model, input_ids, labels, self.optimizer, self.group, max_grad_norm=None)

    def _capture(self, input_ids, labels):
        self.ids, self.labels = input_ids.clone(), labels.clone()
        self.optimizer.init_state()
        self.optimizer.zero_grad(set_to_none=True)  # the gradients are (re)allocated inside the graph's pool
        try:
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1):
                self.loss = self.model(self.ids, self.labels)
                self.loss.backward()
                if not self.split:
                    self.optimizer.step()
                self.loss = self.loss.detach()
            graphs = [g1]
            if self.split:
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2, pool=g1.pool()):
                    self.optimizer.step()
                graphs.append(g2)
        except BaseException:
            # a capture that threw midway must not leave the optimizer "holding a captured step" for good
            self.optimizer.release_captured_step()
            raise
        self.graphs = graphs
        self._token = self.optimizer.capture_token()  # (close() releases THIS capture only: ADVICE r5)
        # what the capture baked in (see the class docstring)
        self._baked = [(tuple(g["betas"]), float(g["eps"])) for g in self.optimizer.param_groups]
        self._grads = [(p, p.grad) for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]

    def close(self):
        """Drop the captured step: the graphs go and the optimizer may capture again (another GraphedTrainStep, e.g. for a new batch shape)."""
        if self.graphs is not None:
            self.graphs = None
            self.optimizer.release_captured_step(getattr(self, "_token", None))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_baked(self):
        for g, (betas, eps) in zip(self.optimizer.param_groups, self._baked):
            if tuple(g["betas"]) != betas or float(g["eps"]) != eps:
                raise RuntimeError("GraphedTrainStep: betas / eps are launch arguments of the captured optimizer step and cannot change "
                                   "after capture (lr and weight_decay can: they travel through device memory)")
        for p, gr in self._grads:
            if p.grad is not gr:
                raise RuntimeError("GraphedTrainStep: p.grad was reset or replaced between replays; the captured graph owns the gradient "
                                   "tensors (use zero_grad(set_to_none=False) if they have to be cleared)")

    def __call__(self, input_ids, labels):
        self.calls += 1
        if self.graphs is None:
            if self.calls <= self.warmup:
                return self._eager(input_ids, labels)
            self._capture(input_ids, labels)
        else:
            if input_ids.shape != self.ids.shape or labels.shape != self.labels.shape:
                raise ValueError(f"GraphedTrainStep was captured for batches {tuple(self.ids.shape)} / {tuple(self.labels.shape)}")
            self.ids.copy_(input_ids, non_blocking=True)
            self.labels.copy_(labels, non_blocking=True)
        self._check_baked()
        self.optimizer.graph_advance()
        self.graphs[0].replay()
        if self.split:
            allreduce_gradients(self.model, self.group)
            self.graphs[1].replay()
        return self.loss
