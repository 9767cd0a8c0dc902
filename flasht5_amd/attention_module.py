"""A `FlashT5Attention`-compatible module on top of the MI355X operators.

Mirrors the interface of the reference module (src/model/modeling_flash_t5.py:166-287): same constructor signature
`(config, has_positional_encoding=False, is_causal=False)`, same parameter names (`Wq`, `Wk`, `Wv`, `o`,
`pe_encoding.relative_attention_bias`) so reference checkpoints load, same `forward(hidden_states, mask=None,
key_value_states=None, position_bias=None) -> (output, position_bias)` with the position bias of block 0 handed on to
the following blocks.  Two attention types:

  * "triton"   -- the reference's name for its `flash_attention_v2_bias` path: dense `(1|B, H, M, N)` bias, here
                  through `flasht5_amd.flash_attention_v2_bias` (drop-in);
  * "fat5_rpe" -- linear memory: the handed-on "position bias" is the `(H, 2R+1)` generator (with its radius), built
                  once by block 0 and consumed in-kernel by every block (`flash_attention_v2_rpe1d`); nothing of size
                  S x S is allocated in either direction (the role of the reference's external "fa2_rpe" type, :272-279).

`position_encoding_type="RoPE"` (config keys `rotary_emb_fraction`, `rotary_base`, `rotary_interleaved`, `rotary_scale_base`,
`max_sequence_length`) builds a `RotaryPositionalEncoding` in EVERY layer, cross-attention included, as the reference does
(:214-220 carry no `has_positional_encoding` condition): q, k and v are rotated (v too, like the reference) in one kernel launch
and the attention runs without a bias.  As in the reference (:259), a layer handed a `position_bias` uses that bias and
does not rotate.

`position_encoding_type="FIRE"` (config key `fire_mlp_width`, default 32) builds, in the layer that owns the position encoding
(block 0's self-attention, as in the reference, :221-225), `FIRE(n_heads, fire_mlp_width, 0.1, relative_attention_max_distance)`:
its (1, H, S, S) bias comes from one HIP kernel (flasht5_amd/fire.py) and is handed on to the following blocks like the T5 bias,
with `use_full_bias_size` and `use_masking` applied the same way.  FIRE needs the dense-bias type ("triton"): its bias is not
Toeplitz once a row passes the threshold T, so `fat5_rpe` cannot carry it.  Other producers' dense outputs (ALiBi, ...) can be
passed as `position_bias`.  Dropout is not supported (like the reference's Triton path, :201)."""
import math

import torch
from torch import nn

from .flash_attention_v2_bias import flash_attention_v2_bias, flash_attention_v2_rpe1d
from .fire import FIRE
from .positional_encoding import RelativePositionalEncoding
from .rotary import RotaryPositionalEncoding, apply_rotary_emb, apply_rotary_emb_packed, apply_rotary_emb_qkv


def _cfg(config, name, default):
    return getattr(config, name, default)


class _UnpackHeads(torch.autograd.Function):
    """(B, S, n * H * D) projection output -> n views (B, H, S, D) (slice i = heads of projection i).  Same values as
    `x.view(B, S, n, H, D)[:, :, i].permute(0, 2, 1, 3)`; the difference is the backward: autograd's select would allocate a
    zero-filled (B, S, n, H, D) tensor per slice, copy the slice's gradient in and add the n tensors up.  The attention
    backward writes the gradients of packed slices into the slices of ONE buffer (flash_attention_v2_bias.packed_slices): when
    the incoming gradients are exactly those, the buffer itself is the result (no kernel at all); otherwise one stack."""

    @staticmethod
    def forward(ctx, x, n, H):
        B, S, W = x.shape
        D = W // (n * H)
        ctx.dims = (B, S, n, H, D)
        p = x.view(B, S, n, H, D)
        return tuple(p[:, :, i].permute(0, 2, 1, 3) for i in range(n))

    @staticmethod
    def backward(ctx, *gs):
        B, S, n, H, D = ctx.dims
        row = n * H * D
        g0 = gs[0]
        if all(g is not None for g in gs):
            same = all(g.untyped_storage().data_ptr() == g0.untyped_storage().data_ptr() and g.dtype == g0.dtype and
                       g.stride() == (S * row, D, row, 1) and g.storage_offset() == g0.storage_offset() + i * H * D
                       for i, g in enumerate(gs))
            if same and g0.untyped_storage().nbytes() >= (g0.storage_offset() + B * S * row) * g0.element_size():
                return g0.as_strided((B, S, row), (S * row, row, 1), g0.storage_offset()), None, None
        ref = next(g for g in gs if g is not None)
        parts = [(g if g is not None else torch.zeros_like(ref)).permute(0, 2, 1, 3) for g in gs]  # (B, S, H, D) each
        return torch.stack(parts, 2).reshape(B, S, row), None, None


def unpack_heads(x, n, n_heads):
    """the n head-major (B, H, S, D) views of a packed (B, S, n * H * D) projection output (see _UnpackHeads)"""
    from . import _lib
    nat = None if (torch.compiler.is_compiling() or not x.is_cuda) else _lib.native()
    if nat is not None:  # (the same function in C++: csrc/torch_binding.cpp::UnpackHeadsFn)
        return tuple(nat.unpack_heads_apply(x, int(n), int(n_heads)))
    return _UnpackHeads.apply(x, n, n_heads)


class FlashT5Attention(nn.Module):
    def __init__(self, config, has_positional_encoding=False, is_causal=False):
        super().__init__()
        self.is_decoder = _cfg(config, "is_decoder", False)
        self.has_positional_encoding = has_positional_encoding
        self.is_causal = is_causal
        self.d_model = config.d_model
        self.key_value_proj_dim = config.d_kv
        self.n_heads = config.num_heads
        self.inner_dim = self.n_heads * self.key_value_proj_dim
        self.attention_type = _cfg(config, "attention_type", "triton")
        self.position_encoding_type = _cfg(config, "position_encoding_type", "t5")
        scale = _cfg(config, "attention_scale", None)
        # (the reference's default is 1/sqrt(n_heads), modeling_flash_t5.py:184 -- kept for checkpoint parity)
        self.softmax_scale = scale if scale is not None else 1.0 / math.sqrt(self.n_heads)
        self.use_full_bias_size = _cfg(config, "use_full_bias_size", False)
        self.use_masking = _cfg(config, "use_masking", False)
        if self.attention_type not in ("triton", "fat5_rpe"):
            raise ValueError(f"attention_type {self.attention_type!r}: this module implements 'triton' (dense bias) and 'fat5_rpe'")
        if _cfg(config, "attention_dropout_rate", 0.0) != 0.0:
            raise ValueError("attention dropout is not supported by the fused kernels")
        if self.attention_type == "fat5_rpe" and self.position_encoding_type == "FIRE":
            raise ValueError("FIRE needs attention_type='triton' (dense bias): its bias is not Toeplitz once a row passes the "
                             "threshold T, so fat5_rpe cannot carry it")
        if self.attention_type == "fat5_rpe" and (self.position_encoding_type not in ("t5", "RoPE") or self.use_masking):
            raise ValueError("fat5_rpe needs the T5 relative-position encoding or RoPE, and no key masking (use var-len batches)")
        self.pe_encoding = None
        self._randomized = bool(_cfg(config, "use_randomized_position_encoding", False))  # (decode time: forward_decode refuses it)
        self.rotary = self.position_encoding_type == "RoPE"
        if self.rotary:  # (every layer: the reference's RoPE branch has no has_positional_encoding condition, :214)
            self.pe_encoding = RotaryPositionalEncoding(
                int(self.key_value_proj_dim * _cfg(config, "rotary_emb_fraction", 1.0)), _cfg(config, "max_sequence_length", 1024),
                _cfg(config, "rotary_base", 10000), _cfg(config, "rotary_interleaved", False), _cfg(config, "rotary_scale_base", None),
                randomized_position=_cfg(config, "use_randomized_position_encoding", False))
        elif self.position_encoding_type == "t5" and has_positional_encoding:
            self.pe_encoding = RelativePositionalEncoding(
                config.relative_attention_num_buckets, config.relative_attention_max_distance, self.n_heads,
                _cfg(config, "max_sequence_length", 0), bidirectional=not self.is_decoder,
                randomized_position=_cfg(config, "use_randomized_position_encoding", False))
        elif self.position_encoding_type == "FIRE" and has_positional_encoding:
            self.pe_encoding = FIRE(num_heads=self.n_heads, mlp_width=_cfg(config, "fire_mlp_width", 32), init_c=0.1,
                                    init_L=config.relative_attention_max_distance)
        elif self.position_encoding_type != "t5" and has_positional_encoding:
            raise ValueError("only the T5, RoPE and FIRE producers are built in; pass other encodings' dense bias as position_bias")
        self.Wq = nn.Linear(self.d_model, self.inner_dim, bias=False)
        self.Wk = nn.Linear(self.d_model, self.inner_dim, bias=False)
        self.Wv = nn.Linear(self.d_model, self.inner_dim, bias=False)
        self.o = nn.Linear(self.inner_dim, self.d_model, bias=False)

    def forward(self, hidden_states, mask=None, key_value_states=None, position_bias=None, cu_seqlens=None, max_seqlen=None,
                kv_cu_seqlens=None, kv_max_seqlen=None):
        """cu_seqlens / max_seqlen (and, for cross-attention, kv_cu_seqlens / kv_max_seqlen of the key / value side): packed
        hidden states (1, total, d_model), every sequence attending inside itself with positions of its own (packed_supported)"""
        if cu_seqlens is not None:
            return self._forward_packed(hidden_states, key_value_states, position_bias, cu_seqlens, max_seqlen, kv_cu_seqlens,
                                        kv_max_seqlen)
        B, M = hidden_states.shape[:2]
        src = hidden_states if key_value_states is None else key_value_states
        N = src.shape[1]
        # (B, S, H, D) storage viewed as (B, H, S, D): the kernels take the strided views as they are
        q = self.Wq(hidden_states).view(B, M, self.n_heads, self.key_value_proj_dim)
        k = self.Wk(src).view(B, N, self.n_heads, self.key_value_proj_dim)
        v = self.Wv(src).view(B, N, self.n_heads, self.key_value_proj_dim)
        if self.rotary and position_bias is None:  # q, k, v in one launch (new tensors: nothing autograd saved is touched)
            q, k, v, _ = self.pe_encoding(q, k, v)
        q, k, v = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        out, position_bias = self._attend(q, k, v, hidden_states.dtype, mask, key_value_states is None, position_bias)
        return self.o(out), position_bias

    def forward_fused(self, hidden_states, norm_weight, eps, mask=None, key_value_states=None, position_bias=None, cu_seqlens=None,
                      max_seqlen=None, kv_cu_seqlens=None, kv_max_seqlen=None):
        """One whole T5 attention sub-layer, `h + o(attention(layer_norm(h)))` (reference modeling_flash_t5.py:304-318 / :321-349),
        with the pre-norm inside the projection GEMM and the residual add as the output projection's epilogue
        (`fused_linear.rmsnorm_linear` / `linear_residual`): `hidden_states` is the UN-normalised residual stream,
        `norm_weight` / `eps` the sub-layer's `layer_norm`.  Returns (new residual stream, position_bias)."""
        from .fused_linear import rmsnorm_linear, linear_residual
        B, M = hidden_states.shape[:2]
        H, Dh = self.n_heads, self.key_value_proj_dim
        if cu_seqlens is not None:    # packed rows: the same GEMMs, then (total, H, D) views of their outputs
            self.packed_supported()
            self._packed_args(hidden_states, key_value_states, cu_seqlens, max_seqlen, kv_cu_seqlens, kv_max_seqlen)
            if key_value_states is None:
                qkv, res = rmsnorm_linear(hidden_states, norm_weight, (self.Wq.weight, self.Wk.weight, self.Wv.weight), eps, return_residual=True)
                q, k, v = (t[0].transpose(0, 1) for t in unpack_heads(qkv, 3, H))
            else:
                q, res = rmsnorm_linear(hidden_states, norm_weight, self.Wq.weight, eps, return_residual=True)
                kv = torch.nn.functional.linear(key_value_states, torch.cat((self.Wk.weight, self.Wv.weight), 0))
                q = q.view(M, H, Dh)
                k, v = (t[0].transpose(0, 1) for t in unpack_heads(kv, 2, H))
            out, position_bias = self._attend_packed(q, k, v, key_value_states is None, position_bias, cu_seqlens, max_seqlen,
                                                     kv_cu_seqlens, kv_max_seqlen)
            return linear_residual(out, self.o.weight, res), position_bias
        if key_value_states is None:  # self-attention: ONE GEMM for q, k, v
            qkv, res = rmsnorm_linear(hidden_states, norm_weight, (self.Wq.weight, self.Wk.weight, self.Wv.weight), eps, return_residual=True)
            if self.rotary and position_bias is None:  # the packed buffer in, a packed buffer out (and its gradient packed again): one launch each way
                (qkv,) = apply_rotary_emb_packed((qkv,), (3,), H, *self._rotary_tables(qkv), nq=1, interleaved=self.pe_encoding.interleaved)
            q, k, v = unpack_heads(qkv, 3, H)
        else:                         # cross-attention: the decoder side is normed, the encoder output is not (:330-336)
            q, res = rmsnorm_linear(hidden_states, norm_weight, self.Wq.weight, eps, return_residual=True)
            kv = torch.nn.functional.linear(key_value_states, torch.cat((self.Wk.weight, self.Wv.weight), 0))
            if self.rotary and position_bias is None:  # q and the packed k | v in one launch
                q, kv = apply_rotary_emb_packed((q, kv), (1, 2), H, *self._rotary_tables(q), nq=1, interleaved=self.pe_encoding.interleaved)
            q = q.view(B, M, H, Dh).permute(0, 2, 1, 3)
            k, v = unpack_heads(kv, 2, H)
        out, position_bias = self._attend(q, k, v, hidden_states.dtype, mask, key_value_states is None, position_bias)
        return linear_residual(out, self.o.weight, res), position_bias

    def packed_supported(self):
        """raise NotImplementedError when this layer cannot run packed (cu_seqlens) rows: the packed kernels carry the T5 generator
        or no bias at all, never a dense (B, H, M, N) one"""
        if self.position_encoding_type == "FIRE":
            raise NotImplementedError("padding masks / segment ids with FIRE: its bias is dense, and the packed (cu_seqlens) kernels "
                                      "take no dense bias")
        if self._randomized:
            raise NotImplementedError("padding masks / segment ids with use_randomized_position_encoding: randomized positions are "
                                      "not a function of n - m, which is what the packed kernels' in-kernel bias is built from")
        if self.position_encoding_type == "t5" and self.attention_type != "fat5_rpe":
            raise NotImplementedError("padding masks / segment ids with the dense T5 bias (attention_type='triton'): the packed "
                                      "(cu_seqlens) kernels take no dense bias; use attention_type='fat5_rpe'")
        if self.position_encoding_type not in ("t5", "RoPE"):
            raise NotImplementedError(f"padding masks / segment ids with position_encoding_type {self.position_encoding_type!r}")

    def _packed_args(self, hidden_states, key_value_states, cu_seqlens, max_seqlen, kv_cu_seqlens, kv_max_seqlen):
        if max_seqlen is None:
            raise ValueError("cu_seqlens needs max_seqlen")
        if hidden_states.dim() != 3 or hidden_states.shape[0] != 1:
            raise ValueError(f"packed hidden states are (1, total, d_model), got {tuple(hidden_states.shape)}")
        if key_value_states is not None:
            if kv_cu_seqlens is None or kv_max_seqlen is None:
                raise ValueError("packed cross-attention needs kv_cu_seqlens and kv_max_seqlen of the key / value side")
            if key_value_states.dim() != 3 or key_value_states.shape[0] != 1:
                raise ValueError(f"packed key / value states are (1, total_k, d_model), got {tuple(key_value_states.shape)}")

    def _forward_packed(self, hidden_states, key_value_states, position_bias, cu_seqlens, max_seqlen, kv_cu_seqlens, kv_max_seqlen):
        self.packed_supported()
        self._packed_args(hidden_states, key_value_states, cu_seqlens, max_seqlen, kv_cu_seqlens, kv_max_seqlen)
        H, Dh = self.n_heads, self.key_value_proj_dim
        src = hidden_states if key_value_states is None else key_value_states
        q = self.Wq(hidden_states).view(hidden_states.shape[1], H, Dh)
        k = self.Wk(src).view(src.shape[1], H, Dh)
        v = self.Wv(src).view(src.shape[1], H, Dh)
        out, position_bias = self._attend_packed(q, k, v, key_value_states is None, position_bias, cu_seqlens, max_seqlen,
                                                 kv_cu_seqlens, kv_max_seqlen)
        return self.o(out), position_bias

    def _attend_packed(self, q, k, v, is_self, position_bias, cu, mx, kv_cu, kv_mx):
        """packed attention of projected (total, H, D) views -> (1, total_q, inner_dim), plus the position bias to hand on: the T5
        generator of block 0's forward_1d() in-kernel, or rotated q / k / v and no bias, positions local to each sequence"""
        from .flash_attention_v2_bias import flash_attn_varlen_func
        if is_self:
            kv_cu, kv_mx = cu, mx
        rpe1d, radius = None, 0
        if self.rotary and position_bias is None:
            cos, sin, cos_k, sin_k = self._rotary_tables(q)
            il = self.pe_encoding.interleaved
            if is_self:
                q, k, v = apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k, sin_k, il, cu_seqlens=cu, max_seqlen=mx)
            else:  # (the two sides count their own positions: q under the decoder's cu_seqlens, k and v under the encoder's)
                ck, sk = (cos, sin) if cos_k is None else (cos_k, sin_k)
                q = apply_rotary_emb(q, cos, sin, il, cu_seqlens=cu, max_seqlen=mx)
                k = apply_rotary_emb(k, ck, sk, il, cu_seqlens=kv_cu, max_seqlen=kv_mx)
                v = apply_rotary_emb(v, ck, sk, il, cu_seqlens=kv_cu, max_seqlen=kv_mx)
        elif is_self:
            if position_bias is None and self.pe_encoding is not None:
                position_bias = self.pe_encoding.forward_1d()
            if position_bias is None:
                raise ValueError("fat5_rpe self-attention without a bias producer needs position_bias=(rpe1d, radius) from the "
                                 "block that owns the RelativePositionalEncoding")
            rpe1d, radius = position_bias
        out = flash_attn_varlen_func(q, k, v, cu, kv_cu, mx, kv_mx, self.is_causal and is_self, self.softmax_scale, rpe1d, radius)
        return out.reshape(1, q.shape[0], self.inner_dim), position_bias

    def decode_supported(self):
        """raise NotImplementedError when this layer cannot run a cached decoding step"""
        if self.position_encoding_type == "FIRE":
            raise NotImplementedError("FIRE at decode time: the bias row of query p needs a query offset the FIRE kernel does not take")
        if self.position_encoding_type == "t5" and self._randomized:
            raise NotImplementedError("randomized positions at decode time: they are not a function of n - m, so no cached row has "
                                      "a fixed bias")
        if self.position_encoding_type not in ("t5", "RoPE"):
            raise NotImplementedError(f"position_encoding_type {self.position_encoding_type!r} at decode time")

    def forward_decode(self, hidden_states, k_cache, v_cache, cache_seqlens=None, position_bias=None, position=None,
                       cache_batch_idx=None, cache_row_batch=None, cross_seqlens=None, chunk_seqlens=None, k_scale=None, v_scale=None):
        """One new token through this layer against a KV cache (flasht5_amd.decode.flash_attn_with_kvcache); returns (B, 1, d_model).

        Self-attention (`cache_seqlens` given): q, k and v are projected from `hidden_states` (B, 1, d_model), k and v are appended
        to `k_cache` / `v_cache` (B, L_cap, H, D) at index cache_seqlens[b] and the row attends over cache_seqlens[b] + 1 keys with
        the decoder's `position_bias = (rpe1d, R)` (block 0's `forward_1d()`, bottom-right aligned: the query sits at the last key).
        Cross-attention (`cache_seqlens` None): the caches hold the encoder's K / V (`project_kv`), all of them attended, no bias.
        RoPE: `position` is a (1,) int64 device tensor (the step's position, shared by the batch); q is rotated with row `position`
        of (cos, sin), the new k and v with that row of (cos_k, sin_k).  Forward only; nothing of the training path changes.
        Beam search: `cache_batch_idx` (B,) int32 lets B * k beam rows read B cross-attention caches; `cache_row_batch`
        (B, L_cap) int32 reads each self-attention key row from the cache row of the beam that wrote it (decode.py).

        A chunk of M > 1 tokens (`hidden_states` (B, M, d_model); returns (B, M, d_model)) goes through
        flash_attn_with_kvcache_chunk: self-attention appends the M rows and is causal inside the chunk, row i at position
        cache_seqlens[b] + i; cross-attention is not causal and has no bias.  RoPE uses rows position + arange(M) of the tables,
        selected and clamped on the device.  The cache maps are for one row only.

        Padding: `cross_seqlens` (B,) int32 (cross-attention only) is the number of valid encoder keys of each query row -- the
        kernels' cache_seqlens without an append; with `cache_batch_idx` it is per query row, not per cache row.  `chunk_seqlens`
        (B,) int32 (chunks only): the rows of the chunk each batch element brings (flash_attn_with_kvcache_chunk).

        FP8 caches: `k_scale` / `v_scale` (B, L_cap, H) fp32, the scales of float8_e4m3fn caches (decode.py); None: 16-bit caches."""
        self.decode_supported()
        B, M = hidden_states.shape[:2]
        H, Dh = self.n_heads, self.key_value_proj_dim
        q = self.Wq(hidden_states).view(B, M, H, Dh)
        k = v = None
        if cache_seqlens is not None:
            k = self.Wk(hidden_states).view(B, M, H, Dh)
            v = self.Wv(hidden_states).view(B, M, H, Dh)
        return self.o(self.attend_decode(q, k, v, k_cache, v_cache, cache_seqlens, position_bias, position, cache_batch_idx,
                                         cache_row_batch, cross_seqlens, chunk_seqlens, k_scale, v_scale))

    def attend_decode(self, q, k, v, k_cache, v_cache, cache_seqlens=None, position_bias=None, position=None, cache_batch_idx=None,
                      cache_row_batch=None, cross_seqlens=None, chunk_seqlens=None, k_scale=None, v_scale=None):
        """`forward_decode` between its projections: q (B, M, H, D) and, for self-attention, the new k / v rows (B, M, H, D; strided
        views are taken as they are) -> the attention output (B, M, inner_dim) in front of `o`; the arguments are forward_decode's"""
        from .decode import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk
        B, M = q.shape[:2]
        if M > 1 and (cache_batch_idx is not None or cache_row_batch is not None):
            raise ValueError("forward_decode: cache_batch_idx / cache_row_batch take one query row per step (beam search has no chunks)")
        if M == 1 and chunk_seqlens is not None:
            raise ValueError("forward_decode: chunk_seqlens needs a chunk of M > 1 rows")
        if cross_seqlens is not None and cache_seqlens is not None:
            raise ValueError("forward_decode: cross_seqlens is for cross-attention (cache_seqlens None)")
        is_self = cache_seqlens is not None
        rpe1d, radius = None, 0
        if self.rotary:
            if position is None:
                raise ValueError("forward_decode with RoPE needs the step's position (a (1,) int64 device tensor)")
            cos, sin, cos_k, sin_k = self.pe_encoding.tables(q.device, q.dtype)
            idx = position  # (device-side: capturable; one row adds no launch, a chunk takes rows position .. position + M - 1)
            if M > 1:
                idx = (position + torch.arange(M, device=position.device)).clamp(0, cos.shape[0] - 1)
            rows = lambda t: None if t is None else t.index_select(0, idx)  # noqa: E731
            if is_self:
                q, k, v = apply_rotary_emb_qkv(q, k, v, rows(cos), rows(sin), rows(cos_k), rows(sin_k), self.pe_encoding.interleaved)
            else:
                q = apply_rotary_emb(q, rows(cos), rows(sin), self.pe_encoding.interleaved)
        elif is_self:
            if position_bias is None:
                raise ValueError("forward_decode: T5 self-attention needs position_bias=(rpe1d, radius) from block 0's forward_1d()")
            rpe1d, radius = position_bias
            if self.attention_type == "triton":  # (the dense path adds the bias after a cast to the activation dtype)
                rpe1d = rpe1d.to(q.dtype).float()
        lens = cache_seqlens if is_self else cross_seqlens
        fp8 = {} if k_scale is None else dict(k_scale=k_scale, v_scale=v_scale)
        if M == 1:
            out = flash_attn_with_kvcache(q, k_cache, v_cache, k, v, lens, self.softmax_scale, rpe1d, radius,
                                          cache_batch_idx=cache_batch_idx, cache_row_batch=cache_row_batch, **fp8)
        else:
            out = flash_attn_with_kvcache_chunk(q, k_cache, v_cache, k, v, lens, self.softmax_scale, causal=is_self, rpe1d=rpe1d,
                                                rpe_radius=radius, chunk_seqlens=chunk_seqlens, **fp8)
        return out.reshape(B, M, self.inner_dim)

    def project_kv(self, key_value_states):
        """the cross-attention K / V of an encoder output (B, L_enc, d_model) as (B, L_enc, H, D) caches for `forward_decode`:
        projected once, and with RoPE rotated once at positions 0..L_enc-1 with (cos_k, sin_k), as the full forward does"""
        self.decode_supported()
        B, N = key_value_states.shape[:2]
        k = self.Wk(key_value_states).view(B, N, self.n_heads, self.key_value_proj_dim)
        v = self.Wv(key_value_states).view(B, N, self.n_heads, self.key_value_proj_dim)
        if self.rotary:
            cos, sin, cos_k, sin_k = self.pe_encoding.tables(k.device, k.dtype)
            ck, sk = (cos, sin) if cos_k is None else (cos_k, sin_k)
            k = apply_rotary_emb(k, ck, sk, self.pe_encoding.interleaved)
            v = apply_rotary_emb(v, ck, sk, self.pe_encoding.interleaved)
        return k.contiguous(), v.contiguous()

    def _rotary_tables(self, x):
        return self.pe_encoding.tables(x.device, x.dtype)

    def _attend(self, q, k, v, dtype, mask, is_self, position_bias):
        """attention of projected (B, H, S, D) views -> (B, M, inner_dim), plus the position bias to hand on"""
        B, _, M, _ = q.shape
        N = k.shape[2]
        if self.rotary and position_bias is None:  # (q, k, v already rotated: no bias, and none handed on)
            out = flash_attention_v2_bias(q, k, v, None, self.is_causal, self.softmax_scale)
            return out.permute(0, 2, 1, 3).reshape(B, M, self.inner_dim), None
        key_value_states = None if is_self else True
        hidden_dtype = dtype
        if self.attention_type == "fat5_rpe":
            if position_bias is None and self.pe_encoding is not None:
                position_bias = self.pe_encoding.forward_1d()
            if position_bias is None:
                # no producer and nothing handed on: T5 cross-attention (reference :207,:324 -> bias=None, HAS_BIAS=False).
                # A SELF-attention layer without a producer must be handed block 0's (rpe1d, radius): training it silently
                # without the T5 bias would be a wiring bug of the caller, not a mode.
                if key_value_states is None and self.position_encoding_type == "t5":
                    raise ValueError("fat5_rpe self-attention without a bias producer needs position_bias=(rpe1d, radius) from the "
                                     "block that owns the RelativePositionalEncoding")
                out = flash_attention_v2_bias(q, k, v, None, self.is_causal, self.softmax_scale)
            else:
                rpe1d, radius = position_bias
                out = flash_attention_v2_rpe1d(q, k, v, rpe1d, radius, self.is_causal, self.softmax_scale)
        else:
            if position_bias is None and isinstance(self.pe_encoding, FIRE):  # (the reference's FIRE.forward: (1, H, S, S), S = M)
                # (no .contiguous(): when S is not a multiple of 8 the bias rows are padded to 16 bytes, which the kernels take as is)
                position_bias = self.pe_encoding.compute_bias(M, M, q.device, q.dtype)
            elif position_bias is None and self.pe_encoding is not None:
                position_bias = self.pe_encoding.compute_bias(M, N, device=q.device).contiguous().to(q.dtype)
            bias = position_bias
            if bias is not None and self.use_full_bias_size:
                bias = bias.expand(B, self.n_heads, M, N).contiguous()
                position_bias = bias
            if bias is not None and mask is not None and self.use_masking:
                m = mask.unsqueeze(1)
                if m.dim() == 3:
                    m = m.unsqueeze(3)
                bias = torch.where(m, bias, torch.finfo(hidden_dtype).min)
                position_bias = bias
            out = flash_attention_v2_bias(q, k, v, bias, self.is_causal, self.softmax_scale)
        return out.permute(0, 2, 1, 3).reshape(B, M, self.inner_dim), position_bias
