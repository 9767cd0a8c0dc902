"""Many-row MXFP4-weight linear layers on gfx950's block-scaled MFMA, W4A8 (include/fat5.h, "MXFP8 activations";
csrc/w4a8_kernels.h): the encoder's side of the quantised formats.

    a8, ax = quantize_activation_mxfp8(x)                # x (..., K) fp16 / bf16 -> uint8 (..., K) e4m3fn, uint8 (..., K / 32) e8m0
    y = w4a8_matmul(a8, ax, w4, e8, x.dtype)             # w4 / e8 from `quantize_weight_mxfp4` -> (..., N)
    y = w4a8_linear(x, w4, e8, norm_weight=g, eps=1e-6, residual=h)      # the two launches in a row

Activations are quantised per row and block of 32 consecutive k: X = floor(log2 amax) - 8 (scale byte X + 127 clamped to
[1, 254]; amax = 0: X = 0), element = round-to-nearest-even of x 2^-X onto e4m3fn, saturating at 448; a block with an inf or a NaN
gets scale byte 255 over zero bytes and makes its output row NaN.  `norm_weight` puts the T5 RMSNorm in front, inside the
quantiser's launch (bit for bit `quantize_activation_mxfp8(fast_rms_layernorm(x, g, eps))`); `residual` is added to the rounded
result inside the GEMM's launch (bit for bit `residual + plain`).  The GEMM sums in an order that depends on K alone: the same
bits for any row count, on every run, under graph replay, and a row's result does not depend on its neighbours.  The sum is the
instruction's, not an fp32 sum of the products: inside a block of 32 k it aligns the products to the block's largest and drops what
lies about 2^-12 below it (measured), so a block whose products are that far apart loses the small ones.

`quantize_encoder_weights_mxfp4(model)` builds, once per model, the MXFP4 copies of the encoder's projections;
`encoder_forward_mxfp4` runs the encoder stack over them (`generate(..., encoder_weight_dtype="mxfp4")`, and
`forward(..., weight_dtype="mxfp4")` of the encoder-only models).  Forward only; there is no CPU path and no fallback."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from . import _lib
from .w4 import BLOCK, _check_packed, _stack, check_shape
from .w8 import _row_ready, _rows

_CODES = {torch.float16: _lib.FAT5_F16, torch.bfloat16: _lib.FAT5_BF16}


def _check_bytes(what, name, t, shape):
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be a uint8 {tuple(shape)} tensor, got {t.dtype} {tuple(t.shape)}")
    if t.numel() and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise ValueError(f"{what}: {name} needs innermost stride 1")


def _check_a8(what, a8, ax):
    """a8 (R, K) and ax (R, K / 32) of one activation -> (R, K)"""
    if a8.dim() != 2 or a8.dtype != torch.uint8 or ax.dim() != 2:
        raise ValueError(f"{what}: a8 must be a uint8 (R, K) tensor, got {a8.dtype} {tuple(a8.shape)}")
    R, K = a8.shape
    if K % BLOCK != 0:
        raise ValueError(f"{what}: K = {K} (the activation's width must be a multiple of 32)")
    _check_bytes(what, "a8", a8, (R, K))
    _check_bytes(what, "ax", ax, (R, K // BLOCK))
    if a8.numel() and (a8.data_ptr() % 16 != 0 or (R > 1 and a8.stride(0) % 16 != 0)):
        raise ValueError(f"{what}: a8 needs a 16-byte aligned base and a row stride that is a multiple of 16 bytes")
    return R, K


def _check_quantize(x, norm_weight, eps, out, scales):
    what = "quantize_activation_mxfp8"
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be (R, K) here, got {tuple(x.shape)}")
    if x.dtype not in _CODES:
        raise ValueError(f"{what}: x of dtype {x.dtype} (fp16 or bf16)")
    R, K = x.shape
    check_shape(8, K, what)
    _check_a8(what, out, scales)
    if tuple(out.shape) != (R, K):
        raise ValueError(f"{what}: out must be {(R, K)}, got {tuple(out.shape)}")
    if norm_weight is not None:
        if norm_weight.dtype != x.dtype or tuple(norm_weight.shape) != (K,) or not norm_weight.is_contiguous() or norm_weight.data_ptr() % 16:
            raise ValueError(f"{what}: norm_weight must be a contiguous, 16-byte aligned {x.dtype} ({K},) tensor, got {norm_weight.dtype} "
                             f"{tuple(norm_weight.shape)}")
        if not (eps >= 0.0 and eps < float("inf")):
            raise ValueError(f"{what}: eps {eps} (finite, >= 0)")
    if x.numel() and not _row_ready(x):
        raise ValueError(f"{what}: x needs innermost stride 1, a 16-byte aligned base and a row stride that is a multiple of 8")


def _one_gpu(what, *ts):
    first = next(t for t in ts if t is not None)
    if any(t is not None and (not t.is_cuda or t.device != first.device) for t in ts):
        raise ValueError(f"{what}: tensors must be on one GPU (there is no CPU path)")


# ------------------------------------------------------------------------------------------------------------------ operators
@torch.library.custom_op("fat5::mx8_quantize", mutates_args=("out", "scales"), device_types="cuda")
def mx8_quantize(x: torch.Tensor, norm_weight: Optional[torch.Tensor], eps: float, out: torch.Tensor, scales: torch.Tensor) -> None:
    """x (R, K) -> out (R, K) e4m3fn bytes, scales (R, K / 32) e8m0 bytes, in one launch (fat5_mx8_quantize)"""
    _check_quantize(x, norm_weight, eps, out, scales)
    _one_gpu("quantize_activation_mxfp8", x, norm_weight, out, scales)
    R, K = x.shape
    if R == 0:
        return
    p = _lib.Mx8QuantParams()
    p.R, p.K, p.dtype = R, K, _CODES[x.dtype]
    p.x, p.x_stride = x.data_ptr(), (x.stride(0) if R > 1 else K)   # (one row: its stride is never used)
    if norm_weight is not None:
        p.norm_weight, p.eps = norm_weight.data_ptr(), float(eps)
    p.a8, p.a_stride = out.data_ptr(), (out.stride(0) if R > 1 else K)
    p.ax, p.ax_stride = scales.data_ptr(), (scales.stride(0) if R > 1 else K // BLOCK)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().fat5_mx8_quantize(p, _lib.stream_ptr(x.device)), "fat5_mx8_quantize")


@mx8_quantize.register_fake
def _mx8_quantize_fake(x, norm_weight, eps, out, scales):
    return None


def _check_matmul(a8, ax, w4, e8, dtype, residual):
    what = "w4a8_matmul"
    if dtype not in _CODES:
        raise ValueError(f"{what}: dtype {dtype} (fp16 or bf16)")
    R, K = _check_a8(what, a8, ax)
    N, Kw = _check_packed(what, w4, e8)
    if K != Kw:
        raise ValueError(f"{what}: a8 has {K} columns, the weight K = {Kw}")
    if residual is not None:
        if residual.dtype != dtype or tuple(residual.shape) != (R, N):
            raise ValueError(f"{what}: residual must be a {dtype} {(R, N)} tensor, got {residual.dtype} {tuple(residual.shape)}")
        if residual.numel() and not _row_ready(residual):
            raise ValueError(f"{what}: residual needs innermost stride 1, a 16-byte aligned base and a row stride that is a multiple of 8")
    return R, N, K


@torch.library.custom_op("fat5::w4a8_matmul", mutates_args=(), device_types="cuda")
def w4a8_matmul_op(a8: torch.Tensor, ax: torch.Tensor, w4: torch.Tensor, e8: torch.Tensor, dtype: torch.dtype,
                   residual: Optional[torch.Tensor]) -> torch.Tensor:
    """a8 (R, K), ax (R, K / 32), w4 (N, K / 2), e8 (N, K / 32) -> (R, N) contiguous of `dtype`, in one launch (fat5_w4a8_linear)"""
    R, N, K = _check_matmul(a8, ax, w4, e8, dtype, residual)
    _one_gpu("w4a8_matmul", a8, ax, w4, e8, residual)
    y = torch.empty((R, N), dtype=dtype, device=a8.device)
    if R == 0 or N == 0:
        return y
    p = _lib.W4A8LinearParams()
    p.R, p.N, p.K, p.dtype = R, N, K, _CODES[dtype]
    p.a8, p.a_stride = a8.data_ptr(), (a8.stride(0) if R > 1 else K)   # (one row: its stride is never used)
    p.ax, p.ax_stride = ax.data_ptr(), (ax.stride(0) if R > 1 else K // BLOCK)
    p.w4, p.w_stride = w4.data_ptr(), (w4.stride(0) if N > 1 else K // 2)
    p.e8, p.e_stride = e8.data_ptr(), (e8.stride(0) if N > 1 else K // BLOCK)
    if residual is not None:
        p.residual, p.residual_stride = residual.data_ptr(), (residual.stride(0) if R > 1 else N)
    p.y, p.y_stride = y.data_ptr(), y.stride(0)
    with _lib.on_device(a8.device):
        _lib.check(_lib.load().fat5_w4a8_linear(p, _lib.stream_ptr(a8.device)), "fat5_w4a8_linear")
    return y


@w4a8_matmul_op.register_fake
def _w4a8_matmul_fake(a8, ax, w4, e8, dtype, residual):
    return a8.new_empty((a8.shape[0], w4.shape[0]), dtype=dtype)


def _no_grad(what, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise RuntimeError(f"{what} is forward only: call it under torch.no_grad() / inference_mode(), or detach")


def quantize_activation_mxfp8(x, *, norm_weight=None, eps=1e-6, out=None, scales=None):
    """x (..., K) fp16 / bf16 on the GPU -> (a8 uint8 (..., K) of e4m3fn bytes, ax uint8 (..., K / 32) of e8m0 bytes), one scale per
    row and block of 32 consecutive k.  `norm_weight` (K,): the T5 RMSNorm of x (with `eps`) is applied first, inside the launch.
    `out` / `scales`: 2-D tensors to write into; by default new ones.  One launch."""
    _no_grad("quantize_activation_mxfp8", x, norm_weight)
    if x.dim() < 1 or x.shape[-1] % BLOCK != 0:
        raise ValueError(f"quantize_activation_mxfp8: x must be (..., K) with K a multiple of 32, got {tuple(x.shape)}")
    if x.dtype not in _CODES:
        raise ValueError(f"quantize_activation_mxfp8: x of dtype {x.dtype} (fp16 or bf16)")
    K, lead = x.shape[-1], tuple(x.shape[:-1])
    x2 = _rows(x, K)
    a8 = torch.empty((x2.shape[0], K), dtype=torch.uint8, device=x.device) if out is None else out
    ax = torch.empty((x2.shape[0], K // BLOCK), dtype=torch.uint8, device=x.device) if scales is None else scales
    _check_quantize(x2, norm_weight, float(eps), a8, ax)
    if not x.is_cuda:
        raise ValueError("quantize_activation_mxfp8: tensors must be on the GPU (there is no CPU path)")
    mx8_quantize(x2, norm_weight, float(eps), a8, ax)
    return (a8.view(lead + (K,)), ax.view(lead + (K // BLOCK,))) if out is None and scales is None else (a8, ax)


def w4a8_matmul(a8, ax, w4, e8, dtype, *, residual=None):
    """y (..., N) of `dtype` (fp16 / bf16) = dequant(a8, ax) @ dequant(w4, e8).T in ONE launch of the block-scaled MFMA kernel, for
    callers that hold quantised rows.  `residual` (..., N) of `dtype` is added to the rounded result, inside the launch."""
    _no_grad("w4a8_matmul", residual)
    if a8.dim() < 1 or ax.dim() != a8.dim() or w4.dim() != 2:
        raise ValueError(f"w4a8_matmul: a8 must be (..., K), ax (..., K / 32) and w4 (N, K / 2), got {tuple(a8.shape)}, {tuple(ax.shape)} "
                         f"and {tuple(w4.shape)}")
    N, K, lead = w4.shape[0], a8.shape[-1], tuple(a8.shape[:-1])
    if residual is not None and tuple(residual.shape) != lead + (N,):
        raise ValueError(f"w4a8_matmul: residual must be {lead + (N,)}, got {tuple(residual.shape)}")
    a2, s2 = a8.reshape(-1, K), ax.reshape(-1, ax.shape[-1])
    r2 = None if residual is None else _rows(residual, N)
    _check_matmul(a2, s2, w4, e8, dtype, r2)
    if not a8.is_cuda:
        raise ValueError("w4a8_matmul: tensors must be on the GPU (there is no CPU path)")
    return w4a8_matmul_op(a2, s2, w4, e8, dtype, r2).view(lead + (N,))


def w4a8_linear(x, w4, e8, *, norm_weight=None, eps=1e-6, residual=None):
    """y (..., N) = x (..., K) @ dequant(w4, e8).T with x quantised to MXFP8 on the way: `quantize_activation_mxfp8`, then
    `w4a8_matmul` -- two launches, no host read, graph-replayable.  `norm_weight` / `eps`: the T5 RMSNorm in front (in the
    quantiser's launch); `residual`: added behind (in the GEMM's launch)."""
    if w4.dim() != 2 or x.dim() < 1 or x.shape[-1] != 2 * w4.shape[1]:
        raise ValueError(f"w4a8_linear: x must be (..., K) and w4 (N, K / 2), got {tuple(x.shape)} and {tuple(w4.shape)}")
    _check_packed("w4a8_linear", w4, e8)
    a8, ax = quantize_activation_mxfp8(x, norm_weight=norm_weight, eps=eps)
    return w4a8_matmul(a8, ax, w4, e8, x.dtype, residual=residual)


# ------------------------------------------------------------------------------------------------- what the encoder stack reads
@dataclass
class EncoderLayerW4:
    """one encoder block's MXFP4 stacks, each a (w4, e8) pair"""
    qkv: Tuple[torch.Tensor, torch.Tensor]        # [Wq; Wk; Wv] (3 * inner, d_model)
    o: Tuple[torch.Tensor, torch.Tensor]          # (d_model, inner)
    wi: Tuple[torch.Tensor, torch.Tensor]         # [wi_0; wi_1] (2 * d_ff, d_model), or wi (d_ff, d_model) without a gate
    wo: Tuple[torch.Tensor, torch.Tensor]         # (d_model, d_ff)


@dataclass
class EncoderW4:
    layers: List[EncoderLayerW4]
    key: tuple = field(default=(), repr=False)    # (data_ptr, _version) of every source weight, in order


def _sources(stack):
    blocks = []
    for blk in stack.block:
        sa, ff = blk.self_attention_layer.self_attention, blk.ff_layer
        wi = [ff.act.wi_0.weight, ff.act.wi_1.weight] if ff.act.glu else [ff.act.wi.weight]
        blocks.append(([sa.Wq.weight, sa.Wk.weight, sa.Wv.weight], [sa.o.weight], wi, [ff.wo.weight]))
    return blocks


def check_encoder_weight_dtype(weight_dtype, what="generate"):
    """None or "mxfp4" -> the format of the encoder weights (None: the 16-bit parameters); host only"""
    if weight_dtype is not None and weight_dtype != "mxfp4":
        raise ValueError(f"{what}: encoder weight dtype {weight_dtype!r} (None or 'mxfp4')")
    return weight_dtype


def check_encoder_weights_mxfp4(model, what="generate"):
    """host-only: an encoder the MXFP4-weight stack can run -- 16-bit weights of one dtype and shapes inside the format's contract"""
    stack = model.encoder
    blocks = _sources(stack)
    every = [w for b in blocks for ws in b for w in ws]
    norms = [ln.weight for blk in stack.block for ln in (blk.self_attention_layer.layer_norm, blk.ff_layer.layer_norm)]
    dt = every[0].dtype
    if dt not in _CODES or any(w.dtype != dt for w in every + norms + [stack.embed_tokens.weight, stack.final_layer_norm.weight]):
        raise ValueError(f"{what}: weight_dtype='mxfp4' needs an encoder whose weights are fp16 or bf16 (one dtype; the activations "
                         f"keep it), got {sorted({str(w.dtype) for w in every + norms})}: convert the model (model.bfloat16()), an "
                         "fp32 model under autocast is not supported")
    for b in blocks:
        for ws in b:
            check_shape(sum(w.shape[0] for w in ws), ws[0].shape[1], f"{what}: weight_dtype='mxfp4'")
            if any(w.shape[0] % 8 != 0 for w in ws):
                raise ValueError(f"{what}: weight_dtype='mxfp4': every stacked weight needs a multiple of 8 rows")


def encoder_weights_mxfp4(model, what="generate"):
    """the model's quantised encoder weights, checked (host only); ValueError before `quantize_encoder_weights_mxfp4` built them"""
    check_encoder_weights_mxfp4(model, what)
    built = getattr(model, "_w4_encoder", None)
    if built is None:
        raise ValueError(f"{what}: weight_dtype='mxfp4' needs the encoder's MXFP4 weights: call model.quantize_encoder_weights_mxfp4() "
                         "first")
    return built


@torch.no_grad()
def quantize_encoder_weights_mxfp4(model):
    """The MXFP4 copies of the encoder weights (`model.encoder`, a FAT5ForConditionalGeneration's or an encoder-only model's): per
    block the stacks [Wq; Wk; Wv], o, [wi_0; wi_1] (or wi) and wo, each a (w4, e8) pair of N * K * 17 / 32 bytes from
    `quantize_weight_mxfp4`, built once and kept on the model; rebuilt when a source weight's storage or version changed.  The
    16-bit parameters stay as they are.  -> EncoderW4"""
    check_encoder_weights_mxfp4(model, "quantize_encoder_weights_mxfp4")
    blocks = _sources(model.encoder)
    key = tuple((w.data_ptr(), w._version) for b in blocks for ws in b for w in ws)
    cached = getattr(model, "_w4_encoder", None)
    if cached is not None and cached.key == key:
        return cached
    if not blocks[0][0][0].is_cuda:
        raise ValueError("quantize_encoder_weights_mxfp4: the model must be on the GPU (there is no CPU path)")
    built = EncoderW4([EncoderLayerW4(*(_stack(ws) for ws in b)) for b in blocks], key)
    model._w4_encoder = built   # (not a parameter, not a buffer: it never reaches a state_dict)
    return built


def encoder_forward_mxfp4(stack, weights, input_ids, packing=None, position_bias=None):
    """`stack(input_ids, packing=packing)` (fat5_step.FAT5Stack, an encoder) over the MXFP4 weights `weights` (EncoderW4): per block
    norm + quantise and the qkv GEMM, the attention operator as it is, quantise and the o GEMM with the residual behind, norm +
    quantise and the wi GEMM, the gated activation as it is, quantise and the wo GEMM with the residual behind; the final norm as
    it is.  `position_bias`: a dense bias handed to every block (a masked one; by default block 0 produces it).  Inference only."""
    if stack.training and torch.is_grad_enabled():
        raise RuntimeError("weight_dtype='mxfp4' is inference only: call model.eval(), or run under torch.no_grad()")
    from .attention_module import apply_rotary_emb_packed, unpack_heads
    from .gated_act import gated_act_packed
    with torch.no_grad():
        h = stack.embed_tokens(input_ids)
        for blk, lw in zip(stack.block, weights.layers):
            sa, ff = blk.self_attention_layer, blk.ff_layer
            att = sa.self_attention
            qkv = w4a8_linear(h, *lw.qkv, norm_weight=sa.layer_norm.weight, eps=sa.layer_norm.variance_epsilon)
            if packing is not None:
                att.packed_supported()
                att._packed_args(h, None, packing.cu_seqlens, packing.max_seqlen, None, None)
                q, k, v = (t[0].transpose(0, 1) for t in unpack_heads(qkv, 3, att.n_heads))
                out, position_bias = att._attend_packed(q, k, v, True, position_bias, packing.cu_seqlens, packing.max_seqlen, None, None)
            else:
                if att.rotary and position_bias is None:
                    (qkv,) = apply_rotary_emb_packed((qkv,), (3,), att.n_heads, *att._rotary_tables(qkv), nq=1,
                                                     interleaved=att.pe_encoding.interleaved)
                q, k, v = unpack_heads(qkv, 3, att.n_heads)
                out, position_bias = att._attend(q, k, v, h.dtype, None, True, position_bias)
            h = w4a8_linear(out, *lw.o, residual=h)
            g = w4a8_linear(h, *lw.wi, norm_weight=ff.layer_norm.weight, eps=ff.layer_norm.variance_epsilon)
            t = gated_act_packed(g, ff.act.act_name) if ff.act.glu else ff.act.act(g)
            h = w4a8_linear(t, *lw.wo, residual=h)
        return stack.final_layer_norm(h)
