"""Weight-only FP8 (e4m3fn) linear layers for cached decoding (include/fat5.h, "FP8 weights"; csrc/w8_kernels.h).

    w8, scale = quantize_weight(W)                       # W (N, K) fp32 / fp16 / bf16 -> float8_e4m3fn (N, K), fp32 (N,)
    y = w8_linear(x, w8, scale)                          # x (..., K) fp16 / bf16 -> (..., N)
    y = w8_linear(x, w8, scale, norm_weight=g, eps=1e-6, residual=h)

One scale per output row, by the rule of the FP8 KV cache (decode.quantize_kv): scale = amax|row| / 448 (1 for a zero row), bytes =
RNE(clamp(W / scale, -448, 448)); a row with an inf or a NaN gets scale +inf and makes its output column NaN.  `w8_linear` is ONE
launch: y = round(scale[n] * sum_k xin * w8) with fp32 accumulation in a fixed order (bitwise reproducible, graph replay included);
`norm_weight` puts the T5 RMSNorm of x in front (bit for bit `w8_linear(fast_rms_layernorm(x, g, eps), ...)`), `residual` adds it
behind (bit for bit `residual + w8_linear(...)`).  Shapes: K a multiple of 64 in [64, 16384], N a multiple of 8.

`quantize_decoder_weights(model)` builds, once per model, what a cached decoding step with `weight_dtype="fp8"` reads
(generation.py).  Forward only; there is no CPU path and no fallback."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from . import _lib

FP8 = torch.float8_e4m3fn
K_MAX = 16384           # (W8_K_MAX, csrc/w8_kernels.h)
COLS_PER_BLOCK = 16     # (W8_COLS)
ROW_TILE = 8            # (W8_RT)
K_TILE = 2048           # (W8_KT)
LANE_K = 512            # (W8_LANE_K): K elements a wave covers per step


def check_shape(N, K, what):
    """the contract's legal (N, K), host only"""
    if K % 64 != 0 or not 64 <= K <= K_MAX:
        raise ValueError(f"{what}: K = {K} (the weight's input width must be a multiple of 64 in [64, {K_MAX}])")
    if N % 8 != 0:
        raise ValueError(f"{what}: N = {N} (the weight's output width must be a multiple of 8)")


def check_weight_dtype(weight_dtype, what="generate"):
    """None, or "fp8" / "fp8_e4m3" -> whether the decoder weights are FP8"""
    if weight_dtype is None:
        return False
    if isinstance(weight_dtype, str) and weight_dtype in ("fp8", "fp8_e4m3"):
        return True
    raise ValueError(f"{what}: weight_dtype {weight_dtype!r} (None, 'fp8' or its alias 'fp8_e4m3')")


# ------------------------------------------------------------------------------------------------------------------ operators
@torch.library.custom_op("fat5::w8_quantize", mutates_args=("out", "scale"), device_types="cuda")
def w8_quantize(w: torch.Tensor, out: torch.Tensor, scale: torch.Tensor) -> None:
    """w (N, K) -> out (N, K) float8_e4m3fn, scale (N,) fp32, in one launch (fat5_w8_quantize)"""
    _check_quantize(w, out, scale)
    if not w.is_cuda or out.device != w.device or scale.device != w.device:
        raise ValueError("quantize_weight: tensors must be on one GPU (there is no CPU path)")
    p = _lib.W8QuantParams()
    p.N, p.K = w.shape
    p.dtype = _lib.dtype_code(w.dtype)
    p.w, p.out, p.scale = w.data_ptr(), out.data_ptr(), scale.data_ptr()
    p.w_stride, p.out_stride = w.stride(0), out.stride(0)
    with _lib.on_device(w.device):
        _lib.check(_lib.load().fat5_w8_quantize(p, _lib.stream_ptr(w.device)), "fat5_w8_quantize")


@w8_quantize.register_fake
def _w8_quantize_fake(w, out, scale):
    return None


def _check_quantize(w, out, scale):
    what = "quantize_weight"
    if w.dim() != 2:
        raise ValueError(f"{what}: W must be (N, K), got {tuple(w.shape)}")
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: dtype {w.dtype} (fp32, fp16 or bf16)")
    check_shape(w.shape[0], w.shape[1], what)
    if out.dtype != FP8 or tuple(out.shape) != tuple(w.shape):
        raise ValueError(f"{what}: out must be a float8_e4m3fn {tuple(w.shape)} tensor, got {out.dtype} {tuple(out.shape)}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (w.shape[0],) or not scale.is_contiguous():
        raise ValueError(f"{what}: scale must be a contiguous fp32 ({w.shape[0]},) tensor, got {scale.dtype} {tuple(scale.shape)}")
    for name, t in (("W", w), ("out", out)):
        if t.numel() and (t.stride(1) != 1 or t.stride(0) % 8 != 0 or t.data_ptr() % 16 != 0):
            raise ValueError(f"{what}: {name} needs innermost stride 1, a 16-byte aligned base and a row stride that is a multiple of 8")


def quantize_weight(W, out=None, scale=None):
    """Quantise a linear layer's weight W (N, K) (fp32, fp16 or bf16, on the GPU) -> (w8 float8_e4m3fn (N, K), scale fp32 (N,)),
    one scale per output row.  `out` / `scale`: tensors to write into (rows of a stack); by default new ones.  One launch."""
    if W.requires_grad and torch.is_grad_enabled():
        W = W.detach()
    if W.dim() == 2 and W.numel() and (W.stride(1) != 1 or W.stride(0) % 8 != 0 or W.data_ptr() % 16 != 0):
        W = W.contiguous()
    if out is None and W.dim() == 2:
        out = torch.empty(tuple(W.shape), dtype=FP8, device=W.device)
    if scale is None and W.dim() == 2:
        scale = torch.empty((W.shape[0],), dtype=torch.float32, device=W.device)
    _check_quantize(W, out, scale)
    if not W.is_cuda:
        raise ValueError("quantize_weight: tensors must be on the GPU (there is no CPU path)")
    w8_quantize(W, out, scale)
    return out, scale


@torch.library.custom_op("fat5::w8_linear", mutates_args=(), device_types="cuda")
def w8_linear_op(x: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor, norm_weight: Optional[torch.Tensor], eps: float,
                 residual: Optional[torch.Tensor]) -> torch.Tensor:
    """x (R, K), w8 (N, K) float8_e4m3fn, scale (N,) -> (R, N) contiguous, in one launch (fat5_w8_linear)"""
    _check_linear(x, w8, scale, norm_weight, eps, residual)
    for t in (x, w8, scale, norm_weight, residual):
        if t is not None and (not t.is_cuda or t.device != x.device):
            raise ValueError("w8_linear: tensors must be on one GPU (there is no CPU path)")
    R, K = x.shape
    N = w8.shape[0]
    y = torch.empty((R, N), dtype=x.dtype, device=x.device)
    if R == 0 or N == 0:
        return y
    p = _lib.W8LinearParams()
    p.R, p.N, p.K = R, N, K
    p.dtype = _lib.dtype_code(x.dtype)
    p.x, p.x_stride = x.data_ptr(), (x.stride(0) if R > 1 else K)   # (one row: its stride is never used)
    p.w8, p.w_stride, p.scale = w8.data_ptr(), w8.stride(0), scale.data_ptr()
    if norm_weight is not None:
        p.norm_weight, p.eps = norm_weight.data_ptr(), float(eps)
    if residual is not None:
        p.residual, p.residual_stride = residual.data_ptr(), (residual.stride(0) if R > 1 else N)
    p.y, p.y_stride = y.data_ptr(), y.stride(0)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().fat5_w8_linear(p, _lib.stream_ptr(x.device)), "fat5_w8_linear")
    return y


@w8_linear_op.register_fake
def _w8_linear_fake(x, w8, scale, norm_weight, eps, residual):
    return x.new_empty((x.shape[0], w8.shape[0]))


def _row_ready(t):
    """a (rows, width) view the kernel reads as it is: innermost stride 1, 16-byte aligned base, row stride a multiple of 8"""
    return t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or (t.stride(0) % 8 == 0 and t.stride(0) >= t.shape[1]))


def _check_linear(x, w8, scale, norm_weight, eps, residual):
    what = "w8_linear"
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be (R, K) here, got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: x of dtype {x.dtype} (fp16 or bf16)")
    if w8.dim() != 2 or w8.dtype != FP8:
        raise ValueError(f"{what}: w8 must be a float8_e4m3fn (N, K) tensor (quantize_weight), got {w8.dtype} {tuple(w8.shape)}")
    N, K = w8.shape
    check_shape(N, K, what)
    if x.shape[1] != K:
        raise ValueError(f"{what}: x has {x.shape[1]} columns, the weight K = {K}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (N,) or not scale.is_contiguous():
        raise ValueError(f"{what}: scale must be a contiguous fp32 ({N},) tensor, got {scale.dtype} {tuple(scale.shape)}")
    if N and (w8.stride(1) != 1 or w8.stride(0) % 8 != 0 or w8.stride(0) < K or w8.data_ptr() % 8 != 0):
        raise ValueError(f"{what}: w8 needs innermost stride 1, an 8-byte aligned base and a row stride that is a multiple of 8")
    if norm_weight is not None:
        if norm_weight.dtype != x.dtype or tuple(norm_weight.shape) != (K,) or not norm_weight.is_contiguous():
            raise ValueError(f"{what}: norm_weight must be a contiguous {x.dtype} ({K},) tensor, got {norm_weight.dtype} "
                             f"{tuple(norm_weight.shape)}")
        if norm_weight.data_ptr() % 16 != 0:
            raise ValueError(f"{what}: norm_weight needs a 16-byte aligned base")
        if not (eps >= 0.0 and eps < float("inf")):
            raise ValueError(f"{what}: eps {eps} (finite, >= 0)")
    if residual is not None and (residual.dtype != x.dtype or tuple(residual.shape) != (x.shape[0], N)):
        raise ValueError(f"{what}: residual must be a {x.dtype} {(x.shape[0], N)} tensor, got {residual.dtype} {tuple(residual.shape)}")
    for name, t in (("x", x), ("residual", residual)):
        if t is not None and t.numel() and not _row_ready(t):
            raise ValueError(f"{what}: {name} needs innermost stride 1, a 16-byte aligned base and a row stride that is a multiple of 8")


def _rows(t, width):
    """(..., width) -> a (rows, width) tensor the kernel reads: a view where the strides allow it"""
    t2 = t.reshape(-1, width)
    return t2 if (t2.numel() == 0 or _row_ready(t2)) else t2.contiguous()


def w8_linear(x, w8, scale, *, norm_weight=None, eps=1e-6, residual=None):
    """y (..., N) = x (..., K) @ (w8 * scale[:, None]).T in ONE launch, x fp16 / bf16 on the GPU, w8 / scale from `quantize_weight`.
    `norm_weight` (K,) of x's dtype: the T5 RMSNorm of x (with `eps`) is applied first, inside the launch; `residual` (..., N) of
    x's dtype is added to the rounded result, inside the launch.  Both are invisible in the bits (see the module's text)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, norm_weight, residual)):
        raise RuntimeError("w8_linear is forward only: call it under torch.no_grad() / inference_mode(), or detach")
    if x.dim() < 1 or w8.dim() != 2:
        raise ValueError(f"w8_linear: x must be (..., K) and w8 (N, K), got {tuple(x.shape)} and {tuple(w8.shape)}")
    N, K = w8.shape
    if x.shape[-1] != K:
        raise ValueError(f"w8_linear: x has {x.shape[-1]} columns, the weight K = {K}")
    lead = tuple(x.shape[:-1])
    if residual is not None and tuple(residual.shape) != lead + (N,):
        raise ValueError(f"w8_linear: residual must be {lead + (N,)}, got {tuple(residual.shape)}")
    x2 = _rows(x, K)
    r2 = None if residual is None else _rows(residual, N)
    _check_linear(x2, w8, scale, norm_weight, float(eps), r2)
    if not x.is_cuda:
        raise ValueError("w8_linear: tensors must be on the GPU (there is no CPU path)")
    return w8_linear_op(x2, w8, scale, norm_weight, float(eps), r2).view(lead + (N,))


# ------------------------------------------------------------------------------------------- what a cached decoding step reads
@dataclass
class LayerW8:
    """one decoder block's quantised stacks, each a (w8, scale) pair"""
    qkv: Tuple[torch.Tensor, torch.Tensor]        # self-attention [Wq; Wk; Wv] (3 * inner, d_model)
    self_o: Tuple[torch.Tensor, torch.Tensor]     # (d_model, inner)
    cross_q: Tuple[torch.Tensor, torch.Tensor]    # (inner, d_model)
    cross_o: Tuple[torch.Tensor, torch.Tensor]
    wi: Tuple[torch.Tensor, torch.Tensor]         # [wi_0; wi_1] (2 * d_ff, d_model), or wi (d_ff, d_model) without a gate
    wo: Tuple[torch.Tensor, torch.Tensor]         # (d_model, d_ff)


@dataclass
class DecoderW8:
    layers: List[LayerW8]
    lm_head: Tuple[torch.Tensor, torch.Tensor]
    key: tuple = field(default=(), repr=False)    # (data_ptr, _version) of every source weight, in order

    def pairs(self):
        """every quantised (w8, scale) pair, block by block, lm_head last (memory accounting, tests)"""
        out = []
        for lw in self.layers:
            out += [lw.qkv, lw.self_o, lw.cross_q, lw.cross_o, lw.wi, lw.wo]
        return out + [self.lm_head]


def _sources(model):
    """the decoder weights a cached step reads, per block as lists to stack, then lm_head"""
    blocks = []
    for blk in model.decoder.block:
        sa, ca, ff = blk.self_attention_layer.self_attention, blk.cross_attention_layer.cross_attention, blk.ff_layer
        wi = [ff.act.wi_0.weight, ff.act.wi_1.weight] if ff.act.glu else [ff.act.wi.weight]
        blocks.append(([sa.Wq.weight, sa.Wk.weight, sa.Wv.weight], [sa.o.weight], [ca.Wq.weight], [ca.o.weight], wi, [ff.wo.weight]))
    return blocks, model.lm_head.weight


def check_decoder_weights(model, what="generate"):
    """host-only: a decoder the FP8-weight step can run -- 16-bit weights of one dtype and shapes inside the contract"""
    blocks, head = _sources(model)
    every = [w for b in blocks for ws in b for w in ws] + [head]
    norms = [ln.weight for blk in model.decoder.block for ln in (blk.self_attention_layer.layer_norm, blk.cross_attention_layer.layer_norm,
                                                                   blk.ff_layer.layer_norm)] + [model.decoder.final_layer_norm.weight]
    dt = head.dtype
    if dt not in (torch.float16, torch.bfloat16) or any(w.dtype != dt for w in every + norms + [model.shared.weight]):
        raise ValueError(f"{what}: weight_dtype='fp8' needs a decoder whose weights are fp16 or bf16 (one dtype; the activations keep "
                         f"it), got {sorted({str(w.dtype) for w in every + norms})}: convert the model (model.bfloat16()), an "
                         "fp32 model under autocast is not supported")
    for b in blocks:
        for ws in b:
            check_shape(sum(w.shape[0] for w in ws), ws[0].shape[1], f"{what}: weight_dtype='fp8'")
            if any(w.shape[0] % 8 != 0 for w in ws):
                raise ValueError(f"{what}: weight_dtype='fp8': every stacked weight needs a multiple of 8 rows")
    check_shape(head.shape[0], head.shape[1], f"{what}: weight_dtype='fp8' (lm_head)")


def _stack(ws):
    """[W ...] -> (w8, scale) of the row-wise concatenation, each weight quantised into its rows of the stack"""
    N, K = sum(w.shape[0] for w in ws), ws[0].shape[1]
    w8 = torch.empty((N, K), dtype=FP8, device=ws[0].device)
    scale = torch.empty((N,), dtype=torch.float32, device=ws[0].device)
    n = 0
    for w in ws:
        quantize_weight(w.detach(), w8[n:n + w.shape[0]], scale[n:n + w.shape[0]])
        n += w.shape[0]
    return w8, scale


@torch.no_grad()
def quantize_decoder_weights(model):
    """The FP8 copies of the decoder weights a cached step reads (self-attention [Wq; Wk; Wv] and o, cross-attention Wq and o,
    [wi_0; wi_1] and wo per block, then lm_head), built once and kept on the model; rebuilt when a source weight's storage or
    version changed.  The 16-bit parameters stay as they are.  -> DecoderW8"""
    check_decoder_weights(model, "quantize_decoder_weights")
    blocks, head = _sources(model)
    key = tuple((w.data_ptr(), w._version) for b in blocks for ws in b for w in ws) + ((head.data_ptr(), head._version),)
    cached = getattr(model, "_w8_decoder", None)
    if cached is not None and cached.key == key:
        return cached
    if not head.is_cuda:
        raise ValueError("quantize_decoder_weights: the model must be on the GPU (there is no CPU path)")
    built = DecoderW8([LayerW8(*(_stack(ws) for ws in b)) for b in blocks], _stack([head]), key)
    model._w8_decoder = built   # (not a parameter, not a buffer: it never reaches a state_dict)
    return built
