"""Weight-only MXFP4 (OCP microscaling FP4) linear layers for cached decoding (include/fat5.h, "MXFP4 weights";
csrc/w4_kernels.h).

    w4, e8 = quantize_weight_mxfp4(W)                    # W (N, K) fp32 / fp16 / bf16 -> uint8 (N, K / 2), uint8 (N, K / 32)
    y = w4_linear(x, w4, e8)                             # x (..., K) fp16 / bf16 -> (..., N)
    y = w4_linear(x, w4, e8, norm_weight=g, eps=1e-6, residual=h)

`w4`: byte j of a row holds element 2 j in its low nibble and 2 j + 1 in its high one, a nibble being an e2m1 value (sign, two
exponent bits, one mantissa bit: 0, 0.5, 1, 1.5, 2, 3, 4, 6).  `e8`: one e8m0 byte per block of 32 consecutive k, 2^(byte - 127);
255 marks a block that held an inf or a NaN and makes its output column NaN.  The quantiser takes X = clamp(floor(log2 amax) - 2,
-13, 13) per block and rounds v * 2^-X to nearest even, saturating at 6, so every dequantised weight is exact in fp16 and bf16.
`w4_linear` is ONE launch of one MFMA kernel for every row count: y = round(sum_k xin * q * 2^X) with fp32 accumulation in an order
that depends on K alone (the same bits for any row count, on every run, under graph replay); `norm_weight` puts the T5 RMSNorm of x
in front (bit for bit `w4_linear(fast_rms_layernorm(x, g, eps), ...)`), `residual` adds it behind (bit for bit `residual +
w4_linear(...)`).  Shapes: K a multiple of 32 in [32, 16384], N a multiple of 8.

`quantize_decoder_weights_mxfp4(model)` builds, once per model, what a cached decoding step with `weight_dtype="mxfp4"` reads
(generation.py).  Forward only; there is no CPU path and no fallback."""
from typing import Optional

import torch

from . import _lib
from .w8 import DecoderW8, LayerW8, _row_ready, _rows, _sources, check_decoder_weights, source_key

BLOCK = 32              # (W4_BLOCK, csrc/w4_kernels.h): k of one scale byte
K_MIN, K_MAX = 32, 16384
ROW_TILE = 32           # (W4_ROWS): rows of one workgroup, two MFMA fragments of 16
COLS = 32               # (W4_COLS): output columns of one workgroup
K_CHUNK = 128           # (W4_KC): K elements one wave stages and multiplies at a time; four waves deal the chunks round-robin


def check_shape(N, K, what):
    """the contract's legal (N, K), host only"""
    if K % BLOCK != 0 or not K_MIN <= K <= K_MAX:
        raise ValueError(f"{what}: K = {K} (the weight's input width must be a multiple of 32 in [32, {K_MAX}])")
    if N % 8 != 0:
        raise ValueError(f"{what}: N = {N} (the weight's output width must be a multiple of 8)")


def _bytes_ready(t, mult):
    """a uint8 (rows, width) tensor the kernels address by rows: innermost stride 1, a row stride that is a multiple of `mult`"""
    return t.stride(1) == 1 and (t.shape[0] <= 1 or (t.stride(0) % mult == 0 and t.stride(0) >= t.shape[1]))


def _check_packed(what, w4, e8):
    """w4 (N, K / 2) and e8 (N, K / 32) of one weight -> (N, K)"""
    if w4.dim() != 2 or w4.dtype != torch.uint8 or e8.dim() != 2 or e8.dtype != torch.uint8:
        raise ValueError(f"{what}: w4 must be a uint8 (N, K / 2) and e8 a uint8 (N, K / 32) tensor (quantize_weight_mxfp4), got "
                         f"{w4.dtype} {tuple(w4.shape)} and {e8.dtype} {tuple(e8.shape)}")
    N, K = w4.shape[0], 2 * w4.shape[1]
    check_shape(N, K, what)
    if tuple(e8.shape) != (N, K // BLOCK):
        raise ValueError(f"{what}: e8 must be {(N, K // BLOCK)} for w4 {tuple(w4.shape)}, got {tuple(e8.shape)}")
    if N and (not _bytes_ready(w4, 16) or w4.data_ptr() % 16 != 0 or not _bytes_ready(e8, 1)):
        raise ValueError(f"{what}: w4 needs innermost stride 1, a 16-byte aligned base and a row stride that is a multiple of 16 bytes; "
                         "e8 innermost stride 1")
    return N, K


# ------------------------------------------------------------------------------------------------------------------ operators
@torch.library.custom_op("fat5::w4_quantize", mutates_args=("out", "scales"), device_types="cuda")
def w4_quantize(w: torch.Tensor, out: torch.Tensor, scales: torch.Tensor) -> None:
    """w (N, K) -> out (N, K / 2) nibbles, scales (N, K / 32) e8m0 bytes, in one launch (fat5_w4_quantize)"""
    _check_quantize(w, out, scales)
    if not w.is_cuda or out.device != w.device or scales.device != w.device:
        raise ValueError("quantize_weight_mxfp4: tensors must be on one GPU (there is no CPU path)")
    p = _lib.W4QuantParams()
    p.N, p.K = w.shape
    p.dtype = _lib.dtype_code(w.dtype)
    p.w, p.out, p.e8 = w.data_ptr(), out.data_ptr(), scales.data_ptr()
    p.w_stride = w.stride(0)
    p.out_stride = out.stride(0) if p.N > 1 else p.K // 2   # (one row: its stride is never used)
    p.e_stride = scales.stride(0) if p.N > 1 else p.K // BLOCK
    with _lib.on_device(w.device):
        _lib.check(_lib.load().fat5_w4_quantize(p, _lib.stream_ptr(w.device)), "fat5_w4_quantize")


@w4_quantize.register_fake
def _w4_quantize_fake(w, out, scales):
    return None


def _check_quantize(w, out, scales):
    what = "quantize_weight_mxfp4"
    if w.dim() != 2:
        raise ValueError(f"{what}: W must be (N, K), got {tuple(w.shape)}")
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: dtype {w.dtype} (fp32, fp16 or bf16)")
    check_shape(w.shape[0], w.shape[1], what)
    if out.dim() != 2 or tuple(out.shape) != (w.shape[0], w.shape[1] // 2):
        raise ValueError(f"{what}: out must be a uint8 {(w.shape[0], w.shape[1] // 2)} tensor, got {out.dtype} {tuple(out.shape)}")
    _check_packed(what, out, scales)
    if w.numel() and (w.stride(1) != 1 or w.stride(0) % 8 != 0 or w.data_ptr() % 16 != 0):
        raise ValueError(f"{what}: W needs innermost stride 1, a 16-byte aligned base and a row stride that is a multiple of 8")


def quantize_weight_mxfp4(W, out=None, scales=None):
    """Quantise a linear layer's weight W (N, K) (fp32, fp16 or bf16, on the GPU) -> (w4 uint8 (N, K / 2), e8 uint8 (N, K / 32)):
    e2m1 nibbles and one e8m0 scale byte per block of 32.  `out` / `scales`: tensors to write into (rows of a stack); by default
    new ones.  One launch."""
    if W.requires_grad and torch.is_grad_enabled():
        W = W.detach()
    if W.dim() == 2 and W.numel() and (W.stride(1) != 1 or W.stride(0) % 8 != 0 or W.data_ptr() % 16 != 0):
        W = W.contiguous()
    if out is None and W.dim() == 2:
        out = torch.empty((W.shape[0], W.shape[1] // 2), dtype=torch.uint8, device=W.device)
    if scales is None and W.dim() == 2:
        scales = torch.empty((W.shape[0], W.shape[1] // BLOCK), dtype=torch.uint8, device=W.device)
    _check_quantize(W, out, scales)
    if not W.is_cuda:
        raise ValueError("quantize_weight_mxfp4: tensors must be on the GPU (there is no CPU path)")
    w4_quantize(W, out, scales)
    return out, scales


@torch.library.custom_op("fat5::w4_linear", mutates_args=(), device_types="cuda")
def w4_linear_op(x: torch.Tensor, w4: torch.Tensor, e8: torch.Tensor, norm_weight: Optional[torch.Tensor], eps: float,
                 residual: Optional[torch.Tensor]) -> torch.Tensor:
    """x (R, K), w4 (N, K / 2), e8 (N, K / 32) -> (R, N) contiguous, in one launch (fat5_w4_linear)"""
    _check_linear(x, w4, e8, norm_weight, eps, residual)
    for t in (x, w4, e8, norm_weight, residual):
        if t is not None and (not t.is_cuda or t.device != x.device):
            raise ValueError("w4_linear: tensors must be on one GPU (there is no CPU path)")
    R, K = x.shape
    N = w4.shape[0]
    y = torch.empty((R, N), dtype=x.dtype, device=x.device)
    if R == 0 or N == 0:
        return y
    p = _lib.W4LinearParams()
    p.R, p.N, p.K = R, N, K
    p.dtype = _lib.dtype_code(x.dtype)
    p.x, p.x_stride = x.data_ptr(), (x.stride(0) if R > 1 else K)   # (one row: its stride is never used)
    p.w4, p.w_stride = w4.data_ptr(), (w4.stride(0) if N > 1 else K // 2)
    p.e8, p.e_stride = e8.data_ptr(), (e8.stride(0) if N > 1 else K // BLOCK)
    if norm_weight is not None:
        p.norm_weight, p.eps = norm_weight.data_ptr(), float(eps)
    if residual is not None:
        p.residual, p.residual_stride = residual.data_ptr(), (residual.stride(0) if R > 1 else N)
    p.y, p.y_stride = y.data_ptr(), y.stride(0)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().fat5_w4_linear(p, _lib.stream_ptr(x.device)), "fat5_w4_linear")
    return y


@w4_linear_op.register_fake
def _w4_linear_fake(x, w4, e8, norm_weight, eps, residual):
    return x.new_empty((x.shape[0], w4.shape[0]))


def _check_linear(x, w4, e8, norm_weight, eps, residual):
    what = "w4_linear"
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be (R, K) here, got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: x of dtype {x.dtype} (fp16 or bf16)")
    N, K = _check_packed(what, w4, e8)
    if x.shape[1] != K:
        raise ValueError(f"{what}: x has {x.shape[1]} columns, the weight K = {K}")
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


def w4_linear(x, w4, e8, *, norm_weight=None, eps=1e-6, residual=None):
    """y (..., N) = x (..., K) @ dequant(w4, e8).T in ONE launch, x fp16 / bf16 on the GPU, w4 / e8 from `quantize_weight_mxfp4`.
    `norm_weight` (K,) of x's dtype: the T5 RMSNorm of x (with `eps`) is applied first, inside the launch; `residual` (..., N) of
    x's dtype is added to the rounded result, inside the launch.  Both are invisible in the bits (see the module's text).  One
    MFMA kernel serves every row count."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, norm_weight, residual)):
        raise RuntimeError("w4_linear is forward only: call it under torch.no_grad() / inference_mode(), or detach")
    if x.dim() < 1 or w4.dim() != 2:
        raise ValueError(f"w4_linear: x must be (..., K) and w4 (N, K / 2), got {tuple(x.shape)} and {tuple(w4.shape)}")
    N, K = w4.shape[0], 2 * w4.shape[1]
    if x.shape[-1] != K:
        raise ValueError(f"w4_linear: x has {x.shape[-1]} columns, the weight K = {K}")
    lead = tuple(x.shape[:-1])
    if residual is not None and tuple(residual.shape) != lead + (N,):
        raise ValueError(f"w4_linear: residual must be {lead + (N,)}, got {tuple(residual.shape)}")
    x2 = _rows(x, K)
    r2 = None if residual is None else _rows(residual, N)
    _check_linear(x2, w4, e8, norm_weight, float(eps), r2)
    if not x.is_cuda:
        raise ValueError("w4_linear: tensors must be on the GPU (there is no CPU path)")
    return w4_linear_op(x2, w4, e8, norm_weight, float(eps), r2).view(lead + (N,))


# ------------------------------------------------------------------------------------------- what a cached decoding step reads
def _stack(ws):
    """[W ...] -> (w4, e8) of the row-wise concatenation, each weight quantised into its rows of the stack"""
    N, K = sum(w.shape[0] for w in ws), ws[0].shape[1]
    w4 = torch.empty((N, K // 2), dtype=torch.uint8, device=ws[0].device)
    e8 = torch.empty((N, K // BLOCK), dtype=torch.uint8, device=ws[0].device)
    n = 0
    for w in ws:
        quantize_weight_mxfp4(w.detach(), w4[n:n + w.shape[0]], e8[n:n + w.shape[0]])
        n += w.shape[0]
    return w4, e8


def check_decoder_weights_mxfp4(model, what="generate"):
    """host-only: a decoder the MXFP4-weight step can run (w8.check_decoder_weights with this format's shapes)"""
    check_decoder_weights(model, what, "mxfp4", check_shape)


@torch.no_grad()
def quantize_decoder_weights_mxfp4(model):
    """The MXFP4 copies of the decoder weights a cached step reads: the stacks of `w8.quantize_decoder_weights` (self-attention
    [Wq; Wk; Wv] and o, cross-attention Wq and o, [wi_0; wi_1] and wo per block, then lm_head), each a (w4, e8) pair of
    N * K * 17 / 32 bytes, built once and kept on the model; rebuilt when a source weight's storage or version changed.  The
    16-bit parameters stay as they are.  -> w8.DecoderW8 (its pairs are (w4, e8))"""
    check_decoder_weights_mxfp4(model, "quantize_decoder_weights_mxfp4")
    blocks, head = _sources(model)
    key = source_key(model)
    cached = getattr(model, "_w4_decoder", None)
    if cached is not None and cached.key == key:
        return cached
    if not head.is_cuda:
        raise ValueError("quantize_decoder_weights_mxfp4: the model must be on the GPU (there is no CPU path)")
    built = DecoderW8([LayerW8(*(_stack(ws) for ws in b)) for b in blocks], _stack([head]), key)
    model._w4_decoder = built   # (not a parameter, not a buffer: it never reaches a state_dict)
    return built
