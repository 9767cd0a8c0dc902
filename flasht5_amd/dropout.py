"""Dropout on MI355X with the mask recomputed, never stored (libfat5.so: fat5_dropout, fat5_dropout_add_rmsnorm_fwd / _bwd).

One call is described by (p, seed, step, site, elem_offset); include/fat5.h and DESIGN 4.21 state which elements it keeps.  `step`
is an int64 device tensor of one element that the kernels read on the device: a captured graph draws a new mask at every replay
once the counter behind it has moved, and a backward pass hands in the same tensor and gets the forward's mask back.

    dropout(x, p, seed, step, site, elem_offset=0)                        -> dropout(x)
    dropout_add(x, residual, p, seed, step, site)                          -> residual + dropout(x)
    dropout_add_rms_layernorm(h, delta, W, eps, p, seed, step, site)       -> (h + dropout(delta), rmsnorm(h + dropout(delta)) * W)

The last one is `fused_add_rms_layernorm` with the delta dropped out inside the same kernel: bit-identical to `dropout` followed
by it, one pass and one tensor less, and its backward writes the delta's gradient beside dx.  There is no CPU fallback, and the
C++ binding is not extended: these operators take the ctypes path."""
import ctypes
from typing import Optional, Tuple

import torch

from . import _lib

__all__ = ["dropout", "dropout_add", "dropout_add_rms_layernorm", "rank_key"]

_MASK64 = (1 << 64) - 1
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def rank_key(seed, rank):
    """the Philox key of data-parallel rank `rank`: seed + rank (mod 2^64), so that ranks do not share masks"""
    return (int(seed) + int(rank)) & _MASK64


def _signed(seed):
    """a 64-bit key as the int64 an operator schema carries"""
    seed = int(seed) & _MASK64
    return seed - (1 << 64) if seed >> 63 else seed


def _desc(p, seed, step, site, elem_offset=0):
    d = _lib.DropoutDesc()
    d.seed, d.step, d.elem_offset, d.site, d.p = int(seed) & _MASK64, step.data_ptr(), int(elem_offset), int(site), float(p)
    return d


def _check_call(name, p, step, site, elem_offset, tensors):
    """everything the host can know before a launch"""
    p = float(p)
    if not 0.0 <= p < 1.0:   # (NaN fails both comparisons)
        raise ValueError(f"{name}: p = {p} outside [0, 1)")
    if not 0 <= int(site) < (1 << 32):
        raise ValueError(f"{name}: site {site} outside [0, 2^32)")
    if not 0 <= int(elem_offset) < (1 << 63):
        raise ValueError(f"{name}: elem_offset {elem_offset} outside [0, 2^63)")
    x = tensors[0][1]
    for what, t in tensors:
        if not torch.is_tensor(t):
            raise TypeError(f"{name}: {what} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"{name}: {what} is on {t.device}; the kernels run on the GPU and there is no CPU fallback")
        if t.device != x.device:
            raise ValueError(f"{name}: {what} is on {t.device}, {tensors[0][0]} on {x.device}")
    if x.dtype not in _DTYPES:
        raise TypeError(f"{name}: float32, float16 or bfloat16, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"{name}: {tensors[0][0]} needs a last dimension of at least one element, got {tuple(x.shape)}")
    if not torch.is_tensor(step) or step.dtype != torch.int64 or step.numel() != 1:
        raise ValueError(f"{name}: step must be an int64 tensor of one element (the kernels read it on the device)")
    if step.device != x.device:
        raise ValueError(f"{name}: step is on {step.device}, {tensors[0][0]} on {x.device}")
    return p


def _rows(t):
    """(rows, n) view with unit inner stride (a copy only when needed)"""
    t2 = t if t.dim() == 2 else t.reshape(-1, t.shape[-1])
    if t2.stride(-1) != 1:
        t2 = t2.contiguous()
    return t2


@torch.library.custom_op("fat5::dropout_fwd", mutates_args=(), device_types="cuda")
def dropout_fwd(x: torch.Tensor, residual: Optional[torch.Tensor], p: float, seed: int, step: torch.Tensor, site: int,
                elem_offset: int) -> torch.Tensor:
    """dropout(x), or residual + dropout(x); also the backward of both (applied to dy without a residual)"""
    a = _rows(x)
    r = None if residual is None else _rows(residual)
    out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    if a.shape[0]:
        d = _desc(p, seed, step, site, elem_offset)
        with _lib.on_device(a.device):
            _lib.check(_lib.load().fat5_dropout(a.data_ptr(), None if r is None else r.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1],
                                                a.stride(0), 0 if r is None else r.stride(0), out.stride(0), ctypes.byref(d),
                                                _lib.dtype_code(a.dtype), _lib.stream_ptr(a.device)), "fat5_dropout")
    return out.reshape(x.shape)


@torch.library.register_fake("fat5::dropout_fwd")
def _dropout_fwd_fake(x, residual, p, seed, step, site, elem_offset):
    return torch.empty(x.shape, dtype=x.dtype, device=x.device)


@torch.library.custom_op("fat5::dropout_add_rmsnorm_fwd", mutates_args=(), device_types="cuda")
def dropout_add_rmsnorm_fwd(X: torch.Tensor, D: torch.Tensor, weight: torch.Tensor, eps: float, p: float, seed: int, step: torch.Tensor,
                            site: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    M, N = X.shape
    X, D = _rows(X), _rows(D)
    weight = weight.contiguous()
    H = torch.empty((M, N), dtype=X.dtype, device=X.device)
    Y = torch.empty((M, N), dtype=X.dtype, device=X.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=X.device)
    if M == 0:
        return H, Y, rstd
    d = _desc(p, seed, step, site)
    with _lib.on_device(X.device):
        _lib.check(_lib.load().fat5_dropout_add_rmsnorm_fwd(
            X.data_ptr(), D.data_ptr(), weight.data_ptr(), H.data_ptr(), Y.data_ptr(), rstd.data_ptr(), M, N, X.stride(0), D.stride(0),
            H.stride(0), Y.stride(0), float(eps), ctypes.byref(d), _lib.dtype_code(X.dtype), _lib.dtype_code(weight.dtype),
            _lib.stream_ptr(X.device)), "fat5_dropout_add_rmsnorm_fwd")
    return H, Y, rstd


@torch.library.register_fake("fat5::dropout_add_rmsnorm_fwd")
def _dropout_add_rmsnorm_fwd_fake(X, D, weight, eps, p, seed, step, site):
    M, N = X.shape
    e = lambda: torch.empty((M, N), dtype=X.dtype, device=X.device)
    return e(), e(), torch.empty((M,), dtype=torch.float32, device=X.device)


@torch.library.custom_op("fat5::dropout_add_rmsnorm_bwd", mutates_args=(), device_types="cuda")
def dropout_add_rmsnorm_bwd(dy: torch.Tensor, h: torch.Tensor, weight: torch.Tensor, rstd: torch.Tensor, dres: torch.Tensor,
                            has_dres: bool, p: float, seed: int, step: torch.Tensor, site: int
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, ddelta, dw): dx and dw as fat5::add_rmsnorm_bwd, ddelta = dropout(dx) under the forward's mask, in the same pass"""
    M, N = h.shape
    dy = _rows(dy if dy.dtype == h.dtype else dy.to(h.dtype))
    if has_dres:
        dres = _rows(dres if dres.dtype == h.dtype else dres.to(h.dtype))
    weight = weight.contiguous()
    dx = torch.empty((M, N), dtype=h.dtype, device=h.device)
    dd = torch.empty((M, N), dtype=h.dtype, device=h.device)
    dw = torch.empty((N,), dtype=weight.dtype, device=weight.device)
    if M == 0:
        return dx, dd, dw.zero_()
    lib = _lib.load()
    nbytes = lib.fat5_rmsnorm_bwd_workspace_bytes(M, N)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=h.device)
    d = _desc(p, seed, step, site)
    with _lib.on_device(h.device):
        _lib.check(lib.fat5_dropout_add_rmsnorm_bwd(
            dy.data_ptr(), h.data_ptr(), weight.data_ptr(), rstd.data_ptr(), dres.data_ptr() if has_dres else None, dx.data_ptr(),
            dd.data_ptr(), dw.data_ptr(), M, N, dy.stride(0), h.stride(0), dres.stride(0) if has_dres else 0, dx.stride(0), dd.stride(0),
            ctypes.byref(d), _lib.dtype_code(h.dtype), _lib.dtype_code(weight.dtype), ws.data_ptr(), ws.numel(),
            _lib.stream_ptr(h.device)), "fat5_dropout_add_rmsnorm_bwd")
    return dx, dd, dw


@torch.library.register_fake("fat5::dropout_add_rmsnorm_bwd")
def _dropout_add_rmsnorm_bwd_fake(dy, h, weight, rstd, dres, has_dres, p, seed, step, site):
    e = lambda: torch.empty(h.shape, dtype=h.dtype, device=h.device)
    return e(), e(), torch.empty(weight.shape, dtype=weight.dtype, device=weight.device)


class Dropout(torch.autograd.Function):
    """dropout(x) (residual None) or residual + dropout(x); the step TENSOR is saved, not its value"""

    @staticmethod
    def forward(ctx, x, residual, p, seed, step, site, elem_offset):
        ctx.save_for_backward(step)
        ctx.call = (p, seed, site, elem_offset)
        return dropout_fwd(x, residual, p, seed, step, site, elem_offset)

    @staticmethod
    def backward(ctx, dy):
        (step,) = ctx.saved_tensors
        p, seed, site, elem_offset = ctx.call
        dx = dropout_fwd(dy, None, p, seed, step, site, elem_offset) if ctx.needs_input_grad[0] else None
        return dx, (dy if ctx.needs_input_grad[1] else None), None, None, None, None, None


class DropoutAddRMSLayernorm(torch.autograd.Function):
    """(h, y) = (x + dropout(d), rmsnorm(h) * W); grad x = rmsnorm_bwd_dx(dy) + dh, grad d = dropout(grad x)"""

    @staticmethod
    def forward(ctx, X, D, W, eps, p, seed, step, site):
        shape = X.shape
        h, y, rstd = dropout_add_rmsnorm_fwd(X.reshape(-1, shape[-1]), D.reshape(-1, shape[-1]), W, float(eps), p, seed, step, site)
        ctx.save_for_backward(h, W, rstd, step)
        ctx.shape = shape
        ctx.call = (p, seed, site)
        return h.reshape(shape), y.reshape(shape)

    @staticmethod
    def backward(ctx, dH, dY):
        h, W, rstd, step = ctx.saved_tensors
        p, seed, site = ctx.call
        n = h.shape[-1]
        if dY is None:  # only the residual stream is used downstream
            return dH, dropout_fwd(dH, None, p, seed, step, site, 0), None, None, None, None, None, None
        has = dH is not None
        dres = dH.reshape(-1, n) if has else h
        dx, dd, dw = dropout_add_rmsnorm_bwd(dY.reshape(-1, n), h, W, rstd, dres, has, p, seed, step, site)
        return dx.reshape(ctx.shape), dd.reshape(ctx.shape), dw, None, None, None, None, None


def dropout(x, p, seed, step, site, elem_offset=0):
    """dropout(x): element e = elem_offset + (row-major index of x) is kept iff its Philox uniform is >= p, kept elements are
    scaled by 1 / (1 - p); differentiable in x (the backward recomputes the mask)."""
    p = _check_call("dropout", p, step, site, elem_offset, [("x", x)])
    return Dropout.apply(x, None, p, _signed(seed), step, int(site), int(elem_offset))


def dropout_add(x, residual, p, seed, step, site):
    """residual + dropout(x) in one pass (the dropped x rounded to the dtype before the add: the bits of the two operations)."""
    p = _check_call("dropout_add", p, step, site, 0, [("x", x), ("residual", residual)])
    if residual.shape != x.shape or residual.dtype != x.dtype:
        raise ValueError(f"dropout_add: residual {tuple(residual.shape)} {residual.dtype} must match x {tuple(x.shape)} {x.dtype}")
    return Dropout.apply(x, residual, p, _signed(seed), step, int(site), 0)


def dropout_add_rms_layernorm(h, delta, W, eps, p, seed, step, site):
    """(h + dropout(delta), fast_rms_layernorm(h + dropout(delta), W, eps)) in one pass; differentiable in h, delta and W.
    Bit-identical to `dropout(delta, ...)` followed by `fused_add_rms_layernorm`."""
    p = _check_call("dropout_add_rms_layernorm", p, step, site, 0, [("h", h), ("delta", delta), ("W", W)])
    if delta.shape != h.shape or delta.dtype != h.dtype:
        raise ValueError(f"dropout_add_rms_layernorm: delta {tuple(delta.shape)} {delta.dtype} must match h {tuple(h.shape)} {h.dtype}")
    if W.dim() != 1 or W.shape[0] != h.shape[-1] or W.dtype not in _DTYPES:
        raise ValueError(f"dropout_add_rms_layernorm: W must be a ({h.shape[-1]},) floating-point vector, got {tuple(W.shape)} {W.dtype}")
    return DropoutAddRMSLayernorm.apply(h, delta, W, float(eps), p, _signed(seed), step, int(site))
