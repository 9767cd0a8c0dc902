"""FIRE position bias on MI355X: the reference's `FIRE` module (src/utils/positional_encoding.py:341-417) with its producer -- an
MLP `Linear(1, W) -> ReLU -> Linear(W, H)` evaluated at every (query, key) pair -- as ONE HIP kernel each way (libfat5.so:
fat5_fire_fwd, fat5_fire_bwd).  Neither direction forms the (M, N, W) hidden layer the eager module materialises (537 MB at
W = 32, S = 2048): the forward writes the (H, M, N) bias and nothing else, the backward recomputes the hidden units and reduces
the six parameter gradients deterministically (fixed-order two-stage reduction in a caller-owned workspace, no float atomics).

  * `fire_bias(w1, b1, w2, b2, c, L_multiplier, init_L, M, N, eps, dtype)`: the (1, H, M, N) bias, differentiable in the five
    trainable parameters.
  * `FIRE(num_heads, mlp_width, init_c, init_L, eps)`: the reference module -- same parameter names and shapes (`mlp.0.*`,
    `mlp.2.*`, `c`, `init_L`, `L_multiplier`), so a reference state dict loads with strict=True; `forward(q, k, v)` on (B, S, H, D)
    tensors returns (q, k, v, bias) with the (1, H, S, S) bias in q's dtype, `compute_bias(M, N, device, dtype)` any (M, N).

Compute is fp32 whatever the parameters' dtype and the autocast state (the reference's `nn.Linear` layers would run in bf16 under
bf16 autocast; this matches its fp32 arithmetic instead).  Parameters may be fp32, fp16 or bf16; their gradients come back in
their own dtype.  There is no CPU fallback."""
import ctypes
from typing import List

import torch
from torch import nn

from . import _lib

__all__ = ["fire_bias", "FIRE"]


def _vec(dtype):
    return 4 if dtype == torch.float32 else 8


def _padded(N, dtype):
    """row length of the bias buffers: N rounded up to whole 16-byte vectors"""
    v = _vec(dtype)
    return (N + v - 1) // v * v


def _ready(t):
    """an (H, M, N) tensor the kernels take as it is: 16-byte aligned base, unit inner stride, outer strides in whole 16-byte vectors,
    and no two (h, m) rows overlapping -- an expanded gradient (stride 0, e.g. from the backward of `bias.sum(-2)`) is not"""
    v = _vec(t.dtype)
    H, M, N = t.shape
    sh, sm, sn = t.stride()
    return (sn == 1 and t.data_ptr() % 16 == 0 and sh % v == 0 and sm % v == 0 and sm >= N and (H == 1 or sh >= sm * M))


_NAMES = ("w1", "b1", "w2", "b2", "c", "L_multiplier", "init_L")


def _check_devices(tensors, device):
    """every parameter on `device`: the kernels dereference their raw pointers on the GPU, so a host tensor (e.g. a CPU `init_L`)
    or one on another GPU must be rejected before any launch"""
    for name, t in zip(_NAMES, tensors):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"FIRE: {name} must be a tensor, got {type(t).__name__}")
        if t.device != device:
            raise ValueError(f"FIRE: {name} is on {t.device}, the other parameters on {device}: all seven must be on one GPU")


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _params(w1, b1, w2, b2, c, lm, l0, M, N, eps, dtype):
    _check_devices((w1, b1, w2, b2, c, lm, l0), w2.device)
    for name, t in zip(_NAMES, (w1, b1, w2, b2, c, lm, l0)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"FIRE: the operators take fp32 contiguous parameters; {name} is {t.dtype}"
                             f"{'' if t.is_contiguous() else ', non-contiguous'}")
    if w2.dim() != 2:
        raise ValueError(f"FIRE: w2 must be (H, W), got {tuple(w2.shape)}")
    H, W = w2.shape
    if w1.numel() != W or b1.numel() != W or b2.numel() != H:
        raise ValueError(f"FIRE: w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, b2 {tuple(b2.shape)} do not match w2 {(H, W)}")
    if c.numel() != 1 or lm.numel() != 1 or l0.numel() != 1:
        raise ValueError("FIRE: c, L_multiplier and init_L are scalars")
    p = _lib.FireParams()
    p.M, p.N, p.H, p.W = int(M), int(N), int(H), int(W)
    p.dtype = _lib.dtype_code(dtype)
    p.eps = float(eps)
    p.w1, p.b1, p.w2, p.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    p.c, p.L_multiplier, p.init_L = c.data_ptr(), lm.data_ptr(), l0.data_ptr()
    return p


@torch.library.custom_op("fat5::fire_fwd", mutates_args=(), device_types="cuda")
def fire_fwd(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, c: torch.Tensor, lm: torch.Tensor,
             l0: torch.Tensor, M: int, N: int, eps: float, dtype: torch.dtype) -> torch.Tensor:
    """(H, M, N) bias in `dtype` from fp32 contiguous parameters (w1 (W,), b1 (W,), w2 (H, W), b2 (H,), c / lm / l0 (1,))"""
    # (rows padded to whole 16-byte vectors when N is not a multiple of one: the bias is then a slice, strides (M Np, Np, 1) --
    #  which the dense-bias attention takes as it is, with 16-byte aligned rows)
    out = torch.empty((w2.shape[0], M, _padded(N, dtype)), dtype=dtype, device=w2.device)[:, :, :N]
    p = _params(w1, b1, w2, b2, c, lm, l0, M, N, eps, dtype)
    p.bias = out.data_ptr()
    p.bias_stride[0], p.bias_stride[1] = out.stride(0), out.stride(1)
    with _lib.on_device(w2.device):
        _lib.check(_lib.load().fat5_fire_fwd(ctypes.byref(p), _lib.stream_ptr(w2.device)), "fat5_fire_fwd")
    return out


@torch.library.register_fake("fat5::fire_fwd")
def _fire_fwd_fake(w1, b1, w2, b2, c, lm, l0, M, N, eps, dtype):
    Np = _padded(N, dtype)
    return w2.new_empty_strided((w2.shape[0], M, N), (M * Np, Np, 1), dtype=dtype)


@torch.library.custom_op("fat5::fire_bwd", mutates_args=(), device_types="cuda")
def fire_bwd(dbias: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, c: torch.Tensor,
             lm: torch.Tensor, l0: torch.Tensor, eps: float) -> List[torch.Tensor]:
    """fp32 gradients [dw1 (W,), db1 (W,), dw2 (H, W), db2 (H,), dc (), dL_multiplier ()] from the (H, M, N) upstream gradient"""
    H, W = w2.shape
    _check_devices((w1, b1, w2, b2, c, lm, l0), w2.device)
    if dbias.device != w2.device or dbias.dim() != 3 or dbias.shape[0] != H:
        raise ValueError(f"FIRE: the bias gradient must be ({H}, M, N) on {w2.device}, got {tuple(dbias.shape)} on {dbias.device}")
    _, M, N = dbias.shape
    new = torch.zeros if M == 0 or N == 0 else torch.empty  # (the kernel writes every gradient; an empty bias has zero ones)
    dw1, db1, dw2, db2, dc, dlm = (new(shape, dtype=torch.float32, device=w2.device) for shape in ((W,), (W,), (H, W), (H,), (), ()))
    if M == 0 or N == 0:
        return [dw1, db1, dw2, db2, dc, dlm]
    if not _ready(dbias):
        dbias = dbias.contiguous()
        if not _ready(dbias):  # (N not a multiple of the vector: a padded copy)
            pad = torch.zeros((H, M, _padded(N, dbias.dtype)), dtype=dbias.dtype, device=dbias.device)
            pad[:, :, :N] = dbias
            dbias = pad[:, :, :N]
    p = _params(w1, b1, w2, b2, c, lm, l0, M, N, eps, dbias.dtype)
    p.dbias = dbias.data_ptr()
    p.bias_stride[0], p.bias_stride[1] = dbias.stride(0), dbias.stride(1)
    p.dw1, p.db1, p.dw2, p.db2, p.dc, p.dL_multiplier = (t.data_ptr() for t in (dw1, db1, dw2, db2, dc, dlm))
    lib = _lib.load()
    nbytes = lib.fat5_fire_bwd_workspace_bytes(ctypes.byref(p))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=w2.device)
    with _lib.on_device(w2.device):
        _lib.check(lib.fat5_fire_bwd(ctypes.byref(p), ws.data_ptr(), nbytes, _lib.stream_ptr(w2.device)), "fat5_fire_bwd")
    return [dw1, db1, dw2, db2, dc, dlm]


@torch.library.register_fake("fat5::fire_bwd")
def _fire_bwd_fake(dbias, w1, b1, w2, b2, c, lm, l0, eps):
    H, W = w2.shape
    e = lambda *shape: w2.new_empty(shape, dtype=torch.float32)  # noqa: E731
    return [e(W), e(W), e(H, W), e(H), e(), e()]


class FireBias(torch.autograd.Function):
    """(1, H, M, N) bias from the five trainable parameters (and init_L); one kernel launch forward, two backward"""

    @staticmethod
    def forward(ctx, w1, b1, w2, b2, c, lm, l0, M, N, eps, dtype):
        f = [_f32(t).reshape(-1) for t in (w1, b1, b2, c, lm, l0)]
        w2f = _f32(w2)
        ctx.save_for_backward(f[0], f[1], w2f, f[2], f[3], f[4], f[5])
        ctx.meta = (eps, [t.dtype for t in (w1, b1, w2, b2, c, lm)], [t.shape for t in (w1, b1, w2, b2, c, lm)])
        return fire_fwd(f[0], f[1], w2f, f[2], f[3], f[4], f[5], M, N, eps, dtype).unsqueeze(0)

    @staticmethod
    def backward(ctx, g):
        eps, dtypes, shapes = ctx.meta
        w1, b1, w2, b2, c, lm, l0 = ctx.saved_tensors
        grads = fire_bwd(g.squeeze(0), w1, b1, w2, b2, c, lm, l0, eps)
        out = [d.reshape(s).to(dt) for d, s, dt in zip(grads, shapes, dtypes)]
        return (*out, None, None, None, None, None)


def fire_bias(w1, b1, w2, b2, c, L_multiplier, init_L, M, N, eps=1e-6, dtype=torch.float32):
    """The FIRE bias (1, H, M, N) in `dtype` (fp32, fp16 or bf16); fp32 arithmetic.  w1 (W, 1) or (W,), b1 (W,), w2 (H, W),
    b2 (H,), c / L_multiplier / init_L scalars -- the reference's `mlp.0.weight`, `mlp.0.bias`, `mlp.2.weight`, `mlp.2.bias`, `c`,
    `L_multiplier`, `init_L`.  Differentiable in all but init_L (not trainable in the reference)."""
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"FIRE: bias dtype {dtype} (fp32, fp16 or bf16)")
    _check_devices((w1, b1, w2, b2, c, L_multiplier, init_L), w2.device)
    if not w2.is_cuda:
        raise RuntimeError("FIRE: the producer is a HIP kernel; the parameters must be on the GPU")
    return FireBias.apply(w1, b1, w2, b2, c, L_multiplier, init_L, int(M), int(N), float(eps), dtype)


class FIRE(nn.Module):
    """The reference's module (positional_encoding.py:341-417): same constructor and parameters.  `init_L` keeps the reference's
    type -- `torch.tensor(init_L)`, int64 for an integer such as the config's `relative_attention_max_distance` -- and is not
    trainable."""

    def __init__(self, num_heads=12, mlp_width=32, init_c=0.1, init_L=512., eps=1e-6):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(1, mlp_width), nn.ReLU(), nn.Linear(mlp_width, num_heads))
        self.c = nn.Parameter(torch.tensor(init_c))
        self.init_L = nn.Parameter(torch.tensor(init_L), requires_grad=False)
        self.L_multiplier = nn.Parameter(torch.tensor(1.0))
        self.eps = eps

    def compute_bias(self, M, N, device=None, dtype=torch.float32):
        """(1, H, M, N) bias: row i, column j as in the reference's (S, S) bias, for any M and N"""
        lin0, lin2 = self.mlp[0], self.mlp[2]
        dev = torch.device(device) if device is not None else lin2.weight.device
        if dev.type != lin2.weight.device.type or (dev.index is not None and dev.index != lin2.weight.device.index):
            raise ValueError(f"FIRE: parameters on {lin2.weight.device}, bias requested on {device}")
        return fire_bias(lin0.weight, lin0.bias, lin2.weight, lin2.bias, self.c, self.L_multiplier, self.init_L, M, N, self.eps, dtype)

    def forward(self, q, k=None, v=None):
        S = q.shape[1]
        return q, k, v, self.compute_bias(S, S, q.device, q.dtype)
