"""Rotary position embedding (RoPE) on MI355X: the reference's `RotaryPositionalEncoding` (src/utils/positional_encoding.py:205-338)
with the rotation itself -- which the reference takes from the external flash_attn package (`apply_rotary_emb`, :5-8) -- as ONE HIP
kernel launch for q, k and v together (libfat5.so: fat5_rope_apply), forward and backward.

  * `apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, cu_seqlens=None, max_seqlen=None)`: flash_attn's argument
    order; x is (B, S, H, D), or (total, H, D) with cu_seqlens (positions count from each sequence's own start).
  * `apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k=None, sin_k=None, interleaved=False)`: q with (cos, sin), k and v with
    (cos_k, sin_k) (= (cos, sin) when None), one launch each way.
  * `rotary_tables(...)`: the tables, built on the host with the reference's torch arithmetic -- positions are `arange` in the
    tables' dtype, so in bf16 they are quantised above 256 exactly as the reference's are.
  * `RotaryPositionalEncoding`: the reference module (constructor, `inv_freq` / `scale` buffers, `forward(q, k, v) -> (q, k, v, None)`).

The rotated width is rd = 2 * cos.shape[-1]; columns from rd on are copied bit for bit.  fp32 arithmetic on the table values as
stored, one rounding per output element.  The backward is the same rotation with sin -> -sin on the same tables; nothing is saved.
There is no CPU fallback."""
import ctypes
from typing import List, Optional

import torch
from torch import nn

from . import _lib

__all__ = ["apply_rotary_emb", "apply_rotary_emb_qkv", "apply_rotary_emb_packed", "rotary_tables", "RotaryPositionalEncoding"]

_DIMS = (16, 32, 64, 128)


def _vec(dtype):
    return 4 if dtype == torch.float32 else 8


def _ready(t):
    """16-byte aligned base, unit inner stride, outer strides in whole 16-byte vectors"""
    v = _vec(t.dtype)
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % v == 0 for s in t.stride()[:-1])


def _strides(t, varlen):
    """[b, s, h] element strides of a (B, S, H, D) tensor, or [0, s, h] of a packed (total, H, D) one"""
    if varlen:
        return (0, t.stride(0), t.stride(1))
    return (t.stride(0), t.stride(1), t.stride(2))


def _consistent(xs, nq, varlen):
    """The kernel addresses every tensor with ONE batch, head count and head_dim, and bounds the tensors of a table group (q: [0, nq),
    k: [nq, n)) by ONE sequence length -- that of the group's first tensor.  A tensor of another length in the same group would be
    read and written past its end (or left partly unrotated), so unequal shapes are rejected here, before anything is launched."""
    if not 1 <= len(xs) <= 3 or not 0 <= nq <= len(xs):
        raise ValueError(f"rotary: {len(xs)} tensors with nq = {nq} (1 to 3 tensors, 0 <= nq <= their number)")
    x0 = xs[0]
    for x in xs:
        if x.dim() != (3 if varlen else 4):
            raise ValueError(f"rotary: expected {'(total, H, D)' if varlen else '(B, S, H, D)'} tensors, got {tuple(x.shape)}")
        if x.dtype != x0.dtype or x.device != x0.device or x.shape[-2:] != x0.shape[-2:]:
            raise ValueError("rotary: q / k / v must agree in dtype, device, heads and head_dim")
        if varlen and x.shape[0] != x0.shape[0]:
            raise ValueError("rotary: packed (total, H, D) tensors share cu_seqlens and must have the same number of tokens")
        if not varlen and x.shape[0] != x0.shape[0]:
            raise ValueError("rotary: q / k / v must agree in batch size")
    if not varlen:
        for name, grp in (("q", xs[:nq]), ("k / v", xs[nq:])):
            if any(x.shape[1] != grp[0].shape[1] for x in grp):
                raise ValueError(f"rotary: the {name} tensors rotate with one table pair and must share their sequence length, got "
                                 f"{[x.shape[1] for x in grp]}")


def _launch(xs, ys, cos, sin, cos_k, sin_k, nq, interleaved, conjugate, cu_seqlens, max_seqlen):
    """ONE fat5_rope_apply: ys[i] = rotate(xs[i]), tensors [0, nq) with (cos, sin), the rest with (cos_k, sin_k)"""
    x0 = xs[0]
    varlen = cu_seqlens is not None
    _consistent(xs, nq, varlen)
    for x, y in zip(xs, ys):
        if y.shape != x.shape:
            raise ValueError("rotary: every output must have its input's shape")
    p = _lib.RopeParams()
    p.H, p.D = x0.shape[-2], x0.shape[-1]
    if varlen:
        p.B = cu_seqlens.numel() - 1
        p.S = p.S_k = int(max_seqlen)
        p.cu_seqlens = cu_seqlens.data_ptr()
    else:
        p.B = x0.shape[0]
        p.S = xs[0].shape[1] if nq > 0 else xs[nq].shape[1]
        p.S_k = xs[nq].shape[1] if nq < len(xs) else p.S
    p.rd = 2 * cos.shape[-1]
    p.dtype = _lib.dtype_code(x0.dtype)
    p.interleaved, p.conjugate = int(bool(interleaved)), int(bool(conjugate))
    p.n_tensors, p.n_q = len(xs), nq
    p.table_rows = cos.shape[0]
    p.cos, p.sin = cos.data_ptr(), sin.data_ptr()
    if cos_k is not None:
        p.cos_k, p.sin_k = cos_k.data_ptr(), sin_k.data_ptr()
    for i, (x, y) in enumerate(zip(xs, ys)):
        p.x[i], p.y[i] = x.data_ptr(), y.data_ptr()
        for d, (a, b) in enumerate(zip(_strides(x, varlen), _strides(y, varlen))):
            p.x_stride[i][d], p.y_stride[i][d] = a, b
    with _lib.on_device(x0.device):
        _lib.check(_lib.load().fat5_rope_apply(ctypes.byref(p), _lib.stream_ptr(x0.device)), "fat5_rope_apply")


def _check(xs, nq, cos, sin, cos_k, sin_k, cu_seqlens, max_seqlen):
    x0 = xs[0]
    varlen = cu_seqlens is not None
    _consistent(xs, nq, varlen)
    if x0.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError("rotary: float32, float16 or bfloat16")
    if x0.shape[-1] not in _DIMS:
        raise ValueError(f"rotary: head_dim {x0.shape[-1]} (16, 32, 64 or 128)")
    for t in (cos, sin) + ((cos_k, sin_k) if cos_k is not None else ()):
        if t.dtype != x0.dtype or t.device != x0.device or t.dim() != 2 or t.shape != cos.shape or not t.is_contiguous():
            raise ValueError("rotary: cos / sin tables must be contiguous (rows, rd / 2) tensors of q's dtype and device, all of one shape")
    if (cos_k is None) != (sin_k is None):
        raise ValueError("rotary: cos_k and sin_k go together")
    if 2 * cos.shape[-1] > x0.shape[-1]:
        raise ValueError(f"rotary: rotated width {2 * cos.shape[-1]} > head_dim {x0.shape[-1]}")
    if varlen:
        if max_seqlen is None:
            raise ValueError("rotary: cu_seqlens needs max_seqlen")
        if cu_seqlens.dtype != torch.int32 or cu_seqlens.device != x0.device:
            raise ValueError("rotary: cu_seqlens must be int32 on the tensors' device")
        rows = int(max_seqlen)
    else:
        rows = max(x.shape[1] for x in xs)
    if rows > cos.shape[0]:
        raise ValueError(f"rotary: positions up to {rows - 1} beyond the table's {cos.shape[0]} rows")


def _ready_copy(x):
    return x if _ready(x) else x.contiguous()


@torch.library.custom_op("fat5::rotary", mutates_args=(), device_types="cuda")
def rotary(xs: List[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, cos_k: Optional[torch.Tensor], sin_k: Optional[torch.Tensor],
           nq: int, interleaved: bool, conjugate: bool, cu_seqlens: Optional[torch.Tensor], max_seqlen: int) -> List[torch.Tensor]:
    """out of place: fresh contiguous outputs"""
    xs = [_ready_copy(x) for x in xs]
    ys = [torch.empty(x.shape, dtype=x.dtype, device=x.device) for x in xs]
    _launch(xs, ys, cos, sin, cos_k, sin_k, nq, interleaved, conjugate, cu_seqlens, max_seqlen)
    return ys


@torch.library.register_fake("fat5::rotary")
def _rotary_fake(xs, cos, sin, cos_k, sin_k, nq, interleaved, conjugate, cu_seqlens, max_seqlen):
    return [torch.empty(x.shape, dtype=x.dtype, device=x.device) for x in xs]


@torch.library.custom_op("fat5::rotary_", mutates_args=("xs",), device_types="cuda")
def rotary_(xs: List[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, cos_k: Optional[torch.Tensor], sin_k: Optional[torch.Tensor],
            nq: int, interleaved: bool, conjugate: bool, cu_seqlens: Optional[torch.Tensor], max_seqlen: int) -> None:
    """in place"""
    for x in xs:
        if not _ready(x):
            raise ValueError("rotary (in place): tensors need a 16-byte aligned base, unit inner stride and whole-vector strides")
    _launch(xs, xs, cos, sin, cos_k, sin_k, nq, interleaved, conjugate, cu_seqlens, max_seqlen)


@torch.library.register_fake("fat5::rotary_")
def _rotary_inplace_fake(xs, cos, sin, cos_k, sin_k, nq, interleaved, conjugate, cu_seqlens, max_seqlen):
    return None


def _packed_head_dim(bufs, ns, H):
    """head_dim of packed buffers bufs[i] = (B, S_i, ns[i] * H * D), after checking that every buffer has exactly that width"""
    if len(bufs) != len(ns) or not bufs or any(n < 1 for n in ns) or sum(ns) > 3 or H < 1:
        raise ValueError("rotary (packed): one tensor count >= 1 per buffer, at most three tensors in all")
    if any(b.dim() != 3 for b in bufs):
        raise ValueError("rotary (packed): buffers are (B, S, n * H * D)")
    D = bufs[0].shape[-1] // (ns[0] * H)
    for b, n in zip(bufs, ns):
        if D < 1 or b.shape[-1] != n * H * D:
            raise ValueError(f"rotary (packed): buffer widths {[b.shape[-1] for b in bufs]} are not {list(ns)} x {H} heads x one head_dim")
    return D


def _packed_views(buf, n, H, D):
    """the n (B, S, H, D) head slices of a (B, S, n * H * D) buffer (no copy)"""
    B, S, _ = buf.shape
    sb, ss = buf.stride(0), buf.stride(1)
    off = buf.storage_offset()
    return [buf.as_strided((B, S, H, D), (sb, ss, D, 1), off + i * H * D) for i in range(n)]


@torch.library.custom_op("fat5::rotary_packed", mutates_args=(), device_types="cuda")
def rotary_packed(bufs: List[torch.Tensor], ns: List[int], H: int, cos: torch.Tensor, sin: torch.Tensor, cos_k: Optional[torch.Tensor],
                  sin_k: Optional[torch.Tensor], nq: int, interleaved: bool, conjugate: bool) -> List[torch.Tensor]:
    """packed projection outputs: bufs[i] is (B, S_i, ns[i] * H * D), slice j of it one tensor; fresh buffers of the same packing.
    All sum(ns) <= 3 tensors rotate in one launch, the first nq with (cos, sin)."""
    D = _packed_head_dim(bufs, ns, H)
    bufs = [b if (b.stride(-1) == 1 and b.data_ptr() % 16 == 0 and b.stride(0) % _vec(b.dtype) == 0 and b.stride(1) % _vec(b.dtype) == 0)
            else b.contiguous() for b in bufs]
    outs = [torch.empty(b.shape, dtype=b.dtype, device=b.device) for b in bufs]
    xs, ys = [], []
    for b, o, n in zip(bufs, outs, ns):
        xs += _packed_views(b, n, H, D)
        ys += _packed_views(o, n, H, D)
    _launch(xs, ys, cos, sin, cos_k, sin_k, nq, interleaved, conjugate, None, 0)
    return outs


@torch.library.register_fake("fat5::rotary_packed")
def _rotary_packed_fake(bufs, ns, H, cos, sin, cos_k, sin_k, nq, interleaved, conjugate):
    return [torch.empty(b.shape, dtype=b.dtype, device=b.device) for b in bufs]


class ApplyRotaryEmb(torch.autograd.Function):
    """rotate xs (q first) out of place or in place; the backward rotates the incoming gradients with sin -> -sin in one launch"""

    @staticmethod
    def forward(ctx, cos, sin, cos_k, sin_k, nq, interleaved, inplace, cu_seqlens, max_seqlen, *xs):
        ctx.tabs = (cos, sin, cos_k, sin_k)
        ctx.args = (nq, interleaved, cu_seqlens, max_seqlen)
        if inplace:
            rotary_(list(xs), cos, sin, cos_k, sin_k, nq, interleaved, False, cu_seqlens, max_seqlen)
            ctx.mark_dirty(*xs)
            return xs
        return tuple(rotary(list(xs), cos, sin, cos_k, sin_k, nq, interleaved, False, cu_seqlens, max_seqlen))

    @staticmethod
    def backward(ctx, *gs):
        cos, sin, cos_k, sin_k = ctx.tabs
        nq, interleaved, cu_seqlens, max_seqlen = ctx.args
        # (no None among gs: autograd materialises unused outputs' gradients as zeros of their own shape)
        dx = rotary(list(gs), cos, sin, cos_k, sin_k, nq, interleaved, True, cu_seqlens, max_seqlen)
        return (None,) * 9 + tuple(dx)


class ApplyRotaryEmbPacked(torch.autograd.Function):
    """packed projection outputs in, packed rotated buffers out (forward and backward one launch each); the gradient of each input
    buffer is again one packed buffer -- what the projection's backward GEMM takes"""

    @staticmethod
    def forward(ctx, ns, H, cos, sin, cos_k, sin_k, nq, interleaved, *bufs):
        ctx.args = (ns, H, cos, sin, cos_k, sin_k, nq, interleaved)
        return tuple(rotary_packed(list(bufs), list(ns), H, cos, sin, cos_k, sin_k, nq, interleaved, False))

    @staticmethod
    def backward(ctx, *gs):
        ns, H, cos, sin, cos_k, sin_k, nq, interleaved = ctx.args
        return (None,) * 8 + tuple(rotary_packed(list(gs), list(ns), H, cos, sin, cos_k, sin_k, nq, interleaved, True))


def apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, cu_seqlens=None, max_seqlen=None):
    """flash_attn.layers.rotary.apply_rotary_emb: x (B, S, H, D) or, with cu_seqlens, (total, H, D); cos / sin (rows, rd / 2).

    With cu_seqlens, max_seqlen must be the true maximum sequence length: it is what is checked against the table rows (cu_seqlens
    stays on the device, unread by the host), and the kernel rotates at most max_seqlen tokens of each sequence -- tokens of a longer
    sequence past that are left as they were in place, and undefined in the out-of-place result (flash_attn behaves the same)."""
    _check([x], 1, cos, sin, None, None, cu_seqlens, max_seqlen)
    ms = int(max_seqlen) if cu_seqlens is not None else 0
    return ApplyRotaryEmb.apply(cos, sin, None, None, 1, bool(interleaved), bool(inplace), cu_seqlens, ms, x)[0]


def apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k=None, sin_k=None, interleaved=False, cu_seqlens=None, max_seqlen=None):
    """q with (cos, sin), k and v with (cos_k, sin_k) -- (cos, sin) when None -- in one launch; (B, S, H, D) tensors (k and v may
    have another S than q: cross-attention), or packed (total, H, D) ones with cu_seqlens.  Returns new tensors (q, k, v)."""
    _check([q, k, v], 1, cos, sin, cos_k, sin_k, cu_seqlens, max_seqlen)
    ms = int(max_seqlen) if cu_seqlens is not None else 0
    return ApplyRotaryEmb.apply(cos, sin, cos_k, sin_k, 1, bool(interleaved), False, cu_seqlens, ms, q, k, v)


def apply_rotary_emb_packed(bufs, ns, n_heads, cos, sin, cos_k=None, sin_k=None, nq=1, interleaved=False):
    """projection outputs as they come from a stacked GEMM: bufs[i] (B, S_i, ns[i] * H * D) holds ns[i] tensors side by side
    (q | k | v, or q and k | v).  The first nq tensors rotate with (cos, sin), the rest with (cos_k, sin_k); one launch, and one
    for the backward, whose gradients are again packed buffers.  Returns the rotated buffers (same packing, contiguous)."""
    D = _packed_head_dim(bufs, ns, n_heads)
    views = [vw for b, n in zip(bufs, ns) for vw in _packed_views(b, n, n_heads, D)]
    _check(views, int(nq), cos, sin, cos_k, sin_k, None, None)
    return ApplyRotaryEmbPacked.apply(tuple(ns), int(n_heads), cos, sin, cos_k, sin_k, int(nq), bool(interleaved), *bufs)


def rotary_tables(dim, seqlen, base=10000.0, scale_base=None, dtype=torch.float32, device=None):
    """(cos, sin, cos_k, sin_k), each (seqlen, dim / 2) in `dtype` -- cos_k / sin_k None without xPos (scale_base None).

    The reference's arithmetic (positional_encoding.py:245-279), on the CPU so that the values do not depend on the device's
    math library: inv_freq = 1 / base ** (arange(0, dim, 2) / dim) in fp32, positions arange(seqlen) in `dtype` (quantised in
    bf16 / fp16 like the reference's), freqs = outer(positions, inv_freq) in fp32; xPos multiplies the q tables by
    scale ** power and divides the k tables by it, in fp32, before the rounding to `dtype`."""
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
    t = torch.arange(seqlen, dtype=dtype)
    freqs = torch.outer(t, inv_freq)
    if scale_base is None:
        tabs = (torch.cos(freqs).to(dtype), torch.sin(freqs).to(dtype), None, None)
    else:
        scale = (torch.arange(0, dim, 2, dtype=torch.float32) + 0.4 * dim) / (1.4 * dim)
        power = (torch.arange(seqlen, dtype=torch.float32) - seqlen // 2) / scale_base
        sc = scale ** power[:, None]
        c, s = torch.cos(freqs), torch.sin(freqs)
        tabs = ((c * sc).to(dtype), (s * sc).to(dtype), (c / sc).to(dtype), (s / sc).to(dtype))
    return tuple(None if t is None else t.to(device) for t in tabs)


class RotaryPositionalEncoding(nn.Module):
    """The reference's module (positional_encoding.py:205-338): same constructor, buffers `inv_freq` and `scale` (xPos), tables
    of `max_sequence_length` rows in q's dtype built on the first forward.

    `forward(q, k, v)` on (B, S, H, D) tensors returns (q, k, v, None): q rotated with (cos, sin), k AND v with (cos_k, sin_k)
    -- (cos, sin) without xPos.  Rotating v is unusual, but it is what the reference module does (:331-336) and its checkpoints
    were trained that way.  One kernel launch forward, one backward; the results are new tensors (the reference rotates q in
    place: same values).  `randomized_position` is stored and, as in the reference, not used by the forward.  `forward(q)` alone
    rotates q alone: the reference's one- and two-argument calls take packed (B, S, 3|2, H, D) q|k|v / k|v tensors instead
    (:299-321); 5-D tensors are rejected here (for packed projections: `apply_rotary_emb_packed`)."""

    def __init__(self, dim, max_sequence_length, base=10000.0, interleaved=False, scale_base=None, randomized_position=False):
        super().__init__()
        if dim <= 0 or dim % 2:
            raise ValueError(f"RotaryPositionalEncoding: dim {dim} must be even and positive")
        self.max_sequence_length = max_sequence_length
        self.randomized_position = randomized_position
        self.dim, self.base, self.interleaved, self.scale_base = dim, base, interleaved, scale_base
        self.register_buffer("inv_freq", 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim)), persistent=False)
        scale = (torch.arange(0, dim, 2, dtype=torch.float32) + 0.4 * dim) / (1.4 * dim) if scale_base is not None else None
        self.register_buffer("scale", scale, persistent=False)
        self._cos_cached = self._sin_cached = self._cos_k_cached = self._sin_k_cached = None

    def tables(self, device, dtype):
        """(cos, sin, cos_k, sin_k) on `device` in `dtype`, built once (again only if the device or dtype changes)"""
        c = self._cos_cached
        if c is None or c.device != device or c.dtype != dtype:
            self._cos_cached, self._sin_cached, self._cos_k_cached, self._sin_k_cached = rotary_tables(
                self.dim, self.max_sequence_length, self.base, self.scale_base, dtype, device)
        return self._cos_cached, self._sin_cached, self._cos_k_cached, self._sin_k_cached

    def forward(self, q, k=None, v=None):
        cos, sin, cos_k, sin_k = self.tables(q.device, q.dtype)
        if k is None and v is None:
            return apply_rotary_emb(q, cos, sin, self.interleaved), k, v, None
        if k is None or v is None:
            raise ValueError("RotaryPositionalEncoding: pass q alone or q, k and v")
        q, k, v = apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k, sin_k, self.interleaved)
        return q, k, v, None
