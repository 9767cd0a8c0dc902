"""Sequence pooling on MI355X (libfat5.so: fat5_seq_pool_fwd, fat5_seq_pool_bwd): per-token hidden states to one vector
per sequence, over padded or packed rows, one launch each way, no host read, no atomics.

    pooled, position, found = sequence_pool(hidden, mode, *, cu_seqlens=None, seqlens=None, input_ids=None, eos_token_id=1)

  * packed: hidden (total, d) with cu_seqlens (nseq + 1,) int32;  padded: hidden (B, L, d) with optional seqlens (B,) int32 (without
    them every row holds L tokens).  fp32, fp16 or bf16, unit inner stride (anything else is copied), any row stride.
  * mode "eos": the row of the last position whose id equals eos_token_id inside the sequence's own length -- the reference's
    pooling (custom_heads_flash_t5.py:180-185) without its host read; a sequence without one is pooled from its last valid token
    and flagged in `found`.  "first" / "last": the first / last valid row.  "mean": the mean over the valid rows, fp32 sums in an
    order the shape alone fixes, rounded once.
  * pooled (nseq, d) in hidden's dtype; position (nseq,) int32, the pooled row's index local to its sequence (-1 for "mean" and for
    an empty sequence); found (nseq,) int32 (0 for an empty sequence, and for "eos" without an EOS).  Differentiable in hidden.

Lengths are read and clamped on the device, so both launches can be captured in a graph and replayed with other lengths and ids.
There is no CPU fallback."""
import ctypes
from typing import Optional, Tuple

import torch

from . import _lib

__all__ = ["sequence_pool", "POOL_TILE", "POOL_SPLIT", "MODES"]

POOL_TILE = 64    # columns of one forward workgroup (pool_kernels.h)
POOL_SPLIT = 16   # token slices of one forward workgroup: token j of a sequence is summed into partial j mod POOL_SPLIT
MODES = {"eos": _lib.POOL_EOS, "first": _lib.POOL_FIRST, "last": _lib.POOL_LAST, "mean": _lib.POOL_MEAN}
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _layout(p, cu_seqlens, seqlens, nseq, L, total):
    p.nseq, p.L, p.total = nseq, L, total
    p.cu_seqlens = None if cu_seqlens is None else cu_seqlens.data_ptr()
    p.seqlens = None if seqlens is None else seqlens.data_ptr()


@torch.library.custom_op("fat5::seq_pool_fwd", mutates_args=(), device_types="cuda")
def seq_pool_fwd(hidden: torch.Tensor, cu_seqlens: Optional[torch.Tensor], seqlens: Optional[torch.Tensor],
                 input_ids: Optional[torch.Tensor], mode: int, eos_token_id: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """hidden (total, d) with cu_seqlens, or (B, L, d); unit inner stride; input_ids (total,) contiguous or (B, L) with unit column stride"""
    packed = cu_seqlens is not None
    nseq = cu_seqlens.numel() - 1 if packed else hidden.shape[0]
    d = hidden.shape[-1]
    dev = hidden.device
    pooled = torch.empty((nseq, d), dtype=hidden.dtype, device=dev)
    if nseq == 0 or d == 0:   # (nothing to launch: the flags of d = 0 say "empty")
        return pooled, torch.full((nseq,), -1, dtype=torch.int32, device=dev), torch.zeros(nseq, dtype=torch.int32, device=dev)
    position = torch.empty(nseq, dtype=torch.int32, device=dev)
    found = torch.empty(nseq, dtype=torch.int32, device=dev)
    p = _lib.SeqPoolParams()
    p.mode, p.dtype, p.d, p.eos_token_id = mode, _lib.dtype_code(hidden.dtype), d, eos_token_id
    _layout(p, cu_seqlens, seqlens, nseq, 0 if packed else hidden.shape[1], hidden.shape[0] if packed else 0)
    p.hidden = hidden.data_ptr()
    if packed:
        p.hidden_row_stride = hidden.stride(0)
    else:
        p.hidden_batch_stride, p.hidden_row_stride = hidden.stride(0), hidden.stride(1)
    if input_ids is not None:
        p.input_ids = input_ids.data_ptr()
        p.ids_batch_stride = 0 if packed else input_ids.stride(0)
    p.pooled, p.pooled_stride, p.position, p.found = pooled.data_ptr(), pooled.stride(0), position.data_ptr(), found.data_ptr()
    with _lib.on_device(dev):
        _lib.check(_lib.load().fat5_seq_pool_fwd(ctypes.byref(p), _lib.stream_ptr(dev)), "fat5_seq_pool_fwd")
    return pooled, position, found


@torch.library.register_fake("fat5::seq_pool_fwd")
def _seq_pool_fwd_fake(hidden, cu_seqlens, seqlens, input_ids, mode, eos_token_id):
    nseq = cu_seqlens.shape[0] - 1 if cu_seqlens is not None else hidden.shape[0]
    i32 = lambda: hidden.new_empty((nseq,), dtype=torch.int32)  # noqa: E731
    return hidden.new_empty((nseq, hidden.shape[-1])), i32(), i32()


@torch.library.custom_op("fat5::seq_pool_bwd", mutates_args=(), device_types="cuda")
def seq_pool_bwd(dpooled: torch.Tensor, position: torch.Tensor, cu_seqlens: Optional[torch.Tensor], seqlens: Optional[torch.Tensor],
                 mode: int, rows: int, L: int) -> torch.Tensor:
    """the whole dhidden in one launch: (rows, d) with cu_seqlens (rows = total), else (rows, L, d) (rows = B)"""
    packed = cu_seqlens is not None
    nseq, d = dpooled.shape
    dev = dpooled.device
    dhidden = torch.empty((rows, d) if packed else (rows, L, d), dtype=dpooled.dtype, device=dev)
    if dhidden.numel() == 0:
        return dhidden
    if dpooled.stride(1) != 1:
        dpooled = dpooled.contiguous()
    p = _lib.SeqPoolParams()
    p.mode, p.dtype, p.d = mode, _lib.dtype_code(dpooled.dtype), d
    _layout(p, cu_seqlens, seqlens, nseq, 0 if packed else L, rows if packed else 0)
    p.position, p.dpooled, p.dpooled_stride = position.data_ptr(), dpooled.data_ptr(), dpooled.stride(0)
    p.dhidden = dhidden.data_ptr()
    if packed:
        p.dhidden_row_stride = d
    else:
        p.dhidden_batch_stride, p.dhidden_row_stride = L * d, d
    with _lib.on_device(dev):
        _lib.check(_lib.load().fat5_seq_pool_bwd(ctypes.byref(p), _lib.stream_ptr(dev)), "fat5_seq_pool_bwd")
    return dhidden


@torch.library.register_fake("fat5::seq_pool_bwd")
def _seq_pool_bwd_fake(dpooled, position, cu_seqlens, seqlens, mode, rows, L):
    d = dpooled.shape[1]
    return dpooled.new_empty((rows, d) if cu_seqlens is not None else (rows, L, d))


class SequencePool(torch.autograd.Function):
    """(pooled, position, found); the backward is one launch that writes the whole dhidden from the saved positions"""

    @staticmethod
    def forward(ctx, hidden, cu_seqlens, seqlens, input_ids, mode, eos_token_id):
        pooled, position, found = seq_pool_fwd(hidden, cu_seqlens, seqlens, input_ids, mode, eos_token_id)
        ctx.save_for_backward(position, cu_seqlens, seqlens)
        ctx.meta = (mode, hidden.shape)
        ctx.mark_non_differentiable(position, found)
        return pooled, position, found

    @staticmethod
    def backward(ctx, dpooled, _dposition, _dfound):
        position, cu_seqlens, seqlens = ctx.saved_tensors
        mode, shape = ctx.meta
        dhidden = seq_pool_bwd(dpooled, position, cu_seqlens, seqlens, mode, shape[0], 0 if cu_seqlens is not None else shape[1])
        return dhidden, None, None, None, None, None


def _check_side(t, name, shape, dtype, dev):
    if not torch.is_tensor(t):
        raise ValueError(f"sequence_pool: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"sequence_pool: {name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"sequence_pool: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.device != dev:
        raise ValueError(f"sequence_pool: {name} is on {t.device}, hidden on {dev}")


def sequence_pool(hidden, mode, *, cu_seqlens=None, seqlens=None, input_ids=None, eos_token_id=1):
    """-> (pooled (nseq, d), position (nseq,) int32, found (nseq,) int32); see the module docstring.  ValueError, before any device
    work, for whatever the arguments themselves show to be wrong."""
    if mode not in MODES:
        raise ValueError(f"sequence_pool: mode {mode!r} (one of {', '.join(repr(m) for m in MODES)})")
    if not torch.is_tensor(hidden):
        raise ValueError(f"sequence_pool: hidden must be a tensor, got {type(hidden).__name__}")
    if hidden.dtype not in _DTYPES:
        raise ValueError(f"sequence_pool: hidden must be float32, float16 or bfloat16, got {hidden.dtype}")
    if not hidden.is_cuda:
        raise ValueError(f"sequence_pool: hidden is on {hidden.device}; the kernels run on the GPU and there is no CPU fallback")
    if cu_seqlens is not None and seqlens is not None:
        raise ValueError("sequence_pool: cu_seqlens (packed rows) and seqlens (padded rows) together: pass the one that describes hidden")
    dev = hidden.device
    if cu_seqlens is not None:
        if hidden.dim() != 2:
            raise ValueError(f"sequence_pool: with cu_seqlens hidden must be (total, d), got {tuple(hidden.shape)}")
        if not torch.is_tensor(cu_seqlens) or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
            raise ValueError("sequence_pool: cu_seqlens must be a (nseq + 1,) tensor")
        _check_side(cu_seqlens, "cu_seqlens", (cu_seqlens.numel(),), torch.int32, dev)
        cu_seqlens = cu_seqlens.contiguous()
        ids_shape = (hidden.shape[0],)
    else:
        if hidden.dim() != 3:
            raise ValueError(f"sequence_pool: without cu_seqlens hidden must be (B, L, d), got {tuple(hidden.shape)}")
        if seqlens is not None:
            _check_side(seqlens, "seqlens", (hidden.shape[0],), torch.int32, dev)
            seqlens = seqlens.contiguous()
        ids_shape = tuple(hidden.shape[:2])
    if input_ids is not None:
        _check_side(input_ids, "input_ids", ids_shape, torch.int64, dev)
        if input_ids.stride(-1) != 1:
            input_ids = input_ids.contiguous()
    elif mode == "eos":
        raise ValueError("sequence_pool: mode 'eos' needs input_ids")
    if not -(1 << 63) <= int(eos_token_id) < (1 << 63):
        raise ValueError(f"sequence_pool: eos_token_id {eos_token_id} is no int64")
    if hidden.shape[-1] > (1 << 22):
        raise ValueError(f"sequence_pool: d = {hidden.shape[-1]} above 2^22")
    if hidden.stride(-1) != 1:
        hidden = hidden.contiguous()
    return SequencePool.apply(hidden, cu_seqlens, seqlens, input_ids if mode == "eos" else None, MODES[mode], int(eos_token_id))
