"""Decode attention against a KV cache: `flash_attn_with_kvcache` (flash_attn's layout and meaning) at seqlen_q = 1, on the
split-KV HIP kernel behind `fat5_attn_decode` (csrc/decode_kernels.h).

    o = flash_attn_with_kvcache(q, k_cache, v_cache, k=k_new, v=v_new, cache_seqlens=lens, rpe1d=rpe1d, rpe_radius=R)

q (B, 1, H, D); caches (B, L_cap, H, D), strided views accepted (a (B, H, L_cap, D) buffer's transpose works as it is); k / v the new
row (B, 1, H, D) or None.  `cache_seqlens` holds each batch element's length BEFORE the append and is not incremented: the caller
advances it.  With k / v the row is written into the caches at index cache_seqlens[b] inside the same launch.  The optional T5 bias
is the (H, 2R+1) fp32 generator of the linear-memory mode, bottom-right aligned: the query sits at position L_b - 1.

`flash_attn_with_kvcache_chunk` is the same call at seqlen_q = M (prompt prefill, speculative-decoding verification, M decoder rows
against the encoder's K / V): q (B, M, H, D), k / v (B, M, H, D) or None, on the chunk kernel behind `fat5_attn_decode_chunk`
(csrc/decode_chunk_kernels.h), causal inside the chunk with `causal=True`, the T5 bias bottom-right aligned per row.

FP8 KV caches: both calls take caches of `torch.float8_e4m3fn` together with `k_scale` / `v_scale`, fp32
(B, L_cap, H) tensors holding one scale per cache row and head (include/fat5.h states the format, tests/kvfp8_ref.py restates it).
An appended row is quantised inside the launch, bytes and scales written in place, and the query attends the quantised row.
`quantize_kv(x)` quantises existing rows (the encoder's K / V) in one launch.

Forward only: inputs that require grad under grad mode are rejected.  There is no eager fallback: CPU tensors are rejected."""
import math
from typing import List, Optional

import torch

from . import _lib


def _dec_view(t):
    """(B, 1, H, D) -> element strides [b, h]"""
    return (t.stride(0), t.stride(2))


FP8 = torch.float8_e4m3fn


def _set_scales(p, k_scale, v_scale):
    if k_scale is not None:
        p.cache_dtype = _lib.KV_FP8_E4M3
        p.k_scale, p.v_scale = k_scale.data_ptr(), v_scale.data_ptr()
        p.k_scale_stride[:] = k_scale.stride()
        p.v_scale_stride[:] = v_scale.stride()


def _check_scales(what, q, k_cache, v_cache, k_scale, v_scale):
    """the FP8-cache rules (host only) -> True in FP8 mode: float8_e4m3fn caches come with both scale tensors, and only they do"""
    fp8 = [t.dtype == FP8 for t in (k_cache, v_cache)]
    if not any(fp8) and k_scale is None and v_scale is None:
        return False
    if not all(fp8):
        raise ValueError(f"{what}: k_scale / v_scale go with float8_e4m3fn caches (both of them), got {k_cache.dtype} and "
                         f"{v_cache.dtype}")
    if k_scale is None or v_scale is None:
        raise ValueError(f"{what}: float8_e4m3fn caches need k_scale and v_scale (fp32 (B, L_cap, H): one scale per row and head)")
    for name, t, c in (("k_scale", k_scale, k_cache), ("v_scale", v_scale, v_cache)):
        want = tuple(c.shape[:3])
        if t.dtype != torch.float32 or tuple(t.shape) != want:
            raise ValueError(f"{what}: {name} must be an fp32 (B, L_cap, H) = {want} tensor, got {t.dtype} {tuple(t.shape)}")
        if any(st == 0 and n > 1 for st, n in zip(t.stride(), t.shape)):
            raise ValueError(f"{what}: {name} has a stride of 0 (an expanded tensor): it is written in place, every row needs its "
                             "own element")
        if t.device != c.device:
            raise ValueError(f"{what}: {name} on {t.device}, its cache on {c.device}")
    return True


def _params(q, k_cache, v_cache, k, v, cache_seqlens, o, lse, sm_scale, rpe1d, radius, num_splits, cache_batch_idx=None,
            cache_row_batch=None, k_scale=None, v_scale=None):
    B, _, H, D = q.shape
    p = _lib.DecodeParams() if k_scale is None else _lib.DecodeKV8Params()   # (the second: the first, then the scale fields)
    p.B, p.H, p.D = B, H, D
    p.dtype = _lib.dtype_code(q.dtype)
    p.capacity = k_cache.shape[1]
    p.N = k_cache.shape[1] if cache_seqlens is None else 0
    p.cache_seqlens = cache_seqlens.data_ptr() if cache_seqlens is not None else None
    p.sm_scale = float(sm_scale)
    if rpe1d is not None:
        p.bias_mode, p.rpe_radius, p.rpe1d = _lib.BIAS_RPE1D, int(radius), rpe1d.data_ptr()
    p.q, p.k_cache, p.v_cache, p.o = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), o.data_ptr()
    p.q_stride[:] = _dec_view(q)
    p.o_stride[:] = _dec_view(o)
    p.k_cache_stride[:] = (k_cache.stride(0), k_cache.stride(1), k_cache.stride(2))
    p.v_cache_stride[:] = (v_cache.stride(0), v_cache.stride(1), v_cache.stride(2))
    if k is not None:
        p.k_new, p.v_new = k.data_ptr(), v.data_ptr()
        p.k_new_stride[:] = _dec_view(k)
        p.v_new_stride[:] = _dec_view(v)
    p.lse = lse.data_ptr() if lse is not None else None
    p.num_splits = int(num_splits)
    if cache_batch_idx is not None or cache_row_batch is not None:
        p.cache_B = k_cache.shape[0]
        p.cache_batch_idx = cache_batch_idx.data_ptr() if cache_batch_idx is not None else None
        p.cache_row_batch = cache_row_batch.data_ptr() if cache_row_batch is not None else None
    _set_scales(p, k_scale, v_scale)
    return p


def _check_shapes(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, radius, cache_batch_idx=None, cache_row_batch=None, k_scale=None,
                  v_scale=None):
    """everything the host can check without touching a device: shapes, dtypes, strides, the bias generator against its radius"""
    if q.dim() != 4 or q.shape[1] != 1:
        raise ValueError(f"flash_attn_with_kvcache: q must be (B, 1, H, D) (one query row per step), got {tuple(q.shape)}")
    B, _, H, D = q.shape
    mapped = cache_batch_idx is not None or cache_row_batch is not None
    CB = k_cache.shape[0] if (mapped and k_cache.dim() == 4) else B  # (a map reads the caches' own batch count)
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dim() != 4 or t.shape[0] != CB or t.shape[2] != H or t.shape[3] != D:
            raise ValueError(f"flash_attn_with_kvcache: {name} must be (B, L_cap, H, D) = ({CB}, L_cap, {H}, {D}), got {tuple(t.shape)}")
    if k_cache.shape[1] != v_cache.shape[1]:
        raise ValueError("flash_attn_with_kvcache: k_cache and v_cache have different capacities")
    if cache_batch_idx is not None and cache_row_batch is not None:
        raise ValueError("flash_attn_with_kvcache: cache_batch_idx and cache_row_batch cannot be combined")
    if cache_batch_idx is not None:
        if k is not None:
            raise ValueError("flash_attn_with_kvcache: cache_batch_idx cannot be combined with an append (k / v)")
        if cache_batch_idx.dim() != 1 or cache_batch_idx.numel() != B:
            raise ValueError(f"flash_attn_with_kvcache: cache_batch_idx must hold {B} entries, got {tuple(cache_batch_idx.shape)}")
    if cache_row_batch is not None:
        if tuple(cache_row_batch.shape) != (B, k_cache.shape[1]):
            raise ValueError(f"flash_attn_with_kvcache: cache_row_batch must be (B, L_cap) = ({B}, {k_cache.shape[1]}), got "
                             f"{tuple(cache_row_batch.shape)}")
        if k is not None and CB < B:
            raise ValueError(f"flash_attn_with_kvcache: an append with cache_row_batch writes row b of the caches: they hold {CB} < {B}")
    if (k is None) != (v is None):
        raise ValueError("flash_attn_with_kvcache: pass both k and v, or neither")
    if k is not None:
        for name, t in (("k", k), ("v", v)):
            if tuple(t.shape) != (B, 1, H, D):
                raise ValueError(f"flash_attn_with_kvcache: {name} must be ({B}, 1, {H}, {D}), got {tuple(t.shape)}")
        if cache_seqlens is None:
            raise ValueError("flash_attn_with_kvcache: appending k / v needs cache_seqlens")
    fp8 = _check_scales("flash_attn_with_kvcache", q, k_cache, v_cache, k_scale, v_scale)
    for t in ([q] if fp8 else [q, k_cache, v_cache]) + ([k, v] if k is not None else []):
        if t.dtype != q.dtype:
            raise ValueError(f"flash_attn_with_kvcache: dtype mismatch ({t.dtype} vs q {q.dtype})")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"flash_attn_with_kvcache: dtype {q.dtype} (fp16 or bf16)")
    if D not in (64, 128):
        raise ValueError(f"flash_attn_with_kvcache: head_dim {D} (64 or 128)")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not _lib.kernel_ready(t):
            raise ValueError(f"flash_attn_with_kvcache: {name} needs innermost stride 1, a 16-byte aligned base and strides that are "
                             "multiples of 8 elements (it is written in place, so it cannot be copied)")
    if cache_seqlens is not None and (cache_seqlens.dim() != 1 or cache_seqlens.numel() != B):
        raise ValueError(f"flash_attn_with_kvcache: cache_seqlens must hold {B} lengths, got shape {tuple(cache_seqlens.shape)}")
    if rpe1d is not None:
        # (the kernel reads rpe1d[h][clamp(rel, -R, R) + R]: a generator narrower than 2R + 1 would be read past its end)
        if not 1 <= int(radius) <= 2048:
            raise ValueError(f"flash_attn_with_kvcache: rpe_radius {radius} outside 1..2048")
        if rpe1d.dtype != torch.float32 or tuple(rpe1d.shape) != (H, 2 * int(radius) + 1) or not rpe1d.is_contiguous():
            raise ValueError(f"flash_attn_with_kvcache: rpe1d must be a contiguous fp32 ({H}, 2 * rpe_radius + 1) = "
                             f"({H}, {2 * int(radius) + 1}) tensor, got {rpe1d.dtype} {tuple(rpe1d.shape)}")


def _check_devices(q, k_cache, v_cache, k, v, rpe1d, what="flash_attn_with_kvcache"):
    for t in (q, k_cache, v_cache, k, v, rpe1d):
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{what}: tensors must be on the GPU (there is no CPU path)")
        if t.device != q.device:
            raise ValueError(f"{what}: tensors on different devices")


def _check(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, radius, cache_batch_idx=None, cache_row_batch=None, k_scale=None,
           v_scale=None):
    _check_shapes(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, radius, cache_batch_idx, cache_row_batch, k_scale, v_scale)
    _check_devices(q, k_cache, v_cache, k, v, rpe1d)
    for name, t in (("cache_seqlens", cache_seqlens), ("cache_batch_idx", cache_batch_idx), ("cache_row_batch", cache_row_batch)):
        if t is not None and (t.dtype != torch.int32 or t.device != q.device or not t.is_contiguous()):
            raise ValueError(f"fat5::attn_decode: {name} must be a contiguous int32 tensor on {q.device}")


def _ready(t):
    return t if (t is None or _lib.kernel_ready(t)) else t.contiguous()


@torch.library.custom_op("fat5::attn_decode", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor], v: Optional[torch.Tensor],
                cache_seqlens: Optional[torch.Tensor], sm_scale: float, rpe1d: Optional[torch.Tensor], rpe_radius: int,
                return_lse: bool, num_splits: int, cache_batch_idx: Optional[torch.Tensor] = None,
                cache_row_batch: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """[o (B, 1, H, D) contiguous, lse (B, H, 1) fp32 (empty (0,) when return_lse is False)]; appends k / v to the caches"""
    return _attn_decode(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, rpe1d, rpe_radius, return_lse, num_splits, cache_batch_idx,
                        cache_row_batch)


def _attn_decode(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, rpe1d, rpe_radius, return_lse, num_splits, cache_batch_idx=None,
                 cache_row_batch=None, k_scale=None, v_scale=None):
    _check(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, rpe_radius, cache_batch_idx, cache_row_batch, k_scale, v_scale)
    q, k, v = _ready(q), _ready(k), _ready(v)
    B, _, H, D = q.shape
    o = torch.empty((B, 1, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, 1), dtype=torch.float32, device=q.device) if return_lse else q.new_empty((0,), dtype=torch.float32)
    p = _params(q, k_cache, v_cache, k, v, cache_seqlens, o, lse if return_lse else None, sm_scale, rpe1d, rpe_radius, num_splits,
                cache_batch_idx, cache_row_batch, k_scale, v_scale)
    lib = _lib.load()
    ws = None
    fp8 = k_scale is not None
    need = lib.fat5_attn_decode_workspace_bytes(p.base if fp8 else p)
    if need:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
    with _lib.on_device(q.device):
        if fp8:
            _lib.check(lib.fat5_attn_decode_kv8(p, _lib.stream_ptr(q.device)), "fat5_attn_decode_kv8")
        else:
            _lib.check(lib.fat5_attn_decode(p, _lib.stream_ptr(q.device)), "fat5_attn_decode")
    return [o, lse]


@attn_decode.register_fake
def _attn_decode_fake(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, rpe1d, rpe_radius, return_lse, num_splits, cache_batch_idx=None,
                      cache_row_batch=None):
    B, _, H, D = q.shape
    o = q.new_empty((B, 1, H, D))
    lse = q.new_empty((B, H, 1), dtype=torch.float32) if return_lse else q.new_empty((0,), dtype=torch.float32)
    return [o, lse]


# the same launch over FP8 caches: an operator of its own, so that the one above keeps its schema (the scales are written in place)
@torch.library.custom_op("fat5::attn_decode_fp8", mutates_args=("k_cache", "v_cache", "k_scale", "v_scale"), device_types="cuda")
def attn_decode_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                    k: Optional[torch.Tensor], v: Optional[torch.Tensor], cache_seqlens: Optional[torch.Tensor], sm_scale: float,
                    rpe1d: Optional[torch.Tensor], rpe_radius: int, return_lse: bool, num_splits: int,
                    cache_batch_idx: Optional[torch.Tensor], cache_row_batch: Optional[torch.Tensor]) -> List[torch.Tensor]:
    """attn_decode over float8_e4m3fn caches with their fp32 scales; appends k / v as bytes and scales"""
    return _attn_decode(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, rpe1d, rpe_radius, return_lse, num_splits, cache_batch_idx,
                        cache_row_batch, k_scale, v_scale)


@attn_decode_fp8.register_fake
def _attn_decode_fp8_fake(q, k_cache, v_cache, k_scale, v_scale, k, v, cache_seqlens, sm_scale, rpe1d, rpe_radius, return_lse, num_splits,
                          cache_batch_idx, cache_row_batch):
    return _attn_decode_fake(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, rpe1d, rpe_radius, return_lse, num_splits)


def _as_seqlens(cache_seqlens, device, name="cache_seqlens"):
    """int32 device lengths, converted the way `_as_cu` converts cu_seqlens -- except inside a graph capture, where a conversion
    would bake one value into the graph: there they must already be an int32 tensor on the device"""
    if cache_seqlens is None:
        return None
    ok = cache_seqlens.dtype == torch.int32 and cache_seqlens.device == device and cache_seqlens.is_contiguous()
    if ok:
        return cache_seqlens
    if torch.cuda.is_current_stream_capturing():
        raise ValueError(f"flash_attn_with_kvcache: inside a graph capture {name} must already be a contiguous int32 tensor on "
                         f"{device} (a conversion would fix its current value in the graph)")
    return cache_seqlens.to(device=device, dtype=torch.int32).contiguous()


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, cache_seqlens=None, softmax_scale=None, rpe1d=None, rpe_radius=0,
                            return_lse=False, num_splits=0, cache_batch_idx=None, cache_row_batch=None, k_scale=None, v_scale=None):
    """flash_attn's `flash_attn_with_kvcache` for one query row: returns o (B, 1, H, D), or (o, lse (B, H, 1) fp32) with
    return_lse.  An int cache_seqlens broadcasts over the batch.  num_splits 0 lets the library pick the key-range split from
    B, H and the cache capacity (never from the lengths: a captured graph stays valid while they grow).

    Indexed reads (beam search): `cache_batch_idx` (B,) int32 -- query row b reads batch element cache_batch_idx[b] of the caches
    (flash_attn's meaning; the caches may then hold another batch count); `cache_row_batch` (B, L_cap) int32 -- key row j of row
    b is read from batch element cache_row_batch[b, j] at row j, while an appended row still goes to element b.  Entries are
    clamped on the device to the caches' batch range.  Both must already be contiguous int32 tensors on the device.

    FP8 caches: `k_cache` / `v_cache` of torch.float8_e4m3fn with `k_scale` / `v_scale`, fp32 (B, L_cap, H) (any strides without
    a 0), one scale per cache row and head; q, k, v and o keep their fp16 / bf16 dtype.  The new row is quantised in the launch
    (bytes and scales written in place at cache_seqlens[b]) and the query attends the quantised row: o is a function of the cache
    contents after the call.  A scale follows its row through cache_batch_idx / cache_row_batch."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k_cache, v_cache, k, v, rpe1d)):
        raise RuntimeError("flash_attn_with_kvcache is forward only: call it under torch.no_grad() / inference_mode(), or detach")
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32)
    _check_shapes(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, rpe_radius, cache_batch_idx,  # (before the device checks: every
                  cache_row_batch, k_scale, v_scale)                                         #  shape error is reported as such)
    _check_devices(q, k_cache, v_cache, k, v, rpe1d)
    lens = _as_seqlens(cache_seqlens, q.device)
    scale = 1.0 / math.sqrt(q.shape[-1]) if softmax_scale is None else float(softmax_scale)
    if k_scale is not None:
        o, lse = attn_decode_fp8(q, k_cache, v_cache, k_scale, v_scale, k, v, lens, scale, rpe1d, int(rpe_radius), bool(return_lse),
                                 int(num_splits), cache_batch_idx, cache_row_batch)
    elif cache_batch_idx is None and cache_row_batch is None:
        o, lse = attn_decode(q, k_cache, v_cache, k, v, lens, scale, rpe1d, int(rpe_radius), bool(return_lse), int(num_splits))
    else:
        o, lse = attn_decode(q, k_cache, v_cache, k, v, lens, scale, rpe1d, int(rpe_radius), bool(return_lse), int(num_splits),
                             cache_batch_idx, cache_row_batch)
    return (o, lse) if return_lse else o


# ------------------------------------------------------------------------------------------------ M query rows per (batch, head)
def _chunk_params(q, k_cache, v_cache, k, v, cache_seqlens, o, lse, sm_scale, causal, rpe1d, radius, num_splits, chunk_seqlens=None,
                  k_scale=None, v_scale=None):
    B, M, H, D = q.shape
    p = _lib.DecodeChunkParams()
    p.B, p.H, p.M, p.D = B, H, M, D
    p.dtype = _lib.dtype_code(q.dtype)
    p.capacity = k_cache.shape[1]
    p.N = k_cache.shape[1] if cache_seqlens is None else 0
    p.causal = int(bool(causal))
    p.cache_seqlens = cache_seqlens.data_ptr() if cache_seqlens is not None else None
    p.sm_scale = float(sm_scale)
    if rpe1d is not None:
        p.bias_mode, p.rpe_radius, p.rpe1d = _lib.BIAS_RPE1D, int(radius), rpe1d.data_ptr()
    p.q, p.k_cache, p.v_cache, p.o = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), o.data_ptr()
    for name, t in (("q", q), ("o", o), ("k_cache", k_cache), ("v_cache", v_cache)):
        getattr(p, name + "_stride")[:] = t.stride()[:3]
    if k is not None:
        p.k_new, p.v_new = k.data_ptr(), v.data_ptr()
        p.k_new_stride[:] = k.stride()[:3]
        p.v_new_stride[:] = v.stride()[:3]
    p.lse = lse.data_ptr() if lse is not None else None
    p.num_splits = int(num_splits)
    p.chunk_seqlens = chunk_seqlens.data_ptr() if chunk_seqlens is not None else None
    _set_scales(p, k_scale, v_scale)
    return p


MAX_CHUNK = 1024  # (CHUNK_MAX_M, csrc/decode_chunk_kernels.h)


def _check_chunk_seqlens(chunk_seqlens, B, device=None, what="flash_attn_with_kvcache_chunk"):
    """chunk_seqlens' errors in their order: the shape, then the dtype, then (with `device`: the operator's strict form, which
    converts nothing) int32 on that device"""
    if chunk_seqlens is None:
        return
    if chunk_seqlens.dim() != 1 or chunk_seqlens.numel() != B:
        raise ValueError(f"{what}: chunk_seqlens must hold {B} lengths, got shape {tuple(chunk_seqlens.shape)}")
    if chunk_seqlens.dtype not in (torch.int32, torch.int64) or (device is not None and chunk_seqlens.dtype != torch.int32):
        raise TypeError(f"{what}: chunk_seqlens must be an int32{'' if device is not None else ' (or int64)'} tensor, got "
                        f"{chunk_seqlens.dtype}")
    if device is not None and (chunk_seqlens.device != device or not chunk_seqlens.is_contiguous()):
        raise ValueError(f"{what}: chunk_seqlens must be a contiguous int32 tensor on {device}, got one on {chunk_seqlens.device}")


def _chunk_check_shapes(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, radius, chunk_seqlens=None, k_scale=None, v_scale=None):
    """everything the host can check without touching a device"""
    what = "flash_attn_with_kvcache_chunk"
    if q.dim() != 4 or not 1 <= q.shape[1] <= MAX_CHUNK:
        raise ValueError(f"{what}: q must be (B, M, H, D) with 1 <= M <= {MAX_CHUNK}, got {tuple(q.shape)}")
    B, M, H, D = q.shape
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dim() != 4 or t.shape[0] != B or t.shape[2] != H or t.shape[3] != D:
            raise ValueError(f"{what}: {name} must be (B, L_cap, H, D) = ({B}, L_cap, {H}, {D}), got {tuple(t.shape)}")
    if k_cache.shape[1] != v_cache.shape[1]:
        raise ValueError(f"{what}: k_cache and v_cache have different capacities")
    if (k is None) != (v is None):
        raise ValueError(f"{what}: pass both k and v, or neither")
    if k is not None:
        for name, t in (("k", k), ("v", v)):
            if tuple(t.shape) != (B, M, H, D):
                raise ValueError(f"{what}: {name} must be ({B}, {M}, {H}, {D}), got {tuple(t.shape)}")
        if cache_seqlens is None:
            raise ValueError(f"{what}: appending k / v needs cache_seqlens")
    fp8 = _check_scales(what, q, k_cache, v_cache, k_scale, v_scale)
    for t in ([q] if fp8 else [q, k_cache, v_cache]) + ([k, v] if k is not None else []):
        if t.dtype != q.dtype:
            raise ValueError(f"{what}: dtype mismatch ({t.dtype} vs q {q.dtype})")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: dtype {q.dtype} (fp16 or bf16)")
    if D not in (64, 128):
        raise ValueError(f"{what}: head_dim {D} (64 or 128)")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not _lib.kernel_ready(t):
            raise ValueError(f"{what}: {name} needs innermost stride 1, a 16-byte aligned base and strides that are multiples of 8 "
                             "elements (it is written in place, so it cannot be copied)")
    if cache_seqlens is not None and (cache_seqlens.dim() != 1 or cache_seqlens.numel() != B):
        raise ValueError(f"{what}: cache_seqlens must hold {B} lengths, got shape {tuple(cache_seqlens.shape)}")
    if rpe1d is not None:
        if not 1 <= int(radius) <= 2048:
            raise ValueError(f"{what}: rpe_radius {radius} outside 1..2048")
        if rpe1d.dtype != torch.float32 or tuple(rpe1d.shape) != (H, 2 * int(radius) + 1) or not rpe1d.is_contiguous():
            raise ValueError(f"{what}: rpe1d must be a contiguous fp32 ({H}, 2 * rpe_radius + 1) = ({H}, {2 * int(radius) + 1}) tensor, "
                             f"got {rpe1d.dtype} {tuple(rpe1d.shape)}")
    _check_chunk_seqlens(chunk_seqlens, B)


@torch.library.custom_op("fat5::attn_decode_chunk", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def attn_decode_chunk(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor],
                      v: Optional[torch.Tensor], cache_seqlens: Optional[torch.Tensor], sm_scale: float, causal: bool,
                      rpe1d: Optional[torch.Tensor], rpe_radius: int, return_lse: bool, num_splits: int,
                      chunk_seqlens: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """[o (B, M, H, D) contiguous, lse (B, H, M) fp32 (empty (0,) when return_lse is False)]; appends k / v to the caches"""
    return _attn_decode_chunk(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, causal, rpe1d, rpe_radius, return_lse, num_splits,
                              chunk_seqlens)


def _attn_decode_chunk(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, causal, rpe1d, rpe_radius, return_lse, num_splits,
                       chunk_seqlens=None, k_scale=None, v_scale=None):
    _chunk_check_shapes(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, rpe_radius, chunk_seqlens, k_scale, v_scale)
    _check_devices(q, k_cache, v_cache, k, v, rpe1d, "flash_attn_with_kvcache_chunk")
    _check_chunk_seqlens(chunk_seqlens, q.shape[0], q.device, "fat5::attn_decode_chunk")
    if cache_seqlens is not None and (cache_seqlens.dtype != torch.int32 or cache_seqlens.device != q.device or
                                      not cache_seqlens.is_contiguous()):
        raise ValueError(f"fat5::attn_decode_chunk: cache_seqlens must be a contiguous int32 tensor on {q.device}")
    q, k, v = _ready(q), _ready(k), _ready(v)
    B, M, H, D = q.shape
    o = torch.empty((B, M, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, M), dtype=torch.float32, device=q.device) if return_lse else q.new_empty((0,), dtype=torch.float32)
    p = _chunk_params(q, k_cache, v_cache, k, v, cache_seqlens, o, lse if return_lse else None, sm_scale, causal, rpe1d, rpe_radius,
                      num_splits, chunk_seqlens, k_scale, v_scale)
    lib = _lib.load()
    ws = None
    need = lib.fat5_attn_decode_chunk_workspace_bytes(p)
    if need:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
    with _lib.on_device(q.device):
        _lib.check(lib.fat5_attn_decode_chunk(p, _lib.stream_ptr(q.device)), "fat5_attn_decode_chunk")
    return [o, lse]


@attn_decode_chunk.register_fake
def _attn_decode_chunk_fake(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, causal, rpe1d, rpe_radius, return_lse, num_splits,
                            chunk_seqlens=None):
    B, M, H, D = q.shape
    o = q.new_empty((B, M, H, D))
    lse = q.new_empty((B, H, M), dtype=torch.float32) if return_lse else q.new_empty((0,), dtype=torch.float32)
    return [o, lse]


@torch.library.custom_op("fat5::attn_decode_chunk_fp8", mutates_args=("k_cache", "v_cache", "k_scale", "v_scale"), device_types="cuda")
def attn_decode_chunk_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                          k: Optional[torch.Tensor], v: Optional[torch.Tensor], cache_seqlens: Optional[torch.Tensor], sm_scale: float,
                          causal: bool, rpe1d: Optional[torch.Tensor], rpe_radius: int, return_lse: bool, num_splits: int,
                          chunk_seqlens: Optional[torch.Tensor]) -> List[torch.Tensor]:
    """attn_decode_chunk over float8_e4m3fn caches with their fp32 scales; appends k / v as bytes and scales"""
    return _attn_decode_chunk(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, causal, rpe1d, rpe_radius, return_lse, num_splits,
                              chunk_seqlens, k_scale, v_scale)


@attn_decode_chunk_fp8.register_fake
def _attn_decode_chunk_fp8_fake(q, k_cache, v_cache, k_scale, v_scale, k, v, cache_seqlens, sm_scale, causal, rpe1d, rpe_radius, return_lse,
                                num_splits, chunk_seqlens):
    return _attn_decode_chunk_fake(q, k_cache, v_cache, k, v, cache_seqlens, sm_scale, causal, rpe1d, rpe_radius, return_lse, num_splits)


def flash_attn_with_kvcache_chunk(q, k_cache, v_cache, k=None, v=None, cache_seqlens=None, softmax_scale=None, causal=False, rpe1d=None,
                                  rpe_radius=0, return_lse=False, num_splits=0, chunk_seqlens=None, k_scale=None, v_scale=None):
    """flash_attn's `flash_attn_with_kvcache` for M query rows: returns o (B, M, H, D), or (o, lse (B, H, M) fp32) with return_lse.

    With k / v (B, M, H, D) the rows are written into the caches at cache_seqlens[b] .. cache_seqlens[b] + M - 1 inside the launch
    and query row i sits at position cache_seqlens[b] + i; without them the rows are bottom-right aligned, row i at
    L_b - M + i.  `causal=True`: row i sees the keys up to its own position.  The T5 bias is aligned per row:
    rpe1d[h][clamp(j - p_i, -R, R) + R].  Rows that no longer fit into the caches are not appended and sit at the last key;
    a row that sees no key gives o = 0, lse = -inf.  cache_seqlens is not incremented: the caller advances it by M.  An int
    cache_seqlens broadcasts over the batch.  num_splits 0 lets the library pick the key-range split from B, H, M and the capacity
    (never from the lengths: a captured graph stays valid while they grow).

    `chunk_seqlens` (B,) int32: a ragged chunk.  Batch element b brings m_b = clamp(chunk_seqlens[b], 0, M) rows; m_b stands for M
    above (m_b rows appended, the alignment without an append from L_b - m_b), query rows i >= m_b give o = 0 and lse = -inf and
    nothing at or past cache_seqlens[b] + m_b is written.  Read and clamped on the device; inside a graph capture it must already
    be a contiguous int32 tensor on the device, as cache_seqlens must.  None: every element brings M rows.

    FP8 caches: float8_e4m3fn `k_cache` / `v_cache` with fp32 (B, L_cap, H) `k_scale` / `v_scale`, as in
    flash_attn_with_kvcache: the M new rows are quantised in the launch and every query row attends the quantised rows."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k_cache, v_cache, k, v, rpe1d)):
        raise RuntimeError("flash_attn_with_kvcache_chunk is forward only: call it under torch.no_grad() / inference_mode(), or detach")
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32)
    _chunk_check_shapes(q, k_cache, v_cache, k, v, cache_seqlens, rpe1d, rpe_radius, chunk_seqlens, k_scale, v_scale)  # (before the device checks)
    _check_devices(q, k_cache, v_cache, k, v, rpe1d, "flash_attn_with_kvcache_chunk")
    lens = _as_seqlens(cache_seqlens, q.device)
    scale = 1.0 / math.sqrt(q.shape[-1]) if softmax_scale is None else float(softmax_scale)
    if k_scale is not None:
        o, lse = attn_decode_chunk_fp8(q, k_cache, v_cache, k_scale, v_scale, k, v, lens, scale, bool(causal), rpe1d, int(rpe_radius),
                                       bool(return_lse), int(num_splits), _as_seqlens(chunk_seqlens, q.device, "chunk_seqlens"))
    elif chunk_seqlens is None:
        o, lse = attn_decode_chunk(q, k_cache, v_cache, k, v, lens, scale, bool(causal), rpe1d, int(rpe_radius), bool(return_lse),
                                   int(num_splits))
    else:
        o, lse = attn_decode_chunk(q, k_cache, v_cache, k, v, lens, scale, bool(causal), rpe1d, int(rpe_radius), bool(return_lse),
                                   int(num_splits), _as_seqlens(chunk_seqlens, q.device, "chunk_seqlens"))
    return (o, lse) if return_lse else o


# ------------------------------------------------------------------------------------------------ the FP8 cache's row quantiser
@torch.library.custom_op("fat5::kv_quantize", mutates_args=("out", "scale"), device_types="cuda")
def kv_quantize(x: torch.Tensor, out: torch.Tensor, scale: torch.Tensor) -> None:
    """x (B, L, H, D) fp16 / bf16 -> out (B, L, H, D) float8_e4m3fn, scale (B, L, H) fp32, in one launch (fat5_kv_quantize)"""
    _check_quantize(x, out, scale)
    if not x.is_cuda or out.device != x.device or scale.device != x.device:
        raise ValueError("quantize_kv: tensors must be on one GPU (there is no CPU path)")
    p = _lib.KvQuantParams()
    p.B, p.L, p.H, p.D = x.shape
    p.dtype = _lib.dtype_code(x.dtype)
    p.x, p.out, p.scale = x.data_ptr(), out.data_ptr(), scale.data_ptr()
    p.x_stride[:] = x.stride()[:3]
    p.out_stride[:] = out.stride()[:3]
    p.scale_stride[:] = scale.stride()
    with _lib.on_device(x.device):
        _lib.check(_lib.load().fat5_kv_quantize(p, _lib.stream_ptr(x.device)), "fat5_kv_quantize")


@kv_quantize.register_fake
def _kv_quantize_fake(x, out, scale):
    return None


def _check_quantize(x, out, scale):
    what = "quantize_kv"
    if x.dim() != 4:
        raise ValueError(f"{what}: x must be (B, L, H, D), got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: dtype {x.dtype} (fp16 or bf16)")
    if x.shape[-1] not in (64, 128):
        raise ValueError(f"{what}: head_dim {x.shape[-1]} (64 or 128)")
    if out.dtype != FP8 or tuple(out.shape) != tuple(x.shape):
        raise ValueError(f"{what}: out must be a float8_e4m3fn {tuple(x.shape)} tensor, got {out.dtype} {tuple(out.shape)}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != tuple(x.shape[:3]):
        raise ValueError(f"{what}: scale must be an fp32 {tuple(x.shape[:3])} tensor, got {scale.dtype} {tuple(scale.shape)}")
    if x.numel() and not _lib.kernel_ready(out):
        raise ValueError(f"{what}: out needs innermost stride 1, a 16-byte aligned base and strides that are multiples of 8")


def quantize_kv(x, out=None, scale=None):
    """Quantise K or V rows for an FP8 cache -> (bytes, scale): x (B, L, H, D) fp16 / bf16 on the GPU (a (L, H, D) or (rows, D)
    tensor is taken as B = 1 / H = 1), any strides the kernels read; bytes float8_e4m3fn of x's shape, scale fp32 of x's shape
    without D: scale = amax|row| / 448 (1 for a zero row), bytes = RNE(clamp(x / scale, -448, 448)); a row with an inf or a NaN
    gets scale +inf and reads back as NaN (include/fat5.h, "FP8 KV cache").  `out` / `scale`: tensors to write into (views of a
    cache, any layout); by default new contiguous ones.  One launch, graph-capturable; no rows, no launch."""
    if x.dim() < 2 or x.dim() > 4:
        raise ValueError(f"quantize_kv: x must be (B, L, H, D), (L, H, D) or (rows, D), got {tuple(x.shape)}")
    if x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("quantize_kv is forward only: call it under torch.no_grad() / inference_mode(), or detach")
    shape = tuple(x.shape)
    x4 = x.reshape((1,) * (4 - x.dim()) + shape) if x.dim() == 4 else (x.unsqueeze(0) if x.dim() == 3 else x.unsqueeze(1).unsqueeze(0))
    if out is None:
        out = torch.empty(shape, dtype=FP8, device=x.device)
    if scale is None:
        scale = torch.empty(shape[:-1], dtype=torch.float32, device=x.device)
    o4, s4 = out.view(x4.shape) if out.dim() != 4 else out, scale.view(x4.shape[:3]) if scale.dim() != 3 else scale
    _check_quantize(x4, o4, s4)
    if not x.is_cuda:
        raise ValueError("quantize_kv: tensors must be on the GPU (there is no CPU path)")
    kv_quantize(_ready(x4), o4, s4)
    return out, scale
