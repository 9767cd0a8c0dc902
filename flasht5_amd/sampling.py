"""Temperature / top-k / top-p sampling of one token per logits row, in one HIP launch (`fat5_sample_logits`,
csrc/sample_kernels.h), with HF's warper order and meaning (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
a draw):

    tokens = sample_logits(logits, temperature=0.7, top_k=50, top_p=0.9, seed=s, offsets=positions)

The randomness is Philox4x32-10 keyed by `seed`, with the counter (offset + offsets[b], b): it lives in the call's arguments and in
device memory, never in torch's generator state, so a captured graph replays it exactly.  `uniforms` (B,) fp32 replaces the draw
(an exact-testing hook; callers may also bring their own randomness).  `return_aux` adds (B, 4) fp32 per row: the lowest kept x,
S_kept / S, u and the kept count (include/fat5.h).

Forward only, no CPU path: CPU tensors are rejected.  Rows that hold a NaN or +inf, or only -inf, give torch.argmax's index."""
from typing import List, Optional

import torch

from . import _lib

MAX_V = 1 << 20


def _u64(seed):
    """a Python int seed -> the int64 carrying its low 64 bits (the op's schema has no uint64)"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >= 1 << 63 else s


def check_args(temperature, top_k, top_p):
    """host-side validation shared with `generate` (before any device work)"""
    t = float(temperature)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be an int >= 0, got {top_k!r}")
    p = float(top_p)
    if not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")


def _check_shapes(logits, offsets, uniforms):
    if logits.dim() != 2:
        raise ValueError(f"sample_logits: logits must be (B, V), got {tuple(logits.shape)}")
    B, V = logits.shape
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"sample_logits: dtype {logits.dtype} (fp32, fp16 or bf16)")
    if not 1 <= V <= MAX_V:
        raise ValueError(f"sample_logits: V {V} outside [1, {MAX_V}]")
    for name, t in (("offsets", offsets), ("uniforms", uniforms)):
        if t is not None and (t.dim() != 1 or t.shape[0] != B):
            raise ValueError(f"sample_logits: {name} must be ({B},), got {tuple(t.shape)}")


def _check_devices(logits, offsets, uniforms):
    if not logits.is_cuda:
        raise ValueError("sample_logits: logits must be on the GPU (there is no CPU path)")
    for name, t, dt in (("offsets", offsets, torch.int32), ("uniforms", uniforms, torch.float32)):
        if t is not None and (t.device != logits.device or t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f"fat5::sample_logits: {name} must be a contiguous {dt} tensor on {logits.device}")


@torch.library.custom_op("fat5::sample_logits", mutates_args=(), device_types="cuda")
def sample_logits_op(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                     offsets: Optional[torch.Tensor], uniforms: Optional[torch.Tensor], return_aux: bool) -> List[torch.Tensor]:
    """[tokens (B,) int64, aux (B, 4) fp32 (empty (0,) when return_aux is False)]"""
    check_args(temperature, top_k, top_p)
    _check_shapes(logits, offsets, uniforms)
    _check_devices(logits, offsets, uniforms)
    B, V = logits.shape
    if logits.stride(-1) != 1 or (B > 1 and logits.stride(0) < V):  # (a row-broadcast view, stride(0) 0: one copy per row)
        logits = logits.contiguous()
    tokens = torch.empty((B,), dtype=torch.int64, device=logits.device)
    aux = torch.empty((B, 4), dtype=torch.float32, device=logits.device) if return_aux else logits.new_empty((0,), dtype=torch.float32)
    p = _lib.SampleParams()
    p.B, p.V, p.dtype, p.top_k = B, V, _lib.dtype_code(logits.dtype), int(top_k)
    p.logits, p.row_stride = logits.data_ptr(), logits.stride(0) if B > 1 else V
    p.temperature, p.top_p = float(temperature), float(top_p)
    p.seed, p.offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset)
    p.offsets = offsets.data_ptr() if offsets is not None else None
    p.uniforms = uniforms.data_ptr() if uniforms is not None else None
    p.tokens = tokens.data_ptr()
    p.aux = aux.data_ptr() if return_aux else None
    if B:
        with _lib.on_device(logits.device):
            _lib.check(_lib.load().fat5_sample_logits(p, _lib.stream_ptr(logits.device)), "fat5_sample_logits")
    return [tokens, aux]


@sample_logits_op.register_fake
def _sample_logits_fake(logits, temperature, top_k, top_p, seed, offset, offsets, uniforms, return_aux):
    B = logits.shape[0]
    tokens = logits.new_empty((B,), dtype=torch.int64)
    aux = logits.new_empty((B, 4), dtype=torch.float32) if return_aux else logits.new_empty((0,), dtype=torch.float32)
    return [tokens, aux]


def _as_device(t, dtype, device, name):
    """a per-row input converted the way `decode._as_seqlens` converts lengths -- except inside a graph capture, where a conversion
    would bake one value into the graph: there it must already be a contiguous tensor of the right dtype on the device"""
    if t is None:
        return None
    if not torch.is_tensor(t):
        if torch.cuda.is_current_stream_capturing():
            raise ValueError(f"sample_logits: inside a graph capture {name} must already be a contiguous {dtype} tensor on {device} "
                             "(a conversion would fix its current value in the graph)")
        t = torch.as_tensor(t)
    if t.dtype == dtype and t.device == device and t.is_contiguous():
        return t
    if torch.cuda.is_current_stream_capturing():
        raise ValueError(f"sample_logits: inside a graph capture {name} must already be a contiguous {dtype} tensor on {device} "
                         "(a conversion would fix its current value in the graph)")
    return t.to(device=device, dtype=dtype).contiguous()


def sample_logits(logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, offsets=None, offset=0, uniforms=None, return_aux=False):
    """One token per row of logits (B, V): tokens (B,) int64, or (tokens, aux (B, 4) fp32) with return_aux.  top_k 0 (or >= V)
    and top_p 1 switch those filters off.  Row b's counter is offset + offsets[b] (offsets: (B,) int, e.g. the decoding
    position); the seed is a uint64 (any int is taken modulo 2^64)."""
    if torch.is_grad_enabled() and logits.requires_grad:
        logits = logits.detach()
    check_args(temperature, top_k, top_p)
    _check_shapes(logits, offsets if torch.is_tensor(offsets) else None, uniforms if torch.is_tensor(uniforms) else None)
    if not logits.is_cuda:
        raise ValueError("sample_logits: logits must be on the GPU (there is no CPU path)")
    offs = _as_device(offsets, torch.int32, logits.device, "offsets")
    unif = _as_device(uniforms, torch.float32, logits.device, "uniforms")
    _check_shapes(logits, offs, unif)
    tokens, aux = sample_logits_op(logits, float(temperature), int(top_k), float(top_p), _u64(seed), int(offset), offs, unif,
                                   bool(return_aux))
    return (tokens, aux) if return_aux else tokens
