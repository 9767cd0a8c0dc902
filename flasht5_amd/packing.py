"""Padding masks and packed examples for training: the device-side pack planner and what the model passes around.

`pack_plan(mask_or_segment_ids)` turns a (B, L) padding mask, or T5X-style segment ids (0 = padding; a row is a run of 1s, then of
2s, ..., then zeros), into what the packed kernels take -- `flash_attn_varlen_func`, `apply_rotary_emb_qkv(..., cu_seqlens=)` --
with two launches of `fat5_pack_plan` and ONE host read (the four status words).  A mask is the one-segment case of segment ids.
`plan_pair` plans the encoder and the decoder side of a batch for the same single host read and checks that every row holds as
many decoder as encoder segments (cross-attention pairs them in order)."""
import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

MAX_SEGMENTS = 256   # fat5_pack_plan's seg_cap
F_ORDER, F_EMPTY, F_SEGMENTS, F_NEGATIVE = 1, 2, 4, 8


@dataclass
class PackPlan:
    """cu_seqlens (nseq + 1,) int32 and index (total,) int64 on the device (index[i] = the flat position b * L + j of packed token
    i), seg_count (B,) int32 on the device; max_seqlen, total and nseq are host integers."""
    cu_seqlens: torch.Tensor
    index: torch.Tensor
    max_seqlen: int
    total: int
    nseq: int
    seg_count: torch.Tensor


@dataclass
class Packed:
    """what the attention layers of one stack take when the hidden states are (1, total, d_model): the stack's own cu_seqlens and,
    for a decoder's cross-attention, the encoder's"""
    cu_seqlens: torch.Tensor
    max_seqlen: int
    kv_cu_seqlens: Optional[torch.Tensor] = None
    kv_max_seqlen: Optional[int] = None


def _check_input(x, name):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{name} must be a (B, L) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if x.dtype.is_floating_point or x.dtype.is_complex:
        raise ValueError(f"{name} must be a bool or integer tensor, got {x.dtype}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name} must have at least one row and one column, got {tuple(x.shape)}")


def _as_segments(x, name):
    _check_input(x, name)
    if not x.is_cuda:
        raise RuntimeError(f"{name} must live on the HIP device (the planner has no CPU fallback)")
    return x.to(torch.int32).contiguous()   # (bool -> 0 / 1)


def _seg_cap(x, seg_cap):
    if seg_cap is None:
        return 1 if x.dtype == torch.bool else min(int(x.shape[1]), MAX_SEGMENTS)
    if not 1 <= int(seg_cap) <= MAX_SEGMENTS:
        raise ValueError(f"seg_cap {seg_cap} outside [1, {MAX_SEGMENTS}]")
    return int(seg_cap)


def launch_plan(seg, seg_cap):
    """fat5_pack_plan on a contiguous (B, L) int32 device tensor -> full-size (cu_seqlens, index, seg_count, status); no host read"""
    B, L = seg.shape
    dev = seg.device
    cu = torch.empty(B * seg_cap + 1, dtype=torch.int32, device=dev)
    index = torch.empty(B * L, dtype=torch.int64, device=dev)
    seg_count = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    p = _lib.PackParams()
    p.B, p.L, p.seg_cap = B, L, seg_cap
    p.seg, p.cu_seqlens, p.index, p.seg_count, p.status = (t.data_ptr() for t in (seg, cu, index, seg_count, status))
    with _lib.on_device(dev):
        _lib.check(_lib.load().fat5_pack_plan(ctypes.byref(p), _lib.stream_ptr(dev)), "fat5_pack_plan")
    return cu, index, seg_count, status


def _raise_flags(flags, name, seg_cap):
    if flags & F_NEGATIVE:
        raise ValueError(f"{name} holds a negative id (0 is padding, segment ids count from 1)")
    if flags & F_EMPTY:
        raise ValueError(f"{name} has an empty row: every row needs at least one valid position")
    if flags & F_ORDER:
        raise ValueError(f"{name} must be right-padded (each row a run of valid positions, then padding; segment ids start at 1 and "
                         "rise by exactly 1): left padding, holes and out-of-order ids are not supported")
    if flags & F_SEGMENTS:
        raise ValueError(f"{name} has a row with more than seg_cap = {seg_cap} segments")


def _finish(raw, host, name, seg_cap):
    cu, index, seg_count, _ = raw
    total, nseq, max_seqlen, flags = host
    _raise_flags(flags, name, seg_cap)
    return PackPlan(cu[:nseq + 1], index[:total], max_seqlen, total, nseq, seg_count)


def pack_plan(mask_or_segment_ids, seg_cap=None, name="mask_or_segment_ids"):
    """(B, L) bool mask (converted to 0 / 1) or integer segment ids on the device -> PackPlan; ONE host read.  seg_cap: the most
    segments a row may hold (default: 1 for a bool mask, else min(L, 256)).  ValueError names what is wrong with the input."""
    seg = _as_segments(mask_or_segment_ids, name)
    cap = _seg_cap(mask_or_segment_ids, seg_cap)
    raw = launch_plan(seg, cap)
    return _finish(raw, raw[3].tolist(), name, cap)   # the one host read


def plan_pair(enc_plan_input, dec_plan_input, seg_cap=None, names=("encoder side", "decoder side")):
    """both sides of an encoder-decoder batch -> (encoder PackPlan, decoder PackPlan), ONE host read in total; a row whose encoder
    and decoder segment counts differ raises ValueError (example i of a row's encoder side belongs to example i of its decoder side)"""
    for x, n in zip((enc_plan_input, dec_plan_input), names):   # (both sides on the host before anything is launched)
        _check_input(x, n)
    segs = [_as_segments(x, n) for x, n in zip((enc_plan_input, dec_plan_input), names)]
    if segs[0].shape[0] != segs[1].shape[0]:
        raise ValueError(f"{names[0]} has {segs[0].shape[0]} rows, {names[1]} {segs[1].shape[0]}")
    caps = [_seg_cap(x, seg_cap) for x in (enc_plan_input, dec_plan_input)]
    raws = [launch_plan(s, c) for s, c in zip(segs, caps)]
    differ = (raws[0][2] != raws[1][2]).any().to(torch.int32).reshape(1)
    host = torch.cat([raws[0][3], raws[1][3], differ]).tolist()   # the one host read
    plans = [_finish(r, host[4 * i:4 * i + 4], n, c) for i, (r, n, c) in enumerate(zip(raws, names, caps))]
    if host[8]:
        raise ValueError(f"a row's {names[0]} and {names[1]} hold different numbers of segments")
    return plans[0], plans[1]
