"""Logits processors in one HIP launch (`fat5_process_logits`, csrc/logits_kernels.h), with HF's order and meaning
(RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinLengthLogitsProcessor -> SuppressTokensLogitsProcessor):

    y = process_logits(logits, labels, cache_seqlens, repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=30)

`sequences` (rows, seq_len) int64 and `lengths` (rows,) int32 live on the device and are read there -- lengths[r] counts the
tokens of row r so far, the start token in column 0 included (HF's input_ids.shape[-1]; cache_seqlens after the decode step's
increment) -- so a captured graph replays the launch while both change.  The result is a new (rows, V) fp32 tensor: the fp32
value of every logit (minus the row's log-sum-exp with log_softmax=True, which is what beam search processes), edited as
include/fat5.h states.  It feeds argmax, `sample_logits` or `beam_step(..., logits_normalized=True)`.

Forward only, no CPU path: CPU tensors are rejected."""
import math
from typing import Optional

import torch

from . import _lib

MAX_V = 1 << 20
MAX_SEQ_LEN = 4096
MAX_SUPPRESS = 4096


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_args(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None, vocab_size=None, eos_token_id=1):
    """host-side validation shared with `generate` (before any device work).  A host list of suppressed ids is checked entry by
    entry (ints in [0, vocab_size)); a device tensor is taken as it is (the kernel skips ids outside the vocabulary)."""
    try:
        t = float(repetition_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"repetition_penalty must be a finite number > 0, got {repetition_penalty!r}") from None
    if isinstance(repetition_penalty, bool) or not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty!r}")
    if not _is_int(no_repeat_ngram_size) or no_repeat_ngram_size < 0:
        raise ValueError(f"no_repeat_ngram_size must be an int >= 0, got {no_repeat_ngram_size!r}")
    if not _is_int(min_length) or min_length < 0:
        raise ValueError(f"min_length must be an int >= 0, got {min_length!r}")
    if not _is_int(eos_token_id) or eos_token_id < 0 or (vocab_size is not None and eos_token_id >= vocab_size):
        raise ValueError(f"eos_token_id must be an int in [0, vocab), got {eos_token_id!r}")
    if suppress_tokens is None:
        return
    if torch.is_tensor(suppress_tokens):
        if suppress_tokens.dim() != 1 or suppress_tokens.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"suppress_tokens must be a 1-D int32 / int64 tensor, got {suppress_tokens.dtype} {tuple(suppress_tokens.shape)}")
        n = suppress_tokens.numel()
    else:
        ids = list(suppress_tokens)
        n = len(ids)
        for t in ids:
            if not _is_int(t):
                raise ValueError(f"suppress_tokens must hold ints, got {t!r}")
            if t < 0 or (vocab_size is not None and t >= vocab_size):
                raise ValueError(f"suppress_tokens: id {t} outside [0, {vocab_size if vocab_size is not None else 'vocab'})")
    if n > MAX_SUPPRESS:
        raise ValueError(f"suppress_tokens: {n} ids, at most {MAX_SUPPRESS}")


def active(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None):
    """whether any processor is switched on (with all of them off `generate` makes no launch)"""
    n = 0 if suppress_tokens is None else (suppress_tokens.numel() if torch.is_tensor(suppress_tokens) else len(list(suppress_tokens)))
    return float(repetition_penalty) != 1.0 or no_repeat_ngram_size > 0 or min_length > 0 or n > 0


def suppress_to_device(suppress_tokens, device):
    """None, a list or a tensor of ids -> None or a contiguous int32 tensor on `device` (one copy per `generate` call)"""
    if suppress_tokens is None:
        return None
    t = suppress_tokens if torch.is_tensor(suppress_tokens) else torch.tensor(list(suppress_tokens), dtype=torch.int32)
    if t.numel() == 0:
        return None
    if t.dtype == torch.int32 and t.device == device and t.is_contiguous():
        return t
    if torch.cuda.is_current_stream_capturing():
        raise ValueError(f"process_logits: inside a graph capture suppress_tokens must already be a contiguous int32 tensor on {device}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _check_tensors(logits, sequences, lengths, suppress):
    if logits.dim() != 2:
        raise ValueError(f"process_logits: logits must be (rows, V), got {tuple(logits.shape)}")
    rows, V = logits.shape
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"process_logits: dtype {logits.dtype} (fp32, fp16 or bf16)")
    if not 2 <= V <= MAX_V:
        raise ValueError(f"process_logits: V {V} outside [2, {MAX_V}]")
    if sequences.dim() != 2 or sequences.shape[0] != rows or sequences.dtype != torch.int64:
        raise ValueError(f"process_logits: sequences must be ({rows}, seq_len) int64, got {sequences.dtype} {tuple(sequences.shape)}")
    if not 1 <= sequences.shape[1] <= MAX_SEQ_LEN:
        raise ValueError(f"process_logits: seq_len {sequences.shape[1]} outside [1, {MAX_SEQ_LEN}]")
    if sequences.stride(1) != 1 or (rows > 1 and sequences.stride(0) < sequences.shape[1]):
        raise ValueError("process_logits: sequences needs innermost stride 1 and non-overlapping rows")
    if lengths.dim() != 1 or lengths.shape[0] != rows or lengths.dtype != torch.int32 or not lengths.is_contiguous():
        raise ValueError(f"process_logits: lengths must be a contiguous ({rows},) int32 tensor, got {lengths.dtype} {tuple(lengths.shape)}")
    if suppress is not None and (suppress.dim() != 1 or suppress.dtype != torch.int32 or not suppress.is_contiguous()
                                 or suppress.numel() > MAX_SUPPRESS):
        raise ValueError(f"process_logits: suppress_tokens must be a contiguous 1-D int32 tensor of at most {MAX_SUPPRESS} ids")


def _check_devices(logits, sequences, lengths, suppress):
    if not logits.is_cuda:
        raise ValueError("process_logits: logits must be on the GPU (there is no CPU path)")
    for name, t in (("sequences", sequences), ("lengths", lengths), ("suppress_tokens", suppress)):
        if t is not None and t.device != logits.device:
            raise ValueError(f"process_logits: {name} must be on {logits.device}, got {t.device}")


@torch.library.custom_op("fat5::process_logits", mutates_args=(), device_types="cuda")
def process_logits_op(logits: torch.Tensor, sequences: torch.Tensor, lengths: torch.Tensor, repetition_penalty: float,
                      no_repeat_ngram_size: int, min_length: int, eos_token_id: int, suppress_tokens: Optional[torch.Tensor],
                      log_softmax: bool) -> torch.Tensor:
    """(rows, V) fp32: the processed row (include/fat5.h, fat5_process_logits)"""
    _check_tensors(logits, sequences, lengths, suppress_tokens)
    _check_devices(logits, sequences, lengths, suppress_tokens)
    rows, V = logits.shape
    check_args(repetition_penalty, no_repeat_ngram_size, min_length, None, V, eos_token_id)
    if logits.stride(-1) != 1 or (rows > 1 and logits.stride(0) < V):
        logits = logits.contiguous()
    out = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    p = _lib.LogitsParams()
    p.rows, p.V, p.dtype, p.log_softmax = rows, V, _lib.dtype_code(logits.dtype), int(bool(log_softmax))
    p.logits, p.row_stride = logits.data_ptr(), logits.stride(0) if rows > 1 else V
    p.out, p.out_stride = out.data_ptr(), V
    p.sequences, p.seq_stride = sequences.data_ptr(), sequences.stride(0) if rows > 1 else sequences.shape[1]
    p.lengths, p.seq_len = lengths.data_ptr(), sequences.shape[1]
    p.repetition_penalty, p.no_repeat_ngram_size, p.min_length = float(repetition_penalty), int(no_repeat_ngram_size), int(min_length)
    p.eos_token_id = int(eos_token_id)
    n = 0 if suppress_tokens is None else suppress_tokens.numel()
    p.n_suppress, p.suppress_tokens = n, suppress_tokens.data_ptr() if n else None
    if rows:
        with _lib.on_device(logits.device):
            _lib.check(_lib.load().fat5_process_logits(p, _lib.stream_ptr(logits.device)), "fat5_process_logits")
    return out


@process_logits_op.register_fake
def _process_logits_fake(logits, sequences, lengths, repetition_penalty, no_repeat_ngram_size, min_length, eos_token_id,
                         suppress_tokens, log_softmax):
    return logits.new_empty(tuple(logits.shape), dtype=torch.float32)


def process_logits(logits, sequences, lengths, *, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, eos_token_id=1,
                   suppress_tokens=None, log_softmax=False):
    """logits (rows, V) fp32 / fp16 / bf16 -> the processed (rows, V) fp32 rows.  sequences (rows, seq_len) int64 and lengths
    (rows,) int32 are device tensors (row r's tokens so far are sequences[r, :lengths[r]], the start token included);
    suppress_tokens is None, a list of ids or a device int32 tensor (inside a graph capture: a device int32 tensor)."""
    if torch.is_grad_enabled() and logits.requires_grad:
        logits = logits.detach()
    check_args(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, logits.shape[-1] if logits.dim() == 2 else None,
               eos_token_id)
    if not logits.is_cuda:
        raise ValueError("process_logits: logits must be on the GPU (there is no CPU path)")
    sup = suppress_to_device(suppress_tokens, logits.device)
    _check_tensors(logits, sequences, lengths, sup)
    return process_logits_op(logits, sequences, lengths, float(repetition_penalty), int(no_repeat_ngram_size), int(min_length),
                             int(eos_token_id), sup, bool(log_softmax))
