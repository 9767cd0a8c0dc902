"""Logits processors in one HIP launch (`fat5_process_logits`, csrc/logits_kernels.h), with HF's order and meaning
(RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinLengthLogitsProcessor -> SuppressTokensLogitsProcessor):

    y = process_logits(logits, labels, cache_seqlens, repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=30)

and, in the same launch and in HF's place in the chain, the processors an encoder-decoder model needs (EncoderRepetitionPenalty,
EncoderNoRepeatNGram, NoBadWords, MinNewTokensLength, ForcedBOSToken, ForcedEOSToken):

    y = process_logits(logits, labels, cache_seqlens, encoder_no_repeat_ngram_size=3, encoder_input_ids=input_ids,
                       bad_words_ids=[[32099, 32098]], min_new_tokens=4, forced_eos_token_id=1, max_new_tokens=64)

`sequences` (rows, seq_len) int64 and `lengths` (rows,) int32 live on the device and are read there -- lengths[r] counts the
tokens of row r so far, the start token in column 0 included (HF's input_ids.shape[-1]; cache_seqlens after the decode step's
increment) -- so a captured graph replays the launch while both change.  The result is a new (rows, V) fp32 tensor: the fp32
value of every logit (minus the row's log-sum-exp with log_softmax=True, which is what beam search processes), edited as
include/fat5.h states.  It feeds argmax, `sample_logits` or `beam_step(..., logits_normalized=True)`.

Forward only, no CPU path: CPU tensors are rejected."""
import ctypes
import math
from typing import List, NamedTuple, Optional

import torch

from . import _lib

MAX_V = 1 << 20
MAX_SEQ_LEN = 4096
MAX_SUPPRESS = 4096
MAX_ENCODER_LEN = 4096
MAX_BAD_WORDS = 1024
MAX_BAD_WORD_IDS = 4096


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_args(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None, vocab_size=None, eos_token_id=1,
               encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
               forced_bos_token_id=None, forced_eos_token_id=None):
    """host-side validation shared with `generate` (before any device work).  A host list of suppressed ids is checked entry by
    entry (ints in [0, vocab_size)); a device tensor is taken as it is (the kernel skips ids outside the vocabulary).  The
    appended arguments are typed as HF's classes type them: encoder_repetition_penalty a float > 0, bad_words_ids a non-empty
    list of non-empty lists of ints (or a `BadWords` packed by `pack_bad_words`), the forced ids None or ints."""
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
    _check_suppress(suppress_tokens, vocab_size)
    if not isinstance(encoder_repetition_penalty, float) or not (encoder_repetition_penalty > 0.0 and math.isfinite(encoder_repetition_penalty)):
        raise ValueError(f"encoder_repetition_penalty must be a finite float > 0, got {encoder_repetition_penalty!r}")
    if not _is_int(encoder_no_repeat_ngram_size) or encoder_no_repeat_ngram_size < 0:
        raise ValueError(f"encoder_no_repeat_ngram_size must be an int >= 0, got {encoder_no_repeat_ngram_size!r}")
    if not _is_int(min_new_tokens) or min_new_tokens < 0:
        raise ValueError(f"min_new_tokens must be an int >= 0, got {min_new_tokens!r}")
    for name, t in (("forced_bos_token_id", forced_bos_token_id), ("forced_eos_token_id", forced_eos_token_id)):
        if t is not None and (not _is_int(t) or t < 0 or (vocab_size is not None and t >= vocab_size)):
            raise ValueError(f"{name} must be None or an int in [0, {vocab_size if vocab_size is not None else 'vocab'}), got {t!r}")
    _check_bad_words(bad_words_ids, vocab_size)


def _check_suppress(suppress_tokens, vocab_size):
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


class BadWords(NamedTuple):
    """bad_words_ids packed for the kernel: the sequences one after the other and their offsets, on the device, and the
    offsets once more on the host (fat5_process_logits checks those before the launch)"""
    ids: torch.Tensor           # (total,) int32
    offsets: torch.Tensor       # (n + 1,) int32
    host_offsets: tuple


def _check_bad_words(bad_words_ids, vocab_size):
    if bad_words_ids is None:
        return
    if isinstance(bad_words_ids, BadWords):
        off = bad_words_ids.host_offsets
        n, total = len(off) - 1, off[-1] if off else 0
        if (n < 1 or off[0] != 0 or any(b <= a for a, b in zip(off, off[1:])) or bad_words_ids.ids.numel() != total
                or bad_words_ids.offsets.numel() != n + 1):
            raise ValueError("bad_words_ids: a BadWords whose offsets do not describe its ids (use pack_bad_words)")
    else:
        if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
            raise ValueError(f"bad_words_ids must be a non-empty list of lists of ints, got {bad_words_ids!r}")
        for seq in bad_words_ids:
            if not isinstance(seq, list) or len(seq) == 0:
                raise ValueError(f"bad_words_ids must hold non-empty lists of ints, got {seq!r}")
            for t in seq:
                if not _is_int(t) or t < 0 or (vocab_size is not None and t >= vocab_size):
                    raise ValueError(f"bad_words_ids: {t!r} is not an int in [0, {vocab_size if vocab_size is not None else 'vocab'})")
        n, total = len(bad_words_ids), sum(len(seq) for seq in bad_words_ids)
    if n > MAX_BAD_WORDS or total > MAX_BAD_WORD_IDS:
        raise ValueError(f"bad_words_ids: {n} sequences of {total} ids in total, at most {MAX_BAD_WORDS} of {MAX_BAD_WORD_IDS}")


def _kept_bad_words(bad_words_ids, eos_token_id):
    """the sequences without [eos] entries, which HF drops"""
    return [seq for seq in bad_words_ids if seq != [eos_token_id]]


def pack_bad_words(bad_words_ids, device, eos_token_id=1):
    """None, a list of lists or a BadWords -> None or a BadWords on `device` (one copy per `generate` call).  A sequence equal
    to [eos_token_id] is dropped, as HF drops it; with nothing left the processor is off."""
    if bad_words_ids is None:
        return None
    device = torch.device(device)
    if isinstance(bad_words_ids, BadWords):
        if bad_words_ids.ids.device != device or bad_words_ids.offsets.device != device:
            raise ValueError(f"process_logits: the packed bad_words_ids must be on {device}")
        return bad_words_ids
    seqs = _kept_bad_words(bad_words_ids, eos_token_id)
    if not seqs:
        return None
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise ValueError(f"process_logits: inside a graph capture bad_words_ids must already be packed on {device} (pack_bad_words)")
    off = [0]
    for seq in seqs:
        off.append(off[-1] + len(seq))
    ids = torch.tensor([t for seq in seqs for t in seq], dtype=torch.int32).to(device)
    return BadWords(ids, torch.tensor(off, dtype=torch.int32).to(device), tuple(off))


def active(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None, encoder_repetition_penalty=1.0,
           encoder_no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, forced_bos_token_id=None, forced_eos_token_id=None,
           eos_token_id=1):
    """whether any processor is switched on (with all of them off `generate` makes no launch)"""
    n = 0 if suppress_tokens is None else (suppress_tokens.numel() if torch.is_tensor(suppress_tokens) else len(list(suppress_tokens)))
    bad = bad_words_ids is not None and (isinstance(bad_words_ids, BadWords) or len(_kept_bad_words(bad_words_ids, eos_token_id)) > 0)
    return (float(repetition_penalty) != 1.0 or no_repeat_ngram_size > 0 or min_length > 0 or n > 0
            or float(encoder_repetition_penalty) != 1.0 or encoder_no_repeat_ngram_size > 0 or bad or min_new_tokens > 0
            or forced_bos_token_id is not None or forced_eos_token_id is not None)


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


def _check_ext_tensors(rows, device, encoder_input_ids, encoder_lengths, rows_per_encoder_row, bad_ids, bad_offsets, prompt_lengths):
    if encoder_input_ids is not None:
        e = encoder_input_ids
        if e.dim() != 2 or e.dtype != torch.int64 or e.stride(1) != 1 or (e.shape[0] > 1 and e.stride(0) < e.shape[1]):
            raise ValueError(f"process_logits: encoder_input_ids must be (encoder rows, L) int64 with innermost stride 1, got {e.dtype} "
                             f"{tuple(e.shape)}")
        if not 1 <= e.shape[1] <= MAX_ENCODER_LEN:
            raise ValueError(f"process_logits: {e.shape[1]} encoder ids per row, outside [1, {MAX_ENCODER_LEN}]")
        if rows_per_encoder_row < 1 or e.shape[0] * rows_per_encoder_row < rows:
            raise ValueError(f"process_logits: {e.shape[0]} encoder rows of {rows_per_encoder_row} rows each do not cover {rows} rows")
        if encoder_lengths is not None and (encoder_lengths.shape != (e.shape[0],) or encoder_lengths.dtype != torch.int32
                                            or not encoder_lengths.is_contiguous()):
            raise ValueError(f"process_logits: encoder_lengths must be a contiguous ({e.shape[0]},) int32 tensor")
    if prompt_lengths is not None and (prompt_lengths.shape != (rows,) or prompt_lengths.dtype != torch.int32
                                       or not prompt_lengths.is_contiguous()):
        raise ValueError(f"process_logits: prompt_lengths must be a contiguous ({rows},) int32 tensor")
    if (bad_ids is None) != (bad_offsets is None):
        raise ValueError("process_logits: bad_words_ids and bad_words_offsets go together")
    for name, t in (("bad_words_ids", bad_ids), ("bad_words_offsets", bad_offsets)):
        if t is not None and (t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError(f"process_logits: {name} must be a contiguous 1-D int32 tensor")
    for name, t in (("encoder_input_ids", encoder_input_ids), ("encoder_lengths", encoder_lengths), ("bad_words_ids", bad_ids),
                    ("bad_words_offsets", bad_offsets), ("prompt_lengths", prompt_lengths)):
        if t is not None and t.device != device:
            raise ValueError(f"process_logits: {name} must be on {device}, got {t.device}")


@torch.library.custom_op("fat5::process_logits", mutates_args=(), device_types="cuda")
def process_logits_op(logits: torch.Tensor, sequences: torch.Tensor, lengths: torch.Tensor, repetition_penalty: float,
                      no_repeat_ngram_size: int, min_length: int, eos_token_id: int, suppress_tokens: Optional[torch.Tensor],
                      log_softmax: bool, encoder_repetition_penalty: float = 1.0, encoder_no_repeat_ngram_size: int = 0,
                      encoder_input_ids: Optional[torch.Tensor] = None, encoder_lengths: Optional[torch.Tensor] = None,
                      rows_per_encoder_row: int = 1, bad_words_ids: Optional[torch.Tensor] = None,
                      bad_words_offsets: Optional[torch.Tensor] = None, bad_words_host_offsets: Optional[List[int]] = None,
                      min_new_tokens: int = 0, prompt_length: int = 1, prompt_lengths: Optional[torch.Tensor] = None,
                      max_new_tokens: int = 0, forced_bos_token_id: int = -1, forced_eos_token_id: int = -1) -> torch.Tensor:
    """(rows, V) fp32: the processed row (include/fat5.h, fat5_process_logits).  The forced ids are -1 when off."""
    _check_tensors(logits, sequences, lengths, suppress_tokens)
    _check_devices(logits, sequences, lengths, suppress_tokens)
    rows, V = logits.shape
    check_args(repetition_penalty, no_repeat_ngram_size, min_length, None, V, eos_token_id, float(encoder_repetition_penalty),
               encoder_no_repeat_ngram_size, None, min_new_tokens, None if forced_bos_token_id < 0 else forced_bos_token_id,
               None if forced_eos_token_id < 0 else forced_eos_token_id)
    enc_on = float(encoder_repetition_penalty) != 1.0 or encoder_no_repeat_ngram_size > 0
    if enc_on and encoder_input_ids is None:
        raise ValueError("process_logits: encoder_repetition_penalty / encoder_no_repeat_ngram_size need encoder_input_ids")
    _check_ext_tensors(rows, logits.device, encoder_input_ids if enc_on else None, encoder_lengths if enc_on else None,
                       rows_per_encoder_row, bad_words_ids, bad_words_offsets, prompt_lengths)
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
    if enc_on:
        e = encoder_input_ids
        p.encoder_repetition_penalty, p.encoder_no_repeat_ngram_size = float(encoder_repetition_penalty), int(encoder_no_repeat_ngram_size)
        p.encoder_input_ids, p.encoder_stride = e.data_ptr(), e.stride(0) if e.shape[0] > 1 else e.shape[1]
        p.encoder_lengths = None if encoder_lengths is None else encoder_lengths.data_ptr()
        p.encoder_rows, p.encoder_len, p.rows_per_encoder_row = e.shape[0], e.shape[1], int(rows_per_encoder_row)
    host_off = None
    if bad_words_ids is not None and bad_words_offsets.numel() > 1:
        p.bad_words_ids, p.bad_words_offsets = bad_words_ids.data_ptr(), bad_words_offsets.data_ptr()
        p.n_bad_words, p.n_bad_word_ids = bad_words_offsets.numel() - 1, bad_words_ids.numel()
        if bad_words_host_offsets is not None:
            if len(bad_words_host_offsets) != bad_words_offsets.numel():
                raise ValueError("process_logits: bad_words_host_offsets and bad_words_offsets differ in length")
            host_off = (ctypes.c_int32 * len(bad_words_host_offsets))(*bad_words_host_offsets)  # (alive until the call returns)
            p.bad_words_offsets_host = ctypes.addressof(host_off)
    p.min_new_tokens, p.prompt_length, p.max_new_tokens = int(min_new_tokens), int(prompt_length), int(max_new_tokens)
    p.prompt_lengths = None if prompt_lengths is None else prompt_lengths.data_ptr()
    if forced_bos_token_id >= 0:
        p.forced_tokens, p.forced_bos_token_id = p.forced_tokens | _lib.FAT5_FORCED_BOS, int(forced_bos_token_id)
    if forced_eos_token_id >= 0:
        p.forced_tokens, p.forced_eos_token_id = p.forced_tokens | _lib.FAT5_FORCED_EOS, int(forced_eos_token_id)
    if rows:
        with _lib.on_device(logits.device):
            _lib.check(_lib.load().fat5_process_logits(p, _lib.stream_ptr(logits.device)), "fat5_process_logits")
    del host_off
    return out


@process_logits_op.register_fake
def _process_logits_fake(logits, sequences, lengths, repetition_penalty, no_repeat_ngram_size, min_length, eos_token_id,
                         suppress_tokens, log_softmax, encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0,
                         encoder_input_ids=None, encoder_lengths=None, rows_per_encoder_row=1, bad_words_ids=None,
                         bad_words_offsets=None, bad_words_host_offsets=None, min_new_tokens=0, prompt_length=1, prompt_lengths=None,
                         max_new_tokens=0, forced_bos_token_id=-1, forced_eos_token_id=-1):
    return logits.new_empty(tuple(logits.shape), dtype=torch.float32)


def process_logits(logits, sequences, lengths, *, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, eos_token_id=1,
                   suppress_tokens=None, log_softmax=False, encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0,
                   bad_words_ids=None, min_new_tokens=0, forced_bos_token_id=None, forced_eos_token_id=None,
                   encoder_input_ids=None, encoder_lengths=None, rows_per_encoder_row=1, prompt_length=1, prompt_lengths=None,
                   max_new_tokens=None):
    """logits (rows, V) fp32 / fp16 / bf16 -> the processed (rows, V) fp32 rows.  sequences (rows, seq_len) int64 and lengths
    (rows,) int32 are device tensors (row r's tokens so far are sequences[r, :lengths[r]], the start token included);
    suppress_tokens is None, a list of ids or a device int32 tensor (inside a graph capture: a device int32 tensor).

    The encoder-side processors read `encoder_input_ids` (encoder rows, L <= 4096) int64 on the device: row r uses encoder row
    r // rows_per_encoder_row (num_beams under beam search) and of it the first encoder_lengths[...] ids (a device int32 vector;
    None: all L).  `bad_words_ids` is a list of lists of ids or a `BadWords` from `pack_bad_words` (inside a graph capture: a
    BadWords).  `min_new_tokens` and `forced_eos_token_id` count from the decoder prompt: `prompt_length` P (the start token
    included), or `prompt_lengths` (rows,) int32 on the device; `forced_eos_token_id` needs `max_new_tokens`."""
    if torch.is_grad_enabled() and logits.requires_grad:
        logits = logits.detach()
    check_args(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, logits.shape[-1] if logits.dim() == 2 else None,
               eos_token_id, encoder_repetition_penalty, encoder_no_repeat_ngram_size, bad_words_ids, min_new_tokens,
               forced_bos_token_id, forced_eos_token_id)
    if not _is_int(prompt_length) or prompt_length < 1:
        raise ValueError(f"prompt_length must be an int >= 1, got {prompt_length!r}")
    if forced_eos_token_id is not None and (not _is_int(max_new_tokens) or max_new_tokens < 1):
        raise ValueError(f"forced_eos_token_id needs max_new_tokens, an int >= 1, got {max_new_tokens!r}")
    enc_on = encoder_repetition_penalty != 1.0 or encoder_no_repeat_ngram_size > 0
    if enc_on and not torch.is_tensor(encoder_input_ids):
        raise ValueError("process_logits: encoder_repetition_penalty / encoder_no_repeat_ngram_size need encoder_input_ids")
    if not logits.is_cuda:
        raise ValueError("process_logits: logits must be on the GPU (there is no CPU path)")
    sup = suppress_to_device(suppress_tokens, logits.device)
    bad = pack_bad_words(bad_words_ids, logits.device, eos_token_id)
    _check_tensors(logits, sequences, lengths, sup)
    return process_logits_op(logits, sequences, lengths, float(repetition_penalty), int(no_repeat_ngram_size), int(min_length),
                             int(eos_token_id), sup, bool(log_softmax), float(encoder_repetition_penalty),
                             int(encoder_no_repeat_ngram_size), encoder_input_ids if enc_on else None,
                             encoder_lengths if enc_on else None, int(rows_per_encoder_row),
                             None if bad is None else bad.ids, None if bad is None else bad.offsets,
                             None if bad is None else list(bad.host_offsets), int(min_new_tokens), int(prompt_length), prompt_lengths,
                             0 if max_new_tokens is None else int(max_new_tokens),
                             -1 if forced_bos_token_id is None else int(forced_bos_token_id),
                             -1 if forced_eos_token_id is None else int(forced_eos_token_id))
