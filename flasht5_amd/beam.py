"""One beam-search step on the device (`fat5_beam_step`, csrc/beam_kernels.h): HF's vectorized `_beam_search` bookkeeping for B
batch items of k beams in two HIP launches, every state tensor updated in place, so the step is captured with the decode step.

    st = new_state(B, k, seq_len, capacity, device)
    beam_step(logits, st, step=cache_seqlens, max_length=32, length_penalty=1.0, early_stopping=False)   # writes st.tokens

The semantics (scores, tie order, stopping, length penalty, the early-stop heuristic, the history tables) are stated in
include/fat5.h.  Forward only, no CPU path: CPU tensors are rejected."""
import math
from dataclasses import dataclass

import torch

from . import _lib

MAX_BEAMS = 16
MAX_V = 1 << 20
_EARLY = {False: 0, True: 1, "never": 2}


def early_code(early_stopping):
    """False / True / "never" -> 0 / 1 / 2 (HF's three modes; anything else is rejected)"""
    for key, code in _EARLY.items():
        if early_stopping is key or (isinstance(early_stopping, str) and early_stopping == key):
            return code
    raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")


def check_args(num_beams, num_return_sequences=1, length_penalty=1.0, early_stopping=False, do_sample=False):
    """host-side validation shared with `generate` (before any device work)"""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not (num_beams == 1 or 2 <= num_beams <= MAX_BEAMS):
        raise ValueError(f"num_beams must be 1 or an int in [2, {MAX_BEAMS}], got {num_beams!r}")
    if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or num_return_sequences < 1:
        raise ValueError(f"num_return_sequences must be an int >= 1, got {num_return_sequences!r}")
    if num_return_sequences > num_beams:
        raise ValueError(f"num_return_sequences {num_return_sequences} > num_beams {num_beams}")
    if num_beams > 1:
        if do_sample:
            raise ValueError("beam sampling (do_sample=True with num_beams > 1) is not supported")
        if not math.isfinite(float(length_penalty)):
            raise ValueError(f"length_penalty must be finite, got {length_penalty}")
        early_code(early_stopping)


@dataclass
class BeamState:
    """the beam search's device state (include/fat5.h, fat5_beam_params), in HF's initial values"""
    running_scores: torch.Tensor   # (B, k) fp32
    running_seqs: torch.Tensor     # (B, k, seq_len) int64
    cache_row_batch: torch.Tensor  # (B * k, capacity) int32
    finished_seqs: torch.Tensor    # (B, k, seq_len) int64
    finished_scores: torch.Tensor  # (B, k) fp32
    finished_flags: torch.Tensor   # (B, k) bool
    finished_lens: torch.Tensor    # (B, k) int32
    heuristic: torch.Tensor        # (B,) bool
    status: torch.Tensor           # (B,) int32
    tokens: torch.Tensor           # (B * k,) int64


def new_state(B, k, seq_len, capacity, device):
    rs = torch.full((B, k), -1.0e9, dtype=torch.float32, device=device)
    rs[:, 0] = 0.0
    return BeamState(
        rs, torch.zeros((B, k, seq_len), dtype=torch.int64, device=device),
        torch.zeros((B * k, capacity), dtype=torch.int32, device=device),
        torch.zeros((B, k, seq_len), dtype=torch.int64, device=device),
        torch.full((B, k), -1.0e9, dtype=torch.float32, device=device),
        torch.zeros((B, k), dtype=torch.bool, device=device), torch.zeros((B, k), dtype=torch.int32, device=device),
        torch.ones((B,), dtype=torch.bool, device=device), torch.zeros((B,), dtype=torch.int32, device=device),
        torch.zeros((B * k,), dtype=torch.int64, device=device))


def keep_going(status, early_stopping):
    """HF's _beam_search_has_unfinished_sequences from the per-item status bits, as a device bool (one host read by the caller)"""
    improve = (status & 1).ne(0).any()
    full = (status & 2).ne(0).all()
    if early_code(early_stopping) == 1:
        improve = improve & ~full
    return improve & ~(status & 4).ne(0).all()


def _check(logits, running_scores, running_seqs, cache_row_batch, finished_seqs, finished_scores, finished_flags, finished_lens,
           heuristic, status, tokens, step, num_beams):
    k = int(num_beams)
    if not 2 <= k <= MAX_BEAMS:
        raise ValueError(f"beam_step: num_beams {k} outside [2, {MAX_BEAMS}]")
    if logits.dim() != 2 or logits.shape[0] % k:
        raise ValueError(f"beam_step: logits must be (B * k, V), got {tuple(logits.shape)} with k = {k}")
    BK, V = logits.shape
    B = BK // k
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"beam_step: logits dtype {logits.dtype} (fp32, fp16 or bf16)")
    if not 2 <= V <= MAX_V:
        raise ValueError(f"beam_step: V {V} outside [2, {MAX_V}]")
    if running_seqs.dim() != 3 or tuple(running_seqs.shape[:2]) != (B, k):
        raise ValueError(f"beam_step: running_seqs must be ({B}, {k}, seq_len), got {tuple(running_seqs.shape)}")
    L = running_seqs.shape[2]
    if cache_row_batch.dim() != 2 or cache_row_batch.shape[0] != BK:
        raise ValueError(f"beam_step: cache_row_batch must be ({BK}, capacity), got {tuple(cache_row_batch.shape)}")
    want = [("running_scores", running_scores, (B, k), torch.float32), ("running_seqs", running_seqs, (B, k, L), torch.int64),
            ("cache_row_batch", cache_row_batch, tuple(cache_row_batch.shape), torch.int32),
            ("finished_seqs", finished_seqs, (B, k, L), torch.int64), ("finished_scores", finished_scores, (B, k), torch.float32),
            ("finished_flags", finished_flags, (B, k), torch.bool), ("finished_lens", finished_lens, (B, k), torch.int32),
            ("heuristic", heuristic, (B,), torch.bool), ("status", status, (B,), torch.int32), ("tokens", tokens, (BK,), torch.int64)]
    for name, t, shape, dt in want:
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"beam_step: {name} must be a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    if step.dtype != torch.int32 or step.dim() != 1 or step.numel() < BK or not step.is_contiguous():
        raise ValueError(f"beam_step: step must be a contiguous int32 tensor of at least {BK} entries (read at [b * k])")
    for t in [logits, step] + [w[1] for w in want]:
        if not t.is_cuda or t.device != logits.device:
            raise ValueError("beam_step: every tensor must be on the logits' GPU (there is no CPU path)")


@torch.library.custom_op("fat5::beam_step", mutates_args=("running_scores", "running_seqs", "cache_row_batch", "finished_seqs",
                                                          "finished_scores", "finished_flags", "finished_lens", "heuristic",
                                                          "status", "tokens"), device_types="cuda")
def beam_step_op(logits: torch.Tensor, running_scores: torch.Tensor, running_seqs: torch.Tensor, cache_row_batch: torch.Tensor,
                 finished_seqs: torch.Tensor, finished_scores: torch.Tensor, finished_flags: torch.Tensor, finished_lens: torch.Tensor,
                 heuristic: torch.Tensor, status: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, num_beams: int,
                 max_length: int, length_penalty: float, early_stopping: int, logits_normalized: bool = False) -> None:
    _check(logits, running_scores, running_seqs, cache_row_batch, finished_seqs, finished_scores, finished_flags, finished_lens,
           heuristic, status, tokens, step, num_beams)
    if logits.stride(-1) != 1:
        logits = logits.contiguous()
    k = int(num_beams)
    BK, V = logits.shape
    p = _lib.BeamParams()
    p.B, p.k, p.V, p.dtype = BK // k, k, V, _lib.dtype_code(logits.dtype)
    p.logits, p.row_stride = logits.data_ptr(), logits.stride(0)
    p.running_scores, p.running_seqs, p.cache_row_batch = running_scores.data_ptr(), running_seqs.data_ptr(), cache_row_batch.data_ptr()
    p.finished_seqs, p.finished_scores = finished_seqs.data_ptr(), finished_scores.data_ptr()
    p.finished_flags, p.finished_lens = finished_flags.data_ptr(), finished_lens.data_ptr()
    p.heuristic, p.status, p.tokens, p.step = heuristic.data_ptr(), status.data_ptr(), tokens.data_ptr(), step.data_ptr()
    p.seq_len, p.capacity = running_seqs.shape[2], cache_row_batch.shape[1]
    p.max_length, p.early_stopping, p.length_penalty = int(max_length), int(early_stopping), float(length_penalty)
    p.logits_normalized = int(bool(logits_normalized))
    lib = _lib.load()
    need = lib.fat5_beam_step_workspace_bytes(p)
    ws = torch.empty(need, dtype=torch.uint8, device=logits.device)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    with _lib.on_device(logits.device):
        _lib.check(lib.fat5_beam_step(p, _lib.stream_ptr(logits.device)), "fat5_beam_step")


@beam_step_op.register_fake
def _beam_step_fake(logits, running_scores, running_seqs, cache_row_batch, finished_seqs, finished_scores, finished_flags,
                    finished_lens, heuristic, status, tokens, step, num_beams, max_length, length_penalty, early_stopping,
                    logits_normalized=False):
    return None


def beam_step(logits, st, step, max_length, length_penalty=1.0, early_stopping=False, logits_normalized=False):
    """one beam-search step over logits (B * k, V) into the BeamState `st`; `step` is the device int32 count of tokens fed so far
    (cache_seqlens after the decode step's increment), read at [b * k].  logits_normalized=True: the rows are log-probabilities
    already (`process_logits(..., log_softmax=True)`, bans included) and are scored as they are, without a renormalisation --
    HF's order, processors on log_softmax(logits)"""
    k = st.running_scores.shape[1]
    if not math.isfinite(float(length_penalty)):
        raise ValueError(f"length_penalty must be finite, got {length_penalty}")
    if int(max_length) < 1:
        raise ValueError(f"max_length must be >= 1, got {max_length}")
    beam_step_op(logits, st.running_scores, st.running_seqs, st.cache_row_batch, st.finished_seqs, st.finished_scores,
                 st.finished_flags, st.finished_lens, st.heuristic, st.status, st.tokens, step, k, int(max_length),
                 float(length_penalty), early_code(early_stopping), bool(logits_normalized))
