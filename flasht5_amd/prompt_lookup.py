"""Prompt-lookup drafting for speculative decoding: the drafter is no model but a search.  Per row, the
tokens that followed the row's last n-gram the first time it occurred -- in the encoder input or in the row's own sequence --
are proposed as the next round's draft (HF's `prompt_lookup_num_tokens`).  One HIP launch per round (`fat5_lookup_draft`,
csrc/lookup_kernels.h) instead of gamma + 1 decoder steps of an assistant; the verification (`speculative_round`) is unchanged,
so the output is what greedy decoding gives (with do_sample=True the drafts are verified as one-hot by the sampled rule).

    draft, n_proposed = prompt_lookup_draft(source, labels, cache_seqlens, tok, seen_eos, num_tokens, max_ngram=2,
                                            src_seqlens=None, vocab_size=None, out=None)
    labels = model.generate(input_ids, max_length=64, prompt_lookup_num_tokens=4, max_matching_ngram_size=2, graph=True)

Nothing here reads the host: every length is read on the device, so a captured round replays it.  Forward only, no CPU path."""
from typing import Optional, Tuple

import torch

from . import _lib
from .speculative import MAX_ASSISTANT_TOKENS, _is_int

MAX_NGRAM = 16         # (LOOKUP_MAX_NGRAM, csrc/lookup_kernels.h)
MAX_COLUMNS = 1 << 20  # (LOOKUP_MAX_LEN: the columns of source and of labels)


def check_args(num_tokens=4, max_ngram=2, vocab_size=None, what="prompt_lookup_draft", names=("num_tokens", "max_ngram")):
    """host-side validation shared with `generate` (before any device work)"""
    if not _is_int(num_tokens) or not 1 <= num_tokens <= MAX_ASSISTANT_TOKENS:
        raise ValueError(f"{what}: {names[0]} must be an int in [1, {MAX_ASSISTANT_TOKENS}], got {num_tokens!r}")
    if not _is_int(max_ngram) or not 1 <= max_ngram <= MAX_NGRAM:
        raise ValueError(f"{what}: {names[1]} must be an int in [1, {MAX_NGRAM}], got {max_ngram!r}")
    if vocab_size is not None and (not _is_int(vocab_size) or not 1 <= vocab_size < 2 ** 31):
        raise ValueError(f"{what}: vocab_size must be None or an int in [1, 2^31), got {vocab_size!r}")


def _check_tensors(source, labels, cache_seqlens, tok, seen_eos, gamma, src_seqlens, out):
    what = "prompt_lookup_draft"
    if not torch.is_tensor(source) or source.dim() != 2 or source.dtype != torch.int64:
        raise ValueError(f"{what}: source must be (B, L_src) int64, got "
                         f"{(source.dtype, tuple(source.shape)) if torch.is_tensor(source) else type(source).__name__}")
    B, L_src = source.shape
    if B > 65535:
        raise ValueError(f"{what}: B {B} (at most 65535)")
    if L_src > MAX_COLUMNS:
        raise ValueError(f"{what}: L_src {L_src} (at most {MAX_COLUMNS})")
    if L_src > 1 and source.stride(1) != 1 or (B > 1 and L_src > 0 and source.stride(0) < L_src):
        raise ValueError(f"{what}: source needs innermost stride 1 and non-overlapping rows")
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[0] != B or labels.dtype != torch.int64 or not 1 <= labels.shape[1] <= MAX_COLUMNS:
        raise ValueError(f"{what}: labels must be ({B}, 1 <= ncols <= {MAX_COLUMNS}) int64, got "
                         f"{(labels.dtype, tuple(labels.shape)) if torch.is_tensor(labels) else type(labels).__name__}")
    if (labels.shape[1] > 1 and labels.stride(1) != 1) or (B > 1 and labels.stride(0) < labels.shape[1]):
        raise ValueError(f"{what}: labels needs innermost stride 1 and non-overlapping rows")
    for name, t, need in (("cache_seqlens", cache_seqlens, True), ("src_seqlens", src_seqlens, False)):
        if t is None and not need:
            continue
        if not torch.is_tensor(t) or t.dim() != 1 or t.shape[0] != B or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous ({B},) int32 tensor, got "
                             f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
    if not torch.is_tensor(tok) or tok.dim() != 1 or tok.shape[0] != B or tok.dtype != torch.int64 or not tok.is_contiguous():
        raise ValueError(f"{what}: tok must be a contiguous ({B},) int64 tensor, got "
                         f"{(tok.dtype, tuple(tok.shape)) if torch.is_tensor(tok) else type(tok).__name__}")
    if not torch.is_tensor(seen_eos) or seen_eos.dim() != 1 or seen_eos.shape[0] != B or seen_eos.dtype != torch.bool or not seen_eos.is_contiguous():
        raise ValueError(f"{what}: seen_eos must be a contiguous ({B},) bool tensor, got "
                         f"{(seen_eos.dtype, tuple(seen_eos.shape)) if torch.is_tensor(seen_eos) else type(seen_eos).__name__}")
    if out is not None:
        if not torch.is_tensor(out) or out.dim() != 2 or tuple(out.shape) != (B, gamma) or out.dtype != torch.int64:
            raise ValueError(f"{what}: out must be ({B}, {gamma}) int64, got "
                             f"{(out.dtype, tuple(out.shape)) if torch.is_tensor(out) else type(out).__name__}")
        if (gamma > 1 and out.stride(1) != 1) or (B > 1 and out.stride(0) < gamma):
            raise ValueError(f"{what}: out needs innermost stride 1 and non-overlapping rows")


def _check_devices(source, labels, cache_seqlens, tok, seen_eos, src_seqlens, out):
    if not source.is_cuda:
        raise ValueError("prompt_lookup_draft: source must be on the GPU (there is no CPU path)")
    for name, t in (("labels", labels), ("cache_seqlens", cache_seqlens), ("tok", tok), ("seen_eos", seen_eos),
                    ("src_seqlens", src_seqlens), ("out", out)):
        if t is not None and t.device != source.device:
            raise ValueError(f"prompt_lookup_draft: {name} must be on {source.device}, got {t.device}")


@torch.library.custom_op("fat5::lookup_draft", mutates_args=("out",), device_types="cuda")
def lookup_draft_op(source: torch.Tensor, labels: torch.Tensor, cache_seqlens: torch.Tensor, tok: torch.Tensor, seen_eos: torch.Tensor,
                    src_seqlens: Optional[torch.Tensor], out: torch.Tensor, max_ngram: int, vocab_size: int) -> torch.Tensor:
    """n_proposed (B,) int32; the draft is written into `out` (B, gamma) in place (include/fat5.h, fat5_lookup_draft);
    vocab_size 0: no id is cut"""
    gamma = out.shape[1] if torch.is_tensor(out) and out.dim() == 2 else 0
    check_args(gamma, max_ngram, vocab_size if vocab_size else None)
    _check_tensors(source, labels, cache_seqlens, tok, seen_eos, gamma, src_seqlens, out)
    _check_devices(source, labels, cache_seqlens, tok, seen_eos, src_seqlens, out)
    B, L_src = source.shape
    dev = source.device
    n_proposed = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return n_proposed
    p = _lib.LookupParams()
    p.B, p.L_src, p.ncols, p.gamma, p.max_ngram, p.V = B, L_src, labels.shape[1], gamma, int(max_ngram), int(vocab_size)
    p.source = source.data_ptr() if L_src > 0 else None
    p.source_stride = source.stride(0) if B > 1 and L_src > 0 else L_src
    p.src_seqlens = src_seqlens.data_ptr() if src_seqlens is not None else None
    p.labels, p.labels_stride = labels.data_ptr(), labels.stride(0) if B > 1 else labels.shape[1]
    p.cache_seqlens, p.tok, p.seen_eos = cache_seqlens.data_ptr(), tok.data_ptr(), seen_eos.data_ptr()
    p.draft, p.draft_stride = out.data_ptr(), out.stride(0) if B > 1 else gamma
    p.n_proposed = n_proposed.data_ptr()
    lib = _lib.load()
    with _lib.on_device(dev):
        _lib.check(lib.fat5_lookup_draft(p, _lib.stream_ptr(dev)), "fat5_lookup_draft")
    return n_proposed


@lookup_draft_op.register_fake
def _lookup_draft_fake(source, labels, cache_seqlens, tok, seen_eos, src_seqlens, out, max_ngram, vocab_size):
    return source.new_empty((source.shape[0],), dtype=torch.int32)


def prompt_lookup_draft(source, labels, cache_seqlens, tok, seen_eos, num_tokens, max_ngram=2, src_seqlens=None, vocab_size=None,
                        out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Draft one round for all B rows on the device (one launch, nothing read back).

    source (B, L_src) int64: the encoder input (L_src may be 0); labels (B, ncols) int64, cache_seqlens (B,) int32, tok (B,) int64
    and seen_eos (B,) bool: the running sequences, their lengths, the pending tokens and the finished rows, as
    `speculative_round` keeps them; num_tokens = gamma in [1, 15]; max_ngram = N in [1, 16]; src_seqlens (B,) int32: the valid
    length of every source row (None: L_src), so that padding is never proposed; vocab_size: a continuation is cut before its first
    id outside [0, vocab_size) (None: no id is cut); out (B, gamma) int64: written in place and returned, so that a captured
    round keeps one static buffer (None: a new tensor).  The rule per row is stated in include/fat5.h (fat5_lookup_draft) and
    restated in tests/lookup_ref.py.  Returns (draft, n_proposed): (B, gamma) int64 -- the proposed tokens, then the pending
    token as filler -- and (B,) int32, the tokens proposed per row."""
    check_args(num_tokens, max_ngram, vocab_size)
    _check_tensors(source, labels, cache_seqlens, tok, seen_eos, num_tokens, src_seqlens, out)
    _check_devices(source, labels, cache_seqlens, tok, seen_eos, src_seqlens, out)
    if out is None:
        out = torch.empty((source.shape[0], num_tokens), dtype=torch.int64, device=source.device)
    n_proposed = lookup_draft_op(source, labels, cache_seqlens, tok, seen_eos, src_seqlens, out, int(max_ngram),
                                 0 if vocab_size is None else int(vocab_size))
    return out, n_proposed
