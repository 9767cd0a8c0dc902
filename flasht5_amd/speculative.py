"""Speculative decoding: a cheap drafter proposes gamma tokens per row, the target model checks all of them
in ONE chunk step (`decode_chunk`, gamma + 1 rows), and a HIP verification kernel rolls the lengths back and does the bookkeeping
of every row on the device.  Greedy (`fat5_spec_accept`, csrc/spec_kernels.h): the longest agreeing prefix plus the target's own
next token; the output is what greedy decoding without a drafter gives.  Sampled (`sampling=...`, `fat5_spec_accept_sampled`,
csrc/spec_sample_kernels.h): draft d ~ q is accepted with probability min(1, p(d) / q(d)) and the first rejection is redrawn from
norm(max(p - q, 0)), so every emitted token is distributed as `sample_logits` would draw it (Leviathan et al., Chen et al.); a
drafter without logits (the prompt lookup) is the one-hot q.

    n_accepted, n_new = speculative_accept(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens=None)
    n_accepted, n_new = speculative_round(model, state, tok, draft, labels, seen_eos, limit, draft_state=None)
    labels = model.generate(input_ids, max_length=64, assistant_model=small, num_assistant_tokens=4, graph=True)
    labels = model.generate(input_ids, max_length=64, prompt_lookup_num_tokens=4, graph=True)   # (no second model: prompt_lookup.py)
    labels = model.generate(input_ids, max_length=64, assistant_model=small, do_sample=True, top_k=50, seed=7, graph=True)
    n_accepted, n_new = speculative_accept(..., sampling=(temperature, top_k, top_p, seed), draft_logits=q_logits)

The invariant at every round boundary, per row b with len_b = cache_seqlens[b]: the self-attention caches of both models hold the
K / V of labels[b, :len_b], and tok[b] = labels[b, len_b] is pending (decided, not yet run through either decoder).  A round
feeds [tok, d_0 .. d_{gamma-1}]; whatever n of the drafts the target agrees with, the first n + 1 rows the chunk appended are the
K / V of tokens that stay, so the roll-back is the write of one length per row -- which is why `cache_seqlens` is per row: rows
advance raggedly.  The model drafter runs gamma + 1 one-token steps (tok, then d_0 .. d_{gamma-1}; the last step's logits are not
used), so its cache is valid for every n as well and its length vector takes the same value.

Nothing here reads the host; `generate(graph=True)` captures one whole round (both models, one stream) and replays it.
Forward only, no CPU path."""
from typing import List, Optional, Tuple

import torch

from . import _lib

MAX_ASSISTANT_TOKENS = 15  # (SPEC_MAX_M - 1, csrc/spec_kernels.h)
MAX_V = 1 << 20
DRAFT_KEY = 0x9E3779B97F4A7C15  # the drafter samples under seed ^ DRAFT_KEY: a Philox key of its own


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_args(num_assistant_tokens=4, eos_token_id=1):
    """host-side validation shared with `generate` (before any device work)"""
    if not _is_int(num_assistant_tokens) or not 1 <= num_assistant_tokens <= MAX_ASSISTANT_TOKENS:
        raise ValueError(f"num_assistant_tokens must be an int in [1, {MAX_ASSISTANT_TOKENS}], got {num_assistant_tokens!r}")
    if not _is_int(eos_token_id) or eos_token_id < 0:
        raise ValueError(f"eos_token_id must be an int >= 0, got {eos_token_id!r}")


def _check_tensors(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens):
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise ValueError(f"speculative_accept: logits must be (B, gamma + 1, V), got {tuple(logits.shape) if torch.is_tensor(logits) else type(logits).__name__}")
    B, M, V = logits.shape
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"speculative_accept: dtype {logits.dtype} (fp32, fp16 or bf16)")
    if not 2 <= M <= MAX_ASSISTANT_TOKENS + 1:
        raise ValueError(f"speculative_accept: logits holds {M} rows per batch element; gamma + 1 must be in [2, {MAX_ASSISTANT_TOKENS + 1}]")
    if not 1 <= V <= MAX_V:
        raise ValueError(f"speculative_accept: V {V} outside [1, {MAX_V}]")
    if B > 65535:
        raise ValueError(f"speculative_accept: B {B} (at most 65535)")
    if draft.dim() != 2 or tuple(draft.shape) != (B, M - 1) or draft.dtype != torch.int64:
        raise ValueError(f"speculative_accept: draft must be ({B}, {M - 1}) int64, got {draft.dtype} {tuple(draft.shape)}")
    if draft.stride(1) != 1 and M - 1 > 1:
        raise ValueError("speculative_accept: draft needs innermost stride 1")
    for name, t in (("cache_seqlens", cache_seqlens), ("draft_seqlens", draft_seqlens)):
        if t is not None and (t.dim() != 1 or t.shape[0] != B or t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError(f"speculative_accept: {name} must be a contiguous ({B},) int32 tensor, got {t.dtype} {tuple(t.shape)}")
    if labels.dim() != 2 or labels.shape[0] != B or labels.dtype != torch.int64 or labels.shape[1] < 2:
        raise ValueError(f"speculative_accept: labels must be ({B}, ncols >= 2) int64, got {labels.dtype} {tuple(labels.shape)}")
    if labels.stride(1) != 1 or (B > 1 and labels.stride(0) < labels.shape[1]):
        raise ValueError("speculative_accept: labels needs innermost stride 1 and non-overlapping rows")
    if tok.dim() != 1 or tok.shape[0] != B or tok.dtype != torch.int64 or not tok.is_contiguous():
        raise ValueError(f"speculative_accept: tok must be a contiguous ({B},) int64 tensor, got {tok.dtype} {tuple(tok.shape)}")
    if seen_eos.dim() != 1 or seen_eos.shape[0] != B or seen_eos.dtype != torch.bool or not seen_eos.is_contiguous():
        raise ValueError(f"speculative_accept: seen_eos must be a contiguous ({B},) bool tensor, got {seen_eos.dtype} {tuple(seen_eos.shape)}")
    if torch.is_tensor(limit):
        if limit.dim() != 1 or limit.shape[0] != B or limit.dtype != torch.int32 or not limit.is_contiguous():
            raise ValueError(f"speculative_accept: limit must be an int or a contiguous ({B},) int32 tensor, got {limit.dtype} {tuple(limit.shape)}")
    elif not _is_int(limit) or not -2 ** 31 <= limit < 2 ** 31:
        raise ValueError(f"speculative_accept: limit must be an int or a ({B},) int32 tensor, got {limit!r}")


def _check_devices(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens):
    if not logits.is_cuda:
        raise ValueError("speculative_accept: logits must be on the GPU (there is no CPU path)")
    for name, t in (("draft", draft), ("cache_seqlens", cache_seqlens), ("labels", labels), ("tok", tok), ("seen_eos", seen_eos),
                    ("limit", limit if torch.is_tensor(limit) else None), ("draft_seqlens", draft_seqlens)):
        if t is not None and t.device != logits.device:
            raise ValueError(f"speculative_accept: {name} must be on {logits.device}, got {t.device}")


def _fill_spec_params(p, logits, draft, cache_seqlens, labels, tok, seen_eos, limit, limit_scalar, draft_seqlens, eos_token_id,
                      n_accepted, n_new):
    """the fields of `SpecParams` both verification ops fill alike (the sampled op's struct embeds one as `spec`); the workspace
    is the op's own"""
    B, M, V = logits.shape
    p.B, p.M, p.V, p.dtype = B, M, V, _lib.dtype_code(logits.dtype)
    p.logits, p.batch_stride, p.row_stride = logits.data_ptr(), logits.stride(0), logits.stride(1)
    p.draft, p.draft_stride = draft.data_ptr(), draft.stride(0) if B > 1 else M - 1
    p.cache_seqlens = cache_seqlens.data_ptr()
    p.draft_seqlens = draft_seqlens.data_ptr() if draft_seqlens is not None else None
    p.labels, p.labels_stride, p.ncols = labels.data_ptr(), labels.stride(0) if B > 1 else labels.shape[1], labels.shape[1]
    p.eos_token_id = int(eos_token_id)
    p.tok, p.seen_eos = tok.data_ptr(), seen_eos.data_ptr()
    p.limit, p.limit_scalar = (limit.data_ptr(), 0) if limit is not None else (None, int(limit_scalar))
    p.n_accepted, p.n_new = n_accepted.data_ptr(), n_new.data_ptr()


@torch.library.custom_op("fat5::spec_accept", mutates_args=("cache_seqlens", "labels", "tok", "seen_eos", "draft_seqlens"),
                         device_types="cuda")
def spec_accept_op(logits: torch.Tensor, draft: torch.Tensor, cache_seqlens: torch.Tensor, labels: torch.Tensor, tok: torch.Tensor,
                   seen_eos: torch.Tensor, limit: Optional[torch.Tensor], limit_scalar: int, draft_seqlens: Optional[torch.Tensor],
                   eos_token_id: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(n_accepted, n_new), each (B,) int32; cache_seqlens, labels, tok, seen_eos and draft_seqlens are written in place
    (include/fat5.h, fat5_spec_accept)"""
    lim = limit if limit is not None else int(limit_scalar)
    _check_tensors(logits, draft, cache_seqlens, labels, tok, seen_eos, lim, draft_seqlens)
    _check_devices(logits, draft, cache_seqlens, labels, tok, seen_eos, lim, draft_seqlens)
    check_args(logits.shape[1] - 1, eos_token_id)
    B, M, V = logits.shape
    if logits.stride(2) != 1 or logits.stride(1) < V or (B > 1 and logits.stride(0) < (M - 1) * logits.stride(1) + V):
        logits = logits.contiguous()
    dev = logits.device
    n_accepted = torch.empty((B,), dtype=torch.int32, device=dev)
    n_new = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return n_accepted, n_new
    p = _lib.SpecParams()
    _fill_spec_params(p, logits, draft, cache_seqlens, labels, tok, seen_eos, limit, limit_scalar, draft_seqlens, eos_token_id,
                      n_accepted, n_new)
    lib = _lib.load()
    need = lib.fat5_spec_accept_workspace_bytes(p)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    with _lib.on_device(dev):
        _lib.check(lib.fat5_spec_accept(p, _lib.stream_ptr(dev)), "fat5_spec_accept")
    return n_accepted, n_new


@spec_accept_op.register_fake
def _spec_accept_fake(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, limit_scalar, draft_seqlens, eos_token_id):
    B = logits.shape[0]
    return logits.new_empty((B,), dtype=torch.int32), logits.new_empty((B,), dtype=torch.int32)


def check_sampling(sampling):
    """`sampling` = (temperature, top_k, top_p, seed) or (..., seed, offset) -> (float, int, float, int seed mod 2^64, int offset)"""
    from .sampling import check_args as check_warpers
    if not isinstance(sampling, (tuple, list)) or len(sampling) not in (4, 5):
        raise ValueError(f"sampling must be (temperature, top_k, top_p, seed) or (temperature, top_k, top_p, seed, offset), got {sampling!r}")
    temperature, top_k, top_p, seed = sampling[:4]
    offset = sampling[4] if len(sampling) == 5 else 0
    check_warpers(temperature, top_k, top_p)
    if not _is_int(seed) or not _is_int(offset):
        raise ValueError(f"sampling: seed and offset must be ints, got {seed!r} and {offset!r}")
    return float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset)


def _check_sampled_tensors(logits, draft_logits, uniforms):
    B, M, V = logits.shape
    if draft_logits is not None:
        if not torch.is_tensor(draft_logits) or tuple(draft_logits.shape) != (B, M - 1, V) or draft_logits.dtype != logits.dtype:
            got = f"{draft_logits.dtype} {tuple(draft_logits.shape)}" if torch.is_tensor(draft_logits) else type(draft_logits).__name__
            raise ValueError(f"speculative_accept: draft_logits must be ({B}, {M - 1}, {V}) {logits.dtype} (the dtype of logits), got {got}")
    if uniforms is not None:
        if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (B, M, 3) or uniforms.dtype != torch.float32 or not uniforms.is_contiguous():
            got = f"{uniforms.dtype} {tuple(uniforms.shape)}" if torch.is_tensor(uniforms) else type(uniforms).__name__
            raise ValueError(f"speculative_accept: uniforms must be a contiguous ({B}, {M}, 3) float32 tensor, got {got}")


@torch.library.custom_op("fat5::spec_accept_sampled", mutates_args=("cache_seqlens", "labels", "tok", "seen_eos", "draft_seqlens"),
                         device_types="cuda")
def spec_accept_sampled_op(logits: torch.Tensor, draft: torch.Tensor, cache_seqlens: torch.Tensor, labels: torch.Tensor,
                           tok: torch.Tensor, seen_eos: torch.Tensor, limit: Optional[torch.Tensor], limit_scalar: int,
                           draft_seqlens: Optional[torch.Tensor], eos_token_id: int, temperature: float, top_k: int, top_p: float,
                           seed: int, offset: int, draft_logits: Optional[torch.Tensor], uniforms: Optional[torch.Tensor],
                           return_sampled: bool, return_aux: bool) -> List[torch.Tensor]:
    """[n_accepted (B,) int32, n_new (B,) int32, sampled (B, M) int64, aux (B, M, 3) fp32] (the last two empty (0,) unless asked
    for); cache_seqlens, labels, tok, seen_eos and draft_seqlens are written in place (include/fat5.h, fat5_spec_accept_sampled)"""
    from .sampling import check_args as check_warpers
    lim = limit if limit is not None else int(limit_scalar)
    _check_tensors(logits, draft, cache_seqlens, labels, tok, seen_eos, lim, draft_seqlens)
    _check_sampled_tensors(logits, draft_logits, uniforms)
    _check_devices(logits, draft, cache_seqlens, labels, tok, seen_eos, lim, draft_seqlens)
    for name, t in (("draft_logits", draft_logits), ("uniforms", uniforms)):
        if t is not None and t.device != logits.device:
            raise ValueError(f"speculative_accept: {name} must be on {logits.device}, got {t.device}")
    check_args(logits.shape[1] - 1, eos_token_id)
    check_warpers(temperature, top_k, top_p)
    B, M, V = logits.shape
    if logits.stride(2) != 1 or logits.stride(1) < V or (B > 1 and logits.stride(0) < (M - 1) * logits.stride(1) + V):
        logits = logits.contiguous()
    if draft_logits is not None and (draft_logits.stride(2) != 1 or draft_logits.stride(1) < V
                                     or (B > 1 and draft_logits.stride(0) < (M - 2) * draft_logits.stride(1) + V)):
        draft_logits = draft_logits.contiguous()
    dev = logits.device
    n_accepted = torch.empty((B,), dtype=torch.int32, device=dev)
    n_new = torch.empty((B,), dtype=torch.int32, device=dev)
    sampled = torch.empty((B, M) if return_sampled else (0,), dtype=torch.int64, device=dev)
    aux = torch.empty((B, M, 3) if return_aux else (0,), dtype=torch.float32, device=dev)
    if B == 0:
        return [n_accepted, n_new, sampled, aux]
    q = _lib.SpecSampleParams()
    p = q.spec
    _fill_spec_params(p, logits, draft, cache_seqlens, labels, tok, seen_eos, limit, limit_scalar, draft_seqlens, eos_token_id,
                      n_accepted, n_new)
    if draft_logits is not None:
        q.draft_logits, q.draft_batch_stride, q.draft_row_stride = draft_logits.data_ptr(), draft_logits.stride(0), draft_logits.stride(1)
        if M - 1 == 1:   # (one row per batch element: its stride is never used)
            q.draft_row_stride = max(int(draft_logits.stride(1)), V)
    q.temperature, q.top_k, q.top_p = float(temperature), int(top_k), float(top_p)
    q.seed, q.offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset)
    q.uniforms = uniforms.data_ptr() if uniforms is not None else None
    q.sampled = sampled.data_ptr() if return_sampled else None
    q.aux = aux.data_ptr() if return_aux else None
    lib = _lib.load()
    need = lib.fat5_spec_accept_sampled_workspace_bytes(q)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    with _lib.on_device(dev):
        _lib.check(lib.fat5_spec_accept_sampled(q, _lib.stream_ptr(dev)), "fat5_spec_accept_sampled")
    return [n_accepted, n_new, sampled, aux]


@spec_accept_sampled_op.register_fake
def _spec_accept_sampled_fake(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, limit_scalar, draft_seqlens, eos_token_id,
                              temperature, top_k, top_p, seed, offset, draft_logits, uniforms, return_sampled, return_aux):
    B, M = logits.shape[0], logits.shape[1]
    return [logits.new_empty((B,), dtype=torch.int32), logits.new_empty((B,), dtype=torch.int32),
            logits.new_empty((B, M) if return_sampled else (0,), dtype=torch.int64),
            logits.new_empty((B, M, 3) if return_aux else (0,), dtype=torch.float32)]


def speculative_accept(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens=None, eos_token_id=1, *,
                       sampling=None, draft_logits=None, uniforms=None, return_sampled=False, return_aux=False):
    """Verify one round for all B rows on the device (one call, two launches, nothing read back).

    logits (B, gamma + 1, V) fp32 / bf16 / fp16: the target's logits of the chunk [tok, d_0 .. d_{gamma-1}]; draft (B, gamma) int64;
    cache_seqlens (B,) int32, ALREADY advanced by gamma + 1 by the chunk step; labels (B, ncols) int64, tok (B,) int64 and seen_eos
    (B,) bool: the running sequences, the pending tokens and the finished rows; limit: the last column of labels a row may write
    (prompt length - 1 + max_length), an int or a (B,) int32 device tensor; draft_seqlens: the drafter's length vector, set to the
    same value as cache_seqlens.

    sampling=None: the greedy rule, stated in include/fat5.h (fat5_spec_accept) and restated in tests/spec_ref.py.
    sampling=(temperature, top_k, top_p, seed[, offset]): speculative sampling (fat5_spec_accept_sampled; restated in
    tests/spec_sample_ref.py).  draft_logits (B, gamma, V), in the dtype of logits: row i holds the logits d_i was drawn from, under
    the same warpers; None: the drafts are taken as one-hot (accepted with probability p(d)).  Chunk row i uses the Philox block
    `sample_logits` would use for the token in column old + 1 + i; uniforms (B, gamma + 1, 3) fp32 replaces its three uniforms
    (u0: the draw after gamma accepted drafts, u1: the acceptance test, u2: the residual draw).  return_sampled adds (B, gamma + 1)
    int64, per chunk row the token it contributes (d_i, then the drawn token, then -1); return_aux adds the uniforms that were used,
    (B, gamma + 1, 3) fp32.

    Returns (n_accepted, n_new), both (B,) int32: the drafts that became output, and the tokens the row gained -- followed by
    `sampled` and `aux` when asked for."""
    check_args(logits.shape[1] - 1 if torch.is_tensor(logits) and logits.dim() == 3 else 1, eos_token_id)
    _check_tensors(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens)
    if sampling is None:
        if draft_logits is not None or uniforms is not None or return_sampled or return_aux:
            raise ValueError("speculative_accept: draft_logits, uniforms, return_sampled and return_aux belong to sampling=(...); "
                             "the greedy verification takes none of them")
    else:
        temperature, top_k, top_p, seed, offset = check_sampling(sampling)
        _check_sampled_tensors(logits, draft_logits, uniforms)
    _check_devices(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens)
    if torch.is_grad_enabled() and logits.requires_grad:
        logits = logits.detach()
    lim_t, lim_s = (limit, 0) if torch.is_tensor(limit) else (None, int(limit))
    if sampling is None:
        return spec_accept_op(logits, draft, cache_seqlens, labels, tok, seen_eos, lim_t, lim_s, draft_seqlens, int(eos_token_id))
    from .sampling import _u64
    if draft_logits is not None and torch.is_grad_enabled() and draft_logits.requires_grad:
        draft_logits = draft_logits.detach()
    n_acc, n_new, sampled, aux = spec_accept_sampled_op(
        logits, draft, cache_seqlens, labels, tok, seen_eos, lim_t, lim_s, draft_seqlens, int(eos_token_id), temperature, top_k, top_p,
        _u64(seed), offset, draft_logits, uniforms, bool(return_sampled), bool(return_aux))
    return (n_acc, n_new) + ((sampled,) if return_sampled else ()) + ((aux,) if return_aux else ())


@torch.no_grad()
def speculative_round(model, state, tok, draft, labels, seen_eos, limit, draft_state=None, *, sampling=None, draft_logits=None):
    """One verification round: `decode_chunk(model, state, cat(tok, draft), logits="all")`, then `speculative_accept`.  `draft`
    (B, gamma) int64 may come from anywhere (a model drafter, a script, an n-gram table); `draft_state` is the model drafter's
    DecodeState, whose lengths are rolled back with the target's.  The caches need room for limit + gamma + 1 positions.
    `sampling` and `draft_logits` are `speculative_accept`'s.  Returns (n_accepted, n_new)."""
    from .generation import decode_chunk
    # the rows' lengths live on the device and roll back every round: the host-side count of appended positions does not bound
    # this path (the kernel never moves a row past `limit`, and the chunk kernel drops rows past the capacity)
    state.steps = 0
    logits = decode_chunk(model, state, torch.cat((tok.unsqueeze(1), draft), 1), logits="all")
    return speculative_accept(logits, draft, state.cache_seqlens, labels, tok, seen_eos, limit,
                              draft_seqlens=None if draft_state is None else draft_state.cache_seqlens,
                              sampling=sampling, draft_logits=draft_logits)


@torch.no_grad()
def draft_tokens(assistant, draft_state, tok, draft, *, sampling=None, draft_logits=None):
    """the model drafter: gamma + 1 one-token steps from `tok`, the tokens of the first gamma written to `draft` (B, gamma) in
    place; the last step only appends d_{gamma-1}'s K / V, so that the cache is valid when every draft is accepted.
    sampling=None: the greedy tokens.  sampling=(temperature, top_k, top_p, seed): each token is drawn by `sample_logits` under
    the same warpers and the key seed ^ DRAFT_KEY (never the verifier's stream), with the drafter's own position as the counter,
    and each step's logits row is copied into draft_logits[:, i] -- a static (B, gamma, V) buffer, so a round stays one graph
    (None: a new one in the logits' dtype; allocate it outside a capture).  Returns draft_logits (None when greedy)."""
    from .generation import decode_step
    gamma = draft.shape[1]
    if sampling is not None:
        from .sampling import sample_logits
        temperature, top_k, top_p, seed = check_sampling(sampling)[:4]
    t = tok
    for i in range(gamma + 1):
        draft_state.steps = 0  # (as in speculative_round)
        lg = decode_step(assistant, draft_state, t)
        if i < gamma:
            t = draft[:, i]
            if sampling is None:
                t.copy_(lg.argmax(-1))
                continue
            if draft_logits is None:
                draft_logits = torch.empty((lg.shape[0], gamma, lg.shape[1]), dtype=lg.dtype, device=lg.device)
            draft_logits[:, i].copy_(lg)
            t.copy_(sample_logits(draft_logits[:, i], temperature, top_k, top_p, seed=seed ^ DRAFT_KEY, offsets=draft_state.cache_seqlens))
    return draft_logits if sampling is not None else None


def check_generate_args(model, assistant_model, input_ids, max_length, num_assistant_tokens, prompt_length, do_sample, num_beams,
                        processors_active):
    """`generate(assistant_model=...)`'s host-side rejections, before either encoder runs"""
    what = "generate: assistant_model (speculative decoding)"
    _check_single_sequence(what, num_beams, processors_active)
    check_args(num_assistant_tokens)
    _check_models(what, "must be", (("the model", model), ("the assistant", assistant_model)), input_ids, max_length,
                  num_assistant_tokens, "num_assistant_tokens", prompt_length, do_sample)


def _check_single_sequence(what, num_beams, processors_active):
    """what no drafter works with: beams, and logits processors"""
    if num_beams > 1:
        raise ValueError(f"{what} with num_beams > 1 is not supported: a beam has no single token for a draft to be checked against")
    if processors_active:
        raise ValueError(f"{what} with logits processors (repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens) "
                         "is not supported: the chunk's rows would each need the sequence up to their own position")


def _check_models(what, must_be, models, input_ids, max_length, gamma, gamma_name, prompt_length, do_sample):
    """the rejections of a speculative loop's `models` (("the model", model), then the assistant when it drafts), whatever drafts:
    the model type, one vocabulary, what the decode path refuses, the two RoPE limits (one rotary position per batch, the tables'
    rows) and last -- the sampler, the drafter's draws and the verification kernels have no CPU path -- inputs of a sampled call
    that are not on the GPU, refused here, before an encoder runs, not by the first launch"""
    from .generation import _check_supported
    for _, m in models:
        if not all(hasattr(m, a) for a in ("encoder", "decoder", "shared", "lm_head")):
            raise ValueError(f"{what} {must_be} a FAT5ForConditionalGeneration, got {type(m).__name__}")
    V, Va = (m.lm_head.weight.shape[0] for _, m in (models[0], models[-1]))
    if V != Va:
        raise ValueError(f"{what}: vocabulary mismatch, the model has {V} ids and the assistant {Va}")
    for _, m in models:
        _check_supported(m)
    cap = int(prompt_length) + int(max_length) + int(gamma) + 1
    for name, m in models:
        first = m.decoder.block[0].self_attention_layer.self_attention
        if not first.rotary:
            continue
        if input_ids.shape[0] > 1:
            raise ValueError(f"{what}: {name} uses RoPE and the batch holds {input_ids.shape[0]} rows; rows advance raggedly and the "
                             "decode path keeps one rotary position for the batch (B = 1 only)")
        if cap > first.pe_encoding.max_sequence_length:
            raise ValueError(f"{what}: the cache of {cap} positions (prompt + max_length + {gamma_name} + 1) exceeds the "
                             f"rotary tables' {first.pe_encoding.max_sequence_length} rows of {name}")
    if do_sample and not input_ids.is_cuda:
        raise ValueError(f"{what} with do_sample=True needs input_ids (and both models) on the GPU, got {input_ids.device}: "
                         "speculative sampling runs on HIP kernels only")


def check_lookup_generate_args(model, input_ids, max_length, prompt_lookup_num_tokens, max_matching_ngram_size, prompt_length,
                               do_sample, num_beams, processors_active, assistant_model=None):
    """`generate(prompt_lookup_num_tokens=...)`'s host-side rejections, before the encoder runs"""
    from .prompt_lookup import check_args as check_lookup_args
    what = "generate: prompt_lookup_num_tokens (prompt-lookup speculative decoding)"
    if assistant_model is not None:
        raise ValueError(f"{what} together with assistant_model is not supported: a round has one drafter")
    _check_single_sequence(what, num_beams, processors_active)
    check_lookup_args(prompt_lookup_num_tokens, max_matching_ngram_size, None, "generate",
                      ("prompt_lookup_num_tokens", "max_matching_ngram_size"))
    _check_models(what, "must be called on", (("the model", model),), input_ids, max_length, prompt_lookup_num_tokens,
                  "prompt_lookup_num_tokens", prompt_length, do_sample)


@torch.no_grad()
def speculative_generate(model, assistant_model, input_ids, attention_mask, max_length, graph, num_assistant_tokens, prompt_length,
                         decoder_input_ids, return_stats, kv_cache_dtype=None, lookup_ngram=None, sampling=None, weight_dtype=None):
    """`generate`'s speculative loop (the arguments are checked already): per round the drafter, one chunk step of the target
    and the verification kernel, then ONE host read (`seen_eos.all()`), as the plain loop does once per token.  The drafter is
    the assistant model (gamma + 1 draft steps) or, with `assistant_model=None`, the prompt lookup (ONE launch over
    input_ids and the rows' own sequences, `lookup_ngram` = N; no second model, no second state).  `attention_mask` is the validated
    `Padding` or None; its device lengths keep the padding of input_ids out of the lookup.  `sampling` = (temperature, top_k,
    top_p, seed) switches the round to speculative sampling: the assistant samples its drafts under a key of its own
    and hands its logits to the verification; the lookup's drafts are verified as one-hot"""
    from .generation import _prefill_prompt, _run_steps, finish_labels, init_decode_state
    lookup = assistant_model is None
    gamma, P, T_max = int(num_assistant_tokens), int(prompt_length), int(max_length)
    B, dev = input_ids.shape[0], input_ids.device
    # capacity P + max_length + gamma + 1: a row at its last free column still appends a whole chunk before the roll-back
    kv = {} if kv_cache_dtype is None else dict(kv_cache_dtype=kv_cache_dtype)   # (both models' caches take the dtype)
    if weight_dtype is not None:   # (and both decoders the weight dtype)
        kv["weight_dtype"] = weight_dtype
    state = init_decode_state(model, input_ids, T_max + gamma + 1, attention_mask, prompt_length=P, **kv)
    dstate = None if lookup else init_decode_state(assistant_model, input_ids, T_max + gamma + 1, attention_mask, prompt_length=P, **kv)
    labels = torch.zeros((B, P + T_max), dtype=torch.long, device=dev)
    limit = P - 1 + T_max
    tok = torch.zeros((B,), dtype=torch.long, device=dev)
    seen_eos = torch.zeros((B,), dtype=torch.bool, device=dev)
    draft = torch.zeros((B, gamma), dtype=torch.long, device=dev)
    # (live rows, accepted drafts) with an assistant; (proposed tokens, accepted ones) with the lookup
    stats = torch.zeros((2,), dtype=torch.long, device=dev) if return_stats else None
    if lookup:
        from .prompt_lookup import prompt_lookup_draft
        source = input_ids.to(torch.int64).contiguous()
        src_seqlens = None if attention_mask is None else attention_mask.lengths_dev
        N, V = int(lookup_ngram), int(model.lm_head.weight.shape[0])
    if decoder_input_ids is not None:
        _prefill_prompt(decoder_input_ids, P, labels, tok, (model, state), (assistant_model, dstate))
    dl = None  # the assistant's logits of a sampled round: allocated by the first (eager) round, static from then on

    def one_round():
        nonlocal dl
        if lookup:
            _, n_prop = prompt_lookup_draft(source, labels, state.cache_seqlens, tok, seen_eos, gamma, N, src_seqlens, V, out=draft)
        else:
            if stats is not None:
                stats[0].add_((~seen_eos).sum())
            dl = draft_tokens(assistant_model, dstate, tok, draft, sampling=sampling, draft_logits=dl)
        n_acc, _ = speculative_round(model, state, tok, draft, labels, seen_eos, limit, draft_state=dstate, sampling=sampling,
                                     draft_logits=dl)
        if stats is not None:
            if lookup:  # (a finished row proposes nothing; a filler the target agrees with is no accepted draft)
                stats[0].add_(n_prop.sum())
                n_acc = torch.minimum(n_acc, n_prop)
            stats[1].add_(n_acc.sum())

    rounds = _run_steps(one_round, lambda: bool(seen_eos.all()), T_max, graph)  # (every live row gains a token per round)
    T = int(state.cache_seqlens.max()) - (P - 1)  # the most new tokens any row produced
    out = finish_labels(labels[:, :P + T])
    if return_stats:
        first, acc = stats.tolist()
        return out, dict(rounds=rounds, drafted=first if lookup else first * gamma, accepted=acc)
    return out
