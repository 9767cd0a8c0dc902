"""Knowledge distillation on MI355X: the student's cross-entropy mixed with the forward KL to a teacher at a temperature, in one
pass over the two logits rows (csrc/kd_kernels.h).

    p = softmax(t / T)     q = softmax(s / T)     kd = sum_j p_j (log p_j - log q_j)
    loss = (1 - alpha) * cross_entropy_loss(s, y, ...) + alpha * T^2 * kd
    d loss / d s_j = (1 - alpha) * d ce / d s_j + alpha * T * (q_j - p_j)          (the teacher gets no gradient)

`distillation_loss` takes the two `(rows, vocab)` logits tensors; `lm_head_distillation` takes the two models' hidden states and
lm_head weights and never holds more than one row chunk of either logits tensor (the chunked form of `lm_head_cross_entropy`).
"""
import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from .lm_head_cross_entropy import _chunks, _dh_gemm

__all__ = ["distillation_loss", "DistillationLoss", "lm_head_distillation", "LMHeadDistillation", "LMHeadDistillationMean"]


def _ready(t):
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(entry, logits, teacher, labels, cfg, dlosses=None, losses=None, kd=None, z=None, ce=None, lse=None, lse_s=None, lse_t=None,
            dlogits=None):
    """fill a fat5_kd_params for (rows, V) tensors and call `entry` (fat5_kd_fwd / fat5_kd_bwd / fat5_kd_fwd_bwd) on the current stream"""
    alpha, temperature, smoothing, logit_scale, lse_square_scale, ignore_index = cfg
    p = _lib.KdParams()
    p.dtype = _lib.dtype_code(logits.dtype)
    p.rows, p.n_cols = logits.shape
    p.logits, p.row_stride = logits.data_ptr(), logits.stride(0)
    p.teacher_logits, p.teacher_row_stride = teacher.data_ptr(), teacher.stride(0)
    p.labels = labels.data_ptr()
    if dlosses is not None:
        p.dlosses, p.dloss_stride = dlosses.data_ptr(), dlosses.stride(0)
    p.losses, p.kd_losses, p.z_losses, p.ce_losses = _ptr(losses), _ptr(kd), _ptr(z), _ptr(ce)
    p.lse, p.lse_student_t, p.lse_teacher_t = _ptr(lse), _ptr(lse_s), _ptr(lse_t)
    if dlogits is not None:
        p.dlogits, p.dlogits_row_stride = dlogits.data_ptr(), dlogits.stride(0)
    p.ignore_index = int(ignore_index)
    p.alpha, p.temperature = float(alpha), float(temperature)
    p.label_smoothing, p.logit_scale, p.lse_square_scale = float(smoothing), float(logit_scale), float(lse_square_scale)
    lib = _lib.load()
    with _lib.on_device(logits.device):
        _lib.check(getattr(lib, entry)(ctypes.byref(p), _lib.stream_ptr(logits.device)), entry)


def _check_pair(logits, teacher_logits):
    if logits.dim() != 2 or teacher_logits.shape != logits.shape or teacher_logits.dtype != logits.dtype:
        raise ValueError(f"student logits {tuple(logits.shape)} {logits.dtype} and teacher logits {tuple(teacher_logits.shape)} "
                         f"{teacher_logits.dtype} must be (rows, vocab) tensors of one shape and dtype")


@torch.library.custom_op("fat5::distillation_fwd", mutates_args=(), device_types="cuda")
def distillation_fwd(logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor, alpha: float, temperature: float,
                     smoothing: float, logit_scale: float, lse_square_scale: float, ignore_index: int
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fat5_kd_fwd -> (losses, kd_losses, z_losses, ce_losses, lse, lse_student_t, lse_teacher_t), fp32 per row"""
    _check_pair(logits, teacher_logits)
    if not _ready(logits):
        logits = logits.contiguous()
    if not _ready(teacher_logits):
        teacher_logits = teacher_logits.contiguous()
    n_rows = logits.shape[0]
    labels = labels.to(torch.int64).contiguous()
    outs = tuple(torch.empty(n_rows, dtype=torch.float32, device=logits.device) for _ in range(7))
    if n_rows > 0:
        losses, kd, z, ce, lse, lse_s, lse_t = outs
        _launch("fat5_kd_fwd", logits, teacher_logits, labels, (alpha, temperature, smoothing, logit_scale, lse_square_scale, ignore_index),
                losses=losses, kd=kd, z=z, ce=ce, lse=lse, lse_s=lse_s, lse_t=lse_t)
    return outs


@torch.library.register_fake("fat5::distillation_fwd")
def _distillation_fwd_fake(logits, teacher_logits, labels, alpha, temperature, smoothing, logit_scale, lse_square_scale, ignore_index):
    return tuple(torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device) for _ in range(7))


@torch.library.custom_op("fat5::distillation_bwd", mutates_args={"logits"}, device_types="cuda")
def distillation_bwd(dlosses: torch.Tensor, logits: torch.Tensor, teacher_logits: torch.Tensor, lse: torch.Tensor, lse_student_t: torch.Tensor,
                     lse_teacher_t: torch.Tensor, labels: torch.Tensor, inplace_backward: bool, alpha: float, temperature: float,
                     smoothing: float, logit_scale: float, lse_square_scale: float, ignore_index: int) -> torch.Tensor:
    """fat5_kd_bwd.  With `inplace_backward` the gradient overwrites `logits` and an empty tensor is returned."""
    _check_pair(logits, teacher_logits)
    n_rows, n_cols = logits.shape
    src = logits
    if not _ready(logits):
        if inplace_backward:
            raise RuntimeError("inplace_backward needs logits with unit inner stride and 16-byte alignment")
        src = logits.contiguous()
    if not _ready(teacher_logits):
        teacher_logits = teacher_logits.contiguous()
    dlogits = src if inplace_backward else torch.empty((n_rows, n_cols), dtype=logits.dtype, device=logits.device)
    labels = labels.to(torch.int64).contiguous()
    dlosses = dlosses.to(torch.float32)
    if n_rows > 0:
        _launch("fat5_kd_bwd", src, teacher_logits, labels, (alpha, temperature, smoothing, logit_scale, lse_square_scale, ignore_index),
                dlosses=dlosses, lse=lse, lse_s=lse_student_t, lse_t=lse_teacher_t, dlogits=dlogits)
    if inplace_backward:
        return torch.empty(0, dtype=logits.dtype, device=logits.device)
    return dlogits


@torch.library.register_fake("fat5::distillation_bwd")
def _distillation_bwd_fake(dlosses, logits, teacher_logits, lse, lse_student_t, lse_teacher_t, labels, inplace_backward, alpha, temperature,
                           smoothing, logit_scale, lse_square_scale, ignore_index):
    if inplace_backward:
        return torch.empty(0, dtype=logits.dtype, device=logits.device)
    return torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)


def distillation_fwd_bwd_(logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor, dlosses: torch.Tensor,
                          losses: torch.Tensor, kd_losses: torch.Tensor, z_losses: torch.Tensor, ce_losses: Optional[torch.Tensor],
                          lse: torch.Tensor, lse_student_t: torch.Tensor, lse_teacher_t: torch.Tensor, alpha: float, temperature: float,
                          smoothing: float, logit_scale: float, lse_square_scale: float, ignore_index: int) -> None:
    """forward AND backward of every row in one launch (fat5_kd_fwd_bwd): writes the per-row outputs (fp32, caller-provided slices)
    and overwrites `logits` with d loss / d logits for the upstream gradients `dlosses` (fp32, one per row, or one element with
    stride 0 via expand).  Same bits as distillation_fwd followed by distillation_bwd(inplace).  `teacher_logits` is only read."""
    _check_pair(logits, teacher_logits)
    if not _ready(logits) or not _ready(teacher_logits):
        raise RuntimeError("distillation_fwd_bwd_ needs logits with unit inner stride and 16-byte alignment")
    if logits.shape[0] == 0:
        return
    labels = labels.to(torch.int64).contiguous()
    per_row = [losses, kd_losses, z_losses, lse, lse_student_t, lse_teacher_t] + ([] if ce_losses is None else [ce_losses])
    assert dlosses.dtype == torch.float32 and all(t.dtype == torch.float32 and t.is_contiguous() for t in per_row)
    _launch("fat5_kd_fwd_bwd", logits, teacher_logits, labels, (alpha, temperature, smoothing, logit_scale, lse_square_scale, ignore_index),
            dlosses=dlosses, losses=losses, kd=kd_losses, z=z_losses, ce=ce_losses, lse=lse, lse_s=lse_student_t, lse_t=lse_teacher_t,
            dlogits=logits)


def _check_mix(alpha, temperature):
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha = {alpha} outside [0, 1]")
    if not (float(temperature) > 0.0 and float(temperature) != float("inf")):
        raise ValueError(f"temperature = {temperature} must be finite and > 0")


class DistillationLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, teacher_logits, labels, alpha, temperature, smoothing, logit_scale, lse_square_scale, ignore_index,
                inplace_backward):
        n_rows = logits.shape[0]
        assert labels.shape == (n_rows,)
        cfg = (float(alpha), float(temperature), float(smoothing), float(logit_scale), float(lse_square_scale), int(ignore_index))
        losses, kd, z, ce, lse, lse_s, lse_t = torch.ops.fat5.distillation_fwd(logits, teacher_logits, labels, *cfg)
        ctx.save_for_backward(logits, teacher_logits, lse, lse_s, lse_t, labels)
        ctx.mark_non_differentiable(kd, z, ce)
        ctx.cfg = cfg + (bool(inplace_backward),)
        return losses, kd, z, ce

    @staticmethod
    def backward(ctx, grad_losses, grad_kd, grad_z, grad_ce):
        del grad_kd, grad_z, grad_ce  # (for logging only)
        logits, teacher_logits, lse, lse_s, lse_t, labels = ctx.saved_tensors
        inplace = ctx.cfg[-1]
        dlogits = torch.ops.fat5.distillation_bwd(grad_losses.contiguous(), logits, teacher_logits, lse, lse_s, lse_t, labels, inplace,
                                                  *ctx.cfg[:-1])
        if inplace:
            dlogits = logits
        return (dlogits,) + (None,) * 9


def distillation_loss(logits: torch.Tensor, teacher_logits: torch.Tensor, labels: torch.Tensor, alpha: float = 0.5,
                      temperature: float = 1.0, label_smoothing: float = 0.0, logit_scale: float = 1.0, lse_square_scale: float = 0.0,
                      ignore_index: int = -100, inplace_backward: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """logits, teacher_logits (..., vocab) of one dtype, labels (...): returns (losses, kd_losses, z_losses), fp32 per row.
    losses = (1 - alpha) * ce + alpha * temperature^2 * kd, with ce the row loss of `cross_entropy_loss(logits, labels,
    label_smoothing=..., logit_scale=..., lse_square_scale=...)` (the z-loss inside it) and kd the forward KL of the student's
    softmax(logits / temperature) from the teacher's; label_smoothing, logit_scale and lse_square_scale act on ce only.
    kd_losses (the bare kd) and z_losses are for logging and not differentiable.  The teacher gets no gradient.

    A row whose label is `ignore_index` gives zeros everywhere, gradient row included; a label outside the vocabulary that is not
    `ignore_index` keeps `cross_entropy_loss`'s meaning and its kd still counts.  A teacher column at -inf (a masked part of the
    vocabulary) adds exactly 0 to kd and pushes the student's probability there down, also where the student is -inf too.  A row
    whose teacher logits are ALL -inf is outside the contract: nothing rejects it on the device, and its kd is NaN.
    With alpha == 0 loss and gradient have the bits of `cross_entropy_loss`."""
    if not logits.is_cuda:
        raise RuntimeError("flasht5_amd operators need tensors on the HIP device (no CPU fallback)")
    _check_mix(alpha, temperature)
    V = logits.shape[-1]
    return DistillationLoss.apply(logits.view(-1, V), teacher_logits.detach().view(-1, V), labels.view(-1), alpha, temperature,
                                  label_smoothing, logit_scale, lse_square_scale, ignore_index, inplace_backward)[:3]


# ------------------------------------------------------------------------------------------------------------------------------
# lm_head -> distillation loss without either (rows, vocab) logits tensor
# ------------------------------------------------------------------------------------------------------------------------------
def _addmm_dw(dw, dlogits, hidden, first):
    """dW (+)= dlogits^T hidden with fp32 accumulation over the chunks (lm_head_cross_entropy's form)"""
    if dw.dtype == hidden.dtype:
        torch.mm(dlogits.t(), hidden, out=dw) if first else dw.addmm_(dlogits.t(), hidden)
    elif first:
        torch.mm(dlogits.t(), hidden, out_dtype=torch.float32, out=dw)
    else:
        torch.addmm(dw, dlogits.t(), hidden, out_dtype=torch.float32, out=dw)


class LMHeadDistillation(torch.autograd.Function):
    """per-row losses; the backward recomputes both chunks of logits"""

    @staticmethod
    def forward(ctx, hidden, weight, teacher_hidden, teacher_weight, labels, cfg, chunk_rows):
        rows, dev = hidden.shape[0], hidden.device
        losses, kd, z, ce, lse, lse_s, lse_t = (torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(7))
        wt, twt = weight.t(), teacher_weight.t()
        m = min(rows, chunk_rows)
        buf = torch.empty((m, weight.shape[0]), dtype=hidden.dtype, device=dev)    # ONE chunk of each model's logits, reused
        tbuf = torch.empty((m, weight.shape[0]), dtype=hidden.dtype, device=dev)
        for s, e in _chunks(rows, chunk_rows):
            logits = torch.mm(hidden[s:e], wt, out=buf[:e - s])
            tlogits = torch.mm(teacher_hidden[s:e], twt, out=tbuf[:e - s])
            _launch("fat5_kd_fwd", logits, tlogits, labels[s:e], cfg, losses=losses[s:e], kd=kd[s:e], z=z[s:e], ce=ce[s:e], lse=lse[s:e],
                    lse_s=lse_s[s:e], lse_t=lse_t[s:e])
        ctx.save_for_backward(hidden, weight, teacher_hidden, teacher_weight, labels, lse, lse_s, lse_t)
        ctx.cfg, ctx.chunk_rows = cfg, chunk_rows
        ctx.mark_non_differentiable(kd, z, ce)
        return losses, kd, z, ce

    @staticmethod
    def backward(ctx, grad_losses, grad_kd, grad_z, grad_ce):
        del grad_kd, grad_z, grad_ce
        hidden, weight, teacher_hidden, teacher_weight, labels, lse, lse_s, lse_t = ctx.saved_tensors
        cfg, chunk_rows = ctx.cfg, ctx.chunk_rows
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        rows, dev = hidden.shape[0], hidden.device
        dh = torch.empty_like(hidden) if need_h else None
        dw = torch.zeros(weight.shape, dtype=torch.float32, device=dev) if need_w else None
        g = grad_losses.contiguous().float()
        wt, twt = weight.t(), teacher_weight.t()
        m = min(rows, chunk_rows)
        buf = torch.empty((m, weight.shape[0]), dtype=hidden.dtype, device=dev)
        tbuf = torch.empty((m, weight.shape[0]), dtype=hidden.dtype, device=dev)
        for s, e in _chunks(rows, chunk_rows):
            logits = torch.mm(hidden[s:e], wt, out=buf[:e - s])
            tlogits = torch.mm(teacher_hidden[s:e], twt, out=tbuf[:e - s])
            _launch("fat5_kd_bwd", logits, tlogits, labels[s:e], cfg, dlosses=g[s:e], lse=lse[s:e], lse_s=lse_s[s:e], lse_t=lse_t[s:e],
                    dlogits=logits)
            if need_h:
                dh[s:e] = _dh_gemm(logits, weight)                       # logits now holds dlogits (in place)
            if need_w:
                _addmm_dw(dw, logits, hidden[s:e], False)
        return dh, (dw.to(weight.dtype) if need_w else None), None, None, None, None, None


class LMHeadDistillationMean(torch.autograd.Function):
    """the MEAN over all rows with the gradients formed in the forward pass, chunk by chunk (LMHeadCrossEntropyMean's form): every
    row's upstream gradient is 1 / rows, so fat5_kd_fwd_bwd turns a chunk of student logits into its gradient in place"""

    @staticmethod
    def forward(ctx, hidden, weight, teacher_hidden, teacher_weight, labels, cfg, chunk_rows):
        rows, dev = hidden.shape[0], hidden.device
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        losses, kd, z, ce, lse, lse_s, lse_t = (torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(7))
        dh = torch.empty_like(hidden) if need_h else None
        dw = torch.empty(weight.shape, dtype=torch.float32, device=dev) if need_w else None
        wt, twt = weight.t(), teacher_weight.t()
        g = torch.full((1,), 1.0 / max(rows, 1), dtype=torch.float32, device=dev)
        m = min(rows, chunk_rows)
        buf = torch.empty((m, weight.shape[0]), dtype=hidden.dtype, device=dev)
        tbuf = torch.empty((m, weight.shape[0]), dtype=hidden.dtype, device=dev)
        for s, e in _chunks(rows, chunk_rows):
            logits = torch.mm(hidden[s:e], wt, out=buf[:e - s])
            tlogits = torch.mm(teacher_hidden[s:e], twt, out=tbuf[:e - s])
            out = dict(losses=losses[s:e], kd=kd[s:e], z=z[s:e], ce=ce[s:e], lse=lse[s:e], lse_s=lse_s[s:e], lse_t=lse_t[s:e])
            if need_h or need_w:
                _launch("fat5_kd_fwd_bwd", logits, tlogits, labels[s:e], cfg, dlosses=g.expand(e - s), dlogits=logits, **out)
                if need_h:
                    _dh_gemm(logits, weight, out=dh[s:e])                # logits now holds dlogits (in place)
                if need_w:
                    _addmm_dw(dw, logits, hidden[s:e], s == 0)
            else:
                _launch("fat5_kd_fwd", logits, tlogits, labels[s:e], cfg, **out)
        if rows == 0 and dw is not None:
            dw.zero_()
        if need_w and dw.dtype != weight.dtype:
            dw = dw.to(weight.dtype)
        ctx.save_for_backward(dh, dw)
        n = max(rows, 1)
        means = tuple(t.sum() / n for t in (losses, kd, z, ce))   # per-row values summed ONCE at the end (fixed order)
        ctx.mark_non_differentiable(*means[1:])
        return means

    @staticmethod
    def backward(ctx, grad_loss, grad_kd, grad_z, grad_ce):
        del grad_kd, grad_z, grad_ce
        dh, dw = ctx.saved_tensors
        gl = grad_loss.float()   # (applied in fp32, as LMHeadCrossEntropyMean does)

        def rescale(t):
            return None if t is None else (t if t.dtype == torch.float32 else t.float()).mul(gl).to(t.dtype)
        return rescale(dh), rescale(dw), None, None, None, None, None


def _lm_head_distillation(hidden, weight, teacher_hidden, teacher_weight, labels, alpha, temperature, label_smoothing, logit_scale,
                          lse_square_scale, ignore_index, chunk_rows, reduction):
    """-> (losses, kd_losses, z_losses, ce_losses): `lm_head_distillation` plus the bare cross-entropy term (DistilledFAT5 logs it)"""
    if not hidden.is_cuda:
        raise RuntimeError("flasht5_amd operators need tensors on the HIP device (no CPU fallback)")
    if reduction not in ("none", "mean"):
        raise ValueError("reduction must be 'none' or 'mean'")
    _check_mix(alpha, temperature)
    h2 = hidden.reshape(-1, hidden.shape[-1])
    th2 = teacher_hidden.detach().reshape(-1, teacher_hidden.shape[-1])
    tw = teacher_weight.detach()
    lab = labels.reshape(-1).to(torch.int64).contiguous()
    if lab.shape[0] != h2.shape[0] or th2.shape[0] != h2.shape[0] or weight.shape[1] != h2.shape[1] or tw.shape[1] != th2.shape[1]:
        raise ValueError(f"hidden {tuple(hidden.shape)}, weight {tuple(weight.shape)}, teacher_hidden {tuple(teacher_hidden.shape)}, "
                         f"teacher_weight {tuple(teacher_weight.shape)}, labels {tuple(labels.shape)} do not match")
    if tw.shape[0] != weight.shape[0]:
        raise ValueError(f"the teacher's vocabulary ({tw.shape[0]}) is not the student's ({weight.shape[0]})")
    if th2.dtype != h2.dtype or tw.dtype != th2.dtype or weight.dtype != h2.dtype:
        raise ValueError("hidden, weight, teacher_hidden and teacher_weight must share one dtype")
    if chunk_rows is None:  # ~64 MB of logits per model and chunk, as lm_head_cross_entropy; the mean form takes chunks twice as long
        chunk_rows = max(256, ((128 if reduction == "mean" else 64) << 20) // (weight.shape[0] * h2.element_size()) // 256 * 256)
    cfg = (float(alpha), float(temperature), float(label_smoothing), float(logit_scale), float(lse_square_scale), int(ignore_index))
    fn = LMHeadDistillationMean if reduction == "mean" else LMHeadDistillation
    return fn.apply(h2, weight, th2, tw, lab, cfg, int(chunk_rows))


def lm_head_distillation(hidden: torch.Tensor, weight: torch.Tensor, teacher_hidden: torch.Tensor, teacher_weight: torch.Tensor,
                         labels: torch.Tensor, alpha: float = 0.5, temperature: float = 1.0, label_smoothing: float = 0.0,
                         logit_scale: float = 1.0, lse_square_scale: float = 0.0, ignore_index: int = -100,
                         chunk_rows: Optional[int] = None, reduction: str = "none"
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """hidden (..., d_student), weight (vocab, d_student), teacher_hidden (..., d_teacher), teacher_weight (vocab, d_teacher), labels
    (...): returns (losses, kd_losses, z_losses), fp32 per row, equal to `distillation_loss(hidden @ weight.T, teacher_hidden @
    teacher_weight.T, labels, ...)` with neither logits tensor ever whole: per chunk of `chunk_rows` rows both lm_head GEMMs write
    into two reused buffers that the HIP kernels consume.  The two models may differ in width, not in vocabulary or dtype.
    reduction="mean": three scalars, the means over ALL rows (the denominator of `lm_head_cross_entropy(reduction="mean")`), with
    the gradients formed during the forward pass (fat5_kd_fwd_bwd in place: no recomputation); reduction="none" recomputes both
    chunks in the backward.  Gradients flow to `hidden` and `weight` only."""
    return _lm_head_distillation(hidden, weight, teacher_hidden, teacher_weight, labels, alpha, temperature, label_smoothing, logit_scale,
                                 lse_square_scale, ignore_index, chunk_rows, reduction)[:3]
