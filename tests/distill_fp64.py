"""fp64 restatements of the distillation loss, written from its definition (TEST INFRASTRUCTURE ONLY).

Per row, with student logits s, teacher logits t, a label y, a temperature T > 0 and a weight alpha in [0, 1]:

    p = softmax(t / T)        q = softmax(s / T)        kd = sum_j p_j (log p_j - log q_j)
    ce = the row loss of rowwise_fp64.ce_fwd(s, y, smoothing, logit_scale, lse_square_scale)   (z-loss inside)
    loss = (1 - alpha) ce + alpha T^2 kd
    d loss / d s_j = (1 - alpha) d ce / d s_j + alpha T (q_j - p_j)

A column with t_j = -inf has p_j = 0 and adds 0 to kd (0 log 0 = 0), whatever s_j is.  A row with y == ignore_index has loss = kd
= z = ce = 0 and a zero gradient row.  Everything takes the tensors a kernel reads -- already rounded to their dtype -- and
returns float64 on the CPU: no intermediate rounding.  tests/test_distill_cpu.py pins these to torch.nn.functional.kl_div +
cross_entropy.
"""
import torch

import rowwise_fp64 as R


def _d(t):
    return t.double().cpu()


def kd_terms(logits, teacher, temperature):
    """-> (kd, q, p, log q, log p) per row / element, in fp64"""
    s, t = _d(logits) / temperature, _d(teacher) / temperature
    logq, logp = torch.log_softmax(s, -1), torch.log_softmax(t, -1)
    p = torch.exp(logp)
    term = torch.where(p > 0, p * (logp - logq), torch.zeros_like(p))  # 0 log 0 = 0 (and no -inf - -inf)
    return term.sum(-1), torch.exp(logq), p, logq, logp


def kd_fwd(logits, teacher, labels, alpha, temperature, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """-> (loss, kd, z, ce, lse, lse_student_t, lse_teacher_t) per row"""
    ce, z, lse = R.ce_fwd(logits, labels, smoothing, logit_scale, lse_square_scale, ignore_index)
    kd = kd_terms(logits, teacher, temperature)[0]
    ign = labels.cpu() == ignore_index
    kd = torch.where(ign, torch.zeros_like(kd), kd)
    loss = (1 - alpha) * ce + alpha * temperature ** 2 * kd
    return (loss, kd, z, ce, lse, torch.logsumexp(_d(logits) / temperature, -1), torch.logsumexp(_d(teacher) / temperature, -1))


def kd_bwd(dlosses, logits, teacher, labels, alpha, temperature, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """-> d loss / d logits (rows, V) for the upstream gradients dlosses (rows,) or a scalar; 0 on ignored rows"""
    dce = R.ce_bwd(dlosses, logits, labels, smoothing, logit_scale, lse_square_scale, ignore_index)
    _, q, p, _, _ = kd_terms(logits, teacher, temperature)
    dl = torch.where(labels.cpu() == ignore_index, torch.zeros(()).double(), _d(dlosses).expand(labels.shape))
    return (1 - alpha) * dce + (dl * alpha * temperature).unsqueeze(-1) * (q - p)
