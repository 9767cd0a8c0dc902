"""Distilling one FAT5 into a smaller one: `DistilledFAT5(student, teacher)` is the training module of the student
-- a draft model for `generate(assistant_model=...)`, or a smaller model for the teacher's task.  Its loss is
`(1 - alpha) * ce + alpha * T^2 * KL(softmax(teacher / T) || softmax(student / T))` over the rows the student's own loss sees,
through the fused HIP loss of distillation.py; ce is the student's training loss with its label smoothing and z-loss.

    student = FAT5ForConditionalGeneration(small_config).cuda().bfloat16()
    model = DistilledFAT5(student, teacher, alpha=0.5, temperature=2.0)
    opt = AdamWScale(model.parameters(), lr=1e-3)            # the student's parameters only
    loss = train_step(model, input_ids, labels, opt)          # or GraphedTrainStep(model, opt)(input_ids, labels)
"""
import torch
from torch import nn

from .distillation import _lm_head_distillation, DistillationLoss, _check_mix

__all__ = ["DistilledFAT5"]


class DistilledFAT5(nn.Module):
    """`forward(input_ids, labels, ...)` returns the mean distillation loss over all rows (the denominator of the student's own
    loss).  The teacher is held OUTSIDE the module tree: `parameters()`, `state_dict()`, `train()` and `.to()` reach the student
    only, so `train_step`, `allreduce_gradients` and `GraphedTrainStep` take this module as they take a model.  The teacher is put
    in `eval()` once, runs under `no_grad`, and must already live on the student's device in the student's dtype.

    Both models must agree on `vocab_size`, `decoder_start_token_id` and `pad_token_id` (ValueError otherwise): the teacher reads
    the student's batch -- for padded or packed batches the pack plan is made once, by the student, and both run over the same
    valid tokens.  `last_kd_loss` and `last_ce_loss` are the means of the bare KL and of the bare cross-entropy term of the last
    forward: detached device scalars (no host read; under a captured step they are static tensors that every replay overwrites)."""

    def __init__(self, student, teacher, alpha=0.5, temperature=2.0):
        super().__init__()
        _check_mix(alpha, temperature)
        for name in ("vocab_size", "decoder_start_token_id", "pad_token_id"):
            a, b = getattr(student.config, name), getattr(teacher.config, name)
            if a != b:
                raise ValueError(f"DistilledFAT5: the student's {name} = {a} is not the teacher's ({b})")
        self.student = student
        self._teacher = (teacher.eval(),)  # (a tuple: nn.Module registers no submodule, so no parameter of it is this module's)
        self.alpha, self.temperature = float(alpha), float(temperature)
        self.last_kd_loss = self.last_ce_loss = None

    @property
    def teacher(self):
        return self._teacher[0]

    @property
    def config(self):
        return self.student.config

    def rpe_tables(self):
        return self.student.rpe_tables()

    def forward(self, input_ids, labels, attention_mask=None, decoder_attention_mask=None, segment_ids=None, decoder_segment_ids=None):
        student, teacher = self.student, self.teacher
        sw, tw = student.lm_head.weight, teacher.lm_head.weight
        if tw.device != sw.device or tw.dtype != sw.dtype:   # (.to() / .cuda() / .bfloat16() on this module reach the student only)
            raise RuntimeError(f"DistilledFAT5: the teacher is on {tw.device} in {tw.dtype}, the student on {sw.device} in {sw.dtype}; "
                               "the teacher lives outside the module tree, move or cast it yourself (model.teacher.to(...))")
        plan = student._plan(input_ids, labels, attention_mask, decoder_attention_mask, segment_ids, decoder_segment_ids)
        if plan is not None:
            teacher.packed_supported()
        dec, lab = student._decoder_states(plan, input_ids, labels)
        with torch.no_grad():
            tdec, _ = teacher._decoder_states(plan, input_ids, labels)
        c = student.config
        if c.fuse_lm_head_ce:
            loss, kd, _, ce = _lm_head_distillation(dec, student.lm_head.weight, tdec, teacher.lm_head.weight, lab, self.alpha,
                                                    self.temperature, c.label_smoothing, 1.0, c.z_loss, -100, None, "mean")
        else:  # full logits, as the student's own loss has them
            logits = student.lm_head(dec)
            with torch.no_grad():
                tlogits = teacher.lm_head(tdec)
            V = logits.shape[-1]
            losses, kd, _, ce = DistillationLoss.apply(logits.view(-1, V), tlogits.view(-1, V), lab.reshape(-1), self.alpha, self.temperature,
                                                   c.label_smoothing, 1.0, c.z_loss, -100, c.crossentropy_inplace_backward)
            loss, kd, ce = losses.mean(), kd.mean(), ce.mean()
        self.last_kd_loss, self.last_ce_loss = kd.detach(), ce.detach()
        return loss
