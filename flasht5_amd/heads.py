"""The reference's four encoder-only models (src/model/custom_heads_flash_t5.py, `FlashT5EncoderModel`) on this project's encoder:
a sentence encoder and the token-classification, sequence-classification and extractive-QA heads a pre-trained FAT5 is fine-tuned
with.  Parameter names are the reference's -- `shared`, `encoder.*`, `classifier.*`, `classification_head.dense.*` /
`.out_proj.*`, `qa_outputs.*` -- so a reference state dict loads with strict=True.

    FAT5EncoderModel(config)(input_ids, attention_mask=None, pool=None)      -> (B, L, d_model), or (B, d_model) with a pooling mode
    FAT5ForTokenClassification(config)(input_ids, labels=None, attention_mask=None)     -> loss, or logits (B, L, num_labels)
    FAT5ForSequenceClassification(config)(input_ids, labels=None, attention_mask=None)  -> loss, or logits (B, num_labels)
    FAT5ForQuestionAnswering(config)(input_ids, labels=None, attention_mask=None)       -> loss, or (start, end) logits (B, L)

Fine-tuning batches are padded, so everything sits on the packed path: with a right-padded `attention_mask` the
encoder runs over the valid tokens only (`pack_plan`: the one host read), the heads run on the packed rows and per-token outputs
are scattered back to (B, L).  A row is classified as it would be alone: what the padding holds reaches no bit of the logits, the
loss or a gradient.  An all-ones mask, or none, is the unpadded path bit for bit.  `train_step(model, input_ids, labels, optimizer,
attention_mask=mask)` and `GraphedTrainStep(model, optimizer)` (unpadded batches) take the three heads as they are.

Where this differs from the reference: the loss and the QA softmax run over valid positions only (the reference lets padded
positions into both); logits at padding are 0, or the dtype's minimum for QA (the reference leaves what the encoder computed
there); a sequence without an <eos> is pooled from its last token and flagged -- `FAT5ForSequenceClassification.check` is the
optional host read that raises for it -- where the reference raises inside every forward."""
import copy

import torch
import torch.distributed as dist
from torch import nn

from .cross_entropy_loss import cross_entropy_loss
from .fat5_step import FAT5Config, FAT5Stack, _Drop, init_stack_weights
from .pooling import MODES, sequence_pool

__all__ = ["FAT5EncoderModel", "FAT5ForTokenClassification", "FAT5ForSequenceClassification", "FAT5ForQuestionAnswering"]


class _Rows:
    """the encoder output of one forward as rows: h (rows, d_model) -- the valid tokens of a padded batch (`plan` set), or all
    B * L of them -- with the ids that belong to the rows"""
    __slots__ = ("h", "ids", "plan", "B", "L")

    def __init__(self, h, ids, plan, B, L):
        self.h, self.ids, self.plan, self.B, self.L = h, ids, plan, B, L

    def gather(self, per_token):
        """a (B, L) tensor as one value per row of h"""
        flat = per_token.reshape(-1)
        return flat if self.plan is None else flat.index_select(0, self.plan.index)

    def scatter(self, rows, fill=0.0):
        """(rows, C) -> (B, L, C), `fill` at the padded positions"""
        if self.plan is None:
            return rows.reshape(self.B, self.L, rows.shape[-1])
        out = rows.new_full((self.B * self.L, rows.shape[-1]), fill)
        return out.index_copy(0, self.plan.index, rows).reshape(self.B, self.L, rows.shape[-1])

    def lengths(self):
        """(B,) valid tokens per row"""
        if self.plan is None:
            return torch.full((self.B,), self.L, dtype=torch.int64, device=self.h.device)
        cu = self.plan.cu_seqlens.long()
        return cu[1:] - cu[:-1]

    def pool(self, mode, eos_token_id):
        if self.plan is None:
            return sequence_pool(self.h.reshape(self.B, self.L, -1), mode, input_ids=self.ids.reshape(self.B, self.L), eos_token_id=eos_token_id)
        return sequence_pool(self.h, mode, cu_seqlens=self.plan.cu_seqlens, input_ids=self.ids, eos_token_id=eos_token_id)


class _EncoderOnly(nn.Module):
    """`shared` + `encoder` with the reference's initialisation, the padded-batch plumbing and the dropout context"""
    head_sites = 0   # dropout sites of the head, numbered from encoder.next_site

    def __init__(self, config: FAT5Config):
        super().__init__()
        self.config = config
        self.shared = nn.Embedding(config.vocab_size, config.d_model)
        enc = copy.copy(config)
        enc.is_decoder = False
        self.encoder = FAT5Stack(enc, self.shared, config.num_layers)
        # dropout: as in FAT5ForConditionalGeneration, a step counter outside the state dict, advanced on the device
        self.dropout_seed = config.dropout_seed
        if config.dropout_rate > 0 or (self.head_sites and config.classifier_dropout > 0):
            if self.dropout_seed is None:
                self.dropout_seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64))
            self.register_buffer("dropout_step", torch.zeros(1, dtype=torch.int64), persistent=False)

    @torch.no_grad()
    def reset_parameters(self):
        """the reference's `_init_weights` for the embedding and the encoder (factor 1.0); the heads initialise their own layers"""
        self.shared.weight.normal_(0.0, 1.0)
        init_stack_weights(self, self.config)

    def _drops(self):
        """(the encoder's dropout context, the head's), each None when it has nothing to do (eval, or a zero rate: no new launch).
        Both read one copy of the step counter, which is advanced on the device right away (FAT5ForConditionalGeneration._drop)."""
        c = self.config
        p_enc = float(c.dropout_rate) if self.training else 0.0
        p_head = float(c.classifier_dropout) if self.training and self.head_sites else 0.0
        if p_enc == 0.0 and p_head == 0.0:
            return None, None
        from .dropout import rank_key
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        key = rank_key(self.dropout_seed, rank)
        step = self.dropout_step.clone()
        self.dropout_step.add_(1)
        return (_Drop(p_enc, key, step) if p_enc > 0 else None), (_Drop(p_head, key, step) if p_head > 0 else None)

    def _plan(self, input_ids, attention_mask):
        """the PackPlan of a padded batch (one host read), or None when nothing is padded"""
        if input_ids.dim() != 2:
            raise ValueError(f"forward: input_ids must be (B, L), got {tuple(input_ids.shape)}")
        if attention_mask is None:
            return None
        if not torch.is_tensor(attention_mask) or tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"forward: attention_mask must be a (B, L) = {tuple(input_ids.shape)} tensor like input_ids, got "
                             f"{tuple(attention_mask.shape) if torch.is_tensor(attention_mask) else type(attention_mask).__name__}")
        if attention_mask.dtype.is_floating_point or attention_mask.dtype.is_complex:
            raise ValueError(f"forward: attention_mask must be a bool or integer tensor, got {attention_mask.dtype}")
        from .packing import pack_plan
        plan = pack_plan(attention_mask.to(input_ids.device) != 0, name="attention_mask")
        if plan.nseq == input_ids.shape[0] and plan.total == input_ids.numel():
            return None
        self.encoder.block[0].self_attention_layer.self_attention.packed_supported()   # (NotImplementedError: dense bias, FIRE, ...)
        return plan

    def _encode(self, input_ids, attention_mask):
        """-> (_Rows, the head's dropout context)"""
        from .packing import Packed
        plan = self._plan(input_ids, attention_mask)
        drop, head_drop = self._drops()
        B, L = input_ids.shape
        if plan is None:
            ids = input_ids.reshape(-1)
            h = self.encoder(input_ids, drop=drop)
        else:
            ids = input_ids.reshape(-1).index_select(0, plan.index)
            h = self.encoder(ids.unsqueeze(0), packing=Packed(plan.cu_seqlens, plan.max_seqlen), drop=drop)
        return _Rows(h.reshape(-1, h.shape[-1]), ids, plan, B, L), head_drop

    def _head_drop(self, x, drop, k):
        """the head's k-th dropout site"""
        return x if drop is None else drop(x, self.encoder.next_site + k)


class FAT5EncoderModel(_EncoderOnly):
    """The reference's `FlashT5EncoderModel`: the encoder alone, optionally pooled to one vector per sequence."""

    def __init__(self, config: FAT5Config):
        super().__init__(config)
        self.reset_parameters()

    def forward(self, input_ids, attention_mask=None, pool=None):
        """pool None: last_hidden_state (B, L, d_model), zero at the padded positions; "eos", "mean", "first" or "last": (B, d_model)
        through `sequence_pool` over each row's valid tokens"""
        if pool is not None and pool not in MODES:
            raise ValueError(f"forward: pool {pool!r} (None or one of {', '.join(repr(m) for m in MODES)})")
        rows, _ = self._encode(input_ids, attention_mask)
        if pool is None:
            return rows.scatter(rows.h)
        return rows.pool(pool, self.config.eos_token_id)[0]


def _masked_mean(losses, counted):
    """the mean of the per-row losses over the rows that count (ignored rows hold 0); 0 when none does"""
    return losses.sum() / counted.sum().clamp(min=1).to(losses.dtype)


class FAT5ForTokenClassification(_EncoderOnly):
    """The reference's `FlashT5ForTokenClassification`: encoder -> dropout -> `classifier`, one label per token."""
    head_sites = 1

    def __init__(self, config: FAT5Config):
        super().__init__(config)
        self.num_labels = config.num_labels
        self.classifier = nn.Linear(config.d_model, config.num_labels)
        self.reset_parameters()
        with torch.no_grad():   # custom_heads_flash_t5.py:35-36
            self.classifier.weight.normal_(0.0, 1.0)
            self.classifier.bias.zero_()

    def forward(self, input_ids, labels=None, attention_mask=None, return_logits=False):
        """labels (B, L) int64, -100 = ignored: the loss, a mean over the labels that are not -100 at valid positions.  Without
        labels: logits (B, L, num_labels), 0 at the padded positions.  return_logits with labels: (loss, logits)."""
        rows, drop = self._encode(input_ids, attention_mask)
        logits = self.classifier(self._head_drop(rows.h, drop, 0))
        if labels is None:
            return rows.scatter(logits)
        if tuple(labels.shape) != tuple(input_ids.shape):
            raise ValueError(f"forward: labels must be (B, L) = {tuple(input_ids.shape)}, got {tuple(labels.shape)}")
        lab = rows.gather(labels.to(logits.device))
        loss = _masked_mean(cross_entropy_loss(logits, lab)[0], lab != -100)
        return (loss, rows.scatter(logits)) if return_logits else loss


class FAT5ClassificationHead(nn.Module):
    """The reference's `FlashT5ClassificationHead`: dropout, dense, tanh, dropout, out_proj (the dropouts are the model's sites)."""

    def __init__(self, config: FAT5Config):
        super().__init__()
        self.dense = nn.Linear(config.d_model, config.d_model)
        self.out_proj = nn.Linear(config.d_model, config.num_labels)
        with torch.no_grad():   # custom_heads_flash_t5.py:99-105
            self.dense.weight.normal_(0.0, config.d_model ** -0.5)
            self.dense.bias.zero_()
            self.out_proj.weight.normal_(0.0, config.d_model ** -0.5)
            self.out_proj.bias.zero_()


class FAT5ForSequenceClassification(_EncoderOnly):
    """The reference's `FlashT5ForSequenceClassification`: encoder -> the row of the last <eos> -> classification head."""
    head_sites = 2
    PROBLEM_TYPES = ("regression", "single_label_classification", "multi_label_classification")

    def __init__(self, config: FAT5Config, problem_type=None):
        super().__init__(config)
        if problem_type is not None and problem_type not in self.PROBLEM_TYPES:
            raise ValueError(f"problem_type {problem_type!r} (None or one of {self.PROBLEM_TYPES})")
        self.num_labels = config.num_labels
        self.problem_type = problem_type
        self.last_found = None
        self.reset_parameters()
        self.classification_head = FAT5ClassificationHead(config)

    def resolve_problem_type(self, labels):
        """the reference's rule (custom_heads_flash_t5.py:191-197), fixed by the first labels the model sees"""
        if self.problem_type is None:
            if self.num_labels == 1:
                self.problem_type = "regression"
            elif labels.dtype in (torch.long, torch.int):
                self.problem_type = "single_label_classification"
            else:
                self.problem_type = "multi_label_classification"
        return self.problem_type

    def forward(self, input_ids, labels=None, attention_mask=None, return_logits=False):
        """labels: (B,) integer classes, (B,) / (B, 1) regression targets (num_labels == 1) or (B, num_labels) floating-point
        multi-label targets -> the loss; without labels: logits (B, num_labels), fp32.  return_logits with labels: (loss, logits).
        Nothing is read on the host: `last_found` keeps the (B,) int32 flags of this forward for `check`."""
        rows, drop = self._encode(input_ids, attention_mask)
        pooled, _, found = rows.pool("eos", self.config.eos_token_id)
        self.last_found = found
        # the head works on B rows: its two small GEMMs, the tanh, the logits and the loss stay in fp32 whatever the model's dtype
        # (three 16-bit roundings in a row cost more than the one-rounding bound the other heads' logits are held to, and 16-bit
        # logit gradients would be summed over the batch after rounding); the parameter gradients are rounded once, on the way back
        head, lin = self.classification_head, nn.functional.linear
        x = torch.tanh(lin(self._head_drop(pooled, drop, 0).float(), head.dense.weight.float(), head.dense.bias.float()))
        logits = lin(self._head_drop(x, drop, 1), head.out_proj.weight.float(), head.out_proj.bias.float())
        if labels is None:
            return logits
        labels = labels.to(logits.device)
        kind = self.resolve_problem_type(labels)
        if kind == "regression":
            if self.num_labels == 1:
                loss = nn.functional.mse_loss(logits.squeeze(-1), labels.reshape(-1).to(logits.dtype))
            else:
                loss = nn.functional.mse_loss(logits, labels.to(logits.dtype))
        elif kind == "single_label_classification":
            lab = labels.reshape(-1)
            loss = _masked_mean(cross_entropy_loss(logits, lab)[0], lab != -100)
        else:
            loss = nn.functional.binary_cross_entropy_with_logits(logits, labels.to(logits.dtype))
        return (loss, logits) if return_logits else loss

    def check(self, found=None):
        """the one optional host read: ValueError naming the rows of `found` (default: the last forward's) without an <eos> inside
        their own length -- what the reference raises for inside every forward"""
        found = self.last_found if found is None else found
        if found is None:
            raise RuntimeError("check: no forward has run yet")
        missing = [i for i, f in enumerate(found.tolist()) if not f]
        if missing:
            raise ValueError(f"row(s) {missing} hold no <eos> (id {self.config.eos_token_id}) among their valid tokens: they were pooled "
                             "from their last token")


class FAT5ForQuestionAnswering(_EncoderOnly):
    """The reference's `FlashT5ForQuestionAnswering`: encoder -> `qa_outputs`, start and end logits per token."""

    def __init__(self, config: FAT5Config):
        super().__init__(config)
        if config.num_labels != 2:
            raise ValueError(f"FAT5ForQuestionAnswering needs num_labels = 2 (start, end), got {config.num_labels}")
        self.qa_outputs = nn.Linear(config.d_model, config.num_labels)
        self.reset_parameters()
        with torch.no_grad():   # custom_heads_flash_t5.py:239-240
            self.qa_outputs.weight.normal_(0.0, 1.0)
            self.qa_outputs.bias.zero_()

    def forward(self, input_ids, labels=None, attention_mask=None, start_positions=None, end_positions=None, return_logits=False):
        """labels (B, 2) = [start, end], or start_positions= / end_positions= (B,): the reference's loss -- positions clamped to
        [0, L], L ignored, the mean of the two cross-entropies over the (B, L) start / end logits -- with a target in a row's
        padding ignored as well.  Without targets: (start_logits, end_logits), both (B, L), the dtype's minimum at the padded
        positions.  return_logits with targets: (loss, start_logits, end_logits)."""
        if labels is not None:
            if start_positions is not None or end_positions is not None:
                raise ValueError("forward: labels (B, 2) or start_positions / end_positions, not both")
            if labels.dim() != 2 or tuple(labels.shape) != (input_ids.shape[0], 2):
                raise ValueError(f"forward: labels must be (B, 2) = [start, end], got {tuple(labels.shape)}")
            start_positions, end_positions = labels[:, 0], labels[:, 1]
        elif (start_positions is None) != (end_positions is None):
            raise ValueError("forward: start_positions and end_positions come together")
        rows, _ = self._encode(input_ids, attention_mask)
        logits = self.qa_outputs(rows.h)
        full = rows.scatter(logits, torch.finfo(logits.dtype).min)
        # (copies, never views of `full`: the loss op's backward is declared to write its logits, and at L = 1 a slice is contiguous)
        start_logits, end_logits = (full[..., k].clone(memory_format=torch.contiguous_format) for k in (0, 1))
        if start_positions is None:
            return start_logits, end_logits
        L, lengths = rows.L, rows.lengths()
        losses = []
        for lg, pos in ((start_logits, start_positions), (end_logits, end_positions)):
            pos = pos.to(lg.device).reshape(-1).long().clamp(0, L)
            pos = torch.where(pos >= lengths, torch.full_like(pos, L), pos)
            losses.append(_masked_mean(cross_entropy_loss(lg, pos, ignore_index=L)[0], pos != L))
        loss = (losses[0] + losses[1]) / 2
        return (loss, start_logits, end_logits) if return_logits else loss
