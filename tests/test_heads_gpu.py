"""GPU tests of the encoder-only models (flasht5_amd/heads.py): FAT5EncoderModel and the token-classification,
sequence-classification and question-answering heads, on padded batches.

Model (that of tests/test_packed_train_gpu.py): 2 layers, d_model 128, d_kv 64, 2 heads, d_ff 256, vocabulary 512, bf16; T5 bias
(fat5_rpe) and RoPE.  Batch: B = 3, L = 80, lengths (80, 33, 1), the <eos> (id 1) last in each row."""
import math

import pytest
import torch

import pool_ref as R

pytestmark = pytest.mark.gpu

L = 80
LENS = (80, 33, 1)
PES = ["t5", "RoPE"]
HEADS = ["token", "sequence", "qa"]
EOS = 1
NUM_LABELS = {"token": 5, "sequence": 5, "qa": 2}


@pytest.fixture
def torch_deterministic():
    """the exact tests compare two runs bit for bit: torch's deterministic mode, as in tests/test_packed_train_gpu.py (the backward
    of the table lookup behind the T5 bias is an index_add_ otherwise)"""
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


def make_model(head, pe, seed=5, **flags):
    import flasht5_amd as F
    cls = {"token": F.FAT5ForTokenClassification, "sequence": F.FAT5ForSequenceClassification, "qa": F.FAT5ForQuestionAnswering,
           "encoder": F.FAT5EncoderModel}[head]
    cfg = F.FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=2, num_decoder_layers=2,
                       position_encoding_type=pe, num_labels=NUM_LABELS.get(head, 2), **flags)
    torch.manual_seed(seed)
    return cls(cfg).cuda().bfloat16()


def examples(head, lens=LENS, seed=1):
    """[(ids (n,) ending in <eos>, label)]: one class per token / one class / (start, end) inside the example"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        x = torch.randint(2, 512, (n,), generator=g)
        x[-1] = EOS
        if head == "token":
            y = torch.randint(0, NUM_LABELS[head], (n,), generator=g)
        elif head == "sequence":
            y = torch.randint(0, NUM_LABELS[head], (), generator=g)
        else:
            y = torch.randint(0, n, (2,), generator=g)
        out.append((x, y))
    return out


def padded(head, exs, garbage=None):
    """(ids (B, L), labels, attention_mask) on the device; `garbage`: a seed for what the padded positions hold instead of 0 / -100
    -- other ids, an <eos> right behind every short row, other labels"""
    B = len(exs)
    ids = torch.zeros(B, L, dtype=torch.long)
    tok = torch.full((B, L), -100, dtype=torch.long)
    if garbage is not None:
        g = torch.Generator().manual_seed(garbage)
        ids = torch.randint(0, 512, (B, L), generator=g)
        tok = torch.randint(0, NUM_LABELS["token"], (B, L), generator=g)
    am = torch.zeros(B, L, dtype=torch.bool)
    for b, (x, y) in enumerate(exs):
        if garbage is not None and len(x) < L:
            ids[b, len(x)] = EOS
        ids[b, :len(x)] = x
        am[b, :len(x)] = True
        if head == "token":
            tok[b, :len(x)] = y
    labels = tok if head == "token" else torch.stack([y for _, y in exs])
    return ids.cuda(), labels.cuda(), am.cuda()


def run(model, ids, labels, **kw):
    """-> (loss, logits tuple, {name: gradient})"""
    model.zero_grad(set_to_none=True)
    out = model(ids, labels, return_logits=True, **kw)
    out[0].backward()
    return out[0].detach().clone(), tuple(t.detach().clone() for t in out[1:]), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def same_bits(a, b):
    assert torch.equal(a[0], b[0]), (a[0].item(), b[0].item())
    assert len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[2].keys() == b[2].keys()
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def valid_logits(head, logits, lens):
    """the logits of the valid positions, row after row, as one fp32 tensor"""
    if head == "sequence":
        return logits[0].float()
    if head == "token":
        return torch.cat([logits[0][b, :n].float() for b, n in enumerate(lens)])
    return torch.cat([torch.stack([logits[0][b, :n], logits[1][b, :n]], -1).float() for b, n in enumerate(lens)])


def alone_combined(head, model, exs):
    """every example through the unmasked forward on its own (B = 1), combined by label counts: the token loss is a mean over an
    example's n tokens, the other two are one term per row"""
    parts = []
    for x, y in exs:
        r = run(model, x[None].cuda(), y[None].cuda())
        parts.append((r, len(x) if head == "token" else 1, valid_logits(head, r[1], [len(x)])))
    n = sum(c for _, c, _ in parts)
    loss = sum(r[0].float() * c for r, c, _ in parts) / n
    grads = {k: sum(r[2][k].float() * c for r, c, _ in parts) / n for k in parts[0][0][2]}
    return loss, torch.cat([lg for _, _, lg in parts]), grads


def rel_err(head, got, ref, lens):
    """max-abs error relative to the tensor's max-abs: the loss, the valid logits, every gradient"""
    mx = lambda a, r: (a.float() - r.float()).abs().max().item() / max(r.float().abs().max().item(), 1e-30)  # noqa: E731
    out = {"loss": abs(got[0].item() - ref[0].item()) / abs(ref[0].item()), "logits": mx(valid_logits(head, got[1], lens), ref[1])}
    for n, r in ref[2].items():
        out[n] = mx(got[2][n], r)
    return out


# ---------------------------------------------------------------- 1, 2: exact
@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_padding_garbage_changes_no_bit(head, pe, torch_deterministic):
    """what the padded positions hold -- other ids, other labels, an <eos> under the padding -- reaches no bit of the logits, the
    loss or a gradient"""
    model = make_model(head, pe)
    exs = examples(head)
    ids0, lab0, am = padded(head, exs)
    ids1, lab1, _ = padded(head, exs, garbage=9)
    assert not torch.equal(ids0, ids1) and bool((ids1[1, LENS[1]:] == EOS).any())
    a = run(model, ids0, lab0, attention_mask=am)
    b = run(model, ids1, lab1, attention_mask=am)
    same_bits(a, b)
    assert torch.isfinite(a[0]) and all(torch.isfinite(g.float()).all() for g in a[2].values())
    if head == "token":      # logits at the padding are 0
        assert not bool(a[1][0][~am].float().abs().sum()) and bool(a[1][0][am].float().abs().sum())
    if head == "qa":         # ... or the dtype's minimum
        assert bool((a[1][0][~am] == torch.finfo(torch.bfloat16).min).all()) and bool((a[1][1][~am] == torch.finfo(torch.bfloat16).min).all())
    if head == "sequence":
        model.check()        # every row holds its <eos> inside its length
        assert model.last_found.tolist() == [1, 1, 1]


@pytest.mark.parametrize("pe", PES)
def test_encoder_model_on_padded_rows(pe, torch_deterministic):
    """the pooled outputs and the hidden states: garbage under the padding changes no bit, the padded positions are zero, and an
    all-ones mask is the unmasked path"""
    model = make_model("encoder", pe)
    exs = examples("sequence")
    ids0, _, am = padded("sequence", exs)
    ids1, _, _ = padded("sequence", exs, garbage=9)
    h0, h1 = model(ids0, attention_mask=am), model(ids1, attention_mask=am.long())
    assert h0.shape == (3, L, 128) and torch.equal(h0, h1)
    assert not bool(h0[~am].float().abs().sum()) and bool(torch.isfinite(h0.float()).all())
    for pool in ("eos", "mean", "first", "last"):
        p0, p1 = model(ids0, attention_mask=am, pool=pool), model(ids1, attention_mask=am, pool=pool)
        assert p0.shape == (3, 128) and torch.equal(p0, p1)
        rows = {"eos": [n - 1 for n in LENS], "last": [n - 1 for n in LENS], "first": [0, 0, 0]}.get(pool)
        if rows is not None:
            assert torch.equal(p0, torch.stack([h0[b, j] for b, j in enumerate(rows)]))
    full, _, _ = padded("sequence", examples("sequence", (L,) * 3, seed=2))
    for pool in (None, "eos", "mean"):
        assert torch.equal(model(full, pool=pool), model(full, attention_mask=torch.ones_like(full), pool=pool))
    with pytest.raises(ValueError):
        model(full, pool="max")
    with pytest.raises(ValueError):
        model(full, attention_mask=torch.ones(3, L, device="cuda"))


@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_all_ones_masks_are_the_unmasked_path(head, pe, torch_deterministic):
    model = make_model(head, pe)
    ids, labels, _ = padded(head, examples(head, (L,) * 3))
    ref = run(model, ids, labels)
    same_bits(ref, run(model, ids, labels, attention_mask=torch.ones_like(ids)))
    same_bits(ref, run(model, ids, labels, attention_mask=torch.ones_like(ids, dtype=torch.bool)))


# ---------------------------------------------------------------- 3: a row is classified as it is classified alone
@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_a_row_is_classified_as_alone(head, pe):
    """The logits, the loss and every parameter gradient of the padded batch against each example run alone (unpadded, B = 1),
    combined by label counts.  The bound is that of tests/test_packed_train_gpu.py: 4 x the batch-composition floor, per tensor, as
    max-abs relative to the tensor's max-abs; the floor is measured here on three equal-length rows through the unmasked path.
    Without the mask the same comparison must break the bound.  Every figure is printed; DESIGN 4.24 records them.

    Measured (MI355X, this file's seeds): the logits agree bit for bit on every path; gradient floors 1.4e-3 .. 2.0e-2 (the QA
    head's `qa_outputs.bias`, whose exact gradient is zero, 2.3 .. 5.0), padded gradients up to 1.4e-2 (that bias 0.18), the worst
    tensor per case at 1.65 .. 3.40 x its floor (3.40: `classification_head.out_proj.bias`, RoPE); without the mask 2.5e-2 .. 0.29
    on the loss, 0.45 .. 0.99 on the logits and 2.0 .. 4.1 on the gradients."""
    model = make_model(head, pe)
    full = examples(head, (L,) * 3, seed=2)
    ids, labels, _ = padded(head, full)
    floor = rel_err(head, run(model, ids, labels), alone_combined(head, model, full), (L,) * 3)

    exs = examples(head)
    ids, labels, am = padded(head, exs)
    ref = alone_combined(head, model, exs)
    err = rel_err(head, run(model, ids, labels, attention_mask=am), ref, LENS)
    nomask = rel_err(head, run(model, ids, labels), ref, LENS)
    floor["loss"] += 16 * 2.0 ** -24   # (the same per-row fp32 values summed in another order: that file's allowance)
    worst = max(err, key=lambda n: err[n] / max(floor[n], 1e-30))
    grads = lambda e: [v for k, v in e.items() if k not in ("loss", "logits")]  # noqa: E731
    print(f"[heads-vs-alone {head} {pe}] floor: loss {floor['loss']:.3e}, logits {floor['logits']:.3e}, gradients {min(grads(floor)):.3e} .. "
          f"{max(grads(floor)):.3e}; padded: loss {err['loss']:.3e}, logits {err['logits']:.3e}, gradients up to {max(grads(err)):.3e}; "
          f"worst ratio {err[worst] / max(floor[worst], 1e-30):.2f} ({worst}); no mask: loss {nomask['loss']:.3e}, logits "
          f"{nomask['logits']:.3e}, gradients up to {max(grads(nomask)):.3e}")
    for n in sorted(err):
        print(f"[heads-vs-alone {head} {pe}]   {n}: floor {floor[n]:.3e} padded {err[n]:.3e} nomask {nomask[n]:.3e}")
    bad = {n: (err[n], floor[n]) for n in err if err[n] > 4 * floor[n]}
    assert not bad, bad
    assert any(nomask[n] > 4 * floor[n] for n in nomask), "dropping the mask must break the bound"


# ---------------------------------------------------------------- 4: the heads against an fp32 restatement
@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_head_against_fp32_restatement(head, pe):
    """the reference's few lines of torch (custom_heads_flash_t5.py) in fp32 on the model's own encoder output, `pool_ref` for the
    pooling: logits within (1e-3 + 2^-8) max(1, max|ref|), head-parameter gradients within (1e-3 + 3 * 2^-8) max(1, max|ref|)"""
    import torch.nn.functional as Fn
    model = make_model(head, pe)
    exs = examples(head)
    ids, labels, am = padded(head, exs)
    seen = []
    hook = model.encoder.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    got = run(model, ids, labels, attention_mask=am)
    hook.remove()
    h = seen[0].reshape(-1, 128).float()                                 # the packed rows, in order
    assert h.shape[0] == sum(LENS)
    cu = [0, LENS[0], LENS[0] + LENS[1], sum(LENS)]
    names = [n for n, _ in model.named_parameters() if not n.startswith(("shared.", "encoder."))]
    prm = {n: p.detach().float().requires_grad_(True) for n, p in model.named_parameters() if n in names}
    if head == "token":
        logits = h @ prm["classifier.weight"].T + prm["classifier.bias"]
        loss = Fn.cross_entropy(logits, torch.cat([y for _, y in exs]).cuda())
    elif head == "sequence":
        ref = R.pool_ref(h.cpu(), "eos", cu_seqlens=torch.tensor(cu, dtype=torch.int32), input_ids=torch.cat([x for x, _ in exs]), eos_token_id=EOS)
        assert ref["position"] == [n - 1 for n in LENS] and ref["found"] == [1, 1, 1]
        x = torch.tanh(ref["pooled"].float().cuda() @ prm["classification_head.dense.weight"].T + prm["classification_head.dense.bias"])
        logits = x @ prm["classification_head.out_proj.weight"].T + prm["classification_head.out_proj.bias"]
        loss = Fn.cross_entropy(logits, labels)
    else:
        logits = h @ prm["qa_outputs.weight"].T + prm["qa_outputs.bias"]  # (total, 2): softmax over each row's own positions
        per_row = [logits[cu[b]:cu[b + 1]] for b in range(3)]
        loss = sum(Fn.cross_entropy(r[:, k][None], labels[b, k][None]) for b, r in enumerate(per_row) for k in (0, 1)) / 6
    loss.backward()
    mine = valid_logits(head, got[1], LENS)
    bound = (1e-3 + 2.0 ** -8) * max(1.0, logits.abs().max().item())
    assert (mine - logits.detach()).abs().max().item() <= bound
    assert abs(got[0].item() - loss.item()) <= (1e-3 + 2.0 ** -8) * max(1.0, abs(loss.item()))
    for n in names:
        rg = prm[n].grad
        d = (got[2][n].float() - rg).abs().max().item()
        assert d <= (1e-3 + 3 * 2.0 ** -8) * max(1.0, rg.abs().max().item()), (n, d, rg.abs().max().item())


# ---------------------------------------------------------------- 5: rows without an <eos>
@pytest.mark.parametrize("pe", PES)
def test_check_names_the_rows_without_eos(pe):
    model = make_model("sequence", pe)
    ids, labels, am = padded("sequence", examples("sequence"), garbage=4)   # (an <eos> under row 1's padding: it must not count)
    model(ids, labels, attention_mask=am)
    model.check()
    ids[1, LENS[1] - 1] = 7
    logits = model(ids, attention_mask=am)
    assert logits.shape == (3, NUM_LABELS["sequence"]) and model.last_found.tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match=r"\[1\]"):
        model.check()
    with pytest.raises(ValueError, match=r"\[1\]"):
        model.check(model.last_found)
    model.check(torch.ones(3, dtype=torch.int32))


# ---------------------------------------------------------------- 6, 7: the optimizer step
@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_train_step_with_a_mask_updates_every_parameter(head, pe):
    from flasht5_amd import AdamWScale, train_step
    model = make_model(head, pe)
    opt = AdamWScale(model.parameters(), lr=1e-2, max_grad_norm=1.0)
    before = [p.detach().clone() for p in model.parameters()]
    ids, labels, am = padded(head, examples(head))
    losses = [train_step(model, ids, labels, opt, max_grad_norm=None, attention_mask=am).item() for _ in range(2)]
    assert all(math.isfinite(l) for l in losses)
    for (n, p), b in zip(model.named_parameters(), before):
        assert not torch.equal(p.detach(), b), n


@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_graphed_train_step_follows_the_eager_step(head, pe, torch_deterministic):
    """unpadded batches; the comparison of tests/test_fire_gpu.py's captured step.

    Under torch's deterministic mode, for the reason the exact tests give: the backward of the table lookup behind the T5 bias
    (`index_select` on the bf16 table) is an `index_add_` with atomics whose bf16 sums depend on the order of arrival, eager or
    captured alike (FIRE, which that file's model uses, has no such table).  Measured without the mode (MI355X, four runs of this
    test): token, sequence and every RoPE case bit for bit in all five losses and all parameters; QA with the T5 bias -- logits of
    the magnitude of sqrt(d_model) and a loss that is a mean over 2 B terms -- anywhere from 2.1e-4 to 2.4e-3 on the losses from
    one run of the same two programs to the next.  That noise is torch's operator's, not the captured step's, and the comparison
    is about the latter.  The test prints every figure."""
    from flasht5_amd import AdamWScale, train_step, GraphedTrainStep
    batches = [padded(head, examples(head, (L,) * 3, seed=10 + i))[:2] for i in range(5)]
    lrs = [1e-3, 2e-3, 3e-3, 2e-3, 1e-3]
    runs = []
    for graphed in (False, True):
        model = make_model(head, pe, seed=7)
        opt = AdamWScale(model.parameters(), lr=lrs[0], kahan_sum=True, max_grad_norm=1.0)
        step = GraphedTrainStep(model, opt, warmup=2) if graphed else (lambda i, l: train_step(model, i, l, opt, max_grad_norm=None))
        losses = []
        for (ids, labels), lr in zip(batches, lrs):
            for grp in opt.param_groups:
                grp["lr"] = lr
            losses.append(float(step(ids, labels)))
        if graphed:
            assert step.graphs is not None
            step.close()
        runs.append((losses, [p.detach().float().clone() for p in model.parameters()]))
    (l0, p0), (l1, p1) = runs
    print(f"[heads-graphed {head} {pe}] loss, eager against captured, relative: {[f'{abs(a - b) / abs(a):.2e}' for a, b in zip(l0, l1)]}; "
          f"parameters, worst max-abs relative: {max(float((a - b).abs().max()) / max(float(a.abs().max()), 1e-3) for a, b in zip(p0, p1)):.2e}")
    assert all(math.isfinite(a) for a in l0)
    assert l0[0] == l1[0]
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for a, b in zip(p0, p1):
        assert float((a - b).abs().max()) <= 2.0 ** -6 * max(float(a.abs().max()), 1e-3)


# ---------------------------------------------------------------- 8: the heads' dropout
@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("head", HEADS)
def test_classifier_dropout(head, pe, torch_deterministic):
    """classifier_dropout = 0.1: two training forwards differ (new masks: the step counter moved on the device) and eval() is the
    zero-rate model bit for bit.  The QA head has no dropout site, in the reference as here: the rate changes nothing."""
    plain = make_model(head, pe)
    model = make_model(head, pe, classifier_dropout=0.1, dropout_seed=11)
    model.load_state_dict(plain.state_dict())
    ids, labels, am = padded(head, examples(head))
    ref = run(plain, ids, labels, attention_mask=am)
    if head == "qa":
        assert not hasattr(model, "dropout_step")
        same_bits(ref, run(model, ids, labels, attention_mask=am))
        return
    a = run(model, ids, labels, attention_mask=am)
    b = run(model, ids, labels, attention_mask=am)
    assert model.dropout_step.item() == 2
    assert not torch.equal(a[1][0], b[1][0]) and not torch.equal(a[1][0], ref[1][0])
    assert torch.isfinite(a[0]) and all(torch.isfinite(g.float()).all() for g in a[2].values())
    model.eval()
    plain.eval()
    same_bits(run(plain, ids, labels, attention_mask=am), run(model, ids, labels, attention_mask=am))
    assert model.dropout_step.item() == 2   # (eval launches nothing new)
    # the encoder's own sites work as in the seq2seq model
    both = make_model(head, pe, dropout_rate=0.1, classifier_dropout=0.1, dropout_seed=11)
    c = run(both, ids, labels, attention_mask=am)
    assert torch.isfinite(c[0]) and not torch.equal(c[1][0], run(both, ids, labels, attention_mask=am)[1][0])


# ---------------------------------------------------------------- 9: configurations the packed path refuses
@pytest.mark.parametrize("head", HEADS)
def test_dense_bias_refuses_a_real_mask(head):
    model = make_model(head, "t5", attention_type="triton")
    ids, labels, am = padded(head, examples(head))
    with pytest.raises(NotImplementedError):
        model(ids, labels, attention_mask=am)
    assert torch.isfinite(model(ids, labels))
    assert torch.isfinite(model(ids, labels, attention_mask=torch.ones_like(ids)))   # (nothing is padded: the unmasked path)
