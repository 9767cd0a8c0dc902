"""GPU tests of training on padded and packed batches (FAT5ForConditionalGeneration.forward with attention_mask /
decoder_attention_mask / segment_ids / decoder_segment_ids).

Model: 2 + 2 layers, d_model 128, d_kv 64, 2 heads, d_ff 256, vocabulary 512, bf16; T5 bias (fat5_rpe) and RoPE.
Batch: B = 3, L_enc = 80, L_dec = 40, encoder lengths (80, 33, 1), decoder lengths (40, 17, 2): the lengths cross the 32- and
64-row tile edges of the attention kernels and include one-token sequences."""
import pytest
import torch

pytestmark = pytest.mark.gpu

L_ENC, L_DEC = 80, 40
ENC_LENS, DEC_LENS = (80, 33, 1), (40, 17, 2)
PES = ["t5", "RoPE"]


@pytest.fixture
def torch_deterministic():
    """The exact tests compare two runs bit for bit.  Everything this project launches is reproducible; one torch operator on the
    way is not by default -- the backward of the table lookup that builds the T5 generator (index_select's index_add_, float
    atomics), on the unmasked path as on the packed one -- so torch's own deterministic mode is on while such a test runs."""
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


def make_model(pe, seed=5, **flags):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    cfg = FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=2, num_decoder_layers=2,
                     position_encoding_type=pe, **flags)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(cfg).cuda().bfloat16()


def examples(enc_lens=ENC_LENS, dec_lens=DEC_LENS, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(1, 512, (e,), generator=g), torch.randint(1, 512, (d,), generator=g)) for e, d in zip(enc_lens, dec_lens)]


def padded(exs, l_enc=L_ENC, l_dec=L_DEC, garbage=None):
    """rows of one example each, right-padded: (ids, labels, attention_mask, decoder_attention_mask) on the device; `garbage`: a
    seed for what the padded positions hold instead of 0 / -100"""
    B = len(exs)
    ids = torch.zeros(B, l_enc, dtype=torch.long)
    labels = torch.full((B, l_dec), -100, dtype=torch.long)
    if garbage is not None:
        g = torch.Generator().manual_seed(garbage)
        ids = torch.randint(0, 512, (B, l_enc), generator=g)
        labels = torch.randint(0, 512, (B, l_dec), generator=g)
        labels[torch.rand(B, l_dec, generator=g) < 0.3] = -100
    am = torch.zeros(B, l_enc, dtype=torch.bool)
    dm = torch.zeros(B, l_dec, dtype=torch.bool)
    for b, (x, y) in enumerate(exs):
        ids[b, :len(x)], labels[b, :len(y)] = x, y
        am[b, :len(x)], dm[b, :len(y)] = True, True
    return ids.cuda(), labels.cuda(), am.cuda(), dm.cuda()


def run(model, ids, labels, **kw):
    model.zero_grad(set_to_none=True)
    loss = model(ids, labels, **kw)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def same_bits(a, b):
    assert torch.equal(a[0], b[0]), (a[0].item(), b[0].item())
    assert a[1].keys() == b[1].keys()
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), n


def rel_err(got, ref):
    """max-abs error of every gradient relative to the tensor's max-abs, and the loss likewise: {name: float}"""
    out = {"loss": abs(got[0].item() - ref[0].item()) / abs(ref[0].item())}
    for n, r in ref[1].items():
        out[n] = (got[1][n].float() - r.float()).abs().max().item() / max(r.float().abs().max().item(), 1e-30)
    return out


def alone_combined(model, exs):
    """every example through the existing forward on its own, unpadded, B = 1; combined with the examples' label counts (the loss
    is a mean over the rows it is given, and no label of these examples is ignored: the count is the length)"""
    assert all(bool((y != -100).all()) for _, y in exs)
    parts = [(run(model, x[None].cuda(), y[None].cuda()), len(y)) for x, y in exs]
    n = sum(c for _, c in parts)
    loss = sum(r[0].float() * c for r, c in parts) / n
    grads = {k: sum(r[1][k].float() * c for r, c in parts) / n for k in parts[0][0][1]}
    return loss, grads


# ---------------------------------------------------------------- (a) exact
@pytest.mark.parametrize("pe", PES)
def test_padding_garbage_changes_no_bit(pe, torch_deterministic):
    """what the padded positions hold -- other ids, other labels, ignored or not -- reaches neither the loss nor a gradient"""
    model = make_model(pe)
    exs = examples()
    ids0, lab0, am, dm = padded(exs)
    ids1, lab1, _, _ = padded(exs, garbage=9)
    assert not torch.equal(ids0, ids1) and not torch.equal(lab0, lab1)
    a = run(model, ids0, lab0, attention_mask=am, decoder_attention_mask=dm)
    b = run(model, ids1, lab1, attention_mask=am, decoder_attention_mask=dm)
    same_bits(a, b)
    assert torch.isfinite(a[0]) and all(torch.isfinite(g.float()).all() for g in a[1].values())


@pytest.mark.parametrize("pe", PES)
def test_all_ones_masks_are_the_unmasked_path(pe, torch_deterministic):
    model = make_model(pe)
    ids, labels, _, _ = padded(examples((L_ENC,) * 3, (L_DEC,) * 3))
    ref = run(model, ids, labels)
    ones = run(model, ids, labels, attention_mask=torch.ones_like(ids), decoder_attention_mask=torch.ones_like(labels, dtype=torch.bool))
    same_bits(ref, ones)
    segs = run(model, ids, labels, segment_ids=torch.ones_like(ids, dtype=torch.int32), decoder_segment_ids=torch.ones_like(labels))
    same_bits(ref, segs)


@pytest.mark.parametrize("pe", PES)
def test_packed_rows_equal_padded_rows(pe, torch_deterministic):
    """rows [a, b] and [c] told apart by segment ids against rows [a], [b], [c] under masks: the same packed token stream and the
    same cu_seqlens (asserted first), so the same bits"""
    from flasht5_amd import pack_plan
    model = make_model(pe)
    a, b, c = examples((33, 1, 80), (17, 2, 40))
    ids3, lab3, am3, dm3 = padded([a, b, c])
    ids2 = torch.zeros(2, L_ENC, dtype=torch.long)
    lab2 = torch.full((2, L_DEC), -100, dtype=torch.long)
    seg2 = torch.zeros(2, L_ENC, dtype=torch.int32)
    dseg2 = torch.zeros(2, L_DEC, dtype=torch.int32)
    ids2[0, :33], ids2[0, 33:34], ids2[1, :80] = a[0], b[0], c[0]
    seg2[0, :33], seg2[0, 33:34], seg2[1, :80] = 1, 2, 1
    lab2[0, :17], lab2[0, 17:19], lab2[1, :40] = a[1], b[1], c[1]
    dseg2[0, :17], dseg2[0, 17:19], dseg2[1, :40] = 1, 2, 1
    ids2, lab2, seg2, dseg2 = ids2.cuda(), lab2.cuda(), seg2.cuda(), dseg2.cuda()
    for x3, m3, x2, s2 in ((ids3, am3, ids2, seg2), (lab3, dm3, lab2, dseg2)):
        p3, p2 = pack_plan(m3), pack_plan(s2)
        assert torch.equal(p3.cu_seqlens, p2.cu_seqlens) and (p3.max_seqlen, p3.total, p3.nseq) == (p2.max_seqlen, p2.total, p2.nseq)
        assert torch.equal(x3.reshape(-1)[p3.index], x2.reshape(-1)[p2.index])
    same_bits(run(model, ids3, lab3, attention_mask=am3, decoder_attention_mask=dm3),
              run(model, ids2, lab2, segment_ids=seg2, decoder_segment_ids=dseg2))


# ---------------------------------------------------------------- (b) a row trains as it trains alone
@pytest.mark.parametrize("pe", PES)
def test_a_row_trains_as_it_trains_alone(pe):
    """The packed loss and every parameter gradient against the existing forward run on each example alone (unpadded, B = 1),
    combined with the examples' label counts: sum n_i loss_i / sum n_i, the gradients likewise.

    The bound is 4 x the batch-composition floor, per tensor, as max-abs relative to the tensor's max-abs.  The floor is measured
    here, on the unmasked paths only: a batch of three equal-length examples (80 / 40 tokens) against the same three run alone and
    combined -- other GEMM shapes and another attention body for the same arithmetic.  The factor 4: the packed path changes the
    GEMM shapes and the attention body at once, on two sides.  Without the masks the same comparison must exceed the bound (the
    padded keys are attended), or the test would pass vacuously.

    Measured (MI355X, this file's seeds; the test prints every figure): floor 3.4e-3 .. 1.5e-2 over the gradients (RoPE 4.4e-3 ..
    1.4e-2) and 0 (RoPE 1.4e-7) on the loss; packed up to 1.8e-2 (RoPE 1.5e-2), the worst tensor at 1.74 x its floor
    (encoder.block.1.ff_layer.act.wi_0.weight; RoPE 1.82 x, encoder.block.0.ff_layer.layer_norm.weight), the packed loss equal to
    the combined one; without the masks 0.51 on the loss and 0.5 .. 1.7 on the gradients."""
    model = make_model(pe)
    full = examples((L_ENC,) * 3, (L_DEC,) * 3, seed=2)
    ids, labels, _, _ = padded(full)
    floor = rel_err(run(model, ids, labels), alone_combined(model, full))

    exs = examples()
    ids, labels, am, dm = padded(exs)
    ref = alone_combined(model, exs)
    err = rel_err(run(model, ids, labels, attention_mask=am, decoder_attention_mask=dm), ref)
    nomask = rel_err(run(model, ids, labels), ref)
    worst = max(err, key=lambda n: err[n] / max(floor[n], 1e-30))
    print(f"[packed-vs-alone {pe}] floor: loss {floor['loss']:.3e}, gradients {min(v for k, v in floor.items() if k != 'loss'):.3e} .. "
          f"{max(v for k, v in floor.items() if k != 'loss'):.3e}; packed: loss {err['loss']:.3e}, gradients up to "
          f"{max(v for k, v in err.items() if k != 'loss'):.3e}; worst ratio {err[worst] / max(floor[worst], 1e-30):.2f} ({worst}); "
          f"no mask: loss {nomask['loss']:.3e}, gradients up to {max(v for k, v in nomask.items() if k != 'loss'):.3e}")
    for n in sorted(err):
        print(f"[packed-vs-alone {pe}]   {n}: floor {floor[n]:.3e} packed {err[n]:.3e} nomask {nomask[n]:.3e}")
    # (the loss: the same per-row fp32 values summed in another order -- the floor can be 0 by luck, so 64 ulp of fp32, the worst
    #  case of a 59-term sum, are allowed on top of it; every gradient: 4 x its floor, nothing added)
    floor["loss"] += 16 * 2.0 ** -24
    bad = {n: (err[n], floor[n]) for n in err if err[n] > 4 * floor[n]}
    assert not bad, bad
    assert any(nomask[n] > 4 * floor[n] for n in nomask), "dropping the masks must break the bound"


# ---------------------------------------------------------------- (c) fusion flags
# (relative loss bound, relative gradient bound, the same for the relative-position tables): what each flag's existing unpadded
#  comparison allows -- tests/test_cfg5_gpu.py (fuse_add_norm, fuse_lm_head_ce), tests/test_fused_linear_gpu.py (fuse_norm_linear).
#  fuse_gated_act has a layer-level comparison only (tests/test_gated_act_gpu.py); switching it off rounds act(wi_0 x) to bf16
#  before the product, so every later activation differs in its last bf16 bit -- the situation fuse_norm_linear's bounds are for.
FLAG_BOUNDS = {
    "fuse_add_norm": (dict(fuse_add_norm=True), 2e-6, 2.0 ** -7, 2.0 ** -4),
    "fuse_norm_linear": (dict(fuse_norm_linear=True), 2e-3, 2.0 ** -4, 2.0 ** -3),
    "fuse_lm_head_ce": (dict(fuse_lm_head_ce=True), 2e-6, 2.0 ** -6, 2.0 ** -4),
    "fuse_gated_act_off": (dict(fuse_gated_act=False), 2e-3, 2.0 ** -4, 2.0 ** -3),
}


@pytest.mark.parametrize("pe", PES)
@pytest.mark.parametrize("flag", sorted(FLAG_BOUNDS))
def test_fusion_flags_on_packed_rows(flag, pe):
    kw, loss_tol, grad_tol, table_tol = FLAG_BOUNDS[flag]
    m0 = make_model(pe)
    m1 = make_model(pe, **kw)
    m1.load_state_dict(m0.state_dict())
    ids, labels, am, dm = padded(examples())
    l0, g0 = run(m0, ids, labels, attention_mask=am, decoder_attention_mask=dm)
    l1, g1 = run(m1, ids, labels, attention_mask=am, decoder_attention_mask=dm)
    assert abs(l0.item() - l1.item()) <= loss_tol * abs(l0.item()), (l0.item(), l1.item())
    for n in g0:
        assert torch.isfinite(g1[n].float()).all(), n
        rel = table_tol if "relative_attention_bias" in n else grad_tol
        d = (g1[n].float() - g0[n].float()).abs().max().item()
        assert d <= rel * max(g0[n].float().abs().max().item(), 1e-6), (n, d)


# ---------------------------------------------------------------- (d) the optimizer step
@pytest.mark.parametrize("pe", PES)
def test_train_step_with_masks_updates_every_parameter(pe):
    from flasht5_amd import AdamWScale, train_step
    model = make_model(pe)
    opt = AdamWScale(model.parameters(), lr=1e-2, max_grad_norm=1.0)
    before = [p.detach().clone() for p in model.parameters()]
    ids, labels, am, dm = padded(examples())
    losses = [train_step(model, ids, labels, opt, max_grad_norm=None, attention_mask=am, decoder_attention_mask=dm).item() for _ in range(2)]
    assert all(l == l and abs(l) != float("inf") for l in losses)
    for (n, p), b in zip(model.named_parameters(), before):
        assert not torch.equal(p.detach(), b), n


@pytest.mark.parametrize("pe", PES)
def test_decoder_lengths_from_labels_equal_an_explicit_mask(pe, torch_deterministic):
    """without a decoder-side argument, row b ends behind its last label that is not -100"""
    model = make_model(pe)
    ids, labels, am, dm = padded(examples())
    same_bits(run(model, ids, labels, attention_mask=am, decoder_attention_mask=dm), run(model, ids, labels, attention_mask=am))
    labels = labels.clone()
    labels[0, 3] = -100   # (an ignored label inside a row does not end it)
    same_bits(run(model, ids, labels, attention_mask=am, decoder_attention_mask=dm), run(model, ids, labels, attention_mask=am))
