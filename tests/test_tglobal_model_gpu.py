"""FAT5Config(encoder_attention_type="transient-global") end to end on a tiny model: d_model 128, 2 heads, 2 encoder layers, vocab 512."""
import math

import pytest
import torch

from test_attention_gpu import gbound
from test_tglobal_attn_gpu import SCALE, _ref

pytestmark = pytest.mark.gpu


def _model(cls_name, seed=5, **flags):
    import flasht5_amd as F
    cfg = F.FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=2, num_decoder_layers=2,
                       encoder_attention_type="transient-global", attention_scale=SCALE, **flags)
    torch.manual_seed(seed)
    return getattr(F, cls_name)(cfg).cuda().bfloat16()


def _ids(B, S, seed=1):
    return torch.randint(2, 512, (B, S), generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("S", [40, 100])
def test_sublayer_matches_fp64(S):
    """Block 0's attention sub-layer against fp64 arithmetic that rounds to bf16 where the model stores a bf16 tensor (the norms,
    the aggregates, the projections, the attention output, the output projection, the residual sum).  What is left is accumulation
    order, the kernels' own bf16 operands and isolated flipped last bits upstream of the last rounding: `gbound`, three half-ulps of
    the largest output."""
    layer = _model("FAT5EncoderModel", local_radius=20).encoder.block[0].self_attention_layer
    sa, B, H = layer.self_attention, 2, 2
    h = torch.randn(B, S, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(S)).bfloat16()
    with torch.no_grad():
        got = layer(h)[0]
    rd = lambda t: t.bfloat16().double()
    norm = lambda t, ln: rd(t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + ln.variance_epsilon) * ln.weight.double())
    lin = lambda t, m: rd(t @ m.weight.double().T)
    heads = lambda t: t.view(B, -1, H, 64).transpose(1, 2)
    x = norm(h.double(), layer.layer_norm)
    blk = (torch.arange(S, device="cuda") // 16).clamp(max=S // 16 - 1)
    agg = torch.zeros(B, S // 16, 128, dtype=torch.float64, device="cuda").index_add_(1, blk, x)
    gx = norm(rd(agg), sa.global_input_layer_norm)
    q, k, v, gk, gv = (heads(lin(t, m)).detach() for t, m in ((x, sa.Wq), (x, sa.Wk), (x, sa.Wv), (gx, sa.Wk), (gx, sa.Wv)))
    (r1, R), (g1, Rg) = sa.pe_encoding.forward_1d(), sa.global_pe_encoding.forward_1d()
    o = _ref(q, k, v, gk, gv, torch.ones_like(q), r1.detach(), g1.detach(), R, Rg, sa.window)[0]
    want = rd(h.double() + lin(rd(o).transpose(1, 2).reshape(B, S, 128), sa.o))
    err = (got.double() - want).abs().max().item()
    print(f"sub-layer S={S}: {err:.3e} / {gbound(want, torch.bfloat16):.3e}")
    assert err <= gbound(want, torch.bfloat16)


def test_a_padded_row_equals_the_row_alone():
    model = _model("FAT5EncoderModel")
    ids, lens = _ids(3, 100), (40, 15, 100)
    am = torch.stack([torch.arange(100) < n for n in lens]).cuda()
    with torch.no_grad():
        padded = model(ids, attention_mask=am)
        for b, n in enumerate(lens):
            assert torch.equal(padded[b, :n], model(ids[b:b + 1, :n])[0]), n
            assert not bool(padded[b, n:].any())


def test_train_step_reaches_the_global_parameters():
    from flasht5_amd import train_step
    model = _model("FAT5ForConditionalGeneration")
    labels = torch.randint(2, 512, (2, 16), generator=torch.Generator().manual_seed(2)).cuda()
    loss = train_step(model, _ids(2, 48), labels, max_grad_norm=None)
    assert math.isfinite(loss.item())
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
    grads = [p.grad for n, p in model.encoder.named_parameters() if "global_input_layer_norm" in n or "global_pe_encoding" in n]
    assert len(grads) == 3 and all(g is not None and bool(g.any()) for g in grads)


def test_generate_runs_with_a_padded_batch():
    model = _model("FAT5ForConditionalGeneration").eval()
    ids = _ids(2, 48)
    am = torch.ones_like(ids)
    am[0, 20:] = 0
    out = model.generate(ids, attention_mask=am, max_length=6)
    assert out.shape[0] == 2 and out.shape[1] >= 1 and bool(((out >= 0) & (out < 512)).all())
