"""FAT5Config(encoder_attention_type="local") end to end on a tiny model: d_model 128, 2 heads, 2 encoder layers, vocab 512,
local_radius 4, S = 48."""
import math

import pytest
import torch

from test_attention_gpu import bound

pytestmark = pytest.mark.gpu

S, LAYERS, RADIUS = 48, 2, 4


def _model(cls_name, seed=5, **flags):
    import flasht5_amd as F
    cfg = F.FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=LAYERS, num_decoder_layers=LAYERS, **flags)
    torch.manual_seed(seed)
    return getattr(F, cls_name)(cfg).cuda().bfloat16()


def _ids(B=2, seed=1):
    return torch.randint(2, 512, (B, S), generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("pe", ["t5", "RoPE"])
def test_a_token_reaches_layers_times_radius(pe):
    model = _model("FAT5EncoderModel", encoder_attention_type="local", local_radius=RADIUS, position_encoding_type=pe)
    ids, j = _ids(), 24
    other = ids.clone()
    other[:, j] = (ids[:, j] + 7) % 510 + 2
    with torch.no_grad():
        a, b = model(ids), model(other)
    far = (torch.arange(S, device="cuda") - j).abs() > LAYERS * RADIUS
    assert torch.equal(a[:, far], b[:, far])
    assert not torch.equal(a[:, ~far], b[:, ~far])
    assert not torch.equal(a[:, j + RADIUS + 1], b[:, j + RADIUS + 1])  # ... through the second layer, beyond one window


def test_a_window_over_the_whole_row_is_full_attention():
    """In fp16.  Both sides are low-precision models: they differ by the two attention kernels' output roundings, carried through
    the second layer's softmax and rounded again at the end.  `bound` allows half an ulp of the output dtype: between two fp16
    results that covers a flipped last bit of the largest element; between two bf16 results it cannot (one flipped bit there is
    2^-7 of it, the bound 2^-8 + 1e-3 of it) -- measured in bf16 on this model: 3.9e-2 against a bound of 2.0e-2."""
    local = _model("FAT5EncoderModel", encoder_attention_type="local", local_radius=S - 1).half()
    full = _model("FAT5EncoderModel").half()
    with torch.no_grad():
        a, b = local(_ids()), full(_ids())
    err = (a.float() - b.float()).abs().max().item()
    print(f"local vs full: {err:.3e} / {bound(b, torch.float16):.3e}")
    assert err <= bound(b, torch.float16)


def test_a_padded_row_equals_the_row_alone():
    model = _model("FAT5EncoderModel", encoder_attention_type="local", local_radius=RADIUS)
    ids, n = _ids(), 30
    am = torch.ones_like(ids)
    am[0, n:] = 0
    with torch.no_grad():
        padded, alone = model(ids, attention_mask=am), model(ids[:1, :n])
    assert torch.equal(padded[0, :n], alone[0])
    assert not bool(padded[0, n:].any())


def test_train_step_reaches_the_bias_table():
    from flasht5_amd import train_step
    model = _model("FAT5ForConditionalGeneration", encoder_attention_type="local", local_radius=RADIUS)
    labels = torch.randint(2, 512, (2, 16), generator=torch.Generator().manual_seed(2)).cuda()
    loss = train_step(model, _ids(), labels, max_grad_norm=None)
    assert math.isfinite(loss.item())
    grads = [p.grad for n, p in model.encoder.named_parameters() if "relative_attention_bias" in n]
    assert len(grads) == 1 and torch.isfinite(grads[0]).all() and bool(grads[0].any())
