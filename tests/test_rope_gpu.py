"""Rotary position embedding on the GPU: the fat5_rope_apply kernel against an eager restatement of flash_attn's rotation
(the reference's RoPE path, src/utils/positional_encoding.py:297-338) over dtype x head_dim x rotated fraction x interleaving x
xPos x in place x strided views x packed batches; its autograd backward; the FlashT5Attention module with
position_encoding_type="RoPE" against an eager fp32 restatement of the reference module; and a captured RoPE training step."""
import math
from types import SimpleNamespace

import pytest
import torch

import oracle
from attn_helpers import maxdiff

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def rope_ref(x, cos, sin, pos, interleaved=False, conjugate=False):
    """flash_attn's rotation restated in eager fp32 on the CPU (every product rounded to fp32, one rounding to x's dtype).
    x (..., S, H, D) with the position of row s in pos[s]; columns >= rd copied."""
    x = x.detach().cpu()
    rd, h = 2 * cos.shape[-1], cos.shape[-1]
    c = cos.detach().cpu().float()[pos.cpu()][:, None, :]
    s = sin.detach().cpu().float()[pos.cpu()][:, None, :]
    if conjugate:
        s = -s
    xf = x.float()
    x0, x1 = (xf[..., 0:rd:2], xf[..., 1:rd:2]) if interleaved else (xf[..., :h], xf[..., h:rd])
    y0, y1 = x0 * c - x1 * s, x0 * s + x1 * c
    out = x.clone()
    if interleaved:
        out[..., 0:rd:2], out[..., 1:rd:2] = y0.to(x.dtype), y1.to(x.dtype)
    else:
        out[..., :h], out[..., h:rd] = y0.to(x.dtype), y1.to(x.dtype)
    return out


def _ordered(t):
    t = t.detach().cpu().contiguous()
    if t.element_size() == 2:
        b, m = t.view(torch.int16).to(torch.int64), 1 << 15
    else:
        b, m = t.view(torch.int32).to(torch.int64), 1 << 31
    return torch.where(b < 0, -(b + m), b)


def assert_ulp(y, ref, rd):
    """<= 1 ulp of the output dtype in the rotated columns, bit-identical beyond them"""
    y, ref = y.detach().cpu(), ref.detach().cpu()
    assert y.shape == ref.shape and y.dtype == ref.dtype
    d = (_ordered(y[..., :rd]) - _ordered(ref[..., :rd])).abs()
    assert int(d.max()) <= 1, int(d.max())
    if rd < y.shape[-1]:
        assert torch.equal(_ordered(y[..., rd:]), _ordered(ref[..., rd:]))


def tables(rd, rows, dtype, xpos, device="cuda"):
    from flasht5_amd.rotary import rotary_tables
    return rotary_tables(rd, rows, 10000.0, 64 if xpos else None, dtype, device)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("frac", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_rope_kernel_matches_oracle(dt, D, frac, interleaved):
    """q with (cos, sin), k and v with the xPos k tables (or the same tables) in one launch; out of place on the permuted views
    of three projections, then in place on the slices of one packed q | k | v buffer; positions past 256 (bf16-quantised)"""
    from flasht5_amd import apply_rotary_emb_qkv
    from flasht5_amd.rotary import rotary_, _packed_views
    dtype = DT[dt]
    rd = int(D * frac)
    B, S, H = 2, 300, 3
    g = torch.Generator(device="cuda").manual_seed(D + int(frac * 8) + interleaved)
    pos = torch.arange(S)
    for xpos in (False, True):
        cos, sin, cos_k, sin_k = tables(rd, 320, dtype, xpos)
        ck, sk = (cos, sin) if cos_k is None else (cos_k, sin_k)
        # (B, H, S, D) storage seen as (B, S, H, D): strided views, as the module's projections are
        q, k, v = (torch.randn(B, H, S, D, device="cuda", generator=g).to(dtype).transpose(1, 2) for _ in range(3))
        yq, yk, yv = apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k, sin_k, interleaved)
        assert_ulp(yq, rope_ref(q, cos, sin, pos, interleaved), rd)
        assert_ulp(yk, rope_ref(k, ck, sk, pos, interleaved), rd)
        assert_ulp(yv, rope_ref(v, ck, sk, pos, interleaved), rd)
        # in place on packed (B, S, 3 * H * D) slices
        buf = torch.randn(B, S, 3 * H * D, device="cuda", generator=g).to(dtype)
        ref = buf.clone()
        views = _packed_views(buf, 3, H, D)
        rotary_(views, cos, sin, cos_k, sin_k, 1, interleaved, False, None, 0)
        rv = _packed_views(ref, 3, H, D)
        assert_ulp(views[0], rope_ref(rv[0], cos, sin, pos, interleaved), rd)
        assert_ulp(views[1], rope_ref(rv[1], ck, sk, pos, interleaved), rd)
        assert_ulp(views[2], rope_ref(rv[2], ck, sk, pos, interleaved), rd)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("dt,D,frac", [("bf16", 64, 1.0), ("fp16", 128, 0.5), ("fp32", 32, 0.25), ("bf16", 16, 0.25)])
def test_rope_varlen(dt, D, frac, interleaved, inplace):
    """packed (total, H, D) batches: positions restart at every sequence; empty and one-token sequences included"""
    from flasht5_amd import apply_rotary_emb
    dtype, rd, H = DT[dt], int(D * frac), 4
    lens = [5, 0, 1, 300, 17, 0, 64, 1]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
    total = int(cu[-1])
    pos = torch.cat([torch.arange(n) for n in lens])
    cos, sin, _, _ = tables(rd, 300, dtype, False)
    x = torch.randn(total, H, D, device="cuda").to(dtype)
    x0 = x.clone()
    y = apply_rotary_emb(x, cos, sin, interleaved, inplace, cu_seqlens=cu, max_seqlen=max(lens))
    assert (y.data_ptr() == x.data_ptr()) == inplace
    ref = rope_ref(x0[None], cos, sin, pos, interleaved)[0]
    assert_ulp(y, ref, rd)


@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_backward_is_the_conjugate_rotation(interleaved):
    from flasht5_amd import apply_rotary_emb, apply_rotary_emb_qkv
    dtype, D, rd = torch.bfloat16, 64, 32
    cos, sin, cos_k, sin_k = tables(rd, 512, dtype, True)
    pos = torch.arange(384)
    q, k, v = (torch.randn(2, 384, 4, D, device="cuda").to(dtype).requires_grad_() for _ in range(3))
    gq, gk, gv = (torch.randn(2, 384, 4, D, device="cuda").to(dtype) for _ in range(3))
    out = apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k, sin_k, interleaved)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), (gq, gk, gv))
    assert_ulp(dq, rope_ref(gq, cos, sin, pos, interleaved, conjugate=True), rd)
    assert_ulp(dk, rope_ref(gk, cos_k, sin_k, pos, interleaved, conjugate=True), rd)
    assert_ulp(dv, rope_ref(gv, cos_k, sin_k, pos, interleaved, conjugate=True), rd)
    # single tensor, in place on a non-leaf
    x = torch.randn(2, 384, 4, D, device="cuda").to(dtype).requires_grad_()
    y = apply_rotary_emb(x * 1, cos, sin, interleaved, inplace=True)
    (dx,) = torch.autograd.grad(y, x, gq)
    assert_ulp(dx, rope_ref(gq, cos, sin, pos, interleaved, conjugate=True), rd)
    # the conjugate rotation undoes the forward one: fp32 tensors and tables, so cos^2 + sin^2 = 1 to fp32 rounding
    from flasht5_amd.rotary import rotary
    c32, s32, _, _ = tables(rd, 512, torch.float32, False)
    x32 = torch.randn(2, 384, 4, D, device="cuda")
    (y32,) = rotary([x32], c32, s32, None, None, 1, interleaved, False, None, 0)
    (z32,) = rotary([y32], c32, s32, None, None, 1, interleaved, True, None, 0)
    assert maxdiff(y32[..., :rd], x32[..., :rd]) > 1e-2  # (it did rotate)
    assert maxdiff(z32, x32) <= 1e-5 * x32.abs().max().item(), maxdiff(z32, x32)


def test_rope_positions_beyond_table_raise():
    from flasht5_amd import apply_rotary_emb, apply_rotary_emb_qkv
    cos, sin, _, _ = tables(64, 128, torch.bfloat16, False)
    with pytest.raises(ValueError, match="beyond the table"):
        apply_rotary_emb(torch.randn(1, 129, 2, 64, device="cuda").bfloat16(), cos, sin)
    q = torch.randn(1, 16, 2, 64, device="cuda").bfloat16()
    kv = torch.randn(1, 200, 2, 64, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="beyond the table"):
        apply_rotary_emb_qkv(q, kv, kv, cos, sin)
    cu = torch.tensor([0, 100, 300], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="beyond the table"):
        apply_rotary_emb(torch.randn(300, 2, 64, device="cuda").bfloat16(), cos, sin, cu_seqlens=cu, max_seqlen=200)
    # the C ABI rejects it too (the custom op called directly, past the Python check)
    from flasht5_amd.rotary import rotary
    with pytest.raises(RuntimeError, match="beyond the table"):
        rotary([torch.randn(1, 129, 2, 64, device="cuda").bfloat16()], cos, sin, None, None, 1, False, False, None, 0)


# ---- the module -----------------------------------------------------------------------------------------------------------

def _cfg(attention_type, decoder, frac=1.0, scale_base=None, interleaved=False):
    return SimpleNamespace(d_model=128, d_kv=64, num_heads=2, relative_attention_num_buckets=32, relative_attention_max_distance=64,
                           is_decoder=decoder, attention_type=attention_type, position_encoding_type="RoPE", attention_scale=None,
                           rotary_emb_fraction=frac, rotary_base=10000, rotary_interleaved=interleaved, rotary_scale_base=scale_base,
                           max_sequence_length=512)


def _eager_layer(w, h, kv, cfg, causal, interleaved):
    """eager fp32 restatement of the reference module with RoPE (modeling_flash_t5.py:214-220, :245-287): bf16 tables, q rotated with
    (cos, sin), k AND v with (cos_k, sin_k), no bias"""
    from flasht5_amd.rotary import rotary_tables
    H, Dh = cfg.num_heads, cfg.d_kv
    B, M, N = h.shape[0], h.shape[1], kv.shape[1]
    cos, sin, cos_k, sin_k = rotary_tables(int(Dh * cfg.rotary_emb_fraction), cfg.max_sequence_length, cfg.rotary_base,
                                           cfg.rotary_scale_base, torch.bfloat16, h.device)
    ck, sk = (cos, sin) if cos_k is None else (cos_k, sin_k)

    def rot(x, c, s):  # differentiable fp32 rotation
        S, hh = x.shape[1], c.shape[-1]
        c, s = c[:S].float()[:, None, :], s[:S].float()[:, None, :]
        rd = 2 * hh
        x0, x1 = (x[..., 0:rd:2], x[..., 1:rd:2]) if interleaved else (x[..., :hh], x[..., hh:rd])
        y0, y1 = x0 * c - x1 * s, x0 * s + x1 * c
        y = torch.stack((y0, y1), -1).flatten(-2) if interleaved else torch.cat((y0, y1), -1)
        return torch.cat((y, x[..., rd:]), -1)
    q = rot((h @ w["Wq"].t()).view(B, M, H, Dh), cos, sin).permute(0, 2, 1, 3)
    k = rot((kv @ w["Wk"].t()).view(B, N, H, Dh), ck, sk).permute(0, 2, 1, 3)
    v = rot((kv @ w["Wv"].t()).view(B, N, H, Dh), ck, sk).permute(0, 2, 1, 3)
    o = oracle.attn_ref(q, k, v, None, 1.0 / math.sqrt(H), causal=causal, upcast=True)
    return o.permute(0, 2, 1, 3).reshape(B, M, H * Dh) @ w["o"].t()


@pytest.mark.parametrize("variant", ["plain", "half_xpos_interleaved"])
@pytest.mark.parametrize("attention_type", ["triton", "fat5_rpe"])
@pytest.mark.parametrize("decoder", [False, True])
def test_flasht5_attention_rope_two_blocks_and_cross(attention_type, decoder, variant):
    """two self-attention blocks (RoPE built in both: the reference has no has_positional_encoding condition) and, for the decoder,
    a cross-attention layer with M != N that rotates too; outputs and every parameter gradient against the eager fp32 restatement;
    forward_fused (packed q | k | v, rotated in one launch) agrees with forward"""
    from flasht5_amd import FlashT5Attention, fast_rms_layernorm
    frac, sb, il = (1.0, None, False) if variant == "plain" else (0.5, 256, True)
    cfg = _cfg(attention_type, decoder, frac, sb, il)
    torch.manual_seed(41)
    blk0 = FlashT5Attention(cfg, has_positional_encoding=True, is_causal=decoder).cuda().bfloat16()
    blk1 = FlashT5Attention(cfg, has_positional_encoding=False, is_causal=decoder).cuda().bfloat16()
    cross = FlashT5Attention(cfg, has_positional_encoding=False).cuda().bfloat16()
    assert all(m.pe_encoding is not None for m in (blk0, blk1, cross))
    assert [n for n, _ in blk1.named_parameters()] == ["Wq.weight", "Wk.weight", "Wv.weight", "o.weight"]
    B, S, N = 2, 300, 136
    x = torch.randn(B, S, cfg.d_model, device="cuda").bfloat16()
    enc = torch.randn(B, N, cfg.d_model, device="cuda").bfloat16()
    gy = torch.randn(B, S, cfg.d_model, device="cuda").bfloat16()
    y0, pb = blk0(x)
    assert pb is None
    y1, pb1 = blk1(y0, position_bias=pb)
    assert pb1 is None
    y2, _ = cross(y1, key_value_states=enc)
    mods = (blk0, blk1, cross)
    params = [p for m in mods for p in m.parameters()]
    grads = torch.autograd.grad(y2, params, gy)

    leaves = [{n.split(".")[0]: p.detach().float().clone().requires_grad_() for n, p in m.named_parameters()} for m in mods]
    r0 = _eager_layer(leaves[0], x.float(), x.float(), cfg, decoder, il)
    r1 = _eager_layer(leaves[1], r0, r0, cfg, decoder, il)
    r2 = _eager_layer(leaves[2], r1, enc.float(), cfg, False, il)
    ref_params = [w[n.split(".")[0]] for m, w in zip(mods, leaves) for n, _ in m.named_parameters()]
    ref_grads = torch.autograd.grad(r2, ref_params, gy.float())
    assert maxdiff(y2, r2) <= 3e-2 * max(1.0, r2.abs().max().item()), maxdiff(y2, r2)
    names = [f"{i}.{n}" for i, m in enumerate(mods) for n, _ in m.named_parameters()]
    for n, g, rg in zip(names, grads, ref_grads):
        assert torch.isfinite(g.float()).all(), n
        assert maxdiff(g, rg) <= 4e-2 * max(1.0, rg.abs().max().item()), (n, maxdiff(g, rg), rg.abs().max().item())

    # forward_fused (norm in the projection GEMM, packed q | k | v rotated in one launch, residual in the output GEMM) == forward
    w = torch.ones(cfg.d_model, device="cuda").bfloat16() + 0.1 * torch.randn(cfg.d_model, device="cuda").bfloat16()
    for m, kvs in ((blk0, None), (cross, enc)):
        a = x.clone().requires_grad_()
        yf, _ = m.forward_fused(a, w, 1e-6, key_value_states=kvs)
        gf = torch.autograd.grad(yf, [a] + list(m.parameters()), gy)
        b = x.clone().requires_grad_()
        ye = b + m(fast_rms_layernorm(b, w, 1e-6), key_value_states=kvs)[0]
        ge = torch.autograd.grad(ye, [b] + list(m.parameters()), gy)
        assert maxdiff(yf, ye) <= 2e-2 * max(1.0, ye.abs().max().item()), maxdiff(yf, ye)
        for g1, g2 in zip(gf, ge):
            assert maxdiff(g1, g2) <= 3e-2 * max(1.0, g2.abs().max().item()), (maxdiff(g1, g2), g2.abs().max().item())


def test_rope_module_does_not_touch_saved_tensors():
    """the rotation of the module's projections leaves every tensor autograd saved as it was (a version-counter bump would raise in
    backward)"""
    from flasht5_amd import FlashT5Attention
    cfg = _cfg("triton", False)
    m = FlashT5Attention(cfg, has_positional_encoding=True).cuda().bfloat16()
    x = torch.randn(2, 64, cfg.d_model, device="cuda").bfloat16().requires_grad_()
    y, _ = m(x)
    y.float().sum().backward()
    yf, _ = m.forward_fused(x, torch.ones(cfg.d_model, device="cuda").bfloat16(), 1e-6)
    yf.float().sum().backward()
    assert torch.isfinite(x.grad.float()).all()


@pytest.mark.parametrize("attention_type", ["triton", "fat5_rpe"])
def test_rope_layer_handed_a_bias_uses_it_and_does_not_rotate(attention_type):
    """the reference rotates only when no position_bias is handed in (modeling_flash_t5.py:259): a RoPE layer given one computes
    exactly what the same layer without a position encoding computes with that bias"""
    from flasht5_amd import FlashT5Attention
    from flasht5_amd.positional_encoding import RelativePositionalEncoding
    cfg = _cfg(attention_type, False)
    rope = FlashT5Attention(cfg, has_positional_encoding=False).cuda().bfloat16()
    plain = FlashT5Attention(SimpleNamespace(**{**vars(cfg), "position_encoding_type": "t5"}), has_positional_encoding=False).cuda().bfloat16()
    plain.load_state_dict(rope.state_dict())
    x = torch.randn(2, 96, cfg.d_model, device="cuda").bfloat16()
    pe = RelativePositionalEncoding(32, 64, cfg.num_heads, 512).cuda()
    pb = pe.forward_1d() if attention_type == "fat5_rpe" else pe.compute_bias(96, 96, device="cuda").contiguous().bfloat16()
    y1, pb1 = rope(x, position_bias=pb)
    y2, pb2 = plain(x, position_bias=pb)
    assert torch.equal(y1, y2) and pb1 is pb and pb2 is pb
    w = torch.ones(cfg.d_model, device="cuda").bfloat16()
    assert torch.equal(rope.forward_fused(x, w, 1e-6, position_bias=pb)[0], plain.forward_fused(x, w, 1e-6, position_bias=pb)[0])


@pytest.mark.parametrize("fuse", [False, True])
def test_graphed_train_step_rope(fuse):
    """a 2-layer RoPE FAT5 model: the captured step (tables built in the eager warm-up, rotary launches inside the graph) follows
    the eager train_step"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, AdamWScale, train_step, GraphedTrainStep
    cfg = FAT5Config(num_layers=2, num_decoder_layers=2, vocab_size=4096, position_encoding_type="RoPE", attention_type="triton")
    cfg.fuse_norm_linear = fuse
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randint(0, cfg.vocab_size, (2, 512), generator=g).cuda(), torch.randint(0, cfg.vocab_size, (2, 128), generator=g).cuda())
               for _ in range(5)]
    lrs = [1e-3, 2e-3, 3e-3, 2e-3, 1e-3]
    runs = []
    for graphed in (False, True):
        torch.manual_seed(7)
        model = FAT5ForConditionalGeneration(cfg).cuda().bfloat16()
        assert model.rpe_tables() == []
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
    assert all(math.isfinite(a) for a in l0)
    assert l0[0] == l1[0]
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for a, b in zip(p0, p1):
        assert float((a - b).abs().max()) <= 2.0 ** -6 * max(float(a.abs().max()), 1e-3)
