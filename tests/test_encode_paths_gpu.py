"""generation.encode on padded batches, bit for bit: `_padded_encoder` runs the blocks' own packed attention
(`FAT5Block.forward(h, bias, None, packing)`) or hands them the masked dense bias, and must give exactly what the explicit
restatements below give -- the two padded encoders generation.py used to spell out by hand, moved here as the reference.  The MXFP4
runner goes through the same helper, and the encoder-only models reach the same stack through their own plan.  Two encoder layers:
the smallest stack in which block 0's bias or generator is handed to a block that does not own it."""
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [12, 7, 1]   # a full row, a ragged row and a one-token row
B_, L_ = 3, 12
KINDS = {
    "rpe_t5": dict(attention_type="fat5_rpe", position_encoding_type="t5"),
    "rpe_rope": dict(attention_type="fat5_rpe", position_encoding_type="RoPE"),
    "dense_t5": dict(attention_type="triton", position_encoding_type="t5"),
    "local_t5": dict(attention_type="fat5_rpe", position_encoding_type="t5", encoder_attention_type="local", local_radius=3),
}


def _config(**kw):
    from flasht5_amd import FAT5Config
    return FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=2, num_decoder_layers=1, **kw)


@lru_cache(maxsize=None)
def _model(kind, fuse_norm_linear=False):
    from flasht5_amd import FAT5ForConditionalGeneration
    torch.manual_seed(21)
    return FAT5ForConditionalGeneration(_config(fuse_norm_linear=fuse_norm_linear, **KINDS[kind])).cuda().bfloat16().eval()


@lru_cache(maxsize=None)
def _inputs():
    from flasht5_amd.generation import check_padding
    ids = torch.randint(2, 128, (B_, L_), generator=torch.Generator().manual_seed(22)).cuda()
    mask = (torch.arange(L_).unsqueeze(0) < torch.tensor(LENS).unsqueeze(1)).cuda()
    pad, _ = check_padding(ids, mask)
    assert pad.lengths == LENS
    return ids, mask, pad


def _indices():
    idx = torch.cat([torch.arange(n) + b * L_ for b, n in enumerate(LENS)]).cuda()
    cu = torch.tensor([0] + [sum(LENS[:b + 1]) for b in range(B_)], dtype=torch.int32).cuda()
    return idx, cu


def _scatter(h, idx):
    enc = h.new_zeros((B_ * L_, h.shape[-1]))
    enc.index_copy_(0, idx, h[0])
    return enc.view(B_, L_, -1)


def _packed_restated(stack, ids):
    """the encoder stack over the valid tokens only, every step of a block's packed self-attention written out: norm, three
    projections, rotary or the T5 generator of block 0, flash_attn_varlen_func, o and the residual; then the feed-forward layer"""
    from flasht5_amd.flash_attention_v2_bias import flash_attn_varlen_func
    from flasht5_amd.rotary import apply_rotary_emb_qkv
    idx, cu = _indices()
    mx, total = max(LENS), sum(LENS)
    h = stack.embed_tokens(ids.reshape(-1).index_select(0, idx).unsqueeze(0))   # (1, total, d_model)
    bias = None
    for blk in stack.block:
        sa = blk.self_attention_layer
        att = sa.self_attention
        H, D = att.n_heads, att.key_value_proj_dim
        n = sa.layer_norm(h)
        q, k, v = (w(n).view(total, H, D) for w in (att.Wq, att.Wk, att.Wv))
        rpe1d, radius = None, 0
        if att.rotary:
            cos, sin, cos_k, sin_k = att.pe_encoding.tables(q.device, q.dtype)
            q, k, v = apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k, sin_k, att.pe_encoding.interleaved, cu_seqlens=cu, max_seqlen=mx)
        else:
            if bias is None:
                bias = att.pe_encoding.forward_1d()   # (block 0 owns the generator; the others are handed it)
            rpe1d, radius = bias
        o = flash_attn_varlen_func(q, k, v, cu, cu, mx, mx, False, att.softmax_scale, rpe1d, radius, window=att.window)
        h = h + att.o(o.reshape(1, total, att.inner_dim))
        h = blk.ff_layer(h)
    return _scatter(stack.final_layer_norm(h), idx)


def _dense_restated(stack, ids, mask):
    """the encoder stack under the dense-bias type: block 0's (1, H, L, L) bias with the padded key columns at the dtype's
    minimum, handed to every block; the padded rows of the result zeroed"""
    h = stack.embed_tokens(ids)
    att = stack.block[0].self_attention_layer.self_attention
    bias = att.pe_encoding.compute_bias(L_, L_, device=h.device).to(h.dtype)
    bias = torch.where(mask.view(B_, 1, 1, L_), bias, torch.finfo(h.dtype).min).contiguous()
    for blk in stack.block:
        h, bias = blk(h, bias, None)
    return stack.final_layer_norm(h).masked_fill(~mask.unsqueeze(-1), 0)


def _restated(model):
    ids, mask, _ = _inputs()
    if model.encoder.block[0].self_attention_layer.self_attention.attention_type == "triton":
        return _dense_restated(model.encoder, ids, mask)
    return _packed_restated(model.encoder, ids)


@torch.no_grad()
@pytest.mark.parametrize("kind", list(KINDS))
def test_padded_encode_is_the_restatement(kind):
    from flasht5_amd.generation import encode
    ids, mask, pad = _inputs()
    model = _model(kind)
    assert len(model.encoder.block) == 2
    if kind == "local_t5":   # (narrower than the longest row: the window cuts keys off)
        assert model.encoder.block[1].self_attention_layer.self_attention.window == 3 < max(LENS) - 1
    got, want = encode(model, ids, pad), _restated(model)
    assert got.shape == (B_, L_, 64) and got.dtype == torch.bfloat16
    assert torch.equal(got, want)
    assert not bool(got[~mask].any()) and bool(got[mask].any(-1).all())   # the padded rows exactly zero, the valid ones not
    assert torch.equal(model.init_decode_state(ids, 4, attention_mask=pad).encoder_hidden_states, want)


@torch.no_grad()
def test_the_padded_path_ignores_the_fuse_flags():
    from flasht5_amd.generation import encode
    ids, _, pad = _inputs()
    model = _model("rpe_t5", fuse_norm_linear=True)
    assert model.encoder.fuse_norm_linear
    assert torch.equal(encode(model, ids, pad), _restated(model))


@torch.no_grad()
def test_mxfp4_runs_through_the_same_plumbing():
    """encode(..., "mxfp4") is w4a8.encoder_forward_mxfp4 over the gathered ids with the rows' Packed, scattered into zeros; the
    encoder-only model, which packs with its own plan, gives the same tensor"""
    from flasht5_amd import FAT5EncoderModel, w4a8
    from flasht5_amd.generation import encode
    from flasht5_amd.packing import Packed
    ids, mask, pad = _inputs()
    model = _model("rpe_t5")
    weights = model.quantize_encoder_weights_mxfp4()
    idx, cu = _indices()
    h = w4a8.encoder_forward_mxfp4(model.encoder, weights, ids.reshape(-1).index_select(0, idx).unsqueeze(0), packing=Packed(cu, 12))
    want = _scatter(h, idx)
    got = encode(model, ids, pad, "mxfp4")
    assert torch.equal(got, want) and not bool(got[~mask].any())
    assert not torch.equal(want, _restated(model))   # (the quantised stack, not the 16-bit one)
    enc = FAT5EncoderModel(_config(**KINDS["rpe_t5"])).cuda().bfloat16().eval()
    enc.encoder.load_state_dict(model.encoder.state_dict())   # (embed_tokens is the model's `shared`)
    enc.quantize_encoder_weights_mxfp4()
    assert torch.equal(enc(ids, attention_mask=mask, weight_dtype="mxfp4"), want)
    assert torch.equal(enc(ids, attention_mask=mask), _restated(model))
