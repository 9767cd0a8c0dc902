"""The MXFP8 activation quantiser and the W4A8 block-scaled MFMA linear on the GPU against tests/w4a8_ref.py: the quantiser's
bytes, the linear inside its fp64 bound (the one-hot case first: it pins the instruction's lane map), the bitwise identities,
NaN poisoning, and the encoder of the models over MXFP4 weights against a hand composition of the public operators."""
import pytest
import torch

import w4_ref
import w4a8_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
INF, NAN = float("inf"), float("nan")
SPECIAL = [[0.0], [4.0, 1.0, -0.5], [28.0, -14.0, 3.0], [32.0, 28.0], [30.0, 29.5, -29.0], [256.0, 17.0, 19.0, -21.0],
           [256.0, 2.0 ** -7, 3 * 2.0 ** -10, -2.0 ** -10], [1.0, INF, -2.0], [NAN, 5.0]]
# the scale byte and the leading e4m3fn codes of each SPECIAL block, by hand: a zero block; amax a power of two; amax = 448 * 2^-4;
# the scale's next step; 480, 472 and the tie 464 saturate at 448; ties to even (17 -> 16, 19 -> 20, -21 -> -20); e4m3 subnormals
# (4, then the ties 1.5 -> 2 and -0.5 -> -0 in units of 2^-9); an inf and a NaN poison their blocks
HAND = [(127, [0x00]), (121, [0x78, 0x68, 0xE0]), (123, [0x7E, 0xF6, 0x64]), (124, [0x78, 0x76]), (123, [0x7E, 0x7E, 0xFE]),
        (127, [0x78, 0x58, 0x5A, 0xDA]), (127, [0x78, 0x04, 0x02, 0x80]), (255, [0, 0, 0]), (255, [0, 0])]


def activations(Rr, K, dtype, seed=0):
    """random rows whose blocks differ in magnitude, the hand-made blocks of SPECIAL in front"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Rr, K // 32, 32, generator=g) * torch.pow(2.0, torch.randint(-6, 7, (Rr, K // 32, 1), generator=g).float())
    flat = x.view(-1, 32)
    for i, blk in enumerate(SPECIAL[:flat.shape[0]]):
        flat[i] = torch.tensor(blk + [0.0] * (32 - len(blk)))
    return x.view(Rr, K).to(dtype)


def weights(N, K, seed=1):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K // 32, 32, generator=g) * torch.pow(2.0, torch.randint(-4, 3, (N, K // 32, 1), generator=g).float())
    return w4_ref.quantize_ref(W.view(N, K))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr, K", [(1, 32), (3, 160), (17, 768)])
def test_quantiser_bytes(Rr, K, dtype):
    from flasht5_amd import fast_rms_layernorm, quantize_activation_mxfp8
    x = activations(Rr, K, dtype)
    a8, ax = quantize_activation_mxfp8(x.cuda())
    want8, wantx = R.quantize_act_ref(x)
    assert torch.equal(ax.cpu(), wantx) and torch.equal(a8.cpu(), want8)
    for i, (byte, codes) in enumerate(HAND[:Rr * K // 32]):
        assert int(ax.view(-1)[i]) == byte and a8.view(-1, 32)[i].tolist() == codes + [0] * (32 - len(codes)), SPECIAL[i]
    xf = activations(Rr, K, dtype, seed=2).nan_to_num(0.0, 1.0, -1.0).cuda()
    g = (1 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(3))).to(dtype).cuda()
    n8, nx = quantize_activation_mxfp8(xf, norm_weight=g, eps=1e-6)
    p8, px = quantize_activation_mxfp8(fast_rms_layernorm(xf, g, 1e-6))
    assert torch.equal(n8, p8) and torch.equal(nx, px)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr, K, N", [(16, 128, 16), (1, 32, 8), (17, 160, 24), (128, 768, 128), (129, 128, 136), (257, 896, 264)])
def test_linear_inside_the_bound(Rr, K, N, dtype):
    """c = 16 of w4a8_ref.bound comes from the c = 1 ratios measured at K = 128 over every (R, N) of these cases (worst 1.5843 bf16,
    4.2946 fp16; twice, next power of two); the one-hot case and (1, 32, 8) are exact"""
    from flasht5_amd import w4a8_matmul
    x = activations(Rr, K, dtype, seed=4).nan_to_num(0.0, 1.0, -1.0)
    if (Rr, K, N) == (16, 128, 16):   # one-hot rows: element (r, n) is ONE product, a[r, k_r] w[n, k_r] -- the lane map
        hot = torch.zeros_like(x)
        for r in range(Rr):
            hot[r, (37 * r + 5) % K] = x[r, (37 * r + 5) % K] + 1
        x = hot
    a8, ax = R.quantize_act_ref(x)
    w4, e8 = weights(N, K)
    y = w4a8_matmul(a8.cuda(), ax.cuda(), w4.cuda(), e8.cuda(), dtype).cpu().double()
    ref, A = R.linear_ref(a8, ax, w4, e8)
    ratio = ((y - ref).abs() / R.bound(ref, A, K, dtype)).nan_to_num(0.0).max()
    ratio1 = ((y - ref).abs() / R.bound(ref, A, K, dtype, c=1)).nan_to_num(0.0).max()
    print(f"w4a8 bound ratio (R, K, N) = {(Rr, K, N)} {dtype}: {float(ratio):.4f} (against c = 1: {float(ratio1):.4f})")
    assert bool(torch.isfinite(y).all()) and float(ratio) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_are_bitwise(dtype):
    from flasht5_amd import quantize_activation_mxfp8, w4a8_linear, w4a8_matmul
    Rr, K, N = 257, 160, 136
    x = activations(Rr, K, dtype, seed=5).nan_to_num(0.0, 1.0, -1.0).cuda()
    w4, e8 = (t.cuda() for t in weights(N, K))
    res = torch.randn(Rr, N, generator=torch.Generator().manual_seed(6)).to(dtype).cuda()
    y = w4a8_linear(x, w4, e8)
    assert torch.equal(w4a8_linear(x, w4, e8, residual=res), res + y)
    for r in (0, 127, 128, 256):
        assert torch.equal(w4a8_linear(x[r:r + 1], w4, e8)[0], y[r]), r
    a8, ax = quantize_activation_mxfp8(x)
    assert torch.equal(w4a8_matmul(a8, ax, w4, e8, dtype), y) and torch.equal(w4a8_linear(x, w4, e8), y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w4a8_linear(x, w4, e8)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = w4a8_linear(x, w4, e8)
    for _ in range(2):
        out.zero_()
        graph.replay()
        assert torch.equal(out, y)


def test_scale_byte_255_poisons_its_row_or_column():
    from flasht5_amd import w4a8_matmul
    Rr, K, N, dtype = 130, 160, 136, torch.bfloat16
    x = activations(Rr, K, dtype, seed=7).nan_to_num(0.0, 1.0, -1.0)
    x[129, 70] = NAN
    a8, ax = R.quantize_act_ref(x)
    w4, e8 = weights(N, K)
    e8[131, 4] = 255
    y = w4a8_matmul(a8.cuda(), ax.cuda(), w4.cuda(), e8.cuda(), dtype).cpu().double()
    bad = torch.zeros(Rr, N, dtype=torch.bool)
    bad[129, :] = True
    bad[:, 131] = True
    assert torch.equal(torch.isnan(y), bad)
    ref, A = R.linear_ref(a8, ax, w4, e8)
    assert bool(((y - ref).abs() <= R.bound(ref, A, K, dtype))[~bad].all())


def _model(cls, **kw):
    import flasht5_amd as F
    cfg = F.FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=1,
                       relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe", **kw)
    torch.manual_seed(11)
    return cls(cfg).cuda().bfloat16().eval()


def _by_hand(m, ids, lens):
    """the one-block encoder over the valid tokens, composed from the public operators"""
    import flasht5_amd as F
    blk, lw = m.encoder.block[0], m.quantize_encoder_weights_mxfp4().layers[0]
    sa, ff, att = blk.self_attention_layer, blk.ff_layer, blk.self_attention_layer.self_attention
    idx = torch.cat([torch.arange(n) + b * ids.shape[1] for b, n in enumerate(lens)]).cuda()
    cu = torch.tensor([0] + [sum(lens[:b + 1]) for b in range(len(lens))], dtype=torch.int32).cuda()
    h = m.shared(ids.reshape(-1)[idx])
    qkv = F.w4a8_linear(h, *lw.qkv, norm_weight=sa.layer_norm.weight, eps=sa.layer_norm.variance_epsilon)
    q, k, v = (t.reshape(-1, att.n_heads, att.key_value_proj_dim) for t in qkv.chunk(3, dim=-1))
    rpe1d, radius = att.pe_encoding.forward_1d()
    o = F.flash_attn_varlen_func(q, k, v, cu, cu, max(lens), max(lens), False, att.softmax_scale, rpe1d, radius)
    h = F.w4a8_linear(o.reshape(-1, att.inner_dim), *lw.o, residual=h)
    g = F.w4a8_linear(h, *lw.wi, norm_weight=ff.layer_norm.weight, eps=ff.layer_norm.variance_epsilon)
    h = F.w4a8_linear(F.gated_act_packed(g, ff.act.act_name), *lw.wo, residual=h)
    h = F.fast_rms_layernorm(h, m.encoder.final_layer_norm.weight, m.encoder.final_layer_norm.variance_epsilon)
    return torch.zeros(ids.numel(), h.shape[-1], dtype=h.dtype, device="cuda").index_copy(0, idx, h).view(*ids.shape, -1)


@torch.no_grad()
def test_models_run_their_encoder_over_mxfp4_weights():
    import flasht5_amd as F
    from flasht5_amd.generation import check_padding, encode
    lens = [12, 7, 16]
    ids = torch.randint(2, 128, (3, 16), generator=torch.Generator().manual_seed(12)).cuda()
    mask = (torch.arange(16).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).cuda()
    m = _model(F.FAT5EncoderModel)
    with pytest.raises(ValueError, match="quantize_encoder_weights_mxfp4"):
        m(ids, attention_mask=mask, weight_dtype="mxfp4")
    want = _by_hand(m, ids, lens)
    got = m(ids, attention_mask=mask, weight_dtype="mxfp4")
    assert torch.equal(got, want) and not torch.equal(got, m(ids, attention_mask=mask))
    for b, n in enumerate(lens):
        assert torch.equal(m(ids[b:b + 1, :n], weight_dtype="mxfp4")[0], got[b, :n]), b
    s = _model(F.FAT5ForConditionalGeneration)
    s.quantize_encoder_weights_mxfp4()
    pad, _ = check_padding(ids, mask)
    assert torch.equal(encode(s, ids, pad, encoder_weight_dtype="mxfp4"), _by_hand(s, ids, lens))
    out = s.generate(ids, attention_mask=mask, max_length=6, encoder_weight_dtype="mxfp4")
    state = s.init_decode_state(ids, 6, attention_mask=mask, encoder_weight_dtype="mxfp4")
    assert out.shape[0] == 3 and torch.equal(state.encoder_hidden_states, _by_hand(s, ids, lens))
