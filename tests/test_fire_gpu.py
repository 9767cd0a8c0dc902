"""GPU tests of the FIRE position bias (flasht5_amd/fire.py, csrc/fire_kernels.h): the forward producer against an fp64 eager
restatement of the reference formula, the backward against fp64 autograd and the reference fixture (tests/golden/fire.npz), bitwise
determinism, a bias of more than 2^31 elements, FlashT5Attention with FIRE over two blocks, and a captured training step."""
import ctypes
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
from attn_helpers import maxdiff
from fire_eager import bwd_scale, fire_eager, fwd_scale
from golden_io import GOLDEN

pytestmark = pytest.mark.gpu

HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}  # relative half-ulp of the output type


def _fire_params(H, W, seed, c=0.1, lm=1.0, l0=128.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    p = {
        "w1": torch.randn(W, 1, generator=g), "b1": torch.randn(W, generator=g) * 0.5,
        "w2": torch.randn(H, W, generator=g) / math.sqrt(W), "b2": torch.randn(H, generator=g) * 0.1,
        "c": torch.tensor(c), "L_multiplier": torch.tensor(lm), "init_L": torch.tensor(l0),
    }
    return {k: v.to(dtype).cuda() for k, v in p.items()}


def _args(p):
    return p["w1"], p["b1"], p["w2"], p["b2"], p["c"], p["L_multiplier"], p["init_L"]


def _check_fwd(out, p, M, N, rows=None):
    """|out - ref| <= 1e-5 * scale (+ half an ulp of a 16-bit output) on `rows` (all when None)"""
    ref = fire_eager(*(t.double() for t in _args(p)), M, N, rows=rows)
    scale = fwd_scale(*(t.double() for t in _args(p)), M, N, dev="cuda", rows=rows)
    got = out if rows is None else out[:, :, torch.as_tensor(rows, device=out.device)]
    err = (got.double() - ref).abs()
    tol = 1e-5 * scale + HALF_ULP[out.dtype] * ref.abs()
    bad = err > tol
    assert not bad.any(), (int(bad.sum()), float(err.max()), float((err / tol.clamp_min(1e-30)).max()))


MN = [(1, 1), (17, 17), (128, 129), (129, 128), (513, 17), (17, 513), (2048, 2048)]
HW = [(1, 1), (12, 32), (16, 64), (12, 8)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H, W", HW)
@pytest.mark.parametrize("M, N", MN)
def test_fire_fwd_matches_eager(M, N, H, W, dtype):
    from flasht5_amd.fire import fire_bias
    p = _fire_params(H, W, seed=M * 31 + N * 7 + H + W)
    out = fire_bias(*_args(p), M, N, 1e-6, dtype)
    assert out.shape == (1, H, M, N) and out.dtype == dtype
    rows = None if M * N <= 1 << 20 else sorted({0, 1, 127, 128, 129, 1000, M - 2, M - 1})
    _check_fwd(out, p, M, N, rows)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fire_fwd_strided_output(dtype):
    """the ABI writes (H, M, N) views with padded row and head strides; nothing outside the view is touched"""
    from flasht5_amd import _lib
    from flasht5_amd.fire import _params
    H, W, M, N = 12, 32, 100, 200
    p = _fire_params(H, W, seed=3)
    buf = torch.full((H, M + 3, N + 24), 7.0, dtype=dtype, device="cuda")
    view = buf[:, :M, :N]
    f = [t.float().contiguous().reshape(-1) for t in (p["w1"], p["b1"], p["b2"], p["c"], p["L_multiplier"], p["init_L"])]
    prm = _params(f[0], f[1], p["w2"].float().contiguous(), f[2], f[3], f[4], f[5], M, N, 1e-6, dtype)
    prm.bias = view.data_ptr()
    prm.bias_stride[0], prm.bias_stride[1] = view.stride(0), view.stride(1)
    _lib.check(_lib.load().fat5_fire_fwd(ctypes.byref(prm), _lib.stream_ptr(view.device)), "fat5_fire_fwd")
    torch.cuda.synchronize()
    _check_fwd(view.unsqueeze(0), p, M, N)
    assert (buf[:, M:, :] == 7).all() and (buf[:, :, N:] == 7).all()


def _check_bwd(grads, p, G, M, N, what="", rel=0.0):
    """each gradient entry within 1e-5 of its terms' magnitudes of fp64 autograd (+ `rel` of its value: a 16-bit parameter's rounding)"""
    leaves = {k: p[k].double().clone().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")}
    ref = fire_eager(leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], leaves["c"], leaves["L_multiplier"], p["init_L"].double(),
                     M, N)
    rg = torch.autograd.grad(ref, list(leaves.values()), G.double())
    bound = bwd_scale(G, *_args(p), M, N)
    for (k, _), g, r in zip(leaves.items(), grads, rg):
        assert g.shape == r.shape, (what, k)
        err = (g.double() - r).abs()
        tol = 1e-5 * bound[k] + rel * r.abs() + 1e-30
        assert (err <= tol).all(), (what, k, float(err.max()), float((err / tol).max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M, N, H, W, c, lm, l0", [
    (256, 256, 12, 32, 0.1, 1.0, 128),    # row 128 ties with T
    (129, 200, 16, 64, 0.1, 1.0, 64),     # M != N, N % 8 == 0
    (17, 513, 1, 1, 0.3, 1.0, 8),
    (300, 37, 12, 8, -0.3, -0.75, 40),    # negative c, L_multiplier; N % 8 != 0
    (96, 96, 64, 128, 0.25, 1.0, 48),     # the largest supported H and W
    (100, 100, 33, 17, 0.1, 0.5, 200),    # padded head and unit tiles; every row below T
])
def test_fire_bwd_matches_fp64_autograd(M, N, H, W, c, lm, l0, dtype):
    from flasht5_amd.fire import fire_bias
    p = _fire_params(H, W, seed=M + N + H + W, c=c, lm=lm, l0=float(l0))
    with torch.no_grad():
        p["b1"][::4] = 0.0  # relu'(0) = 0 on the diagonal
    leaves = [p[k].clone().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")]
    out = fire_bias(*leaves, p["init_L"], M, N, 1e-6, dtype)
    G = torch.randn(out.shape, device="cuda").to(dtype)
    grads = torch.autograd.grad(out, leaves, G)
    assert all(g.dtype == torch.float32 for g in grads)
    _check_bwd(grads, p, G.float(), M, N, str(dtype))


def test_fire_bwd_param_dtypes():
    """bf16 / fp16 parameters: fp32 compute, gradients in each parameter's dtype"""
    from flasht5_amd.fire import fire_bias
    for pdt in (torch.bfloat16, torch.float16):
        p = _fire_params(12, 32, seed=9, dtype=pdt)
        leaves = [p[k].clone().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")]
        out = fire_bias(*leaves, p["init_L"], 200, 200, 1e-6, torch.bfloat16)
        G = torch.randn(out.shape, device="cuda").bfloat16()
        grads = torch.autograd.grad(out, leaves, G)
        assert [g.dtype for g in grads] == [pdt] * 6
        pf = {k: v.float() for k, v in p.items()}
        _check_fwd(out, pf, 200, 200)
        leaves32 = [pf[k].clone().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")]
        g32 = torch.autograd.grad(fire_bias(*leaves32, pf["init_L"], 200, 200, 1e-6, torch.bfloat16), leaves32, G)
        for a, b in zip(grads, g32):
            assert torch.equal(a, b.to(pdt))


@pytest.mark.parametrize("name", ["t128_tie", "zero_b1", "neg_c_lm", "w8_h6"])
def test_fire_matches_reference_fixture(name):
    from flasht5_amd.fire import fire_bias
    z = np.load(os.path.join(GOLDEN, "fire.npz"))
    g = {k.split("__")[1]: z[k] for k in z.files if k.startswith(name + "__")}
    t = {k: torch.from_numpy(np.array(v, copy=True)).cuda() for k, v in g.items() if k not in ("dbias", "meta")}
    G = torch.from_numpy(g["dbias"].view(np.int16).copy()).view(torch.bfloat16).float().cuda()
    S, H, W, eps = g["meta"].tolist()
    S = int(S)
    p = {k: t[k] for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier", "init_L")}
    leaves = [p[k].clone().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")]
    out = fire_bias(*leaves, p["init_L"], S, S, eps, torch.float32)
    scale = fwd_scale(*(x.double() for x in _args(p)), S, S, eps, dev="cuda")
    assert ((out.double() - t["bias"].double()).abs() <= 1e-5 * scale).all()
    grads = torch.autograd.grad(out, leaves, G)
    bound = bwd_scale(G, *_args(p), S, S, eps)
    for k, gk in zip(("w1", "b1", "w2", "b2", "c", "L_multiplier"), grads):
        err = (gk.double() - t[f"grad_{k}"].double()).abs()
        assert (err <= 1e-5 * bound[k] + 1e-30).all(), (name, k, float(err.max()))
    _check_bwd(grads, {k: v for k, v in p.items()}, G, S, S, name)


def test_fire_rejects_host_parameters_before_launch():
    """a CPU init_L (the natural way to pass the non-trainable scalar) or c is rejected; nothing is launched"""
    from flasht5_amd.fire import FIRE, fire_bias
    p = _fire_params(12, 32, seed=21)
    for name in ("init_L", "c", "w1"):
        args = dict(p)
        args[name] = args[name].cpu()
        with pytest.raises(ValueError, match=f"{name} is on cpu"):
            fire_bias(*_args(args), 64, 64)
    m = FIRE(12, 32, 0.1, 128)
    m.mlp.cuda()  # (c, L_multiplier, init_L left on the host)
    with pytest.raises(ValueError, match="is on cpu"):
        m.compute_bias(64, 64, "cuda", torch.bfloat16)
    torch.cuda.synchronize()
    out = fire_bias(*_args(p), 64, 64)  # (the device is fine afterwards)
    _check_fwd(out, p, 64, 64)


@pytest.mark.parametrize("N", [64, 37])
def test_fire_fwd_strides_match_fake(N):
    """the real op's strides are the fake's (rows padded to 16 bytes when N % 8 != 0)"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd.fire import fire_fwd
    p = _fire_params(12, 8, seed=22)
    f = [p[k].float().contiguous().reshape(-1) for k in ("w1", "b1", "b2", "c", "L_multiplier", "init_L")]
    args = (f[0], f[1], p["w2"].float().contiguous(), f[2], f[3], f[4], f[5], 50, N, 1e-6, torch.bfloat16)
    real = fire_fwd(*args)
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        fake = fire_fwd(*(mode.from_tensor(a) if isinstance(a, torch.Tensor) else a for a in args))
    assert real.shape == fake.shape and real.stride() == fake.stride()
    _check_fwd(real.unsqueeze(0), p, 50, N)


@pytest.mark.parametrize("reduce", ["sum_rows", "mean_heads"])
def test_fire_bwd_expanded_upstream_gradient(reduce):
    """a stride-0 upstream gradient (the backward of bias.sum(-2) / bias.mean(1)) takes the copy path and is exact"""
    from flasht5_amd.fire import fire_bias
    H, W, M, N = 12, 32, 96, 80
    p = _fire_params(H, W, seed=23)
    leaves = [p[k].clone().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")]
    out = fire_bias(*leaves, p["init_L"], M, N, 1e-6, torch.float32)
    red = out.sum(-2) if reduce == "sum_rows" else out.mean(1)
    r = torch.randn(red.shape, device="cuda")
    grads = torch.autograd.grad((red * r).sum(), leaves)
    G = (r.unsqueeze(-2).expand(1, H, M, N) if reduce == "sum_rows" else (r / H).unsqueeze(1).expand(1, H, M, N))[0]
    _check_bwd(grads, p, G.unsqueeze(0).contiguous(), M, N, reduce)


def test_fire_bwd_is_deterministic():
    from flasht5_amd.fire import fire_bwd
    H, W, S = 12, 32, 1024
    p = _fire_params(H, W, seed=11)
    G = torch.randn(H, S, S, device="cuda").bfloat16()
    f = [p[k].float().contiguous().reshape(-1) for k in ("w1", "b1", "b2", "c", "L_multiplier", "init_L")]
    args = (f[0], f[1], p["w2"].float().contiguous(), f[2], f[3], f[4], f[5], 1e-6)
    a = fire_bwd(G, *args)
    b = fire_bwd(G, *args)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = fire_bwd(G, *args)
    g.replay()
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))


def test_fire_fwd_more_than_2_31_elements():
    """H = 1, M = N = 46341: 2 147 488 281 bias elements; sampled rows, the last included"""
    from flasht5_amd.fire import fire_bias
    M = N = 46341
    p = _fire_params(1, 8, seed=13)
    out = fire_bias(*_args(p), M, N, 1e-6, torch.bfloat16)
    assert out.numel() > 2 ** 31
    rows = [0, 1, 128, 46339 // 2, M - 2, M - 1]
    _check_fwd(out, p, M, N, rows)
    del out
    torch.cuda.empty_cache()


def _cfg(decoder):
    return SimpleNamespace(d_model=128, d_kv=64, num_heads=4, relative_attention_num_buckets=32, relative_attention_max_distance=64,
                           is_decoder=decoder, attention_type="triton", position_encoding_type="FIRE", attention_scale=None,
                           fire_mlp_width=32)


def _eager_layer(w, h, cfg, causal, bias):
    """eager fp32 restatement of the reference's self-attention (modeling_flash_t5.py:245-287) with a given bias"""
    H, Dh = cfg.num_heads, cfg.d_kv
    B, M = h.shape[0], h.shape[1]
    q = (h @ w["Wq"].t()).view(B, M, H, Dh).permute(0, 2, 1, 3)
    k = (h @ w["Wk"].t()).view(B, M, H, Dh).permute(0, 2, 1, 3)
    v = (h @ w["Wv"].t()).view(B, M, H, Dh).permute(0, 2, 1, 3)
    o = oracle.attn_ref(q, k, v, bias, 1.0 / math.sqrt(H), causal=causal, upcast=True)
    return o.permute(0, 2, 1, 3).reshape(B, M, H * Dh) @ w["o"].t()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("decoder", [False, True])
def test_flasht5_attention_fire_two_blocks(decoder, fused):
    """block 0 builds FIRE and hands its bias to block 1; output and every parameter gradient (FIRE's included) against the eager
    fp32 restatement (the reference formula in fp32, the bias rounded to bf16 as the module does, the oracle attention)"""
    from flasht5_amd import FlashT5Attention
    cfg = _cfg(decoder)
    torch.manual_seed(43)
    blk0 = FlashT5Attention(cfg, has_positional_encoding=True, is_causal=decoder).cuda().bfloat16()
    blk1 = FlashT5Attention(cfg, has_positional_encoding=False, is_causal=decoder).cuda().bfloat16()
    B, S = 2, 300  # rows 64.. are past T = 64
    x = torch.randn(B, S, cfg.d_model, device="cuda").bfloat16()
    gy = torch.randn(B, S, cfg.d_model, device="cuda").bfloat16()
    nw = torch.ones(cfg.d_model, device="cuda").bfloat16()
    if fused:
        y0, pb = blk0.forward_fused(x, nw, 1e-6)
        y1, pb1 = blk1.forward_fused(y0, nw, 1e-6, position_bias=pb)
    else:
        y0, pb = blk0(x)
        y1, pb1 = blk1(y0, position_bias=pb)
    assert pb.shape == (1, cfg.num_heads, S, S) and pb.dtype == torch.bfloat16 and pb1 is pb
    assert pb.stride() == (cfg.num_heads * S * 304, S * 304, 304, 1)  # (S = 300: rows padded to 16 bytes, no contiguous copy)
    mods = (blk0, blk1)
    params = [p for m in mods for p in m.parameters() if p.requires_grad]
    *grads, dS_mod = torch.autograd.grad(y1, params + [pb], gy)

    names = [(i, n) for i, m in enumerate(mods) for n, p in m.named_parameters() if p.requires_grad]
    leaves = {(i, n): p.detach().float().clone().requires_grad_() for (i, n), p in zip(names, params)}
    w0 = {n.split(".")[0]: leaves[(0, n)] for i, n in names if i == 0 and not n.startswith("pe_encoding")}
    w1 = {n.split(".")[0]: leaves[(1, n)] for i, n in names if i == 1}
    fp = {n[len("pe_encoding."):]: leaves[(0, n)] for i, n in names if n.startswith("pe_encoding")}
    bias = fire_eager(fp["mlp.0.weight"], fp["mlp.0.bias"], fp["mlp.2.weight"], fp["mlp.2.bias"], fp["c"], fp["L_multiplier"],
                      blk0.pe_encoding.init_L.float(), S, S, dtype=torch.float32)
    bias = bias + (bias.detach().bfloat16().float() - bias.detach())  # the module's cast of the bias to q's dtype
    xr = x.float()
    rms = lambda t: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)  # noqa: E731  (T5 RMSNorm, unit weight)
    if fused:
        r0 = xr + _eager_layer(w0, rms(xr), cfg, decoder, bias)
        r1 = r0 + _eager_layer(w1, rms(r0), cfg, decoder, bias)
    else:
        r0 = _eager_layer(w0, xr, cfg, decoder, bias)
        r1 = _eager_layer(w1, r0, cfg, decoder, bias)
    *ref_grads, dS = torch.autograd.grad(r1, [leaves[k] for k in names] + [bias], gy.float())
    assert maxdiff(y1, r1) <= 3e-2 * max(1.0, r1.abs().max().item()), maxdiff(y1, r1)
    # (1) the gradient that reaches the bias (summed over both blocks) against the eager one, under the parity bound
    assert maxdiff(dS_mod, dS) <= 4e-2 * max(1e-3, dS.abs().max().item()), (maxdiff(dS_mod, dS), dS.abs().max().item())
    # (2) FIRE's parameter gradients in the module against fp64 autograd of the formula driven by THAT gradient, entry by entry
    #     within 1e-5 of each entry's term magnitudes (the wiring: the module's FIRE receives and reduces exactly what attention sends)
    ps = {"mlp.0.weight": "w1", "mlp.0.bias": "b1", "mlp.2.weight": "w2", "mlp.2.bias": "b2", "c": "c", "L_multiplier": "L_multiplier"}
    fire_mod = blk0.pe_encoding
    p32 = {"w1": fire_mod.mlp[0].weight.float(), "b1": fire_mod.mlp[0].bias.float(), "w2": fire_mod.mlp[2].weight.float(),
           "b2": fire_mod.mlp[2].bias.float(), "c": fire_mod.c.float(), "L_multiplier": fire_mod.L_multiplier.float(),
           "init_L": fire_mod.init_L.float()}
    own = {ps[n[len("pe_encoding."):]]: g.float() for (i, n), g in zip(names, grads) if n.startswith("pe_encoding")}
    _check_bwd([own[k] for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")], {k: v.detach() for k, v in p32.items()},
               dS_mod.float(), S, S, "module", rel=2.0 ** -8)
    # (3) and against the fully eager chain entry by entry: relative, plus 2^-8 of each entry's term magnitudes for the bf16
    #     rounding of the S^2 bias-gradient entries FIRE sums (b2's exact gradient is zero: softmax ignores a constant shift)
    scale = bwd_scale(dS, fp["mlp.0.weight"].detach(), fp["mlp.0.bias"].detach(), fp["mlp.2.weight"].detach(), fp["mlp.2.bias"].detach(),
                      fp["c"].detach(), fp["L_multiplier"].detach(), blk0.pe_encoding.init_L.float(), S, S)
    for (i, n), g, rg in zip(names, grads, ref_grads):
        assert torch.isfinite(g.float()).all(), n
        if n.startswith("pe_encoding"):
            err = (g.double() - rg.double()).abs()
            tol = 4e-2 * rg.double().abs() + 2.0 ** -8 * scale[ps[n[len("pe_encoding."):]]].reshape(rg.shape)
            assert (err <= tol).all(), (n, float(err.max()), float((err / tol).max()))
        else:
            assert maxdiff(g, rg) <= 4e-2 * max(1.0, rg.abs().max().item()), (n, maxdiff(g, rg), rg.abs().max().item())


def test_graphed_train_step_fire():
    """a 2-layer FIRE FAT5 model: the captured step (FIRE forward and backward launches inside the graph) follows the eager step"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, AdamWScale, train_step, GraphedTrainStep
    cfg = FAT5Config(num_layers=2, num_decoder_layers=2, vocab_size=4096, position_encoding_type="FIRE", attention_type="triton")
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
        for stack in (model.encoder, model.decoder):  # FIRE's parameters received gradients (the optimizer's first moments)
            fire = stack.block[0].self_attention_layer.self_attention.pe_encoding
            for prm in (fire.c, fire.L_multiplier, fire.mlp[0].weight, fire.mlp[2].weight):
                assert float(opt.state[prm]["exp_avg"].float().abs().max()) > 0
        runs.append((losses, [p.detach().float().clone() for p in model.parameters()]))
    (l0, p0), (l1, p1) = runs
    assert all(math.isfinite(a) for a in l0)
    assert l0[0] == l1[0]
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(l0, l1)), (l0, l1)
    for a, b in zip(p0, p1):
        assert float((a - b).abs().max()) <= 2.0 ** -6 * max(float(a.abs().max()), 1e-3)
