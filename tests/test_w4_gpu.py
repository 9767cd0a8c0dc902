"""MXFP4 weights on the device (csrc/w4_kernels.h): the quantiser's bytes against the restated rule, `w4_linear` inside the derived
per-element bound against fp64 (tests/w4_ref.py) at the seams of its tiling, the bit identities of norm, residual, replay and row
count, poison, and `generate(weight_dtype="mxfp4")`."""
import copy
import ctypes

import pytest
import torch

import w4_ref as R
from test_w4_cpu import hand_blocks
from test_w8_generation_gpu import _decisive, _small

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def w4():
    from flasht5_amd import w4 as mod
    return mod


def _problem(Rr, K, N, dtype, seed=0):
    """test_w8_gpu._problem's inputs, quantised by the rule: (x, w4, e8, gamma, residual) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Rr, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    gam = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    res = torch.randn(Rr, N, generator=g).to(dtype)
    return (x,) + R.quantize_ref(W) + (gam, res)


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32])
@pytest.mark.parametrize("N, K", [(8, 32), (24, 96), (40, 160), (16, 2080)])
def test_quantiser_bits(w4, dtype, N, K):
    W = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 3
    W[N - 1] *= 2.0 ** -20                                  # blocks far below the clamp
    for i, (v, _, _) in enumerate(hand_blocks().values()):  # row i opens with hand-made block i
        W[i, :32] = v
    W = W.to(dtype)
    want4, want8 = R.quantize_ref(W)
    out = torch.full((N + 2, K // 2 + 16), 0x55, dtype=torch.uint8, device=DEV)      # strided rows, guarded all round
    sc = torch.full((N + 2, K // 32 + 3), 0x55, dtype=torch.uint8, device=DEV)
    got4, got8 = w4.quantize_weight_mxfp4(W.to(DEV), out[1:N + 1, :K // 2], sc[1:N + 1, :K // 32])
    assert torch.equal(got4.cpu(), want4) and torch.equal(got8.cpu(), want8)
    out[1:N + 1, :K // 2], sc[1:N + 1, :K // 32] = 0x55, 0x55
    assert bool((out == 0x55).all()) and bool((sc == 0x55).all())
    b4, b8 = w4.quantize_weight_mxfp4(W.to(DEV))                                     # new tensors: the same bytes
    assert torch.equal(b4.cpu(), want4) and torch.equal(b8.cpu(), want8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [32, 96, 128, 160, 832])
def test_linear_inside_the_bound(w4, dtype, K):
    assert (w4.ROW_TILE, w4.COLS, w4.K_CHUNK) == (32, 32, 128)      # (the seams below: 16-row fragments, 32-row tiles, 128-k chunks)
    worst = 0.0
    for Rr in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        for N in (8, 24, 40):
            x, q4, e8, _, _ = _problem(Rr, K, N, dtype, seed=Rr * 131 + N)
            wide = torch.zeros(Rr, K + 24, dtype=dtype, device=DEV)   # a row stride larger than the width
            wide[:, :K] = x.to(DEV)
            y = w4.w4_linear(wide[:, :K], q4.to(DEV), e8.to(DEV)).cpu()
            ref, A = R.linear_ref(x, q4, e8)
            ratio = float(((y.double() - ref).abs() / R.bound(ref, A, K, dtype)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (Rr, K, N, ratio)
    print(f"[w4] K {K} {dtype}: worst |y - ref| / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr, K, N", [(9, 832, 24), (65, 768, 40), (17, 160, 16)])
def test_fusion_is_invisible_in_the_bits(w4, dtype, Rr, K, N):
    from flasht5_amd import _lib, fast_rms_layernorm
    x, q4, e8, gam, res = (t.to(DEV) for t in _problem(Rr, K, N, dtype, seed=11))
    plain = w4.w4_linear(x, q4, e8)
    normed = w4.w4_linear(fast_rms_layernorm(x, gam, 1e-6), q4, e8)
    assert torch.equal(w4.w4_linear(x, q4, e8, norm_weight=gam, eps=1e-6), normed)
    assert torch.equal(w4.w4_linear(x, q4, e8, residual=res), res + plain)
    assert torch.equal(w4.w4_linear(x, q4, e8, norm_weight=gam, eps=1e-6, residual=res), res + normed)
    assert not torch.equal(plain, normed)
    ybuf = torch.full((Rr, N + 8), 77.0, dtype=dtype, device=DEV)      # a strided y through the C ABI
    p = _lib.W4LinearParams()
    p.R, p.N, p.K, p.dtype = Rr, N, K, _lib.dtype_code(dtype)
    p.x, p.x_stride, p.w4, p.w_stride, p.e8, p.e_stride = x.data_ptr(), K, q4.data_ptr(), K // 2, e8.data_ptr(), K // 32
    p.residual, p.residual_stride, p.y, p.y_stride = res.data_ptr(), N, ybuf.data_ptr(), N + 8
    _lib.check(_lib.load().fat5_w4_linear(ctypes.byref(p), _lib.stream_ptr(x.device)), "fat5_w4_linear")
    torch.cuda.synchronize()
    assert torch.equal(ybuf[:, :N], res + plain) and bool((ybuf[:, N:] == 77.0).all())


def test_same_bits_in_two_runs_under_a_graph_and_for_any_row_count(w4):
    x, q4, e8, gam, res = (t.to(DEV) for t in _problem(64, 768, 72, torch.bfloat16, seed=5))
    run = lambda: w4.w4_linear(x, q4, e8, norm_weight=gam, residual=res)  # noqa: E731
    a = run()
    assert torch.equal(a, run())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = run()
    for _ in range(3):
        c.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, c)
    x, q4, e8, _, _ = (t.to(DEV) for t in _problem(65, 832, 72, torch.bfloat16, seed=6))
    whole = w4.w4_linear(x, q4, e8)
    for r0 in (0, 16, 24, 48):
        assert torch.equal(whole[r0:r0 + 16], w4.w4_linear(x[r0:r0 + 16], q4, e8))
    for r in (0, 21, 63, 64):
        assert torch.equal(whole[r:r + 1], w4.w4_linear(x[r:r + 1], q4, e8))


def test_poison_stays_where_it_is(w4):
    Rr, K, N = 17, 160, 24
    x = _problem(Rr, K, N, torch.bfloat16, seed=9)[0]
    W = (torch.randn(N, K, generator=torch.Generator().manual_seed(1)) * 0.05).bfloat16()
    x[2, 17] = float("nan")
    y = w4.w4_linear(x.to(DEV), *w4.quantize_weight_mxfp4(W.to(DEV))).cpu()
    assert bool(torch.isnan(y[2]).all()) and bool(torch.isfinite(y[[r for r in range(Rr) if r != 2]]).all())
    x[2, 17] = 0.5
    W[3, 133] = float("inf")
    y = w4.w4_linear(x.to(DEV), *w4.quantize_weight_mxfp4(W.to(DEV))).cpu()
    assert bool(torch.isnan(y[:, 3]).all()) and bool(torch.isfinite(y[:, [c for c in range(N) if c != 3]]).all())


# ------------------------------------------------------------------------------------------------------------------ generation
def _ids(B, vocab=128, L=12):
    return torch.randint(2, vocab, (B, L), generator=torch.Generator().manual_seed(5)).to(DEV)


@pytest.mark.parametrize("mode", [dict(), dict(num_beams=2), dict(prompt_lookup_num_tokens=2, kv_cache_dtype="fp8")])
def test_generate_eager_and_graph(mode):
    small = _small()
    eager = small.generate(_ids(12), max_length=8, weight_dtype="mxfp4", **mode)
    graph = small.generate(_ids(12), max_length=8, weight_dtype="mxfp4", graph=True, **mode)
    assert torch.equal(eager, graph) and eager.shape[1] >= 2


def test_generate_decodes_the_dequantised_model(w4):
    """seed 3: the 16-bit model with the dequantised weights decides every step by a top-1 / top-2 logit gap of at least 1.0, so a
    summation-order difference cannot flip a token; the MXFP4 path must then decode that model's tokens"""
    m, _ = _decisive("t5_rpe", 3)
    ids = _ids(12, vocab=512, L=33)
    prompt = torch.tensor([[0, 5, 7 + b] for b in range(12)]).to(DEV)
    packed = m.quantize_decoder_weights_mxfp4()

    def stacks(mod):   # (the order of DecoderW8.pairs())
        blocks, head = w4._sources(mod)
        return [ws for b in blocks for ws in b] + [[head]]

    assert sum(t.numel() for pair in packed.pairs() for t in pair) == sum(w.numel() for ws in stacks(m) for w in ws) * 17 // 32
    assert "_w4_decoder" not in m.state_dict() and packed is m.quantize_decoder_weights_mxfp4()
    twin = copy.deepcopy(m)
    with torch.no_grad():
        for ws, (q4, e8) in zip(stacks(twin), packed.pairs()):
            deq = R.dequant(q4.cpu(), e8.cpu())
            assert torch.equal(deq.bfloat16().double(), deq)      # (exact in bf16)
            n = 0
            for w in ws:
                w.copy_(deq[n:n + w.shape[0]].to(DEV))
                n += w.shape[0]
    want = twin.generate(ids, max_length=6, decoder_input_ids=prompt)
    st = twin.init_decode_state(ids, max_length=6, prompt_length=3)
    gap = float("inf")
    for t in range(want.shape[1] - 1):
        top = twin.decode_step(st, want[:, t]).float().topk(2, -1).values
        if t >= 2:                                               # (the decoded steps: from the prompt's last token on)
            gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    assert gap >= 1.0, gap
    assert torch.equal(m.generate(ids, max_length=6, decoder_input_ids=prompt, weight_dtype="mxfp4"), want)
