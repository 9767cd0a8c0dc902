"""`w8_linear(kernel="matrix")` on the device (csrc/w8_mma_kernels.h): inside the bound of its summation order against fp64 at the
seams of its tiling, the bit identities of norm and residual, determinism, poison, and `generate(weight_kernel="matrix")`.
The bound (no fitted constant): exact products, at most K - 1 additions on a path, each charged 2 u, one rounding for the scale:
|y - ref| <= e + ulp_T(|ref| + e) / 2, e = gamma(2 K) * A (w8_ref.linear_ref).  Worst ratio on an MI355X: 0.994."""
import ctypes

import pytest
import torch

import w8_ref as R
from test_w8_generation_gpu import _decisive, _small
from test_w8_gpu import _problem

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def w8():
    from flasht5_amd import w8 as mod
    return mod


def _ratio(y, xin, w8_, s):
    """max |y - ref| / bound over the elements, with c = 2 K"""
    ref, A = R.linear_ref(xin, w8_, s)
    e = R.gamma(2 * xin.shape[-1]) * A
    return float(((y.double() - ref).abs() / (e + R.ulp(ref.abs() + e, y.dtype) / 2)).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [64, 128, 832, "piece + 64"])
def test_matrix_inside_the_bound(w8, dtype, K):
    assert (w8.MMA_ROW_TILE, w8.MMA_COLS, w8.MMA_K_PIECE) == (64, 32, 256)
    K = w8.MMA_K_PIECE + 64 if isinstance(K, str) else K
    rt, c = w8.MMA_ROW_TILE, w8.MMA_COLS
    worst = 0.0
    for Rr in (1, 9, 15, 16, 17, rt - 1, rt, rt + 1):
        for N in (8, 24, c - 8, c + 8):
            x, w8_, s, _, _ = _problem(Rr, K, N, dtype, seed=Rr * 131 + N)
            wide = torch.zeros(Rr, K + 24, dtype=dtype, device=DEV)   # a row stride larger than the width
            wide[:, :K] = x.to(DEV)
            y = w8.w8_linear(wide[:, :K], w8_.to(DEV), s.to(DEV), kernel="matrix").cpu()
            ratio = _ratio(y, x, w8_, s)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (Rr, K, N, ratio)
    print(f"[w8 mma] K {K} {dtype}: worst |y - ref| / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr, K, N", [(9, 832, 24), (65, 768, 40), (17, "piece + 64", 16)])
def test_fusion_is_invisible_in_the_bits(w8, dtype, Rr, K, N):
    from flasht5_amd import _lib, fast_rms_layernorm
    K = w8.MMA_K_PIECE + 64 if isinstance(K, str) else K
    x, w8_, s, gam, res = (t.to(DEV) for t in _problem(Rr, K, N, dtype, seed=11))
    plain = w8.w8_linear(x, w8_, s, kernel="matrix")
    normed = w8.w8_linear(fast_rms_layernorm(x, gam, 1e-6), w8_, s, kernel="matrix")
    assert torch.equal(w8.w8_linear(x, w8_, s, norm_weight=gam, eps=1e-6, kernel="matrix"), normed)
    assert torch.equal(w8.w8_linear(x, w8_, s, residual=res, kernel="matrix"), res + plain)
    assert torch.equal(w8.w8_linear(x, w8_, s, norm_weight=gam, eps=1e-6, residual=res, kernel="matrix"), res + normed)
    assert not torch.equal(plain, normed)
    ybuf = torch.full((Rr, N + 8), 77.0, dtype=dtype, device=DEV)
    rbuf = torch.zeros((Rr, N + 16), dtype=dtype, device=DEV)
    rbuf[:, :N] = res
    p = _lib.W8LinearParams()
    p.R, p.N, p.K, p.dtype = Rr, N, K, _lib.dtype_code(dtype)
    p.x, p.x_stride, p.w8, p.w_stride, p.scale = x.data_ptr(), K, w8_.data_ptr(), K, s.data_ptr()
    p.residual, p.residual_stride, p.y, p.y_stride = rbuf.data_ptr(), N + 16, ybuf.data_ptr(), N + 8
    _lib.check(_lib.load().fat5_w8_linear_mma(ctypes.byref(p), _lib.stream_ptr(x.device)), "fat5_w8_linear_mma")
    torch.cuda.synchronize()
    assert torch.equal(ybuf[:, :N], res + plain) and bool((ybuf[:, N:] == 77.0).all())


def test_same_bits_in_two_runs_under_a_graph_and_for_any_row_count(w8):
    x, w8_, s, gam, res = (t.to(DEV) for t in _problem(64, 768, 72, torch.bfloat16, seed=5))
    run = lambda: w8.w8_linear(x, w8_, s, norm_weight=gam, residual=res, kernel="matrix")  # noqa: E731
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
    x, w8_, s, _, _ = (t.to(DEV) for t in _problem(65, 768, 72, torch.bfloat16, seed=6))
    whole = w8.w8_linear(x, w8_, s, kernel="matrix")
    for r0 in (0, 16, 48):
        assert torch.equal(whole[r0:r0 + 16], w8.w8_linear(x[r0:r0 + 16], w8_, s, kernel="matrix"))
    for r in (0, 21, 63, 64):
        assert torch.equal(whole[r:r + 1], w8.w8_linear(x[r:r + 1], w8_, s, kernel="matrix"))


def test_poison_stays_where_it_is(w8):
    Rr, K, N = 17, 128, 24
    x, _, _, _, _ = _problem(Rr, K, N, torch.bfloat16, seed=9)
    W = (torch.randn(N, K, generator=torch.Generator().manual_seed(1)) * 0.05).bfloat16()
    x[2, 17] = float("nan")
    y = w8.w8_linear(x.to(DEV), *w8.quantize_weight(W.to(DEV)), kernel="matrix").cpu()
    assert bool(torch.isnan(y[2]).all()) and bool(torch.isfinite(y[[r for r in range(Rr) if r != 2]]).all())
    x[2, 17] = 0.5
    W[3, 5] = float("inf")
    y = w8.w8_linear(x.to(DEV), *w8.quantize_weight(W.to(DEV)), kernel="matrix").cpu()
    assert bool(torch.isnan(y[:, 3]).all()) and bool(torch.isfinite(y[:, [c for c in range(N) if c != 3]]).all())


def _ids(B, vocab=128, L=12):
    return torch.randint(2, vocab, (B, L), generator=torch.Generator().manual_seed(5)).to(DEV)


@pytest.fixture(scope="module")
def small():
    return _small()


@pytest.mark.parametrize("mode", [dict(), dict(num_beams=2), dict(prompt_lookup_num_tokens=2, kv_cache_dtype="fp8")])
def test_generate_matrix_eager_and_graph(small, mode):
    eager = small.generate(_ids(12), max_length=8, weight_dtype="fp8", weight_kernel="matrix", **mode)
    graph = small.generate(_ids(12), max_length=8, weight_dtype="fp8", weight_kernel="matrix", graph=True, **mode)
    assert torch.equal(eager, graph) and eager.shape[1] >= 2
    if not mode:
        rows = small.generate(_ids(12), max_length=8, weight_dtype="fp8", weight_kernel="rows")
        assert torch.equal(rows, small.generate(_ids(12), max_length=8, weight_dtype="fp8", weight_kernel=None))


def test_prompt_in_one_chunk_equals_token_by_token():
    from flasht5_amd.generation import finish_labels
    m, _ = _decisive("t5_rpe", 3)
    ids = _ids(12, vocab=512, L=33)
    prompt = torch.tensor([[0, 5, 7 + b] for b in range(12)]).to(DEV)
    kw = dict(weight_dtype="fp8", weight_kernel="matrix")
    out = m.generate(ids, max_length=6, decoder_input_ids=prompt, **kw)      # (the prefill chunk: 24 rows)
    st = m.init_decode_state(ids, max_length=6, prompt_length=3, **kw)
    assert st.w8_kernel == "matrix"
    for t in range(2):
        m.decode_step(st, prompt[:, t])
    tok, want = prompt[:, 2], [prompt]
    for _ in range(out.shape[1] - 3):
        tok = m.decode_step(st, tok).argmax(-1)
        want.append(tok.unsqueeze(1))
    assert torch.equal(out, finish_labels(torch.cat(want, 1)))


def test_the_row_count_chooses_the_kernel(small, w8, monkeypatch):
    kernels, real = [], w8.w8_linear
    monkeypatch.setattr(w8, "w8_linear", lambda *a, **k: (kernels.append(k.get("kernel", "rows")), real(*a, **k))[1])
    small.generate(_ids(4), max_length=3, weight_dtype="fp8", weight_kernel="matrix")
    assert kernels and set(kernels) == {"rows"}
    del kernels[:]
    small.generate(_ids(12), max_length=3, weight_dtype="fp8", weight_kernel="matrix")
    assert kernels and set(kernels) == {"matrix"}
