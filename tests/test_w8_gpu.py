"""FP8 weights on the device: the quantiser's bytes and scales against the restatement, `w8_linear` inside the derived per-element
bound (tests/w8_ref.py) at every boundary of the kernel's tiling, the two bit identities that make the fusion invisible,
determinism (two runs, graph replay) and poisoned inputs."""
import ctypes

import pytest
import torch

import w8_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def w8():
    from flasht5_amd import w8 as mod
    return mod


# ------------------------------------------------------------------------------------------------------------------ quantiser
def _every_tie():
    """the midpoints of adjacent e4m3fn values, both signs: 5 significant bits each, exact in bf16, fp16 and fp32"""
    vals = torch.arange(0, 0x7F, dtype=torch.uint8).view(R.FP8).float()     # 0 .. 448, ascending
    mid = (vals[:-1] + vals[1:]) / 2
    return torch.cat([mid, -mid])


def _special_weight(N, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 3
    ties = _every_tie()
    per_row = min(K - 1, 63)
    rows = -(-ties.numel() // per_row)
    assert rows <= 4 and N >= 8
    for r in range(rows):                 # rows 0 .. 3: amax 448 (s = 1) and the ties behind it
        chunk = ties[r * per_row:(r + 1) * per_row]
        W[r] = 0
        W[r, 0] = 448.0
        W[r, 1:1 + chunk.numel()] = chunk
    W[4] = 0                              # a zero row: s = 1
    W[5] = 0
    W[5, K - 1] = -7.0                    # one element at -amax
    W = W.to(dtype)
    W[6, 3] = float("inf")                # non-finite rows: s = +inf
    W[7, K // 2] = float("nan")
    return W


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("N, K", [(8, 64), (72, 64), (8, 832), (72, 832)])
def test_quantiser_bits(w8, dtype, N, K):
    W = _special_weight(N, K, dtype)
    want8, wants = R.quantize_ref(W)
    if K == 64 and N == 8:   # (the restatement itself on the tie rows: every tie went to the even byte)
        b = want8[:4].view(torch.uint8)
        assert float(wants[0]) == 1.0 and int(b[0, 0]) == 0x7E
    out = torch.full((N + 2, K), 0x55, dtype=torch.uint8, device=DEV).view(R.FP8)
    scale = torch.full((N + 2,), -3.0, dtype=torch.float32, device=DEV)
    got8, gots = w8.quantize_weight(W.to(DEV), out[1:N + 1], scale[1:N + 1])
    assert R.same_bits(got8.cpu(), gots.cpu(), want8, wants)
    guard = out.view(torch.uint8)
    assert bool((guard[0] == 0x55).all()) and bool((guard[N + 1] == 0x55).all())
    assert float(scale[0]) == -3.0 and float(scale[N + 1]) == -3.0
    # without destinations: new tensors, the same bits; and a weight whose rows are strided
    b2, s2 = w8.quantize_weight(W.to(DEV))
    assert R.same_bits(b2.cpu(), s2.cpu(), want8, wants)
    wide = torch.zeros(N, K + 64, dtype=dtype, device=DEV)
    wide[:, :K] = W.to(DEV)
    b3, s3 = w8.quantize_weight(wide[:, :K])
    assert R.same_bits(b3.cpu(), s3.cpu(), want8, wants)


# ------------------------------------------------------------------------------------------------- linear inside the bound
def _problem(Rr, K, N, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Rr, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    gam = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    res = torch.randn(Rr, N, generator=g).to(dtype)
    w8_, s = R.quantize_ref(W)
    return x, w8_, s, gam, res


def _row_counts(w8):
    rt = w8.ROW_TILE
    return [1, rt - 1, rt, rt + 1, 64, 65]


def _column_counts(w8):
    c = w8.COLS_PER_BLOCK
    return sorted({8, c - 8, c + 8})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [64, 128, 832, 2048])
def test_linear_inside_the_bound(w8, dtype, K):
    assert (w8.ROW_TILE, w8.COLS_PER_BLOCK, w8.K_TILE, w8.LANE_K) == (8, 16, 2048, R.LANE_K)
    for Rr in _row_counts(w8) + [2, 3]:        # (2 and 3: the short row tiles of 2 and 4 rows)
        for N in _column_counts(w8):
            x, w8_, s, _, _ = _problem(Rr, K, N, dtype, seed=Rr * 131 + N)
            wide = torch.zeros(Rr, K + 24, dtype=dtype, device=DEV)   # a row stride larger than the width
            wide[:, :K] = x.to(DEV)
            y = w8.w8_linear(wide[:, :K], w8_.to(DEV), s.to(DEV)).cpu()
            assert y.shape == (Rr, N) and y.dtype == dtype
            print(f"R {Rr} K {K} N {N} {dtype}: worst |y - ref| / bound {R.worst(y, x, w8_, s):.3f}")
            assert R.accepts(y, x, w8_, s), (Rr, K, N)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_with_norm_inside_the_bound_from_the_kernel_xin(w8, dtype):
    from flasht5_amd import fast_rms_layernorm
    for Rr, K, N in ((9, 832, 24), (3, 4160, 8)):     # (4160: three K tiles, the last one short)
        x, w8_, s, gam, _ = _problem(Rr, K, N, dtype, seed=7)
        xin = fast_rms_layernorm(x.to(DEV), gam.to(DEV), 1e-6).cpu()
        y = w8.w8_linear(x.to(DEV), w8_.to(DEV), s.to(DEV), norm_weight=gam.to(DEV), eps=1e-6).cpu()
        print(f"norm R {Rr} K {K} N {N} {dtype}: worst {R.worst(y, xin, w8_, s):.3f}")
        assert R.accepts(y, xin, w8_, s)


def test_strided_y_through_the_c_abi(w8):
    """y (and the residual) with a row stride larger than N: the Python operator allocates y itself, so this goes through the ABI"""
    from flasht5_amd import _lib
    Rr, K, N, dtype = 9, 128, 24, torch.bfloat16
    x, w8_, s, _, res = _problem(Rr, K, N, dtype, seed=3)
    xd, wd, sd = x.to(DEV), w8_.to(DEV), s.to(DEV)
    ybuf = torch.full((Rr, N + 8), 77.0, dtype=dtype, device=DEV)
    rbuf = torch.zeros((Rr, N + 16), dtype=dtype, device=DEV)
    rbuf[:, :N] = res.to(DEV)
    p = _lib.W8LinearParams()
    p.R, p.N, p.K, p.dtype = Rr, N, K, _lib.FAT5_BF16
    p.x, p.x_stride, p.w8, p.w_stride, p.scale = xd.data_ptr(), K, wd.data_ptr(), K, sd.data_ptr()
    p.residual, p.residual_stride, p.y, p.y_stride = rbuf.data_ptr(), N + 16, ybuf.data_ptr(), N + 8
    _lib.check(_lib.load().fat5_w8_linear(ctypes.byref(p), _lib.stream_ptr(xd.device)), "fat5_w8_linear")
    torch.cuda.synchronize()
    want = w8.w8_linear(xd, wd, sd, residual=res.to(DEV))
    assert torch.equal(ybuf[:, :N], want) and bool((ybuf[:, N:] == 77.0).all())


# ------------------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Rr, K, N", [(1, 64, 8), (9, 832, 24), (65, 768, 40), (5, 2112, 16)])
def test_fusion_is_invisible_in_the_bits(w8, dtype, Rr, K, N):
    from flasht5_amd import fast_rms_layernorm
    x, w8_, s, gam, res = (t.to(DEV) for t in _problem(Rr, K, N, dtype, seed=11))
    plain = w8.w8_linear(x, w8_, s)
    xin = fast_rms_layernorm(x, gam, 1e-6)
    normed = w8.w8_linear(xin, w8_, s)
    assert torch.equal(w8.w8_linear(x, w8_, s, norm_weight=gam, eps=1e-6), normed)                    # NORM = norm, then plain
    assert torch.equal(w8.w8_linear(x, w8_, s, residual=res), res + plain)                           # RES = plain, then add
    assert torch.equal(w8.w8_linear(x, w8_, s, norm_weight=gam, eps=1e-6, residual=res), res + normed)  # both
    assert not torch.equal(plain, normed)
    # leading dimensions are only a view
    x3 = x.view(1, Rr, K)
    assert torch.equal(w8.w8_linear(x3, w8_, s, residual=res.view(1, Rr, N)), (res + plain).view(1, Rr, N))


# --------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_and_a_graph_replay_give_the_same_bits(w8):
    x, w8_, s, gam, res = (t.to(DEV) for t in _problem(64, 768, 72, torch.bfloat16, seed=5))
    a = w8.w8_linear(x, w8_, s, norm_weight=gam, residual=res)
    b = w8.w8_linear(x, w8_, s, norm_weight=gam, residual=res)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = w8.w8_linear(x, w8_, s, norm_weight=gam, residual=res)
    c.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c)
    x.mul_(2)     # the replay reads the buffers, not a snapshot
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(c, w8.w8_linear(x, w8_, s, norm_weight=gam, residual=res))


# ------------------------------------------------------------------------------------------------------------ poisoned input
def test_poison_stays_where_it_is(w8):
    Rr, K, N, dtype = 9, 128, 24, torch.bfloat16
    x, _, _, gam, _ = _problem(Rr, K, N, dtype, seed=9)
    g = torch.Generator().manual_seed(1)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    x[2, 17] = float("nan")
    y = w8.w8_linear(x.to(DEV), *w8.quantize_weight(W.to(DEV))).cpu()
    assert bool(torch.isnan(y[2]).all()) and bool(torch.isfinite(y[[0, 1, 3, 4, 5, 6, 7, 8]]).all())
    yn = w8.w8_linear(x.to(DEV), *w8.quantize_weight(W.to(DEV)), norm_weight=gam.to(DEV)).cpu()
    assert bool(torch.isnan(yn[2]).all()) and bool(torch.isfinite(yn[[0, 1, 3, 4, 5, 6, 7, 8]]).all())
    x[2, 17] = 0.5
    W[3, 5] = float("inf")
    W[20, 0] = float("nan")
    b, s = w8.quantize_weight(W.to(DEV))
    assert bool(torch.isinf(s[[3, 20]]).all())
    y = w8.w8_linear(x.to(DEV), b, s).cpu()
    cols = [c for c in range(N) if c not in (3, 20)]
    assert bool(torch.isnan(y[:, [3, 20]]).all()) and bool(torch.isfinite(y[:, cols]).all())


def test_no_rows_no_launch(w8):
    w8_, s = w8.quantize_weight(torch.randn(8, 64, device=DEV))
    y = w8.w8_linear(torch.empty(0, 64, dtype=torch.bfloat16, device=DEV), w8_, s)
    assert y.shape == (0, 8)
    y = w8.w8_linear(torch.empty(2, 0, 64, dtype=torch.bfloat16, device=DEV), w8_, s)
    assert y.shape == (2, 0, 8)
