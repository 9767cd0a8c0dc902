"""Every launch path of the row-wise kernels (csrc/rowwise_kernels.h, csrc/fold_weights.h; host dispatch in csrc/api_rowwise.hip)
against the fp64 restatements of tests/rowwise_fp64.py, on both sides of each dispatch predicate.  Each case names the kernel
instance it targets.  The module-level wrappers are called directly (rms_norm.rmsnorm_fwd, fused_linear.fold_weights, ...) so
that strided views reach the kernels as they are; a misaligned base, which every wrapper would copy, goes through the C ABI.

Bounds (u = 2^-24, the fp32 unit roundoff; ulp_T(r) = the spacing of dtype T at |r|).  None is a flat tolerance:
  * Rounded once from fp32 math (y, h, xhat, gated outputs, folded weights): |got - ref| <= ulp_T(ref) / 2 + k u |ref|, k the
    number of fp32 roundings before the store (<= 1 ulp_T for 16-bit outputs).  h = x + r, fold_weights and the dW_i of
    fold_weights_bwd are one sum / product of two 16-bit values, exact in fp32: they must equal the fp64 result rounded once, bit
    for bit.
  * RMSNorm rstd: the sum of n squares runs ceil(n / 64) deep per lane, then 6 wave levels: depth D = ceil(n / 64) + 6, and
    |rstd - ref| <= (D / 2 + 4) u rstd (half the relative error of the sum, plus the divide, the add, the sqrt and the reciprocal).
    y carries that on top of its own k = 2 roundings.
  * RMSNorm dx (the kernel's rstd as input): ulp_T(ref) / 2 + (D + 6) u T with the term magnitude
    T = (|w dy| + |xhat| mean|xhat w dy|) rstd; with dres the normalised part is rounded to T first (what autograd's sum of the two
    branch gradients computes): + ulp_T(dx_norm) / 2.  The unit-weight backward adds dres in fp32 before its one rounding.
  * dw and dg (column sums): ulp_W(ref) / 2 + c u sum_rows |dy xhat|, c the depth of the summation tree: rows per wave + 8 waves +
    the reduce kernel's 16 + 2 rounds + 16 groups (vector backward), rows per workgroup (scalar backward: LDS atomics in any
    order) + 8; dg: rows per slab / 32 + 32 LDS rows + the slabs + 1.
  * Gated GELU: u(x) = k x (1 + c x^2) is formed with 5 roundings, e^(-2u) by exp2 and the reciprocal by rcp (1 ulp each), so
    sigmoid(2u) is off by at most (10 |u| (1 - s) + 3) u relative; the output by (10 |u| (1 - s) + 8) u |ref| (+ ulp/2), the
    derivative by that much of its term magnitude |s| + |x s (1 - s) 2k (1 + 3c x^2)|.  The kernel clamps u at -40
    (x < -9.65): there the true s is below e^-80 and the kernel's is e^-80, so an absolute floor 2 e^-80 |x h1| (derivative:
    2 e^-80 (1 + 2k|x| (1 + 3c x^2)) |dout h1|) is added -- 1e-34 relative to the inputs, and nowhere else does it matter.
  * Cross-entropy: the per-thread online sum of exponentials runs D = VEC + chunks + 12 deep (scalar path: ceil(V / 256) + 12),
    so lse is within (D + 4) u T_lse, T_lse = 1 + |lse| + sum_j p_j |x_j| (the rounding of each scaled logit moves its
    exponential by u |x_j|).  loss and z carry that plus 4 u of their own terms (|lse|, |x_label|, smoothing mean|x|, |z|);
    dlogits = g (p zf - onehot - s/V) carries, per element, u |g| (p zf ((D + 6) T_lse + 2|x| + 2|lse| + 6) + 2 (1 + s/V)).
  * Determinism: the vector RMSNorm backward and the CE kernels give the same bits on a second run.  The scalar RMSNorm backward
    accumulates dw with LDS atomics in whatever order the waves arrive, and is exempt.
  * The 65535-row grid split of the gated activation: the rows around each split and the last rows are checked against fp64;
    the rest bit for bit against a launch on the row slice [65535:] (a row's result does not depend on its neighbours).
"""
import importlib
import math
import zlib

import pytest
import torch

import rowwise_fp64 as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
VEC = {F32: 4, F16: 8, BF16: 8}
PAIRS = [(x, w) for x in DTYPES for w in DTYPES]


def _name(d):
    return str(d)[6:]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(shape, dtype, g, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).cuda()


def _check(got, ref, bound, what):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} out of bound; first at flat {i}: got {got.flatten()[i].item()!r} "
                             f"ref {ref.flatten()[i].item()!r} bound {bound.flatten()[i].item():.3e}")


def _once(ref, dtype, k):
    """one rounding to `dtype` after k fp32 roundings"""
    return 0.5 * R.ulp(ref, dtype) + k * U * ref.abs()


def _exact(got, ref, what):
    want = ref.to(got.dtype)
    assert torch.equal(got.cpu(), want), f"{what}: {int((got.cpu() != want).sum())} elements differ from the fp64 result rounded once"


def _lib():
    from flasht5_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------------------
# RMSNorm forward / backward
# ------------------------------------------------------------------------------------------------------------------------------
def _depth(n):
    return math.ceil(n / 64) + 6


def _check_fwd(y, rstd, x, w, eps, what):
    y_ref, r_ref = R.rmsnorm_fwd(x, w, eps)
    d = _depth(x.shape[-1])
    _check(rstd, r_ref, (d / 2 + 4) * U * r_ref, f"{what} rstd")
    _check(y, y_ref, _once(y_ref, x.dtype, 2 + d / 2 + 4), f"{what} y")


def _bwd_blocks(rows):
    return min(512, (rows + 15) // 16)


def _check_bwd(dx, dw, dy, x, w, rstd, what, vector, dres=None):
    rows, n = x.shape
    dx_ref, dw_ref = R.rmsnorm_bwd(dy, x, w, rstd)
    xd, dyd, wd, r = x.double().cpu(), dy.double().cpu(), w.double().cpu(), rstd.double().cpu().unsqueeze(-1)
    xhat = xd * r
    T = ((wd * dyd).abs() + xhat.abs() * (xhat * wd * dyd).abs().mean(-1, keepdim=True)) * r
    bound = 0.5 * R.ulp(dx_ref, x.dtype) + (_depth(n) + 6) * U * T
    if dres is not None:
        bound = bound + 0.5 * R.ulp(dx_ref + dres.double().cpu(), x.dtype)
        dx_ref = dx_ref + dres.double().cpu()
    _check(dx, dx_ref, bound, f"{what} dx")
    blocks = _bwd_blocks(rows)
    c = (math.ceil(rows / (8 * blocks)) + 8 + 16 + 2 + 16) if vector else (math.ceil(rows / blocks) + 8)
    _check(dw, dw_ref, 0.5 * R.ulp(dw_ref, w.dtype) + c * U * (dyd * xhat).abs().sum(0), f"{what} dw")


def _rows_vec(n, dtype, *ts):
    """the 16-byte-row part of the host's `vecok` (fat5_rmsnorm_fwd and its siblings, api_rowwise.hip): n a multiple of 8, row strides of VEC, 16-byte aligned bases
    (the outputs and w the wrappers allocate or make contiguous are aligned)"""
    return n % 8 == 0 and all(t.stride(0) % VEC[dtype] == 0 and t.data_ptr() % 16 == 0 for t in ts)


def _fwd_bwd(x, w, dy, eps, what, vector, deterministic=False):
    from flasht5_amd import rms_norm
    n = x.shape[-1]
    assert vector == (_rows_vec(n, x.dtype, x, dy) and n <= 16 * 64 * VEC[x.dtype]), f"{what}: the case does not reach the kernel it names"
    y, rstd = rms_norm.rmsnorm_fwd(x, w, eps)
    _check_fwd(y, rstd, x, w, eps, what)
    dx, dw = rms_norm.rmsnorm_bwd(dy, x, w, rstd, eps)
    _check_bwd(dx, dw, dy, x, w, rstd, what, vector)
    if deterministic:
        dx2, dw2 = rms_norm.rmsnorm_bwd(dy, x, w, rstd, eps)
        assert torch.equal(dx, dx2) and torch.equal(dw, dw2), f"{what}: the vector backward is not deterministic"


# (x dtype, n, vector): rmsnorm_bwd_kernel<X, W, NCH> for NCH = 2 / 4 / 8 / 16 at both ends of each range, then
# rmsnorm_bwd_scalar_kernel past the vector limit (16-bit n > 8192, fp32 n > 4096), at 48 KB of dynamic LDS (n = 12288) and
# above it (12296, 16384: the hipFuncSetAttribute launch)
NCH_CASES = [
    (BF16, 1024, True), (BF16, 1032, True), (BF16, 2048, True), (F16, 2056, True), (BF16, 4096, True),  # NCH 2, 4, 4, 8, 8
    (BF16, 4104, True), (F16, 8192, True), (BF16, 7688, True),                                           # NCH 16
    (BF16, 8200, False), (F16, 12288, False), (BF16, 12296, False), (BF16, 16384, False),                # scalar
    (F32, 512, True), (F32, 1024, True), (F32, 2048, True), (F32, 4096, True),                           # fp32 NCH 2, 4, 8, 16
    (F32, 4104, False), (F32, 12296, False),                                                             # fp32 scalar
]


@pytest.mark.parametrize("dtype,n,vector", NCH_CASES, ids=[f"{_name(d)}-{n}" for d, n, _ in NCH_CASES])
def test_rmsnorm_widths(dtype, n, vector):
    """rmsnorm_fwd_kernel<X, X, true>, then rmsnorm_bwd_kernel<X, X, NCH> / rmsnorm_bwd_scalar_kernel<X, X> per NCH_CASES"""
    g = _gen("w", dtype, n)
    rows = 40
    x, dy = _randn((rows, n), dtype, g), _randn((rows, n), dtype, g)
    w = _randn((n,), dtype, g, 0.1, 1.0)
    _fwd_bwd(x, w, dy, 1e-6, f"{_name(dtype)} n={n}", vector, deterministic=vector)


@pytest.mark.parametrize("rows", [4096, 4097, 8192, 9000])
def test_rmsnorm_dw_reduce_rounds(rows):
    """rmsnorm_dw_reduce_kernel<BF16> over 256 partial rows (4096 rows), 257 (the second p0 += 256 round), 512 (two full rounds) and
    512 at the workgroup cap (9000 rows: several rows per wave); rmsnorm_bwd_kernel<BF16, F32, 2>"""
    g = _gen("rows", rows)
    n = 256
    x, dy = _randn((rows, n), BF16, g), _randn((rows, n), BF16, g)
    w = _randn((n,), F32, g, 0.1, 1.0)
    _fwd_bwd(x, w, dy, 1e-6, f"rows={rows}", True, deterministic=True)


@pytest.mark.parametrize("xdt,wdt", PAIRS, ids=[f"x{_name(a)}-w{_name(b)}" for a, b in PAIRS])
@pytest.mark.parametrize("n", [1024, 1004])
def test_rmsnorm_dtype_pairs(xdt, wdt, n):
    """every (x, w) dtype pair: n = 1024 -> rmsnorm_fwd_kernel<X, W, true> + rmsnorm_bwd_kernel<X, W, 2 or 4> (load_w's three weight
    forms); n = 1004 (not a multiple of 8) -> rmsnorm_fwd_kernel<X, W, false> + rmsnorm_bwd_scalar_kernel<X, W>"""
    g = _gen("pair", xdt, wdt, n)
    x, dy = _randn((48, n), xdt, g, 2.0), _randn((48, n), xdt, g)
    w = _randn((n,), wdt, g, 0.3, 1.0)
    _fwd_bwd(x, w, dy, 1e-5, f"x {_name(xdt)} w {_name(wdt)} n={n}", n % 8 == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad,vector", [(8, True), (1, False)])
def test_rmsnorm_row_stride(dtype, pad, vector):
    """row stride n + 8 (a multiple of VEC): rmsnorm_fwd_kernel<X, X, true> / rmsnorm_bwd_kernel<X, X, 4 (16-bit) or 8 (fp32)> read the strided rows as
    they are; n + 1: rmsnorm_fwd_kernel<X, X, false> / rmsnorm_bwd_scalar_kernel<X, X> (the stride is not a multiple of VEC)"""
    g = _gen("stride", dtype, pad)
    rows, n = 33, 1536
    xb, db = _randn((rows, n + pad), dtype, g), _randn((rows, n + pad), dtype, g)
    x, dy = xb[:, :n], db[:, :n]
    w = _randn((n,), dtype, g, 0.1, 1.0)
    assert x.stride(0) == n + pad and x.data_ptr() % 16 == 0
    _fwd_bwd(x, w, dy, 1e-6, f"{_name(dtype)} stride {n + pad}", vector)


@pytest.mark.parametrize("xdt,wdt", PAIRS, ids=[f"x{_name(a)}-w{_name(b)}" for a, b in PAIRS])
def test_rmsnorm_misaligned_base(xdt, wdt):
    """a base 2 or 4 bytes off 16-byte alignment with n a multiple of 8 (the wrappers would copy such a tensor, so the C ABI is
    called directly): rmsnorm_fwd_kernel<X, W, false> and rmsnorm_bwd_scalar_kernel<X, W> reached by the alignment alone"""
    dtype = xdt
    L = _lib()
    lib = L.load()
    g = _gen("mis", dtype, wdt)
    rows, n = 24, 2048
    xb, db = _randn((rows * n + 8,), dtype, g), _randn((rows * n + 8,), dtype, g)
    x, dy = xb[1:1 + rows * n].view(rows, n), db[1:1 + rows * n].view(rows, n)
    assert x.data_ptr() % 16 != 0
    w = _randn((n,), wdt, g, 0.1, 1.0)
    y = torch.empty((rows, n), dtype=dtype, device="cuda")
    rstd = torch.empty((rows,), dtype=torch.float32, device="cuda")
    dev = x.device
    L.check(lib.fat5_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, n, n, n, 1e-6, L.dtype_code(dtype),
                                 L.dtype_code(wdt), L.stream_ptr(dev)), "fat5_rmsnorm_fwd")
    _check_fwd(y, rstd, x, w, 1e-6, f"misaligned x {_name(dtype)} w {_name(wdt)}")
    dx = torch.empty((rows, n), dtype=dtype, device="cuda")
    dw = torch.empty((n,), dtype=wdt, device="cuda")
    ws = torch.empty(lib.fat5_rmsnorm_bwd_workspace_bytes(rows, n), dtype=torch.uint8, device="cuda")
    L.check(lib.fat5_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dw.data_ptr(), rows, n, n, n, n,
                                 L.dtype_code(dtype), L.dtype_code(wdt), ws.data_ptr(), ws.numel(), L.stream_ptr(dev)), "fat5_rmsnorm_bwd")
    _check_bwd(dx, dw, dy, x, w, rstd, f"misaligned x {_name(dtype)} w {_name(wdt)}", False)


# ------------------------------------------------------------------------------------------------------------------------------
# residual add + RMSNorm
# ------------------------------------------------------------------------------------------------------------------------------
def _add_norm(x, r, w, eps, what, dres=True, vector=True):
    from flasht5_amd import rms_norm
    h, y, rstd = rms_norm.add_rmsnorm_fwd(x, r, w, eps)
    _exact(h, x.double().cpu() + r.double().cpu(), f"{what} h")
    _check_fwd(y, rstd, h, w, eps, what)
    g = _gen("addbwd", what)
    dy = _randn(x.shape, x.dtype, g)
    dr = _randn(x.shape, x.dtype, g) if dres else h
    n = x.shape[-1]
    assert vector == (_rows_vec(n, x.dtype, h, dy, dr) and n <= 16 * 64 * VEC[x.dtype]), f"{what}: the case does not reach the kernel it names"
    dx, dw = rms_norm.add_rmsnorm_bwd(dy, h, w, rstd, dr, dres)
    _check_bwd(dx, dw, dy, h, w, rstd, f"{what} (add+norm bwd)", vector, dr if dres else None)


# (x dtype, n): add_rmsnorm_fwd_reg_kernel<X, W, 2> (n <= 2 * 64 * VEC), <X, W, 4> (<= 4 * 64 * VEC), add_rmsnorm_fwd_kernel<X, W, true>
# above that (16-bit n > 2048, fp32 n > 1024), add_rmsnorm_fwd_kernel<X, W, false> for n not a multiple of 8
ADD_CASES = [(BF16, 1024, "reg2"), (F16, 2048, "reg4"), (BF16, 2056, "vector"), (BF16, 8192, "vector"), (F16, 1004, "scalar"), (BF16, 1004, "scalar"),
             (F32, 512, "reg2"), (F32, 1024, "reg4"), (F32, 1032, "vector"), (F32, 4100, "scalar")]


@pytest.mark.parametrize("dtype,n,kind", ADD_CASES, ids=[f"{_name(d)}-{n}-{k}" for d, n, k in ADD_CASES])
def test_add_rmsnorm_kernels(dtype, n, kind):
    g = _gen("add", dtype, n)
    x, r = _randn((40, n), dtype, g, 1.5), _randn((40, n), dtype, g)
    nch = math.ceil(n / (64 * VEC[dtype]))
    assert kind == ("scalar" if not _rows_vec(n, dtype, x, r) else "reg2" if nch <= 2 else "reg4" if nch <= 4 else "vector")
    w = _randn((n,), dtype, g, 0.1, 1.0)
    _add_norm(x, r, w, 1e-6, f"{kind} {_name(dtype)} n={n}", dres=kind != "reg4", vector=kind != "scalar" and n <= 16 * 64 * VEC[dtype])


@pytest.mark.parametrize("xdt,wdt", PAIRS, ids=[f"x{_name(a)}-w{_name(b)}" for a, b in PAIRS])
@pytest.mark.parametrize("n", [1024, 4096, 1004])
def test_add_rmsnorm_dtype_pairs(xdt, wdt, n):
    """every (x, w) pair on the register kernel (n = 1024: add_rmsnorm_fwd_reg_kernel<X, W, 2 or 4>), the re-reading vector kernel
    (n = 4096: add_rmsnorm_fwd_kernel<X, W, true>) and the scalar one (n = 1004, not a multiple of 8: add_rmsnorm_fwd_kernel<X, W,
    false>); backward with dres: rmsnorm_bwd_kernel<X, W, NCH>, or rmsnorm_bwd_scalar_kernel<X, W> at n = 1004"""
    g = _gen("addpair", xdt, wdt, n)
    x, r = _randn((32, n), xdt, g, 1.5), _randn((32, n), xdt, g)
    w = _randn((n,), wdt, g, 0.3, 1.0)
    _add_norm(x, r, w, 1e-6, f"x {_name(xdt)} w {_name(wdt)} n={n}", vector=n % 8 == 0)


def test_add_rmsnorm_strided_rows():
    """row strides n + 8 on x and r: add_rmsnorm_fwd_kernel<BF16, BF16, true> at n = 3072 reads strided rows; the backward
    (rmsnorm_bwd_kernel<BF16, BF16, 8>) reads the contiguous h and dy -- strided backward rows: test_rmsnorm_row_stride"""
    g = _gen("addstride")
    n = 3072
    x = _randn((24, n + 8), BF16, g)[:, 8:]
    r = _randn((24, n + 8), BF16, g)[:, :n]
    w = _randn((n,), BF16, g, 0.1, 1.0)
    _add_norm(x, r, w, 1e-6, "strided add+norm")


# ------------------------------------------------------------------------------------------------------------------------------
# unit-weight norm backward, fold_weights
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [(BF16, 1024), (F16, 2048), (BF16, 520), (F32, 512), (F32, 1024)])
@pytest.mark.parametrize("dres", [False, True])
def test_unit_rmsnorm_bwd(dtype, n, dres):
    """rmsnorm_unit_bwd_kernel<X, 2> (n <= 2 * 64 * VEC) and <X, 4>, with and without the residual gradient"""
    from flasht5_amd import fused_linear
    g = _gen("unit", dtype, n, dres)
    x, gy = _randn((40, n), dtype, g, 2.0), _randn((40, n), dtype, g)
    rstd = R.rmsnorm_fwd(x, torch.ones(n), 1e-6)[1].float().cuda()
    dr = _randn((40, n), dtype, g) if dres else None
    dx, xhat = fused_linear.rmsnorm_unit_bwd_op(gy, x, rstd, dr)
    dx_ref, xh_ref = R.unit_rmsnorm_bwd(gy, x, rstd, dr)
    _check(xhat, xh_ref, _once(xh_ref, dtype, 1), "xhat")
    xh, gyd = xh_ref, gy.double().cpu()
    T = (gyd.abs() + xh.abs() * (xh * gyd).abs().mean(-1, keepdim=True)) * rstd.double().cpu().unsqueeze(-1)
    if dres:
        T = T + dr.double().cpu().abs()
    _check(dx, dx_ref, 0.5 * R.ulp(dx_ref, dtype) + (_depth(n) + 6) * U * T, "dx")


# (stacked row counts, K): the slab count of fold_weights_bwd_kernel is ceil(N / rows_per), rows_per = max(64, ceil(N / 64) rounded up
# to 32): one slab (N = 64), two (96), 64 slabs of 64 (N = 4096), 44 of 96 (4160), 64 of 96 (6144: N > 4096)
FOLD_CASES = [((64,), 128), ((32, 64), 64), ((2048, 1024, 1024), 128), ((4160,), 64), ((2048, 2048, 2048), 64), ((8, 16, 40), 192)]


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("ns,K", FOLD_CASES, ids=[f"{'+'.join(map(str, ns))}x{k}" for ns, k in FOLD_CASES])
def test_fold_weights(dtype, ns, K):
    """fold_weights_kernel<BF16?> with 1, 2 or 3 stacked weights, with and without the norm weight, one of them row-strided; then
    fold_weights_bwd_kernel<BF16?> (dW_i bit for bit) + fold_weights_dg_kernel<BF16?> over the slab counts of FOLD_CASES"""
    from flasht5_amd import fused_linear
    g = _gen("fold", dtype, ns, K)
    ws = [_randn((n, K), dtype, g, 0.05) for n in ns]
    ws[-1] = torch.cat([ws[-1], ws[-1][:, :8]], 1)[:, :K] if len(ns) > 1 else ws[-1]  # (row stride K + 8 on the last of a stack)
    if len(ns) > 1:
        assert ws[-1].stride(0) == K + 8
    gw = _randn((K,), dtype, g, 0.2, 1.0)
    _exact(fused_linear.fold_weights(ws, None), R.fold_weights(ws), "fold_weights stack")
    _exact(fused_linear.fold_weights(ws, gw), R.fold_weights(ws, gw), "fold_weights diag(g)")
    N = sum(ns)
    dwg = _randn((N, K), dtype, g, 3.0)
    *dws, dg = fused_linear.fold_weights_bwd_op(dwg, ws, gw)
    dws_ref, dg_ref = R.fold_weights_bwd(dwg, ws, gw)
    for i, (a, b) in enumerate(zip(dws, dws_ref)):
        _exact(a, b, f"dW_{i}")
    rp = max(64, ((N + 63) // 64 + 31) // 32 * 32)
    c = rp // 32 + 32 + math.ceil(N / rp) + 1
    T = (dwg.double().cpu() * R.fold_weights(ws)).abs().sum(0)
    _check(dg, dg_ref, 0.5 * R.ulp(dg_ref, dtype) + c * U * T, "dg")


# ------------------------------------------------------------------------------------------------------------------------------
# gated activation
# ------------------------------------------------------------------------------------------------------------------------------
ACT = {"gelu_tanh": 0, "relu": 1}
TAIL = 2 * math.exp(-80)


def _gelu_terms(x):
    u = R.GELU_K * x * (1 + R.GELU_C * x * x)
    s = torch.sigmoid(2 * u)
    return u, s


def _gated_bounds(h0, h1, dout, act, dtype, out_ref, d0_ref, d1_ref):
    x, b = h0.double().cpu(), h1.double().cpu()
    gd = dout.double().cpu() if dout is not None else None
    if act == "relu":
        return (_once(out_ref, dtype, 1), None if gd is None else _once(d0_ref, dtype, 2), None if gd is None else _once(d1_ref, dtype, 1))
    u, s = _gelu_terms(x)
    rel = (10 * u.abs() * (1 - s) + 8) * U
    b_out = 0.5 * R.ulp(out_ref, dtype) + rel * out_ref.abs() + TAIL * (x * b).abs()
    if gd is None:
        return b_out, None, None
    da_T = s + (x * s * (1 - s) * 2 * R.GELU_K * (1 + 3 * R.GELU_C * x * x)).abs()
    b0 = (0.5 * R.ulp(d0_ref, dtype) + (rel + 6 * U) * (gd * b).abs() * da_T +
          TAIL * (gd * b).abs() * (1 + 2 * R.GELU_K * x.abs() * (1 + 3 * R.GELU_C * x * x)))
    b1 = 0.5 * R.ulp(d1_ref, dtype) + (rel + U) * (gd * R.gated_act_fwd(h0, torch.ones_like(h0), act)).abs() + TAIL * (gd * x).abs()
    return b_out, b0, b1


def _gated_check(h0, h1, dout, act, out, dh, rows, what):
    F = h0.shape[-1]
    dtype = h0.dtype
    out_ref = R.gated_act_fwd(h0[rows], h1[rows], act)
    d0_ref, d1_ref = R.gated_act_bwd(dout[rows], h0[rows], h1[rows], act)
    bo, b0, b1 = _gated_bounds(h0[rows], h1[rows], dout[rows], act, dtype, out_ref, d0_ref, d1_ref)
    _check(out[rows], out_ref, bo, f"{what} out")
    _check(dh[rows][:, :F], d0_ref, b0, f"{what} dh0")
    _check(dh[rows][:, F:], d1_ref, b1, f"{what} dh1")


@pytest.mark.parametrize("act", ["gelu_tanh", "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gated_act_range(act, dtype):
    """gated_act_fwd_kernel<X, ACT> / gated_act_bwd_kernel<X, ACT> on h0 over [-12, 12] (the GELU's u clamp at -40 lies at x = -9.65),
    h0 / h1 the two halves of one packed (rows, 2F) projection as the feed-forward stores them"""
    gated_act = importlib.import_module("flasht5_amd.gated_act")
    g = _gen("gact", act, dtype)
    rows, F = 64, 1024
    h = torch.empty((rows, 2 * F), dtype=dtype)
    h[:, :F] = torch.linspace(-12, 12, rows * F).reshape(rows, F)[torch.randperm(rows, generator=g)].to(dtype)
    h[:, F:] = torch.randn(rows, F, generator=g).to(dtype)
    h = h.cuda()
    h0, h1 = h[:, :F], h[:, F:]
    dout = _randn((rows, F), dtype, g)
    out = gated_act.gated_act_fwd(h0, h1, ACT[act])
    dh = gated_act.gated_act_bwd(dout, h0, h1, ACT[act])
    _gated_check(h0, h1, dout, act, out, dh, slice(None), f"{act} {_name(dtype)}")


# rows on both sides of the host's 65535-row grid split (grid.y limit) and two full chunks plus one row
@pytest.mark.parametrize("rows,dtype,act", [(65535, BF16, "gelu_tanh"), (65536, F16, "gelu_tanh"), (65537, F32, "relu"), (131071, BF16, "gelu_tanh")])
def test_gated_act_row_split(rows, dtype, act):
    """gated_act_fwd_kernel<X, ACT> / gated_act_bwd_kernel<X, ACT> launched once per 65535 rows with the bases moved by
    r0 * stride * esz (packed (rows, 2F) input, so the row stride is 2F, not F)"""
    gated_act = importlib.import_module("flasht5_amd.gated_act")
    g = _gen("split", rows, dtype)
    F = 16
    h = _randn((rows, 2 * F), dtype, g, 3.0)
    h0, h1 = h[:, :F], h[:, F:]
    dout = _randn((rows, F), dtype, g)
    out = gated_act.gated_act_fwd(h0, h1, ACT[act])
    dh = gated_act.gated_act_bwd(dout, h0, h1, ACT[act])
    w = 64
    idx = sorted({i for c in range(0, rows, 65535) for i in range(c - w, c + w) if 0 <= i < rows} | set(range(max(0, rows - w), rows)))
    sel = torch.tensor(idx)
    _gated_check(h0.cpu(), h1.cpu(), dout.cpu(), act, out.cpu(), dh.cpu(), sel, f"rows={rows}")
    # the rest of the second and later chunks: bit for bit against a launch on the slice [65535:]
    out2 = gated_act.gated_act_fwd(h0[65535:], h1[65535:], ACT[act])
    dh2 = gated_act.gated_act_bwd(dout[65535:], h0[65535:], h1[65535:], ACT[act])
    assert torch.equal(out[65535:], out2) and torch.equal(dh[65535:], dh2)


# ------------------------------------------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------------------------------------------
def _ce_check(loss, z, lse, dlogits, logits, labels, dl, sm, scale, zs, ign, vector, what):
    V = logits.shape[-1]
    dtype = logits.dtype
    loss_ref, z_ref, lse_ref = R.ce_fwd(logits, labels, sm, scale, zs, ign)
    x = logits.double().cpu() * scale
    p = torch.exp(x - lse_ref.unsqueeze(-1))
    xf = torch.where(torch.isfinite(x), x, torch.zeros(()).double())
    D = (VEC[dtype] + math.ceil(V / (256 * VEC[dtype])) + 12) if vector else (math.ceil(V / 256) + 12)
    T = 1 + lse_ref.abs() + (p * xf.abs()).sum(-1)
    e_lse = (D + 4) * U * T
    _check(lse, lse_ref, 0.5 * R.ulp(lse_ref, F32) + e_lse, f"{what} lse")
    lab = labels.cpu()
    picked = xf.gather(-1, lab.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    e_z = 2 * zs * lse_ref.abs() * e_lse + 4 * U * z_ref.abs()
    _check(z, z_ref, 0.5 * R.ulp(z_ref, F32) + e_z, f"{what} z")
    own = 4 * U * (lse_ref.abs() + picked.abs() + z_ref.abs() + sm * (D + 4) * xf.abs().sum(-1) / V)
    _check(loss, loss_ref, 0.5 * R.ulp(loss_ref, F32) + e_lse + e_z + own, f"{what} loss")
    d_ref = R.ce_bwd(dl, logits, labels, sm, scale, zs, ign)
    gabs = torch.where(lab == ign, torch.zeros(()).double(), dl.double().cpu().expand(lab.shape).abs() * scale).unsqueeze(-1)
    zf = (1 + 2 * zs * lse_ref).abs().unsqueeze(-1)
    bd = 0.5 * R.ulp(d_ref, dtype) + U * gabs * (p * zf * ((D + 6) * T.unsqueeze(-1) + 2 * xf.abs() + 2 * lse_ref.abs().unsqueeze(-1) + 6) +
                                                 2 * (1 + sm / V))
    _check(dlogits, d_ref, bd, f"{what} dlogits")


def _ce_all(logits, labels, dl, sm=0.0, scale=1.0, zs=0.0, ign=-100, what=""):
    """the two launches (ce_fwd_kernel / ce_bwd_kernel) and the one-launch form (ce_fwd_bwd_kernel) on the same problem, each twice"""
    ce = importlib.import_module("flasht5_amd.cross_entropy_loss")
    V = logits.shape[-1]
    vector = V % VEC[logits.dtype] == 0 and logits.stride(0) % VEC[logits.dtype] == 0 and logits.data_ptr() % 16 == 0
    runs = []
    for _ in range(2):
        loss, z, lse = ce.cross_entropy_fwd(logits, labels, None, sm, scale, zs, ign)
        d = ce.cross_entropy_bwd(dl, logits, lse, labels, False, sm, scale, zs, ign)
        runs.append((loss, z, lse, d))
    _ce_check(*runs[0], logits, labels, dl, sm, scale, zs, ign, vector, f"{what} two launches")
    assert all(torch.equal(a, b) for a, b in zip(*runs)), f"{what}: two launches not deterministic"
    if logits.stride(-1) == 1 and logits.data_ptr() % 16 == 0:
        fused = []
        rows, s0 = logits.shape[0], logits.stride(0)
        for _ in range(2):
            buf = torch.empty((rows, s0), dtype=logits.dtype, device="cuda")[:, s0 - V:]  # (in place, at the logits' row stride)
            buf.copy_(logits)
            assert buf.stride(0) == s0 and buf.data_ptr() % 16 == 0
            loss, z, lse = (torch.empty(rows, device="cuda") for _ in range(3))
            ce.cross_entropy_fwd_bwd_(buf, labels, dl, loss, z, lse, sm, scale, zs, ign)
            fused.append((loss, z, lse, buf))
        _ce_check(*fused[0], logits, labels, dl, sm, scale, zs, ign, vector, f"{what} one launch")
        assert all(torch.equal(a, b) for a, b in zip(*fused)), f"{what}: one launch not deterministic"


# vocabulary widths on both sides of ce_fwd_bwd_kernel's HOLD bound (16 * 256 * VEC columns) and a width that is not a multiple of
# VEC (ce_fwd_kernel<X, false> / ce_bwd_kernel<X, false>; the one-launch entry point falls back to the two launches)
CE_V = [(BF16, 32768), (BF16, 32776), (F16, 32768), (F16, 32776), (F32, 16384), (F32, 16388), (BF16, 32767), (F32, 1001)]


@pytest.mark.parametrize("dtype,V", CE_V, ids=[f"{_name(d)}-{v}" for d, v in CE_V])
@pytest.mark.parametrize("sm,scale,zs", [(0.0, 1.0, 0.0), (0.1, 0.5, 1e-4)])
def test_ce_widths(dtype, V, sm, scale, zs):
    """ce_fwd_kernel<X, VECOK> + ce_bwd_kernel<X, VECOK>, and ce_fwd_bwd_kernel<X, HOLD> with HOLD = (V <= 16 * 256 * VEC); labels in
    the vocabulary, ignored, and outside it on either side"""
    g = _gen("ce", dtype, V, sm)
    rows = 6
    logits = _randn((rows, V), dtype, g, 4.0)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[1], labels[3], labels[4] = -100, V + 5, -3
    labels[5] = V - 1
    dl = torch.randn(rows, generator=g).cuda()
    _ce_all(logits, labels.cuda(), dl, sm, scale, zs, -100, f"{_name(dtype)} V={V}")


@pytest.mark.parametrize("dtype,V", [(BF16, 32768), (BF16, 40000), (F16, 8192), (F32, 16384), (F32, 20000), (BF16, 32767)])
def test_ce_minus_inf_rows(dtype, V):
    """rows that are -inf everywhere but at the label (smoothing 0; with smoothing the loss is infinite by definition), the label
    at the row's start, in a thread's later chunk and at its end: a thread whose first chunks hold only -inf starts its running max at
    -inf.  ce_fwd_kernel / ce_bwd_kernel and ce_fwd_bwd_kernel (HOLD for 32768 bf16 and 16384 fp32, re-reading for 40000 and 20000)"""
    g = _gen("inf", dtype, V)
    labels = torch.tensor([0, 5, 256 * VEC[dtype] + 3, V // 2 + 1, V - 1, V - 2 * 256 * VEC[dtype] - 1])
    rows = labels.numel()
    logits = torch.full((rows, V), float("-inf"))
    logits[torch.arange(rows), labels] = torch.tensor([2.0, -3.0, 0.5, 7.0, -1.0, 4.0])
    logits[1, 100] = 1.0  # (a second finite logit)
    dl = torch.randn(rows, generator=g).cuda()
    _ce_all(logits.to(dtype).cuda(), labels.cuda(), dl, 0.0, 1.0, 1e-4, -100, f"-inf {_name(dtype)} V={V}")


@pytest.mark.parametrize("V", [4096, 20000])
def test_ce_large_logits(V):
    """fp32 logits of +-1e4 (the exponent argument and lse are ~1e4: every rounding is 1e-3 absolute): ce_fwd_bwd_kernel<F32, HOLD>
    (4096) and <F32, false> (20000), and the two launches"""
    g = _gen("big", V)
    rows = 6
    logits = torch.randn(rows, V, generator=g)
    logits[:, ::7] = 1e4 - torch.rand(rows, len(range(0, V, 7)), generator=g) * 30
    logits[:, 3::7] = -1e4
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[0] = 7  # a large one
    labels[1] = 3  # a -1e4 one
    dl = torch.randn(rows, generator=g).cuda()
    _ce_all(logits.cuda(), labels.cuda(), dl, 0.0, 1.0, 1e-4, -100, f"+-1e4 V={V}")
    _ce_all(logits.cuda(), labels.cuda(), dl, 0.1, 0.5, 0.0, -100, f"+-1e4 smoothed V={V}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_all_rows_ignored(dtype):
    """a batch in which every row is ignored: loss = z = 0 and dlogits = 0 exactly (ce_fwd_bwd_kernel<X, true> and the two launches)"""
    ce = importlib.import_module("flasht5_amd.cross_entropy_loss")
    g = _gen("ign", dtype)
    rows, V = 5, 4096
    logits = _randn((rows, V), dtype, g, 3.0)
    labels = torch.full((rows,), -1, dtype=torch.int64).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    _ce_all(logits, labels, dl, 0.1, 1.0, 1e-4, -1, f"ignored {_name(dtype)}")
    loss, z, lse = ce.cross_entropy_fwd(logits, labels, None, 0.1, 1.0, 1e-4, -1)
    d = ce.cross_entropy_bwd(dl, logits, lse, labels, False, 0.1, 1.0, 1e-4, -1)
    assert not bool(loss.any()) and not bool(z.any()) and not bool(d.any())
    assert torch.isfinite(lse).all()


def test_ce_strided_rows():
    """logits rows with stride V + 8 (bf16): ce_fwd_kernel<BF16, true> / ce_bwd_kernel<BF16, true> read strided rows (their dlogits
    are contiguous), ce_fwd_bwd_kernel<BF16, true> reads and rewrites strided rows in place"""
    g = _gen("cestride")
    V = 8192
    logits = _randn((6, V + 8), BF16, g, 3.0)[:, 8:]
    labels = torch.randint(0, V, (6,), generator=g).cuda()
    dl = torch.randn(6, generator=g).cuda()
    _ce_all(logits, labels, dl, 0.0, 1.0, 1e-4, -100, "strided")
