"""FP8 weights in plain torch: the contract of include/fat5.h ("FP8 weights") restated -- the per-row weight quantiser, the linear
layer in fp64, its per-element bound, and an fp32 emulation of the kernel's arithmetic with defects, to show that the checks tell
them from the truth.  CPU only; imports no GPU code.  Used by tests/test_w8_cpu.py, tests/test_w8_gpu.py and
tests/test_w8_generation_gpu.py.

The rule.  A weight W (N, K) becomes w8 (N, K) e4m3fn bytes and scale (N,) fp32, one scale per output row n over its K elements,
by the rule of the FP8 KV cache (tests/kvfp8_ref.py: amax / 448, 1 for a zero row, RNE, a non-finite row gets +inf), and
    y[r, n]   = round_T( scale[n] * sum_k fp32(xin[r, k]) * fp32(w8[n, k]) )        T = bf16 | fp16, fp32 accumulation
    xin       = x, or with a norm weight g:  round_T(fp32(x) * rstd_r * fp32(g[k])),  rstd_r = 1 / sqrt(mean_k x^2 + eps)
    out[r, n] = y[r, n], or with a residual: round_T(fp32(y[r, n]) + fp32(residual[r, n]))   (y already rounded to T)

The bound.  ref[r, n] = scale[n] * sum_k xin[r, k] * w8[n, k] in fp64, from the T-rounded xin (exact products, exact sum to
fp64's precision).  With u = 2^-24 and A[r, n] = |scale[n]| * sum_k |xin[r, k]| |w8[n, k]|,
    |y - ref| <= e + ulp_T(|ref| + e) / 2,      e = gamma(c(K)) * A,   gamma(c) = c u / (1 - c u).
c(K) counts the fp32 roundings on the longest path from a product to the scaled sum, from the kernel's own operation counts
(csrc/w8_kernels.h): a product is exact (a 16-bit significand of at most 11 bits times an e4m3 one of at most 4); lane l adds its
products with one fma each, 8 per step of 512 elements, so at most 8 * ceil(K / 512) roundings; the 64 lane sums go through
wave_sum's six-level tree, 6 more; the multiply by the scale is 1 more:
    c(K) = 8 * ceil(K / 512) + 6 + 1.
Every rounding is relative to a partial sum whose magnitude is at most sum |terms|, which gives e (the standard gamma bound).  The
store rounds the fp32 value y' with |y' - ref| <= e to T: half an ulp of y', and |y'| <= |ref| + e -- so the half ulp is taken at
|ref| + e, which is ulp_T(ref) / 2 wherever y' stays in ref's binade.  No constant is fitted.

The residual add is no part of the bound: it is defined on the rounded y, so it is checked exactly (`residual_ref`); so is the
norm in front (the kernel's xin equals the RMSNorm kernel's output bit for bit, and ref starts from that xin).
"""
import math

import torch

from kvfp8_ref import FP8, quantize_ref as _quantize_rows, same_bits  # noqa: F401  (the rule is the KV cache's)

U32 = 2.0 ** -24
LANE_K, TREE_DEPTH = 512, 6     # the kernel's constants: K elements a wave covers per step (W8_LANE_K), wave_sum's levels


# ------------------------------------------------------------------------------------------------------------------ the rule
def quantize_ref(W):
    """W (N, K) fp32 / fp16 / bf16 -> (w8 (N, K) float8_e4m3fn, scale (N,) fp32): one KV-cache row per output row"""
    return _quantize_rows(W)


def dequant(w8, scale, dtype=torch.float64):
    return w8.to(dtype) * scale.to(dtype).unsqueeze(-1)


def norm_ref(x, g, eps):
    """the T-rounded RMSNorm of x (rows, K) in the contract's operation order, with the row statistic in fp64 (the kernels' fp32
    statistic can differ from it in the last bit: GPU tests take xin from the RMSNorm kernel itself)"""
    xf = x.float()
    rstd = (1.0 / torch.sqrt(x.double().pow(2).mean(-1, keepdim=True) + eps)).float()
    return (xf * rstd * g.float()).to(x.dtype)


def residual_ref(y, residual):
    """the epilogue, exact: round_T(fp32(y) + fp32(residual)) of the ALREADY ROUNDED y"""
    return (y.float() + residual.float()).to(y.dtype)


# ------------------------------------------------------------------------------------------------------------- fp64 and the bound
def c_of_K(K):
    return 8 * math.ceil(K / LANE_K) + TREE_DEPTH + 1


def gamma(c):
    return c * U32 / (1.0 - c * U32)


def ulp(v, dtype):
    """the spacing of `dtype` at magnitude v (fp64 tensor), subnormals included"""
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def linear_ref(xin, w8, scale):
    """(ref (R, N) fp64, A (R, N) fp64): the exact result from the T-rounded xin (R, K), and the magnitude sum of the bound"""
    x, w, s = xin.double(), w8.double(), scale.double()
    return (x @ w.t()) * s, (x.abs() @ w.abs().t()) * s.abs()


def linear_bound(ref, A, K, dtype):
    e = gamma(c_of_K(K)) * A
    return e + ulp(ref.abs() + e, dtype) / 2


def accepts(y, xin, w8, scale):
    """whether y (R, N) of dtype T is inside the bound everywhere; NaN / inf in ref must be matched by non-finite y"""
    ref, A = linear_ref(xin, w8, scale)
    bound = linear_bound(ref, A, xin.shape[-1], y.dtype)
    fin = torch.isfinite(ref)
    ok = torch.where(fin, (y.double() - ref).abs() <= bound, ~torch.isfinite(y.double()))
    return bool(ok.all())


def worst(y, xin, w8, scale):
    """max over the elements of |y - ref| / bound (a figure to print; finite elements only)"""
    ref, A = linear_ref(xin, w8, scale)
    bound = linear_bound(ref, A, xin.shape[-1], y.dtype)
    fin = torch.isfinite(ref) & (bound > 0)
    return float(((y.double() - ref).abs()[fin] / bound[fin]).max()) if bool(fin.any()) else 0.0


# ---------------------------------------------------------------------------------- an fp32 emulation of the kernel's arithmetic
def _sum_kernel_order(t):
    """t (..., K) fp32 products -> their fp32 sum in the kernel's order: lane l = (k // 8) % 64 adds its terms in ascending k,
    then a pairwise tree over the 64 lanes"""
    K = t.shape[-1]
    steps = math.ceil(K / LANE_K)
    pad = torch.zeros(t.shape[:-1] + (steps * LANE_K,), dtype=torch.float32)
    pad[..., :K] = t
    pad = pad.view(t.shape[:-1] + (steps, 64, 8))
    acc = torch.zeros(t.shape[:-1] + (64,), dtype=torch.float32)
    for i in range(steps):
        for j in range(8):
            acc = acc + pad[..., i, :, j]
    while acc.shape[-1] > 1:   # (lane ^ 1, lane ^ 2, ... : adjacent pairs first)
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def _sum_pairwise(t):
    """a second order: a pairwise tree over k itself"""
    K = t.shape[-1]
    n = 1 << (K - 1).bit_length()
    acc = torch.zeros(t.shape[:-1] + (n,), dtype=torch.float32)
    acc[..., :K] = t
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


ORDERS = {"kernel": _sum_kernel_order, "pairwise": _sum_pairwise}
MUTANTS = ("scale not applied", "scale from row n + 1", "norm output not rounded", "residual added before the rounding",
           "one k-chunk of 64 dropped")


def emulate(x, w8, scale, norm_weight=None, eps=1e-6, residual=None, order="kernel", mutant=None):
    """The linear layer in fp32 as the kernel computes it -> (xin, y, out): the T-rounded input of the dot product, the rounded
    result before the residual, and the final output (y itself without a residual).  `mutant`: one of MUTANTS."""
    T = x.dtype
    xin = x if norm_weight is None else norm_ref(x, norm_weight, eps)
    xd = xin.float()
    if mutant == "norm output not rounded" and norm_weight is not None:
        xf = x.float()
        rstd = (1.0 / torch.sqrt(x.double().pow(2).mean(-1, keepdim=True) + eps)).float()
        xd = xf * rstd * norm_weight.float()
    w = w8.float()
    prod = xd.unsqueeze(1) * w.unsqueeze(0)    # (R, N, K): exact in fp32 for T-rounded inputs
    if mutant == "one k-chunk of 64 dropped":
        prod = prod.clone()
        prod[..., 64:128] = 0
    acc = ORDERS[order](prod)
    s = scale
    if mutant == "scale not applied":
        s = torch.ones_like(scale)
    if mutant == "scale from row n + 1":
        s = scale.roll(-1, 0)
    y32 = acc * s
    y = y32.to(T)
    if residual is None:
        return xin, y, y
    if mutant == "residual added before the rounding":
        return xin, y, (y32 + residual.float()).to(T)
    return xin, y, residual_ref(y, residual)
