"""MXFP4 weights in plain torch: the contract of include/fat5.h ("MXFP4 weights") restated -- the block quantiser, the
dequantiser, the linear layer in fp64 and its per-element bound.  CPU only; imports no GPU code.

The rule.  W (N, K) becomes w4 (N, K / 2) bytes (element 2 j in the low nibble of byte j, 2 j + 1 in the high one; a nibble is
sign | e2m1 code, the codes 0 .. 7 meaning GRID) and e8 (N, K / 32) e8m0 bytes (2^(byte - 127), 255 = NaN).  Per block of 32 values
as fp32: a non-finite value -> byte 255 and nibbles 0; amax = 0 -> X = 0; else X = clamp(floor(log2 amax) - 2, -13, 13); byte =
X + 127; code = round-to-nearest-even of |v| 2^-X onto GRID (a tie goes to the even code), saturating at 6; sign = v's sign bit.

The bound.  ref = sum_k xin q 2^X in fp64 from the T-rounded xin.  Every q 2^X is a value of T and every product is exact in fp32
(11 + 2 significand bits), there is no scale rounding, and at most K - 1 additions lie on a path from a product to the sum, each
charged 2 u (u = 2^-24): with A = sum_k |xin| |q 2^X|,
    |y - ref| <= e + ulp_T(|ref| + e) / 2,      e = gamma(2 K) A,   gamma(c) = c u / (1 - c u)
(tests/test_w8_mma_gpu.py's derivation without the scale term; the half ulp is the store's).  No constant is fitted."""
import torch

from w8_ref import gamma, ulp

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def quantize_ref(W):
    """W (N, K) fp32 / fp16 / bf16 -> (w4 (N, K / 2) uint8, e8 (N, K / 32) uint8)"""
    N, K = W.shape
    v = W.float().view(N, K // 32, 32)
    bad = ~torch.isfinite(v).all(-1)
    amax = torch.where(bad, torch.ones(()), v.abs().amax(-1))
    X = (torch.frexp(amax)[1] - 1 - 2).clamp(-13, 13)            # amax = m 2^e, m in [0.5, 1): floor(log2 amax) = e - 1
    X = torch.where(amax == 0, torch.zeros_like(X), X)
    a = (v.abs().double() * torch.pow(2.0, -X.double()).unsqueeze(-1)).unsqueeze(-1)    # exact
    mid = (GRID[:-1] + GRID[1:]) / 2                              # a tie at mid[i] goes up iff code i + 1 is even
    code = ((a > mid) | ((a == mid) & (torch.arange(7) % 2 == 1))).sum(-1)
    nib = (code | (torch.signbit(v).long() << 3)).masked_fill(bad.unsqueeze(-1), 0).view(N, K)
    e8 = (X + 127).masked_fill(bad, 255)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8), e8.to(torch.uint8)


def dequant(w4, e8):
    """-> (N, K) fp64, NaN in the blocks whose byte is 255"""
    nib = torch.stack([w4 & 15, w4 >> 4], -1).view(w4.shape[0], -1).long()
    q = GRID[nib & 7] * (1.0 - 2.0 * (nib >> 3).double())
    s = torch.pow(2.0, e8.double() - 127).masked_fill(e8 == 255, float("nan"))
    return q * s.repeat_interleave(32, dim=1)


def linear_ref(xin, w4, e8):
    """(ref (R, N) fp64, A (R, N) fp64): the exact result from the T-rounded xin (R, K), and the magnitude sum of the bound"""
    x, w = xin.double(), dequant(w4, e8)
    return x @ w.t(), x.abs() @ w.abs().t()


def bound(ref, A, K, dtype):
    e = gamma(2 * K) * A
    return e + ulp(ref.abs() + e, dtype) / 2
