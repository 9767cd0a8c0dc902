"""MXFP8 activations and the W4A8 linear in plain torch: the contract of include/fat5.h ("MXFP8 activations") restated -- the
activation quantiser, its dequantiser, the linear layer in fp64 and its per-element bound.  CPU only; imports no GPU code.

The rule.  x (R, K), fp16 / bf16, becomes a8 (R, K) e4m3fn bytes (sign << 7 | exponent << 3 | mantissa, bias 7; exponent 0: m 2^-9)
and ax (R, K / 32) e8m0 bytes (2^(byte - 127), 255 = NaN).  Per block of 32 values as fp32: a non-finite value -> byte 255 over
zero bytes; amax = 0 -> byte 127; else byte = max(exponent field of amax - 8, 1), that is X = floor(log2 amax) - 8 clamped; element
= round-to-nearest-even of |v| 2^-X onto the e4m3fn grid, saturating at 448; sign = v's sign bit.

The bound.  ref = sum over the dequantised operands in fp64.  Every product a q is exact in fp32 (4 + 2 significand bits, times
powers of two), so the only roundings are the additions and the store: with A = sum_k |a| |w|,
    |y - ref| <= e + ulp_T(|ref| + e) / 2,      e = gamma(c K) A.
c describes the instruction, not the kernel: the project's charge c = 2 (w4_ref.bound) is missed on the hardware, because
v_mfma_scale_f32_16x16x128_f8f6f4 does not sum like an fp32 addition tree: inside one 32-k block it aligns the products to the
block's largest and drops what lies some 2^-12 below it (256 - 256 + 2^-3 comes out as 2^-3, 256 - 256 + 2^-6 as 0; the same small
term in ANOTHER block survives).  c is therefore measured, on the one-step shape K = 128 -- the instruction alone -- with the
linear test's own operands at every (R, N) of its cases: the worst |y - ref| over the c = 1 bound is 1.5843 in bf16 (at (257, 264))
and 4.2946 in fp16 (at (128, 128)); c is the next power of two at or above twice the worst ratio: c = 16 (DESIGN 4.28 lists every
case).  It holds for operands like the tests'; a block whose products span more than those can lose more."""
import torch

import w4_ref
from w8_ref import gamma, ulp


def quantize_act_ref(x):
    """x (R, K) fp16 / bf16 -> (a8 (R, K) uint8, ax (R, K / 32) uint8)"""
    R, K = x.shape
    v = x.float().view(R, K // 32, 32)
    bits = v.contiguous().view(torch.int32)
    am = (bits & 0x7fffffff).amax(-1)
    bad = am >= 0x7f800000
    byte = ((am >> 23) - 8).clamp(min=1)
    byte = torch.where(am == 0, torch.full_like(byte, 127), byte)
    a = (torch.where(bad.unsqueeze(-1), torch.zeros(()), v).double().abs() * torch.pow(2.0, (127 - byte).double()).unsqueeze(-1)).clamp(max=448.0)
    e = (torch.frexp(a)[1] - 1).clamp(min=-6)                       # the grid's step around a is 2^(e - 3); below 2^-6: 2^-9
    q = torch.round(a * torch.pow(2.0, (3 - e).double())) * torch.pow(2.0, (e - 3).double())     # (round: half to even)
    eq = torch.frexp(q)[1] - 1                                       # (a carry moved q into the next binade)
    normal = ((eq + 7) << 3) | (q * torch.pow(2.0, (3 - eq).double()) - 8).long()
    code = torch.where(q < 2.0 ** -6, (q * 512).long(), normal)
    a8 = (code | ((bits >> 31) & 1) << 7).masked_fill(bad.unsqueeze(-1), 0)
    return a8.view(R, K).to(torch.uint8), byte.masked_fill(bad, 255).to(torch.uint8)


def decode_e4m3(b):
    """uint8 -> fp64 (0x7f / 0xff: NaN)"""
    b = b.long()
    e, m = (b >> 3) & 15, (b & 7).double()
    f = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * torch.pow(2.0, (e - 7).double()))
    f = f.masked_fill((b & 127) == 127, float("nan"))
    return torch.where((b & 128) != 0, -f, f)


def dequant_act(a8, ax):
    """-> (R, K) fp64, NaN in the blocks whose byte is 255"""
    s = torch.pow(2.0, ax.double() - 127).masked_fill(ax == 255, float("nan"))
    return decode_e4m3(a8) * s.repeat_interleave(32, dim=1)


def linear_ref(a8, ax, w4, e8):
    """(ref (R, N) fp64, A (R, N) fp64): the exact result over the dequantised operands, and the magnitude sum of the bound"""
    a, w = dequant_act(a8, ax), w4_ref.dequant(w4, e8)
    return a @ w.t(), a.abs() @ w.abs().t()


def bound(ref, A, K, dtype, c=16):
    e = gamma(c * K) * A
    return e + ulp(ref.abs() + e, dtype) / 2
