"""The FP8 KV cache in plain torch: the storage contract of include/fat5.h ("FP8 KV cache") restated, mutants of the rule, the fp64
reference and the per-element bound of attention over an FP8 cache, and an fp32 emulation of the kernels' FP8 arithmetic with
defects to show that the bound tells them from the truth.  CPU only; imports no GPU code.  Used by tests/test_kvfp8_cpu.py,
tests/test_kvfp8_gpu.py and tests/test_kvfp8_generation_gpu.py.

The rule.  A row x of D elements (fp16 / bf16):
    a_d = |fp32(x_d)|, a NaN counted as +inf;  amax = max_d a_d;  s = amax / 448 (fp32 division), s = 1 when amax == 0
    byte_d = (fp32(x_d) / s).clamp(-448, 448).to(torch.float8_e4m3fn)     (round to nearest even, subnormals included)
and the value read back is fp32(byte_d) * s.  Non-finite rows: amax = +inf, so s = +inf; a finite element then gives 0, an inf
gives inf / inf = NaN, a NaN stays NaN, and NaN is stored as the byte 0x7F whatever its sign (torch keeps the sign bit of a NaN,
which differs between machines for inf / inf; a NaN's sign is not a value).  Such a row reads back as NaN everywhere.

The bound.  The reference is fp64 attention over the dequantised contents of the cache AFTER the call (bytes x scales, exact in
fp64) through decode_fp64.decode_ref / decode_chunk_fp64.chunk_ref, and the bound is theirs plus the two roundings the FP8 path adds
(u = 2^-24; A, T and the other symbols as in decode_fp64's docstring):
  * the K scale multiplies the finished dot product, one more fp32 rounding of the score before the bias is added: the score error
    ds grows by u A (log2 units), a key's weight error e_p = ln2 2 ds + e_w by 2 ln2 u A, and the bounds hold 2 e_p (o) and e_p (lse);
  * the V scale multiplies the softmax weight that goes into acc[] (not the one summed into l): one rounding per term of the
    numerator, u T.
      extra_o = (4 ln2 u A log2e + u) T,   extra_lse = 2 ln2 u A log2e.
The conversions byte -> fp32 are exact and the scales are read, not computed, so nothing else is added.  No term is fitted.
"""
import math

import torch

import decode_chunk_fp64 as C
import decode_fp64 as F

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


# ------------------------------------------------------------------------------------------------------------------ the rule
def scale_ref(x):
    a = x.float().abs()
    a = torch.where(torch.isnan(a), torch.full_like(a, math.inf), a)
    amax = a.amax(-1)
    return torch.where(amax == 0, torch.ones_like(amax), amax / torch.tensor(FP8_MAX, dtype=torch.float32))


def quantize_ref(x):
    """x (..., D) fp16 / bf16 -> (bytes (..., D) float8_e4m3fn, s (...) fp32)"""
    s = scale_ref(x)
    y = (x.float() / s.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX)
    b = y.to(FP8)
    b = torch.where(torch.isnan(y), torch.full_like(b.view(torch.uint8), 0x7F), b.view(torch.uint8)).view(FP8)
    return b, s


def dequant(b, s, dtype=torch.float64):
    """the value read back: fp(byte) * s (exact in fp64; in fp32 what the contract defines)"""
    return b.to(dtype) * s.to(dtype).unsqueeze(-1)


def same_bits(b0, s0, b1, s1):
    return torch.equal(b0.view(torch.uint8), b1.view(torch.uint8)) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


def roundtrip_bound(x, s):
    """|deq - x| <= max(2^-4 |x|, 2^-10 s): half an ulp of a 3-bit mantissa, or half the subnormal spacing 2^-9, times the scale"""
    return torch.maximum(x.double().abs() * 2.0 ** -4, s.double().unsqueeze(-1) * 2.0 ** -10)


# -- mutants of the rule: each returns (bytes, s) as a defective quantiser would
def _trunc_to_fp8(y):
    """round toward zero instead of to nearest even"""
    b = y.to(FP8)
    up = b.float().abs() > y.abs()
    bits = b.view(torch.uint8).clone()
    bits[up] -= 1   # (the next e4m3fn value toward zero has the next smaller byte: the encoding is monotone in magnitude)
    return bits.view(FP8)


def mutant_truncate(x):
    s = scale_ref(x)
    return _trunc_to_fp8((x.float() / s.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX)), s


def mutant_no_clamp(x):
    """no clamp, seen where it matters: under the exact scale no quotient exceeds 448, so the defect shows only with a scale that
    is a little small -- here amax / 512, the power of two a shift-based scale would take -- where the unclamped conversion turns the
    row's largest elements (above 464) into NaN instead of saturating them"""
    s = scale_ref(x) * 0.875
    return (x.float() / s.unsqueeze(-1)).to(FP8), s


def mutant_fnuz(x):
    """e4m3fnuz bytes (bias 8) under the same scale"""
    s = scale_ref(x)
    return (x.float() / s.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fnuz).view(torch.uint8).view(FP8), s


def mutant_wrong_axis(x):
    """amax over the rows instead of over D"""
    a = x.float().abs().amax(-2, keepdim=True).expand(x.shape).amax(-1) if x.dim() > 1 else x.float().abs().amax(-1)
    s = torch.where(a == 0, torch.ones_like(a), a / FP8_MAX)
    return (x.float() / s.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(FP8), s


def mutant_multiply(x):
    """the element multiplied by the scale instead of divided"""
    s = scale_ref(x)
    return (x.float() * s.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(FP8), s


RULE_MUTANTS = {
    "truncation instead of RNE": mutant_truncate,
    "no clamp": mutant_no_clamp,
    "fnuz bias": mutant_fnuz,
    "amax over the wrong axis": mutant_wrong_axis,
    "scale multiplied instead of divided": mutant_multiply,
}


# ------------------------------------------------------------------------------------------- attention over an FP8 cache: fp64
def _extra(ref):
    dds = F.U32 * ref["smag"] * F.LOG2E                      # the K scale's rounding of the score, log2 units
    eo = (4 * F.LN2 * dds + F.U32).unsqueeze(-1) * ref["absv"]
    return eo, 2 * F.LN2 * dds


def decode_ref8(q, kb, ks, vb, vs, lens_before, append, sm_scale, rpe1d=None, R=0, batch_idx=None, row_batch=None, splits=1):
    """fat5_attn_decode over FP8 caches: kb / vb, ks / vs the bytes and scales AFTER the call; lens_before the lengths before it;
    `append`: the call appended a row (then row len_b of the cache after the call is the row the query attended)."""
    kc, vc = dequant(kb, ks), dequant(vb, vs)
    cap = kb.shape[1]
    lens = [max(0, min(int(n), cap)) for n in lens_before]
    after = [min(n + 1, cap) if append else n for n in lens]
    if append and row_batch is not None:   # (the appended row is written to, and attended at, the sequence's own batch element)
        row_batch = row_batch.clone()
        for b, n in enumerate(lens):
            if n < cap:
                row_batch[b, n] = b
    return F.decode_ref(q, kc, vc, None, None, after, sm_scale, rpe1d, R, batch_idx, row_batch, splits)


def decode_bound8(ref, dtype, D, splits):
    bo, bl = F.decode_bound(ref, dtype, D, splits)
    eo, el = _extra(ref)
    return bo + eo, bl + el


def chunk_ref8(q, kb, ks, vb, vs, lens_before, kn_like, sm_scale, causal, rpe1d=None, R=0, splits=1):
    """fat5_attn_decode_chunk over FP8 caches after the call.  With an append (kn_like: any (B, M, H, D) tensor, only its being there
    matters) the new rows are taken from the cache after the call: chunk_ref is handed the dequantised rows as k_new / v_new, so
    its positions and visibility are the contract's."""
    kc, vc = dequant(kb, ks), dequant(vb, vs)
    B, M = q.shape[:2]
    cap = kb.shape[1]
    kn = vn = None
    if kn_like is not None:
        kn, vn = torch.zeros(q.shape, dtype=torch.float64), torch.zeros(q.shape, dtype=torch.float64)
        for b in range(B):
            n = max(0, min(int(lens_before[b]), cap))
            a = min(M, cap - n)
            kn[b, :a], vn[b, :a] = kc[b, n:n + a], vc[b, n:n + a]
    return C.chunk_ref(q, kc, vc, kn, vn, lens_before, sm_scale, causal, rpe1d, R, splits)


def chunk_bound8(ref, dtype, D, splits):
    bo, bl = C.chunk_bound(ref, dtype, D, splits)
    eo, el = _extra(ref)
    return bo + eo, bl + el


# ------------------------------------------------------------------------------- an fp32 emulation of the kernel's FP8 arithmetic
def emulate_decode8(q, kb, ks, vb, vs, lens_before, kn, vn, sm_scale, mutant=None):
    """One-row decode over FP8 caches in fp32, the operations the kernel performs (not their order inside a sum): the dot product
    of q with the converted bytes, times the K scale, softmax weights, each weight times its V scale into the output.  kb / vb /
    ks / vs: the caches BEFORE the call; kn / vn (B, 1, H, D) or None.  Returns (o (B, H, D), lse (B, H), caches after the call).
    `mutant`: "k scale not applied", "v scale from the wrong row", "new row attended unquantised"."""
    B, H, D = q.shape[0], q.shape[-2], q.shape[-1]
    cap = kb.shape[1]
    kb, ks, vb, vs = kb.clone(), ks.clone(), vb.clone(), vs.clone()
    o = torch.zeros(B, H, D, dtype=torch.float32)
    lse = torch.full((B, H), -math.inf, dtype=torch.float32)
    for b in range(B):
        n = max(0, min(int(lens_before[b]), cap))
        L = n
        if kn is not None and n < cap:
            (kb[b, n], ks[b, n]), (vb[b, n], vs[b, n]) = quantize_ref(kn[b, 0]), quantize_ref(vn[b, 0])
            L = n + 1
        if L == 0:
            continue
        K, V = kb[b, :L].float(), vb[b, :L].float()          # (L, H, D) converted bytes
        ksc, vsc = ks[b, :L].clone(), vs[b, :L].clone()       # (L, H)
        if mutant == "new row attended unquantised" and L == n + 1:
            K[n], V[n] = kn[b, 0].float(), vn[b, 0].float()
            ksc[n], vsc[n] = 1.0, 1.0
        if mutant == "k scale not applied":
            ksc = torch.ones_like(ksc)
        if mutant == "v scale from the wrong row":
            vsc = vsc.roll(1, 0)
        s = torch.einsum("hd,lhd->hl", q.reshape(B, H, D)[b].float(), K) * ksc.t() * float(sm_scale)
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        l = p.sum(-1)
        o[b] = torch.einsum("hl,lhd->hd", p * vsc.t(), V) / l.unsqueeze(-1)
        lse[b] = m[:, 0] + torch.log(l)
    return o, lse, (kb, ks, vb, vs)


EMU_MUTANTS = ("k scale not applied", "v scale from the wrong row", "new row attended unquantised")
