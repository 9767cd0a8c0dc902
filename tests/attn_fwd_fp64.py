"""fp64 restatement of `fat5_attn_fwd` in the dense (B, H, S, D) layout (the contract above `fat5_attn_params` in include/fat5.h), a
per-element error bound derived from the operation counts of the forward bodies, a float32 emulation of their arithmetic, and mutants:
restatements with one realistic defect each, which the bound must tell from the truth.  CPU only; imports no GPU code.  Used by
tests/test_attn_fwd_fp64_cpu.py and tests/test_attn_fwd_fp64_gpu.py.  Gradients and unit ranges are not covered; the packed (cu_seqlens)
layout is covered by tests/attn_packed_fp64.py, which calls this file per sequence.

The bound.  u = 2^-24 (fp32 unit roundoff); an addition inside an MFMA is charged 2 u = 2^-23 (its rounding mode is not documented: the
charge covers truncation); u_T = 2^-8 (bf16) / 2^-11 (fp16), the unit roundoff of the input dtype; ulp_T(r) the spacing of the storage dtype at |r|.  All scores in log2 units,
as in the kernels.  `body` is the `fwd=` field of fat5_attn_describe: 32row, 32row-split, 64row, 64row-ksplit, 64row-mixed.  Lines cited
as h:LINE (attn_fwd.h), h64:LINE (attn_fwd64.h), c:LINE (attn_common.h).  Per row, with A = (smag + bmag) log2e, rng = srange log2e,
nblk = ceil(N / 32) (a wave handles at most that many 32-key blocks):

  Score.  x_j = fma(s_j, c2, bias_j log2e) (h:255, h:275, h:286, h:344; h64:535, h64:598).  s_j = q . k_j accumulates D products in fp32
      on the matrix pipe (h:245, h64:1103): D additions, 2 D u relative to sum_i |q_i k_ji|.  c2 = scale * kLog2e (h:205, h64:426; c:29):
      the constant and the product, 2 u.  The bias in the exp2 domain: table entry * kLog2e (c:326) or bias_log2 (c:152), 2 u of bmag;
      a dense bias is exact in its 16 bits.  The FMA itself: u.  The reference point enters as the FMA's addend ad = add - m (h:339,
      h64:578) and x * mul + ad (h:344, h64:598): two roundings of at most u (|x| + |m|) <= 2 u A each.  Together
          ds <= (2 D + 9) u A.
      The reference point m itself need not be exact: the same stored m serves p, l and the result (h:11-14), so only ds enters:
          e_k = exp(ln2 ds) (1 + e_exp) - 1,   e_exp = 2^-23   (fast_exp2 = v_exp_f32, c:181: 1 ulp)
      v_exp_f32 flushes results below 2^-126: `attn_fwd_bound` asserts rng + log2 N + 6 < 120 (running maximum, stale by at most
      FAT5_DEFER_THR = 6, h:27; renormalisation h:392-404 moves m by at most log2 N beyond the maximum) and, for the 64-row bodies,
      whose bf16 sweep uses the reference point 0 (h64:16-23, h64:1071), A < 120.  Inside these ranges no weight is flushed.
  Rescales and merges.  alpha = exp2(m_old - m_new) (h:331, h64:583) multiplies l and O alike (h:332-336), at most once per block:
      it reweights the keys seen so far, e_exp + ln2 u (rng + 6) for the exponential of a rounded difference and 2 u for the products.
      The power-of-two renormalisation (h:397) is exact.  The split and key-split forms merge two partial states through LDS with two
      more such weights and an FMA each (h:486-494, h64:1153-1163): merges = 2 for 32row-split, 64row-ksplit, 64row-mixed, else 0.
          e_f = (nblk + merges) (e_exp + ln2 u (rng + 6) + 2 u)
      The exact second pass of a pipelined body (h:407-470, h64:1060-1194) is the running-maximum algorithm above: the same terms.
      (Inputs that force it are left to the max-norm tests: its flushed weights need a term of their own.)
  Sums.  l adds N weights in fp32 (h:349; h64:605-609; on the matrix pipe in the pipelined blocks, h64:271-275), O accumulates N
      products per element on the matrix pipe (h:355, h64:617), then the pair sum (h:498): e_sum = (N + nblk + 4) 2 u.
  P rounded for P.V.  pack8 / pack2 round p to the input dtype (h:353, c:66, c:681; h64:604, h64:614): |dp_j| <= u_T p_j, i.e.
      u_T absv on the numerator -- the leading term.  (The issue behind this file names u_T = 2^-9 / 2^-12; that is half the unit
      roundoff of a format with 8 / 11 significand bits: round-to-nearest of 1 + 2^-8 to bf16 errs by 2^-8 relative.  With the halved
      value `emulate` -- correct arithmetic -- left the bound by up to 1.35 on the 32-row cases.)  In the 64-row bodies the row sum adds the ROUNDED probabilities (h64:601-606,
      h64:782): the same u_T on the denominator and in lse.  The 32-row bodies sum the unrounded ones (h:349).
  fp16 underflow.  p is rounded relative to its reference point (running maximum, or the first tile's row maximum, h64:257-260,
      h64:1086); below 2^-14 fp16 is subnormal and the rounding error is absolute, 2^-25 per key.  The reference point is a score the
      row attains, so l >= 1 in its frame: 2^-25 sum_j |v_j| / l <= 2^-25 vsum on the numerator, N 2^-25 on the denominator.
  Result.  inv = 1 / l and O * inv (h:499, h:507): 3 u; one rounding to the storage dtype (pack2, h:507).  With
          e_num = e_k + e_f + e_sum + u_T + 3 u,   e_den = e_k + e_f + e_sum + [u_T: 64-row] + [N 2^-25: fp16]
          err_o <= (exp(e_num) / (1 - e_den) - 1) absv + [2^-25 vsum / (1 - e_den): fp16]
          |o - ref|   <= err_o + ulp_T(|ref| + err_o) / 2
          |lse - ref| <= -ln(1 - e_den) + 4 u |ref| + ln2 2^-23 (|ref| log2e + rng + log2 N + 6)
      (lse = (m + fast_log2(l)) * kLn2, h:511, h64:1223: v_log_f32 within 1 ulp of log2 l, |log2 l| <= |lse log2e - m|; the add, the
      constant kLn2 and the product: 4 u |ref|.)
No term is fitted to a measured error and there is no max(1, .) clamp: a row without a visible key has the bound 0 around o = 0, and
its lse = -inf is compared as a pattern.  A dense bias entry at or below -1e38 (finfo.min: the reference's additive mask) marks a masked
key: exp2 of it is exactly 0 in the kernels and here, and such keys are left out of bmag / srange.  A row whose visible keys are ALL
masked this way gets uniform weights in the kernels (the clamped entry absorbs the score, c:142-152) and here alike, so its o is bounded
like any other; its lse (about -2e38 in the kernels, the clamp; finfo.min here) is compared as a pattern: at or below -1e38.
"""
import math

import torch

from rowwise_fp64 import ulp

U32 = 2.0 ** -24
E_EXP = 2.0 ** -23
LOG2E = 1.0 / math.log(2.0)
LN2 = math.log(2.0)
U_T = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoff: 8 / 11 significand bits
MASKED = -1e38      # a dense bias entry at or below this is an additive mask
DEFER = 6.0         # FAT5_DEFER_THR
BODIES = ("32row", "32row-split", "64row", "64row-ksplit", "64row-mixed")


def _bias_block(c, bias, rpe1d, R, M, N):
    """the (M, N) fp64 additive term of (b, h) under the context's (possibly mutated) indexing, or None"""
    b, h = c["b"], c["h"]
    if bias is not None:
        bb = 0 if (bias.shape[0] == 1 or c["bias_b0"]) else b
        t = bias[bb, 0 if bias.shape[1] == 1 else h].double()
        if c["row_shift"]:
            t = t[(torch.arange(M) + c["row_shift"]).clamp(max=M - 1)]
        return t
    if rpe1d is not None:
        rel = torch.arange(N)[None, :] - torch.arange(M)[:, None] + c["shift"]
        return rpe1d[(h + c["head_shift"]) % rpe1d.shape[0]].double()[rel.clamp(-c["rclamp"], c["rclamp"]) + R]
    return None


def _visible(c, M, N):
    vis = torch.ones(M, N, dtype=torch.bool)
    if c["causal"]:
        vis = torch.arange(M)[:, None] + c["P"] + c["cshift"] >= torch.arange(N)[None, :]
    return vis


def attn_fwd_ref(q, k, v, sm_scale, causal, bias=None, rpe1d=None, R=0, mutant=None):
    """q (B, H, M, D), k / v (B, H, N, D) in bf16 / fp16 (any strides); bias dense (B|1, H|1, M, N) in q's dtype or None; rpe1d (H, 2R + 1)
    fp32 or None.  Returns a dict: o (B, H, M, D), lse (B, H, M), absv (B, H, M, D) = sum_j p_j |v_j|, vsum (B, H, M, D) = sum over the
    visible keys of |v_j|, smag / bmag / srange (B, H, M) in nats, nvis (B, H, M) visible-key counts, marker (B, H, M) rows all of whose
    visible keys carry a masking bias entry, applied (the mutant changed something).  `mutant` is one of MUTANTS' functions."""
    B, H, M, D = q.shape
    N = k.shape[2]
    scale = float(torch.tensor(float(sm_scale), dtype=torch.float32))   # (the ABI's field is a float)
    z3 = lambda: torch.zeros(B, H, M, dtype=torch.float64)
    out = dict(o=torch.zeros(B, H, M, D, dtype=torch.float64), lse=torch.full((B, H, M), -math.inf, dtype=torch.float64),
               absv=torch.zeros(B, H, M, D, dtype=torch.float64), vsum=torch.zeros(B, H, M, D, dtype=torch.float64),
               smag=z3(), bmag=z3(), srange=z3(), nvis=torch.zeros(B, H, M, dtype=torch.int64),
               marker=torch.zeros(B, H, M, dtype=torch.bool), applied=False)
    for b in range(B):
        for h in range(H):
            base = dict(b=b, h=h, B=B, H=H, M=M, N=N, R=R, causal=bool(causal), P=N - M, cshift=0, shift=0, rclamp=R, head_shift=0,
                        row_shift=0, bias_b0=False, w=torch.ones(N, dtype=torch.float64), ragged=False, lse_div=1.0, lse_nobias=False,
                        dead_finite=False, dense=bias is not None, rpe=rpe1d is not None)
            c = dict(base, w=base["w"].clone())
            if mutant is not None:
                mutant(c)
            qd, kd, vd = q[b, h].double(), k[b, h].double(), v[b, h].double()
            vis = _visible(c, M, N)
            qk = (qd @ kd.T) * scale
            bt = _bias_block(c, bias, rpe1d, R, M, N)
            s = qk if bt is None else qk + bt
            if mutant is not None:   # did the defect change anything a correct kernel would compute?
                vis0 = _visible(base, M, N)
                bt0 = _bias_block(base, bias, rpe1d, R, M, N)
                ch = bool((vis != vis0).any()) or bool(((c["w"] != 1)[None, :] & vis0).any())
                ch = ch or (bt is not None and bool(((bt != bt0) & vis0).any()))
                ch = ch or (c["ragged"] and M >= 2) or (c["lse_div"] != 1.0 and N > 0) or (c["lse_nobias"] and bt is not None)
                ch = ch or (c["dead_finite"] and bool((~vis0.any(-1)).any()))
                out["applied"] = out["applied"] or bool(ch)
            masked = (bt <= MASKED) & vis if (bt is not None and bias is not None) else torch.zeros_like(vis)
            live = vis & ~masked
            marker = vis.any(-1) & ~live.any(-1)
            eff = torch.where(marker[:, None], vis, live)           # the keys that carry weight
            sm = s.masked_fill(~vis, -math.inf)
            m = sm.amax(-1, keepdim=True) if N else torch.full((M, 1), -math.inf, dtype=torch.float64)
            m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            p = torch.exp(sm - m0) * c["w"][None, :]
            l = p.sum(-1, keepdim=True)
            pn = torch.where(l > 0, p / l, torch.zeros_like(p))
            o = pn @ vd
            s_l = sm if not (c["lse_nobias"] and bt is not None) else qk.masked_fill(~vis, -math.inf)
            if c["lse_nobias"] and bt is not None:
                lse = torch.logsumexp(s_l, -1) if N else torch.full((M,), -math.inf, dtype=torch.float64)
            else:
                lse = torch.where(l[:, 0] > 0, m0[:, 0] + torch.log(l[:, 0]), torch.full_like(l[:, 0], -math.inf))
            lse = torch.where(torch.isfinite(lse), lse / c["lse_div"], lse)
            if c["dead_finite"]:
                lse = torch.where(vis.any(-1), lse, torch.zeros_like(lse))
            if c["ragged"] and M >= 2:
                o[M - 1], lse[M - 1] = o[M - 2], lse[M - 2]
            out["o"][b, h], out["lse"][b, h] = o, lse
            out["absv"][b, h] = pn @ vd.abs()
            out["vsum"][b, h] = vis.double() @ vd.abs()
            out["nvis"][b, h], out["marker"][b, h] = vis.sum(-1), marker
            if N:
                zero = torch.zeros(M, N, dtype=torch.float64)
                out["smag"][b, h] = torch.where(eff & ~marker[:, None], (qd.abs() @ kd.abs().T) * abs(scale), zero).amax(-1)
                if bt is not None:
                    out["bmag"][b, h] = torch.where(live, bt.abs(), zero).amax(-1)
                out["srange"][b, h] = torch.where(live, m0 - s, zero).amax(-1)
    return out


def attn_fwd_bound(ref, dtype, D, body, N):
    """(bound_o (B, H, M, D), bound_lse (B, H, M)) for an `attn_fwd_ref` result computed by the forward body `body` at head dimension D"""
    assert body in BODIES, body
    row64, fp16 = body.startswith("64row"), dtype == torch.float16
    merges = 0 if body in ("32row", "64row") else 2
    uT = U_T[dtype]
    nblk = -(-N // 32)
    logn = math.log2(max(N, 2))
    A = (ref["smag"] + ref["bmag"]) * LOG2E
    rng = ref["srange"] * LOG2E
    assert float(rng.max()) + logn + DEFER < 120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    assert not row64 or float(A.max()) < 120.0, "the reference-point-0 sweep would flush a weight: outside the derivation"
    ds = (2 * D + 9) * U32 * A
    e_k = torch.exp(LN2 * ds) * (1 + E_EXP) - 1
    e_f = (nblk + merges) * (E_EXP + LN2 * U32 * (rng + DEFER) + 2 * U32)
    e_sum = (N + nblk + 4) * 2 * U32
    e_num = e_k + e_f + e_sum + uT + 3 * U32
    e_den = e_k + e_f + e_sum + (uT if row64 else 0.0) + (N * 2.0 ** -25 if fp16 else 0.0)
    err = ((torch.exp(e_num) / (1 - e_den)) - 1).unsqueeze(-1) * ref["absv"]
    if fp16:
        err = err + 2.0 ** -25 * ref["vsum"] / (1 - e_den).unsqueeze(-1)
    bo = err + 0.5 * ulp(ref["o"].abs() + err, dtype)
    lse = torch.where(torch.isfinite(ref["lse"]), ref["lse"], torch.zeros_like(ref["lse"])).abs()
    bl = -torch.log(1 - e_den) + 4 * U32 * lse + LN2 * 2.0 ** -23 * (lse * LOG2E + rng + logn + DEFER)
    dead = ref["nvis"] == 0
    return torch.where(dead.unsqueeze(-1), torch.zeros_like(bo), bo), torch.where(dead, torch.zeros_like(bl), bl)


def emulate(q, k, v, sm_scale, causal, bias=None, rpe1d=None, R=0, body="32row"):
    """What the kernels do arithmetically, in float32 torch ops: scores in fp32, p rounded to the dtype before P.V, row sums of the
    rounded p in the 64-row bodies, one output rounding.  Returns (o in q's dtype, lse fp32)."""
    B, H, M, D = q.shape
    N = k.shape[2]
    dtype = q.dtype
    o, lse = torch.zeros(B, H, M, D, dtype=dtype), torch.full((B, H, M), -math.inf)
    if N == 0:
        return o, lse
    vis = torch.ones(M, N, dtype=torch.bool)
    if causal:
        vis = torch.arange(M)[:, None] + (N - M) >= torch.arange(N)[None, :]
    for b in range(B):
        s = torch.einsum("hmd,hnd->hmn", q[b].float(), k[b].float()) * torch.tensor(float(sm_scale), dtype=torch.float32)
        if bias is not None:
            s = s + bias[0 if bias.shape[0] == 1 else b].float()   # ((1|H, M, N) broadcasts over the heads)
        elif rpe1d is not None:
            rel = (torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R
            s = s + rpe1d.float()[:, rel]
        s = s.masked_fill(~vis, -math.inf)
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = torch.exp(s - m)
        pr = p.to(dtype).float()
        l = (pr if body.startswith("64row") else p).sum(-1, keepdim=True)
        o[b] = torch.where(l > 0, (pr @ v[b].float()) / l, torch.zeros(())).to(dtype)
        lse[b] = torch.where(l[..., 0] > 0, m[..., 0] + torch.log(l[..., 0]), torch.full_like(l[..., 0], -math.inf))
    return o, lse


def ratios(o, lse, ref, bound_o, bound_lse):
    """(worst |o - ref| / bound, worst |lse - ref| / bound over the rows compared by value, the lse patterns agree).  The patterns: -inf
    exactly where the reference has it; at or below MASKED on the marker rows.  A non-finite o gives inf."""
    o, lse = o.double(), lse.double()
    eo = (o - ref["o"]).abs()
    ro = torch.where(eo == 0, torch.zeros_like(eo), eo / bound_o)   # (an exact result is within a bound of zero)
    ro = torch.where(torch.isfinite(o), ro, torch.full_like(ro, math.inf))
    fin, mk = torch.isfinite(ref["lse"]), ref["marker"]
    same = torch.equal(torch.isfinite(lse), fin) and bool((lse[~fin] == -math.inf).all()) and bool((lse[mk] <= MASKED).all())
    val = fin & ~mk
    el = (lse - ref["lse"]).abs()[val]
    rl = torch.where(el == 0, torch.zeros_like(el), el / bound_lse[val])
    rl = torch.where(torch.isfinite(lse[val]), rl, torch.full_like(rl, math.inf))
    return (float(ro.max()) if ro.numel() else 0.0), (float(rl.max()) if rl.numel() else 0.0), same


def within(o, lse, ref, bound_o, bound_lse):
    ro, rl, same = ratios(o, lse, ref, bound_o, bound_lse)
    return same and ro <= 1.0 and rl <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- mutants
# Each takes the per-(b, h) context of attn_fwd_ref and changes it the way the defect would; attn_fwd_ref reports whether that
# changed anything a correct kernel computes (`applied`).  Returns whether the defect exists at this shape at all.
def seam_key(N):
    """the first key of the second 32-key block of the last 64-key tile that has one: where the split and key-split forms change waves"""
    return 32 + 64 * ((N - 33) // 64) if N > 32 else None


def _drop(pos):
    def f(c):
        j = pos(c["N"])
        if j is None or not 0 <= j < c["N"]:
            return False
        c["w"][j] = 0
        return True
    return f


def _dup_block(c):
    j = seam_key(c["N"])
    if j is None:
        return False
    c["w"][j:min(c["N"], j + 32)] = 2
    return True


def _set(key, value, need=None):
    def f(c):
        if need is not None and not need(c):
            return False
        c[key] = value(c) if callable(value) else value
        return True
    return f


MUTANTS = {
    "drop key 0": _drop(lambda N: 0),
    "drop key N-1": _drop(lambda N: N - 1),
    "drop the last key of a ragged last tile": _drop(lambda N: N - 1 if N % 64 else None),
    "drop the first key of a tile's second block": _drop(seam_key),
    "count a 32-key block twice": _dup_block,
    "causal cut one key late": _set("cshift", 1, lambda c: c["causal"]),
    "causal cut one key early": _set("cshift", -1, lambda c: c["causal"]),
    "causal aligned top-left": _set("P", 0, lambda c: c["causal"] and c["M"] != c["N"]),
    "rpe index +1": _set("shift", 1, lambda c: c["rpe"]),
    "rpe index -1": _set("shift", -1, lambda c: c["rpe"]),
    "rpe clamped at R-1": _set("rclamp", lambda c: c["R"] - 1, lambda c: c["rpe"]),
    "rpe row of the neighbouring head": _set("head_shift", 1, lambda c: c["rpe"] and c["H"] > 1),
    "dense bias of row m+1": _set("row_shift", 1, lambda c: c["dense"]),
    "dense bias of batch 0": _set("bias_b0", True, lambda c: c["dense"] and c["B"] > 1),
    "last row of a ragged 64-row block from row M-2": _set("ragged", True, lambda c: c["M"] % 64 != 0 and c["M"] >= 2),
    "lse in log2 units": _set("lse_div", LN2),
    "lse without the bias": _set("lse_nobias", True, lambda c: c["dense"] or c["rpe"]),
    "fully masked row with a finite lse": _set("dead_finite", True, lambda c: c["causal"] and c["M"] > c["N"]),
}
