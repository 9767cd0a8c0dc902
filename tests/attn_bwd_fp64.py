"""fp64 restatement of `fat5_attn_bwd` in the dense (B, H, S, D) layout -- the FA2 backward from a GIVEN (o, lse), the contract of the
C ABI (include/fat5.h: o, lse and dout are inputs) --, a per-element error bound in units of each element's own term magnitudes, a
float32 emulation of the bodies' arithmetic, and mutants: restatements with one realistic defect each, which the bound must tell from
the truth.  CPU only; imports no GPU code.  Used by tests/test_attn_bwd_fp64_cpu.py and tests/test_attn_bwd_fp64_gpu.py.

Covered: the 32-wide bodies of csrc/attn_bwd.h (dq=32row, dkdv=32key) at every head dimension, as separate launches and in the
one-launch form (fused=1), with their bias gradients: dense dbias by the routes "direct", "staged" and "inkernel", drpe1d and the T5
table gradient in both reduction forms (dtable=runs / scan).
Not covered: the 64-wide bodies (dq=64row, 64row-batch4; dkdv=64key, 64key-half, 64key-mixed; their one-launch forms; qdiag=1; the
dbias routes "dq-kernel" and "dq-kernel+partials").  Their derivation (statistics as accumulator initial values, the bias on the matrix
pipe, the LDS merges, the diagonal sums of the pipelined steps) is not written: `attn_bwd_bound` raises for them, and the case list holds
none.  They stay with the max-norm tests (tests/test_bwd64_gpu.py, test_dense64_gpu.py, test_qdiag_gpu.py).  Also left to the existing
tests: the packed (cu_seqlens) layout, unit ranges, zero and negative sm_scale, head dimensions and dtypes the dispatcher rejects, the
forward, any timing.

The restatement.  Per (b, h), in fp64, from the given o and lse:  p = exp(s - lse) on visible keys, exact 0 elsewhere (a dense bias
entry <= -1e38 is a masked key; a row with lse < -1e30 -- kDeadRowLse, c:180: -inf, or the clamp of a fully masked row -- is dead: p, dS,
dq exact zeros);  delta = rowsum(o do);  dP = do v^T;  dS = p (dP - delta);  dv = p^T do;  dk = scale dS^T q;  dq = scale dS k;
dbias = dS summed over what the bias broadcasts;  drpe1d[h, r] = sum over the batch and the diagonal clamp(n - m, -R, R) = r - R of dS;
drpe_table[bucket, h] = drpe1d summed per bucket.  sm_scale is the float32 the ABI carries.

Term magnitudes.  a_ij = p_ij (sum_d |do_id v_jd| + |delta_i|) dominates |dS_ij|.  T_dv[j, d] = sum_i p_ij |do_id|,
T_dk[j, d] = |scale| sum_i a_ij |q_id|,  T_dq[i, d] = |scale| sum_j a_ij |k_jd|,  T of a dbias / drpe1d / table entry = the sum of a_ij over
what it reduces, with the count of terms.  Two companions of every T carry what is not a constant times a_ij:
  TA (a_ij replaced by a_ij A_i,  A_i = (smag_i + bmag_i + |lse_i|) log2e):  the error of the recomputed probability grows with A_i;
  TD (a_ij replaced by p_ij sum_d |o_id do_id|):  the rounding of delta is relative to sum_d |o_id do_id|, not to |delta_i|.
(The issue behind this file gives the bound the shape c T + ...; TA and TD are the two places where an honest c is not one number per
body.  With A_max the largest A_i, c T would need c >= A_max-dependent, a whole-tensor quantity.)

The bound.  u = 2^-24; an addition inside an MFMA is charged 2 u; u_T = 2^-8 / 2^-11; gamma_k(n) = k n u / (1 - k n u) the any-order
summation constant.  Lines cited as b:LINE (csrc/attn_bwd.h), c:LINE (attn_common.h), d:LINE (attn_bwd_dbias.h), r:LINE
(reduce_kernels.h), ds:LINE (diag_sum.h), api:LINE (fat5_api.hip).
  e_p, the recomputed probability.  dQ body: s = k . q accumulates D products on the matrix pipe (b:215), 2 D u of smag; one FMA
      x = fma(s, c2, bias2 + nL2) in front of v_exp_f32 (b:221, b:228, b:237-240, b:244): c2 = scale * kLog2e (b:181) 2 u, the table entry
      * kLog2e (c:326) or bias_log2 (c:152) 2 u of bmag, nL2 = -L * kLog2e (b:114) 2 u of |L|, the add bias2 + nL2 and the FMA u each of
      at most A.  dK/dV body: the accumulator starts at -L * (1 / scale) (b:538, b:548, b:636), so the D MFMA additions (b:643) are 2 D u of
      smag + |L|, the reciprocal and its product 2 u, then fma(s, c2, bias2) (b:662, b:672, b:690-693) or s * c2 (b:697).  Both:
          dx <= (2 D + 9) u A_i  in log2 units,   e_p = exp(ln2 dx) (1 + 2^-23) - 1   (fast_exp2 = v_exp_f32, c:181: 1 ulp)
      `attn_bwd_bound` asserts ln2 (2 D + 9) u A_i < 2^-7, so e_p a_ij <= [ln2 (2 D + 9) u (1 + 2^-23) / (1 - 2^-7)] A_i a_ij + 2^-23 a_ij:
      the first on TA, the second on T.  It also asserts (s - lse) log2e > -120 on the live keys: no weight is flushed by v_exp_f32.
  dS.  dP' = dO V^T - delta: the accumulator starts at -delta (b:179, b:216; b:648, b:655), D additions of at most
      sum_d |do v| + |delta|: 2 D u; the product p * dP' (b:221, b:247, b:663, b:702): u.  delta itself: an fmaf chain over this lane's half
      of the row and the pair sum (b:104-108), or in the one-launch form 8 fmaf and a butterfly over D / 8 lanes (b:573-581): at most
      D u sum_d |o do| (the products of two 16-bit values are exact in fp32) -- on TD.
  P and dS rounded to the input dtype before the contractions (pack8, b:260, b:723-724): u_T each -- the leading term.  fp16: below 2^-14
      the rounding is absolute, 2^-25 per term: 2^-25 times the sum of |do| (dv), |scale| |q| (dk), |scale| |k| (dq) over the live terms.
  Contractions.  dV^T += dO^T P, dK^T += Q^T dS over the M rows (b:755-756), dQ^T += K^T dS over the N keys (b:288), on the matrix
      pipe: gamma_2(M + 1) / gamma_2(N + 1); the scale afterwards (b:360, b:847): u; one rounding to the storage dtype (pack2).
          c_dv = (1 + u_T) (1 + 2^-23 + gamma_2(M + 1)) - 1
          c_dk = (1 + u_T) (1 + 2^-23 + (2 D + 1) u + gamma_2(M + 1) + u) - 1,   c_dq likewise with N
          err_X = c_X T_X + (1 + u_T) (c_A TA_X + D u TD_X) + [fp16: the absolute term],   |got - ref| <= err + ulp_T(|ref| + err) / 2
  dbias.  Every route of these bodies starts from the dS the dQ body (b:260-282) or the batch-inner kernel (d:193-198) has ROUNDED to
      the dtype.  "direct" (api:308): that rounded dS is dbias: err = e_dS T + ..., one rounding.  "staged" (api:306, r:53-72): the rounded
      dS of the nsum (batch, head) pairs are summed in fp32 and rounded once: u_T T + gamma_1(nsum) T (1 + u_T) (+ nsum 2^-25 in fp16).
      "inkernel" (d:192-198, d:226, d:240): the same, the fp32 sum passing through a scratch slab beyond four batch elements.
  drpe1d / table.  The 32-key body forms the diagonal sums from the fp32 dS, NOT the rounded one (b:730, b:736, b:742: `s`, before
      pack8): no u_T.  Band blocks add every element into U and the borrowed ones also into B, and take U - B (ds:50-59, ds:99): each term
      enters up to twice; then the carries, the wave sum (b:822), the per-wave arrays (b:833) and the partial rows (r:115-146, or r:192-217
      per bucket run): gamma_1(2 n + 8) for n terms.  Stored as fp32: no output rounding.
No constant is fitted to a measured error and nothing is put on top.  Where T = 0 (a dead row's dq, a dbias entry above the causal
diagonal or under a masking bias entry, a diagonal no visible score lies on) the bound is 0 and the kernels must give an exact zero.
"""
import math

import torch

from attn_fwd_fp64 import _bias_block, _visible, seam_key, U_T, U32, E_EXP, LOG2E, LN2, MASKED
from rowwise_fp64 import ulp

DEAD_LSE = -1.0e30          # kDeadRowLse
OUTPUTS = ("dq", "dk", "dv", "dbias", "drpe1d", "drpe_table")
DBIAS_ROUTES = ("direct", "staged", "inkernel")


def _gamma(n, k=1):
    x = k * n * U32
    return x / (1 - x)


def _knobs(B, H, M, N, D, R, causal, scale, bias, rpe1d, bucket):
    return dict(B=B, H=H, M=M, N=N, D=D, R=R, causal=bool(causal), P=N - M, cshift=0, shift=0, rclamp=R, head_shift=0, row_shift=0,
                bias_b0=False, dense=bias is not None, rpe=rpe1d is not None, table=bucket is not None, scale=scale,
                red_b=bias is not None and bias.shape[0] == 1 and B > 1, red_h=bias is not None and bias.shape[1] == 1 and H > 1,
                wq=torch.ones(N, dtype=torch.float64), wr=torch.ones(M, dtype=torch.float64), delta_shift=0, delta_true=False,
                own_softmax=False, dk_noscale=False, dq_scale2=False, db_drop=False, db_dup=False, db_above=False, db_row_shift=0,
                g_shift=0, g_far_band=False, g_head_shift=0, bucket_shift=0, ragged=False)


def _bias_all(c, bias, rpe1d, R, M, N):
    """(B|1, H, M, N) fp64 additive term under the context's indexing, or None (`_bias_block` of the forward file per (b, h))"""
    if bias is None and rpe1d is None:
        return None
    nb = 1 if rpe1d is not None else c["B"]
    return torch.stack([torch.stack([_bias_block(dict(c, b=b, h=h), bias, rpe1d, R, M, N) for h in range(c["H"])]) for b in range(nb)])


def attn_bwd_ref(q, k, v, o, lse, do, sm_scale, causal, bias=None, rpe1d=None, R=0, bucket=None, num_buckets=0, mutant=None):
    """q, o, do (B, H, M, D), k / v (B, H, N, D) in bf16 / fp16 (any strides); lse (B, H, M) fp32; bias dense (B|1, H|1, M, N) or None; rpe1d
    (H, 2R + 1) fp32 or None; bucket (2R + 1) int ids or None.  Returns a dict: for X in dq, dk, dv and, where they exist, dbias, drpe1d,
    drpe_table: X (fp64), T_X, TA_X, TD_X (see the module docstring; TA_dv / TD_dv: dv has no delta, TD_dv = 0); S_dv, S_dk, S_dq the fp16
    absolute-term sums; nsum (dbias) and n_drpe1d / n_drpe_table term counts; per row (B, H, M): smag, bmag, lse_abs, smax / smin (the
    extremes of s - lse over the live keys, 0 on rows without one), dsmax (the largest |dS_ij|), dead; applied (the mutant changed something
    a correct kernel computes)."""
    B, H, M, D = q.shape
    N = k.shape[2]
    scale = float(torch.tensor(float(sm_scale), dtype=torch.float32))   # (the ABI's field is a float)
    base = _knobs(B, H, M, N, D, R, causal, scale, bias, rpe1d, bucket)
    c = dict(base, wq=base["wq"].clone(), wr=base["wr"].clone())
    exists = True
    if mutant is not None:
        exists = bool(mutant(c))
    qd, kd, vd, od, dod = (t.double() for t in (q, k, v, o, do))
    kt, vt = kd.transpose(-1, -2), vd.transpose(-1, -2)
    vis = _visible(c, M, N)
    qk = (qd @ kt) * scale
    bt = _bias_all(c, bias, rpe1d, R, M, N)
    s = qk if bt is None else qk + bt
    masked = ((bt <= MASKED) & vis) if bias is not None else torch.zeros(1, 1, M, N, dtype=torch.bool)
    L = lse.double()
    dead = ~(L >= DEAD_LSE)
    ok = vis & ~masked & ~dead[..., None]                               # (B, H, M, N): the scores that carry weight
    ninf = torch.full_like(s, -math.inf)
    L_true = torch.logsumexp(torch.where(vis & ~masked, s, ninf), -1) if mutant is not None else None
    Lu = L_true if c["own_softmax"] else L
    L0 = torch.where(dead, torch.zeros_like(L), Lu)
    x = torch.where(ok, s - L0[..., None], ninf)
    p = torch.exp(x)
    if c["delta_true"]:
        od_true = torch.nan_to_num(torch.softmax(torch.where(vis & ~masked, s, ninf), -1)) @ vd
        delta = (od_true * dod).sum(-1)
    else:
        delta = (od * dod).sum(-1)
    if c["delta_shift"]:
        delta = delta[..., (torch.arange(M) + c["delta_shift"]).clamp(max=M - 1)]
    dP = dod @ vt
    dS = p * (dP - delta[..., None])
    a = p * (dod.abs() @ vt.abs() + delta.abs()[..., None])
    zero = torch.zeros_like(s)
    smag = torch.where(ok, (qd.abs() @ kt.abs()) * abs(scale), zero).amax(-1) if N else torch.zeros_like(L)
    bmag = torch.where(ok, bt.abs().expand_as(s), zero).amax(-1) if (bt is not None and N) else torch.zeros_like(L)
    A = (smag + bmag + L0.abs()) * LOG2E
    pd = p * (od.abs() * dod.abs()).sum(-1)[..., None]
    mags = (a, a * A[..., None], pd)                                    # -> T, TA, TD
    out = dict(smag=smag, bmag=bmag, lse_abs=L0.abs(), dead=dead, applied=False)
    anyok = ok.any(-1)
    out["smax"] = torch.where(anyok, x.amax(-1), torch.zeros_like(L)) if N else torch.zeros_like(L)
    out["smin"] = torch.where(anyok, torch.where(ok, x, -ninf).amin(-1), torch.zeros_like(L)) if N else torch.zeros_like(L)
    out["dsmax"] = dS.abs().amax(-1) if N else torch.zeros_like(L)
    okf = ok.double().expand_as(s)
    wr, wq = c["wr"][:, None], c["wq"][None, :]
    # ---- dv, dk, dq ----
    out["dv"] = (p * wr).transpose(-1, -2) @ dod
    out["T_dv"] = p.transpose(-1, -2) @ dod.abs()
    out["TA_dv"] = (p * A[..., None]).transpose(-1, -2) @ dod.abs()
    out["TD_dv"] = torch.zeros_like(out["T_dv"])
    out["S_dv"] = okf.transpose(-1, -2) @ dod.abs()
    out["dk"] = ((dS * wr).transpose(-1, -2) @ qd) * (1.0 if c["dk_noscale"] else scale)
    out["dq"] = ((dS * wq) @ kd) * (scale * scale if c["dq_scale2"] else scale)
    if c["ragged"] and M >= 2:
        out["dq"][:, :, M - 1] = out["dq"][:, :, M - 2]
    for tag, m in zip(("T", "TA", "TD"), mags):
        out[tag + "_dk"] = (m.transpose(-1, -2) @ qd.abs()) * abs(scale)
        out[tag + "_dq"] = (m @ kd.abs()) * abs(scale)
    out["S_dk"] = (okf.transpose(-1, -2) @ qd.abs()) * abs(scale)
    out["S_dq"] = (okf @ kd.abs()) * abs(scale)
    # ---- dbias ----
    if bias is not None:
        def red(t, mut=False):
            if bias.shape[0] == 1 and B > 1:
                w = torch.ones(B, dtype=torch.float64)
                if mut and c["db_drop"]:
                    w[B - 1] = 0
                if mut and c["db_dup"] and B > 4:
                    w[4] = 2
                t = (t * w[:, None, None, None]).sum(0, keepdim=True)
            if bias.shape[1] == 1 and H > 1:
                t = t.sum(1, keepdim=True)
            return t
        dsb = dS
        if c["db_row_shift"]:
            dsb = dS[:, :, (torch.arange(M) + c["db_row_shift"]).clamp(max=M - 1)]
        if c["db_above"]:
            dsb = torch.where(vis, dsb, dP - delta[..., None])
        out["dbias"] = red(dsb, True)
        for tag, m in zip(("T", "TA", "TD"), mags):
            out[tag + "_dbias"] = red(m)
        out["nsum"] = (B if bias.shape[0] == 1 else 1) * (H if bias.shape[1] == 1 else 1)
    # ---- drpe1d, drpe_table ----
    if rpe1d is not None:
        n1 = 2 * R + 1
        rel = torch.arange(N)[None, :] - torch.arange(M)[:, None]
        gidx = ((rel + c["g_shift"]).clamp(-R, R) + R).reshape(-1)
        wg = (rel.abs() <= R).double() if c["g_far_band"] else torch.ones(M, N, dtype=torch.float64)
        X = torch.stack([(dS * wg).sum(0)] + [m.sum(0) for m in mags])                   # (4, H, M, N), summed over the batch
        g = torch.zeros(4, H, n1, dtype=torch.float64).index_add_(2, gidx, X.reshape(4, H, -1))
        if c["g_head_shift"]:
            g[0] = g[0].roll(c["g_head_shift"], 0)
        cnt = torch.zeros(n1, dtype=torch.float64).index_add_(0, gidx, okf.sum((0, 1)).reshape(-1) / H)
        out["drpe1d"], out["T_drpe1d"], out["TA_drpe1d"], out["TD_drpe1d"], out["n_drpe1d"] = g[0], g[1], g[2], g[3], cnt
        if bucket is not None:
            bk0 = torch.as_tensor(bucket, dtype=torch.int64)
            bk = bk0[(torch.arange(n1) + c["bucket_shift"]).clamp(0, n1 - 1)]
            inr = (bk >= 0) & (bk < num_buckets)
            t = torch.zeros(4, num_buckets, H, dtype=torch.float64)
            t[0].index_add_(0, bk[inr], g[0].T[inr])
            inr0 = (bk0 >= 0) & (bk0 < num_buckets)
            t[1:].index_add_(1, bk0[inr0], g[1:].transpose(1, 2)[:, inr0])
            out["drpe_table"], out["T_drpe_table"], out["TA_drpe_table"], out["TD_drpe_table"] = t[0], t[1], t[2], t[3]
            out["n_drpe_table"] = torch.zeros(num_buckets, dtype=torch.float64).index_add_(0, bk0[inr0], cnt[inr0])[:, None].expand(num_buckets, H)
        out["n_drpe1d"] = cnt[None, :].expand(H, n1)
    if mutant is not None and exists:   # did the defect change anything a correct kernel would compute?
        vis0 = _visible(base, M, N)
        ok0 = vis0 & ~masked & ~dead[..., None]
        ch = bool(((vis != vis0) & ~masked & ~dead[..., None]).any())   # (a dead row stays dead whatever it is shown)
        if bt is not None:
            bt0 = _bias_all(base, bias, rpe1d, R, M, N)
            ch = ch or bool(((bt != bt0) & ok0).any())
        ch = ch or bool(((c["wq"] != 1)[None, :] & ok0).any()) or bool(((c["wr"] != 1)[:, None] & ok0).any())
        ch = ch or (c["delta_shift"] != 0 and bool(anyok[..., :M - 1].any()))
        ch = ch or (c["delta_true"] and float(((od_true - od).abs() * anyok[..., None]).max()) > 0.25)
        ch = ch or (c["own_softmax"] and float(torch.where(anyok, (L_true - L).abs(), torch.zeros_like(L)).max()) > 0.1)
        ch = ch or ((c["dk_noscale"] or c["dq_scale2"]) and scale != 1.0 and bool(ok0.any()))
        ch = ch or ((c["db_drop"] or c["db_dup"] or c["db_row_shift"] != 0) and bool(ok0.any()))
        ch = ch or (c["db_above"] and bool((~vis0).any()))
        ch = ch or (c["g_shift"] != 0 and bool(ok0.any())) or (c["g_head_shift"] != 0 and bool(ok0.any()))
        ch = ch or (c["g_far_band"] and bool(((torch.arange(N)[None, :] - torch.arange(M)[:, None]).abs() > R)[None, None].logical_and(ok0).any()))
        ch = ch or (c["bucket_shift"] != 0 and bool((bk != bk0).any()) and bool(ok0.any()))
        ch = ch or (c["ragged"] and M >= 2 and bool(anyok[:, :, M - 2:].any()))
        out["applied"] = bool(ch)
    return out


def outputs_of(ref):
    return [x for x in OUTPUTS if x in ref]


def attn_bwd_bound(ref, dtype, D, bodies, N, M):
    """{output: bound tensor} for an `attn_bwd_ref` result computed by the bodies `bodies` names (the dq=, dkdv=, fused=, dbias=, qdiag=,
    dtable= fields of fat5_attn_describe, as a dict) at head dimension D"""
    if bodies.get("dq") != "32row" or bodies.get("dkdv") != "32key" or bodies.get("qdiag", "0") != "0":
        raise NotImplementedError(f"not covered: {bodies} (the 64-wide bodies; see the module docstring)")
    fp16 = dtype == torch.float16
    uT = U_T[dtype]
    kap = LN2 * (2 * D + 9) * U32
    Amax = max(float((ref["smag"] + ref["bmag"] + ref["lse_abs"]).max()) * LOG2E, 0.0) if ref["smag"].numel() else 0.0
    assert kap * Amax < 2.0 ** -7, "scores beyond the range the derivation of e_p covers"
    assert float(ref["smin"].min() if ref["smin"].numel() else 0.0) * LOG2E > -120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    assert not fp16 or float(ref["dsmax"].max() if ref["dsmax"].numel() else 0.0) < 60000.0, "dS would overflow fp16: outside the derivation"
    cA = kap * (1 + E_EXP) / (1 - 2.0 ** -7)
    e_ds = E_EXP + (2 * D + 1) * U32

    def close(x, err):
        b = err + 0.5 * ulp(ref[x].abs() + err, dtype)
        return torch.where(ref["T_" + x] == 0, torch.zeros_like(b), b)

    out = {}
    for x, n, e in (("dv", M, E_EXP), ("dk", M, e_ds + U32), ("dq", N, e_ds + U32)):
        cT = (1 + uT) * (1 + e + _gamma(n + 1, 2)) - 1
        err = cT * ref["T_" + x] + (1 + uT) * (cA * ref["TA_" + x] + D * U32 * ref["TD_" + x])
        if fp16:
            err = err + 2.0 ** -25 * ref["S_" + x]
        out[x] = close(x, err)
    if "dbias" in ref:
        route = bodies.get("dbias")
        if route not in DBIAS_ROUTES:
            raise NotImplementedError(f"not covered: dbias={route}")
        T = ref["T_dbias"]
        err = e_ds * T + cA * ref["TA_dbias"] + D * U32 * ref["TD_dbias"]
        if route != "direct":
            ns = ref["nsum"]
            err = (1 + uT) * err + uT * T + _gamma(ns) * (1 + uT) * T + (ns * 2.0 ** -25 if fp16 else 0.0)
        out["dbias"] = close("dbias", err)
    for x in ("drpe1d", "drpe_table"):
        if x in ref:
            T = ref["T_" + x]
            err = e_ds * T + cA * ref["TA_" + x] + D * U32 * ref["TD_" + x]
            g = 2 * ref["n_" + x] + 8
            err = err + (g * U32 / (1 - g * U32)) * (T + err)
            out[x] = torch.where(T == 0, torch.zeros_like(err), err)
    return out


def emulate(q, k, v, o, lse, do, sm_scale, causal, bias=None, rpe1d=None, R=0, bucket=None, num_buckets=0, dbias_route="direct"):
    """What the 32-wide bodies do arithmetically, in float32 torch ops (not in their summation order): scores, p, delta, dP and dS in fp32;
    P and dS rounded to the dtype before the three contractions; dbias from the rounded dS (summed in fp32 and rounded once where the
    route reduces); the diagonal sums from the fp32 dS; one output rounding.  Returns {output: tensor}."""
    B, H, M, D = q.shape
    N = k.shape[2]
    dt = q.dtype
    f = lambda t: t.float()
    scale = torch.tensor(float(sm_scale), dtype=torch.float32)
    s = (f(q) @ f(k).transpose(-1, -2)) * scale
    vis = torch.ones(M, N, dtype=torch.bool)
    if causal:
        vis = torch.arange(M)[:, None] + (N - M) >= torch.arange(N)[None, :]
    rel = (torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R
    if bias is not None:
        s = s + f(bias)
        vis = vis & ~(bias <= MASKED)
    elif rpe1d is not None:
        s = s + f(rpe1d)[:, rel][None]
    L = f(lse)
    ok = vis & (L >= DEAD_LSE)[..., None]
    p = torch.where(ok, torch.exp(s - torch.where(L >= DEAD_LSE, L, torch.zeros(()))[..., None]), torch.zeros(()))
    delta = (f(o) * f(do)).sum(-1, keepdim=True)
    ds = p * (f(do) @ f(v).transpose(-1, -2) - delta)
    pr, dsr = f(p.to(dt)), f(ds.to(dt))
    out = dict(dv=(pr.transpose(-1, -2) @ f(do)).to(dt), dk=((dsr.transpose(-1, -2) @ f(q)) * scale).to(dt), dq=((dsr @ f(k)) * scale).to(dt))
    if bias is not None:
        t = dsr
        if bias.shape[0] == 1 and B > 1:
            t = t.sum(0, keepdim=True)
        if bias.shape[1] == 1 and H > 1:
            t = t.sum(1, keepdim=True)
        assert dbias_route in DBIAS_ROUTES and (dbias_route != "direct" or t is dsr)
        out["dbias"] = t.to(dt)
    if rpe1d is not None:
        n1 = 2 * R + 1
        g = torch.zeros(H, n1).index_add_(1, rel.reshape(-1), ds.sum(0).reshape(H, -1))
        out["drpe1d"] = g
        if bucket is not None:
            bk = torch.as_tensor(bucket, dtype=torch.int64)
            inr = (bk >= 0) & (bk < num_buckets)
            out["drpe_table"] = torch.zeros(num_buckets, H).index_add_(0, bk[inr], g.T[inr])
    return out


def ratios(got, ref, bound):
    """{output: worst |got - ref| / bound}.  An exact result is within a bound of zero; where the bound is zero anything but an exact
    zero gives inf, and so does a non-finite value."""
    res = {}
    for x, b in bound.items():
        if x not in got:
            continue
        g = got[x].double()
        e = (g - ref[x]).abs()
        r = torch.where(e == 0, torch.zeros_like(e), e / b)
        r = torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))
        res[x] = float(r.max()) if r.numel() else 0.0
    return res


def within(got, ref, bound):
    return all(r <= 1.0 for r in ratios(got, ref, bound).values())


# ---------------------------------------------------------------------------------------------------------------------- mutants
# Each takes the knobs of attn_bwd_ref and changes them the way the defect would; it returns whether the defect exists at this shape at
# all, and attn_bwd_ref reports whether it changed anything a correct kernel computes (`applied`).
def seam_row(M):
    """the first row of the second 32-row half of the last 64-row step that has one"""
    return seam_key(M)


def _w(which, pos, value=0.0, width=1):
    def f(c):
        n = c["N"] if which == "wq" else c["M"]
        j = pos(n)
        if j is None or not 0 <= j < n:
            return False
        c[which][j:min(n, j + width)] = value
        return True
    return f


def _set(key, value, need=None):
    def f(c):
        if need is not None and not need(c):
            return False
        c[key] = value(c) if callable(value) else value
        return True
    return f


MUTANTS = {
    "dK/dV without query row 0": _w("wr", lambda M: 0),
    "dK/dV without query row M-1": _w("wr", lambda M: M - 1),
    "dK/dV without the first row of a step's second half": _w("wr", seam_row),
    "dK/dV with a 32-row step counted twice": _w("wr", seam_row, 2.0, 32),
    "dQ without key 0": _w("wq", lambda N: 0),
    "dQ without key N-1": _w("wq", lambda N: N - 1),
    "dQ without the seam key": _w("wq", seam_key),
    "dQ without the last key of a ragged last tile": _w("wq", lambda N: N - 1 if N % 64 else None),
    "dQ with a 32-key block counted twice": _w("wq", seam_key, 2.0, 32),
    "causal cut one key late": _set("cshift", 1, lambda c: c["causal"]),
    "causal cut one key early": _set("cshift", -1, lambda c: c["causal"]),
    "causal aligned top-left": _set("P", 0, lambda c: c["causal"] and c["M"] != c["N"]),
    "rpe index +1": _set("shift", 1, lambda c: c["rpe"]),
    "rpe index -1": _set("shift", -1, lambda c: c["rpe"]),
    "rpe clamped at R-1": _set("rclamp", lambda c: c["R"] - 1, lambda c: c["rpe"]),
    "rpe row of the neighbouring head": _set("head_shift", 1, lambda c: c["rpe"] and c["H"] > 1),
    "dense bias of row m+1": _set("row_shift", 1, lambda c: c["dense"]),
    "dense bias of batch 0": _set("bias_b0", True, lambda c: c["dense"] and c["B"] > 1),
    "delta of row m+1": _set("delta_shift", 1, lambda c: c["M"] >= 2),
    "delta from the fp64-true o": _set("delta_true", True),
    "p from a softmax of its own": _set("own_softmax", True),
    "dk without the scale": _set("dk_noscale", True),
    "dq with the scale squared": _set("dq_scale2", True),
    "dbias without a batch element": _set("db_drop", True, lambda c: c["red_b"]),
    "dbias with batch element 4 counted twice": _set("db_dup", True, lambda c: c["red_b"] and c["B"] > 4),
    "dbias nonzero above the causal diagonal": _set("db_above", True, lambda c: c["dense"] and c["causal"]),
    "dbias from dS of row m+1": _set("db_row_shift", 1, lambda c: c["dense"] and c["M"] >= 2),
    "drpe1d diagonal index +1": _set("g_shift", 1, lambda c: c["rpe"]),
    "drpe1d diagonal index -1": _set("g_shift", -1, lambda c: c["rpe"]),
    "drpe1d far entries without what lies beyond the band": _set("g_far_band", True, lambda c: c["rpe"]),
    "drpe1d of the neighbouring head": _set("g_head_shift", 1, lambda c: c["rpe"] and c["H"] > 1),
    "table gradient with a bucket boundary one entry off": _set("bucket_shift", 1, lambda c: c["table"]),
    "last row of a ragged 64-row block from row M-2": _set("ragged", True, lambda c: c["M"] % 64 != 0 and c["M"] >= 2),
}
