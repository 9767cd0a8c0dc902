"""fp64 restatement of local (sliding-window) attention -- `fat5_attn_local_fwd` and `fat5_attn_local_bwd`, the backward from a GIVEN
(o, lse) as the C ABI has it --, a per-element error bound derived from the operation counts of csrc/local_attn_kernels.h, a float32
emulation of the kernels' arithmetic, the host restatement `steps` of their step selection, the shared case list, and mutants:
restatements with one realistic defect each, which the bound must tell from the truth.  CPU only; imports no GPU code.  Used by
tests/test_local_attn_fp64_cpu.py and tests/test_local_attn_fp64_gpu.py.

Layout.  Every case is a list of sequences (a dense (B, H, S, D) batch is B sequences of length S); tensors are "flat": q, k, v, do, o,
dq, dk, dv (total, H, D), lse (H, total), drpe1d (H, 2 R + 1) -- the packed layout of the kernels; the GPU test views a dense case as
(B, H, S, D).

The restatement.  Per sequence and head, in fp64: key n is visible to row m iff |n - m| <= window, both inside the sequence; scores
s = scale q . k + rpe1d[h, clamp(n - m, -R, R) + R]; o, lse the softmax over the visible keys with the companions of attn_fwd_fp64.py
(absv, vsum, smag, bmag, srange, nvis).  Backward from the given (o, lse, do): p = exp(s - lse) on the visible keys, delta = rowsum(o do),
dS = p (do v^T - delta), dv = p^T do, dk = scale dS^T q, dq = scale dS k, drpe1d[h, r] = the sum over the batch and the diagonals
clamp(n - m, -R, R) = r - R of dS over the visible pairs; with the term magnitudes T, TA, TD, the fp16 sums S and the per-entry term
counts of attn_bwd_fp64.py.  An entry no visible pair reaches has T = 0: an exact zero with bound 0.

The bound.  u = 2^-24, an addition inside an MFMA 2 u, u_T = 2^-8 / 2^-11, gamma_k(n) = k n u / (1 - k n u).  Lines cited as L:LINE
(csrc/local_attn_kernels.h).  Per sequence w = min(window, L) (L:141); a wave's 32 own rows meet at most
nblk = min(ceil((2 w + 63) / 32) + 1, ceil(L / 32)) 32-row steps of the streamed side (L:108, L:155: the band of 32 rows spans
2 w + 32 positions, which touch at most that many aligned steps), n = 32 nblk terms on the matrix pipe per output element.
  Score (forward L:173-174, L:92-95; dQ L:276, L:279; dK/dV L:387, L:390).  s = k . q accumulates D products from zero: 2 D u of smag;
      c2 = scale * kLog2e (L:159) 2 u and the product s * c2 (L:92) u; the table entry * kLog2e (L:70) 2 u of bmag and the add (L:95) u.
      Forward: s - ref (L:186) one rounding of at most u (|x| + |m|) <= 2 u A.  Backward: lse2 = lse * kLog2e is ONE product (L:248;
      the dK/dV body's stat * stat_mul, L:365) -- the constant and the product 2 u of |lse| -- and x - lse2 (L:281, L:394) u.  Both at
      most (2 D + 9) u A in log2 units, A = (smag + bmag [+ |lse|]) log2e: the constant of attn_fwd_fp64.py ("Score") and of
      attn_bwd_fp64.py ("e_p") -- so e_k, kap and c_A are theirs.  fast_exp2: 1 ulp, 2^-23; no weight is flushed while
      rng + log2 n < 120 (forward) and (s - lse) log2e > -120 (backward): asserted.
  Forward reference point.  The plain running maximum, with a rescale at EVERY visited step (L:175-183): no deferral, so the DEFER term
      of attn_fwd_fp64.py drops out and there is no merge: e_f = nblk (2^-23 + ln2 u rng + 2 u).  l sums the UNROUNDED p (L:187), 16
      per step and lane, then the pair sum (L:197); O accumulates n products on the matrix pipe (L:193): e_sum = (n + nblk + 4) 2 u
      as there.  p is rounded to the dtype for P.V (pack8, L:191): u_T absv on the numerator only; fp16: 2^-25 vsum, and nothing on the
      denominator (l never sees the rounded p).  1 / l and the product (L:199) 3 u, one rounding to the storage dtype.
          e_num = e_k + e_f + e_sum + u_T + 3 u,   e_den = e_k + e_f + e_sum
          |o - ref| <= err_o + ulp_T(|ref| + err_o) / 2,  err_o = (exp(e_num) / (1 - e_den) - 1) absv + [fp16: 2^-25 vsum / (1 - e_den)]
          |lse - ref| <= -ln(1 - e_den) + 4 u |ref| + ln2 2^-23 (|ref| log2e + rng + log2 n)     (L:200, as attn_fwd_fp64.py "Result")
  delta (L:237-247).  The lane's chain over its 32 elements -- the products of two 16-bit values are exact in fp32 -- and `pair_sum`:
      at most 33 additions, charged D u sum |o do| on TD as in attn_bwd_fp64.py.
  dS.  dP accumulates D products from ZERO (L:278, L:389): 2 D u; then dp - delta in fp32 AFTER the MFMA (L:281; the dK/dV body reads
      lse and delta from LDS, L:394-395: they are not accumulator initial values): u of at most sum |do v| + |delta|; the product u:
      e_dS = 2^-23 + (2 D + 2) u  (one u more than the 32-wide bodies, whose accumulator starts at -delta).
  P and dS rounded to the dtype before the second contractions (pack8, L:284, L:399): u_T each; fp16 2^-25 absolute per term (S_X).
  Contractions over the visited steps on the matrix pipe (L:286, L:402-403): gamma_2(n + 1); * scale (L:318, L:409) u; one rounding.
          c_dv = (1 + u_T) (1 + 2^-23 + gamma_2(n + 1)) - 1,   c_dk = c_dq = (1 + u_T) (1 + e_dS + gamma_2(n + 1) + u) - 1
          err_X = c_X T_X + (1 + u_T) (c_A TA_X + D u TD_X) + [fp16: 2^-25 S_X],   |got - ref| <= err + ulp_T(|ref| + err) / 2
  drpe1d.  The diagonal sums take the fp32 dS (`s` before pack8 is read again at L:294): no u_T.  A term passes through: the lane's sum
      over a step's diagonal (L:300, at most 31 additions), the wave-private row once per visited step (L:304, nblk), for the clamp
      ends one `wave_sum` (L:307, L:311: at most 63) and its add (L:308, L:312), wave 0 + wave 1 (L:322) and `local_drpe_reduce_kernel`
      over (b, block) (L:422-425: B n_blk): depth = 32 + nblk + 64 + 1 + B n_blk additions.  Masked entries and rows past L hold exact
      zeros (p = exp2(-inf) = 0, L:97, L:281), which add without rounding, so an entry of cnt terms sees at most cnt - 1 rounding
      additions whatever the order: gamma_1(min(cnt, depth)).  Stored as fp32: no output rounding.
          err = e_dS T + c_A TA + D u TD,   |got - ref| <= err + gamma_1(min(cnt, depth)) (T + err)
No constant is fitted to a measured error and nothing is put on top.
"""
import math

import numpy as np
import torch

from attn_fwd_fp64 import U32, E_EXP, U_T, LOG2E, LN2
from attn_bwd_fp64 import _gamma, ratios  # noqa: F401  (`ratios` is the tests' per-element comparison)
from rowwise_fp64 import ulp

D = 64
H = 2
BOOST = 32.0
FWD, BWD = ("o", "lse"), ("dq", "dk", "dv", "drpe1d")
TILE, SCRATCH = 64 * 64 * 2, 32 * 33 * 4


def local_smem_q(wc, diag):
    """`local_smem_q` (L:45-47) restated: the dQ kernel's dynamic LDS bytes"""
    return 2 * TILE + (2 * wc + 1) * 4 * (3 if diag else 1) + (2 * SCRATCH if diag else 0) + 16


# ------------------------------------------------------------------------------------------------------------------- step selection
def _pairs(r0, sb, w, L):
    m, n = np.arange(r0, min(r0 + 32, L)), np.arange(sb, min(sb + 32, L))
    return int((np.abs(n[None, :] - m[:, None]) <= w).sum()) if len(m) and len(n) else 0


def steps(L, window, block):
    """`local_skip`, `local_full` and t_begin / t_end (L:108-109, L:155) on the host, for the 64-row block `block` of a sequence of
    length L: None where the block exits (m0 >= L, L:140), else dict(m0, t_begin, t_end, left / right = the whole tiles of the sequence
    it does not stream on either side, waves = [dict(r0, visited, full, masked, corner, skipped)] with lists of step offsets sb:
    visited = not skipped, full = mask-free, masked = visited and not full, corner = visited with exactly one visible pair, skipped =
    skipped inside a streamed tile).  The three kernels share these functions and they are symmetric in (own, streamed)."""
    m0 = 64 * block
    if m0 >= L:
        return None
    w = min(window, L)
    tb, te = max(0, m0 - w) // 64, min(L - 1, m0 + 63 + w) // 64
    waves = []
    for wv in (0, 1):
        r0 = m0 + 32 * wv
        d = dict(r0=r0, visited=[], full=[], masked=[], corner=[], skipped=[])
        for t in range(tb, te + 1):
            for blk in (0, 1):
                sb = 64 * t + 32 * blk
                if r0 >= L or sb >= L or sb > r0 + 31 + w or sb + 31 < r0 - w:
                    d["skipped"].append(sb)
                    continue
                d["visited"].append(sb)
                if sb + 31 - r0 <= w and r0 + 31 - sb <= w and sb + 31 < L and r0 + 31 < L:
                    d["full"].append(sb)
                else:
                    d["masked"].append(sb)
                    if _pairs(r0, sb, w, L) == 1:
                        d["corner"].append(sb)
        waves.append(d)
    return dict(m0=m0, t_begin=tb, t_end=te, left=tb, right=(L - 1) // 64 - te, waves=waves)


def all_steps(L, window):
    return [s for s in (steps(L, window, b) for b in range((L + 63) // 64)) if s is not None]


def nblk_of(L, window):
    w = min(window, L)
    return max(1, min((2 * w + 63 + 31) // 32 + 1, (L + 31) // 32))


# ------------------------------------------------------------------------------------------------------------------- restatement
def _knobs(**kw):
    c = dict(rs=0, ls=0, pw=None, vis_or=None, ext=None, global_pos=False, shift=0, rclamp=None, head_shift=0, lse_mul=1.0,
             lse_in_mul=1.0, delta_shift=0, g_noends=False, g_plus_minus=False, grow=None, g_shift=0)
    c.update(kw)
    return c


def _seq(c, q, k, v, rpe, R, scale, do=None, o=None, lse=None):
    """one sequence, all heads: q, k, v, do, o (H, L, D) fp64, lse (H, L) fp64; returns the forward (do is None) or backward fields"""
    Hh, L, _ = q.shape
    w = min(c["window"], L)
    m = torch.arange(L)
    n, kk, vv = m, k, v
    if c["ext"] is not None:                                            # keys the defect shows beyond the sequence: (positions, k, v)
        n, kk, vv = torch.cat([m, c["ext"][0]]), torch.cat([k, c["ext"][1]], 1), torch.cat([v, c["ext"][2]], 1)
    d = n[None, :] - m[:, None]
    vis = (d <= w + c["rs"]) & (d >= -(w + c["ls"]))
    if c["vis_or"] is not None:
        vis[:, :L] |= c["vis_or"]
    if c["global_pos"]:
        vis &= ((c["tok0"] + n)[None, :] < L) & ((c["tok0"] + m)[:, None] < L)
    s = (q @ kk.transpose(-1, -2)) * scale
    bt = None
    if rpe is not None:
        rc = R if c["rclamp"] is None else c["rclamp"]
        hh = (torch.arange(Hh) + c["head_shift"]) % Hh
        bt = rpe.double()[hh][:, (d + c["shift"]).clamp(-rc, rc) + R]
        s = s + bt
    zero, ninf = torch.zeros_like(s), torch.full_like(s, -math.inf)
    smag = torch.where(vis, (q.abs() @ kk.abs().transpose(-1, -2)) * abs(scale), zero).amax(-1)
    bmag = torch.where(vis, bt.abs(), zero).amax(-1) if bt is not None else torch.zeros_like(smag)
    pw = torch.ones(L, len(n), dtype=torch.float64)
    if c["pw"] is not None:
        pw[:, :L] = c["pw"]
    if do is None:
        sm = torch.where(vis, s, ninf)
        mx = sm.amax(-1, keepdim=True)
        mx0 = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        p = torch.exp(sm - mx0) * pw
        l = p.sum(-1, keepdim=True)
        pn = torch.where(l > 0, p / l, zero)
        lse_ = torch.where(l[..., 0] > 0, (mx0[..., 0] + torch.log(l[..., 0])) * c["lse_mul"], ninf[..., 0])
        return dict(o=pn @ vv, lse=lse_, absv=pn @ vv.abs(), vsum=vis.double() @ vv.abs(), smag=smag, bmag=bmag,
                    srange=torch.where(vis, mx0 - s, zero).amax(-1), nvis=vis.sum(-1)[None].expand(Hh, L))
    Lu = lse * c["lse_in_mul"]
    x = torch.where(vis, s - Lu[..., None], ninf)
    p = torch.exp(x)
    delta = (o * do).sum(-1)
    if c["delta_shift"]:
        delta = delta[:, (m + c["delta_shift"]).clamp(max=L - 1)]
    dP = do @ vv.transpose(-1, -2)
    dS = p * (dP - delta[..., None])
    a = p * (do.abs() @ vv.abs().transpose(-1, -2) + delta.abs()[..., None])
    A = (smag + bmag + lse.abs()) * LOG2E
    pd = p * (o.abs() * do.abs()).sum(-1)[..., None]
    visf = vis.double()[None].expand_as(s)
    tr = lambda t: t[..., :L].transpose(-1, -2)
    pwk = pw[:, :L].T[None]                                             # (the step selection is symmetric: the dK/dV body's view of it)
    out = dict(dq=((dS * pw) @ kk) * scale, dk=(tr(dS) * pwk @ q) * scale, dv=tr(p) * pwk @ do, smag=smag, bmag=bmag,
               smin=torch.where(vis, x, -ninf).amin(-1), dsmax=dS.abs().amax(-1), A=A)
    out["T_dv"], out["TA_dv"], out["S_dv"] = tr(p) @ do.abs(), tr(p * A[..., None]) @ do.abs(), tr(visf) @ do.abs()
    out["TD_dv"] = torch.zeros_like(out["T_dv"])
    for tag, mg in (("T", a), ("TA", a * A[..., None]), ("TD", pd), ("S", visf)):
        out[tag + "_dk"] = (tr(mg) @ q.abs()) * abs(scale)
        out[tag + "_dq"] = (mg @ kk.abs()) * abs(scale)
    if rpe is not None:
        n1, wc = 2 * R + 1, min(c["window"], R)
        gidx = ((d + c["g_shift"]).clamp(-R, R) + R).reshape(-1)
        gw = pw if c["grow"] is None else pw * c["grow"][:, None]
        if c["g_noends"]:
            gw = gw * (d.abs() <= wc).double()
        X = torch.stack([dS * gw, a, a * A[..., None], pd])
        g = torch.zeros(4, Hh, n1, dtype=torch.float64).index_add_(2, gidx, X.reshape(4, Hh, -1))
        out["drpe1d"], out["T_drpe1d"], out["TA_drpe1d"], out["TD_drpe1d"] = g[0], g[1], g[2], g[3]
        out["n_drpe1d"] = torch.zeros(n1, dtype=torch.float64).index_add_(0, gidx, vis.double().reshape(-1))[None].expand(Hh, n1)
    return out


def _seqs(case):
    lens = case["lens"]
    cu = [0]
    for x in lens:
        cu.append(cu[-1] + x)
    return cu


def local_ref(case, t, mutant=None, given=None):
    """The restatement of a case on its inputs `t` (`inputs`): the forward fields, and from given = (o (total, H, D), lse (H, total)) --
    default: this forward's o rounded to the dtype and its lse as fp32 -- the backward fields.  `mutant`: one of MUTANTS' functions;
    `exists` then says whether the defect exists in the case at all."""
    lens, R, scale = case["lens"], case["R"], float(torch.tensor(case["scale"], dtype=torch.float32))
    cu, B = _seqs(case), len(case["lens"])
    rpe = t["rpe"] if R else None
    total = cu[-1]
    sl = lambda x, b: x[cu[b]:cu[b + 1]].double().transpose(0, 1)        # (H, L, D)
    live = [b for b in range(B) if lens[b] > 0]
    ctxs, exists = [], mutant is None
    for b in range(B):
        nx = next((b2 for b2 in range(b + 1, B) if lens[b2] > 0), None)
        c = _knobs(window=case["window"], R=R, wc=min(case["window"], R), b=b, B=B, L=lens[b], tok0=cu[b], b_last=live[-1], H=H,
                   packed=case["packed"], nxt=None if nx is None else (t["k"][cu[nx]].double(), t["v"][cu[nx]].double()))
        if mutant is not None and lens[b] > 0:
            exists = bool(mutant(c)) or exists
        ctxs.append(c)
    out = dict(exists=exists)
    fw = [_seq(ctxs[b], sl(t["q"], b), sl(t["k"], b), sl(t["v"], b), rpe, R, scale) for b in live]
    for x in ("o", "lse", "absv", "vsum", "smag", "bmag", "srange", "nvis"):
        out[x] = torch.cat([f[x] for f in fw], 1).transpose(0, 1) if fw[0][x].dim() == 3 else torch.cat([f[x] for f in fw], 1)
    if given is None:
        given = (out["o"].to(case["dtype"]), out["lse"].float())
    og, lg = given
    bw = [_seq(ctxs[b], sl(t["q"], b), sl(t["k"], b), sl(t["v"], b), rpe, R, scale, do=sl(t["do"], b), o=sl(og, b),
               lse=lg[:, cu[b]:cu[b + 1]].double()) for b in live]
    for x in bw[0]:
        if x.endswith("drpe1d"):
            out[x] = sum(f[x] for f in bw)
        elif bw[0][x].dim() == 3:
            out[x] = torch.cat([f[x] for f in bw], 1).transpose(0, 1)
        else:
            out[x] = torch.cat([f[x] for f in bw], 1)
    if R and mutant is not None and any(c["g_plus_minus"] for c in ctxs):
        wc = min(case["window"], R)
        out["drpe1d"] = out["drpe1d"].clone()
        out["drpe1d"][:, R + wc] += out["drpe1d"][:, R - wc]
    assert out["o"].shape[0] == total
    return out, given


def local_bound(case, ref):
    """{output: bound} of a `local_ref` result (see the module docstring)"""
    dtype, lens = case["dtype"], [x for x in case["lens"] if x > 0]
    fp16, uT = dtype == torch.float16, U_T[dtype]
    nblk = max(nblk_of(L, case["window"]) for L in lens)
    n = 32 * nblk
    logn = math.log2(n)
    # ---- forward
    A = (ref["smag"] + ref["bmag"]) * LOG2E
    rng = ref["srange"] * LOG2E
    assert float(rng.max()) + logn < 120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    e_k = torch.exp(LN2 * (2 * D + 9) * U32 * A) * (1 + E_EXP) - 1
    e_f = nblk * (E_EXP + LN2 * U32 * rng + 2 * U32)
    e_sum = (n + nblk + 4) * 2 * U32
    e_num, e_den = e_k + e_f + e_sum + uT + 3 * U32, e_k + e_f + e_sum
    tk = lambda x: x.transpose(0, 1).unsqueeze(-1)                       # (H, total) -> (total, H, 1)
    err = tk(torch.exp(e_num) / (1 - e_den) - 1) * ref["absv"]
    if fp16:
        err = err + 2.0 ** -25 * ref["vsum"] / tk(1 - e_den)
    out = dict(o=err + 0.5 * ulp(ref["o"].abs() + err, dtype))
    la = ref["lse"].abs()
    out["lse"] = -torch.log(1 - e_den) + 4 * U32 * la + LN2 * 2.0 ** -23 * (la * LOG2E + rng + logn)
    # ---- backward
    kap = LN2 * (2 * D + 9) * U32
    assert kap * float(ref["A"].max()) < 2.0 ** -7, "scores beyond the range the derivation of e_p covers"
    assert float(ref["smin"].min()) * LOG2E > -120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    assert not fp16 or float(ref["dsmax"].max()) < 60000.0, "dS would overflow fp16: outside the derivation"
    cA = kap * (1 + E_EXP) / (1 - 2.0 ** -7)
    e_ds = E_EXP + (2 * D + 2) * U32
    for x, e in (("dv", E_EXP), ("dk", e_ds + U32), ("dq", e_ds + U32)):
        cT = (1 + uT) * (1 + e + _gamma(n + 1, 2)) - 1
        err = cT * ref["T_" + x] + (1 + uT) * (cA * ref["TA_" + x] + D * U32 * ref["TD_" + x])
        if fp16:
            err = err + 2.0 ** -25 * ref["S_" + x]
        b = err + 0.5 * ulp(ref[x].abs() + err, dtype)
        out[x] = torch.where(ref["T_" + x] == 0, torch.zeros_like(b), b)
    if "drpe1d" in ref:
        T = ref["T_drpe1d"]
        err = e_ds * T + cA * ref["TA_drpe1d"] + D * U32 * ref["TD_drpe1d"]
        depth = 32 + nblk + 64 + 1 + len(case["lens"]) * ((case["S"] + 63) // 64)
        g = torch.minimum(ref["n_drpe1d"], torch.full_like(T, float(depth))) * U32
        err = err + g / (1 - g) * (T + err)
        out["drpe1d"] = torch.where(T == 0, torch.zeros_like(err), err)
    return out


def emulate(case, t, given):
    """What the kernels do arithmetically, in float32 torch ops (not in their summation order): fp32 scores, the forward's p rounded to
    the dtype before P.V with l from the unrounded p; the backward's P and dS rounded before the second contractions, the diagonal
    sums from the fp32 dS; one output rounding.  Returns {output: flat tensor}."""
    dt, R, cu = case["dtype"], case["R"], _seqs(case)
    scale = torch.tensor(float(case["scale"]), dtype=torch.float32)
    total = cu[-1]
    res = dict(o=torch.zeros(total, H, D, dtype=dt), lse=torch.zeros(H, total), dq=torch.zeros(total, H, D, dtype=dt),
               dk=torch.zeros(total, H, D, dtype=dt), dv=torch.zeros(total, H, D, dtype=dt))
    if R:
        res["drpe1d"] = torch.zeros(H, 2 * R + 1)
    f = lambda x, b: x[cu[b]:cu[b + 1]].float().transpose(0, 1)
    for b, L in enumerate(case["lens"]):
        if L == 0:
            continue
        q, k, v, do, o = [f(t[x], b) for x in ("q", "k", "v", "do")] + [f(given[0], b)]
        lse = given[1][:, cu[b]:cu[b + 1]].float()
        pos = torch.arange(L)
        d = pos[None, :] - pos[:, None]
        vis = d.abs() <= min(case["window"], L)
        s = (q @ k.transpose(-1, -2)) * scale
        idx = d.clamp(-R, R) + R
        if R:
            s = s + t["rpe"].float()[:, idx]
        sm = s.masked_fill(~vis, -math.inf)
        mx = sm.amax(-1, keepdim=True)
        p = torch.exp(sm - mx)
        l = p.sum(-1, keepdim=True)
        sel = slice(cu[b], cu[b + 1])
        res["o"][sel] = ((p.to(dt).float() @ v) / l).to(dt).transpose(0, 1)
        res["lse"][:, sel] = mx[..., 0] + torch.log(l[..., 0])
        p = torch.where(vis, torch.exp(s - lse[..., None]), torch.zeros(()))
        delta = (o * do).sum(-1, keepdim=True)
        ds = p * (do @ v.transpose(-1, -2) - delta)
        pr, dsr = p.to(dt).float(), ds.to(dt).float()
        res["dv"][sel] = (pr.transpose(-1, -2) @ do).to(dt).transpose(0, 1)
        res["dk"][sel] = ((dsr.transpose(-1, -2) @ q) * scale).to(dt).transpose(0, 1)
        res["dq"][sel] = ((dsr @ k) * scale).to(dt).transpose(0, 1)
        if R:
            res["drpe1d"] += torch.zeros(H, 2 * R + 1).index_add_(1, idx.reshape(-1), ds.reshape(H, -1))
    return res


# ------------------------------------------------------------------------------------------------------------------- cases
LS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 333)
WS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
PACK_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
DTYPES = (torch.bfloat16, torch.float16)


def _radius(i, w):
    """None and the radii {1, 8, 31, 32, w - 1, w, w + 1, 128} in turn"""
    r = (None, 1, 8, 31, 32, w - 1, w, w + 1, 128)[i % 9]
    return None if r is None else max(1, min(r, 1024))


def _case(i, lens, window, R, packed=False, S=None, scale=0.125, dtype=None):
    dtype = DTYPES[i % 2] if dtype is None else dtype
    S = max(lens) if S is None else S
    name = ("packed" + str(len(lens)) + f"-max{S}") if packed else f"B{len(lens)}-L{lens[0]}"
    return dict(id=f"{i:02d}-{name}-w{window}-R{R or 0}-{'bf16' if dtype == torch.bfloat16 else 'fp16'}" + ("" if scale == 0.125 else f"-scale{scale}"),
                lens=list(lens), window=window, R=R or 0, packed=packed, S=S, scale=scale, dtype=dtype, strided=(not packed and i % 4 == 3), seed=1000 + i)


def _build_cases():
    cs = []
    add = lambda *a, **kw: cs.append(_case(len(cs), *a, **kw))
    for i in range(2 * len(WS)):                                        # lengths x windows, a cycling pairing (12 and 13 are coprime)
        L, w = LS[(5 * i) % len(LS)], WS[i % len(WS)]
        add([L] * (1 + i % 2), w, _radius(i, w), scale=0.3 if i == 7 else 0.125)
    for j, L in enumerate((33, 64, 129)):                               # w = L - 1, L, 4 L
        for w in (L - 1, L, 4 * L):
            add([L] * (1 + len(cs) % 2), w, _radius(4 + len(cs), w))
    add([700], 127, 128)                                                # the LongT5 setting: whole skipped tiles on both sides
    add([700], 127, 128)
    for w in (1012, 1013, 1024):                                        # either side of the dQ kernel's 48 KiB seam; S = 40
        add([40], w, 1024)
        add([40], w, 1024)
    cyc = lambda k, off=0: [PACK_LENS[(off + 5 * j) % len(PACK_LENS)] for j in range(k)]
    add(cyc(42), 33, 32, packed=True, S=200)                            # 42 sequences, max_seqlen = the longest
    add(cyc(41, 3), 65, 8, packed=True, S=200)
    add([129, 0, 1, 64, 0, 33, 128, 65, 31, 127, 63, 32, 0], 127, 128, packed=True, S=129 + 64)   # max_seqlen 64 beyond
    add([0, 65, 1, 200, 33, 0, 31, 127, 0, 64, 129, 32], 95, 96, packed=True, S=200 + 64)
    add([1, 32, 63, 0, 128, 64, 33], 31, 31, packed=True, S=128 + 200)  # 200 beyond: whole blocks that only zero their partial row
    add([65, 0, 31, 129, 1, 0], 2, None, packed=True, S=129 + 200)
    return cs


CASES = _build_cases()


def boosted(L):
    """the positions of a sequence whose rows carry BOOST times the others' magnitude: key 0, key L - 1 and the tile seams"""
    pos = {0, L - 1, 32}
    for t in range(1, L // 64 + 2):
        pos |= {64 * t - 1, 64 * t, 64 * t + 32}
    return sorted(p for p in pos if 0 <= p < L)


def inputs(case):
    """q, k (0.02 randn at the scale 0.125), v, do (0.25 randn) as flat (total, H, D) tensors in the dtype, the boosted rows times BOOST; rpe (H, 2 R + 1)
    fp32 i.i.d., every entry distinct, so a wrong index shows.  (q and k are kept small because a boosted q row meets a boosted k row
    on the diagonal and at the band's corners, 1024 times a plain score: at 0.1 such a pair's weight is as good as 0 or 1 and a
    defect on exactly that pair cannot be seen by anyone.)"""
    g = torch.Generator().manual_seed(case["seed"])
    total, cu = sum(case["lens"]), _seqs(case)
    t = {}
    qk = 0.02 * math.sqrt(0.125 / case["scale"])                          # (the same score magnitudes at every scale)
    for x, mag in (("q", qk), ("k", qk), ("v", 0.25), ("do", 0.25)):
        y = torch.randn(total, H, D, generator=g) * mag
        for b, L in enumerate(case["lens"]):
            for p in boosted(L):
                y[cu[b] + p] *= BOOST
        t[x] = y.to(case["dtype"])
    t["rpe"] = torch.randn(H, 2 * case["R"] + 1, generator=g) if case["R"] else None
    return t


STRUCTURES = ("visited-but-masked step", "mask-free step", "single-corner step", "skipped step inside a visited tile", "skipped tile on the left",
              "skipped tile on the right", "block with m0 >= L in a packed batch", "both clamp ends in one step", "wc == w", "wc < w")


def structures_of(case):
    got = set()
    for L in case["lens"]:
        for s in all_steps(L, case["window"]):
            got |= {"skipped tile on the left"} if s["left"] else set()
            got |= {"skipped tile on the right"} if s["right"] else set()
            for wv in s["waves"]:
                for key, name in (("masked", STRUCTURES[0]), ("full", STRUCTURES[1]), ("corner", STRUCTURES[2]), ("skipped", STRUCTURES[3])):
                    if wv[key]:
                        got.add(name)
        if case["packed"] and 64 * ((case["S"] + 63) // 64 - 1) >= L:
            got.add("block with m0 >= L in a packed batch")
    if case["R"]:
        wc, w = min(case["window"], case["R"]), case["window"]
        if wc <= 31 and any(L > wc for L in case["lens"]):
            got.add("both clamp ends in one step")
        got.add("wc == w" if wc == w else "wc < w")
    return got


# ------------------------------------------------------------------------------------------------------------------- mutants
# Each takes a sequence's knobs (`_knobs` plus window, R, wc, b, B, L, tok0, b_last, packed, nxt) and changes them the way the defect
# would; it returns whether the defect exists for this sequence.  Whether it changed anything a correct kernel computes (`applied`)
# is read off the restatement: some output differs from the truth.
def _set(key, value, need=None):
    def f(c):
        if need is not None and not need(c):
            return False
        c[key] = value(c) if callable(value) else value
        return True
    return f


def _pw(pick):
    """zero the pair weights of the 32 x 32 steps (or 64 x 64 tiles) `pick` names: [(row lo, row hi, key lo, key hi)]"""
    def f(c):
        L = c["L"]
        rects = pick(c, all_steps(L, c["window"]))
        if not rects:
            return False
        pw = torch.ones(L, L, dtype=torch.float64)
        for r0, r1, k0, k1 in rects:
            pw[r0:r1, k0:k1] = 0.0
        c["pw"] = pw
        return True
    return f


def _last_steps(c, blocks):
    return [(wv["r0"], wv["r0"] + 32, wv["visited"][-1], wv["visited"][-1] + 32) for s in blocks for wv in s["waves"]
            if len(wv["visited"]) >= 2 and wv["visited"][-1] in wv["masked"]]


def _corner_steps(c, blocks):
    return [(wv["r0"], wv["r0"] + 32, sb, sb + 32) for s in blocks for wv in s["waves"] for sb in wv["corner"]]


def _tile(which):
    def pick(c, blocks):
        return [(s["m0"], s["m0"] + 64, 64 * s[which], 64 * s[which] + 64) for s in blocks if s["t_end"] > s["t_begin"]]
    return pick


def _masked_as_full(c):
    L = c["L"]
    for s in all_steps(L, c["window"]):
        for wv in s["waves"]:
            for sb in wv["masked"]:
                if sb + 31 < L and wv["r0"] + 31 < L:
                    vo = torch.zeros(L, L, dtype=torch.bool)
                    vo[wv["r0"]:wv["r0"] + 32, sb:sb + 32] = True
                    c["vis_or"] = vo
                    return True
    return False


def _zero_rows(c):
    L = c["L"]
    if L % 32 == 0:
        return False
    pos = torch.arange(L, (L + 31) // 32 * 32)
    z = torch.zeros(c["H"], len(pos), D, dtype=torch.float64)
    c["ext"] = (pos, z, z)
    return True


def _next_key(c):
    if not c["packed"] or c["nxt"] is None:
        return False
    c["ext"] = (torch.tensor([c["L"]]), c["nxt"][0][:, None, :], c["nxt"][1][:, None, :])
    return True


def _grow(pick):
    def f(c):
        if not c["R"]:
            return False
        g = pick(c)
        if g is None:
            return False
        c["grow"] = g
        return True
    return f


def _g_block(value):
    def pick(c):
        if c["b"] != c["b_last"]:
            return None
        g = torch.ones(c["L"], dtype=torch.float64)
        g[64 * ((c["L"] - 1) // 64):] = value
        return g
    return pick


def _g_wave1(c):
    g = torch.ones(c["L"], dtype=torch.float64)
    g[(torch.arange(c["L"]) % 64) >= 32] = 0.0
    return g if c["L"] > 32 else None


rpe = lambda c: bool(c["R"])
MUTANTS = {
    "band one key wider on the right": _set("rs", 1),
    "band one key narrower on the right": _set("rs", -1),
    "band one key wider on the left": _set("ls", 1),
    "band one key narrower on the left": _set("ls", -1),
    "the last visited step of a wave skipped": _pw(_last_steps),
    "a single-corner step skipped": _pw(_corner_steps),
    "a masked step treated as full": _masked_as_full,
    "the first streamed tile dropped": _pw(_tile("t_begin")),
    "the last streamed tile dropped": _pw(_tile("t_end")),
    "keys at or past L visible as zero rows": _zero_rows,
    "the first key of the next packed sequence visible": _next_key,
    "positions global instead of local to the sequence": _set("global_pos", True, lambda c: c["packed"] and c["tok0"] > 0),
    "bias index +1": _set("shift", 1, rpe),
    "bias index -1": _set("shift", -1, rpe),
    "bias clamped at wc - 1": _set("rclamp", lambda c: c["wc"] - 1, rpe),
    "the neighbouring head's table row": _set("head_shift", 1, rpe),
    "lse in log2 units": lambda c: bool(c.update(lse_mul=LOG2E, lse_in_mul=LN2)) or True,
    "delta of row m + 1": _set("delta_shift", 1, lambda c: c["L"] >= 2),
    "the end diagonals beyond +-wc not collected": _set("g_noends", True, lambda c: c["R"] and min(c["window"], c["L"]) > c["wc"]),
    "the +wc end also given the -wc sum": _set("g_plus_minus", True, rpe),
    "one workgroup's partial row left out": _grow(_g_block(0.0)),
    "one workgroup's partial row counted twice": _grow(_g_block(2.0)),
    "one batch element left out of the reduction": _grow(lambda c: torch.zeros(c["L"], dtype=torch.float64) if (c["b"] == c["b_last"] and c["B"] > 1) else None),
    "wave 1's row left out": _grow(_g_wave1),
    "a diagonal sum shifted by one": _set("g_shift", 1, rpe),
}
DRPE_ONLY = ("the end diagonals beyond +-wc not collected", "the +wc end also given the -wc sum", "one workgroup's partial row left out",
             "one workgroup's partial row counted twice", "one batch element left out of the reduction", "wave 1's row left out",
             "a diagonal sum shifted by one")


def differs(mut, ref):
    """the outputs in which a mutated restatement differs from the truth (`applied`: the list is not empty)"""
    out = []
    for x in FWD + BWD:
        if x in ref:
            a, b = mut[x], ref[x]
            if not torch.equal(torch.nan_to_num(a, neginf=-1e300), torch.nan_to_num(b, neginf=-1e300)):
                out.append(x)
    return out
