"""fp64 restatement of `fat5_attn_decode` (the contract at the head of csrc/decode_kernels.h), a per-element error bound derived from
the kernel's operation counts, and mutants: restatements with one realistic defect each, which the bound must tell from the truth.
CPU only; imports no GPU code.  Used by tests/test_decode_fp64_cpu.py and tests/test_decode_fp64_gpu.py.

The bound (u = 2^-24, the fp32 unit roundoff; ulp_T(r) the spacing of the storage dtype T at |r|).  Kernel constants: a key row is
owned by TPR = D / 8 lanes, a workgroup holds G = 256 / TPR row groups, a row group takes U = DEC_UNROLL = 4 rows per step; split s
of `splits` covers c = ceil(L / splits) keys.  All scores are in log2 units, as in the kernel.  Per (b, h):

  Score.  s_j = fma(bias_j, log2e, (q . k_j) * scale_log2).  The dot product is an 8-deep fmaf chain and log2(TPR) shuffle adds
      (relative to sum_i |q_i k_ij|: 8 + log2 TPR roundings), then the multiply and the bias fmaf (2), the constant log2e in fp32
      (1), and the host's scale_log2 = sm_scale * log2e formed in fp32 from the ABI's float sm_scale (2: the constant, the product;
      the reference uses the same float sm_scale).  With A = max_j sum_i |q_i k_ij| |sm_scale| log2e and Bm = max_j |bias_j| log2e:
          ds <= (8 + log2 TPR + 5) u (A + Bm).
      (The issue's count is 8 + log2 TPR + 3; the two roundings inside scale_log2 are the ones it leaves out.)
  Weight.  p_j = exp2(s_j - m).  The subtraction rounds once (u |s_j - m|), s_j and m each carry ds, and `fast_exp2` is
      `__builtin_amdgcn_exp2f`, i.e. one v_exp_f32, whose accuracy the ISA manual gives as 1 ulp: e_exp = 2^-23.  With
      range = max_j (m - s_j):
          e_w = e_exp + ln2 u range           (an exp2 of a rounded difference of computed maxima: alpha and both merges' weights)
          e_p = ln2 2 ds + e_w                (a key's weight, relative)
      v_exp_f32 flushes results below 2^-126 to zero; `decode_bound` requires range < 120, so no weight is flushed.
  Rescales and merges.  alpha = exp2(m_old - m_new) multiplies a row group's l and acc[] alike, so its error reweights the keys
      seen so far against the later ones; m only grows, so the differences telescope to at most `range`, and there are
      steps = ceil(c / (G U)) of them.  The row-group merge and the split merge each apply one more such weight:
          e_f = (steps + 2) e_exp + 3 ln2 u range.
  Sums.  l and acc[] run n = steps (U + 1) + G + splits + 1 roundings deep: U adds and one rescale multiply per step, the G-term
      row-group merge, the split merge, the divide.
  Result.  o = N / l with |N| <= sum_j p_j |v_j| =: T (per d; p normalised); numerator and denominator carry the weight errors
      independently:
          |o - ref|     <= ulp_T(ref) / 2 + ((n + 4) u + 2 e_p + 2 e_f) T
          |lse - ref|   <= (n + 4) u + e_p + e_f + 4 u |ref| + 2 u ln(L)
      (lse = (M + log2f(l)) ln2: log2f within 1 ulp of log2 l <= log2 L, the add, the constant ln2 and the product: 4 u |ref|.
      The issue's formula has neither e_f nor the log2f term; both are roundings the kernel performs, stated above.)
No term is fitted to a measured error and there is no max(1, .) clamp: for L = 0 the bound is the exact o = 0, lse = -inf.
"""
import math

import torch

from rowwise_fp64 import ulp

U32 = 2.0 ** -24
E_EXP = 2.0 ** -23      # v_exp_f32: 1 ulp
LOG2E = 1.0 / math.log(2.0)
LN2 = math.log(2.0)
DEC_THREADS, DEC_UNROLL, DEC_MAX_SPLITS = 256, 4, 128   # csrc/decode_kernels.h


def groups(D):
    """row groups per workgroup"""
    return DEC_THREADS // (D // 8)


def wg_pass(D):
    """rows one workgroup takes per step of its loop"""
    return groups(D) * DEC_UNROLL


def split_range(L, splits, s):
    c = -(-L // splits)
    lo = min(L, s * c)
    return lo, min(L, lo + c)


def _clampi(v, n):
    return max(0, min(int(v), n - 1))


def decode_ref(q, kc, vc, kn, vn, lens, sm_scale, rpe1d=None, R=0, batch_idx=None, row_batch=None, splits=1, mutant=None):
    """q (B, 1, H, D) or (B, H, D); kc / vc (cacheB, cap, H, D); kn / vn like q or None; lens: B ints (before the append); rpe1d
    (H, 2R + 1) or None; batch_idx: B ints or None; row_batch (B, cap) or None.  Returns a dict: o (B, H, D), lse (B, H), absv
    (B, H, D) = sum_j p_j |v_j|, smag (B, H) = max_j sum_i |q_i k_ij| |sm_scale|, bmag (B, H) = max_j |bias_j|, srange (B, H) =
    max_j (m - s_j) (all three in nats), L (the key counts), kc / vc (the caches after the append), applied (the mutant changed
    something).  `mutant` is one of MUTANTS' functions; `splits` only tells a mutant where the kernel's split boundaries are."""
    B, H, D = q.shape[0], q.shape[-2], q.shape[-1]
    cacheB, cap = kc.shape[0], kc.shape[1]
    qd = q.reshape(B, H, D).double()
    knd = kn.reshape(B, H, D).double() if kn is not None else None
    vnd = vn.reshape(B, H, D).double() if vn is not None else None
    scale = float(torch.tensor(float(sm_scale), dtype=torch.float32))  # (the ABI's field is a float)
    out = dict(o=torch.zeros(B, H, D, dtype=torch.float64), lse=torch.full((B, H), -math.inf, dtype=torch.float64),
               absv=torch.zeros(B, H, D, dtype=torch.float64), smag=torch.zeros(B, H, dtype=torch.float64),
               bmag=torch.zeros(B, H, dtype=torch.float64), srange=torch.zeros(B, H, dtype=torch.float64), L=[], applied=False,
               kc=kc.clone(), vc=vc.clone())
    for b in range(B):
        n = max(0, min(int(lens[b]), cap))
        app = kn is not None and n < cap
        L = n + 1 if app else n
        out["L"].append(L)
        if app:
            out["kc"][b, n], out["vc"][b, n] = kn.reshape(B, H, D)[b], vn.reshape(B, H, D)[b]
        if L == 0:
            continue
        j = torch.arange(L)
        if row_batch is not None:
            src = row_batch[b, :L].long().clamp(0, cacheB - 1)
        elif batch_idx is not None:
            src = torch.full((L,), _clampi(batch_idx[b], cacheB))
        else:
            src = torch.full((L,), b)
        c = dict(b=b, L=L, n=n, app=app, splits=splits, D=D, R=R, bias=rpe1d is not None, cacheB=cacheB, src=src,
                 row_batch=row_batch, w=torch.ones(L, dtype=torch.float64), pos=L - 1, shift=0, rclamp=R, lse_div=1.0)
        if mutant is not None and mutant(c):
            out["applied"] = True
        src = c["src"].clone()
        if app:
            src[L - 1] = 0  # (never read from the cache)
        K, V = kc[src, j].double(), vc[src, j].double()  # (L, H, D)
        if app:
            K[L - 1], V[L - 1] = knd[b], vnd[b]
        s = torch.einsum("hd,lhd->hl", qd[b], K) * scale
        out["smag"][b] = (torch.einsum("hd,lhd->hl", qd[b].abs(), K.abs()) * abs(scale)).amax(-1)
        if rpe1d is not None:
            rel = (j - c["pos"] + c["shift"]).clamp(-c["rclamp"], c["rclamp"]) + R
            bias = rpe1d.double()[:, rel]
            s = s + bias
            out["bmag"][b] = bias.abs().amax(-1)
        m = s.amax(-1, keepdim=True)
        out["srange"][b] = (m - s).amax(-1)
        p = torch.exp(s - m) * c["w"]
        l = p.sum(-1, keepdim=True)
        live = l[:, 0] > 0
        pn = torch.where(l > 0, p / l, torch.zeros_like(p))
        out["o"][b] = torch.einsum("hl,lhd->hd", pn, V)
        out["absv"][b] = torch.einsum("hl,lhd->hd", pn, V.abs())
        out["lse"][b] = torch.where(live, (m[:, 0] + torch.log(l[:, 0])) / c["lse_div"], torch.full_like(l[:, 0], -math.inf))
    return out


def decode_bound(ref, dtype, D, splits):
    """(bound_o (B, H, D), bound_lse (B, H)) for a `decode_ref` result, the kernel at head dimension D run with `splits` splits"""
    G, tpr = groups(D), D // 8
    assert float(ref["srange"].max()) * LOG2E < 120.0, "a weight would be flushed by v_exp_f32: outside the derivation"
    B = len(ref["L"])
    bo, bl = torch.zeros_like(ref["o"]), torch.zeros_like(ref["lse"])
    for b in range(B):
        L = ref["L"][b]
        if L == 0:
            continue  # (exactly o = 0; lse = -inf is compared as a pattern)
        steps = -(-(-(-L // splits)) // (G * DEC_UNROLL))
        n = steps * (DEC_UNROLL + 1) + G + splits + 1
        ds = (8 + math.log2(tpr) + 5) * U32 * (ref["smag"][b] + ref["bmag"][b]) * LOG2E   # (H,), log2 units
        rng = ref["srange"][b] * LOG2E
        e_w = E_EXP + LN2 * U32 * rng
        e_p = LN2 * 2 * ds + e_w
        e_f = (steps + 2) * E_EXP + 3 * LN2 * U32 * rng
        bo[b] = ((n + 4) * U32 + 2 * e_p + 2 * e_f).unsqueeze(-1) * ref["absv"][b]
        bl[b] = (n + 4) * U32 + e_p + e_f + 4 * U32 * ref["lse"][b].abs() + 2 * U32 * math.log(L)
    return bo + 0.5 * ulp(ref["o"], dtype), bl


def ratios(o, lse, ref, bound_o, bound_lse):
    """(worst |o - ref| / bound, worst |lse - ref| / bound over the finite reference entries, the finiteness patterns agree);
    o (B, H, D) and lse (B, H) in any float type.  A non-finite o gives inf."""
    o, lse = o.double(), lse.double()
    eo = (o - ref["o"]).abs()
    ro = torch.where(eo == 0, torch.zeros_like(eo), eo / bound_o)   # (an exact result is within a bound of zero)
    ro = torch.where(torch.isfinite(o), ro, torch.full_like(ro, math.inf))
    fin = torch.isfinite(ref["lse"])
    same = torch.equal(torch.isfinite(lse), fin) and torch.equal(lse[~fin], ref["lse"][~fin])
    rl = ((lse - ref["lse"]).abs()[fin] / bound_lse[fin])
    rl = torch.where(torch.isfinite(lse[fin]), rl, torch.full_like(rl, math.inf))
    return float(ro.max()), float(rl.max()) if rl.numel() else 0.0, same


def within(o, lse, ref, bound_o, bound_lse):
    ro, rl, same = ratios(o, lse, ref, bound_o, bound_lse)
    return same and ro <= 1.0 and rl <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- mutants
# Each takes the per-sequence context of decode_ref, changes it the way the defect would, and returns whether it changed anything.
def _mid(c):
    return (c["splits"] - 1) // 2


def _drop_first(c):
    c["w"][0] = 0
    return True


def _drop_last(c):
    c["w"][c["L"] - 1] = 0
    return True


def _drop_split_end(c):
    if c["splits"] < 2:
        return False
    lo, hi = split_range(c["L"], c["splits"], _mid(c))
    if hi <= lo:
        return False
    c["w"][hi - 1] = 0
    return True


def _dup_split_start(c):
    if c["splits"] < 2:
        return False
    lo, hi = split_range(c["L"], c["splits"], _mid(c) + 1)
    if hi <= lo:
        return False
    c["w"][lo] = 2
    return True


def _drop_group_last_pass(c):
    """row group 0 of the last pass of the last non-empty split"""
    G, P, L = groups(c["D"]), wg_pass(c["D"]), c["L"]
    s = (L - 1) // -(-L // c["splits"])
    lo, hi = split_range(L, c["splits"], s)
    p0 = lo + (hi - lo - 1) // P * P
    c["w"][p0:hi:G] = 0
    return True


def _bias_shift(d):
    def f(c):
        if not c["bias"]:
            return False
        c["shift"] = d
        return True
    return f


def _bias_clamp(c):
    if not c["bias"] or c["L"] - 1 < c["R"]:
        return False  # (no key at distance R or more)
    c["rclamp"] = c["R"] - 1
    return True


def _bias_prelen(c):
    """the query placed from the length before the append (len_b - 1) instead of L_b - 1"""
    if not c["bias"] or not c["app"]:
        return False
    c["pos"] = c["n"] - 1
    return True


def _rowmap_neighbour(c):
    L, rb = c["L"], c["row_batch"]
    if rb is None or L < 2:
        return False
    j = L - 2  # (with an append row L - 1 is not read through the map, but its entry exists)
    a, b_ = _clampi(rb[c["b"], j], c["cacheB"]), _clampi(rb[c["b"], j + 1], c["cacheB"])
    if a == b_:
        return False
    c["src"] = c["src"].clone()
    c["src"][j] = b_
    return True


def _lse_log2(c):
    c["lse_div"] = LN2
    return True


MUTANTS = {
    "drop key 0": _drop_first,
    "drop key L-1": _drop_last,
    "drop the last key of a middle split": _drop_split_end,
    "count the first key of the next split twice": _dup_split_start,
    "drop one row group in the last pass": _drop_group_last_pass,
    "bias index +1": _bias_shift(1),
    "bias index -1": _bias_shift(-1),
    "bias clamped at R-1": _bias_clamp,
    "bias aligned to the length before the append": _bias_prelen,
    "cache_row_batch entry taken from the next row": _rowmap_neighbour,
    "lse in log2 units": _lse_log2,
}
