"""Exact restatement of the fused AdamWScale step (flasht5_amd/csrc/adamw_kernels.h), TEST INFRASTRUCTURE ONLY, no GPU.

The kernel header promises the reference optimizer's arithmetic "op by op including its intermediate roundings".  Every op of the
update is ONE IEEE fp32 operation followed by an explicit `rnd<>`; hipcc's default divide and square root are correctly rounded
(see DISASSEMBLY below); the only order-dependent quantity is the sum of squares behind rms(p), and the generator below draws
parameters whose squares sum exactly in fp32 in any order.  So the check is bit for bit: no tolerance exists to fit.

  emulate        one step on one tensor, line by line (`adamw_sumsq_kernel`'s result and the `one` lambda), numpy float32 = one IEEE
                 fp32 operation per line, `rnd<DT>` / `rnd<SDT>` through torch.bfloat16 / torch.float16
  fma32          the three explicit `fmaf` sites (and the contracted products) as exact fused multiply-adds
  run_table      the whole launch: every tensor of a descriptor table, optionally with one defect (MUTANTS)
  admissible     per element the tuple (p, k, m, v) equals one compiler variant's tuple (m and v differ between variants only in fp16)
  adamw_fp64 / bound_fp64   the same step in plain fp64 and a derived per-element bound on emulate minus it (keeps emulate honest)
  make_tensors   the seeded inputs (dyadic parameters: exact sum of squares, proven per tensor by `exactness_proof`)

CONTRACTION.  hipcc's default -ffp-contract=fast may fuse a product into the sum that consumes it wherever no `rnd` and no explicit
`fmaf` stands between.  Read from the kernel source (adamw_kernels.h:130-150), these are the only such sites:
    :138 -> :140   kf + upd   (Kahan)       upd = neg_step * (mf / den)      -> fma(neg_step, mf / den, kf)
    :138 -> :146   pf + upd   (no Kahan)                                     -> fma(neg_step, mf / den, pf)
Everything else is a product that feeds a `rnd`, a multiplicand of an explicit `fmaf` (:135 `a2 * gf`, :131 `gf * gcoef` with
DT = fp32) or the ADDEND of an explicit `fmaf` (:132 -> :133 `mf * beta1`, :134 -> :135 `vf * beta2` with SDT = fp32): a fused
multiply-add has one product, so none of these can contract.  :118 / :119 are products of products.  The vector loop and the tail
loop are separate inlined copies of `one`, so the choice may differ from element to element: `admissible` allows either per
element.

SINGLE ROUNDING TO HALF (found on the first hardware run: edges, fp32 parameters with fp16 states, tensor 1 element 202:
m = 0x3bf3, beta1 = 0.9f: the fp32 product lands exactly on the midpoint of two halves and the conversion then rounds to even,
0x3b28; the kernel stored 0x3b27, the exact product rounded once).  Where a product or an fmaf feeds `rnd<FAT5_F16>`, the compiler
emits
    v_fma_mixlo_f16 v15, s16, v15, 0 op_sel_hi:[0,1,0]        (:132 rnd<SDT>(mf * beta1))
    v_fma_mixlo_f16 v15, s18, v5, v15 op_sel_hi:[0,0,1]       (:133 rnd<SDT>(fmaf(a1, gf, mf)))
and the MI355X rounds that instruction's exact a * b + c once to half, not to fp32 first.  This is one more freedom of the same
kind as contraction (a result closer to the exact one, chosen by the compiler per site), not a defect of the kernel: `mix` selects
it for every such site together -- :119, :131, :132, :133, :134, :135, :148 and the contracted :140 / :146 -- as the compiled bodies do.

DISASSEMBLY (hipcc -O3 --offload-arch=gfx950 -S of the update kernels, recorded before the first hardware run):
  * `mf / den`: v_div_scale_f32 x2, v_rcp_f32, v_fma_f32 / v_fmac_f32 refinement, v_div_fmas_f32, v_div_fixup_f32 -- the correctly
    rounded fp32 division;
  * `sqrtf` with fp32 / bf16 operands: v_sqrt_f32, then the two candidates one ulp below and above tested by v_fma_f32 residuals
    and selected -- the correctly rounded sequence; with fp16 operands (an extended half is never an fp32 subnormal): v_rsq_f32 and
    the Goldschmidt / Newton refinement with a final v_fma_f32 residual -- the compiler's other correctly rounded sequence;
  * `(float)sqrt((double)numel)`: v_rsq_f64 with two refinement steps, then v_cvt_f32_f64.  For numel < 2^24 sqrt(numel) is either
    exact or at least 2^-38 away from every fp32 rounding boundary (a boundary b has 25 significant bits, |numel - b^2| >= 2^-26
    and sqrt(numel) + b < 2^13), far more than the fp64 sequence's error, so the cast equals the correctly rounded value;
  * fp16: the compiler uses v_fma_mixlo_f16 for products and fmafs that are rounded to half (see SINGLE ROUNDING TO HALF: not the
    same values as the source's two roundings) and v_add_f16 / v_sub_f16 for `rnd(a + b)` of two halves -- these are the same
    values as the fp32 operation followed by the conversion (24 >= 2 * 11 + 2: no double rounding);
  * both contraction sites above are fused in the fp32 and fp16 bodies (v_fmac_f32 / v_pk_fma_f32 / v_fma_mixlo_f16).
"""
import math

import numpy as np
import torch

CHUNK = 8192                                          # adamw_kernels.h:20 kAdamChunk
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SIZE = {F32: 4, F16: 2, BF16: 2}
U16 = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}    # unit roundoff of the storage rounding (none for fp32)
TINY = {F32: 0.0, F16: 2.0 ** -25, BF16: 0.0}         # half the spacing of fp16 subnormals (fp32 / bf16 values stay normal here)
U32 = 2.0 ** -24
f32 = np.float32

# (DT, SDT, KAHAN): every instantiation the host dispatches (adamw_step_impl, api_rowwise.hip)
TRIPLES = [(F32, F32, 0), (F32, BF16, 0), (F32, F16, 0), (BF16, BF16, 0), (BF16, BF16, 1), (F16, F16, 0), (F16, F16, 1),
           (BF16, F16, 1), (F16, BF16, 0)]


def vec(dt):
    """elements per 16-byte vector of p / g / k (adamw_kernels.h:152)"""
    return 16 // SIZE[dt]


def rnd(x, dt):
    """`rnd<DT>` (adamw_kernels.h:27-31): the rounding at the end of one in-place op, round to nearest even"""
    x = np.ascontiguousarray(x, dtype=f32)
    if dt is F32:
        return x
    return torch.from_numpy(x).to(dt).float().numpy()


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: ONE rounding of a * b + c.

    The product of two 24-bit significands has at most 48 bits: it is exact in fp64 (2 * 24 <= 53).  The fp64 sum s = pr + c is
    rounded; TwoSum gives its error e exactly.  Where e != 0 the true value lies strictly between s and its fp64 neighbour in the
    direction of e; of those two the one with an odd last bit is taken (round to odd: the sticky bit).  Rounding a value that was
    rounded to odd at 53 bits to nearest-even at 24 bits equals rounding the true value once, because 53 >= 24 + 2 (in all
    53 >= 2 * 24 + 2: exact product, guard and sticky bit) -- the sticky bit keeps a true value just off an fp32 midpoint off it."""
    with np.errstate(invalid="ignore", over="ignore"):
        return fma_odd(a, b, c).astype(f32)


def fma_odd(a, b, c):
    """a * b + c of float32 arrays rounded to odd at 53 bits (see fma32): one more rounding to nearest of it, to any format of at
    most 51 bits, is the single rounding of the exact result"""
    a, b, c = (np.asarray(t, dtype=f32).astype(np.float64) for t in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        pr = a * b
        s = pr + c
        bb = s - pr
        e = (pr - (s - bb)) + (c - bb)
        s = np.ascontiguousarray(s)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (e != 0) & even
        return np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def rnd_fma(a, b, c, dt, mix):
    """rnd<dt>(fmaf(a, b, c)).  mix (dt = fp16 only): the compiler's v_fma_mixlo_f16, which rounds the exact a * b + c ONCE to half
    (numpy converts double to half directly) instead of to fp32 and then to half"""
    if mix and dt is F16:
        with np.errstate(invalid="ignore", over="ignore"):
            return fma_odd(a, b, c).astype(np.float16).astype(f32)
    return rnd(fma32(a, b, c), dt)


def rnd_mul(a, b, dt, mix):
    """rnd<dt>(a * b); with mix as v_fma_mixlo_f16 a, b, 0"""
    if mix and dt is F16:
        return rnd_fma(a, b, f32(-0.0), dt, True)
    return rnd(np.asarray(a, dtype=f32) * np.asarray(b, dtype=f32), dt)


def prefactor(cfg):
    """the table's `step_prefactor` / dev_scalars[0]: AdamWScale._prefactor (adamw_scaled.py:60-68)"""
    from flasht5_amd.adamw_scaled import AdamWScale
    return AdamWScale._prefactor(cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["step"], not cfg["plain"])


def dev_scalars(cfg):
    """what graph_advance writes (adamw_scaled.py:305): three Python doubles, each cast once by fill_"""
    lr, wd = float(cfg["lr"]), float(cfg["wd"])
    return np.array([prefactor(cfg), -lr * wd if wd > 0.0 else 0.0, lr * 1e-3], dtype=f32)


def host_scalars(cfg, mut=None):
    """the fp32 values the kernel sees: adamw_step_impl's double-to-float casts (api_rowwise.hip), the c_float of the
    descriptor (adamw_scaled.py:145), or the three device scalars (adamw_kernels.h:107-109)"""
    lr, wd = float(cfg["lr"]), float(cfg["wd"])
    H = {"beta1": f32(cfg["beta1"]), "beta2": f32(cfg["beta2"]), "eps": f32(cfg["eps"]),               # :1592
         "a1": f32(1.0 - cfg["beta1"]), "a2": f32(1.0 - cfg["beta2"])}                                   # :1593
    if cfg["entry"] == "dev":
        d = dev_scalars(cfg)
        H["prefactor"], H["wdf"], H["lr_small"] = d[0], d[1], d[2]                                       # kernel :107-109
        if mut == "table_prefactor_in_dev":
            H["prefactor"] = f32(TABLE_PREFACTOR_DEV)
    else:
        H["prefactor"] = f32(prefactor(cfg))
        H["wdf"] = f32(-lr * wd) if wd > 0.0 else f32(0.0)                                               # :1594
        H["lr_small"] = f32(lr * 1e-3)                                                                   # :1595
    H["clip"] = cfg["entry"] == "clipped"
    H["gcoef"] = f32(cfg["coef"]) if H["clip"] else f32(1.0)                                             # kernel :102-103
    if mut == "betas_swapped":
        H["beta1"], H["beta2"] = H["beta2"], H["beta1"]
    return H


TABLE_PREFACTOR_DEV = 1e30   # what the `dev` cases put into every descriptor's step_prefactor: the kernel must ignore it


def sumsq_exact(p):
    """the sum of squares of stored values in fp64, asserted to be an fp32 number (then every summation order gives it)"""
    s = float((p.double() ** 2).sum())
    assert float(f32(s)) == s, "the sum of squares is not exact in fp32: not an input of this generator"
    return s


def tensor_scalars(p, cfg, H, mut=None, mix=False):
    """sumsq -> norm -> rms -> neg_step of one tensor (adamw_kernels.h:111-119); every intermediate is returned"""
    dt, n = cfg["dt"], p.numel()
    src = p
    if mut == "rms_first_chunk":
        src = p[:CHUNK]
    elif mut == "rms_first_256_partials":
        src = p[:256 * CHUNK]
    with np.errstate(over="ignore", invalid="ignore"):
        sumsq = f32(sumsq_exact(src))                                        # :113-114 (exact: any order)
        norm = rnd(np.sqrt(np.array([sumsq], f32)), dt)[0]                   # :116  rnd<DT>(sqrtf(sumsq))
        sn = f32(np.sqrt(np.float64(n)))                                     # :117  (float)sqrt((double)numel)
        rms = rnd(np.array([norm / sn], f32), dt)[0]                         # :117  rnd<DT>(norm / ...)
        floor = f32(1e-3)
        if mut == "no_floor":
            neg = -(H["prefactor"] * rms)
            if cfg["plain"]:
                neg = -rnd_mul(np.array([H["prefactor"]], f32), rms, dt, mix)[0]
        else:
            neg = -(H["prefactor"] * max(floor, rms))                        # :118  -(prefactor * fmaxf(1e-3f, rms))
            if cfg["plain"]:                                                 # :119
                if mut == "lr_small_always":
                    neg = -H["lr_small"]
                elif rms > floor:
                    neg = -(H["prefactor"] * rms) if mut == "plain_not_rounded" else -rnd_mul(np.array([H["prefactor"]], f32), rms, dt, mix)[0]
                else:
                    neg = -H["lr_small"]
    return {"sumsq": sumsq, "norm": norm, "rms": rms, "neg_step": f32(neg)}


def emulate(p, g, m, v, k, cfg, contract, *, mix=False, mut=None, neg_step=None, skip=None, H=None):
    """One step on one tensor.  p, g, k: stored values of dtype DT (k None without Kahan); m, v: of dtype SDT.
    contract: whether the compiler fused `neg_step * (mf / den)` into the following sum (module docstring).
    mix: whether a product or fmaf whose result is rounded to fp16 is rounded once (v_fma_mixlo_f16, module docstring).
    neg_step: per element or scalar (default: this tensor's own, `tensor_scalars`); skip: elements the launch leaves untouched
    (mutants only).  -> dict of stored results p, m, v, k and every fp32 intermediate."""
    dt, sdt, kahan = cfg["dt"], cfg["sdt"], bool(cfg["kahan"])
    H = H or host_scalars(cfg, mut)
    sc = None
    if neg_step is None:
        sc = tensor_scalars(p, cfg, H, mut, mix)
        neg_step = sc["neg_step"]
    ns = np.asarray(neg_step, dtype=f32)
    srd = dt if mut == "state_rounded_to_DT" else sdt
    pf, gf, mf, vf = (t.float().numpy() for t in (p, g, m, v))              # :168 / :181 (float) of the stored values
    kf = k.float().numpy() if kahan else np.zeros_like(pf)
    p0, m0, v0, k0 = pf, mf, vf, kf
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if H["clip"]:
            gf = gf * H["gcoef"] if mut == "clip_not_rounded" else rnd_mul(gf, H["gcoef"], dt, mix)     # :131
        mf = rnd_mul(mf, H["beta1"], srd, mix)                                                           # :132
        mf = rnd_fma(H["a1"], gf, mf, srd, mix)                                                          # :133  fmaf(a1, gf, mf)
        vf = rnd_mul(vf, H["beta2"], srd, mix)                                                           # :134
        vf = rnd_fma(H["a2"] * gf, gf, vf, srd, mix)                                                     # :135  fmaf(a2 * gf, gf, vf)
        if mut == "eps_before_sqrt":
            den = rnd(np.sqrt(rnd(vf + H["eps"], srd)), srd)
        elif mut == "den_fp32":
            den = rnd(np.sqrt(vf) + H["eps"], srd)
        else:
            den = rnd(np.sqrt(vf), srd)                                                                  # :136
            den = rnd(den + H["eps"], srd)                                                               # :137
        q = mf / den                                                                                     # :138  (mf / den)
        wdf = H["wdf"]
        if mut == "wd_before_update" and wdf != 0:
            pf = rnd_fma(wdf, pf, pf, dt, mix)

        def plus_upd(x, round_to=None):                                                                  # :138 -> :140 / :146
            if round_to is None:
                return fma32(ns, q, x) if contract else x + ns * q
            return rnd_fma(ns, q, x, round_to, mix) if contract else rnd(x + ns * q, round_to)

        upd = ns * q
        if kahan:
            kf = plus_upd(kf) if mut == "kahan_k_not_rounded" else plus_upd(kf, dt)                      # :140
            old = pf                                                                                     # :141
            pf = rnd(pf + kf, dt)                                                                        # :142
            err = rnd(pf - old, dt) if mut == "kahan_err_sign" else rnd(old - pf, dt)                    # :143
            kf = rnd(kf + err, dt)                                                                       # :144
        else:
            pf = plus_upd(pf, dt)                                                                        # :146
        p_mid = pf
        if mut != "wd_before_update":
            if wdf != 0 or mut == "wd_when_zero":
                pf = rnd_fma(wdf, pf, pf, dt, mix)                                                       # :148
    if skip is not None:
        pf, mf, vf, kf = (np.where(skip, a, b) for a, b in ((p0, pf), (m0, mf), (v0, vf), (k0, kf)))
    out = {"p": torch.from_numpy(np.ascontiguousarray(pf, dtype=f32)).to(dt),                           # :169 / :182  (T)po ...
           "m": torch.from_numpy(np.ascontiguousarray(mf, dtype=f32)).to(sdt),
           "v": torch.from_numpy(np.ascontiguousarray(vf, dtype=f32)).to(sdt),
           "k": torch.from_numpy(np.ascontiguousarray(kf, dtype=f32)).to(dt) if kahan else None,
           "g_used": gf, "p_mid": p_mid, "den": den, "q": q, "upd": upd, "neg_step": ns, "scalars": sc, "contract": contract, "mix": mix}
    return out


def bits(t):
    """the stored bit patterns"""
    return t.contiguous().view(torch.int32 if t.dtype is F32 else torch.int16)


def same_bits(a, b):
    """per element: the same bit pattern, or a NaN on both sides (IEEE 754 leaves a NaN's sign and payload open: inf - inf is 0xfe00
    from the MI355X's half subtraction and 0x7fff from the conversion here)"""
    return (bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))


def admissible(got, variants):
    """got: dict p, m, v, k of stored tensors; variants: emulate() results (not contracted, contracted).
    -> (ok, per-element failure mask, per-variant match masks).  The tuple (p, k, m, v) must equal one variant's tuple per element; the
    variant may differ from element to element.  m and v do not depend on the contraction site: they are bit for bit the same in
    the variants that differ only there, and differ between variants only with fp16 states (`mix`)."""
    bad = torch.zeros(got["p"].shape, dtype=torch.bool)
    match = []
    for var in variants:
        ok = same_bits(got["p"], var["p"]) & same_bits(got["m"], var["m"]) & same_bits(got["v"], var["v"])
        if var["k"] is not None:
            ok = ok & same_bits(got["k"], var["k"])
        match.append(ok)
    anyv = match[0]
    for mm in match[1:]:
        anyv = anyv | mm
    bad = bad | ~anyv
    return not bool(bad.any()), bad, match


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch: every tensor of a table, optionally with one defect
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    # name: applicability predicate on (cfg, tensors)
    "skip_last_of_chunk": lambda cfg, ts: True,
    "skip_tail_after_vectors": lambda cfg, ts: any(min(CHUNK, t["p"].numel() - e0) % vec(cfg["dt"]) for t in ts
                                                   for e0 in range(0, t["p"].numel(), CHUNK)),
    "next_tensors_rms": lambda cfg, ts: len(ts) > 1,
    "rms_first_chunk": lambda cfg, ts: any(t["p"].numel() > CHUNK for t in ts),
    "rms_first_256_partials": lambda cfg, ts: any(t["p"].numel() > 256 * CHUNK for t in ts),
    "no_floor": lambda cfg, ts: any(t["floor"] for t in ts),
    "plain_not_rounded": lambda cfg, ts: bool(cfg["plain"]) and cfg["dt"] is not F32 and any(not t["floor"] for t in ts),
    "lr_small_always": lambda cfg, ts: bool(cfg["plain"]) and any(not t["floor"] for t in ts),
    "state_rounded_to_DT": lambda cfg, ts: cfg["sdt"] is not cfg["dt"],
    "eps_before_sqrt": lambda cfg, ts: True,
    "betas_swapped": lambda cfg, ts: True,
    "wd_before_update": lambda cfg, ts: cfg["wd"] > 0,
    # fmaf(0, p, p) = p for every finite p (signed zeros included), so this one changes bits only where p left the finite range
    "wd_when_zero": lambda cfg, ts: cfg["wd"] == 0 and any(t.get("overflow") for t in ts),
    "kahan_err_sign": lambda cfg, ts: bool(cfg["kahan"]),
    "kahan_k_not_rounded": lambda cfg, ts: bool(cfg["kahan"]),
    "clip_not_rounded": lambda cfg, ts: cfg["entry"] == "clipped" and cfg["dt"] is not F32,
    "table_prefactor_in_dev": lambda cfg, ts: cfg["entry"] == "dev",
    "den_fp32": lambda cfg, ts: cfg["sdt"] is not F32,
}


SCALAR_MUTANTS = ("next_tensors_rms", "rms_first_chunk", "rms_first_256_partials", "no_floor", "plain_not_rounded", "lr_small_always",
                  "table_prefactor_in_dev")


def applies(name, cfg, tensors, truth, mutant):
    """A mutant applies to a case when its predicate holds and, for the ones that only change a tensor's step size (SCALAR_MUTANTS),
    when some element's neg_step is then another fp32 number: a norm that rounds to the same bf16 value from one chunk as from two is
    not a defect anyone could observe."""
    if not MUTANTS[name](cfg, tensors):
        return False
    if any(t["overflow"] for t in tensors) and name in SCALAR_MUTANTS + ("eps_before_sqrt", "den_fp32"):
        return False   # every p of the overflow table ends infinite whatever the size of the update: nothing to observe there
    if name in SCALAR_MUTANTS:
        return any(bool(np.any(np.broadcast_to(a[0]["neg_step"], b[0]["neg_step"].shape).view(np.int32) != b[0]["neg_step"].view(np.int32))
                        if b[0]["neg_step"].ndim else a[0]["neg_step"].view(np.int32) != b[0]["neg_step"].view(np.int32))
                   for a, b in zip(truth, mutant))
    return True


def run_table(tensors, cfg, mut=None):
    """The launch on a whole table -> per tensor [emulate(not contracted), emulate(contracted)], and the same two with `mix` where
    a dtype is fp16.  mut: one of MUTANTS."""
    H = host_scalars(cfg, mut)
    live = [t for t in tensors if t["p"].numel() > 0]
    mixes = (False, True) if F16 in (cfg["dt"], cfg["sdt"]) else (False,)
    scal = {mix: [tensor_scalars(t["p"], cfg, H, mut, mix) for t in live] for mix in mixes}
    out = []
    V = vec(cfg["dt"])
    for i, t in enumerate(live):
        n = t["p"].numel()
        skip = None
        idx = np.arange(n)
        if mut == "skip_last_of_chunk":
            skip = (idx % CHUNK == CHUNK - 1) | (idx == n - 1)
        elif mut == "skip_tail_after_vectors":
            e0 = idx // CHUNK * CHUNK
            cnt = np.minimum(CHUNK, n - e0)
            skip = (idx - e0) >= cnt // V * V
        res = []
        for mix in mixes:                                       # order: (contract, mix) = (0, 0), (1, 0), then (0, 1), (1, 1) with fp16
            ns = scal[mix][i]["neg_step"]
            if mut == "next_tensors_rms" and i + 1 < len(live):     # the tensor's last chunk resolves to the next table entry
                ns = np.where(idx >= (n - 1) // CHUNK * CHUNK, scal[mix][i + 1]["neg_step"], ns).astype(f32)
            for contract in (False, True):
                r = emulate(t["p"], t["g"], t["m"], t["v"], t["k"], cfg, contract, mix=mix, mut=mut, neg_step=ns, skip=skip, H=H)
                r["scalars"] = scal[mix][i]
                res.append(r)
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# plain fp64 and the derived bound
# ---------------------------------------------------------------------------------------------------------------------------------
def adamw_fp64(p, g, m, v, k, cfg):
    """The same step on the same stored inputs and the same fp32 scalars (`host_scalars`), in fp64 with no intermediate rounding.
    -> dict of fp64 arrays: every quantity `bound_fp64` needs."""
    H = {key: (float(val) if not isinstance(val, bool) else val) for key, val in host_scalars(cfg).items()}
    P, G, M0, V0 = (t.double().numpy() for t in (p, g, m, v))
    K0 = k.double().numpy() if cfg["kahan"] else np.zeros_like(P)
    n = p.numel()
    SUMSQ = sumsq_exact(p)
    NORM = math.sqrt(SUMSQ)
    RMS = NORM / math.sqrt(n)
    if cfg["plain"]:
        NS = -(H["prefactor"] * RMS) if RMS > float(f32(1e-3)) else -H["lr_small"]
    else:
        NS = -(H["prefactor"] * max(float(f32(1e-3)), RMS))
    G1 = G * H["gcoef"] if H["clip"] else G
    M = H["a1"] * G1 + H["beta1"] * M0
    V = H["a2"] * G1 * G1 + H["beta2"] * V0
    DEN = np.sqrt(V) + H["eps"]
    Q = M / DEN
    UPD = NS * Q
    if cfg["kahan"]:
        K1 = K0 + UPD
        P1 = P + K1
        ERR = P - P1
        K2 = K1 + ERR          # = 0 up to fp64 rounding: exact arithmetic has nothing to compensate
    else:
        K1 = ERR = K2 = np.zeros_like(P)
        P1 = P + UPD
    P2 = P1 * (1.0 + H["wdf"]) if H["wdf"] != 0 else P1
    return {"p": P2, "m": M, "v": V, "k": K2, "H": H, "G0": G, "G1": G1, "M0": M0, "V0": V0, "K0": K0, "NORM": NORM, "RMS": RMS,
            "NS": NS, "DEN": DEN, "Q": Q, "UPD": UPD, "K1": K1, "P1": P1, "ERR": ERR, "n": n}


def _e(dt):
    """relative error of one fp32 operation followed by rnd<dt>: (1 + 2^-24)(1 + u_dt) - 1"""
    return (1.0 + U32) * (1.0 + U16[dt]) - 1.0


def _op(X, d_in, dt):
    """|rnd<dt>(fl32(x^)) - X| where the exact operands carry the absolute error d_in into the op's exact result x^:
    |x^| <= |X| + d_in, one relative error _e(dt), and half an fp16 subnormal spacing where the target may be subnormal"""
    return d_in * (1.0 + _e(dt)) + np.abs(X) * _e(dt) + TINY[dt]


def bound_fp64(R, cfg):
    """Per element bounds on |emulate - adamw_fp64| for p, m, v, k (either contraction variant), from the operation counts.
    R = adamw_fp64(...).  Every line names the kernel line whose rounding it accounts for; d* are absolute errors."""
    dt, sdt, H = cfg["dt"], cfg["sdt"], R["H"]
    a = np.abs
    # -- the tensor's scalars (:116-119)
    d_norm = _op(R["NORM"], 0.0, dt)                                               # :116 sqrtf, rnd<DT>
    sn = math.sqrt(R["n"])
    d_sn = sn * (U32 + 2.0 ** -52)                                                 # :117 fp64 sqrt, cast to float
    d_rms = _op(R["RMS"], (d_norm + R["RMS"] * d_sn) / (sn - d_sn), dt)            # :117 divide, rnd<DT>
    floor = float(f32(1e-3))
    assert abs(R["RMS"] - floor) > d_rms, "rms within its own error of the 1e-3 floor: the branch is not determined"
    if R["RMS"] <= floor:
        d_ns = 0.0 if cfg["plain"] else abs(R["NS"]) * U32                         # :119 -lr_small itself / :118 one fp32 product
    elif cfg["plain"]:
        d_ns = _op(R["NS"], d_rms * H["prefactor"], dt)                            # :119 product, rnd<DT>
    else:
        d_ns = _op(R["NS"], d_rms * H["prefactor"], F32)                           # :118 product
    # -- the element (:131-148)
    d_g = _op(R["G1"], 0.0, dt) if H["clip"] else 0.0                              # :131 product, rnd<DT>
    d_m1 = _op(H["beta1"] * R["M0"], 0.0, sdt)                                     # :132
    d_m = _op(R["m"], H["a1"] * d_g + d_m1, sdt)                                   # :133 fmaf, rnd<SDT>
    d_v1 = _op(H["beta2"] * R["V0"], 0.0, sdt)                                     # :134
    gg = H["a2"] * R["G1"] ** 2
    d_t = (H["a2"] * (2 * a(R["G1"]) * d_g + d_g ** 2)) * (1 + U32) + gg * U32     # :135 a2 * gf (one fp32 product), times gf exactly
    d_v = _op(R["v"], d_t + d_v1, sdt)                                             # :135 fmaf, rnd<SDT>
    rootV = np.sqrt(R["v"])
    d_s = _op(rootV, np.minimum(d_v / rootV, np.sqrt(d_v)), sdt)                   # :136 |sqrt(v^) - sqrt(V)| <= d_v / sqrt(V), <= sqrt(d_v)
    d_den = _op(R["DEN"], d_s, sdt)                                                # :137
    # an fp16 state whose v underflows (half a subnormal spacing, 2^-25, against v ~ 1e-10) loses its denominator altogether: there
    # plain fp64 says nothing about the update, and the bound is infinite (m and v stay bounded)
    lost = R["DEN"] <= 2 * d_den
    assert sdt is F16 or not lost.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        d_q = ((d_m + a(R["Q"]) * d_den) / (R["DEN"] - d_den)) * (1 + U32) + a(R["Q"]) * U32      # :138 divide
    d_q = np.where(lost, np.inf, d_q)
    with np.errstate(invalid="ignore"):
        d_u = (abs(R["NS"]) * d_q + a(R["Q"]) * d_ns + d_ns * d_q) * (1 + U32) + a(R["UPD"]) * U32    # :138 product (absent when fused)
    d_u = np.where(lost, np.inf, d_u)
    if cfg["kahan"]:
        d_k1 = _op(R["K1"], d_u, dt)                                               # :140
        d_p = _op(R["P1"], d_k1, dt)                                               # :142
        d_err = _op(R["ERR"], d_p, dt)                                             # :143
        d_k = _op(0.0, d_k1 + d_err, dt)                                           # :144 (exact K2 = 0)
    else:
        d_p = _op(R["P1"], d_u, dt)                                                # :146
        d_k = np.zeros_like(d_p)
    if H["wdf"] != 0:
        d_p = _op(R["p"], d_p * abs(1.0 + H["wdf"]), dt)                           # :148 fmaf, rnd<DT>
    slack = 1.0 + 2.0 ** -40                                                       # the fp64 evaluation of these formulas itself
    return {"p": d_p * slack, "m": d_m * slack, "v": d_v * slack, "k": d_k * slack + 2.0 ** -50 * a(R["K1"])}


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
EDGES = [1, 8191, 8192, 8193, 7, 16384, 16385, 3, 24571, 65536, 9, 1]
DEEP = [5, 257 * CHUNK - 5, 8192]
TAILS = list(range(CHUNK - 7, CHUNK + 9))            # every residue mod 8 (and mod 4) on both sides of a chunk
FLOOR_AT = (1, 5)                                    # tensors of the `floor` table that sit below the 1e-3 rms floor


def many_numels(n=301):
    """301 tensors of 1 to 3 chunks with pseudo-random small numels; the first three have 1, 2 and 3 chunks"""
    rs = np.random.RandomState(301)
    out = []
    for i in range(n):
        chunks = 3 if i % 25 == 2 else 2 if i % 10 == 1 else 1
        out.append((chunks - 1) * CHUNK + int(rs.randint(1, 300)))
    return out[:n]


def _round_to(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dt)


def make_tensors(numels, cfg, seed, floor_at=(), overflow=False, dyadic_g=False):
    """The seeded operands of one table: list of dicts p, g, m, v, k (stored dtypes, 1-D), `quantum` (every p is an integer
    multiple of it), `floor`.  Parameters (see `exactness_proof`):
        up to 65536 elements  k / 16, |k| <= amp <= 16 (amp varies from tensor to tensor: no two neighbours share an rms)
        larger                {0, +-0.5}
        floor tensors         k * 2^-14, |k| <= 8   (rms <= 2^-11 < 1e-3; 2^-14 is fp16's smallest normal)
        overflow tensors      one element +-65504 = 2047 * 32 (fp16's largest; with lr = 1e-2 the update leaves the finite range)
    g, m, v >= 0, k: random, already rounded to their dtypes; |g| in [2^-12, 2], |m| in [2^-12, 2], v in [2^-30, 4] (then rounded to
    SDT: fp16 states reach its subnormals and zero), k within a few ulps of p's dtype at p.  No zeros in g or m."""
    dt, sdt = cfg["dt"], cfg["sdt"]
    rs = np.random.RandomState(seed)
    out = []
    for i, n in enumerate(numels):
        fl = i in floor_at
        if overflow:
            quantum = 32.0
        elif fl:
            quantum = 2.0 ** -14
        elif n > 65536:
            quantum = 0.5
        else:
            quantum = 1.0 / 16
        amp = 8 if fl else 1 if n > 65536 else (16, 11, 7, 13, 5, 9)[i % 6]
        kk = rs.randint(-amp, amp + 1, size=n).astype(np.float64)
        sg = np.where(rs.randint(0, 2, size=n) == 0, -1.0, 1.0)
        gmag = 2.0 ** rs.uniform(-12, 1, size=n)
        mmag = 2.0 ** rs.uniform(-12, 1, size=n)
        msg = np.where(rs.randint(0, 2, size=n) == 0, -1.0, 1.0)
        vv = 2.0 ** rs.uniform(-30, 2, size=n)
        if dt is F16 and sdt is F16:   # a v that rounds to zero gives m / eps ~ 2e6 times the step: beyond fp16 parameters' range
            vv = np.maximum(vv, 2.0 ** -24)
        if overflow:   # g and m share a sign, p has the sign of the coming update: |p| grows past fp16's largest
            sg = msg
            kk = -msg * 2047.0
            gmag, mmag, vv = np.clip(gmag, 0.5, 2), np.clip(mmag, 0.5, 2), np.clip(vv, 2.0 ** -4, 4)
        p = _round_to(kk * quantum, dt)
        if dyadic_g:
            g = _round_to(rs.randint(-16, 17, size=n) / 16.0, dt)
        else:
            g = _round_to(sg * gmag, dt)
        m = _round_to(msg * mmag, sdt)
        v = _round_to(vv, sdt)
        k = None
        if cfg["kahan"]:
            ulp_p = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(p.double().numpy()), quantum))) - (10 if dt is F16 else 7))
            k = _round_to(rs.uniform(-3, 3, size=n) * ulp_p, dt)
        below = math.sqrt(float((p.double() ** 2).sum()) / n) < 1e-3    # (a lone zero is below the floor too)
        assert below or not fl
        out.append({"p": p, "g": g, "m": m, "v": v, "k": k, "quantum": quantum, "floor": below, "overflow": overflow})
    return out


def exactness_proof(p, quantum):
    """True iff the sum of squares of p is the same fp32 number in ANY summation order: every element is an integer multiple of
    `quantum` (a power of two), so every square and every partial sum is an integer multiple of quantum^2; the whole sum is below
    2^24 such units, so every partial sum of any subset is an fp32 number and no addition (nor the kernel's fmaf) rounds."""
    x = p.double()
    units = x / quantum
    if not bool((units == units.round()).all()) or math.frexp(quantum)[0] != 0.5:
        return False
    s = float((x * x).sum())
    return s / (quantum * quantum) < 2.0 ** 24 and float(f32(s)) == s and float(f32(s)) == float(np.float64(f32(s)))


def layout(numels, dt, shift):
    """Element offsets of the tensors of one role inside ONE buffer: 64 sentinel elements before and after each tensor, every base a
    multiple of 16 elements (>= 32 bytes: 16-byte aligned for every dtype when the buffer is) plus `shift` elements.
    -> (offsets, buffer length)"""
    offs, cur = [], 0
    for n in numels:
        start = (cur + 64 + 15) // 16 * 16 + shift
        offs.append(start)
        cur = start + n
    return offs, (cur + 64 + 15) // 16 * 16


SENTINEL = 1.5


def pack(tensors, role, dt, shift):
    """one buffer of `role` with the tensors at `layout` and SENTINEL everywhere else -> (buffer, offsets)"""
    numels = [t["p"].numel() for t in tensors]
    offs, total = layout(numels, dt, shift)
    buf = torch.full((total,), SENTINEL, dtype=dt)
    for t, o, n in zip(tensors, offs, numels):
        buf[o:o + n] = t[role]
    return buf, offs


def chunk_begins(numels):
    """the ABI's rule (include/fat5.h): chunk_begin[i] = sum over j < i of ceil(numel[j] / 8192), one terminator"""
    cb, c = [], 0
    for n in numels:
        cb.append(c)
        c += (n + CHUNK - 1) // CHUNK
    return cb + [c]
