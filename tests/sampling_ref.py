"""fp64 restatement of fat5_sample_logits (include/fat5.h, csrc/sample_kernels.h) and a Python Philox4x32-10, for the sampling
tests.  Steps: x = fp32(logit) / fp32(T) in fp32; top-k keeps x >= the k-th largest (duplicates counted); e = exp(x - max) and
S over the kept tokens in fp64; top-p keeps x >= the smallest kept x with C(x) > (1 - p) S; the token is the first kept j whose
inclusive prefix of e exceeds u * S_kept.  `margin` is how close (relative to S) the top-p decision came to its threshold, so a
test can tell the rows whose boundary lies within fp32 rounding of (1 - p) S."""
import math

import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, counter, row):
    """the kernel's u for row `row` at counter offset + offsets[row] (exact: a 24-bit integer times 2^-24)"""
    ctr = int(counter) & 0xFFFFFFFFFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = philox4x32_10((ctr & MASK, ctr >> 32, row, 0), (seed & MASK, seed >> 32))[0]
    return (w0 >> 8) * 2.0 ** -24


def scaled(logits_row, temperature):
    """step 1 in fp32, as the kernel and HF's warper compute it"""
    return (logits_row.float() / torch.tensor(float(temperature), dtype=torch.float32)).numpy()


def restate(x, top_k, top_p):
    """x: fp32 numpy row (no NaN / +inf, not all -inf).  -> dict(tau, kept (bool mask), e (fp64, 0 outside the kept set),
    ratio = S_kept / S, margin)"""
    V = x.shape[0]
    xd = x.astype(np.float64)
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        tau_k = np.sort(xd)[::-1][top_k - 1]
        keep = xd >= tau_k
    m = xd.max()
    e = np.where(keep, np.exp(xd - m), 0.0)
    S = e.sum()
    margin = math.inf
    if top_p < 1.0:
        thr = (1.0 - float(np.float32(top_p))) * S
        vals = np.unique(xd[keep])  # ascending
        mass = np.array([e[keep & (xd == v)].sum() for v in vals]) if len(vals) < 4096 else None
        if mass is None:  # (long rows: group by value through a sort)
            order = np.argsort(xd[keep], kind="stable")
            sx, se = xd[keep][order], e[keep][order]
            idx = np.searchsorted(vals, sx)
            mass = np.bincount(idx, weights=se, minlength=len(vals))
        C = np.cumsum(mass)
        first = int(np.argmax(C > thr))
        keep = keep & (xd >= vals[first])
        margin = float(np.min(np.abs(C - thr)) / S)
    ek = np.where(keep, e, 0.0)
    return dict(tau=float(x[keep].min()), kept=keep, e=ek, ratio=ek.sum() / S, margin=margin)


def draw(r, u, tol=0.0):
    """the inverse-CDF token(s) of a restated row for uniform u: the first kept j whose inclusive prefix exceeds u * S_kept --
    with tol > 0 every kept j whose prefix interval lies within tol * S_kept of the target (either neighbour of a boundary)"""
    e = r["e"]
    P = np.cumsum(e)
    Sk = P[-1]
    t = u * Sk
    excl = P - e
    if tol == 0.0:
        j = int(np.argmax(P > t))
        return {j}
    ok = r["kept"] & (e > 0) & (excl <= t + tol * Sk) & (P > t - tol * Sk)
    return set(np.nonzero(ok)[0].tolist())


def argmax_rule(x):
    """torch.argmax's index on a degenerate row: the first NaN, else the first +inf, else (all -inf) 0"""
    return int(torch.argmax(torch.from_numpy(np.ascontiguousarray(x))))
