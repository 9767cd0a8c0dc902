"""Restatement of `flasht5_amd.sequence_pool` (include/fat5.h, "Sequence pooling") in loops, fp64 on the CPU: both layouts, the four
modes and the backward -- and the bound its "mean" mode is held to.

The bound is derived, not fitted.  For a column of n = len values x_i summed in fp32 in ANY order, the computed sum S satisfies
|S - sum x_i| <= gamma(n - 1) * sum |x_i| (Higham, Accuracy and Stability, 4.2), gamma(c) = c u / (1 - c u), u = 2^-24; the fp32
division by n and a possible second rounding add two more factors (1 + delta), so with A = (sum |x_i|) / n

    |y - ref| <= e + ulp_T(|ref| + e) / 2,     e = gamma(n + 2) * A,

the last term being the one rounding to the output dtype T of a value that lies within e of ref.  The backward is one division and
one rounding: the same form with c = 2 and A = |ref|."""
import torch

U = 2.0 ** -24
MODES = ("eos", "first", "last", "mean")
_PREC = {torch.float32: (24, -149), torch.float16: (11, -24), torch.bfloat16: (8, -133)}   # significand bits, log2 of the smallest subnormal


def gamma(c):
    return c * U / (1.0 - c * U)


def ulp(v, dtype):
    """the spacing of dtype's numbers at |v| (fp64 tensor in, fp64 tensor out); the subnormal spacing below the normal range"""
    p, emin = _PREC[dtype]
    _, e = torch.frexp(v.double().abs())          # |v| = m * 2^e, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, emin + p), e)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - p).clamp(min=emin).double())


def spans(shape, cu_seqlens=None, seqlens=None):
    """[(first flat row, length)] per sequence, lengths clamped as the kernel clamps them"""
    clamp = lambda v, hi: min(max(int(v), 0), hi)  # noqa: E731
    if cu_seqlens is not None:
        total = shape[0]
        cu = [clamp(v, total) for v in cu_seqlens.tolist()]
        return [(cu[b], max(cu[b + 1] - cu[b], 0)) for b in range(len(cu) - 1)]
    B, L = shape[0], shape[1]
    lens = [L] * B if seqlens is None else [clamp(v, L) for v in seqlens.tolist()]
    return [(b * L, lens[b]) for b in range(B)]


def pool_ref(hidden, mode, cu_seqlens=None, seqlens=None, input_ids=None, eos_token_id=1):
    """hidden: a CPU tensor (total, d) with cu_seqlens or (B, L, d) -> dict(pooled (nseq, d) fp64, position, found (lists),
    absmean (nseq, d) fp64 = A of the bound, lens)"""
    assert mode in MODES
    d = hidden.shape[-1]
    rows = hidden.double().reshape(-1, d)
    ids = None if input_ids is None else input_ids.reshape(-1).tolist()
    sp = spans(hidden.shape, cu_seqlens, seqlens)
    pooled = torch.zeros(len(sp), d, dtype=torch.float64)
    absmean = torch.zeros(len(sp), d, dtype=torch.float64)
    position, found = [], []
    for b, (s, n) in enumerate(sp):
        if n == 0:
            position.append(-1)
            found.append(0)
            continue
        if mode == "mean":
            acc = torch.zeros(d, dtype=torch.float64)
            aabs = torch.zeros(d, dtype=torch.float64)
            for j in range(n):
                acc += rows[s + j]
                aabs += rows[s + j].abs()
            pooled[b] = acc / n
            absmean[b] = aabs / n
            position.append(-1)
            found.append(1)
            continue
        pos, hit = {"first": 0, "last": n - 1, "eos": n - 1}[mode], 1
        if mode == "eos":
            hits = [j for j in range(n) if ids[s + j] == eos_token_id]
            hit = 1 if hits else 0
            if hits:
                pos = hits[-1]
        pooled[b] = rows[s + pos]
        position.append(pos)
        found.append(hit)
    return dict(pooled=pooled, position=position, found=found, absmean=absmean, lens=[n for _, n in sp])


def pool_bwd_ref(dpooled, shape, mode, position, cu_seqlens=None, seqlens=None):
    """dhidden fp64 of `shape`: dpooled[b] at the saved position (gather modes) or dpooled[b] / len on the valid rows (mean)"""
    d = shape[-1]
    dh = torch.zeros(shape, dtype=torch.float64).reshape(-1, d)
    dp = dpooled.double()
    for b, (s, n) in enumerate(spans(shape, cu_seqlens, seqlens)):
        if mode == "mean":
            for j in range(n):
                dh[s + j] = dp[b] / n
        elif n > 0 and 0 <= position[b] < n:
            dh[s + position[b]] = dp[b]
    return dh.reshape(shape)


def mean_bound(ref, absmean, lens, dtype):
    """(nseq, d) fp64: the most |y - ref| may be for the forward of "mean" """
    n = torch.tensor(lens, dtype=torch.float64).unsqueeze(1)
    e = gamma(n + 2) * absmean
    return e + ulp(ref.abs() + e, dtype) / 2


def mean_bwd_bound(ref, dtype):
    """the same for the backward: one division, one rounding"""
    e = gamma(2.0) * ref.abs()
    return e + ulp(ref.abs() + e, dtype) / 2


def check_pool(got, ref, mode, dtype):
    """the kernel's (pooled, position, found) against pool_ref's dict: gather modes exact, "mean" inside its bound"""
    pooled, position, found = got
    assert position.tolist() == ref["position"], (mode, position.tolist(), ref["position"])
    assert found.tolist() == ref["found"], (mode, found.tolist(), ref["found"])
    assert pooled.dtype == dtype
    if mode == "mean":
        err = (pooled.double().cpu() - ref["pooled"]).abs()
        bound = mean_bound(ref["pooled"], ref["absmean"], ref["lens"], dtype)
        assert bool((err <= bound).all()), (mode, float((err - bound).max()))
    else:
        assert torch.equal(pooled.cpu(), ref["pooled"].to(dtype)), mode


def check_pool_bwd(dhidden, ref, mode, dtype):
    assert not bool(torch.isnan(dhidden.float()).any()), mode
    if mode == "mean":
        err = (dhidden.double().cpu() - ref).abs()
        assert bool((err <= mean_bwd_bound(ref, dtype)).all()), (mode, float(err.max()))
    else:
        assert torch.equal(dhidden.cpu(), ref.to(dtype)), mode
