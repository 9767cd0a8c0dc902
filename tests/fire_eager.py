"""Eager restatement of the reference's FIRE producer (src/utils/positional_encoding.py:341-417) for the FIRE tests, plus the
per-entry error scales the kernels are held to (the sums of the absolute values of each quantity's terms)."""
import torch


def fire_eager(w1, b1, w2, b2, c, lm, l0, M, N, eps=1e-6, dtype=torch.float64, rows=None):
    """(1, H, M, N) bias, differentiable in every argument tensor; all arithmetic in `dtype`; `rows`: only those query rows"""
    cast = lambda t: torch.as_tensor(t).to(dtype)  # noqa: E731
    w1, b1, w2, b2, c, lm, l0 = (cast(t) for t in (w1, b1, w2, b2, c, lm, l0))
    dev = w2.device
    pi = torch.arange(M, dtype=dtype, device=dev) if rows is None else torch.as_tensor(rows, device=dev).to(dtype)
    pj = torch.arange(N, dtype=dtype, device=dev)
    d = pi[:, None] - pj[None, :]
    T = torch.abs(lm * l0)
    P = torch.max(pi, T)[:, None]
    num = torch.sign(d) * torch.log(torch.abs(c * d) + 1)
    den = torch.log(torch.abs(c * P) + 1) + eps
    x = num / den
    a = x[..., None] * w1.reshape(-1) + b1
    out = torch.relu(a) @ w2.t() + b2
    return out.permute(2, 0, 1).unsqueeze(0)


def _parts(w1, b1, w2, b2, c, lm, l0, M, N, eps, dev, rows=None):
    f = lambda t: torch.as_tensor(t).to(torch.float64).to(dev)  # noqa: E731
    w1, b1, w2, b2, c, lm, l0 = (f(t) for t in (w1, b1, w2, b2, c, lm, l0))
    pi = torch.arange(M, dtype=torch.float64, device=dev) if rows is None else torch.as_tensor(rows, device=dev).to(torch.float64)
    pj = torch.arange(N, dtype=torch.float64, device=dev)
    d = pi[:, None] - pj[None, :]
    T = torch.abs(lm * l0)
    P = torch.max(pi, T)[:, None]
    den = torch.log(torch.abs(c * P) + 1) + eps
    x = torch.sign(d) * torch.log(torch.abs(c * d) + 1) / den
    a = x[..., None] * w1.reshape(-1) + b1
    return w1.reshape(-1), b1, w2, b2, c, lm, l0, d, T, P, den, x, a


def fwd_scale(w1, b1, w2, b2, c, lm, l0, M, N, eps=1e-6, dev="cpu", rows=None):
    """(1, H, M, N): |b2[h]| + sum_k |w2[h,k]| (|w1[k] x| + |b1[k]|)"""
    w1, b1, w2, b2, c, lm, l0, d, T, P, den, x, a = _parts(w1, b1, w2, b2, c, lm, l0, M, N, eps, dev, rows)
    t = (x[..., None] * w1).abs() + b1.abs()
    return (t @ w2.abs().t() + b2.abs()).permute(2, 0, 1).unsqueeze(0)


def bwd_scale(G, w1, b1, w2, b2, c, lm, l0, M, N, eps=1e-6):
    """per gradient entry, the fp64 sum of the absolute values of its terms: dict name -> tensor of the parameter's shape"""
    dev = G.device
    w1, b1, w2, b2, c, lm, l0, d, T, P, den, x, a = _parts(w1, b1, w2, b2, c, lm, l0, M, N, eps, dev)
    Ga = G.to(torch.float64).abs().reshape(-1, M, N).permute(1, 2, 0)  # (M, N, H)
    on = (a > 0).to(torch.float64)
    r = torch.relu(a)
    ga = (Ga @ w2.abs()) * on  # |dL/da| bound, (M, N, W)
    dx = ga @ w1.abs()         # (M, N)
    dnum = dx / den
    dden = dx * x.abs() / den
    u = torch.abs(c * d) + 1
    v = torch.abs(c * P) + 1
    tie = torch.where(torch.arange(M, dtype=torch.float64, device=dev)[:, None] < T, 1.0,
                      torch.where(torch.arange(M, dtype=torch.float64, device=dev)[:, None] == T, 0.5, 0.0))
    dc = (dnum / u * d.abs()).sum() + (dden / v * P).sum()
    dT = (dden / v * c.abs() * tie).sum()
    return {
        "w1": (ga * x.abs()[..., None]).sum((0, 1)).reshape(-1, 1), "b1": ga.sum((0, 1)),
        "w2": torch.einsum("mnh,mnk->hk", Ga, r), "b2": Ga.sum((0, 1)),
        "c": dc, "L_multiplier": dT * l0.abs(),
    }
