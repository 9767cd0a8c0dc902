"""fp64 restatements of the row-wise operations, written from their definitions (TEST INFRASTRUCTURE ONLY).

Each function takes the tensors a kernel reads -- already rounded to their dtypes -- and returns float64 results: no
intermediate rounding, so the difference between a kernel and these is the kernel's own rounding error, which
tests/test_rowwise_fp64_gpu.py bounds per output.  tests/test_rowwise_fp64_cpu.py pins these to the fp32 oracle (oracle/).

  rmsnorm_fwd       y = x rstd w,  rstd = 1 / sqrt(mean(x^2) + eps)
  rmsnorm_bwd       dx = (w dy - xhat mean(xhat w dy)) rstd (+ dres),  dw = sum_rows dy xhat,  xhat = x rstd
  unit_rmsnorm_bwd  the same with w = 1, and xhat itself
  fold_weights      [W_0; W_1; W_2] diag(g);  backward dW_i = dWg_i diag(g), dg = sum_n dWg W
  gated_act         act(h0) h1 with act = GELU(tanh) or ReLU;  backward (dout h1 act'(h0), dout act(h0))
  ce_fwd / ce_bwd   cross-entropy with label smoothing, logit scale, z-loss, ignore_index and out-of-range labels
"""
import math

import torch

GELU_K = math.sqrt(2.0 / math.pi)
GELU_C = 0.044715

_MANT = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}
_EMIN = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}


def ulp(r, dtype):
    """spacing of `dtype`'s values at |r| (the subnormal spacing below the normal range)"""
    _, e = torch.frexp(r.double().abs())
    e = torch.where(r == 0, torch.full_like(e, _EMIN[dtype] + 1), e)
    return torch.pow(2.0, (e - 1).clamp_min(_EMIN[dtype]).double() - _MANT[dtype])


def _d(t):
    return t.double().cpu()


def rmsnorm_fwd(x, w, eps):
    """-> (y, rstd)"""
    xd = _d(x)
    rstd = 1.0 / torch.sqrt((xd * xd).mean(-1) + eps)
    return xd * rstd.unsqueeze(-1) * _d(w), rstd


def rmsnorm_bwd(dy, x, w, rstd, dres=None):
    """-> (dx, dw); `rstd` is the forward's (the kernel reads it).  dres: the gradient of x's other consumer, added to dx."""
    xd, dyd, wd = _d(x), _d(dy), _d(w)
    r = _d(rstd).unsqueeze(-1)
    xhat = xd * r
    wdy = wd * dyd
    dx = (wdy - xhat * (xhat * wdy).mean(-1, keepdim=True)) * r
    if dres is not None:
        dx = dx + _d(dres)
    return dx, (dyd * xhat).reshape(-1, x.shape[-1]).sum(0)


def unit_rmsnorm_bwd(gy, x, rstd, dres=None):
    """-> (dx, xhat) of xhat = x rstd, given dL/dxhat = gy"""
    xhat = _d(x) * _d(rstd).unsqueeze(-1)
    gyd = _d(gy)
    dx = (gyd - xhat * (xhat * gyd).mean(-1, keepdim=True)) * _d(rstd).unsqueeze(-1)
    if dres is not None:
        dx = dx + _d(dres)
    return dx, xhat


def fold_weights(weights, g=None):
    w = torch.cat([_d(t) for t in weights], 0)
    return w if g is None else w * _d(g)


def fold_weights_bwd(dwg, weights, g):
    """-> ([dW_i], dg)"""
    dd, gd = _d(dwg), _d(g)
    dws, n0 = [], 0
    for t in weights:
        dws.append(dd[n0:n0 + t.shape[0]] * gd)
        n0 += t.shape[0]
    return dws, (dd * fold_weights(weights)).sum(0)


def _act(x, act):
    """(act(x), act'(x)); GELU(approximate='tanh') = x/2 (1 + tanh(u)), u = k (x + c x^3).  Written with s = (1 + tanh u) / 2 =
    sigmoid(2u) and 1 - tanh^2 u = 4 s (1 - s): in fp64, 1 + tanh(u) is 0 below u = -19, where the GELU is still e^(2u) x."""
    if act == "relu":
        return x.clamp_min(0.0), (x > 0).double()
    if act != "gelu_tanh":
        raise ValueError(act)
    s = torch.sigmoid(2 * GELU_K * (x + GELU_C * x ** 3))
    return x * s, s + 2 * x * s * (1 - s) * GELU_K * (1 + 3 * GELU_C * x * x)


def gated_act_fwd(h0, h1, act):
    return _act(_d(h0), act)[0] * _d(h1)


def gated_act_bwd(dout, h0, h1, act):
    """-> (dh0, dh1)"""
    a, da = _act(_d(h0), act)
    g = _d(dout)
    return g * _d(h1) * da, g * a


def ce_fwd(logits, labels, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """-> (loss, z_loss, lse) per row.  Row loss: lse - x_label, or with smoothing s: lse - s mean(x) - (1 - s) x_label; a label
    outside [0, V) picks no logit (s (lse - mean(x)), or 0 without smoothing); z = lse_square_scale lse^2 joins the loss; an
    ignored row has loss = z = 0.  x = logit_scale * logits."""
    x = _d(logits) * logit_scale
    V = x.shape[-1]
    labels = labels.cpu()
    lse = torch.logsumexp(x, -1)
    inb = (labels >= 0) & (labels < V)
    picked = x.gather(-1, labels.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    if smoothing > 0.0:
        mean = x.sum(-1) / V
        loss = torch.where(inb, lse - smoothing * mean - (1 - smoothing) * picked, smoothing * (lse - mean))
    else:
        loss = torch.where(inb, lse - picked, torch.zeros_like(lse))
    z = lse_square_scale * lse * lse
    ign = labels == ignore_index
    zero = torch.zeros_like(lse)
    return torch.where(ign, zero, loss + z), torch.where(ign, zero, z), lse


def ce_bwd(dlosses, logits, labels, smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100, lse=None):
    """-> dlogits = dloss * logit_scale * (p (1 + 2 lse_square_scale lse) - (1 - s) onehot - s / V), p = softmax(x); 0 on ignored
    rows.  `lse` defaults to the exact one."""
    x = _d(logits) * logit_scale
    V = x.shape[-1]
    labels = labels.cpu()
    lse = torch.logsumexp(x, -1) if lse is None else _d(lse)
    p = torch.exp(x - lse.unsqueeze(-1)) * (1 + 2 * lse_square_scale * lse).unsqueeze(-1)
    onehot = torch.zeros_like(p)
    rows = torch.nonzero((labels >= 0) & (labels < V)).squeeze(-1)
    onehot[rows, labels[rows]] = 1.0
    p = p - (1 - smoothing) * onehot - smoothing / V if smoothing > 0.0 else p - onehot
    dl = torch.where(labels == ignore_index, torch.zeros(()).double(), _d(dlosses).expand(labels.shape))
    return (dl * logit_scale).unsqueeze(-1) * p
