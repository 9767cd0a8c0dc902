"""The fp64 restatements of tests/rowwise_fp64.py against the fp32 oracle (oracle/) within fp32 tolerance, and the tanh GELU
against torch's own.  CPU only: these references are the truth of tests/test_rowwise_fp64_gpu.py."""
import pytest
import torch

import oracle
import rowwise_fp64 as R


def _close(a, b, rel=1e-5, abs_=1e-5):
    a, b = a.double(), b.double()
    assert bool(((a - b).abs() <= rel * b.abs() + abs_).all()), float((a - b).abs().max())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("dres", [False, True])
def test_rmsnorm_matches_oracle(dres):
    g = _gen(1)
    x, dy = torch.randn(37, 520, generator=g), torch.randn(37, 520, generator=g)
    w = 1 + 0.1 * torch.randn(520, generator=g)
    y, rstd = R.rmsnorm_fwd(x, w, 1e-6)
    y32, rstd32 = oracle.rmsnorm_fwd_oracle(x, w, 1e-6)
    _close(y, y32)
    _close(rstd, rstd32)
    r = torch.randn(37, 520, generator=g) if dres else None
    dx, dw = R.rmsnorm_bwd(dy, x, w, rstd32, r)
    dx32, dw32 = oracle.rmsnorm_bwd_oracle(dy, x, w, rstd32)
    _close(dx, dx32 + (r if dres else 0))
    _close(dw, dw32, abs_=1e-4)


def test_unit_rmsnorm_bwd_is_rmsnorm_bwd_at_unit_weight():
    g = _gen(2)
    x, gy, r = (torch.randn(9, 256, generator=g) for _ in range(3))
    _, rstd = oracle.rmsnorm_fwd_oracle(x, torch.ones(256), 1e-6)
    dx, xhat = R.unit_rmsnorm_bwd(gy, x, rstd, r)
    dx32, _ = oracle.rmsnorm_bwd_oracle(gy, x, torch.ones(256), rstd)
    _close(dx, dx32 + r)
    _close(xhat, x * rstd.unsqueeze(-1))


def test_fold_weights_by_autograd():
    g = _gen(3)
    ws = [torch.randn(n, 64, generator=g) for n in (8, 16, 24)]
    gw = 1 + 0.1 * torch.randn(64, generator=g)
    dwg = torch.randn(48, 64, generator=g)
    _close(R.fold_weights(ws), torch.cat(ws))
    wl = [t.clone().requires_grad_() for t in ws]
    gl = gw.clone().requires_grad_()
    (torch.cat(wl) * gl).backward(dwg)
    dws, dg = R.fold_weights_bwd(dwg, ws, gw)
    for a, t in zip(dws, wl):
        _close(a, t.grad)
    _close(dg, gl.grad, abs_=1e-4)
    # the oracle's projection through the folded weight
    x = torch.randn(5, 64, generator=g)
    out32, rstd = oracle.rmsnorm_linear_oracle(x, gw, torch.cat(ws), 1e-6)
    _close((x.double() * rstd.double().unsqueeze(-1)) @ R.fold_weights(ws, gw).t(), out32, abs_=1e-4)


@pytest.mark.parametrize("act", ["gelu_tanh", "relu"])
def test_gated_act_matches_oracle_and_torch(act):
    x = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    h1 = torch.cos(x)
    dout = torch.sin(3 * x)
    _close(R.gated_act_fwd(x, h1, act), oracle.gated_act_oracle(x, h1, act), rel=1e-12, abs_=1e-14)
    for a, b in zip(R.gated_act_bwd(dout, x, h1, act), oracle.gated_act_bwd_oracle(dout, x, h1, act)):
        _close(a, b, rel=1e-12, abs_=1e-14)
    xl = x.clone().requires_grad_()
    a = torch.nn.functional.gelu(xl, approximate="tanh") if act == "gelu_tanh" else torch.relu(xl)
    _close(R.gated_act_fwd(x, torch.ones_like(x), act), a.detach(), rel=1e-12, abs_=1e-14)
    (a * h1).backward(dout)
    _close(R.gated_act_bwd(dout, x, h1, act)[0], xl.grad, rel=1e-12, abs_=1e-14)


@pytest.mark.parametrize("smoothing,scale,zs", [(0.0, 1.0, 0.0), (0.1, 1.0, 1e-4), (0.0, 0.5, 1e-2), (0.2, 2.0, 0.0)])
def test_ce_matches_oracle(smoothing, scale, zs):
    g = _gen(4)
    V = 300
    logits = torch.randn(12, V, generator=g) * 3
    labels = torch.randint(0, V, (12,), generator=g)
    labels[2], labels[5], labels[7] = -100, V + 3, -7  # ignored, beyond the vocabulary, negative (not ignored)
    loss, z, lse = R.ce_fwd(logits, labels, smoothing, scale, zs, -100)
    loss32, z32, lse32 = oracle.ce_fwd_oracle(logits, labels, smoothing, scale, zs, -100)
    _close(loss, loss32)
    _close(z, z32)
    _close(lse, lse32)
    dl = torch.randn(12, generator=g)
    _close(R.ce_bwd(dl, logits, labels, smoothing, scale, zs, -100), oracle.ce_bwd_oracle(dl, logits, lse32, labels, smoothing, scale, zs, -100))
    # and against autograd through the fp64 forward, on the rows whose label is in the vocabulary or ignored (a label outside it is
    # the vocabulary-parallel convention: another shard holds it, and the gradient keeps the softmax term its loss lacks here)
    lg = logits.double().requires_grad_()
    (d,) = torch.autograd.grad((R.ce_fwd(lg, labels, smoothing, scale, zs, -100)[0] * dl.double()).sum(), lg)
    keep = ((labels >= 0) & (labels < V)) | (labels == -100)
    _close(R.ce_bwd(dl, logits, labels, smoothing, scale, zs, -100)[keep], d[keep], rel=1e-10, abs_=1e-12)


def test_ce_extreme_rows():
    V = 64
    logits = torch.full((3, V), float("-inf"))
    labels = torch.tensor([0, 40, 63])
    logits[0, 0] = 2.0
    logits[1, 40] = -3.0
    logits[2, 63] = 1e4
    loss, _, lse = R.ce_fwd(logits, labels)
    assert torch.equal(loss, torch.zeros(3, dtype=torch.float64))
    assert torch.equal(lse, torch.tensor([2.0, -3.0, 1e4], dtype=torch.float64))
    assert torch.equal(R.ce_bwd(torch.ones(3), logits, labels), torch.zeros(3, V, dtype=torch.float64))


def test_ulp():
    assert R.ulp(torch.tensor([1.0, 1.5, 2.0, 0.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]
    assert R.ulp(torch.tensor([1.0, 65504.0, 1e-8]), torch.float16).tolist() == [2.0 ** -10, 32.0, 2.0 ** -24]
    assert R.ulp(torch.tensor([1.0, -3.0]), torch.float32).tolist() == [2.0 ** -23, 2.0 ** -22]
