"""Local (sliding-window) attention (csrc/local_attn_kernels.h) against a plain fp64 restatement: dense scores + band mask + bias from
rpe1d, softmax, gradients from autograd.  Bounds: test_attention_gpu.py's `bound` / `gbound`; the table gradient per diagonal with
the 4-sigma allowance plus slack of test_bwd64_gpu.py (::_table_truth and its assertion), restated per diagonal."""
import pytest
import torch

from test_attention_gpu import bound, gbound

pytestmark = pytest.mark.gpu

SCALE = 0.125


def _ref(q, k, v, do, r1, radius, window):
    """q, k, v, do: (B, H, S, D).  Returns o, (dq, dk, dv), and per table entry: gradient, sum of dS^2, visible-pair count."""
    q, k, v = (t.double().requires_grad_() for t in (q, k, v))
    S = q.shape[2]
    pos = torch.arange(S, device=q.device)
    d = pos[None, :] - pos[:, None]  # n - m
    s = (q @ k.transpose(-1, -2)) * SCALE
    idx = (d.clamp(-radius, radius) + radius).flatten()
    r = r1.double().requires_grad_() if r1 is not None else None
    if r is not None:
        s = s + r[:, idx].view(1, -1, S, S)
    o = torch.softmax(s.masked_fill(d.abs() > window, float("-inf")), -1) @ v
    dq, dk, dv, ds, *dr = torch.autograd.grad(o, [q, k, v, s] + ([r] if r is not None else []), do.double())
    H = q.shape[1]
    sq = torch.zeros(H, 2 * radius + 1, dtype=torch.float64, device=q.device).index_add_(1, idx, (ds * ds).sum(0).flatten(1))
    cnt = torch.zeros(2 * radius + 1, dtype=torch.float64, device=q.device).index_add_(0, idx, (d.abs() <= window).double().flatten())
    return o.detach(), (dq, dk, dv), (dr[0] if dr else None, sq, cnt)


def _run(q, k, v, do, r1, radius, window, cu=None, mx=None):
    from flasht5_amd import flash_attention_v2_rpe1d, flash_attn_varlen_func
    leaves = [t.detach().requires_grad_() for t in (q, k, v)] + ([r1.detach().requires_grad_()] if r1 is not None else [])
    r = leaves[3] if r1 is not None else None
    if cu is None:
        o = flash_attention_v2_rpe1d(leaves[0], leaves[1], leaves[2], r, radius, False, SCALE, window=window)
    else:
        o = flash_attn_varlen_func(leaves[0], leaves[1], leaves[2], cu, cu, mx, mx, False, SCALE, r, radius, window=window)
    return [o.detach()] + list(torch.autograd.grad(o, leaves, do))


CASES = [  # (B, H, S) or packed lengths, window, radius (None: no bias), layout
    ((1, 2, 40), 127, 128, "dense"),       # window >= S - 1: full attention, one ragged block
    ((2, 2, 200), 1, 128, "strided"),      # narrowest band; S not a tile multiple
    ((1, 2, 300), 64, 128, "dense"),       # band edge on a tile boundary
    ((2, 3, 333), 100, 128, "strided"),    # band edge inside tiles, ragged tail, B * H > 1 for the diagonal reduction
    ((1, 2, 700), 127, 128, "dense"),      # the LongT5 setting: interior blocks have whole skipped tiles on both sides
    ((1, 2, 400), 200, 32, "dense"),       # window > radius: the clamp ends collect gradient
    ((1, 2, 300), 127, None, "dense"),     # no-bias body
    ((70, 1, 257, 64), 100, 128, "packed"),  # H = 2: sequence ends inside a block, a 1-token sequence, masked neighbours in reach
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape,window,radius,layout", CASES)
def test_local_matches_fp64(shape, window, radius, layout, dtype):
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + window)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    R = radius or 1
    r1 = rnd(2 if layout == "packed" else shape[1], 2 * R + 1) * 0.5 if radius else None
    if layout == "packed":
        H, total = 2, sum(shape)
        q, k, v, do = (rnd(total, H, 64).to(dtype) for _ in range(4))
        bounds = [sum(shape[:i]) for i in range(len(shape) + 1)]
        cu = torch.tensor(bounds, dtype=torch.int32, device="cuda")
        got = _run(q, k, v, do, r1, R, window, cu, max(shape))
        again = _run(q, k, v, do, r1, R, window, cu, max(shape))
        refs = [_ref(*(t[a:b].transpose(0, 1)[None] for t in (q, k, v, do)), r1, R, window) for a, b in zip(bounds, bounds[1:])]
        ro = torch.cat([x[0][0].transpose(0, 1) for x in refs])
        rg = [torch.cat([x[1][i][0].transpose(0, 1) for x in refs]) for i in range(3)]
        rt = [sum(x[2][i] for x in refs) for i in range(3)]
    else:
        B, H, S = shape
        if layout == "strided":  # the model's (B, S, H, D) storage
            q, k, v, do = (rnd(B, S, H, 64).to(dtype).permute(0, 2, 1, 3) for _ in range(4))
        else:
            q, k, v, do = (rnd(B, H, S, 64).to(dtype) for _ in range(4))
        got = _run(q, k, v, do, r1, R, window)
        again = _run(q, k, v, do, r1, R, window)
        ro, rg, rt = _ref(q, k, v, do, r1, R, window)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    err = lambda a, b: (a.double() - b.double()).abs().max().item()
    print(f"o {err(got[0], ro):.3e} / {bound(ro, dtype):.3e}")
    assert err(got[0], ro) <= bound(ro, dtype)
    for name, a, b in zip(("dq", "dk", "dv"), got[1:4], rg):
        assert torch.isfinite(a.float()).all(), name
        print(f"{name} {err(a, b):.3e} / {gbound(b, dtype):.3e}")
        assert err(a, b) <= gbound(b, dtype), name
    if radius:
        want, sq, cnt = rt
        e = (got[4].double() - want).abs()
        allow = 4.0 * 2.0 ** -9 / 3 ** 0.5 * sq.sqrt() + 2e-3 * max(1.0, want.abs().max().item()) + 1e-2
        print(f"drpe1d {e.max().item():.3e} / {allow.max().item():.3e}")
        assert bool((e <= allow).all()), (e.max().item(), allow.max().item())
        assert bool((got[4][:, cnt == 0] == 0).all())  # entries no diagonal reaches
        assert bool((cnt == 0).any()) == (window < R)


def test_local_host_rejections():
    from flasht5_amd import flash_attention_v2_rpe1d
    t = lambda S, D=64: torch.zeros(1, 2, S, D, dtype=torch.bfloat16, device="cuda")
    r1 = torch.zeros(2, 17, device="cuda")
    for q, k, causal, window in ((t(32), t(32), True, 4), (t(32), t(48), False, 4), (t(32, 128), t(32, 128), False, 4), (t(32), t(32), False, 0)):
        with pytest.raises(ValueError):
            flash_attention_v2_rpe1d(q, k, k, r1, 8, causal, None, window=window)
