"""Transient-global attention (csrc/tglobal_attn_kernels.h) against a plain fp64 restatement: dense band scores and the scores of
GIVEN global keys under their two tables, one softmax over both, gradients from autograd.  Bounds: test_attention_gpu.py's `bound` /
`gbound`; both table gradients per entry with the allowance of test_local_attn_gpu.py; exact zeros where no pair reaches."""
import pytest
import torch

from test_attention_gpu import bound, gbound

pytestmark = pytest.mark.gpu

SCALE = 0.125


def _ref(q, k, v, gk, gv, do, r1, g1, R, Rg, window):
    """q, k, v, do: (B, H, S, D); gk, gv: (B, H, S // 16, D).  Returns o, (dq, dk, dv, dgk, dgv) and per table (gradient, sum of dS^2,
    pair count) per entry."""
    q, k, v, gk, gv = (t.double().requires_grad_() for t in (q, k, v, gk, gv))
    S, G, H = q.shape[2], gk.shape[2], q.shape[1]
    pos, gpos = torch.arange(S, device=q.device), torch.arange(G, device=q.device)
    d = pos[None, :] - pos[:, None]                                   # n - m
    dg = gpos[None, :] - (pos // 16).clamp(max=G - 1)[:, None]        # g - blk(m)
    idx, gidx = (d.clamp(-R, R) + R).flatten(), (dg.clamp(-Rg, Rg) + Rg).flatten()
    s, sg = (q @ k.transpose(-1, -2)) * SCALE, (q @ gk.transpose(-1, -2)) * SCALE
    tabs = [t.double().requires_grad_() for t in (r1, g1)] if r1 is not None else []
    if tabs:
        s, sg = s + tabs[0][:, idx].view(1, H, S, S), sg + tabs[1][:, gidx].view(1, H, S, G)
    p = torch.softmax(torch.cat((s.masked_fill(d.abs() > window, float("-inf")), sg), -1), -1)
    o = p[..., :S] @ v + p[..., S:] @ gv
    dq, dk, dv, dgk, dgv, ds, dsg, *dt = torch.autograd.grad(o, [q, k, v, gk, gv, s, sg] + tabs, do.double())
    stats = []
    for n, ix, e, vis in ((2 * R + 1, idx, ds, (d.abs() <= window).double()), (2 * Rg + 1, gidx, dsg, torch.ones_like(dg).double())):
        sq = torch.zeros(H, n, dtype=torch.float64, device=q.device).index_add_(1, ix, (e * e).sum(0).flatten(1))
        cnt = torch.zeros(n, dtype=torch.float64, device=q.device).index_add_(0, ix, vis.flatten())
        stats.append([dt.pop(0) if dt else None, sq, cnt])
    return o.detach(), (dq, dk, dv, dgk, dgv), stats


def _run(ts, r1, g1, R, Rg, window, cu=None, cu_g=None, mx=None):
    from flasht5_amd import flash_attention_v2_rpe1d, flash_attn_varlen_func
    q, k, v, gk, gv, do = ts
    lv = [t.detach().requires_grad_() for t in (q, k, v, gk, gv)] + ([t.detach().requires_grad_() for t in (r1, g1)] if r1 is not None else [])
    r, g = (lv[5], lv[6]) if r1 is not None else (None, None)
    kw = dict(window=window, global_kv=(lv[3], lv[4]), global_rpe1d=g, global_radius=Rg if g is not None else None)
    if cu is None:
        o = flash_attention_v2_rpe1d(lv[0], lv[1], lv[2], r, R, False, SCALE, **kw)
    else:
        o = flash_attn_varlen_func(lv[0], lv[1], lv[2], cu, cu, mx, mx, False, SCALE, r, R, cu_seqlens_g=cu_g, **kw)
    return [o.detach()] + list(torch.autograd.grad(o, lv, do))


CASES = [  # (B, H, S) or packed lengths, window, global radius (None: no tables), layout
    ((1, 2, 15), 127, 128, "dense"),        # G = 0: the windowed operator
    ((1, 2, 40), 127, 128, "dense"),        # G = 2, 8 orphans, one ragged block
    ((2, 2, 200), 1, 128, "strided"),       # narrowest band; the model's (B, S, H, D) storage
    ((2, 3, 333), 100, 4, "strided"),       # Rg = 4 < G - 1: the global table's clamp ends collect gradient; B * H > 1 in the reduction
    ((1, 2, 1047), 64, 128, "dense"),       # G = 65: a second global tile holding one key; 7 orphans; several dgK / dgV Q-tiles
    ((1, 2, 300), 127, None, "dense"),      # no-bias body
    ((70, 1, 257, 15, 64), 100, 128, "packed"),  # H = 2: G = 4, 0, 16, 0, 4 (cu_seqlens_g repeats entries); a sequence ends inside a block
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape,window,g_radius,layout", CASES)
def test_tglobal_matches_fp64(shape, window, g_radius, layout, dtype):
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + window)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    R, Rg = 128, g_radius or 1
    H = 2 if layout == "packed" else shape[1]
    r1, g1 = (rnd(H, 2 * R + 1) * 0.5, rnd(H, 2 * Rg + 1) * 0.5) if g_radius else (None, None)
    if layout == "packed":
        total = sum(shape)
        q, k, v, do = (rnd(total, H, 64).to(dtype) for _ in range(4))
        gk, gv = (rnd(total // 16, H, 64).to(dtype) for _ in range(2))
        ends = [sum(shape[:i]) for i in range(len(shape) + 1)]
        gends = [sum(n // 16 for n in shape[:i]) for i in range(len(shape) + 1)]
        cu, cu_g = (torch.tensor(e, dtype=torch.int32, device="cuda") for e in (ends, gends))
        got = _run((q, k, v, gk, gv, do), r1, g1, R, Rg, window, cu, cu_g, max(shape))
        again = _run((q, k, v, gk, gv, do), r1, g1, R, Rg, window, cu, cu_g, max(shape))
        seq = lambda t, a, b: t[a:b].transpose(0, 1)[None]
        refs = [_ref(*(seq(t, a, b) for t in (q, k, v)), seq(gk, c, d), seq(gv, c, d), seq(do, a, b), r1, g1, R, Rg, window)
                for a, b, c, d in zip(ends, ends[1:], gends, gends[1:])]
        ro = torch.cat([x[0][0].transpose(0, 1) for x in refs])
        rg = [torch.cat([x[1][i][0].transpose(0, 1) for x in refs]) for i in range(5)]
        rt = [[sum(x[2][t][i] for x in refs) for i in range(3)] for t in range(2)]
    else:
        B, _, S = shape
        if layout == "strided":
            mk = lambda n: rnd(B, n, H, 64).to(dtype).permute(0, 2, 1, 3)
        else:
            mk = lambda n: rnd(B, H, n, 64).to(dtype)
        q, k, v, do, gk, gv = mk(S), mk(S), mk(S), mk(S), mk(S // 16), mk(S // 16)
        got = _run((q, k, v, gk, gv, do), r1, g1, R, Rg, window)
        again = _run((q, k, v, gk, gv, do), r1, g1, R, Rg, window)
        ro, rg, rt = _ref(q, k, v, gk, gv, do, r1, g1, R, Rg, window)
        if S < 16:
            from flasht5_amd import flash_attention_v2_rpe1d
            assert torch.equal(got[0], flash_attention_v2_rpe1d(q, k, v, r1, R, False, SCALE, window=window))
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    if layout == "packed":  # the rows of gk / gv past cu_seqlens_g[-1] belong to no sequence
        assert not bool(got[4][gends[-1]:].any()) and not bool(got[5][gends[-1]:].any())
        got[4], got[5] = got[4][:gends[-1]], got[5][:gends[-1]]
    err =lambda a, b: (a.double() - b.double()).abs().max().item() if b.numel() else 0.0
    print(f"o {err(got[0], ro):.3e} / {bound(ro, dtype):.3e}")
    assert err(got[0], ro) <= bound(ro, dtype)
    for name, a, b in zip(("dq", "dk", "dv", "dgk", "dgv"), got[1:6], rg):
        assert a.shape == b.shape and torch.isfinite(a.float()).all(), name
        if b.numel():
            print(f"{name} {err(a, b):.3e} / {gbound(b, dtype):.3e}")
            assert err(a, b) <= gbound(b, dtype), name
    if g_radius:
        for name, have, (want, sq, cnt) in zip(("drpe1d", "dgrpe1d"), got[6:8], rt):
            e = (have.double() - want).abs()
            allow = 4.0 * 2.0 ** -9 / 3 ** 0.5 * sq.sqrt() + 2e-3 * max(1.0, want.abs().max().item()) + 1e-2
            print(f"{name} {e.max().item():.3e} / {allow.max().item():.3e}")
            assert bool((e <= allow).all()), (name, e.max().item(), allow.max().item())
            assert bool((have[:, cnt == 0] == 0).all()), name  # entries no pair reaches


def test_tglobal_host_rejections():
    from flasht5_amd import flash_attention_v2_rpe1d
    t = lambda S, D=64: torch.zeros(1, 2, S, D, dtype=torch.bfloat16, device="cuda")
    r1, g1 = torch.zeros(2, 17, device="cuda"), torch.zeros(2, 9, device="cuda")
    ok = dict(q=t(32), gk=t(2), causal=False, window=4, r=r1, g=g1)
    for bad in (dict(window=None), dict(causal=True), dict(q=t(32, 128), gk=t(2, 128)), dict(gk=t(3)), dict(gk=t(2).half()), dict(g=None),
                dict(r=None)):
        c = {**ok, **bad}
        with pytest.raises(ValueError):
            flash_attention_v2_rpe1d(c["q"], c["q"], c["q"], c["r"], 8, c["causal"], None, window=c["window"], global_kv=(c["gk"], c["gk"]),
                                     global_rpe1d=c["g"], global_radius=4)
