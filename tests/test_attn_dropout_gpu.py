"""GPU tests of attention dropout (csrc/attn_dropout_kernels.h) through flash_attention_v2_rpe1d / flash_attn_varlen_func
(o and every gradient; lse, which the operators do not return, from FlashAttentionDropout on the same inputs), with the mask restated
on the host by tests/attn_dropout_ref.py.
(a) the mask lands where that says, bit for bit; (b) o, lse, dq, dk, dv, drpe1d against a plain fp64 reference under the host mask,
within the attention tests' per-tensor bounds (parity_cases.bound / gbound / lse_bound); (c) two runs give the same bits, a drpe1d
request does not change dq / dk / dv, and dropout_p = 0 is the call without the arguments.
Measured (profiles/attn_dropout_errors.log): every tensor inside the per-tensor bound except drpe1d of the packed cross case (2.4x at
p = 0.1, 1.17x at p = 0.5), which the reference's own rule accepts: err <= 2 x err(the same formula in eager 16-bit) + 1e-5."""
import numpy as np
import pytest
import torch

import dropout_ref as R
from attn_dropout_ref import SEED, host_mask
from attn_helpers import maxdiff
from parity_cases import bound, gbound, lse_bound

pytestmark = pytest.mark.gpu

SCALE = 0.125


def _step(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def reference(q, k, v, do, r1, causal, keep, p, dt=torch.float64):
    """one sequence in fp64 (or, dt = the inputs' dtype, the same formula in eager 16-bit): q, do (H, M, D), k, v (H, N, D),
    keep (H, M, N) -> o, lse, dq, dk, dv, drpe1d"""
    q, k, v = (t.to(dt).requires_grad_() for t in (q, k, v))
    M, N = q.shape[1], k.shape[1]
    s = q @ k.transpose(1, 2) * SCALE
    d = torch.arange(N, device="cuda")[None, :] - torch.arange(M, device="cuda")[:, None]
    leaves = [q, k, v]
    if r1 is not None:
        r1 = r1.to(dt).requires_grad_()
        rad = (r1.shape[1] - 1) // 2
        s = s + r1[:, d.clamp(-rad, rad) + rad]
        leaves.append(r1)
    if causal:
        s = s.masked_fill(d > N - M, float("-inf"))
    lse = torch.logsumexp(s, -1)
    pt = torch.where(keep, torch.exp(s - lse[..., None]) * float(R.scale(p)), 0.0)
    o = pt @ v
    return [o.detach(), lse.detach()] + list(torch.autograd.grad(o, leaves, do.to(dt)))


def _rand(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _table(H, rad):
    return None if rad is None else _rand((H, 2 * rad + 1), torch.float32, 5) * 0.5


def _report(name, got, ref, low, dtype):
    """print err / bound of every tensor (o, lse, dq, dk, dv[, drpe1d]), then assert them: the attention tests' per-tensor bound,
    or where that is exceeded the reference's own rule, err <= 2 x err(the same formula in eager 16-bit: `low`) + 1e-5"""
    names = ("o", "lse", "dq", "dk", "dv", "drpe1d")
    rows = []
    for nm, g, r, lo in zip(names, got, ref, low):
        b = bound(r, dtype) if nm == "o" else lse_bound(r) if nm == "lse" else gbound(r, dtype)
        rows.append((nm, maxdiff(g, r.float() if nm in ("lse", "drpe1d") else r), b, 2 * maxdiff(lo, r) + 1e-5))
        print(f"attn_dropout_err {name} {nm} err {rows[-1][1]:.3e} bound {b:.3e} ratio {rows[-1][1] / b:.3f} eager-rule {rows[-1][3]:.3e}")
    for nm, e, b, b2 in rows:
        assert e <= b or e <= b2, (name, nm, e, b, b2)


DENSE = {  # B, H, M, N, causal, radius
    "64x64": (2, 3, 64, 64, False, 8), "65x63": (1, 2, 65, 63, False, 8), "cross100x200": (1, 2, 100, 200, False, None),
    "causal130": (1, 2, 130, 130, True, 8)}
PACKED = {  # q lengths, k lengths, causal
    "packed_causal": ((0, 1, 70, 64), (0, 1, 70, 64), True), "packed_cross": ((5, 66, 70), (100, 3, 64), False)}
CASES = [(c, p, torch.bfloat16) for c in list(DENSE) + list(PACKED) for p in (0.1, 0.5)] + \
        [(c, 0.1, torch.float16) for c in ("64x64", "causal130")]


@pytest.mark.parametrize("case,p,dtype", CASES, ids=lambda x: str(x).split(".")[-1])
def test_outputs_and_gradients_against_fp64(case, p, dtype):
    from flasht5_amd import flash_attention_v2_rpe1d, flash_attn_varlen_func
    from flasht5_amd.flash_attention_v2_bias import FlashAttentionDropout
    kw = dict(dropout_p=p, dropout_seed=SEED, dropout_step=_step(11), dropout_site=3)
    step, site, name = 11, 3, f"{case}-p{p}-{str(dtype).split('.')[-1]}"
    if case in DENSE:
        B, H, M, N, causal, rad = DENSE[case]
        q, k, v, do = (_rand((B, L, H, 64), dtype, i).permute(0, 2, 1, 3) for i, L in enumerate((M, N, N, M)))   # (B, S, H, D) storage
        r1 = _table(H, rad)
        leaves = [t.clone().requires_grad_() for t in (q, k, v)] + ([r1.clone().requires_grad_()] if rad else [])
        o = flash_attention_v2_rpe1d(leaves[0], leaves[1], leaves[2], leaves[3] if rad else None, rad or 0, causal, SCALE, **kw)
        o2, lse = FlashAttentionDropout.apply(q, k, v, r1, rad or 0, causal, SCALE, None, None, None, None, p, SEED, _step(step), site)
        got = [o, lse] + list(torch.autograd.grad(o, leaves, do))
        keep = host_mask(B * H, 0, M, N, p, step, site).view(B, H, M, N)
        ref, low = ([torch.stack([x[i] for x in per]) for i in range(5)] + ([sum(x[5] for x in per)] if rad else [])
                    for per in ([reference(q[b], k[b], v[b], do[b], r1, causal, keep[b], p, dt) for b in range(B)]
                                for dt in (torch.float64, dtype)))
    else:
        lq, lk, causal = PACKED[case]
        H, rad = 2, 8
        cq, ck = (torch.tensor(np.concatenate(([0], np.cumsum(x))), dtype=torch.int32).cuda() for x in (lq, lk))
        q, k, v, do = (_rand((T, H, 64), dtype, i) for i, T in enumerate((sum(lq), sum(lk), sum(lk), sum(lq))))
        r1 = _table(H, rad)
        leaves = [t.clone().requires_grad_() for t in (q, k, v, r1)]
        o = flash_attn_varlen_func(leaves[0], leaves[1], leaves[2], cq, ck, max(lq), max(lk), causal, SCALE, leaves[3], rad, **kw)
        o2, lse = FlashAttentionDropout.apply(q, k, v, r1, rad, causal, SCALE, cq, ck, max(lq), max(lk), p, SEED, _step(step), site)
        got = [o, lse] + list(torch.autograd.grad(o, leaves, do))
        both = []
        for dt in (torch.float64, dtype):
            per = []
            for b in range(len(lq)):
                sq, sk = slice(int(cq[b]), int(cq[b + 1])), slice(int(ck[b]), int(ck[b + 1]))
                keep = host_mask(H, b * H, lq[b], lk[b], p, step, site)
                per.append(reference(q[sq].transpose(0, 1), k[sk].transpose(0, 1), v[sk].transpose(0, 1), do[sq].transpose(0, 1), r1, causal,
                                     keep, p, dt))
            cat = lambda i: torch.cat([x[i].transpose(0, 1) for x in per])  # noqa: E731
            both.append([cat(0), torch.cat([x[1] for x in per], 1), cat(2), cat(3), cat(4), sum(x[5] for x in per)])
        ref, low = both
    assert torch.equal(o2, o)   # (lse belongs to the very forward the operators ran)
    _report(name, got, ref, low, dtype)


@pytest.mark.parametrize("site,step", [(0, 0), (0, 7), (5, 0), (5, 7), ("packed", 2 ** 32 + 9)])
def test_the_mask_lands_where_the_header_says(site, step):
    """q = 0, v = the identity, N = 64: every P is exactly 1/64, so o[b, h, m, n] != 0 is the keep bit of (b, h, m, n)"""
    from flasht5_amd import flash_attention_v2_rpe1d, flash_attn_varlen_func
    B, H, M, p, dt = 2, 3, 96, 0.3, torch.bfloat16
    eye = torch.eye(64, dtype=dt, device="cuda")
    if site == "packed":   # lengths (64, 0, 64): b is the sequence's index, and only the counter's low 32 bits of step enter
        cu = torch.tensor([0, 64, 64, 128], dtype=torch.int32, device="cuda")
        v = eye[:, None, :].expand(64, H, 64).repeat(2, 1, 1)
        o = flash_attn_varlen_func(torch.zeros_like(v), v, v, cu, cu, 64, 64, False, SCALE, dropout_p=p, dropout_seed=SEED,
                                   dropout_step=_step(step), dropout_site=9)
        want = torch.cat([host_mask(H, b * H, 64, 64, p, step & R.MASK, 9).transpose(0, 1) for b in (0, 2)])
    else:
        v = eye.expand(B, H, 64, 64)
        o = flash_attention_v2_rpe1d(torch.zeros(B, H, M, 64, dtype=dt, device="cuda"), v, v, None, 0, dropout_p=p, dropout_seed=SEED,
                                     dropout_step=_step(step), dropout_site=site)
        want = host_mask(B * H, 0, M, 64, p, step, site).view(B, H, M, 64)
    assert torch.equal(o != 0, want)
    assert 0.6 < want.float().mean().item() < 0.8
    assert torch.equal(o[want].float(), torch.full_like(o[want], float(torch.tensor(float(R.scale(p)) / 64).to(dt))).float())


def test_reproducible_and_p0_is_todays_call():
    from flasht5_amd import flash_attention_v2_rpe1d
    B, H, S, rad, dt = 2, 2, 130, 8, torch.bfloat16
    q, k, v, do = (_rand((B, S, H, 64), dt, 20 + i).permute(0, 2, 1, 3) for i in range(4))
    r1 = _table(H, rad)

    def run(need_table, **kw):
        leaves = [t.clone().requires_grad_() for t in (q, k, v)] + ([r1.clone().requires_grad_()] if need_table else [])
        o = flash_attention_v2_rpe1d(leaves[0], leaves[1], leaves[2], leaves[3] if need_table else r1, rad, True, SCALE, **kw)
        return [o.detach()] + list(torch.autograd.grad(o, leaves, do))

    kw = dict(dropout_p=0.1, dropout_seed=SEED, dropout_step=_step(4), dropout_site=1)
    a, b, c = run(True, **kw), run(True, **kw), run(False, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(a[:4], c))
    assert not torch.equal(a[0], run(True, **dict(kw, dropout_step=_step(5)))[0])
    assert all(torch.equal(x, y) for x, y in zip(run(True, dropout_p=0.0), run(True)))
