"""Local (sliding-window) attention -- `fat5_attn_local_fwd` and `fat5_attn_local_bwd` over the C ABI -- per element of o, lse, dq, dk, dv
and drpe1d against the fp64 restatement and the derived bound of tests/local_attn_fp64.py, on its case list (proven on the CPU by
tests/test_local_attn_fp64_cpu.py): the band seams of the step selection, both clamp ends in one step, window = R and R +- 1, the
dynamic-LDS seam of the dQ kernel, lengths around the step and tile sizes, packed batches with empty sequences and a max_seqlen beyond
every length.

The test owns the output buffers: they are pre-filled with NaN, a strided (B, S, H, D) output has a guard behind every row and every
buffer a guard region behind it, which must come back bit-identical.  The backward runs from the GIVEN (o, lse): the restatement's o
rounded to the dtype and its lse as fp32, never from a forward launch; a second run gives the same bits, and a run without a drpe1d
request the same dq, dk, dv.  Three cases run once more through the public functions, from the kernels' own (o, lse)."""
import ctypes
import importlib

import pytest
import torch

import local_attn_fp64 as LA
from local_attn_fp64 import CASES, D, H

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
PAD = 8
WORST = {}   # (output, dtype name) -> [worst ratio, its case]
_TRUTH = {}


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def truth(case):
    if case["id"] not in _TRUTH:
        t = LA.inputs(case)
        ref, given = LA.local_ref(case, t)
        _TRUTH[case["id"]] = (t, ref, given, LA.local_bound(case, ref))
    return _TRUTH[case["id"]]


def _to_dev(case, flat):
    """a flat (total, H, D) tensor in the kernels' layout on the device: packed as it is; dense (B, H, S, D), contiguous or as a view of
    (B, S, H, D) storage"""
    if case["packed"]:
        return flat.cuda().contiguous()
    x = flat.view(len(case["lens"]), case["S"], H, D).cuda().permute(0, 2, 1, 3)
    return x if case["strided"] else x.contiguous()


class Out:
    """an output tensor in the case's layout, NaN-filled, with SENTINEL guards: behind every row of a strided tensor, and behind the whole"""

    def __init__(self, case, dtype, tail=4096):
        self.case, B, S = case, len(case["lens"]), case["S"]
        total = sum(case["lens"])
        if case["packed"]:
            shape, self.width = (total, H, D), D
        elif case["strided"]:
            shape, self.width = (B, S, H, D + PAD), D + PAD
        else:
            shape, self.width = (B, H, S, D), D
        self.n = 1
        for s in shape:
            self.n *= s
        self.buf = torch.full((self.n + tail,), SENTINEL, dtype=dtype, device="cuda")
        self.all = self.buf[:self.n].view(*shape)
        self.body = self.all[..., :D]
        self.view = self.body.permute(0, 2, 1, 3) if (not case["packed"] and case["strided"]) else self.body
        self.refill()
        self.before = self.buf.clone()

    def refill(self):
        self.body.fill_(float("nan"))

    def intact(self):
        now = self.buf.clone()
        now[:self.n].view_as(self.all)[..., :D] = float("nan")
        return torch.equal(_bits(now), _bits(self.before))

    def flat(self):
        x = self.view if self.case["packed"] else self.view.permute(0, 2, 1, 3)
        return x.reshape(-1, H, D).cpu()


def _lse_dev(case, lse_flat):
    if case["packed"]:
        return lse_flat.cuda().contiguous()
    return lse_flat.view(H, len(case["lens"]), case["S"]).permute(1, 0, 2).cuda().contiguous()


def _lse_flat(case, lse):
    return lse.cpu() if case["packed"] else lse.permute(1, 0, 2).reshape(H, -1).cpu()


def _record(case, r):
    for x, v in r.items():
        key = (x, "bf16" if case["dtype"] == torch.bfloat16 else "fp16")
        if v >= WORST.setdefault(key, [0.0, ""])[0]:
            WORST[key] = [v, case["id"]]


def _worst_element(got, ref, bound):
    g = got.double()
    e = (g - ref).abs()
    q = torch.where(e == 0, torch.zeros_like(e), e / bound)
    q = torch.nan_to_num(torch.where(torch.isfinite(g), q, torch.full_like(q, float("inf"))), nan=float("inf"))
    idx = tuple(int(v) for v in torch.nonzero(q == q.max())[0])
    return f"at {idx}: got {float(g[idx])!r} ref {float(ref[idx])!r} bound {float(bound[idx]):.3e}"


def _verdict(case, got, ref, bound):
    r = LA.ratios(got, ref, bound)
    assert sorted(r) == sorted(got)
    _record(case, r)
    print(f"[local-fp64] {case['id']}: err / bound " + " ".join(f"{x} {r[x]:.3f}" for x in r))
    msg = []
    for x in got:
        assert bool(torch.isfinite(got[x].float()).all()), f"{case['id']}: {x} keeps a NaN of the pre-fill (or holds a non-finite value)"
        assert not bool(got[x][bound[x] == 0].double().abs().any()), f"{case['id']}: {x} is not an exact zero where the bound is 0"
        if not r[x] <= 1.0:
            msg.append(f"{x} err/bound {r[x]:.3f} " + _worst_element(got[x], ref[x], bound[x]))
    assert not msg, f"{case['id']}: " + "; ".join(msg)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_local_attention_within_the_fp64_bound(case):
    from flasht5_amd import _lib
    fa = importlib.import_module("flasht5_amd.flash_attention_v2_bias")
    t, ref, given, bound = truth(case)
    dtype, R, window = case["dtype"], case["R"], case["window"]
    wc = min(window, R)
    if R == 1024:   # the dQ kernel's LDS on either side of 48 KiB: above it the launch goes through hipFuncSetAttribute
        assert (LA.local_smem_q(wc, True) > 48 * 1024) == (wc >= 1013) and LA.local_smem_q(wc, False) <= 48 * 1024
    dev = {x: _to_dev(case, t[x]) for x in ("q", "k", "v", "do")}
    dev["o"], dev["lse"] = _to_dev(case, given[0]), _lse_dev(case, given[1])
    r1 = t["rpe"].cuda() if R else None
    cu = torch.tensor(LA._seqs(case), dtype=torch.int32, device="cuda") if case["packed"] else None
    kept = {x: v.clone() for x, v in dev.items()}
    lib, stream = _lib.load(), _lib.stream_ptr(dev["q"].device)
    # ---------------------------------------------------------------- forward
    go = Out(case, dtype)
    gl = torch.full((dev["lse"].numel() + 1024,), SENTINEL, dtype=torch.float32, device="cuda")
    lse_view = gl[:dev["lse"].numel()].view_as(dev["lse"])
    lse_view.fill_(float("nan"))
    p = fa._local_params((dev["q"], dev["k"], dev["v"], go.view), ("q", "k", "v", "o"), window, case["scale"], r1, R, cu, case["S"])
    p.lse = lse_view.data_ptr()
    _lib.check(lib.fat5_attn_local_fwd(ctypes.byref(p), stream), "fat5_attn_local_fwd")
    torch.cuda.synchronize()
    assert go.intact() and bool((gl[dev["lse"].numel():] == SENTINEL).all()), f"{case['id']}: the forward wrote outside o or lse"
    fwd = dict(o=go.flat(), lse=_lse_flat(case, lse_view))
    # ---------------------------------------------------------------- backward, from the given (o, lse)
    gq, gk, gv = Out(case, dtype), Out(case, dtype), Out(case, dtype)
    gr = torch.full((H * (2 * R + 1) + 64,), SENTINEL, dtype=torch.float32, device="cuda") if R else None

    def backward(want_drpe):
        for x in (gq, gk, gv):
            x.refill()
        ts = (dev["q"], dev["k"], dev["v"], dev["o"], dev["do"], gq.view, gk.view, gv.view)
        p = fa._local_params(ts, ("q", "k", "v", "o", "dout", "dq", "dk", "dv"), window, case["scale"], r1, R, cu, case["S"])
        p.lse = dev["lse"].data_ptr()
        if R and want_drpe:
            gr[:H * (2 * R + 1)] = float("nan")
            p.drpe1d = gr.data_ptr()
        ws = fa._workspace(lib.fat5_attn_local_bwd_workspace_bytes(ctypes.byref(p)), dev["q"].device)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        _lib.check(lib.fat5_attn_local_bwd(ctypes.byref(p), stream), "fat5_attn_local_bwd")
        torch.cuda.synchronize()
        got = dict(dq=gq.flat(), dk=gk.flat(), dv=gv.flat())
        if R and want_drpe:
            got["drpe1d"] = gr[:H * (2 * R + 1)].view(H, -1).cpu()
        return got

    got = backward(True)
    again = backward(True)
    plain = backward(False) if R else None
    assert all(x.intact() for x in (gq, gk, gv)) and (gr is None or bool((gr[H * (2 * R + 1):] == SENTINEL).all())), \
        f"{case['id']}: the backward wrote outside dq, dk, dv or drpe1d"
    for x, was in kept.items():
        assert torch.equal(_bits(dev[x]), _bits(was)), f"{case['id']}: the calls changed {x}"
    for x in got:
        assert torch.equal(_bits(got[x]), _bits(again[x])), f"{case['id']}: a second call gives other bits in {x}"
    if plain is not None:
        for x in plain:
            assert torch.equal(_bits(got[x]), _bits(plain[x])), f"{case['id']}: {x} differs without a drpe1d request"
    _verdict(case, dict(fwd, **got), ref, bound)


PUBLIC = [c for c in CASES if c["id"].split("-")[0] in ("07", "22", "45")]


@pytest.mark.parametrize("case", PUBLIC, ids=[c["id"] for c in PUBLIC])
def test_public_path_from_its_own_forward(case):
    """`flash_attention_v2_rpe1d(..., window=)` / `flash_attn_varlen_func(..., window=)`: the backward from the kernels' own (o, lse),
    against the restatement from that very (o, lse), under the same bound"""
    from flasht5_amd import flash_attention_v2_rpe1d, flash_attn_varlen_func
    t, ref, _, bound = truth(case)
    R, window = case["R"], case["window"]
    leaves = [_to_dev(case, t[x]).requires_grad_() for x in ("q", "k", "v")] + ([t["rpe"].cuda().requires_grad_()] if R else [])
    r1 = leaves[3] if R else None
    if case["packed"]:
        cu = torch.tensor(LA._seqs(case), dtype=torch.int32, device="cuda")
        o = flash_attn_varlen_func(leaves[0], leaves[1], leaves[2], cu, cu, case["S"], case["S"], False, case["scale"], r1, R, window=window)
    else:
        o = flash_attention_v2_rpe1d(leaves[0], leaves[1], leaves[2], r1, R or 1, False, case["scale"], window=window)
    lse = o.grad_fn.saved_tensors[4]
    grads = torch.autograd.grad(o, leaves, _to_dev(case, t["do"]))
    flat = (lambda x: x.detach().cpu()) if case["packed"] else (lambda x: x.detach().permute(0, 2, 1, 3).reshape(-1, H, D).cpu())
    own = (flat(o), _lse_flat(case, lse.detach()))
    assert own[1].dtype == torch.float32 and own[1].shape == ref["lse"].shape
    ref2, _ = LA.local_ref(case, t, given=own)
    got = dict(o=own[0], lse=own[1], dq=flat(grads[0]), dk=flat(grads[1]), dv=flat(grads[2]))
    if R:
        got["drpe1d"] = grads[3].cpu()
    _verdict(case, got, ref2, LA.local_bound(case, ref2))


def test_zz_summary():
    """(runs last) the worst err / bound per output and dtype of this session"""
    for (x, dt), (v, cid) in sorted(WORST.items()):
        print(f"[local-fp64] {dt} {x}: worst err / bound {v:.3f} ({cid})")
    assert all(v[0] <= 1.0 for v in WORST.values())
