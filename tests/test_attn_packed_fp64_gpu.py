"""Packed (cu_seqlens) attention -- `fat5_attn_fwd` and `fat5_attn_bwd` with cu_seqlens_q / cu_seqlens_k set -- per element of o, lse, dq,
dk, dv and drpe1d against the fp64 restatement of tests/attn_packed_fp64.py: the dense references and bounds of tests/attn_fwd_fp64.py and
tests/attn_bwd_fp64.py applied per sequence.  The case list (tests/attn_packed_fp64.py, proven on the CPU by
tests/test_attn_packed_fp64_cpu.py) holds the edges specific to packing: sequences without keys, without queries, without either, first,
in the middle, last and two in a row; one sequence; max_seqlen beyond the longest sequence by more than a workgroup (the forward's early
exit, the zeroed partial diagonal-sum rows of key blocks past a short sequence's end); causal batches with M_b <, =, > N_b (rows without a
visible key); the T5 generator with cu_seqlens_q != cu_seqlens_k; sequence starts at odd token offsets; q, k, v as views of one
(total, 3, H, D) buffer; bf16 and fp16; D = 16 .. 128; the 32-row body at two and four waves, its split form, the backward as separate
launches and as one launch.  Every case asserts its bodies through fat5_attn_describe before it launches.

The test owns the output buffers: the descriptor is built the way `_varlen_fwd_impl` / `_varlen_bwd_impl` build it, o, lse, dq, dk, dv and
drpe1d are pre-filled with NaN (every element the contract covers must come back finite, or -inf for lse of a row without a visible
key), and each has a guard region behind it inside the allocation that must come back bit-identical.  The backward runs from the GIVEN
(o, lse) of the case (in "perturbed" cases lse shifted on every third row and an unrelated o), never from a forward launch.
"""
import ctypes
import importlib

import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
import attn_packed_fp64 as P
from attn_packed_fp64 import CASES, inputs, describe, assert_bodies, variant_bits

GUARD_TOKENS = 48
SENTINEL = 777.0
WORST = {}   # group (bodies) -> [launches, {output: [worst ratio, its case]}]


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Guarded:
    """`shape` elements of NaN with a SENTINEL-filled guard region behind them, in one allocation"""

    def __init__(self, shape, dtype, guard):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + guard,), float("nan"), dtype=dtype, device="cuda")
        self.buf[n:] = SENTINEL
        self.view = self.buf[:n].view(*shape)
        self.guard0 = self.buf[n:].clone()

    def refill(self):
        self.buf[:self.n] = float("nan")

    def intact(self):
        return torch.equal(_bits(self.buf[self.n:]), _bits(self.guard0))


def _record(case, side, r):
    tag = f"{case['group']} {side} (" + (f"fwd={case['body']} waves={case['waves']}" if side == "fwd" else
                                        f"fused={case['bodies']['fused']} waves={case['bwd_waves']}") + ")"
    w = WORST.setdefault(tag, [0, {}])
    w[0] += 1
    for x, val in r.items():
        if val >= w[1].setdefault(x, [0.0, ""])[0]:
            w[1][x] = [val, case["id"]]


def _worst_element(got, ref, bound):
    g = got.double()
    e = (g - ref).abs()
    q = torch.where(e == 0, torch.zeros_like(e), e / bound)
    q = torch.where(torch.isfinite(g), q, torch.full_like(q, float("inf")))
    q = torch.nan_to_num(q, nan=float("inf"))
    idx = tuple(int(v) for v in torch.nonzero(q == q.max())[0])
    return f"at {idx}: got {float(g[idx])!r} ref {float(ref[idx])!r} bound {float(bound[idx]):.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_packed_attention_within_the_fp64_bound(case):
    from flasht5_amd import _lib
    fa = importlib.import_module("flasht5_amd.flash_attention_v2_bias")   # (the package exports a function of the same name)
    assert_bodies(case, describe(case))
    t = inputs(case)
    H, D, dtype, R = case["H"], case["D"], case["dtype"], case["R"]
    Tq, Tk = t["cu_q"][-1], t["cu_k"][-1]
    fwd = t["fwd"]
    bo, bl = P.packed_fwd_bound(fwd, dtype, D, case["body"])
    bwd = P.packed_bwd_ref(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], t["cu_q"], t["cu_k"], case["scale"], case["causal"], t["rpe"], R)
    bb = P.packed_bwd_bound(bwd, dtype, D, case["bodies"])

    names = ("q", "k", "v", "do", "o", "lse") + (("rpe",) if R else ())
    if case["qkv"]:
        base = t["q"]._base if t["q"]._base is not None else t["q"]
        dbuf = base.to("cuda")
        dev = dict(q=dbuf[:, 0], k=dbuf[:, 1], v=dbuf[:, 2])
        assert all(dev[x].stride() == t[x].stride() and fa._varlen_ok(dev[x]) for x in "qkv") and dev["k"].data_ptr() == dev["q"].data_ptr() + H * D * 2
    else:
        dev = {x: t[x].to("cuda") for x in "qkv"}
    for x in names[3:]:
        dev[x] = t[x].to("cuda").contiguous()
    assert all(fa._varlen_ok(dev[x]) for x in ("q", "k", "v", "do", "o"))   # (the library's own predicate: nothing would be copied)
    cu_q = torch.tensor(t["cu_q"], dtype=torch.int32, device="cuda")
    cu_k = torch.tensor(t["cu_k"], dtype=torch.int32, device="cuda")
    given = {x: dev[x].clone() for x in names}
    given["cu_q"], given["cu_k"] = cu_q.clone(), cu_k.clone()
    fa._check_varlen(dev["q"], dev["k"], dev["v"], cu_q, cu_k, dev.get("rpe"), R)

    def params():
        p = fa._varlen_params(dev["q"], dev["k"], dev["v"], cu_q, cu_k, case["max_q"], case["max_k"], case["causal"], case["scale"])
        if R:
            p.bias_mode, p.rpe1d, p.rpe_radius = _lib.BIAS_RPE1D, dev["rpe"].data_ptr(), R
        return p

    def st(x):
        return _lib.c_i64x3(0, x.stride(1), x.stride(0))

    lib = _lib.load()
    stream = _lib.stream_ptr(dev["q"].device)
    # ---------------------------------------------------------------- forward
    go = Guarded((Tq, H, D), dtype, GUARD_TOKENS * H * D)
    gl = Guarded((H, Tq), torch.float32, GUARD_TOKENS * H)
    with _lib.variant(variant_bits(case)):
        p = params()
        p.o, p.lse, p.o_stride = go.view.data_ptr(), gl.view.data_ptr(), st(go.view)
        _lib.check(lib.fat5_attn_fwd(ctypes.byref(p), stream), "fat5_attn_fwd(varlen)")
    torch.cuda.synchronize()
    oc, lc = go.view.cpu(), gl.view.cpu()
    assert go.intact() and gl.intact(), f"{case['id']}: the forward wrote behind o or lse"
    ro, rl, same = F.ratios(oc, lc, fwd, bo, bl)
    # ---------------------------------------------------------------- backward, from the given (o, lse)
    gq, gk, gv = (Guarded((T, H, D), dtype, GUARD_TOKENS * H * D) for T in (Tq, Tk, Tk))
    gr = Guarded((H, 2 * R + 1), torch.float32, 64) if R else None

    def backward():
        for x in (gq, gk, gv) + ((gr,) if R else ()):
            x.refill()
        with _lib.variant(variant_bits(case)):
            p = params()
            p.o, p.lse, p.dout = dev["o"].data_ptr(), dev["lse"].data_ptr(), dev["do"].data_ptr()
            p.dq, p.dk, p.dv = gq.view.data_ptr(), gk.view.data_ptr(), gv.view.data_ptr()
            for name, x in (("o_stride", dev["o"]), ("do_stride", dev["do"]), ("dq_stride", gq.view), ("dk_stride", gk.view), ("dv_stride", gv.view)):
                setattr(p, name, st(x))
            if R:
                p.drpe1d = gr.view.data_ptr()
            ws = fa._workspace(lib.fat5_attn_bwd_workspace_bytes(ctypes.byref(p)), dev["q"].device)
            p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
            _lib.check(lib.fat5_attn_bwd(ctypes.byref(p), stream), "fat5_attn_bwd(varlen)")
        torch.cuda.synchronize()
        got = dict(dq=gq.view.cpu(), dk=gk.view.cpu(), dv=gv.view.cpu())
        if R:
            got["drpe1d"] = gr.view.cpu()
        return got

    got = backward()
    again = backward()
    assert all(x.intact() for x in (gq, gk, gv) + ((gr,) if R else ())), f"{case['id']}: the backward wrote behind dq, dk, dv or drpe1d"
    for x, was in given.items():
        now = cu_q if x == "cu_q" else (cu_k if x == "cu_k" else dev[x])
        assert torch.equal(_bits(now), _bits(was)), f"{case['id']}: the calls changed {x}"
    for x in got:
        assert torch.equal(_bits(got[x]), _bits(again[x])), f"{case['id']}: a second call gives other bits in {x}"
    r = G.ratios(got, bwd, bb)
    assert sorted(r) == sorted(got)
    _record(case, "fwd", dict(o=ro, lse=rl))
    _record(case, "bwd", r)
    print(f"[attn-packed-fp64] {case['id']}: err / bound o {ro:.3f} lse {rl:.3f} " + " ".join(f"{x} {r[x]:.3f}" for x in r))
    # ---------------------------------------------------------------- the verdicts
    assert bool(torch.isfinite(oc).all()), f"{case['id']}: o keeps a NaN of the pre-fill (or holds a non-finite value)"
    assert not bool(torch.isnan(lc).any()), f"{case['id']}: lse keeps a NaN of the pre-fill"
    assert same, f"{case['id']}: the finiteness pattern of lse differs from the reference's"
    for x in got:
        assert bool(torch.isfinite(got[x]).all()), f"{case['id']}: {x} keeps a NaN of the pre-fill (or holds a non-finite value)"
        zero = bb[x] == 0
        assert not bool(got[x][zero].double().abs().any()), f"{case['id']}: {x} is not an exact zero where the bound is 0"
    msg = []
    if ro > 1.0:
        msg.append(f"o err/bound {ro:.3f} " + _worst_element(oc, fwd["o"], bo))
    if rl > 1.0:
        val = torch.isfinite(fwd["lse"])
        msg.append(f"lse err/bound {rl:.3f} " + _worst_element(torch.where(val, lc.double(), torch.zeros(())), torch.where(val, fwd["lse"], torch.zeros(())).double(),
                                                              torch.where(val, bl, torch.ones(()).double())))
    for x in got:
        if not r[x] <= 1.0:
            msg.append(f"{x} err/bound {r[x]:.3f} " + _worst_element(got[x], bwd[x], bb[x]))
    assert not msg, f"{case['id']} (cu_q {t['cu_q']}, cu_k {t['cu_k']}): " + "; ".join(msg)


@pytest.mark.gpu
def test_zz_summary():
    """(runs last) one line per group and side: the launches and the worst err / bound of this session"""
    for tag, (n, worst) in sorted(WORST.items()):
        print(f"[attn-packed-fp64] {tag}: {n} launches, worst err/bound " + ", ".join(f"{x} {v[0]:.3f} ({v[1]})" for x, v in sorted(worst.items())))
    assert all(v[0] <= 1.0 for _, worst in WORST.values() for v in worst.values())
