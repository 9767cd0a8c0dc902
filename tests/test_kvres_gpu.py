"""The resident K / V form of the 64-row dQ body (csrc/attn_bwd64.h, attn_bwd_q64_body<..., KVRES>: a head's whole K and V stay in LDS -- the four ring slots
plus the bytes of the staging images -- instead of cycling through the ring; two barriers in all instead of one per key step).

Checked per case, with FAT5_V_KVRES_ON and FAT5_V_KVRES_OFF on the same inputs, in the one-launch form and stage by stage:
  * the plan's describe() reports the form (fat5_attn_bwd_kvres; kvres=1 where it is legal: operands staged, at most 16 key steps; kvres=0 beyond 512 keys and at radius 512);
  * dq and the bias gradient (T5 table / drpe1d) are the same BITS in both forms -- every wave does the same arithmetic in the same order --, dk and dv too
    (the dK/dV half is not touched);
  * dq, dk, dv and the bias gradient are inside the per-element fp64 bound of tests/attn_bwd_fp64.py, with the inputs, the reference and the bound of
    tests/test_attn_bwd_fp64_gpu.py (imported, not copied).
Shapes are the smallest at which the structure differs: fewer steps than the four prefilled slots (32, 96 keys), exactly four (128), the first slot inside the
former staging area (160), the last one (512), a key tail inside it with general iterations (500), one step too many (544: the ring form); 64, 200 (rows past M
inside a wave), 256 and 512 rows; M != N; radius 16, 128 and 512; no bias; fp16; causal; unit ranges.  One more test replays the call twenty times inside one HIP
graph and asks for the same bits every time: a barrier missing at the hand-over of the staging bytes or ahead of the dQ image would show as a race there.
"""
import pytest
import torch

import attn_bwd_fp64 as G
import test_attn_bwd_fp64_gpu as W

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16


def _case(B, H, M, N, bias="t5b", R=128, dtype=BF16, causal=False, kvres=1, scale=0.125, strided=False):
    """a case in the format of tests/test_attn_bwd_fp64_gpu.py (its `inputs`, `reference` and `describe` read it); kvres: what describe has to say with KVRES_ON"""
    table = bias[:2] == "t5"
    bodies = dict(dq="64row", dkdv="64key", fused="1", qdiag="1" if bias != "none" else "0")
    if table:
        bodies["dtable"] = "runs"
    cid = f"kvres-{B}x{H}x{M}x{N}-{str(dtype)[6:]}-{bias}{R if bias != 'none' else ''}{'-causal' if causal else ''}{'-strided' if strided else ''}"
    return dict(id=cid, group="kvres", bodies=bodies, bits=("V_FUSED64_ON", "V_KVRES_ON"), B=B, H=H, M=M, N=N, D=64, dtype=dtype, causal=causal, bias=bias,
                R=R if bias != "none" else 0, scale=scale, strided=strided, pert=False, split=False, wide=True, dense64=False, kvres=str(kvres))


CASES = [
    _case(1, 2, 64, 32, R=16),                      # one step: nothing behind the prefilled slots, no second request batch
    _case(1, 2, 200, 96),                           # three steps; rows past M inside the last wave
    _case(2, 1, 256, 128, R=16),                    # exactly four steps: one aligned trip, no second visibility point
    _case(1, 2, 256, 160, bias="rpe"),              # five steps: the first slot inside the former staging area (general iteration behind one trip)
    _case(1, 2, 512, 512, strided=True),            # the benchmark's form: sixteen steps, the last slot, two row blocks
    _case(1, 2, 200, 500, R=16),                    # key tail inside the last resident slot: general iterations behind three trips; far trips on both sides
    _case(1, 2, 256, 544, kvres=0),                 # seventeen steps: the ring form
    _case(1, 2, 256, 512, bias="none"),             # M != N, no bias
    _case(2, 2, 512, 160, R=16, dtype=F16),         # M != N, fp16, narrow band
    _case(1, 2, 512, 512, R=512, kvres=0),          # radius 512: no room for the staging images -> the ring form
    _case(1, 2, 512, 512, bias="none", causal=True),
    _case(1, 2, 300, 512, causal=True, dtype=F16),  # causal with the table carrying the mask (0 < N - M < R)
]

_REF = {}  # case id -> (inputs, reference): computed once, shared, never written


def _ref(case):
    if case["id"] not in _REF:
        t = W.inputs(case)
        _REF[case["id"]] = (t, W.reference(case, t))
    return _REF[case["id"]]


def _bits(names):
    from flasht5_amd import _lib
    out = 0
    for n in names:
        out |= getattr(_lib, n)
    return out


def _plan(case, t, bits, units=None):
    from flasht5_amd.flash_attention_v2_bias import AttentionPlan
    dev = {key: (x.to("cuda") if x is not None else None) for key, x in t.items()}
    plan = AttentionPlan(dev["q"], dev["k"], dev["v"], dev["do"], rpe1d=dev["rpe"], radius=case["R"], causal=case["causal"], sm_scale=case["scale"],
                         need_dbias=True, rpe_bucket=dev["bucket"], num_buckets=W.NUM_BUCKETS if dev["bucket"] is not None else 0, variant=bits, units=units)
    plan.o.copy_(dev["o"])
    plan.lse.copy_(dev["lse"])
    return plan


def _run(plan, staged):
    for x in (plan.dq, plan.dk, plan.dv, plan.dbias):
        if x is not None:
            x.fill_(W.SENTINEL)   # (every element has to be written)
    plan.ws.view(torch.uint8).fill_(255)   # (NaN patterns: nothing may be read that this call did not write)
    if staged:
        for stage in (1, 2, 4):
            plan.backward(stage)
    else:
        plan.backward()
    torch.cuda.synchronize()
    return [None if x is None else x.clone() for x in (plan.dq, plan.dk, plan.dv, plan.dbias)]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kvres_same_bits_as_the_ring_and_inside_the_fp64_bound(case):
    t, ref = _ref(case)
    on, off = _bits(("V_FUSED64_ON", "V_KVRES_ON")), _bits(("V_FUSED64_ON", "V_KVRES_OFF"))
    W.assert_bodies(case, W.describe(case))
    plan = _plan(case, t, _bits(("V_FUSED64_ON",)))
    assert plan.describe()["kvres"] == case["kvres"], plan.describe()   # (legal means taken)
    plan.set_variant(on)
    W.assert_bodies(case, plan.describe())
    assert plan.describe()["kvres"] == case["kvres"] and plan.bwd_launches() == 1
    res = {}
    for name, bits in (("on", on), ("off", off)):
        plan.set_variant(bits)
        assert plan.describe()["kvres"] == (case["kvres"] if name == "on" else "0")
        for staged in (False, True):
            res[name, staged] = _run(plan, staged)
    names = ("dq", "dk", "dv", "bias gradient")
    for staged in (False, True):
        for i, x in enumerate(names):
            if res["on", staged][i] is not None:
                assert torch.equal(W._bits(res["on", staged][i]), W._bits(res["off", staged][i])), f"{x}, {'stage by stage' if staged else 'one launch'}"
    # the same dQ body in the one-launch and the stage-by-stage form
    assert torch.equal(W._bits(res["on", True][0]), W._bits(res["on", False][0]))
    bound = G.attn_bwd_bound(ref, case["dtype"], case["D"], case["bodies"], case["N"], case["M"])
    outs = W.compared(case, ref)
    for staged in (False, True):
        dq, dk, dv, db = res["on", staged]
        got = dict(dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
        if db is not None:
            got["drpe_table" if t["bucket"] is not None else "drpe1d"] = db.cpu()
        assert sorted(got) == sorted(outs)
        r = G.ratios(got, ref, bound)
        print(f"[kvres] {case['id']} {'stages' if staged else 'one launch'}: err / bound " + " ".join(f"{x} {r[x]:.3f}" for x in outs))
        assert all(r[x] <= 1.0 for x in outs), (case["id"], staged, r)


def test_kvres_unit_ranges():
    """two unit ranges (head-major units u = h * B + b) run the same resident form on the units each owns: dq of the units, partial tables that add up"""
    case = _case(2, 2, 256, 512)
    t, ref = _ref(case)
    on = _bits(("V_FUSED64_ON", "V_KVRES_ON"))
    whole = _plan(case, t, on)
    want = _run(whole, False)
    parts = []
    for rng in ((0, 3), (3, 1)):
        pl = _plan(case, t, on, units=rng)
        assert pl.describe()["kvres"] == "1"
        pl.dq.zero_(); pl.dk.zero_(); pl.dv.zero_()
        pl.backward()
        torch.cuda.synchronize()
        parts.append(pl)
    for i, x in enumerate(("dq", "dk", "dv")):
        assert torch.equal(W._bits(getattr(parts[0], x) + getattr(parts[1], x)), W._bits(want[i])), x
    tot = parts[0].dbias + parts[1].dbias
    assert float((tot - want[3]).abs().max()) <= 1e-5 * max(1.0, float(want[3].abs().max()))   # (two partial tables: one fp32 addition apart)


def test_kvres_is_the_plain_choice_at_the_benchmark_shape():
    from flasht5_amd import _lib
    assert _lib.describe(B=4, H=12, M=512, N=512, bias_mode=_lib.BIAS_RPE1D, radius=128, need_dbias=True)["kvres"] == "1"
    assert _lib.describe(B=4, H=12, M=512, N=512, bias_mode=_lib.BIAS_NONE)["kvres"] == "1"
    assert _lib.describe(B=4, H=12, M=2048, N=2048, bias_mode=_lib.BIAS_RPE1D, radius=128, need_dbias=True)["kvres"] == "0"


def test_kvres_replays_to_the_same_bits():
    """the same call twenty times inside one HIP graph: every replay of every call leaves the same bits (a race screen for the two added barriers)"""
    case = _case(1, 2, 512, 512, strided=True)
    t, _ = _ref(case)
    plan = _plan(case, t, _bits(("V_FUSED64_ON", "V_KVRES_ON")))
    assert plan.describe()["kvres"] == "1"
    want = _run(plan, False)
    n = 20
    dqs = torch.empty((n,) + tuple(plan.dq.shape), dtype=plan.dq.dtype, device="cuda")
    dts = torch.empty((n,) + tuple(plan.dbias.shape), dtype=plan.dbias.dtype, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan.backward()
        with torch.cuda.graph(g, stream=s):
            for i in range(n):
                plan.backward()
                dqs[i].copy_(plan.dq)
                dts[i].copy_(plan.dbias)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        dqs.fill_(W.SENTINEL)
        dts.fill_(W.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for i in range(n):
            assert torch.equal(W._bits(dqs[i]), W._bits(want[0])), i
            assert torch.equal(W._bits(dts[i]), W._bits(want[3])), i
