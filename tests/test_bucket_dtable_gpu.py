"""GPU tests of the bucket-run form of the T5 table gradient (csrc/reduce_kernels.h: drpe_runs_reduce_kernel): the reduction launch sums every
bucket's run of the partial per-diagonal rows straight into the (num_buckets, H) table, where the per-diagonal form (drpe_reduce_kernel,
FAT5_V_DTABLE_RUNS_OFF) first reduces the 2R+1 diagonals and then scans them for their bucket.

Reference: the bias gradient is the dS tensor summed over the batch (src/model/ops/flash_attention_v2_bias.py:214-215); with the Toeplitz T5 bias
(src/utils/positional_encoding.py:100-101) it lands in the table through the bucket map.  Checked: against the fp32 oracle (the allowance of
tests/test_bwd64_gpu.py), against the per-diagonal form (the same partial rows, another fp32 summation order), dq / dk / dv bit-identical between the
two forms, the same bits from run to run and in graph replay, stage-by-stage calls, unit ranges, and the fall-backs."""
import pytest
import torch

from attn_helpers import oracle_all, maxdiff
from test_attention_gpu import gbound, _rpe_case
from test_bwd64_gpu import _table_truth

pytestmark = pytest.mark.gpu


def _plan(q, k, v, do, table, md, causal, bits=0, units=None, bucket=None):
    from flasht5_amd.flash_attention_v2_bias import AttentionPlan
    from flasht5_amd import positional_encoding as pe
    R = pe.rpe_radius(md)
    bk = pe.bucket_index32(R, True, 32, md, q.device) if bucket is None else bucket
    rpe1d = table.cuda().index_select(0, bk.long()).transpose(0, 1).float().contiguous()
    plan = AttentionPlan(q, k, v, do, causal=causal, sm_scale=0.125, variant=bits, units=units, rpe1d=rpe1d, radius=R,
                         rpe_bucket=bk, num_buckets=32)
    plan.forward()
    plan.ws.view(torch.uint8).fill_(255)  # (NaN patterns in the workspace: nothing may be read that was not written)
    plan.dbias.fill_(float("nan"))
    return plan


def _tol(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


CASES = [
    (4, 12, 512, 512, False, 128),    # cfg2: the dQ workgroups form the partial rows (one per 256-row block)
    (2, 12, 512, 512, False, 128),
    (8, 12, 512, 512, False, 128),    # two rounds of the chip: the dK/dV workgroups form them (one per key block)
    (1, 2, 1000, 1100, False, 128),   # ragged
    (1, 2, 1100, 1000, True, 128),    # causal, the mask carried by the table (P < 0: dead rows)
    (1, 2, 1000, 1100, True, 128),    # ... 0 < P < R
    (1, 2, 768, 768, False, 512),     # radius 512: the last bucket of each side is a run of 422 entries
    (1, 2, 2048, 2048, False, 32),    # narrow band, 8 partial rows per head
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,M,N,causal,md", CASES)
def test_runs_match_oracle_and_the_per_diagonal_form(B, H, M, N, causal, md, dtype):
    from flasht5_amd import _lib
    q, k, v, do, table, bias = _rpe_case(B, H, M, N, dtype, causal, True, md, seed=M + 7 * N + B)
    ref = oracle_all(q, k, v, bias, do, 0.125, causal)
    outs = {}
    for name, bits in (("runs", 0), ("scan", _lib.V_DTABLE_RUNS_OFF)):
        plan = _plan(q, k, v, do, table, md, causal, bits)
        assert plan.describe()["dtable"] == name
        outs[name] = [t.clone() for t in plan.backward()] + [plan.o.clone()]
        torch.cuda.synchronize()
    dq, dk, dv, dt, o = outs["runs"]
    for got, key in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
        assert torch.isfinite(got.float()).all(), key
        assert maxdiff(got, ref[key]) <= gbound(ref[key], dtype), key
    for i in range(3):  # the reduction touches none of dq / dk / dv
        assert torch.equal(outs["runs"][i], outs["scan"][i]), ("dq", "dk", "dv")[i]
    want, allow = _table_truth(q, k, v, bias, o, ref["L"], do, 0.125, causal, table, M, N, True, md)
    assert torch.isfinite(dt).all()
    err = (dt.cpu() - want).abs()
    assert bool((err <= allow + 2e-3 * max(1.0, want.abs().max().item()) + 1e-2).all()), (err.max().item(), allow.max().item())
    # the same partial rows, summed in another fp32 order
    assert maxdiff(dt, outs["scan"][3]) <= _tol(outs["scan"][3])


def test_runs_bitwise_stable_and_graph_replay():
    q, k, v, do, table, bias = _rpe_case(4, 12, 512, 512, torch.bfloat16, False, True, 128, seed=5)
    plan = _plan(q, k, v, do, table, 128, False)
    assert plan.describe()["dtable"] == "runs"
    first = plan.backward()[3].clone()
    for _ in range(3):
        plan.dbias.fill_(float("nan"))
        assert torch.equal(plan.backward()[3], first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.backward()
    for _ in range(3):
        plan.dbias.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(plan.dbias, first)


@pytest.mark.parametrize("B,H,M,N,causal", [(2, 3, 512, 768, False), (1, 2, 1000, 1100, True)])
def test_runs_stage_by_stage_and_unit_ranges(B, H, M, N, causal):
    from flasht5_amd import _lib
    q, k, v, do, table, bias = _rpe_case(B, H, M, N, torch.bfloat16, causal, True, 128, seed=13)
    bits = _lib.V_FUSED64_ON | _lib.V_QDIAG_ON
    whole = _plan(q, k, v, do, table, 128, causal, bits)
    want = [t.clone() for t in whole.backward()]
    scan = _plan(q, k, v, do, table, 128, causal, bits | _lib.V_DTABLE_RUNS_OFF)
    ref_scan = scan.backward()[3].clone()
    st = _plan(q, k, v, do, table, 128, causal, bits)
    st.backward(1)
    st.backward(2)
    st.backward(4)
    torch.cuda.synchronize()
    assert maxdiff(st.dbias, want[3]) <= 1e-5 * max(1.0, float(want[3].abs().max()))
    assert maxdiff(want[3], ref_scan) <= _tol(ref_scan)
    n = B * H
    cut = n // 2 + (1 if n > 2 else 0)
    parts = []
    for rng in ((0, cut), (cut, n - cut)):
        pl = _plan(q, k, v, do, table, 128, causal, bits, units=rng)
        assert pl.describe()["dtable"] == "runs"
        pl.backward()
        parts.append(pl)
    torch.cuda.synchronize()
    assert maxdiff(parts[0].dbias + parts[1].dbias, want[3]) <= 1e-4 * max(1.0, float(want[3].abs().max()))


def test_non_contiguous_map_falls_back():
    """a bucket map with an id in two places is not a sequence of runs: the per-diagonal reduction, whatever the variant bits"""
    from flasht5_amd import _lib
    from flasht5_amd import positional_encoding as pe
    q, k, v, do, table, bias = _rpe_case(2, 4, 512, 512, torch.bfloat16, False, True, 128, seed=17)
    base = pe.bucket_index32(128, True, 32, 128, torch.device("cpu")).clone()
    base[0], base[128] = int(base[128]), int(base[0])  # buckets 15 (d = -128) and 0 (d = 0) swap one entry each
    bk = base.cuda()
    outs = []
    for bits in (0, _lib.V_DTABLE_RUNS_ON, _lib.V_DTABLE_RUNS_OFF):
        plan = _plan(q, k, v, do, table, 128, False, bits, bucket=bk)
        assert plan.describe()["dtable"] == "scan"
        outs.append(plan.backward()[3].clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # the map's own gradient: the generator's (H, 2R+1) sums scattered through the swapped map
    from flasht5_amd.flash_attention_v2_bias import AttentionPlan
    rpe1d = table.cuda().index_select(0, bk.long()).transpose(0, 1).float().contiguous()
    g = AttentionPlan(q, k, v, do, sm_scale=0.125, rpe1d=rpe1d, radius=128)
    g.forward()
    d1 = g.backward()[3]
    assert "dtable" not in g.describe()
    want = torch.zeros(32, 4, device=d1.device).index_add_(0, bk.long(), d1.transpose(0, 1))
    assert maxdiff(outs[0], want) <= _tol(want)
