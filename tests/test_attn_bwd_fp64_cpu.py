"""What tests/test_attn_bwd_fp64_gpu.py rests on, proven without a GPU, on that file's own case list:
  * every case names the bodies the dispatcher runs it with (fat5_attn_describe is host-only);
  * attn_bwd_ref agrees with fp64 autograd of the forward's formula to 1e-9 of the term magnitudes and with oracle.attn_bwd_oracle --
    an fp32 evaluation -- to fp32 evaluation noise, on the cases whose (o, lse) are consistent;
  * the term magnitudes dominate the outputs;
  * the bound of tests/attn_bwd_fp64.py is not below what correct arithmetic achieves: `emulate` (fp32 scores, P and dS rounded to the
    dtype before the contractions, dbias from the rounded dS, the diagonal sums from the fp32 dS, one output rounding) and the fp64
    reference rounded once to the storage dtype lie within it on every case and every output;
  * the bound is not too loose: every mutant that applies to a case leaves it on that case, except for the (mutant, case) pairs of
    EXCUSED, each with its reason: at most 5 % of the applied pairs, and no mutant in every case of a group;
  * the bound's shape: 0 on a dead row's dq and above the causal diagonal of dbias, finite everywhere.
"""
import functools

import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
import oracle
from test_attn_bwd_fp64_gpu import CASES, inputs, reference, describe, compared

IDS = [c["id"] for c in CASES]
DETECTED = {name: {} for name in G.MUTANTS}   # mutant -> {case id: caught} over the cases where it applied
EMU = {}                                      # group -> {output: [worst ratio of `emulate`, its case]}

# (mutant, case id): why the bound cannot see this defect on this case.  Nothing else is excused.
_ONE_KEY = ("one live key per row: p = 1 and delta = do . o = do . v up to the rounding of o, so dS = p (dP - delta) and with it dq, dk and the diagonal "
            "sums are rounding noise: there is nothing a defect could move (dv and the exact zeros are still checked)")
EXCUSED = {(m, "w2-1x2x1x1-D16-bfloat16-none-strided"): _ONE_KEY
           for m in ("dQ without key 0", "dQ without key N-1", "dQ without the last key of a ragged last tile", "dk without the scale", "dq with the scale squared")}
EXCUSED.update({(m, "w2-2x2x32x1-D32-bfloat16-rpe8-causal"): _ONE_KEY   # (causal, N = 1: row 31 alone sees the key, the other rows are dead)
                for m in ("dQ without key 0", "dQ without key N-1", "dQ without the last key of a ragged last tile", "dk without the scale", "dq with the scale squared",
                          "drpe1d diagonal index +1", "drpe1d diagonal index -1", "drpe1d far entries without what lies beyond the band",
                          "drpe1d of the neighbouring head", "last row of a ragged 64-row block from row M-2")})
EXCUSED[("drpe1d far entries without what lies beyond the band", "t5-3x2x65x300-D128-bfloat16-t5u128-runs")] = (
    "the unidirectional map puts every n >= m into bucket 0 and only the table gradient is written: that entry sums some 50 000 terms of both "
    "signs whose rows each sum to zero, and what lies beyond the band is a partial sum of the same kind, inside the fp32 summation term")


@functools.lru_cache(maxsize=2)
def _truth(i):
    case = CASES[i]
    t = inputs(case)
    ref = reference(case, t)
    return t, ref, G.attn_bwd_bound(ref, case["dtype"], case["D"], case["bodies"], case["N"], case["M"])


def test_the_case_list_is_what_the_issue_asks_for():
    def of(group, key):
        return {c[key] for c in CASES if c["group"] == group}
    assert {c["bodies"]["dq"] for c in CASES} == {"32row"} and {c["bodies"]["dkdv"] for c in CASES} == {"32key"}   # (the 64-wide bodies: not covered)
    assert {1, 31, 32, 33, 64, 65, 129} <= of("w2", "M") and {1, 63, 64, 65, 127, 128, 129, 200} <= of("w2", "N")
    assert of("w2", "D") == {16, 32, 64, 128} and {1, 8, 128} <= of("w2", "R")
    assert {"none", "rpe", "11", "1h", "b1", "bh"} <= of("w2", "bias") | of("causal", "bias")
    for c in CASES:
        if c["group"] in ("w4", "fused32"):   # four waves in at least one stage (both in the one-launch form)
            nq, nk = (c["B"] * c["H"] * -(-c[x] // 128) >= 160 for x in ("M", "N"))
            assert (nq and nk) if c["group"] == "fused32" else (nq or nk), c["id"]
        if c["group"] == "w2":
            assert c["B"] * c["H"] * -(-max(c["M"], c["N"]) // 128) < 160
        assert (c["bodies"]["fused"] == "1") == (c["group"] == "fused32") and (c["group"] != "fused32" or c["D"] <= 64)
    assert {c["N"] - c["M"] for c in CASES if c["group"] == "causal"} == {0, 1, 100, -1, -100} and all(of("causal", "causal"))
    assert {c["bodies"].get("dbias") for c in CASES} >= set(G.DBIAS_ROUTES)
    assert {c["B"] for c in CASES if c["bodies"].get("dbias") == "inkernel"} >= {2, 5} and any("V_DBIAS_NOSPLIT" in c["bits"] for c in CASES)
    assert {(c["bias"], c["R"], c["B"], c["bodies"].get("dtable")) for c in CASES if c["group"] == "t5"} >= {
        (b, R, B, d) for b in ("t5b",) for R in (8, 128) for B in (1, 3) for d in ("runs", "scan")}
    assert {c["bias"] for c in CASES if c["group"] == "t5"} >= {"t5b", "t5u", "rpe"}
    for g in ("w2", "causal", "t5", "dbias", "pert", "fused32"):
        assert of(g, "dtype") == {torch.bfloat16, torch.float16}, g
    assert sum(c["pert"] for c in CASES) >= 4 and sum(c["split"] for c in CASES) >= 4 and sum(c["strided"] for c in CASES) >= 6
    assert any(c["bias"].endswith("-min") for c in CASES)
    assert any(c["dtype"] == torch.bfloat16 and c["D"] == 64 and c["N"] % 8 and c["bias"] == "1h" and "V_QDB64_ON" in c["bits"] for c in CASES)   # the fallback
    assert max(c["B"] * c["H"] * c["M"] * c["N"] for c in CASES) <= 700 * 700 * 12


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_case_names_the_bodies_the_dispatcher_runs(i):
    from flasht5_amd import _lib
    if _lib.load().fat5_chip_cus() != 256:
        pytest.skip("the case list is laid out for the 256 compute units of the MI355X")
    d = describe(CASES[i])
    assert {key: d.get(key) for key in CASES[i]["bodies"]} == CASES[i]["bodies"]


def _autograd(case, t):
    """fp64 autograd of the forward's formula: (dq, dk, dv, dS) with dS the gradient of the additive score term"""
    B, H, M, N = case["B"], case["H"], case["M"], case["N"]
    q, k, v = (t[x].double().clone().requires_grad_(True) for x in ("q", "k", "v"))
    scale = float(torch.tensor(case["scale"], dtype=torch.float32))
    if t["bias"] is not None:
        add = t["bias"].double().expand(B, H, M, N)
    elif t["rpe"] is not None:
        R = case["R"]
        add = t["rpe"].double()[:, (torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R][None].expand(B, H, M, N)
    else:
        add = torch.zeros(B, H, M, N, dtype=torch.float64)
    add = add.clone().requires_grad_(True)
    s = (q @ k.transpose(-1, -2)) * scale + add
    vis = torch.ones(M, N, dtype=torch.bool)
    if case["causal"]:
        vis = torch.arange(M)[:, None] + (N - M) >= torch.arange(N)[None, :]
    vis = vis & ~(add <= F.MASKED)
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1))
    (p @ v).backward(t["do"].double())
    return q.grad, k.grad, v.grad, torch.where(vis, add.grad, torch.zeros(()).double())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_agrees_with_autograd_and_the_oracle(i):
    case = CASES[i]
    if case["pert"]:
        return   # (an inconsistent (o, lse) is no derivative of anything)
    t, ref, _ = _truth(i)
    B, H, M, N, R = case["B"], case["H"], case["M"], case["N"], case["R"]
    if bool((ref["dead"] & (t["lse"] > float("-inf"))).any()):
        return   # (finfo.min on every key of a row: the kernels' dead row is a uniform softmax to autograd)
    # the restatement uses the stored o (rounded to the dtype) and lse (rounded to fp32); autograd its own.  Both roundings move the result by
    # at most u_T TD-like and 2^-24 |lse| T-like amounts: compare with the exact (o, lse) of the same formula instead
    fwd = F.attn_fwd_ref(t["q"], t["k"], t["v"], case["scale"], case["causal"], t["bias"], t["rpe"], R)
    ex = G.attn_bwd_ref(t["q"], t["k"], t["v"], fwd["o"], fwd["lse"], t["do"], case["scale"], case["causal"], t["bias"], t["rpe"], R,
                        t["bucket"], 32 if t["bucket"] is not None else 0)
    dq, dk, dv, ds = _autograd(case, t)
    for x, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool(((ex[x] - g).abs() <= 1e-9 * ex["T_" + x] + 1e-300).all()), (case["id"], x)
    if "dbias" in ex:
        g = ds
        if t["bias"].shape[0] == 1:
            g = g.sum(0, keepdim=True)
        if t["bias"].shape[1] == 1:
            g = g.sum(1, keepdim=True)
        assert bool(((ex["dbias"] - g).abs() <= 1e-9 * ex["T_dbias"] + 1e-300).all()), case["id"]
    if "drpe1d" in ex:
        idx = ((torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R).reshape(-1)
        g = torch.zeros(H, 2 * R + 1, dtype=torch.float64).index_add_(1, idx, ds.sum(0).reshape(H, -1))
        assert bool(((ex["drpe1d"] - g).abs() <= 1e-9 * ex["T_drpe1d"] + 1e-300).all()), case["id"]
        if "drpe_table" in ex:
            gt = torch.zeros(32, H, dtype=torch.float64).index_add_(0, t["bucket"].long(), g.T)
            assert bool(((ex["drpe_table"] - gt).abs() <= 1e-9 * ex["T_drpe_table"] + 1e-300).all()), case["id"]
    # the fp32 oracle, from the stored (o, lse): its evaluation noise is that of fp32 sums of up to max(M, N) terms and of exp at |s - lse|
    b = t["bias"]
    if t["rpe"] is not None:
        b = t["rpe"][:, (torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R].unsqueeze(0)
    if b is not None and bool((b <= F.MASKED).any()):
        return   # (the fp32 oracle has no contract for masking entries)
    L = torch.where(ref["dead"], torch.full_like(t["lse"], float("inf")), t["lse"])   # (dead rows: p = exp(s - inf) = 0 in the oracle)
    oq, ok_, ov, _, ob = oracle.attn_bwd_oracle(t["q"], t["k"], t["v"], b, t["o"], L, t["do"], case["scale"], case["causal"])
    tol = (max(M, N) + 2 * case["D"] + 64) * 2.0 ** -23
    for x, g in (("dq", oq), ("dk", ok_), ("dv", ov)):
        assert bool(((ref[x] - g.double()).abs() <= tol * (ref["T_" + x] + ref["TA_" + x])).all()), (case["id"], x)
    if "dbias" in ref:
        assert bool(((ref["dbias"] - ob.double()).abs() <= tol * (ref["T_dbias"] + ref["TA_dbias"])).all()), case["id"]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_term_magnitudes_dominate_and_the_bound_has_its_shape(i):
    case = CASES[i]
    t, ref, bound = _truth(i)
    for x in G.outputs_of(ref):
        assert bool((ref[x].abs() <= ref["T_" + x] * (1 + 1e-12)).all()), (case["id"], x)
        assert bool(torch.isfinite(bound[x]).all()) and bool((bound[x] >= 0).all()), (case["id"], x)
        assert bool(((bound[x] == 0) == (ref["T_" + x] == 0)).all()), (case["id"], x)
    assert bool((bound["dq"][ref["dead"]] == 0).all())
    if case["causal"] and case["M"] > case["N"]:
        assert bool(ref["dead"][:, :, :case["M"] - case["N"]].all())
    if "dbias" in ref and case["causal"]:
        above = ~(torch.arange(case["M"])[:, None] + (case["N"] - case["M"]) >= torch.arange(case["N"])[None, :])
        assert bool((bound["dbias"][..., above] == 0).all()) and bool((ref["dbias"][..., above] == 0).all())
    if not case["pert"]:
        assert float(ref["smax"].max()) <= 1e-6   # a consistent lse: no p above 1 (+ the fp32 rounding of lse)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_correct_arithmetic_satisfies_the_bound(i):
    case = CASES[i]
    t, ref, bound = _truth(i)
    emu = G.emulate(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], case["scale"], case["causal"], t["bias"], t["rpe"], case["R"], t["bucket"],
                    32 if t["bucket"] is not None else 0, case["bodies"].get("dbias", "direct"))
    r = G.ratios(emu, ref, bound)
    w = EMU.setdefault(case["group"], {})
    for x, v in r.items():
        if v >= w.setdefault(x, [0.0, ""])[0]:
            w[x] = [v, case["id"]]
    assert all(v <= 1.0 for v in r.values()), (case["id"], r)
    # ... and the fp64 result rounded once to the storage dtype
    once = {x: (ref[x].to(case["dtype"]) if x in ("dq", "dk", "dv", "dbias") else ref[x].float()) for x in G.outputs_of(ref)}
    r = G.ratios(once, ref, bound)
    assert all(v <= 1.0 for v in r.values()), (case["id"], r)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_applicable_mutant_violates_the_bound(i):
    case = CASES[i]
    t, ref, bound = _truth(i)
    outs = compared(case, ref)
    bnd = {x: bound[x] for x in outs}
    missed = []
    for name, mutant in G.MUTANTS.items():
        mut = reference(case, t, mutant)
        if not mut["applied"]:
            continue
        caught = not G.within({x: mut[x] for x in outs}, ref, bnd)
        DETECTED[name][case["id"]] = caught
        if not caught and (name, case["id"]) not in EXCUSED:
            missed.append(name)
    assert not missed, f"{case['id']}: the bound does not see {missed}"


def test_zz_every_mutant_applied_and_was_caught():
    """(runs last) per mutant: killed / applied; the excused pairs stay under 5 % and excuse no mutant in a whole group"""
    if sum(len(d) for d in DETECTED.values()) == 0:
        return  # (the mutant test was deselected in this session)
    for group, w in sorted(EMU.items()):
        print(f"[attn-bwd-fp64] emulation, {group}: worst err/bound " + ", ".join(f"{x} {v[0]:.3f} ({v[1]})" for x, v in sorted(w.items())))
    group_of = {c["id"]: c["group"] for c in CASES}
    applied = killed = 0
    for name, d in DETECTED.items():
        print(f"[attn-bwd-fp64] mutant '{name}': killed {sum(d.values())} / applied {len(d)}")
        applied += len(d)
        killed += sum(d.values())
        for cid, caught in d.items():
            assert caught or (name, cid) in EXCUSED, (name, cid)
    if {cid for d in DETECTED.values() for cid in d} != set(group_of):
        return  # (only some cases ran in this session: the limits below are over the whole list)
    print(f"[attn-bwd-fp64] mutants: killed {killed} / applied {applied}, excused {len(EXCUSED)}")
    for name, d in DETECTED.items():
        assert len(d) >= 3, (name, "applies to fewer than three cases")
        for group in {group_of[cid] for cid in d}:
            assert any(caught for cid, caught in d.items() if group_of[cid] == group), (name, group, "excused in every case of the group")
    assert applied - killed <= 0.05 * applied, (killed, applied)
    for name, cid in EXCUSED:
        assert DETECTED[name].get(cid) is False, (name, cid, "a stale exclusion")
