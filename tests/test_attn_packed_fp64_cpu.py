"""What tests/test_attn_packed_fp64_gpu.py rests on, proven without a GPU, on the case list of tests/attn_packed_fp64.py:
  * the list holds every structural edge of the packed (cu_seqlens) layout it is meant to hold, and every case names the bodies the
    dispatcher runs it with (fat5_attn_describe is host-only; the wave counts are restated from pick_nw);
  * the packed restatement IS the dense one per sequence (the same numbers on a one-sequence batch);
  * the bounds of the dense harnesses, applied per sequence, are not below what correct arithmetic achieves: `emulate_packed_*` lies
    within them on every case, forward and backward;
  * they are not too loose: every packed mutant that applies to a case leaves the bound on that case, and every mutant applies to at
    least three cases.
"""
import functools

import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
import attn_packed_fp64 as P
from attn_packed_fp64 import CASES, inputs, fwd_reference, bwd_reference, describe, assert_bodies, cumulate

IDS = [c["id"] for c in CASES]
DETECTED = {("fwd", name): [0, 0] for name in P.PACKED_MUTANTS_FWD}   # [cases where it applied, cases where the bound caught it]
DETECTED.update({("bwd", name): [0, 0] for name in P.PACKED_MUTANTS_BWD})


@functools.lru_cache(maxsize=2)
def _truth(i):
    case = CASES[i]
    t = inputs(case)
    fwd = fwd_reference(case, t)
    bwd = bwd_reference(case, t)
    return t, fwd, P.packed_fwd_bound(fwd, case["dtype"], case["D"], case["body"]), bwd, P.packed_bwd_bound(bwd, case["dtype"], case["D"], case["bodies"])


def _pairs(c):
    return list(zip(c["lens_q"], c["lens_k"]))


def test_the_case_list_is_what_the_issue_asks_for():
    allp = {p for c in CASES for p in _pairs(c)}
    assert {(0, 0), (1, 1)} <= allp and any(m == 0 and n > 0 for m, n in allp) and any(m > 0 and n == 0 for m, n in allp)
    assert {x for c in CASES for x in c["lens_q"] + c["lens_k"]} == set(P.LENGTHS)
    empty = lambda c, b: _pairs(c)[b] == (0, 0)
    assert any(empty(c, 0) for c in CASES) and any(empty(c, len(c["lens_q"]) - 1) for c in CASES)
    assert any(empty(c, b) and 0 < b < len(c["lens_q"]) - 1 for c in CASES for b in range(len(c["lens_q"])))
    assert any(empty(c, b) and empty(c, b + 1) for c in CASES for b in range(len(c["lens_q"]) - 1))
    assert any(len(c["lens_q"]) == 1 for c in CASES)
    for g, over in (("w2", 128), ("w4", 128), ("one", 64)):   # (more than one workgroup's rows / keys: 128 at four waves, 64 in the split body and at two waves)
        cs = [c for c in CASES if c["group"] == g]
        assert any(c["max_q"] == max(c["lens_q"]) and c["max_k"] == max(c["lens_k"]) for c in cs), g
        assert any(c["max_q"] - max(c["lens_q"]) > over for c in cs) and any(c["max_k"] - max(c["lens_k"]) > over for c in cs), g
        assert {c["dtype"] for c in cs} == {torch.bfloat16, torch.float16} and {c["D"] for c in cs} == {16, 32, 64, 128}, g
        assert any(c["pert"] for c in cs) and any(c["causal"] for c in cs) and any(c["R"] for c in cs), g
    for rpe in (False, True):   # causal with M_b < N_b, = N_b and > N_b in one batch
        assert any(c["causal"] and bool(c["R"]) == rpe and {(m < n) - (m > n) for m, n in _pairs(c) if m and n} == {-1, 0, 1} for c in CASES), rpe
    cross = lambda c: cumulate(c["lens_q"]) != cumulate(c["lens_k"])
    assert {c["R"] for c in CASES if c["R"] and cross(c)} == {1, 8, 128} and {c["R"] for c in CASES if c["R"] and not cross(c)} == {1, 8, 128}
    assert any(c["qkv"] for c in CASES) and all(not cross(c) for c in CASES if c["qkv"])
    assert any(s % 2 for c in CASES for s in cumulate(c["lens_q"])[1:-1]) and any(s % 8 and s % 32 for c in CASES for s in cumulate(c["lens_k"])[1:-1])
    assert {(c["body"], c["waves"]) for c in CASES} == {("32row", 2), ("32row", 4), ("32row-split", 2)}
    assert {(c["bodies"]["fused"], c["bwd_waves"]) for c in CASES} == {("0", 2), ("0", 4), ("1", 4)}
    assert max(max(sum(c["lens_q"]), sum(c["lens_k"])) for c in CASES) <= 1500
    assert all(c["H"] == 2 for c in CASES if c["group"] == "w2")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_case_names_the_bodies_the_dispatcher_runs(i):
    from flasht5_amd import _lib
    if _lib.load().fat5_chip_cus() != 256:
        pytest.skip("the case list is laid out for the 256 compute units of the MI355X")
    assert_bodies(CASES[i], describe(CASES[i]))


def test_describe_reads_the_packed_flag():
    """the 64-wide bodies are never chosen for a packed call (`!k.packed`, attn_dispatch.h), whatever the variant asks for"""
    from flasht5_amd import _lib
    bits = _lib.V_FWD64_ON | _lib.V_KV64_ON | _lib.V_Q64_ON
    dense = _lib.describe(4, 12, 1024, 1024, variant=bits)
    packed = _lib.describe(4, 12, 1024, 1024, variant=bits, packed=True, total_q=4096)
    assert dense["fwd"].startswith("64row") and dense["dq"] == "64row" and dense["dkdv"].startswith("64key")
    assert packed["fwd"].startswith("32row") and packed["dq"] == "32row" and packed["dkdv"] == "32key"


def test_one_sequence_is_the_dense_restatement():
    case = next(c for c in CASES if len(c["lens_q"]) == 1 and c["R"])
    t, fwd, (bo, bl), bwd, bb = _truth(CASES.index(case))
    q, k, v, o, do = (x.permute(1, 0, 2).unsqueeze(0) for x in (t["q"], t["k"], t["v"], t["o"], t["do"]))
    M, N = case["lens_q"][0], case["lens_k"][0]
    df = F.attn_fwd_ref(q, k, v, case["scale"], case["causal"], None, t["rpe"], case["R"])
    dbo, dbl = F.attn_fwd_bound(df, case["dtype"], case["D"], case["body"], N)
    assert torch.equal(df["o"][0].permute(1, 0, 2), fwd["o"]) and torch.equal(df["lse"][0], fwd["lse"])
    assert torch.equal(dbo[0].permute(1, 0, 2), bo) and torch.equal(dbl[0], bl)
    db = G.attn_bwd_ref(q, k, v, o, t["lse"].unsqueeze(0), do, case["scale"], case["causal"], None, t["rpe"], case["R"])
    dbb = G.attn_bwd_bound(db, case["dtype"], case["D"], case["bodies"], N, M)
    for x in ("dq", "dk", "dv"):
        assert torch.equal(db[x][0].permute(1, 0, 2), bwd[x]) and torch.equal(dbb[x][0].permute(1, 0, 2), bb[x]), x
    assert torch.equal(db["drpe1d"], bwd["drpe1d"]) and torch.equal(dbb["drpe1d"], bb["drpe1d"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_structural_exact_zeros(i):
    """a sequence without keys: o = 0, lse = -inf, dq = 0 with the bound 0; without queries: dk = dv = 0 with the bound 0; causal rows
    without a visible key likewise"""
    case = CASES[i]
    t, fwd, (bo, bl), bwd, bb = _truth(i)
    cq, ck = t["cu_q"], t["cu_k"]
    for b, (m, n) in enumerate(_pairs(case)):
        if n == 0 and m:
            sl = slice(cq[b], cq[b + 1])
            assert not fwd["o"][sl].any() and not bo[sl].any() and bool((fwd["lse"][:, sl] == -float("inf")).all())
            assert not bwd["dq"][sl].any() and not bb["dq"][sl].any()
        if m == 0 and n:
            sl = slice(ck[b], ck[b + 1])
            assert not bwd["dk"][sl].any() and not bwd["dv"][sl].any() and not bb["dk"][sl].any() and not bb["dv"][sl].any()
        if case["causal"] and m > n:
            sl = slice(cq[b], cq[b] + m - n)
            assert bool((fwd["lse"][:, sl] == -float("inf")).all()) and not bo[sl].any() and not bb["dq"][sl].any()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_correct_arithmetic_satisfies_the_bound(i):
    case = CASES[i]
    t, fwd, (bo, bl), bwd, bb = _truth(i)
    o, lse = P.emulate_packed_fwd(t["q"], t["k"], t["v"], t["cu_q"], t["cu_k"], case["scale"], case["causal"], t["rpe"], case["R"], case["body"])
    ro, rl, same = F.ratios(o, lse, fwd, bo, bl)
    assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ro, rl, same)
    ro, rl, same = F.ratios(fwd["o"].to(case["dtype"]), fwd["lse"].float(), fwd, bo, bl)      # ... and the fp64 result rounded once
    assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ro, rl, same)
    got = P.emulate_packed_bwd(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], t["cu_q"], t["cu_k"], case["scale"], case["causal"], t["rpe"], case["R"])
    r = G.ratios(got, bwd, bb)
    assert sorted(r) == sorted(["dq", "dk", "dv"] + (["drpe1d"] if case["R"] else [])) and all(x <= 1.0 for x in r.values()), (case["id"], r)
    once = {x: (bwd[x].to(case["dtype"]) if x != "drpe1d" else bwd[x].float()) for x in r}
    assert G.within(once, bwd, bb), (case["id"], G.ratios(once, bwd, bb))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_applicable_mutant_violates_the_bound(i):
    case = CASES[i]
    t, fwd, (bo, bl), bwd, bb = _truth(i)
    missed = []
    for name, mutant in P.PACKED_MUTANTS_FWD.items():
        mut = fwd_reference(case, t, mutant)
        if not mut["applied"]:
            continue
        caught = not F.within(mut["o"], mut["lse"], fwd, bo, bl)
        DETECTED[("fwd", name)][0] += 1
        DETECTED[("fwd", name)][1] += caught
        if not caught:
            missed.append("fwd: " + name)
    for name, mutant in P.PACKED_MUTANTS_BWD.items():
        mut = bwd_reference(case, t, mutant)
        if not mut["applied"]:
            continue
        caught = not G.within(mut, bwd, bb)
        DETECTED[("bwd", name)][0] += 1
        DETECTED[("bwd", name)][1] += caught
        if not caught:
            missed.append("bwd: " + name)
    assert not missed, f"{case['id']}: the bound does not see {missed}"


def test_zz_every_mutant_applied_and_was_caught():
    """(runs last) per mutant: the cases where it applied, and where the bound caught it -- all of them"""
    if sum(a for a, _ in DETECTED.values()) == 0:
        return  # (the mutant test was deselected in this session)
    for (side, name), (applied, caught) in DETECTED.items():
        print(f"[attn-packed-fp64] {side} mutant '{name}': applied in {applied} cases, caught in {caught}")
    for key, (applied, caught) in DETECTED.items():
        assert applied >= 3 and caught == applied, (key, applied, caught)
