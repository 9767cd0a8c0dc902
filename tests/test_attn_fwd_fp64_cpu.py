"""What tests/test_attn_fwd_fp64_gpu.py rests on, proven without a GPU, on that file's own case list:
  * attn_fwd_ref agrees with oracle.attn_ref(..., upcast=True) and the oracle's L to fp32 evaluation noise, and with the reference's own
    o in the attention fixtures under tests/golden/ within the tolerance tests/test_oracle_golden.py uses for them;
  * the bound of tests/attn_fwd_fp64.py is not below what correct arithmetic achieves: `emulate` (fp32 scores, p rounded to the dtype
    for P.V, row sums of the rounded p in the 64-row bodies, one output rounding) lies within it on every case;
  * the bound is not too loose: every mutant that applies to a case leaves it on that case, in o or in lse; every mutant applies to at
    least three cases and every case has at least two mutants caught on it;
  * every case names the body the dispatcher runs it with (fat5_attn_describe is host-only).
"""
import functools

import pytest
import torch

import attn_fwd_fp64 as F
import oracle
from golden_io import load_attn, ATTN_CASES
from test_attn_fwd_fp64_gpu import CASES, inputs, reference, describe

IDS = [c["id"] for c in CASES]
DETECTED = {name: [0, 0] for name in F.MUTANTS}   # [cases where it applied, cases where the bound caught it]


@functools.lru_cache(maxsize=2)
def _truth(i):
    case = CASES[i]
    t = inputs(case)
    ref = reference(case, t)
    return (t, ref) + F.attn_fwd_bound(ref, case["dtype"], case["D"], case["body"], case["N"])


def test_the_case_list_is_what_the_issue_asks_for():
    def of(group, key):
        return {c[key] for c in CASES if c["group"] == group}
    assert {c["body"] for c in CASES} == set(F.BODIES)
    assert {1, 31, 32, 33, 64, 65, 129} <= of("r32w2", "M") and {1, 63, 64, 65, 127, 128, 129, 200} <= of("r32w2", "N")
    assert of("r32w2", "D") == {16, 32, 64, 128} and all(c["B"] * c["H"] * -(-c["M"] // 128) >= 160 for c in CASES if c["group"] == "r32w4")
    assert {(c["M"], c["N"]) for c in CASES if c["group"] == "split"} >= {(128, n) for n in (128, 129, 160, 191, 192, 193)} | {(100, 200)}
    for g in ("r64", "ksplit"):
        assert {1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300} <= of(g, "M")
        assert {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 320, 513} <= of(g, "N")
    assert of("mixed", "M") == {384, 385, 640, 700} and of("mixed", "N") == {256, 321, 640} and not any(of("mixed", "causal"))
    for g in ("r32w2", "r32w4", "split", "r64", "ksplit", "mixed", "d128", "d128w"):
        assert of(g, "dtype") == {torch.bfloat16, torch.float16}, g
        assert any(of(g, "strided")) or g == "d128w", g
    for g in ("dense64", "dense128"):
        assert {"11", "1h", "b1", "bh", "1h-min"} <= of(g, "bias") and of(g, "causal") == {True, False} and any(of(g, "strided"))
        assert {c["body"] for c in CASES if c["group"] == g and c["N"] % 8} == {"32row"}
    for g in ("r32w2", "split", "r64", "ksplit", "d128"):
        assert {c["R"] for c in CASES if c["group"] == g and c["bias"][:2] == "t5"} == {1, 8, 128}, g
        assert {c["N"] - c["M"] for c in CASES if c["group"] == g and c["causal"]} >= {0, 1, 100, -1, -100}, g
    assert {c["bias"] for c in CASES if c["bias"][:2] == "t5"} == {"t5b", "t5u"}
    assert max(max(c["M"], c["N"]) for c in CASES) <= 700


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_case_names_the_body_the_dispatcher_runs(i):
    from flasht5_amd import _lib
    if _lib.load().fat5_chip_cus() != 256:
        pytest.skip("the case list is laid out for the 256 compute units of the MI355X")
    assert describe(CASES[i])[0] == CASES[i]["body"]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_agrees_with_the_oracle(i):
    case = CASES[i]
    t, ref, _, _ = _truth(i)
    if bool(ref["marker"].any()):
        return   # (finfo.min on every key of a row: the fp32 oracle has no contract for it)
    b = t["bias"]
    if t["rpe"] is not None:
        M, N, R = case["M"], case["N"], case["R"]
        b = t["rpe"][:, (torch.arange(N)[None, :] - torch.arange(M)[:, None]).clamp(-R, R) + R].unsqueeze(0)
    if case["N"] == 0:
        return
    o32, L32 = oracle.attn_fwd_oracle(t["q"], t["k"], t["v"], b, case["scale"], case["causal"])
    live = ref["nvis"] > 0
    o2 = oracle.attn_ref(t["q"], t["k"], t["v"], b, case["scale"], causal=case["causal"], upcast=True)
    # fp32 evaluation noise: N-term sums of weights <= 1 next to values of at most BOOST-fold magnitude
    tol = 1e-5 * (1 + ref["absv"].amax(-1))
    assert bool(((o32.double() - ref["o"]).abs().amax(-1) <= tol).all())
    # (attn_ref rounds p to the dtype it computes in -- fp32 after the upcast -- and leaves dead rows as NaN)
    assert bool(((torch.nan_to_num(o2.double()) - ref["o"]).abs().amax(-1)[live] <= tol[live]).all())
    assert torch.equal(torch.isfinite(L32), torch.isfinite(ref["lse"]))
    assert bool(((L32.double() - ref["lse"]).abs()[live] <= 1e-5 * (1 + ref["lse"].abs()[live])).all())


@pytest.mark.parametrize("name", ATTN_CASES)
def test_agrees_with_the_reference_fixtures(name):
    c = load_attn(name)
    ref = F.attn_fwd_ref(c["q"], c["k"], c["v"], c["sm_scale"], c["causal"], bias=c["bias"])
    # the fixtures hold the reference's fp32 results: 2e-5 is what test_oracle_golden.py::test_attn_cfg1_golden allows between them and an
    # evaluation in another order (its 1e-6 is for the fp32 oracle that repeats the reference's own order of operations)
    assert float((ref["o"] - c["o"].double()).abs().max()) < 2e-5
    assert float((ref["lse"] - c["L"].double()).nan_to_num(0, 0, 0).abs().max()) < 2e-5


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_correct_arithmetic_satisfies_the_bound(i):
    case = CASES[i]
    t, ref, bo, bl = _truth(i)
    o, lse = F.emulate(t["q"], t["k"], t["v"], case["scale"], case["causal"], t["bias"], t["rpe"], case["R"], case["body"])
    ro, rl, same = F.ratios(o, lse, ref, bo, bl)
    assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ro, rl, same)
    # ... and the fp64 result rounded once to the storage dtype
    ro, rl, same = F.ratios(ref["o"].to(case["dtype"]), ref["lse"].float(), ref, bo, bl)
    assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ro, rl, same)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_applicable_mutant_violates_the_bound(i):
    case = CASES[i]
    t, ref, bo, bl = _truth(i)
    caught_here, missed = 0, []
    for name, mutant in F.MUTANTS.items():
        mut = reference(case, t, mutant)
        if not mut["applied"]:
            continue
        caught = not F.within(mut["o"], mut["lse"], ref, bo, bl)
        DETECTED[name][0] += 1
        DETECTED[name][1] += caught
        caught_here += caught
        if not caught:
            missed.append(name)
    assert not missed, f"{case['id']}: the bound does not see {missed}"
    assert caught_here >= 2, f"{case['id']}: fewer than two mutants apply"


def test_zz_every_mutant_applied_and_was_caught():
    """(runs last) per mutant: the cases where it applied, and where the bound caught it -- all of them"""
    if sum(a for a, _ in DETECTED.values()) == 0:
        return  # (the mutant test was deselected in this session)
    for name, (applied, caught) in DETECTED.items():
        print(f"[attn-fwd-fp64] mutant '{name}': applied in {applied} cases, caught in {caught}")
    for name, (applied, caught) in DETECTED.items():
        assert applied >= 3 and caught == applied, (name, applied, caught)
