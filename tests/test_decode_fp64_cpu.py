"""What tests/test_decode_fp64_gpu.py rests on, proven without a GPU, on that file's own case table:
  * the bound of tests/decode_fp64.py tells every applicable mutant from the truth in every case (a bound that a kernel with a
    dropped key, a shifted bias index or a wrong parent row would pass checks nothing);
  * the bound is not below what correct arithmetic achieves: the fp64 result rounded once to the storage dtype satisfies it, and
    a float32 eager evaluation of the same formula satisfies it with the ulp_T / 2 term removed;
  * decode_ref agrees with the restatement the older decode tests use.
"""
import functools
import math

import pytest
import torch

import decode_fp64 as F
from rowwise_fp64 import ulp
from test_decode_fp64_gpu import CASES, RUNS, launches, reference
from test_decode_gpu import LEN_SETS, _ref

RUN_IDS = [f"{c['id']}-s{eff}" for c, _, eff in RUNS]
DETECTED = {name: [0, 0] for name in F.MUTANTS}   # [cases where it applied, cases where the bound caught it]


@functools.lru_cache(maxsize=2)
def _truth(i):
    """(launch, reference, bound_o, bound_lse) per launch of RUNS[i]"""
    case, _, eff = RUNS[i]
    out = []
    for ln in launches(case, eff):
        ref = reference(case, ln, eff)
        out.append((ln, ref) + F.decode_bound(ref, case["dtype"], case["D"], eff))
    return out


def test_the_case_table_is_what_the_issue_asks_for():
    kinds = {c["kind"] for c in CASES}
    assert kinds == {"table", "auto", "spot", "mirror", "radius", "bidx", "rowmap", "fused", "abi"}
    for kind in kinds:
        assert {c["dtype"] for c in CASES if c["kind"] == kind} == {torch.bfloat16, torch.float16}, kind
    for kind in ("table", "spot", "mirror"):
        assert {c["D"] for c in CASES if c["kind"] == kind} == {64, 128}, kind
    assert {(c["append"], bool(c["R"])) for c in CASES if c["kind"] == "table"} == {(a, b) for a in (True, False) for b in (True, False)}
    assert all({e for _, e in c["splits"]} == {1, 2, 5, F.DEC_MAX_SPLITS} for c in CASES if c["kind"] == "table")
    assert len({c["scale"] for c in CASES if "scale" in c}) == 2
    for c, _, eff in RUNS:   # the sizes stay small
        for ln in launches(c, eff) if c["kind"] != "table" else []:
            assert ln["q"].shape[0] <= 4 and ln["q"].shape[2] <= 12 and ln["kc"].shape[1] <= 8256
    # lengths on both sides of every boundary, from the constants
    for D in (64, 128):
        G, P = F.groups(D), F.wg_pass(D)
        assert (G, P) == ((32, 128) if D == 64 else (16, 64))
        for s in (1, 2, 5, 128):
            from test_decode_fp64_gpu import table_lengths
            Ls = table_lengths(D, s)
            assert {1, 2, G - 1, G, G + 1, P - 1, P, P + 1, 2 * P + 1} <= set(Ls)
            assert s * P > 8255 or {s * P, s * P + 1, s * P + P - 1} <= set(Ls)
            assert {s, s + 1} <= set(Ls) and (s == 1 or s - 1 in Ls)
        assert 1 in table_lengths(D, 128)   # one key, 127 empty splits


@pytest.mark.parametrize("i", range(len(RUNS)), ids=RUN_IDS)
def test_every_applicable_mutant_violates_the_bound(i):
    case, _, eff = RUNS[i]
    truth = _truth(i)
    for name, mutant in F.MUTANTS.items():
        applied = caught = False
        for ln, ref, bo, bl in truth:
            mut = reference(case, ln, eff, mutant)
            if not mut["applied"]:
                continue
            applied = True
            if not F.within(mut["o"], mut["lse"], ref, bo, bl):
                caught = True
                break
        DETECTED[name][0] += applied
        DETECTED[name][1] += caught
        assert caught or not applied, f"{case['id']} at {eff} splits: the bound does not see the mutant '{name}'"


@pytest.mark.parametrize("i", range(len(RUNS)), ids=RUN_IDS)
def test_correct_arithmetic_satisfies_the_bound(i):
    case, _, eff = RUNS[i]
    for ln, ref, bo, bl in _truth(i):
        # the fp64 result rounded once to the storage dtype
        ro, rl, same = F.ratios(ref["o"].to(case["dtype"]), ref["lse"].float(), ref, bo, bl)
        assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ln["lens"], ro, rl)
        # float32 eager, without the storage rounding's share of the bound
        o32, l32 = _eager32(ln)
        ro, rl, same = F.ratios(o32, l32, ref, bo - 0.5 * ulp(ref["o"], case["dtype"]), bl)
        assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ln["lens"], ro, rl)


def _eager32(ln):
    """the contract in float32 torch ops"""
    q, kc, vc = ln["q"][:, 0].float(), ln["kc"].float(), ln["vc"].float()
    B, H, D = q.shape
    cacheB, cap = kc.shape[:2]
    o, lse = torch.zeros(B, H, D), torch.full((B, H), -math.inf)
    for b in range(B):
        n = max(0, min(ln["lens"][b], cap))
        app = ln["kn"] is not None and n < cap
        L = n + app
        if L == 0:
            continue
        j = torch.arange(L)
        if ln["row_batch"] is not None:
            src = ln["row_batch"][b, :L].long().clamp(0, cacheB - 1)
        elif ln["batch_idx"] is not None:
            src = torch.full((L,), max(0, min(ln["batch_idx"][b], cacheB - 1)))
        else:
            src = torch.full((L,), b)
        if app:
            src[L - 1] = 0
        K, V = kc[src, j], vc[src, j]
        if app:
            K[L - 1], V[L - 1] = ln["kn"][b, 0].float(), ln["vn"][b, 0].float()
        s = torch.einsum("hd,lhd->hl", q[b], K) * ln["scale"]
        if ln["rpe"] is not None:
            s = s + ln["rpe"][:, (j - (L - 1)).clamp(-ln["R"], ln["R"]) + ln["R"]]
        lse[b] = torch.logsumexp(s, -1)
        o[b] = torch.einsum("hl,lhd->hd", torch.softmax(s, -1), V)
    return o, lse


def test_zz_every_mutant_applied_and_was_caught():
    """(runs last) per mutant: the cases where it applied, and where the bound caught it -- all of them"""
    if sum(a for a, _ in DETECTED.values()) == 0:
        return  # (the mutant test was deselected in this session)
    for name, (applied, caught) in DETECTED.items():
        print(f"[decode-fp64] mutant '{name}': applied in {applied} cases, caught in {caught}")
    for name, (applied, caught) in DETECTED.items():
        assert applied >= 3 and caught == applied, (name, applied, caught)


@pytest.mark.parametrize("append", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_agrees_with_the_older_restatement(append, bias):
    g = torch.Generator().manual_seed(11)
    B, H, D, R = 3, 4, 64, 128
    cap = max(max(s) for s in LEN_SETS) + 2
    kc, vc = (torch.randn(B, cap, H, D, generator=g).bfloat16() for _ in range(2))
    rpe = torch.randn(H, 2 * R + 1, generator=g) if bias else None
    for lens in LEN_SETS:
        q, kn, vn = (torch.randn(B, 1, H, D, generator=g).bfloat16() for _ in range(3))
        if not append:
            kn = vn = None
        ref = F.decode_ref(q, kc, vc, kn, vn, lens, 0.125, rpe, R if bias else 0)
        o, lse = _ref(q, kc, vc, kn[:, 0] if append else None, vn[:, 0] if append else None, lens, 0.125, rpe, R)
        assert float((ref["o"] - o).abs().max()) <= 1e-12
        fin = torch.isfinite(lse)
        assert torch.equal(torch.isfinite(ref["lse"]), fin) and float((ref["lse"] - lse)[fin].abs().max()) <= 1e-12
