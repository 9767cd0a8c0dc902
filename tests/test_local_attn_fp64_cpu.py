"""The bound, the emulation, the mutants, `steps` and the case list of tests/local_attn_fp64.py, proven on the CPU: a float32
emulation of the local kernels' arithmetic stays inside the derived bound on every case; every mutant leaves it wherever it changes
anything; `steps` agrees with a brute-force count of the visible pairs; the case list holds every structure it claims."""
import numpy as np
import pytest
import torch

import local_attn_fp64 as LA
from local_attn_fp64 import CASES, MUTANTS, DRPE_ONLY, STRUCTURES

_TRUTH = {}

# (mutant, case id) pairs that apply and stay inside the bound, each with its reason.  Only mutants that touch nothing but drpe1d may be
# listed (asserted below), at most 5 % of the applied pairs, and never every case of a mutant.
BLIND = {
}


def truth(case):
    if case["id"] not in _TRUTH:
        t = LA.inputs(case)
        ref, given = LA.local_ref(case, t)
        _TRUTH[case["id"]] = (t, ref, given, LA.local_bound(case, ref))
    return _TRUTH[case["id"]]


def test_emulation_stays_inside_the_bound():
    worst = {}
    for case in CASES:
        t, ref, given, bound = truth(case)
        r = LA.ratios(LA.emulate(case, t, given), ref, bound)
        assert sorted(r) == sorted(x for x in LA.FWD + LA.BWD if x in ref)
        for x, v in r.items():
            key = (x, "bf16" if case["dtype"] == torch.bfloat16 else "fp16")
            if v >= worst.get(key, (0.0, ""))[0]:
                worst[key] = (v, case["id"])
    for (x, dt), (v, cid) in sorted(worst.items()):
        print(f"[local-fp64] emulation {dt} {x}: worst err / bound {v:.3f} ({cid})")
    assert all(v <= 1.0 for v, _ in worst.values()), worst


def test_zero_bound_means_exact_zero_in_the_restatement():
    for case in CASES:
        _, ref, _, bound = truth(case)
        for x in LA.BWD:
            if x in ref:
                assert not bool(ref[x][bound[x] == 0].abs().any()), (case["id"], x)
        if case["R"]:                                                    # the entries no visible pair reaches
            reach = (torch.arange(2 * case["R"] + 1) - case["R"]).abs() <= min(case["window"], max(case["lens"]) - 1)
            assert torch.equal(ref["n_drpe1d"][0] > 0, reach) and torch.equal(bound["drpe1d"][0] > 0, reach), case["id"]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_leaves_the_bound(name):
    applied = {torch.bfloat16: 0, torch.float16: 0}
    missed = []
    for case in CASES:
        t, ref, given, bound = truth(case)
        mut, _ = LA.local_ref(case, t, mutant=MUTANTS[name], given=given)
        if not mut["exists"]:
            continue
        diff = LA.differs(mut, ref)
        if not diff:
            continue
        assert name not in DRPE_ONLY or diff == ["drpe1d"], (name, case["id"], diff)
        applied[case["dtype"]] += 1
        r = LA.ratios({x: mut[x] for x in bound}, ref, bound)
        if not any(r[x] > 1.0 for x in diff):
            missed.append((case["id"], {x: round(r[x], 3) for x in diff}))
    print(f"[local-fp64] mutant {name!r}: applied on {applied[torch.bfloat16]} bf16 and {applied[torch.float16]} fp16 cases, missed {missed}")
    assert all(applied.values()), f"{name}: applies on no case of a dtype: {applied}"
    listed = {cid for (m, cid) in BLIND if m == name}
    assert not listed or name in DRPE_ONLY, f"{name}: only the drpe1d-only mutants may have blind pairs"
    assert {cid for cid, _ in missed} == listed, f"{name}: inside the bound on {missed}; listed {sorted(listed)}"
    assert len(listed) < sum(applied.values()), f"{name}: every applied case is listed"
    _APPLIED[name] = sum(applied.values())


_APPLIED = {}


def test_zz_blind_pairs_are_few():
    """(runs after the mutants) the listed pairs are at most 5 % of the applied ones"""
    if len(_APPLIED) == len(MUTANTS):
        assert len(BLIND) <= 0.05 * sum(_APPLIED.values())
    assert all(m in DRPE_ONLY and reason for (m, _), reason in BLIND.items())


def test_steps_match_brute_force():
    for L in range(1, 201):
        pos = np.arange(L)
        dist = np.abs(pos[None, :] - pos[:, None])
        nb = (L + 31) // 32
        for window in list(range(1, 131, 3)) + [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130]:
            vis = np.zeros((32 * nb, 32 * nb), dtype=np.int64)
            vis[:L, :L] = dist <= window
            cnt = vis.reshape(nb, 32, nb, 32).sum((1, 3))                # visible pairs per (row step, key step)
            seen = np.zeros_like(cnt)
            for s in LA.all_steps(L, window):
                for wv in s["waves"]:
                    i = wv["r0"] // 32
                    if wv["r0"] >= L:
                        assert not wv["visited"]
                        continue
                    for sb in wv["visited"]:
                        seen[i, sb // 32] = 1
                        assert (cnt[i, sb // 32] == 1024) == (sb in wv["full"]), (L, window, wv["r0"], sb)
                        assert (cnt[i, sb // 32] == 1) == (sb in wv["corner"]), (L, window, wv["r0"], sb)
                        assert s["t_begin"] <= sb // 64 <= s["t_end"]
                    for sb in wv["skipped"]:
                        assert (sb >= 32 * nb or cnt[i, sb // 32] == 0) and s["t_begin"] <= sb // 64 <= s["t_end"], (L, window, wv["r0"], sb)
                    assert sorted(wv["full"] + wv["masked"]) == wv["visited"]
            assert not (cnt * (1 - seen)).any(), (L, window)             # every visible pair lies in a visited step of a streamed tile
            assert len(LA.all_steps(L, window)) == (L + 63) // 64
    # the seams the issue names: skipped iff 32 j > 31 + w, mask-free iff 32 |j| + 31 <= w, one corner pair at w = 32 j - 31
    for w in LA.WS:
        wv = LA.steps(1024, w, 8)["waves"][0]
        for j in range(-6, 7):
            sb = wv["r0"] + 32 * j
            assert (sb in wv["visited"]) == (32 * abs(j) <= 31 + w) and (sb in wv["full"]) == (32 * abs(j) + 31 <= w)
            assert (sb in wv["corner"]) == (j != 0 and w == 32 * abs(j) - 31)


def test_case_list_covers_its_structures():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    for dtype in LA.DTYPES:
        got = set()
        for c in CASES:
            if c["dtype"] == dtype:
                got |= LA.structures_of(c)
        assert got == set(STRUCTURES), (dtype, set(STRUCTURES) - got)
    dense = [c for c in CASES if not c["packed"]]
    assert {c["lens"][0] for c in dense} >= set(LA.LS) | {700, 40} and {c["window"] for c in dense} >= set(LA.WS) | {1012, 1013, 1024}
    for L in (33, 64, 129):
        assert {c["window"] for c in dense if c["lens"][0] == L} >= {L - 1, L, 4 * L}
    assert any(c["R"] == 0 for c in dense) and any(c["scale"] == 0.3 for c in dense) and any(c["strided"] for c in dense)
    rel = {("w-1" if c["R"] == c["window"] - 1 else "w" if c["R"] == c["window"] else "w+1" if c["R"] == c["window"] + 1 else c["R"]) for c in dense}
    assert rel >= {1, 8, 31, 32, 128, "w-1", "w", "w+1"}
    # the dQ kernel's dynamic LDS passes 48 KiB between wc = 1012 and 1013 with the diagonal sums, and not at all without them
    assert LA.local_smem_q(1012, True) <= 48 * 1024 < LA.local_smem_q(1013, True) and LA.local_smem_q(1024, False) <= 48 * 1024
    assert LA.local_smem_q(1024, True) <= 160 * 1024                     # (the LDS of a gfx950 workgroup)
    packed = [c for c in CASES if c["packed"]]
    assert {x for c in packed for x in c["lens"]} >= set(LA.PACK_LENS) and max(len(c["lens"]) for c in packed) >= 40
    assert {c["S"] - max(c["lens"]) for c in packed} >= {0, 64, 200} and {c["dtype"] for c in packed} == set(LA.DTYPES)
    for c in CASES:                                                      # the boosted rows: ends and tile seams of every sequence
        for L in c["lens"]:
            assert not L or {0, L - 1} <= set(LA.boosted(L))
