"""What tests/test_adamw_exact_gpu.py rests on, proven without a GPU on that file's own cases:
  * the fused multiply-add helper is exact (against fractions.Fraction);
  * the generator's parameters have a sum of squares that is exact in fp32 in any order, tensor by tensor;
  * the emulation lies within a derived bound of the same step in plain fp64, its two contraction variants agree to one ulp, and it
    agrees with the CPU oracle (oracle/adamw_scale.py) to one ulp per element in fp32 and at the fixture test's bar in 16 bit;
  * every mutant of adamw_exact.MUTANTS, on every case it applies to, leaves at least one element outside `admissible`;
  * every GPU case's descriptor table satisfies the ABI's chunk_begin rule and the placement it claims.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import adamw_exact as X
import oracle
from adamw_exact import F32, F16, BF16
from rowwise_fp64 import ulp
from test_adamw_exact_gpu import CASES, IDS, ROLES, case_pointers, host_table, inputs, table_prefactor

DETECTED = {name: [0, 0] for name in X.MUTANTS}   # [cases where it applied, cases where `admissible` caught it]
FINITE = [i for i, c in enumerate(CASES) if not c["overflow"]]


def _rne32(fr):
    """a Fraction rounded once to the nearest float32, ties to even (normal range)"""
    if fr == 0:
        return np.float32(0.0)
    s, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    scaled = a / Fraction(2) ** (e - 23)          # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(s * float(Fraction(n) * Fraction(2) ** (e - 23)))


def test_fma32_is_one_rounding_of_the_exact_result():
    rs = np.random.RandomState(5)
    n = 4000
    a = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(np.float32)
    b = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(np.float32)
    c = (rs.standard_normal(n) * 2.0 ** rs.randint(-30, 30, n)).astype(np.float32)
    # near-cancellation and near-midpoint triples: c close to -a*b, and c huge against a*b (the sticky bit decides)
    c[:1000] = -(a[:1000] * b[:1000]) * (1 + rs.randint(-3, 4, 1000) * 2.0 ** -23).astype(np.float32)
    c[1000:1500] = (a[1000:1500] * b[1000:1500]) * np.float32(2.0 ** 24) * (1 + rs.randint(0, 2, 500) * 2.0 ** -23).astype(np.float32)
    c[1500:2000] = (a[1500:2000] * b[1500:2000]) * np.float32(2.0 ** 25)
    got = X.fma32(a, b, c)
    differs_from_two_roundings = 0
    for i in range(n):
        want = _rne32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)
        differs_from_two_roundings += (a[i] * b[i] + c[i]) != want
    assert differs_from_two_roundings > 50   # the triples do tell a fused from an unfused multiply-add


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_generator_sum_of_squares_is_exact_in_any_order(i):
    tensors, _ = inputs(i)
    cfg = CASES[i]["cfg"]
    assert all(tensors[j]["floor"] for j in CASES[i]["floor_at"])
    for t in tensors:
        assert X.exactness_proof(t["p"], t["quantum"]), (CASES[i]["id"], t["p"].numel())
        rms = (float((t["p"].double() ** 2).sum()) / t["p"].numel()) ** 0.5
        assert (rms < 4.9e-4) if t["floor"] else (rms > 1e-2), (CASES[i]["id"], rms)     # far from the 1e-3 floor on its side
        assert t["p"].dtype is cfg["dt"] and t["g"].dtype is cfg["dt"] and t["m"].dtype is cfg["sdt"] and t["v"].dtype is cfg["sdt"]
        assert bool((t["g"] != 0).all()) and bool((t["m"] != 0).all()) and bool((t["v"] >= 0).all())
        assert float(t["g"].float().abs().max()) <= 2.0 and float(t["g"].float().abs().min()) >= 2.0 ** -12.01


def test_the_case_list_is_what_the_issue_asks_for():
    edges = [c for c in CASES if c["table"] == "edges" and c["id"].endswith("aligned")]
    for tr in X.TRIPLES:
        mine = [c["cfg"] for c in edges if (c["cfg"]["dt"], c["cfg"]["sdt"], c["cfg"]["kahan"]) == tr]
        assert {c["plain"] for c in mine} == {0, 1} and {c["wd"] > 0 for c in mine} == {False, True}, tr
        assert {c["entry"] for c in mine} == {"step", "clipped", "dev"} and {c["step"] for c in mine} == {1, 1000}, tr
    assert X.EDGES == [1, 8191, 8192, 8193, 7, 16384, 16385, 3, 24571, 65536, 9, 1]
    assert {n % 8 for n in X.TAILS if n < X.CHUNK} == set(range(1, 8)) and {n % 8 for n in X.TAILS if n >= X.CHUNK} == set(range(8))
    many = X.many_numels()
    assert len(many) == 301 and {(n + X.CHUNK - 1) // X.CHUNK for n in many} == {1, 2, 3}
    assert [(n + X.CHUNK - 1) // X.CHUNK for n in many[:3]] == [1, 2, 3]
    assert {c["table"] for c in CASES} >= {"edges", "tails", "many301", "many1", "many2", "many3", "deep", "floor", "overflow"}
    assert sum(c["table"] == "deep" for c in CASES) == 2 and (X.DEEP[1] + X.CHUNK - 1) // X.CHUNK == 257
    assert len({(c["cfg"]["dt"], c["cfg"]["sdt"], c["cfg"]["kahan"]) for c in CASES if c["table"] == "many301"}) == 2
    assert {c["cfg"]["plain"] for c in CASES if c["table"] == "floor"} == {0, 1}
    assert {c["id"].rsplit("-", 1)[1] for c in CASES} >= {"aligned", "p+1", "g+1", "k+1", "mv+1"}
    assert all(sum(c["numels"]) <= 2_200_000 for c in CASES)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_descriptor_table_follows_the_abi(i):
    from flasht5_amd.adamw_scaled import _Desc, CHUNK
    case = CASES[i]
    cfg = case["cfg"]
    bases = {r: (j + 1) << 32 for j, r in enumerate(ROLES)}          # 16-byte aligned stand-ins for the device buffers
    ptrs = case_pointers(case, bases)
    tab, total = host_table(case["numels"], cfg, ptrs, table_prefactor(cfg))
    assert CHUNK == X.CHUNK and ctypes.sizeof(_Desc) == 56
    run = 0
    for j, n in enumerate(case["numels"]):
        assert tab[j].chunk_begin == run and tab[j].numel == n
        run += (n + CHUNK - 1) // CHUNK
        for r in ROLES:
            if r == "k" and not cfg["kahan"]:
                assert tab[j].k is None
                continue
            dt = cfg["sdt"] if r in "mv" else cfg["dt"]
            want = case["shifts"][r] * X.SIZE[dt]
            assert getattr(tab[j], r) % 16 == want, (case["id"], j, r)
    assert tab[len(case["numels"])].chunk_begin == run == total
    # sentinels: at least 64 elements between neighbours and at both ends
    for r in ROLES:
        dt = cfg["sdt"] if r in "mv" else cfg["dt"]
        offs, size = X.layout(case["numels"], dt, case["shifts"][r])
        ends = [0] + [o + n for o, n in zip(offs, case["numels"])]
        assert all(o - e >= 64 for o, e in zip(offs, ends)) and size - ends[-1] >= 64
    if cfg["entry"] == "dev":
        assert tab[0].step_prefactor == np.float32(1e30) and float(X.dev_scalars(cfg)[0]) != tab[0].step_prefactor


def _ulp_apart(a, b, dt, before):
    """|a - b| in units of the spacing of dt at the larger of |b| and |before| (the operand the result was formed from: a sum that
    cancels is exact, and its error is the error of its operands)"""
    at = torch.maximum(b.double().abs(), before.double().abs())
    return ((a.double() - b.double()).abs() / ulp(at, dt)).max().item() if a.numel() else 0.0


@pytest.mark.parametrize("i", FINITE, ids=[IDS[i] for i in FINITE])
def test_emulation_is_within_its_bound_of_fp64_and_its_variants_within_one_ulp(i):
    case = CASES[i]
    cfg = case["cfg"]
    tensors, expect = inputs(i)
    for t, var in zip(tensors, expect):
        R = X.adamw_fp64(t["p"], t["g"], t["m"], t["v"], t["k"], cfg)
        B = X.bound_fp64(R, cfg)
        for r in var:
            for key in ("p", "m", "v") + (("k",) if cfg["kahan"] else ()):
                err = np.abs(r[key].double().numpy() - R[key])
                assert (err <= B[key]).all(), (case["id"], key, t["p"].numel(), float((err / np.maximum(B[key], 1e-300)).max()))
        assert torch.equal(X.bits(var[0]["m"]), X.bits(var[1]["m"])) and torch.equal(X.bits(var[0]["v"]), X.bits(var[1]["v"]))
        # one ulp of p's dtype at the larger of |p| before and after the update: where p + upd cancels, the sum is exact and the
        # variants differ by the rounding of upd itself (half an ulp of upd, |upd| <= |p| + |p'|), which is many ulps of a small result.
        # The decay op then rounds each variant once more: two ulps after it.
        mid = [torch.from_numpy(np.ascontiguousarray(r["p_mid"])).double() for r in var]
        at = torch.maximum(t["p"].double().abs(), torch.maximum(mid[0].abs(), mid[1].abs()))
        apart = ((mid[0] - mid[1]).abs() / ulp(at, cfg["dt"])).max().item()
        after = ((var[0]["p"].double() - var[1]["p"].double()).abs() / ulp(at, cfg["dt"])).max().item()
        print(f"[adamw-exact] {case['id']} numel {t['p'].numel()}: variants apart {apart} ulp before the decay, {after} after")
        assert apart <= 1.0 and after <= 2.0, (case["id"], apart, after)


ULP_MAX = {F32: 2.0 ** -23, F16: 2.0 ** -10, BF16: 2.0 ** -7}     # tests/test_adamw_gpu.py ULP / TINY: the fixture test's bar
TINY_MAX = {F32: 0.0, F16: 2.0 ** -24, BF16: 0.0}


@pytest.mark.parametrize("i", FINITE, ids=[IDS[i] for i in FINITE])
def test_emulation_agrees_with_the_cpu_oracle(i):
    case = CASES[i]
    cfg = case["cfg"]
    tensors, expect = inputs(i)   # (torch's CPU norm sums in its own order: exact all the same, the parameters are dyadic)
    for t, var in zip(tensors, expect):
        p, m, v = t["p"].clone(), t["m"].clone(), t["v"].clone()
        k = t["k"].clone() if cfg["kahan"] else None
        g = t["g"].clone()
        if cfg["entry"] == "clipped":
            g.mul_(cfg["coef"])                                        # clip_grad_norm_'s in-place multiply
        oracle.adamw_scale_step(p, g, m, v, k, cfg["step"], cfg["lr"], cfg["beta1"], cfg["beta2"], cfg["wd"], cfg["eps"], not cfg["plain"])
        # the oracle restates the reference's ops, each an fp32 operation and then a conversion: it is compared with the variants
        # that round that way.  The once-rounded half variants (`mix`) differ from those by at most one ulp at each of the two
        # sites of m and of v (the product, then the fmaf that takes it), at the magnitude of the operand or the result.
        for r in var:
            if r["mix"]:
                twin = var[int(r["contract"])]
                for key in ("m", "v"):
                    far = _ulp_apart(r[key], twin[key], cfg["sdt"], t[key])
                    # (the clipped entry adds the site :131: g one ulp apart moves a1 * g by one ulp of that term, a2 * g * g by two)
                    extra = {"m": 1.0, "v": 2.0}[key] if cfg["entry"] == "clipped" and cfg["dt"] is F16 else 0.0
                    assert far <= 2.0 + extra, (case["id"], key, "once / twice rounded", far)
                continue
            if cfg["dt"] is F32 and cfg["sdt"] is F32:
                for got, want, key in ((r["m"], m, "m"), (r["v"], v, "v")):
                    far = _ulp_apart(got, want, F32, t[key])
                    assert far <= 1.0, (case["id"], key, t["p"].numel(), far)
                # p: torch's CPU addcdiv forms (value * m) / den where the kernel (and torch's device kernel) forms value * (m / den):
                # two roundings each, every one at most 2^-24 |upd| <= 1 ulp of upd: 4 ulp apart; the sum p + upd rounds once on either
                # side (1 ulp apart more), the decay once more.  The unit is the spacing at the largest operand, max(|p|, |upd|, |p'|).
                at = torch.maximum(torch.maximum(t["p"].double().abs(), p.double().abs()), torch.from_numpy(np.abs(r["upd"])).double())
                far = ((r["p"].double() - p.double()).abs() / ulp(at, F32)).max().item()
                assert far <= (6.0 if cfg["wd"] > 0 else 5.0), (case["id"], "p", t["p"].numel(), far)
                continue

            def ulp_err(got, want):
                w = want.float()
                return (got.float() - w).abs().max().item() / (ULP_MAX[got.dtype] * max(w.abs().max().item(), 1e-30))

            assert ulp_err(r["m"], m) <= 1.0, (case["id"], "m", ulp_err(r["m"], m))
            assert ulp_err(r["v"], v) <= 1.0 or (r["v"].float() - v.float()).abs().max().item() <= 2 * TINY_MAX[v.dtype], (case["id"], "v")
            moved = (p.float() - t["p"].float()).abs().max().item()
            if True:
                # the fixture test's bar for p in its general form (its `use_state_dtype` branch): the one-ulp freedom of m and v moves
                # each update by that relative amount.  With states of p's own dtype the fixture drops that term because its updates
                # are small beside p; here a small v makes them as large as p itself.
                perr = (r["p"].float() - p.float()).abs().max().item()
                assert perr <= 3 * ULP_MAX[cfg["sdt"]] * moved + 2 * ULP_MAX[cfg["dt"]] * p.float().abs().max().item(), (case["id"], "p", perr, moved)
            if cfg["kahan"]:
                gsum, wsum = r["p"].float() + r["k"].float(), p.float() + k.float()
                tol = ULP_MAX[cfg["dt"]] * (2 * moved + 4 * k.float().abs().max().item()) + 1e-12
                assert (gsum - wsum).abs().max().item() <= tol, (case["id"], "p+k", (gsum - wsum).abs().max().item(), tol)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_applicable_mutant_leaves_the_admissible_set(i):
    case = CASES[i]
    cfg = case["cfg"]
    tensors, expect = inputs(i)
    missed = []
    for name in X.MUTANTS:
        if not X.MUTANTS[name](cfg, tensors):
            continue
        mutant = X.run_table(tensors, cfg, name)
        if not X.applies(name, cfg, tensors, expect, mutant):
            continue
        caught = False
        for var, mut in zip(expect, mutant):
            # the mutant kernel is free to contract either way too: it is caught only if NEITHER of its variants is admissible
            if all(not X.admissible(mv, var)[0] for mv in mut):
                caught = True
                break
        DETECTED[name][0] += 1
        DETECTED[name][1] += caught
        if not caught:
            missed.append(name)
    assert not missed, f"{case['id']}: the check does not see the mutants {missed}"


def test_zz_every_mutant_applied_and_was_caught():
    """(runs last) per mutant: the cases where it applied, and where the check caught it -- all of them"""
    if sum(a for a, _ in DETECTED.values()) == 0:
        return  # (the mutant test was deselected in this session)
    for name, (applied, caught) in DETECTED.items():
        print(f"[adamw-exact] mutant '{name}': applied in {applied} cases, caught in {caught}")
    for name, (applied, caught) in DETECTED.items():
        assert applied >= 1 and caught == applied, (name, applied, caught)
