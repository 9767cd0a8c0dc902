"""Where the T5 radius changes the STRUCTURE of an attention call, found on the host and pinned as a table.

`fat5_attn_describe`, `fat5_attn_bwd_kvres`, `fat5_attn_bwd_launches` and the parameter check of `fat5_attn_bwd_stages` (its LDS refusal
comes ahead of the pointer checks, so a call without tensors answers it) are host-only.  `scan()` walks R = 1 .. 2048 at head dimensions
16 / 32 / 64 / 128, without variant bits and with the forcing bits of the fp64 suites, causal on and off, with and without a bias gradient,
at the shape classes of tests/test_attn_radius_fp64_gpu.py, and lists every R at which a reported field changes.  TRANSITIONS is that list
as committed: a change to an LDS budget (csrc/attn_dispatch.h, the smem_* formulas) shows up here as a diff.  Some entries move with
the class's shape rather than with the table (N = R + 200 passing 512 keys ends the resident K / V form; B H ceil(M / 64) reaching 96
starts the split forward): they are marked "shape".

The GPU case list has, for every transition, a pair of cases that differ in nothing but the radius -- one at the last radius before it, one at the first radius
after it -- and whose structures differ in exactly the fields the transition names (same class, head dimension, variant bits, mask, gradient asked for or not);
the reduce kernel's chain seams and 1024-thread trips, which no
host call reports, are asserted from the kernel's own rule.  Three perturbed restatements -- one clamped diagonal dropped, the table shifted by
one entry, entry n1 - 1 dropped -- leave the bound at the new inputs: a kernel with such a defect could not pass.
"""
import ctypes

import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
import test_attn_bwd_fp64_gpu as W
import test_attn_radius_fp64_gpu as T

CLASSES = {   # name -> (B, H, (M, N) of R): the shape classes of the GPU cases
    "small": (1, 2, lambda R: (100, 130)),            # the problem smaller than the table (from R = 130 on)
    "small3": (3, 2, lambda R: (100, 130)),
    "edge": (1, 2, lambda R: (R + 76, R + 76)),       # the band edge inside the problem on both sides
    "wideN": (3, 2, lambda R: (130, R + 200)),        # one side far only
    "wideM": (1, 2, lambda R: (R + 200, 130)),
    "waves4": (1, 80, lambda R: (100, 130)),          # 160 dK/dV workgroups: four waves per workgroup in the 32-key body
    "fwd384": (1, 96, lambda R: (256, 300)),          # 384 waves of 64 rows: the forward's own rule picks the 64-row body
}
FIELDS = ("fwd", "dq", "dkdv", "fused", "qdiag", "kvres", "launches", "refused")


def _state(lib, p, buf):
    from flasht5_amd import _lib
    _lib.check(lib.fat5_attn_describe(ctypes.byref(p), buf, 256), "fat5_attn_describe")
    d = dict(kv.split("=") for kv in buf.value.decode().split())
    rc = lib.fat5_attn_bwd_stages(ctypes.byref(p), 7, None)   # (no tensors: refused either for the radius or for the null pointers)
    msg = lib.fat5_last_error().decode()
    assert rc == -1 and ("bytes of LDS" in msg or "null tensor pointer" in msg), msg
    d.update(kvres=str(lib.fat5_attn_bwd_kvres(ctypes.byref(p))), launches=str(lib.fat5_attn_bwd_launches(ctypes.byref(p))), refused=str(int("bytes of LDS" in msg)))
    return tuple(d[f] for f in FIELDS)


def params(B, H, M, N, D, R, variant, causal, grad):
    from flasht5_amd import _lib
    p = _lib.AttnParams()
    p.B, p.H, p.M, p.N, p.D = B, H, M, N, D
    p.dtype, p.causal, p.bias_mode, p.rpe_radius, p.variant = _lib.FAT5_BF16, int(causal), _lib.BIAS_RPE1D, R, T.variant_bits(variant)
    p.sm_scale, p.rpe1d, p.drpe1d = float(D) ** -0.5, 16, 16 if grad else 0   # (never followed)
    return p


def scan():
    """[(class, D, variant, causal, grad, R, {field: (before, after)})]: every R in 2 .. 2048 at which a field differs from R - 1"""
    from flasht5_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    out = []
    for cname, (B, H, shape) in CLASSES.items():
        for D in (16, 32, 64, 128):
            for variant in T.VARIANTS:
                if D != 64 and variant in ("sep64", "half64"):   # (bits of bodies that exist at D = 64 only)
                    continue
                for causal in (False, True):
                    for grad in (True, False):
                        p = params(B, H, 1, 1, D, 1, variant, causal, grad)
                        prev = None
                        for R in range(1, 2049):
                            p.M, p.N = shape(R)
                            p.rpe_radius = R
                            now = _state(lib, p, buf)
                            if prev is not None and now != prev:
                                out.append((cname, D, variant, causal, grad, R, {f: (a, b) for f, a, b in zip(FIELDS, prev, now) if a != b}))
                            prev = now
    return out


def _fold(found):
    """{(D, R, changes as text, the variants it occurs with)}: the transitions without the class and the mask (most occur in every class)"""
    out = {}
    for _, D, variant, _, grad, R, ch in found:
        out.setdefault((D, R, " ".join(f"{f}:{a}>{b}" for f, (a, b) in sorted(ch.items()))), set()).add(variant + ("" if grad else "-nograd"))
    return {key + (" ".join(sorted(v)),) for key, v in out.items()}


TRANSITIONS = T.TRANSITIONS


@pytest.fixture(scope="module")
def found():
    from flasht5_amd import _lib
    if _lib.load().fat5_chip_cus() != 256:
        pytest.skip("the table is laid out for the 256 compute units of the MI355X")
    return scan()


def test_the_transitions_are_the_committed_table(found):
    got, want = _fold(found), set(TRANSITIONS)
    for x in sorted(got - want):
        print("[radius] found, not in the table:", x)
    for x in sorted(want - got):
        print("[radius] in the table, not found:", x)
    assert got == want


def test_the_refused_radii_per_head_dimension_and_wave_count(found):
    first = {}
    for cname, D, variant, causal, grad, R, ch in found:
        if "refused" in ch:
            assert ch["refused"] == ("0", "1")   # (never accepted again beyond it)
            first.setdefault((D, "four waves" if cname in ("waves4", "fwd384") else "two waves"), set()).add(R)
    assert {key: sorted(v) for key, v in first.items()} == {key: [R] for key, R in T.FIRST_REFUSED.items()}


def _pairs(D, R, variants):
    """(before, after): cases at R - 1 and R that differ in nothing but the radius (and what follows from it: the shape of the class, the dtype in rotation, the form
    of the bias gradient), at head dimension D, with one of the variants the transition was found with"""
    same = ("shape", "B", "H", "D", "variant", "grad", "causal")
    for a in T.CASES:
        if (a["D"], a["R"]) == (D, R - 1) and a["variant"] + ("" if a["grad"] else "-nograd") in variants.split():
            for b in T.CASES:
                if b["R"] == R and all(a[x] == b[x] for x in same):
                    yield a, b


def test_every_transition_has_a_case_on_either_side():
    """For every row of TRANSITIONS a pair of cases, one at the last radius before it and one at the first radius after it, whose structures differ in EXACTLY the
    fields the row names (a pair that shows more, or less, is another row's), and which run what changed: the forward for `fwd`, the backward (or its refusal) else."""
    for D, R, text, variants in TRANSITIONS:
        ch = dict(x.split(":") for x in text.split())
        want = {f: tuple(v.split(">")) for f, v in ch.items()}
        hits = []
        for a, b in _pairs(D, R, variants):
            sa, sb = T.structure(a), T.structure(b)
            if {f: (sa[f], sb[f]) for f in sa if sa[f] != sb[f]} != want:
                continue
            runs_fwd = a["fwd_check"] and b["fwd_check"]
            runs_bwd = a["bwd"] and (b["bwd"] or b["refused"])
            if ("fwd" not in ch or runs_fwd) and (all(f == "fwd" for f in ch) or runs_bwd) and ("refused" not in ch or runs_fwd):   # (a refused radius: the forward still runs)
                hits.append((a["id"], b["id"]))
        assert hits, f"no pair of cases on either side of {(D, R, text, variants)}"


def test_every_case_names_what_the_library_reports():
    from flasht5_amd import _lib
    if _lib.load().fat5_chip_cus() != 256:
        pytest.skip("the case list is laid out for the 256 compute units of the MI355X")
    for case in T.CASES:
        W.assert_bodies(case, W.describe(case))   # (with the form of the table gradient, which the case claims by itself)
        have, d = T.structure(case), T.reported(case)
        assert have == {f: d[f] for f in have}, case["id"]
        if case["variant"] == "w32":
            assert (have["dq"], have["dkdv"]) == ("32row", "32key"), case["id"]
        if case["variant"] in ("one64", "sep64", "half64") and case["D"] == 64 and case["R"] < 640:
            assert "64" in have["dq"] + have["dkdv"], case["id"]


def test_the_reduce_kernel_seams_and_rounds_are_in_the_case_list():
    """drpe_reduce_kernel (csrc/reduce_kernels.h): 4 / 3 / 2 / 1 interleaved chains by n1 = 2R + 1 <= 256 / 341 / 512 / beyond; one more trip of its 1024 threads per 1024
    entries; more than one round of sixteen partial rows per chain from B nblk > 16 NG on.  Only the cases that reach it count: a bias gradient other than dtable=runs."""
    reach = [c for c in T.CASES if c["bwd"] and not c["refused"] and c["grad"] and c["bodies"].get("dtable") != "runs"]
    radii = {c["R"] for c in reach}
    assert {127, 128, 170, 171, 255, 256, 511, 512, 1024} <= radii
    for form in ("rpe", "scan"):
        assert {T.chains(c["R"]) for c in reach if c["form"] == form} == {1, 2, 3, 4}
        assert {T.trips(c["R"]) for c in reach if c["form"] == form} >= {1, 2, 3}
    rounds = {T.chains(c["R"]) for c in reach if c["B"] * T.part_rows(c) > 16 * T.chains(c["R"])}
    assert rounds == {1, 2, 3, 4}
    assert any(c["R"] == 2048 and c["fwd_check"] for c in T.CASES)   # (n1 = 4097: forward only -- the backward's reduction never sees it at D = 128; at D <= 64 it does)
    for dtype in (T.BF16, T.F16):
        assert {c["R"] for c in T.CASES if c["dtype"] == dtype} >= {128, 256, 512, 1024}


def _far_mask(M, N, pred):
    d = torch.arange(N)[None, :] - torch.arange(M)[:, None]
    return pred(d)


def _perturbations(case):
    R = case["R"]
    drop = lambda pred: (lambda B, H, M, N: (~_far_mask(M, N, pred)).double()[None, None].expand(B, H, M, N))
    return {
        "one clamped diagonal dropped (n - m = R + 1 read as R + 2)": G._set("g_w", lambda c: drop(lambda d: d == R + 1), lambda c: c["rpe"] and c["N"] - 1 >= R + 1),
        "the table shifted by one entry": G._set("shift", 1, lambda c: c["rpe"]),
        "the gradient shifted by one entry": G._set("g_shift", 1, lambda c: c["rpe"]),
        "entry n1 - 1 dropped": G._set("g_w", lambda c: drop(lambda d: d >= R), lambda c: c["rpe"] and c["N"] - 1 >= R),
    }


PERTURBED = [c for c in T.CASES if c["bwd"] and not c["refused"] and c["grad"] and c["perturb"]]


@pytest.mark.parametrize("case", PERTURBED, ids=[c["id"] for c in PERTURBED])
def test_the_perturbed_restatements_leave_the_bound(case):
    t, ref = T.truth(case)
    bound = G.attn_bwd_bound(ref, case["dtype"], case["D"], case["bodies"], case["N"], case["M"])
    outs = W.compared(case, ref)
    applied = 0
    for name, mutant in _perturbations(case).items():
        mut = W.reference(case, t, mutant)
        if not mut["applied"]:
            continue
        applied += 1
        r = G.ratios({x: mut[x] for x in outs}, ref, {x: bound[x] for x in outs})
        print(f"[radius] {case['id']}, {name}: err / bound " + " ".join(f"{x} {r[x]:.3g}" for x in outs))
        assert max(r.values()) > 1.0, (case["id"], name, r)
    assert applied == 2 + (case["N"] - 1 >= case["R"]) + (case["N"] - 1 >= case["R"] + 1), case["id"]   # (the shifts always; the last entry and the first clamped diagonal where keys reach them)
    # ... and the forward with the table shifted by one entry
    if case["fwd_check"]:
        tf = {key: t[key] for key in ("q", "k", "v", "bias", "rpe")}
        fr = F.attn_fwd_ref(tf["q"], tf["k"], tf["v"], case["scale"], case["causal"], None, tf["rpe"], case["R"])
        mu = F.attn_fwd_ref(tf["q"], tf["k"], tf["v"], case["scale"], case["causal"], None, tf["rpe"], case["R"], mutant=F.MUTANTS["rpe index +1"])
        bo, bl = F.attn_fwd_bound(fr, case["dtype"], case["D"], case["fwd"], case["N"])
        ro, rl, _ = F.ratios(mu["o"].to(case["dtype"]), mu["lse"].float(), fr, bo, bl)
        assert max(ro, rl) > 1.0, (case["id"], ro, rl)
