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
  * the bound's shape: 0 on a dead row's dq and above the causal diagonal of dbias, finite everywhere;
  * for the non-dense 64-wide cases: the host restatement of the kernels' step classification (which steps run in pipelined trips: far-positive,
    far-negative, band, on the causal diagonal; which run the general iteration: remainders, key tails, short sweeps) agrees with hand-worked
    examples and finds every kind of step in the case list, per body; `emulate` runs in its 64-wide setting (statistics as accumulator initial
    values, the far bins of the pipelined trips from the rounded dS); and twelve more mutants break what only these bodies have (a trip's last
    step, the remainder, the second pair's half, the hand-over, a key step of the dQ trips, the key tail, the 8-row statistic groups, 1 / scale,
    the far bins, the mirrored diagonal index, the partial rows of a mixed launch).
  * for the dense 64-wide cases (dq=64row-batch4, the DENSE 64-key body, the dense one-launch form): the restatement of split16 on the host agrees with
    hand-checked splits; `steps_qdb64` and the dense setting of `steps_kv64` agree with hand-worked examples and find every kind of step in the case list
    (padded causal trips, a refused padding and row blocks without a step included); `emulate` runs in its dense setting (the bias through the two-term
    selector in fp32, -L through the FMA or as the start value, dbias from the rounded dS summed in fp32); and the mutants of MUTANTS_DENSE64 break what
    only these bodies have (the selector's low term, an idle wave, a slab, a batch element at a group's edge, the key interleave of the dbias store, the
    bias tile's step or row block, the mask of a padded step, the clamp in front of the bias MFMAs).
"""
import functools

import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
import oracle
from test_attn_bwd_fp64_gpu import CASES, inputs, reference, describe, compared

IDS = [c["id"] for c in CASES]
DETECTED = {name: {} for name in list(G.MUTANTS) + list(G.MUTANTS64) + list(G.MUTANTS_DENSE64)}   # mutant -> {case id: caught} over the cases where it applied
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

# The 64-wide cases.  Their far bins are summed from the dS ROUNDED to the dtype, so the bound of a far entry carries u_T times the magnitudes of
# all its terms -- tens of thousands, of both signs, whose true sum is of the order of their square root.
_FAR_BIN = ("a far bin of the 64-wide bodies: the bound is u_T times the summed magnitudes of all the bin's terms (the pipelined trips sum the rounded dS), and "
            "what the defect adds or leaves out is a partial sum of the same terms of both signs, below that; the same defect is caught on the smaller bins of the group's other cases")
_FAR_CASES = {
    "a far bin with the band's blocks added": (
        "kv64h-1x2x256x256-float16-rpe64-s0.3",
        "kv64-2x2x129x64-float16-rpe8-s1.0-strided",
        "kv64-1x2x255x256-bfloat16-rpe8-s0.125-pert",
        "kv64-2x2x257x257-float16-rpe1-s1.0",
        "kv64-2x2x127x520-float16-rpe128-s0.125-strided",
        "kv64-1x2x255x257-float16-rpe8-s0.125",
        "kv64-2x2x384x384-float16-t5b8-s0.3-runs",
        "kv64-1x2x385x520-bfloat16-t5u128-s1.0-scan",
        "kv64h-1x2x415x300-bfloat16-rpe8-s0.3-strided",
        "kv64m-4x4x140x384-float16-t5b128-s0.3-scan",
        "kv64m-3x8x130x520-float16-t5u8-s1.0-scan",
        "kv64m-2x8x160x300-bfloat16-rpe8-s0.3",
        "sep64-1x2x257x300-bfloat16-rpe8-s0.3",
        "fused64-2x2x129x385-float16-rpe8-s1.0-plain",
        "fused64-1x4x512x512-bfloat16-t5b128-s1.0-runs-plain",
        "fused64-1x2x300x520-float16-rpe128-s0.3-stages",
        "qdiag-1x2x384x384-bfloat16-rpe8-s0.125-qd1",
        "qdiag-1x2x384x384-bfloat16-rpe8-s0.125-qd0",
        "qdiag-3x2x257x300-float16-t5b8-s1.0-runs-qd1",
        "qdiag-3x2x257x300-float16-t5b8-s1.0-runs-qd0",
        "qdiag-1x2x300x385-bfloat16-t5u128-s0.3-scan-qd1",
        "qdiag-1x2x300x385-bfloat16-t5u128-s0.3-scan-qd0",
        "qdiag-3x2x129x257-float16-t5b128-s0.125-stages-scan-qd1",
        "qdiag-3x2x129x257-float16-t5b128-s0.125-stages-scan-qd0",
        "qdiag-1x2x385x257-bfloat16-t5u8-s1.0-runs-qd1",
        "qdiag-1x2x385x257-bfloat16-t5u8-s1.0-runs-qd0",
        "causal64-fused64-1x2x284x384-bfloat16-rpe8-s0.125-causal",
    ),
    "a far bin without one pipelined step's block": (
        "kv64-1x2x256x65-bfloat16-rpe1-s0.3",
        "kv64-1x2x255x256-bfloat16-rpe8-s0.125-pert",
        "kv64-2x2x257x257-float16-rpe1-s1.0",
        "kv64-2x2x127x520-float16-rpe128-s0.125-strided",
        "kv64-1x2x385x128-float16-rpe8-s0.3",
        "kv64-1x2x384x384-bfloat16-rpe8-s0.125",
        "kv64-2x2x384x384-float16-t5b8-s0.3-runs",
        "kv64-1x2x385x520-bfloat16-t5u128-s1.0-scan",
        "kv64h-1x2x415x300-bfloat16-rpe8-s0.3-strided",
        "kv64h-1x2x544x130-bfloat16-t5b8-s1.0-runs",
        "kv64h-1x2x385x384-bfloat16-rpe128-s0.125-causal",
        "kv64m-4x4x140x384-float16-t5b128-s0.3-scan",
        "kv64m-3x8x130x520-float16-t5u8-s1.0-scan",
        "kv64m-2x8x160x300-bfloat16-rpe8-s0.3",
        "sep64-1x2x257x300-bfloat16-rpe8-s0.3",
        "sep64-1x2x300x385-float16-t5b8-s1.0-scan",
        "fused64-2x2x129x385-float16-rpe8-s1.0-plain",
        "fused64-1x2x384x384-float16-rpe1-s0.3-pert-plain",
        "fused64-1x4x512x512-bfloat16-t5b128-s1.0-runs-plain",
        "fused64-1x2x300x520-float16-rpe128-s0.3-stages",
        "qdiag-1x2x384x384-bfloat16-rpe8-s0.125-qd1",
        "qdiag-1x2x384x384-bfloat16-rpe8-s0.125-qd0",
        "qdiag-3x2x257x300-float16-t5b8-s1.0-runs-qd1",
        "qdiag-3x2x257x300-float16-t5b8-s1.0-runs-qd0",
        "qdiag-1x2x300x385-bfloat16-t5u128-s0.3-scan-qd1",
        "qdiag-1x2x300x385-bfloat16-t5u128-s0.3-scan-qd0",
        "qdiag-1x2x385x257-bfloat16-t5u8-s1.0-runs-qd1",
        "qdiag-1x2x385x257-bfloat16-t5u8-s1.0-runs-qd0",
        "causal64-kv64-1x2x357x257-bfloat16-rpe128-s0.125-causal",
        "causal64-kv64-1x2x284x384-bfloat16-rpe8-s1.0-causal",
        "causal64-kv64-1x2x512x512-float16-rpe128-s0.3-causal",
        "causal64-fused64-1x2x257x257-bfloat16-rpe8-s1.0-causal",
        "causal64-fused64-1x2x258x257-float16-rpe8-s1.0-causal-pert",
        "causal64-fused64-1x2x284x384-bfloat16-rpe8-s0.125-causal",
        "causal64-fused64-1x2x512x512-float16-rpe128-s1.0-causal",
    ),
    "drpe1d far entries without what lies beyond the band": (
        "kv64-2x2x127x520-float16-rpe128-s0.125-strided",
        "kv64-2x2x384x384-float16-t5b8-s0.3-runs",
        "kv64-1x2x385x520-bfloat16-t5u128-s1.0-scan",
        "kv64h-1x2x544x130-bfloat16-t5b8-s1.0-runs",
        "kv64h-1x2x385x384-bfloat16-rpe128-s0.125-causal",
        "q64-2x2x300x384-bfloat16-t5b8-s0.3-runs",
        "fused64-1x4x512x512-bfloat16-t5b128-s1.0-runs-plain",
        "qdiag-1x2x384x384-bfloat16-rpe8-s0.125-qd1",
        "qdiag-1x2x384x384-bfloat16-rpe8-s0.125-qd0",
        "qdiag-1x2x385x257-bfloat16-t5u8-s1.0-runs-qd1",
        "causal64-kv64-1x2x512x512-float16-rpe128-s0.3-causal",
    ),
}
EXCUSED.update({(m, cid): _FAR_BIN for m, ids in _FAR_CASES.items() for cid in ids})
_ALL_FAR = "N - M = -100 at R = 8: every visible score lies beyond -R, the clamped index does not move and the result is the reference's own (ratio 0)"
EXCUSED[("drpe1d diagonal index +1", "causal64-q64-1x2x357x257-float16-rpe8-s1.0-causal-pert")] = _ALL_FAR
EXCUSED[("drpe1d diagonal index -1", "causal64-q64-1x2x357x257-float16-rpe8-s1.0-causal-pert")] = _ALL_FAR
_LAST_KEY = "key N - 1 is visible to the last row alone, with p = 8.5e-4 there: the dropped term is 0.92 of that row's bound"
EXCUSED[("dQ without key N-1", "causal64-kv64-1x2x257x357-bfloat16-none-s1.0-causal")] = _LAST_KEY
EXCUSED[("dQ without the last key of a ragged last tile", "causal64-kv64-1x2x257x357-bfloat16-none-s1.0-causal")] = _LAST_KEY


def _rpe(case):
    return case["bias"] != "none" and case["bias"][:2] not in ("11", "1h", "b1", "bh")


def _layout(case):
    """what the mutants of the 64-wide bodies need of a case: its bodies and their step walks"""
    return dict(bodies=case["bodies"], walks=G.layout_of(case["bodies"], case["M"], case["N"], case["R"], case["causal"], _rpe(case) and not case["dense64"]), B=case["B"], H=case["H"],
                M=case["M"], N=case["N"], R=case["R"], drpe=_rpe(case))


def _mutants(case):
    muts = dict(G.MUTANTS)
    if case["wide"]:
        lay = _layout(case)
        for name, make in G.MUTANTS64.items():
            m = make(lay)
            if m is not None:
                muts[name] = m
    if case["dense64"]:
        lay = _layout(case)
        for name, make in G.MUTANTS_DENSE64.items():
            m = make(lay)
            if m is not None:
                muts[name] = m
    return muts


@functools.lru_cache(maxsize=2)
def _truth(i):
    case = CASES[i]
    t = inputs(case)
    ref = reference(case, t)
    return t, ref, G.attn_bwd_bound(ref, case["dtype"], case["D"], case["bodies"], case["N"], case["M"])


def test_the_case_list_is_what_the_issue_asks_for():
    def of(group, key):
        return {c[key] for c in CASES if c["group"] == group}
    OLD = ("w2", "w4", "causal", "t5", "dbias", "pert", "fused32")
    assert {c["bodies"]["dq"] for c in CASES if c["group"] in OLD} == {"32row"} and {c["bodies"]["dkdv"] for c in CASES if c["group"] in OLD} == {"32key"}
    assert sum(c["group"] in OLD for c in CASES) == 63 and all(c["wide"] == (c["group"] not in OLD) for c in CASES if not c["dense64"])
    assert sum(not c["dense64"] for c in CASES) == 151
    _the_64_wide_groups(of)
    _the_dense_64_wide_groups(of)
    assert {1, 31, 32, 33, 64, 65, 129} <= of("w2", "M") and {1, 63, 64, 65, 127, 128, 129, 200} <= of("w2", "N")
    assert of("w2", "D") == {16, 32, 64, 128} and {1, 8, 128} <= of("w2", "R")
    assert {"none", "rpe", "11", "1h", "b1", "bh"} <= of("w2", "bias") | of("causal", "bias")
    for c in (c for c in CASES if c["group"] in OLD):
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


def _the_dense_64_wide_groups(of):
    """the dense 64-wide groups: batch groups, rows, keys, causal sweeps, the workgroup decode, scales, bias kinds, forms -- and by the host restatement of both
    bodies' step loops every kind of step"""
    X = [c for c in CASES if c["dense64"]]
    Q = [c for c in X if c["bodies"]["dq"] == "64row-batch4"]
    K = [c for c in X if c["bodies"]["dq"] == "32row"]
    assert 0 < len(X) <= 80 and all(c["D"] == 64 and c["N"] % 8 == 0 and c["B"] * c["H"] * c["M"] * c["N"] <= 2 ** 20 for c in X)
    assert {c["group"] for c in X} == {"qdb", "qdbkv", "dfused", "dplain", "dkv64", "dcausal"}
    for g, dq, kv, fused in (("qdb", "64row-batch4", "32key", "0"), ("qdbkv", "64row-batch4", "64key", "0"), ("dfused", "64row-batch4", "64key", "1"),
                             ("dplain", "64row-batch4", "64key", "1"), ("dkv64", "32row", "64key", "0")):
        assert {(c["bodies"]["dq"], c["bodies"]["dkdv"], c["bodies"]["fused"]) for c in X if c["group"] == g} == {(dq, kv, fused)}, g
    assert all(c["bodies"]["dbias"] == ("dq-kernel" if c["B"] <= 4 else "dq-kernel+partials") for c in Q)
    assert {c["bodies"]["dbias"] for c in K} == set(G.DBIAS_ROUTES) and {c["bias"][:2] for c in K} == {"1h", "bh", "11", "b1"}
    assert {c["B"] for c in Q} >= {1, 2, 3, 4, 5, 6, 8, 9}
    assert {c["M"] for c in Q} >= {1, 63, 64, 65, 130} and {c["N"] for c in Q} >= {8, 24, 32, 40, 128, 136, 160, 264}
    assert {c["M"] for c in K} >= {90, 128, 160, 300} and {c["N"] for c in K} >= {64, 72, 256, 264, 520}
    for cs, name in ((Q, "qdb"), (K, "dkv64")):
        assert {c["N"] - c["M"] for c in cs if c["causal"]} >= {0, 1, 100, -1, -100}, name
    for part in (False, True):   # the final tensor and the slabs, for P > 0 and P < 0
        ps = {(c["N"] > c["M"]) - (c["N"] < c["M"]) for c in Q if c["causal"] and (c["B"] > 4) == part}
        assert ps >= {1, -1}, part
    assert any(c["causal"] and c["M"] == c["N"] == 256 for c in Q) and any(c["causal"] and c["M"] == c["N"] == 248 for c in Q)
    wg = lambda c: c["H"] * ((c["B"] + 3) // 4) * ((c["M"] + 63) // 64)
    assert any(wg(c) > 8 and wg(c) % 8 for c in Q) and any(wg(c) < 8 for c in Q)
    assert any(c["causal"] and (c["H"] * ((c["B"] + 3) // 4)) % 8 == 0 for c in Q) and any(c["causal"] and (c["H"] * ((c["B"] + 3) // 4)) % 8 for c in Q)
    assert {c["scale"] for c in X} == {0.125, 1.0, -0.5, 0.3, 1.3, 0.0884, -0.3}
    for c in X:   # ONE exactly where 1 / scale is a single 16-bit term
        assert G.split16_of(c["scale"], c["dtype"])["one"] == (c["scale"] in (0.125, 1.0, -0.5)), c["id"]
    for cs in (Q, K):
        assert {c["dtype"] for c in cs} == {torch.bfloat16, torch.float16} and {c["scale"] for c in cs} >= {0.125, 1.0, -0.5, 0.3, 1.3, 0.0884, -0.3}
    kinds = {c["bias"] for c in Q}
    assert kinds >= {"1h", "1h-min", "1h-inf", "1h-big", "1h-view"} and {c["bias"] for c in K} >= {"1h-min", "1h-inf", "1h-big"}
    assert all(c["dtype"] == torch.bfloat16 and not G.split16_of(c["scale"], c["dtype"])["one"] for c in X if c["bias"].endswith("-big"))
    assert any(c["causal"] and c["bias"].endswith("-inf") for c in Q)
    F1 = [c for c in X if c["bodies"]["fused"] == "1"]
    assert any((c["B"] * c["H"] * ((c["N"] + 255) // 256)) % 8 for c in F1) and any((c["B"] * c["H"] * ((c["N"] + 255) // 256)) % 8 == 0 for c in F1)
    plain = [c for c in X if not c["bits"]]
    assert len(plain) >= 2 and all(c["bodies"]["fused"] == "1" for c in plain) and any((c["B"], c["H"], c["M"], c["N"]) == (2, 8, 128, 128) for c in plain)
    assert sum(c["pert"] for c in X) >= 6 and any(c["pert"] for c in F1) and sum(c["split"] for c in X) >= 4 and sum(c["strided"] for c in X) >= 4
    # every kind of step, per body
    kq, kk = set(), set()
    for c in X:
        lay = G.layout_of(c["bodies"], c["M"], c["N"], 0, c["causal"], False)
        if lay["qdb"] is not None:
            kq |= G.kinds_of_qdb(lay["qdb"])
        if lay["kv"] is not None:
            kk |= G.kinds_of(lay["kv"])
    assert kq == set(G.KINDS_QDB), set(G.KINDS_QDB) - kq
    want = {"far-negative trip", "causal-diagonal trip", "general step", "remainder behind the last trip", "fewer steps than ring slots", "key-tail wave"}
    assert kk == want, (want - kk, kk - want)   # (without a table the all-visible trips carry the name of the far-negative ones)
    from test_attn_bwd_fp64_gpu import seams_dense64
    for c in X:
        rows, keys = seams_dense64(c)
        assert set(range(0, c["M"], 64)) <= set(rows) and set(range(0, c["N"], 128)) <= set(keys) and set(range(0, c["N"], 256)) <= set(keys)
        assert set(range(0, c["M"], 32)) <= set(rows) and set(range(0, c["N"], 32)) <= set(keys)


def _the_64_wide_groups(of):
    """the non-dense 64-wide groups: shapes, forms and -- by the host restatement of the kernels' step classification -- every kind of step"""
    W = [c for c in CASES if c["wide"]]
    assert all(c["D"] == 64 and c["B"] * c["H"] * c["M"] * c["N"] <= 2 ** 22 and c["bias"] in ("none", "rpe", "t5b", "t5u") for c in W)
    assert {90, 127, 128, 129, 255, 256, 257, 300, 385} <= of("kv64", "M") and {63, 64, 65, 128, 192, 255, 256, 257, 300, 520} <= of("kv64", "N")
    assert {0, 1, 8, 128} <= of("kv64", "R") and any(c["M"] == c["N"] == 384 and c["R"] == 8 for c in W if c["group"] == "kv64")
    assert {63, 64, 65, 128, 255, 256, 257} <= of("q64", "M") and {90, 127, 128, 129, 256, 300, 385} <= of("q64", "N")
    for g, dq, kv in (("kv64", "32row", "64key"), ("kv64h", "32row", "64key-half"), ("q64", "64row", "32key"), ("fused64", "64row", "64key"), ("qdiag", "64row", "64key")):
        assert {(c["bodies"]["dq"], c["bodies"]["dkdv"]) for c in W if c["group"] == g} == {(dq, kv)}, g
    for c in W:
        if c["group"] == "kv64m":
            assert c["bodies"]["dkdv"].startswith("64key-mixed:") and (c["B"] * c["H"]) % 8 == 0 and c["B"] * c["H"] >= 16
        assert (c["bodies"]["fused"] == "1") == (c["group"] in ("fused64", "qdiag") or "-fused64-" in c["id"]), c["id"]
    assert {c["N"] for c in W if c["group"] == "kv64m"} >= {300, 384, 520}
    assert {c["bodies"].get("dtable") for c in W if c["group"] == "kv64m"} >= {"runs", "scan"}
    assert any(((c["M"] + 31) // 32) % 2 == 1 for c in W if c["group"] == "kv64h") and any((c["M"] + 31) // 32 < 8 for c in W if c["group"] == "kv64h")
    plain = [c for c in W if c["group"] == "fused64" and not c["bits"]]
    assert len(plain) >= 4 and all(c["bodies"]["fused"] == "1" for c in plain)
    assert any(c["bodies"]["qdiag"] == "1" and c["bodies"].get("dtable") == "runs" and c["bias"] == "t5b" and c["M"] == c["N"] == 512 and c["R"] == 128 for c in plain)
    qd = [c for c in W if c["group"] == "qdiag"]
    assert {c["B"] for c in qd} >= {1, 3} and {c["bias"] for c in qd} >= {"rpe", "t5b", "t5u"} and {c["bodies"].get("dtable") for c in qd} >= {None, "runs", "scan"}
    for c in qd:   # ON and OFF on the same inputs
        twin = [x for x in qd if x is not c and all(x[key] == c[key] for key in ("B", "H", "M", "N", "bias", "R", "dtype", "scale"))]
        assert len(twin) == 1 and {twin[0]["bodies"]["qdiag"], c["bodies"]["qdiag"]} == {"0", "1"}
    for form in ("-kv64-", "-q64-", "-fused64-"):
        cs = [c for c in W if c["group"] == "causal64" and form in c["id"]]
        assert all(c["causal"] for c in cs) and {c["N"] - c["M"] for c in cs} >= {0, 1, 100, -1, -100}
        assert any(c["bias"] == "none" for c in cs) and any(c["bias"] == "rpe" and -c["R"] <= c["N"] - c["M"] < c["R"] for c in cs)
        assert any(c["bias"] == "rpe" and c["R"] == 8 and c["N"] - c["M"] == 100 for c in cs)
    assert sum(c["scale"] == 0.3 for c in W) >= 6 and sum(c["scale"] == 1.0 for c in W) >= 6 and {c["scale"] for c in W} == {0.125, 1.0, 0.3}
    for g in ("kv64", "kv64h", "kv64m", "q64", "sep64", "fused64", "qdiag", "causal64"):
        assert of(g, "dtype") == {torch.bfloat16, torch.float16}, g
        assert {c["scale"] for c in W if c["group"] == g} >= {0.3}, g
    assert sum(c["pert"] for c in W) >= 4 and sum(c["split"] for c in W) >= 4 and sum(c["strided"] for c in W) >= 6
    assert any(c["pert"] and c["bodies"]["fused"] == "1" for c in W)   # (the SELF form follows the stored o, lse)
    # every kind of step, per body: over all the cases that run it, and -- but for the causal diagonal, which only a causal case has -- inside its own group
    kinds = {}
    for c in W:
        lay = G.layout_of(c["bodies"], c["M"], c["N"], c["R"], c["causal"], c["bias"] != "none")
        for body in ("kv", "kvh", "q"):
            if lay[body] is not None:
                for key in (body, (body, c["group"])):
                    kinds.setdefault(key, set()).update(G.kinds_of(lay[body]))
    for body in ("kv", "kvh", "q"):
        assert kinds[body] == set(G.KINDS), (body, set(G.KINDS) - kinds[body])
    for key in (("kv", "kv64"), ("kvh", "kv64h"), ("q", "q64"), ("kv", "fused64"), ("q", "fused64")):
        assert kinds[key] >= set(G.KINDS) - ({"causal-diagonal trip"} if key != ("kvh", "kv64h") else set()), (key, set(G.KINDS) - kinds[key])
    for body in ("kv", "q"):
        assert "causal-diagonal trip" in kinds[(body, "causal64")] and "general step" in kinds[(body, "causal64")]
    # the boosted seams: every wave's first key, every trip's first row, the first step behind the last aligned trip, the second pair's first step
    from test_attn_bwd_fp64_gpu import seams64
    for c in W:
        rows, keys = seams64(c)
        nst = (c["M"] + 31) // 32
        assert set(range(0, c["N"], 64)) <= set(keys) and set(range(0, c["M"], 128)) <= set(rows)
        assert all(r in rows for r in ((nst - nst % 4) * 32, (nst + 1) // 2 * 32) if r < c["M"])


def test_the_bound_raises_for_impossible_bodies_and_returns_for_the_dense_64_wide_ones():
    i = next(i for i, c in enumerate(CASES) if c["group"] == "dbias" and c["D"] == 64)
    case, (t, ref, _) = CASES[i], _truth(i)
    for bodies, D in ((dict(dq="32row", dkdv="32key", fused="0", qdiag="0", dbias="dq-kernel"), 64), (dict(dq="32row", dkdv="64key", fused="0", qdiag="0", dbias="dq-kernel+partials"), 64),
                      (dict(dq="64row-batch4", dkdv="64key", fused="1", qdiag="0", dbias="staged"), 64), (dict(dq="32row", dkdv="64key", fused="0", qdiag="0", dbias="somewhere"), 64),
                      (dict(dq="64row-batch4", dkdv="64key", fused="1", qdiag="1", dbias="dq-kernel"), 64), (dict(dq="32row", dkdv="64key", fused="0", qdiag="1", dbias="staged"), 64),
                      (dict(dq="64row-batch4", dkdv="32key", fused="0", qdiag="0", dbias="dq-kernel"), 128), (dict(dq="32row", dkdv="64key", fused="0", qdiag="0", dbias="staged"), 32),
                      (dict(dq="64row", dkdv="64key", fused="1", qdiag="0", dbias="staged"), 64), (dict(dq="32row", dkdv="64key-half", fused="0", qdiag="0", dbias="staged"), 64),
                      (dict(dq="64row-batch4", dkdv="32key", fused="1", qdiag="0", dbias="dq-kernel"), 64)):
        with pytest.raises(NotImplementedError):
            G.attn_bwd_bound(ref, case["dtype"], D, bodies, case["N"], case["M"])
    for bodies in (dict(dq="64row-batch4", dkdv="32key", fused="0", qdiag="0", dbias="dq-kernel"), dict(dq="64row-batch4", dkdv="64key", fused="0", qdiag="0", dbias="dq-kernel+partials"),
                   dict(dq="64row-batch4", dkdv="64key", fused="1", qdiag="0", dbias="dq-kernel"), dict(dq="32row", dkdv="64key", fused="0", qdiag="0", dbias="staged")):
        b = G.attn_bwd_bound(ref, case["dtype"], 64, bodies, case["N"], case["M"])
        assert sorted(b) == ["dbias", "dk", "dq", "dv"] and all(bool(torch.isfinite(x).all()) for x in b.values())


def test_the_selector_split_restates_split16():
    """hand-checked: 1 / 0.125 = 8 and 1 / -0.5 = -2 are one term; 1 / 0.3 in bf16 truncates to 3.328125 + 0.005187988..., in fp16 rounds to 3.333984375 - 0.00065088..."""
    for dt_ in (torch.bfloat16, torch.float16):
        for sc in (0.125, 1.0, -0.5):
            s = G.split16_of(sc, dt_)
            assert s["one"] and s["rel"] == 0.0 and s["hi"] == 1.0 / sc
    s = G.split16_of(0.3, torch.bfloat16)
    assert s["hi"] == 3.328125 and 0 < s["lo"] < 2.0 ** -7 and not s["one"] and 0 < s["rel"] < 2.0 ** -14
    assert s["hi"] == float(torch.tensor(s["hi"]).bfloat16()) and s["lo"] == float(torch.tensor(s["lo"]).bfloat16())
    s = G.split16_of(0.3, torch.float16)
    assert s["hi"] == float(torch.tensor(1 / 0.3).half()) and s["lo"] == float(torch.tensor(s["invf"] - s["hi"]).half()) and s["rel"] < 2.0 ** -21
    for sc in (0.3, 1.3, 0.0884, -0.3):
        assert 2.0 ** -18 < G.split16_of(sc, torch.bfloat16)["rel"] < 2.0 ** -14, sc
    assert G.bias_clamp_limit(0.3, torch.bfloat16) == float(torch.tensor(-2.0e38 * 0.3).view(torch.int32).bitwise_and(-65536).view(torch.float32))
    assert G.bias_clamp_limit(1.3, torch.bfloat16) < -1.99e38 and G.bias_clamp_limit(1.3, torch.float16) == -65504.0


def test_the_step_classification_on_hand_worked_examples():
    """M = N = 384, R = 8, the dK/dV body (one 256-key workgroup + one of 128 live keys): the wave at keys 192.. sees rows 0..127 far to its left (far-positive) and the rest across
    the band (key 255 is only 1 above row 256), the wave at keys 0.. rows 128.. far-negative: one workgroup holds all three kinds of trip"""
    w = {x["kw0"]: [k for _, k in x["segs"]] for x in G.steps_kv64(384, 384, 8, False, True)}
    assert w[192] == ["far+", "band", "band"] and w[64] == ["band", "band", "far-"] and w[0] == ["band", "far-", "far-"] and w[320] == ["far+", "far+", "band"]
    # 90 rows: three steps, fewer than the ring has slots -- all general; 65 keys: the second wave has a key tail and stays general
    assert all(k == "general" for x in G.steps_kv64(90, 128, 0, False, False) for _, k in x["segs"])
    w = {x["kw0"]: [k for _, k in x["segs"]] for x in G.steps_kv64(128, 65, 0, False, False)}
    assert w[0] == ["far-"] and w[64] == ["general"] * 4
    # no bias, causal, M = N = 256: the wave at keys 64.. has its diagonal in the first trip (mask in the C operand), then sees everything
    w = {x["kw0"]: [k for _, k in x["segs"]] for x in G.steps_kv64(256, 256, 0, True, False)}
    assert w[64] == ["diag", "far-"] and w[0] == ["diag", "far-"]
    # the dQ body, M = 64, N = 300, no bias: two trips, one whole general step, one with a key tail
    (x,) = G.steps_q64(64, 300, 0, False, False)
    assert [k for _, k in x["segs"]] == ["far-", "far-", "general", "general"] and x["tail"]
    # half-length form, 9 steps: the pairs walk 5 and 4 (+ 1 empty) steps
    hs = [(x["pair"], x["mt0"], x["ns"]) for x in G.steps_kv64(288, 128, 0, False, False, half=True) if x["kw0"] == 0]
    assert hs == [(0, 0, 5), (1, 5, 5)]
    # ---- the dQ + dBias body (one walk per 64-row block) ----
    kinds = lambda b: [k for _, k in b["segs"]]
    # N = 264, not causal: two trips and a 8-key tail step; N = 160: one trip and one whole general step; N = 24: one partial step
    (b,) = G.steps_qdb64(64, 264, False)
    assert kinds(b) == ["trip", "trip", "general"] and b["tail"] and b["nt"] == 9 and not b["padded"]
    (b,) = G.steps_qdb64(1, 160, False)
    assert kinds(b) == ["trip", "general"] and not b["tail"]
    (b,) = G.steps_qdb64(63, 24, False)
    assert kinds(b) == ["general"] and b["tail"]
    # causal, M = N = 256: block 0 sees 64 keys = 2 steps, padded to one trip of 4 (128 <= 256), all of it on or above the diagonal: masked;
    # block 1: 4 steps, masked; block 2: 6 steps padded to 8 (256 <= 256), both trips masked -- an iteration forms the scores of the NEXT step, so a trip is
    # unmasked only if step t + 4 is visible to all 64 rows (q:681), and keys 128..159 are not to row 128; block 3: 8 steps, keys ..159 lie below row 192
    bs = G.steps_qdb64(256, 256, True)
    assert [(b["nt0"], b["nt"], b["padded"]) for b in bs] == [(2, 4, True), (4, 4, False), (6, 8, True), (8, 8, False)]
    assert [kinds(b) for b in bs] == [["mtrip"], ["mtrip"], ["mtrip", "mtrip"], ["trip", "mtrip"]]
    # ... M = N = 248: block 2 would need 8 steps = 256 keys > 248: refused, its steps 4 and 5 run the general iteration; block 3 (rows 192..247) sees all 248 keys:
    # 8 steps, the last a key tail, so the second trip is not whole: four general steps
    bs = G.steps_qdb64(248, 248, True)
    assert [(b["nt0"], b["nt"], b["refused"]) for b in bs] == [(2, 4, False), (4, 4, False), (6, 6, True), (8, 8, False)]
    assert kinds(bs[2]) == ["mtrip", "general", "general"] and kinds(bs[3]) == ["trip"] + ["general"] * 4 and bs[3]["tail"]
    # M = 300, N = 40, causal (P = -260): rows 0..259 are dead; blocks 0..3 end at keys <= 0: no step; block 4 (rows 256..299) sees 40 keys: two steps, the second a tail
    bs = G.steps_qdb64(300, 40, True)
    assert [b["nt"] for b in bs] == [0, 0, 0, 0, 2] and kinds(bs[4]) == ["general", "general"] and bs[4]["tail"] and bs[4]["refused"]
    # ---- the DENSE 64-key body: the loop of the bodies without a table ----
    w = {x["kw0"]: [k for _, k in x["segs"]] for x in G.steps_kv64(256, 264, 0, False, False, dense=True)}
    assert w[0] == ["far-", "far-"] and w[192] == ["far-", "far-"] and w[256] == ["general"] * 8   # (the second workgroup's 8 keys: a key-tail wave)
    w = {x["kw0"]: [k for _, k in x["segs"]] for x in G.steps_kv64(256, 256, 0, True, False, dense=True)}
    assert w[0] == ["diag", "far-"] and w[128] == ["diag", "diag"]   # (the workgroup's waves share its first row: keys 128.. stay on the diagonal)
    with pytest.raises(AssertionError):
        G.steps_kv64(256, 256, 0, False, False, half=True, dense=True)


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
    kw = {}
    if case["wide"]:   # the 64-wide setting: the statistics as accumulator initial values, the far bins of the pipelined trips from the rounded dS
        kw["stats"] = "self" if case["bodies"]["fused"] == "1" else "stat2"
        if t["rpe"] is not None:
            kw["rounded_sums"] = G.far_rounded_mask(case["bodies"], case["M"], case["N"], case["R"], case["causal"])
    if case["dense64"]:   # the dense 64-wide setting: the bias through the two-term selector, -L through the FMA (dQ + dBias) / as the start value (64-key)
        kw["dense64"] = (("q",) if case["bodies"]["dq"] == "64row-batch4" else ()) + (("kv",) if case["bodies"]["dkdv"] == "64key" else ())
    emu = G.emulate(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], case["scale"], case["causal"], t["bias"], t["rpe"], case["R"], t["bucket"],
                    32 if t["bucket"] is not None else 0, case["bodies"].get("dbias", "direct"), **kw)
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
    for name, mutant in _mutants(case).items():
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
