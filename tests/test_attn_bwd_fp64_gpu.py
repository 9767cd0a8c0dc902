"""The attention backward per element of dq, dk, dv, dbias, drpe1d and the T5 table gradient against the fp64 restatement and the derived
bound of tests/attn_bwd_fp64.py: the FA2 backward from a GIVEN (o, lse).  The test fills `plan.o` and `plan.lse` of an AttentionPlan
itself -- no forward launch is involved -- so delta = rowsum(o do) is formed from the same numbers on both sides, and the bound is in
units of each element's own term magnitudes: no tensor maximum, no max(1, .).

Covered (csrc/attn_bwd.h): the 32-wide bodies dq=32row, dkdv=32key at D = 16 / 32 / 64 / 128, both wave counts, as separate launches
(groups w2, w4, causal, t5, dbias, pert) and in the one-launch form (group fused32); dense dbias by the routes direct, staged and inkernel
(with its fp32 scratch at B = 5, and unsplit); drpe1d; the table gradient as dtable=runs and dtable=scan, bidirectional and
unidirectional maps.  Shapes are the smallest at which the structure exists: rows and keys around every 32 / 64 / 128 boundary, radius
1 / 8 / 128, bottom-right causal masks with N - M in {0, 1, 100, -1, -100} (dead rows included), dense biases of every broadcast kind and
one holding finfo.min.  "Perturbed" cases shift lse by 0.25 on every third row and replace o by an unrelated tensor: the contract is
"from the stored o, lse", and a kernel that recomputed either would leave the bound.  Some cases call the stages one by one.
Covered (csrc/attn_bwd64.h, D = 64, bias none / rpe1d / T5 table): the non-dense 64-wide bodies.  Groups kv64 (dkdv=64key beside the 32-row dQ kernel,
whose statistics it starts from), kv64h (64key-half: two wave pairs, each half of the steps, and the hand-over), kv64m (64key-mixed: both in one
launch), q64 (dq=64row beside the 32-key body), sep64 (both 64-wide bodies as two launches), fused64 (one launch, the dK/dV half on statistics of
its own; five cases carry NO variant bit -- the path a plain call takes --, one of them the benchmark's configuration at B = 1, H = 4 with qdiag=1
dtable=runs), qdiag (V_QDIAG_ON and V_QDIAG_OFF on the same inputs) and causal64 (each form at N - M in {0, 1, 100, -1, -100}, without bias, with
the table inside the band, with a table far from the diagonal).  sm_scale is 0.125, 1.0 or 0.3 (no exact reciprocal); q is scaled so that the
scores spread alike.  Shapes sit around the trip (128 rows), ring (4 steps), wave (64 keys) and workgroup (128 / 256 keys, 256 rows) boundaries;
tests/test_attn_bwd_fp64_cpu.py asserts with the host restatement of the kernels' step classification that every kind of step occurs.
Covered (csrc/attn_bwd_qdb64.h and the DENSE form of the 64-key body of csrc/attn_bwd64.h, D = 64, a dense bias): groups qdb (dq=64row-batch4 beside the 32-key body:
B = 1 .. 9 -- three, two, one and no idle waves, two and three fp32 slabs --, rows 1 .. 130, keys 8 .. 264 around the step (32) and trip (128) boundaries, the
eight-chunk workgroup cut with a remainder), qdbkv (both dense bodies as two launches), dfused (one launch behind bwd_stat2_kernel, the dK/dV workgroup count
mostly no multiple of eight), dplain (NO variant bit: what a plain model call takes, (2, 8, 128, 128) among them), dkv64 (the DENSE 64-key body beside the 32-row dQ
kernel: bias kinds 1h / bh / 11 / b1, dbias routes direct / staged / inkernel) and dcausal (each form at N - M in {0, 1, 100, -1, -100}; M = N = 256 with padded
sweeps, 248 with the padding refused, M >> N with row blocks that have no step; the final tensor and the slabs).  sm_scale rotates through 0.125, 1.0, -0.5 (one
selector term) and 0.3, 1.3, 0.0884, -0.3 (two).  Bias kinds beyond the plain one: -min (finfo.min on half the keys and on whole rows), -inf (the same written as
-inf, single entries included), -big (|bias| up to 64 through a two-term bf16 selector: the cases on which the selector's residual term of the bound is largest) and -view (a
(1, H, M, N) view of a tensor with row pitch N + 64, whose padding must stay untouched).  These cases fill the workspace with 0xFF bytes before every run, so the
statistics and the fp32 slabs hold NaN wherever the call does not write.

The value rows at key 0, N - 1 and the block seam and the `do` rows 0, M - 1 and the first rows of the last 32- / 64-row blocks carry 32
times the others' magnitude -- in the 64-wide cases also the keys at every wave start (64 w: the 128- and 256-key block starts among them) and the
rows at every trip start (multiples of 128), at the first step behind the last aligned trip and at the first step of the second pair's half; in the dense
64-wide cases every step start (multiples of 32 rows and keys: the 64-row blocks, the 128-key trips and the 256-key workgroups among them) and row 2 of the first
and the last element of every batch group --,
so that one dropped key or row there moves the gradients beyond the bound (tests/test_attn_bwd_fp64_cpu.py proves that on these very inputs,
without a GPU).  Every case asserts its bodies through fat5_attn_describe before it launches.

CASES, `inputs`, `reference` and `describe` are module-level and CPU-only.
"""
import ctypes
import zlib

import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
from oracle.rpe import relative_position_bucket

BF16, F16 = torch.bfloat16, torch.float16
BOOST = 32.0
NUM_BUCKETS = 32
WORST = {}   # group (bodies) -> [launches, {output: [worst ratio, its case]}]

# fat5_variant bits by name (flasht5_amd/_lib.py), resolved where the library is loaded
SEP32 = ("V_KV64_OFF", "V_Q64_OFF", "V_QDB64_OFF", "V_NO_FUSE")
ONE32 = ("V_KV64_OFF", "V_Q64_OFF", "V_QDB64_OFF")
FORCE64 = ("V_KV64_ON", "V_Q64_ON", "V_QDB64_ON", "V_FUSED64_ON")   # (dense rows that are no multiple of 8 keys cannot travel by LDS-DMA: the dispatcher keeps the 32-wide bodies)
DENSE_SHAPE = {"11": (1, 1), "1h": (1, 0), "b1": (0, 1), "bh": (0, 0)}   # 1 = broadcast


def _name(dtype):
    return str(dtype)[6:]


def _build_cases():
    out = []

    def add(group, bits, B, H, M, N, D, dtype, causal=False, bias="none", R=0, strided=False, pert=False, split=False, fused=0, route=None,
            dtable=None):
        cid = (f"{group}-{B}x{H}x{M}x{N}-D{D}-{_name(dtype)}-{bias}{R if R else ''}{'-causal' if causal else ''}{'-strided' if strided else ''}"
               f"{'-pert' if pert else ''}{'-stages' if split else ''}{'-' + route if route in ('inkernel', 'nosplit') else ''}{'-' + dtable if dtable else ''}")
        dense = bias[:2] in DENSE_SHAPE
        if dense and route is None:
            assert bias[:2] == "bh" or (B > 1 and H > 1)
            route = "direct" if bias[:2] == "bh" else "staged"
        if route in ("inkernel", "nosplit"):
            bits = bits + ("V_DBIAS_INKERNEL",) + (("V_DBIAS_NOSPLIT",) if route == "nosplit" else ())
        elif route == "staged" and bits is not FORCE64:
            bits = bits + ("V_DBIAS_STAGED",)
        if dtable == "scan":
            bits = bits + ("V_DTABLE_RUNS_OFF",)
        bodies = dict(dq="32row", dkdv="32key", fused=str(fused), qdiag="0")
        if dense:
            bodies["dbias"] = "inkernel" if route == "nosplit" else route
        if dtable:
            bodies["dtable"] = dtable
        out.append(dict(id=cid, group=group, bodies=bodies, bits=bits, B=B, H=H, M=M, N=N, D=D, dtype=dtype, causal=causal, bias=bias, R=R,
                        scale=float(D) ** -0.5, strided=strided, pert=pert, split=split))

    # ---- 32-wide bodies, separate launches, two waves (fewer than 160 workgroups) ----
    Ms, Ns = (1, 31, 32, 33, 64, 65, 129), (1, 63, 64, 65, 127, 128, 129, 200)
    kinds = ("none", "rpe", "1h", "rpe", "bh", "none", "11", "rpe", "b1")
    i = 0
    for j, N in enumerate(Ns):
        for M in (Ms[j % 7], Ms[(3 * j + 2) % 7]):
            bias = kinds[i % 9]
            add("w2", SEP32, 1 + i % 2 if bias not in ("1h", "b1", "11") else 2, 2, M, N, (16, 32, 64, 128)[i % 4], (BF16, F16)[(i // 2) % 2], causal=i % 5 in (1, 3),
                bias=bias, R=(8, 128, 1)[(i // 2) % 3] if bias == "rpe" else 0, strided=i % 4 == 0, split=i % 5 == 2)
            i += 1
    # ---- ... four waves (160 workgroups or more in the stage) ----
    for i, (H, M, N, D, bias) in enumerate(((80, 33, 129, 64, "rpe"), (40, 128, 200, 32, "none"), (80, 65, 64, 64, "1h"), (40, 129, 65, 128, "none"))):
        add("w4", SEP32, 2, H, M, N, D, (BF16, F16)[i % 2], causal=i == 1, bias=bias, R=8 if bias == "rpe" else 0, strided=i == 0)
    # ---- causal, bottom-right: N - M in {0, 1, 100, -1, -100} (the last two with dead rows), with the table, without, dense ----
    for i, d in enumerate((0, 1, 100, -1, -100)):
        M, N = (129, 129 + d) if d >= 0 else (129 - d, 129)
        bias = ("rpe", "none")[i % 2]
        add("causal", SEP32, 1, 2, M, N, 64, (BF16, F16)[(i // 2) % 2], causal=True, bias=bias, R=(128, 8)[(i // 2) % 2] if bias == "rpe" else 0)
        add("causal", SEP32, 2, 2, M, N, (32, 128)[i % 2], (F16, BF16)[(i // 2) % 2], causal=True, bias=("1h", "bh", "11")[i % 3], strided=i == 3)
    # ---- T5 tables through the bucket map: the table gradient per bucket run and by the scan, and drpe1d of an i.i.d. generator ----
    i = 0
    for R in (8, 128):
        for B in (1, 3):
            M, N = ((100, 140 + R), (131, 330))[i % 2] if R == 8 else ((200, 330), (65, 300))[i % 2]
            add("t5", SEP32, B, 2, M, N, (64, 32)[i % 2], (BF16, F16)[i % 2], bias="t5b", R=R, dtable="runs", causal=i == 3)
            add("t5", SEP32, B, 2, M, N, (64, 128)[i % 2], (F16, BF16)[i % 2], bias="t5u", R=R, dtable=("scan", "runs")[i % 2], split=i == 2)
            add("t5", SEP32, B, 2, M, N, 64, (BF16, F16)[i % 2], bias="t5b", R=R, dtable="scan", strided=i == 1)
            i += 1
    add("t5", SEP32, 3, 2, 100, 141, 64, BF16, bias="rpe", R=1)
    # ---- dense dbias: the batch-inner kernel (split over two wave groups, unsplit, with the fp32 scratch at B = 5), staged at B = 5 ----
    for i, (B, M, N, D, route) in enumerate(((2, 65, 64, 64, "inkernel"), (5, 129, 136, 64, "inkernel"), (5, 65, 127, 64, "nosplit"), (4, 33, 200, 128, "inkernel"),
                                             (5, 129, 136, 64, "staged"), (9, 64, 65, 32, "inkernel"))):
        add("dbias", SEP32, B, 2, M, N, D, (BF16, F16)[i % 2], causal=i in (1, 4), bias="1h", route=route, split=i == 1)
    add("dbias", SEP32, 2, 2, 130, 192, 64, BF16, bias="1h-min", route="staged")          # finfo.min on half the keys, and on all keys of some rows
    add("dbias", FORCE64, 2, 2, 65, 63, 64, BF16, bias="1h")                              # the 64-wide bodies asked for, N % 8 != 0: falls back to the 32-wide ones
    # ---- perturbed (o, lse): the kernels follow what is stored ----
    add("pert", SEP32, 1, 2, 65, 129, 64, BF16, pert=True)
    add("pert", SEP32, 2, 2, 129, 200, 128, F16, bias="rpe", R=8, causal=True, pert=True)
    add("pert", SEP32, 2, 2, 64, 65, 32, BF16, bias="bh", pert=True, split=True)
    add("pert", SEP32, 2, 2, 33, 128, 16, F16, bias="1h", pert=True, strided=True)
    # ---- the 32-wide one-launch form: both stages at four waves, D <= 64, both grids together at most four workgroups per CU ----
    add("fused32", ONE32, 2, 80, 129, 200, 64, BF16, fused=1)
    add("fused32", ONE32, 2, 80, 33, 65, 32, F16, causal=True, fused=1, strided=True)
    add("fused32", ONE32, 2, 80, 65, 129, 64, F16, bias="rpe", R=8, fused=1)
    add("fused32", ONE32, 2, 80, 64, 100, 16, BF16, bias="t5b", R=128, dtable="runs", causal=True, fused=1)
    add("fused32", ONE32, 2, 80, 33, 64, 64, BF16, bias="1h", fused=1)
    add("fused32", ONE32, 2, 80, 31, 63, 64, F16, bias="bh", causal=True, fused=1)
    add("fused32", ONE32, 2, 80, 65, 33, 64, BF16, causal=True, pert=True, fused=1)
    add("fused32", ONE32, 2, 80, 32, 127, 32, BF16, bias="rpe", R=1, pert=True, fused=1)
    # ================================================================================================================================
    # The non-dense 64-wide bodies of csrc/attn_bwd64.h (D = 64): smallest shapes at which their trips, rings, wave and workgroup seams exist
    # ================================================================================================================================
    SCALES = (0.125, 1.0, 0.3)   # (0.125 = 64 ** -0.5 has an exact reciprocal; 0.3 has none in fp32 or in 16 bits)
    KV, KVH, KVM = ("V_KV64_ON", "V_KV64_HALF_OFF", "V_KV64_MIX_OFF"), ("V_KV64_ON", "V_KV64_HALF_ON"), ("V_KV64_ON", "V_KV64_MIX_ON")
    Q32, Q64, SEP = ("V_Q64_OFF", "V_FUSED64_OFF"), ("V_Q64_ON", "V_FUSED64_OFF"), ("V_FUSED64_OFF",)
    n64 = [0]

    def add64(group, bits, dq, dkdv, B, H, M, N, dtype, fused=0, qdiag=0, causal=False, bias="none", R=0, scale=None, dtable=None, strided=False, pert=False,
              split=False, tag=""):
        i = n64[0]
        n64[0] += 1
        scale = SCALES[i % 3] if scale is None else scale
        if dtable == "scan":
            bits = bits + ("V_DTABLE_RUNS_OFF",)
        cid = (f"{group}{tag}-{B}x{H}x{M}x{N}-{_name(dtype)}-{bias}{R if R else ''}-s{scale}{'-causal' if causal else ''}{'-strided' if strided else ''}"
               f"{'-pert' if pert else ''}{'-stages' if split else ''}{'-' + dtable if dtable else ''}{'-qd%d' % qdiag if 'V_QDIAG_ON' in bits or 'V_QDIAG_OFF' in bits else ''}"
               f"{'-plain' if not bits else ''}")
        if group == "fused64":
            fused = 1
        bodies = dict(dq=dq, dkdv=dkdv, fused=str(fused), qdiag=str(qdiag))
        if dtable:
            bodies["dtable"] = dtable
        out.append(dict(id=cid, group=group, bodies=bodies, bits=bits, B=B, H=H, M=M, N=N, D=64, dtype=dtype, causal=causal, bias=bias, R=R, scale=scale,
                        strided=strided, pert=pert, split=split, wide=True))

    dt = lambda i: (BF16, F16)[i % 2]
    # ---- kv64: the 64-key dK/dV body on the statistics of the 32-row dQ kernel ----
    Ms, Ns = (90, 127, 128, 129, 255, 256, 257, 300, 385), (63, 64, 65, 128, 192, 255, 256, 257, 300, 520)
    kinds = (("none", 0), ("rpe", 8), ("rpe", 1), ("none", 0), ("rpe", 128))
    for i, N in enumerate(Ns):
        bias, R = kinds[i % 5]
        add64("kv64", KV + Q32, "32row", "64key", 1 + i % 2, 2, Ms[(2 * i + 1) % 9], N, dt(i), bias=bias, R=R, strided=i % 4 == 1, split=i % 5 == 3, pert=i == 6)
    for i, (M, N) in enumerate(((90, 300), (128, 64), (255, 257), (300, 192), (385, 128))):   # (the M values the pairing above left out)
        add64("kv64", KV + Q32, "32row", "64key", 1, 2, M, N, dt(i + 1), bias=("rpe", "none")[i % 2], R=8 if i % 2 == 0 else 0)
    add64("kv64", KV + Q32, "32row", "64key", 1, 2, 384, 384, BF16, bias="rpe", R=8)          # far-positive, band and far-negative trips in one workgroup
    add64("kv64", KV + Q32, "32row", "64key", 2, 2, 384, 384, F16, bias="t5b", R=8, dtable="runs", scale=0.3)
    add64("kv64", KV + Q32, "32row", "64key", 1, 2, 385, 520, BF16, bias="t5u", R=128, dtable="scan", scale=1.0)
    # ---- kv64h: 128-key workgroups, two pairs: an odd number of steps (unequal halves), fewer steps than two rings ----
    for i, (M, N, bias, R, causal) in enumerate(((288, 257, "none", 0, False), (160, 128, "rpe", 8, False), (415, 300, "rpe", 8, False), (96, 192, "none", 0, False),
                                                 (544, 130, "t5b", 8, False), (300, 300, "none", 0, True), (385, 384, "rpe", 128, True))):
        add64("kv64h", KVH + Q32, "32row", "64key-half", 1 + i % 2, 2, M, N, dt(i), bias=bias, R=R, causal=causal, dtable="runs" if bias == "t5b" else None,
              strided=i == 2, pert=i == 3, split=i == 1)
    # ---- kv64m: 256-key and half-length workgroups in one launch: B H a multiple of 8, at least 16 ----
    for i, (B, H, M, N, bias, R, dtable) in enumerate(((2, 8, 129, 300, "t5b", 8, "runs"), (4, 4, 140, 384, "t5b", 128, "scan"), (2, 8, 257, 520, "none", 0, None),
                                                       (3, 8, 130, 520, "t5u", 8, "scan"), (2, 8, 160, 300, "rpe", 8, None))):
        add64("kv64m", KVM + Q32, "32row", "64key-mixed:1", B, H, M, N, dt(i), bias=bias, R=R, dtable=dtable, strided=i == 2, split=i == 0)
    # ---- q64: the 64-row dQ body beside the 32-key dK/dV body (the mirror of kv64) ----
    Ms, Ns = (63, 64, 65, 128, 255, 256, 257), (90, 127, 128, 129, 256, 300, 385)
    for i, M in enumerate(Ms):
        bias, R = kinds[(i + 1) % 5]
        add64("q64", ("V_KV64_OFF",) + Q64, "64row", "32key", 1 + i % 2, 2, M, Ns[(3 * i + 2) % 7], dt(i), bias=bias, R=R, strided=i % 4 == 2, split=i == 4, pert=i == 5)
    add64("q64", ("V_KV64_OFF",) + Q64, "64row", "32key", 1, 2, 384, 385, F16, bias="rpe", R=8)
    add64("q64", ("V_KV64_OFF",) + Q64, "64row", "32key", 2, 2, 300, 384, BF16, bias="t5b", R=8, dtable="runs")
    # ---- sep64: both 64-wide bodies as separate launches (the statistics as the dQ kernel's quotient -L / scale) ----
    add64("sep64", KV + ("V_Q64_ON",) + SEP, "64row", "64key", 1, 2, 257, 300, BF16, bias="rpe", R=8, scale=0.3)
    add64("sep64", KV + ("V_Q64_ON",) + SEP, "64row", "64key", 2, 2, 385, 257, F16, scale=0.3, split=True)
    add64("sep64", KVH + ("V_Q64_ON",) + SEP, "64row", "64key-half", 1, 2, 300, 385, F16, bias="t5b", R=8, dtable="scan", scale=1.0)
    # ---- fused64: one launch, the dK/dV half on statistics of its own (SELF) ----
    ONE = ("V_FUSED64_ON",)
    add64("fused64", (), "64row", "64key", 1, 2, 257, 300, BF16)                                                      # no variant bit: the path a plain call takes
    add64("fused64", (), "64row", "64key", 2, 2, 129, 385, F16, bias="rpe", R=8, qdiag=1)
    add64("fused64", (), "64row", "64key", 1, 2, 384, 384, F16, bias="rpe", R=1, qdiag=1, pert=True)
    add64("fused64", (), "64row", "64key", 1, 4, 512, 512, BF16, bias="t5b", R=128, qdiag=1, dtable="runs", scale=1.0)  # the benchmark's configuration at B = 1, H = 4
    add64("fused64", (), "64row", "64key", 2, 2, 90, 63, BF16, scale=0.3, strided=True)
    add64("fused64", ONE, "64row", "64key", 1, 2, 300, 520, F16, bias="rpe", R=128, qdiag=1, split=True)
    add64("fused64", ONE, "64row", "64key", 2, 2, 255, 256, BF16, pert=True)
    add64("fused64", ONE, "64row", "64key", 1, 2, 128, 129, F16, bias="t5u", R=8, qdiag=1, dtable="scan", strided=True)
    # ---- qdiag: the diagonal sums in the dQ workgroups always / never, on the same inputs ----
    for i, (B, M, N, bias, R, dtable) in enumerate(((1, 384, 384, "rpe", 8, None), (3, 257, 300, "t5b", 8, "runs"), (1, 300, 385, "t5u", 128, "scan"),
                                                    (3, 129, 257, "t5b", 128, "scan"), (1, 385, 257, "t5u", 8, "runs"), (1, 257, 300, "rpe", 128, None))):
        for qd in (1, 0):
            add64("qdiag", ONE + (("V_QDIAG_ON",) if qd else ("V_QDIAG_OFF",)), "64row", "64key", B, 2, M, N, dt(i), fused=1, qdiag=qd, bias=bias, R=R, dtable=dtable,
                  scale=SCALES[i % 3], split=i == 3)
    # ---- causal64: bottom-right masks; no bias (the mask in the C operand), the table inside the band, a table at R = 8 far from the diagonal ----
    forms = (("kv64", KV + Q32, "32row", "64key", 0), ("q64", ("V_KV64_OFF",) + Q64, "64row", "32key", 0), ("fused64", ONE, "64row", "64key", 1))
    for f, (name, bits, dq, dkdv, fused) in enumerate(forms):
        for i, d in enumerate((0, 1, 100, -1, -100)):
            M, N = (257, 257 + d) if d >= 0 else (257 - d, 257)
            bias, R = (("none", 0), ("rpe", 128), ("rpe", 8))[(i + f) % 3] if d != 100 else ("none", 0)
            add64("causal64", bits, dq, dkdv, 1, 2, M, N, dt(i + f), fused=fused, causal=True, bias=bias, R=R, qdiag=1 if (fused and bias == "rpe") else 0,
                  strided=(i + f) == 3, pert=(i + f) == 5, tag="-" + name)
        add64("causal64", bits, dq, dkdv, 1, 2, 284, 384, dt(f), fused=fused, causal=True, bias="rpe", R=8, qdiag=1 if fused else 0, tag="-" + name)   # N - M = 100, R = 8: general diagonal steps
        add64("causal64", bits, dq, dkdv, 1, 2, 512, 512, dt(f + 1), fused=fused, causal=True, bias="rpe", R=128, qdiag=1 if fused else 0, tag="-" + name)   # band trips on the diagonal
    # ---- far bins small enough that one pipelined step's block more or less leaves their bound (u_T times the bin's summed magnitudes) ----
    add64("fused64", ONE, "64row", "64key", 1, 2, 64, 256, F16, bias="rpe", R=8, qdiag=1, scale=0.3)
    add64("fused64", ONE, "64row", "64key", 1, 2, 64, 256, BF16, bias="rpe", R=64, qdiag=1, scale=0.3)
    add64("kv64h", KVH + Q32, "32row", "64key-half", 1, 2, 256, 256, F16, bias="rpe", R=64, scale=0.3)
    add64("sep64", KV + ("V_Q64_ON",) + SEP, "64row", "64key", 1, 2, 128, 256, F16, bias="rpe", R=64, scale=0.3)
    add64("causal64", ONE, "64row", "64key", 1, 2, 256, 256, F16, fused=1, causal=True, bias="rpe", R=64, qdiag=1, scale=0.3, tag="-fused64")
    # ================================================================================================================================
    # The DENSE 64-wide bodies (D = 64): dq=64row-batch4 (csrc/attn_bwd_qdb64.h), the DENSE form of dkdv=64key (csrc/attn_bwd64.h), both in one launch
    # ================================================================================================================================
    SC7 = (0.125, 1.0, -0.5, 0.3, 1.3, 0.0884, -0.3)   # (the first three: 1 / scale is one 16-bit term -- the ONE kernels; the others need two)
    QDB, QDBKV, DFUSED, DKV = ("V_QDB64_ON", "V_KV64_OFF"), ("V_QDB64_ON", "V_KV64_ON", "V_FUSED64_OFF"), ("V_QDB64_ON", "V_KV64_ON", "V_FUSED64_ON"), ("V_KV64_ON", "V_QDB64_OFF")
    nd = [0]

    def addd(group, bits, B, H, M, N, dtype=None, causal=False, bias="1h", scale=None, route=None, pert=False, split=False, strided=False, tag=""):
        i = nd[0]
        nd[0] += 1
        scale = SC7[i % 7] if scale is None else scale
        dtype = dt(i) if dtype is None else dtype
        if bits is DKV:
            dq, dkdv, fused = "32row", "64key", 0
            route = route or ("direct" if bias[:2] == "bh" else "staged")
            if route == "inkernel":
                bits = bits + ("V_DBIAS_INKERNEL",)
            elif route == "staged":
                bits = bits + ("V_DBIAS_STAGED",)
        else:
            dq, dkdv, fused = "64row-batch4", "32key" if bits is QDB else "64key", int(bits is DFUSED or group == "dplain")
            route = "dq-kernel" if B <= 4 else "dq-kernel+partials"
        cid = (f"{group}{tag}-{B}x{H}x{M}x{N}-{_name(dtype)}-{bias}-s{scale}{'-causal' if causal else ''}{'-strided' if strided else ''}{'-pert' if pert else ''}"
               f"{'-stages' if split else ''}{'-' + route if dq == '32row' and bias[:2] != 'bh' else ''}{'-plain' if not bits else ''}")
        out.append(dict(id=cid, group=group, bodies=dict(dq=dq, dkdv=dkdv, fused=str(fused), qdiag="0", dbias=route), bits=bits, B=B, H=H, M=M, N=N, D=64, dtype=dtype,
                        causal=causal, bias=bias, R=0, scale=scale, strided=strided, pert=pert, split=split, wide=False, dense64=True))

    # ---- qdb: the dQ + dBias body beside the 32-key dK/dV body.  Batch groups (idle waves, slabs), rows, keys, the workgroup decode ----
    for i, (B, M, N) in enumerate(((1, 1, 8), (2, 63, 24), (3, 64, 32), (4, 65, 40), (5, 130, 128), (6, 64, 136), (8, 65, 160), (9, 63, 264))):
        addd("qdb", QDB, B, 2, M, N, bias=("1h", "1h", "1h-inf", "1h", "1h-view", "1h", "1h", "1h")[i], strided=i % 3 == 1, split=i == 5, pert=i == 6)
    addd("qdb", QDB, 4, 3, 192, 64)                                  # H ngrp n_mblk = 9: the eight-chunk cut with a remainder
    addd("qdb", QDB, 2, 2, 130, 192, BF16, bias="1h-min", scale=0.3)   # finfo.min on half the keys, and on all keys of some rows
    addd("qdb", QDB, 3, 2, 65, 136, BF16, bias="1h-big", scale=0.3)    # |bias| up to 64 through a two-term selector: its residual term at its largest
    addd("qdb", QDB, 5, 2, 64, 160, BF16, bias="1h-big", scale=1.3)
    addd("qdb", QDB, 2, 2, 64, 128, F16, bias="1h-inf", scale=0.0884)
    # ---- qdbkv: both dense 64-wide bodies as two launches (the dK/dV body on the dQ kernel's statistics) ----
    for i, (B, M, N, bias) in enumerate(((2, 130, 264, "1h"), (4, 64, 128, "1h-view"), (5, 65, 136, "1h"), (3, 128, 256, "1h-inf"), (1, 160, 72, "1h"), (6, 90, 64, "1h"))):
        addd("qdbkv", QDBKV, B, 2, M, N, bias=bias, split=i == 2, pert=i == 3, strided=i == 0)
    # ---- dfused: one launch behind the statistics kernel; B H ceil(N / 256) no multiple of 8 (the padding exits) but for the last ----
    for i, (B, H, M, N, bias) in enumerate(((3, 2, 130, 264, "1h"), (2, 3, 64, 128, "1h"), (5, 2, 65, 136, "1h-inf"), (9, 1, 128, 256, "1h"), (1, 3, 300, 72, "1h"),
                                            (2, 2, 160, 520, "1h-view"), (4, 2, 90, 264, "1h-big"), (2, 4, 128, 160, "1h"))):
        addd("dfused", DFUSED, B, H, M, N, bias=bias, pert=i in (1, 5), split=i == 3, strided=i == 4, dtype=BF16 if bias == "1h-big" else None,
             scale=0.3 if bias == "1h-big" else None)
    addd("dplain", (), 2, 8, 128, 128, BF16, scale=0.125)             # no variant bit: what a plain model call takes
    addd("dplain", (), 4, 2, 192, 264, F16, scale=1.0)
    addd("dplain", (), 6, 2, 65, 136, BF16, scale=0.3, pert=True)
    # ---- dkv64: the DENSE 64-key dK/dV body beside the 32-row dQ kernel: every broadcast kind, every dbias route of that kernel ----
    for i, (B, M, N, bias, route, causal) in enumerate(((2, 90, 64, "bh", None, False), (2, 128, 72, "1h", "staged", False), (2, 160, 256, "11", "staged", False),
                                                        (2, 300, 264, "b1", "staged", False), (2, 128, 520, "1h", "inkernel", False), (1, 300, 256, "bh", None, True),
                                                        (2, 160, 264, "1h-min", "staged", False), (5, 130, 64, "1h-inf", "inkernel", False), (2, 256, 256, "bh", None, True),
                                                        (2, 129, 72, "1h-big", "staged", False))):
        addd("dkv64", DKV, B, 2, M, N, bias=bias, route=route, causal=causal, split=i == 3, pert=i == 4, strided=i == 1,
             dtype=BF16 if bias in ("1h-min", "1h-big") else None, scale=0.3 if bias in ("1h-min", "1h-big") else None)
    # ---- dcausal: bottom-right masks, N - M in {0, 1, 100, -1, -100} per form; the final tensor (B <= 4) and the slabs (B > 4) for P > 0 and P < 0 ----
    for f, (name, bits) in enumerate((("qdb", QDB), ("dfused", DFUSED), ("dkv64", DKV))):
        for i, d in enumerate((0, 1, 100, -1, -100)):
            M, N = 136 - d, 136
            addd("dcausal", bits, (2, 5, 3, 6, 4)[(i + f) % 5] if bits is not DKV else 2, 2, M, N, causal=True, bias=("1h", "bh")[i % 2] if bits is DKV else "1h",
                 pert=(i + f) == 3, strided=(i + f) == 4, tag="-" + name)
    addd("dcausal", QDB, 5, 2, 36, 136, causal=True, tag="-qdb")     # P = 100 into the slabs
    addd("dcausal", QDB, 6, 2, 236, 136, causal=True, tag="-qdb")    # P = -100 into the slabs: dead rows, row blocks without steps
    addd("dcausal", QDB, 2, 2, 256, 256, causal=True, tag="-qdb")    # the sweeps of blocks 0 and 2 padded to whole trips
    addd("dcausal", DFUSED, 5, 2, 256, 256, causal=True, tag="-dfused")
    addd("dcausal", QDB, 2, 2, 248, 248, causal=True, tag="-qdb")    # ... and the padding refused for the third block (6 -> 8 steps = 256 keys > 248)
    addd("dcausal", DFUSED, 3, 2, 300, 40, causal=True, tag="-dfused")   # M >> N: row blocks with nt = 0
    addd("dcausal", DFUSED, 2, 8, 128, 128, causal=True, tag="-dfused")  # (H ngrp) % 8 == 0: the row-block-major order
    addd("dcausal", QDB, 4, 2, 192, 192, causal=True, bias="1h-inf", tag="-qdb")
    for c in out:
        c.setdefault("wide", False)   # (wide: a case of the 64-wide groups)
        c.setdefault("dense64", False)   # (dense64: a case of the dense 64-wide groups)
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _build_cases()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def boosted_rows(M):
    """the `do` rows that carry BOOST times the others' magnitude: 0, M - 1, the first rows of the last 32- and 64-row blocks and the seam row"""
    return sorted({0, M - 1, (M - 1) // 32 * 32, (M - 1) // 64 * 64, G.seam_row(M)} - {None})


def seams64(case):
    """(rows, keys) of the 64-wide bodies' seams: keys at every wave start (64 w, which covers the 128- and 256-key workgroup starts); rows at
    every trip start (multiples of 128), at the first step behind the last aligned trip and at the first step of the second pair's half"""
    M, N = case["M"], case["N"]
    nst = (M + 31) // 32
    rows = set(range(0, M, 128)) | {(nst - nst % 4) * 32, (nst + 1) // 2 * 32}
    return sorted(r for r in rows if r < M), list(range(0, N, 64))


def seams_dense64(case):
    """(rows, keys) of the dense 64-wide bodies' seams: every step start (multiples of 32 rows and of 32 keys), which covers the trip starts (128 keys of the
    dQ + dBias body, 128 rows of the 64-key body), the 64-row blocks and the 256-key workgroups"""
    return list(range(0, case["M"], 32)), list(range(0, case["N"], 32))


def bucket_map(case):
    if case["bias"][:2] != "t5":
        return None
    R = case["R"]
    return torch.from_numpy(relative_position_bucket(torch.arange(-R, R + 1).numpy(), case["bias"] == "t5b", NUM_BUCKETS, 128)).to(torch.int32)


def inputs(case):
    """CPU tensors of a case: q, k, v, do (strided views where the case says so), bias (dense, in the dtype) or None, rpe (H, 2R + 1) fp32 or
    None, bucket (2R + 1) int32 or None, and the given o (in the dtype) and lse (fp32)"""
    B, H, M, N, D, dtype = (case[x] for x in ("B", "H", "M", "N", "D", "dtype"))
    g = _gen(case["id"])

    def rnd(S):
        if case["strided"]:   # the model's layout: (B, S, H, D) storage viewed as (B, H, S, D)
            return torch.randn(B, S, H, D, generator=g).to(dtype).permute(0, 2, 1, 3)
        return torch.randn(B, H, S, D, generator=g).to(dtype)

    q, k, v, do = rnd(M), rnd(N), rnd(N), rnd(M)
    rows64, keys64 = seams64(case) if case["wide"] else (seams_dense64(case) if case["dense64"] else ([], []))
    if (case["wide"] or case["dense64"]) and case["scale"] != 0.125:   # (the same spread of scores at every sm_scale: the softmax stays as flat as in the other cases)
        q.copy_((q.float() * (0.125 / case["scale"])).to(dtype))
    for j in ({0, N - 1, F.seam_key(N)} | set(keys64)) - {None}:
        v[:, :, j] = (v[:, :, j].float() * BOOST).to(dtype)
    for m in sorted(set(boosted_rows(M)) | set(rows64)):
        do[:, :, m] = (do[:, :, m].float() * BOOST).to(dtype)
    if case["dense64"]:   # the first and the last element of every batch group (four elements per dQ workgroup), on a row nothing else boosts
        for b in sorted({x for g4 in range(0, B, 4) for x in (g4, min(g4 + 3, B - 1))}):
            if M > 2:
                do[b, :, 2] = (do[b, :, 2].float() * BOOST).to(dtype)
    bias = rpe = None
    kind = case["bias"]
    bucket = bucket_map(case)
    if kind == "rpe":      # an i.i.d. generator: every entry distinct, so a wrong index shows
        rpe = torch.randn(H, 2 * case["R"] + 1, generator=g)
    elif bucket is not None:   # a T5 table through its bucket map (bidirectional / unidirectional), clamped at R
        rpe = torch.randn(NUM_BUCKETS, H, generator=g)[bucket.long()].T.contiguous()
    elif kind != "none":
        sb, sh = DENSE_SHAPE[kind[:2]]
        bias = torch.randn(1 if sb else B, 1 if sh else H, M, N, generator=g).to(dtype)
        if kind.endswith("-min"):
            bias[..., N // 2:] = torch.finfo(dtype).min
            bias[:, :, 7::64, :] = torch.finfo(dtype).min
        elif kind.endswith("-inf"):   # -inf as the additive mask: a run of keys, single entries (one per 32-row operand and more), whole rows
            bias[..., N // 4:N // 2] = -float("inf")
            bias[:, :, 3::16, 1::8] = -float("inf")
            bias[:, :, 5::32, :] = -float("inf")
        elif kind.endswith("-big"):   # |bias| up to 64, flat within a row (the softmax stays as flat as elsewhere): row offsets of both signs in [40, 62]
            off = (40.0 + 22.0 * torch.rand(M, generator=g)) * (1.0 - 2.0 * (torch.arange(M) % 2))
            bias = (bias.float() * 0.5 + off[:, None]).to(dtype)
        elif kind.endswith("-view"):  # a (1, H, M, N) view of a wider tensor: row pitch N + 64
            wide_ = torch.full(bias.shape[:3] + (N + 64,), SENTINEL, dtype=dtype)
            wide_[..., :N] = bias
            bias = wide_[..., :N]
    fwd = F.attn_fwd_ref(q, k, v, case["scale"], case["causal"], bias, rpe, case["R"])
    o = torch.empty_like(q).copy_(fwd["o"].to(dtype))
    lse = fwd["lse"].float()
    if case["pert"]:
        o = rnd(M)
        lse[:, :, ::3] += 0.25   # (-inf stays -inf)
    return dict(q=q, k=k, v=v, do=do, bias=bias, rpe=rpe, bucket=bucket, o=o, lse=lse)


def reference(case, t, mutant=None):
    return G.attn_bwd_ref(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], case["scale"], case["causal"], t["bias"], t["rpe"], case["R"],
                          t["bucket"], NUM_BUCKETS if t["bucket"] is not None else 0, mutant=mutant)


def compared(case, ref):
    """the outputs the kernels write for this case: with a bucket map the table gradient alone"""
    outs = [x for x in G.outputs_of(ref) if x != "drpe1d" or "drpe_table" not in ref]
    return outs


def variant_bits(case):
    from flasht5_amd import _lib
    bits = 0
    for name in case["bits"]:
        bits |= getattr(_lib, name)
    return bits


def describe(case):
    """the backward bodies the library would run this case with (fat5_attn_describe: host-only, no pointer but the host bucket map is followed)"""
    from flasht5_amd import _lib
    B, H, M, N = case["B"], case["H"], case["M"], case["N"]
    p = _lib.AttnParams()
    p.B, p.H, p.M, p.N, p.D = B, H, M, N, case["D"]
    p.dtype, p.causal, p.variant, p.sm_scale = _lib.dtype_code(case["dtype"]), int(case["causal"]), variant_bits(case), case["scale"]
    kind = case["bias"]
    host = None
    if kind[:2] in DENSE_SHAPE:
        sb, sh = DENSE_SHAPE[kind[:2]]
        nh = 1 if sh else H
        p.bias_mode, p.bias, p.dbias = _lib.BIAS_DENSE, 16, 16
        pitch = N + 64 if kind.endswith("-view") else N
        p.bias_stride[0], p.bias_stride[1], p.bias_stride[2] = (0 if sb else nh * M * pitch), (0 if sh else M * pitch), pitch
        p.dbias_batch, p.dbias_heads = (1 if sb else B), nh
    elif kind != "none":
        p.bias_mode, p.rpe1d, p.rpe_radius = _lib.BIAS_RPE1D, 16, case["R"]
        bucket = bucket_map(case)
        if bucket is not None:
            host = (ctypes.c_int32 * len(bucket))(*[int(x) for x in bucket])
            p.rpe_bucket, p.drpe_table, p.rpe_num_buckets, p.rpe_bucket_host = 16, 16, NUM_BUCKETS, ctypes.addressof(host)
        else:
            p.drpe1d = 16
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().fat5_attn_describe(ctypes.byref(p), buf, 256), "fat5_attn_describe")
    return dict(kv.split("=") for kv in buf.value.decode().split())


def assert_bodies(case, d):
    want = case["bodies"]
    got = {key: d.get(key) for key in want}
    assert got == want, f"{case['id']}: the dispatcher runs {got}, the case is meant for {want}"


SENTINEL = 777.0


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _guarded(t):
    """a (B, H, S, D) view with t's shape inside a sentinel-filled buffer that has one spare head slot behind every row of heads"""
    B, H, S, D = t.shape
    buf = torch.full((B, S, H + 1, D), SENTINEL, dtype=t.dtype, device=t.device)
    return buf, buf[:, :, :H].permute(0, 2, 1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_backward_within_the_fp64_bound(case):
    from flasht5_amd import _lib
    from flasht5_amd.flash_attention_v2_bias import AttentionPlan
    assert_bodies(case, describe(case))
    t = inputs(case)
    ref = reference(case, t)
    bound = G.attn_bwd_bound(ref, case["dtype"], case["D"], case["bodies"], case["N"], case["M"])
    dev = {key: (x.to("cuda") if x is not None else None) for key, x in t.items()}
    if case["bias"].endswith("-view"):   # (a copy to the device would pack the rows: build the wider tensor there)
        wide_ = torch.full(t["bias"].shape[:3] + (case["N"] + 64,), SENTINEL, dtype=case["dtype"], device="cuda")
        wide_[..., :case["N"]] = t["bias"].to("cuda")
        dev["bias"] = wide_[..., :case["N"]]
        assert dev["bias"].stride(2) == case["N"] + 64
    if case["strided"]:
        assert dev["q"].stride() == t["q"].stride() and dev["do"].stride() == t["do"].stride() and _lib.kernel_ready(dev["q"])   # (never copied)
    plan = AttentionPlan(dev["q"], dev["k"], dev["v"], dev["do"], bias=dev["bias"], rpe1d=dev["rpe"], radius=case["R"], causal=case["causal"],
                         sm_scale=case["scale"], need_dbias=True, rpe_bucket=dev["bucket"], num_buckets=NUM_BUCKETS if dev["bucket"] is not None else 0,
                         variant=variant_bits(case))
    assert plan.q.data_ptr() == dev["q"].data_ptr() and plan.do.data_ptr() == dev["do"].data_ptr()
    assert_bodies(case, plan.describe())
    assert plan.bwd_launches() == (1 if case["bodies"]["fused"] == "1" else 2)
    guards = []
    if case["strided"]:   # the gradients inside larger sentinel-filled buffers
        for name in ("dq", "dk", "dv"):
            buf, view = _guarded(getattr(plan, name))
            guards.append(buf)
            setattr(plan, name, view)
            setattr(plan.p, name, view.data_ptr())
            setattr(plan.p, name + "_stride", _lib.strides3(view))
    plan.o.copy_(dev["o"])
    plan.lse.copy_(dev["lse"])
    given = {key: x.clone() for key, x in dev.items() if x is not None}
    given["o"], given["lse"] = plan.o.clone(), plan.lse.clone()

    def run():
        for x in (plan.dq, plan.dk, plan.dv, plan.dbias):
            if x is not None:
                x.fill_(SENTINEL)   # (every element has to be written)
        if case["dense64"] and plan.ws is not None and plan.ws.numel():
            plan.ws.view(torch.uint8).fill_(255)   # (NaN patterns in the statistics and in the fp32 slabs: nothing may be read that this call did not write)
        if case["split"]:
            for stage in (1, 2, 4):   # FAT5_BWD_DQ, FAT5_BWD_DKDV, FAT5_BWD_REDUCE
                plan.backward(stage)
        else:
            plan.backward()
        torch.cuda.synchronize()
        got = dict(dq=plan.dq.cpu(), dk=plan.dk.cpu(), dv=plan.dv.cpu())
        if plan.dbias is not None:
            got["dbias" if t["bias"] is not None else ("drpe_table" if t["bucket"] is not None else "drpe1d")] = plan.dbias.cpu()
        return got

    got = run()
    again = run()
    for key, x in given.items():   # lse, o and the inputs are unchanged by the call
        now = plan.o if key == "o" else (plan.lse if key == "lse" else dev[key])
        assert torch.equal(_bits(now), _bits(x)), f"{case['id']}: the call changed {key}"
    for buf in guards:
        assert bool((buf[:, :, case["H"]] == SENTINEL).all()), f"{case['id']}: written outside the gradient's view"
    if case["bias"].endswith("-view"):
        assert bool((wide_[..., case["N"]:] == SENTINEL).all()), f"{case['id']}: the bias tensor's padding changed"
    outs = compared(case, ref)
    assert sorted(got) == sorted(outs)
    for x in outs:
        assert torch.equal(_bits(got[x]), _bits(again[x])), f"{case['id']}: a second call gives other bits in {x}"
    r = G.ratios(got, ref, bound)
    tag = case["group"] + " (" + " ".join(f"{key}={val}" for key, val in case["bodies"].items()) + ")"
    w = WORST.setdefault(tag, [0, {}])
    w[0] += 1
    for x in outs:
        if r[x] >= w[1].setdefault(x, [0.0, ""])[0]:
            w[1][x] = [r[x], case["id"]]
    print(f"[attn-bwd-fp64] {case['id']}: err / bound " + " ".join(f"{x} {r[x]:.3f}" for x in outs))
    bad = [x for x in outs if not r[x] <= 1.0]
    if bad:
        msg = []
        for x in bad:
            gx = got[x].double()
            e = (gx - ref[x]).abs()
            q = torch.where(e == 0, torch.zeros_like(e), e / bound[x])
            q = torch.where(torch.isfinite(gx), q, torch.full_like(q, float("inf")))
            idx = tuple(int(v) for v in torch.nonzero(q == q.max())[0])
            msg.append(f"{x} err/bound {r[x]:.3f} at {idx}: got {float(gx[idx])!r} ref {float(ref[x][idx])!r} bound {float(bound[x][idx]):.3e} "
                       f"T {float(ref['T_' + x][idx]):.3e}")
        raise AssertionError(f"{case['id']}: " + "; ".join(msg))


@pytest.mark.gpu
def test_zz_summary():
    """(runs last) one line per group: the launches and the worst err / bound of this session"""
    for tag, (n, worst) in sorted(WORST.items()):
        print(f"[attn-bwd-fp64] {tag}: {n} launches, worst err/bound " + ", ".join(f"{x} {v[0]:.3f} ({v[1]})" for x, v in sorted(worst.items())))
    assert all(v[0] <= 1.0 for _, worst in WORST.values() for v in worst.values())
