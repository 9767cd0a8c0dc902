"""The attention forward and backward with a T5 table across the accepted radius range 1 <= R <= 2048, per element against the fp64
restatements and the derived bounds of tests/attn_fwd_fp64.py and tests/attn_bwd_fp64.py, with the inputs, the references and the helpers of
tests/test_attn_fwd_fp64_gpu.py / tests/test_attn_bwd_fp64_gpu.py (imported, not copied).

The radius decides structure: the size of the LDS table and of the per-wave diagonal accumulators, which key steps are band steps, which
body the dispatcher may take (TRANSITIONS: found on the host by tests/test_radius_seams_cpu.py, which also proves that every entry has a pair of cases on
either side that differ in exactly the fields it names), whether the backward accepts the call at all (FIRST_REFUSED), and in drpe_reduce_kernel (csrc/reduce_kernels.h) the number of
interleaved chains -- 4 up to n1 = 2R + 1 = 256, 3 up to 341, 2 up to 512, 1 beyond -- and of trips of its 1024 threads (one more per 1024 entries).
Radii: 127 / 128, 170 / 171, 255 / 256 (the chain seams), 511 / 512 (the second trip), 1024 (the third), either side of every transition, the last accepted
and the first refused radius per head dimension and wave count (FIRST_REFUSED), and 2048 (n1 = 4097: the fifth trip) -- forward only where the backward refuses.
Shapes per radius class (B in {1, 3}, H = 2): the problem smaller than the table ("small": only the table's centre is read, most diagonal sums are exact zeros
that must still be written), the band edge inside the problem on both sides ("edge": M = N = R + 76), one side far only ("wideN": (130, R + 200), "wideM":
(R + 200, 130)), causal with 0 < N - M < R and with N - M < 0, and "rounds": B nblk > 16 NG partial rows per head, more than one round of the reduce kernel's
sixteen-row batches, once per chain count.  Bias gradient in its three forms: drpe1d of an i.i.d. table ("rpe": a mis-indexed entry is a different number), the
T5 table gradient per bucket run ("runs") and by the scan ("scan"), with relative_position_bucket at 32 buckets and max_distance = R; at 128 buckets (the limit of
BucketRuns: runs) and 129 (scan); with ids outside [0, num_buckets) at the table's ends (they stay out of the table; still runs) and inside a run (scan); with one id
in two runs (scan).

The bound's reduction term.  attn_bwd_fp64.py charges the diagonal sums gamma_1(2 n + 8) for the n terms of an entry (U - B of the band blocks: each term up to
twice).  That constant holds for ANY order and ANY grouping of the additions of an entry's own terms, and an addition with an exact zero is exact: the kernel's
ceil(nparts / NG) additions per chain, its 2 + 1 tree, the ceil(n1 / 32) + 5 additions of the bucket scan and the run form's order all add partial sums of the
entry's (the bucket's) own n terms or exact zeros, so at most n - 1 of them round, whatever R is.  Nothing in the derivation assumed the chain lengths of R <= 128;
no term had to be extended.

Every case carries the structure the library reports for it (host-only, at import) and asserts it against the plan's own describe before it launches, prints one
`[radius] <case id>: err / bound ...` line, fills the outputs with the sentinel and the workspace with 0xFF bytes, and -- in the backward --
takes o and lse from the test.  CASES and the helpers are module-level and CPU-only.
"""
import pytest
import torch

import attn_bwd_fp64 as G
import attn_fwd_fp64 as F
import test_attn_bwd_fp64_gpu as W

BF16, F16 = torch.bfloat16, torch.float16
SEP32 = W.SEP32
VARIANTS = {   # the forcing bits of the fp64 suites (forward and backward bits are independent)
    "plain": (),
    "w32": SEP32 + ("V_NO_SPLIT", "V_FWD64_OFF"),
    "one64": ("V_FUSED64_ON", "V_FWD64_ON", "V_FWD64_KSPLIT_OFF", "V_FWD64_MIX_OFF"),
    "sep64": ("V_KV64_ON", "V_KV64_HALF_OFF", "V_KV64_MIX_OFF", "V_Q64_ON", "V_FUSED64_OFF", "V_FWD64_ON", "V_FWD64_KSPLIT_ON"),
    "half64": ("V_KV64_ON", "V_KV64_HALF_ON", "V_Q64_OFF", "V_FUSED64_OFF", "V_FWD64_ON"),
}

# every radius at which a host-reported field changes, on 256 compute units
TRANSITIONS = [   # (head_dim, first R of the new structure, field:before>after ..., the variants -- "-nograd": no bias gradient asked for -- it was found with)
    (64, 31, "dkdv:32key>64key dq:32row>64row fused:0>1 kvres:0>1 launches:2>1", "plain-nograd"),   # (causal, N - M = 30 < R: the table carries the mask)
    (64, 31, "dkdv:32key>64key dq:32row>64row fused:0>1 kvres:0>1 launches:2>1 qdiag:0>1", "plain"),
    (64, 45, "fwd:32row-split>64row-ksplit", "plain plain-nograd"),                                  # (causal, N - M = 44 < R, 384 waves of 64 rows)
    (64, 298, "kvres:1>0", "one64 plain"),                                                           # stage_bwd_q64_d64 with the diagonal arrays of qdiag=1
    (64, 313, "kvres:1>0", "one64-nograd plain-nograd sep64 sep64-nograd"),                          # shape: N = R + 200 passes 512 keys
    (64, 414, "fwd:64row-ksplit>32row-split", "plain plain-nograd"),                                 # smem_fwd64_d64 > 80 KiB: no two workgroups per CU
    (64, 416, "kvres:1>0", "one64 one64-nograd plain-nograd"),                                       # stage_bwd_q64_d64 inside the one-launch form
    (64, 437, "kvres:1>0", "sep64 sep64-nograd"),                                                    # shape: N = R + 76 passes 512 keys
    (64, 640, "dkdv:64key-half>32key", "half64 half64-nograd"),                                      # smem_bwd_kv64h_d64 > 160 KiB
    (64, 640, "dkdv:64key-half>32key fused:0>1 launches:2>1", "half64 half64-nograd"),               # ... and at four waves the 32-wide bodies share a launch
    (64, 926, "kvres:1>0", "sep64 sep64-nograd"),                                                    # stage_bwd_q64_d64 of the dQ launch by itself
    (64, 1098, "dkdv:64key>32key dq:64row>32row", "one64 one64-nograd"),                             # smem_bwd_fused64_d64 > 160 KiB (four waves: fused=1 stays, the 32-wide form)
    (64, 1098, "dkdv:64key>32key dq:64row>32row fused:1>0 launches:1>2", "one64-nograd plain-nograd"),
    (64, 1098, "dkdv:64key>32key dq:64row>32row fused:1>0 launches:1>2 qdiag:1>0", "one64 plain"),
    (64, 1152, "dkdv:64key>32key", "sep64 sep64-nograd"),                                            # smem_bwd_kv64_d64 > 160 KiB
    (64, 1984, "refused:0>1", "half64 half64-nograd one64 one64-nograd plain plain-nograd sep64 sep64-nograd w32 w32-nograd"),   # smem_bwd_kv_d64(4, R) > 160 KiB
    (128, 926, "fwd:64row>32row", "one64 one64-nograd"),                                             # smem_fwd64_d128 > 160 KiB
    (128, 926, "fwd:64row>32row-split", "one64 one64-nograd"),
    (128, 1472, "refused:0>1", "one64 one64-nograd plain plain-nograd w32 w32-nograd"),              # smem_bwd_kv_d128(4, R) > 160 KiB
    (128, 1962, "refused:0>1", "one64 one64-nograd plain plain-nograd w32 w32-nograd"),              # smem_bwd_kv_d128(2, R) > 160 KiB
]
# first radius the backward's parameter check refuses, by (head_dim, waves of the 32-key dK/dV body): smem_bwd_kv_d*(nw, R) > 160 KiB.  Head dimensions 16 and 32, and 64
# at two waves, are accepted up to 2048.
FIRST_REFUSED = {(64, "four waves"): 1984, (128, "two waves"): 1962, (128, "four waves"): 1472}


def variant_bits(variant, extra=()):
    from flasht5_amd import _lib
    bits = 0
    for name in VARIANTS[variant] + tuple(extra):
        bits |= getattr(_lib, name)
    return bits


def chains(R):
    n1 = 2 * R + 1
    return 4 if n1 <= 256 else (3 if n1 <= 341 else (2 if n1 <= 512 else 1))   # (reduce_kernels.h: NG)


def trips(R):
    return (2 * R + 1 + 1023) // 1024


def part_rows(case):
    """partial diagonal-sum rows per (b, h) (BwdLayout::part_rows): one per 256-row block with qdiag=1, else one per key block of the dK/dV body"""
    b = case["bodies"]
    if b["qdiag"] == "1":
        return (case["M"] + 255) // 256
    if b["dkdv"] == "64key":
        return (case["N"] + 255) // 256
    if b["dkdv"] == "64key-half":
        return (case["N"] + 127) // 128
    return (case["N"] + 32 * case["nw_kv"] - 1) // (32 * case["nw_kv"])


def reported(case):
    """the structure of a case as the library reports it (host-only; the params are those of the call the test makes: W.describe_params)"""
    import ctypes
    from flasht5_amd import _lib
    lib = _lib.load()
    p, host = W.describe_params(case)
    buf = ctypes.create_string_buffer(256)
    _lib.check(lib.fat5_attn_describe(ctypes.byref(p), buf, 256), "fat5_attn_describe")
    d = dict(kv.split("=") for kv in buf.value.decode().split())
    rc = lib.fat5_attn_bwd_stages(ctypes.byref(p), 7, None)   # (no tensors: refused for the radius, or for the null pointers)
    msg = lib.fat5_last_error().decode()
    assert rc == -1
    d.update(kvres=str(lib.fat5_attn_bwd_kvres(ctypes.byref(p))), launches=str(lib.fat5_attn_bwd_launches(ctypes.byref(p))), refused=str(int("bytes of LDS" in msg)))
    return d


def _build_cases():
    out = []

    def add(R, shape, B=1, variant="w32", form="rpe", D=64, dtype=BF16, causal=False, grad=True, fwd_check=False, bwd=True, perturb=False, H=2, tag="", **extra):
        M, N = {"small": (100, 130), "edge": (R + 76, R + 76), "wideN": (130, R + 200), "wideM": (R + 200, 130)}[shape] if isinstance(shape, str) else shape
        bias = "rpe" if form == "rpe" else extra.pop("kind", "t5b")
        xbits = ("V_DTABLE_RUNS_OFF",) if form == "scan" and not extra.pop("scan_by_itself", False) else ()
        sname = shape if isinstance(shape, str) else f"{M}x{N}"
        cid = (f"{variant}-{B}x{H}x{M}x{N}-D{D}-{str(dtype)[6:]}-{form}{R}-{sname}{'-causal' if causal else ''}{'' if grad else '-nograd'}{'' if bwd else '-fwd'}"
               f"{'-' + tag if tag else ''}")
        case = dict(id=cid, group="radius", variant=variant, form=form, shape=sname, bits=VARIANTS[variant] + xbits, B=B, H=H, M=M, N=N, D=D, dtype=dtype, causal=causal,
                    bias=bias, R=R, scale=float(D) ** -0.5, strided=False, pert=False, split=False, wide=D == 64 and variant != "w32", dense64=False, grad=grad,
                    fwd_check=fwd_check, perturb=perturb, max_distance=R, **extra)
        # the structure is the library's own answer (host-only), pinned through TRANSITIONS: tests/test_radius_seams_cpu.py asserts that the cases on either side of every
        # transition differ in exactly the fields the table names; the form of the table gradient is the case's own claim
        d = reported(case)
        bodies = {f: d[f] for f in ("dq", "dkdv", "fused", "qdiag")}
        if form != "rpe":
            bodies["dtable"] = form
        refused = d["refused"] == "1"
        case.update(bodies=bodies, fwd=d["fwd"], kvres=d["kvres"], launches=int(d["launches"]), refused=refused, bwd=bwd and not refused,
                    nw_kv=2 if B * H * ((N + 127) // 128) < 160 else 4)   # (waves of the 32-key dK/dV body: four from 160 workgroups on)
        out.append(case)

    dt = lambda i: (BF16, F16)[i % 2]
    shapes = ("edge", "wideN", "small", "wideM")
    # ---- the reduce kernel's chain seams and trips, D = 64: the three forms of the bias gradient, the shape classes and the launch forms in rotation ----
    for i, R in enumerate((127, 128, 170, 171, 255, 256, 511, 512, 1024)):
        for j, form in enumerate(("rpe", "scan", "runs")):
            k = i + j
            add(R, shapes[k % 4], B=(1, 3)[k % 2] if R < 1024 or shapes[k % 4] == "small" else 1, variant=("w32", "one64", "sep64", "plain")[(i + 2 * j) % 4], form=form,
                dtype=dt(i + j), fwd_check=j == 0, perturb=(i + 2 * j) % 4 == 0)
    # (perturb: the 32-wide cases, in all three forms of the bias gradient and in every shape class -- their diagonal sums are formed from the fp32 dS, so one dropped
    # diagonal leaves the bound; the far bins of the 64-wide bodies carry u_T of tens of thousands of terms, attn_bwd_fp64.py, and cannot see it: DESIGN.md)
    # ---- more than one round of sixteen partial rows per chain: B nblk > 16 NG, the 32-key body at two waves (64 keys per partial row) ----
    for i, (R, N) in enumerate(((100, 1400), (150, 1100), (200, 720), (300, 400))):
        add(R, (65, N), B=3, variant="w32", form=("rpe", "scan")[i % 2], dtype=dt(i), tag="rounds")
        add(R, (65, N), B=3, variant="w32", form=("scan", "rpe")[i % 2], dtype=dt(i + 1), tag="rounds")
    # ---- causal: 0 < N - M < R (the table carries the mask in the 64-wide bodies) and N - M < 0, once per radius class ----
    for i, R in enumerate((128, 171, 256, 512)):
        add(R, (R + 40, R + 140), variant=("one64", "w32")[i % 2], form=("rpe", "scan")[i % 2], dtype=dt(i), causal=True, fwd_check=True)
        add(R, (R + 140, R + 40), variant=("w32", "one64")[i % 2], form=("runs", "rpe")[i % 2], dtype=dt(i + 1), causal=True)
    # ---- either side of every transition: the same class, head dimension, variant, mask and gradient at R - 1 and at R ----
    w4, f384 = dict(H=80), dict(H=96)   # ("waves4": 160 dK/dV workgroups at (100, 130); "fwd384": 384 waves of 64 rows at (256, 300))
    for R in (30, 31):      # causal, N - M = 30 < R: the table carries the mask
        add(R, "small", variant="plain", form="rpe", dtype=dt(R), causal=True, tag="seam")
        add(R, "small", variant="plain", form="rpe", dtype=dt(R + 1), causal=True, grad=False, tag="seam")
    for R in (44, 45):      # causal, N - M = 44 < R
        add(R, (256, 300), variant="plain", form="rpe", dtype=BF16, causal=True, fwd_check=True, tag="seam", **f384)   # (bf16: with fp16 the forward's own rule asks for four times the waves)
    for R in (297, 298):
        add(R, "small", variant="one64", form="rpe", dtype=dt(R), tag="seam")
    for R in (312, 313):    # shape: N = R + 200 passes 512 keys
        add(R, "wideN", variant="sep64", form="scan", dtype=dt(R), tag="seam")
    for R in (413, 414):    # smem_fwd64_d64 > 80 KiB
        add(R, (256, 300), variant="plain", form="rpe", dtype=BF16, fwd_check=True, tag="seam", **f384)
    for R in (415, 416):
        add(R, "small", variant="one64", form="rpe", dtype=dt(R), grad=False, tag="seam")
    for R in (436, 437):    # shape: N = R + 76 passes 512 keys
        add(R, "edge", variant="sep64", form="runs", dtype=dt(R), tag="seam")
    for R in (639, 640):    # smem_bwd_kv64h_d64 > 160 KiB: at two waves, and at four (the 32-wide bodies then share a launch)
        add(R, "small", B=3, variant="half64", form=("rpe", "scan")[R % 2], dtype=dt(R), tag="seam")
        add(R, (256, 300), variant="half64", form="rpe", dtype=dt(R + 1), tag="seam", **f384)
    for R in (925, 926):
        add(R, "small", variant="sep64", form="rpe", dtype=dt(R), fwd_check=True, tag="seam")
        add(R, "small", variant="one64", form="rpe", D=128, dtype=dt(R + 1), fwd_check=True, tag="seam")
        add(R, "small", variant="one64", form="rpe", D=128, dtype=dt(R), fwd_check=True, tag="seam", **w4)   # (... to the split form)
    for R in (1097, 1098):  # smem_bwd_fused64_d64 > 160 KiB
        add(R, "small", variant="one64", form=("rpe", "scan")[R % 2], dtype=dt(R), fwd_check=True, tag="seam")
        add(R, "small", variant="one64", form="rpe", dtype=dt(R + 1), grad=False, tag="seam")
        add(R, (256, 300), variant="one64", form="rpe", dtype=dt(R), tag="seam", **f384)   # (four waves: one launch stays, in the 32-wide form)
    for R in (1151, 1152):
        add(R, "small", B=3, variant="sep64", form=("runs", "rpe")[R % 2], dtype=dt(R), tag="seam")
    # ---- the last accepted and the first refused radius of the four-wave 32-key body (the forward still runs) ----
    for R in (1983, 1984):
        add(R, "small", variant="w32", form="rpe", D=64, dtype=dt(R), fwd_check=True, tag="seam", **w4)
    for R in (1471, 1472):
        add(R, "small", variant="w32", form="rpe", D=128, dtype=dt(R), fwd_check=True, tag="seam", **w4)
    # ---- the 160 KiB rules at D = 32 and 128; the last accepted and the first refused radius at D = 128 (the forward still runs); 2048: n1 = 4097 ----
    add(1024, "small", variant="w32", form="rpe", D=32, dtype=F16, fwd_check=True)
    add(1024, "edge", variant="w32", form="scan", D=128, dtype=BF16, fwd_check=True)
    add(1961, "small", variant="w32", form="rpe", D=128, dtype=F16, fwd_check=True, tag="seam")
    add(1962, "small", variant="w32", form="rpe", D=128, dtype=BF16, fwd_check=True, tag="seam")
    add(2048, "small", B=3, variant="w32", form="scan", D=64, dtype=BF16, fwd_check=True)
    add(2048, "small", variant="w32", form="rpe", D=32, dtype=F16, fwd_check=True)
    add(2048, "small", variant="one64", form="rpe", D=64, dtype=F16, fwd_check=True, bwd=False)
    add(2048, "small", variant="w32", form="rpe", D=128, dtype=BF16, fwd_check=True)
    # ---- bucket maps: 128 buckets (the limit of BucketRuns) and 129; ids outside the table at its ends and inside a run; one id in two runs ----
    def ends(ids):
        ids = ids.clone()
        ids[0], ids[-1] = -1, 32
        return ids

    def inside(ids):
        ids = ids.clone()
        ids[3], ids[len(ids) // 2 + 40] = -5, 1000
        return ids

    def twice(ids):
        ids = ids.clone()
        ids[0] = ids[len(ids) // 2]
        return ids
    add(512, "edge", variant="w32", form="runs", num_buckets=128, tag="b128")
    add(512, "edge", variant="one64", form="scan", scan_by_itself=True, num_buckets=129, tag="b129")
    add(256, "wideN", B=3, variant="one64", form="runs", bucket_edit=ends, tag="ends")
    add(256, "wideN", B=3, variant="w32", form="scan", scan_by_itself=True, bucket_edit=inside, tag="inside")
    add(171, "edge", variant="w32", form="scan", scan_by_itself=True, bucket_edit=twice, tag="twice")
    return out


CASES = _build_cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def structure(case):
    """the fields of the host calls as the case carries them"""
    b = case["bodies"]
    return dict(fwd=case["fwd"], dq=b["dq"], dkdv=b["dkdv"], fused=b["fused"], qdiag=b["qdiag"], kvres=case["kvres"], launches=str(case["launches"]),
                refused=str(int(case["refused"])))


_REF = {}  # case id -> (inputs, reference): computed once, shared, never written


def truth(case):
    if case["id"] not in _REF:
        t = W.inputs(case)
        _REF[case["id"]] = (t, W.reference(case, t))
    return _REF[case["id"]]


def _plan(case, t):
    from flasht5_amd.flash_attention_v2_bias import AttentionPlan
    dev = {key: (x.to("cuda") if torch.is_tensor(x) else None) for key, x in t.items()}
    plan = AttentionPlan(dev["q"], dev["k"], dev["v"], dev["do"], rpe1d=dev["rpe"], radius=case["R"], causal=case["causal"], sm_scale=case["scale"],
                         need_dbias=case["grad"], rpe_bucket=dev["bucket"], num_buckets=W.num_buckets(case) if dev["bucket"] is not None else 0,
                         variant=variant_bits(case["variant"], [b for b in case["bits"] if b not in VARIANTS[case["variant"]]]))
    return plan, dev


def _fill(plan):
    for x in (plan.dq, plan.dk, plan.dv, plan.dbias):
        if x is not None:
            x.fill_(W.SENTINEL)   # (every element has to be written)
    plan.ws.view(torch.uint8).fill_(255)   # (NaN patterns: nothing may be read that this call did not write)


def _untouched(plan):
    return all(bool((x == W.SENTINEL).all()) for x in (plan.dq, plan.dk, plan.dv, plan.dbias) if x is not None)


def check_forward(case, t, plan):
    """(text for the case's line, inside the bound?)"""
    ref = F.attn_fwd_ref(t["q"], t["k"], t["v"], case["scale"], case["causal"], None, t["rpe"], case["R"])
    bo, bl = F.attn_fwd_bound(ref, case["dtype"], case["D"], case["fwd"], case["N"])
    plan.o.fill_(W.SENTINEL)
    plan.lse.fill_(W.SENTINEL)
    plan.forward()
    torch.cuda.synchronize()
    ro, rl, same = F.ratios(plan.o.cpu(), plan.lse.cpu(), ref, bo, bl)
    return f"fwd {case['fwd']} o {ro:.3f} lse {rl:.3f}", bool(same and ro <= 1.0 and rl <= 1.0)


def check_backward(case, t, ref, plan, dev, stages=(False, True)):
    """(text for the case's line, inside the bound?): the backward as one call and stage by stage"""
    bound = G.attn_bwd_bound(ref, case["dtype"], case["D"], case["bodies"], case["N"], case["M"])
    outs = [x for x in W.compared(case, ref) if case["grad"] or x in ("dq", "dk", "dv")]
    plan.o.copy_(dev["o"])
    plan.lse.copy_(dev["lse"])
    text, ok = [], True
    for staged in stages:
        _fill(plan)
        if staged:
            for stage in (1, 2, 4):
                plan.backward(stage)
        else:
            plan.backward()
        torch.cuda.synchronize()
        got = dict(dq=plan.dq.cpu(), dk=plan.dk.cpu(), dv=plan.dv.cpu())
        if plan.dbias is not None:
            got["drpe_table" if t["bucket"] is not None else "drpe1d"] = plan.dbias.cpu()
        assert sorted(got) == sorted(outs)
        r = G.ratios(got, ref, bound)
        text.append(("stages " if staged else "one call ") + " ".join(f"{x} {r[x]:.3f}" for x in outs))
        ok = ok and all(r[x] <= 1.0 for x in outs)
    return f"bwd chains {chains(case['R'])} trips {trips(case['R'])} " + " | ".join(text), ok


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_radius_within_the_fp64_bounds(case):
    t, ref = truth(case)
    plan, dev = _plan(case, t)
    d = plan.describe()
    W.assert_bodies(case, d)
    assert (d["fwd"], d["kvres"], plan.bwd_launches()) == (case["fwd"], case["kvres"], case["launches"]), d
    line, good = [], True
    if case["fwd_check"]:
        text, ok = check_forward(case, t, plan)
        line.append(text)
        good = good and ok
    if case["refused"]:
        _fill(plan)
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            plan.backward()
        torch.cuda.synchronize()
        ok = _untouched(plan)
        line.append("bwd refused, outputs " + ("untouched" if ok else "WRITTEN"))
        good = good and ok
    elif case["bwd"]:
        text, ok = check_backward(case, t, ref, plan, dev)
        line.append(text)
        good = good and ok
    print(f"[radius] {case['id']}: err / bound " + "; ".join(line))
    assert good, case["id"]


LAST_ACCEPTED = [c for c in CASES if c["bwd"] and FIRST_REFUSED.get((c["D"], "two waves" if c["nw_kv"] == 2 else "four waves")) == c["R"] + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAST_ACCEPTED, ids=[c["id"] for c in LAST_ACCEPTED])
def test_a_refused_radius_leaves_the_plan_usable(case):
    """Per head dimension and wave count: the first refused radius is refused with the LDS message (0 and 2049 by the range check) and nothing is written; the next
    accepted call on the same plan -- the last accepted radius again -- is inside the bound.  (The refusals launch nothing, so the table of the accepted radius is
    never read at another one.)"""
    t, ref = truth(case)
    plan, dev = _plan(case, t)
    for R, msg in ((case["R"] + 1, "bytes of LDS"), (0, "out of range"), (2049, "out of range")):
        plan.p.rpe_radius = R
        _fill(plan)
        with pytest.raises(RuntimeError, match=msg):
            plan.backward()
        torch.cuda.synchronize()
        assert _untouched(plan), R
    plan.p.rpe_radius = case["R"]
    text, ok = check_backward(case, t, ref, plan, dev, stages=(False,))
    print(f"[radius] {case['id']} after the refusals: err / bound {text}")
    assert ok, case["id"]
