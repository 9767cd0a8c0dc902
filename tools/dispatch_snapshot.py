"""Snapshot of the attention dispatch policy (host-only, no GPU needed): for a deterministic grid of problems, what
fat5_attn_describe, fat5_attn_bwd_workspace_bytes and fat5_attn_bwd_launches answer.

    python tools/dispatch_snapshot.py            # (re)write tests/dispatch_snapshot.txt from the library in the tree
    python tools/dispatch_snapshot.py --check    # compare instead; exit status 1 and the differing cases on a mismatch

tests/test_dispatch_snapshot_cpu.py runs the same comparison.  The snapshot holds the outputs only -- the cases come from
`cases()` below, in order -- with equal consecutive outputs grouped as "<count>x <output>".  A pull request that moves a dispatch
rule on purpose regenerates the file and shows the moved lines in its diff; a refactor must leave it untouched.  The lines hold
for the 256 compute units the rules were measured on (and for no device at all).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPSHOT = os.path.join(ROOT, "tests", "dispatch_snapshot.txt")

NONE, DENSE, RPE = 0, 1, 2
F16, BF16 = 1, 2
COLUMNS = ("fwd", "dq", "dkdv", "fused", "dbias", "qdiag", "[dtable=...]", "workspace_bytes", "launches")
PTR = 16  # a fake, 16-byte aligned device pointer: the policy follows none


def case(B, H, M, N, D=64, dtype=BF16, causal=0, mode=NONE, radius=128, variant=0, scale=None, dbias="shared", bias="shared",
         bias_base=PTR, unit=None, packed=None, grad="rpe1d"):
    """One problem as a plain dict (the snapshot's unit).  dbias: None / "shared" (1, H) / "full" (B, H) / "one" (1, 1);
    bias: "shared" / "perbatch" / "s2odd" (row stride no multiple of 8); grad: "rpe1d" / "table" / None (T5 bias)."""
    return dict(B=B, H=H, M=M, N=N, D=D, dtype=dtype, causal=causal, mode=mode, radius=radius, variant=variant, scale=scale, dbias=dbias,
                bias=bias, bias_base=bias_base, unit=unit, packed=packed, grad=grad)


def cases():
    out = []
    modes = (dict(mode=NONE), dict(mode=RPE), dict(mode=DENSE))
    # square problems over batch, heads, length, head_dim, mask and bias mode
    for m in modes:
        for D in (64, 128):
            for causal in (0, 1):
                for H in (8, 12):
                    for S in (128, 256, 384, 512, 640, 768, 1024, 1536, 2048, 3072, 3584, 4096, 8192):
                        for B in (1, 2, 4, 8, 16):
                            out.append(case(B, H, S, S, D=D, causal=causal, **m))
    # rectangular ones
    for m in modes:
        for causal in (0, 1):
            for B in (4, 16):
                for M in (512, 1024, 2048, 4096, 8192):
                    for N in (512, 1024, 2048, 4096, 8192):
                        if M != N:
                            out.append(case(B, 12, M, N, causal=causal, **m))
    # off the power-of-two grid: batch sizes and head counts
    for m in modes:
        for causal in (0, 1):
            for H in (1, 5, 16, 32):
                for S in (384, 512, 1024, 2048):
                    for B in (3, 5, 6, 7):
                        out.append(case(B, H, S, S, causal=causal, **m))
    # the remaining axes, one at a time around the headline shapes
    import flasht5_amd._lib as L
    bits = [1 << i for i in range(27)]  # every FAT5_V_* bit of include/fat5.h on its own
    pairs = [L.V_KV64_ON | L.V_KV64_HALF_ON | L.V_Q64_ON | L.V_FWD64_OFF, L.V_KV64_ON | L.V_KV64_MIX_ON, L.V_FWD64_ON | L.V_FWD64_KSPLIT_ON,
             L.V_FUSED64_ON | L.V_QDIAG_ON, L.V_QDB64_ON | L.V_FUSED64_ON]
    for S in (512, 1024, 2048, 4096, 8192):
        for m in modes:
            for causal in (0, 1):
                base = dict(B=4, H=12, M=S, N=S, causal=causal, **m)
                out.append(case(dtype=F16, **base))
                for D in (16, 32):
                    out.append(case(D=D, **base))
                for scale in (0.0, 1.3, 1e-6):
                    out.append(case(scale=scale, **base))
                    out.append(case(scale=scale, dtype=F16, **base))
                for v in bits + pairs:
                    out.append(case(variant=v, **base))
                out.append(case(unit=(8, 16), dbias="full", bias="perbatch", **base))
                if m["mode"] != DENSE:
                    out.append(case(packed=4 * S - 100, **base))
                if m["mode"] == RPE:
                    for R in (32, 600, 2048):
                        out.append(case(radius=R, **base))
                    for grad in (None, "table"):
                        out.append(case(grad=grad, **base))
                if m["mode"] == DENSE:
                    for dbias in (None, "full", "one"):
                        out.append(case(dbias=dbias, **base))
                    out.append(case(bias="perbatch", dbias="full", **base))
                    out.append(case(bias="perbatch", dbias="shared", **base))
                    out.append(case(bias="s2odd", **base))
                    out.append(case(bias_base=PTR + 8, **base))
                    out.append(case(D=128, dbias="shared", variant=L.V_DBIAS_INKERNEL, **base))
    return out


_keep = []  # host arrays the descriptors point to


def params(c):
    import flasht5_amd._lib as L
    p = L.AttnParams()
    p.B, p.H, p.M, p.N, p.D = c["B"], c["H"], c["M"], c["N"], c["D"]
    p.dtype, p.causal, p.bias_mode, p.variant = c["dtype"], c["causal"], c["mode"], c["variant"]
    p.sm_scale = float(c["D"]) ** -0.5 if c["scale"] is None else c["scale"]
    M, N, H, B = c["M"], c["N"], c["H"], c["B"]
    if c["mode"] == DENSE:
        p.bias = c["bias_base"]
        row = N + 4 if c["bias"] == "s2odd" else N
        p.bias_stride[0], p.bias_stride[1], p.bias_stride[2] = (H * M * row if c["bias"] == "perbatch" else 0), M * row, row
        if c["dbias"]:
            p.dbias = PTR
            p.dbias_batch, p.dbias_heads = {"shared": (1, H), "full": (B, H), "one": (1, 1)}[c["dbias"]]
    elif c["mode"] == RPE:
        p.rpe1d, p.rpe_radius = PTR, c["radius"]
        if c["grad"] == "rpe1d":
            p.drpe1d = PTR
        elif c["grad"] == "table":
            n1 = 2 * c["radius"] + 1
            host = (ctypes.c_int32 * n1)(*[i * 32 // n1 for i in range(n1)])
            _keep.append(host)
            p.rpe_bucket, p.drpe_table, p.rpe_num_buckets, p.rpe_bucket_host = PTR, PTR, 32, ctypes.addressof(host)
    if c["unit"]:
        p.unit_begin, p.unit_count = c["unit"]
    if c["packed"]:
        p.cu_seqlens_q = p.cu_seqlens_k = PTR
        p.total_q = p.total_k = c["packed"]
    return p


def answer(lib, c):
    p = params(c)
    buf = ctypes.create_string_buffer(256)
    rc = lib.fat5_attn_describe(ctypes.byref(p), buf, 256)
    if rc != 0:
        return f"error {rc}"
    text = buf.value.decode()
    for i, key in enumerate(COLUMNS[:6]):  # (the describe text's leading fields by position; a trailing dtable=... stays as it is)
        assert text.split()[i].startswith(key + "="), text
    text = " ".join(kv.split("=", 1)[1] if i < 6 else kv for i, kv in enumerate(text.split()))
    return f"{text} {lib.fat5_attn_bwd_workspace_bytes(ctypes.byref(p))} {lib.fat5_attn_bwd_launches(ctypes.byref(p))}"


def label(c):
    return " ".join(f"{k}={v}" for k, v in c.items())


def group(lines):
    """["a", "a", "b"] -> ["2x a", "1x b"]"""
    out, i = [], 0
    while i < len(lines):
        j = i
        while j < len(lines) and lines[j] == lines[i]:
            j += 1
        out.append(f"{j - i}x {lines[i]}")
        i = j
    return out


def ungroup(grouped):
    out = []
    for g in grouped:
        n, _, text = g.partition("x ")
        out.extend([text] * int(n))
    return out


def compare(lib):
    """[(case label, snapshot line, library's line)] for every case that differs (a length mismatch is one entry)"""
    cs = cases()
    want = ungroup([ln for ln in open(SNAPSHOT).read().splitlines() if not ln.startswith("#")])
    if len(want) != len(cs):
        return [("case count", str(len(want)), str(len(cs)))]
    return [(label(c), w, g) for c, w, g in zip(cs, want, (answer(lib, c) for c in cs)) if w != g]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import flasht5_amd._lib as L
    lib = L.load()
    if lib.fat5_chip_cus() != 256:
        sys.exit("the snapshot holds for a 256-CU device (or none): run this where fat5_chip_cus() is 256")
    if "--check" in sys.argv:
        bad = compare(lib)
        for lab, w, g in bad[:50]:
            print(f"{lab}\n  snapshot: {w}\n  library:  {g}")
        print(f"{len(cases())} cases, {len(bad)} differ")
        sys.exit(1 if bad else 0)
    lines = group([answer(lib, c) for c in cases()])
    with open(SNAPSHOT, "w") as f:
        f.write("# <count>x " + " ".join(COLUMNS) + "\n" + "\n".join(lines) + "\n")
    print(f"{len(cases())} cases -> {len(lines)} lines in {SNAPSHOT}")
