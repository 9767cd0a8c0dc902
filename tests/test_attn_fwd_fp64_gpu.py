"""The attention forward (csrc/attn_fwd.h, csrc/attn_fwd64.h) per element of o and lse against the fp64 restatement and the derived
bound of tests/attn_fwd_fp64.py, in every forward body `fat5_attn_describe` names: the 32-row body at two and four waves, its
two-waves-per-32-rows split form, the 64-row pipelined body at D = 64 as 256-row workgroups, as key-split 128-row workgroups and as both
in one launch, the 64-row body at D = 128 (the "spread" launch, and the 256-row one from 257 workgroups on), and the dense-bias 64-row
bodies at D = 64 and D = 128.  Shapes are the smallest at which each body's structure exists: rows and keys around every 32 / 64 / 128 /
256 boundary, shorter than a block, one 4-tile trip plus remainder tiles, masked tails, T5 tables of radius 1, 8 and 128 whose band edges
sweep over block and tile boundaries, bottom-right causal masks with N - M in {0, 1, 100, -1, -100}, dense biases of every broadcast kind
and one holding finfo.min.  The value rows at key 0, key N - 1 and the block seam carry 32 times the magnitude of the others, so that one
dropped key there moves o beyond the bound (tests/test_attn_fwd_fp64_cpu.py proves that on these very inputs, without a GPU).

Every case asserts the body through `_lib.describe` before it launches (describe does not expose the wave count of the 32-row body: the
four-wave cases are the ones with 160 workgroups or more, csrc/attn_dispatch.h pick_nw; eight waves are never chosen by the dispatcher).
Inputs that send a pipelined body through its exact second pass are left to the max-norm tests (tests/test_fwd64_gpu.py).

CASES and `inputs` are module-level and CPU-only.
"""
import math
import zlib

import pytest
import torch

import attn_fwd_fp64 as F
from oracle.rpe import relative_position_bucket

BF16, F16 = torch.bfloat16, torch.float16
BOOST = 32.0
WORST = {}   # body -> [launches, worst o ratio, its case, worst lse ratio, its case]

# fat5_variant bits by name (flasht5_amd/_lib.py), resolved on the GPU side
OFF32 = ("V_NO_SPLIT", "V_FWD64_OFF")
ROWS256 = ("V_FWD64_ON", "V_FWD64_KSPLIT_OFF", "V_FWD64_MIX_OFF")
KSPLIT = ("V_FWD64_ON", "V_FWD64_KSPLIT_ON")
MIXED = ("V_FWD64_ON", "V_FWD64_MIX_ON")
ON64 = ("V_FWD64_ON",)
DENSE_KINDS = ("11", "1h", "b1", "bh")


def _name(dtype):
    return str(dtype)[6:]


def _build_cases():
    out = []

    def add(group, body, bits, B, H, M, N, D, dtype, causal=False, bias="none", R=0, scale=None, strided=False):
        cid = f"{group}-{B}x{H}x{M}x{N}-D{D}-{_name(dtype)}-{bias}{R if R else ''}{'-causal' if causal else ''}{'-strided' if strided else ''}"
        out.append(dict(id=cid, group=group, body=body, bits=bits, B=B, H=H, M=M, N=N, D=D, dtype=dtype, causal=causal, bias=bias, R=R,
                        scale=float(D) ** -0.5 if scale is None else scale, strided=strided))

    # ---- 32-row body, two waves (fewer than 160 workgroups) ----
    Ms, Ns = (1, 31, 32, 33, 64, 65, 129), (1, 63, 64, 65, 127, 128, 129, 200)
    i = 0
    for j, N in enumerate(Ns):
        for M in (Ms[j % 7], Ms[(3 * j + 2) % 7]):
            bias = ("none", "rpe", "1h", "rpe", "bh", "none")[i % 6]
            add("r32w2", "32row", OFF32, 1 + i % 2, 2, M, N, (16, 32, 64, 128)[i % 4], (BF16, F16)[(i // 2) % 2], causal=i % 5 in (1, 3),
                bias=bias, R=(8, 128, 1)[i % 3] if bias == "rpe" else 0, strided=i % 4 == 0)
            i += 1
    # ---- 32-row body, four waves (160 workgroups) ----
    for i, (M, N, D, bias) in enumerate(((33, 129, 64, "rpe"), (128, 200, 32, "none"), (65, 64, 64, "1h"), (129, 65, 128, "none"))):
        add("r32w4", "32row", OFF32, 2, 80, M, N, D, (BF16, F16)[i % 2], causal=i == 1, bias=bias, R=8 if bias == "rpe" else 0, strided=i == 0)
    # ---- 32-row split: chosen by itself ----
    for i, N in enumerate((128, 129, 160, 191, 192, 193)):
        bias = ("none", "rpe", "1h")[i % 3]
        add("split", "32row-split", (), 4, 12, 128, N, 64, (BF16, F16)[i % 2], causal=i in (2, 5), bias=bias, R=128 if bias == "rpe" else 0,
            strided=i == 1)
    add("split", "32row-split", (), 4, 12, 100, 200, 64, BF16, bias="rpe", R=8)
    add("split", "32row-split", (), 4, 12, 100, 200, 64, F16, causal=True)
    # ---- 64-row body, D = 64: 256-row workgroups and key-split ----
    Ms = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
    Ns = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 320, 513)
    for f, (group, body, bits) in enumerate((("r64", "64row", ROWS256), ("ksplit", "64row-ksplit", KSPLIT))):
        for j, N in enumerate(Ns):
            i = j + f
            bias = ("none", "rpe")[i % 2]
            add(group, body, bits, 1, 2, Ms[(2 * j + 1 + 5 * f) % 11], N, 64, (BF16, F16)[(i // 2) % 2], causal=i % 3 == 2, bias=bias,
                R=(128, 8)[(i // 2) % 2] if bias == "rpe" else 0, strided=j % 4 == 0)
    add("r64", "64row", ROWS256, 1, 2, 129, 320, 64, BF16, scale=1.0)      # |sm_scale| sqrt(D) >= 8: the first tile's row maxima as reference point in bf16 too
    add("ksplit", "64row-ksplit", KSPLIT, 1, 2, 129, 320, 64, BF16, scale=1.0)
    # ---- 64-row mixed: 256-row and key-split workgroups in one launch ----
    for i, (M, N) in enumerate(((384, 256), (385, 321), (640, 640), (700, 256), (700, 321))):
        bias = ("none", "rpe")[i % 2]
        add("mixed", "64row-mixed", MIXED, 1, 8, M, N, 64, (BF16, F16)[(i // 2) % 2], bias=bias, R=128 if bias == "rpe" else 0, strided=i == 0)
    # ---- 64-row body, D = 128: "spread" (at most 256 workgroups) and 256-row launches ----
    for i, (M, N) in enumerate(((1, 1), (63, 33), (64, 64), (65, 257), (129, 31), (257, 320), (300, 513), (256, 255))):
        bias = ("none", "rpe")[i % 2]
        add("d128", "64row", ON64, 1, 2, M, N, 128, (BF16, F16)[(i // 2) % 2], causal=i % 3 == 2, bias=bias, R=(128, 8)[(i // 2) % 2] if bias == "rpe" else 0,
            strided=i == 3)
    add("d128w", "64row", ON64, 257, 1, 65, 65, 128, BF16, bias="rpe", R=8)
    add("d128w", "64row", ON64, 257, 1, 33, 129, 128, F16, causal=True)
    # ---- dense-bias 64-row bodies, bf16 ----
    for D in (64, 128):
        for i, (M, N) in enumerate(((65, 64), (129, 256), (300, 328), (256, 512))):
            add(f"dense{D}", "64row", ON64, 2, 2, M, N, D, BF16, causal=i % 2 == 1, bias=DENSE_KINDS[i], strided=i == 2)
            add(f"dense{D}", "64row", ON64, 2, 2, M + 1, N + 8, D, BF16, causal=i % 2 == 0, bias=DENSE_KINDS[3 - i])
        add(f"dense{D}", "32row", ON64, 2, 2, 65, 63, D, BF16, bias="1h")                 # N % 8 != 0: the rows cannot travel by LDS-DMA
        add(f"dense{D}", "64row", ON64, 1, 2, 130, 192, D, BF16, bias="1h-min")           # finfo.min on half the keys, and on all keys of some rows
    # ---- T5 tables: radius 1, 8, 128; the band edges n - m = +-R sweep over the block and tile boundaries as m runs ----
    i = 0
    for group, body, bits, B, H, D in (("r32w2", "32row", OFF32, 1, 2, 64), ("split", "32row-split", (), 4, 12, 64), ("r64", "64row", ROWS256, 1, 2, 64),
                                       ("ksplit", "64row-ksplit", KSPLIT, 1, 2, 64), ("d128", "64row", ON64, 1, 2, 128)):
        for R in (1, 8, 128):
            M, N = (128, 330) if group == "split" else ((200, 330) if R == 128 else (100 + 31 * (i % 2), 140 + R))
            add(group, body, bits, B, H, M, N, D, (BF16, F16)[i % 2], bias=("t5b", "t5u")[(i + i // 3) % 2], R=R)
            i += 1
    # ---- causal, bottom-right: N - M in {0, 1, 100, -1, -100}; with the T5 table (inside the band it carries the mask in the 64-row bodies) and without ----
    i = 0
    for group, body, bits, B, H, D, base in (("r32w2", "32row", OFF32, 1, 2, 64, 129), ("split", "32row-split", (), 4, 12, 64, 128),
                                             ("r64", "64row", ROWS256, 1, 2, 64, 192), ("ksplit", "64row-ksplit", KSPLIT, 1, 2, 64, 192),
                                             ("d128", "64row", ON64, 1, 2, 128, 129), ("dense64", "64row", ON64, 2, 2, 64, 136)):
        for d in ((0, 8, 104, -8, -104) if group == "dense64" else (0, 1, 100, -1, -100)):   # (dense: N % 8 == 0)
            M, N = (base, base + d) if d >= 0 else (base - d, base)
            bias = ("1h", "bh")[i % 2] if group == "dense64" else ("rpe", "none")[i % 2]
            add(group, body, bits, B, H, M, N, D, BF16 if group == "dense64" else (BF16, F16)[(i // 2) % 2], causal=True, bias=bias,
                R=(128, 8)[(i // 4) % 2] if bias == "rpe" else 0)
            i += 1
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _build_cases()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def inputs(case):
    """CPU tensors of a case: q, k, v (strided views where the case says so), bias (dense, in the dtype) or None, rpe (H, 2R + 1) fp32 or None"""
    B, H, M, N, D, dtype = (case[x] for x in ("B", "H", "M", "N", "D", "dtype"))
    g = _gen(case["id"])

    def rnd(S):
        if case["strided"]:   # the model's layout: (B, S, H, D) storage viewed as (B, H, S, D)
            return torch.randn(B, S, H, D, generator=g).to(dtype).permute(0, 2, 1, 3)
        return torch.randn(B, H, S, D, generator=g).to(dtype)

    q, k, v = rnd(M), rnd(N), rnd(N)
    if case["scale"] * math.sqrt(D) >= 8:
        q = (q.float() * 0.125).to(dtype)   # (an exact scaling: the scores stay those of the usual scale)
    for j in {0, N - 1, F.seam_key(N)} - {None}:   # the structural keys carry BOOST times the others' magnitude
        v[:, :, j] = (v[:, :, j].float() * BOOST).to(dtype)
    bias = rpe = None
    kind = case["bias"]
    if kind == "rpe":      # an i.i.d. generator: every entry distinct, so a wrong index shows
        rpe = torch.randn(H, 2 * case["R"] + 1, generator=g)
    elif kind in ("t5b", "t5u"):   # a T5 table through its bucket map (bidirectional / unidirectional), clamped at R
        R = case["R"]
        table = torch.randn(32, H, generator=g)
        bucket = relative_position_bucket(torch.arange(-R, R + 1).numpy(), kind == "t5b", 32, 128)
        rpe = table[torch.from_numpy(bucket)].T.contiguous()
    elif kind != "none":
        shape = {"11": (1, 1), "1h": (1, H), "b1": (B, 1), "bh": (B, H)}[kind[:2]]
        bias = torch.randn(*shape, M, N, generator=g).to(dtype)
        if kind.endswith("-min"):
            bias[..., N // 2:] = torch.finfo(dtype).min
            bias[:, :, 7::64, :] = torch.finfo(dtype).min
    return dict(q=q, k=k, v=v, bias=bias, rpe=rpe)


def reference(case, t, mutant=None):
    return F.attn_fwd_ref(t["q"], t["k"], t["v"], case["scale"], case["causal"], t["bias"], t["rpe"], case["R"], mutant=mutant)


def describe(case):
    """the forward body the library would run this case with"""
    from flasht5_amd import _lib
    bits = 0
    for name in case["bits"]:
        bits |= getattr(_lib, name)
    mode = _lib.BIAS_NONE if case["bias"] == "none" else (_lib.BIAS_RPE1D if case["R"] else _lib.BIAS_DENSE)
    d = _lib.describe(case["B"], case["H"], case["M"], case["N"], case["D"], _lib.dtype_code(case["dtype"]), case["causal"], mode, case["R"],
                      variant=bits, sm_scale=case["scale"])
    return d["fwd"], bits


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_forward_within_the_fp64_bound(case):
    from flasht5_amd import _lib
    from flasht5_amd.flash_attention_v2_bias import _attn_fwd
    body, bits = describe(case)
    assert body == case["body"], f"{case['id']}: the dispatcher runs '{body}', the case is meant for '{case['body']}'"
    t = inputs(case)
    ref = reference(case, t)
    bo, bl = F.attn_fwd_bound(ref, case["dtype"], case["D"], body, case["N"])
    dev = {key: (x.to("cuda") if x is not None else None) for key, x in t.items()}
    if case["strided"]:
        assert dev["q"].stride() == t["q"].stride() and dev["v"].stride() == t["v"].stride() and _lib.kernel_ready(dev["q"])   # (never copied)
    with _lib.variant(bits):
        o, lse = _attn_fwd(dev["q"], dev["k"], dev["v"], dev["bias"], dev["rpe"], case["R"], case["causal"], case["scale"])
    torch.cuda.synchronize()
    oc, lc = o.cpu(), lse.cpu()
    ro, rl, same = F.ratios(oc, lc, ref, bo, bl)
    w = WORST.setdefault(case["group"] + " (" + body + ")", [0, 0.0, "", 0.0, ""])
    w[0] += 1
    if ro > w[1]:
        w[1], w[2] = ro, case["id"]
    if rl > w[3]:
        w[3], w[4] = rl, case["id"]
    print(f"[attn-fwd-fp64] {case['id']}: err / bound o {ro:.3f} lse {rl:.3f}")
    assert same, f"{case['id']}: the finiteness pattern of lse differs from the reference's"
    if ro > 1.0 or rl > 1.0:
        eo = (oc.double() - ref["o"]).abs() / bo
        eo = torch.nan_to_num(eo, nan=0.0)
        el = torch.nan_to_num((lc.double() - ref["lse"]).abs() / bl, nan=0.0, posinf=0.0)
        b, h, m, d = (int(x) for x in torch.nonzero(eo == eo.max())[0])
        lb, lh, lm = (int(x) for x in torch.nonzero(el == el.max())[0])
        raise AssertionError(f"{case['id']}: o err/bound {ro:.3f} at (b {b}, h {h}, m {m}, d {d}): got {float(oc[b, h, m, d])!r} ref "
                             f"{float(ref['o'][b, h, m, d])!r} bound {float(bo[b, h, m, d]):.3e}; lse err/bound {rl:.3f} at (b {lb}, h {lh}, m {lm}): "
                             f"got {float(lc[lb, lh, lm])!r} ref {float(ref['lse'][lb, lh, lm])!r} bound {float(bl[lb, lh, lm]):.3e}")


@pytest.mark.gpu
def test_zz_summary():
    """(runs last) one line per body: the launches and the worst err / bound of this session"""
    for body, (n, ro, co, rl, cl) in sorted(WORST.items()):
        print(f"[attn-fwd-fp64] {body}: {n} launches, worst err/bound o {ro:.3f} ({co}), lse {rl:.3f} ({cl})")
    assert all(w[1] <= 1.0 and w[3] <= 1.0 for w in WORST.values())
