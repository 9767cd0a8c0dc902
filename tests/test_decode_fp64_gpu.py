"""The decode attention kernels (csrc/decode_kernels.h: decode_attn_kernel, decode_combine_kernel) per element against the fp64
restatement and the derived bound of tests/decode_fp64.py, at their structural edges: lengths around every row-group, pass and
split boundary at 1, 2, 5 and 128 splits, the automatic split at its maximum, keys that carry all of the softmax weight at the
places where the running maximum, the row-group merge and the split merge change hands, bias radii from 1 to 2048 with i.i.d.
tables, indexed cache reads with out-of-range entries, and element strides of q / k_new / v_new / o that no wrapper produces.

Every launch asserts: the bound per element of o and lse, the finiteness pattern of lse, the caches bit for bit against the expected
image after the append (padding included), cache_seqlens unchanged, and the same bits on a second run.

CASES and `launches` are module-level and CPU-only: tests/test_decode_fp64_cpu.py imports them and proves, without a GPU, that the
bound tells every mutant of decode_fp64.MUTANTS from the truth on these very inputs.
"""
import math
import zlib

import pytest
import torch

import decode_fp64 as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
SENT = -12288.0  # (exact in bf16 and fp16)
SPLITS = ((1, 1), (2, 2), (5, 5), (128, 128))   # (num_splits as passed, splits the kernel runs)
SPLITS_2 = ((1, 1), (5, 5))
CAP_MAX = 8256
SPOT_NATS = 40.0
WORST = {"o": (0.0, ""), "lse": (0.0, ""), "launches": 0}


def _name(dtype):
    return str(dtype)[6:]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rn(shape, dtype, g):
    return torch.randn(shape, generator=g).to(dtype)


def _table(H, R, g):
    """an i.i.d. bias generator: every entry distinct, so a wrong index shows"""
    return torch.randn(H, 2 * R + 1, generator=g)


def table_lengths(D, splits):
    """key counts around every boundary of the kernel at head dimension D and `splits` splits"""
    G, P = F.groups(D), F.wg_pass(D)
    Ls = {1, 2, G - 1, G, G + 1, P - 1, P, P + 1, 2 * P + 1}
    for c in (P, P + 1, 1):              # a split of exactly one pass, one pass + 1, a single key
        for r in (0, 1, c - 1):
            Ls.add(splits * c + r)
    Ls |= {splits - 1, max(1, splits // 2)}  # fewer keys than splits: empty splits
    return sorted(L for L in Ls if 1 <= L <= CAP_MAX - 1)


def _basic(g, B, H, D, dtype, cap, lens, append, R, scale, cacheB=None):
    ln = dict(q=_rn((B, 1, H, D), dtype, g), kc=_rn((cacheB or B, cap, H, D), dtype, g), vc=_rn((cacheB or B, cap, H, D), dtype, g),
              kn=_rn((B, 1, H, D), dtype, g) if append else None, vn=_rn((B, 1, H, D), dtype, g) if append else None,
              lens=list(lens), scale=scale, rpe=_table(H, R, g) if R else None, R=R, batch_idx=None, row_batch=None)
    return ln


def _launches_table(case, eff):
    D, dtype, append = case["D"], case["dtype"], case["append"]
    P = F.wg_pass(D)
    Ls = table_lengths(D, eff)
    if not append:
        Ls = [0] + Ls
    out = []
    for i in range(0, len(Ls), 4):
        batch = Ls[i:i + 4]
        g = _gen(case["id"], eff, i)
        out.append(_basic(g, len(batch), 2, D, dtype, min(CAP_MAX, max(batch) + 5), [L - append for L in batch], append, case["R"],
                          case["scale"]))
    C = 2 * P + 3   # a full cache (the append is skipped), a cache with one free row (the append fills it)
    out.append(_basic(_gen(case["id"], eff, "cap"), 4, 2, D, dtype, C, [C, C - 1, C - 2, 3], append, case["R"], case["scale"]))
    return out


def _launches_auto(case, eff):
    return [_basic(_gen(case["id"], n), 1, 4, 128, case["dtype"], CAP_MAX, [n], True, 128, 0.125) for n in (8191, 64)]


def spot_positions(D, L, append):
    """where one key holds all of the weight: per head; None = a plain head (the mutants must show there).  c is the split size at 5 splits."""
    G, P = F.groups(D), F.wg_pass(D)
    c = -(-L // 5)
    return [0, L - 1,                    # the first key; the last (the appended row, or the cache's last row)
            L - 2 if append else L - 3,  # the cache's last row under an append
            c - 1, c,                    # the last key of split 0, the first of split 1
            2 * c + P,                   # the first row group of a pass
            2 * c + P - 1,               # the last row group of a pass, last unrolled row
            L - 4,                       # the last pass of the last split
            None, None, None, None]


def _launches_spot(case, eff):
    D, dtype, append, mirror = case["D"], case["dtype"], case["append"], case["kind"] == "mirror"
    P = F.wg_pass(D)
    L = 5 * (P + 9) - 2   # five splits of two passes each; the last pass of the last split holds 7 keys
    pos = spot_positions(D, L, append)
    B, H = 4, len(pos)
    g = _gen(case["id"], eff)
    ln = _basic(g, B, H, D, dtype, L + 3, [L - append] * B, append, 2048 if mirror else 0, case["scale"])
    for h, j in enumerate(pos):
        if j is None:
            continue
        if mirror:   # every other key of this head SPOT_NATS below, through its own table entry (R >= L: nothing is clamped)
            ln["rpe"][h] -= SPOT_NATS
            ln["rpe"][h, 2048 + j - (L - 1)] += SPOT_NATS
            continue
        for b in range(B):
            q = ln["q"][b, 0, h].double()
            k = (SPOT_NATS / (ln["scale"] * float(q @ q)) * q).to(dtype)   # q . k * scale = SPOT_NATS (up to k's rounding)
            v = (3.0 + torch.randn(D, generator=g)).to(dtype)
            if append and j == L - 1:
                ln["kn"][b, 0, h], ln["vn"][b, 0, h] = k, v
            else:
                ln["kc"][b, j, h], ln["vc"][b, j, h] = k, v
    return [ln]


def _launches_radius(case, eff):
    L, R = case["L"], case["R"]
    return [_basic(_gen(case["id"], eff), 2, 4, case["D"], case["dtype"], L + 4, [L - 1, L - 8], True, R, case["scale"])]


def _launches_bidx(case, eff):
    out = []
    for i, (idx, lens) in enumerate((([2, 2, 0, 1], [300, 37, 129, 1]), ([-1, 3, 2 ** 31 - 1, 1], [5, 260, 130, 64]))):
        ln = _basic(_gen(case["id"], eff, i), 4, 4, case["D"], case["dtype"], 300, lens, False, 128, case["scale"], cacheB=3)
        ln["batch_idx"] = idx
        out.append(ln)
    return out


def _launches_rowmap(case, eff):
    B, cacheB, cap = 4, 5, 300
    g = _gen(case["id"], eff)
    ln = _basic(g, B, 4, case["D"], case["dtype"], cap, [298, 130, 2, 63], case["append"], 128, case["scale"], cacheB=cacheB)
    # a random parent table whose neighbouring entries differ; some entries out of range on either side (they clamp to 0 / cacheB - 1)
    t = torch.randint(1, cacheB, (B, cap), generator=g).cumsum(1) % cacheB
    pick = torch.rand(B, cap, generator=g) < 0.3
    big = torch.rand(B, cap, generator=g) < 0.5
    t = torch.where(pick & (t == 0), torch.where(big, torch.full_like(t, -2 ** 31), torch.full_like(t, -1)), t)
    t = torch.where(pick & (t == cacheB - 1), torch.where(big, torch.full_like(t, 2 ** 31 - 1), torch.full_like(t, cacheB)), t)
    ln["row_batch"] = t.int()
    return [ln]


def _launches_strided(case, eff):
    if case["kind"] == "fused":
        return [_basic(_gen(case["id"], eff), 3, 4, case["D"], case["dtype"], 200, [199, 64, 0], True, 128, case["scale"])]
    return [_basic(_gen(case["id"], eff), 3, 5, case["D"], case["dtype"], 160, [150, 1, 77], True, 128, case["scale"])]


_MAKERS = {"table": _launches_table, "auto": _launches_auto, "spot": _launches_spot, "mirror": _launches_spot,
           "radius": _launches_radius, "bidx": _launches_bidx, "rowmap": _launches_rowmap, "fused": _launches_strided,
           "abi": _launches_strided}


def launches(case, eff):
    """the launches of `case` at `eff` splits: dicts of CPU tensors (q, kc, vc, kn, vn, rpe, row_batch), lens, batch_idx, scale, R"""
    return _MAKERS[case["kind"]](case, eff)


def _build_cases():
    out = []

    def add(kind, D, dtype, splits=SPLITS_2, layout="blhd", entry="python", **kw):
        tag = "-".join(f"{k}{v}" for k, v in kw.items())
        out.append(dict(kind=kind, D=D, dtype=dtype, splits=splits, layout=layout, entry=entry,
                        id=f"{kind}-D{D}-{_name(dtype)}" + (f"-{tag}" if tag else ""), **kw))

    for dtype in (BF16, F16):
        for D in (64, 128):
            for append in (True, False):
                for R in (0, 128):
                    add("table", D, dtype, SPLITS, "bhld" if D == 128 else "blhd", append=append, R=R, scale=0.125 if append else 0.1)
                add("spot", D, dtype, append=append, scale=0.125)
            add("mirror", D, dtype, append=True, scale=0.1)
        add("auto", 128, dtype, ((0, 128),))
        for R, L in ((1, 300), (2048, 100), (2048, 4200), (3, 300)):
            add("radius", 64, dtype, R=R, L=L, scale=0.125)
        add("bidx", 64, dtype, scale=0.125)
        for append in (True, False):
            add("rowmap", 64, dtype, append=append, scale=0.1)
        for layout in ("blhd_pad", "bhld_pad"):
            add("fused", 64, dtype, layout=layout, entry="fused", scale=0.125)
        add("abi", 64, dtype, entry="abi", scale=0.125)
    return out


CASES = _build_cases()
RUNS = [(c, ns, eff) for c in CASES for ns, eff in c["splits"]]


def reference(case, ln, eff, mutant=None):
    return F.decode_ref(ln["q"], ln["kc"], ln["vc"], ln["kn"], ln["vn"], ln["lens"], ln["scale"], ln["rpe"], ln["R"], ln["batch_idx"],
                        ln["row_batch"], splits=eff, mutant=mutant)


# ------------------------------------------------------------------------------------------------------------------- the GPU side
def _place(t, layout):
    """a cache on the device in `layout`: (the (B, L, H, D) view, the buffer that holds it -- padding included)"""
    B, L, H, D = t.shape
    if layout == "blhd":
        buf = t.to(DEV)
        return buf, buf
    if layout == "bhld":
        buf = t.transpose(1, 2).contiguous().to(DEV)
        return buf.transpose(1, 2), buf
    if layout == "blhd_pad":   # padded row, head and element strides
        buf = torch.full((B, L + 3, H + 1, D + 8), SENT, dtype=t.dtype, device=DEV)
        view = buf[:, :L, :H, :D]
    else:
        buf = torch.full((B, H + 1, L + 3, D + 8), SENT, dtype=t.dtype, device=DEV)
        view = buf[:, :H, :L, :D].transpose(1, 2)
    view.copy_(t)
    return view, buf


def _padded(t):
    """(B, 1, H, D) -> the same values inside a (B, 1, H + 3, D + 8) buffer of sentinels: batch and head strides that are multiples
    of 8 but not H * D and D"""
    B, _, H, D = t.shape
    buf = torch.full((B, 1, H + 3, D + 8), SENT, dtype=t.dtype, device=DEV)
    view = buf[:, :, :H, :D]
    view.copy_(t)
    return view, buf


def _bits(t):
    return t.view(torch.int16) if t.dtype != torch.float32 else t.view(torch.int32)


def _ws_bytes(B, H, D, splits):
    """fat5_attn_decode_workspace_bytes at `splits` splits: (max, sum, o[D]) in fp32 per split, rounded up to 16 bytes"""
    return -(-B * H * splits * (D + 2) * 4 // 16) * 16 if splits > 1 else 0


class _Launch:
    def __init__(self, case, ln, num_splits, eff):
        from flasht5_amd import _lib
        from flasht5_amd import decode
        self.case, self.ln, self.num_splits, self.eff = case, ln, num_splits, eff
        self.kc, self.kbuf = _place(ln["kc"], case["layout"])
        self.vc, self.vbuf = _place(ln["vc"], case["layout"])
        self.k0, self.v0 = self.kbuf.clone(), self.vbuf.clone()
        self.lens = torch.tensor(ln["lens"], dtype=torch.int32, device=DEV)
        self.rpe = ln["rpe"].to(DEV) if ln["rpe"] is not None else None
        self.bidx = torch.tensor(ln["batch_idx"], dtype=torch.int32, device=DEV) if ln["batch_idx"] is not None else None
        self.rowmap = ln["row_batch"].to(DEV) if ln["row_batch"] is not None else None
        app = ln["kn"] is not None
        self.pads = []
        if case["entry"] == "fused":    # q, k, v as slices of one projection output: kernel-ready as they are, so never copied
            B, _, H, D = ln["q"].shape
            fused = torch.cat([ln["q"], ln["kn"], ln["vn"]], 2).to(DEV)
            self.q, self.kn, self.vn = fused[:, :, :H], fused[:, :, H:2 * H], fused[:, :, 2 * H:]
            for t in (self.q, self.kn, self.vn):
                assert not t.is_contiguous() and _lib.kernel_ready(t) and decode._ready(t) is t
        elif case["entry"] == "abi":
            (self.q, qb), (self.kn, kb), (self.vn, vb) = _padded(ln["q"]), _padded(ln["kn"]), _padded(ln["vn"])
            self.o, self.obuf = _padded(torch.zeros_like(ln["q"]))
            self.pads = [(b, b.clone()) for b in (qb, kb, vb)]
        else:
            self.q = ln["q"].to(DEV)
            self.kn, self.vn = (ln["kn"].to(DEV), ln["vn"].to(DEV)) if app else (None, None)

    def restore(self):
        self.kbuf.copy_(self.k0), self.vbuf.copy_(self.v0)

    def run(self):
        from flasht5_amd import _lib, decode, flash_attn_with_kvcache
        ln, R = self.ln, self.ln["R"]
        B, _, H, D = ln["q"].shape
        lib = _lib.load()
        if self.case["entry"] == "abi":
            self.obuf.fill_(SENT)
            lse = torch.full((B, H, 1), math.nan, dtype=torch.float32, device=DEV)
            p = decode._params(self.q, self.kc, self.vc, self.kn, self.vn, self.lens, self.o, lse, ln["scale"], self.rpe, R,
                               self.num_splits)
            for name, t in (("q", self.q), ("k_new", self.kn), ("v_new", self.vn), ("o", self.o)):
                st = tuple(getattr(p, name + "_stride"))
                assert st == (t.stride(0), t.stride(2)) and st != (H * D, D) and all(s % 8 == 0 for s in st), (name, st)
            need = lib.fat5_attn_decode_workspace_bytes(p)
            assert need == _ws_bytes(B, H, D, self.eff)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
            if need:
                p.workspace, p.workspace_bytes = ws.data_ptr(), need
            _lib.check(lib.fat5_attn_decode(p, _lib.stream_ptr(self.q.device)), "fat5_attn_decode")
            torch.cuda.synchronize()
            assert bool((self.obuf[:, :, H:] == SENT).all()) and bool((self.obuf[:, :, :H, D:] == SENT).all()), "o: padding written"
            for buf, before in self.pads:
                assert torch.equal(_bits(buf), _bits(before)), "an input buffer changed"
            return self.o.clone(), lse
        # the split count the library runs, through the workspace it asks for
        p = decode._params(self.q, self.kc, self.vc, self.kn, self.vn, self.lens, torch.empty_like(self.q), None, ln["scale"], self.rpe,
                           R, self.num_splits, self.bidx, self.rowmap)
        assert lib.fat5_attn_decode_workspace_bytes(p) == _ws_bytes(B, H, D, self.eff)
        o, lse = flash_attn_with_kvcache(self.q, self.kc, self.vc, self.kn, self.vn, self.lens, ln["scale"], self.rpe, R,
                                         return_lse=True, num_splits=self.num_splits, cache_batch_idx=self.bidx,
                                         cache_row_batch=self.rowmap)
        torch.cuda.synchronize()
        return o, lse


def _record(kind, ratio, what):
    if ratio > WORST[kind][0]:
        WORST[kind] = (ratio, what)


@pytest.mark.parametrize("case, num_splits, eff", RUNS, ids=[f"{c['id']}-s{ns}" for c, ns, _ in RUNS])
def test_decode_within_the_fp64_bound(case, num_splits, eff):
    worst_o = worst_l = 0.0
    for i, ln in enumerate(launches(case, eff)):
        what = f"{case['id']} splits {num_splits} launch {i} lens {ln['lens']}"
        ref = reference(case, ln, eff)
        bo, bl = F.decode_bound(ref, case["dtype"], case["D"], eff)
        run = _Launch(case, ln, num_splits, eff)
        o, lse = run.run()
        # the caches: the expected image after the append, bit for bit, padding included; the lengths: never written
        for got, want in ((run.kbuf, ref["kc"]), (run.vbuf, ref["vc"])):
            assert torch.equal(_bits(got), _bits(_place(want, case["layout"])[1])), f"{what}: cache image"
        assert torch.equal(run.lens.cpu(), torch.tensor(ln["lens"], dtype=torch.int32)), f"{what}: cache_seqlens written"
        run.restore()
        o2, lse2 = run.run()
        assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(lse), _bits(lse2)), f"{what}: a second run gives other bits"
        oc, lc = o[:, 0].cpu(), lse[:, :, 0].cpu()
        ro, rl, same = F.ratios(oc, lc, ref, bo, bl)
        worst_o, worst_l = max(worst_o, ro), max(worst_l, rl)
        WORST["launches"] += 1
        _record("o", ro, what)
        _record("lse", rl, what)
        assert same, f"{what}: finiteness pattern of lse: got {lc.tolist()} want {ref['lse'].tolist()}"
        if ro > 1.0 or rl > 1.0:
            eo = (oc.double() - ref["o"]).abs() / bo
            el = torch.nan_to_num((lc.double() - ref["lse"]).abs() / bl, nan=0.0)
            b, h, d = (int(x) for x in torch.nonzero(eo == eo.max())[0])
            lb, lh = (int(x) for x in torch.nonzero(el == el.max())[0])
            raise AssertionError(f"{what}: o err/bound {ro:.3f} at (b {b}, h {h}, d {d}): got {float(oc[b, h, d])!r} ref "
                                 f"{float(ref['o'][b, h, d])!r} bound {float(bo[b, h, d]):.3e}; lse err/bound {rl:.3f} at (b {lb}, h {lh}): "
                                 f"got {float(lc[lb, lh])!r} ref {float(ref['lse'][lb, lh])!r} bound {float(bl[lb, lh]):.3e}")
    print(f"[decode-fp64] {case['id']} splits {num_splits}: worst err / bound o {worst_o:.3f} lse {worst_l:.3f}")


def test_zz_summary():
    """(runs last) the worst err / bound of this session"""
    print(f"[decode-fp64] {WORST['launches']} launches: worst err / bound o {WORST['o'][0]:.3f} ({WORST['o'][1]}), "
          f"lse {WORST['lse'][0]:.3f} ({WORST['lse'][1]})")
    assert WORST["o"][0] <= 1.0 and WORST["lse"][0] <= 1.0
