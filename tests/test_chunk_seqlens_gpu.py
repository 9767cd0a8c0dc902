"""Per-row chunk lengths of the chunk decode kernel (`chunk_seqlens` of flash_attn_with_kvcache_chunk / fat5_attn_decode_chunk): per
element against the fp64 restatement of tests/decode_chunk_fp64.py, wrapped so that batch element b brings only its first m_b rows,
under that file's own bound, unchanged.  Also asserted here: rows i >= m_b give o = 0 and lse = -inf exactly; cache rows outside
[len_b, len_b + m_b) keep their bits (guard rows on both sides of every batch element); None and full(M) give the same bits; a
captured launch replayed after the lengths moved on the device gives what an eager launch gives.

The shapes are the smallest at which the kernel can go wrong: B = 3, H = 2, M = 5 (two tiles of CHUNK_TQ = 4 rows, the second one
partial), chunk lengths (5, 2, 0) -- a whole chunk, one that ends inside the first tile, an empty one -- at cache lengths (0, 3, 11)
in a capacity of 16: row 0 is a pure prefill and row 2 appends nothing."""
import math
import zlib

import pytest
import torch

import decode_chunk_fp64 as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
B_, H_, M_, CAP = 3, 2, 5, 16
MLENS, LENS = (5, 2, 0), (0, 3, 11)
GUARD = 3
SCALE = 0.125


def _cases():
    out = []

    def add(kind, D, dtype, causal, R, append, lens=LENS, mlens=MLENS, splits=1):
        out.append(dict(kind=kind, D=D, dtype=dtype, causal=causal, R=R, append=append, lens=list(lens), mlens=list(mlens), splits=splits,
                        id=f"{kind}-D{D}-{str(dtype)[6:]}-{'causal' if causal else 'full'}-R{R}-{'append' if append else 'read'}-s{splits}"))

    for D in (64, 128):
        for dtype in (BF16, F16):
            for causal in (True, False):
                for R in (4, 0):
                    for append in (True, False):
                        add("base", D, dtype, causal, R, append)
        add("split", D, BF16, True, 4, True, splits=3)
        add("split", D, F16, False, 0, False, splits=2)
        # rows that do not all fit: 13 + 5 > 16 (three of five fit), 15 + 2 > 16 (one of two), a full cache with a length past M
        add("overflow", D, BF16, True, 4, True, lens=(13, 15, 16), mlens=(5, 2, 9))
        # lengths outside [0, M] are clamped on the device
        add("clamped", D, F16, True, 4, True, mlens=(7, -3, 1))
    return out


CASES = _cases()


def inputs(case):
    g = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    D, dtype = case["D"], case["dtype"]
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    ln = dict(q=rn(B_, M_, H_, D), kc=rn(B_, CAP, H_, D), vc=rn(B_, CAP, H_, D), kn=None, vn=None, rpe=None)
    if case["append"]:
        ln["kn"], ln["vn"] = rn(B_, M_, H_, D), rn(B_, M_, H_, D)
    if case["R"]:
        ln["rpe"] = torch.randn(H_, 2 * case["R"] + 1, generator=g)
    return ln


def rows(case):
    return [max(0, min(m, M_)) for m in case["mlens"]]


def ragged_ref(case, ln):
    """decode_chunk_fp64.chunk_ref with the rows i >= m_b dropped: batch element b is the restatement's launch of its first m_b rows
    (m_b stands for M in every rule of the contract); the dropped rows are o = 0, lse = -inf and see no key"""
    D = case["D"]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    out = dict(o=z(B_, M_, H_, D), lse=torch.full((B_, M_, H_), -math.inf, dtype=torch.float64), absv=z(B_, M_, H_, D),
               smag=z(B_, M_, H_), bmag=z(B_, M_, H_), srange=z(B_, M_, H_), nvis=[[0] * M_ for _ in range(B_)],
               kend=[[0] * M_ for _ in range(B_)], kc=ln["kc"].clone(), vc=ln["vc"].clone())
    for b, m in enumerate(rows(case)):
        if m == 0:
            continue
        cut = lambda t: None if t is None else t[b:b + 1, :m]  # noqa: E731
        r = C.chunk_ref(cut(ln["q"]), ln["kc"][b:b + 1], ln["vc"][b:b + 1], cut(ln["kn"]), cut(ln["vn"]), [case["lens"][b]], SCALE,
                        case["causal"], ln["rpe"], case["R"], splits=case["splits"])
        for name in ("o", "lse", "absv", "smag", "bmag", "srange"):
            out[name][b, :m] = r[name][0]
        out["nvis"][b][:m], out["kend"][b][:m] = r["nvis"][0], r["kend"][0]
        out["kc"][b], out["vc"][b] = r["kc"][0], r["vc"][0]
    return out


def _bits(t):
    return t.view(torch.int16) if t.dtype != torch.float32 else t.view(torch.int32)


def _guarded(t):
    B, cap, H, D = t.shape
    buf = torch.randn(B, cap + 2 * GUARD, H, D, generator=torch.Generator().manual_seed(cap)).to(t.dtype).to(DEV)
    view = buf[:, GUARD:GUARD + cap]
    view.copy_(t)
    return view, buf


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _run(case, ln, kc, vc, lens, mlens):
    from flasht5_amd import flash_attn_with_kvcache_chunk
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    o, lse = flash_attn_with_kvcache_chunk(dev(ln["q"]), kc, vc, dev(ln["kn"]), dev(ln["vn"]), lens, SCALE, case["causal"], dev(ln["rpe"]),
                                           case["R"], return_lse=True, num_splits=case["splits"], chunk_seqlens=mlens)
    torch.cuda.synchronize()
    return o, lse


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_ragged_chunk_within_the_fp64_bound(case):
    ln = inputs(case)
    ref = ragged_ref(case, ln)
    (kc, kbuf), (vc, vbuf) = _guarded(ln["kc"]), _guarded(ln["vc"])
    k0, v0 = kbuf.clone(), vbuf.clone()
    lens, mlens = _i32(case["lens"]), _i32(case["mlens"])
    o, lse = _run(case, ln, kc, vc, lens, mlens)
    assert o.shape == (B_, M_, H_, case["D"]) and lse.shape == (B_, H_, M_)
    bo, bl = C.chunk_bound(ref, case["dtype"], case["D"], case["splits"])
    ro, rl, same = C.ratios(o.cpu(), lse.cpu().transpose(1, 2), ref, bo, bl)
    print(f"[chunk-seqlens] {case['id']}: worst err / bound o {ro:.3f} lse {rl:.3f}")
    assert same, f"{case['id']}: finiteness pattern of lse: got {lse.cpu().transpose(1, 2).tolist()}"
    assert ro <= 1.0 and rl <= 1.0, f"{case['id']}: err / bound o {ro:.3f} lse {rl:.3f}"
    # rows the batch element does not bring: exactly zero, exactly -inf
    for b, m in enumerate(rows(case)):
        assert bool((_bits(o[b, m:]) == 0).all()) and bool((lse[b, :, m:] == -math.inf).all()), (case["id"], b)
    # the caches: rows [len_b, len_b + a_b) hold the new rows bit for bit, every other element -- rows past them, the other batch
    # elements, the guard rows -- is what it was; neither length vector is written
    wk, wv = k0.clone(), v0.clone()
    wk[:, GUARD:GUARD + CAP], wv[:, GUARD:GUARD + CAP] = ref["kc"].to(DEV), ref["vc"].to(DEV)
    assert torch.equal(_bits(kbuf), _bits(wk)) and torch.equal(_bits(vbuf), _bits(wv)), f"{case['id']}: cache image"
    if case["append"]:
        for b, m in enumerate(rows(case)):
            n = max(0, min(case["lens"][b], CAP))
            a = min(m, CAP - n)
            assert torch.equal(_bits(kc[b, n:n + a]), _bits(ln["kn"][b, :a].to(DEV)))
            assert torch.equal(_bits(kbuf[b, GUARD + n + a:]), _bits(k0[b, GUARD + n + a:])), "a row at or past len_b + m_b was written"
    else:
        assert torch.equal(_bits(kbuf), _bits(k0)) and torch.equal(_bits(vbuf), _bits(v0))
    assert lens.tolist() == case["lens"] and mlens.tolist() == case["mlens"]


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] in ("base", "split") and c["dtype"] == BF16 and c["R"]],
                         ids=lambda c: c["id"])
def test_none_and_full_lengths_give_the_same_bits(case):
    ln = inputs(case)
    lens = _i32(case["lens"])
    res = []
    for mlens in (None, _i32([M_] * B_)):
        (kc, kbuf), (vc, vbuf) = _guarded(ln["kc"]), _guarded(ln["vc"])
        o, lse = _run(case, ln, kc, vc, lens, mlens)
        res.append((o, lse, kbuf, vbuf))
    for x, y in zip(*res):
        assert torch.equal(_bits(x), _bits(y)), case["id"]


@pytest.mark.parametrize("append", [True, False])
def test_graph_replay_after_the_lengths_move_equals_eager(append):
    from flasht5_amd import flash_attn_with_kvcache_chunk
    case = dict(id=f"graph-{append}", D=64, dtype=BF16, append=append, R=4)
    ln = {k: (None if v is None else v.to(DEV)) for k, v in inputs(case).items()}
    lens, mlens = _i32(LENS), _i32(MLENS)
    kc, vc = ln["kc"].clone(), ln["vc"].clone()
    call = lambda k_, v_: flash_attn_with_kvcache_chunk(ln["q"], k_, v_, ln["kn"], ln["vn"], lens, SCALE, True, ln["rpe"], 4,  # noqa: E731
                                                        return_lse=True, num_splits=2, chunk_seqlens=mlens)
    call(kc.clone(), vc.clone())   # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = call(kc, vc)
    graph.replay()
    torch.cuda.synchronize()
    ks, vs = kc.clone(), vc.clone()
    lens.copy_(_i32([2, 9, 4]))     # on the device: both vectors move, the empty row now brings a whole chunk
    mlens.copy_(_i32([1, 3, 5]))
    graph.replay()
    torch.cuda.synchronize()
    oe, le = call(ks, vs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(oe)) and torch.equal(_bits(lse), _bits(le))
    assert torch.equal(_bits(kc), _bits(ks)) and torch.equal(_bits(vc), _bits(vs))
    assert bool((_bits(o[0, 1:]) == 0).all()) and bool((lse[0, :, 1:] == -math.inf).all())
    if append:
        assert bool(torch.isfinite(lse[2]).all())
        assert torch.equal(_bits(kc[2, 4:9]), _bits(ln["kn"][2])) and torch.equal(_bits(kc[0, 2:3]), _bits(ln["kn"][0, :1]))
    del graph


def test_conversion_and_capture_rule():
    """an int64 / CPU chunk_seqlens is converted like cache_seqlens -- except inside a capture, where it must be int32 on the device"""
    from flasht5_amd import flash_attn_with_kvcache_chunk
    q = torch.randn(2, 3, 2, 64, device=DEV).to(BF16)
    kc = torch.randn(2, 16, 2, 64, device=DEV).to(BF16)
    lens = _i32([3, 5])
    a = flash_attn_with_kvcache_chunk(q, kc.clone(), kc.clone(), q, q, lens, causal=True, chunk_seqlens=torch.tensor([2, 3]))
    b = flash_attn_with_kvcache_chunk(q, kc.clone(), kc.clone(), q, q, lens, causal=True, chunk_seqlens=_i32([2, 3]))
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="contiguous int32 tensor on"):
        torch.ops.fat5.attn_decode_chunk(q, kc, kc.clone(), q, q, lens, SCALE, True, None, 0, False, 0, torch.tensor([2, 3], dtype=torch.int32))
    bad = torch.tensor([2, 3], device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="graph capture chunk_seqlens"):
        with torch.cuda.graph(graph):
            flash_attn_with_kvcache_chunk(q, kc, kc, q, q, lens, chunk_seqlens=bad)
    del graph
