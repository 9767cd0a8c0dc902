"""The FP8 KV cache on the GPU: the row quantiser and the decode kernels' appends bit for bit against the restatement of
tests/kvfp8_ref.py (torch.equal on bytes and on scales), and attention over FP8 caches against fp64 attention over the dequantised
cache contents AFTER the call, inside the derived per-element bound of decode_fp64 / decode_chunk_fp64 extended by the two roundings
the FP8 path adds (kvfp8_ref's docstring).  The `[kvfp8] ...` lines (worst error / bound per case) are what DESIGN 4.17 records."""
import math

import pytest
import torch

import decode_chunk_fp64 as C
import decode_fp64 as F
import kvfp8_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
SENT_B, SENT_S = 0x55, -777.0   # what the guard rows hold


def _pass(D):
    return F.wg_pass(D)   # rows one workgroup takes per step: 128 at D = 64, 64 at D = 128


class Cache:
    """an FP8 cache pair of (B, cap, H, D) views with their (B, cap, H) scales, in either storage layout, one guard row before
    and after every sequence (bytes 0x55, scales -777) so that a write outside [0, cap) shows"""

    def __init__(self, B, cap, H, D, layout, fill=None):
        self.shape, self.layout = (B, cap, H, D), layout
        self.buf, self.sbuf, self.view, self.sview = [], [], [], []
        for i in range(2):
            if layout == "blhd":
                buf = torch.full((B, cap + 2, H, D), SENT_B, dtype=torch.uint8, device=DEV)
                sbuf = torch.full((B, cap + 2, H), SENT_S, dtype=torch.float32, device=DEV)
                v, sv = buf[:, 1:-1], sbuf[:, 1:-1]
            else:
                buf = torch.full((B, H, cap + 2, D), SENT_B, dtype=torch.uint8, device=DEV)
                sbuf = torch.full((B, H, cap + 2), SENT_S, dtype=torch.float32, device=DEV)
                v, sv = buf[:, :, 1:-1].transpose(1, 2), sbuf[:, :, 1:-1].transpose(1, 2)
            v.zero_()
            sv.zero_()
            if fill is not None:
                b, s = fill[i]
                v.copy_(b.view(torch.uint8))
                sv.copy_(s)
            self.buf.append(buf), self.sbuf.append(sbuf), self.view.append(v.view(FP8)), self.sview.append(sv)
        (self.k, self.v), (self.ks, self.vs) = self.view, self.sview

    def guards_intact(self):
        for buf, sbuf in zip(self.buf, self.sbuf):
            g = (buf[:, [0, -1]], sbuf[:, [0, -1]]) if self.layout == "blhd" else (buf[:, :, [0, -1]], sbuf[:, :, [0, -1]])
            if not (bool((g[0] == SENT_B).all()) and bool((g[1] == SENT_S).all())):
                return False
        return True

    def cpu(self):
        return self.k.cpu().contiguous(), self.ks.cpu().contiguous(), self.v.cpu().contiguous(), self.vs.cpu().contiguous()

    def kw(self):
        return dict(k_scale=self.ks, v_scale=self.vs)


def _rand_rows(shape, dtype, seed, spread=4.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * (torch.rand(shape[:-1] + (1,), generator=g) * spread + 0.05)).to(dtype)


# --------------------------------------------------------------------------------------------------------------- the quantiser
def _quantiser_rows(D, dtype):
    """(rows, D): normal rows, tiny ones, zeros, one element at +-amax, the format's ties and subnormals under s = 1, non-finite rows"""
    g = torch.Generator().manual_seed(D)
    normal = torch.randn(40, D, generator=g) * torch.logspace(-2, 2, 40).unsqueeze(1)
    tiny = torch.randn(4, D, generator=g) * 1e-20 if dtype == torch.bfloat16 else torch.randn(4, D, generator=g) * 3e-6
    zeros = torch.zeros(2, D)
    one = torch.zeros(4, D)
    one[0, 0], one[1, D - 1], one[2, 7], one[3, 8] = 3.0, -3.0, 1e-3, -65504.0 if dtype == torch.float16 else -3e38
    # s = 1 rows (the first element is 448): every e4m3fn value, every midpoint between neighbours (the ties), and points just off them
    v = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    v = torch.sort(v[(v >= 0) & ~torch.isnan(v)]).values
    mid = (v[:-1] + v[1:]) / 2
    def s1_rows(pts):
        pts = torch.cat((pts, torch.zeros((-len(pts)) % (D - 1)))).view(-1, D - 1)
        return torch.cat((torch.full((pts.shape[0], 1), 448.0), pts), 1)
    exact = s1_rows(torch.cat((v, -v, mid, -mid, torch.tensor([2.0 ** -10, 3 * 2.0 ** -11, 2.0 ** -11]))))
    near = s1_rows(torch.cat((mid * (1 + 2.0 ** -7), -mid * (1 - 2.0 ** -7))))   # (just off the ties, as the input dtype rounds them)
    bad = torch.ones(4, D)
    bad[0, 5], bad[1, 0], bad[2, D - 1], bad[3, 1], bad[3, 2] = float("nan"), float("inf"), float("-inf"), float("nan"), float("inf")
    rows = torch.cat((normal, tiny, zeros, one, exact, near, bad)).to(dtype)
    assert torch.equal(rows[50:50 + exact.shape[0]].float(), exact), "the tie points must be exact in the input dtype"
    return rows


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantiser_equals_the_restatement(dtype, D):
    from flasht5_amd import quantize_kv
    rows = _quantiser_rows(D, dtype)
    H = 2
    n = rows.shape[0] // (2 * H) * (2 * H)
    x = rows[:n].view(2, n // (2 * H), H, D).clone()                          # (B, L, H, D)
    x[1, -1] = rows[-2:]                                                      # (the non-finite rows are at the end: keep them in)
    xs = rows                                                                 # (rows, D)
    wb, ws = R.quantize_ref(x)
    b, s = quantize_kv(x.to(DEV))
    assert b.dtype == FP8 and s.dtype == torch.float32 and b.shape == x.shape and s.shape == x.shape[:3]
    assert R.same_bits(b.cpu(), s.cpu(), wb, ws)
    b2, s2 = quantize_kv(xs.to(DEV))
    assert b2.shape == xs.shape and s2.shape == xs.shape[:1] and R.same_bits(b2.cpu(), s2.cpu(), *R.quantize_ref(xs))
    # strided inputs and outputs in both cache layouts, guard rows around them
    B, L = x.shape[:2]
    for lay_in in ("blhd", "bhld"):
        xin = x.to(DEV) if lay_in == "blhd" else x.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
        for lay_out in ("blhd", "bhld"):
            c = Cache(B, L, H, D, lay_out)
            quantize_kv(xin, out=c.k, scale=c.ks)
            assert R.same_bits(c.k.cpu().contiguous(), c.ks.cpu().contiguous(), wb, ws), (lay_in, lay_out)
            assert c.guards_intact()
    # a slice with a row stride: every second position
    b3, s3 = quantize_kv(x.to(DEV)[:, ::2])
    assert R.same_bits(b3.cpu(), s3.cpu(), wb[:, ::2].contiguous(), ws[:, ::2].contiguous())
    # no rows: nothing happens; and a second run gives the same bits
    e, es = quantize_kv(x.to(DEV)[:, :0])
    assert e.shape == (B, 0, H, D) and es.shape == (B, 0, H)
    b4, s4 = quantize_kv(x.to(DEV))
    assert R.same_bits(b4.cpu(), s4.cpu(), b.cpu(), s.cpu())


def test_quantiser_in_a_graph_and_the_non_finite_rule():
    from flasht5_amd import quantize_kv
    x = _rand_rows((2, 9, 2, 64), torch.bfloat16, 3).to(DEV)
    x[0, 1, 0, 5] = float("nan")
    x[1, 2, 1, 0] = float("-inf")
    out = torch.zeros(x.shape, dtype=torch.uint8, device=DEV).view(FP8)
    sc = torch.zeros(x.shape[:3], device=DEV)
    quantize_kv(x, out=out, scale=sc)   # (warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        quantize_kv(x, out=out, scale=sc)
    x.copy_(_rand_rows((2, 9, 2, 64), torch.bfloat16, 4))
    x[0, 1, 0, 5] = float("nan")
    x[1, 2, 1, 0] = float("-inf")
    g.replay()
    torch.cuda.synchronize()
    wb, ws = R.quantize_ref(x.cpu())
    assert R.same_bits(out.cpu(), sc.cpu(), wb, ws)
    # the rule: s = +inf, the NaN / inf element is the byte 0x7F, finite ones are zero, the row reads back as NaN -- other rows do not
    for (b, l, h, d) in ((0, 1, 0, 5), (1, 2, 1, 0)):
        assert math.isinf(float(sc[b, l, h])) and int(out.view(torch.uint8)[b, l, h, d]) == 0x7F
        assert bool(((out.view(torch.uint8)[b, l, h] & 0x7F) == 0).sum() == 63)
    deq = R.dequant(out.cpu(), sc.cpu())
    assert int(torch.isnan(deq).any(-1).sum()) == 2
    del g


# ------------------------------------------------------------------------------------------------------------------ the appends
@pytest.mark.parametrize("D, dtype, layout", [(64, torch.bfloat16, "blhd"), (128, torch.float16, "bhld")])
def test_one_row_and_chunk_appends_leave_the_same_bytes(D, dtype, layout):
    from flasht5_amd import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk, quantize_kv
    B, H, T, cap = 3, 2, 7, 8
    kn, vn = _rand_rows((B, T, H, D), dtype, 1).to(DEV), _rand_rows((B, T, H, D), dtype, 2).to(DEV)
    q = _rand_rows((B, T, H, D), dtype, 3, 1.0).to(DEV)
    start = torch.tensor([0, 2, 1], dtype=torch.int32, device=DEV)
    one = Cache(B, cap, H, D, layout)
    lens = start.clone()
    o1 = []
    for t in range(T):   # the same T rows one at a time (batch element 1 runs into the full cache: its last appends are skipped)
        o1.append(flash_attn_with_kvcache(q[:, t:t + 1], one.k, one.v, kn[:, t:t + 1], vn[:, t:t + 1], lens, **one.kw()))
        lens += 1
    chunked = Cache(B, cap, H, D, layout)
    o2 = torch.cat([flash_attn_with_kvcache_chunk(q[:, :4], chunked.k, chunked.v, kn[:, :4], vn[:, :4], start, causal=True, **chunked.kw()),
                    flash_attn_with_kvcache_chunk(q[:, 4:], chunked.k, chunked.v, kn[:, 4:], vn[:, 4:], start + 4, causal=True,
                                                  **chunked.kw())], 1)
    a, b = one.cpu(), chunked.cpu()
    assert all(torch.equal(x.view(torch.uint8) if x.dtype == FP8 else x.view(torch.int32), y.view(torch.uint8) if y.dtype == FP8 else
                           y.view(torch.int32)) for x, y in zip(a, b))
    assert one.guards_intact() and chunked.guards_intact()
    (wk, wks), (wv, wvs) = quantize_kv(kn), quantize_kv(vn)
    for bb, s0 in enumerate(start.tolist()):
        n = min(T, cap - s0)   # rows that fit
        assert R.same_bits(a[0][bb, s0:s0 + n], a[1][bb, s0:s0 + n], wk[bb, :n].cpu(), wks[bb, :n].cpu())
        assert R.same_bits(a[2][bb, s0:s0 + n], a[3][bb, s0:s0 + n], wv[bb, :n].cpu(), wvs[bb, :n].cpu())
        assert bool((a[0][bb, :s0].view(torch.uint8) == 0).all()) and bool((a[1][bb, s0 + n:] == 0).all())   # nothing else written
    assert R.same_bits(wk.cpu(), wks.cpu(), *R.quantize_ref(kn.cpu()))
    # a one-row step and a chunk step attend the same cache contents: where every row of the chunk fits they agree to the bound's
    # two sides (checked against fp64 below); here only that both are finite and close
    o1 = torch.cat(o1, 1)
    fits = [bb for bb, s0 in enumerate(start.tolist()) if s0 + T <= cap]
    assert torch.isfinite(o1).all() and torch.isfinite(o2).all()
    assert float((o1[fits].float() - o2[fits].float()).abs().max()) <= 2.0 ** -6 * float(o1.float().abs().max())


@pytest.mark.parametrize("D, layout", [(64, "bhld"), (128, "blhd")])
def test_appends_under_garbage_lengths_and_ragged_chunks(D, layout):
    """lengths below 0 and above the capacity, a full cache, chunk_seqlens shorter than M (and garbage): the rows the contract names
    are written, nothing else, and the guard rows around caches and scales stay"""
    from flasht5_amd import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk
    dtype = torch.bfloat16
    B, H, M, cap = 4, 2, 5, 6
    kn, vn = _rand_rows((B, M, H, D), dtype, 5).to(DEV), _rand_rows((B, M, H, D), dtype, 6).to(DEV)
    q = _rand_rows((B, M, H, D), dtype, 7, 1.0).to(DEV)
    wk, wks = R.quantize_ref(kn.cpu())
    lens = torch.tensor([-5, 6, 1000, 3], dtype=torch.int32, device=DEV)          # -> 0, full, full, 3
    c = Cache(B, cap, H, D, layout)
    o = flash_attn_with_kvcache(q[:, :1], c.k, c.v, kn[:, :1], vn[:, :1], lens, **c.kw())
    kb, ks, _, _ = c.cpu()
    assert c.guards_intact() and torch.isfinite(o).all()
    for b, at in ((0, 0), (3, 3)):
        assert R.same_bits(kb[b, at], ks[b, at], wk[b, 0], wks[b, 0])
    written = ks != 0
    assert int(written.sum()) == 2 * H and bool(written[0, 0].all()) and bool(written[3, 3].all())   # elements 1 and 2: skipped
    mlen = torch.tensor([2, 5, 9, -1], dtype=torch.int32, device=DEV)             # -> 2, 5, 5, 0 rows of the chunk
    lens = torch.tensor([-5, 4, 1000, 3], dtype=torch.int32, device=DEV)          # -> 0, 4 (2 fit), full, 3
    c = Cache(B, cap, H, D, layout)
    o = flash_attn_with_kvcache_chunk(q, c.k, c.v, kn, vn, lens, causal=True, chunk_seqlens=mlen, **c.kw())
    kb, ks, _, _ = c.cpu()
    assert c.guards_intact() and torch.isfinite(o).all()
    want = {0: (0, 2), 1: (4, 2), 2: (0, 0), 3: (3, 0)}                           # element -> (first row, rows written)
    for b, (at, n) in want.items():
        assert R.same_bits(kb[b, at:at + n], ks[b, at:at + n], wk[b, :n], wks[b, :n])
        assert int((ks[b] != 0).any(-1).sum()) == n


# ----------------------------------------------------------------------------------------------------- attention against fp64
def _filled(B, cap, H, D, dtype, layout, seed, cacheB=None):
    CB = cacheB or B
    fill = [R.quantize_ref(_rand_rows((CB, cap, H, D), dtype, seed + i)) for i in range(2)]
    return Cache(CB, cap, H, D, layout, fill)


def _check_decode(tag, D, dtype, layout, lens, append, bias, splits, cap, seed, batch_idx=None, permute=False, worst=None):
    from flasht5_amd import flash_attn_with_kvcache
    B, H, Rr = len(lens), 2, 5
    cacheB = 2 if batch_idx is not None else B
    c = _filled(B, cap, H, D, dtype, layout, seed, cacheB)
    q = _rand_rows((B, 1, H, D), dtype, seed + 7, 1.0)
    kn = vn = None
    if append:
        kn, vn = _rand_rows((B, 1, H, D), dtype, seed + 8), _rand_rows((B, 1, H, D), dtype, seed + 9)
    rpe = torch.randn(H, 2 * Rr + 1, generator=torch.Generator().manual_seed(seed)) if bias else None
    rb = None
    if permute:   # key row j of sequence b comes from batch element (b + j) % B: the scales must follow the rows
        rb = ((torch.arange(B).view(B, 1) + torch.arange(cap).view(1, cap)) % B).to(torch.int32)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    scale = D ** -0.5

    def run():
        return flash_attn_with_kvcache(dv(q), c.k, c.v, dv(kn), dv(vn), lens_t, scale, dv(rpe), Rr if bias else 0, return_lse=True,
                                       num_splits=splits, cache_batch_idx=dv(torch.tensor(batch_idx, dtype=torch.int32))
                                       if batch_idx is not None else None, cache_row_batch=dv(rb), **c.kw())
    o, lse = run()
    kb, ks, vb, vs = c.cpu()
    assert c.guards_intact(), tag
    if append:   # the appended rows are the restatement's
        wk, wks = R.quantize_ref(kn[:, 0])
        for b, n in enumerate(lens):
            if 0 <= n < cap:
                assert R.same_bits(kb[b, n], ks[b, n], wk[b], wks[b]), tag
    ref = R.decode_ref8(q, kb, ks, vb, vs, lens, append, scale, rpe, Rr, batch_idx, rb, splits)
    bo, bl = R.decode_bound8(ref, dtype, D, splits)
    ro, rl, same = F.ratios(o[:, 0].cpu(), lse[:, :, 0].cpu(), ref, bo, bl)
    print(f"[kvfp8] decode {tag}: o {ro:.3f} lse {rl:.3f} of the bound")
    assert same and ro <= 1.0 and rl <= 1.0, (tag, ro, rl, same)
    o2, lse2 = run()   # (the append writes the same bytes again: the call is repeatable)
    assert torch.equal(o, o2) and torch.equal(lse, lse2), tag
    if worst is not None:
        worst[0] = max(worst[0], ro, rl)


@pytest.mark.parametrize("D, dtype, layout", [(64, torch.bfloat16, "blhd"), (64, torch.float16, "bhld"), (128, torch.bfloat16, "bhld"),
                                              (128, torch.float16, "blhd")])
def test_decode_attention_within_the_fp64_bound(D, dtype, layout):
    P = _pass(D)
    worst = [0.0]
    seed = 10
    for append in (True, False):
        for bias in (False, True):
            small = [0, 1, 2] if append else [1, 2, 3]      # (with an append, length 0: the new row is the only key)
            for lens, splits, cap in ((small, 1, 4), ([P - 2, P - 1, P], 1, P + 1), ([2 * P - 2, 2 * P - 1, 2 * P], 2, 2 * P + 1)):
                seed += 1
                _check_decode(f"D{D} {layout} append={append} bias={bias} lens={lens} splits={splits}", D, dtype, layout, lens, append,
                              bias, splits, cap, seed, worst=worst)
    # a full cache (the append is skipped), and the maps: cache_batch_idx, and a parent table that permutes rows
    _check_decode(f"D{D} full", D, dtype, layout, [5, 5, 3], True, True, 1, 5, 50, worst=worst)
    _check_decode(f"D{D} cache_batch_idx", D, dtype, layout, [P + 1, 3, P], False, False, 1, P + 1, 51, batch_idx=[1, 0, 1], worst=worst)
    _check_decode(f"D{D} cache_row_batch", D, dtype, layout, [P, P, P], True, True, 2, P + 2, 52, permute=True, worst=worst)
    _check_decode(f"D{D} cache_row_batch no append", D, dtype, layout, [P + 1, 2, 7], False, False, 1, P + 2, 53, permute=True, worst=worst)
    print(f"[kvfp8] decode D{D} {dtype} {layout}: worst error / bound {worst[0]:.3f}")


@pytest.mark.parametrize("D, dtype, layout", [(64, torch.bfloat16, "bhld"), (128, torch.float16, "blhd")])
def test_chunk_attention_within_the_fp64_bound(D, dtype, layout):
    from flasht5_amd import flash_attn_with_kvcache_chunk
    P, H, Rr = _pass(D), 2, 5
    scale = D ** -0.5
    worst, seed = 0.0, 100
    for M in (C.CHUNK_TQ - 1, C.CHUNK_TQ, C.CHUNK_TQ + 1):
        for append, causal, bias, lens, splits in ((True, True, True, [0, P - 2, P - M + 1], 1), (True, True, False, [1, 2 * P - M, P], 2),
                                                   (False, False, False, [M, P + 1, P], 1), (False, True, True, [M + 1, P - 1, 2 * P], 2)):
            seed += 1
            B, cap = 3, 2 * P + 2
            c = _filled(B, cap, H, D, dtype, layout, seed)
            q = _rand_rows((B, M, H, D), dtype, seed + 7, 1.0)
            kn = vn = None
            if append:
                kn, vn = _rand_rows((B, M, H, D), dtype, seed + 8), _rand_rows((B, M, H, D), dtype, seed + 9)
            rpe = torch.randn(H, 2 * Rr + 1, generator=torch.Generator().manual_seed(seed)) if bias else None
            dv = lambda t: None if t is None else t.to(DEV)  # noqa: E731
            lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)

            def run():
                return flash_attn_with_kvcache_chunk(dv(q), c.k, c.v, dv(kn), dv(vn), lens_t, scale, causal, dv(rpe), Rr if bias else 0,
                                                     return_lse=True, num_splits=splits, **c.kw())
            o, lse = run()
            kb, ks, vb, vs = c.cpu()
            assert c.guards_intact()
            ref = R.chunk_ref8(q, kb, ks, vb, vs, lens, kn, scale, causal, rpe, Rr, splits)
            bo, bl = R.chunk_bound8(ref, dtype, D, splits)
            ro, rl, same = C.ratios(o.cpu(), lse.permute(0, 2, 1).cpu(), ref, bo, bl)
            tag = f"D{D} {layout} M={M} append={append} causal={causal} bias={bias} lens={lens} splits={splits}"
            print(f"[kvfp8] chunk {tag}: o {ro:.3f} lse {rl:.3f} of the bound")
            assert same and ro <= 1.0 and rl <= 1.0, (tag, ro, rl, same)
            o2, lse2 = run()
            assert torch.equal(o, o2) and torch.equal(lse, lse2), tag
            worst = max(worst, ro, rl)
    print(f"[kvfp8] chunk D{D} {dtype} {layout}: worst error / bound {worst:.3f}")


def test_graph_replay_gives_the_eager_bits_while_the_lengths_grow():
    from flasht5_amd import flash_attn_with_kvcache
    B, H, D, cap, steps = 2, 2, 64, 140, 6
    dtype = torch.bfloat16
    rows_k, rows_v = _rand_rows((B, steps, H, D), dtype, 1).to(DEV), _rand_rows((B, steps, H, D), dtype, 2).to(DEV)
    qs = _rand_rows((B, steps, H, D), dtype, 3, 1.0).to(DEV)
    start = torch.tensor([126, 0], dtype=torch.int32, device=DEV)   # element 0 crosses one workgroup pass (128 rows) on the way

    def fresh():
        return _filled(B, cap, H, D, dtype, "blhd", 20), start.clone()
    c, lens = fresh()
    eager = []
    for t in range(steps):
        eager.append(flash_attn_with_kvcache(qs[:, t:t + 1], c.k, c.v, rows_k[:, t:t + 1], rows_v[:, t:t + 1], lens, num_splits=2, **c.kw()))
        lens += 1
    want = c.cpu()
    c, lens = fresh()
    q, kn, vn = qs[:, :1].clone(), rows_k[:, :1].clone(), rows_v[:, :1].clone()
    w, wl = fresh()   # (warm-up on a copy)
    flash_attn_with_kvcache(q, w.k, w.v, kn, vn, wl, num_splits=2, **w.kw())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = flash_attn_with_kvcache(q, c.k, c.v, kn, vn, lens, num_splits=2, **c.kw())
        lens.add_(1)
    for t in range(steps):
        q.copy_(qs[:, t:t + 1]), kn.copy_(rows_k[:, t:t + 1]), vn.copy_(rows_v[:, t:t + 1])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, eager[t]), t
    got = c.cpu()
    assert all(torch.equal(a.view(torch.uint8) if a.dtype == FP8 else a, b.view(torch.uint8) if b.dtype == FP8 else b) for a, b in zip(got, want))
    del g


def test_a_poisoned_row_reads_back_as_nan_and_nothing_faults():
    """a NaN in a cached K row (scale +inf) and an inf in the appended V row: the rows read back as NaN, and the kernel does with them
    what the 16-bit kernel does with the NaN rows they stand for -- a NaN in V reaches o, a NaN score makes the softmax sum NaN,
    which the decode kernels have always answered with o = 0 (`sum > 0 ? o / sum : 0`) -- on the poisoned heads only"""
    from flasht5_amd import flash_attn_with_kvcache
    B, H, D, cap = 2, 2, 64, 8
    dtype = torch.bfloat16
    x = _rand_rows((B, cap, H, D), dtype, 1)
    x[0, 2, 1, 9] = float("nan")
    fill = [R.quantize_ref(x), R.quantize_ref(_rand_rows((B, cap, H, D), dtype, 2))]
    c = Cache(B, cap, H, D, "blhd", fill)
    q = _rand_rows((B, 1, H, D), dtype, 3, 1.0).to(DEV)
    kn, vn = _rand_rows((B, 1, H, D), dtype, 4), _rand_rows((B, 1, H, D), dtype, 5)
    vn[1, 0, 0, 3] = float("inf")
    lens = torch.tensor([4, 4], dtype=torch.int32, device=DEV)
    o = flash_attn_with_kvcache(q, c.k, c.v, kn.to(DEV), vn.to(DEV), lens, **c.kw())
    kb, ks, vb, vs = c.cpu()
    assert c.guards_intact()
    assert R.same_bits(vb[:, 4], vs[:, 4], *R.quantize_ref(vn[:, 0])) and math.isinf(float(vs[1, 4, 0]))
    kd, vd = R.dequant(kb, ks, torch.float32), R.dequant(vb, vs, torch.float32)
    assert bool(torch.isnan(kd[0, 2, 1]).all()) and bool(torch.isnan(vd[1, 4, 0]).all())
    assert int(torch.isnan(kd).any(-1).sum()) == 1 and int(torch.isnan(vd).any(-1).sum()) == 1
    # the 16-bit kernel over the dequantised caches
    o16 = flash_attn_with_kvcache(q, kd.to(dtype).to(DEV), vd.to(dtype).to(DEV), cache_seqlens=lens + 1)
    assert torch.equal(torch.isnan(o), torch.isnan(o16))
    assert torch.isnan(o[1, 0, 0]).all() and bool((o[0, 0, 1] == 0).all())
    clean = torch.ones(B, H, dtype=torch.bool)
    clean[0, 1] = clean[1, 0] = False
    assert torch.isfinite(o[:, 0].cpu()[clean]).all() and bool((o[:, 0].cpu()[clean].abs().amax(-1) > 0).all())
