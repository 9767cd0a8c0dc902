"""GPU tests of `flasht5_amd.sequence_pool` against the fp64 restatement (tests/pool_ref.py), at the seams only:
widths around the 16-byte vector and the column tile, lengths around the token split and the wave, both layouts, the three dtypes,
strided and misaligned inputs, EOS placement, clamped lengths, guard elements, NaN-prefilled gradients, and graph replay.
Gather modes and their backward are exact; "mean" is held to the derived bound of pool_ref."""
import ctypes

import pytest
import torch

import pool_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = ["padded", "packed"]
EOS = 1
GUARD = 64   # elements on either side of every buffer the raw calls hand to the library


def _constants():
    from flasht5_amd.pooling import POOL_SPLIT, POOL_TILE
    widths = sorted({1, 7, 8, 72, POOL_TILE - 8, POOL_TILE, POOL_TILE + 8})
    lengths = [0, 1, 2, POOL_SPLIT - 1, POOL_SPLIT, POOL_SPLIT + 1, 63, 64, 65, 200]
    return widths, lengths


def make_batch(lens, L, d, dtype, layout, seed=0):
    """random hidden states and ids for sequences of `lens`; ids avoid EOS except where row b's pattern (b mod 4) puts one: at the
    last valid position / at 0 / at 0, the middle and the last but one / nowhere inside, but right behind the sequence"""
    g = torch.Generator().manual_seed(seed + 131 * d + L)
    B = len(lens)
    if layout == "padded":
        hidden = torch.randn(B, L, d, generator=g).to(dtype)
        ids = torch.randint(2, 30, (B, L), generator=g)
        starts, flat = [b * L for b in range(B)], ids.view(-1)
    else:
        total = sum(lens)
        hidden = torch.randn(total, d, generator=g).to(dtype)
        ids = torch.randint(2, 30, (total,), generator=g)
        starts, flat = [sum(lens[:b]) for b in range(B)], ids
    for b, (s, n) in enumerate(zip(starts, lens)):
        if n == 0:
            continue
        if b % 4 == 0:
            flat[s + n - 1] = EOS
        elif b % 4 == 1:
            flat[s] = EOS
        elif b % 4 == 2:
            for j in (0, n // 2, max(n - 2, 0)):
                flat[s + j] = EOS
    for b, (s, n) in enumerate(zip(starts, lens)):   # (afterwards: an EOS behind the sequence may be the neighbour's first id)
        if b % 4 == 3 and s + n < flat.numel() and (layout == "packed" or n < L):
            flat[s + n] = EOS
    if layout == "padded":
        kw = dict(seqlens=torch.tensor(lens, dtype=torch.int32))
    else:
        kw = dict(cu_seqlens=torch.tensor([0] + [sum(lens[:b + 1]) for b in range(B)], dtype=torch.int32))
    return hidden, ids, kw


def check_all_modes(hidden_dev, hidden_cpu, ids, kw, dtype, seed=0):
    """forward and backward of the four modes through the public operator against the restatement; returns {mode: (pooled, dhidden)}"""
    from flasht5_amd import sequence_pool
    dev_kw = {k: v.cuda() for k, v in kw.items()}
    out = {}
    for mode in R.MODES:
        h = hidden_dev.detach().requires_grad_(True)
        got = sequence_pool(h, mode, input_ids=ids.cuda() if mode == "eos" else None, eos_token_id=EOS, **dev_kw)
        ref = R.pool_ref(hidden_cpu, mode, input_ids=ids, eos_token_id=EOS, **kw)
        R.check_pool(got, ref, mode, dtype)
        dp = torch.randn(got[0].shape, generator=torch.Generator().manual_seed(seed + 7)).to(dtype)
        (dh,) = torch.autograd.grad(got[0], h, dp.cuda())
        assert dh.shape == hidden_dev.shape and dh.dtype == dtype
        R.check_pool_bwd(dh, R.pool_bwd_ref(dp, tuple(hidden_cpu.shape), mode, ref["position"], **kw), mode, dtype)
        out[mode] = (got[0].detach(), dh)
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_widths_and_lengths_at_the_seams(dtype, layout):
    """ten ragged sequences (an empty one and a full row among them) at every width; all modes, forward and backward"""
    widths, lengths = _constants()
    for d in widths:
        hidden, ids, kw = make_batch(lengths, max(lengths), d, dtype, layout)
        check_all_modes(hidden.cuda(), hidden, ids, kw, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_one_sequence(dtype):
    """B = 1 at every length, the row exactly as long as the sequence (L = 0 included), with and without seqlens"""
    _, lengths = _constants()
    for n in lengths:
        for d in (8, 72):
            hidden, ids, kw = make_batch([n], n, d, dtype, "padded", seed=n)
            check_all_modes(hidden.cuda(), hidden, ids, kw, dtype)
            check_all_modes(hidden.cuda(), hidden, ids, {}, dtype)
            hidden, ids, kw = make_batch([n], n, d, dtype, "packed", seed=n)
            check_all_modes(hidden.cuda(), hidden, ids, kw, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_strides_and_misaligned_bases(dtype):
    """B = 5 ragged (a full row, an empty one): a row stride of d + 1 and a base one element off 16 bytes take the element path, a
    row stride of d + 8 and an odd batch stride the vector path -- the same bits either way"""
    lens, L, d = [40, 0, 17, 1, 33], 40, 72
    hidden, ids, kw = make_batch(lens, L, d, dtype, "padded", seed=3)
    dev = hidden.cuda()
    base = check_all_modes(dev, hidden, ids, kw, dtype)
    variants = {}
    for name, pad in (("row stride d + 1", 1), ("row stride d + 8", 8)):
        buf = torch.zeros(len(lens), L, d + pad, dtype=dtype, device="cuda")
        buf[..., :d] = dev
        variants[name] = buf[..., :d]
        assert variants[name].stride() == (L * (d + pad), d + pad, 1)
    buf = torch.zeros(hidden.numel() + 1, dtype=dtype, device="cuda")
    buf[1:] = dev.reshape(-1)
    variants["misaligned base"] = buf[1:].view(hidden.shape)
    assert variants["misaligned base"].data_ptr() % 16 != 0
    buf = torch.zeros(len(lens), L + 1, d, dtype=dtype, device="cuda")
    buf[:, :L] = dev
    variants["batch stride (L + 1) d"] = buf[:, :L]
    for name, v in variants.items():
        got = check_all_modes(v, hidden, ids, kw, dtype)
        for mode in R.MODES:
            assert torch.equal(got[mode][0], base[mode][0]) and torch.equal(got[mode][1], base[mode][1]), (name, mode)
    # packed rows with a stride, and an upstream gradient whose rows are strided
    from flasht5_amd import sequence_pool
    hidden, ids, kw = make_batch(lens, L, d, dtype, "packed", seed=4)
    base = check_all_modes(hidden.cuda(), hidden, ids, kw, dtype)
    buf = torch.zeros(hidden.shape[0], d + 1, dtype=dtype, device="cuda")
    buf[:, :d] = hidden.cuda()
    got = check_all_modes(buf[:, :d], hidden, ids, kw, dtype)
    for mode in R.MODES:
        assert torch.equal(got[mode][0], base[mode][0]) and torch.equal(got[mode][1], base[mode][1]), mode
    h = hidden.cuda().requires_grad_(True)
    pooled = sequence_pool(h, "mean", cu_seqlens=kw["cu_seqlens"].cuda())[0]
    dp = torch.randn(len(lens), d + 1, generator=torch.Generator().manual_seed(11)).to(dtype).cuda()[:, :d]
    (dh,) = torch.autograd.grad(pooled, h, dp)
    R.check_pool_bwd(dh, R.pool_bwd_ref(dp.cpu(), tuple(hidden.shape), "mean", [-1] * len(lens), **kw), "mean", dtype)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_eos_placement(layout):
    from flasht5_amd import sequence_pool
    L, d = 8, 8
    # (ids, length) -> (position, found)
    rows = {
        "under the padding only": ([5, 6, 7, 8, 9, EOS, 9, 9], 4, (3, 0)),   # in the packed layout: the neighbour's first id
        "at 0": ([EOS, 6, 7, 8, 9, 9, 9, 9], 5, (0, 1)),
        "at the last valid position": ([5, 6, 7, 8, EOS, 9, 9, 9], 5, (4, 1)),
        "several": ([5, EOS, 7, EOS, 9, 9, 9, 9], 6, (3, 1)),
        "none, full row": ([5, 6, 7, 8, 9, 9, 9, 9], 8, (7, 0)),
    }
    lens = [n for _, n, _ in rows.values()]
    want_pos, want_found = [w[0] for _, _, w in rows.values()], [w[1] for _, _, w in rows.values()]
    g = torch.Generator().manual_seed(2)
    if layout == "padded":
        hidden = torch.randn(len(rows), L, d, generator=g).bfloat16().cuda()
        ids = torch.tensor([r for r, _, _ in rows.values()]).cuda()
        pooled, position, found = sequence_pool(hidden, "eos", seqlens=torch.tensor(lens, dtype=torch.int32).cuda(), input_ids=ids, eos_token_id=EOS)
        picked = torch.stack([hidden[b, p] for b, p in enumerate(want_pos)])
    else:
        flat = [t for r, n, _ in rows.values() for t in r[:n]]
        assert flat[lens[0]] == EOS     # the sequence after the EOS-free one starts with an EOS
        hidden = torch.randn(len(flat), d, generator=g).bfloat16().cuda()
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        pooled, position, found = sequence_pool(hidden, "eos", cu_seqlens=torch.tensor(cu, dtype=torch.int32).cuda(),
                                                input_ids=torch.tensor(flat).cuda(), eos_token_id=EOS)
        picked = torch.stack([hidden[cu[b] + p] for b, p in enumerate(want_pos)])
    assert position.tolist() == want_pos and found.tolist() == want_found
    assert torch.equal(pooled, picked)


# ---------------------------------------------------------------- the C ABI on buffers with guards
def _guarded(shape, dtype, fill):
    n = 1
    for s in shape:
        n *= s
    sentinel = 77 if not dtype.is_floating_point else 1234.0
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n].view(shape), sentinel


def _guards_intact(buf, n, sentinel):
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())


def _raw(hidden, mode, kw, ids, dpooled=None, position=None):
    """fat5_seq_pool_fwd (dpooled None) or _bwd on guarded outputs: the outputs, after asserting that no guard element changed.
    The backward's dhidden is pre-filled with NaN."""
    from flasht5_amd import _lib, pooling
    packed = "cu_seqlens" in kw
    nseq = kw["cu_seqlens"].numel() - 1 if packed else hidden.shape[0]
    d = hidden.shape[-1]
    p = _lib.SeqPoolParams()
    p.mode, p.dtype, p.nseq, p.d, p.eos_token_id = pooling.MODES[mode], _lib.dtype_code(hidden.dtype), nseq, d, EOS
    if packed:
        p.total, p.cu_seqlens = hidden.shape[0], kw["cu_seqlens"].data_ptr()
    else:
        p.L = hidden.shape[1]
        p.seqlens = kw["seqlens"].data_ptr() if "seqlens" in kw else None
    bufs = []
    if dpooled is None:
        p.hidden = hidden.data_ptr()
        p.hidden_row_stride, p.hidden_batch_stride = d, 0 if packed else hidden.shape[1] * d
        if ids is not None:
            p.input_ids, p.ids_batch_stride = ids.data_ptr(), 0 if packed else hidden.shape[1]
        outs = [_guarded((nseq, d), hidden.dtype, float("nan")), _guarded((nseq,), torch.int32, -9), _guarded((nseq,), torch.int32, -9)]
        p.pooled, p.pooled_stride, p.position, p.found = outs[0][1].data_ptr(), d, outs[1][1].data_ptr(), outs[2][1].data_ptr()
        call = _lib.load().fat5_seq_pool_fwd
    else:
        outs = [_guarded(tuple(hidden.shape), hidden.dtype, float("nan"))]
        p.dpooled, p.dpooled_stride, p.position = dpooled.data_ptr(), d, position.data_ptr()
        p.dhidden, p.dhidden_row_stride, p.dhidden_batch_stride = outs[0][1].data_ptr(), d, 0 if packed else hidden.shape[1] * d
        call = _lib.load().fat5_seq_pool_bwd
    _lib.check(call(ctypes.byref(p), _lib.stream_ptr(hidden.device)), "seq_pool")
    torch.cuda.synchronize()
    for buf, view, sentinel in outs:
        assert _guards_intact(buf, view.numel(), sentinel)
    return [view for _, view, _ in outs]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_clamped_lengths_guards_and_full_gradient(dtype, layout):
    """negative lengths and lengths above L (entries outside [0, total]) are clamped on the device; nothing is written outside
    the outputs; the backward leaves no element of a NaN-filled dhidden unwritten"""
    g = torch.Generator().manual_seed(6)
    d = 24
    if layout == "padded":
        hidden = torch.randn(4, 20, d, generator=g).to(dtype)
        ids = torch.randint(1, 4, (4, 20), generator=g)
        kw = dict(seqlens=torch.tensor([-5, 27, 3, 20], dtype=torch.int32))
    else:
        hidden = torch.randn(30, d, generator=g).to(dtype)
        ids = torch.randint(1, 4, (30,), generator=g)
        kw = dict(cu_seqlens=torch.tensor([-3, 4, 4, 99, 12], dtype=torch.int32))   # read as 0, 4, 4, 30, 12: lengths 4, 0, 26, 0
    dev_kw = {k: v.cuda() for k, v in kw.items()}
    for mode in R.MODES:
        ref = R.pool_ref(hidden, mode, input_ids=ids, eos_token_id=EOS, **kw)
        got = _raw(hidden.cuda(), mode, dev_kw, ids.cuda() if mode == "eos" else None)
        R.check_pool(got, ref, mode, dtype)
        dp = torch.randn(ref["pooled"].shape, generator=g).to(dtype)
        (dh,) = _raw(hidden.cuda(), mode, dev_kw, None, dpooled=dp.cuda(), position=got[1])
        R.check_pool_bwd(dh, R.pool_bwd_ref(dp, tuple(hidden.shape), mode, ref["position"], **kw), mode, dtype)
    if layout == "padded":   # no seqlens: every row holds L tokens
        got = _raw(hidden.cuda(), "last", {}, None)
        R.check_pool(got, R.pool_ref(hidden, "last"), "last", dtype)


def test_empty_shapes():
    from flasht5_amd import sequence_pool
    hidden = torch.randn(5, 16, device="cuda").bfloat16()
    cu = torch.zeros(1, dtype=torch.int32, device="cuda")
    pooled, position, found = sequence_pool(hidden, "mean", cu_seqlens=cu)
    assert pooled.shape == (0, 16) and position.shape == (0,) and found.shape == (0,)
    (dh,) = _raw(hidden, "mean", dict(cu_seqlens=cu), None, dpooled=pooled, position=position)   # rows no sequence owns: zeros
    assert not bool(dh.float().abs().sum())
    pooled, position, found = sequence_pool(torch.zeros(2, 3, 0, device="cuda"), "last")
    assert pooled.shape == (2, 0) and position.tolist() == [-1, -1] and found.tolist() == [0, 0]


# ---------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["eos", "mean"])
def test_two_runs_and_graph_replay_follow_eager_bit_for_bit(mode, layout):
    from flasht5_amd import sequence_pool
    lens_a, lens_b, L, d = [70, 0, 33, 1, 17, 64], [5, 70, 16, 0, 31, 63], 70, 72
    batches = []
    for lens in (lens_a, lens_b):
        if layout == "packed":   # (both splits of the same 185 rows)
            assert sum(lens) == sum(lens_a)
        hidden, ids, kw = make_batch(lens, L, d, torch.bfloat16, layout, seed=sum(lens[:2]))
        batches.append((ids.cuda(), {k: v.cuda() for k, v in kw.items()}))
    hidden = hidden.cuda().requires_grad_(True)
    dp = torch.randn(len(lens_a), d, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()

    def eager(ids, kw):
        out = sequence_pool(hidden, mode, input_ids=ids, eos_token_id=EOS, **kw)
        return [t.detach().clone() for t in (*out, torch.autograd.grad(out[0], hidden, dp)[0])]

    first, again = eager(*batches[0]), eager(*batches[0])
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    other = eager(*batches[1])
    assert not torch.equal(first[0], other[0])
    static_ids, static_kw = batches[0][0].clone(), {k: v.clone() for k, v in batches[0][1].items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sequence_pool(hidden, mode, input_ids=static_ids, eos_token_id=EOS, **static_kw)
        captured = [*out, torch.autograd.grad(out[0], hidden, dp)[0]]
    for (ids, kw), want in ((batches[1], other), (batches[0], first)):
        static_ids.copy_(ids)
        for k in kw:
            static_kw[k].copy_(kw[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(captured, want):
            assert torch.equal(got, ref)
