"""GPU tests of the pack planner (fat5_pack_plan, csrc/pack_kernels.h) against a numpy restatement of its contract
(include/fat5.h), exact integer equality: cu_seqlens, index, seg_count and status for valid rows, every flag bit provoked alone
with all outputs in bounds, identical bytes run to run, and the two launches captured in a HIP graph and replayed on new ids.

The buffers are filled with a sentinel and carry a guard tail, so a store outside what the contract names shows up as a changed
sentinel, not as a fault."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -7


def ref_plan(seg, cap):
    """the contract, row by row: a row contributes its leading run of positive ids, cut wherever the id changes, the segments past
    `cap` merged into the last one"""
    seg = np.asarray(seg, dtype=np.int64)
    B, L = seg.shape
    lengths, index, counts, flags = [], [], [], 0
    for b in range(B):
        x = seg[b]
        stop = np.nonzero(x <= 0)[0]
        n = int(stop[0]) if stop.size else L
        pos = np.nonzero(x > 0)[0]
        if (x < 0).any():
            flags |= 8
        if pos.size == 0:
            flags |= 2
        elif pos[-1] >= n:
            flags |= 1
        if n > 0 and x[0] != 1:
            flags |= 1
        d = np.diff(x[:n])
        if ((d != 0) & (d != 1)).any():
            flags |= 1
        ends = [int(j) + 1 for j in np.nonzero(d != 0)[0]]
        if n > 0 and len(ends) + 1 > cap:
            flags |= 4
        ends = (ends[:cap - 1] + [n]) if n > 0 else []
        lengths += list(np.diff([0] + ends))
        counts.append(len(ends))
        index += [b * L + j for j in range(n)]
    total = len(index)
    cu = np.full(B * cap + 1, total, dtype=np.int32)
    cu[:len(lengths) + 1] = np.concatenate([[0], np.cumsum(lengths)])
    status = np.array([total, len(lengths), max(lengths, default=0), flags], dtype=np.int32)
    return cu, np.array(index, dtype=np.int64), np.array(counts, dtype=np.int32), status


class Buffers:
    def __init__(self, B, L, cap):
        dev = "cuda"
        self.B, self.L, self.cap = B, L, cap
        self.cu = torch.full((B * cap + 1 + GUARD,), SENT, dtype=torch.int32, device=dev)
        self.index = torch.full((B * L + GUARD,), SENT, dtype=torch.int64, device=dev)
        self.seg_count = torch.full((B + GUARD,), SENT, dtype=torch.int32, device=dev)
        self.status = torch.full((4 + GUARD,), SENT, dtype=torch.int32, device=dev)

    def launch(self, seg):
        from flasht5_amd import _lib
        p = _lib.PackParams()
        p.B, p.L, p.seg_cap = self.B, self.L, self.cap
        p.seg, p.cu_seqlens, p.index, p.seg_count, p.status = (t.data_ptr() for t in (seg, self.cu, self.index, self.seg_count, self.status))
        _lib.check(_lib.load().fat5_pack_plan(ctypes.byref(p), _lib.stream_ptr(seg.device)), "fat5_pack_plan")

    def host(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.cu, self.index, self.seg_count, self.status))


def run_plan(seg_np, cap):
    seg = torch.from_numpy(np.ascontiguousarray(seg_np, dtype=np.int32)).cuda()
    B, L = seg.shape
    buf = Buffers(B, L, cap)
    buf.launch(seg)
    return buf.host()


def check(seg_np, cap):
    """run, compare with the restatement, check the guards and the bounds; returns the status words"""
    seg_np = np.asarray(seg_np, dtype=np.int32)
    B, L = seg_np.shape
    cu, index, seg_count, status = run_plan(seg_np, cap)
    rcu, rindex, rcount, rstatus = ref_plan(seg_np, cap)
    total = int(rstatus[0])
    assert (status[:4] == rstatus).all(), (status[:4], rstatus)
    assert (cu[:B * cap + 1] == rcu).all(), (cu[:B * cap + 1], rcu)
    assert (index[:total] == rindex).all()
    assert (seg_count[:B] == rcount).all(), (seg_count[:B], rcount)
    # nothing outside what the contract names was written
    assert (index[total:] == SENT).all() and (cu[B * cap + 1:] == SENT).all()
    assert (seg_count[B:] == SENT).all() and (status[4:] == SENT).all()
    # in bounds whatever the input
    assert 0 <= total <= B * L and (index[:total] >= 0).all() and (index[:total] < B * L).all()
    assert cu[0] == 0 and (np.diff(cu[:B * cap + 1].astype(np.int64)) >= 0).all() and cu[B * cap] == total
    return status[:4]


def base_rows(L=70):
    rows = np.zeros((5, L), dtype=np.int32)
    rows[0, :] = 1                                   # fully valid
    rows[1, :1] = 1                                  # length 1
    rows[2, :9], rows[2, 9:10], rows[2, 10:41] = 1, 2, 3   # three segments, one of length 1
    rows[3, :20], rows[3, 20:] = 1, 2                # a segment ending at column L - 1
    rows[4, :33] = 1                                 # one segment, then padding
    return rows


def test_base_case():
    st = check(base_rows(), 4)
    assert list(st) == [70 + 1 + 41 + 70 + 33, 1 + 1 + 3 + 2 + 1, 70, 0]


@pytest.mark.parametrize("L", [1, 3, 4, 64, 67, 1024, 1031, 2500])
def test_row_lengths_and_alignment(L):
    """one quad, one chunk of the row kernel (1024 columns), more than one; rows that start 0 .. 3 ints past a 16-byte boundary"""
    rng = np.random.default_rng(L)
    B, cap = 6, 5
    rows = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        n = int(rng.integers(1, L + 1)) if b else L
        k = int(rng.integers(1, min(cap, n) + 1))
        cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False)) if k > 1 else np.array([], dtype=np.int64)
        ids = np.ones(n, dtype=np.int32)
        for c in cuts:
            ids[c:] += 1
        rows[b, :n] = ids
    assert check(rows, cap)[3] == 0


def test_single_row_single_column_and_mask():
    assert list(check(base_rows()[2:3], 4)) == [41, 3, 31, 0]          # B = 1
    assert list(check(np.array([[1], [1], [1]]), 2)) == [3, 3, 1, 0]    # L = 1
    mask = (np.arange(70)[None, :] < np.array([70, 1, 33])[:, None]).astype(np.int32)
    assert list(check(mask, 1)) == [104, 3, 70, 0]                      # seg_cap = 1 with a mask


def test_many_rows_cross_the_scan_chunks():
    """B * seg_cap = 3000 slots: three chunks of the one-workgroup scan, live and dead slots mixed"""
    rng = np.random.default_rng(3)
    B, L, cap = 750, 9, 4
    rows = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        n = int(rng.integers(1, L + 1))
        rise = rng.random(n) < 0.3
        rise[0] = False
        rows[b, :n] = np.minimum(1 + np.cumsum(rise), cap)
    assert check(rows, cap)[3] == 0


@pytest.mark.parametrize("name, row, flag", [
    ("hole", [1, 1, 0, 1, 1, 0, 0, 0], 1),
    ("left padding", [0, 0, 1, 1, 1, 1, 1, 1], 1),
    ("id 1 -> 3", [1, 1, 3, 3, 0, 0, 0, 0], 1),
    ("a falling id", [1, 2, 2, 1, 0, 0, 0, 0], 1),
    ("first id 2", [2, 2, 3, 0, 0, 0, 0, 0], 1),
    ("an empty row", [0, 0, 0, 0, 0, 0, 0, 0], 2),
    ("too many segments", [1, 2, 3, 4, 4, 0, 0, 0], 4),
    ("a negative id", [1, 1, -1, 0, 0, 0, 0, 0], 8),
])
def test_every_flag_alone_and_in_bounds(name, row, flag):
    rows = np.array([[1, 1, 2, 2, 2, 3, 0, 0], row, [1, 1, 1, 1, 1, 1, 1, 1]], dtype=np.int32)
    st = check(rows, 3)
    assert st[3] == flag, (name, st)


def test_two_runs_give_equal_bytes():
    a, b = run_plan(base_rows(), 4), run_plan(base_rows(), 4)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_planner_replays_from_a_captured_graph():
    """the two launches are sized by (B, L, seg_cap) alone and read nothing back: captured once, a replay plans whatever the ids
    buffer holds by then"""
    first, second = base_rows(), base_rows()[::-1].copy()
    second[0, 5:] = 0
    seg = torch.from_numpy(first).cuda()
    buf = Buffers(5, 70, 4)
    buf.launch(seg)          # (module load and first launch outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.launch(seg)
    for rows in (second, first):
        seg.copy_(torch.from_numpy(rows).cuda())
        g.replay()
        cu, index, seg_count, status = buf.host()
        rcu, rindex, rcount, rstatus = ref_plan(rows, 4)
        assert (status[:4] == rstatus).all() and (cu[:21] == rcu).all() and (seg_count[:5] == rcount).all()
        assert (index[:rstatus[0]] == rindex).all()


def test_pack_plan_and_plan_pair_python_entry():
    from flasht5_amd import pack_plan, plan_pair
    rows = torch.from_numpy(base_rows()).cuda()
    plan = pack_plan(rows, seg_cap=4)
    rcu, rindex, rcount, rstatus = ref_plan(base_rows(), 4)
    assert (plan.total, plan.nseq, plan.max_seqlen) == tuple(int(v) for v in rstatus[:3])
    assert plan.cu_seqlens.dtype == torch.int32 and plan.cu_seqlens.cpu().tolist() == rcu[:plan.nseq + 1].tolist()
    assert plan.index.dtype == torch.int64 and plan.index.cpu().tolist() == rindex.tolist()
    assert plan.seg_count.cpu().tolist() == rcount.tolist()
    mask = rows != 0
    m = pack_plan(mask)                                   # bool mask: 0 / 1, one segment per row
    assert m.nseq == 5 and m.total == plan.total and torch.equal(m.index, plan.index)
    for bad, word in ((torch.tensor([[1, 0, 1]]), "right-padded"), (torch.tensor([[0, 0, 0]]), "at least one valid position"),
                      (torch.tensor([[1, -1, 0]]), "negative")):
        with pytest.raises(ValueError, match=word):
            pack_plan(bad.cuda())
    with pytest.raises(ValueError, match="seg_cap"):
        pack_plan(rows, seg_cap=2)
    e, d = plan_pair(rows, rows[:, :40].contiguous())
    assert e.nseq == d.nseq == 8
    with pytest.raises(ValueError, match="different numbers of segments"):
        plan_pair(rows, mask)
