"""Host restatement of the attention-dropout mask (csrc/attn_dropout_kernels.h) on tests/dropout_ref.py's Philox, for
the attention-dropout tests.  For query m, key n (positions inside the sequence) of head h of batch row / packed sequence b:
    w = Philox4x32-10(key = (seed lo, seed hi ^ 0x80000000), counter = (n >> 2, m, (site << 20) | (b H + h), step mod 2^32))
    kept iff (w[n & 3] >> 8) * 2^-24 >= p (as fp32)."""
import numpy as np
import torch

import dropout_ref as R

SEED = 0x9E3779B97F4A7C15   # (top bit set: the flipped key bit clears it)


def host_mask(nbh, bh0, M, N, p, step, site, seed=SEED):
    """(nbh, M, N) bool keep mask of units b H + h = bh0 .. bh0 + nbh - 1, on the GPU"""
    n, m, bh = np.arange(N, dtype=np.uint64), np.arange(M, dtype=np.uint64), np.arange(bh0, bh0 + nbh, dtype=np.uint64)
    ctr = ((n >> np.uint64(2))[None, None, :], m[None, :, None], (np.uint64(site << 20) | bh)[:, None, None], np.uint64(step))
    w = R.philox4x32_10_np(ctr, (seed & R.MASK, (seed >> 32) ^ 0x80000000))
    wl = np.choose(np.broadcast_to((n & np.uint64(3)).astype(np.int64), w[0].shape), w)
    return torch.from_numpy((wl >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) >= np.float32(p)).cuda()
