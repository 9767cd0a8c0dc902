"""Host restatement of the dropout contract (include/fat5.h), for the dropout tests: a numpy-vectorised Philox4x32-10,
the keep mask and the scale, and torch restatements of the three operators that apply an uploaded mask with the contract's
roundings.  For the element at logical row i, column c of a (rows, n) operand:

    e = elem_offset + i * n + c;  block j = e >> 2, lane l = e & 3
    w = Philox4x32-10(key = (seed lo, seed hi), counter = (j lo, j hi, site, step mod 2^32));  u = (w[l] >> 8) * 2^-24
    kept iff u >= p (as fp32; both sides exact);  s = 1.0f / (1.0f - p);  dropout(x) = round_to_dtype(fp32(x) * s) or +0
"""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10_np(ctr, key):
    """ctr: four uint32 arrays of one shape (or scalars), key: two Python ints -> four uint32 arrays"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in np.broadcast_arrays(*ctr))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m32, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2     # (32 x 32 -> 64 bits: exact in uint64)
        c0, c1, c2, c3 = ((p1 >> sh) ^ c1 ^ np.uint64(k0)) & m32, p1 & m32, ((p0 >> sh) ^ c3 ^ np.uint64(k1)) & m32, p0 & m32
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def keep_mask(rows, n, p, seed, step, site, elem_offset=0):
    """(rows, n) bool: True where the element is kept"""
    seed = int(seed) & MASK64
    e = (np.uint64(int(elem_offset)) + np.arange(rows * n, dtype=np.uint64)).reshape(rows, n)
    j, lane = e >> np.uint64(2), (e & np.uint64(3)).astype(np.int64)
    w = philox4x32_10_np((j & np.uint64(MASK), j >> np.uint64(32), np.uint64(int(site) & MASK), np.uint64(int(step) & MASK)),
                         (seed & MASK, seed >> 32))
    wl = np.choose(lane, w)
    u = (wl >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)   # exact: a 24-bit integer times 2^-24
    return u >= np.float32(p)


def scale(p):
    """s = 1.0f / (1.0f - p): one fp32 subtraction and one fp32 division"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def apply_mask(x, keep, p):
    """dropout(x) with the mask given: fp32(x) * s rounded to x's dtype where kept, +0 where dropped (x: any shape, keep: the same
    number of elements, row-major)"""
    s = torch.tensor(float(scale(p)), dtype=torch.float32, device=x.device)
    keep = keep.reshape(x.shape)
    return torch.where(keep, (x.float() * s).to(x.dtype), torch.zeros((), dtype=x.dtype, device=x.device))


def mask_for(x, p, seed, step, site, elem_offset=0):
    """the contract's mask of x as a logical (numel / n, n) operand, uploaded to x's device"""
    n = x.shape[-1]
    k = keep_mask(x.numel() // n, n, p, seed, int(step), site, elem_offset)
    return torch.from_numpy(k).to(x.device).reshape(x.shape)


# ---- torch restatements of flasht5_amd.dropout's three operators (autograd flows through torch.where: the backward multiplies the
# ---- incoming gradient by the same mask and scale and rounds it to the dtype, which is what the kernels' backward computes)
class _MaskedScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep, p):
        ctx.save_for_backward(keep)
        ctx.p = p
        return apply_mask(x, keep, p)

    @staticmethod
    def backward(ctx, dy):
        (keep,) = ctx.saved_tensors
        return apply_mask(dy, keep, ctx.p), None, None


def dropout_restated(x, p, seed, step, site, elem_offset=0):
    return _MaskedScale.apply(x, mask_for(x, p, seed, step, site, elem_offset), p)


def dropout_add_restated(x, residual, p, seed, step, site):
    return residual + dropout_restated(x, p, seed, step, site)
