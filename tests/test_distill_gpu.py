"""GPU tests of knowledge distillation (csrc/kd_kernels.h, flasht5_amd/distillation.py, flasht5_amd/distill.py)
against the fp64 restatements of tests/distill_fp64.py, per element.

Bounds (u = 2^-24, the fp32 unit roundoff; ulp_T(r) = the spacing of dtype T at |r|).  Each is half an ulp of the output's dtype
plus u x (the depth of the kernel's own summation tree) x the sum of term magnitudes, derived from the kernel:

  * DEPTH, roundings on a carried sum: VEC adds inside a 16-byte chunk; per chunk of a thread the rescale of the carried sum --
    exp2 (1 ulp = 2 u), a multiply and an add: 4; the wave combine -- a rescale (3) and wave_sum's 6 levels; the 4-wave combine
    -- a rescale (3) and 4 adds.  DEPTH = VEC + 4 ceil(V / (256 VEC)) + 16 (vector) or 4 ceil(V / 256) + 16 (scalar: one element
    per step).  The plain sum of the scaled logits (label smoothing) is DSUM = VEC ceil(V / (256 VEC)) + 10 deep (scalar:
    ceil(V / 256) + 10).
  * One exponential e_j = exp(x_j - m) of a stream x = c * logits (c = logit_scale, or 1 / T as the rounded reciprocal): x_j
    carries 2 u |x_j| (the scale and the product), the exponent's subtraction, its product with log2(e) and that constant 3 u
    |x_j - m|, the later rescales of the carried sum another 3 u |x_j - m| (the running maxima only rise, from at least x_j to
    m), exp2 itself 2 u; with |x_j - m| <= |x_j| + |lse| + log V the relative error of e_j is at most
    eps_j = u (8 |x_j| + 6 |lse| + 6 log V + 2).
  * A log-sum-exp (lse of logit_scale * s, of s / T and of t / T): the sum's relative error is sum_j p_j eps_j + DEPTH u, logf
    adds 2 u log V and the final add u |lse|:   e_lse = u (DEPTH + 2 + 8 sum_j p_j |x_j| + 7 |lse| + 8 log V).
  * kd = A / l_t - lse_t + lse_s.  A / l_t = sum_j p_j d_j with d_j = (t_j - s_j) / T is a ratio of two sums over the SAME
    computed exponentials, so the reference point cancels; each d_j carries 2 u (|t_j / T| + |s_j / T|) + u |d_j|, the product
    u, both sums DEPTH u, the division u:
        e_ratio = u (sum_j p_j |d_j| eps_j / u + S_d sum_j p_j eps_j / u + (2 DEPTH + 4) S_d + 2 sum_j p_j (|t_j / T| + |s_j / T|)),
    S_d = sum_j p_j |d_j|, and  e_kd = e_ratio + e_lse_t + e_lse_s + 2 u (|A / l_t| + |lse_t| + |lse_s|).
  * ce (rowwise_kernels.h's arithmetic): e_ce = e_lse + e_z + 4 u (|lse| + |x_label| + |z|) + s u (DSUM + 3) mean |x|, with
    e_z = 2 zs |lse| e_lse + 4 u |z|;   loss = (1 - alpha) ce + alpha T^2 kd:  (1 - alpha) e_ce + alpha T^2 e_kd + 4 u ((1 -
    alpha) |ce| + alpha T^2 |kd|).
  * dlogits_j = g (P_j zf - onehot terms) + k (q_j - p_j), g = dloss logit_scale (1 - alpha), k = dloss alpha T.  A probability
    from a stored lse is exp2(fma(x, c log2 e, -lse log2 e)): the two constants 3 u |x_j| + 2 u |lse|, the fma u |x_j - lse|,
    exp2 2 u and the lse's own error:  rel(P_j) = e_lse + u (4 |x_j| + 3 |lse| + 2).  So
        |g| (P_j |zf| (rel(P_j) + 6 u) + 2 zs P_j e_lse + 4 u (P_j |zf| + onehot + s / V))
      + |k| (q_j rel(q_j) + p_j rel(p_j) + 4 u (q_j + p_j)) + u (|g term| + |k term|) + ulp_T(ref) / 2.
  * Underflow: exp2 returns 0 below the smallest normal fp32, TINY = 2^-126, and an fp32 product below it may be flushed too.
    A probability is then off by up to TINY in absolute terms and a gradient element by TINY (|g zf| + 2 |k| + 2); in the
    forward sums every flushed exponential is below TINY of the largest term, which is 1: V TINY joins e_lse and
    V TINY (1 + max_j |d_j|) joins e_ratio.
  * Exact: an ignored row is zero in every output; alpha = 0 gives the bits of cross_entropy_fwd / cross_entropy_bwd; the one
    launch gives the bits of the two; a second run gives the bits of the first; guard elements keep theirs.

Scalars reach the reference as the kernel reads them: rounded to fp32.  The scaled-logit magnitudes in the bounds take 0 for a
-inf entry (its probability is exactly 0 on both sides).
"""
import importlib
import math
import zlib

import pytest
import torch

import distill_fp64 as D
import rowwise_fp64 as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
VEC = {F32: 4, F16: 8, BF16: 8}
OUT_NAMES = ("loss", "kd", "z", "ce", "lse", "lse_student_t", "lse_teacher_t")


def _name(d):
    return str(d)[6:]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _check(got, ref, bound, what):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} out of bound; first at flat {i}: got {got.flatten()[i].item()!r} "
                             f"ref {ref.flatten()[i].item()!r} bound {bound.flatten()[i].item():.3e}")


def _mod():
    return importlib.import_module("flasht5_amd.distillation")


def _fin(x):
    return torch.where(torch.isfinite(x), x, torch.zeros(()).double()).abs()


def _w(p, x):
    """p * x with 0 wherever p is 0 (x may be infinite or NaN there)"""
    return torch.where(p > 0, p * x, torch.zeros(()).double())


def _vector(*tensors):
    return all(t.shape[-1] % VEC[t.dtype] == 0 and t.stride(0) % VEC[t.dtype] == 0 and t.data_ptr() % 16 == 0 for t in tensors)


class Bounds:
    """the docstring's bounds for one problem, from the fp64 reference"""

    def __init__(self, logits, teacher, labels, cfg, vector):
        alpha, T, sm, scale, zs, ign = cfg
        V, dtype = logits.shape[-1], logits.dtype
        v = VEC[dtype]
        self.depth = (v + 4 * math.ceil(V / (256 * v)) + 16) if vector else (4 * math.ceil(V / 256) + 16)
        dsum = (v * math.ceil(V / (256 * v)) + 10) if vector else (math.ceil(V / 256) + 10)
        logV = math.log(V)
        self.ref = D.kd_fwd(logits, teacher, labels, alpha, T, sm, scale, zs, ign)
        loss, kd, z, ce, lse, lse_s, lse_t = self.ref
        lab = labels.cpu()
        self.keep = (lab != ign).double()
        x = logits.double().cpu() * scale
        ss, tt = logits.double().cpu() / T, teacher.double().cpu() / T
        self.P = torch.exp(x - lse.unsqueeze(-1))
        _, self.q, self.p, _, _ = D.kd_terms(logits, teacher, T)
        self.xa, self.sa, self.ta = _fin(x), _fin(ss), _fin(tt)

        def e_lse(prob, mag, l):
            return U * (self.depth + 2 + 8 * (prob * mag).sum(-1) + 7 * l.abs() + 8 * logV) + V * TINY

        self.e_lse, self.e_lse_s, self.e_lse_t = e_lse(self.P, self.xa, lse), e_lse(self.q, self.sa, lse_s), e_lse(self.p, self.ta, lse_t)
        eps = 8 * self.ta + (6 * lse_t.abs() + 6 * logV + 2).unsqueeze(-1)          # eps_j / u of the teacher's stream
        d = _w(self.p, (tt - ss).abs()) / torch.where(self.p > 0, self.p, torch.ones(()).double())  # |d_j|, 0 where p_j = 0
        S_d = (self.p * d).sum(-1)
        e_ratio = U * ((self.p * d * eps).sum(-1) + S_d * (self.p * eps).sum(-1) + (2 * self.depth + 4) * S_d
                       + 2 * (self.p * (self.ta + self.sa)).sum(-1)) + V * TINY * (1 + d.amax(-1))
        ratio = _w(self.p, tt - ss).sum(-1)
        kd_raw = D.kd_terms(logits, teacher, T)[0]
        self.b_kd = self.keep * (e_ratio + self.e_lse_t + self.e_lse_s + 2 * U * (ratio.abs() + lse_t.abs() + lse_s.abs()) + U * kd_raw.abs())
        picked = self.xa.gather(-1, lab.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
        zr = zs * lse * lse
        e_z = 2 * zs * lse.abs() * self.e_lse + 4 * U * zr.abs()
        self.b_z = self.keep * (0.5 * R.ulp(z, F32) + e_z)
        self.b_ce = self.keep * (0.5 * R.ulp(ce, F32) + self.e_lse + e_z + 4 * U * (lse.abs() + picked + zr.abs())
                                 + sm * U * (dsum + 3) * self.xa.sum(-1) / V)
        self.b_loss = self.keep * (0.5 * R.ulp(loss, F32) + (1 - alpha) * self.b_ce + alpha * T * T * self.b_kd
                                   + 4 * U * ((1 - alpha) * ce.abs() + alpha * T * T * kd.abs()))
        self.cfg, self.lab, self.lse = cfg, lab, lse
        self.lse_s, self.lse_t = lse_s, lse_t

    def check_fwd(self, outs, what):
        loss, kd, z, ce, lse, lse_s, lse_t = outs
        r = self.ref
        _check(lse, r[4], 0.5 * R.ulp(r[4], F32) + self.e_lse, f"{what} lse")
        _check(lse_s, r[5], 0.5 * R.ulp(r[5], F32) + self.e_lse_s, f"{what} lse_student_t")
        _check(lse_t, r[6], 0.5 * R.ulp(r[6], F32) + self.e_lse_t, f"{what} lse_teacher_t")
        _check(kd, r[1], 0.5 * R.ulp(r[1], F32) * self.keep + self.b_kd, f"{what} kd")
        _check(z, r[2], self.b_z, f"{what} z")
        _check(ce, r[3], self.b_ce, f"{what} ce")
        _check(loss, r[0], self.b_loss, f"{what} loss")

    def grad_bound(self, dl, ref, dtype):
        alpha, T, sm, scale, zs, ign = self.cfg
        V = ref.shape[-1]
        dla = (dl.double().cpu().expand(self.lab.shape).abs() * self.keep).unsqueeze(-1)
        g, k = dla * scale * (1 - alpha), dla * alpha * T
        zf = (1 + 2 * zs * self.lse).abs().unsqueeze(-1)
        onehot = torch.zeros_like(ref)
        rows = torch.nonzero((self.lab >= 0) & (self.lab < V)).squeeze(-1)
        onehot[rows, self.lab[rows]] = 1.0

        def rel(e, mag, l):
            return e.unsqueeze(-1) + U * (4 * mag + 3 * l.abs().unsqueeze(-1) + 2)
        b_ce = g * (self.P * zf * (rel(self.e_lse, self.xa, self.lse) + 6 * U) + 2 * zs * self.P * self.e_lse.unsqueeze(-1)
                    + 4 * U * (self.P * zf + onehot + sm / V))
        b_kd = k * (self.q * rel(self.e_lse_s, self.sa, self.lse_s) + self.p * rel(self.e_lse_t, self.ta, self.lse_t) + 4 * U * (self.q + self.p))
        mag = g * (self.P * zf + onehot + sm / V) + k * (self.q - self.p).abs()
        return 0.5 * R.ulp(ref, dtype) + b_ce + b_kd + U * mag + TINY * (g * zf + 2 * k + 2)

    def check_bwd(self, dlogits, dl, logits, teacher, labels, what):
        ref = D.kd_bwd(dl, logits, teacher, labels, *self.cfg)
        _check(dlogits, ref, self.grad_bound(dl, ref, logits.dtype), f"{what} dlogits")
        return ref


def _kd_all(logits, teacher, labels, dl, cfg, what):
    """the two launches (kd_fwd_kernel / kd_bwd_kernel) and the one launch (kd_fwd_bwd_kernel) on the same problem, each twice:
    both against fp64, each run against its repeat, the one launch against the two, bit for bit.  -> (bounds, outputs, dlogits)"""
    m = _mod()
    cfg = tuple(_f32(c) for c in cfg[:5]) + (cfg[5],)
    b = Bounds(logits, teacher, labels, cfg, _vector(logits, teacher))
    runs = []
    for _ in range(2):
        outs = m.distillation_fwd(logits, teacher, labels, *cfg)
        d = m.distillation_bwd(dl, logits, teacher, outs[4], outs[5], outs[6], labels, False, *cfg)
        runs.append(tuple(outs) + (d,))
    b.check_fwd(runs[0][:7], f"{what} two launches")
    b.check_bwd(runs[0][7], dl, logits, teacher, labels, f"{what} two launches")
    assert all(torch.equal(x, y) for x, y in zip(*runs)), f"{what}: two launches not deterministic"
    ign = (labels == cfg[5]).cpu()
    for name, t in zip(OUT_NAMES[:4], runs[0][:4]):
        assert not t.cpu()[ign].any(), f"{what}: {name} of an ignored row is not zero"
    assert not runs[0][7].cpu()[ign].any(), f"{what}: the gradient row of an ignored row is not zero"
    rows, s0, V = logits.shape[0], logits.stride(0), logits.shape[1]
    fused = []
    for _ in range(2):
        buf = torch.empty((rows, s0), dtype=logits.dtype, device="cuda")[:, s0 - V:]  # (in place, at the logits' row stride)
        buf.copy_(logits)
        outs = tuple(torch.empty(rows, device="cuda") for _ in range(7))
        m.distillation_fwd_bwd_(buf, teacher, labels, dl, *outs, *cfg)
        fused.append(outs + (buf,))
    assert all(torch.equal(x, y) for x, y in zip(*fused)), f"{what}: one launch not deterministic"
    for name, x, y in zip(OUT_NAMES + ("dlogits",), fused[0], runs[0]):
        assert torch.equal(x, y), f"{what}: {name} of the one launch differs from the two launches"
    return b, runs[0][:7], runs[0][7]


def _labels(V, rows, g):
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[1], labels[3], labels[4], labels[5] = -100, V + 5, -3, V - 1
    return labels


# the issue's widths: the pairs around 16 * 256 * VEC columns, where fat5_ce_fwd_bwd changes kernels (the distillation kernels
# have no compile-time width branch: the pairs differ in the trip count of the chunk loop and in its ragged last trip), widths that
# are no multiple of VEC (kd_fwd_kernel<X, false> / kd_bwd_kernel<X, false>; the one-launch entry falls back to the two launches)
# and a width at which most threads see no column
KD_V = [(BF16, 32768), (BF16, 32776), (F32, 16384), (F32, 16388), (BF16, 32767), (F32, 1001), (BF16, 64)]
KD_CFG = [(0.5, 1.0, 0.0, 1.0, 0.0), (0.9, 2.0, 0.1, 0.5, 1e-4), (1.0, 0.25, 0.0, 1.0, 0.0)]


@pytest.mark.parametrize("dtype,V", KD_V, ids=[f"{_name(d)}-{v}" for d, v in KD_V])
@pytest.mark.parametrize("cfg", KD_CFG, ids=["a.5-T1", "a.9-T2-sm-scale-z", "a1-T.25"])
def test_kd_widths(dtype, V, cfg):
    g = _gen("kd", dtype, V, cfg)
    rows = 6
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype).cuda()
    teacher = (torch.randn(rows, V, generator=g) * 4).to(dtype).cuda()
    labels = _labels(V, rows, g).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    _kd_all(logits, teacher, labels, dl, cfg + (-100,), f"{_name(dtype)} V={V} {cfg}")


@pytest.mark.parametrize("dtype,V", [(BF16, 32768), (BF16, 32776), (F32, 16384), (F32, 1001), (BF16, 64)])
@pytest.mark.parametrize("sm,scale,zs", [(0.0, 1.0, 0.0), (0.1, 0.5, 1e-4)])
def test_alpha_zero_is_cross_entropy(dtype, V, sm, scale, zs):
    """alpha = 0: loss, z, lse and dlogits have the bits of cross_entropy_fwd / cross_entropy_bwd, in the two launches and the one,
    and through the public operators"""
    m, ce = _mod(), importlib.import_module("flasht5_amd.cross_entropy_loss")
    g = _gen("a0", dtype, V, sm)
    rows = 6
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype).cuda()
    teacher = (torch.randn(rows, V, generator=g) * 4).to(dtype).cuda()
    labels = _labels(V, rows, g).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    loss, z, lse = ce.cross_entropy_fwd(logits, labels, None, sm, scale, zs, -100)
    d = ce.cross_entropy_bwd(dl, logits, lse, labels, False, sm, scale, zs, -100)
    cfg = (0.0, 2.0, sm, scale, zs, -100)
    outs = m.distillation_fwd(logits, teacher, labels, *cfg)
    d2 = m.distillation_bwd(dl, logits, teacher, outs[4], outs[5], outs[6], labels, False, *cfg)
    assert torch.equal(outs[0], loss) and torch.equal(outs[2], z) and torch.equal(outs[4], lse) and torch.equal(outs[3], loss)
    assert torch.equal(d2, d)
    buf = logits.clone()
    o1 = tuple(torch.empty(rows, device="cuda") for _ in range(7))
    m.distillation_fwd_bwd_(buf, teacher, labels, dl, *o1, *cfg)
    assert torch.equal(o1[0], loss) and torch.equal(buf, d)
    a = logits.clone().requires_grad_()
    b = logits.clone().requires_grad_()
    la, _, za = m.distillation_loss(a, teacher, labels, 0.0, 2.0, sm, scale, zs)
    lb, zb = ce.cross_entropy_loss(b, labels, None, sm, scale, zs)
    la.backward(dl)
    lb.backward(dl)
    assert torch.equal(la, lb) and torch.equal(za, zb) and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("dtype,V", [(BF16, 32768), (F32, 1001)])
def test_teacher_equals_student(dtype, V):
    """kd within its bound of 0, and with alpha = 1 (no cross-entropy part) the whole gradient within its bound of 0"""
    g = _gen("same", dtype, V)
    rows = 6
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype).cuda()
    labels = _labels(V, rows, g).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    b, outs, d = _kd_all(logits, logits.clone(), labels, dl, (1.0, 2.0, 0.0, 1.0, 0.0, -100), f"teacher = student {_name(dtype)} V={V}")
    assert float(b.ref[1].abs().max()) < 1e-12
    _check(outs[1], torch.zeros(rows).double(), b.b_kd + 0.0, "kd against 0")
    zero = torch.zeros(rows, V).double()
    _check(d, zero, b.grad_bound(dl, zero, dtype), "KD gradient against 0")


@pytest.mark.parametrize("dtype,V", [(BF16, 32768), (BF16, 40000), (F32, 16384), (BF16, 32767)])
@pytest.mark.parametrize("both", [False, True], ids=["teacher", "teacher+student"])
def test_masked_teacher_columns(dtype, V, both):
    """teacher columns at -inf -- a prefix (the first chunks of every thread: its running max starts at -inf), a suffix that covers
    whole thread chunks, odd pieces inside -- and with `both` the same columns -inf in the student too: nothing is NaN, the masked
    columns add 0 to kd, the ignored row is exactly zero (checked by _kd_all)"""
    g = _gen("mask", dtype, V, both)
    rows = 6
    v = VEC[dtype]
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    teacher = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    mask = torch.zeros(rows, V, dtype=torch.bool)
    mask[0, :3 * 256 * v + 5] = True            # a prefix: three whole rounds of every thread and a piece of the next
    mask[1, :V // 2] = True                     # (the ignored row)
    mask[2, V - 2 * 256 * v:] = True            # a suffix of two whole rounds of chunks
    mask[3, 256 * v - 3:V - 7] = True           # everything but a head and a tail
    mask[4, ::2] = True                         # every other column
    mask[5, 1:] = True                          # one column left
    teacher[mask] = -math.inf
    if both:
        logits[mask] = -math.inf
    labels = torch.tensor([V - 1, -100, 3, V + 5, 1, 0])   # (in-range labels sit on unmasked columns)
    dl = torch.randn(rows, generator=g).cuda()
    _, outs, d = _kd_all(logits.cuda(), teacher.cuda(), labels.cuda(), dl, (0.7, 2.0, 0.0, 1.0, 1e-4, -100),
                         f"masked {_name(dtype)} V={V} both={both}")
    assert all(bool(torch.isfinite(t).all()) for t in outs) and bool(torch.isfinite(d.float()).all())


@pytest.mark.parametrize("dtype,V", [(BF16, 32768), (BF16, 32776), (F32, 1001)])
def test_ignored_rows_are_selected_to_zero(dtype, V):
    """ignored rows whose teacher logits are -inf everywhere, NaN, or whose student logits are NaN (what a padded position of the
    dense path may hold): loss, kd, z, ce and the gradient row are exactly zero in the two launches and the one, and the other
    rows have the bits they have without that garbage"""
    m = _mod()
    g = _gen("ignored", dtype, V)
    rows = 6
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    teacher = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    labels = torch.tensor([3, -100, -100, V - 1, -100, 0]).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    cfg = (0.5, 2.0, _f32(0.1), 1.0, _f32(1e-4), -100)

    def run(s, t):
        s, t = s.cuda(), t.cuda()
        outs = m.distillation_fwd(s, t, labels, *cfg)
        d = m.distillation_bwd(dl, s, t, outs[4], outs[5], outs[6], labels, False, *cfg)
        buf = s.clone()
        o1 = tuple(torch.empty(rows, device="cuda") for _ in range(7))
        m.distillation_fwd_bwd_(buf, t, labels, dl, *o1, *cfg)
        assert all(torch.equal(x[[0, 3, 5]], y[[0, 3, 5]]) for x, y in zip(o1[:4] + (buf,), tuple(outs[:4]) + (d,)))
        assert not buf[[1, 2, 4]].any()
        return outs[:4], d
    clean_outs, clean_d = run(logits, teacher)
    bad_s, bad_t = logits.clone(), teacher.clone()
    bad_t[1] = -math.inf
    bad_t[2] = math.nan
    bad_s[4] = math.nan
    outs, d = run(bad_s, bad_t)
    ign = [1, 2, 4]
    for name, t in zip(OUT_NAMES[:4], outs):
        assert not t[ign].any(), f"{name} of an ignored row is not zero"
    assert not d[ign].any(), "the gradient row of an ignored row is not zero"
    assert all(torch.equal(a, b) for a, b in zip(outs, clean_outs)) and torch.equal(d, clean_d)


@pytest.mark.parametrize("V", [32768, 32776, 1001])
def test_fp16_extremes_small_temperature(V):
    """fp16 logits at +-6e4 with T = 0.25 (exponents of +-2.4e5 before the running max is taken off): everything finite and
    within the bounds"""
    g = _gen("f16", V)
    rows = 6
    logits = ((torch.rand(rows, V, generator=g) < 0.5).float() * 2 - 1) * 6e4
    teacher = ((torch.rand(rows, V, generator=g) < 0.5).float() * 2 - 1) * 6e4
    logits[0] = torch.randn(V, generator=g) * 3e4          # (a spread of magnitudes besides the two-valued rows)
    teacher[2] = torch.randn(V, generator=g) * 3e4
    logits, teacher = logits.clamp(-6e4, 6e4).to(F16).cuda(), teacher.clamp(-6e4, 6e4).to(F16).cuda()
    labels = _labels(V, rows, g).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    _, outs, d = _kd_all(logits, teacher, labels, dl, (1.0, 0.25, 0.0, 1.0, 0.0, -100), f"fp16 extremes V={V}")
    assert all(bool(torch.isfinite(t).all()) for t in outs) and bool(torch.isfinite(d.float()).all())


@pytest.mark.parametrize("dtype,V", [(BF16, 4096), (F32, 1000), (BF16, 1003)])
def test_strides_in_place_and_guards(dtype, V):
    """student rows at one stride, teacher rows at another, dlogits in place and out of place, through the C ABI so that the views
    reach the kernels as they are; guard elements around every output keep their bits"""
    m = _mod()
    g = _gen("stride", dtype, V)
    rows, pad = 6, 16
    sbuf = torch.full((rows, V + 2 * pad), 7.0, dtype=dtype, device="cuda")
    tbuf = torch.full((rows, V + 5 * pad), -5.0, dtype=dtype, device="cuda")
    logits, teacher = sbuf[:, pad:pad + V], tbuf[:, 3 * pad:3 * pad + V]
    logits.copy_((torch.randn(rows, V, generator=g) * 4).to(dtype))
    teacher.copy_((torch.randn(rows, V, generator=g) * 4).to(dtype))
    labels = _labels(V, rows, g).cuda()
    dl = torch.randn(rows, generator=g).cuda()
    cfg = tuple(_f32(c) for c in (0.6, 2.0, 0.1, 0.5, 1e-4)) + (-100,)
    b = Bounds(logits, teacher, labels, cfg, _vector(logits, teacher))
    keep_s, keep_t = sbuf.clone(), tbuf.clone()
    per_row = torch.full((7, rows + 2), 3.0, device="cuda")
    outs = [per_row[i, 1:rows + 1] for i in range(7)]
    dbuf = torch.full((rows, V + 3 * pad), 9.0, dtype=dtype, device="cuda")
    dlogits = dbuf[:, pad:pad + V]
    kw = dict(losses=outs[0], kd=outs[1], z=outs[2], ce=outs[3], lse=outs[4], lse_s=outs[5], lse_t=outs[6])
    m._launch("fat5_kd_fwd", logits, teacher, labels, cfg, **kw)
    m._launch("fat5_kd_bwd", logits, teacher, labels, cfg, dlosses=dl, lse=outs[4], lse_s=outs[5], lse_t=outs[6], dlogits=dlogits)
    b.check_fwd(outs, "strided")
    b.check_bwd(dlogits, dl, logits, teacher, labels, "strided")
    assert torch.equal(sbuf, keep_s) and torch.equal(tbuf, keep_t), "an input changed"
    assert bool((per_row[:, 0] == 3.0).all()) and bool((per_row[:, -1] == 3.0).all()), "a per-row guard changed"
    assert bool((dbuf[:, :pad] == 9.0).all()) and bool((dbuf[:, pad + V:] == 9.0).all()), "a dlogits guard changed"
    # the one launch, out of place at a third stride, then in place on the student
    per_row2 = torch.full((7, rows + 2), 3.0, device="cuda")
    outs2 = [per_row2[i, 1:rows + 1] for i in range(7)]
    kw2 = dict(losses=outs2[0], kd=outs2[1], z=outs2[2], ce=outs2[3], lse=outs2[4], lse_s=outs2[5], lse_t=outs2[6])
    dbuf2 = torch.full((rows, V + 3 * pad), 9.0, dtype=dtype, device="cuda")
    m._launch("fat5_kd_fwd_bwd", logits, teacher, labels, cfg, dlosses=dl, dlogits=dbuf2[:, pad:pad + V], **kw2)
    assert torch.equal(per_row2, per_row) and torch.equal(dbuf2, dbuf) and torch.equal(sbuf, keep_s)
    per_row3 = torch.full((7, rows + 2), 3.0, device="cuda")
    outs3 = [per_row3[i, 1:rows + 1] for i in range(7)]
    kw3 = dict(losses=outs3[0], kd=outs3[1], z=outs3[2], ce=outs3[3], lse=outs3[4], lse_s=outs3[5], lse_t=outs3[6])
    m._launch("fat5_kd_fwd_bwd", logits, teacher, labels, cfg, dlosses=dl, dlogits=logits, **kw3)
    assert torch.equal(per_row3, per_row) and torch.equal(logits, dlogits) and torch.equal(tbuf, keep_t)
    assert torch.equal(sbuf[:, :pad], keep_s[:, :pad]) and torch.equal(sbuf[:, pad + V:], keep_s[:, pad + V:]), "a guard of the in-place rows changed"


# ------------------------------------------------------------------------------------------------------------------------------
# lm_head_distillation
# ------------------------------------------------------------------------------------------------------------------------------
def _parity(ref, u):
    """the project's parity bound (tests/parity_cases.py): (1e-3 + u half-ulps of bf16) * max(1, max|ref|)"""
    return (1e-3 + u * 2.0 ** -8) * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("reduction", ["none", "mean"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_lm_head_distillation(dtype, reduction):
    """rows 300 in chunks of 128 (two full chunks and a short one), student width 64, teacher width 128, V 2048: losses, dh and dW
    against the fp64 composition (fp64 logits from the rounded hidden states and weights); no teacher gradient"""
    from flasht5_amd import lm_head_distillation
    g = _gen("lmhead", dtype)
    rows, V, ds, dt = 300, 2048, 64, 128
    h = torch.randn(rows, ds, generator=g).to(dtype).cuda().requires_grad_()
    w = (torch.randn(V, ds, generator=g) * ds ** -0.5).to(dtype).cuda().requires_grad_()
    th = torch.randn(rows, dt, generator=g).to(dtype).cuda().requires_grad_()
    tw = (torch.randn(V, dt, generator=g) * dt ** -0.5).to(dtype).cuda().requires_grad_()
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[::7] = -100
    labels = labels.cuda()
    alpha, T, sm, zs = 0.5, 2.0, 0.1, _f32(1e-4)
    sm = _f32(sm)
    logits64 = h.detach().double().cpu() @ w.detach().double().cpu().t()
    tlogits64 = th.detach().double().cpu() @ tw.detach().double().cpu().t()
    ref = D.kd_fwd(logits64, tlogits64, labels, alpha, T, sm, 1.0, zs)
    out = lm_head_distillation(h, w, th, tw, labels, alpha, T, sm, 1.0, zs, chunk_rows=128, reduction=reduction)
    if reduction == "none":
        dl = torch.randn(rows, generator=g).cuda()
        for got, want, name in zip(out, ref[:3], OUT_NAMES):
            assert got.shape == (rows,) and got.dtype == F32
            assert float((got.detach().double().cpu() - want).abs().max()) <= _parity(want, 1), name
        out[0].backward(dl)
    else:
        dl = torch.ones(rows).cuda()
        for got, want, name in zip(out, ref[:3], OUT_NAMES):
            assert got.dim() == 0
            assert abs(float(got.detach()) - float(want.mean())) <= _parity(want.mean(), 1), name
        out[0].backward(torch.tensor(float(rows)).cuda())   # (the upstream scalar undoes the 1 / rows: per-row gradients of 1)
    dlog = D.kd_bwd(dl, logits64, tlogits64, labels, alpha, T, sm, 1.0, zs)
    dh_ref, dw_ref = dlog @ w.detach().double().cpu(), dlog.t() @ h.detach().double().cpu()
    assert float((h.grad.double().cpu() - dh_ref).abs().max()) <= _parity(dh_ref, 3)
    assert float((w.grad.double().cpu() - dw_ref).abs().max()) <= _parity(dw_ref, 3)
    assert not out[1].requires_grad and not out[2].requires_grad
    assert tw.grad is None and th.grad is None


# ------------------------------------------------------------------------------------------------------------------------------
# DistilledFAT5
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def torch_deterministic():
    """the exact tests compare two runs bit for bit: torch's deterministic mode, as in tests/test_packed_train_gpu.py (the backward
    of the table lookup behind the T5 bias is an index_add_ with atomics otherwise)"""
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


B, L_ENC, L_DEC = 3, 24, 16


def _models(seed=3, alpha=0.5, T=2.0, **flags):
    from flasht5_amd import DistilledFAT5, FAT5Config, FAT5ForConditionalGeneration
    kw = dict(vocab_size=512, num_layers=2, num_decoder_layers=2, num_heads=2)
    torch.manual_seed(seed)
    student = FAT5ForConditionalGeneration(FAT5Config(d_model=64, d_kv=32, d_ff=128, **kw, **flags)).cuda().bfloat16()
    teacher = FAT5ForConditionalGeneration(FAT5Config(d_model=128, d_kv=64, d_ff=256, **kw)).cuda().bfloat16()
    return DistilledFAT5(student, teacher, alpha=alpha, temperature=T)


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 512, (B, L_ENC), generator=g).cuda(), torch.randint(1, 512, (B, L_DEC), generator=g).cuda()


@pytest.mark.parametrize("fuse", [False, True], ids=["full-logits", "fuse_lm_head_ce"])
def test_distilled_loss_is_the_composition(fuse):
    """the loss, last_kd_loss and last_ce_loss equal the fp64 composition on the two models' own decoder states (both lm_heads in
    fp64), under the parity bound of a bf16 forward; the teacher keeps no gradient"""
    model = _models(fuse_lm_head_ce=fuse)
    ids, labels = _batch()
    labels[1, 10:] = -100
    loss = model(ids, labels)
    loss.backward()
    c = model.student.config
    with torch.no_grad():
        dec, lab = model.student._decoder_states(None, ids, labels)
        tdec, _ = model.teacher._decoder_states(None, ids, labels)
    s64 = dec.double().cpu().reshape(-1, 64) @ model.student.lm_head.weight.detach().double().cpu().t()
    t64 = tdec.double().cpu().reshape(-1, 128) @ model.teacher.lm_head.weight.detach().double().cpu().t()
    ref = D.kd_fwd(s64, t64, lab.reshape(-1), 0.5, 2.0, _f32(c.label_smoothing), 1.0, _f32(c.z_loss))
    for got, want, name in ((loss, ref[0], "loss"), (model.last_kd_loss, ref[1], "kd"), (model.last_ce_loss, ref[3], "ce")):
        assert got.dim() == 0 and got.is_cuda and got.requires_grad == (name == "loss")
        assert abs(float(got.detach()) - float(want.mean())) <= _parity(want.mean(), 1), (name, float(got.detach()), float(want.mean()))
    assert all(p.grad is not None for p in model.student.parameters())
    assert all(p.grad is None for p in model.teacher.parameters())


def test_train_step_moves_the_student_only_and_lowers_kd():
    """30 train_steps on one fixed batch: last_kd_loss falls, every student parameter moves, no teacher parameter does or has a
    gradient.  alpha = 1: the loss IS T^2 kd, so descent has to lower it; with a cross-entropy share the two terms pull apart on a
    batch of random labels against a randomly initialised teacher (the student sharpens on the labels, away from the teacher's
    flat distribution), and kd alone need not fall"""
    from flasht5_amd import AdamWScale, train_step
    model = _models(alpha=1.0)
    ids, labels = _batch()
    opt = AdamWScale(model.parameters(), lr=5e-3)
    before_s = [p.detach().clone() for p in model.student.parameters()]
    before_t = [p.detach().clone() for p in model.teacher.parameters()]
    kds = []
    for _ in range(30):
        train_step(model, ids, labels, opt)
        kds.append(model.last_kd_loss)          # (device scalars: read once, after the loop)
    kds = [float(k) for k in kds]
    print(f"[distill] last_kd_loss over 30 steps: first {kds[0]:.4f} last {kds[-1]:.4f}")
    assert all(math.isfinite(k) for k in kds) and kds[-1] < kds[0]
    assert all(not torch.equal(p.detach(), b) for p, b in zip(model.student.parameters(), before_s))
    assert all(torch.equal(p.detach(), b) and p.grad is None for p, b in zip(model.teacher.parameters(), before_t))


@pytest.mark.parametrize("fuse", [False, True], ids=["full-logits", "fuse_lm_head_ce"])
def test_padding_garbage_changes_no_bit(fuse, torch_deterministic):
    """a right-padded batch: the loss and every student gradient keep their bits when the padded ids and labels hold other
    values (one pack plan, made by the student; both models run over the same valid tokens)"""
    model = _models(fuse_lm_head_ce=fuse)
    enc_lens, dec_lens = (24, 9, 1), (16, 7, 2)
    g = torch.Generator().manual_seed(4)
    am = torch.zeros(B, L_ENC, dtype=torch.bool)
    dm = torch.zeros(B, L_DEC, dtype=torch.bool)
    for b_, (e, d) in enumerate(zip(enc_lens, dec_lens)):
        am[b_, :e], dm[b_, :d] = True, True
    ids0, lab0 = torch.randint(1, 512, (B, L_ENC), generator=g), torch.randint(1, 512, (B, L_DEC), generator=g)
    ids1 = torch.where(am, ids0, torch.randint(0, 512, (B, L_ENC), generator=g))
    lab1 = torch.where(dm, lab0, torch.randint(0, 512, (B, L_DEC), generator=g))
    lab1[2, 5] = -100
    ids0, lab0 = torch.where(am, ids0, torch.zeros(())).long(), torch.where(dm, lab0, torch.full((), -100)).long()
    assert not torch.equal(ids0, ids1) and not torch.equal(lab0, lab1)
    runs = []
    for ids, lab in ((ids0, lab0), (ids1, lab1)):
        model.zero_grad(set_to_none=True)
        loss = model(ids.cuda(), lab.cuda(), attention_mask=am.cuda(), decoder_attention_mask=dm.cuda())
        loss.backward()
        runs.append((loss.detach().clone(), model.last_kd_loss.clone(), {n: p.grad.clone() for n, p in model.named_parameters()}))
    (l0, k0, g0), (l1, k1, g1) = runs
    assert torch.isfinite(l0) and torch.equal(l0, l1) and torch.equal(k0, k1)
    assert g0.keys() == g1.keys() and all(torch.equal(g0[n], g1[n]) for n in g0)
    assert all(p.grad is None for p in model.teacher.parameters())


def test_graphed_train_step_gives_the_eager_losses(torch_deterministic):
    """GraphedTrainStep takes the module as it is: from the same state and on the same batch, two eager warm-up calls and four
    replays give the six losses (and last_kd_loss values) of six eager train_steps, bit for bit"""
    from flasht5_amd import AdamWScale, train_step, GraphedTrainStep
    ids, labels = _batch()
    runs = []
    for graphed in (False, True):
        model = _models(seed=11)
        opt = AdamWScale(model.parameters(), lr=2e-3, max_grad_norm=1.0)
        step = GraphedTrainStep(model, opt, warmup=2) if graphed else (lambda i, l: train_step(model, i, l, opt, max_grad_norm=None))
        losses = []
        for _ in range(6):
            losses.append((step(ids, labels).clone(), model.last_kd_loss.clone()))
        if graphed:
            assert step.graphs is not None
            step.close()
        runs.append([(float(a), float(b)) for a, b in losses])
    print(f"[distill-graphed] eager {runs[0]}\n[distill-graphed] graph {runs[1]}")
    assert all(math.isfinite(a) for a, _ in runs[0])
    assert runs[0] == runs[1]
