"""CPU tests of knowledge distillation: the fp64 restatements of tests/distill_fp64.py against
torch.nn.functional.kl_div + cross_entropy, the C ABI's exports, the ctypes mirror of fat5_kd_params and every argument check of
the three entry points (all before any launch: fake, aligned pointers are enough), and the Python layers' own rejections."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import distill_fp64 as D

ENTRIES = ("fat5_kd_fwd", "fat5_kd_bwd", "fat5_kd_fwd_bwd")


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ------------------------------------------------------------------------------------------------------------------------------
def _rows(V=97, rows=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(rows, V, generator=g) * 3).double()
    t = (torch.randn(rows, V, generator=g) * 3).double()
    y = torch.randint(0, V, (rows,), generator=g)
    return s, t, y


@pytest.mark.parametrize("alpha,T,sm", [(0.5, 1.0, 0.0), (0.9, 2.0, 0.1), (1.0, 0.25, 0.0), (0.0, 3.0, 0.0)])
def test_restatement_matches_torch(alpha, T, sm):
    s, t, y = _rows()
    y[2] = -100
    sr = s.clone().requires_grad_()
    kd = F.kl_div(F.log_softmax(sr / T, -1), F.log_softmax(t / T, -1), reduction="none", log_target=True).sum(-1)
    ce = F.cross_entropy(sr, y, reduction="none", label_smoothing=sm, ignore_index=-100)
    keep = (y != -100).double()
    loss = (1 - alpha) * ce + alpha * T * T * kd * keep
    dl = torch.linspace(0.5, 1.5, s.shape[0]).double()
    (grad,) = torch.autograd.grad(loss, sr, dl)
    got = D.kd_fwd(s, t, y, alpha, T, sm)
    assert torch.allclose(got[0], loss.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got[1], (kd * keep).detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got[3], ce.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got[5], torch.logsumexp(s / T, -1)) and torch.allclose(got[6], torch.logsumexp(t / T, -1))
    assert got[0][2] == 0 and got[1][2] == 0 and got[2][2] == 0
    d = D.kd_bwd(dl, s, t, y, alpha, T, sm)
    assert torch.allclose(d, grad, rtol=1e-11, atol=1e-13)
    assert not d[2].any()


def test_restatement_scale_and_z_loss_act_on_ce_only():
    s, t, y = _rows(seed=1)
    base = D.kd_fwd(s, t, y, 0.7, 2.0)
    full = D.kd_fwd(s, t, y, 0.7, 2.0, 0.1, 0.5, 1e-3)
    assert torch.equal(base[1], full[1]) and torch.equal(base[5], full[5]) and torch.equal(base[6], full[6])
    lse = torch.logsumexp(0.5 * s, -1)
    assert torch.allclose(full[2], 1e-3 * lse * lse) and torch.allclose(full[4], lse)
    assert torch.allclose(full[0], 0.3 * full[3] + 0.7 * 4.0 * full[1])


def test_restatement_masked_teacher_columns():
    """t_j = -inf adds 0 to kd and alpha T (q_j - 0) to the gradient (a descent step lowers q_j), also where s_j = -inf too; kd is that of the renormalised rest"""
    s, t, y = _rows(V=40, rows=3, seed=2)
    t[:, :8] = -math.inf
    s2 = s.clone()
    s2[:, :4] = -math.inf
    for ss in (s, s2):
        loss, kd, *_ = D.kd_fwd(ss, t, y, 1.0, 2.0)
        assert torch.isfinite(loss).all() and (kd >= 0).all()
        d = D.kd_bwd(torch.ones(3), ss, t, y, 1.0, 2.0)
        assert torch.isfinite(d).all()
        q = torch.softmax(ss / 2.0, -1)
        assert torch.allclose(d[:, :8], 2.0 * q[:, :8], rtol=1e-12, atol=0)   # alpha T (q_j - 0)
        # the same kd from the definition over the unmasked columns only
        p = torch.softmax(t[:, 8:] / 2.0, -1)
        want = (p * (torch.log(p) - torch.log_softmax(ss / 2.0, -1)[:, 8:])).sum(-1)
        assert torch.allclose(kd, want, rtol=1e-12)


def test_restatement_teacher_equals_student():
    s, _, y = _rows(seed=3)
    loss, kd, z, ce, *_ = D.kd_fwd(s, s, y, 1.0, 0.5)
    assert kd.abs().max() < 1e-14 and D.kd_bwd(torch.ones(7), s, s, y, 1.0, 0.5).abs().max() < 1e-15


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.KdParams()
    base = 1 << 20  # (never dereferenced: every call below is rejected before a launch)
    p.dtype, p.rows, p.n_cols = _lib.FAT5_BF16, 4, 64
    for i, f in enumerate(("logits", "teacher_logits", "labels", "dlosses", "losses", "kd_losses", "z_losses", "ce_losses", "lse",
                           "lse_student_t", "lse_teacher_t", "dlogits")):
        setattr(p, f, base + 4096 * i)
    p.row_stride = p.teacher_row_stride = p.dlogits_row_stride = 64
    p.dloss_stride, p.ignore_index = 1, -100
    p.alpha, p.temperature, p.label_smoothing, p.logit_scale, p.lse_square_scale = 0.5, 2.0, 0.0, 1.0, 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_exports_and_struct_size(lib):
    from flasht5_amd import _lib
    for name in ENTRIES + ("fat5_sizeof_kd_params",):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_kd_params() == ctypes.sizeof(_lib.KdParams) == 184
    assert lib.fat5_version() == 114


BAD_ALL = [
    (dict(dtype=7), "dtype"), (dict(dtype=-1), "dtype"), (dict(rows=0), "rows"), (dict(rows=-3), "rows"), (dict(rows=1 << 31), "rows"),
    (dict(n_cols=0), "n_cols"), (dict(n_cols=-1), "n_cols"), (dict(n_cols=1 << 31), "n_cols"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=math.inf), "temperature"),
    (dict(temperature=math.nan), "temperature"), (dict(alpha=-0.01), "alpha"), (dict(alpha=1.01), "alpha"), (dict(alpha=math.nan), "alpha"),
    (dict(logits=None), "logits"), (dict(logits=(1 << 20) + 1), "logits"), (dict(teacher_logits=None), "teacher_logits"),
    (dict(labels=None), "labels"), (dict(labels=(1 << 20) + 4), "labels"), (dict(lse=None), "lse"),
    (dict(lse_student_t=None), "lse_student_t"), (dict(lse_teacher_t=None), "lse_teacher_t"), (dict(ce_losses=(1 << 20) + 2), "ce_losses"),
]
BAD_FWD = [(dict(losses=None), "losses"), (dict(kd_losses=None), "kd_losses"), (dict(z_losses=None), "z_losses")]
BAD_BWD = [(dict(dlosses=None), "dlosses"), (dict(dlogits=None), "dlogits"), (dict(dlogits=(1 << 20) + 1), "dlogits"),
           (dict(n_cols=256 * 8 * 65535 + 1), "columns")]


@pytest.mark.parametrize("entry,bad,msg", [(e, b, m) for e in ENTRIES for b, m in BAD_ALL] +
                         [(e, b, m) for e in ("fat5_kd_fwd", "fat5_kd_fwd_bwd") for b, m in BAD_FWD] +
                         [(e, b, m) for e in ("fat5_kd_bwd", "fat5_kd_fwd_bwd") for b, m in BAD_BWD[:3]] +
                         [("fat5_kd_bwd", *BAD_BWD[3]), ("fat5_kd_fwd_bwd", dict(n_cols=256 * 8 * 65535 + 1), "columns")])
def test_rejects_before_launch(lib, entry, bad, msg):
    p = _params(**bad)
    fn = getattr(lib, entry)
    assert fn(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode() and entry[5:] in lib.fat5_last_error().decode()
    assert fn(None, None) == -1 and "null params" in lib.fat5_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layers
# ------------------------------------------------------------------------------------------------------------------------------
def test_operators_reject_before_device_work():
    import flasht5_amd
    from flasht5_amd import distillation_loss, lm_head_distillation
    assert flasht5_amd.DistilledFAT5 is not None
    x = torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        distillation_loss(x, x, torch.zeros(4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="HIP device"):
        lm_head_distillation(x, torch.zeros(32, 16), x, torch.zeros(32, 16), torch.zeros(4, dtype=torch.long))


def test_distilled_model_holds_the_teacher_outside_the_tree():
    from flasht5_amd import DistilledFAT5, FAT5Config, FAT5ForConditionalGeneration
    kw = dict(vocab_size=64, d_kv=16, d_ff=32, num_heads=2, num_layers=1, num_decoder_layers=1)
    student = FAT5ForConditionalGeneration(FAT5Config(d_model=16, **kw))
    teacher = FAT5ForConditionalGeneration(FAT5Config(d_model=32, **kw)).train()
    m = DistilledFAT5(student, teacher, alpha=0.3, temperature=2.0)
    assert not teacher.training and m.teacher is teacher
    mine = {id(p) for p in m.parameters()}
    assert mine == {id(p) for p in student.parameters()} and not any(id(p) in mine for p in teacher.parameters())
    assert all(k.startswith("student.") for k in m.state_dict())
    m.train()
    assert student.training and not teacher.training
    assert [id(t) for t in m.rpe_tables()] == [id(t) for t in student.rpe_tables()]
    for name, val in (("vocab_size", 65), ("decoder_start_token_id", 3), ("pad_token_id", 2)):
        other = FAT5ForConditionalGeneration(FAT5Config(d_model=32, **{**kw, name: val}))
        with pytest.raises(ValueError, match=name):
            DistilledFAT5(student, other)
    for bad in (dict(alpha=1.5), dict(alpha=-0.1), dict(temperature=0.0), dict(temperature=math.inf)):
        with pytest.raises(ValueError):
            DistilledFAT5(student, teacher, **bad)
    # a cast of the module reaches the student only: the mismatch is named before any model runs
    m.bfloat16()
    assert student.lm_head.weight.dtype == torch.bfloat16 and teacher.lm_head.weight.dtype == torch.float32
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="outside the module tree"):
        m(ids, ids)
