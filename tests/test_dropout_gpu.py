"""GPU tests of dropout (flasht5_amd/dropout.py, csrc/dropout_kernels.h).  Every comparison is BITWISE:

  * `dropout` / `dropout_add`, forward and backward, against the host restatement tests/dropout_ref.py (numpy Philox mask uploaded,
    fp32 scale, one rounding) -- three dtypes, rows 1 / 5 / 9, n 8 / 100 / 768 (vector and element paths), p 0 / 0.1 / 0.5, a row
    stride larger than n, and elem_offset = 2^32 - 3 on a (2, 8) operand (the 64-bit block index, an offset that is no multiple of 4);
  * `dropout_add_rms_layernorm`, forward and backward, against `dropout` followed by `fused_add_rms_layernorm`, at one n per
    launch path of csrc/api_dropout.hip (bf16: forward register NCH 2 / 4, generic vector, element -- 768, 1032, 2056, 100; backward
    NCH 2 / 4 / 8 / 16, element because of n and because of width -- 768, 2048, 4096, 4104, 100, 8200; fp32 shifts the thresholds)
    and rows 1 and 5;
  * a captured graph holding a `dropout`, replayed around an increment of the step buffer;
  * the model (2 + 2 layers, d_model 64, 4 heads, d_ff 128, vocabulary 128, B 2, L 16, bf16): eval against a dropout_rate 0 model,
    the plain path against fuse_add_norm, repeatability in the step counter, and all six kinds of sites with their numbering
    against the three operators monkeypatched by torch restatements that upload tests/dropout_ref.py's masks -- also on a padded
    batch.

The model comparisons run under torch.use_deterministic_algorithms (torch's embedding and index_select backward otherwise
accumulate with atomics, which no bitwise comparison of two runs survives)."""
import numpy as np
import pytest
import torch

import dropout_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SEED = 0x9E3779B97F4A7C15   # (a key with its top bit set: the operator schema carries it as a negative int64)


def _dev():
    return torch.device("cuda:0")


def _step(v):
    return torch.tensor([v], dtype=torch.int64, device=_dev())


def _rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 3).to(dtype).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_dropout_and_dropout_add_equal_the_restatement(dtype):
    from flasht5_amd import dropout, dropout_add
    site = 0
    for rows in (1, 5, 9):
        for n in (8, 100, 768):
            x, r, dy = (_rand((rows, n), dtype, 10 * rows + n + k) for k in range(3))
            for p in (0.0, 0.1, 0.5):
                site += 1
                step = _step(3 + site)
                keep = torch.from_numpy(R.keep_mask(rows, n, p, SEED, 3 + site, site)).to(_dev())
                xg = x.clone().requires_grad_()
                y = dropout(xg, p, SEED, step, site)
                assert same(y, R.apply_mask(x, keep, p)), (rows, n, p)
                (dx,) = torch.autograd.grad(y, xg, dy)
                assert same(dx, R.apply_mask(dy, keep, p)), (rows, n, p)
                xg, rg = x.clone().requires_grad_(), r.clone().requires_grad_()
                y = dropout_add(xg, rg, p, SEED, step, site)
                assert same(y, r + R.apply_mask(x, keep, p)), (rows, n, p)
                dx, dr = torch.autograd.grad(y, (xg, rg), dy)
                assert same(dx, R.apply_mask(dy, keep, p)) and same(dr, dy), (rows, n, p)
                if p == 0.0:
                    assert same(dropout(x, p, SEED, step, site), x)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_row_stride_and_higher_rank(dtype):
    """rows that are not contiguous (stride 776 > n = 768; stride 104 on the element path) and a 3-D operand: e counts logical
    elements, strides do not enter"""
    from flasht5_amd import dropout, dropout_add
    for n, pitch in ((768, 776), (100, 104)):
        big, rbig = _rand((5, pitch), dtype, n), _rand((5, pitch + 8), dtype, n + 1)
        x, r = big[:, :n], rbig[:, :n]
        assert x.stride(0) == pitch and not x.is_contiguous()
        keep = torch.from_numpy(R.keep_mask(5, n, 0.1, SEED, 7, 2)).to(_dev())
        assert same(dropout(x, 0.1, SEED, _step(7), 2), R.apply_mask(x, keep, 0.1))
        assert same(dropout_add(x, r, 0.1, SEED, _step(7), 2), r + R.apply_mask(x, keep, 0.1))
    x3 = _rand((2, 3, 64), dtype, 5)
    keep = torch.from_numpy(R.keep_mask(6, 64, 0.5, SEED, 0, 9)).to(_dev())
    assert same(dropout(x3, 0.5, SEED, _step(0), 9), R.apply_mask(x3, keep, 0.5))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_elem_offset_crosses_the_32_bit_block_index(dtype):
    """elem_offset = 2^32 - 3 on a (2, 8) operand: e runs over 2^32, so the block index j = e >> 2 carries past 2^30 into the
    counter's words exactly as the contract says, and e & 3 != 0 takes the unaligned form of the vector path"""
    from flasht5_amd import dropout
    off = (1 << 32) - 3
    x, dy = _rand((2, 8), dtype, 1), _rand((2, 8), dtype, 2)
    for off in ((1 << 32) - 3, (1 << 34) - 6, (1 << 34) - 8):   # (j crossing 2^32 -- the counter's second word -- unaligned and aligned)
        for p in (0.1, 0.5):
            keep = torch.from_numpy(R.keep_mask(2, 8, p, SEED, 1, 4, elem_offset=off)).to(_dev())
            xg = x.clone().requires_grad_()
            y = dropout(xg, p, SEED, _step(1), 4, elem_offset=off)
            assert same(y, R.apply_mask(x, keep, p)), (off, p)
            assert same(torch.autograd.grad(y, xg, dy)[0], R.apply_mask(dy, keep, p)), (off, p)


def _fused_vs_unfused(dtype, wdtype, rows, n, p, use_h=True, use_y=True):
    from flasht5_amd import dropout, dropout_add_rms_layernorm, fused_add_rms_layernorm
    h0, delta, gh, gy = (_rand((rows, n), dtype, 100 * rows + n + k) for k in range(4))
    w = (1 + 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(n))).to(wdtype).to(_dev())
    step, site = _step(n), rows
    outs = []
    for fused in (True, False):
        a, b, c = h0.clone().requires_grad_(), delta.clone().requires_grad_(), w.clone().requires_grad_()
        if fused:
            h, y = dropout_add_rms_layernorm(a, b, c, 1e-6, p, SEED, step, site)
        else:
            h, y = fused_add_rms_layernorm(a, dropout(b, p, SEED, step, site), c, 1e-6)
        tops = [(t, g) for t, g, use in ((h, gh, use_h), (y, gy, use_y)) if use]
        grads = torch.autograd.grad([t for t, _ in tops], (a, b, c), [g for _, g in tops], allow_unused=True)
        outs.append((h, y) + grads)
    names = ("h", "y", "dh", "ddelta", "dw")
    for name, f, u in zip(names, *outs):
        if f is None or u is None:
            assert f is None and u is None, name
            continue
        assert same(f, u), (name, str(dtype), rows, n, (_bits(f) != _bits(u)).sum().item())
    # and the mask is the contract's: h against the host restatement
    keep = torch.from_numpy(R.keep_mask(rows, n, p, SEED, n, site)).to(_dev())
    assert same(outs[0][0], h0 + R.apply_mask(delta, keep, p)), ("h vs host", rows, n)


@pytest.mark.parametrize("n", [768, 1032, 2048, 2056, 4096, 4104, 100, 8200])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_dropout_add_rms_layernorm_equals_the_unfused_composition(dtype, n):
    """bf16 at 768 ... 100: the cases of the kernels' specification, rows 1 and 5.  Added here: fp32 (no rounding hides a differently
    fused operation) and n = 8200 (the element path taken for width).  The element path of the backward -- the parent's as well --
    sums dw with fp32 LDS atomics in arrival order, so its fp32 dw is not a function of the inputs once a column has three or more
    terms (measured: 11 of 100, 1291 of 4104, 2126 of 8200 fp32 values differ in the last bit between the two kernels at 5 rows;
    dx and ddelta are exact).  The added cases therefore take that path with one row."""
    element_path_bwd = n % 8 != 0 or n > (4096 if dtype == torch.float32 else 8192)
    added = dtype == torch.float32 or n == 8200
    for rows in ((1,) if element_path_bwd and added else (1, 5)):
        _fused_vs_unfused(dtype, dtype, rows, n, 0.1)


def test_dropout_add_rms_layernorm_variants():
    """fp16; fp32 weights beside 16-bit activations; p = 0 and 0.5; only one of the two outputs used downstream; enough rows for
    more than one workgroup of each kernel (forward: 4 rows per workgroup, backward: 16)"""
    _fused_vs_unfused(torch.float16, torch.float16, 5, 768, 0.1)
    _fused_vs_unfused(torch.bfloat16, torch.float32, 5, 768, 0.5)
    _fused_vs_unfused(torch.bfloat16, torch.bfloat16, 5, 1032, 0.0)
    _fused_vs_unfused(torch.bfloat16, torch.bfloat16, 5, 768, 0.1, use_h=False)
    _fused_vs_unfused(torch.bfloat16, torch.bfloat16, 5, 768, 0.1, use_y=False)
    _fused_vs_unfused(torch.bfloat16, torch.bfloat16, 37, 768, 0.1)


def test_captured_graph_draws_a_new_mask_per_replay():
    from flasht5_amd import dropout
    x = _rand((5, 768), torch.bfloat16, 0)
    step = _step(41)
    dropout(x, 0.1, SEED, step, 3)   # (warm-up: the first call loads the code object)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = dropout(x, 0.1, SEED, step, 3)
    seen = []
    for k in range(2):
        g.replay()
        seen.append(y.clone())
        step.add_(1)
    torch.cuda.synchronize()
    for k, got in enumerate(seen):
        keep = torch.from_numpy(R.keep_mask(5, 768, 0.1, SEED, 41 + k, 3)).to(_dev())
        assert same(got, R.apply_mask(x, keep, 0.1)), k
    assert not same(seen[0], seen[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


def _model(p, seed=1234, **flags):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    cfg = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=4, num_layers=2, num_decoder_layers=2,
                     dropout_rate=p, dropout_seed=seed, **flags)
    torch.manual_seed(0)
    return FAT5ForConditionalGeneration(cfg).cuda().bfloat16()


def _batch():
    g = torch.Generator().manual_seed(3)
    return torch.randint(1, 128, (2, 16), generator=g).cuda(), torch.randint(1, 128, (2, 16), generator=g).cuda()


def _loss_and_grads(m, step=None, **kw):
    ids, labels = _batch()
    if step is not None:
        m.dropout_step.fill_(step)
    m.zero_grad(set_to_none=True)
    loss = m(ids, labels, **kw)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}


def _assert_same_run(a, b, what):
    (la, ga), (lb, gb) = a, b
    assert same(la, lb), (what, la.item(), lb.item())
    assert ga.keys() == gb.keys()
    for n in ga:
        assert same(ga[n], gb[n]), (what, n, (ga[n].float() - gb[n].float()).abs().max().item())


def test_model_eval_equals_a_model_without_dropout(deterministic):
    m0, m1 = _model(0.0), _model(0.1)
    m1.load_state_dict(m0.state_dict(), strict=True)
    ids, labels = _batch()
    m0.eval(), m1.eval()
    with torch.no_grad():
        assert same(m0(ids, labels), m1(ids, labels))
    assert m1.dropout_step.item() == 0          # eval draws nothing and advances nothing
    m0.train(), m1.train()
    assert not same(m0(ids, labels).detach(), m1(ids, labels).detach())
    assert m1.dropout_step.item() == 1 and m1.dropout_step.device.type == "cuda"


def test_model_plain_and_fuse_add_norm_agree(deterministic):
    m0, m1 = _model(0.1), _model(0.1, fuse_add_norm=True)
    m1.load_state_dict(m0.state_dict(), strict=True)
    _assert_same_run(_loss_and_grads(m0, step=5), _loss_and_grads(m1, step=5), "plain vs fuse_add_norm")


@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "fuse_add_norm"])
def test_model_masks_follow_the_step_counter(deterministic, fuse):
    m = _model(0.1, fuse_add_norm=fuse)
    a = _loss_and_grads(m, step=9)
    assert m.dropout_step.item() == 10          # advanced on the device by the forward
    b = _loss_and_grads(m)                      # step 10: other masks
    c = _loss_and_grads(m, step=9)
    _assert_same_run(a, c, "the same step twice")
    assert not same(a[0], b[0])


def _patch_with_restatements(monkeypatch):
    """the three operators replaced by torch restatements on uploaded tests/dropout_ref.py masks; returns the list of (site, shape)
    they were called with"""
    import importlib
    from flasht5_amd import fused_add_rms_layernorm
    D = importlib.import_module("flasht5_amd.dropout")   # (the package attribute of that name is the operator)
    calls = []

    def dropout(x, p, seed, step, site, elem_offset=0):
        calls.append((site, tuple(x.shape)))
        return R.dropout_restated(x, p, seed, step, site, elem_offset)

    def dropout_add(x, residual, p, seed, step, site):
        calls.append((site, tuple(x.shape)))
        return R.dropout_add_restated(x, residual, p, seed, step, site)

    def dropout_add_rms_layernorm(h, delta, W, eps, p, seed, step, site):
        calls.append((site, tuple(delta.shape)))
        return fused_add_rms_layernorm(h, R.dropout_restated(delta, p, seed, step, site), W, eps)

    monkeypatch.setattr(D, "dropout", dropout)
    monkeypatch.setattr(D, "dropout_add", dropout_add)
    monkeypatch.setattr(D, "dropout_add_rms_layernorm", dropout_add_rms_layernorm)
    return calls


@pytest.mark.parametrize("padded", [False, True], ids=["full", "padded"])
@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "fuse_add_norm"])
def test_model_sites_equal_the_restatement(deterministic, monkeypatch, fuse, padded):
    """loss and every gradient with the HIP operators equal those with the operators restated in torch on host masks: pins the
    masks of all six kinds of sites, their numbers (0 .. 17, forward order) and, on a padded batch, that e counts packed rows"""
    m = _model(0.1, fuse_add_norm=fuse)
    kw = {}
    if padded:
        am = torch.ones(2, 16, dtype=torch.bool)
        am[1, 11:] = False
        dm = torch.ones(2, 16, dtype=torch.bool)
        dm[0, 13:] = False
        kw = dict(attention_mask=am.cuda(), decoder_attention_mask=dm.cuda())
    kernels = _loss_and_grads(m, step=21, **kw)
    with monkeypatch.context() as mp:
        calls = _patch_with_restatements(mp)
        restated = _loss_and_grads(m, step=21, **kw)
    assert [s for s, _ in calls] == list(range(18))
    if padded:
        assert calls[0][1] == (1, 16 + 11, 64) and calls[8][1] == (1, 13 + 16, 64)   # the packed rows of both stacks
    _assert_same_run(kernels, restated, "kernels vs restatement")
    assert m.dropout_seed == 1234 and torch.isfinite(kernels[0]).item()
