"""CPU tests of dropout: the numpy Philox of tests/dropout_ref.py against the scalar one of tests/sampling_ref.py, the statistics and
the site / step separation of the reference mask, the ctypes mirror and the exports, the C ABI's rejections (before any launch:
fake, aligned pointers are enough), the configuration rule and the rank-to-key helper."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dropout_ref as R
from sampling_ref import philox4x32_10

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_numpy_philox_matches_the_scalar_reference():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, size=(64, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(64, 2), dtype=np.uint64)
    ctr[0], ctr[1] = 0, 0xFFFFFFFF          # (the all-zero and all-one counters among them)
    key[0], key[1] = 0, 0xFFFFFFFF
    for c, k in zip(ctr, key):
        got = R.philox4x32_10_np(tuple(np.full((3,), int(v), dtype=np.uint64) for v in c), (int(k[0]), int(k[1])))
        want = philox4x32_10([int(v) for v in c], [int(v) for v in k])
        for g, w in zip(got, want):
            assert g.dtype == np.uint32 and (g == w).all(), (c, k)
    # vectorised over the counter in one call
    got = R.philox4x32_10_np(tuple(ctr[:, i] for i in range(4)), (7, 9))
    for r in range(64):
        assert tuple(int(g[r]) for g in got) == philox4x32_10([int(v) for v in ctr[r]], (7, 9))


def test_mask_follows_the_contract_element_by_element():
    """keep_mask against the contract written out with the scalar Philox, across a 64-bit block index"""
    p, seed, step, site, off = 0.3, 0x0123456789ABCDEF, (1 << 32) + 5, 11, (1 << 32) - 3
    k = R.keep_mask(2, 8, p, seed, step, site, off)
    for i in range(2):
        for c in range(8):
            e = off + i * 8 + c
            w = philox4x32_10(((e >> 2) & R.MASK, (e >> 2) >> 32, site, step & R.MASK), (seed & R.MASK, seed >> 32))[e & 3]
            assert bool(k[i, c]) == (np.float32((w >> 8) * 2.0 ** -24) >= np.float32(p))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    """N = 2^16 elements: the kept share within 5 sigma of 1 - p (the mask is deterministic: these inputs pass)"""
    N = 1 << 16
    k = R.keep_mask(N // 256, 256, p, seed=1234, step=0, site=0)
    assert abs(k.mean() - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / N)
    assert R.keep_mask(4, 64, 0.0, seed=1234, step=0, site=0).all()


def test_sites_and_steps_draw_different_masks():
    a = R.keep_mask(8, 64, 0.5, seed=5, step=0, site=0)
    assert (a == R.keep_mask(8, 64, 0.5, seed=5, step=0, site=0)).all()
    for other in (dict(step=0, site=1), dict(step=1, site=0), dict(step=1 << 32, site=1)):
        b = R.keep_mask(8, 64, 0.5, seed=5, **other)
        assert 0.3 < (a != b).mean() < 0.7, other
    assert (a == R.keep_mask(8, 64, 0.5, seed=5, step=1 << 32, site=0)).all()   # step enters mod 2^32
    # elem_offset shifts the stream: rows 1.. of one operand are rows 0.. of the operand that starts one row later
    assert (R.keep_mask(8, 64, 0.5, 5, 0, 0)[1:] == R.keep_mask(7, 64, 0.5, 5, 0, 0, elem_offset=64)).all()


def test_scale_is_one_fp32_division():
    assert R.scale(0.0) == np.float32(1.0) and R.scale(0.5) == np.float32(2.0)
    assert R.scale(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)) and R.scale(0.1).dtype == np.float32


def test_exports_and_struct_size(lib):
    from flasht5_amd import _lib
    for name in ("fat5_dropout", "fat5_dropout_add_rmsnorm_fwd", "fat5_dropout_add_rmsnorm_bwd", "fat5_sizeof_dropout_desc"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_dropout_desc() == ctypes.sizeof(_lib.DropoutDesc) == 32
    assert lib.fat5_version() == 114


def _desc(p=0.1, step=BASE):
    from flasht5_amd import _lib
    d = _lib.DropoutDesc()
    d.seed, d.step, d.elem_offset, d.site, d.p = 1, step, 0, 0, p
    return d


def _calls(lib, d, dtype):
    """the three entry points with fake, aligned pointers and a valid shape"""
    dp = ctypes.byref(d) if d is not None else None
    return [
        ("dropout", lambda: lib.fat5_dropout(BASE, None, BASE, 4, 64, 64, 0, 64, dp, dtype, None)),
        ("dropout_add_rmsnorm_fwd", lambda: lib.fat5_dropout_add_rmsnorm_fwd(BASE, BASE, BASE, BASE, BASE, BASE, 4, 64, 64, 64, 64, 64,
                                                                              1e-6, dp, dtype, dtype, None)),
        ("dropout_add_rmsnorm_bwd", lambda: lib.fat5_dropout_add_rmsnorm_bwd(BASE, BASE, BASE, BASE, None, BASE, BASE, BASE, 4, 64, 64, 64,
                                                                              0, 64, 64, dp, dtype, dtype, BASE, 1 << 30, None)),
    ]


def test_bad_calls_are_rejected_before_any_launch(lib):
    from flasht5_amd import _lib
    bf = _lib.FAT5_BF16
    for what, d, dtype, word in (("p < 0", _desc(p=-0.1), bf, b"outside [0, 1)"), ("p = 1", _desc(p=1.0), bf, b"outside [0, 1)"),
                                 ("p > 1", _desc(p=1.5), bf, b"outside [0, 1)"), ("p NaN", _desc(p=float("nan")), bf, b"outside [0, 1)"),
                                 ("null step", _desc(step=None), bf, b"step"), ("misaligned step", _desc(step=BASE + 4), bf, b"step"),
                                 ("bad dtype", _desc(), 7, b"bad dtype"), ("null descriptor", None, bf, b"null descriptor")):
        for name, call in _calls(lib, d, dtype):
            assert call() == -1, (what, name)
            msg = lib.fat5_last_error()
            assert word in msg and name.encode() in msg, (what, name, msg)
    d = _desc()
    assert lib.fat5_dropout(None, None, BASE, 4, 64, 64, 0, 64, ctypes.byref(d), bf, None) == -1 and b"null" in lib.fat5_last_error()
    assert lib.fat5_dropout(BASE, None, BASE, 0, 64, 64, 0, 64, ctypes.byref(d), bf, None) == -1 and b"shape" in lib.fat5_last_error()
    assert lib.fat5_dropout(BASE, None, BASE, 1 << 31, 64, 64, 0, 64, ctypes.byref(d), bf, None) == -1 and b"too large" in lib.fat5_last_error()
    assert lib.fat5_dropout_add_rmsnorm_bwd(BASE, BASE, BASE, BASE, None, BASE, BASE, BASE, 4, 64, 64, 64, 0, 64, 64, ctypes.byref(d), bf, bf,
                                            BASE, 8, None) == -3   # FAT5_EWORKSPACE, the parent's workspace function
    assert lib.fat5_rmsnorm_bwd_workspace_bytes(4, 64) > 8


def test_python_operators_check_on_the_host():
    from flasht5_amd import dropout, dropout_add, dropout_add_rms_layernorm
    x = torch.zeros(4, 64)
    step = torch.zeros(1, dtype=torch.int64)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="outside"):
            dropout(x, p, 0, step, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dropout(x, 0.1, 0, step, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dropout_add(x, x, 0.1, 0, step, 0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        dropout_add_rms_layernorm(x, x, torch.ones(64), 1e-6, 0.1, 0, step, 0)
    with pytest.raises(ValueError, match="site"):
        dropout(x, 0.1, 0, step, -1)


def test_fake_implementations():
    """shape / dtype propagation of the custom ops on the meta device (what torch.compile traces)"""
    x = torch.empty(3, 5, 64, dtype=torch.bfloat16, device="meta")
    step = torch.empty(1, dtype=torch.int64, device="meta")
    y = torch.ops.fat5.dropout_fwd(x, None, 0.1, 1, step, 0, 0)
    assert y.shape == x.shape and y.dtype == x.dtype
    x2, w = x.reshape(15, 64), torch.empty(64, dtype=torch.float32, device="meta")
    h, n, rstd = torch.ops.fat5.dropout_add_rmsnorm_fwd(x2, x2, w, 1e-6, 0.1, 1, step, 0)
    assert h.shape == n.shape == x2.shape and rstd.shape == (15,) and rstd.dtype == torch.float32
    dx, dd, dw = torch.ops.fat5.dropout_add_rmsnorm_bwd(x2, x2, w, rstd, x2, True, 0.1, 1, step, 0)
    assert dx.shape == dd.shape == x2.shape and dw.shape == w.shape and dw.dtype == w.dtype


def test_config_rules():
    from flasht5_amd import FAT5Config
    assert FAT5Config().dropout_rate == 0.0 and FAT5Config().dropout_seed is None
    with pytest.raises(ValueError, match="fuse_norm_linear"):
        FAT5Config(dropout_rate=0.1, fuse_norm_linear=True)
    FAT5Config(dropout_rate=0.0, fuse_norm_linear=True)
    FAT5Config(dropout_rate=0.1, fuse_add_norm=True)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="dropout_rate"):
            FAT5Config(dropout_rate=bad)


def test_model_sites_seed_and_state_dict():
    """the site numbers are distinct, in forward order and the same for both paths; the seed is drawn once; the step counter stays out
    of the state dict; a dropout_rate of 0 builds none of it and leaves torch's generator where it was"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(vocab_size=128, d_model=64, d_kv=16, d_ff=128, num_heads=4, num_layers=2, num_decoder_layers=2)
    torch.manual_seed(0)
    m0 = FAT5ForConditionalGeneration(FAT5Config(**kw))
    after0 = torch.get_rng_state()
    torch.manual_seed(0)
    m = FAT5ForConditionalGeneration(FAT5Config(dropout_rate=0.1, **kw))
    assert not hasattr(m0, "dropout_step") and m0.dropout_seed is None
    assert all(torch.equal(a, b) for a, b in zip(m0.state_dict().values(), m.state_dict().values()))   # same draws for the weights
    assert not torch.equal(after0, torch.get_rng_state())   # (the seed came from the default generator, after the weights)
    assert isinstance(m.dropout_seed, int) and 0 <= m.dropout_seed < 2 ** 62
    assert m.dropout_step.dtype == torch.int64 and m.dropout_step.numel() == 1 and "dropout_step" not in m.state_dict()
    m.load_state_dict(m0.state_dict(), strict=True)
    assert FAT5ForConditionalGeneration(FAT5Config(dropout_rate=0.1, dropout_seed=77, **kw)).dropout_seed == 77

    def sites(model):
        out = []
        for st in (model.encoder, model.decoder):
            out.append(st.site_embed)
            for blk in st.block:
                out.append(blk.self_attention_layer.site)
                if blk.is_decoder:
                    out.append(blk.cross_attention_layer.site)
                out += [blk.ff_layer.site_act, blk.ff_layer.site]
            out.append(st.site_final)
        return out

    assert sites(m) == list(range(2 + 2 * 3 + 2 + 2 * 4))   # 18 sites: encoder 1 + 2 * 3 + 1, decoder 1 + 2 * 4 + 1
    assert sites(FAT5ForConditionalGeneration(FAT5Config(dropout_rate=0.1, fuse_add_norm=True, **kw))) == sites(m)


def test_rank_key():
    from flasht5_amd.dropout import rank_key
    assert rank_key(5, 0) == 5 and rank_key(5, 3) == 8
    assert rank_key((1 << 64) - 1, 1) == 0 and rank_key((1 << 64) - 2, 5) == 3    # mod 2^64
    assert len({rank_key(123, r) for r in range(8)}) == 8
