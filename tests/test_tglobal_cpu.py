"""Transient-global attention without a GPU: the C ABI's exports and descriptor, host rejections, config validation."""
import ctypes

import pytest
import torch


def test_exports_and_descriptor():
    from flasht5_amd import _lib
    lib = _lib.load()
    names = ("fat5_attn_tglobal_fwd", "fat5_attn_tglobal_bwd", "fat5_attn_tglobal_bwd_workspace_bytes", "fat5_sizeof_tglobal_attn_params")
    assert all(n in _lib.EXPORTS and hasattr(lib, n) for n in names)
    assert lib.fat5_sizeof_tglobal_attn_params() == ctypes.sizeof(_lib.TGlobalAttnParams)


def test_the_library_rejects_before_any_launch():
    from flasht5_amd import _lib
    lib = _lib.load()
    # (-1: FAT5_EINVAL)
    ok = dict(B=1, H=2, S=64, D=64, dtype=_lib.dtype_code(torch.bfloat16), window=8, bias_mode=_lib.BIAS_RPE1D, rpe_radius=8, g_radius=8)
    for bad in (dict(D=128), dict(window=0), dict(g_radius=0), dict(g_radius=1025), dict(dtype=_lib.dtype_code(torch.float32)), dict(S=0)):
        p = _lib.TGlobalAttnParams(**{**ok, **bad})
        assert lib.fat5_attn_tglobal_fwd(ctypes.byref(p), None) == -1, bad
        assert lib.fat5_attn_tglobal_bwd(ctypes.byref(p), None) == -1, bad
        assert lib.fat5_attn_tglobal_bwd_workspace_bytes(ctypes.byref(p)) == 0, bad
    p = _lib.TGlobalAttnParams(**ok)   # an accepted shape without tensors: its workspace is answered, its launch refused
    assert lib.fat5_attn_tglobal_bwd_workspace_bytes(ctypes.byref(p)) > 0
    assert lib.fat5_attn_tglobal_fwd(ctypes.byref(p), None) == -1


def test_the_operators_reject_before_any_launch():
    from flasht5_amd import flash_attention_v2_rpe1d, flash_attn_varlen_func
    t = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    q, gk, r1, g1 = t(1, 2, 32, 64), t(1, 2, 2, 64), torch.zeros(2, 17), torch.zeros(2, 9)
    for kw in (dict(global_kv=(gk, gk), global_rpe1d=g1, global_radius=4),                      # no window
               dict(window=4, global_rpe1d=g1, global_radius=4),                                  # tables without global keys
               dict(window=4, global_kv=(gk, t(1, 2, 3, 64)), global_rpe1d=g1, global_radius=4),  # gk / gv disagree
               dict(window=4, global_kv=(gk, gk)),                                                # one table of the two
               dict(window=4, global_kv=(gk, gk), global_rpe1d=g1, global_radius=5)):             # table of another radius
        with pytest.raises(ValueError):
            flash_attention_v2_rpe1d(q, q, q, r1, 8, False, None, **kw)
    pq, cu = t(32, 2, 64), torch.tensor([0, 32], dtype=torch.int32)
    with pytest.raises(ValueError):   # packed global keys without their offsets
        flash_attn_varlen_func(pq, pq, pq, cu, cu, 32, 32, window=4, global_kv=(t(2, 2, 64), t(2, 2, 64)))


def test_config_validation():
    from flasht5_amd import FAT5Config
    assert FAT5Config(encoder_attention_type="transient-global").local_radius == 127
    for bad in (dict(attention_type="triton"), dict(d_kv=128), dict(position_encoding_type="RoPE"), dict(local_radius=0)):
        with pytest.raises(ValueError):
            FAT5Config(encoder_attention_type="transient-global", **bad)
