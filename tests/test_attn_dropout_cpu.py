"""Host-side tests of attention dropout: the exports, every rejection of the C ABI (before a launch: no device is
needed) and the errors of the operators and of the model's configuration."""
import ctypes

import pytest
import torch

from flasht5_amd import _lib

NAMES = ("fat5_sizeof_attn_dropout_params", "fat5_attn_dropout_fwd", "fat5_attn_dropout_bwd_workspace_bytes", "fat5_attn_dropout_bwd")


def _params(**kw):
    p = _lib.AttnDropoutParams()
    p.B, p.H, p.M, p.N, p.D, p.dtype, p.p, p.sm_scale = 2, 3, 64, 64, 64, _lib.dtype_code(torch.bfloat16), 0.1, 0.125
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_exports():
    lib = _lib.load()
    assert all(n in _lib.EXPORTS and hasattr(lib, n) for n in NAMES)
    assert lib.fat5_sizeof_attn_dropout_params() == ctypes.sizeof(_lib.AttnDropoutParams)
    assert lib.fat5_attn_dropout_bwd_workspace_bytes(ctypes.byref(_params())) == 2 * 3 * 64 * 4
    assert lib.fat5_attn_dropout_bwd_workspace_bytes(ctypes.byref(_params(bias_mode=_lib.BIAS_RPE1D, rpe_radius=8))) == 1536 + 6 * 17 * 4


@pytest.mark.parametrize("kw,msg", [
    (dict(p=1.0), "outside [0, 1)"), (dict(p=-0.1), "outside [0, 1)"), (dict(p=float("nan")), "outside [0, 1)"),
    (dict(D=128), "head_dim 128"), (dict(bias_mode=_lib.BIAS_DENSE), "dense bias is not supported"),
    (dict(B=1025, H=1024), "below 2^20"), (dict(site=1 << 12), "below 2^12"),
    (dict(bias_mode=_lib.BIAS_RPE1D, rpe_radius=0), "rpe_radius"), (dict(cu_seqlens_q=64), "both cu_seqlens_q and cu_seqlens_k"),
    (dict(), "q/k/v/o must be non-null"), (dict(dtype=_lib.dtype_code(torch.float32)), "dtype"),
], ids=lambda x: x if isinstance(x, str) else None)
def test_rejections(kw, msg):
    lib = _lib.load()
    assert lib.fat5_attn_dropout_fwd(ctypes.byref(_params(**kw)), None) == -1
    assert msg in lib.fat5_last_error().decode()
    assert lib.fat5_attn_dropout_bwd(ctypes.byref(_params(**kw)), None) == -1
    assert lib.fat5_attn_dropout_fwd(None, None) == -1 and "NULL" in lib.fat5_last_error().decode()


def test_null_step_and_lse_are_rejected():
    lib, buf = _lib.load(), (ctypes.c_char * 64)()
    ptr = (ctypes.addressof(buf) + 15) & ~15
    kw = dict(q=ptr, k=ptr, v=ptr, o=ptr, q_stride=_lib.c_i64x3(8, 8, 8), k_stride=_lib.c_i64x3(8, 8, 8), v_stride=_lib.c_i64x3(8, 8, 8),
              o_stride=_lib.c_i64x3(8, 8, 8))
    assert lib.fat5_attn_dropout_fwd(ctypes.byref(_params(**kw)), None) == -1 and "null lse" in lib.fat5_last_error().decode()
    assert lib.fat5_attn_dropout_fwd(ctypes.byref(_params(lse=ptr, **kw)), None) == -1 and "step" in lib.fat5_last_error().decode()


def test_operator_and_model_errors():
    from flasht5_amd import FAT5Config, flash_attention_v2_rpe1d, flash_attn_varlen_func
    from flasht5_amd.attention_module import FlashT5Attention
    q = torch.zeros(1, 1, 8, 64)
    with pytest.raises(NotImplementedError, match="window"):
        flash_attention_v2_rpe1d(q, q, q, None, 0, window=4, dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="global_kv"):
        flash_attn_varlen_func(q[0], q[0], q[0], None, None, 8, 8, global_kv=(q, q), dropout_p=0.1)
    with pytest.raises(ValueError, match="outside"):
        flash_attention_v2_rpe1d(q, q, q, None, 0, dropout_p=1.0)
    kw = dict(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=4, num_layers=1, num_decoder_layers=1)
    for bad in (dict(attention_type="triton"), dict(attention_type="triton", position_encoding_type="FIRE"),
                dict(attention_type="fat5_rpe", encoder_attention_type="local"), dict(attention_type="fat5_rpe", d_kv=32)):
        with pytest.raises(ValueError, match="attention_dropout_rate"):
            FAT5Config(attention_dropout_rate=0.1, **{**kw, **bad})
    with pytest.raises(ValueError, match="outside"):
        FAT5Config(attention_dropout_rate=1.0, attention_type="fat5_rpe", **kw)
    cfg = FAT5Config(attention_type="fat5_rpe", **kw)
    cfg.attention_dropout_rate, cfg.attention_type = 0.1, "triton"
    with pytest.raises(ValueError, match="attention dropout needs"):
        FlashT5Attention(cfg)
    cfg.attention_type = "fat5_rpe"
    layer = FlashT5Attention(cfg, has_positional_encoding=True)
    with pytest.raises(RuntimeError, match="attn_drop"):
        layer(torch.zeros(1, 8, 64))
