"""Host side of local attention: exports, the descriptor mirror, rejections before any launch, and the config's validation."""
import ctypes

import pytest

FAT5_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_local_exports_and_descriptor_size(lib):
    from flasht5_amd import _lib
    for name in ("fat5_attn_local_fwd", "fat5_attn_local_bwd", "fat5_attn_local_bwd_workspace_bytes", "fat5_sizeof_local_attn_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.fat5_sizeof_local_attn_params() == ctypes.sizeof(_lib.LocalAttnParams)


@pytest.mark.parametrize("change", [None, {"D": 128}, {"D": 32}, {"window": 0}, {"window": -3}])
def test_local_rejected_before_any_launch(lib, change):
    """no pointer is set: an accepted shape would fail at the pointer check, these fail earlier with their own message"""
    from flasht5_amd import _lib
    p = _lib.LocalAttnParams()
    p.B, p.H, p.S, p.D, p.dtype, p.window, p.sm_scale = 1, 2, 128, 64, _lib.FAT5_BF16, 127, 0.125
    for key, val in (change or {}).items():
        setattr(p, key, val)
    arg = None if change is None else ctypes.byref(p)
    for fn in (lib.fat5_attn_local_fwd, lib.fat5_attn_local_bwd):
        assert fn(arg, None) == FAT5_EINVAL
        msg = lib.fat5_last_error().decode()
        assert ("NULL" if change is None else ("head_dim" if "D" in change else "window")) in msg, msg
    assert lib.fat5_attn_local_bwd_workspace_bytes(arg) == 0


@pytest.mark.parametrize("kwargs", [{"attention_type": "triton"}, {"attention_type": "triton", "position_encoding_type": "FIRE"},
                                    {"d_kv": 128}, {"local_radius": 0}])
def test_config_rejects_local_without_its_kernels(kwargs):
    from flasht5_amd.fat5_step import FAT5Config
    with pytest.raises(ValueError):
        FAT5Config(encoder_attention_type="local", **kwargs)
    FAT5Config(**{k: v for k, v in kwargs.items() if k != "local_radius"})  # the same model with full attention is accepted
    assert FAT5Config(encoder_attention_type="local").local_radius == 127
