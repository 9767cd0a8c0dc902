"""MXFP8 activations and the W4A8 linear without a device: the ABI
(exports, struct sizes, FAT5_EINVAL before any launch), the Python checks, and the models' host checks before an encoder runs."""
import ctypes

import pytest
import torch

from test_w8_cpu import _no_encoder, _small_model


def _params(entry, **kw):
    """legal parameters with pointers that are never followed: every check comes before the launch"""
    from flasht5_amd import _lib
    if entry == "w4a8_linear":
        p = _lib.W4A8LinearParams()
        p.R, p.N, p.K, p.dtype, p.a8, p.ax, p.w4, p.e8, p.y = 4, 16, 128, _lib.FAT5_BF16, 4096, 4096, 4096, 4096, 4096
        p.a_stride, p.ax_stride, p.w_stride, p.e_stride, p.y_stride = 128, 4, 64, 4, 16
    else:
        p = _lib.Mx8QuantParams()
        p.R, p.K, p.dtype, p.x, p.a8, p.ax, p.x_stride, p.a_stride, p.ax_stride = 4, 64, _lib.FAT5_F16, 4096, 4096, 4096, 64, 64, 2
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_exports_struct_sizes_and_nothing_to_do():
    from flasht5_amd import _lib
    lib = _lib.load()
    for name in ("fat5_mx8_quantize", "fat5_sizeof_mx8_quant_params", "fat5_w4a8_linear", "fat5_sizeof_w4a8_linear_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_mx8_quant_params() == ctypes.sizeof(_lib.Mx8QuantParams)
    assert lib.fat5_sizeof_w4a8_linear_params() == ctypes.sizeof(_lib.W4A8LinearParams)
    assert lib.fat5_w4a8_linear(_params("w4a8_linear", R=0, a8=None, ax=None, y=None), None) == 0
    assert lib.fat5_w4a8_linear(_params("w4a8_linear", N=0, w4=None, e8=None, y=None), None) == 0
    assert lib.fat5_mx8_quantize(_params("mx8_quantize", R=0, x=None, a8=None, ax=None), None) == 0
    assert lib.fat5_w4a8_linear(None, None) == -1 and lib.fat5_mx8_quantize(None, None) == -1


@pytest.mark.parametrize("entry, kw, msg", [("w4a8_linear", kw, msg) for kw, msg in [
    (dict(K=48), "K 48"), (dict(K=16416), "K 16416"), (dict(N=12), "N 12"), (dict(R=-1), "R -1"), (dict(dtype=0), "dtype 0"),
    (dict(a_stride=120), "a_stride"), (dict(ax_stride=3), "ax_stride"), (dict(w_stride=72), "w_stride"), (dict(e_stride=3), "e_stride"),
    (dict(y_stride=8), "y_stride"), (dict(a8=4104), "a8: null or misaligned"), (dict(ax=None), "ax"), (dict(y=None), "y: null or misaligned"),
    (dict(residual=4096, residual_stride=8), "residual_stride"),
]] + [("mx8_quantize", kw, msg) for kw, msg in [
    (dict(K=16), "K 16"), (dict(dtype=0), "dtype 0"), (dict(x_stride=32), "x_stride"), (dict(a_stride=72), "a_stride"),
    (dict(ax_stride=1), "ax_stride"), (dict(x=8), "x: null or misaligned"), (dict(norm_weight=4096, eps=-1.0), "eps"), (dict(reserved=1), "reserved"),
]])
def test_einval_without_a_device(entry, kw, msg):
    from flasht5_amd import _lib
    lib = _lib.load()
    assert getattr(lib, "fat5_" + entry)(_params(entry, **kw), None) == -1, msg   # FAT5_EINVAL
    assert msg in lib.fat5_last_error().decode()


def test_python_checks_come_before_the_device():
    from flasht5_amd import quantize_activation_mxfp8, w4a8_linear, w4a8_matmul
    w4, e8 = torch.zeros(16, 64, dtype=torch.uint8), torch.zeros(16, 4, dtype=torch.uint8)
    x = torch.zeros(2, 3, 128, dtype=torch.bfloat16)
    a8, ax = torch.zeros(6, 128, dtype=torch.uint8), torch.zeros(6, 4, dtype=torch.uint8)
    for call in (lambda: w4a8_linear(x, w4, e8), lambda: quantize_activation_mxfp8(x), lambda: w4a8_matmul(a8, ax, w4, e8, torch.bfloat16)):
        with pytest.raises(ValueError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_activation_mxfp8(x[..., :48])
    with pytest.raises(ValueError, match="fp16 or bf16"):
        quantize_activation_mxfp8(x.float())
    with pytest.raises(ValueError, match="fp16 or bf16"):
        w4a8_matmul(a8, ax, w4, e8, torch.float32)
    with pytest.raises(ValueError, match="e8 must be"):
        w4a8_linear(x, w4, e8[:, :3])
    with pytest.raises(ValueError, match="columns"):
        w4a8_matmul(a8[:, :64], ax[:, :2], w4, e8, torch.bfloat16)
    with pytest.raises(ValueError, match="residual must be"):
        w4a8_matmul(a8, ax, w4, e8, torch.bfloat16, residual=torch.zeros(6, 8, dtype=torch.bfloat16))


def test_models_check_on_the_host_before_the_encoder(monkeypatch):
    import flasht5_amd as F
    from flasht5_amd.w4a8 import encoder_forward_mxfp4
    import flasht5_amd.w4a8 as w4a8
    m = _small_model().bfloat16()
    _no_encoder(monkeypatch, m)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="inference only"):   # (before the stand-in below replaces it)
        encoder_forward_mxfp4(F.FAT5EncoderModel(m.config).train().encoder, None, ids)

    def boom(*a, **k):
        raise AssertionError("the MXFP4 encoder ran before the arguments were checked")
    monkeypatch.setattr(w4a8, "encoder_forward_mxfp4", boom)   # (the path under test goes through this, not encoder.forward)
    with pytest.raises(ValueError, match="quantize_encoder_weights_mxfp4"):
        m.generate(ids, max_length=4, encoder_weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="quantize_encoder_weights_mxfp4"):
        m.init_decode_state(ids, max_length=4, encoder_weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="None or 'mxfp4'"):
        m.generate(ids, max_length=4, encoder_weight_dtype="fp8")
    with pytest.raises(ValueError, match="fp16 or bf16"):
        _small_model().quantize_encoder_weights_mxfp4()
    enc = F.FAT5EncoderModel(m.config).bfloat16()
    with pytest.raises(ValueError, match="quantize_encoder_weights_mxfp4"):
        enc(ids, weight_dtype="mxfp4")
