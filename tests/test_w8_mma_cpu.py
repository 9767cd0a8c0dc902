"""The matrix-pipe FP8-weight linear without a device: its export, its checks (those of fat5_w8_linear, with its messages, before
any launch) and the host checks of `kernel=` and `weight_kernel=`."""
import ctypes

import pytest
import torch

from test_w8_cpu import _linear_params, _no_encoder, _small_model


@pytest.mark.parametrize("kw", [dict(K=96), dict(N=12), dict(dtype=0), dict(x_stride=132), dict(y=None), dict(w8=4097),
                                dict(residual=4096, residual_stride=8), dict(norm_weight=4096, eps=float("nan")), dict(reserved=1)])
def test_einval_with_the_row_kernels_message_and_no_device(kw):
    from flasht5_amd import _lib
    lib = _lib.load()
    assert lib.fat5_w8_linear(ctypes.byref(_linear_params(**kw)), None) == -1
    want = lib.fat5_last_error().decode()
    assert lib.fat5_w8_linear_mma(ctypes.byref(_linear_params(**kw)), None) == -1   # FAT5_EINVAL
    assert lib.fat5_last_error().decode() == want and want.startswith("w8_linear: ")


def test_exported_and_no_rows_is_ok_without_a_device():
    from flasht5_amd import _lib
    lib = _lib.load()
    assert "fat5_w8_linear_mma" in _lib.EXPORTS
    assert lib.fat5_w8_linear_mma(ctypes.byref(_linear_params(R=0, x=None, y=None)), None) == 0
    assert lib.fat5_w8_linear_mma(None, None) == -1
    assert lib.fat5_w8_linear_mma(ctypes.byref(_linear_params(R=-1)), None) == -1
    assert "R -1 (0 .. 4194240 rows)" in lib.fat5_last_error().decode()   # (its own limit: 65535 row tiles of 64)


def test_kernel_names_are_checked_on_the_host(monkeypatch):
    from flasht5_amd import w8, w8_linear
    w, s = torch.empty(16, 128, dtype=torch.float8_e4m3fn), torch.empty(16)
    with pytest.raises(ValueError, match="kernel 'x'"):
        w8_linear(torch.zeros(2, 128, dtype=torch.bfloat16), w, s, kernel="x")
    with pytest.raises(ValueError, match="no CPU path"):
        w8_linear(torch.zeros(2, 128, dtype=torch.bfloat16), w, s, kernel="matrix")
    assert [w8.kernel_for_rows("matrix", r) for r in (8, 9)] == ["rows", "matrix"] and w8.kernel_for_rows("rows", 64) == "rows"
    m = _small_model().bfloat16()
    _no_encoder(monkeypatch, m)
    ids = torch.zeros(2, 4, dtype=torch.long)
    for kw in (dict(weight_kernel="matrix"), dict(weight_kernel="rows"), dict(weight_dtype="fp8", weight_kernel="mfma"),
               dict(weight_dtype="fp8", weight_kernel=1)):
        with pytest.raises(ValueError, match="weight_kernel"):
            m.generate(ids, max_length=4, **kw)
        with pytest.raises(ValueError, match="weight_kernel"):
            m.init_decode_state(ids, max_length=4, **kw)
