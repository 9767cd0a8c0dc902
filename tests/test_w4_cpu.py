"""MXFP4 weights without a device: the restated rule (tests/w4_ref.py) on hand-made blocks, the ABI (exports, struct sizes,
FAT5_EINVAL before any launch), the Python checks, and generate's `weight_dtype="mxfp4"` checks before an encoder runs."""
import ctypes

import pytest
import torch

import w4_ref as R
from test_w8_cpu import _no_encoder, _small_model

INF = float("inf")


def hand_blocks():
    """{name: (32 values, scale byte, the first codes | sign << 3)}; every value is exact in fp32 and bf16, and in fp16 but 2^17"""
    def blk(*v):
        return torch.tensor(list(v) + [0.0] * (32 - len(v)))
    return {
        # amax 6 -> X = 0; every midpoint of the grid, both signs: ties go to the even code (0, 1, 1, 2, 2, 4, 4)
        "ties": (blk(6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, -.25, -.75, -1.25, -1.75, -2.5, -3.5, -5), 127,
                 [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14]),
        # amax = 6 * 2^3 exactly: floor(log2 48) - 2 = 3, the element is 6; 28 = 3.5 * 8 is a tie -> 4
        "amax 6 * 2^X": (blk(48, -28, 4), 130, [7, 14, 1]),
        # ... and above it, still X = 3: 50 / 8 = 6.25 and 60 / 8 = 7.5 saturate at 6
        "amax above 6 * 2^X": (blk(50, -60, 12), 130, [7, 15, 3]),
        "zero": (blk(), 127, [0, 0]),
        # the sign bit of -0 and of a value that rounds to zero stays (amax 4 -> X = 0)
        "minus zero": (blk(4, -0.0, -0.125, 0.125), 127, [6, 8, 8, 0]),
        "inf": (blk(1, -2, INF, -3), 255, [0, 0, 0, 0]),
        # amax 2^-14: floor(log2) - 2 = -16, clamped to -13 -> 2^-14 * 2^13 = 0.5; 2^-15 * 2^13 = 0.25 is a tie -> 0
        "clamp below": (blk(2.0 ** -14, -2.0 ** -15, 3 * 2.0 ** -14), 114, [1, 8, 3]),
        # amax 2^17: 17 - 2 = 15, clamped to 13 -> 16 saturates at 6; 2^13 is 1
        "clamp above": (blk(2.0 ** 17, -2.0 ** 13, 3 * 2.0 ** 12), 140, [7, 10, 3]),
    }


@pytest.mark.parametrize("name", sorted(hand_blocks()))
def test_the_rule_on_hand_made_blocks(name):
    v, byte, codes = hand_blocks()[name]
    w4, e8 = R.quantize_ref(v.view(1, 32))
    nib = torch.stack([w4 & 15, w4 >> 4], -1).view(-1).tolist()
    assert e8.tolist() == [[byte]] and nib[:len(codes)] == codes and not any(nib[len(codes):])
    if byte != 255:
        got = R.dequant(w4, e8)[0]
        sat = v.double().abs().clamp(max=6 * 2.0 ** (byte - 127))
        assert float((got.abs() - sat).abs().max()) <= 2.0 ** (byte - 127)     # (a grid step is at most 2 * 2^X)
        assert torch.equal(torch.signbit(got), torch.signbit(v))
    else:
        assert bool(torch.isnan(R.dequant(w4, e8)).all())


# ----------------------------------------------------------------------------------------------------------------------- ABI
def _params(entry, **kw):
    """legal parameters of fat5_w4_<entry> with pointers that are never followed: every check comes before the launch"""
    from flasht5_amd import _lib
    if entry == "linear":
        p = _lib.W4LinearParams()
        p.R, p.N, p.K, p.dtype, p.x, p.w4, p.e8, p.y = 4, 16, 128, _lib.FAT5_BF16, 4096, 4096, 4096, 4096
        p.x_stride, p.w_stride, p.e_stride, p.y_stride = 128, 64, 4, 16
    else:
        p = _lib.W4QuantParams()
        p.N, p.K, p.dtype, p.w, p.out, p.e8, p.w_stride, p.out_stride, p.e_stride = 8, 64, _lib.FAT5_F32, 4096, 4096, 4096, 64, 32, 2
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def test_exports_struct_sizes_and_nothing_to_do():
    from flasht5_amd import _lib
    lib = _lib.load()
    for name in ("fat5_w4_quantize", "fat5_sizeof_w4_quant_params", "fat5_w4_linear", "fat5_sizeof_w4_linear_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_w4_quant_params() == ctypes.sizeof(_lib.W4QuantParams)
    assert lib.fat5_sizeof_w4_linear_params() == ctypes.sizeof(_lib.W4LinearParams)
    assert lib.fat5_w4_linear(_params("linear", R=0, x=None, y=None), None) == 0
    assert lib.fat5_w4_linear(_params("linear", N=0, w4=None, e8=None, y=None), None) == 0
    assert lib.fat5_w4_quantize(_params("quantize", N=0, w=None, out=None, e8=None), None) == 0
    assert lib.fat5_w4_linear(None, None) == -1 and lib.fat5_w4_quantize(None, None) == -1


@pytest.mark.parametrize("entry, kw, msg", [("linear", kw, msg) for kw, msg in [
    (dict(K=16), "K 16"), (dict(K=48), "K 48"), (dict(K=16416), "K 16416"), (dict(N=12), "N 12"), (dict(R=-1), "R -1"),
    (dict(dtype=0), "dtype 0"), (dict(x_stride=64), "x_stride"), (dict(x_stride=132), "x_stride"), (dict(w_stride=72), "w_stride"),
    (dict(w_stride=48), "w_stride"), (dict(e_stride=3), "e_stride"), (dict(y_stride=8), "y_stride"),
    (dict(x=4100), "x: null or misaligned"), (dict(w4=4104), "w4: null or misaligned"), (dict(e8=None), "e8"),
    (dict(y=None), "y: null or misaligned"), (dict(residual=4096, residual_stride=8), "residual_stride"),
    (dict(norm_weight=4098), "norm_weight"), (dict(norm_weight=4096, eps=INF), "eps"), (dict(reserved=1), "reserved"),
]] + [("quantize", kw, msg) for kw, msg in [
    (dict(K=16), "K 16"), (dict(N=4), "N 4"), (dict(dtype=7), "dtype 7"), (dict(w_stride=32), "w_stride"),
    (dict(out_stride=40), "out_stride"), (dict(e_stride=1), "e_stride"), (dict(w=8), "w: null or misaligned"),
    (dict(out=4104), "out: null or misaligned"), (dict(e8=None), "e8"),
]])
def test_einval_without_a_device(entry, kw, msg):
    from flasht5_amd import _lib
    lib = _lib.load()
    assert getattr(lib, "fat5_w4_" + entry)(_params(entry, **kw), None) == -1, msg   # FAT5_EINVAL
    assert msg in lib.fat5_last_error().decode()


# ----------------------------------------------------------------------------------------------------------------- operators
def test_python_checks_come_before_the_device():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import quantize_weight_mxfp4, w4_linear
    w4, e8 = torch.zeros(16, 64, dtype=torch.uint8), torch.zeros(16, 4, dtype=torch.uint8)
    x = torch.zeros(2, 3, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU path"):
        w4_linear(x, w4, e8)
    with pytest.raises(TypeError, match="fp16 or bf16"):
        w4_linear(x.float(), w4, e8)
    with pytest.raises(ValueError, match="columns"):
        w4_linear(x[..., :64], w4, e8)
    with pytest.raises(ValueError, match="residual must be"):
        w4_linear(x, w4, e8, residual=torch.zeros(2, 3, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="multiple of 32"):
        w4_linear(x[..., :48].contiguous(), torch.zeros(16, 24, dtype=torch.uint8), e8)
    with pytest.raises(ValueError, match="multiple of 8"):
        quantize_weight_mxfp4(torch.zeros(12, 64))
    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_weight_mxfp4(torch.zeros(8, 16416))
    with pytest.raises(ValueError, match="no CPU path"):
        quantize_weight_mxfp4(torch.zeros(8, 32))
    with FakeTensorMode():
        y = torch.ops.fat5.w4_linear(torch.empty(3, 128, dtype=torch.bfloat16), torch.empty(24, 64, dtype=torch.uint8),
                                     torch.empty(24, 4, dtype=torch.uint8), None, 1e-6, None)
        assert y.shape == (3, 24) and y.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------------ generate's host checks
@pytest.mark.parametrize("kernel", ["matrix", "rows"])
def test_mxfp4_has_no_weight_kernel(kernel, monkeypatch):
    m = _small_model().bfloat16()
    _no_encoder(monkeypatch, m)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="weight_kernel"):
        m.generate(ids, max_length=4, weight_dtype="mxfp4", weight_kernel=kernel)
    with pytest.raises(ValueError, match="weight_kernel"):
        m.init_decode_state(ids, max_length=4, weight_dtype="mxfp4", weight_kernel=kernel)


def test_fp32_models_are_refused_before_the_encoder(monkeypatch):
    m = _small_model()
    _no_encoder(monkeypatch, m)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="mxfp4.*fp16 or bf16"):
        m.generate(ids, max_length=4, weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="mxfp4.*fp16 or bf16"):
        m.init_decode_state(ids, max_length=4, weight_dtype="mxfp4")
    with pytest.raises(ValueError, match="fp16 or bf16"):
        m.quantize_decoder_weights_mxfp4()
