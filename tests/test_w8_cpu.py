"""FP8 weights without a device: the restatement (tests/w8_ref.py) on a hand-worked case, its bound against an fp32 emulation of
the kernel's arithmetic in two summation orders and with the defects it must tell apart, the ABI (exports, struct sizes,
FAT5_EINVAL before any launch), the operators' fakes, and generate's `weight_dtype` checks before an encoder runs."""
import ctypes

import pytest
import torch

import w8_ref as R


# ----------------------------------------------------------------------------------------------------------- the restatement
def test_hand_worked_2x64():
    W = torch.zeros(2, 64)
    W[0, 0] = 448.0                                   # amax 448 -> s = 1, the element is the largest e4m3 value, byte 0x7E
    W[1, 0], W[1, 1], W[1, 2] = 224.0, 1.0, -0.5      # amax 224 -> s = 0.5: 448 -> 0x7E, 2.0 -> 0x40, -1.0 -> 0xB8
    w8, s = R.quantize_ref(W.bfloat16())
    assert s.tolist() == [1.0, 0.5]
    b = w8.view(torch.uint8)
    assert b[0, 0] == 0x7E and int(b[0, 1:].max()) == 0
    assert b[1, :3].tolist() == [0x7E, 0x40, 0xB8] and int(b[1, 3:].max()) == 0
    x = torch.zeros(1, 64)
    x[0, 0], x[0, 1], x[0, 2] = 1.0, 2.0, -4.0
    x = x.bfloat16()
    ref, A = R.linear_ref(x, w8, s)
    assert ref.tolist() == [[448.0, 228.0]]           # 1 * 448 * 1;  0.5 * (448 + 2 * 2 + (-4) * (-1))
    assert A.tolist() == [[448.0, 228.0]]
    _, y, out = R.emulate(x, w8, s)
    assert y.tolist() == [[448.0, 228.0]] and out is y
    res = torch.tensor([[1.0, 0.5]]).bfloat16()
    _, y, out = R.emulate(x, w8, s, residual=res)
    assert out.tolist() == [[448.0, 228.0]]           # 449 and 228.5 are no bf16 values: both ties go to even
    assert R.c_of_K(64) == 8 + 7 and R.c_of_K(512) == 15 and R.c_of_K(513) == 23 and R.c_of_K(2048) == 39


def test_zero_and_non_finite_rows():
    W = torch.randn(8, 64).bfloat16()
    W[1] = 0
    W[2, 5] = float("inf")
    W[3, 7] = float("nan")
    w8, s = R.quantize_ref(W)
    assert float(s[1]) == 1.0 and int(w8[1].view(torch.uint8).max()) == 0
    assert torch.isinf(s[2]) and torch.isinf(s[3])
    x = torch.randn(3, 64).bfloat16()
    ref, _ = R.linear_ref(x, w8, s)
    assert bool(torch.isnan(ref[:, 2:4]).all()) and bool(torch.isfinite(ref[:, [0, 1, 4, 5, 6, 7]]).all())


def _case(dtype, Rr=5, N=16, K=832, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Rr, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    gam = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    res = torch.randn(Rr, N, generator=g).to(dtype)
    w8, s = R.quantize_ref(W)
    return x, w8, s, gam, res


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("order", sorted(R.ORDERS))
@pytest.mark.parametrize("norm", [False, True])
def test_bound_accepts_the_emulation(dtype, order, norm):
    x, w8, s, gam, res = _case(dtype)
    xin, y, out = R.emulate(x, w8, s, norm_weight=gam if norm else None, residual=res, order=order)
    print(f"worst |y - ref| / bound: {R.worst(y, xin, w8, s):.3f}")
    assert R.accepts(y, xin, w8, s)
    assert torch.equal(out, R.residual_ref(y, res))


def test_the_two_orders_differ_somewhere():
    x, w8, s, _, _ = _case(torch.bfloat16, Rr=16, N=64)
    p = x.float().unsqueeze(1) * w8.float().unsqueeze(0)
    assert not torch.equal(R.ORDERS["kernel"](p), R.ORDERS["pairwise"](p))   # (so accepting both is no accident of equal sums)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_rejected(dtype, mutant):
    x, w8, s, gam, res = _case(dtype, Rr=16, N=32)
    good_xin, good_y, good_out = R.emulate(x, w8, s, norm_weight=gam, residual=res)
    xin, y, out = R.emulate(x, w8, s, norm_weight=gam, residual=res, mutant=mutant)
    assert torch.equal(xin, good_xin)   # (the contract's xin: what the reference starts from)
    if mutant == "residual added before the rounding":
        # a single rounding is closer to the truth, so no bound against fp64 can reject it: the epilogue is checked exactly
        assert R.accepts(y, xin, w8, s) and not torch.equal(out, R.residual_ref(y, res))
    else:
        assert not R.accepts(y, xin, w8, s)
        assert R.worst(y, xin, w8, s) > 1.0


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_exports_and_struct_sizes():
    from flasht5_amd import _lib
    lib = _lib.load()
    for name in ("fat5_w8_quantize", "fat5_sizeof_w8_quant_params", "fat5_w8_linear", "fat5_sizeof_w8_linear_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_w8_quant_params() == ctypes.sizeof(_lib.W8QuantParams)
    assert lib.fat5_sizeof_w8_linear_params() == ctypes.sizeof(_lib.W8LinearParams)


def _linear_params(**kw):
    from flasht5_amd import _lib
    p = _lib.W8LinearParams()
    p.R, p.N, p.K, p.dtype = 4, 16, 128, _lib.FAT5_BF16
    p.x = p.w8 = p.scale = p.y = 4096      # (never followed: every check comes before the launch)
    p.x_stride, p.w_stride, p.y_stride = 128, 128, 16
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, msg", [
    (dict(K=96), "K 96"), (dict(K=32), "K 32"), (dict(K=16448), "K 16448"), (dict(N=12), "N 12"), (dict(N=-8), "N -8"),
    (dict(R=-1), "R -1"), (dict(dtype=0), "dtype 0"), (dict(x_stride=64), "x_stride"), (dict(x_stride=132), "x_stride"),
    (dict(y_stride=8), "y_stride"), (dict(w_stride=120), "w_stride"), (dict(x=4100), "x: null or misaligned"),
    (dict(y=None), "y: null or misaligned"), (dict(w8=4097), "w8: null or misaligned"), (dict(scale=None), "scale"),
    (dict(residual=4096, residual_stride=8), "residual_stride"), (dict(norm_weight=4098), "norm_weight"),
    (dict(norm_weight=4096, eps=float("nan")), "eps"), (dict(reserved=1), "reserved"),
])
def test_linear_einval_without_a_device(kw, msg):
    from flasht5_amd import _lib
    lib = _lib.load()
    assert lib.fat5_w8_linear(ctypes.byref(_linear_params(**kw)), None) == -1, msg   # FAT5_EINVAL
    assert msg in lib.fat5_last_error().decode()


def test_linear_no_rows_or_columns_is_ok_without_a_device():
    from flasht5_amd import _lib
    lib = _lib.load()
    assert lib.fat5_w8_linear(ctypes.byref(_linear_params(R=0, x=None, y=None)), None) == 0
    assert lib.fat5_w8_linear(ctypes.byref(_linear_params(N=0, w8=None, scale=None, y=None)), None) == 0
    assert lib.fat5_w8_linear(None, None) == -1


@pytest.mark.parametrize("kw, msg", [
    (dict(K=100), "K 100"), (dict(N=4), "N 4"), (dict(dtype=7), "dtype 7"), (dict(w_stride=32), "w_stride"),
    (dict(out_stride=60), "out_stride"), (dict(w=8), "w: null or misaligned"), (dict(out=4), "out: null or misaligned"),
    (dict(scale=2), "scale"),
])
def test_quantize_einval_without_a_device(kw, msg):
    from flasht5_amd import _lib
    lib = _lib.load()
    p = _lib.W8QuantParams()
    p.N, p.K, p.dtype, p.w, p.out, p.scale, p.w_stride, p.out_stride = 8, 64, _lib.FAT5_F32, 4096, 4096, 4096, 64, 64
    for k, v in kw.items():
        setattr(p, k, v)
    assert lib.fat5_w8_quantize(ctypes.byref(p), None) == -1, msg
    assert msg in lib.fat5_last_error().decode()
    p = _lib.W8QuantParams()
    p.N, p.K, p.dtype = 0, 64, _lib.FAT5_F32
    assert lib.fat5_w8_quantize(ctypes.byref(p), None) == 0


# ----------------------------------------------------------------------------------------------------------------- operators
def test_operators_have_schemas_and_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import w8  # noqa: F401  (registers the ops)
    schema = torch.ops.fat5.w8_quantize.default._schema
    assert {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write} == {"out", "scale"}
    schema = torch.ops.fat5.w8_linear.default._schema
    assert not any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments)
    with FakeTensorMode():
        x = torch.empty(3, 128, dtype=torch.bfloat16)
        y = torch.ops.fat5.w8_linear(x, torch.empty(24, 128, dtype=torch.float8_e4m3fn), torch.empty(24), None, 1e-6, None)
        assert y.shape == (3, 24) and y.dtype == torch.bfloat16


def test_python_checks_come_before_the_device():
    from flasht5_amd import quantize_weight, w8_linear
    w8, s = torch.empty(16, 128, dtype=torch.float8_e4m3fn), torch.empty(16)
    x = torch.zeros(2, 3, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU path"):
        w8_linear(x, w8, s)
    with pytest.raises(TypeError, match="fp16 or bf16"):
        w8_linear(x.float(), w8, s)
    with pytest.raises(ValueError, match="columns"):
        w8_linear(x[..., :64], w8, s)
    with pytest.raises(ValueError, match="residual must be"):
        w8_linear(x, w8, s, residual=torch.zeros(2, 3, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="norm_weight"):
        w8_linear(x, w8, s, norm_weight=torch.ones(128))
    with pytest.raises(ValueError, match="multiple of 64"):
        w8_linear(x[..., :96].contiguous(), torch.empty(16, 96, dtype=torch.float8_e4m3fn), s)
    with pytest.raises(ValueError, match="multiple of 8"):
        quantize_weight(torch.zeros(12, 64))
    with pytest.raises(ValueError, match="multiple of 64"):
        quantize_weight(torch.zeros(8, 16448))
    with pytest.raises(ValueError, match="no CPU path"):
        quantize_weight(torch.zeros(8, 64))


# ------------------------------------------------------------------------------------------------------ generate's host checks
def _small_model(vocab=128, **kw):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    cfg = dict(vocab_size=vocab, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
               relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe")
    cfg.update(kw)
    return FAT5ForConditionalGeneration(FAT5Config(**cfg))


def _no_encoder(monkeypatch, *models):
    def boom(*a, **k):
        raise AssertionError("an encoder ran before the arguments were checked")
    for m in models:
        monkeypatch.setattr(m.encoder, "forward", boom)


@pytest.mark.parametrize("value", ["int4", "fp16", 8, True])
def test_weight_dtype_is_checked_before_the_encoder(value, monkeypatch):
    m = _small_model().bfloat16()
    _no_encoder(monkeypatch, m)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="weight_dtype"):
        m.generate(ids, max_length=4, weight_dtype=value)
    with pytest.raises(ValueError, match="weight_dtype"):
        m.init_decode_state(ids, max_length=4, weight_dtype=value)


@pytest.mark.parametrize("alias", ["fp8", "fp8_e4m3"])
def test_fp32_weights_are_refused_before_the_encoder(alias, monkeypatch):
    m = _small_model()
    _no_encoder(monkeypatch, m)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        m.generate(ids, max_length=4, weight_dtype=alias)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        m.init_decode_state(ids, max_length=4, weight_dtype=alias)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        m.quantize_decoder_weights()
    mixed = _small_model().bfloat16()
    mixed.decoder.block[0].ff_layer.wo.float()
    _no_encoder(monkeypatch, mixed)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        mixed.generate(ids, max_length=4, weight_dtype=alias)


def test_shapes_outside_the_contract_and_the_assistant_are_refused_before_the_encoders(monkeypatch):
    ids = torch.zeros(2, 4, dtype=torch.long)
    odd = _small_model(vocab=100).bfloat16()          # lm_head: N = 100, no multiple of 8
    _no_encoder(monkeypatch, odd)
    with pytest.raises(ValueError, match="multiple of 8"):
        odd.generate(ids, max_length=4, weight_dtype="fp8")
    m, a = _small_model().bfloat16(), _small_model(num_decoder_layers=1)   # (the assistant's weights are fp32)
    _no_encoder(monkeypatch, m, a)
    with pytest.raises(ValueError, match="assistant_model.*fp16 or bf16"):
        m.generate(ids, max_length=4, assistant_model=a, num_assistant_tokens=2, weight_dtype="fp8")


def test_none_goes_on_to_the_encoder(monkeypatch):
    m = _small_model()

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached

    monkeypatch.setattr(m.encoder, "forward", reached)
    with pytest.raises(Reached):
        m.generate(torch.zeros(2, 4, dtype=torch.long), max_length=4, weight_dtype=None)
