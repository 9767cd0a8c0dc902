"""The FP8 KV cache without a device: the ABI (struct sizes, exports, FAT5_EINVAL before any launch), the operators' host-side
rejections, generate's `kv_cache_dtype` check before an encoder runs, the restatement of the storage rule (tests/kvfp8_ref.py)
with its round-trip property and the mutants it must tell apart, and the fp64 helper of the attention tests against an fp32
emulation of the kernel's arithmetic, with and without defects."""
import ctypes
import math

import pytest
import torch

import kvfp8_ref as R

FP8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_struct_sizes_and_exports():
    from flasht5_amd import _lib
    lib = _lib.load()
    assert lib.fat5_sizeof_decode_params() == ctypes.sizeof(_lib.DecodeParams)
    assert lib.fat5_sizeof_decode_chunk_params() == ctypes.sizeof(_lib.DecodeChunkParams)
    assert lib.fat5_sizeof_decode_kv8_params() == ctypes.sizeof(_lib.DecodeKV8Params)
    assert lib.fat5_sizeof_kv_quant_params() == ctypes.sizeof(_lib.KvQuantParams)
    for name in ("fat5_kv_quantize", "fat5_sizeof_kv_quant_params", "fat5_attn_decode_kv8", "fat5_sizeof_decode_kv8_params"):
        assert name in _lib.EXPORTS
    for name in _lib.EXPORTS:
        getattr(lib, name)
    # the new fields are the last ones: everything before them sits where it sat.  The one-row descriptor keeps its own end
    # (cache_B) and its size; the fields follow it in the descriptor that extends it
    new = ["cache_dtype", "k_scale", "v_scale", "k_scale_stride", "v_scale_stride"]
    assert [f[0] for f in _lib.DecodeParams._fields_][-1] == "cache_B"
    assert [f[0] for f in _lib.DecodeKV8Params._fields_] == ["base"] + new and _lib.DecodeKV8Params.base.offset == 0
    assert _lib.DecodeKV8Params.base.size == ctypes.sizeof(_lib.DecodeParams) <= _lib.DecodeKV8Params.cache_dtype.offset
    names = [f[0] for f in _lib.DecodeChunkParams._fields_]
    assert names[names.index("chunk_seqlens") + 1:] == new
    import flasht5_amd
    assert callable(flasht5_amd.quantize_kv)


def _decode_params(chunk=False, D=64):
    """a descriptor that passes every check up to the workspace (pointers are never followed: the checks run first)"""
    from flasht5_amd import _lib
    p = _lib.DecodeChunkParams() if chunk else _lib.DecodeKV8Params()
    p.B, p.H, p.D, p.dtype, p.capacity, p.N, p.sm_scale, p.num_splits = 1, 2, D, _lib.FAT5_BF16, 8, 8, 0.125, 1
    if chunk:
        p.M = 2
    p.q = p.k_cache = p.v_cache = p.o = 4096
    return p


def _einval(call, p, msg):
    from flasht5_amd import _lib
    assert call(ctypes.byref(p), None) == -1, msg       # FAT5_EINVAL
    assert msg in _lib.load().fat5_last_error().decode()


@pytest.mark.parametrize("chunk", [False, True])
def test_einval_without_a_device(chunk):
    from flasht5_amd import _lib
    lib = _lib.load()
    call = lib.fat5_attn_decode_chunk if chunk else lib.fat5_attn_decode_kv8
    p = _decode_params(chunk)
    p.cache_dtype = 2
    _einval(call, p, "cache_dtype 2")
    p.cache_dtype = -1
    _einval(call, p, "cache_dtype -1")
    p.cache_dtype = _lib.KV_FP8_E4M3
    _einval(call, p, "needs k_scale and v_scale")
    p.k_scale = 4096
    _einval(call, p, "needs k_scale and v_scale")         # (one of the two)
    p.v_scale = 4098
    _einval(call, p, "needs k_scale and v_scale")         # (misaligned)
    p = _decode_params(chunk, D=32)
    p.cache_dtype, p.k_scale, p.v_scale = _lib.KV_FP8_E4M3, 4096, 4096
    _einval(call, p, "head_dim 32")


def test_quantizer_einval_and_empty_without_a_device():
    from flasht5_amd import _lib
    lib = _lib.load()
    p = _lib.KvQuantParams()
    p.B, p.L, p.H, p.D, p.dtype = 1, 4, 2, 64, _lib.FAT5_BF16
    p.x = p.out = p.scale = 4096
    p.x_stride[:] = p.out_stride[:] = (512, 128, 64)
    p.scale_stride[:] = (8, 2, 1)
    for field, val, msg in (("D", 32, "head_dim 32"), ("dtype", _lib.FAT5_F32, "dtype 0"), ("L", -1, "L -1"), ("x", 4100, "x: null or unaligned"),
                            ("out", 4100, "out: null or unaligned"), ("scale", 0, "scale: null or unaligned")):
        old = getattr(p, field)
        setattr(p, field, val)
        _einval(lib.fat5_kv_quantize, p, msg)
        setattr(p, field, old)
    p.x_stride[1] = 100
    _einval(lib.fat5_kv_quantize, p, "multiples of 8")
    p.L = 0                                                # no rows: a no-op, whatever the pointers are, and nothing is launched
    assert lib.fat5_kv_quantize(ctypes.byref(p), None) == 0
    assert lib.fat5_kv_quantize(None, None) == -1


# ------------------------------------------------------------------------------------------------- the operators' host checks
def _op_args(D=64, M=1, B=2, cap=8, H=2):
    q = torch.zeros(B, M, H, D, dtype=torch.bfloat16)
    kc = torch.zeros(B, cap, H, D, dtype=torch.uint8).view(FP8)
    vc = torch.zeros(B, cap, H, D, dtype=torch.uint8).view(FP8)
    ks, vs = torch.zeros(B, cap, H), torch.zeros(B, cap, H)
    return q, kc, vc, ks, vs


@pytest.mark.parametrize("chunk", [False, True])
def test_operator_rejections_on_the_host(chunk):
    from flasht5_amd import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk
    op = flash_attn_with_kvcache_chunk if chunk else flash_attn_with_kvcache
    M = 3 if chunk else 1
    q, kc, vc, ks, vs = _op_args(M=M)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        op(q, kc, vc)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        op(q, kc, vc, k_scale=ks)
    with pytest.raises(ValueError, match=r"k_scale must be an fp32 \(B, L_cap, H\)"):
        op(q, kc, vc, k_scale=ks[:, :4], v_scale=vs)                               # shape
    with pytest.raises(ValueError, match=r"v_scale must be an fp32"):
        op(q, kc, vc, k_scale=ks, v_scale=vs.double())                             # dtype
    with pytest.raises(ValueError, match="stride of 0"):
        op(q, kc, vc, k_scale=ks[:, :1].expand(-1, 8, -1), v_scale=vs)             # stride: every row needs its own element
    with pytest.raises(ValueError, match="go with float8_e4m3fn caches"):
        op(q, kc.view(torch.uint8).to(torch.bfloat16), vc.view(torch.uint8).to(torch.bfloat16), k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="go with float8_e4m3fn caches"):
        op(q, kc, vc.view(torch.uint8).to(torch.bfloat16), k_scale=ks, v_scale=vs)
    q32, kc32, vc32, ks32, vs32 = _op_args(D=32, M=M)
    with pytest.raises(ValueError, match="head_dim 32"):
        op(q32, kc32, vc32, k_scale=ks32, v_scale=vs32)
    with pytest.raises(ValueError, match="dtype mismatch"):                         # the new rows keep q's dtype
        op(q, kc, vc, k=torch.zeros_like(q).half(), v=torch.zeros_like(q).half(), cache_seqlens=torch.zeros(2, dtype=torch.int32),
           k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="tensors must be on the GPU"):            # valid arguments reach the device check
        op(q, kc, vc, k_scale=ks, v_scale=vs)
    # today's messages for today's mistakes
    with pytest.raises(ValueError, match="dtype mismatch"):
        op(q, kc.view(torch.uint8).to(torch.float16), vc.view(torch.uint8).to(torch.float16))
    with pytest.raises(TypeError, match="fp16 or bf16"):
        op(q.float(), torch.zeros(2, 8, 2, 64), torch.zeros(2, 8, 2, 64))


def test_quantize_kv_rejections_on_the_host():
    from flasht5_amd import quantize_kv
    with pytest.raises(ValueError, match="head_dim 32"):
        quantize_kv(torch.zeros(1, 2, 2, 32, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="fp16 or bf16"):
        quantize_kv(torch.zeros(1, 2, 2, 64))
    with pytest.raises(ValueError, match="out must be a float8_e4m3fn"):
        quantize_kv(torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16), out=torch.zeros(1, 2, 2, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="scale must be an fp32"):
        quantize_kv(torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16), scale=torch.zeros(1, 2, 3))
    with pytest.raises(ValueError, match="on the GPU"):
        quantize_kv(torch.zeros(1, 2, 2, 64, dtype=torch.bfloat16))


def test_custom_ops_declare_their_mutations_and_have_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import decode  # noqa: F401  (registers the ops)
    def written(op):
        return {a.name for a in op.default._schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    for op in (torch.ops.fat5.attn_decode_fp8, torch.ops.fat5.attn_decode_chunk_fp8):
        assert written(op) == {"k_cache", "v_cache", "k_scale", "v_scale"}
    for op in (torch.ops.fat5.attn_decode, torch.ops.fat5.attn_decode_chunk):   # (the 16-bit operators keep their schemas)
        assert written(op) == {"k_cache", "v_cache"}
    assert written(torch.ops.fat5.kv_quantize) == {"out", "scale"}
    with FakeTensorMode():
        q, kc, vc, ks, vs = _op_args(M=1)
        o, lse = torch.ops.fat5.attn_decode_fp8(q, kc, vc, ks, vs, None, None, None, 0.125, None, 0, True, 0, None, None)
        assert o.shape == (2, 1, 2, 64) and o.dtype == torch.bfloat16 and lse.shape == (2, 2, 1)
        q, kc, vc, ks, vs = _op_args(M=3)
        o, lse = torch.ops.fat5.attn_decode_chunk_fp8(q, kc, vc, ks, vs, None, None, None, 0.125, True, None, 0, False, 0, None)
        assert o.shape == (2, 3, 2, 64) and lse.shape == (0,)
        assert torch.ops.fat5.kv_quantize(torch.empty(1, 2, 2, 64, dtype=torch.bfloat16), torch.empty(1, 2, 2, 64, dtype=FP8),
                                          torch.empty(1, 2, 2)) is None


# ------------------------------------------------------------------------------------------------------- generate's host check
def _small_model(**kw):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    cfg = dict(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
               relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe")
    cfg.update(kw)
    return FAT5ForConditionalGeneration(FAT5Config(**cfg))


class _Reached(Exception):
    pass


def test_generate_checks_kv_cache_dtype_before_the_encoder(monkeypatch):
    m, a = _small_model(), _small_model(num_decoder_layers=1)

    def boom(*args, **kw):
        raise AssertionError("an encoder ran before the arguments were checked")
    for x in (m, a):
        monkeypatch.setattr(x.encoder, "forward", boom)
    ids = torch.zeros(2, 4, dtype=torch.long)
    for bad in ("int4", "fp8_e5m2", "FP8", 8, torch.float8_e4m3fn):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            m.generate(ids, max_length=8, kv_cache_dtype=bad)
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            m.init_decode_state(ids, max_length=8, kv_cache_dtype=bad)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m.generate(ids, max_length=8, kv_cache_dtype="int4", num_beams=3)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m.generate(ids, max_length=8, kv_cache_dtype="int4", assistant_model=a)

    def reached(*args, **kw):
        raise _Reached()
    for x in (m, a):
        monkeypatch.setattr(x.encoder, "forward", reached)
    for good in (None, "fp8", "fp8_e4m3"):                      # valid values pass the host checks and go on to the encoder
        with pytest.raises(_Reached):
            m.generate(ids, max_length=8, kv_cache_dtype=good)
        with pytest.raises(_Reached):
            m.generate(ids, max_length=8, kv_cache_dtype=good, num_beams=2, graph=True)
        with pytest.raises(_Reached):
            m.generate(ids, max_length=8, kv_cache_dtype=good, assistant_model=a)


def test_decode_state_keeps_its_constructor():
    from flasht5_amd.generation import DecodeState
    z = torch.zeros(1)
    st = DecodeState(z, [z], [z], [z], [z], torch.zeros(1, dtype=torch.int32), None, 4)
    assert st.self_k_scale is None and st.cross_v_scale is None and st.scales(0) == ({}, {})


# ---------------------------------------------------------------------------------------------------------- the restatement
def _rows(dtype, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    normal = torch.randn(48, D, generator=g) * torch.logspace(-3, 3, 48).unsqueeze(1)
    # rows spanning 12 binades: element d at 2^(-12 d / (D - 1)) of the row's largest, signs mixed
    span = torch.exp2(-12.0 * torch.arange(D) / (D - 1)).unsqueeze(0) * (torch.rand(16, 1, generator=g) + 0.5)
    span = span * torch.where(torch.rand(16, D, generator=g) < 0.5, -1.0, 1.0)
    span = span[:, torch.randperm(D, generator=g)]
    # 20 binades below a largest element of 1: the small end lands in the format's subnormal range (quotients below 2^-6)
    deep = torch.exp2(-20.0 * torch.arange(D) / (D - 1)).unsqueeze(0) * torch.where(torch.rand(8, D, generator=g) < 0.5, -1.0, 1.0)
    return torch.cat((normal, span, deep)).to(dtype)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_trip_property(dtype, D):
    x = _rows(dtype, D)
    b, s = R.quantize_ref(x)
    assert b.dtype == FP8 and s.dtype == torch.float32 and s.shape == x.shape[:-1]
    err = (R.dequant(b, s) - x.double()).abs()
    bound = R.roundtrip_bound(x, s)
    assert bool((err <= bound).all()), float((err / bound).max())
    # the row's largest element sits at +-448 exactly, and nothing is NaN
    assert bool((b.float().abs().amax(-1) == 448).all()) and not bool(torch.isnan(b.float()).any())
    # the 12-binade rows stay normal numbers of the format (448 * 2^-12 > 2^-6); the 20-binade rows reach its subnormals and the
    # bound's second branch, down to quotients that round to zero
    y = x.float() / s.unsqueeze(-1)
    assert bool((y[48:64].abs() >= 2.0 ** -6).all())
    assert bool((y[64:].abs() < 2.0 ** -6).any()) and bool((bound[64:] > x[64:].double().abs() * 2.0 ** -4).any())
    assert bool(((b[64:].float() == 0) & (x[64:] != 0)).any())


def test_special_rows_of_the_rule():
    x = torch.zeros(6, 64, dtype=torch.bfloat16)
    x[1, 5] = -3.0                                   # one element at -amax
    x[2] = 1e-30                                     # tiny
    x[3, 0], x[3, 1] = 1.0, float("nan")
    x[4, 0], x[4, 1] = 1.0, float("-inf")
    x[5, :4] = torch.tensor([448.0, 17.0, 19.0, 0.9])  # s = 1: 17 and 19 are ties between (16, 18, 20): to even -> 16 and 20
    b, s = R.quantize_ref(x)
    u8 = b.view(torch.uint8)
    assert s[0] == 1 and bool((u8[0] == 0).all())
    assert s[1] == torch.tensor(3.0) / 448 and u8[1, 5] == 0xFE and bool((u8[1, :5] == 0).all())
    assert bool((u8[2] == 0x7E).all()) and math.isfinite(float(s[2])) and s[2] > 0
    for r in (3, 4):                                 # the documented non-finite rule: s = +inf, the row reads back as NaN
        assert math.isinf(float(s[r])) and s[r] > 0 and u8[r, 1] == 0x7F and (u8[r, 0] & 0x7F) == 0
        assert bool(torch.isnan(R.dequant(b, s)[r]).all())
    assert s[5] == 1 and b[5, :4].float().tolist() == [448.0, 16.0, 20.0, 0.875]


@pytest.mark.parametrize("name", list(R.RULE_MUTANTS))
def test_the_restatement_tells_the_mutants_apart(name):
    """bytes or scales differ from the rule's on ordinary rows, and (all but the wrong axis, which is a valid quantisation of
    another grouping) the round-trip property or finiteness breaks"""
    x = _rows(torch.bfloat16, 64, seed=1)
    b, s = R.quantize_ref(x)
    bm, sm = R.RULE_MUTANTS[name](x)
    assert not R.same_bits(b, s, bm, sm)
    if name != "amax over the wrong axis":
        d = R.dequant(bm, sm)
        ok = torch.isfinite(d).all() and bool(((d - x.double()).abs() <= R.roundtrip_bound(x, s)).all())
        assert not ok


# ---------------------------------------------------------------------- the fp64 helper against an fp32 emulation and its defects
def _emu_case(D, L, seed=0, B=2, H=2, cap=None):
    g = torch.Generator().manual_seed(seed)
    cap = cap or L + 3
    q = torch.randn(B, 1, H, D, generator=g).bfloat16()
    kb, ks = R.quantize_ref((torch.randn(B, cap, H, D, generator=g) * torch.rand(B, cap, H, 1, generator=g) * 4).bfloat16())
    vb, vs = R.quantize_ref((torch.randn(B, cap, H, D, generator=g) * torch.rand(B, cap, H, 1, generator=g) * 4).bfloat16())
    kn, vn = torch.randn(B, 1, H, D, generator=g).bfloat16(), torch.randn(B, 1, H, D, generator=g).bfloat16()
    return q, kb, ks, vb, vs, [L, max(L - 1, 0)], kn, vn


@pytest.mark.parametrize("D, L", [(64, 0), (64, 5), (128, 65), (64, 130)])
def test_helper_accepts_the_emulation_and_catches_its_defects(D, L):
    q, kb, ks, vb, vs, lens, kn, vn = _emu_case(D, L)
    scale = D ** -0.5

    def ratio(mutant):
        o, lse, (kb2, ks2, vb2, vs2) = R.emulate_decode8(q, kb, ks, vb, vs, lens, kn, vn, scale, mutant)
        ref = R.decode_ref8(q, kb2, ks2, vb2, vs2, lens, True, scale)
        bo, bl = R.decode_bound8(ref, torch.float32, D, 1)
        ro, rl, same = F_ratios(o, lse, ref, bo, bl)
        return max(ro, rl) if same else math.inf
    # the emulation sums in another order than the kernel, in fp32 like it: it must sit inside the bound with the fp32 output ulp
    assert ratio(None) <= 1.0
    for mutant in R.EMU_MUTANTS:
        if mutant == "v scale from the wrong row" and L == 0:
            continue   # (one key: there is no other row)
        assert ratio(mutant) > 1.0, mutant


def F_ratios(o, lse, ref, bo, bl):
    import decode_fp64 as F
    return F.ratios(o, lse, ref, bo, bl)
