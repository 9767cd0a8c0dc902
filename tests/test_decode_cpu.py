"""CPU tests of KV-cached decoding: the C ABI's argument checks of fat5_attn_decode (all before any launch: fake, aligned pointers
are enough), the ctypes mirror of fat5_decode_params, the workspace query, the custom op's fake implementation, the Python-side
rejections, the refusal of FIRE and randomized positions at decode time, and a state dict loading unchanged into a model used for
generation."""
import ctypes

import pytest
import torch

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.DecodeParams()
    B, H, D, cap = 2, 4, 64, 256
    p.B, p.H, p.D, p.dtype, p.capacity, p.N = B, H, D, _lib.FAT5_BF16, cap, 0
    p.cache_seqlens = BASE
    p.sm_scale = 0.125
    for i, f in enumerate(("q", "k_cache", "v_cache", "k_new", "v_new", "o", "lse")):
        setattr(p, f, BASE + 4096 * (i + 1))
    p.q_stride[:] = (H * D, D)
    p.o_stride[:] = (H * D, D)
    p.k_new_stride[:] = (H * D, D)
    p.v_new_stride[:] = (H * D, D)
    p.k_cache_stride[:] = (cap * H * D, H * D, D)
    p.v_cache_stride[:] = (cap * H * D, H * D, D)
    p.num_splits = 1  # (no workspace needed unless a case asks for one)
    for k, v in kw.items():
        if k.endswith("_stride"):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    return p


def test_struct_size_matches_library(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_decode_params() == ctypes.sizeof(_lib.DecodeParams)
    assert "fat5_attn_decode" in _lib.EXPORTS and "fat5_attn_decode_workspace_bytes" in _lib.EXPORTS


@pytest.mark.parametrize("bad, msg", [
    (dict(D=32), "head_dim"), (dict(D=96), "head_dim"), (dict(dtype=0), "dtype"), (dict(dtype=5), "dtype"),
    (dict(B=0), "B 0"), (dict(H=0), "H 0"), (dict(capacity=-1), "capacity"), (dict(num_splits=129), "num_splits"),
    (dict(bias_mode=2, rpe_radius=0, rpe1d=BASE), "rpe_radius"), (dict(bias_mode=2, rpe_radius=2049, rpe1d=BASE), "rpe_radius"),
    (dict(bias_mode=2, rpe_radius=16, rpe1d=None), "needs rpe1d"), (dict(bias_mode=1), "bias_mode"),
    (dict(v_new=None), "both"), (dict(k_new=None), "both"), (dict(cache_seqlens=None), "needs cache_seqlens"),
    (dict(cache_seqlens=None, k_new=None, v_new=None, N=300), "N 300"),
    (dict(q=None), "q:"), (dict(q=BASE + 8), "unaligned"), (dict(k_cache=BASE + 2), "k_cache"), (dict(o=None), "o:"),
    (dict(q_stride=(4 * 64, 60)), "multiples"), (dict(k_cache_stride=(256 * 256, 256, 65)), "multiples"),
    (dict(v_new_stride=(3, 64)), "multiples"), (dict(sm_scale=float("inf")), "sm_scale"),
])
def test_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_attn_decode(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


def test_workspace_checked(lib):
    p = _params(num_splits=8)
    need = lib.fat5_attn_decode_workspace_bytes(ctypes.byref(p))
    assert need == 2 * 4 * 8 * (64 + 2) * 4  # [B][H][splits] (max, sum) + o[D], fp32
    assert lib.fat5_attn_decode(ctypes.byref(p), None) == -3
    assert "workspace" in lib.fat5_last_error().decode()
    p.workspace, p.workspace_bytes = BASE + 65536, need - 16
    assert lib.fat5_attn_decode(ctypes.byref(p), None) == -3
    p.workspace, p.workspace_bytes = BASE + 65536 + 8, need
    assert lib.fat5_attn_decode(ctypes.byref(p), None) == -3


def test_split_policy_is_host_known(lib):
    # one split (no workspace) when the capacity holds one workgroup pass; the library's choice never exceeds 128 splits
    assert lib.fat5_attn_decode_workspace_bytes(ctypes.byref(_params(num_splits=0, capacity=33))) == 0
    for B, cap in ((1, 4096), (16, 1024), (64, 4096), (1, 1 << 20)):
        n = lib.fat5_attn_decode_workspace_bytes(ctypes.byref(_params(num_splits=0, B=B, capacity=cap)))
        splits = n // (B * 4 * (64 + 2) * 4)
        assert 1 <= splits <= 128 or n == 0


def test_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import decode  # noqa: F401  (registers the op)
    with FakeTensorMode():
        B, H, D, cap = 3, 6, 64, 40
        q = torch.empty(B, 1, H, D, dtype=torch.bfloat16)
        kc = torch.empty(B, H, cap, D, dtype=torch.bfloat16).transpose(1, 2)  # (a (B, H, L, D) buffer seen as (B, L, H, D))
        vc = torch.empty(B, cap, H, D, dtype=torch.bfloat16)
        lens = torch.empty(B, dtype=torch.int32)
        o, lse = torch.ops.fat5.attn_decode(q, kc, vc, q, q, lens, 0.125, None, 0, True, 0)
        assert o.shape == (B, 1, H, D) and o.dtype == torch.bfloat16 and o.is_contiguous()
        assert lse.shape == (B, H, 1) and lse.dtype == torch.float32 and lse.is_contiguous()
        o, lse = torch.ops.fat5.attn_decode(q, kc, vc, None, None, None, 0.125, None, 0, False, 0)
        assert o.stride() == (H * D, H * D, D, 1) and lse.numel() == 0


def test_python_rejections():
    from flasht5_amd.decode import flash_attn_with_kvcache
    bf = torch.bfloat16
    q = torch.zeros(2, 1, 4, 64, dtype=bf)
    kc = torch.zeros(2, 16, 4, 64, dtype=bf)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_attn_with_kvcache(q.clone().requires_grad_(), kc, kc)
    # shape / dtype / bias checks come before the device check: reachable on any host
    cases = [
        (dict(q=torch.zeros(2, 2, 4, 64, dtype=bf)), ValueError, r"\(B, 1, H, D\)"),
        (dict(q=q.float(), k_cache=kc.float(), v_cache=kc.float()), TypeError, "fp16 or bf16"),
        (dict(q=q.half()), ValueError, "dtype mismatch"),
        (dict(q=torch.zeros(2, 1, 4, 32, dtype=bf), k_cache=torch.zeros(2, 16, 4, 32, dtype=bf),
              v_cache=torch.zeros(2, 16, 4, 32, dtype=bf)), ValueError, "head_dim"),
        (dict(k_cache=torch.zeros(2, 16, 3, 64, dtype=bf)), ValueError, "k_cache must be"),
        (dict(v_cache=torch.zeros(2, 17, 4, 64, dtype=bf)), ValueError, "capacities"),
        (dict(k=q), ValueError, "both k and v"),
        (dict(k=q, v=q), ValueError, "needs cache_seqlens"),
        (dict(k=q, v=q, cache_seqlens=torch.zeros(3, dtype=torch.int32)), ValueError, "2 lengths"),
        (dict(rpe1d=torch.zeros(4, 257), rpe_radius=0), ValueError, "rpe_radius 0"),
        (dict(rpe1d=torch.zeros(4, 129), rpe_radius=128), ValueError, r"\(4, 257\)"),  # (a generator of radius 64 claimed as 128)
        (dict(rpe1d=torch.zeros(3, 257), rpe_radius=128), ValueError, "rpe1d must be"),
        (dict(rpe1d=torch.zeros(4, 257, dtype=torch.float64), rpe_radius=128), ValueError, "rpe1d must be"),
        (dict(), ValueError, "GPU"),
    ]
    for kw, exc, msg in cases:
        args = dict(q=q, k_cache=kc, v_cache=kc)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            flash_attn_with_kvcache(**args)


def _small_config(**kw):
    from flasht5_amd import FAT5Config
    base = dict(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                relative_attention_max_distance=64, max_sequence_length=64)
    base.update(kw)
    return FAT5Config(**base)


def test_fire_refused_at_decode_time():
    from flasht5_amd import FAT5ForConditionalGeneration
    m = FAT5ForConditionalGeneration(_small_config(attention_type="triton", position_encoding_type="FIRE"))
    with pytest.raises(NotImplementedError, match="FIRE"):
        m.generate(torch.zeros(1, 4, dtype=torch.long))
    attn = m.decoder.block[0].self_attention_layer.self_attention
    with pytest.raises(NotImplementedError, match="FIRE"):
        attn.forward_decode(torch.zeros(1, 1, 64), torch.zeros(1, 4, 2, 64), torch.zeros(1, 4, 2, 64), torch.zeros(1, dtype=torch.int32))


def test_randomized_positions_refused_at_decode_time():
    from flasht5_amd import FAT5ForConditionalGeneration
    c = _small_config()
    c.use_randomized_position_encoding = True
    m = FAT5ForConditionalGeneration(c)
    with pytest.raises(NotImplementedError, match="randomized"):
        m.generate(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="randomized"):
        m.decoder.block[1].self_attention_layer.self_attention.forward_decode(
            torch.zeros(1, 1, 64), torch.zeros(1, 4, 2, 64), torch.zeros(1, 4, 2, 64), torch.zeros(1, dtype=torch.int32))


def test_rope_capacity_beyond_the_tables_is_refused():
    from flasht5_amd import FAT5ForConditionalGeneration
    m = FAT5ForConditionalGeneration(_small_config(position_encoding_type="RoPE"))  # (tables of max_sequence_length = 64 rows)
    with pytest.raises(ValueError, match="rotary tables"):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=64)  # (before any encoder or device work)
    with pytest.raises(ValueError, match="rotary tables"):
        m.init_decode_state(torch.zeros(1, 4, dtype=torch.long), max_length=1000)


def test_decode_step_refuses_to_run_past_the_capacity():
    from flasht5_amd import FAT5ForConditionalGeneration
    from flasht5_amd.generation import DecodeState
    m = FAT5ForConditionalGeneration(_small_config(position_encoding_type="RoPE"))
    z = torch.zeros(1, 4, 2, 64)
    state = DecodeState(torch.zeros(1, 3, 64), [z, z], [z, z], [z, z], [z, z], torch.full((1,), 4, dtype=torch.int32), None, 4, steps=4)
    with pytest.raises(ValueError, match="all of them are used"):
        m.decode_step(state, torch.zeros(1, dtype=torch.long))
    state.cache_seqlens.fill_(1000)  # (a caller-written length: the RoPE row is clamped to the capacity on the device)
    assert int(state.position) == 3


@pytest.mark.parametrize("kw", [dict(), dict(attention_type="triton"), dict(position_encoding_type="RoPE", rotary_scale_base=512.0)])
def test_state_dict_loads_unchanged(kw):
    from flasht5_amd import FAT5ForConditionalGeneration
    torch.manual_seed(0)
    a = FAT5ForConditionalGeneration(_small_config(**kw))
    b = FAT5ForConditionalGeneration(_small_config(**kw))
    sd = a.state_dict()
    assert b.load_state_dict(sd, strict=True) is not None
    assert sorted(b.state_dict().keys()) == sorted(sd.keys())
    assert all(torch.equal(b.state_dict()[k], v) for k, v in sd.items())
    assert callable(b.generate) and callable(b.decode_step) and callable(b.init_decode_state)
