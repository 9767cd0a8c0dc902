"""CPU tests of the FIRE position bias: the C ABI's argument checks (all before any launch: fake, aligned pointers are enough), the
ctypes mirror of fat5_fire_params, the custom ops' fake implementations, the module's parameter names against the reference's, the
eager restatement against the reference fixture (tests/golden/fire.npz, tests/golden/make_golden_fire.py), and the FIRE wiring of
FlashT5Attention / FAT5Config."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fire_eager import fire_eager
from golden_io import GOLDEN

CASES = ("t128_tie", "zero_b1", "neg_c_lm", "w8_h6")


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "fire.npz"))


def _case(z, name):
    g = {k.split("__")[1]: z[k] for k in z.files if k.startswith(name + "__")}
    out = {k: torch.from_numpy(np.array(v, copy=True)) for k, v in g.items() if k != "dbias"}
    out["dbias"] = torch.from_numpy(g["dbias"].view(np.int16).copy()).view(torch.bfloat16).float()
    return out


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.FireParams()
    base = 1 << 20  # (never dereferenced: every call below is rejected before a launch)
    p.M, p.N, p.H, p.W, p.dtype, p.eps = 64, 64, 4, 8, 2, 1e-6
    for i, f in enumerate(("w1", "b1", "w2", "b2", "c", "L_multiplier", "init_L", "bias", "dbias", "dw1", "db1", "dw2", "db2", "dc",
                           "dL_multiplier")):
        setattr(p, f, base + 4096 * i)
    p.bias_stride[0], p.bias_stride[1] = 64 * 64, 64
    for k, v in kw.items():
        if k == "bias_stride":
            p.bias_stride[0], p.bias_stride[1] = v
        else:
            setattr(p, k, v)
    return p


def test_struct_size_matches_library(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_fire_params() == ctypes.sizeof(_lib.FireParams)


@pytest.mark.parametrize("bad, msg", [
    (dict(H=0), "heads"), (dict(H=65), "heads"), (dict(W=0), "width"), (dict(W=129), "width"),
    (dict(dtype=7), "dtype"), (dict(M=-1), "outside"), (dict(N=1 << 31), "outside"),
    (dict(w1=None), "parameter 0"), (dict(c=(1 << 20) + 2), "parameter 4"), (dict(bias=None), "bias"),
    (dict(bias=(1 << 20) + 8), "unaligned"), (dict(bias_stride=(64 * 64, 63)), "multiples"),
    (dict(bias_stride=(64 * 64, 56)), "overlap"), (dict(bias_stride=(64 * 8, 64)), "overlap"), (dict(eps=float("nan")), "eps"),
])
def test_fwd_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_fire_fwd(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


@pytest.mark.parametrize("bad, msg", [
    (dict(dbias=None), "dbias"), (dict(dw2=None), "gradient 2"), (dict(dL_multiplier=(1 << 20) + 1), "gradient 5"),
    (dict(H=100), "heads"),
])
def test_bwd_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_fire_bwd(ctypes.byref(p), ctypes.c_void_p(1 << 24), 1 << 30, None) == -1
    assert msg in lib.fat5_last_error().decode()


def test_bwd_workspace_query_and_check(lib):
    p = _params()
    need = lib.fat5_fire_bwd_workspace_bytes(ctypes.byref(p))
    nout = 4 * 8 + 2 * 8 + 4 + 2
    assert need == (nout * 16 * 4 + 15) // 16 * 16  # 64 x 64 positions = 16 tiles of 256 -> 16 partials per output
    assert lib.fat5_fire_bwd(ctypes.byref(p), ctypes.c_void_p(1 << 24), need - 16, None) == -3
    assert lib.fat5_fire_bwd(ctypes.byref(p), ctypes.c_void_p((1 << 24) + 4), need, None) == -3
    assert lib.fat5_fire_bwd_workspace_bytes(ctypes.byref(_params(M=0))) == 0


def test_zero_sizes_are_a_no_op(lib):
    for kw in (dict(M=0), dict(N=0), dict(M=0, bias_stride=(0, 0))):
        p = _params(**kw)
        assert lib.fat5_fire_fwd(ctypes.byref(p), None) == 0
        assert lib.fat5_fire_bwd(ctypes.byref(p), None, 0, None) == 0


def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import fire  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        H, W = 12, 32
        w1, b1, w2, b2 = torch.empty(W), torch.empty(W), torch.empty(H, W), torch.empty(H)
        s = torch.empty(1)
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            out = torch.ops.fat5.fire_fwd(w1, b1, w2, b2, s, s, s, 100, 37, 1e-6, dt)
            assert out.shape == (H, 100, 37) and out.dtype == dt
            Np = 40  # (the real op's rows are padded to whole 16-byte vectors: the fake has its strides)
            assert out.stride() == (100 * Np, Np, 1)
            assert torch.ops.fat5.fire_fwd(w1, b1, w2, b2, s, s, s, 100, 64, 1e-6, dt).is_contiguous()
            gs = torch.ops.fat5.fire_bwd(torch.empty(H, 100, 37, dtype=dt), w1, b1, w2, b2, s, s, s, 1e-6)
            assert [tuple(g.shape) for g in gs] == [(W,), (W,), (H, W), (H,), (), ()]
            assert all(g.dtype == torch.float32 for g in gs)


def test_reference_state_dict_loads_strict():
    from flasht5_amd.fire import FIRE
    H, W = 12, 32
    sd = {"c": torch.tensor(0.2), "init_L": torch.tensor(128), "L_multiplier": torch.tensor(0.9),
          "mlp.0.weight": torch.randn(W, 1), "mlp.0.bias": torch.randn(W), "mlp.2.weight": torch.randn(H, W),
          "mlp.2.bias": torch.randn(H)}
    m = FIRE(num_heads=H, mlp_width=W, init_c=0.1, init_L=128)
    assert sorted(m.state_dict().keys()) == sorted(sd.keys())
    assert m.init_L.dtype == torch.int64 and not m.init_L.requires_grad  # torch.tensor(128), like the reference
    m.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["c", "L_multiplier", "mlp.0.weight", "mlp.0.bias",
                                                                      "mlp.2.weight", "mlp.2.bias"]


@pytest.mark.parametrize("name", CASES)
def test_eager_restatement_matches_fixture(golden, name):
    from fire_eager import bwd_scale, fwd_scale
    z = _case(golden, name)
    S, H, W, eps = z["meta"].tolist()
    S, H, W = int(S), int(H), int(W)
    leaves = {k: z[k].double().requires_grad_() for k in ("w1", "b1", "w2", "b2", "c", "L_multiplier")}
    bias = fire_eager(leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], leaves["c"], leaves["L_multiplier"], z["init_L"],
                      S, S, eps)
    scale = fwd_scale(z["w1"], z["b1"], z["w2"], z["b2"], z["c"], z["L_multiplier"], z["init_L"], S, S, eps)
    assert ((bias.detach() - z["bias"].double()).abs() <= 1e-5 * scale).all()
    grads = torch.autograd.grad(bias, list(leaves.values()), z["dbias"].double())
    bound = bwd_scale(z["dbias"], z["w1"], z["b1"], z["w2"], z["b2"], z["c"], z["L_multiplier"], z["init_L"], S, S, eps)
    for (k, _), g in zip(leaves.items(), grads):
        ref = z[f"grad_{k}"].double()
        assert ((g - ref).abs() <= 1e-5 * bound[k] + 1e-30).all(), (k, (g - ref).abs().max().item())


def test_fixture_covers_the_corner_cases(golden):
    z = _case(golden, "t128_tie")
    assert z["init_L"].item() == 128.0 and z["meta"][0] == 256  # row 128 ties with T
    z = _case(golden, "zero_b1")
    assert (z["b1"] == 0).any()
    z = _case(golden, "neg_c_lm")
    assert z["c"].item() < 0 and z["L_multiplier"].item() < 0
    z = _case(golden, "w8_h6")
    assert tuple(z["w2"].shape) == (6, 8)


def _cfg(attention_type, **kw):
    base = dict(d_model=128, d_kv=64, num_heads=2, relative_attention_num_buckets=32, relative_attention_max_distance=64,
                is_decoder=False, attention_type=attention_type, position_encoding_type="FIRE", attention_scale=None,
                fire_mlp_width=16)
    base.update(kw)
    return SimpleNamespace(**base)


def test_flasht5_attention_builds_fire_in_block0_only():
    from flasht5_amd import FlashT5Attention
    from flasht5_amd.fire import FIRE
    blk0 = FlashT5Attention(_cfg("triton"), has_positional_encoding=True)
    blk1 = FlashT5Attention(_cfg("triton"), has_positional_encoding=False)
    assert isinstance(blk0.pe_encoding, FIRE) and blk1.pe_encoding is None
    pe = blk0.pe_encoding
    assert tuple(pe.mlp[0].weight.shape) == (16, 1) and tuple(pe.mlp[2].weight.shape) == (2, 16)
    assert pe.c.item() == pytest.approx(0.1) and pe.init_L.item() == 64 and pe.L_multiplier.item() == 1.0
    assert sorted(n for n, _ in blk0.named_parameters()) == sorted(
        ["Wq.weight", "Wk.weight", "Wv.weight", "o.weight", "pe_encoding.c", "pe_encoding.init_L", "pe_encoding.L_multiplier",
         "pe_encoding.mlp.0.weight", "pe_encoding.mlp.0.bias", "pe_encoding.mlp.2.weight", "pe_encoding.mlp.2.bias"])


def test_fire_rejected_with_fat5_rpe():
    from flasht5_amd import FAT5Config, FlashT5Attention
    with pytest.raises(ValueError, match="FIRE needs attention_type='triton'"):
        FlashT5Attention(_cfg("fat5_rpe"), has_positional_encoding=True)
    with pytest.raises(ValueError, match="FIRE"):
        FAT5Config(position_encoding_type="FIRE")
    cfg = FAT5Config(position_encoding_type="FIRE", attention_type="triton")
    assert cfg.fire_mlp_width == 32


def test_fat5_model_with_fire():
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    from flasht5_amd.fire import FIRE
    cfg = FAT5Config(num_layers=2, num_decoder_layers=2, vocab_size=256, d_model=64, d_kv=16, num_heads=4, d_ff=128,
                     position_encoding_type="FIRE", attention_type="triton", fire_mlp_width=8)
    torch.manual_seed(0)
    m = FAT5ForConditionalGeneration(cfg)
    assert m.rpe_tables() == []
    fires = [mod for mod in m.modules() if isinstance(mod, FIRE)]
    assert len(fires) == 2  # block 0 of the encoder and of the decoder
    torch.manual_seed(0)
    fresh = FIRE(4, 8, 0.1, 128)  # reset_parameters leaves FIRE at its own initialisation (as the reference's _init_weights)
    assert fires[0].mlp[0].weight.shape == fresh.mlp[0].weight.shape
    assert fires[0].c.item() == pytest.approx(0.1) and fires[0].L_multiplier.item() == 1.0 and fires[0].init_L.item() == 128


def _meta_params(H=4, W=8):
    """parameters on a non-CPU device (meta): enough to reach the checks, which run before anything is launched"""
    m = lambda *shape: torch.empty(shape, device="meta")  # noqa: E731
    return [m(W, 1), m(W), m(H, W), m(H), m(), m(), m()]


@pytest.mark.parametrize("which", range(7))
def test_fire_bias_rejects_a_parameter_on_another_device(which):
    """a host tensor's pointer must never reach the kernels (the natural call passes init_L = torch.tensor(128.))"""
    from flasht5_amd.fire import _NAMES, fire_bias
    args = _meta_params()
    args[which] = torch.zeros(args[which].shape)  # on the CPU
    # (the devices are compared with w2's: when w2 is the odd one out, w1 is reported)
    with pytest.raises(ValueError, match=f"{_NAMES[which]} is on cpu" if which != 2 else "w1 is on meta"):
        fire_bias(*args, 16, 16)


def test_fire_ops_reject_host_and_non_fp32_parameters():
    """the custom ops themselves (callable directly) check devices, dtypes and contiguity before building the ABI call"""
    from flasht5_amd.fire import _params
    args = _meta_params()
    args[6] = torch.tensor([128.0])
    with pytest.raises(ValueError, match="init_L is on cpu"):
        _params(*args, 16, 16, 1e-6, torch.bfloat16)
    args = _meta_params()
    args[4] = torch.empty((), device="meta", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="fp32 contiguous"):
        _params(*args, 16, 16, 1e-6, torch.bfloat16)
    args = _meta_params()
    args[2] = torch.empty(8, 4, device="meta").t()
    with pytest.raises(ValueError, match="non-contiguous"):
        _params(*args, 16, 16, 1e-6, torch.bfloat16)


def test_ready_rejects_overlapping_gradients():
    """an expanded upstream gradient (stride 0: the backward of bias.sum(-2) or bias.mean(1)) takes the copy path"""
    from flasht5_amd.fire import _ready
    H, M, N = 4, 16, 32
    g = torch.zeros(H, M, N, dtype=torch.bfloat16)
    assert _ready(g)
    assert not _ready(torch.zeros(H, 1, N, dtype=torch.bfloat16).expand(H, M, N))
    assert not _ready(torch.zeros(1, M, N, dtype=torch.bfloat16).expand(H, M, N))
    assert _ready(torch.zeros(1, M, N, dtype=torch.bfloat16).expand(1, M, N))
    assert not _ready(torch.zeros(H, M, 36, dtype=torch.bfloat16)[:, :, :34])  # (row stride 36: not whole 16-byte vectors)
    assert _ready(torch.zeros(H, M, 40, dtype=torch.bfloat16)[:, :, :34])
