"""CPU tests of padded / packed training: the planner's exports and layout mirror, every rejection of the C ABI and
of the Python entry points that happens on the host before a launch, and the unchanged positional signatures."""
import ctypes
import inspect

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_exports_and_layout(lib):
    import flasht5_amd
    from flasht5_amd import _lib
    for name in ("fat5_pack_plan", "fat5_sizeof_pack_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_pack_params() == ctypes.sizeof(_lib.PackParams)
    assert lib.fat5_version() == 114
    assert flasht5_amd.pack_plan is flasht5_amd.packing.pack_plan


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.PackParams()
    p.B, p.L, p.seg_cap = 4, 64, 2
    p.seg, p.cu_seqlens, p.index, p.seg_count, p.status = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # fake, aligned, never followed
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(seg=0), b"seg"), (dict(cu_seqlens=0), b"cu_seqlens"), (dict(index=0), b"index"), (dict(seg_count=0), b"seg_count"),
    (dict(status=0), b"status"),
    (dict(seg=0x1004), b"seg"), (dict(cu_seqlens=0x2002), b"cu_seqlens"), (dict(index=0x3004), b"index"),
    (dict(seg_count=0x4001), b"seg_count"), (dict(status=0x5003), b"status"),
    (dict(B=0), b"B 0"), (dict(B=-3), b"B -3"), (dict(L=0), b"L 0"), (dict(L=-1), b"L -1"),
    (dict(B=1 << 16, L=1 << 15), b"2^31"), (dict(B=(1 << 31) - 1, L=(1 << 31) - 1), b"2^31"),
    (dict(seg_cap=0), b"seg_cap 0"), (dict(seg_cap=257), b"seg_cap 257"), (dict(seg_cap=-1), b"seg_cap -1"),
])
def test_c_abi_rejects_before_any_launch(lib, kw, word):
    p = _params(**kw)
    assert lib.fat5_pack_plan(ctypes.byref(p), None) == -1
    assert word in lib.fat5_last_error(), lib.fat5_last_error()


def test_c_abi_rejects_null_params(lib):
    assert lib.fat5_pack_plan(None, None) == -1 and b"null params" in lib.fat5_last_error()


def _model(**kw):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    cfg = FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=1, num_decoder_layers=1, **kw)
    return FAT5ForConditionalGeneration(cfg)


IDS = torch.zeros(2, 8, dtype=torch.long)
LABELS = torch.zeros(2, 4, dtype=torch.long)


@pytest.mark.parametrize("kw, word", [
    (dict(attention_mask=torch.ones(2, 8, dtype=torch.bool), segment_ids=torch.ones(2, 8, dtype=torch.int32),
          decoder_segment_ids=torch.ones(2, 4, dtype=torch.int32)), "encoder side"),
    (dict(decoder_attention_mask=torch.ones(2, 4, dtype=torch.bool), decoder_segment_ids=torch.ones(2, 4, dtype=torch.int32)),
     "decoder side"),
    (dict(segment_ids=torch.ones(2, 8, dtype=torch.int32)), "needs decoder_segment_ids"),
    (dict(attention_mask=torch.ones(2, 7, dtype=torch.bool)), r"attention_mask must be a \(B, L\)"),
    (dict(attention_mask=torch.ones(8, dtype=torch.bool)), r"attention_mask must be a \(B, L\)"),
    (dict(decoder_attention_mask=torch.ones(2, 8, dtype=torch.bool)), r"decoder_attention_mask must be a \(B, L\)"),
    (dict(attention_mask=torch.ones(2, 8)), "bool or integer"),
    (dict(segment_ids=torch.ones(2, 8), decoder_segment_ids=torch.ones(2, 4, dtype=torch.int32)), "integer"),
    (dict(segment_ids=torch.ones(2, 8, dtype=torch.bool), decoder_segment_ids=torch.ones(2, 4, dtype=torch.int32)), "integer"),
])
def test_forward_rejects_on_the_host(kw, word):
    from flasht5_amd import train_step
    model = _model()
    with pytest.raises(ValueError, match=word):
        model(IDS, LABELS, **kw)
    with pytest.raises(ValueError, match=word):
        train_step(model, IDS, LABELS, **kw)


@pytest.mark.parametrize("cfg", [
    dict(attention_type="triton", position_encoding_type="t5"),
    dict(attention_type="triton", position_encoding_type="FIRE"),
])
def test_dense_bias_models_refuse_masks(cfg):
    model = _model(**cfg)
    with pytest.raises(NotImplementedError, match="dense"):
        model(IDS, LABELS, attention_mask=torch.ones(2, 8, dtype=torch.bool))


def test_randomized_positions_refuse_masks():
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    for pe in ("t5", "RoPE"):
        cfg = FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2, num_layers=1, num_decoder_layers=1,
                         position_encoding_type=pe)
        cfg.use_randomized_position_encoding = True
        with pytest.raises(NotImplementedError, match="randomized"):
            FAT5ForConditionalGeneration(cfg)(IDS, LABELS, attention_mask=torch.ones(2, 8, dtype=torch.bool))


def test_attention_layer_packed_argument_checks():
    from flasht5_amd import FAT5Config, FlashT5Attention
    cfg = FAT5Config(vocab_size=512, d_model=128, d_kv=64, d_ff=256, num_heads=2)
    att = FlashT5Attention(cfg, has_positional_encoding=True)
    cu = torch.tensor([0, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match="max_seqlen"):
        att(torch.zeros(1, 3, 128), cu_seqlens=cu)
    with pytest.raises(ValueError, match=r"\(1, total, d_model\)"):
        att(torch.zeros(2, 3, 128), cu_seqlens=cu, max_seqlen=3)
    with pytest.raises(ValueError, match="kv_cu_seqlens"):
        att(torch.zeros(1, 3, 128), key_value_states=torch.zeros(1, 5, 128), cu_seqlens=cu, max_seqlen=3)
    for fn in (att.forward, att.forward_fused):
        sig = inspect.signature(fn)
        for name in ("cu_seqlens", "max_seqlen", "kv_cu_seqlens", "kv_max_seqlen"):
            assert sig.parameters[name].default is None


def test_pack_plan_rejects_shape_and_dtype_on_the_host():
    from flasht5_amd import pack_plan, plan_pair
    with pytest.raises(ValueError, match=r"\(B, L\)"):
        pack_plan(torch.ones(8, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or integer"):
        pack_plan(torch.ones(2, 8))
    with pytest.raises(ValueError, match=r"\(B, L\)"):
        pack_plan([[1, 1, 0]])
    with pytest.raises(ValueError, match="bool or integer"):
        plan_pair(torch.ones(2, 8, dtype=torch.bool), torch.ones(2, 4, dtype=torch.float16))


def test_old_positional_calls_still_bind():
    from flasht5_amd import FAT5ForConditionalGeneration, train_step, GraphedTrainStep
    new = ("attention_mask", "decoder_attention_mask", "segment_ids", "decoder_segment_ids")
    sig = inspect.signature(FAT5ForConditionalGeneration.forward)
    assert list(sig.parameters)[:3] == ["self", "input_ids", "labels"] and list(sig.parameters)[3:] == list(new)
    sig.bind(None, IDS, LABELS)
    ts = inspect.signature(train_step)
    assert list(ts.parameters)[:6] == ["model", "input_ids", "labels", "optimizer", "group", "max_grad_norm"]
    ts.bind(None, IDS, LABELS, None, None, 1.0)
    for s in (sig, ts):
        for name in new:
            prm = s.parameters[name]
            assert prm.default is None and prm.kind in (prm.POSITIONAL_OR_KEYWORD, prm.KEYWORD_ONLY)
    assert list(inspect.signature(GraphedTrainStep.__call__).parameters) == ["self", "input_ids", "labels"]


def test_train_step_without_masks_calls_the_model_as_before():
    """a model that takes (input_ids, labels) only -- anything with the old forward -- still trains through train_step"""
    from flasht5_amd import train_step

    class Old(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))

        def forward(self, input_ids, labels):
            return self.w * (input_ids.float().mean() + labels.float().mean() + 1)

    m = Old()
    assert float(train_step(m, IDS, LABELS)) == 1.0 and float(m.w.grad) == 1.0
