"""CPU tests of padding in generation: the masks are validated before an encoder runs (holes, left padding, an empty
row, a wrong shape), an all-ones mask and None reach the encoder with identical state, the fake of fat5::attn_decode_chunk takes the
new argument, chunk_seqlens' shape / dtype / device errors come in that order, the C ABI rejects a misaligned chunk_seqlens before a
launch, and tests/test_chunk_seqlens_gpu.py's wrapped restatement is the restatement itself where every row brings a whole chunk."""
import ctypes

import pytest
import torch

import decode_chunk_fp64 as C
from test_chunk_seqlens_gpu import B_, CASES, M_, inputs, ragged_ref, rows


def _small_config(**kw):
    from flasht5_amd import FAT5Config
    base = dict(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                relative_attention_max_distance=64, max_sequence_length=64)
    base.update(kw)
    return FAT5Config(**base)


class _EncoderRan(Exception):
    def __init__(self, seen):
        self.seen = seen


def _no_encoder(monkeypatch, *models):
    """every encoder raises, and reports what reached `encode`: the ids and the validated padding"""
    from flasht5_amd import generation

    def boom(model, input_ids, pad=None):
        raise _EncoderRan((input_ids, pad))
    monkeypatch.setattr(generation, "encode", boom)
    for m in models:
        m.encoder.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the encoder ran outside generation.encode"))


IDS = torch.arange(2, 38).view(3, 12)


def _mask(lens, L=12, dtype=torch.long):
    return (torch.arange(L).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).to(dtype)


BAD_MASKS = [
    (lambda: _mask([12, 7, 1]).index_put((torch.tensor(1), torch.tensor(3)), torch.tensor(0)), "right-padded"),      # a hole
    (lambda: _mask([12, 7, 1]).flip(1), "right-padded"),                                                               # left padding
    (lambda: _mask([12, 0, 1]), "empty row"),
    (lambda: _mask([12, 7, 1])[:, :11], r"\(B, L\)"),
    (lambda: _mask([12, 7]), r"\(B, L\)"),
    (lambda: _mask([12, 7, 1]).view(-1), r"\(B, L\)"),
    (lambda: _mask([12, 7, 1]).float(), "bool or integer"),
    (lambda: [[1] * 12] * 3, r"\(B, L\)"),
]


@pytest.mark.parametrize("mode", ["greedy", "sample", "beam", "speculative", "init_decode_state"])
def test_mask_validation_comes_before_the_encoder(monkeypatch, mode):
    from flasht5_amd import FAT5ForConditionalGeneration
    m, a = FAT5ForConditionalGeneration(_small_config()), FAT5ForConditionalGeneration(_small_config(num_decoder_layers=1))
    _no_encoder(monkeypatch, m, a)
    kw = dict(greedy={}, sample=dict(do_sample=True, seed=1), beam=dict(num_beams=2), speculative=dict(assistant_model=a))
    if mode == "init_decode_state":
        call = lambda mask: m.init_decode_state(IDS, 4, mask)  # noqa: E731
    else:
        call = lambda mask: m.generate(IDS, mask, max_length=4, **kw[mode])  # noqa: E731
    for make, msg in BAD_MASKS:
        with pytest.raises(ValueError, match=msg):
            call(make())
    for dtype in (torch.long, torch.bool, torch.int32, torch.uint8):
        with pytest.raises(_EncoderRan) as e:   # (a valid mask gets as far as the encoder, validated)
            call(_mask([12, 7, 1], dtype=dtype))
        ids, pad = e.value.seen
        assert pad.lengths == [12, 7, 1] and pad.lengths_dev.dtype == torch.int32 and pad.lengths_dev.tolist() == [12, 7, 1]
        assert torch.equal(pad.mask, _mask([12, 7, 1], dtype=torch.bool)) and ids is IDS


def test_all_ones_and_none_reach_the_encoder_alike(monkeypatch):
    from flasht5_amd import FAT5ForConditionalGeneration
    m = FAT5ForConditionalGeneration(_small_config())
    _no_encoder(monkeypatch, m)
    seen = []
    for mask in (None, _mask([12, 12, 12]), torch.ones(3, 12, dtype=torch.bool)):
        with pytest.raises(_EncoderRan) as e:
            m.generate(IDS, mask, max_length=4)
        seen.append(e.value.seen)
    assert all(ids is IDS and pad is None for ids, pad in seen)
    # ... and the decoder mask: all ones is no mask (a prompt with one is today's path, which is not ragged)
    from flasht5_amd.generation import check_padding
    prompt = torch.tensor([[0, 5, 6, 7]] * 3)
    assert check_padding(IDS, None, prompt, torch.ones(3, 4, dtype=torch.long)) == (None, None)
    enc, dec = check_padding(IDS, _mask([12, 7, 1]), prompt, _mask([1, 3, 4], 4))
    assert enc.lengths == [12, 7, 1] and dec.lengths == [1, 3, 4]
    assert check_padding(IDS, enc, prompt, dec) == (enc, dec)   # (validated masks pass through, unread)


def test_one_host_read(monkeypatch):
    """both masks in one `tolist`: the lengths and the prefix flags travel in one tensor"""
    from flasht5_amd import generation
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (reads.append(t.numel()), real(t))[1])
    generation.check_padding(IDS, _mask([12, 7, 1]), torch.zeros(3, 4, dtype=torch.long), _mask([1, 3, 4], 4))
    assert reads == [2 * (3 + 1)]


def test_decoder_mask_validation_comes_before_the_encoder(monkeypatch):
    from flasht5_amd import FAT5ForConditionalGeneration
    m, a = FAT5ForConditionalGeneration(_small_config()), FAT5ForConditionalGeneration(_small_config())
    r = FAT5ForConditionalGeneration(_small_config(position_encoding_type="RoPE"))
    _no_encoder(monkeypatch, m, a, r)
    prompt = torch.tensor([[0, 1, 1, 1], [0, 5, 6, 127], [0, 7, 8, 9]])   # (the ids under the padding are not looked at: EOS, 127)
    ok = _mask([1, 3, 4], 4)
    with pytest.raises(_EncoderRan):
        m.generate(IDS, max_length=4, decoder_input_ids=prompt, decoder_attention_mask=ok)
    with pytest.raises(ValueError, match="EOS"):
        m.generate(IDS, max_length=4, decoder_input_ids=prompt, decoder_attention_mask=_mask([2, 3, 4], 4))
    clean = torch.tensor([[0, 5, 6, 7]] * 3)   # (no id that the prompt's own checks refuse, wherever the mask uncovers it)
    for bad, msg in ((ok.flip(1), "right-padded"), (_mask([0, 3, 4], 4), "empty row"), (_mask([1, 3, 4], 5), r"\(B, L\)"),
                     (torch.tensor([[1, 0, 0, 0], [1, 0, 1, 0], [1, 1, 1, 1]]), "right-padded")):
        with pytest.raises(ValueError, match=msg):
            m.generate(IDS, max_length=4, decoder_input_ids=clean, decoder_attention_mask=bad)
    with pytest.raises(ValueError, match="needs decoder_input_ids"):
        m.generate(IDS, max_length=4, decoder_attention_mask=ok)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(IDS, max_length=4, decoder_input_ids=prompt, decoder_attention_mask=ok, num_beams=2)
    with pytest.raises(ValueError, match="assistant_model is not supported"):
        m.generate(IDS, max_length=4, decoder_input_ids=prompt, decoder_attention_mask=ok, assistant_model=a)
    with pytest.raises(ValueError, match="RoPE needs B = 1"):
        r.generate(IDS, max_length=4, decoder_input_ids=prompt, decoder_attention_mask=ok)
    with pytest.raises(_EncoderRan):   # (one row has one rotary position)
        r.generate(IDS[:1], max_length=4, decoder_input_ids=prompt[1:2], decoder_attention_mask=ok[1:2])
    with pytest.raises(_EncoderRan):   # (an all-ones decoder mask is no mask: not ragged)
        r.generate(IDS, max_length=4, decoder_input_ids=prompt[:, :1], decoder_attention_mask=ok[:, :1])


def test_finish_labels_per_row():
    from flasht5_amd.generation import finish_labels
    lab = torch.tensor([[0, 5, 6, 7, 0, 0], [0, 9, 1, 4, 4, 4], [0, 3, 3, 3, 3, 3]])
    out = finish_labels(lab, last=torch.tensor([3, 4, 5]))
    assert out.tolist() == [[0, 5, 6, 1, 0, 0], [0, 9, 1, 0, 0, 0], [0, 3, 3, 3, 3, 1]]
    assert finish_labels(lab).tolist() == [[0, 5, 6, 7, 0, 1], [0, 9, 1, 0, 0, 0], [0, 3, 3, 3, 3, 1]]


# ------------------------------------------------------------------------------------------------------------------ the operator
def test_fake_takes_chunk_seqlens():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import decode  # noqa: F401  (registers the op)
    with FakeTensorMode():
        B, M, H, D, cap = 3, 5, 2, 64, 16
        q = torch.empty(B, M, H, D, dtype=torch.bfloat16)
        kc = torch.empty(B, cap, H, D, dtype=torch.bfloat16)
        lens = torch.empty(B, dtype=torch.int32)
        o, lse = torch.ops.fat5.attn_decode_chunk(q, kc, kc, q, q, lens, 0.125, True, None, 0, True, 0, lens)
        assert o.shape == (B, M, H, D) and lse.shape == (B, H, M)
        o, lse = torch.ops.fat5.attn_decode_chunk(q, kc, kc, q, q, lens, 0.125, True, None, 0, False, 0, chunk_seqlens=None)
        assert o.shape == (B, M, H, D) and lse.numel() == 0
        o, _ = torch.ops.fat5.attn_decode_chunk(q, kc, kc, q, q, lens, 0.125, True, None, 0, False, 0)   # (the old call site)
        assert o.shape == (B, M, H, D)
    schema = str(torch.ops.fat5.attn_decode_chunk.default._schema)
    assert schema.rstrip().endswith("Tensor? chunk_seqlens=None) -> Tensor[]"), schema


def test_chunk_seqlens_errors_in_order():
    from flasht5_amd.decode import _check_chunk_seqlens, flash_attn_with_kvcache_chunk
    bf = torch.bfloat16
    q, kc = torch.zeros(2, 3, 4, 64, dtype=bf), torch.zeros(2, 16, 4, 64, dtype=bf)
    call = lambda cs: flash_attn_with_kvcache_chunk(q, kc, kc, q, q, 3, chunk_seqlens=cs)  # noqa: E731
    # the wrapper: the shape first, then the dtype, both before the device check of the tensors (reachable on any host)
    with pytest.raises(ValueError, match="chunk_seqlens must hold 2 lengths"):
        call(torch.zeros(3, dtype=torch.float32))          # (wrong shape AND wrong dtype: the shape is reported)
    with pytest.raises(ValueError, match="chunk_seqlens must hold 2 lengths"):
        call(torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(TypeError, match="chunk_seqlens must be an int32"):
        call(torch.zeros(2, dtype=torch.float32))
    with pytest.raises(TypeError, match="chunk_seqlens must be an int32"):
        call(torch.zeros(2, dtype=torch.bool))
    with pytest.raises(ValueError, match="GPU"):
        call(torch.zeros(2, dtype=torch.int64))
    # the operator's strict form: shape, then int32 exactly, then the device
    gpu = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="must hold 2 lengths"):
        _check_chunk_seqlens(torch.zeros(3, dtype=torch.int64), 2, gpu)
    with pytest.raises(TypeError, match="int32 tensor, got torch.int64"):
        _check_chunk_seqlens(torch.zeros(2, dtype=torch.int64), 2, gpu)      # (wrong dtype AND wrong device: the dtype is reported)
    with pytest.raises(ValueError, match="on cuda:0, got one on cpu"):
        _check_chunk_seqlens(torch.zeros(2, dtype=torch.int32), 2, gpu)
    _check_chunk_seqlens(torch.zeros(2, dtype=torch.int32), 2, torch.device("cpu"))
    _check_chunk_seqlens(None, 2, gpu)


def test_c_abi_rejects_a_misaligned_chunk_seqlens_before_launch():
    from flasht5_amd import _lib
    from test_decode_chunk_cpu import BASE, _params
    lib = _lib.load()
    assert lib.fat5_sizeof_decode_chunk_params() == ctypes.sizeof(_lib.DecodeChunkParams)
    p = _params(chunk_seqlens=BASE + 2)
    assert lib.fat5_attn_decode_chunk(ctypes.byref(p), None) == -1
    assert "chunk_seqlens misaligned" in lib.fat5_last_error().decode()
    # the workspace is a function of B, H, M, D, the capacity and num_splits only: the field does not move it
    a, b = _params(num_splits=0, capacity=1 << 14), _params(num_splits=0, capacity=1 << 14, chunk_seqlens=BASE)
    assert lib.fat5_attn_decode_chunk_workspace_bytes(ctypes.byref(a)) == lib.fat5_attn_decode_chunk_workspace_bytes(ctypes.byref(b)) > 0


def test_decode_chunk_refuses_bad_chunk_seqlens():
    from flasht5_amd import FAT5ForConditionalGeneration
    from flasht5_amd.generation import DecodeState
    m = FAT5ForConditionalGeneration(_small_config())
    z = torch.zeros(2, 8, 2, 64)
    state = DecodeState(torch.zeros(2, 3, 64), [z, z], [z, z], [z, z], [z, z], torch.zeros(2, dtype=torch.int32), None, 8)
    with pytest.raises(ValueError, match=r"\(2,\) int32"):
        m.decode_chunk(state, torch.zeros(2, 3, dtype=torch.long), chunk_seqlens=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\(2,\) int32"):
        m.decode_chunk(state, torch.zeros(2, 3, dtype=torch.long), chunk_seqlens=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="M > 1"):
        m.decode_chunk(state, torch.zeros(2, 1, dtype=torch.long), chunk_seqlens=torch.zeros(2, dtype=torch.int32))
    assert state.steps == 0


# ------------------------------------------------------------------------------------- what test_chunk_seqlens_gpu.py rests on
def test_the_wrapped_restatement_is_the_restatement_for_whole_chunks():
    case = dict(next(c for c in CASES if c["kind"] == "base" and c["append"] and c["causal"] and c["R"]), mlens=[M_] * B_)
    ln = inputs(case)
    a = ragged_ref(case, ln)
    b = C.chunk_ref(ln["q"], ln["kc"], ln["vc"], ln["kn"], ln["vn"], case["lens"], 0.125, True, ln["rpe"], case["R"])
    for name in ("o", "lse", "absv", "smag", "bmag", "srange", "kc", "vc"):
        assert torch.equal(a[name], b[name]), name
    assert a["nvis"] == b["nvis"] and a["kend"] == b["kend"]


def test_the_case_table_is_what_the_issue_asks_for():
    base = [c for c in CASES if c["kind"] == "base"]
    assert len(base) == 32 and len({c["id"] for c in CASES}) == len(CASES)
    for c in base:
        assert (c["mlens"], c["lens"]) == ([5, 2, 0], [0, 3, 11]) and rows(c) == [5, 2, 0]
    assert {(c["D"], c["dtype"], c["causal"], c["R"], c["append"]) for c in base} == {
        (D, t, ca, R, ap) for D in (64, 128) for t in (torch.bfloat16, torch.float16) for ca in (True, False) for R in (4, 0)
        for ap in (True, False)}
    assert any(c["splits"] > 1 for c in CASES)
    over = [c for c in CASES if c["kind"] == "overflow"]
    assert over and all(any(n + m > 16 for n, m in zip(c["lens"], rows(c))) for c in over)


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] != "base" or c["dtype"] == torch.bfloat16], ids=lambda c: c["id"])
def test_the_bound_holds_for_the_rounded_truth_and_sees_dropped_row_mistakes(case):
    """correct arithmetic satisfies the bound; treating a row the element does not bring as a real row (the defect the wrapper is
    there to catch) does not"""
    ln = inputs(case)
    ref = ragged_ref(case, ln)
    bo, bl = C.chunk_bound(ref, case["dtype"], case["D"], case["splits"])
    assert C.within(ref["o"].to(case["dtype"]), ref["lse"].float(), ref, bo, bl)
    if rows(case) != [M_] * B_:
        full = dict(case, mlens=[M_] * B_)
        wrong = ragged_ref(full, ln)
        if not (torch.equal(wrong["o"], ref["o"]) and torch.equal(wrong["lse"], ref["lse"])):
            assert not C.within(wrong["o"].to(case["dtype"]), wrong["lse"].float(), ref, bo, bl)
