"""CPU tests of speculative greedy decoding: the C ABI of fat5_spec_accept (exports, the struct size against the ctypes mirror,
every rejection before any launch: fake, aligned pointers are enough), the operator's argument checks (shapes and dtypes before
devices), the custom op's schema and fake implementation, `generate`'s host-side rejections before either encoder runs, and the
proof that the case list of tests/spec_ref.py tells every mutant of the accept rule from the restatement."""
import ctypes

import pytest
import torch

import spec_ref as R

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_exports_and_struct_size(lib):
    from flasht5_amd import _lib
    for name in ("fat5_spec_accept", "fat5_spec_accept_workspace_bytes", "fat5_sizeof_spec_params"):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.fat5_sizeof_spec_params() == ctypes.sizeof(_lib.SpecParams) == 160
    assert [f[0] for f in _lib.SpecParams._fields_][:4] == ["B", "M", "V", "dtype"]


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.SpecParams()
    p.B, p.M, p.V, p.dtype = 3, 5, 1000, _lib.FAT5_BF16
    p.logits, p.batch_stride, p.row_stride = BASE + 4096, 5000, 1000
    p.draft, p.draft_stride = BASE + 8192, 4
    p.cache_seqlens, p.draft_seqlens = BASE + 12288, BASE + 12544
    p.labels, p.labels_stride, p.ncols, p.eos_token_id = BASE + 16384, 40, 40, 1
    p.tok, p.seen_eos = BASE + 20480, BASE + 20737
    p.limit, p.limit_scalar = BASE + 24576, 39
    p.n_accepted, p.n_new = BASE + 28672, BASE + 28928
    p.workspace, p.workspace_bytes = BASE + 65536, 1 << 16
    for key, val in kw.items():
        setattr(p, key, val)
    return p


@pytest.mark.parametrize("bad, msg", [
    (dict(B=-1), "B -1"), (dict(B=65536), "B 65536"), (dict(M=1), "M 1"), (dict(M=17), "M 17"), (dict(M=0), "M 0"),
    (dict(V=0), "V 0"), (dict(V=(1 << 20) + 1), "V"), (dict(dtype=5), "dtype"), (dict(row_stride=999), "row_stride"),
    (dict(batch_stride=4999), "batch_stride"), (dict(draft_stride=3), "draft_stride"), (dict(ncols=1), "ncols"),
    (dict(labels_stride=39), "labels_stride"), (dict(eos_token_id=-1), "eos_token_id"),
    (dict(logits=None), "logits"), (dict(logits=BASE + 1), "logits"), (dict(draft=None), "draft"), (dict(draft=BASE + 4), "draft"),
    (dict(cache_seqlens=None), "cache_seqlens"), (dict(cache_seqlens=BASE + 2), "cache_seqlens"),
    (dict(labels=None), "labels"), (dict(labels=BASE + 4), "labels"), (dict(tok=None), "tok"), (dict(tok=BASE + 4), "tok"),
    (dict(seen_eos=None), "seen_eos"), (dict(draft_seqlens=BASE + 2), "draft_seqlens"), (dict(limit=BASE + 2), "limit"),
    (dict(n_accepted=BASE + 2), "n_accepted"), (dict(n_new=BASE + 1), "n_new"),
])
def test_spec_accept_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_spec_accept(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


@pytest.mark.parametrize("bad", [dict(workspace=None), dict(workspace=BASE + 8), dict(workspace_bytes=127)])
def test_spec_accept_workspace(lib, bad):
    p = _params(**bad)
    assert lib.fat5_spec_accept_workspace_bytes(ctypes.byref(p)) == 128   # one 64-bit word per (row, slice of 8192): 120, to 16 bytes
    assert lib.fat5_spec_accept(ctypes.byref(p), None) == -3
    assert "workspace" in lib.fat5_last_error().decode()


def test_spec_accept_workspace_bytes_depend_on_the_shape_only(lib):
    assert lib.fat5_spec_accept_workspace_bytes(None) == 0
    assert lib.fat5_spec_accept_workspace_bytes(ctypes.byref(_params(M=1))) == 0
    for B, M, V, want in ((1, 2, 1, 16), (1, 2, 8192, 16), (1, 2, 8193, 32), (8, 16, 32128, 8 * 16 * 4 * 8), (2, 5, 1 << 20, 2 * 5 * 128 * 8)):
        assert lib.fat5_spec_accept_workspace_bytes(ctypes.byref(_params(B=B, M=M, V=V))) == want


def test_spec_accept_null_and_empty(lib):
    assert lib.fat5_spec_accept(None, None) == -1
    assert lib.fat5_spec_accept(ctypes.byref(_params(B=0, workspace=None, workspace_bytes=0)), None) == 0
    assert lib.fat5_spec_accept(ctypes.byref(_params(B=0, M=1)), None) == -1   # (an empty batch is still checked)
    # the optional pointers may be NULL: the next check (the workspace) is then the one that fires
    p = _params(draft_seqlens=None, limit=None, n_accepted=None, n_new=None, workspace=None)
    assert lib.fat5_spec_accept(ctypes.byref(p), None) == -3


# ------------------------------------------------------------------------------------------------ the operator
def _call(**kw):
    B, g, V = 2, 4, 16
    a = dict(logits=torch.zeros(B, g + 1, V), draft=torch.zeros(B, g, dtype=torch.int64), cache_seqlens=torch.zeros(B, dtype=torch.int32),
             labels=torch.zeros(B, 12, dtype=torch.int64), tok=torch.zeros(B, dtype=torch.int64), seen_eos=torch.zeros(B, dtype=torch.bool),
             limit=11)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(logits=torch.zeros(2, 16)), ValueError, "logits must be"),
    (dict(logits=torch.zeros(2, 5, 16, dtype=torch.float64)), TypeError, "dtype"),
    (dict(logits=torch.zeros(2, 1, 16), draft=torch.zeros(2, 0, dtype=torch.int64)), ValueError, "num_assistant_tokens|gamma"),
    (dict(logits=torch.zeros(2, 17, 16), draft=torch.zeros(2, 16, dtype=torch.int64)), ValueError, "num_assistant_tokens|gamma"),
    (dict(logits=torch.zeros(2, 5, 0)), ValueError, "V 0"),
    (dict(draft=torch.zeros(2, 3, dtype=torch.int64)), ValueError, "draft must be"),
    (dict(draft=torch.zeros(2, 4, dtype=torch.int32)), ValueError, "draft must be"),
    (dict(draft=torch.zeros(2, 8, dtype=torch.int64)[:, ::2]), ValueError, "innermost stride"),
    (dict(cache_seqlens=torch.zeros(2, dtype=torch.int64)), ValueError, "cache_seqlens must be"),
    (dict(cache_seqlens=torch.zeros(3, dtype=torch.int32)), ValueError, "cache_seqlens must be"),
    (dict(draft_seqlens=torch.zeros(2, dtype=torch.int64)), ValueError, "draft_seqlens must be"),
    (dict(draft_seqlens=torch.zeros(4, dtype=torch.int32)[::2]), ValueError, "draft_seqlens must be"),
    (dict(labels=torch.zeros(2, 12, dtype=torch.int32)), ValueError, "labels must be"),
    (dict(labels=torch.zeros(2, 1, dtype=torch.int64)), ValueError, "labels must be"),
    (dict(labels=torch.zeros(3, 12, dtype=torch.int64)), ValueError, "labels must be"),
    (dict(labels=torch.zeros(2, 24, dtype=torch.int64)[:, ::2]), ValueError, "labels needs"),
    (dict(tok=torch.zeros(2, dtype=torch.int32)), ValueError, "tok must be"),
    (dict(tok=torch.zeros(2, 1, dtype=torch.int64)), ValueError, "tok must be"),
    (dict(seen_eos=torch.zeros(2, dtype=torch.uint8)), ValueError, "seen_eos must be"),
    (dict(limit=torch.zeros(2, dtype=torch.int64)), ValueError, "limit must be"),
    (dict(limit=torch.zeros(3, dtype=torch.int32)), ValueError, "limit must be"),
    (dict(limit=3.5), ValueError, "limit must be"),
    (dict(limit=True), ValueError, "limit must be"),
    (dict(eos_token_id=-1), ValueError, "eos_token_id"),
    (dict(eos_token_id=1.0), ValueError, "eos_token_id"),
])
def test_operator_checks_shapes_and_dtypes(kw, exc, msg):
    from flasht5_amd import speculative_accept
    with pytest.raises(exc, match=msg):
        speculative_accept(**_call(**kw))


def test_operator_checks_shapes_before_devices_and_rejects_cpu_tensors():
    import flasht5_amd
    from flasht5_amd import speculative_accept, speculative_round
    assert flasht5_amd.speculative_accept is speculative_accept and flasht5_amd.speculative_round is speculative_round
    with pytest.raises(ValueError, match="GPU"):           # every shape and dtype is right: the device check is what is left
        speculative_accept(**_call())
    with pytest.raises(ValueError, match="draft must be"):  # a wrong shape on the CPU: the shape is reported, not the device
        speculative_accept(**_call(draft=torch.zeros(2, 3, dtype=torch.int64)))


def test_custom_op_declares_its_mutations_and_has_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import speculative  # noqa: F401  (registers the op)
    schema = torch.ops.fat5.spec_accept.default._schema
    written = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert written == {"cache_seqlens", "labels", "tok", "seen_eos", "draft_seqlens"}
    with FakeTensorMode():
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            a = _call(logits=torch.empty(2, 5, 16, dtype=dt))
            na, nn = torch.ops.fat5.spec_accept(a["logits"], a["draft"], a["cache_seqlens"], a["labels"], a["tok"], a["seen_eos"],
                                                None, 11, None, 1)
            assert na.shape == nn.shape == (2,) and na.dtype == nn.dtype == torch.int32
            na, nn = torch.ops.fat5.spec_accept(a["logits"], a["draft"], a["cache_seqlens"], a["labels"], a["tok"], a["seen_eos"],
                                                torch.empty(2, dtype=torch.int32), 0, torch.empty(2, dtype=torch.int32), 1)
            assert na.shape == nn.shape == (2,)


# ------------------------------------------------------------------------------------------------ generate's host checks
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


@pytest.mark.parametrize("kw, msg", [
    (dict(do_sample=True, seed=1), "do_sample"),
    (dict(num_beams=3), "num_beams"),
    (dict(repetition_penalty=1.2), "logits processors"), (dict(no_repeat_ngram_size=2), "logits processors"),
    (dict(min_length=3), "logits processors"), (dict(suppress_tokens=[5]), "logits processors"),
    (dict(num_assistant_tokens=0), "num_assistant_tokens"), (dict(num_assistant_tokens=16), "num_assistant_tokens"),
    (dict(num_assistant_tokens=2.0), "num_assistant_tokens"), (dict(num_assistant_tokens=True), "num_assistant_tokens"),
])
def test_generate_rejects_before_the_encoders(kw, msg, monkeypatch):
    m, a = _small_model(), _small_model(num_decoder_layers=1)
    _no_encoder(monkeypatch, m, a)
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(2, 4, dtype=torch.long), max_length=8, assistant_model=a, **kw)


def test_generate_rejects_models_before_the_encoders(monkeypatch):
    m = _small_model()
    ids = torch.zeros(2, 4, dtype=torch.long)
    other = _small_model(vocab=96)
    _no_encoder(monkeypatch, m, other)
    with pytest.raises(ValueError, match="vocabulary mismatch"):
        m.generate(ids, max_length=8, assistant_model=other)
    with pytest.raises(ValueError, match="FAT5ForConditionalGeneration"):
        m.generate(ids, max_length=8, assistant_model=torch.nn.Linear(2, 2))
    fire = _small_model(position_encoding_type="FIRE", attention_type="triton")
    _no_encoder(monkeypatch, fire)
    with pytest.raises(NotImplementedError, match="FIRE"):     # (what the decode path refuses, it refuses here, for either model)
        m.generate(ids, max_length=8, assistant_model=fire)
    with pytest.raises(NotImplementedError, match="FIRE"):
        fire.generate(ids, max_length=8, assistant_model=m)
    rope = _small_model(position_encoding_type="RoPE")
    _no_encoder(monkeypatch, rope)
    with pytest.raises(ValueError, match="RoPE"):              # ragged rows need per-row rotary positions: B = 1 only
        rope.generate(ids, max_length=8, assistant_model=m)
    with pytest.raises(ValueError, match="RoPE"):
        m.generate(ids, max_length=8, assistant_model=rope)
    with pytest.raises(ValueError, match="rotary tables"):     # 1 + 60 + 4 + 1 positions against 64 table rows
        rope.generate(ids[:1], max_length=60, assistant_model=m, num_assistant_tokens=4)


class _Reached(Exception):
    pass


def test_generate_accepts_the_assistant_arguments(monkeypatch):
    """`generate(..., assistant_model=...)` is a TypeError without the feature; with it valid arguments pass the host checks and
    the call goes on to the model's encoder; without an assistant the new keywords change nothing"""
    m, a, rope = _small_model(), _small_model(num_decoder_layers=1), _small_model(position_encoding_type="RoPE")

    def reached(*a_, **k):
        raise _Reached()
    for x in (m, a, rope):
        monkeypatch.setattr(x.encoder, "forward", reached)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, assistant_model=a, num_assistant_tokens=15, return_stats=True, graph=True)
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, assistant_model=a, decoder_input_ids=torch.tensor([[0, 5], [0, 6]]))
    with pytest.raises(_Reached):
        rope.generate(ids[:1], max_length=8, assistant_model=m, num_assistant_tokens=1)   # RoPE at B = 1
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, assistant_model=None, num_assistant_tokens=99)      # (not read without an assistant)


# ------------------------------------------------------------------------------------------------ the restatement and its mutants
def test_restatement_on_a_hand_worked_round():
    """gamma = 3, V = 6: the target's choices are 4, 2, 5, 3; rows draft [4, 2, 5] (all agree), [4, 3, 5] (one agrees) and a
    frozen row"""
    lg = torch.zeros(3, 4, 6)
    for i, t in enumerate([4, 2, 5, 3]):
        lg[:, i, t] = 1.0
    draft = torch.tensor([[4, 2, 5], [4, 3, 5], [4, 2, 5]])
    lens = torch.tensor([2 + 4, 7 + 4, 5 + 4], dtype=torch.int32)
    labels = torch.full((3, 12), 9)
    seen = torch.tensor([False, False, True])
    r = R.accept_ref(lg, draft, lens, labels, torch.tensor([7, 7, 7]), seen, 11, lens.clone())
    assert r["labels"][0].tolist() == [9, 9, 9, 4, 2, 5, 3, 9, 9, 9, 9, 9]
    assert r["labels"][1].tolist() == [9, 9, 9, 9, 9, 9, 9, 9, 4, 2, 9, 9]
    assert r["labels"][2].tolist() == [9] * 12
    assert r["tok"].tolist() == [3, 2, 7] and r["cache_seqlens"].tolist() == [6, 9, 5] == r["draft_seqlens"].tolist()
    assert r["n_accepted"].tolist() == [3, 1, 0] and r["n_new"].tolist() == [4, 2, 0]
    assert r["seen_eos"].tolist() == [False, False, True]
    r = R.accept_ref(lg, draft, lens, labels, torch.tensor([7, 7, 7]), seen, torch.tensor([4, 9, 11], dtype=torch.int32))
    assert r["n_new"].tolist() == [2, 2, 0] and r["n_accepted"].tolist() == [2, 1, 0] and r["seen_eos"].tolist() == [True, True, True]
    assert r["draft_seqlens"] is None


def test_argmax_rule_of_the_restatement():
    inf, nan = float("inf"), float("nan")
    assert R.argmax_row(torch.tensor([1.0, 3.0, 3.0, 2.0])) == 1 and R.argmax_row(torch.tensor([1.0, 3.0, 3.0]), highest=True) == 2
    assert R.argmax_row(torch.tensor([0.0, inf, nan, inf, nan])) == 2 and R.argmax_row(torch.tensor([0.0, inf, 5.0, inf])) == 1
    assert R.argmax_row(torch.tensor([-inf, -inf])) == 0 and R.argmax_row(torch.tensor([-0.0, 0.0, -1.0])) == 0


def test_every_case_builds_and_the_restatement_writes_inside_labels():
    assert len({c["id"] for c in R.CASES}) == len(R.CASES)
    for case in R.CASES:
        ln = R.inputs(case)
        r = R.reference(case, ln)
        changed = (r["labels"] != ln["labels"]).nonzero()
        assert not len(changed) or int(changed[:, 1].min()) >= 1, case["id"]
        assert int(r["n_new"].max()) <= case["gamma"] + 1 and bool((r["n_accepted"] <= r["n_new"]).all())


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_cases_tell_every_mutant_from_the_restatement(mutant):
    hit = [c["id"] for c in R.CASES if c["V"] <= 512 and not R.same(R.reference(c, R.inputs(c)), R.reference(c, R.inputs(c), mutant))]
    assert hit, f"no case tells mutant {mutant!r} from the restatement"
