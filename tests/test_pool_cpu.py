"""CPU tests of sequence pooling and the encoder-only heads: the C ABI's exports and argument checks (all before any
launch: fake, aligned pointers are enough), the ctypes mirror of fat5_seq_pool_params, the operator's own rejections, the fp64
restatement (tests/pool_ref.py) against hand-written cases, what the "mean" bound accepts and rejects, and the four models'
construction, parameter names and problem-type resolution."""
import ctypes

import pytest
import torch

import pool_ref as R


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.SeqPoolParams()
    base = 1 << 20  # (never dereferenced: every call below is rejected before a launch)
    p.mode, p.dtype, p.nseq, p.L, p.d, p.eos_token_id = _lib.POOL_EOS, _lib.FAT5_BF16, 4, 32, 64, 1
    for i, f in enumerate(("hidden", "seqlens", "input_ids", "pooled", "position", "found", "dpooled", "dhidden")):
        setattr(p, f, base + 4096 * i)
    p.hidden_row_stride, p.hidden_batch_stride, p.ids_batch_stride = 64, 32 * 64, 32
    p.pooled_stride = p.dpooled_stride = p.dhidden_row_stride = 64
    p.dhidden_batch_stride = 32 * 64
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_exports_and_struct_size(lib):
    from flasht5_amd import _lib
    for name in ("fat5_seq_pool_fwd", "fat5_seq_pool_bwd", "fat5_sizeof_seq_pool_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fat5_sizeof_seq_pool_params() == ctypes.sizeof(_lib.SeqPoolParams)


BAD_BOTH = [
    (dict(mode=4), "mode"), (dict(mode=-1), "mode"), (dict(dtype=7), "dtype"), (dict(nseq=-1), "nseq"), (dict(d=-1), "2^22"),
    (dict(d=(1 << 22) + 1), "2^22"), (dict(cu_seqlens=1 << 22), "together"), (dict(L=-1), "L "),
    (dict(nseq=1 << 20, L=1 << 20), "nseq * L"), (dict(seqlens=None, cu_seqlens=1 << 22, total=-1), "total"),
    (dict(seqlens=None, cu_seqlens=1 << 22, total=1 << 31), "total"), (dict(pooled_stride=-64), "stride"),
    (dict(dhidden_row_stride=-1), "stride"), (dict(seqlens=(1 << 20) + 2), "seqlens"), (dict(position=None), "position"),
    (dict(position=(1 << 20) + 1), "position"), (dict(seqlens=None, cu_seqlens=(1 << 22) + 2), "cu_seqlens"),
]


@pytest.mark.parametrize("bad, msg", BAD_BOTH + [
    (dict(input_ids=None), "input_ids"), (dict(input_ids=(1 << 21) + 4), "input_ids"), (dict(hidden=None), "hidden"),
    (dict(hidden=(1 << 20) + 1), "hidden"), (dict(dtype=0, hidden=(1 << 20) + 2), "hidden"), (dict(pooled=None), "pooled"),
    (dict(found=None), "found"),
])
def test_fwd_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_seq_pool_fwd(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()
    assert lib.fat5_seq_pool_fwd(None, None) == -1


@pytest.mark.parametrize("bad, msg", BAD_BOTH + [
    (dict(dpooled=None), "dpooled"), (dict(dhidden=None), "dhidden"), (dict(dhidden=(1 << 21) + 1), "dhidden"),
])
def test_bwd_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_seq_pool_bwd(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()
    assert lib.fat5_seq_pool_bwd(None, None) == -1


def test_zero_sizes_launch_nothing(lib):
    for kw in (dict(nseq=0), dict(d=0)):
        p = _params(**kw)
        assert lib.fat5_seq_pool_fwd(ctypes.byref(p), None) == 0
    for kw in (dict(nseq=0), dict(d=0), dict(L=0)):   # (no row of dhidden to write)
        p = _params(**kw)
        assert lib.fat5_seq_pool_bwd(ctypes.byref(p), None) == 0


def test_operator_rejects_before_device_work():
    from flasht5_amd import sequence_pool
    h3, h2 = torch.zeros(2, 4, 8), torch.zeros(8, 8)
    cu = torch.tensor([0, 3, 8], dtype=torch.int32)
    ids = torch.zeros(2, 4, dtype=torch.int64)
    for args, kw in [
        ((h3, "max"), {}), ((h3.double(), "mean"), {}), ((h3.int(), "mean"), {}), ((h3, "mean"), {}),           # mode, dtypes, a CPU tensor
        (([1.0], "mean"), {}), ((h3, "eos"), {}),                                                               # no tensor; eos without ids
        ((h2, "mean"), dict(cu_seqlens=cu, seqlens=torch.zeros(2, dtype=torch.int32))),                         # both layouts
    ]:
        with pytest.raises(ValueError):
            sequence_pool(*args, **kw)
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import pooling
    with FakeTensorMode():   # (fake CUDA tensors: the checks that follow the device check, and the ops' fake implementations)
        dev = "cuda"
        h3, h2 = torch.empty(2, 4, 8, device=dev, dtype=torch.bfloat16), torch.empty(8, 8, device=dev, dtype=torch.bfloat16)
        cu, ids = torch.empty(3, device=dev, dtype=torch.int32), torch.empty(2, 4, device=dev, dtype=torch.int64)
        for args, kw in [
            ((h3, "mean"), dict(cu_seqlens=cu)), ((h2, "mean"), {}),                                            # layout against rank
            ((h2, "mean"), dict(cu_seqlens=cu.long())), ((h3, "mean"), dict(seqlens=torch.empty(3, device=dev, dtype=torch.int32))),
            ((h3, "eos"), dict(input_ids=ids.int())), ((h3, "eos"), dict(input_ids=ids[:, :3])),                # ids dtype, shape
            ((h3, "eos"), dict(input_ids=torch.empty(2, 4, dtype=torch.int64))),                                # ids on another device
            ((h2, "eos"), dict(cu_seqlens=cu, input_ids=ids)),
        ]:
            with pytest.raises(ValueError):
                sequence_pool(*args, **kw)
        pooled, position, found = torch.ops.fat5.seq_pool_fwd(h3, None, None, ids, pooling.MODES["eos"], 1)
        assert pooled.shape == (2, 8) and pooled.dtype == torch.bfloat16 and position.shape == found.shape == (2,)
        assert position.dtype == found.dtype == torch.int32
        pooled, position, found = torch.ops.fat5.seq_pool_fwd(h2, cu, None, None, pooling.MODES["mean"], 1)
        assert pooled.shape == (2, 8)
        assert torch.ops.fat5.seq_pool_bwd(pooled, position, cu, None, pooling.MODES["mean"], 8, 0).shape == (8, 8)
        assert torch.ops.fat5.seq_pool_bwd(pooled, position, None, None, pooling.MODES["mean"], 2, 4).shape == (2, 4, 8)


# ---------------------------------------------------------------- the restatement, by hand
def test_restatement_padded_by_hand():
    h = torch.arange(24, dtype=torch.float32).reshape(2, 4, 3)     # row (b, j) = 12 b + 3 j + (0, 1, 2)
    ids = torch.tensor([[5, 1, 1, 7], [9, 9, 1, 1]])
    lens = torch.tensor([3, 2], dtype=torch.int32)
    r = R.pool_ref(h, "eos", seqlens=lens, input_ids=ids)
    assert r["position"] == [2, 1] and r["found"] == [1, 0]        # (row 1's EOS lies under the padding)
    assert r["pooled"].tolist() == [[6, 7, 8], [15, 16, 17]]
    r = R.pool_ref(h, "first", seqlens=lens)
    assert r["position"] == [0, 0] and r["pooled"].tolist() == [[0, 1, 2], [12, 13, 14]]
    r = R.pool_ref(h, "last", seqlens=torch.tensor([9, -3], dtype=torch.int32))   # (clamped to 4 and 0)
    assert r["position"] == [3, -1] and r["found"] == [1, 0] and r["pooled"].tolist() == [[9, 10, 11], [0, 0, 0]]
    r = R.pool_ref(h, "mean", seqlens=lens)
    assert r["position"] == [-1, -1] and r["pooled"].tolist() == [[3, 4, 5], [13.5, 14.5, 15.5]]
    assert r["absmean"].tolist() == r["pooled"].tolist()
    assert R.pool_ref(h, "mean")["pooled"].tolist() == [[4.5, 5.5, 6.5], [16.5, 17.5, 18.5]]
    dp = torch.tensor([[1.0, 2, 3], [4, 5, 6]])
    g = R.pool_bwd_ref(dp, h.shape, "eos", [2, 1], seqlens=lens)
    assert g[0, 2].tolist() == [1, 2, 3] and g[1, 1].tolist() == [4, 5, 6] and float(g.abs().sum()) == 21
    g = R.pool_bwd_ref(dp, h.shape, "mean", [-1, -1], seqlens=lens)
    assert g[0, :3].tolist() == [[1 / 3, 2 / 3, 1.0]] * 3 and g[1, :2].tolist() == [[2, 2.5, 3]] * 2
    assert float(g[0, 3].abs().sum() + g[1, 2:].abs().sum()) == 0


def test_restatement_packed_by_hand():
    h = torch.arange(12, dtype=torch.float32).reshape(6, 2)
    cu = torch.tensor([0, 2, 2, 6], dtype=torch.int32)             # lengths 2, 0, 4
    ids = torch.tensor([3, 4, 1, 5, 1, 6])                         # the neighbour's first id is EOS: sequence 0 must not see it
    r = R.pool_ref(h, "eos", cu_seqlens=cu, input_ids=ids)
    assert r["position"] == [1, -1, 2] and r["found"] == [0, 0, 1] and r["lens"] == [2, 0, 4]
    assert r["pooled"].tolist() == [[2, 3], [0, 0], [8, 9]]
    assert R.pool_ref(h, "mean", cu_seqlens=cu)["pooled"].tolist() == [[1, 2], [0, 0], [7, 8]]
    r = R.pool_ref(h, "last", cu_seqlens=torch.tensor([-4, 9, 3], dtype=torch.int32))   # clamped to 0, 6, 3: lengths 6, 0
    assert r["lens"] == [6, 0] and r["position"] == [5, -1]
    g = R.pool_bwd_ref(torch.ones(3, 2), h.shape, "mean", [-1] * 3, cu_seqlens=cu)
    assert g.tolist() == [[0.5, 0.5]] * 2 + [[0.25, 0.25]] * 4


def test_ulp():
    one = torch.tensor([1.0, 1.5, 2.0, 0.0, 2.0 ** -130], dtype=torch.float64)
    assert R.ulp(one, torch.float32).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149]
    assert R.ulp(one, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133]
    assert R.ulp(one, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24]


# ---------------------------------------------------------------- what the "mean" bound accepts and rejects
def _sum_sequential(x):
    acc = torch.zeros(x.shape[1], dtype=torch.float32)
    for row in x:
        acc = acc + row
    return acc


def _sum_pairwise(x):
    if x.shape[0] == 1:
        return x[0].clone()
    half = x.shape[0] // 2
    return _sum_pairwise(x[:half]) + _sum_pairwise(x[half:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_mean_bound_accepts_fp32_sums_and_rejects_wrong_means(dtype):
    g = torch.Generator().manual_seed(3)
    L, d = 96, 40
    lens = [1, 2, 37, 95, 96]
    h = (torch.randn(len(lens), L, d, generator=g) * 3 + 0.5).to(dtype)
    seqlens = torch.tensor(lens, dtype=torch.int32)
    ref = R.pool_ref(h, "mean", seqlens=seqlens)
    bound = R.mean_bound(ref["pooled"], ref["absmean"], lens, dtype)

    def emulate(summed, rows_of, divisor_of):
        out = torch.stack([(summed(rows_of(b).float()) / torch.tensor(float(divisor_of(b)), dtype=torch.float32)).to(dtype)
                           for b in range(len(lens))])
        return (out.double() - ref["pooled"]).abs()

    valid = lambda b: h[b, :lens[b]]  # noqa: E731
    for summed in (_sum_sequential, _sum_pairwise):
        err = emulate(summed, valid, lambda b: lens[b])
        assert bool((err <= bound).all()), (summed.__name__, float((err - bound).max()))
    # one token dropped (rows of at least two tokens), one padded token included (rows shorter than L), the divisor L for len
    rows = [b for b, n in enumerate(lens) if n >= 2]
    err = emulate(_sum_sequential, lambda b: h[b, :max(lens[b] - 1, 1)], lambda b: lens[b])
    assert all(bool((err[b] > bound[b]).any()) for b in rows)
    rows = [b for b, n in enumerate(lens) if n < L]
    err = emulate(_sum_sequential, lambda b: h[b, :min(lens[b] + 1, L)], lambda b: lens[b])
    assert all(bool((err[b] > bound[b]).any()) for b in rows)
    err = emulate(_sum_sequential, valid, lambda b: L)
    assert all(bool((err[b] > bound[b]).any()) for b in rows)


def test_mean_bwd_bound():
    dp = torch.tensor([[1.0, -3.0, 1e-3, 7.0]]).bfloat16()
    for n in (1, 3, 7, 200):
        ref = dp.double() / n
        bound = R.mean_bwd_bound(ref, torch.bfloat16)
        got = (dp.float() / torch.tensor(float(n))).bfloat16()
        assert bool(((got.double() - ref).abs() <= bound).all())
        if n <= 7:   # (the next divisor is further away than bf16's rounding)
            assert not bool((((dp.float() / torch.tensor(float(n + 1))).bfloat16().double() - ref).abs() <= bound).all())


# ---------------------------------------------------------------- the models
def _config(**kw):
    from flasht5_amd import FAT5Config
    return FAT5Config(vocab_size=64, d_model=32, d_kv=16, d_ff=64, num_heads=2, num_layers=2, num_decoder_layers=1, **kw)


def test_state_dict_keys_are_the_references():
    import flasht5_amd as F
    torch.manual_seed(0)
    cfg = _config(num_labels=2)
    # (the encoder's names are those of the seq2seq model, which loads reference checkpoints; the heads' are custom_heads_flash_t5.py's)
    seq2seq = F.FAT5ForConditionalGeneration(cfg).state_dict()
    encoder = {k for k in seq2seq if k.startswith(("shared.", "encoder."))}
    assert "shared.weight" in encoder and "encoder.embed_tokens.weight" in encoder and "encoder.final_layer_norm.weight" in encoder
    heads = {
        F.FAT5EncoderModel: set(),
        F.FAT5ForTokenClassification: {"classifier.weight", "classifier.bias"},
        F.FAT5ForSequenceClassification: {"classification_head.dense.weight", "classification_head.dense.bias",
                                          "classification_head.out_proj.weight", "classification_head.out_proj.bias"},
        F.FAT5ForQuestionAnswering: {"qa_outputs.weight", "qa_outputs.bias"},
    }
    for cls, names in heads.items():
        model = cls(cfg)
        sd = model.state_dict()
        assert set(sd) == encoder | names, (cls.__name__, set(sd) ^ (encoder | names))
        assert model.shared.weight is model.encoder.embed_tokens.weight
        for k in encoder:
            assert sd[k].shape == seq2seq[k].shape, k
        model.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    cfg5 = _config(num_labels=5)
    assert F.FAT5ForTokenClassification(cfg5).classifier.weight.shape == (5, 32)
    head = F.FAT5ForSequenceClassification(cfg5).classification_head
    assert head.dense.weight.shape == (32, 32) and head.out_proj.weight.shape == (5, 32)
    assert float(head.dense.bias.detach().abs().sum()) == 0 and float(head.out_proj.bias.detach().abs().sum()) == 0
    with pytest.raises(ValueError):
        F.FAT5ForQuestionAnswering(cfg5)


def test_config_defaults_and_checks():
    from flasht5_amd import FAT5Config
    c = FAT5Config()
    assert (c.num_labels, c.classifier_dropout, c.eos_token_id) == (2, 0.0, 1)
    for kw in (dict(classifier_dropout=1.0), dict(classifier_dropout=-0.1), dict(num_labels=0)):
        with pytest.raises(ValueError):
            FAT5Config(**kw)


def test_dropout_buffers_stay_out_of_the_state_dict():
    import flasht5_amd as F
    plain = F.FAT5ForSequenceClassification(_config())
    assert not hasattr(plain, "dropout_step")
    for kw in (dict(classifier_dropout=0.1), dict(dropout_rate=0.1)):
        model = F.FAT5ForSequenceClassification(_config(dropout_seed=3, **kw))
        assert model.dropout_step.dtype == torch.int64 and "dropout_step" not in model.state_dict()
    assert not hasattr(F.FAT5EncoderModel(_config(classifier_dropout=0.1)), "dropout_step")   # (the encoder model has no head site)


def test_problem_type_resolution():
    from flasht5_amd import FAT5ForSequenceClassification
    m = FAT5ForSequenceClassification(_config(num_labels=1))
    assert m.resolve_problem_type(torch.zeros(3)) == "regression"
    m = FAT5ForSequenceClassification(_config(num_labels=3))
    assert m.resolve_problem_type(torch.zeros(3, dtype=torch.long)) == "single_label_classification"
    assert m.resolve_problem_type(torch.zeros(3, 3)) == "single_label_classification"   # (fixed by the first labels, as in the reference)
    m = FAT5ForSequenceClassification(_config(num_labels=3))
    assert m.resolve_problem_type(torch.zeros(3, dtype=torch.int32)) == "single_label_classification"
    m = FAT5ForSequenceClassification(_config(num_labels=3))
    assert m.resolve_problem_type(torch.zeros(3, 3)) == "multi_label_classification"
    assert FAT5ForSequenceClassification(_config(num_labels=3), problem_type="regression").resolve_problem_type(torch.zeros(3)) == "regression"
    with pytest.raises(ValueError):
        FAT5ForSequenceClassification(_config(), problem_type="ranking")
    with pytest.raises(RuntimeError):
        m.check()
    m.check(torch.tensor([1, 1, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        m.check(torch.tensor([1, 0, 0], dtype=torch.int32))
