"""CPU tests of the logits processors: the restatement (tests/logits_proc_ref.py) against HF's four processor classes and against
HF's own `generate(...)` with the same processor arguments on a tiny randomly initialised T5ForConditionalGeneration (nothing is
downloaded), the C ABI of fat5_process_logits and of the extended fat5_beam_params (struct sizes against the ctypes mirrors,
rejections before any launch: fake, aligned pointers are enough), the custom op's fake implementation, and the argument checks of
`generate`, done before the encoder runs."""
import ctypes
import itertools

import pytest
import torch

import logits_proc_ref as ref

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


# ------------------------------------------------------------------------------------------------ the restatement against HF
def _hf_chain(theta, n, m, sup):
    tf = pytest.importorskip("transformers")
    chain = tf.LogitsProcessorList()
    chain.append(tf.RepetitionPenaltyLogitsProcessor(penalty=theta))
    chain.append(tf.NoRepeatNGramLogitsProcessor(n))
    chain.append(tf.MinLengthLogitsProcessor(m, 1, device="cpu"))
    if sup:
        chain.append(tf.SuppressTokensLogitsProcessor(sup, device="cpu"))
    return chain


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("theta", [0.8, 1.0, 1.3])
def test_restatement_equals_hf_processors(n, theta):
    V, L, rows = 11, 12, 6
    g = torch.Generator().manual_seed(100 * n + int(theta * 10))
    for s in range(1, L + 1):
        seqs = torch.randint(0, 4, (rows, L), generator=g)  # (a small alphabet: n-grams and tokens repeat)
        seqs[:, 0] = 0
        logits = torch.randn(rows, V, generator=g) * 3.0   # (positive and negative)
        for m, sup in itertools.product((max(s - 1, 1), s, s + 1), ([], [2, 7])):
            # (HF's MinLength needs a positive int; m = s - 1 and m = s leave EOS alone, m = s + 1 bans it)
            hf = _hf_chain(theta, n, m, sup)(seqs[:, :s], logits.clone())
            mine = ref.process(logits, seqs, torch.full((rows,), s, dtype=torch.int32), repetition_penalty=theta,
                               no_repeat_ngram_size=n, min_length=m, suppress_tokens=sup)
            assert torch.equal(hf, mine), (s, m, sup)


def test_restatement_per_row_lengths_and_guards():
    """rows of different lengths, a length past the buffer and below 0 (clamped), entries outside the vocabulary (no token)"""
    V, L = 9, 8
    g = torch.Generator().manual_seed(7)
    seqs = torch.randint(0, 3, (5, L), generator=g)
    logits = torch.randn(5, V, generator=g)
    lens = torch.tensor([3, 8, 13, -1, 5], dtype=torch.int32)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4)
    y = ref.process(logits, seqs, lens, **kw)
    for r, s in enumerate([3, 8, 8, 0, 5]):
        one = ref.process(logits[r:r + 1], seqs[r:r + 1], torch.tensor([s], dtype=torch.int32), **kw)
        assert torch.equal(y[r:r + 1], one)
    assert torch.equal(y[3, torch.arange(V) != 1], logits[3, torch.arange(V) != 1]) and y[3, 1] == float("-inf")
    bad = seqs.clone()
    bad[0, 1], bad[0, 2] = -1, V
    yb = ref.process(logits[:1], bad[:1], torch.tensor([3], dtype=torch.int32), repetition_penalty=2.0)
    touched = (yb != logits[:1]).nonzero()[:, 1].tolist()
    assert touched == [int(bad[0, 0])]


def _hf_model(seed):
    """test_beam_cpu.py's `_hf_model` recipe, restated"""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.T5Config(vocab_size=24, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4,
                                relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=0.0,
                                decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    torch.manual_seed(seed)
    m = transformers.T5ForConditionalGeneration(cfg).eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(2.0)
    return m


def _hf_generate(m, ids, max_length, proc, k=1, lp=1.0, es=False, R=1):
    from transformers import GenerationConfig
    sup = proc.get("suppress_tokens") or None
    gc = GenerationConfig(num_beams=k, max_new_tokens=max_length, length_penalty=lp, early_stopping=es, num_return_sequences=R,
                          do_sample=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, bos_token_id=None,
                          min_length=proc.get("min_length", 0), no_repeat_ngram_size=proc.get("no_repeat_ngram_size", 0),
                          repetition_penalty=proc.get("repetition_penalty", 1.0), suppress_tokens=sup, forced_eos_token_id=None,
                          forced_bos_token_id=None, return_dict_in_generate=True, output_scores=True, output_logits=True)
    with torch.no_grad():
        out = m.generate(ids, generation_config=gc)
    seqs = out.sequences.clone()
    if k > 1:
        lens = (out.beam_indices >= 0).sum(1)
        for r in range(seqs.shape[0]):
            seqs[r, 1 + int(lens[r]):] = 0  # HF fills past a hypothesis's end with its EOS id; the restatement with 0
        return seqs, out.sequences_scores, out.logits
    return seqs, None, out.logits


def _given_logits(logits):
    """HF's own raw per-step logits, fed back by step: the decisions are then HF's"""
    return lambda prefix: logits[prefix.shape[1] - 1].float()


def _finish(labels):
    """flasht5_amd.generation.finish_labels without the forced last column: 0 after each row's first 1 (HF pads with 0)"""
    out = labels.clone()
    for r in range(out.shape[0]):
        hit = (out[r] == 1).nonzero()
        if len(hit):
            out[r, int(hit[0]) + 1:] = 0
    return out


PROCS = [
    dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=3, min_length=6), dict(repetition_penalty=1.3),
    dict(repetition_penalty=0.8, no_repeat_ngram_size=1), dict(min_length=9), dict(suppress_tokens=[2, 3, 5, 7, 11]),
    dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=5, suppress_tokens=[4, 20]),
]


@pytest.mark.parametrize("proc", PROCS, ids=[str(i) for i in range(len(PROCS))])
def test_greedy_loop_matches_hf(proc):
    for seed in range(4):
        m = _hf_model(seed)
        ids = torch.randint(2, 24, (3, 7), generator=torch.Generator().manual_seed(50 + seed))
        hs, _, hl = _hf_generate(m, ids, 12, proc)
        mine = _finish(ref.greedy(_given_logits(hl), 3, 12, proc))
        assert torch.equal(hs, mine), (seed, hs, mine)


BEAM = [(2, 1.0, False), (4, 2.0, True), (4, 0.0, "never"), (3, -0.5, False)]


@pytest.mark.parametrize("proc", PROCS, ids=[str(i) for i in range(len(PROCS))])
@pytest.mark.parametrize("k, lp, es", BEAM)
def test_beam_loop_matches_hf(proc, k, lp, es):
    for seed, R in itertools.product(range(3), sorted({1, k})):
        m = _hf_model(seed)
        ids = torch.randint(2, 24, (2, 7), generator=torch.Generator().manual_seed(50 + seed))
        hs, hsc, hl = _hf_generate(m, ids, 10, proc, k, lp, es, R)
        rs, rsc = ref.beam_search(_given_logits(hl), 2, k, 10, proc, lp, es, R)
        assert torch.equal(hs, rs), (seed, R, hs, rs)
        assert torch.allclose(hsc, rsc, rtol=1e-5, atol=1e-5), (seed, R, hsc, rsc)


def test_t5_summarization_setting_matches_hf():
    """HF's T5 summarization defaults: num_beams=4, no_repeat_ngram_size=3, min_length > 1, length_penalty=2, early_stopping"""
    proc = dict(no_repeat_ngram_size=3, min_length=8)
    for seed in range(4):
        m = _hf_model(seed)
        ids = torch.randint(2, 24, (2, 9), generator=torch.Generator().manual_seed(80 + seed))
        hs, hsc, hl = _hf_generate(m, ids, 14, proc, 4, 2.0, True, 1)
        rs, rsc = ref.beam_search(_given_logits(hl), 2, 4, 14, proc, 2.0, True, 1)
        assert torch.equal(hs, rs), (seed, hs, rs)
        assert torch.allclose(hsc, rsc, rtol=1e-5, atol=1e-5), (seed, hsc, rsc)
        for row in hs:
            row = row.tolist()
            end = row.index(1) if 1 in row else len(row)
            assert end >= 8 or 1 not in row  # (no EOS before column min_length)


REPEAT_SEED = 0  # (picked on CPU: the unprocessed greedy output of this model repeats a 2-gram)


def test_processor_acts_where_the_plain_greedy_output_repeats():
    m = _hf_model(REPEAT_SEED)
    ids = torch.randint(2, 24, (3, 7), generator=torch.Generator().manual_seed(50 + REPEAT_SEED))
    plain, _, _ = _hf_generate(m, ids, 12, {})

    def repeats(row, n):
        row = row.tolist()
        end = row.index(1) + 1 if 1 in row else len(row)
        grams = [tuple(row[i:i + n]) for i in range(end - n + 1)]
        return len(grams) != len(set(grams))
    assert any(repeats(r, 2) for r in plain), plain
    proc = dict(no_repeat_ngram_size=2)
    hs, _, hl = _hf_generate(m, ids, 12, proc)
    mine = _finish(ref.greedy(_given_logits(hl), 3, 12, proc))
    assert torch.equal(hs, mine)
    assert not any(repeats(r, 2) for r in mine), mine
    assert not torch.equal(plain, hs)


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_struct_sizes_match_library(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_logits_params() == ctypes.sizeof(_lib.LogitsParams)
    assert lib.fat5_sizeof_beam_params() == ctypes.sizeof(_lib.BeamParams)
    for name in ("fat5_process_logits", "fat5_sizeof_logits_params"):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert _lib.BeamParams._fields_[-1][0] == "logits_normalized"  # (appended: the existing fields keep their offsets)
    assert _lib.BeamParams._fields_[-2][0] == "workspace_bytes"


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.LogitsParams()
    p.rows, p.V, p.dtype, p.log_softmax = 4, 1000, _lib.FAT5_BF16, 0
    p.logits, p.row_stride = BASE + 4096, 1000
    p.out, p.out_stride = BASE + 65536, 1000
    p.sequences, p.seq_stride, p.seq_len = BASE + 8192, 33, 33
    p.lengths = BASE + 12288
    p.repetition_penalty, p.no_repeat_ngram_size, p.min_length, p.eos_token_id = 1.2, 3, 5, 1
    p.n_suppress, p.suppress_tokens = 2, BASE + 16384
    for key, val in kw.items():
        setattr(p, key, val)
    return p


@pytest.mark.parametrize("bad, msg", [
    (dict(rows=-1), "rows -1"), (dict(V=1), "V 1"), (dict(V=(1 << 20) + 1), "V"), (dict(dtype=5), "dtype"),
    (dict(row_stride=999), "row_stride"), (dict(out_stride=999), "out_stride"), (dict(seq_len=0), "seq_len"),
    (dict(seq_len=4097, seq_stride=4097), "seq_len"), (dict(seq_stride=32), "seq_stride"),
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.0), "repetition_penalty"),
    (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(min_length=-1), "min_length"),
    (dict(eos_token_id=-1), "eos_token_id"), (dict(eos_token_id=1000), "eos_token_id"),
    (dict(n_suppress=-1), "n_suppress"), (dict(n_suppress=4097), "n_suppress"),
    (dict(logits=None), "logits"), (dict(logits=BASE + 1), "logits"), (dict(out=None), "out"), (dict(out=BASE + 2), "out"),
    (dict(sequences=None), "sequences"), (dict(sequences=BASE + 4), "sequences"), (dict(lengths=None), "lengths"),
    (dict(lengths=BASE + 2), "lengths"), (dict(suppress_tokens=None), "suppress_tokens"),
    (dict(suppress_tokens=BASE + 2), "suppress_tokens"), (dict(out=BASE + 4096), "in place"),
    (dict(dtype=0, out=BASE + 4096, out_stride=1008), "in place"),
])
def test_process_logits_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_process_logits(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


def test_process_logits_empty_is_a_no_op(lib):
    assert lib.fat5_process_logits(ctypes.byref(_params(rows=0)), None) == 0
    assert lib.fat5_process_logits(None, None) == -1


def test_beam_params_reject_still_first(lib):
    """the appended field changes no check: a bad descriptor is rejected as before whatever logits_normalized holds"""
    from flasht5_amd import _lib
    p = _lib.BeamParams()
    p.B, p.k, p.V, p.logits_normalized = 2, 1, 1000, 1
    assert lib.fat5_beam_step(ctypes.byref(p), None) == -1


# ------------------------------------------------------------------------------------------------ fakes and host checks
def test_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import logits_process, beam  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            logits = torch.empty(6, 100, dtype=dt)
            seqs = torch.empty(6, 9, dtype=torch.int64)
            lens = torch.empty(6, dtype=torch.int32)
            y = torch.ops.fat5.process_logits(logits, seqs, lens, 1.2, 3, 5, 1, None, False)
            assert y.shape == (6, 100) and y.dtype == torch.float32
            y = torch.ops.fat5.process_logits(logits, seqs, lens, 1.0, 0, 0, 1, torch.empty(3, dtype=torch.int32), True)
            assert y.shape == (6, 100) and y.dtype == torch.float32
        B, k, cap, L = 2, 4, 40, 41
        st = beam.new_state(B, k, L, cap, "cpu")
        r = torch.ops.fat5.beam_step(torch.empty(B * k, 100), st.running_scores, st.running_seqs, st.cache_row_batch,
                                     st.finished_seqs, st.finished_scores, st.finished_flags, st.finished_lens, st.heuristic,
                                     st.status, st.tokens, torch.empty(B * k, dtype=torch.int32), k, 32, 1.0, 0, True)
        assert r is None


def test_process_logits_is_exported_and_rejects_cpu_tensors():
    import flasht5_amd
    from flasht5_amd import process_logits
    assert flasht5_amd.process_logits is process_logits
    with pytest.raises(ValueError, match="GPU"):
        process_logits(torch.zeros(2, 8), torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, dtype=torch.int32),
                       no_repeat_ngram_size=2)


@pytest.mark.parametrize("kw, msg", [
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.5), "repetition_penalty"),
    (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=2.0), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"), (dict(min_length=-3), "min_length"),
    (dict(min_length=1.5), "min_length"), (dict(suppress_tokens=[3, 1.0]), "suppress_tokens"),
    (dict(suppress_tokens=[True]), "suppress_tokens"), (dict(suppress_tokens=[128]), "suppress_tokens"),
    (dict(suppress_tokens=[-1]), "suppress_tokens"), (dict(suppress_tokens=["a"]), "suppress_tokens"),
])
def test_check_args(kw, msg):
    from flasht5_amd.logits_process import check_args
    with pytest.raises(ValueError, match=msg):
        check_args(vocab_size=128, **kw)
    check_args(1.2, 3, 30, [0, 127], 128)
    check_args()


def _small_model():
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    c = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe")
    return FAT5ForConditionalGeneration(c)


@pytest.mark.parametrize("beams", [dict(), dict(num_beams=4), dict(do_sample=True, seed=1)])
@pytest.mark.parametrize("kw, msg", [
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
    (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(no_repeat_ngram_size=-2), "no_repeat_ngram_size"),
    (dict(min_length=-1), "min_length"), (dict(suppress_tokens=[5, 2.5]), "suppress_tokens"),
    (dict(suppress_tokens=[128]), "suppress_tokens"),
])
def test_generate_rejects_before_the_encoder(kw, msg, beams, monkeypatch):
    m = _small_model()

    def boom(*a, **k):
        raise AssertionError("the encoder ran before the arguments were checked")
    monkeypatch.setattr(m.encoder, "forward", boom)
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=8, **beams, **kw)
    with pytest.raises(ValueError, match="4096"):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=4096, no_repeat_ngram_size=2, **beams)


class _Reached(Exception):
    pass


def test_generate_accepts_the_processor_arguments(monkeypatch):
    """`generate(model, ids, no_repeat_ngram_size=2)` is a TypeError without the feature; with it the valid arguments pass the
    host checks and the call goes on to the encoder"""
    from flasht5_amd.generation import generate
    m = _small_model()

    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(m.encoder, "forward", reached)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(_Reached):
        generate(m, ids, no_repeat_ngram_size=2)
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, num_beams=4, repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=5,
                   suppress_tokens=[100, 101])
