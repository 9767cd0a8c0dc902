"""CPU tests of prompt-lookup speculative decoding: the proof that the case list of tests/lookup_ref.py tells every mutant of the
lookup rule from the restatement, the C ABI of fat5_lookup_draft (exports, the struct size against the ctypes mirror, every
rejection before any launch: fake, aligned pointers are enough), the operator's argument checks (shapes and dtypes before
devices), the custom op's schema and fake implementation, `generate`'s host-side rejections before the encoder runs, and the
lookup loop of `generate` simulated on the CPU (permutation chains for the model, the restatement for the kernel, spec_ref's
accept_ref for the verification) against the plain greedy chain."""
import ctypes

import pytest
import torch

import lookup_ref as R
import spec_ref

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


# ------------------------------------------------------------------------------------------------ the restatement and its mutants
def test_restatement_on_hand_worked_rows():
    """N = 2, gamma = 4: the key (6, 7) is in the source at position 2; in the own sequence at position 3, where the continuation
    ends in the pending token; in both, where the source wins"""
    case = next(c for c in R.CASES if c["id"].startswith("where-g4-N2"))
    draft, n = R.reference(case, R.inputs(case))
    assert draft.tolist() == [[8, 9, 10, 11], [8, 5, 6, 7], [40, 41, 42, 43]] and n.tolist() == [4, 4, 4]
    case = next(c for c in R.CASES if c["id"].startswith("ends-g4"))
    draft, n = R.reference(case, R.inputs(case))   # the last source token alone; nothing (a match at Ls - 1); the own match
    assert draft.tolist() == [[99, 7, 7, 7], [7, 7, 7, 7], [50, 51, 6, 7]] and n.tolist() == [1, 0, 4]
    case = next(c for c in R.CASES if c["id"].startswith("oov-g4-N2") and c["V"] == R.V)
    draft, n = R.reference(case, R.inputs(case))
    assert draft.tolist() == [[8, 7, 7, 7], [7, 7, 7, 7], [8, 7, 7, 7]] and n.tolist() == [1, 0, 1]
    case = next(c for c in R.CASES if c["id"].startswith("garbage-g4"))
    draft, n = R.reference(case, R.inputs(case))
    assert draft.tolist() == [[7] * 4] * 3 and n.tolist() == [0, 0, 0]
    case = next(c for c in R.CASES if c["id"].startswith("garbage-src"))
    draft, n = R.reference(case, R.inputs(case))   # Ls clamped to 0, to L_src = 7, to 0 (the own match is left)
    assert draft.tolist() == [[7] * 4, [8, 9, 10, 11], [21, 6, 7, 7]] and n.tolist() == [0, 4, 3]


def test_every_case_builds():
    assert len({c["id"] for c in R.CASES}) == len(R.CASES) and 24 <= len(R.CASES) <= 60
    assert {c["gamma"] for c in R.CASES} >= {1, 4, 15} and {c["N"] for c in R.CASES} >= {1, 2, 3, 16}
    assert {c["L_src"] for c in R.CASES} >= {0, 1, 2, 7, 600, 4099} and {c["ncols"] for c in R.CASES} == {R.NCOLS, R.NCOLS_BIG}
    some = 0
    for case in R.CASES:
        ln = R.inputs(case)
        assert ln["source"].shape == (3, case["L_src"]) and ln["labels"].shape == (3, case["ncols"])
        assert (ln["src_seqlens"] is None) == (not case["seqlens"])
        draft, n = R.reference(case, ln)
        assert draft.shape == (3, case["gamma"]) and n.dtype == torch.int32 and 0 <= int(n.min()) and int(n.max()) <= case["gamma"]
        for b in range(3):   # past the proposed tokens the draft is the pending token
            assert bool((draft[b, int(n[b]):] == ln["tok"][b]).all()), case["id"]
        some += int((n > 0).sum())
    assert some >= len(R.CASES)


def test_the_late_pass_and_the_ragged_tail_are_reached():
    """in the long random cases the planted key wins: a position beyond the first pass of a 256-thread workgroup"""
    case = next(c for c in R.CASES if c["id"].startswith("random-g4-N16-L4099"))
    ln = R.inputs(case)
    draft, n = R.reference(case, ln)
    Ls = int(ln["src_seqlens"][2])
    assert Ls > 2048 and int(n[2]) == 2 and draft[2, :2].tolist() == ln["source"][2, Ls - 2:Ls].tolist()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_cases_tell_every_mutant_from_the_restatement(mutant):
    hit = [c["id"] for c in R.CASES if not R.same(R.reference(c, R.inputs(c)), R.reference(c, R.inputs(c), mutant))]
    assert hit, f"no case tells mutant {mutant!r} from the restatement"


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_exports_and_struct_size(lib):
    from flasht5_amd import _lib
    for name in ("fat5_lookup_draft", "fat5_sizeof_lookup_params"):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.fat5_sizeof_lookup_params() == ctypes.sizeof(_lib.LookupParams) == 112
    assert [f[0] for f in _lib.LookupParams._fields_][:6] == ["B", "L_src", "ncols", "gamma", "max_ngram", "V"]
    assert lib.fat5_version() == 114


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.LookupParams()
    p.B, p.L_src, p.ncols, p.gamma, p.max_ngram, p.V = 3, 600, 40, 4, 2, 1000
    p.source, p.source_stride, p.src_seqlens = BASE + 4096, 600, BASE + 65536
    p.labels, p.labels_stride = BASE + 131072, 40
    p.cache_seqlens, p.tok, p.seen_eos = BASE + 140000, BASE + 141000, BASE + 142001
    p.draft, p.draft_stride, p.n_proposed = BASE + 143000, 4, BASE + 144000
    for key, val in kw.items():
        setattr(p, key, val)
    return p


@pytest.mark.parametrize("bad, msg", [
    (dict(B=-1), "B -1"), (dict(B=65536), "B 65536"), (dict(L_src=-1), "L_src"), (dict(L_src=(1 << 20) + 1, source_stride=1 << 21), "L_src"),
    (dict(ncols=0), "ncols 0"), (dict(ncols=(1 << 20) + 1, labels_stride=1 << 21), "ncols"), (dict(gamma=0), "gamma 0"),
    (dict(gamma=16, draft_stride=16), "gamma 16"), (dict(max_ngram=0), "max_ngram 0"), (dict(max_ngram=17), "max_ngram 17"),
    (dict(V=-1), "V -1"), (dict(source_stride=599), "source_stride"), (dict(labels_stride=39), "labels_stride"),
    (dict(draft_stride=3), "draft_stride"), (dict(source=None), "source"), (dict(source=BASE + 4), "source"),
    (dict(labels=None), "labels"), (dict(labels=BASE + 4), "labels"), (dict(cache_seqlens=None), "cache_seqlens"),
    (dict(cache_seqlens=BASE + 2), "cache_seqlens"), (dict(tok=None), "tok"), (dict(tok=BASE + 4), "tok"), (dict(seen_eos=None), "seen_eos"),
    (dict(draft=None), "draft"), (dict(draft=BASE + 4), "draft"), (dict(src_seqlens=BASE + 2), "src_seqlens"),
    (dict(n_proposed=BASE + 2), "n_proposed"),
])
def test_lookup_draft_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_lookup_draft(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


def test_lookup_draft_null_and_empty(lib):
    assert lib.fat5_lookup_draft(None, None) == -1
    assert "null params" in lib.fat5_last_error().decode()
    assert lib.fat5_lookup_draft(ctypes.byref(_params(B=0)), None) == 0
    assert lib.fat5_lookup_draft(ctypes.byref(_params(B=0, gamma=0)), None) == -1   # (an empty batch is still checked)
    # the optional pointers may be NULL, a source of no columns too, and the widest shapes the header states pass the checks
    assert lib.fat5_lookup_draft(ctypes.byref(_params(B=0, src_seqlens=None, n_proposed=None, L_src=0, source=None, source_stride=0)), None) == 0
    assert lib.fat5_lookup_draft(ctypes.byref(_params(B=0, L_src=1 << 20, source_stride=1 << 20, ncols=1 << 20, labels_stride=1 << 20,
                                                      gamma=15, draft_stride=15, max_ngram=16, V=0)), None) == 0


# ------------------------------------------------------------------------------------------------ the operator
def _call(**kw):
    B = 2
    a = dict(source=torch.zeros(B, 9, dtype=torch.int64), labels=torch.zeros(B, 12, dtype=torch.int64),
             cache_seqlens=torch.zeros(B, dtype=torch.int32), tok=torch.zeros(B, dtype=torch.int64),
             seen_eos=torch.zeros(B, dtype=torch.bool), num_tokens=4)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw, msg", [
    (dict(source=torch.zeros(2, dtype=torch.int64)), "source must be"),
    (dict(source=torch.zeros(2, 9, dtype=torch.int32)), "source must be"),
    (dict(source=torch.zeros(2, 18, dtype=torch.int64)[:, ::2]), "source needs"),
    (dict(labels=torch.zeros(2, 12, dtype=torch.int32)), "labels must be"),
    (dict(labels=torch.zeros(3, 12, dtype=torch.int64)), "labels must be"),
    (dict(labels=torch.zeros(2, 0, dtype=torch.int64)), "labels must be"),
    (dict(labels=torch.zeros(2, 24, dtype=torch.int64)[:, ::2]), "labels needs"),
    (dict(cache_seqlens=torch.zeros(2, dtype=torch.int64)), "cache_seqlens must be"),
    (dict(cache_seqlens=torch.zeros(3, dtype=torch.int32)), "cache_seqlens must be"),
    (dict(src_seqlens=torch.zeros(2, dtype=torch.int64)), "src_seqlens must be"),
    (dict(src_seqlens=torch.zeros(4, dtype=torch.int32)[::2]), "src_seqlens must be"),
    (dict(tok=torch.zeros(2, dtype=torch.int32)), "tok must be"),
    (dict(tok=torch.zeros(2, 1, dtype=torch.int64)), "tok must be"),
    (dict(seen_eos=torch.zeros(2, dtype=torch.uint8)), "seen_eos must be"),
    (dict(out=torch.zeros(2, 3, dtype=torch.int64)), "out must be"),
    (dict(out=torch.zeros(2, 4, dtype=torch.int32)), "out must be"),
    (dict(out=torch.zeros(2, 8, dtype=torch.int64)[:, ::2]), "out needs"),
    (dict(num_tokens=0), "num_tokens"), (dict(num_tokens=16), "num_tokens"), (dict(num_tokens=2.0), "num_tokens"),
    (dict(num_tokens=True), "num_tokens"), (dict(max_ngram=0), "max_ngram"), (dict(max_ngram=17), "max_ngram"),
    (dict(max_ngram=2.0), "max_ngram"), (dict(vocab_size=0), "vocab_size"), (dict(vocab_size=1.5), "vocab_size"),
])
def test_operator_checks_shapes_and_dtypes(kw, msg):
    from flasht5_amd import prompt_lookup_draft
    with pytest.raises(ValueError, match=msg):
        prompt_lookup_draft(**_call(**kw))


def test_operator_checks_shapes_before_devices_and_rejects_cpu_tensors():
    import flasht5_amd
    from flasht5_amd.prompt_lookup import prompt_lookup_draft
    assert flasht5_amd.prompt_lookup_draft is prompt_lookup_draft
    with pytest.raises(ValueError, match="GPU"):           # every shape and dtype is right: the device check is what is left
        prompt_lookup_draft(**_call())
    with pytest.raises(ValueError, match="GPU"):
        prompt_lookup_draft(**_call(out=torch.zeros(2, 4, dtype=torch.int64), src_seqlens=torch.zeros(2, dtype=torch.int32),
                                    vocab_size=100, max_ngram=16, source=torch.zeros(2, 0, dtype=torch.int64)))
    with pytest.raises(ValueError, match="tok must be"):   # a wrong shape on the CPU: the shape is reported, not the device
        prompt_lookup_draft(**_call(tok=torch.zeros(3, dtype=torch.int64)))


def test_custom_op_declares_its_mutation_and_has_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import prompt_lookup  # noqa: F401  (registers the op)
    schema = torch.ops.fat5.lookup_draft.default._schema
    written = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert written == {"out"}
    with FakeTensorMode():
        a = _call()
        out = torch.empty(2, 4, dtype=torch.int64)
        for lens in (None, torch.empty(2, dtype=torch.int32)):
            n = torch.ops.fat5.lookup_draft(a["source"], a["labels"], a["cache_seqlens"], a["tok"], a["seen_eos"], lens, out, 2, 0)
            assert n.shape == (2,) and n.dtype == torch.int32


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
    (dict(prompt_lookup_num_tokens=0), "prompt_lookup_num_tokens"), (dict(prompt_lookup_num_tokens=16), "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=2.0), "prompt_lookup_num_tokens"), (dict(prompt_lookup_num_tokens=True), "prompt_lookup_num_tokens"),
    (dict(max_matching_ngram_size=0), "max_matching_ngram_size"), (dict(max_matching_ngram_size=17), "max_matching_ngram_size"),
    (dict(max_matching_ngram_size=2.0), "max_matching_ngram_size"), (dict(max_matching_ngram_size=None), "max_matching_ngram_size"),
    (dict(decoder_input_ids=torch.tensor([[0, 5], [0, 6]]), decoder_attention_mask=torch.tensor([[1, 1], [1, 0]])), "ragged decoder prompt"),
])
def test_generate_rejects_before_the_encoder(kw, msg, monkeypatch):
    m = _small_model()
    _no_encoder(monkeypatch, m)
    kw = dict(dict(prompt_lookup_num_tokens=4), **kw)
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(2, 4, dtype=torch.long), max_length=8, **kw)


def test_generate_rejects_models_before_the_encoder(monkeypatch):
    m, a = _small_model(), _small_model(num_decoder_layers=1)
    ids = torch.zeros(2, 4, dtype=torch.long)
    _no_encoder(monkeypatch, m, a)
    with pytest.raises(ValueError, match="assistant_model"):
        m.generate(ids, max_length=8, prompt_lookup_num_tokens=4, assistant_model=a)
    fire = _small_model(position_encoding_type="FIRE", attention_type="triton")
    _no_encoder(monkeypatch, fire)
    with pytest.raises(NotImplementedError, match="FIRE"):     # (what the decode path refuses, it refuses here)
        fire.generate(ids, max_length=8, prompt_lookup_num_tokens=4)
    rope = _small_model(position_encoding_type="RoPE")
    _no_encoder(monkeypatch, rope)
    with pytest.raises(ValueError, match="RoPE"):              # ragged rows need per-row rotary positions: B = 1 only
        rope.generate(ids, max_length=8, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match="rotary tables"):     # 1 + 60 + 4 + 1 positions against 64 table rows
        rope.generate(ids[:1], max_length=60, prompt_lookup_num_tokens=4)


class _Reached(Exception):
    pass


def test_generate_accepts_the_lookup_arguments(monkeypatch):
    """`generate(..., prompt_lookup_num_tokens=...)` is a TypeError without the feature; with it valid arguments pass the host
    checks and the call goes on to the encoder; at None the second keyword is not read"""
    m, rope = _small_model(), _small_model(position_encoding_type="RoPE")

    def reached(*a_, **k):
        raise _Reached()
    for x in (m, rope):
        monkeypatch.setattr(x.encoder, "forward", reached)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, prompt_lookup_num_tokens=15, max_matching_ngram_size=16, return_stats=True, graph=True)
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, prompt_lookup_num_tokens=1, max_matching_ngram_size=1, kv_cache_dtype="fp8",
                   decoder_input_ids=torch.tensor([[0, 5], [0, 6]]), attention_mask=torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(_Reached):
        rope.generate(ids[:1], max_length=8, prompt_lookup_num_tokens=4)                 # RoPE at B = 1
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, prompt_lookup_num_tokens=None, max_matching_ngram_size=99)   # (not read without the lookup)


# ------------------------------------------------------------------------------------------------ the loop, simulated
def _setting(seed):
    """one random setting: a permutation with EOS kept out of some chains and inside others, a source that holds parts of the
    rows' greedy chains, padding behind it, a decoder prompt"""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    Vn = ri(6, 40)
    B, P, T, gamma, N, L = ri(1, 4), ri(1, 4), ri(1, 24), ri(1, 15), ri(1, 16), ri(0, 30)
    sigma = torch.randperm(Vn, generator=g)
    prompt = torch.randint(2, Vn, (B, P), generator=g)
    prompt[:, 0] = 0
    ids = torch.randint(0, Vn, (B, L), generator=g)
    lens = torch.full((B,), L, dtype=torch.int32)
    for b in range(B):
        if L and ri(0, 2):   # a stretch of the row's own chain, somewhere in its source
            t, chain = int(prompt[b, P - 1]), []
            for _ in range(ri(1, L)):
                t = int(sigma[t])
                chain.append(t)
            at = ri(0, L - len(chain))
            ids[b, at:at + len(chain)] = torch.tensor(chain)
        if L and ri(0, 1):
            lens[b] = ri(1, L)
    return sigma, ids, (lens if ri(0, 1) else None), prompt, T, gamma, N


def test_the_lookup_loop_equals_the_plain_greedy_chain():
    accepted = drafted = rounds = tokens = 0
    for seed in range(200):
        sigma, ids, lens, prompt, T, gamma, N = _setting(seed)
        want = R.greedy_chain(sigma, prompt, T)
        P = prompt.shape[1]
        for accept in (spec_ref.accept_ref, None):
            labels, ln, st = R.simulate_generate(sigma, ids, lens, prompt, T, gamma, N, accept=accept)
            new = int(ln.max()) - (P - 1)
            assert torch.equal(R.finish(labels[:, :P + new]), want), seed
            assert 0 <= st["accepted"] <= st["drafted"] <= st["rounds"] * gamma * prompt.shape[0] and 1 <= st["rounds"] <= T
        if lens is not None:   # padding is never proposed: what lies behind a row's length does not matter
            junk = ids.clone()
            for b in range(ids.shape[0]):
                junk[b, int(lens[b]):] = int(sigma[prompt[b, -1]])
            again = R.simulate_generate(sigma, junk, lens, prompt, T, gamma, N)
            assert torch.equal(again[0], labels) and again[2] == st, seed
        accepted, drafted, rounds, tokens = accepted + st["accepted"], drafted + st["drafted"], rounds + st["rounds"], tokens + want.shape[1] - P
    assert accepted > 0 and drafted > accepted and rounds < 200 * 24   # (the settings exercise acceptance and rejection alike)
