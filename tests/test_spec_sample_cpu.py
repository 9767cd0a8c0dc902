"""CPU tests of speculative sampling: the proof that the cases of tests/spec_sample_ref.py tell every mutant of the rule from the
restatement, a 200 000-draw Monte Carlo of the restatement (the first emitted token follows P, the acceptance rate is
sum min(P, Q), and the mutant that redraws from P_n fails), the C ABI of fat5_spec_accept_sampled (exports, the struct size
against the ctypes mirror, every rejection before any launch: fake, aligned pointers are enough), the operator's argument
checks and fake implementation, and `generate`'s host-side checks with do_sample=True."""
import ctypes

import numpy as np
import pytest
import torch

import spec_sample_ref as R

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


# ------------------------------------------------------------------------------------------------ the restatement and its mutants
def _calls():
    """(id, kwargs of accept_sampled_ref) over the hand-made calls and the small grid cases, Philox and hook, both drafters"""
    for name, kw in R.hand_cases():
        yield name, kw
    for case in R.SMALL_CASES:
        if case["dtype"] != torch.float32 and case["gamma"] != 4:
            continue
        ln = R.inputs(case, near=True)
        base = {k: ln[k] for k in ("logits", "draft", "cache_seqlens", "labels", "tok", "seen_eos", "limit", "draft_seqlens")}
        for T, k, p in R.GRID[:4]:
            for with_q in (True, False):
                for hook in (False, True):
                    yield (f"{case['id']}-{T}-{k}-{p}-{with_q}-{hook}",
                           dict(base, sampling=(T, k, p, R.SEED, R.OFFSET), draft_logits=ln["draft_logits"] if with_q else None,
                                uniforms=ln["uniforms"] if hook else None))


@pytest.fixture(scope="module")
def truth():
    return [(name, kw, R.accept_sampled_ref(**kw)) for name, kw in _calls()]


def test_the_restatement_on_the_hand_made_calls(truth):
    by = {name: out for name, _, out in truth}
    assert by["r0-fallback"]["n"].tolist() == [0, 0]                      # u1 = 1 rejects even P = Q; the token is a draw from P_0
    assert by["q-zero"]["n"].tolist() == [3, 3]                           # Q = 0 < P: accepted whatever u1 < 1
    assert by["draft-oob"]["n"].tolist() == [1, 0]                        # ids V and -1 end the accepted prefix
    assert (by["draft-oob"]["labels"] >= 0).all() and (by["draft-oob"]["labels"] < 100).all()
    ns = [int(n) for name, _, out in truth if name.startswith("philox") for n in out["n"]]
    assert min(ns) == 0 and max(ns) > 0                                   # the Philox calls both accept and reject


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_cases_tell_every_mutant_from_the_restatement(mutant, truth):
    differs = [name for name, kw, out in truth if not R.same(out, R.accept_sampled_ref(**kw, mutant=mutant))]
    assert differs, f"no case distinguishes the mutant {mutant}"


# ------------------------------------------------------------------------------------------------ Monte Carlo of the rule
MC_N, MC_V = 200_000, 12


def _bound(dof):
    """the 0.999 chi-square quantile by the Wilson-Hilferty approximation (as tests/test_sampling_gpu.py computes it)"""
    return dof * (1 - 2 / (9 * dof) + 3.09 * (2 / (9 * dof)) ** 0.5) ** 3


def _first_tokens(P, Q, rng, mutant=None):
    """MC_N independent rounds of the restated rule, vectorised: d ~ Q by inverse CDF with a uniform of its own (the drafter's
    stream), the acceptance test with u1, the residual draw with u2.  -> (first emitted tokens, accepted mask)"""
    ud, u1, u2 = (np.floor(rng.random(MC_N) * 2 ** 24) * 2.0 ** -24 for _ in range(3))   # (24-bit uniforms, as the kernel's)
    d = np.minimum(np.searchsorted(np.cumsum(Q["p"]), ud * Q["p"].sum(), side="right"), MC_V - 1)
    acc = u1 * (Q["p"][d] if Q["r"] is not None else 1.0) < P["p"][d]      # (verified as one-hot: Q(d) = 1)
    if mutant == "residual_from_p":
        w = np.trunc(P["p"] * float(R.ONE)).astype(np.int64)
        pre = np.cumsum(w)
        tok = np.searchsorted(pre, np.minimum(np.floor(u2 * pre[-1]), pre[-1] - 1), side="right")
        return np.where(acc, d, tok), acc
    tok = np.empty(MC_N, dtype=np.int64)
    if Q["r"] is None:   # one-hot drafts: Q depends on the draft
        for v in np.unique(d):
            tok[d == v] = _residual_tokens(P, R.one_hot(MC_V, int(v)), u2[d == v])
    else:
        tok[:] = _residual_tokens(P, Q, u2)
    return np.where(acc, d, tok), acc


def _residual_tokens(P, Q, u2):
    r = R.residual(P, Q)
    Rs = int(r.sum())
    if Rs == 0:
        r = np.trunc(P["p"] * float(R.ONE)).astype(np.int64)
        Rs = int(r.sum())
    return np.searchsorted(np.cumsum(r), np.minimum(np.floor(u2 * Rs), Rs - 1), side="right")


def _mc_rows():
    g = torch.Generator().manual_seed(2024)
    p_row = torch.randn(MC_V, generator=g) * 1.5
    rows = dict(same=p_row.clone(), near=p_row + 0.4 * torch.randn(MC_V, generator=g), far=torch.randn(MC_V, generator=g) * 1.5)
    return p_row, rows


def _chi2(tok, P):
    prob = P["p"]
    cnt = np.bincount(tok, minlength=MC_V)
    assert cnt[prob == 0].sum() == 0      # no token outside P's kept set ever appears
    big = prob * MC_N >= 5
    chi2 = float(((cnt[big] - prob[big] * MC_N) ** 2 / (prob[big] * MC_N)).sum())
    return chi2, int(big.sum()) - 1


@pytest.mark.parametrize("which", ["same", "near", "far", "onehot"])
def test_monte_carlo_the_first_token_follows_p(which):
    p_row, rows = _mc_rows()
    P = R.dist(p_row, 1.0, 9, 0.95)
    rng = np.random.default_rng(12345)
    if which == "onehot":   # drafts from a far model, verified without its logits
        drafts_from = R.dist(rows["far"], 1.0, 9, 0.95)
        Q = dict(p=drafts_from["p"], r=None, margin=np.inf)
        a = float((drafts_from["p"] * P["p"]).sum())      # sum_d q(d) * min(P(d), 1)
    else:
        Q = R.dist(rows[which], 1.0, 9, 0.95)
        a = float(np.minimum(P["p"], Q["p"]).sum())
    tok, acc = _first_tokens(P, Q, rng)
    chi2, dof = _chi2(tok, P)
    print(f"[spec-sample] monte carlo {which}: chi2 {chi2:.2f} (dof {dof}, bound {_bound(dof):.2f}), acceptance {acc.mean():.4f} "
          f"against {a:.4f}")
    assert chi2 < _bound(dof), (chi2, _bound(dof), dof)
    assert abs(acc.mean() - a) <= 5 * (a * (1 - a) / MC_N) ** 0.5, (acc.mean(), a)


def test_monte_carlo_the_mutant_that_redraws_from_p_fails_the_law():
    p_row, rows = _mc_rows()
    P, Q = R.dist(p_row, 1.0, 9, 0.95), R.dist(rows["far"], 1.0, 9, 0.95)
    tok, _ = _first_tokens(P, Q, np.random.default_rng(12345), mutant="residual_from_p")
    prob = P["p"]
    cnt = np.bincount(tok, minlength=MC_V)
    big = prob * MC_N >= 5
    chi2 = float(((cnt[big] - prob[big] * MC_N) ** 2 / (prob[big] * MC_N)).sum())
    assert chi2 > _bound(int(big.sum()) - 1), chi2


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_exports_and_struct_size(lib):
    from flasht5_amd import _lib
    for name in ("fat5_spec_accept_sampled", "fat5_spec_accept_sampled_workspace_bytes", "fat5_sizeof_spec_sample_params"):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.fat5_sizeof_spec_sample_params() == ctypes.sizeof(_lib.SpecSampleParams) == 240
    assert lib.fat5_sizeof_spec_params() == ctypes.sizeof(_lib.SpecParams) == 160      # (the greedy struct is untouched)
    assert _lib.SpecSampleParams._fields_[0] == ("spec", _lib.SpecParams)


def _params(**kw):
    from flasht5_amd import _lib
    q = _lib.SpecSampleParams()
    p = q.spec
    p.B, p.M, p.V, p.dtype = 3, 5, 1000, _lib.FAT5_BF16
    p.logits, p.batch_stride, p.row_stride = BASE + 4096, 5000, 1000
    p.draft, p.draft_stride = BASE + 8192, 4
    p.cache_seqlens, p.draft_seqlens = BASE + 12288, BASE + 12544
    p.labels, p.labels_stride, p.ncols, p.eos_token_id = BASE + 16384, 40, 40, 1
    p.tok, p.seen_eos = BASE + 20480, BASE + 20737
    p.limit, p.limit_scalar = BASE + 24576, 39
    p.n_accepted, p.n_new = BASE + 28672, BASE + 28928
    p.workspace, p.workspace_bytes = BASE + 65536, 1 << 16
    q.draft_logits, q.draft_batch_stride, q.draft_row_stride = BASE + 32768, 4000, 1000
    q.temperature, q.top_p, q.top_k = 0.7, 0.9, 50
    q.seed, q.offset = 1234, 0
    q.uniforms, q.sampled, q.aux = BASE + 36864, BASE + 40960, BASE + 45056
    for key, val in kw.items():
        setattr(q if hasattr(type(q), key) and key != "spec" else p, key, val)
    return q


@pytest.mark.parametrize("bad, msg", [
    # everything fat5_spec_accept rejects
    (dict(B=-1), "B -1"), (dict(B=65536), "B 65536"), (dict(M=1), "M 1"), (dict(M=17), "M 17"), (dict(M=0), "M 0"),
    (dict(V=0), "V 0"), (dict(V=(1 << 20) + 1), "V"), (dict(dtype=5), "dtype"), (dict(row_stride=999), "row_stride"),
    (dict(batch_stride=4999), "batch_stride"), (dict(draft_stride=3), "draft_stride"), (dict(ncols=1), "ncols"),
    (dict(labels_stride=39), "labels_stride"), (dict(eos_token_id=-1), "eos_token_id"),
    (dict(logits=None), "logits"), (dict(logits=BASE + 1), "logits"), (dict(draft=None), "draft"), (dict(draft=BASE + 4), "draft"),
    (dict(cache_seqlens=None), "cache_seqlens"), (dict(cache_seqlens=BASE + 2), "cache_seqlens"),
    (dict(labels=None), "labels"), (dict(labels=BASE + 4), "labels"), (dict(tok=None), "tok"), (dict(tok=BASE + 4), "tok"),
    (dict(seen_eos=None), "seen_eos"), (dict(draft_seqlens=BASE + 2), "draft_seqlens"), (dict(limit=BASE + 2), "limit"),
    (dict(n_accepted=BASE + 2), "n_accepted"), (dict(n_new=BASE + 1), "n_new"),
    # what fat5_sample_logits rejects for T, k and p
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(top_k=-1), "top_k"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"),
    (dict(top_p=float("nan")), "top_p"),
    # the drafter's logits, and the optional arrays
    (dict(draft_logits=BASE + 32769), "draft_logits"), (dict(draft_row_stride=999), "draft_row_stride"),
    (dict(draft_batch_stride=3999), "draft_batch_stride"),
    (dict(uniforms=BASE + 2), "uniforms"), (dict(sampled=BASE + 4), "sampled"), (dict(aux=BASE + 2), "aux"),
])
def test_spec_accept_sampled_rejects_before_launch(lib, bad, msg):
    q = _params(**bad)
    assert lib.fat5_spec_accept_sampled(ctypes.byref(q), None) == -1
    err = lib.fat5_last_error().decode()
    assert msg in err and "spec_accept_sampled" in err


@pytest.mark.parametrize("bad", [dict(workspace=None), dict(workspace=BASE + 8), dict(workspace_bytes=655)])
def test_spec_accept_sampled_workspace(lib, bad):
    q = _params(**bad)
    assert lib.fat5_spec_accept_sampled_workspace_bytes(ctypes.byref(q)) == 656   # three words per logits row: (15 + 12) * 24 = 648, to 16 bytes
    assert lib.fat5_spec_accept_sampled(ctypes.byref(q), None) == -3
    assert "workspace" in lib.fat5_last_error().decode()


def test_workspace_bytes_depend_on_the_shape_and_the_drafter_only(lib):
    assert lib.fat5_spec_accept_sampled_workspace_bytes(None) == 0
    assert lib.fat5_spec_accept_sampled_workspace_bytes(ctypes.byref(_params(M=1))) == 0
    for B, M, V, dl, want in ((1, 2, 1, False, 48), (1, 2, 1 << 20, True, 80), (8, 16, 32128, False, 8 * 16 * 24),
                              (8, 16, 32128, True, 8 * 31 * 24), (3, 5, 7, False, 368)):
        q = _params(B=B, M=M, V=V, **({} if dl else dict(draft_logits=None)))
        assert lib.fat5_spec_accept_sampled_workspace_bytes(ctypes.byref(q)) == want, (B, M, V, dl)


def test_null_and_empty(lib):
    assert lib.fat5_spec_accept_sampled(None, None) == -1
    assert lib.fat5_spec_accept_sampled(ctypes.byref(_params(B=0, workspace=None, workspace_bytes=0)), None) == 0
    assert lib.fat5_spec_accept_sampled(ctypes.byref(_params(B=0, top_p=2.0)), None) == -1   # (an empty batch is still checked)
    # the optional pointers may be NULL, and without draft_logits its strides are not looked at: the workspace check fires next
    q = _params(draft_seqlens=None, limit=None, n_accepted=None, n_new=None, draft_logits=None, draft_row_stride=0,
                draft_batch_stride=0, uniforms=None, sampled=None, aux=None, workspace=None)
    assert lib.fat5_spec_accept_sampled(ctypes.byref(q), None) == -3


# ------------------------------------------------------------------------------------------------ the operator
def _call(**kw):
    B, g, V = 2, 4, 16
    a = dict(logits=torch.zeros(B, g + 1, V), draft=torch.zeros(B, g, dtype=torch.int64), cache_seqlens=torch.zeros(B, dtype=torch.int32),
             labels=torch.zeros(B, 12, dtype=torch.int64), tok=torch.zeros(B, dtype=torch.int64), seen_eos=torch.zeros(B, dtype=torch.bool),
             limit=11, sampling=(1.0, 0, 1.0, 1))
    a.update(kw)
    return a


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(sampling=(1.0, 0, 1.0)), ValueError, "sampling must be"),
    (dict(sampling=1.0), ValueError, "sampling must be"),
    (dict(sampling=(0.0, 0, 1.0, 1)), ValueError, "temperature"),
    (dict(sampling=(1.0, -1, 1.0, 1)), ValueError, "top_k"),
    (dict(sampling=(1.0, 0, 0.0, 1)), ValueError, "top_p"),
    (dict(sampling=(1.0, 0, 1.0, 1.5)), ValueError, "seed"),
    (dict(sampling=(1.0, 0, 1.0, 1, 2.5)), ValueError, "offset"),
    (dict(draft_logits=torch.zeros(2, 5, 16)), ValueError, "draft_logits must be"),
    (dict(draft_logits=torch.zeros(2, 4, 16, dtype=torch.bfloat16)), ValueError, "draft_logits must be"),
    (dict(uniforms=torch.zeros(2, 5, 2)), ValueError, "uniforms must be"),
    (dict(uniforms=torch.zeros(2, 5, 3, dtype=torch.float64)), ValueError, "uniforms must be"),
    (dict(draft=torch.zeros(2, 3, dtype=torch.int64)), ValueError, "draft must be"),
    (dict(sampling=None, draft_logits=torch.zeros(2, 4, 16)), ValueError, "belong to sampling"),
    (dict(sampling=None, return_sampled=True), ValueError, "belong to sampling"),
])
def test_operator_checks_its_arguments(kw, exc, msg):
    from flasht5_amd import speculative_accept
    with pytest.raises(exc, match=msg):
        speculative_accept(**_call(**kw))


def test_operator_rejects_cpu_tensors_after_the_shapes():
    import flasht5_amd
    from flasht5_amd import speculative_accept
    assert callable(flasht5_amd.draft_tokens)
    with pytest.raises(ValueError, match="GPU"):
        speculative_accept(**_call())
    with pytest.raises(ValueError, match="GPU"):
        speculative_accept(**_call(draft_logits=torch.zeros(2, 4, 16), uniforms=torch.zeros(2, 5, 3), return_sampled=True))


def test_custom_op_declares_its_mutations_and_has_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import speculative  # noqa: F401  (registers the ops)
    schema = torch.ops.fat5.spec_accept_sampled.default._schema
    written = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert written == {"cache_seqlens", "labels", "tok", "seen_eos", "draft_seqlens"}
    greedy = torch.ops.fat5.spec_accept.default._schema       # (the greedy op's schema is what it was)
    assert [a.name for a in greedy.arguments] == ["logits", "draft", "cache_seqlens", "labels", "tok", "seen_eos", "limit", "limit_scalar",
                                                  "draft_seqlens", "eos_token_id"]
    with FakeTensorMode():
        a = _call(logits=torch.empty(2, 5, 16, dtype=torch.bfloat16))
        for dl, rs, ra in ((None, False, False), (torch.empty(2, 4, 16, dtype=torch.bfloat16), True, True)):
            na, nn, sampled, aux = torch.ops.fat5.spec_accept_sampled(
                a["logits"], a["draft"], a["cache_seqlens"], a["labels"], a["tok"], a["seen_eos"], None, 11, None, 1, 0.7, 50, 0.9, 3, 0,
                dl, None, rs, ra)
            assert na.shape == nn.shape == (2,) and na.dtype == nn.dtype == torch.int32
            assert tuple(sampled.shape) == ((2, 5) if rs else (0,)) and sampled.dtype == torch.int64
            assert tuple(aux.shape) == ((2, 5, 3) if ra else (0,)) and aux.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ generate's host checks
def _small_model(vocab=128, **kw):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    cfg = dict(vocab_size=vocab, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
               relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe")
    cfg.update(kw)
    return FAT5ForConditionalGeneration(FAT5Config(**cfg))


class _Reached(Exception):
    pass


def _stop_at_the_encoder(monkeypatch, *models):
    def reached(*a, **k):
        raise _Reached()
    for m in models:
        monkeypatch.setattr(m.encoder, "forward", reached)


@pytest.mark.parametrize("kw, msg", [
    (dict(assistant=True, num_beams=3), "num_beams|beam"),
    (dict(lookup=4, num_beams=3), "num_beams|beam"),
    (dict(assistant=True, repetition_penalty=1.2), "logits processors"), (dict(lookup=4, no_repeat_ngram_size=2), "logits processors"),
    (dict(assistant=True, min_length=3), "logits processors"), (dict(lookup=4, suppress_tokens=[5]), "logits processors"),
    (dict(assistant=True, lookup=4), "together with assistant_model"),
    (dict(assistant=True, temperature=0.0), "temperature"), (dict(lookup=4, top_p=0.0), "top_p"), (dict(lookup=4, top_k=-1), "top_k"),
])
def test_generate_with_do_sample_still_rejects_before_the_encoders(kw, msg, monkeypatch):
    m, a = _small_model(), _small_model(num_decoder_layers=1)
    _stop_at_the_encoder(monkeypatch, m, a)
    kw = dict(kw)
    if kw.pop("assistant", False):
        kw["assistant_model"] = a
    if "lookup" in kw:
        kw["prompt_lookup_num_tokens"] = kw.pop("lookup")
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(2, 4, dtype=torch.long), max_length=8, do_sample=True, seed=1, **kw)


def test_generate_rejects_rope_at_two_rows_with_do_sample(monkeypatch):
    m, rope = _small_model(), _small_model(position_encoding_type="RoPE")
    _stop_at_the_encoder(monkeypatch, m, rope)
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="RoPE"):
        rope.generate(ids, max_length=8, assistant_model=m, do_sample=True, seed=1)
    with pytest.raises(ValueError, match="RoPE"):
        rope.generate(ids, max_length=8, prompt_lookup_num_tokens=2, do_sample=True, seed=1)


def test_the_host_checks_no_longer_reject_do_sample(monkeypatch):
    """without the feature both checks raise ValueError ("the verification is greedy") for every input; with it they pass for
    inputs on the GPU (a stand-in with the three attributes the checks read: there is no GPU here), and inputs on the CPU are
    refused last of all, before an encoder runs, because speculative sampling has no CPU path"""
    import types
    from flasht5_amd.speculative import check_generate_args, check_lookup_generate_args
    m, a = _small_model(), _small_model(num_decoder_layers=1)
    on_gpu = types.SimpleNamespace(shape=(2, 4), is_cuda=True, device=torch.device("cuda:0"))
    for do_sample in (False, True):
        check_generate_args(m, a, on_gpu, 8, 4, 1, do_sample, 1, False)
        check_lookup_generate_args(m, on_gpu, 8, 4, 2, 1, do_sample, 1, False)
    with pytest.raises(ValueError, match="num_beams"):
        check_generate_args(m, a, on_gpu, 8, 4, 1, True, 3, False)
    _stop_at_the_encoder(monkeypatch, m, a)
    ids = torch.zeros(2, 4, dtype=torch.long)
    for kw in (dict(assistant_model=a), dict(assistant_model=a, seed=3, graph=True, return_stats=True, top_k=1),
               dict(prompt_lookup_num_tokens=4), dict(prompt_lookup_num_tokens=4, temperature=0.7, top_p=0.9, seed=5)):
        with pytest.raises(ValueError, match="do_sample=True needs input_ids .* on the GPU"):
            m.generate(ids, max_length=8, do_sample=True, **kw)
        with pytest.raises(_Reached):      # (the greedy call on the same inputs goes on to the encoder, as before)
            m.generate(ids, max_length=8, **{k: v for k, v in kw.items() if k not in ("seed", "top_k", "top_p", "temperature")})
