"""`generate(kv_cache_dtype="fp8")` on the GPU: the cache bytes, exact equality with the default caches on decisive models (greedy
eager and graphed, a decoder prompt, a padded encoder, beam search, an assistant), the logits of a random-lm_head model against
the bf16-cache logits and the training forward, and seeded sampling.

Decisive models (test_speculative_gpu.py's construction): lm_head row sigma(t) is token t's embedding, so the logit of sigma(t) is
|e_t|^2-like and the others are near-orthogonal products -- a margin of several units against a quantisation error of the hidden
state that moves logits by a few percent, so the FP8 caches decode the same tokens.

The random-lm_head measurement (MEASURED below): teacher-forced decode-step logits with FP8 caches against the same
steps with bf16 caches, over 32 forced tokens, as a fraction of max |logits|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
T_MAX = 16
LOGIT_BOUND = 2e-2     # decode-path logits against the training forward, times max(1, max |Z|)
# max |Z_fp8 - Z_bf16| / max |Z_bf16| over 32 teacher-forced steps, as measured on an MI355X with the models and seeds of
# test_random_lm_head_logits (printed by that test as "[kvfp8] ... gap"); the test allows twice this on top of LOGIT_BOUND
MEASURED = {"t5_rpe": 0.0305, "rope": 0.0270}


def _model(kind, seed=0, vocab=512):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(attention_type="fat5_rpe")
    if kind == "rope":
        kw = dict(position_encoding_type="RoPE")
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


def _decisive(kind, seed):
    m = _model(kind, seed=seed).to(DEV).bfloat16()
    sigma = torch.randperm(m.config.vocab_size, generator=torch.Generator().manual_seed(1000 + seed))
    with torch.no_grad():
        m.lm_head.weight[sigma] = m.shared.weight
    return m, sigma


class _Setup:
    def __init__(self, kind, B):
        self.m, self.sigma = _decisive(kind, 3)
        self.a, _ = _decisive(kind, 53)
        with torch.no_grad():   # (the assistant decides like the target on half the ids)
            half = torch.rand(len(self.sigma), generator=torch.Generator().manual_seed(77)) < 0.5
            self.a.lm_head.weight.zero_()
            sg = self.sigma.clone()
            other = half.nonzero()[:, 0]
            sg[other] = self.sigma[other.roll(1)]
            self.a.lm_head.weight[sg] = self.a.shared.weight
        V = self.m.config.vocab_size
        self.ids = torch.randint(2, V, (B, 33), generator=torch.Generator().manual_seed(103)).to(DEV)
        inv = torch.argsort(self.sigma)
        last = [7, int(inv[inv[1]]), 11, 13][:B]   # row 1 reaches EOS two tokens after its prompt
        self.prompt = torch.tensor([[0, 5, t] for t in last]).to(DEV)
        self.mask = torch.ones_like(self.ids)
        for b, n in enumerate([33, 20, 9, 27][:B]):
            self.mask[b, n:] = 0


@pytest.fixture(scope="module")
def t5():
    return _Setup("t5_rpe", 4)


@pytest.fixture(scope="module")
def rope():
    return _Setup("rope", 1)


def _kv_bytes(st):
    n = sum(t.nbytes for lst in (st.self_k, st.self_v, st.cross_k, st.cross_v) for t in lst)
    for lst in (st.self_k_scale, st.self_v_scale, st.cross_k_scale, st.cross_v_scale):
        n += sum(t.nbytes for t in lst) if lst is not None else 0
    return n


def test_cache_bytes(t5):
    D = 64
    for kw in (dict(), dict(num_beams=3)):
        from flasht5_amd.generation import init_decode_state
        a = init_decode_state(t5.m, t5.ids, 16, **kw)
        b = init_decode_state(t5.m, t5.ids, 16, kv_cache_dtype="fp8", **kw)
        assert a.self_k_scale is None and all(t.dtype == torch.bfloat16 for t in a.self_k + a.cross_v)
        assert all(t.dtype == torch.float8_e4m3fn for t in b.self_k + b.self_v + b.cross_k + b.cross_v)
        assert all(t.dtype == torch.float32 and t.shape == c.shape[:3] for t, c in zip(b.self_k_scale + b.cross_v_scale, b.self_k + b.cross_v))
        assert _kv_bytes(b) * 2 * D == _kv_bytes(a) * (D + 4)
    c = t5.m.init_decode_state(t5.ids, 16, kv_cache_dtype="fp8_e4m3")
    assert _kv_bytes(c) == _kv_bytes(init_decode_state(t5.m, t5.ids, 16, kv_cache_dtype="fp8"))


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_equals_the_default_caches(t5, rope, graph):
    for s in (t5, rope):
        want = s.m.generate(s.ids, max_length=T_MAX)
        got = s.m.generate(s.ids, max_length=T_MAX, graph=graph, kv_cache_dtype="fp8")
        assert torch.equal(got, want)
        assert want.shape[1] > 8   # (the run is long enough to mean something)
        wantp = s.m.generate(s.ids, max_length=T_MAX, decoder_input_ids=s.prompt)
        gotp = s.m.generate(s.ids, max_length=T_MAX, graph=graph, decoder_input_ids=s.prompt, kv_cache_dtype="fp8")
        assert torch.equal(gotp, wantp)
        wantm = s.m.generate(s.ids, s.mask, max_length=T_MAX)
        gotm = s.m.generate(s.ids, s.mask, max_length=T_MAX, graph=graph, kv_cache_dtype="fp8_e4m3")
        assert torch.equal(gotm, wantm)


def test_ragged_prompt_and_processors_equal_the_default_caches(t5):
    dmask = torch.ones_like(t5.prompt)
    dmask[2, 2:] = 0
    dmask[3, 1:] = 0
    kw = dict(max_length=T_MAX, decoder_input_ids=t5.prompt, decoder_attention_mask=dmask)
    assert torch.equal(t5.m.generate(t5.ids, kv_cache_dtype="fp8", graph=True, **kw), t5.m.generate(t5.ids, **kw))
    kw = dict(max_length=T_MAX, repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4, suppress_tokens=[5, 9])
    assert torch.equal(t5.m.generate(t5.ids, kv_cache_dtype="fp8", graph=True, **kw), t5.m.generate(t5.ids, **kw))


@pytest.mark.parametrize("graph", [False, True])
def test_beam_search_equals_the_default_caches(t5, graph):
    want, ws = t5.m.generate(t5.ids, t5.mask, max_length=T_MAX, num_beams=3, num_return_sequences=2, return_scores=True)
    got, gs = t5.m.generate(t5.ids, t5.mask, max_length=T_MAX, num_beams=3, num_return_sequences=2, return_scores=True, graph=graph,
                            kv_cache_dtype="fp8")
    assert torch.equal(got, want)
    assert float((gs - ws).abs().max()) <= 0.05 * max(1.0, float(ws.abs().max()))   # (scores are sums of log-probabilities: close, not equal)


@pytest.mark.parametrize("graph", [False, True])
def test_an_assistant_equals_greedy_fp8(t5, rope, graph):
    for s in (t5, rope):
        want = s.m.generate(s.ids, max_length=T_MAX, kv_cache_dtype="fp8")
        got, st = s.m.generate(s.ids, max_length=T_MAX, assistant_model=s.a, num_assistant_tokens=4, graph=graph, return_stats=True,
                               kv_cache_dtype="fp8")
        assert torch.equal(got, want) and 0 <= st["accepted"] <= st["drafted"]
        if s is t5:   # (the assistant agrees on about half the ids: some drafts are kept, some are not)
            assert 0 < st["accepted"] < st["drafted"]
        wantp = s.m.generate(s.ids, max_length=T_MAX, decoder_input_ids=s.prompt, kv_cache_dtype="fp8")
        gotp = s.m.generate(s.ids, max_length=T_MAX, assistant_model=s.a, graph=graph, decoder_input_ids=s.prompt, kv_cache_dtype="fp8")
        assert torch.equal(gotp, wantp)


def _forced_logits(m, ids, tokens, kv):
    st = m.init_decode_state(ids, max_length=tokens.shape[1], kv_cache_dtype=kv)
    return torch.stack([m.decode_step(st, tokens[:, t]).float() for t in range(tokens.shape[1])], 1)


@pytest.mark.parametrize("kind", ["t5_rpe", "rope"])
def test_random_lm_head_logits(kind):
    """32 teacher-forced steps of a random-lm_head model.  FP8-cache logits against bf16-cache logits: the measured gap (printed;
    MEASURED holds what an MI355X gave: t5_rpe 0.0305, rope 0.0270 of max |Z|, where max |Z| is 3.84 and 3.92, |bf16 - Z| 0.031
    in both and |fp8 - Z| 0.109 and 0.106, against bounds of 0.311 and 0.290).  Against the training forward's logits Z the FP8
    path must stay within LOGIT_BOUND * max(1, max |Z|), the bf16 decode path's bound, plus twice the measured gap."""
    m = _model(kind, seed=11).to(DEV).bfloat16()
    V = m.config.vocab_size
    B = 2 if kind == "t5_rpe" else 1
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, V, (B, 33), generator=g).to(DEV)
    tokens = torch.cat((torch.zeros(B, 1, dtype=torch.long), torch.randint(2, V, (B, 31), generator=g)), 1).to(DEV)
    z16 = _forced_logits(m, ids, tokens, None)
    z8 = _forced_logits(m, ids, tokens, "fp8")
    with torch.no_grad():   # the training forward over the same decoder inputs
        enc = m.encoder(ids)
        Z = m.lm_head(m.decoder(tokens, encoder_hidden_states=enc)).float()
    zmax = float(Z.abs().max())
    gap = float((z8 - z16).abs().max()) / float(z16.abs().max())
    e16, e8 = float((z16 - Z).abs().max()), float((z8 - Z).abs().max())
    print(f"[kvfp8] {kind}: max|Z| {zmax:.3f}; fp8-vs-bf16 gap {gap:.5f} of max|Z|; |bf16 - Z| {e16:.4f}, |fp8 - Z| {e8:.4f}")
    bound = LOGIT_BOUND * max(1.0, zmax) + 2 * MEASURED[kind] * zmax
    print(f"[kvfp8] {kind}: bound {bound:.4f}")
    assert torch.isfinite(z8).all()
    assert gap > 0            # (the caches are quantised: the logits cannot be the bf16 ones)
    assert e8 <= bound


def test_sampling_is_seeded_and_the_same_eager_and_graphed(t5):
    m = _model("t5_rpe", seed=11).to(DEV).bfloat16()
    kw = dict(max_length=12, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=1234, kv_cache_dtype="fp8")
    a = m.generate(t5.ids, **kw)
    b = m.generate(t5.ids, **kw)
    c = m.generate(t5.ids, graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert a.shape[0] == t5.ids.shape[0] and a.shape[1] > 2
    d = m.generate(t5.ids, **dict(kw, seed=99))
    assert d.shape != a.shape or not torch.equal(a, d)
