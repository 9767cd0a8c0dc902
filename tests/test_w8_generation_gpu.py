"""`generate(weight_dtype="fp8")` on the GPU: eager against graph replay in every mode, a decoder prompt prefilled in one chunk
against the same prompt fed token by token, an assistant against plain greedy decoding, the launch plan of a step (the recording
wrappers of test_generation_trace_gpu.py, extended to `w8_linear`), the logits against an fp64 forward of the dequantised weights,
and the memory the quantised weights take.

The logits measurement.  Z is the forward of the unquantised model and Z_q that of a twin whose quantised decoder
weights are replaced by w8 * scale, both in fp64 plain torch on the CPU (`_forward_ref`: the attention kernels take no fp32, and
a reference should not share code with what it checks).  Over 16 teacher-forced tokens, e16 = max |default 16-bit decode
logits - Z| / max |Z| is measured on the existing path, and the FP8-weight path must satisfy
max |logits_w8 - Z_q| / max |Z_q| <= 2 e16 + 2^-8: both paths carry the same activation roundings, only the weights differ."""
import copy
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
V, H, D, L_ENC, LAYERS, T = 128, 2, 64, 12, 2, 4
KV, CHUNK, W8, GATED = "flash_attn_with_kvcache", "flash_attn_with_kvcache_chunk", "w8_linear", "gated_act_packed"


def _small(rope=False, decoder_layers=LAYERS, seed=0):
    """test_generation_trace_gpu.py's small model, restated"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(position_encoding_type="RoPE") if rope else dict(attention_type="fat5_rpe")
    c = FAT5Config(vocab_size=V, d_model=64, d_kv=D, d_ff=128, num_heads=H, num_layers=1, num_decoder_layers=decoder_layers,
                   relative_attention_max_distance=64, max_sequence_length=64, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c).to(DEV).bfloat16().eval()


def _decisive(kind, seed, vocab=512):
    """test_speculative_gpu.py's decisive model, restated: lm_head row sigma(t) is token t's embedding, so the next token is
    sigma(current token) by a margin of several units -- far more than the few percent FP8 weights move a logit"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(position_encoding_type="RoPE") if kind == "rope" else dict(attention_type="fat5_rpe")
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    m = FAT5ForConditionalGeneration(c).to(DEV).bfloat16().eval()
    sigma = torch.randperm(vocab, generator=torch.Generator().manual_seed(1000 + seed))
    with torch.no_grad():
        m.lm_head.weight[sigma] = m.shared.weight
    return m, sigma


@pytest.fixture(scope="module")
def models():
    return dict(t5=_small(), rope=_small(rope=True))


@pytest.fixture(scope="module")
def decisive():
    m, sigma = _decisive("t5_rpe", 3)
    a, _ = _decisive("t5_rpe", 53)
    with torch.no_grad():   # (the assistant decides like the target: its drafts are accepted, the rounds are ragged at EOS only)
        a.lm_head.weight.zero_()
        a.lm_head.weight[sigma] = a.shared.weight
    ids = torch.randint(2, 512, (3, 33), generator=torch.Generator().manual_seed(103)).to(DEV)
    return m, a, sigma, ids


def _ids(B):
    return torch.randint(2, V, (B, L_ENC), generator=torch.Generator().manual_seed(5)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ eager vs graph
MODES = {
    "greedy": dict(),
    "sampled": dict(do_sample=True, top_k=20, seed=11),
    "beams": dict(num_beams=2),
    "processor": dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
    "prompt lookup": dict(prompt_lookup_num_tokens=2),
    "fp8 caches": dict(kv_cache_dtype="fp8"),
    "decoder prompt": dict(decoder_input_ids=torch.tensor([[0, 7, 9], [0, 23, 5]])),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_eager_and_graph_give_the_same_tokens(models, mode):
    kw = MODES[mode]
    eager = models["t5"].generate(_ids(2), max_length=8, weight_dtype="fp8", **kw)
    graph = models["t5"].generate(_ids(2), max_length=8, weight_dtype="fp8_e4m3", graph=True, **kw)
    assert torch.equal(eager, graph)
    assert eager.shape[1] >= 2


@pytest.mark.parametrize("sampled", [False, True])
def test_rope_and_padding_eager_and_graph(models, sampled):
    kw = dict(do_sample=True, top_k=20, seed=3) if sampled else {}
    eager = models["rope"].generate(_ids(1), max_length=8, weight_dtype="fp8", **kw)
    graph = models["rope"].generate(_ids(1), max_length=8, weight_dtype="fp8", graph=True, **kw)
    assert torch.equal(eager, graph)
    mask = torch.ones((2, L_ENC), dtype=torch.long, device=DEV)
    mask[1, 7:] = 0
    eager = models["t5"].generate(_ids(2), attention_mask=mask, max_length=8, weight_dtype="fp8", **kw)
    graph = models["t5"].generate(_ids(2), attention_mask=mask, max_length=8, weight_dtype="fp8", graph=True, **kw)
    assert torch.equal(eager, graph)


# ------------------------------------------------------------------------------------------------- prompts and the assistant
def test_prompt_in_one_chunk_equals_token_by_token(decisive):
    m, _, sigma, ids = decisive
    inv = torch.argsort(sigma)
    prompt = torch.tensor([[0, 5, 7], [0, 5, int(inv[inv[1]])], [0, 5, 11]]).to(DEV)   # (row 1 reaches EOS two tokens on)
    P, T_MAX = prompt.shape[1], 8
    out = m.generate(ids, max_length=T_MAX, decoder_input_ids=prompt, weight_dtype="fp8")
    st = m.init_decode_state(ids, max_length=T_MAX, prompt_length=P, weight_dtype="fp8")
    assert st.w8 is m.quantize_decoder_weights()
    for t in range(P - 1):
        m.decode_step(st, prompt[:, t])
    tok, want = prompt[:, P - 1], [prompt]
    for _ in range(out.shape[1] - P):
        tok = m.decode_step(st, tok).argmax(-1)
        want.append(tok.unsqueeze(1))
    from flasht5_amd.generation import finish_labels
    assert torch.equal(out, finish_labels(torch.cat(want, 1)))
    assert out[1, P:P + 2].tolist() == [int(sigma[prompt[1, 2]]), 1]
    # on a decisive model the FP8 weights decode the tokens of the 16-bit ones
    assert torch.equal(out, m.generate(ids, max_length=T_MAX, decoder_input_ids=prompt))


@pytest.mark.parametrize("graph", [False, True])
def test_assistant_equals_plain_greedy(decisive, graph):
    m, a, _, ids = decisive
    plain = m.generate(ids, max_length=12, weight_dtype="fp8")
    out, stats = m.generate(ids, max_length=12, weight_dtype="fp8", assistant_model=a, num_assistant_tokens=3, return_stats=True,
                            graph=graph)
    assert torch.equal(out, plain)
    assert stats["accepted"] > 0 and getattr(a, "_w8_decoder", None) is not None   # (the assistant read FP8 weights too)


def test_quantised_weights_are_built_once_and_rebuilt_on_change(models):
    m = _small(seed=9)
    first = m.quantize_decoder_weights()
    assert m.quantize_decoder_weights() is first
    m.generate(_ids(2), max_length=3, weight_dtype="fp8")
    assert m.quantize_decoder_weights() is first
    with torch.no_grad():
        m.decoder.block[1].ff_layer.wo.weight.mul_(2)
    second = m.quantize_decoder_weights()
    assert second is not first
    assert torch.equal(second.layers[1].wo[1], first.layers[1].wo[1] * 2)
    assert torch.equal(second.layers[0].wo[0].view(torch.uint8), first.layers[0].wo[0].view(torch.uint8))
    assert "_w8_decoder" not in m.state_dict() and all(p.dtype == torch.bfloat16 for p in m.parameters())


# --------------------------------------------------------------------------------------------------------------- launch trace
@pytest.fixture
def trace(monkeypatch):
    import importlib
    from flasht5_amd import decode, w8
    gated_act = importlib.import_module("flasht5_amd.gated_act")   # (the package exports a function of that name)
    calls = []

    def wrap(module, name):
        fn = getattr(module, name)
        sig = inspect.signature(fn)

        def recorder(*args, **kwargs):
            given = sig.bind(*args, **kwargs).arguments
            first = next(a for a in given.values() if torch.is_tensor(a))
            optional = frozenset(n for n, p in sig.parameters.items() if p.default is None and given.get(n) is not None)
            calls.append((name, tuple(first.shape), optional))
            return fn(*args, **kwargs)
        monkeypatch.setattr(module, name, recorder)

    for module, name in ((decode, KV), (decode, CHUNK), (w8, W8), (gated_act, GATED)):
        wrap(module, name)
    return calls


def _plan(rows, M, layers=LAYERS, last_rows=None, head=True):
    """the launches of one decoder pass over the FP8 weights (d_model 64, inner H * D = 128, d_ff 128, gated)"""
    att = KV if M == 1 else CHUNK
    normed, added = frozenset({"norm_weight"}), frozenset({"residual"})
    layer = [(W8, (rows, M, 64), normed),                                                                # norm + qkv
             (att, (rows, M, H, D), frozenset({"k", "v", "cache_seqlens", "softmax_scale", "rpe1d"})),   # self-attention
             (W8, (rows, M, H * D), added),                                                              # o + residual
             (W8, (rows, M, 64), normed),                                                                # norm + q
             (att, (rows, M, H, D), frozenset({"softmax_scale"})),                                       # cross-attention
             (W8, (rows, M, H * D), added),                                                              # o + residual
             (W8, (rows, M, 64), normed),                                                                # norm + wi
             (GATED, (rows, M, 256), frozenset()),                                                       # the gated activation
             (W8, (rows, M, 128), added)]                                                                # wo + residual
    return layer * layers + ([(W8, (rows, M if last_rows is None else last_rows, 64), normed)] if head else [])   # final norm + lm_head


def _same(calls, expected):
    assert len(calls) == len(expected), (len(calls), len(expected), calls)
    for i, (got, want) in enumerate(zip(calls, expected)):
        assert got == want, (i, got, want)


def test_trace_of_a_step(models, trace):
    m = models["t5"]
    assert m.decoder.block[0].ff_layer.act.glu
    out = m.generate(_ids(2), max_length=T, weight_dtype="fp8")
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    _same(trace, _plan(2, 1) * steps)
    assert sum(1 for c in trace if c[0] == W8) == (6 * LAYERS + 1) * steps


def test_trace_of_a_prompt_chunk(models, trace):
    m = models["t5"]
    prompt = torch.tensor([[0, 7, 9], [0, 23, 5]], device=DEV)
    out = m.generate(_ids(2), max_length=T, decoder_input_ids=prompt, weight_dtype="fp8")
    steps = out.shape[1] - 3
    _same(trace, _plan(2, 2, head=False) + _plan(2, 1) * steps)     # (the prefill makes no logits: no head)
    del trace[:]
    st = m.init_decode_state(_ids(2), max_length=4, prompt_length=3, weight_dtype="fp8")
    m.decode_chunk(st, prompt, logits="last")
    _same(trace, _plan(2, 3, last_rows=1))                          # (final norm + lm_head on the selected row only)


def test_no_w8_launch_without_the_argument(models, trace):
    models["t5"].generate(_ids(2), max_length=T)
    models["t5"].generate(_ids(2), max_length=T, weight_dtype=None, kv_cache_dtype="fp8")
    assert trace and not any(c[0] in (W8, GATED) for c in trace)


# -------------------------------------------------------------------------------------------------------------------- logits
def _rot(x, cos, sin, interleaved):
    """flash_attn's rotation of x (B, S, H, D) by the table rows 0 .. S - 1"""
    rd = 2 * cos.shape[-1]
    c, s = cos[None, :x.shape[1], None, :], sin[None, :x.shape[1], None, :]
    xr, rest = x[..., :rd], x[..., rd:]
    x1, x2 = (xr[..., 0::2], xr[..., 1::2]) if interleaved else (xr[..., :rd // 2], xr[..., rd // 2:])
    o1, o2 = x1 * c - x2 * s, x1 * s + x2 * c
    out = torch.stack([o1, o2], -1).flatten(-2) if interleaved else torch.cat([o1, o2], -1)
    return torch.cat([out, rest], -1)


def _norm(ln, h):
    return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + ln.variance_epsilon) * ln.weight


def _attention_ref(att, x, kv, bias, causal, tables):
    B, M, _ = x.shape
    Hh, Dh = att.n_heads, att.key_value_proj_dim
    q = (x @ att.Wq.weight.t()).view(B, M, Hh, Dh)
    k = (kv @ att.Wk.weight.t()).view(B, kv.shape[1], Hh, Dh)
    v = (kv @ att.Wv.weight.t()).view(B, kv.shape[1], Hh, Dh)
    if tables is not None:   # (the module rotates v as it rotates k)
        cos, sin, cos_k, sin_k = tables
        ck, sk = (cos, sin) if cos_k is None else (cos_k, sin_k)
        il = att.pe_encoding.interleaved
        q, k, v = _rot(q, cos, sin, il), _rot(k, ck, sk, il), _rot(v, ck, sk, il)
    s = torch.einsum("bmhd,bnhd->bhmn", q, k) * att.softmax_scale
    if bias is not None:
        s = s + bias
    if causal:
        s = s.masked_fill(torch.ones(M, kv.shape[1], dtype=torch.bool).triu(1), float("-inf"))
    o = torch.einsum("bhmn,bnhd->bmhd", torch.softmax(s, -1), v).reshape(B, M, Hh * Dh)
    return o @ att.o.weight.t()


def _tables64(pe):
    """rotary.rotary_tables' arithmetic in fp64"""
    dim, n = pe.dim, pe.max_sequence_length
    inv_freq = 1.0 / (pe.base ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    freqs = torch.outer(torch.arange(n, dtype=torch.float64), inv_freq)
    c, s = torch.cos(freqs), torch.sin(freqs)
    if pe.scale_base is None:
        return c, s, None, None
    scale = (torch.arange(0, dim, 2, dtype=torch.float64) + 0.4 * dim) / (1.4 * dim)
    sc = scale ** ((torch.arange(n, dtype=torch.float64) - n // 2) / pe.scale_base)[:, None]
    return c * sc, s * sc, c / sc, s / sc


def _stack_ref(stack, ids, enc=None):
    h = stack.embed_tokens(ids)
    first = stack.block[0].self_attention_layer.self_attention
    S = ids.shape[1]
    tables = bias = None
    if first.rotary:
        tables = _tables64(first.pe_encoding)
    else:
        bias = first.pe_encoding.compute_bias(S, S)
    for blk in stack.block:
        sa = blk.self_attention_layer
        n = _norm(sa.layer_norm, h)
        h = h + _attention_ref(sa.self_attention, n, n, bias, sa.self_attention.is_causal, tables)
        if enc is not None:
            ca = blk.cross_attention_layer
            h = h + _attention_ref(ca.cross_attention, _norm(ca.layer_norm, h), enc, None, False, tables)
        ff = blk.ff_layer
        n = _norm(ff.layer_norm, h)
        a = ff.act
        t = a.act(n @ a.wi_0.weight.t()) * (n @ a.wi_1.weight.t()) if a.glu else a.act(n @ a.wi.weight.t())
        h = h + t @ ff.wo.weight.t()
    return _norm(stack.final_layer_norm, h)


@torch.no_grad()
def _forward_ref(twin, ids, tokens):
    """the full forward in fp64 plain torch on the CPU -> logits (B, T, V)"""
    enc = _stack_ref(twin.encoder, ids)
    return _stack_ref(twin.decoder, tokens, enc) @ twin.lm_head.weight.t()


def _dequantised_twin(m):
    """an fp64 CPU copy of m whose quantised decoder weights are replaced by w8 * scale"""
    twin = copy.deepcopy(m).cpu().double()
    q = m.quantize_decoder_weights()
    deq = lambda pair: (pair[0].double() * pair[1].double().unsqueeze(1)).cpu()  # noqa: E731
    with torch.no_grad():
        for blk, lw in zip(twin.decoder.block, q.layers):
            sa, ca, ff = blk.self_attention_layer.self_attention, blk.cross_attention_layer.cross_attention, blk.ff_layer
            for lin, w in zip((sa.Wq, sa.Wk, sa.Wv), deq(lw.qkv).chunk(3, 0)):
                lin.weight.copy_(w)
            sa.o.weight.copy_(deq(lw.self_o))
            ca.Wq.weight.copy_(deq(lw.cross_q))
            ca.o.weight.copy_(deq(lw.cross_o))
            if ff.act.glu:
                for lin, w in zip((ff.act.wi_0, ff.act.wi_1), deq(lw.wi).chunk(2, 0)):
                    lin.weight.copy_(w)
            else:
                ff.act.wi.weight.copy_(deq(lw.wi))
            ff.wo.weight.copy_(deq(lw.wo))
        twin.lm_head.weight.copy_(deq(q.lm_head))
    return twin


def _forced_logits(m, ids, tokens, **kw):
    st = m.init_decode_state(ids, max_length=tokens.shape[1], **kw)
    return torch.stack([m.decode_step(st, tokens[:, t]).double().cpu() for t in range(tokens.shape[1])], 1)


@pytest.mark.parametrize("kind", ["t5", "rope"])
def test_logits_against_the_dequantised_forward(models, kind):
    """Measured on an MI355X (printed as "[w8] ..."): see DESIGN 4.23 for the figures of both models."""
    m = models[kind]
    ids = _ids(2)
    tokens = torch.randint(2, V, (2, 16), generator=torch.Generator().manual_seed(21)).to(DEV)
    tokens[:, 0] = 0
    Z = _forward_ref(copy.deepcopy(m).cpu().double(), ids.cpu(), tokens.cpu())
    Zq = _forward_ref(_dequantised_twin(m), ids.cpu(), tokens.cpu())
    z16 = _forced_logits(m, ids, tokens)
    z8 = _forced_logits(m, ids, tokens, weight_dtype="fp8")
    e16 = float((z16 - Z).abs().max() / Z.abs().max())
    e8 = float((z8 - Zq).abs().max() / Zq.abs().max())
    shift = float((Zq - Z).abs().max() / Z.abs().max())
    print(f"[w8] {kind}: e16 {e16:.5f}  fp8-weight path against its own truth {e8:.5f}  allowed {2 * e16 + 2 ** -8:.5f}  "
          f"(quantisation itself moves the logits by {shift:.5f} of max |Z| = {float(Z.abs().max()):.3f})")
    assert e8 <= 2 * e16 + 2.0 ** -8


# -------------------------------------------------------------------------------------------------------------------- memory
def test_memory_of_the_quantised_weights(models):
    m = models["t5"]
    q = m.quantize_decoder_weights()
    pairs = q.pairs()
    assert len(pairs) == 6 * LAYERS + 1
    for w8_, scale in pairs:
        N, K = w8_.shape
        assert w8_.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and tuple(scale.shape) == (N,)
        assert (w8_.nbytes + scale.nbytes) / (2 * N * K) == (N * K + 4 * N) / (2 * N * K)
    src = [p for blk in m.decoder.block for p in (
        blk.self_attention_layer.self_attention.Wq.weight, blk.self_attention_layer.self_attention.Wk.weight,
        blk.self_attention_layer.self_attention.Wv.weight, blk.self_attention_layer.self_attention.o.weight,
        blk.cross_attention_layer.cross_attention.Wq.weight, blk.cross_attention_layer.cross_attention.o.weight,
        blk.ff_layer.act.wi_0.weight, blk.ff_layer.act.wi_1.weight, blk.ff_layer.wo.weight)] + [m.lm_head.weight]
    assert sum(w.shape[0] for w, _ in pairs) == sum(p.shape[0] for p in src)
    assert sum(w.nbytes + s.nbytes for w, s in pairs) == sum(p.numel() + 4 * p.shape[0] for p in src)
