"""Padding in generation on the GPU: with a right-padded `attention_mask` the ids under the padding reach neither the
encoder's valid rows nor the decoder (the check that fails without the feature); a row of a padded batch decodes what it decodes
alone, unpadded -- exactly on a decisive model in every mode, eager and graphed, and within the decode path's logit bound (DESIGN
4.10, as the speculative tests apply it) on a model with a random lm_head; ragged decoder prompts (`decoder_attention_mask`) give
each row the single-row run of its own prompt.

The model is the small one of the CPU tests: d_model 64, 2 heads of 64, 1 encoder and 2 decoder layers, vocabulary 128; B = 3,
L = 12 with lengths (12, 7, 1): a full row, a padded one and a single token."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, L, LENS = 3, 12, (12, 7, 1)
T = 6
KINDS = ["t5_rpe", "t5_triton", "rope"]
LOGIT_BOUND = 0.02   # the decode path's logits against the training forward's, relative to max(1, max|Z|)


def _model(kind, seed=0, decoder_layers=2):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(t5_rpe=dict(attention_type="fat5_rpe"), t5_triton=dict(attention_type="triton"),
              rope=dict(position_encoding_type="RoPE"))[kind]
    c = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=decoder_layers,
                   relative_attention_max_distance=64, max_sequence_length=64, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c).to(DEV).bfloat16()


def _decisive(m, seed=3):
    """the speculative tests' construction: lm_head row sigma(t) is token t's embedding, so the next token is sigma(current token)"""
    sigma = torch.randperm(m.config.vocab_size, generator=torch.Generator().manual_seed(1000 + seed))
    with torch.no_grad():
        m.lm_head.weight[sigma.to(DEV)] = m.shared.weight
    return sigma


def _ids(seed=5):
    return torch.randint(2, 128, (B, L), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _mask(lens=LENS, width=L):
    return (torch.arange(width, device=DEV).unsqueeze(0) < torch.tensor(lens, device=DEV).unsqueeze(1)).long()


def _row_equals(out, b, single):
    """row b of a batch result is the single-row result, then zeros (the batch is as wide as its longest row)"""
    w = single.shape[1]
    return w <= out.shape[1] and torch.equal(out[b, :w], single[0]) and bool((out[b, w:] == 0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_ids_under_the_padding_change_nothing(kind):
    """the encoder's valid rows and the first decoder step's logits, bit for bit, under two fillings of the padded positions"""
    from flasht5_amd.generation import init_decode_state
    m = _model(kind)
    ids, mask = _ids(), _mask()
    other = torch.where(mask.bool(), ids, (ids * 7 + 3) % 126 + 2)
    assert not torch.equal(ids, other)
    tok = torch.zeros(B, dtype=torch.long, device=DEV)
    a, b = m.init_decode_state(ids, T, mask), m.init_decode_state(other, T, mask)
    assert a.cross_seqlens.tolist() == list(LENS) and a.cross_seqlens.dtype == torch.int32
    for r, n in enumerate(LENS):
        assert torch.equal(a.encoder_hidden_states[r, :n], b.encoder_hidden_states[r, :n]), (kind, r)
    la, lb = m.decode_step(a, tok), m.decode_step(b, tok)
    assert torch.equal(la, lb), kind
    # the chunk step carries the lengths too
    ca, cb = m.init_decode_state(ids, T, mask), m.init_decode_state(other, T, mask)
    two = torch.tensor([[0, 5]] * B, device=DEV)
    assert torch.equal(m.decode_chunk(ca, two), m.decode_chunk(cb, two)), kind
    # beam rows read their input's length
    s = init_decode_state(m, ids, T, mask, num_beams=2)
    assert s.cross_seqlens.tolist() == [12, 12, 7, 7, 1, 1]
    # an all-ones mask is no mask
    assert m.init_decode_state(ids, T, torch.ones_like(mask)).cross_seqlens is None


MODES = {
    "greedy": dict(),
    "beam": dict(num_beams=2),
    "sample_top1": dict(do_sample=True, top_k=1, seed=11),
    "assistant": None,
}


# every mode under fat5_rpe; the dense-bias and the RoPE variant in the modes that reach their own code (the masked-bias and the
# rotated packed encoder, the beam step's repeated lengths); speculative decoding with RoPE is B = 1 only: nothing to pad against
ROW_CASES = [("t5_rpe", mode) for mode in MODES] + [(kind, mode) for kind in ("t5_triton", "rope") for mode in ("greedy", "beam")] + [
    ("t5_triton", "assistant")]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind, mode", ROW_CASES)
def test_rows_decode_what_they_decode_alone(kind, mode, graph):
    m = _model(kind)
    _decisive(m)
    kw = MODES[mode]
    if mode == "assistant":
        a = _model(kind, seed=50, decoder_layers=1)
        _decisive(a)
        kw = dict(assistant_model=a, num_assistant_tokens=3)
    ids, mask = _ids(), _mask()
    out = m.generate(ids, mask, max_length=T, graph=graph, **kw)
    assert out.shape[0] == B
    for r, n in enumerate(LENS):
        single = m.generate(ids[r:r + 1, :n], max_length=T, **kw)
        assert _row_equals(out, r, single), (kind, mode, graph, r, out[r].tolist(), single[0].tolist())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", KINDS)
def test_random_lm_head_stays_within_the_logit_bound(kind, graph):
    """every produced token against the teacher-forced logits Z of the unpadded single-row training forward:
    Z[token] >= max Z - 2 * 0.02 * max(1, max|Z|)"""
    m = _model(kind, seed=11)
    ids, mask = _ids(7), _mask()
    out = m.generate(ids, mask, max_length=T, graph=graph)
    W = out.shape[1]
    worst, checked = 0.0, 0
    for r, n in enumerate(LENS):
        row = out[r]
        ones = (row == 1).nonzero()
        e = int(ones[0])
        last = e if e < W - 1 else W - 2   # (the last column of the result is forced to 1: not a produced token)
        with torch.no_grad():
            Z = m.lm_head(m.decoder(row[:last].unsqueeze(0), encoder_hidden_states=m.encoder(ids[r:r + 1, :n]))).float()[0]
        for t in range(last):   # Z[t] chooses column t + 1
            gap = float(Z[t].max() - Z[t, row[t + 1]]) / max(1.0, float(Z[t].abs().max()))
            worst = max(worst, gap)
            checked += 1
            assert gap <= 2 * LOGIT_BOUND, (kind, graph, r, t, gap)
    print(f"[padding] {kind} {'graph' if graph else 'eager'}: {checked} tokens, worst gap {worst:.3e} of {2 * LOGIT_BOUND:.1e}")
    assert checked >= B


PROMPT_LENS = (1, 3, 4)


def _prompt():
    """(B, 4) right-padded prompts of lengths (1, 3, 4); the padding holds an id the prompt's own checks would refuse (EOS)"""
    return torch.tensor([[0, 1, 1, 1], [0, 5, 9, 1], [0, 7, 11, 13]]).to(DEV)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("padded_input", [False, True], ids=["full", "padded"])
def test_ragged_prompts_equal_the_single_row_runs(graph, padded_input):
    m = _model("t5_rpe")
    _decisive(m)
    ids = _ids()
    mask = _mask() if padded_input else None
    prompt, pmask = _prompt(), _mask(PROMPT_LENS, 4)
    out = m.generate(ids, mask, max_length=T, graph=graph, decoder_input_ids=prompt, decoder_attention_mask=pmask)
    assert out.shape[0] == B and out.shape[1] <= 4 + T
    sampled = m.generate(ids, mask, max_length=T, graph=graph, decoder_input_ids=prompt, decoder_attention_mask=pmask,
                         do_sample=True, top_k=1, seed=3)
    assert torch.equal(sampled, out)
    for r, (n, p) in enumerate(zip(LENS, PROMPT_LENS)):
        src = ids[r:r + 1, :n] if padded_input else ids[r:r + 1]
        single = m.generate(src, max_length=T, decoder_input_ids=prompt[r:r + 1, :p].clone())
        assert torch.equal(single[0, :p], prompt[r, :p])
        assert _row_equals(out, r, single), (graph, padded_input, r, out[r].tolist(), single[0].tolist())


def test_ragged_prompt_bookkeeping():
    """one chunk step prefills all rows; the lengths advance by P_b; each row's logits are taken at its own last prompt row"""
    from flasht5_amd import decode
    m = _model("t5_rpe")
    sigma = _decisive(m)
    ids = _ids()
    prompt, pmask = _prompt(), _mask(PROMPT_LENS, 4)
    st = m.init_decode_state(ids, T, prompt_length=4)
    lens = torch.tensor(PROMPT_LENS, dtype=torch.int32, device=DEV)
    lg = m.decode_chunk(st, prompt.masked_fill(pmask == 0, 0), logits="last", chunk_seqlens=lens)
    assert st.cache_seqlens.tolist() == list(PROMPT_LENS) and lg.shape == (B, 128)
    for r, p in enumerate(PROMPT_LENS):   # row r's logits are those of its own last prompt token: the decisive successor
        assert int(lg[r].argmax()) == int(sigma[prompt[r, p - 1]])
        for i in range(len(st.self_k)):
            assert bool((st.self_k[i][r, p:] == 0).all()), "a cache row past the row's prompt was written"
    calls = []
    real = decode.flash_attn_with_kvcache_chunk
    decode.flash_attn_with_kvcache_chunk = lambda *a, **k: (calls.append(k.get("chunk_seqlens") is not None), real(*a, **k))[1]
    try:
        m.generate(ids, max_length=3, decoder_input_ids=prompt, decoder_attention_mask=pmask)
    finally:
        decode.flash_attn_with_kvcache_chunk = real
    assert calls == [True] * (2 * len(m.decoder.block))   # ONE prefill step: self- and cross-attention of every block


def test_ragged_prompt_rope_one_row():
    m = _model("rope")
    _decisive(m)
    ids = _ids()[:1]
    prompt = torch.tensor([[0, 5, 9, 1]], device=DEV)
    out = m.generate(ids, max_length=T, decoder_input_ids=prompt, decoder_attention_mask=_mask((3,), 4))
    single = m.generate(ids, max_length=T, decoder_input_ids=prompt[:, :3].clone())
    assert _row_equals(out, 0, single), (out.tolist(), single.tolist())
