"""Which device entry points every mode of `generate` calls, and in what order.

The public entry points of the decode path are wrapped (never replaced: each wrapper records and calls through), one eager
`generate(graph=False)` runs per mode on a small model, and the recorded sequence must equal the one written out here as a function
of the decoder layers, the prompt length P, gamma and the number of steps or rounds the call ran (the output's width, or
`return_stats`).  A record is (entry point, shape of its first tensor argument, the optional arguments -- those whose default is
None -- that were given).  The tokens themselves are other tests' business."""
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
V, H, D, L_ENC, LAYERS, DRAFT_LAYERS, T, GAMMA = 128, 2, 64, 12, 2, 1, 4, 2

KV, CHUNK, QUANT, SAMPLE, PROC, BEAM, ACCEPT, LOOKUP = (
    "flash_attn_with_kvcache", "flash_attn_with_kvcache_chunk", "quantize_kv", "sample_logits", "process_logits", "beam_step",
    "speculative_accept", "prompt_lookup_draft")


def _model(rope=False, decoder_layers=LAYERS, seed=0):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(position_encoding_type="RoPE") if rope else dict(attention_type="fat5_rpe")
    c = FAT5Config(vocab_size=V, d_model=64, d_kv=D, d_ff=128, num_heads=H, num_layers=1, num_decoder_layers=decoder_layers,
                   relative_attention_max_distance=64, max_sequence_length=64, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c).to(DEV).bfloat16().eval()


@pytest.fixture(scope="module")
def models():
    return dict(t5=_model(), rope=_model(rope=True), draft=_model(decoder_layers=DRAFT_LAYERS, seed=1))


def _ids(B):
    return torch.randint(2, V, (B, L_ENC), generator=torch.Generator().manual_seed(5)).to(DEV)


@pytest.fixture
def trace(monkeypatch):
    """the recording wrappers around the eight entry points -> the list they append to"""
    from flasht5_amd import beam, decode, logits_process, prompt_lookup, sampling, speculative
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

    for module, name in ((decode, KV), (decode, CHUNK), (decode, QUANT), (sampling, SAMPLE), (logits_process, PROC), (beam, BEAM),
                         (speculative, ACCEPT), (prompt_lookup, LOOKUP)):
        wrap(module, name)
    return calls


# ------------------------------------------------------------------------------------------------------- the expected sequences
def _attention(name, rows, M, layers, self_extra=(), cross_extra=(), both=(), rope=False):
    """one pass through `layers` decoder blocks: per block the self-attention launch (it appends: k, v, the lengths; the T5 bias
    unless RoPE), then the cross-attention launch (no append, no bias)"""
    self_opts = {"k", "v", "cache_seqlens", "softmax_scale"} | (set() if rope else {"rpe1d"}) | set(self_extra) | set(both)
    cross_opts = {"softmax_scale"} | set(cross_extra) | set(both)
    return [(name, (rows, M, H, D), frozenset(self_opts)), (name, (rows, M, H, D), frozenset(cross_opts))] * layers


def _step(rows, layers=LAYERS, **kw):
    return _attention(KV, rows, 1, layers, **kw)


def _chunk(rows, M, layers=LAYERS, **kw):
    return _attention(CHUNK, rows, M, layers, **kw)


def _call(name, shape, *optional):
    return [(name, tuple(shape), frozenset(optional))]


def _check(calls, expected):
    assert len(calls) == len(expected), (len(calls), len(expected), calls)
    for i, (got, want) in enumerate(zip(calls, expected)):
        assert got == want, (i, got, want)


# ------------------------------------------------------------------------------------------------------------------ plain loop
def test_greedy(models, trace):
    out = models["t5"].generate(_ids(2), max_length=T)
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    _check(trace, _step(2) * steps)


def test_greedy_with_a_processor(models, trace):
    out = models["t5"].generate(_ids(2), max_length=T, repetition_penalty=1.3)
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    _check(trace, (_step(2) + _call(PROC, (2, V), "max_new_tokens")) * steps)


def test_sampled(models, trace):
    out = models["t5"].generate(_ids(2), max_length=T, do_sample=True, top_k=20, seed=11)
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    _check(trace, (_step(2) + _call(SAMPLE, (2, V), "offsets")) * steps)


@pytest.mark.parametrize("processor", [False, True])
def test_beams(models, trace, processor):
    k = 2
    out = models["t5"].generate(_ids(2), max_length=T, num_beams=k, **(dict(repetition_penalty=1.3) if processor else {}))
    # (the width is the longest returned hypothesis, which may end before the search does: the steps are the beam steps made)
    steps = sum(1 for c in trace if c[0] == BEAM)
    assert 1 <= out.shape[1] - 1 <= steps <= T
    step = _step(2 * k, self_extra=("cache_row_batch",), cross_extra=("cache_batch_idx",))
    if processor:
        step = step + _call(PROC, (2 * k, V), "max_new_tokens")
    _check(trace, (step + _call(BEAM, (2 * k, V))) * steps)


def test_rope_greedy(models, trace):
    out = models["rope"].generate(_ids(1), max_length=T)
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    _check(trace, _step(1, rope=True) * steps)


# ------------------------------------------------------------------------------------------------- prompts, padding, FP8 caches
def test_decoder_prompt(models, trace):
    P = 3
    prompt = torch.tensor([[0, 7, 9], [0, 23, 5]], device=DEV)
    out = models["t5"].generate(_ids(2), max_length=T, decoder_input_ids=prompt)
    steps = out.shape[1] - P
    assert 1 <= steps <= T and torch.equal(out[:, :P], prompt)
    _check(trace, _chunk(2, P - 1) + _step(2) * steps)


def test_ragged_prompt(models, trace):
    P = 3
    prompt = torch.tensor([[0, 0, 0], [0, 23, 5]], device=DEV)
    mask = torch.tensor([[1, 0, 0], [1, 1, 1]], device=DEV)
    out = models["t5"].generate(_ids(2), max_length=T, decoder_input_ids=prompt, decoder_attention_mask=mask)
    steps = out.shape[1] - P
    assert 1 <= steps <= T
    # (one chunk step over the whole prompts gives every row's first token: a step without a one-row launch)
    _check(trace, _chunk(2, P, both=("chunk_seqlens",)) + _step(2) * (steps - 1))


def test_padded_encoder_input(models, trace):
    mask = torch.ones((2, L_ENC), dtype=torch.long, device=DEV)
    mask[1, 7:] = 0
    out = models["t5"].generate(_ids(2), attention_mask=mask, max_length=T)
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    _check(trace, _step(2, cross_extra=("cache_seqlens",)) * steps)


def test_fp8_caches(models, trace):
    out = models["t5"].generate(_ids(2), max_length=T, kv_cache_dtype="fp8")
    steps = out.shape[1] - 1
    assert 1 <= steps <= T
    # (per decoder layer the encoder's K, then its V, quantised once; every launch of a step reads bytes and scales)
    _check(trace, _call(QUANT, (2, L_ENC, H, D)) * (2 * LAYERS) + _step(2, both=("k_scale", "v_scale")) * steps)


# ----------------------------------------------------------------------------------------------------------- speculative rounds
@pytest.mark.parametrize("sampled", [False, True])
def test_assistant(models, trace, sampled):
    kw = dict(do_sample=True, top_k=20, seed=11) if sampled else {}
    out, stats = models["t5"].generate(_ids(2), max_length=T, assistant_model=models["draft"], num_assistant_tokens=GAMMA,
                                       return_stats=True, **kw)
    rounds = stats["rounds"]
    assert 1 <= rounds <= T and 2 <= out.shape[1] <= T + 1
    draft_step = _step(2, DRAFT_LAYERS)
    if sampled:   # (gamma draws from the drafter's logits; the last draft step only appends)
        draft = (draft_step + _call(SAMPLE, (2, V), "offsets")) * GAMMA + draft_step
        accept = _call(ACCEPT, (2, GAMMA + 1, V), "draft_seqlens", "sampling", "draft_logits")
    else:
        draft = draft_step * (GAMMA + 1)
        accept = _call(ACCEPT, (2, GAMMA + 1, V), "draft_seqlens")
    _check(trace, (draft + _chunk(2, GAMMA + 1) + accept) * rounds)


@pytest.mark.parametrize("sampled", [False, True])
def test_prompt_lookup(models, trace, sampled):
    kw = dict(do_sample=True, top_k=20, seed=11) if sampled else {}
    out, stats = models["t5"].generate(_ids(2), max_length=T, prompt_lookup_num_tokens=GAMMA, return_stats=True, **kw)
    rounds = stats["rounds"]
    assert 1 <= rounds <= T and 2 <= out.shape[1] <= T + 1
    accept = _call(ACCEPT, (2, GAMMA + 1, V), *(("sampling",) if sampled else ()))
    _check(trace, (_call(LOOKUP, (2, L_ENC), "vocab_size", "out") + _chunk(2, GAMMA + 1) + accept) * rounds)
