"""The chunk decode kernel (csrc/decode_chunk_kernels.h through flash_attn_with_kvcache_chunk) per element against the fp64 restatement
and the derived bound of tests/decode_chunk_fp64.py at its structural edges, its append and bounds behaviour, determinism and graph
replay, M one-row launches against one chunk launch; and the model level: `decode_chunk` against the full decoder forward and
`generate(decoder_input_ids=...)` against the unprompted run, step-by-step prefill, and the logits processors.

CASES and `inputs` are module-level and CPU-only: tests/test_decode_chunk_cpu.py imports them and proves, without a GPU, that the
bound tells every applicable mutant of decode_chunk_fp64.MUTANTS from the truth on these very inputs.
"""
import math
import zlib

import pytest
import torch

import decode_chunk_fp64 as C
import decode_fp64 as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
TQ = C.CHUNK_TQ
B_, H_ = 2, 2
GUARD = 3          # guard rows on either side of every batch element's cache rows
SCALE = 0.125


def _name(dtype):
    return str(dtype)[6:]


def _build_cases():
    out = []

    def add(kind, D, dtype, M, lens, cap, append=True, causal=True, R=16, splits=1):
        out.append(dict(kind=kind, D=D, dtype=dtype, M=M, lens=lens, cap=cap, append=append, causal=causal, R=R, splits=splits,
                        id=f"{kind}-D{D}-{_name(dtype)}-M{M}-lens{lens}-s{splits}".replace(" ", "")))

    for D in (64, 128):
        P = F.wg_pass(D)   # rows one workgroup takes per step: G * U
        for dtype in (BF16, F16):
            # every M around the tile, with len + M one below, at and one above a multiple of the workgroup pass
            for M in (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 1):
                for d in (-1, 0, 1):
                    add("edge", D, dtype, M, [P + d - M, 2 * P + d - M], 2 * P + 8)
            for s in (1, 2, 3):   # L = 163 and 295: neither divisible by 2 or 3
                add("split", D, dtype, TQ + 1, [163 - TQ - 1, 295 - TQ - 1], 300, splits=s)
            add("empty", D, dtype, TQ + 1, [0, 7], 24, splits=2)
            add("radius1", D, dtype, TQ + 1, [40, 100], 110, R=1)
            add("cross", D, dtype, TQ + 1, [33, 140], 150, append=False, causal=False, R=0)
            add("cross", D, dtype, TQ + 1, None, 150, append=False, causal=False, R=0, splits=2)
            add("cross-bias", D, dtype, TQ - 1, [33, 140], 150, append=False, causal=False, R=16)
            add("masked", D, dtype, 2 * TQ + 1, [3, 6], 16, append=False, causal=True, splits=2)   # M > L: leading rows see nothing
            add("overflow", D, dtype, TQ + 1, [38, 40], 40)                 # len + M > capacity; len == capacity
            add("overflow", D, dtype, TQ + 1, [45, -3], 40, splits=2)       # len > capacity; a negative length
    return out


CASES = _build_cases()


def inputs(case):
    """the launch of `case`: CPU tensors q, kc, vc, kn, vn, rpe (an i.i.d. table: every entry distinct, so a wrong index shows)"""
    g = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    D, dtype, M, cap = case["D"], case["dtype"], case["M"], case["cap"]
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    ln = dict(q=rn(B_, M, H_, D), kc=rn(B_, cap, H_, D), vc=rn(B_, cap, H_, D), kn=None, vn=None, rpe=None)
    if case["append"]:
        ln["kn"], ln["vn"] = rn(B_, M, H_, D), rn(B_, M, H_, D)
    if case["R"]:
        ln["rpe"] = torch.randn(H_, 2 * case["R"] + 1, generator=g)
    return ln


def reference(case, ln, mutant=None):
    return C.chunk_ref(ln["q"], ln["kc"], ln["vc"], ln["kn"], ln["vn"], case["lens"], SCALE, case["causal"], ln["rpe"], case["R"],
                       splits=case["splits"], mutant=mutant)


# ------------------------------------------------------------------------------------------------------------------- the GPU side
def _bits(t):
    return t.view(torch.int16) if t.dtype != torch.float32 else t.view(torch.int32)


def _guarded(t, fill=None):
    """a cache on the device inside a buffer with GUARD rows before and after each batch element: (the view, the buffer)"""
    B, cap, H, D = t.shape
    g = torch.Generator().manual_seed(cap)
    buf = torch.randn(B, cap + 2 * GUARD, H, D, generator=g).to(t.dtype).to(DEV)
    if fill is not None:
        buf.fill_(fill)
    view = buf[:, GUARD:GUARD + cap]
    view.copy_(t)
    return view, buf


def _run(case, ln, kc, vc, lens):
    from flasht5_amd import flash_attn_with_kvcache_chunk
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    o, lse = flash_attn_with_kvcache_chunk(dev(ln["q"]), kc, vc, dev(ln["kn"]), dev(ln["vn"]), lens, SCALE, case["causal"], dev(ln["rpe"]),
                                           case["R"], return_lse=True, num_splits=case["splits"])
    torch.cuda.synchronize()
    return o, lse


def _lens(case):
    return None if case["lens"] is None else torch.tensor(case["lens"], dtype=torch.int32, device=DEV)


def _assert_within(o, lse, ref, case, what):
    bo, bl = C.chunk_bound(ref, case["dtype"], case["D"], case["splits"])
    oc, lc = o.cpu(), lse.cpu().transpose(1, 2)   # (B, H, M) -> (B, M, H)
    ro, rl, same = C.ratios(oc, lc, ref, bo, bl)
    print(f"[decode-chunk] {what}: worst err / bound o {ro:.3f} lse {rl:.3f}")
    assert same, f"{what}: finiteness pattern of lse: got {lc.tolist()} want {ref['lse'].tolist()}"
    assert ro <= 1.0 and rl <= 1.0, f"{what}: err / bound o {ro:.3f} lse {rl:.3f}"
    return ro, rl


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_chunk_within_the_fp64_bound(case):
    ln = inputs(case)
    ref = reference(case, ln)
    (kc, kbuf), (vc, vbuf) = _guarded(ln["kc"]), _guarded(ln["vc"])
    k0, v0 = kbuf.clone(), vbuf.clone()
    lens = _lens(case)
    o, lse = _run(case, ln, kc, vc, lens)
    assert o.shape == (B_, case["M"], H_, case["D"]) and lse.shape == (B_, H_, case["M"])
    _assert_within(o, lse, ref, case, case["id"])
    # the caches: the appended rows bit for bit at len_b .. L_b - 1, every other element as it was -- rows past L_b, the other batch
    # element and the guard rows included; the lengths are never written
    wk, wv = k0.clone(), v0.clone()
    wk[:, GUARD:GUARD + case["cap"]] = ref["kc"].to(DEV)
    wv[:, GUARD:GUARD + case["cap"]] = ref["vc"].to(DEV)
    assert torch.equal(_bits(kbuf), _bits(wk)) and torch.equal(_bits(vbuf), _bits(wv)), f"{case['id']}: cache image"
    if case["append"]:
        for b in range(B_):
            n = max(0, min(case["lens"][b], case["cap"]))
            assert ref["L"][b] == min(case["cap"], n + case["M"])
            assert torch.equal(_bits(kc[b, n:ref["L"][b]]), _bits(ln["kn"][b, :ref["L"][b] - n].to(DEV)))
    if lens is not None:
        assert torch.equal(lens.cpu(), torch.tensor(case["lens"], dtype=torch.int32)), "cache_seqlens written"
    kbuf.copy_(k0), vbuf.copy_(v0)
    o2, lse2 = _run(case, ln, kc, vc, lens)
    assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(lse), _bits(lse2)), f"{case['id']}: a second run gives other bits"


def test_masked_rows_are_zero_with_lse_minus_inf():
    case = next(c for c in CASES if c["kind"] == "masked")
    ln = inputs(case)
    o, lse = _run(case, ln, ln["kc"].to(DEV), ln["vc"].to(DEV), _lens(case))
    for b, L in enumerate(case["lens"]):
        dead = case["M"] - L   # rows 0 .. M - L - 1 sit at negative positions
        assert dead > 0 and bool((o[b, :dead] == 0).all()) and bool((lse[b, :, :dead] == -math.inf).all())
        assert bool(torch.isfinite(lse[b, :, dead:]).all())


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] in ("overflow", "empty", "cross", "masked") and c["dtype"] == BF16],
                         ids=lambda c: c["id"])
def test_poisoned_rows_beyond_the_length_never_reach_o(case):
    """NaN in every cache row at or beyond len_b (the rows an append overwrites included: a new row is read from k_new / v_new) and
    in the guard rows"""
    ln = inputs(case)
    ref = reference(case, ln)
    (kc, kbuf), (vc, vbuf) = _guarded(ln["kc"], math.nan), _guarded(ln["vc"], math.nan)
    for b in range(B_):
        n = case["cap"] if case["lens"] is None else max(0, min(case["lens"][b], case["cap"]))
        kc[b, n:], vc[b, n:] = math.nan, math.nan
    o, lse = _run(case, ln, kc, vc, _lens(case))
    assert bool(torch.isfinite(o).all())
    _assert_within(o, lse, ref, case, case["id"] + " (poisoned)")


def test_graph_replay_after_the_lengths_grow_equals_eager():
    from flasht5_amd import flash_attn_with_kvcache_chunk
    g = torch.Generator().manual_seed(5)
    B, M, H, D, cap = 2, TQ + 1, 2, 64, 200
    rn = lambda *s: torch.randn(*s, generator=g).to(BF16).to(DEV)  # noqa: E731
    q, kn, vn, kc, vc = rn(B, M, H, D), rn(B, M, H, D), rn(B, M, H, D), rn(B, cap, H, D), rn(B, cap, H, D)
    rpe = torch.randn(H, 33, generator=g).to(DEV)
    lens = torch.tensor([120, 7], dtype=torch.int32, device=DEV)
    call = lambda k_, v_: flash_attn_with_kvcache_chunk(q, k_, v_, kn, vn, lens, SCALE, True, rpe, 16, return_lse=True, num_splits=2)  # noqa: E731
    call(kc.clone(), vc.clone())  # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = call(kc, vc)
    graph.replay()
    torch.cuda.synchronize()
    ks, vs = kc.clone(), vc.clone()
    lens.add_(M)   # on the device
    graph.replay()
    torch.cuda.synchronize()
    oe, le = call(ks, vs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o), _bits(oe)) and torch.equal(_bits(lse), _bits(le))
    assert torch.equal(_bits(kc), _bits(ks)) and torch.equal(_bits(vc), _bits(vs))
    assert torch.equal(_bits(kc[0, 125:130]), _bits(kn[0])) and torch.equal(_bits(kc[1, 7:12]), _bits(kn[1]))
    del graph


@pytest.mark.parametrize("D, dtype", [(64, BF16), (128, F16)])
def test_one_row_launches_and_one_chunk_agree(D, dtype):
    """M sequential one-row launches and one chunk launch lie within their own bounds of the same reference, and leave the same caches"""
    from flasht5_amd import flash_attn_with_kvcache
    case = dict(id=f"seq-D{D}", D=D, dtype=dtype, M=2 * TQ + 1, lens=[130, 61], cap=150, append=True, causal=True, R=16, splits=2)
    ln = inputs(case)
    ref = reference(case, ln)
    kc, vc = ln["kc"].to(DEV), ln["vc"].to(DEV)
    o, lse = _run(case, ln, kc, vc, _lens(case))
    _assert_within(o, lse, ref, case, case["id"] + " chunk")
    k1, v1 = ln["kc"].to(DEV), ln["vc"].to(DEV)
    rpe = ln["rpe"].to(DEV)
    for i in range(case["M"]):
        li = [n + i for n in case["lens"]]
        r1 = F.decode_ref(ln["q"][:, i:i + 1], k1.cpu(), v1.cpu(), ln["kn"][:, i:i + 1], ln["vn"][:, i:i + 1], li, SCALE, ln["rpe"], 16)
        o1, l1 = flash_attn_with_kvcache(ln["q"][:, i:i + 1].to(DEV), k1, v1, ln["kn"][:, i:i + 1].to(DEV), ln["vn"][:, i:i + 1].to(DEV),
                                         torch.tensor(li, dtype=torch.int32, device=DEV), SCALE, rpe, 16, return_lse=True, num_splits=2)
        assert float((r1["o"] - ref["o"][:, i]).abs().max()) <= 1e-12   # (the same reference)
        assert F.within(o1[:, 0].cpu(), l1[:, :, 0].cpu(), r1, *F.decode_bound(r1, dtype, D, 2)), f"one-row launch {i}"
    assert torch.equal(_bits(kc), _bits(k1)) and torch.equal(_bits(vc), _bits(v1))


def test_python_rejections_on_the_gpu():
    from flasht5_amd import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk
    q = torch.zeros(2, 3, 4, 64, dtype=BF16, device=DEV)
    kc = torch.zeros(2, 16, 4, 64, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="GPU"):
        flash_attn_with_kvcache_chunk(q, kc, kc.cpu())
    with pytest.raises(ValueError, match=r"\(B, 1, H, D\)"):   # (the one-row operator keeps refusing chunks)
        flash_attn_with_kvcache(q, kc, kc)
    o64 = flash_attn_with_kvcache_chunk(q, kc, kc.clone(), q, q, torch.tensor([3, 5]), causal=True)
    o32 = flash_attn_with_kvcache_chunk(q, kc, kc.clone(), q, q, torch.tensor([3, 5], dtype=torch.int32, device=DEV), causal=True)
    assert torch.equal(o64, o32)
    lens = torch.tensor([3, 5], device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="graph capture"):
        with torch.cuda.graph(graph):
            flash_attn_with_kvcache_chunk(q, kc, kc, q, q, lens)
    del graph


# ---------------------------------------------------------------------------------------------------------------- model level
def _model(kind, seed=0, vocab=512):
    """test_decode_gpu.py's small model, restated"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(attention_type="fat5_rpe")
    if kind == "t5_triton":
        kw = dict(attention_type="triton")
    elif kind == "rope":
        kw = dict(position_encoding_type="RoPE")
    elif kind == "xpos":
        kw = dict(position_encoding_type="RoPE", rotary_scale_base=512.0, attention_type="triton")
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


LOGIT_BOUND = 0.02  # the one-row step's bound (tests/test_decode_gpu.py; measured worst there 1.03e-2): the same GEMMs at other row counts


def _full_logits(model, ids, dec_in):
    enc = model.encoder(ids)
    return model.lm_head(model.decoder(dec_in, encoder_hidden_states=enc)).float()


def _rel_err(lg, full):
    return ((lg.float() - full).abs().amax(-1) / full.abs().amax(-1).clamp(min=1)).max().item()


@pytest.mark.parametrize("kind", ["t5_rpe", "t5_triton", "rope", "xpos"])
def test_decode_chunk_matches_full_forward(kind):
    m = _model(kind).to(DEV).bfloat16()
    g = torch.Generator().manual_seed(7)
    B, L_enc, T = 3, 40, 20
    V = m.config.vocab_size
    ids = torch.randint(2, V, (B, L_enc), generator=g).to(DEV)
    dec_in = m._shift_right(torch.randint(2, V, (B, T), generator=g).to(DEV))
    with torch.no_grad():
        full = _full_logits(m, ids, dec_in)
        state = m.init_decode_state(ids, max_length=T)
        worst = _rel_err(m.decode_step(state, dec_in[:, 0]), full[:, 0])          # a mixed schedule: 1, 5, 4 and 10 tokens
        t = 1
        for M in (5, 4, 10):
            lg = m.decode_chunk(state, dec_in[:, t:t + M])
            assert lg.shape == (B, M, V)
            worst = max(worst, _rel_err(lg, full[:, t:t + M]))
            t += M
        assert state.steps == T and state.cache_seqlens.tolist() == [T] * B
        with pytest.raises(ValueError, match="the chunk brings 2"):
            m.decode_chunk(state, dec_in[:, :2])                                   # 20 + 2 > 21 positions: refused on the host
        state = m.init_decode_state(ids, max_length=T)
        assert m.decode_chunk(state, dec_in[:, :6], logits="none") is None
        last = m.decode_chunk(state, dec_in[:, 6:], logits="last")
        assert last.shape == (B, V)
        worst = max(worst, _rel_err(last, full[:, -1]))
    print(f"[decode-chunk] {kind}: worst relative logit error {worst:.3e}")
    assert worst <= LOGIT_BOUND, f"{kind}: worst relative logit error {worst:.3e}"


def _decisive(m, seed):
    """test_decode_gpu.py's construction: lm_head row sigma(t) is token t's embedding, so the next token is sigma(current token)"""
    V = m.config.vocab_size
    sigma = torch.randperm(V, generator=torch.Generator().manual_seed(1000 + seed))
    with torch.no_grad():
        m.lm_head.weight[sigma] = m.shared.weight
    return sigma


def _decisive_run(kind, T=16):
    """a decisive model, inputs and its unprompted output whose first five columns hold no EOS (the first seed where that is so)"""
    for seed in range(8):
        m = _model(kind, seed=seed).to(DEV).bfloat16()
        sigma = _decisive(m, seed)
        ids = torch.randint(2, m.config.vocab_size, (4, 33), generator=torch.Generator().manual_seed(100 + seed)).to(DEV)
        out = m.generate(ids, max_length=T)
        if out.shape[1] > 6 and not bool((out[:, :5] == 1).any()):
            return m, sigma, ids, out
    raise AssertionError("no seed gives five EOS-free columns")


@pytest.mark.parametrize("kind", ["t5_rpe", "rope"])
def test_generate_with_a_prompt_continues_the_unprompted_run(kind):
    T = 16
    m, _, ids, out = _decisive_run(kind, T)
    for P in (1, 2, 5):
        got = m.generate(ids, max_length=T - (P - 1), decoder_input_ids=out[:, :P].clone())
        assert torch.equal(got, out), (kind, P)
        got = m.generate(ids, max_length=T - (P - 1), decoder_input_ids=out[:, :P].clone(), graph=True)
        assert torch.equal(got, out), (kind, P, "graph")


def test_prompt_of_one_token_makes_no_chunk_launch(monkeypatch):
    from flasht5_amd import decode
    m, _, ids, out = _decisive_run("t5_rpe")
    calls = []
    real = decode.flash_attn_with_kvcache_chunk
    monkeypatch.setattr(decode, "flash_attn_with_kvcache_chunk", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m.generate(ids, max_length=8, decoder_input_ids=out[:, :1].clone())
    assert not calls
    m.generate(ids, max_length=8, decoder_input_ids=out[:, :3].clone())
    assert len(calls) == 2 * len(m.decoder.block)  # (one prefill step: self- and cross-attention of every block)


def test_sampling_after_chunk_prefill_draws_the_step_prefill_tokens():
    """a sampled run prefilled by one chunk against one prefilled by P - 1 decode_step calls, per row up to the first step whose
    top-two margin is within twice the measured logit error between the two paths (test_generate_matches_recompute's rule)"""
    from flasht5_amd.sampling import sample_logits
    T, P, seed, temp, top_k = 12, 5, 4321, 0.5, 50
    m, _, ids, out = _decisive_run("t5_rpe")
    prompt = out[:, :P].clone()
    got = m.generate(ids, max_length=T, decoder_input_ids=prompt, do_sample=True, temperature=temp, top_k=top_k, seed=seed)
    with torch.no_grad():
        a = m.init_decode_state(ids, max_length=T, prompt_length=P)     # prefilled step by step
        for t in range(P - 1):
            m.decode_step(a, prompt[:, t])
        b = m.init_decode_state(ids, max_length=T, prompt_length=P)     # prefilled by one chunk, then teacher-forced along a's tokens
        m.decode_chunk(b, prompt[:, :P - 1], logits="none")
        tok, toks, margins, err = prompt[:, P - 1].clone(), [], [], 0.0
        for _ in range(T):
            raw = m.decode_step(a, tok)
            la, lb = raw.float(), m.decode_step(b, tok).float()
            err = max(err, _rel_err(lb, la))
            top = la.topk(2, -1).values
            margins.append(((top[:, 0] - top[:, 1]) / la.abs().amax(-1).clamp(min=1)).cpu())
            tok = sample_logits(raw, temp, top_k, 1.0, seed=seed, offsets=a.cache_seqlens)
            toks.append(tok.cpu())
    want, margins = torch.stack(toks, 1), torch.stack(margins, 1)
    print(f"[decode-chunk] sampling: logit error between the two prefills {err:.3e}")
    assert err <= LOGIT_BOUND
    compared = 0
    for r in range(ids.shape[0]):
        low = (margins[r] <= 2 * err).nonzero()
        n = int(low[0]) if len(low) else T
        eos = (want[r, :n] == 1).nonzero()
        n = min(n, int(eos[0]) + 1 if len(eos) else n, got.shape[1] - P - 1)   # (the ending rewrites the last column)
        compared += n
        assert torch.equal(got[r, P:P + n].cpu(), want[r, :n]), (r, n)
    assert compared >= ids.shape[0] * 4, f"only {compared} row-steps were decisive enough to compare"


def test_processors_see_the_prompt():
    m, sigma, ids, _ = _decisive_run("t5_rpe")
    B = ids.shape[0]
    inv = torch.argsort(sigma)
    # no_repeat_ngram_size=2: the prompt ends in a, after holding the bigram (a, sigma(a)): the model's choice sigma(a) is banned
    a = torch.tensor([t for t in range(2, 40) if int(sigma[t]) > 1][:B])
    prompt = torch.stack([torch.zeros(B, dtype=torch.long), a, sigma[a], a], 1).to(DEV)
    plain = m.generate(ids, max_length=10, decoder_input_ids=prompt)
    assert torch.equal(plain[:, 4].cpu(), sigma[a])   # (without the processor the bigram is repeated)
    out = m.generate(ids, max_length=10, decoder_input_ids=prompt, no_repeat_ngram_size=2)
    assert torch.equal(out[:, :4], prompt)
    for r in range(B):
        row = out[r].tolist()
        end = row.index(1) if 1 in row else len(row)
        grams = list(zip(row[:end], row[1:end]))
        assert len(grams) == len(set(grams)), (r, row)
    # min_length: the prompt ends in the token whose successor is EOS; the prompt's columns count towards the length
    e = int(inv[1])
    prompt = torch.tensor([[0, 5, e]] * B).to(DEV)
    assert bool((m.generate(ids, max_length=6, decoder_input_ids=prompt)[:, 3] == 1).all())
    assert bool((m.generate(ids, max_length=6, decoder_input_ids=prompt, min_length=3)[:, 3] == 1).all())   # 3 columns are there already
    out = m.generate(ids, max_length=6, decoder_input_ids=prompt, min_length=5)
    assert not bool((out[:, 3:5] == 1).any()), out.tolist()
