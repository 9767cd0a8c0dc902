"""GPU tests of KV-cached decoding: the split-KV decode kernel (fat5_attn_decode through flash_attn_with_kvcache) against an eager
fp64 restatement, its append, its bounds (NaN past the length, lengths past the capacity inside guard bands), cross-checks against
the existing attention kernels, determinism under graph replay, a cache of more than 2^31 elements; and the model level:
`decode_step` against the full decoder forward (teacher forcing), `generate` against a restatement of the reference's recompute
loop, and graph mode against eager mode.

Tolerance (DESIGN section 2 style): the kernel accumulates in fp32 and rounds o once to the storage dtype, so
    |o - o_fp64| <= (1e-3 + half-ulp(dtype)) * max(1, max |o_fp64|),   |lse - lse_fp64| <= 1e-4 * max(1, |lse_fp64|).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _ref(q, kc, vc, kn, vn, lens, scale, rpe1d, R):
    """fp64 restatement: per batch element the clamped length, the appended row, the bottom-right aligned T5 bias"""
    B, _, H, D = q.shape
    cap = kc.shape[1]
    o = torch.zeros(B, H, D, dtype=torch.float64)
    lse = torch.full((B, H), -math.inf, dtype=torch.float64)
    for b in range(B):
        n = max(0, min(int(lens[b]), cap))
        k, v = kc[b, :n].double().cpu(), vc[b, :n].double().cpu()  # (n, H, D)
        if kn is not None and n < cap:
            k = torch.cat([k, kn[b].double().cpu().unsqueeze(0)], 0)
            v = torch.cat([v, vn[b].double().cpu().unsqueeze(0)], 0)
        L = k.shape[0]
        if L == 0:
            continue
        s = torch.einsum("hd,lhd->hl", q[b, 0].double().cpu(), k) * scale
        if rpe1d is not None:
            rel = (torch.arange(L) - (L - 1)).clamp(-R, R) + R
            s = s + rpe1d.double().cpu()[:, rel]
        lse[b] = torch.logsumexp(s, -1)
        o[b] = torch.einsum("hl,lhd->hd", torch.softmax(s, -1), v)
    return o, lse


def _rpe(H, R, decoder, g):
    t = torch.randn(32, H, generator=g) * 0.5
    from flasht5_amd.positional_encoding import rpe1d_from_table
    return rpe1d_from_table(t, bidirectional=not decoder, num_buckets=32, max_distance=R).to(DEV)


def _cache(B, cap, H, D, dtype, layout, g):
    if layout == "bhld":
        return (torch.randn(B, H, cap, D, generator=g).to(dtype).to(DEV).transpose(1, 2),
                torch.randn(B, H, cap, D, generator=g).to(dtype).to(DEV).transpose(1, 2))
    return torch.randn(B, cap, H, D, generator=g).to(dtype).to(DEV), torch.randn(B, cap, H, D, generator=g).to(dtype).to(DEV)


def _check(o, lse, ref_o, ref_lse, dtype, what):
    o = o[:, 0].double().cpu()
    bound = (1e-3 + HALF_ULP[dtype]) * max(1.0, ref_o.abs().max().item())
    err = (o - ref_o).abs().max().item()
    assert torch.isfinite(o).all() and err <= bound, f"{what}: o error {err:.3e} > {bound:.3e}"
    if lse is not None:
        lse = lse[:, :, 0].double().cpu()
        fin = torch.isfinite(ref_lse)
        assert torch.equal(torch.isfinite(lse), fin), what
        e = ((lse - ref_lse).abs()[fin] / ref_lse.abs()[fin].clamp(min=1)).max().item() if fin.any() else 0.0
        assert e <= 1e-4, f"{what}: lse error {e:.3e}"


R_T5 = 128
# lengths (before the append): empty, 1, 7, around a 128-row workgroup pass and a split boundary, around R, 1024, 4097
LEN_SETS = [[0, 1, 7], [127, 128, 129], [R_T5 - 1, R_T5 + 1, 255], [1024, 3, 256], [4097, 0, 1000]]


def _cases():
    out = []
    for D in (64, 128):
        for dtype in (torch.bfloat16, torch.float16):
            for B, H in ((1, 6), (3, 12), (16, 32)):
                for bias in ("none", "enc", "dec"):
                    out.append((D, dtype, B, H, bias))
    return out


@pytest.mark.parametrize("D, dtype, B, H, bias", _cases())
@pytest.mark.parametrize("append", [True, False])
def test_decode_vs_fp64(D, dtype, B, H, bias, append):
    g = torch.Generator().manual_seed(D * 7 + B * 3 + H + len(bias) + append)
    layout = "bhld" if (B + H) % 2 else "blhd"
    rpe = None if bias == "none" else _rpe(H, R_T5, bias == "dec", g)
    lens_all = [l for s in LEN_SETS for l in s] if B <= 3 else [0, 1, 7, 127, 128, 129, 255, 1000] * 2
    cap = max(lens_all) + 2
    kc, vc = _cache(B, cap, H, D, dtype, layout, g)
    kc0, vc0 = kc.clone(), vc.clone()
    from flasht5_amd import flash_attn_with_kvcache
    for i in range(0, len(lens_all), B):
        lens = (lens_all[i:i + B] + [5] * B)[:B]
        q = torch.randn(B, 1, H, D, generator=g).to(dtype).to(DEV)
        kn = torch.randn(B, 1, H, D, generator=g).to(dtype).to(DEV) if append else None
        vn = torch.randn(B, 1, H, D, generator=g).to(dtype).to(DEV) if append else None
        ro, rl = _ref(q, kc0, vc0, kn[:, 0] if append else None, vn[:, 0] if append else None, lens, 0.125, rpe, R_T5)
        for splits in (0, 3):
            kc.copy_(kc0), vc.copy_(vc0)
            lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
            o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, lt, 0.125, rpe, R_T5 if rpe is not None else 0, return_lse=True,
                                             num_splits=splits)
            torch.cuda.synchronize()
            _check(o, lse, ro, rl, dtype, f"lens {lens} splits {splits} layout {layout}")
            assert torch.equal(lt.cpu(), torch.tensor(lens, dtype=torch.int32))  # (never written)


def test_append_lands_bit_exact_and_nothing_else_changes():
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(1)
    B, H, D, cap = 4, 12, 64, 300
    for layout in ("blhd", "bhld"):
        kc, vc = _cache(B, cap, H, D, torch.bfloat16, layout, g)
        kn, vn = (torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV) for _ in range(2))
        q = torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV)
        lens = [0, 17, 128, 299]
        k0, v0 = kc.clone(), vc.clone()
        flash_attn_with_kvcache(q, kc, vc, kn, vn, torch.tensor(lens, dtype=torch.int32, device=DEV), num_splits=4)
        torch.cuda.synchronize()
        for b, n in enumerate(lens):
            k0[b, n], v0[b, n] = kn[b, 0], vn[b, 0]
        assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16))


def test_never_reads_past_the_length():
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(2)
    B, H, D, cap = 3, 12, 128, 700
    rpe = _rpe(H, R_T5, True, g)
    kc, vc = _cache(B, cap, H, D, torch.bfloat16, "blhd", g)
    q, kn, vn = (torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV) for _ in range(3))
    lens = [5, 333, 690]
    for b, n in enumerate(lens):
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    k0, v0 = kc.clone(), vc.clone()
    for splits in (0, 1, 7):
        kc.copy_(k0), vc.copy_(v0)
        o, lse = flash_attn_with_kvcache(q, kc, vc, kn, vn, torch.tensor(lens, dtype=torch.int32, device=DEV), 0.1, rpe, R_T5,
                                         return_lse=True, num_splits=splits)
        ro, rl = _ref(q, k0, v0, kn[:, 0], vn[:, 0], lens, 0.1, rpe, R_T5)
        _check(o, lse, ro, rl, torch.bfloat16, f"NaN past the length, splits {splits}")
        kc.copy_(k0), vc.copy_(v0)
        o = flash_attn_with_kvcache(q, kc, vc, None, None, torch.tensor(lens, dtype=torch.int32, device=DEV), 0.1, rpe, R_T5,
                                    num_splits=splits)
        ro, rl = _ref(q, k0, v0, None, None, lens, 0.1, rpe, R_T5)
        _check(o, None, ro, rl, torch.bfloat16, f"NaN past the length, no append, splits {splits}")


def test_lengths_past_capacity_stay_inside_the_cache():
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(3)
    B, H, D, cap, guard = 4, 6, 64, 200, 4096
    per = B * cap * H * D
    SENT = -12288.0  # (exact in bf16)
    for append in (True, False):
        buf_k = torch.full((2 * guard + per,), SENT, dtype=torch.bfloat16, device=DEV)
        buf_v = torch.full((2 * guard + per,), SENT, dtype=torch.bfloat16, device=DEV)
        kc, vc = buf_k[guard:guard + per].view(B, cap, H, D), buf_v[guard:guard + per].view(B, cap, H, D)
        kc.copy_(torch.randn(B, cap, H, D, generator=g).bfloat16())
        vc.copy_(torch.randn(B, cap, H, D, generator=g).bfloat16())
        k0, v0 = kc.clone(), vc.clone()
        q, kn, vn = (torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV) for _ in range(3))
        lens = [cap + 5, cap, -3, 2 ** 31 - 1]
        o, lse = flash_attn_with_kvcache(q, kc, vc, kn if append else None, vn if append else None,
                                         torch.tensor(lens, dtype=torch.int32, device=DEV), 0.125, return_lse=True)
        torch.cuda.synchronize()
        for buf in (buf_k, buf_v):
            assert (buf[:guard].float() == SENT).all() and (buf[guard + per:].float() == SENT).all()
        ro, rl = _ref(q, k0, v0, kn[:, 0] if append else None, vn[:, 0] if append else None, lens, 0.125, None, 0)
        _check(o, lse, ro, rl, torch.bfloat16, f"over-capacity lengths, append {append}")
        if append:  # only batch element 2 (length -3 -> 0) had room: its row 0 is the new one, nothing else changed
            k0[2, 0] = kn[2, 0]
            v0[2, 0] = vn[2, 0]
        assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16))


@pytest.mark.parametrize("D", [64, 128])
def test_matches_existing_kernels(D):
    from flasht5_amd import flash_attn_with_kvcache, flash_attention_v2_rpe1d, flash_attention_v2_bias
    g = torch.Generator().manual_seed(4)
    B, H, S = 2, 12, 384
    rpe = _rpe(H, R_T5, True, g)
    q, k, v = (torch.randn(B, H, S, D, generator=g).bfloat16().to(DEV) for _ in range(3))
    full = flash_attention_v2_rpe1d(q, k, v, rpe, R_T5, True, 0.125)  # (B, H, S, D) causal
    kc, vc = k.transpose(1, 2), v.transpose(1, 2)  # (B, S, H, D) views of (B, H, S, D) storage
    for t in (0, 1, 63, 127, 128, 200, S - 1):
        o = flash_attn_with_kvcache(q[:, :, t:t + 1].transpose(1, 2), kc, vc, None, None,
                                    torch.full((B,), t + 1, dtype=torch.int32, device=DEV), 0.125, rpe, R_T5)
        ref = full[:, :, t].float()
        err = (o[:, 0].float() - ref).abs().max().item()
        assert err <= 2 * (1e-3 + 2 ** -8) * max(1.0, ref.abs().max().item()), (t, err)
    # the cross-attention shape: fat5_attn_fwd at M = 1, no bias, against the whole cache
    o1 = flash_attention_v2_bias(q[:, :, :1], k, v, None, False, 0.125)
    o = flash_attn_with_kvcache(q[:, :, :1].transpose(1, 2), kc, vc, softmax_scale=0.125)
    err = (o[:, 0].float() - o1[:, :, 0].float()).abs().max().item()
    assert err <= 2 * (1e-3 + 2 ** -8) * max(1.0, o1.float().abs().max().item()), err


def test_deterministic_and_graph_replay_with_device_lengths():
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(5)
    B, H, D, cap, steps = 3, 12, 64, 1200, 6
    rpe = _rpe(H, R_T5, True, g)
    kc, vc = _cache(B, cap, H, D, torch.bfloat16, "blhd", g)
    qs = [torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV) for _ in range(steps)]
    kns = [torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV) for _ in range(steps)]
    start = torch.tensor([900, 3, 511], dtype=torch.int32, device=DEV)
    k0, v0 = kc.clone(), vc.clone()

    def eager():
        kc.copy_(k0), vc.copy_(v0)
        lens, outs = start.clone(), []
        for s in range(steps):
            outs.append(flash_attn_with_kvcache(qs[s], kc, vc, kns[s], kns[s], lens, 0.125, rpe, R_T5, return_lse=True))
            lens += 1
        return [torch.cat([o.flatten().view(torch.int16).float(), l.flatten()]) for o, l in outs]

    a, b = eager(), eager()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # one captured step, replayed with the lengths advanced on the device and the inputs copied into static buffers
    kc.copy_(k0), vc.copy_(v0)
    lens = start.clone()
    sq, sk = qs[0].clone(), kns[0].clone()
    flash_attn_with_kvcache(sq, kc, vc, sk, sk, lens.clone(), 0.125, rpe, R_T5, return_lse=True)  # (warm-up, then restore)
    kc.copy_(k0), vc.copy_(v0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        so, sl = flash_attn_with_kvcache(sq, kc, vc, sk, sk, lens, 0.125, rpe, R_T5, return_lse=True)
        lens.add_(1)
    for s in range(steps):
        sq.copy_(qs[s]), sk.copy_(kns[s])
        graph.replay()
        got = torch.cat([so.flatten().view(torch.int16).float(), sl.flatten()])
        assert torch.equal(got, a[s]), s
    torch.cuda.synchronize()
    assert torch.equal(lens.cpu(), (start + steps).cpu())
    del graph


def test_cache_larger_than_2_31_elements():
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(6)
    B, H, D = 2, 8, 128
    cap = (1 << 31) // (H * D) + 64  # batch element 1 starts past 2^31 elements
    kc = torch.empty(B, cap, H, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.empty(B, cap, H, D, dtype=torch.bfloat16, device=DEV)
    assert kc.numel() > 2 ** 31
    lens = [300, 300]
    for b in range(B):
        kc[b, :301] = torch.randn(301, H, D, generator=g).bfloat16().to(DEV)
        vc[b, :301] = torch.randn(301, H, D, generator=g).bfloat16().to(DEV)
    kc[1, cap - 4:] = torch.randn(4, H, D, generator=g).bfloat16().to(DEV)
    vc[1, cap - 4:] = torch.randn(4, H, D, generator=g).bfloat16().to(DEV)
    q, kn, vn = (torch.randn(B, 1, H, D, generator=g).bfloat16().to(DEV) for _ in range(3))
    small_k, small_v = kc[:, :301].clone(), vc[:, :301].clone()
    o = flash_attn_with_kvcache(q, kc, vc, kn, vn, torch.tensor(lens, dtype=torch.int32, device=DEV), 0.125)
    ro, _ = _ref(q, small_k, small_v, kn[:, 0], vn[:, 0], lens, 0.125, None, 0)
    _check(o, None, ro, None, torch.bfloat16, "2^31 cache")
    assert torch.equal(kc[1, 300].view(torch.int16), kn[1, 0].view(torch.int16))
    # the last rows of the last batch element (offsets near 2 * 2^31), without an append: full-capacity length is too slow here,
    # so look at them through a view that starts at cap - 4
    o = flash_attn_with_kvcache(q, kc[:, cap - 4:], vc[:, cap - 4:], softmax_scale=0.125)
    ro, _ = _ref(q[1:], kc[1:, cap - 4:].clone(), vc[1:, cap - 4:].clone(), None, None, [4], 0.125, None, 0)
    _check(o[1:], None, ro, None, torch.bfloat16, "2^31 cache, tail")
    del kc, vc
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- model level
def _model(kind, base_shape=False, seed=0, vocab=512):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(attention_type="fat5_rpe")
    if kind == "t5_triton":
        kw = dict(attention_type="triton")
    elif kind == "rope":
        kw = dict(position_encoding_type="RoPE")
    elif kind == "xpos":
        kw = dict(position_encoding_type="RoPE", rotary_scale_base=512.0, attention_type="triton")
    if base_shape:  # FAT5-base shapes, two layers per stack
        c = FAT5Config(num_layers=2, num_decoder_layers=2, **kw)
    else:
        c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                       relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


LOGIT_BOUND = 0.02  # |decode_step - full forward| <= LOGIT_BOUND * max(1, max |logits|): bf16 logits (2^-7 relative), other GEMM shapes;
# measured worst 1.03e-2 over every mode and shape below


def _full_logits(model, ids, dec_in):
    enc = model.encoder(ids)
    return model.lm_head(model.decoder(dec_in, encoder_hidden_states=enc)).float()


@pytest.mark.parametrize("kind", ["t5_rpe", "t5_triton", "rope", "xpos"])
@pytest.mark.parametrize("base_shape", [False, True])
@pytest.mark.parametrize("autocast", [False, True])
def test_decode_step_matches_full_forward(kind, base_shape, autocast):
    if autocast and base_shape:
        pytest.skip("(autocast is covered on the small config)")
    m = _model(kind, base_shape).to(DEV)
    if not autocast:
        m = m.bfloat16()
    g = torch.Generator().manual_seed(7)
    B, L_enc, T = 3, 40, 20
    V = m.config.vocab_size
    ids = torch.randint(2, V, (B, L_enc), generator=g).to(DEV)
    labels = torch.randint(2, V, (B, T), generator=g).to(DEV)
    dec_in = m._shift_right(labels)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        full = _full_logits(m, ids, dec_in)
        state = m.init_decode_state(ids, max_length=T)
        worst = 0.0
        for t in range(T):
            lg = m.decode_step(state, dec_in[:, t]).float()
            scale = max(1.0, full[:, t].abs().max().item())
            worst = max(worst, (lg - full[:, t]).abs().max().item() / scale)
    print(f"[decode] {kind} base_shape={base_shape} autocast={autocast}: worst relative logit error {worst:.3e}")
    assert worst <= LOGIT_BOUND, f"{kind}: worst relative logit error {worst:.3e}"


def _recompute_generate(model, ids, max_length):
    """the reference's algorithm (start 0, greedy, stop once every row holds a 1), rerunning the whole decoder per step; also
    returns every row's top-1 / top-2 logit margin per step, relative to max(1, max |logits|) of the row"""
    B = ids.shape[0]
    labels = torch.zeros(B, 1, dtype=torch.long, device=ids.device)
    enc = model.encoder(ids)
    margins = []
    for _ in range(max_length):
        lg = model.lm_head(model.decoder(labels, encoder_hidden_states=enc))[:, -1].float()
        top = lg.topk(2, -1).values
        margins.append(((top[:, 0] - top[:, 1]) / lg.abs().amax(-1).clamp(min=1)).cpu())
        labels = torch.cat([labels, lg.argmax(-1, keepdim=True)], -1)
        if bool((labels == 1).any(-1).all()):
            break
    from flasht5_amd.generation import finish_labels
    return finish_labels(labels), labels, torch.stack(margins, 1)


def _decisive(m, seed):
    """a random model whose greedy choices have clear winners: lm_head row sigma(t) is token t's embedding for a seeded permutation
    sigma, so the next token is sigma(current token) with a wide margin (the residual stream keeps the token's embedding; measured: in
    every step).  (A random lm_head gives flat logits: the top two are often no further apart than the decode path's bf16 error.)"""
    V = m.config.vocab_size
    sigma = torch.randperm(V, generator=torch.Generator().manual_seed(1000 + seed))
    with torch.no_grad():
        m.lm_head.weight[sigma] = m.shared.weight
    return sigma


@pytest.mark.parametrize("kind", ["t5_rpe", "t5_triton", "rope"])
@pytest.mark.parametrize("variant, min_share", [("decisive", 0.9), ("random16", 0.45)])
def test_generate_matches_recompute(kind, variant, min_share):
    """generate against the recompute loop, per row, up to the first step whose recompute margin is within twice the decode path's
    error (the decode path's worst relative logit error on THIS model, measured by teacher-forcing decode_step along the recompute
    tokens; at most LOGIT_BOUND).  Two models: `decisive` (_decisive: every step compared, the tokens follow the permutation, so this
    checks the loop -- token feedback, output columns, stop rule, ending) and a plain random one with a 16-token vocabulary, whose
    tokens the layers decide but whose flat logits leave only about half of the steps decisive (measured 98 / 200, 98 / 200 and
    132 / 256 row-steps)."""
    compared = total = context = 0
    for seed in range(4):
        m = _model(kind, seed=seed, vocab=512 if variant == "decisive" else 16).to(DEV).bfloat16()
        sigma = _decisive(m, seed).to(DEV) if variant == "decisive" else torch.arange(16, device=DEV)
        g = torch.Generator().manual_seed(100 + seed)
        ids = torch.randint(2, m.config.vocab_size, (4, 33), generator=g).to(DEV)
        with torch.no_grad():
            ref, raw, margins = _recompute_generate(m, ids, 16)
            out = m.generate(ids, max_length=16)
            state, err = m.init_decode_state(ids, max_length=16), 0.0
            full = _full_logits(m, ids, raw)
            for t in range(margins.shape[1]):
                lg = m.decode_step(state, raw[:, t]).float()
                err = max(err, ((lg - full[:, t]).abs().amax(-1) / full[:, t].abs().amax(-1).clamp(min=1)).max().item())
        assert err <= LOGIT_BOUND, (kind, seed, err)
        context += int((raw[:, 1:] != sigma[raw[:, :-1]]).sum())  # (steps where the layers, not the permutation, decided)
        bound = 2 * err
        steps = margins.shape[1]
        total += margins.numel()
        if bool((margins > bound).all()):
            assert torch.equal(out, ref), (kind, seed)
            compared += margins.numel()
            continue
        # the reference's ending zeroes what follows a row's first 1: compare the raw tokens under the same masking
        first = torch.where((raw == 1).any(-1), (raw == 1).long().argmax(-1), raw.shape[1])
        keep = torch.arange(raw.shape[1], device=DEV).unsqueeze(0) <= first.unsqueeze(1)
        expect = raw.masked_fill(~keep, 0)
        for r in range(ids.shape[0]):
            low = (margins[r] <= bound).nonzero()
            n = int(low[0]) if len(low) else steps
            compared += n
            w = min(n, out.shape[1] - 2)
            assert torch.equal(out[r, 1:w + 1], expect[r, 1:w + 1]), (kind, seed, r, n)
    print(f"[decode] generate vs recompute ({kind}, {variant}): {compared} of {total} row-steps compared, {context} not "
          "following the permutation")
    assert compared >= min_share * total, f"only {compared} of {total} row-steps were decisive enough to compare"


def test_python_rejections_on_the_gpu():
    """what only a device can reach: tensors on different devices, and lengths that need a conversion inside a graph capture"""
    from flasht5_amd import flash_attn_with_kvcache
    q = torch.zeros(2, 1, 4, 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(2, 16, 4, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="GPU"):
        flash_attn_with_kvcache(q, kc, kc.cpu())
    with pytest.raises(ValueError, match="GPU"):
        flash_attn_with_kvcache(q, kc, kc, rpe1d=torch.zeros(4, 257), rpe_radius=128)
    with pytest.raises(ValueError, match=r"\(B, 1, H, D\)"):
        flash_attn_with_kvcache(torch.zeros(2, 2, 4, 64, dtype=torch.bfloat16, device=DEV), kc, kc)
    # host / int64 lengths are converted outside a capture (the way _as_cu converts cu_seqlens) ...
    o64 = flash_attn_with_kvcache(q, kc, kc, q, q, torch.tensor([3, 5]))
    o32 = flash_attn_with_kvcache(q, kc, kc, q, q, torch.tensor([3, 5], dtype=torch.int32, device=DEV))
    assert torch.equal(o64, o32)
    # ... and refused inside one, where a conversion would fix today's value in the graph
    lens = torch.tensor([3, 5], device=DEV)
    flash_attn_with_kvcache(q, kc, kc, q, q, lens.int())  # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="graph capture"):
        with torch.cuda.graph(graph):
            flash_attn_with_kvcache(q, kc, kc, q, q, lens)
    del graph


@pytest.mark.parametrize("kind", ["t5_rpe", "t5_triton", "xpos"])
def test_graph_generate_equals_eager(kind):
    m = _model(kind, seed=3).to(DEV).bfloat16()
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(2, m.config.vocab_size, (5, 29), generator=g).to(DEV)
    a = m.generate(ids, max_length=20)
    b = m.generate(ids, max_length=20, graph=True)
    assert torch.equal(a, b)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m32 = _model(kind, seed=3).to(DEV)
        a = m32.generate(ids, max_length=12)
        b = m32.generate(ids, max_length=12, graph=True)
    assert torch.equal(a, b)
