"""GPU tests of beam search: the decode kernel's indexed cache reads (cache_batch_idx, cache_row_batch) bitwise against the same
kernel on caches gathered with torch and against fp64; the beam-step kernel driven directly over logits, against the restatement
(tests/beam_ref.py) fed the same logits -- bitwise where the row's lse is exact in fp32, within a stated bound where it is not --,
its determinism and graph replay; and `generate(num_beams=k)`: every beam row's decode logits against the recompute decoder on
that row's prefix, the restatement fed the same logits, graph against eager, and the self-attention caches never rewritten.

Score bound (random logits): the kernel forms x - lse with its own fp32 reduction order, HF's log_softmax another one, so one step
differs by a few ulp of max(|lse|, |score|):  |score - ref| <= 1e-5 * max(1, |ref|)."""
import itertools

import pytest
import torch

import beam_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATE = ("running_scores", "running_seqs", "cache_row_batch", "finished_seqs", "finished_scores", "finished_flags", "finished_lens",
         "heuristic", "status")


# ------------------------------------------------------------------------------------------------ decode: indexed reads
def _ref64(q, kc, vc, kn, vn, lens, scale, rpe1d, R):
    """fp64: per row b, keys [0, lens[b]) of the caches given (already gathered), plus the appended row"""
    B, _, H, D = q.shape
    o = torch.zeros(B, H, D, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        k, v = kc[b, :n].double().cpu(), vc[b, :n].double().cpu()
        if kn is not None:
            k = torch.cat([k, kn[b].double().cpu()], 0)
            v = torch.cat([v, vn[b].double().cpu()], 0)
        L = k.shape[0]
        s = torch.einsum("hd,lhd->hl", q[b, 0].double().cpu(), k) * scale
        if rpe1d is not None:
            s = s + rpe1d.double().cpu()[:, (torch.arange(L) - (L - 1)).clamp(-R, R) + R]
        o[b] = torch.einsum("hl,lhd->hd", torch.softmax(s, -1), v)
    return o


def _rpe(H, R, g):
    from flasht5_amd.positional_encoding import rpe1d_from_table
    return rpe1d_from_table(torch.randn(32, H, generator=g) * 0.5, bidirectional=False, num_buckets=32, max_distance=R).to(DEV)


HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


@pytest.mark.parametrize("D, dtype", [(64, torch.bfloat16), (128, torch.bfloat16), (64, torch.float16), (128, torch.float16)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("splits", [1, 4])
def test_cache_batch_idx_bitwise(D, dtype, bias, splits):
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(D + splits + bias)
    Bc, k, H, L = 3, 4, 6, 300
    B = Bc * k
    kc, vc = (torch.randn(Bc, L, H, D, generator=g).to(dtype).to(DEV) for _ in range(2))
    q = torch.randn(B, 1, H, D, generator=g).to(dtype).to(DEV)
    idx = torch.tensor([(b // k + (b % 3 == 2)) % Bc for b in range(B)] , dtype=torch.int32, device=DEV)
    rpe = _rpe(H, 128, g) if bias else None
    R = 128 if bias else 0
    lens = torch.randint(1, L + 1, (B,), generator=g).int().to(DEV)
    o = flash_attn_with_kvcache(q, kc, vc, None, None, lens, 0.125, rpe, R, num_splits=splits, cache_batch_idx=idx)
    kg, vg = kc[idx.long()].contiguous(), vc[idx.long()].contiguous()
    o_ref = flash_attn_with_kvcache(q, kg, vg, None, None, lens, 0.125, rpe, R, num_splits=splits)
    assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16))
    r64 = _ref64(q, kg, vg, None, None, lens.cpu(), 0.125, rpe, R)
    err = (o[:, 0].double().cpu() - r64).abs().max().item()
    assert err <= (1e-3 + HALF_ULP[dtype]) * max(1.0, r64.abs().max().item()), err


@pytest.mark.parametrize("D, dtype", [(64, torch.bfloat16), (128, torch.bfloat16), (64, torch.float16), (128, torch.float16)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("splits", [1, 3])
def test_cache_row_batch_bitwise(D, dtype, bias, append, splits):
    from flasht5_amd import flash_attn_with_kvcache
    g = torch.Generator().manual_seed(7 * D + splits + 2 * bias + append)
    B, H, cap = 8, 4, 520
    kc, vc = (torch.randn(B, cap, H, D, generator=g).to(dtype).to(DEV) for _ in range(2))
    q, kn, vn = (torch.randn(B, 1, H, D, generator=g).to(dtype).to(DEV) for _ in range(3))
    table = torch.randint(0, B, (B, cap), generator=g).int()
    table[0, :5] = torch.tensor([-7, B, B + 100, 2 ** 31 - 1, -(2 ** 31)], dtype=torch.int32)  # (clamped on the device)
    lens = torch.tensor([0, 1, 5, 127, 128, 129, 400, cap - 1][:B], dtype=torch.int32)
    if append:  # (no row may read element e's row lens[e] while e appends there in the same launch: fat5.h's contract)
        e = table.long().clamp(0, B - 1)
        table = torch.where((torch.arange(cap).unsqueeze(0) == lens[e]) & (e != torch.arange(B).unsqueeze(1)),
                            torch.arange(B, dtype=torch.int32).unsqueeze(1).expand(B, cap), table)
    table, lens = table.to(DEV), lens.to(DEV)
    rpe = _rpe(H, 128, g) if bias else None
    R = 128 if bias else 0
    rows = torch.arange(cap, device=DEV).unsqueeze(0).expand(B, cap)
    tb = table.long().clamp(0, B - 1)
    kg, vg = kc[tb, rows].contiguous(), vc[tb, rows].contiguous()  # (B, cap, H, D): row j of row b from element table[b, j]
    k0, v0, kg0, vg0 = kc.clone(), vc.clone(), kg.clone(), vg.clone()
    own = torch.arange(B, dtype=torch.int32, device=DEV).unsqueeze(1).expand(B, cap).contiguous()
    o = flash_attn_with_kvcache(q, kc, vc, kn if append else None, vn if append else None, lens, 0.125, rpe, R, num_splits=splits,
                                cache_row_batch=table)
    # the same kernel (the row-map instantiation) on the gathered caches, each row reading its own rows: bit for bit.  (The plain
    # instantiation is another compilation: its FMA contraction of q.k * scale - max may differ in the last bit, e.g. at D 64 with
    # an append and no bias, so it is held to the fp64 bound below like the mapped one.)
    o_ref = flash_attn_with_kvcache(q, kg, vg, kn if append else None, vn if append else None, lens, 0.125, rpe, R,
                                    num_splits=splits, cache_row_batch=own)
    torch.cuda.synchronize()
    assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16))
    if append:  # the new row lands in batch element b at row lens[b], nothing else changes
        for b in range(B):
            k0[b, int(lens[b])], v0[b, int(lens[b])] = kn[b, 0], vn[b, 0]
    assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16))
    r64 = _ref64(q, kg0, vg0, kn if append else None, vn if append else None, lens.cpu(), 0.125, rpe, R)
    o_plain = flash_attn_with_kvcache(q, kg0.clone(), vg0.clone(), kn if append else None, vn if append else None, lens, 0.125, rpe,
                                      R, num_splits=splits)
    for out in (o, o_plain):
        err = (out[:, 0].double().cpu() - r64).abs().max().item()
        assert err <= (1e-3 + HALF_ULP[dtype]) * max(1.0, r64.abs().max().item()), err


# ------------------------------------------------------------------------------------------------ the beam step, driven directly
def _dev_state(B, k, L, cap):
    from flasht5_amd.beam import new_state
    return new_state(B, k, L, cap, DEV)


def _exact_logits(B, k, V, g, eos_p, dtype):
    """logits whose row lse is exactly the row maximum in fp32 (every other entry at least 104 below it: its exp is below 2^-149
    or sums to less than half an ulp of 1), so the kernel and the restatement see identical log-probabilities and every decision,
    ties included, must agree bit for bit"""
    x = torch.rand(B * k, V, generator=g) * -40.0 - 110.0
    x = x.to(dtype).float()
    if V > 8:  # exact duplicates inside a row (ties inside a row go to the lower token)
        x[:, 2:4] = x[:, 4:5]
    top = torch.randint(0, V, (B * k,), generator=g)
    top = torch.where(torch.rand(B * k, generator=g) < eos_p, torch.ones_like(top), top)
    x[torch.arange(B * k), top] = (torch.rand(B * k, generator=g) * 4.0).to(dtype).float()
    return x.to(dtype)


@pytest.mark.parametrize("k, V, dtype", [(2, 7, torch.float32), (4, 32128, torch.bfloat16), (4, 50000, torch.float16),
                                         (16, 1000, torch.float32), (3, 5, torch.bfloat16)])
@pytest.mark.parametrize("lp, es", [(1.0, False), (0.0, True), (2.0, "never"), (-0.5, False)])
def test_beam_step_exact_against_restatement(k, V, dtype, lp, es):
    from flasht5_amd.beam import beam_step
    g = torch.Generator().manual_seed(k * 1000 + V + int(10 * lp))
    B, max_length = 3, 14
    L = cap = max_length + 1
    st = _dev_state(B, k, L, cap)
    ref = beam_ref.init(B, k, L, cap)
    lens = torch.zeros(B * k, dtype=torch.int32, device=DEV)
    for s in range(1, max_length + 1):
        x = _exact_logits(B, k, V, g, 0.15, dtype)
        lens.fill_(s)
        beam_step(x.to(DEV), st, lens, max_length, lp, es)
        tok_ref, _ = beam_ref.step(ref, x, s, max_length, lp, es)
        torch.cuda.synchronize()
        assert torch.equal(st.tokens.cpu(), tok_ref), s
        for name in STATE:
            got = getattr(st, name).cpu()
            assert torch.equal(got, ref[name]), (s, name, got, ref[name])
        if not beam_ref.keep_going(ref, es):
            break


@pytest.mark.parametrize("k, V, dtype", [(4, 32128, torch.bfloat16), (2, 300, torch.float32), (8, 40000, torch.float16)])
def test_beam_step_random_logits(k, V, dtype):
    """ordinary logits: the kernel's lse and HF's log_softmax differ by ulps, so a step is compared where no decision of the batch
    item lies within 1e-5 (relative) of a tie; every step starts from the kernel's state (copied into the restatement)"""
    from flasht5_amd.beam import beam_step
    g = torch.Generator().manual_seed(k + V)
    B, max_length = 4, 24
    L = cap = max_length + 1
    st = _dev_state(B, k, L, cap)
    lens = torch.zeros(B * k, dtype=torch.int32, device=DEV)
    compared = total = 0
    for s in range(1, max_length + 1):
        x = (torch.randn(B * k, V, generator=g) * 3.0).to(dtype)
        x[:, 1] -= 4.0  # (EOS now and then, not always)
        ref = {n: getattr(st, n).cpu().clone() for n in STATE}
        lens.fill_(s)
        beam_step(x.to(DEV), st, lens, max_length, 1.0, False)
        tok_ref, amb = beam_ref.step(ref, x, s, max_length, 1.0, False, tol=1e-5)
        tok = st.tokens.cpu().view(B, k)
        for b in range(B):
            total += 1
            if amb[b]:
                continue
            compared += 1
            assert torch.equal(tok[b], tok_ref.view(B, k)[b]), (s, b)
            for name in ("running_seqs", "finished_seqs", "finished_flags", "finished_lens"):
                assert torch.equal(getattr(st, name).cpu()[b], ref[name][b]), (s, b, name)
            assert torch.equal(st.cache_row_batch.cpu().view(B, k, -1)[b], ref["cache_row_batch"].view(B, k, -1)[b])
            for name in ("running_scores", "finished_scores"):
                got, want = getattr(st, name).cpu()[b], ref[name][b]
                assert ((got - want).abs() <= 1e-5 * want.abs().clamp(min=1.0)).all(), (s, b, name, got, want)
    print(f"[beam] random logits k={k} V={V}: {compared} of {total} item-steps compared")
    assert compared >= 0.8 * total


def test_beam_step_deterministic_and_graph_replay():
    from flasht5_amd.beam import beam_step
    g = torch.Generator().manual_seed(11)
    B, k, V, max_length = 5, 4, 32128, 10
    xs = [(torch.randn(B * k, V, generator=g) * 3).bfloat16().to(DEV) for _ in range(max_length)]

    def eager():
        st = _dev_state(B, k, max_length + 1, max_length + 1)
        lens = torch.zeros(B * k, dtype=torch.int32, device=DEV)
        out = []
        for s in range(1, max_length + 1):
            lens.fill_(s)
            beam_step(xs[s - 1], st, lens, max_length, 1.0, False)
            out.append([getattr(st, n).clone() for n in STATE] + [st.tokens.clone()])
        return out

    a, b = eager(), eager()
    assert all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    st = _dev_state(B, k, max_length + 1, max_length + 1)
    lens = torch.ones(B * k, dtype=torch.int32, device=DEV)
    sx = xs[0].clone()
    beam_step(sx, st, lens, max_length, 1.0, False)  # (step 1 eagerly, then one captured step replayed)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lens.add_(1)
        beam_step(sx, st, lens, max_length, 1.0, False)
    for s in range(2, max_length + 1):
        sx.copy_(xs[s - 1])
        graph.replay()
        got = [getattr(st, n) for n in STATE] + [st.tokens]
        assert all(torch.equal(x, y) for x, y in zip(got, a[s - 1])), s
    del graph


# ------------------------------------------------------------------------------------------------ generate
def _model(kind, seed=0, vocab=512):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(attention_type="fat5_rpe")
    if kind == "t5_triton":
        kw = dict(attention_type="triton")
    elif kind == "rope":
        kw = dict(position_encoding_type="RoPE")
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


LOGIT_BOUND = 0.02  # |decode_step - full forward| <= LOGIT_BOUND * max(1, max |logits|) (tests/test_decode_gpu.py's bound)

OPTS = [dict(num_beams=4, length_penalty=1.0, early_stopping=False, num_return_sequences=1),
        dict(num_beams=2, length_penalty=2.0, early_stopping=True, num_return_sequences=2),
        dict(num_beams=4, length_penalty=-0.5, early_stopping="never", num_return_sequences=4)]


@pytest.mark.parametrize("kind", ["t5_rpe", "t5_triton", "rope"])
def test_generate_matches_restatement(kind):
    """generate(num_beams=k), step by step.  (1) At every step every beam row's decode logits (its self-attention history read
    through the cache_row_batch table, the cross K / V shared through cache_batch_idx) match the recompute decoder run on that
    row's own prefix within LOGIT_BOUND: a wrong parent or encoder row would give another row's logits.  (2) The restatement fed
    the same logits reaches the same result: every run without a decision within 1e-5 (relative) of a tie returns the same tokens
    and scores within 1e-5 * max(1, |score|); and generate() returns bit for bit what the step-by-step loop returned.  (The
    restatement over the recompute decoder's own logits would compare few runs: bf16 decoding moves logits by up to 2 % of their
    range, more than the gaps between the 2k runners-up of a random model.)"""
    from flasht5_amd.beam import new_state, keep_going, beam_step
    from flasht5_amd.generation import init_decode_state, decode_step
    compared = total = 0
    worst = 0.0
    for seed, opts in itertools.product(range(3), OPTS):
        m = _model(kind, seed=seed, vocab=256).to(DEV).bfloat16()
        g = torch.Generator().manual_seed(100 + seed)
        B, max_length = 3, 12
        k, R, lp, es = opts["num_beams"], opts["num_return_sequences"], opts["length_penalty"], opts["early_stopping"]
        ids = torch.randint(2, m.config.vocab_size, (B, 21), generator=g).to(DEV)
        with torch.no_grad():
            enc = m.encoder(ids).repeat_interleave(k, 0)
            state = init_decode_state(m, ids, max_length, num_beams=k)
            bs = new_state(B, k, max_length + 1, state.capacity, DEV)
            bs.cache_row_batch = state.row_batch
            seen = []
            for s in range(1, max_length + 1):
                prefix = bs.running_seqs[:, :, :s].reshape(B * k, s).clone()
                lg = decode_step(m, state, prefix[:, -1].contiguous())  # (generation._beam_step's two calls)
                beam_step(lg, bs, state.cache_seqlens, max_length, lp, es)
                full = m.lm_head(m.decoder(prefix, encoder_hidden_states=enc))[:, -1].float()
                err = ((lg.float() - full).abs().amax(-1) / full.abs().amax(-1).clamp(min=1)).max().item()
                worst = max(worst, err)
                assert err <= LOGIT_BOUND, (kind, seed, s, err)
                seen.append(lg.float().cpu())
                if not bool(keep_going(bs.status, es)):
                    break
            T = int(bs.finished_lens[:, :R].max())
            loop_out = bs.finished_seqs[:, :R].reshape(B * R, -1)[:, :T + 1]
            out, sc = m.generate(ids, max_length=max_length, return_scores=True, **opts)
        assert torch.equal(out, loop_out) and torch.equal(sc, bs.finished_scores[:, :R].reshape(-1)), (kind, seed, opts)
        rs, rsc, amb = beam_ref.beam_search(lambda p: seen[min(p.shape[1], len(seen)) - 1], B, k, max_length, lp, es, R, tol=1e-5)
        total += 1
        if amb:
            continue
        compared += 1
        assert out.shape == rs.shape and torch.equal(out.cpu(), rs), (kind, seed, opts, out, rs)
        assert ((sc.cpu() - rsc).abs() <= 1e-5 * rsc.abs().clamp(min=1.0)).all(), (kind, seed, opts, sc, rsc)
    print(f"[beam] generate ({kind}): worst relative logit error {worst:.3e}; {compared} of {total} runs compared with the "
          "restatement")
    # (measured on MI355X: 8 / 9 runs compared for t5 fat5_rpe and triton, 4 / 9 for RoPE; every compared run agreed)
    assert compared >= 0.4 * total, f"only {compared} of {total} runs were clear of ties"


@pytest.mark.parametrize("kind", ["t5_rpe", "t5_triton", "rope"])
def test_graph_generate_equals_eager(kind):
    m = _model(kind, seed=3).to(DEV).bfloat16()
    ids = torch.randint(2, m.config.vocab_size, (3, 29), generator=torch.Generator().manual_seed(9)).to(DEV)
    for opts in OPTS:
        a, sa = m.generate(ids, max_length=16, return_scores=True, **opts)
        b, sb = m.generate(ids, max_length=16, graph=True, return_scores=True, **opts)
        assert torch.equal(a, b) and torch.equal(sa, sb), opts
        assert a.shape[0] == 3 * opts["num_return_sequences"] and a.dtype == torch.int64 and bool((a[:, 0] == 0).all())


def test_self_attention_caches_never_rewritten():
    """eager steps: once a cache row is written it keeps its bits (the history is a table of parents, not a reordered cache)"""
    from flasht5_amd.beam import new_state
    from flasht5_amd.generation import init_decode_state, _beam_step
    m = _model("t5_rpe", seed=1).to(DEV).bfloat16()
    ids = torch.randint(2, m.config.vocab_size, (2, 17), generator=torch.Generator().manual_seed(1)).to(DEV)
    k, max_length = 4, 10
    with torch.no_grad():
        state = init_decode_state(m, ids, max_length, num_beams=k)
        bs = new_state(2, k, max_length + 1, state.capacity, DEV)
        bs.cache_row_batch = state.row_batch
        tok = torch.zeros(2 * k, dtype=torch.long, device=DEV)
        snaps = []
        parents_moved = False
        for s in range(1, max_length + 1):
            _beam_step(m, state, tok, bs, (max_length, 1.0, False))
            torch.cuda.synchronize()
            snaps.append([(kc[:, :s].clone(), vc[:, :s].clone()) for kc, vc in zip(state.self_k, state.self_v)])
            for earlier in snaps:
                n = earlier[0][0].shape[1]
                for (k0, v0), kc, vc in zip(earlier, state.self_k, state.self_v):
                    assert torch.equal(kc[:, :n].view(torch.int16), k0.view(torch.int16)), (s, n)
                    assert torch.equal(vc[:, :n].view(torch.int16), v0.view(torch.int16)), (s, n)
            own = torch.arange(2 * k, device=DEV, dtype=torch.int32).unsqueeze(1)
            parents_moved |= bool((state.row_batch[:, :s] != own).any())
    assert parents_moved  # (the history really was re-pointed, not copied)
