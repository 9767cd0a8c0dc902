"""GPU tests of the logits processors: the kernel (fat5_process_logits) bit for bit against the restatement
(tests/logits_proc_ref.py) without log_softmax -- only exact fp32 operations are involved --, with log_softmax bit for bit on
rows whose lse is exact in fp32 and within 1e-5 (relative, the bound tests/test_beam_gpu.py applies to the beam step's scores)
on ordinary rows, bans -inf exactly in both; the device-side guards; beam_step(logits_normalized=True); determinism and graph
replay; and greedy, sampled and beam `generate` with processors against the restatement loop over the decode path's own
per-step logits."""
import ctypes

import pytest
import torch

import beam_ref
import logits_proc_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATE = ("running_scores", "running_seqs", "cache_row_batch", "finished_seqs", "finished_scores", "finished_flags", "finished_lens",
         "heuristic", "status")
NINF = float("-inf")


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _strided(x, stride):
    """x (rows, V) on the device as a view with row stride `stride` elements inside a larger allocation"""
    rows, V = x.shape
    buf = torch.zeros(rows * stride + 16, dtype=x.dtype, device=DEV)
    v = buf[8:8 + rows * stride].view(rows, stride)[:, :V]
    v.copy_(x)
    return v


def _case(V, L, n, g, dtype, bad_entries=True, pos_inf=True):
    """sequences over a small alphabet (tokens and n-grams repeat) with a few vocabulary-wide tokens, rows covering every
    interesting length, inside a buffer with slack on every side (filled with a valid, seen-nowhere-else token: a missing clamp
    would read it and change a value, not fault)"""
    lens = [0, 1, max(n - 1, 0), n, n + 1, L, L // 2, L - 1, -1, L + 5, 7, 3]
    rows = len(lens)
    alpha = torch.randint(0, V, (4,), generator=g)
    seqs = alpha[torch.randint(0, 4, (rows, L), generator=g)]
    seqs[:, 0] = 0
    wide = torch.rand(rows, L, generator=g) < 0.1
    seqs = torch.where(wide, torch.randint(0, V, (rows, L), generator=g), seqs)
    if bad_entries:
        seqs[5, 2], seqs[5, 4], seqs[6, 1] = -1, V, V + 7
    slack_tok = V - 1
    buf = torch.full((rows + 2, L + 16), slack_tok, dtype=torch.int64)
    buf[1:-1, 8:8 + L] = seqs
    view = buf.to(DEV)[1:-1, 8:8 + L]
    x = (torch.randn(rows, V, generator=g) * 3.0).to(dtype)
    x[1, int(seqs[1, 0])] = NINF           # (a seen token at -inf / +inf)
    if pos_inf:
        x[5, int(seqs[5, 1])] = float("inf")
    x[3, V // 2] = NINF
    return x, seqs, view, torch.tensor(lens, dtype=torch.int32)


CONFIGS = [dict(repetition_penalty=1.3), dict(repetition_penalty=0.8), dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2),
           dict(no_repeat_ngram_size=3), dict(min_length=5), dict(suppress_tokens=[0, 3, 4]),
           dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=4, suppress_tokens=[2]), dict()]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V, pad", [(5, 0), (5, 3), (1000, 0), (1000, 5), (32128, 0), (32128, 1), (250112, 0), (250112, 3)])
def test_kernel_bitwise_against_restatement(dtype, V, pad):
    from flasht5_amd import process_logits
    g = torch.Generator().manual_seed(V + pad)
    L = 40
    for cfg in CONFIGS:
        n = cfg.get("no_repeat_ngram_size", 0)
        x, seqs, view, lens = _case(V, L, n, g, dtype)
        xd = _strided(x.to(DEV), V + pad) if pad else x.to(DEV)
        y = process_logits(xd, view, lens.to(DEV), **cfg)
        want = ref.process(x, seqs, lens, **cfg)
        assert y.dtype == torch.float32 and y.shape == (x.shape[0], V)
        assert torch.equal(_bits(y), _bits(want)), (cfg, (_bits(y) != _bits(want)).nonzero()[:8])


def test_banned_wins_over_penalised_and_duplicates_penalised_once():
    from flasht5_amd import process_logits
    V = 64
    x = torch.arange(V, dtype=torch.float32).sub(20.0).unsqueeze(0)
    seq = torch.tensor([[0, 5, 9, 5, 9, 30, 30, 30, 7, 5]])
    lens = torch.tensor([10], dtype=torch.int32)
    y = process_logits(x.to(DEV), seq.to(DEV), lens.to(DEV), repetition_penalty=2.0, no_repeat_ngram_size=2).cpu()
    assert y[0, 9] == NINF                      # (5, 9) seen and the sequence ends in 5: banned although penalised
    assert y[0, 30] == (30.0 - 20.0) / 2.0      # three occurrences, one penalty
    assert y[0, 5] == (5.0 - 20.0) * 2.0 and y[0, 0] == -40.0
    assert torch.equal(_bits(y), _bits(ref.process(x, seq, lens, repetition_penalty=2.0, no_repeat_ngram_size=2)))


def test_long_sequences():
    from flasht5_amd import process_logits
    g = torch.Generator().manual_seed(5)
    V = 32128
    for L in (512, 2048, 4096):
        seqs = torch.randint(0, 50, (3, L), generator=g)
        x = torch.randn(3, V, generator=g).bfloat16()
        lens = torch.tensor([L, L - 1, 600], dtype=torch.int32)
        cfg = dict(repetition_penalty=1.5, no_repeat_ngram_size=3, min_length=L)
        y = process_logits(x.to(DEV), seqs.to(DEV), lens.to(DEV), **cfg)
        assert torch.equal(_bits(y), _bits(ref.process(x, seqs, lens, **cfg))), L
    with pytest.raises(ValueError, match="seq_len"):
        process_logits(x.to(DEV), torch.zeros(3, 4097, dtype=torch.int64, device=DEV), lens.to(DEV), min_length=3)


def _exact_rows(rows, V, g, dtype, eos_p=0.0):
    """test_beam_gpu.py's construction: the row lse is exactly the row maximum in fp32"""
    x = (torch.rand(rows, V, generator=g) * -40.0 - 110.0).to(dtype).float()
    top = torch.randint(0, V, (rows,), generator=g)
    top = torch.where(torch.rand(rows, generator=g) < eos_p, torch.ones_like(top), top)  # (EOS on top now and then)
    x[torch.arange(rows), top] = (torch.rand(rows, generator=g) * 4.0).to(dtype).float()
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V, pad", [(5, 0), (1000, 5), (32128, 0), (250112, 3)])
def test_log_softmax(dtype, V, pad):
    from flasht5_amd import process_logits
    g = torch.Generator().manual_seed(3 * V + pad)
    L = 24
    cfg = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=6, suppress_tokens=[2, 4])
    for exact in (True, False):
        x, seqs, view, lens = _case(V, L, 2, g, dtype, pos_inf=False)  # (+inf would turn the whole normalised row NaN)
        if exact:
            x = _exact_rows(x.shape[0], V, g, dtype)
        xd = _strided(x.to(DEV), V + pad) if pad else x.to(DEV)
        for c in (cfg, dict()):
            y = process_logits(xd, view, lens.to(DEV), log_softmax=True, **c).cpu()
            want = ref.process(x, seqs, lens, log_softmax=True, **c)
            assert torch.equal(y == NINF, want == NINF), (exact, c)
            if exact:
                assert torch.equal(_bits(y), _bits(want)), (exact, c)
            else:
                fin = torch.isfinite(want)
                err = ((y - want).abs() / want.abs().clamp(min=1.0))[fin].max().item()
                print(f"[logits] log_softmax {dtype} V={V}: worst relative error {err:.3e}")
                assert err <= 1e-5, err
                assert torch.equal(_bits(y)[~fin], _bits(want)[~fin])


def test_in_place_fp32_through_the_c_abi():
    """out == logits (fp32): every edit is computed from the input value, so the result is the out-of-place one bit for bit"""
    from flasht5_amd import _lib, process_logits
    g = torch.Generator().manual_seed(17)
    V, L = 1000, 24
    for ls in (False, True):
        x, seqs, view, lens = _case(V, L, 2, g, torch.float32)
        cfg = dict(repetition_penalty=1.7, no_repeat_ngram_size=2, min_length=5)
        xd, ld = x.to(DEV), lens.to(DEV)
        seq_d = seqs.clamp(-1, V).to(DEV).contiguous()
        want = process_logits(xd, seq_d, ld, log_softmax=ls, **cfg)
        p = _lib.LogitsParams()
        p.rows, p.V, p.dtype, p.log_softmax = x.shape[0], V, _lib.FAT5_F32, int(ls)
        p.logits, p.row_stride, p.out, p.out_stride = xd.data_ptr(), V, xd.data_ptr(), V
        p.sequences, p.seq_stride, p.seq_len, p.lengths = seq_d.data_ptr(), L, L, ld.data_ptr()
        p.repetition_penalty, p.no_repeat_ngram_size, p.min_length, p.eos_token_id = 1.7, 2, 5, 1
        _lib.check(_lib.load().fat5_process_logits(ctypes.byref(p), _lib.stream_ptr(xd.device)), "fat5_process_logits")
        torch.cuda.synchronize()
        assert torch.equal(_bits(xd), _bits(want)), ls


# ------------------------------------------------------------------------------------------------ the beam step on processed rows
def _copy_state(st):
    return {n: getattr(st, n).cpu().clone() for n in STATE}


@pytest.mark.parametrize("k, V, dtype", [(2, 7, torch.float32), (4, 32128, torch.bfloat16), (3, 1000, torch.float16)])
@pytest.mark.parametrize("lp, es", [(1.0, False), (2.0, True), (-0.5, "never")])
def test_beam_step_normalized(k, V, dtype, lp, es):
    from flasht5_amd import process_logits
    from flasht5_amd.beam import beam_step, new_state
    g = torch.Generator().manual_seed(k * 100 + V)
    B, max_length = 3, 12
    L = cap = max_length + 1
    raw, norm, proc = (new_state(B, k, L, cap, DEV) for _ in range(3))
    rst = beam_ref.init(B, k, L, cap)
    lens = torch.zeros(B * k, dtype=torch.int32, device=DEV)
    cfg = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=4, suppress_tokens=[3])
    for s in range(1, max_length + 1):
        x = _exact_rows(B * k, V, g, dtype, 0.15)
        lens.fill_(s)
        xd = x.to(DEV)
        # (1) raw rows against the same rows normalised (fp32): every state tensor equal
        beam_step(xd, raw, lens, max_length, lp, es)
        logp = process_logits(xd, norm.running_seqs.view(B * k, L), lens, log_softmax=True)
        beam_step(logp, norm, lens, max_length, lp, es, logits_normalized=True)
        assert torch.equal(raw.tokens, norm.tokens), s
        for name in STATE:
            assert torch.equal(getattr(raw, name), getattr(norm, name)), (s, name)
        # (2) processed rows against the restatement's step
        seqs = proc.running_seqs.view(B * k, L)
        y = process_logits(xd, seqs, lens, log_softmax=True, **cfg)
        want = ref.process(x, seqs.cpu(), lens.cpu(), log_softmax=True, **cfg)
        assert torch.equal(_bits(y), _bits(want)), s
        beam_step(y, proc, lens, max_length, lp, es, logits_normalized=True)
        tok_ref = ref.beam_step_normalized(rst, want, s, max_length, lp, es)
        assert torch.equal(proc.tokens.cpu(), tok_ref), s
        for name in STATE:
            assert torch.equal(getattr(proc, name).cpu(), rst[name]), (s, name)
        if not beam_ref.keep_going(rst, es):
            break


# ------------------------------------------------------------------------------------------------ determinism, graph replay
def test_deterministic_and_graph_replay():
    from flasht5_amd import process_logits
    g = torch.Generator().manual_seed(23)
    rows, V, L = 6, 32128, 32
    cfg = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=9)
    sup = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    xs = [(torch.randn(rows, V, generator=g) * 3).bfloat16().to(DEV) for _ in range(6)]
    sq = [torch.randint(0, 6, (rows, L), generator=g).to(DEV) for _ in range(6)]
    ln = [torch.randint(0, L + 1, (rows,), generator=g).int().to(DEV) for _ in range(6)]

    def eager(ls):
        return [process_logits(xs[i], sq[i], ln[i], suppress_tokens=sup, log_softmax=ls, **cfg).clone() for i in range(6)]

    for ls in (False, True):
        a, b = eager(ls), eager(ls)
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))
        for i in range(6):
            want = ref.process(xs[i], sq[i], ln[i], suppress_tokens=sup, log_softmax=ls, **cfg)
            if not ls:
                assert torch.equal(_bits(a[i]), _bits(want))
        sx, ss, sl = xs[0].clone(), sq[0].clone(), ln[0].clone()
        process_logits(sx, ss, sl, suppress_tokens=sup, log_softmax=ls, **cfg)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = process_logits(sx, ss, sl, suppress_tokens=sup, log_softmax=ls, **cfg)
        for i in range(6):  # (lengths and sequences change on the device only)
            sx.copy_(xs[i]), ss.copy_(sq[i]), sl.copy_(ln[i])
            graph.replay()
            assert torch.equal(_bits(out), _bits(a[i])), (ls, i)
        del graph


# ------------------------------------------------------------------------------------------------ generate
def _model(kind, seed=0, vocab=256):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(attention_type="fat5_rpe") if kind == "t5_rpe" else dict(position_encoding_type="RoPE")
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


PROC = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=6, suppress_tokens=[7, 8, 9, 200])
MAXLEN = 20


def _check_properties(out, n, min_length, suppressed):
    """no n-gram twice up to a row's EOS, no EOS before column min_length, no suppressed id anywhere"""
    for row in out.cpu().tolist():
        end = row.index(1) + 1 if 1 in row else len(row)
        if 1 in row:
            assert row.index(1) >= min_length, row
        grams = [tuple(row[i:i + n]) for i in range(end - n + 1)]
        assert len(grams) == len(set(grams)), row
        assert not set(row) & set(suppressed), row


@pytest.mark.parametrize("kind", ["t5_rpe", "rope"])
@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_generate_greedy_and_sampled_match_restatement_loop(kind, mode):
    from flasht5_amd import sample_logits
    from flasht5_amd.generation import init_decode_state, decode_step, finish_labels
    for seed in range(2):
        m = _model(kind, seed=seed).to(DEV).bfloat16()
        with torch.no_grad():
            m.lm_head.weight[1].mul_(3.0)  # (EOS wanted early: min_length has something to hold back)
        B = 3
        ids = torch.randint(2, 256, (B, 21), generator=torch.Generator().manual_seed(100 + seed)).to(DEV)
        skw = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=1234 + seed) if mode == "sample" else {}
        with torch.no_grad():
            state = init_decode_state(m, ids, MAXLEN)
            labels = torch.zeros(B, MAXLEN + 1, dtype=torch.long)
            tok = torch.zeros(B, dtype=torch.long, device=DEV)
            seen = torch.zeros(B, dtype=torch.bool)
            steps = 0
            for s in range(1, MAXLEN + 1):
                lg = decode_step(m, state, tok)
                y = ref.process(lg, labels, torch.full((B,), s, dtype=torch.int32), **PROC).to(DEV)
                if mode == "sample":
                    nxt = sample_logits(y, 0.8, 20, 0.9, seed=1234 + seed, offsets=state.cache_seqlens)
                else:
                    nxt = y.argmax(-1)
                tok.copy_(nxt)
                labels[:, s] = nxt.cpu()
                seen |= nxt.cpu() == 1
                steps = s
                if bool(seen.all()):
                    break
            want = finish_labels(labels[:, :steps + 1])
            a = m.generate(ids, max_length=MAXLEN, **skw, **PROC)
            b = m.generate(ids, max_length=MAXLEN, graph=True, **skw, **PROC)
        assert torch.equal(a.cpu(), want), (kind, mode, seed, a, want)
        assert torch.equal(a, b), (kind, mode, seed)
        _check_properties(a, 2, 6, PROC["suppress_tokens"])


@pytest.mark.parametrize("kind", ["t5_rpe", "rope"])
@pytest.mark.parametrize("opts", [dict(num_beams=4, length_penalty=2.0, early_stopping=True, num_return_sequences=1),
                                  dict(num_beams=3, length_penalty=1.0, early_stopping=False, num_return_sequences=3)])
def test_generate_beam_matches_restatement_loop(kind, opts):
    """every step: the kernel's processed rows equal the restatement's edits applied to the kernel's own log-probabilities (the
    processor-free call, held to 1e-5 of the restatement's by test_log_softmax) bit for bit, and the beam state equals the
    restatement's step over them; generate() returns what the loop returned, eager and replayed"""
    from flasht5_amd import process_logits
    from flasht5_amd.beam import new_state, keep_going, beam_step
    from flasht5_amd.generation import init_decode_state, decode_step
    k, R, lp, es = opts["num_beams"], opts["num_return_sequences"], opts["length_penalty"], opts["early_stopping"]
    for seed in range(2):
        m = _model(kind, seed=seed).to(DEV).bfloat16()
        with torch.no_grad():
            m.lm_head.weight[1].mul_(3.0)
        B = 2
        ids = torch.randint(2, 256, (B, 21), generator=torch.Generator().manual_seed(200 + seed)).to(DEV)
        with torch.no_grad():
            state = init_decode_state(m, ids, MAXLEN, num_beams=k)
            bs = new_state(B, k, MAXLEN + 1, state.capacity, DEV)
            bs.cache_row_batch = state.row_batch
            rst = beam_ref.init(B, k, MAXLEN + 1, state.capacity)
            for s in range(1, MAXLEN + 1):
                seqs = bs.running_seqs.view(B * k, -1)
                lg = decode_step(m, state, seqs[:, s - 1].contiguous())
                logp = process_logits(lg, seqs, state.cache_seqlens, log_softmax=True)
                y = process_logits(lg, seqs, state.cache_seqlens, log_softmax=True, **PROC)
                want = ref.process(logp, seqs.cpu(), state.cache_seqlens.cpu(), **PROC)
                assert torch.equal(_bits(y), _bits(want)), (kind, seed, s)
                beam_step(y, bs, state.cache_seqlens, MAXLEN, lp, es, logits_normalized=True)
                ref.beam_step_normalized(rst, want, s, MAXLEN, lp, es)
                for name in STATE:
                    assert torch.equal(getattr(bs, name).cpu(), rst[name]), (kind, seed, s, name)
                if not bool(keep_going(bs.status, es)):
                    break
            T = int(bs.finished_lens[:, :R].max())
            loop_out = bs.finished_seqs[:, :R].reshape(B * R, -1)[:, :T + 1]
            a, sa = m.generate(ids, max_length=MAXLEN, return_scores=True, **opts, **PROC)
            b, sb = m.generate(ids, max_length=MAXLEN, graph=True, return_scores=True, **opts, **PROC)
        assert torch.equal(a, loop_out) and torch.equal(sa, bs.finished_scores[:, :R].reshape(-1)), (kind, seed)
        assert torch.equal(a, b) and torch.equal(sa, sb), (kind, seed)
        _check_properties(a, 2, 6, PROC["suppress_tokens"])


@pytest.mark.parametrize("kw", [dict(), dict(do_sample=True, seed=5), dict(num_beams=4)])
def test_defaults_make_no_launch(kw, monkeypatch):
    from flasht5_amd import logits_process
    m = _model("t5_rpe", seed=2).to(DEV).bfloat16()
    ids = torch.randint(2, 256, (2, 17), generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = []
    real = logits_process.process_logits
    monkeypatch.setattr(logits_process, "process_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for graph in (False, True):
        a = m.generate(ids, max_length=12, graph=graph, **kw)
        b = m.generate(ids, max_length=12, graph=graph, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0,
                       suppress_tokens=None, **kw)
        c = m.generate(ids, max_length=12, graph=graph, suppress_tokens=[], **kw)
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not calls
    m.generate(ids, max_length=12, min_length=3, **kw)
    assert calls  # (the counter does see the call when a processor is on)
