"""GPU tests of the six further logits processors (encoder repetition penalty, encoder no-repeat n-grams, bad words,
min_new_tokens, forced BOS / EOS) in fat5_process_logits: the kernel bit for bit against the restatement
(tests/logits_proc_ext_ref.py) without log_softmax -- only exact fp32 operations are involved -- and with it on rows whose lse is
exact in fp32 (tests/test_logits_proc_gpu.py's constructions); the encoder-length edges of the 512-thread workgroup and its LDS;
the beam mapping, ragged prompt lengths and the device-side guards; the in-place fp32 call of the C ABI; determinism and graph
replay; and greedy, sampled and beam `generate` against the restatement loop over the decode path's own per-step logits, with
direct properties of the outputs, padding, ragged decoder prompts and the FP8 caches."""
import ctypes

import pytest
import torch

import beam_ref
import logits_proc_ext_ref as ref
from test_logits_proc_gpu import STATE, _bits, _case, _exact_rows, _model, _strided

pytestmark = pytest.mark.gpu

DEV = "cuda"
NINF = float("-inf")
MAX_NEW = 7   # (_case has a row of length 7: with P = 1 it sits at s - P = max_new_tokens - 1)


def _dev(v):
    return v.to(DEV) if torch.is_tensor(v) else v


def _kernel(xd, view, lens, cfg, ctx, **kw):
    from flasht5_amd import process_logits
    return process_logits(xd, view, lens.to(DEV), **cfg, **{k: _dev(v) for k, v in ctx.items()}, **kw)


def _encoder(seqs, V, Le, enc_rows, g, bad_entries=True):
    """encoder rows that share tokens and n-grams with the sequences (half of the ids are drawn from a sequence row's own
    tokens), with vocabulary-wide ids in between and, with bad_entries, entries outside the vocabulary"""
    rows, L = seqs.shape
    src = seqs[torch.arange(enc_rows) * (rows // enc_rows)].clamp(0, V - 1)
    enc = src[:, torch.randint(0, L, (Le,), generator=g)]
    wide = torch.rand(enc_rows, Le, generator=g) < 0.3
    enc = torch.where(wide, torch.randint(0, V, (enc_rows, Le), generator=g), enc)
    if bad_entries and Le > 3:
        enc[0, 1], enc[-1, 2] = -1, V + 3
    return enc


def _context(x, seqs, lens, V, g, Le=37, k=1):
    """encoder ids with per-row lengths below 0, inside and above the buffer, and ragged prompt lengths"""
    rows = x.shape[0]
    enc = _encoder(seqs, V, Le, rows // k, g)
    el = torch.randint(-1, Le + 4, (rows // k,), generator=g).int()
    el[0] = Le
    pl = torch.randint(1, 5, (rows,), generator=g).int()
    pl[10 % rows] = 1
    return dict(encoder_input_ids=enc, encoder_lengths=el, rows_per_encoder_row=k, prompt_lengths=pl, max_new_tokens=MAX_NEW)


def _bad_words(seqs, lens, V):
    """length 1, 2 and 3, one matching the tail of row 5 (length L), two ending in the same token, and [eos]"""
    r, s = 5, int(lens[5])
    tail = [int(t) % V for t in seqs[r, s - 2:s]]
    return [[V - 1], [1], [tail[1], 3 % V], [tail[0], tail[1], 2 % V], [0, 3 % V], [int(seqs[10, 6]) % V, 4 % V]]


def _configs(seqs, lens, V):
    bad = _bad_words(seqs, lens, V)
    return [dict(encoder_repetition_penalty=1.4), dict(encoder_repetition_penalty=0.7, repetition_penalty=1.3),
            dict(encoder_no_repeat_ngram_size=1), dict(encoder_no_repeat_ngram_size=2), dict(encoder_no_repeat_ngram_size=3),
            dict(bad_words_ids=bad), dict(min_new_tokens=3), dict(forced_bos_token_id=3 % V), dict(forced_eos_token_id=1),
            dict(forced_bos_token_id=2, forced_eos_token_id=1, suppress_tokens=[1, 3 % V]),
            dict(encoder_repetition_penalty=1.4, repetition_penalty=1.2, no_repeat_ngram_size=2, encoder_no_repeat_ngram_size=2,
                 bad_words_ids=bad, min_length=4, min_new_tokens=3, forced_bos_token_id=2, forced_eos_token_id=1, suppress_tokens=[2])]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V, pad", [(5, 0), (5, 3), (1000, 0), (1000, 5), (32128, 0), (32128, 1)])
def test_kernel_bitwise_against_restatement(dtype, V, pad):
    g = torch.Generator().manual_seed(7 * V + pad)
    L = 40
    x, seqs, view, lens = _case(V, L, 2, g, dtype)
    ctx = _context(x, seqs, lens, V, g)
    xd = _strided(x.to(DEV), V + pad) if pad else x.to(DEV)
    plain = x.float()
    for cfg in _configs(seqs, lens, V):
        y = _kernel(xd, view, lens, cfg, ctx)
        want = ref.process(x, seqs, lens, **cfg, **ctx)
        assert y.dtype == torch.float32 and y.shape == (x.shape[0], V)
        assert torch.equal(_bits(y), _bits(want)), (cfg, (_bits(y) != _bits(want)).nonzero()[:8])
        assert not torch.equal(_bits(want), _bits(plain)), cfg   # (the processor acted on some row)


def test_kernel_bitwise_large_vocabulary():
    V = 250112
    g = torch.Generator().manual_seed(V)
    x, seqs, view, lens = _case(V, 40, 2, g, torch.bfloat16)
    ctx = _context(x, seqs, lens, V, g)
    xd = _strided(x.to(DEV), V + 3)
    cfg = _configs(seqs, lens, V)[-1]
    for c in (cfg, dict(cfg, forced_bos_token_id=V - 1, forced_eos_token_id=None)):
        assert torch.equal(_bits(_kernel(xd, view, lens, c, ctx)), _bits(ref.process(x, seqs, lens, **c, **ctx))), c


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_encoder_length_edges(dtype):
    """encoder lengths 1, n - 1, n and around the 512 threads and the 4096-entry LDS copy; 1 to 3 rows"""
    V, L, n = 32128, 24, 3
    g = torch.Generator().manual_seed(31)
    for i, Le in enumerate([1, n - 1, n, 511, 512, 513, 4096]):
        rows = 1 + i % 3
        seqs = torch.randint(0, 6, (rows, L), generator=g)
        lens = torch.randint(n, L + 1, (rows,), generator=g).int()
        x = (torch.randn(rows, V, generator=g) * 3.0).to(dtype)
        enc = torch.randint(0, 6, (rows, Le), generator=g)
        far = torch.rand(rows, Le, generator=g) < 0.5
        enc = torch.where(far, torch.randint(0, V, (rows, Le), generator=g), enc)
        enc[:, -1] = V - 1 - torch.arange(rows)   # (the last id of every row: one past a wrong bound is missed or read)
        ctx = dict(encoder_input_ids=enc, max_new_tokens=9)
        for cfg in (dict(encoder_repetition_penalty=1.4, repetition_penalty=1.3, encoder_no_repeat_ngram_size=n),
                    dict(encoder_repetition_penalty=0.7, encoder_no_repeat_ngram_size=1),
                    dict(encoder_no_repeat_ngram_size=min(2, Le))):
            want = ref.process(x, seqs, lens, **cfg, **ctx)
            y = _kernel(x.to(DEV), seqs.to(DEV), lens, cfg, ctx)
            assert torch.equal(_bits(y), _bits(want)), (Le, cfg, (_bits(y) != _bits(want)).nonzero()[:8])
        short = dict(ctx, encoder_lengths=torch.full((rows,), Le - 1, dtype=torch.int32))   # (the last id is outside the length)
        cfg = dict(encoder_repetition_penalty=1.4, encoder_no_repeat_ngram_size=1)
        y = _kernel(x.to(DEV), seqs.to(DEV), lens, cfg, short)
        assert torch.equal(_bits(y), _bits(ref.process(x, seqs, lens, **cfg, **short))), Le
    with pytest.raises(ValueError, match="4096"):
        _kernel(x.to(DEV), seqs.to(DEV), lens, dict(encoder_no_repeat_ngram_size=2), dict(encoder_input_ids=torch.zeros(rows, 4097, dtype=torch.long)))


def test_beam_rows_and_ragged_prompt_lengths():
    """k = 3: rows 0..2 read encoder row 0, rows 3..5 encoder row 1, each inside its own length; every row its own P_r"""
    V, L, k = 1000, 30, 3
    g = torch.Generator().manual_seed(41)
    seqs = torch.randint(0, 5, (2 * k, L), generator=g)
    lens = torch.tensor([1, 4, 9, 12, 30, 6], dtype=torch.int32)
    x = torch.randn(2 * k, V, generator=g).bfloat16()
    enc = torch.stack([torch.randint(0, 5, (20,), generator=g), torch.randint(5, 10, (20,), generator=g)])
    enc[1, :4] = seqs[4, 26:30]
    ctx = dict(encoder_input_ids=enc, encoder_lengths=torch.tensor([20, 11], dtype=torch.int32), rows_per_encoder_row=k,
               prompt_lengths=torch.tensor([1, 2, 3, 6, 24, 1], dtype=torch.int32), max_new_tokens=7)
    cfg = dict(encoder_repetition_penalty=1.4, encoder_no_repeat_ngram_size=3, min_new_tokens=3, forced_eos_token_id=1, forced_bos_token_id=4)
    y = _kernel(x.to(DEV), seqs.to(DEV), lens, cfg, ctx).cpu()
    want = ref.process(x, seqs, lens, **cfg, **ctx)
    assert torch.equal(_bits(y), _bits(want))
    forced = torch.full((V,), NINF)
    assert torch.equal(y[0], forced.index_fill(0, torch.tensor([4]), 0.0))      # s = 1: the forced BOS
    for r in (2, 3, 4):                                                         # s - P_r = 6 = max_new_tokens - 1
        assert torch.equal(y[r], forced.index_fill(0, torch.tensor([1]), 0.0)), r
    assert y[1, 1] == NINF                                                      # min_new_tokens: 4 - 2 < 3
    swapped = ref.process(x, seqs, lens, **cfg, **dict(ctx, encoder_input_ids=enc.flip(0), encoder_lengths=ctx["encoder_lengths"].flip(0)))
    assert not torch.equal(_bits(want[1]), _bits(swapped[1])) and not torch.equal(_bits(want[5]), _bits(swapped[5]))   # (the mapping matters)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V, pad", [(1000, 5), (32128, 0)])
def test_log_softmax_on_exact_lse_rows(dtype, V, pad):
    g = torch.Generator().manual_seed(3 * V + pad)
    L = 24
    _, seqs, view, lens = _case(V, L, 2, g, dtype, pos_inf=False)
    x = _exact_rows(len(lens), V, g, dtype)
    ctx = _context(x, seqs, lens, V, g)
    xd = _strided(x.to(DEV), V + pad) if pad else x.to(DEV)
    for cfg in _configs(seqs, lens, V)[-2:]:
        y = _kernel(xd, view, lens, cfg, ctx, log_softmax=True)
        want = ref.process(x, seqs, lens, log_softmax=True, **cfg, **ctx)
        assert torch.equal(_bits(y), _bits(want)), cfg


def test_in_place_fp32_through_the_c_abi():
    """out == logits (fp32) with every new processor on: each edit is computed from the input value, so the result is the
    out-of-place one bit for bit"""
    from flasht5_amd import _lib, pack_bad_words
    g = torch.Generator().manual_seed(19)
    V, L = 1000, 24
    for ls in (False, True):
        x, seqs, view, lens = _case(V, L, 2, g, torch.float32, pos_inf=not ls)
        ctx = _context(x, seqs, lens, V, g)
        cfg = _configs(seqs, lens, V)[-1]
        xd, ld = x.to(DEV), lens.to(DEV)
        seq_d = seqs.clamp(-1, V).to(DEV).contiguous()
        want = _kernel(xd, seq_d, lens, cfg, ctx, log_softmax=ls)
        assert torch.equal(_bits(want), _bits(ref.process(x, seqs, lens, **cfg, **ctx))) or ls
        enc, el, pl = (ctx[n].to(DEV) for n in ("encoder_input_ids", "encoder_lengths", "prompt_lengths"))
        bad = pack_bad_words(cfg["bad_words_ids"], DEV)
        sup = torch.tensor(cfg["suppress_tokens"], dtype=torch.int32, device=DEV)
        off = (ctypes.c_int32 * len(bad.host_offsets))(*bad.host_offsets)
        p = _lib.LogitsParams()
        p.rows, p.V, p.dtype, p.log_softmax = x.shape[0], V, _lib.FAT5_F32, int(ls)
        p.logits, p.row_stride, p.out, p.out_stride = xd.data_ptr(), V, xd.data_ptr(), V
        p.sequences, p.seq_stride, p.seq_len, p.lengths = seq_d.data_ptr(), L, L, ld.data_ptr()
        p.repetition_penalty, p.no_repeat_ngram_size, p.min_length, p.eos_token_id = 1.2, 2, 4, 1
        p.n_suppress, p.suppress_tokens = sup.numel(), sup.data_ptr()
        p.encoder_repetition_penalty, p.encoder_no_repeat_ngram_size = 1.4, 2
        p.encoder_input_ids, p.encoder_stride, p.encoder_lengths = enc.data_ptr(), enc.shape[1], el.data_ptr()
        p.encoder_rows, p.encoder_len, p.rows_per_encoder_row = enc.shape[0], enc.shape[1], 1
        p.bad_words_ids, p.bad_words_offsets, p.bad_words_offsets_host = bad.ids.data_ptr(), bad.offsets.data_ptr(), ctypes.addressof(off)
        p.n_bad_words, p.n_bad_word_ids = len(off) - 1, bad.ids.numel()
        p.min_new_tokens, p.prompt_lengths, p.max_new_tokens = 3, pl.data_ptr(), MAX_NEW
        p.forced_tokens, p.forced_bos_token_id, p.forced_eos_token_id = _lib.FAT5_FORCED_BOS | _lib.FAT5_FORCED_EOS, 2, 1
        _lib.check(_lib.load().fat5_process_logits(ctypes.byref(p), _lib.stream_ptr(xd.device)), "fat5_process_logits")
        torch.cuda.synchronize()
        assert torch.equal(_bits(xd), _bits(want)), ls


def test_deterministic_and_graph_replay():
    """two runs and a replayed graph, with lengths, sequences, encoder ids and prompt lengths changed on the device between the
    replays, give the restatement's bits each time"""
    from flasht5_amd import pack_bad_words, process_logits
    g = torch.Generator().manual_seed(29)
    rows, V, L, Le, N = 6, 32128, 32, 520, 5
    cfg = dict(encoder_repetition_penalty=1.4, repetition_penalty=1.2, no_repeat_ngram_size=2, encoder_no_repeat_ngram_size=2,
               min_length=3, min_new_tokens=4, forced_bos_token_id=9, forced_eos_token_id=1, max_new_tokens=12)
    words = [[5], [1, 2], [3, 4, 5], [0, 2]]
    bad = pack_bad_words(words, DEV)
    sup = torch.tensor([6, 7], dtype=torch.int32, device=DEV)
    xs = [(torch.randn(rows, V, generator=g) * 3).bfloat16().to(DEV) for _ in range(N)]
    sq = [torch.randint(0, 6, (rows, L), generator=g).to(DEV) for _ in range(N)]
    ln = [torch.randint(0, L + 1, (rows,), generator=g).int().to(DEV) for _ in range(N)]
    en = [torch.randint(0, 8, (rows, Le), generator=g).to(DEV) for _ in range(N)]
    el = [torch.randint(0, Le + 1, (rows,), generator=g).int().to(DEV) for _ in range(N)]
    pl = [torch.randint(1, 6, (rows,), generator=g).int().to(DEV) for _ in range(N)]
    for i in range(N):
        ln[i][0], pl[i][0] = 15 + i % 2, 4    # (row 0 at the forced EOS on every other replay)

    def run(x, s, n, e, m, q, b):
        return process_logits(x, s, n, suppress_tokens=sup, bad_words_ids=b, encoder_input_ids=e, encoder_lengths=m, prompt_lengths=q, **cfg)

    a = [run(xs[i], sq[i], ln[i], en[i], el[i], pl[i], bad).clone() for i in range(N)]
    b = [run(xs[i], sq[i], ln[i], en[i], el[i], pl[i], words).clone() for i in range(N)]
    for i in range(N):
        want = ref.process(xs[i], sq[i], ln[i], suppress_tokens=sup, bad_words_ids=words, encoder_input_ids=en[i], encoder_lengths=el[i],
                           prompt_lengths=pl[i], **cfg)
        assert torch.equal(_bits(a[i]), _bits(want)) and torch.equal(_bits(a[i]), _bits(b[i])), i
    bufs = [t[0].clone() for t in (xs, sq, ln, en, el, pl)]
    run(*bufs, bad)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(*bufs, bad)
        with pytest.raises(ValueError, match="graph capture"):
            run(*bufs, words)   # (a host list cannot be packed inside a capture)
    for i in range(N):
        for buf, src in zip(bufs, (xs, sq, ln, en, el, pl)):
            buf.copy_(src[i])
        graph.replay()
        assert torch.equal(_bits(out), _bits(a[i])), i
    del graph


# ------------------------------------------------------------------------------------------------ generate
MAXLEN = 16
PROC = dict(encoder_repetition_penalty=1.4, repetition_penalty=1.2, encoder_no_repeat_ngram_size=2, bad_words_ids=[[7], [1], [8, 9]],
            min_new_tokens=6, forced_bos_token_id=11, forced_eos_token_id=1, suppress_tokens=[200])


def _eos_model(seed):
    m = _model("t5_rpe", seed=seed).to(DEV).bfloat16()
    with torch.no_grad():
        m.lm_head.weight[1].mul_(3.0)   # (EOS wanted early: min_new_tokens has something to hold back)
    return m


@pytest.mark.parametrize("mode", ["greedy", "sample"])
def test_generate_greedy_and_sampled_match_restatement_loop(mode):
    from flasht5_amd import sample_logits
    from flasht5_amd.generation import decode_step, finish_labels, init_decode_state
    m = _eos_model(0)
    B = 3
    ids = torch.randint(2, 256, (B, 21), generator=torch.Generator().manual_seed(100)).to(DEV)
    skw = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=1234) if mode == "sample" else {}
    with torch.no_grad():
        state = init_decode_state(m, ids, MAXLEN)
        labels = torch.zeros(B, MAXLEN + 1, dtype=torch.long)
        tok = torch.zeros(B, dtype=torch.long, device=DEV)
        seen = torch.zeros(B, dtype=torch.bool)
        steps = 0
        for s in range(1, MAXLEN + 1):
            lg = decode_step(m, state, tok)
            y = ref.process(lg, labels, torch.full((B,), s, dtype=torch.int32), encoder_input_ids=ids, max_new_tokens=MAXLEN, **PROC).to(DEV)
            nxt = sample_logits(y, 0.8, 20, 0.9, seed=1234, offsets=state.cache_seqlens) if mode == "sample" else y.argmax(-1)
            tok.copy_(nxt)
            labels[:, s] = nxt.cpu()
            seen |= nxt.cpu() == 1
            steps = s
            if bool(seen.all()):
                break
        want = finish_labels(labels[:, :steps + 1])
        a = m.generate(ids, max_length=MAXLEN, **skw, **PROC)
        b = m.generate(ids, max_length=MAXLEN, graph=True, **skw, **PROC)
    assert torch.equal(a.cpu(), want), (mode, a, want)
    assert torch.equal(a, b), mode
    _check_properties(a, ids, None, [1] * B, MAXLEN)


def _check_properties(out, ids, enc_lens, P, max_length, n=2, words=((7,), (8, 9)), min_new=6, bos=11, suppressed=(200,)):
    """per row, over the windows that end at a generated position up to the row's EOS: no encoder n-gram is copied, no bad word
    occurs, no suppressed id; no EOS before min_new_tokens; the forced BOS behind a lone start token; an unfinished row ends in
    the EOS at its own P_r + max_length - 1"""
    for r, row in enumerate(out.cpu().tolist()):
        e = ids[r].cpu().tolist()[:None if enc_lens is None else enc_lens[r]]
        grams = {tuple(e[i:i + n]) for i in range(len(e) - n + 1)}
        end = row.index(1) + 1 if 1 in row[P[r]:] else len(row)
        assert 1 in row[P[r]:] and row.index(1) >= P[r] + min_new, row
        assert row.index(1) <= P[r] + max_length - 1, row
        if P[r] == 1:
            assert row[1] == bos, row
        for j in range(P[r], end):
            assert tuple(row[j - n + 1:j + 1]) not in grams, (row, j)
            assert row[j] not in suppressed
            for w in words:
                assert j + 1 < len(w) or tuple(row[j + 1 - len(w):j + 1]) != w, (row, j, w)


@pytest.mark.parametrize("opts", [dict(num_beams=4, length_penalty=2.0, early_stopping=True, num_return_sequences=1),
                                  dict(num_beams=3, length_penalty=1.0, early_stopping=False, num_return_sequences=3)])
def test_generate_beam_matches_restatement_loop(opts):
    """every step: the kernel's processed rows equal the restatement's edits applied to the kernel's own log-probabilities bit
    for bit, and the beam state equals the restatement's step over them; generate() returns what the loop returned, eager and
    replayed; every returned hypothesis ends in the forced EOS"""
    from flasht5_amd import process_logits
    from flasht5_amd.beam import beam_step, keep_going, new_state
    from flasht5_amd.generation import decode_step, init_decode_state
    import logits_proc_ref as base
    k, R, lp, es = opts["num_beams"], opts["num_return_sequences"], opts["length_penalty"], opts["early_stopping"]
    m = _eos_model(1)
    B = 2
    ids = torch.randint(2, 256, (B, 21), generator=torch.Generator().manual_seed(200)).to(DEV)
    ctx = dict(encoder_input_ids=ids, rows_per_encoder_row=k, max_new_tokens=MAXLEN)
    with torch.no_grad():
        state = init_decode_state(m, ids, MAXLEN, num_beams=k)
        bs = new_state(B, k, MAXLEN + 1, state.capacity, DEV)
        bs.cache_row_batch = state.row_batch
        rst = beam_ref.init(B, k, MAXLEN + 1, state.capacity)
        for s in range(1, MAXLEN + 1):
            seqs = bs.running_seqs.view(B * k, -1)
            lg = decode_step(m, state, seqs[:, s - 1].contiguous())
            logp = process_logits(lg, seqs, state.cache_seqlens, log_softmax=True)
            y = process_logits(lg, seqs, state.cache_seqlens, log_softmax=True, **PROC, **ctx)
            want = ref.process(logp, seqs.cpu(), state.cache_seqlens.cpu(), **PROC, **ctx)
            assert torch.equal(_bits(y), _bits(want)), s
            beam_step(y, bs, state.cache_seqlens, MAXLEN, lp, es, logits_normalized=True)
            base.beam_step_normalized(rst, want, s, MAXLEN, lp, es)
            for name in STATE:
                assert torch.equal(getattr(bs, name).cpu(), rst[name]), (s, name)
            if not bool(keep_going(bs.status, es)):
                break
        T = int(bs.finished_lens[:, :R].max())
        loop_out = bs.finished_seqs[:, :R].reshape(B * R, -1)[:, :T + 1]
        a, sa = m.generate(ids, max_length=MAXLEN, return_scores=True, **opts, **PROC)
        b, sb = m.generate(ids, max_length=MAXLEN, graph=True, return_scores=True, **opts, **PROC)
    assert torch.equal(a, loop_out) and torch.equal(sa, bs.finished_scores[:, :R].reshape(-1))
    assert torch.equal(a, b) and torch.equal(sa, sb)
    _check_properties(a, ids.repeat_interleave(R, 0), None, [1] * (B * R), MAXLEN)


def test_ragged_decoder_prompts_count_from_each_rows_own_prompt():
    """min_new_tokens and the forced EOS are per row under decoder_attention_mask: each row equals the same row generated
    alone with its own prompt, eager and replayed"""
    m = _eos_model(2)
    ids = torch.randint(2, 256, (3, 21), generator=torch.Generator().manual_seed(300)).to(DEV)
    prompt = torch.tensor([[0, 5, 6], [0, 5, 0], [0, 0, 0]]).to(DEV)
    dmask = torch.tensor([[1, 1, 1], [1, 1, 0], [1, 0, 0]]).to(DEV)
    P = [3, 2, 1]
    kw = dict(max_length=9, **PROC)
    a = m.generate(ids, decoder_input_ids=prompt, decoder_attention_mask=dmask, **kw)
    b = m.generate(ids, decoder_input_ids=prompt, decoder_attention_mask=dmask, graph=True, **kw)
    assert torch.equal(a, b)
    _check_properties(a, ids, None, P, 9)
    for r in range(3):
        one = m.generate(ids[r:r + 1], decoder_input_ids=prompt[r:r + 1, :P[r]], **kw)
        assert torch.equal(a[r, :one.shape[1]], one[0]) and not bool(a[r, one.shape[1]:].any()), r


def test_padded_rows_equal_the_rows_alone_and_fp8():
    """the encoder ids of a row are those inside its attention_mask: a padded batch row -- its padding filled with ids the row
    itself produces, which a processor that read the padding would ban -- equals the row generated alone, in greedy and beam
    mode; and the FP8 caches give the same tokens (a decisive model, tests/test_kvfp8_generation_gpu.py)"""
    from test_kvfp8_generation_gpu import _decisive
    m, _ = _decisive("t5_rpe", 3)
    V = m.config.vocab_size
    lens = [33, 20, 9]
    ids = torch.randint(2, V, (3, 33), generator=torch.Generator().manual_seed(103)).to(DEV)
    mask = torch.ones_like(ids)
    proc = dict(encoder_repetition_penalty=1.4, encoder_no_repeat_ngram_size=1, min_new_tokens=5, forced_eos_token_id=1, bad_words_ids=[[3]])
    alone = [m.generate(ids[r:r + 1, :n], max_length=MAXLEN, **proc) for r, n in enumerate(lens)]
    for r, n in enumerate(lens):
        mask[r, n:] = 0
        fill = alone[r][0, 1:][alone[r][0, 1:] > 1]
        ids[r, n:] = fill[torch.arange(33 - n, device=DEV) % len(fill)]
    for kw in (dict(), dict(graph=True), dict(kv_cache_dtype="fp8"), dict(num_beams=3)):
        got = m.generate(ids, mask, max_length=MAXLEN, **proc, **kw)
        for r, n in enumerate(lens):
            one = alone[r] if "num_beams" not in kw else m.generate(ids[r:r + 1, :n], max_length=MAXLEN, **proc, **kw)
            assert torch.equal(got[r, :one.shape[1]], one[0]) and not bool(got[r, one.shape[1]:].any()), (kw, r)
            assert not set(got[r, 1:].tolist()) & set(ids[r, :n].tolist()), (kw, r)   # (n = 1: no encoder id is produced)
    assert any(a.shape[1] > 6 for a in alone)
