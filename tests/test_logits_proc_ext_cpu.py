"""CPU tests of the six further logits processors (encoder repetition penalty, encoder no-repeat n-grams, bad words,
min_new_tokens, forced BOS / EOS): the restatement (tests/logits_proc_ext_ref.py) against HF's ten processor classes chained in
`_get_logits_processor`'s order and against HF's own `generate(...)` on the tiny T5 of tests/test_logits_proc_cpu.py, the appended
fields of fat5_logits_params (sizes, all-zero = the call as it was, rejections before any launch: fake pointers are enough), the
custom op's fake implementation with and without the appended arguments, and the host checks of `generate`."""
import ctypes
import itertools

import pytest
import torch

import logits_proc_ext_ref as ref
from test_logits_proc_cpu import BASE, BEAM, PROCS, _finish, _given_logits, _hf_model, _params, _small_model

NINF = float("-inf")


# ------------------------------------------------------------------------------------------------ the restatement against HF
def _hf_chain(enc, P=1, max_new=0, phi=1.0, theta=1.0, n=0, ne=0, bad=None, m=0, mn=0, fbos=None, feos=None, sup=None):
    """HF's classes in `GenerationMixin._get_logits_processor`'s order"""
    tf = pytest.importorskip("transformers")
    chain = tf.LogitsProcessorList()
    chain.append(tf.EncoderRepetitionPenaltyLogitsProcessor(penalty=phi, encoder_input_ids=enc))
    chain.append(tf.RepetitionPenaltyLogitsProcessor(penalty=theta))
    if n:
        chain.append(tf.NoRepeatNGramLogitsProcessor(n))
    if ne:
        chain.append(tf.EncoderNoRepeatNGramLogitsProcessor(ne, enc))
    if bad and ref.kept_bad_words(bad):   # (HF's class raises when only [eos] entries were given)
        chain.append(tf.NoBadWordsLogitsProcessor(bad, eos_token_id=1))
    if m:
        chain.append(tf.MinLengthLogitsProcessor(m, 1, device="cpu"))
    if mn:
        chain.append(tf.MinNewTokensLengthLogitsProcessor(P, mn, 1, device="cpu"))
    if fbos is not None:
        chain.append(tf.ForcedBOSTokenLogitsProcessor(fbos))
    if feos is not None:
        chain.append(tf.ForcedEOSTokenLogitsProcessor(P + max_new, feos, device="cpu"))
    if sup:
        chain.append(tf.SuppressTokensLogitsProcessor(sup, device="cpu"))
    return chain


def _mine(logits, seqs, s, enc, P=1, max_new=0, phi=1.0, theta=1.0, n=0, ne=0, bad=None, m=0, mn=0, fbos=None, feos=None, sup=None):
    rows = logits.shape[0]
    return ref.process(logits, seqs, torch.full((rows,), s, dtype=torch.int32), encoder_input_ids=enc, prompt_length=P,
                       max_new_tokens=max_new, encoder_repetition_penalty=phi, repetition_penalty=theta, no_repeat_ngram_size=n,
                       encoder_no_repeat_ngram_size=ne, bad_words_ids=bad, min_length=m, min_new_tokens=mn, forced_bos_token_id=fbos,
                       forced_eos_token_id=feos, suppress_tokens=sup)


def _rows(g, rows, V, L, Le, alphabet=5):
    """sequences and encoder rows over a small alphabet (tokens in both sets, repeated n-grams in the encoder rows), logits with
    positive, negative, zero and -inf entries on tokens of both sets"""
    seqs = torch.randint(0, alphabet, (rows, L), generator=g)
    seqs[:, 0] = 0
    enc = torch.randint(1, alphabet + 1, (rows, Le), generator=g)
    enc[:, Le - 3:] = enc[:, :3]          # (the first 3-gram once more: a repeated encoder n-gram)
    logits = torch.randn(rows, V, generator=g) * 3.0
    logits[0, 1], logits[0, 2], logits[1, 3], logits[1, 4] = 0.0, NINF, 0.0, NINF
    logits[2, 0], logits[3, 5] = NINF, 0.0
    return logits, seqs, enc


@pytest.mark.parametrize("theta", [0.8, 1.0, 1.3])
@pytest.mark.parametrize("phi", [0.7, 1.0, 1.4])
def test_restatement_equals_hf_chain(phi, theta):
    V, L, Le, rows = 13, 10, 9, 5
    g = torch.Generator().manual_seed(int(phi * 100) + int(theta * 10))
    bad = [[6], [1], [2, 3], [4, 3], [1, 2, 3], [0, 1]]
    for s in range(1, L + 1):
        logits, seqs, enc = _rows(g, rows, V, L, Le)
        for ne, n, b, fe in itertools.product((0, 1, 2, 3, 4), (0, 2), (None, bad), (None, 7)):
            kw = dict(phi=phi, theta=theta, n=n, ne=ne, bad=b, m=4, mn=3, feos=fe, max_new=6, sup=[7] if ne == 2 else None)
            hf = _hf_chain(enc, **kw)(seqs[:, :s], logits.clone())
            assert torch.equal(hf, _mine(logits, seqs, s, enc, **kw)), (s, kw)


@pytest.mark.parametrize("ne", [1, 2, 3, 4])
def test_encoder_ngrams_at_the_first_lengths(ne):
    """nothing is banned while s < n - 1 (HF's slice is then shorter than a key), n = 1 bans every encoder id"""
    V, L, Le, rows = 9, 8, 7, 6
    g = torch.Generator().manual_seed(ne)
    hit = 0
    for s in sorted({max(ne - 2, 1), max(ne - 1, 1), ne, ne + 1, L}):
        logits, seqs, enc = _rows(g, rows, V, L, Le, alphabet=3)
        if ne > 1 and s >= ne - 1:
            seqs[0, s - ne + 1:s] = enc[0, :ne - 1]   # (row 0 ends in the encoder row's first n - 1 ids)
        hf = _hf_chain(enc, ne=ne)(seqs[:, :s], logits.clone())
        mine = _mine(logits, seqs, s, enc, ne=ne)
        assert torch.equal(hf, mine), s
        if s < ne - 1:
            assert torch.equal(mine, logits)
        hit += int((mine != logits).any())
    assert hit
    if ne == 1:
        assert bool((mine[0, enc[0]] == NINF).all())


def test_bad_words_lengths_and_the_context_rule():
    """length 1 always; length L > 1 needs s >= L (HF skips a sequence longer than the context: at s = L - 1 the prefix could
    match and still nothing is banned); two sequences ending in the same token; an [eos] entry is dropped"""
    V, L = 10, 6
    logits = torch.linspace(-2.0, 2.0, V).repeat(2, 1)
    seqs = torch.tensor([[0, 4, 5, 6, 4, 5], [0, 5, 4, 5, 5, 4]])
    enc = torch.zeros(2, 1, dtype=torch.long)
    for s in range(1, L + 1):
        for bad in ([[9]], [[4, 5]], [[0, 4, 5]], [[4, 5], [6, 5]], [[5, 6], [4, 6]], [[1], [4, 5]], [[1]],
                    [seqs[0, :s].tolist() + [8]] if s > 0 else [[8]], [seqs[0, 1:s].tolist() + [8]]):
            hf = _hf_chain(enc, bad=bad)(seqs[:, :s], logits.clone())
            mine = _mine(logits, seqs, s, enc, bad=bad)
            assert torch.equal(hf, mine), (s, bad)
            if bad == [[1]]:
                assert torch.equal(mine, logits)       # dropped: EOS stays
            if bad == [seqs[0, :s].tolist() + [8]]:    # L = s + 1: longer than the context
                assert mine[0, 8] == logits[0, 8]
            if bad == [seqs[0, 1:s].tolist() + [8]]:   # L = s (for s = 1 the length-1 sequence [8])
                assert mine[0, 8] == NINF
    assert _mine(logits, seqs, 3, enc, bad=[[4, 5]])[0, 5] == logits[0, 5]   # ... 4 5 | ends in 5, not in 4
    assert _mine(logits, seqs, 2, enc, bad=[[4, 5]])[0, 5] == NINF


@pytest.mark.parametrize("P", [1, 3])
def test_min_new_tokens_counts_from_the_prompt(P):
    V, L = 8, 9
    g = torch.Generator().manual_seed(P)
    logits = torch.randn(3, V, generator=g)
    seqs = torch.randint(2, V, (3, L), generator=g)
    enc = torch.zeros(3, 1, dtype=torch.long)
    for s, mn in itertools.product(range(P, L + 1), (1, 2, 4)):
        hf = _hf_chain(enc, P=P, mn=mn, m=2)(seqs[:, :s], logits.clone())
        mine = _mine(logits, seqs, s, enc, P=P, mn=mn, m=2)
        assert torch.equal(hf, mine), (s, mn)
        assert bool((mine[:, 1] == NINF).all()) == (s - P < mn or s < 2)


@pytest.mark.parametrize("fbos, feos", [(None, None), (5, None), (None, 1), (5, 1), (5, 6), (6, 6)])
def test_forced_tokens(fbos, feos):
    """on, off and coinciding (P = 1, max_new_tokens = 1: both fire at s = 1 and the EOS decides), the forced id suppressed too"""
    V, L = 8, 6
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, V, generator=g)
    seqs = torch.randint(2, V, (2, L), generator=g)
    enc = torch.randint(2, V, (2, 4), generator=g)
    for s, max_new, P, sup in itertools.product(range(1, L + 1), (1, 3), (1, 2), (None, [6], [1, 5])):
        if s < P:
            continue
        kw = dict(P=P, max_new=max_new, fbos=fbos, feos=feos, sup=sup, phi=1.4, theta=1.3, ne=2, mn=2)
        hf = _hf_chain(enc, **kw)(seqs[:, :s], logits.clone())
        mine = _mine(logits, seqs, s, enc, **kw)
        assert torch.equal(hf, mine), (s, kw)
        if feos is not None and s - P == max_new - 1:
            want = torch.full((V,), NINF)
            want[feos] = 0.0
            for t in sup or []:
                want[t] = NINF
            assert torch.equal(mine[0], want)
        elif fbos is not None and s == 1:
            assert mine[0, fbos] == (NINF if fbos in (sup or []) else 0.0) and int((mine[0] > NINF).sum()) <= 1


def test_per_row_encoder_lengths_prompt_lengths_and_beam_rows():
    """row r reads encoder row r // k inside its own length, and its own P_r; entries outside the vocabulary are no tokens"""
    V, L, Le, k = 9, 7, 6, 3
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(2 * k, V, generator=g)
    seqs = torch.randint(0, 4, (2 * k, L), generator=g)
    enc = torch.randint(0, 4, (2, Le), generator=g)
    enc[1, 2], enc[1, 3] = -1, V + 2
    el = torch.tensor([4, 9], dtype=torch.int32)
    pl = torch.tensor([1, 2, 3, 1, 4, 2], dtype=torch.int32)
    lens = torch.tensor([3, 4, 5, 6, 7, 2], dtype=torch.int32)
    kw = dict(encoder_repetition_penalty=1.4, encoder_no_repeat_ngram_size=2, min_new_tokens=2, forced_eos_token_id=1, max_new_tokens=3)
    y = ref.process(logits, seqs, lens, encoder_input_ids=enc, encoder_lengths=el, rows_per_encoder_row=k, prompt_lengths=pl, **kw)
    for r in range(2 * k):
        e = enc[r // k, :min(int(el[r // k]), Le)].unsqueeze(0)
        one = ref.process(logits[r:r + 1], seqs[r:r + 1], lens[r:r + 1], encoder_input_ids=e, prompt_length=int(pl[r]), **kw)
        assert torch.equal(y[r:r + 1], one), r
    assert torch.equal(y[1], torch.full((V,), NINF).index_fill(0, torch.tensor([1]), 0.0))   # s - P = 2 = max_new - 1


# ------------------------------------------------------------------------------------------------ loops against HF's generate
SUMMARISATION = dict(encoder_no_repeat_ngram_size=3, forced_eos_token_id=1, min_new_tokens=4, bad_words_ids=[[5, 9]])
EXT = [
    dict(encoder_no_repeat_ngram_size=1), dict(encoder_no_repeat_ngram_size=2, no_repeat_ngram_size=2),
    dict(encoder_repetition_penalty=1.4), dict(encoder_repetition_penalty=0.7, repetition_penalty=1.3),
    dict(bad_words_ids=[[3], [1], [5, 9], [4, 6, 2]]), dict(min_new_tokens=6), dict(forced_bos_token_id=7),
    dict(forced_eos_token_id=1, min_length=5), dict(forced_bos_token_id=7, forced_eos_token_id=1, suppress_tokens=[4, 20]),
    SUMMARISATION,
]
EXT_IDS = [str(i) for i in range(len(EXT))]


def _hf_generate(m, ids, max_length, proc, k=1, lp=1.0, es=False, R=1):
    """tests/test_logits_proc_cpu.py's `_hf_generate` with the six further arguments handed to HF's GenerationConfig"""
    from transformers import GenerationConfig
    gc = GenerationConfig(num_beams=k, max_new_tokens=max_length, length_penalty=lp, early_stopping=es, num_return_sequences=R,
                          do_sample=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, bos_token_id=None,
                          min_length=proc.get("min_length", 0), no_repeat_ngram_size=proc.get("no_repeat_ngram_size", 0),
                          repetition_penalty=proc.get("repetition_penalty", 1.0), suppress_tokens=proc.get("suppress_tokens") or None,
                          encoder_repetition_penalty=proc.get("encoder_repetition_penalty", 1.0),
                          encoder_no_repeat_ngram_size=proc.get("encoder_no_repeat_ngram_size", 0),
                          bad_words_ids=proc.get("bad_words_ids"), min_new_tokens=proc.get("min_new_tokens", 0) or None,
                          forced_bos_token_id=proc.get("forced_bos_token_id"), forced_eos_token_id=proc.get("forced_eos_token_id"),
                          return_dict_in_generate=True, output_scores=True, output_logits=True)
    with torch.no_grad():
        out = m.generate(ids, generation_config=gc)
    seqs = out.sequences.clone()
    if k > 1:
        lens = (out.beam_indices >= 0).sum(1)
        for r in range(seqs.shape[0]):
            seqs[r, 1 + int(lens[r]):] = 0
        return seqs, out.sequences_scores, out.logits
    return seqs, None, out.logits


@pytest.mark.parametrize("proc", EXT + [dict(p, **SUMMARISATION) for p in PROCS], ids=EXT_IDS + [f"old{i}" for i in range(len(PROCS))])
def test_greedy_loop_matches_hf(proc):
    for seed in range(4):
        m = _hf_model(seed)
        ids = torch.randint(2, 24, (3, 7), generator=torch.Generator().manual_seed(50 + seed))
        hs, _, hl = _hf_generate(m, ids, 12, proc)
        mine = _finish(ref.greedy(_given_logits(hl), 3, 12, proc, encoder_input_ids=ids))
        if mine.shape[1] < hs.shape[1]:   # (HF pads to the batch's longest row: the same)
            mine = torch.nn.functional.pad(mine, (0, hs.shape[1] - mine.shape[1]))
        assert torch.equal(hs, mine), (seed, hs, mine)


def _model_logits(m, ids, k):
    """the tiny T5's own next-token logits for a (B * k, s) prefix"""
    rep = ids.repeat_interleave(k, 0)

    def f(prefix):
        with torch.no_grad():
            return m(input_ids=rep, decoder_input_ids=prefix).logits[:, -1].float()
    return f


@pytest.mark.parametrize("proc", EXT, ids=EXT_IDS)
@pytest.mark.parametrize("k, lp, es", BEAM)
def test_beam_loop_matches_hf(proc, k, lp, es):
    """Against HF's own `generate`, except with encoder_repetition_penalty: HF's EncoderRepetitionPenaltyLogitsProcessor gathers
    the (B * k, V) scores with the (B, L) encoder ids, so under beams it edits only the first B rows, with the wrong rows' ids.
    Those cases are compared against HF's ten classes chained by hand over repeat_interleave'd encoder ids, both loops run
    over the model's own logits."""
    for seed, R in itertools.product(range(3), sorted({1, k})):
        m = _hf_model(seed)
        ids = torch.randint(2, 24, (2, 7), generator=torch.Generator().manual_seed(50 + seed))
        if "encoder_repetition_penalty" in proc:
            chain = _hf_chain(ids.repeat_interleave(k, 0), max_new=10, phi=proc["encoder_repetition_penalty"],
                              theta=proc.get("repetition_penalty", 1.0))
            f = _model_logits(m, ids, k)
            hs, hsc = ref.beam_search(f, 2, k, 10, {}, lp, es, R, process_fn=lambda logp, seqs, s: chain(seqs[:, :s], logp.clone()))
            rs, rsc = ref.beam_search(f, 2, k, 10, proc, lp, es, R, encoder_input_ids=ids)
        else:
            hs, hsc, hl = _hf_generate(m, ids, 10, proc, k, lp, es, R)
            rs, rsc = ref.beam_search(_given_logits(hl), 2, k, 10, proc, lp, es, R, encoder_input_ids=ids)
        assert torch.equal(hs, rs), (seed, R, hs, rs)
        assert torch.allclose(hsc, rsc, rtol=1e-5, atol=1e-5), (seed, R, hsc, rsc)


def test_summarisation_setting_properties():
    """the summarisation-style setting on HF's own output and on the loop: no encoder 3-gram is copied, the bad word does not
    occur, no EOS in the first 4 new tokens, an unfinished row ends in the forced EOS"""
    for seed in range(4):
        m = _hf_model(seed)
        ids = torch.randint(2, 24, (3, 9), generator=torch.Generator().manual_seed(80 + seed))
        hs, _, hl = _hf_generate(m, ids, 8, SUMMARISATION)
        mine = _finish(ref.greedy(_given_logits(hl), 3, 8, SUMMARISATION, encoder_input_ids=ids))
        assert torch.equal(hs, torch.nn.functional.pad(mine, (0, hs.shape[1] - mine.shape[1])))
        for r, row in enumerate(mine.tolist()):
            assert 1 in row and row.index(1) >= 5 and (row.index(1) < 8 or row[8] == 1), row
            grams = {tuple(ids[r, i:i + 3].tolist()) for i in range(7)}
            assert not any(tuple(row[i:i + 3]) in grams for i in range(row.index(1) - 1)), row
            assert not any(row[i:i + 2] == [5, 9] for i in range(len(row) - 1)), row


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


NEW_FIELDS = ["encoder_repetition_penalty", "encoder_input_ids", "encoder_stride", "encoder_lengths", "encoder_rows", "encoder_len",
              "rows_per_encoder_row", "encoder_no_repeat_ngram_size", "bad_words_ids", "bad_words_offsets", "bad_words_offsets_host",
              "n_bad_words", "n_bad_word_ids", "min_new_tokens", "prompt_length", "prompt_lengths", "max_new_tokens", "forced_tokens",
              "forced_bos_token_id", "forced_eos_token_id"]


def test_struct_is_extended_at_its_end(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_logits_params() == ctypes.sizeof(_lib.LogitsParams)
    names = [f[0] for f in _lib.LogitsParams._fields_]
    assert names[-len(NEW_FIELDS):] == NEW_FIELDS and names[-len(NEW_FIELDS) - 1] == "suppress_tokens"
    assert _lib.LogitsParams.suppress_tokens.offset == 96   # (the old fields keep their offsets)
    for name in ("fat5_process_logits", "fat5_sizeof_logits_params"):
        assert name in _lib.EXPORTS
    import flasht5_amd
    assert flasht5_amd.pack_bad_words is flasht5_amd.logits_process.pack_bad_words


def _ext_params(**kw):
    """a valid descriptor with every new processor on (fake pointers; rows = 0: nothing is launched)"""
    from flasht5_amd import _lib
    off = (ctypes.c_int32 * 4)(0, 1, 3, 6)
    p = _params(rows=0)
    p.encoder_repetition_penalty, p.encoder_no_repeat_ngram_size = 1.4, 3
    p.encoder_input_ids, p.encoder_stride, p.encoder_rows, p.encoder_len, p.rows_per_encoder_row = BASE + 20480, 512, 4, 512, 1
    p.encoder_lengths = BASE + 24576
    p.bad_words_ids, p.bad_words_offsets, p.n_bad_words, p.n_bad_word_ids = BASE + 28672, BASE + 32768, 3, 6
    p.bad_words_offsets_host = ctypes.addressof(off)
    p.min_new_tokens, p.prompt_length, p.max_new_tokens = 4, 1, 32
    p.forced_tokens, p.forced_bos_token_id, p.forced_eos_token_id = _lib.FAT5_FORCED_BOS | _lib.FAT5_FORCED_EOS, 5, 1
    for key, val in kw.items():
        setattr(p, key, val)
    p._keep = off
    return p


def test_zero_new_fields_are_the_old_call(lib):
    """all-zero appended fields pass every check as the descriptor did before them (and an encoder pointer, lengths or counts
    left behind by a switched-off processor are not looked at)"""
    assert lib.fat5_process_logits(ctypes.byref(_params(rows=0)), None) == 0
    assert lib.fat5_process_logits(ctypes.byref(_ext_params()), None) == 0
    assert lib.fat5_process_logits(ctypes.byref(_params(rows=0, encoder_repetition_penalty=1.0, encoder_len=9999)), None) == 0


def _offsets(*v):
    return (ctypes.c_int32 * len(v))(*v)


BAD_OFFSETS = {"flat": _offsets(0, 3, 3, 6), "down": _offsets(0, 4, 2, 6), "start": _offsets(1, 2, 3, 6), "end": _offsets(0, 1, 3, 5)}


@pytest.mark.parametrize("bad, msg", [
    (dict(encoder_input_ids=None), "encoder_input_ids"), (dict(encoder_input_ids=BASE + 4), "encoder_input_ids"),
    (dict(encoder_repetition_penalty=1.0, encoder_input_ids=None), "encoder_input_ids"),   # (the n-gram processor alone)
    (dict(encoder_len=4097, encoder_stride=4097), "encoder_len"), (dict(encoder_len=0), "encoder_len"),
    (dict(encoder_stride=511), "encoder_stride"), (dict(encoder_lengths=BASE + 2), "encoder_lengths"),
    (dict(rows=9), "encoder_rows"), (dict(rows_per_encoder_row=0), "encoder_rows"),
    (dict(encoder_repetition_penalty=-1.0), "encoder_repetition_penalty"),
    (dict(encoder_repetition_penalty=float("inf")), "encoder_repetition_penalty"),
    (dict(encoder_repetition_penalty=float("nan")), "encoder_repetition_penalty"),
    (dict(encoder_no_repeat_ngram_size=-1), "encoder_no_repeat_ngram_size"),
    (dict(n_bad_words=-1), "n_bad_words"), (dict(n_bad_words=1025), "n_bad_words"), (dict(n_bad_word_ids=4097), "n_bad_word_ids"),
    (dict(n_bad_word_ids=2), "n_bad_word_ids"), (dict(bad_words_ids=None), "bad_words_ids"), (dict(bad_words_offsets=None), "bad_words_offsets"),
    (dict(bad_words_offsets=BASE + 2), "bad_words_offsets"),
    (dict(bad_words_offsets_host="flat"), "not increasing"), (dict(bad_words_offsets_host="down"), "not increasing"),
    (dict(bad_words_offsets_host="start"), "bad_words_offsets"), (dict(bad_words_offsets_host="end"), "bad_words_offsets"),
    (dict(min_new_tokens=-1), "min_new_tokens"), (dict(forced_tokens=4), "forced_tokens"),
    (dict(forced_bos_token_id=1000), "forced_bos_token_id"), (dict(forced_bos_token_id=-1), "forced_bos_token_id"),
    (dict(forced_eos_token_id=1000), "forced_eos_token_id"), (dict(forced_eos_token_id=-2), "forced_eos_token_id"),
    (dict(max_new_tokens=0), "max_new_tokens"), (dict(prompt_length=0), "prompt_length"), (dict(prompt_lengths=BASE + 2), "prompt_length"),
])
def test_new_fields_reject_before_launch(lib, bad, msg):
    if isinstance(bad.get("bad_words_offsets_host"), str):
        bad = dict(bad, bad_words_offsets_host=ctypes.addressof(BAD_OFFSETS[bad["bad_words_offsets_host"]]))
    p = _ext_params(**bad)
    assert lib.fat5_process_logits(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


# ------------------------------------------------------------------------------------------------ fakes and host checks
def test_fake_implementation_with_and_without_the_new_arguments():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import logits_process  # noqa: F401  (registers the op)
    with FakeTensorMode():
        logits = torch.empty(6, 100, dtype=torch.bfloat16)
        seqs = torch.empty(6, 9, dtype=torch.int64)
        lens = torch.empty(6, dtype=torch.int32)
        y = torch.ops.fat5.process_logits(logits, seqs, lens, 1.2, 3, 5, 1, None, False)   # (the old positional call)
        assert y.shape == (6, 100) and y.dtype == torch.float32
        y = torch.ops.fat5.process_logits(logits, seqs, lens, 1.0, 0, 0, 1, None, True, 1.4, 3, torch.empty(2, 40, dtype=torch.int64),
                                          torch.empty(2, dtype=torch.int32), 3, torch.empty(6, dtype=torch.int32),
                                          torch.empty(4, dtype=torch.int32), [0, 1, 3, 6], 4, 1, torch.empty(6, dtype=torch.int32), 32, 5, 1)
        assert y.shape == (6, 100) and y.dtype == torch.float32


@pytest.mark.parametrize("kw, msg", [
    (dict(encoder_repetition_penalty=0.0), "encoder_repetition_penalty"), (dict(encoder_repetition_penalty=-1.5), "encoder_repetition_penalty"),
    (dict(encoder_repetition_penalty=2), "encoder_repetition_penalty"), (dict(encoder_repetition_penalty=True), "encoder_repetition_penalty"),
    (dict(encoder_repetition_penalty=float("inf")), "encoder_repetition_penalty"),
    (dict(encoder_repetition_penalty=float("nan")), "encoder_repetition_penalty"),
    (dict(encoder_no_repeat_ngram_size=-1), "encoder_no_repeat_ngram_size"), (dict(encoder_no_repeat_ngram_size=2.0), "encoder_no_repeat_ngram_size"),
    (dict(encoder_no_repeat_ngram_size=True), "encoder_no_repeat_ngram_size"),
    (dict(bad_words_ids=[]), "bad_words_ids"), (dict(bad_words_ids=[[]]), "bad_words_ids"), (dict(bad_words_ids=[3]), "bad_words_ids"),
    (dict(bad_words_ids=((3,),)), "bad_words_ids"), (dict(bad_words_ids=[[3, 1.0]]), "bad_words_ids"),
    (dict(bad_words_ids=[[True]]), "bad_words_ids"), (dict(bad_words_ids=[[128]]), "bad_words_ids"), (dict(bad_words_ids=[[-1]]), "bad_words_ids"),
    (dict(bad_words_ids=[[5]] * 1025), "1024"), (dict(bad_words_ids=[[5] * 4097]), "4096"),
    (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=1.5), "min_new_tokens"),
    (dict(forced_bos_token_id=128), "forced_bos_token_id"), (dict(forced_bos_token_id=-1), "forced_bos_token_id"),
    (dict(forced_bos_token_id=2.0), "forced_bos_token_id"), (dict(forced_eos_token_id=128), "forced_eos_token_id"),
    (dict(forced_eos_token_id=True), "forced_eos_token_id"),
])
@pytest.mark.parametrize("beams", [dict(), dict(num_beams=4), dict(do_sample=True, seed=1)])
def test_host_checks_before_the_encoder(kw, msg, beams, monkeypatch):
    from flasht5_amd.logits_process import check_args
    with pytest.raises(ValueError, match=msg):
        check_args(vocab_size=128, **kw)
    m = _small_model()

    def boom(*a, **k):
        raise AssertionError("the encoder ran before the arguments were checked")
    monkeypatch.setattr(m.encoder, "forward", boom)
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=8, **beams, **kw)


def test_check_args_accepts_and_active():
    from flasht5_amd.logits_process import active, check_args
    check_args(1.2, 3, 30, [0, 127], 128, 1, 1.4, 3, [[5], [6, 7]], 4, 0, 127)
    check_args(vocab_size=128, bad_words_ids=[[5]] * 1024)
    assert not active() and not active(bad_words_ids=[[1]])   # ([eos] is dropped: nothing is left)
    for kw in (dict(encoder_repetition_penalty=1.4), dict(encoder_no_repeat_ngram_size=1), dict(bad_words_ids=[[1], [2]]),
               dict(min_new_tokens=1), dict(forced_bos_token_id=0), dict(forced_eos_token_id=1)):
        assert active(**kw), kw


class _Reached(Exception):
    pass


def test_generate_accepts_the_new_arguments_and_limits_the_encoder_ids(monkeypatch):
    """a TypeError without the feature; with it the valid arguments pass the host checks and the call goes on to the encoder"""
    from flasht5_amd.generation import generate
    m = _small_model()

    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(m.encoder, "forward", reached)
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(_Reached):
        generate(m, ids, encoder_no_repeat_ngram_size=3, forced_eos_token_id=1, min_new_tokens=4, bad_words_ids=[[5, 9]])
    with pytest.raises(_Reached):
        m.generate(ids, max_length=8, num_beams=4, encoder_repetition_penalty=1.4, forced_bos_token_id=7, bad_words_ids=[[1]])
    long = torch.zeros(1, 4097, dtype=torch.long)
    for kw in (dict(encoder_repetition_penalty=1.4), dict(encoder_no_repeat_ngram_size=2)):
        with pytest.raises(ValueError, match="4096"):
            m.generate(long, max_length=8, **kw)
    with pytest.raises(_Reached):   # (the other processors do not read the encoder ids)
        m.generate(long, max_length=8, min_new_tokens=2)


@pytest.mark.parametrize("kw", [dict(encoder_repetition_penalty=1.4), dict(encoder_no_repeat_ngram_size=2), dict(bad_words_ids=[[5, 6]]),
                                dict(min_new_tokens=2), dict(forced_bos_token_id=3), dict(forced_eos_token_id=1)])
@pytest.mark.parametrize("spec", ["assistant", "lookup"])
def test_speculative_decoding_rejects_the_new_processors(kw, spec, monkeypatch):
    m, a = _small_model(), _small_model()

    def boom(*a, **k):
        raise AssertionError("an encoder ran before the arguments were checked")
    monkeypatch.setattr(m.encoder, "forward", boom)
    monkeypatch.setattr(a.encoder, "forward", boom)
    skw = dict(assistant_model=a) if spec == "assistant" else dict(prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match="logits processors"):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=8, **skw, **kw)
