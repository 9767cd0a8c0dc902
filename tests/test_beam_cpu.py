"""CPU tests of beam search: the restatement (tests/beam_ref.py) against HF's own `generate(num_beams=...)` on a tiny randomly
initialised T5ForConditionalGeneration (nothing is downloaded), the C ABI of fat5_beam_step and of the extended
fat5_decode_params (struct sizes against the ctypes mirrors, rejections before any launch: fake, aligned pointers are enough),
the custom ops' fake implementations, and the argument checks of `generate`, done before the encoder runs."""
import ctypes
import itertools

import pytest
import torch

import beam_ref

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)


# ------------------------------------------------------------------------------------------------ the restatement against HF
def _hf_model(seed):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.T5Config(vocab_size=24, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4,
                                relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=0.0,
                                decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    torch.manual_seed(seed)
    m = transformers.T5ForConditionalGeneration(cfg).eval()
    with torch.no_grad():  # (sharper logits than the default init: fewer near-ties, hypotheses of several lengths)
        m.lm_head.weight.mul_(2.0)
    return m


def _hf_generate(m, ids, k, max_length, lp, es, R):
    from transformers import GenerationConfig
    gc = GenerationConfig(num_beams=k, max_new_tokens=max_length, length_penalty=lp, early_stopping=es, num_return_sequences=R,
                          do_sample=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, bos_token_id=None,
                          min_length=0, no_repeat_ngram_size=0, repetition_penalty=1.0, forced_eos_token_id=None,
                          forced_bos_token_id=None, return_dict_in_generate=True, output_scores=True,
                          output_logits=True)
    with torch.no_grad():
        out = m.generate(ids, generation_config=gc)
    seqs = out.sequences.clone()
    lens = (out.beam_indices >= 0).sum(1)  # (generated tokens per returned hypothesis: HF's own crop rule)
    for r in range(seqs.shape[0]):
        seqs[r, 1 + int(lens[r]):] = 0     # HF fills past a hypothesis's end with its EOS id; the restatement with 0
    return seqs, out.sequences_scores, out.logits


def _given_logits(logits):
    """HF's own per-step logits (the running beams in HF's order), fed back by step: the restatement must then reach HF's
    decisions and scores from HF's numbers"""
    return lambda prefix: logits[prefix.shape[1] - 1].float()


def _recompute_logits(m, ids, k):
    enc_ids = ids.repeat_interleave(k, 0)

    def next_logits(prefix):
        with torch.no_grad():
            return m(input_ids=enc_ids, decoder_input_ids=prefix).logits[:, -1].float()
    return next_logits


GRID = list(itertools.product([2, 4], [1.0, 0.0, 2.0, -0.5], [False, True, "never"]))


@pytest.mark.parametrize("k, lp, es", GRID)
def test_restatement_matches_hf(k, lp, es):
    compared = runs = 0
    for seed, R in itertools.product(range(5), sorted({1, k})):
        m = _hf_model(seed)
        g = torch.Generator().manual_seed(50 + seed)
        ids = torch.randint(2, 24, (2, 7), generator=g)
        max_length = 9
        runs += 1
        hs, hsc, hl = _hf_generate(m, ids, k, max_length, lp, es, R)
        rs, rsc, amb = beam_ref.beam_search(_given_logits(hl), 2, k, max_length, lp, es, R, tol=1e-4)
        if amb:
            continue  # (a decision within rounding of a tie: another evaluation order may take either side)
        assert torch.equal(hs, rs), (seed, R, hs, rs)
        assert torch.allclose(hsc, rsc, rtol=1e-5, atol=1e-5), (seed, R, hsc, rsc)
        # the same over the model's recompute path (no cache: logits within ~1e-6 of the cached ones, summed over the steps)
        rs2, rsc2, amb2 = beam_ref.beam_search(_recompute_logits(m, ids, k), 2, k, max_length, lp, es, R, tol=1e-4)
        if not amb2:
            assert torch.equal(hs, rs2), (seed, R, hs, rs2)
            assert torch.allclose(hsc, rsc2, rtol=1e-4, atol=1e-4), (seed, R, hsc, rsc2)
        compared += 1
    assert compared >= runs // 3, f"only {compared} of {runs} runs were clear of ties"


def test_restatement_stops_and_crops_like_hf():
    """runs that end before max_length (EOS made likely): the loop's stop rule and the crop to the longest returned hypothesis"""
    early = 0
    for seed in range(12):
        m = _hf_model(seed)
        with torch.no_grad():
            m.lm_head.weight[1].mul_(8.0)  # (EOS prominent for some inputs)
        ids = torch.randint(2, 24, (3, 5), generator=torch.Generator().manual_seed(seed))
        for es in (False, True):
            hs, hsc, hl = _hf_generate(m, ids, 3, 12, 1.0, es, 3)
            rs, rsc, amb = beam_ref.beam_search(_given_logits(hl), 3, 3, 12, 1.0, es, 3, tol=1e-4)
            if amb:
                continue
            assert torch.equal(hs, rs) and torch.allclose(hsc, rsc, rtol=1e-5, atol=1e-5), (seed, es)
            early += len(hl) < 12
    assert early >= 2, f"only {early} runs stopped before max_length"


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def test_struct_sizes_match_library(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_beam_params() == ctypes.sizeof(_lib.BeamParams)
    assert lib.fat5_sizeof_decode_params() == ctypes.sizeof(_lib.DecodeParams)
    for name in ("fat5_beam_step", "fat5_beam_step_workspace_bytes", "fat5_sizeof_beam_params"):
        assert name in _lib.EXPORTS
    names = [f[0] for f in _lib.DecodeParams._fields_]
    assert names[-3:] == ["cache_batch_idx", "cache_row_batch", "cache_B"]  # (appended: the existing fields keep their offsets)


def _beam_params(**kw):
    from flasht5_amd import _lib
    p = _lib.BeamParams()
    p.B, p.k, p.V, p.dtype = 2, 4, 1000, _lib.FAT5_BF16
    p.row_stride = 1000
    ptrs = ("logits", "running_scores", "running_seqs", "cache_row_batch", "finished_seqs", "finished_scores", "finished_flags",
            "finished_lens", "heuristic", "status", "tokens", "step")
    for i, f in enumerate(ptrs):
        setattr(p, f, BASE + 4096 * (i + 1))
    p.seq_len, p.capacity, p.max_length, p.early_stopping, p.length_penalty = 33, 33, 32, 0, 1.0
    p.workspace, p.workspace_bytes = BASE + 65536, 1 << 16
    for key, val in kw.items():
        setattr(p, key, val)
    return p


def test_beam_workspace_query(lib):
    p = _beam_params()
    assert lib.fat5_beam_step_workspace_bytes(ctypes.byref(p)) == 2 * 4 * 8 * 8  # [B * k][2k] scores + tokens
    assert lib.fat5_beam_step_workspace_bytes(ctypes.byref(_beam_params(k=17))) == 0


@pytest.mark.parametrize("bad, msg", [
    (dict(k=1), "num_beams 1"), (dict(k=17), "num_beams 17"), (dict(V=1), "V 1"), (dict(V=(1 << 20) + 1), "V"),
    (dict(B=0), "B 0"), (dict(dtype=5), "dtype"), (dict(row_stride=999), "row_stride"), (dict(seq_len=1), "seq_len"),
    (dict(capacity=0), "capacity"), (dict(capacity=1 << 28), "int32"), (dict(max_length=0), "max_length"),
    (dict(length_penalty=float("inf")), "length_penalty"), (dict(length_penalty=float("nan")), "length_penalty"),
    (dict(early_stopping=3), "early_stopping"), (dict(logits=None), "logits"), (dict(logits=BASE + 1), "logits"),
    (dict(running_seqs=BASE + 4), "running_seqs"), (dict(tokens=None), "tokens"), (dict(step=BASE + 2), "step"),
    (dict(finished_lens=BASE + 2), "finished_lens"), (dict(cache_row_batch=None), "cache_row_batch"),
])
def test_beam_rejects_before_launch(lib, bad, msg):
    p = _beam_params(**bad)
    assert lib.fat5_beam_step(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


def test_beam_workspace_checked(lib):
    for ws, n in ((None, 1 << 16), (BASE + 65536, 16), (BASE + 65536 + 8, 1 << 16)):
        assert lib.fat5_beam_step(ctypes.byref(_beam_params(workspace=ws, workspace_bytes=n)), None) == -3


def _decode_params(**kw):
    from flasht5_amd import _lib
    p = _lib.DecodeParams()
    B, H, D, cap = 4, 4, 64, 256
    p.B, p.H, p.D, p.dtype, p.capacity, p.N = B, H, D, _lib.FAT5_BF16, cap, 0
    p.cache_seqlens = BASE
    p.sm_scale = 0.125
    for i, f in enumerate(("q", "k_cache", "v_cache", "k_new", "v_new", "o", "lse")):
        setattr(p, f, BASE + 4096 * (i + 1))
    for f in ("q_stride", "o_stride", "k_new_stride", "v_new_stride"):
        getattr(p, f)[:] = (H * D, D)
    p.k_cache_stride[:] = (cap * H * D, H * D, D)
    p.v_cache_stride[:] = (cap * H * D, H * D, D)
    p.num_splits = 1
    for key, val in kw.items():
        setattr(p, key, val)
    return p


@pytest.mark.parametrize("bad, msg", [
    (dict(cache_batch_idx=BASE, cache_row_batch=BASE, k_new=None, v_new=None), "cannot be combined"),
    (dict(cache_batch_idx=BASE), "with an append"),
    (dict(cache_row_batch=BASE + 2), "misaligned"), (dict(cache_batch_idx=BASE + 1, k_new=None, v_new=None), "misaligned"),
    (dict(cache_B=-1), "cache_B -1"), (dict(cache_B=3), "cache_B 3 < B 4"),
    (dict(cache_row_batch=BASE, cache_B=2), "cache_B 2 < B 4"),
])
def test_decode_map_rejections(lib, bad, msg):
    p = _decode_params(**bad)
    assert lib.fat5_attn_decode(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


# ------------------------------------------------------------------------------------------------ fakes and host checks
def test_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import beam, decode  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        B, k, H, D, cap, L = 2, 4, 6, 64, 40, 41
        q = torch.empty(B * k, 1, H, D, dtype=torch.bfloat16)
        cross = torch.empty(B, 33, H, D, dtype=torch.bfloat16)
        idx = torch.empty(B * k, dtype=torch.int32)
        o, lse = torch.ops.fat5.attn_decode(q, cross, cross, None, None, None, 0.125, None, 0, True, 0, idx, None)
        assert o.shape == (B * k, 1, H, D) and lse.shape == (B * k, H, 1)
        kc = torch.empty(B * k, cap, H, D, dtype=torch.bfloat16)
        table = torch.empty(B * k, cap, dtype=torch.int32)
        lens = torch.empty(B * k, dtype=torch.int32)
        o, _ = torch.ops.fat5.attn_decode(q, kc, kc, q, q, lens, 0.125, None, 0, False, 0, None, table)
        assert o.shape == (B * k, 1, H, D)
        o, _ = torch.ops.fat5.attn_decode(q, kc, kc, q, q, lens, 0.125, None, 0, False, 0)  # (the 11 positional arguments)
        st = beam.new_state(B, k, L, cap, "cpu")
        logits = torch.empty(B * k, 100, dtype=torch.float32)
        r = torch.ops.fat5.beam_step(logits, st.running_scores, st.running_seqs, st.cache_row_batch, st.finished_seqs,
                                     st.finished_scores, st.finished_flags, st.finished_lens, st.heuristic, st.status, st.tokens,
                                     lens, k, 32, 1.0, 0)
        assert r is None


def test_beam_state_initial_values():
    from flasht5_amd.beam import new_state
    st = new_state(3, 4, 9, 9, "cpu")
    ref = beam_ref.init(3, 4, 9, 9)
    for name in ("running_scores", "running_seqs", "cache_row_batch", "finished_seqs", "finished_scores", "finished_flags",
                 "finished_lens", "heuristic"):
        assert torch.equal(getattr(st, name), ref[name]), name


def _small_model():
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    c = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe")
    return FAT5ForConditionalGeneration(c)


@pytest.mark.parametrize("kw, msg", [
    (dict(num_beams=4, do_sample=True), "beam sampling"), (dict(num_beams=2, num_return_sequences=3), "num_return_sequences 3"),
    (dict(num_return_sequences=2), "num_return_sequences 2"), (dict(num_beams=17), "num_beams"), (dict(num_beams=0), "num_beams"),
    (dict(num_beams=True), "num_beams"), (dict(num_beams=2.0), "num_beams"), (dict(num_beams=4, num_return_sequences=0), ">= 1"),
    (dict(num_beams=4, early_stopping="always"), "early_stopping"), (dict(num_beams=4, early_stopping=1), "early_stopping"),
    (dict(num_beams=4, length_penalty=float("nan")), "length_penalty"),
])
def test_generate_rejects_before_the_encoder(kw, msg, monkeypatch):
    m = _small_model()

    def boom(*a, **k):
        raise AssertionError("the encoder ran before the arguments were checked")
    monkeypatch.setattr(m.encoder, "forward", boom)
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=8, **kw)


def test_keep_going_matches_hf_rule():
    from flasht5_amd.beam import keep_going
    for bits in itertools.product(range(8), repeat=2):
        st = torch.tensor(bits, dtype=torch.int32)
        for es in (False, True, "never"):
            assert bool(keep_going(st, es)) == beam_ref.keep_going(dict(status=st), es), (bits, es)
