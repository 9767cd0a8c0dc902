"""GPU tests of the UL2 collator (fat5_ul2_collate, csrc/ul2_kernels.h), exact integer equality throughout: given-mask
mode against the reference collator's recorded runs (tests/golden/ul2_collator.npz), drawn mode against the host restatement of
the contract (tests/ul2_ref.py) over every denoiser, the lengths at which the kernel changes its loop counts and the 4096-token
limit, each clamp of the span count, each status bit provoked alone, a captured call replayed twice, and the model's loss on a
collated batch."""
import os

import numpy as np
import pytest
import torch

import ul2_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("input_ids", "labels", "attention_mask", "decoder_attention_mask", "enc_len", "dec_len", "denoiser", "status")

# the reference's training set, one denoiser with few spans, one whose span count is bounded by its non-noise tokens
DENOISERS = [
    dict(mu=3.0, r=0.15, max_spans=4096, prefix_ids=[31990, 31991]),
    dict(mu=8.0, r=0.15, max_spans=4096, prefix_ids=[31990, 31991]),
    dict(mu=4.0, r=0.0, max_spans=1, prefix_ids=[31992]),
    dict(mu=3.0, r=0.5, max_spans=4096, prefix_ids=[31993, 31994, 31995]),
    dict(mu=64.0, r=0.15, max_spans=4096, prefix_ids=[31993, 31994, 31995]),
    dict(mu=64.0, r=0.5, max_spans=4096, prefix_ids=[31993, 31994, 31995]),   # tokens_len 4096 at max_length 2084
    dict(mu=3.0, r=0.15, max_spans=7, prefix_ids=[]),
    dict(mu=1.0, r=0.9, max_spans=4096, prefix_ids=[31990]),
]
VOCAB = dict(sentinel_first_id=32099, num_sentinels=100, eos_token_id=1, pad_token_id=0)
BIG = dict(max_length=2084, max_labels_length=2084, **VOCAB)
SEED = 15   # (with it the drawn batch below meets every denoiser: asserted there)


def host_tables(denoisers, proportions, args):
    from flasht5_amd.ul2 import _host_tables
    return _host_tables(denoisers, proportions, args["max_length"], args["max_labels_length"], args["sentinel_first_id"], args["num_sentinels"])


def on_host(out):
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in KEYS}


def assert_equal(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = np.argwhere(np.asarray(got[k] != want[k]))
        assert bad.size == 0, (what, k, bad[:5].tolist())


def raw_tokens(B, L, seed, eos_every=37):
    """(B, L) int64 raw tokens in [2, 31000) with an eos at every 37th column of every third row"""
    t = np.random.default_rng(seed).integers(2, 31000, size=(B, L)).astype(np.int64)
    t[::3, ::eos_every] = 1
    return t


def strided(t_np, extra=56):
    """the rows of t_np as a strided view of a wider device buffer"""
    B, L = t_np.shape
    buf = torch.full((B, L + extra), -5, dtype=torch.int64, device="cuda")
    buf[:, :L] = torch.from_numpy(t_np).cuda()
    return buf[:, :L]


def test_given_masks_reproduce_the_reference():
    """the reference's own masks replayed: input_ids and labels of every recorded case bit for bit, in one call"""
    from flasht5_amd import UL2Collator
    fx = np.load(os.path.join(ROOT, "tests", "golden", "ul2_collator.npz"))
    first, count, eos, pad = (int(x) for x in fx["vocab"])
    ml, mll = (int(x) for x in fx["settings"][0])
    off = fx["prefix_off"]
    dens = [dict(mu=float(fx["den_mu"][d]), r=float(fx["den_r"][d]), max_spans=int(fx["den_max_spans"][d]),
                 prefix_ids=[int(x) for x in fx["prefix_ids"][off[d]:off[d + 1]]]) for d in range(len(off) - 1)]
    c = UL2Collator(dens, [1.0] * len(dens), max_length=ml, max_labels_length=mll, sentinel_first_id=first, num_sentinels=count,
                    eos_token_id=eos, pad_token_id=pad, seed=0)
    assert c.tokens_len == [int(x) for x in fx["optimal_len"][0, :, 0]]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()   # noqa: E731
    out = c(dev(fx["tokens"], torch.int64), dev(fx["lengths"], torch.int32), noise_mask=dev(fx["mask"], torch.uint8),
            denoiser=dev(fx["denoiser"], torch.int32))
    got = on_host(out)
    assert np.array_equal(got["input_ids"], fx["ref_input_ids"].astype(np.int64))
    assert np.array_equal(got["labels"], fx["ref_labels"].astype(np.int64))
    assert np.array_equal(got["attention_mask"], fx["ref_input_ids"] != pad)
    assert np.array_equal(got["decoder_attention_mask"], fx["ref_labels"] != -100)
    assert np.array_equal(got["denoiser"], fx["denoiser"])
    assert got["status"][0] == 0 and got["status"][1] == 0
    c.check(out)
    # the lengths the reference raises on (its optimum for mu = 64, r = 0.15 is a column too long): cut, bit 1
    for row in range(len(fx["raised_lengths"])):
        d = int(fx["raised_denoiser"][row])
        one = UL2Collator(dens, [float(i == d) for i in range(len(dens))], max_length=ml, max_labels_length=mll, sentinel_first_id=first,
                          num_sentinels=count, eos_token_id=eos, pad_token_id=pad, seed=3)
        got = on_host(one(dev(fx["raised_tokens"][row:row + 1], torch.int64), dev(fx["raised_lengths"][row:row + 1], torch.int32)))
        assert got["denoiser"][0] == d and got["status"].tolist() == [1, 1, ml, got["dec_len"][0]]
        assert got["input_ids"][0, -1] == eos and got["attention_mask"][0].all()


# n_b of the drawn batch: the smallest rows, both sides of the 64-lane and 256-thread counts, 1024, the 4096-token limit (rows
# above every tokens_len: the chunk start is drawn) and rows below it
DRAWN_LENGTHS = [2, 3, 11, 64, 65, 256, 257, 1024, 4096, 6000, 5000, 2, 700, 1500, 33, 100, 3000, 12, 4097, 2500]


def test_drawn_batch_equals_the_restatement():
    from flasht5_amd import UL2Collator
    L = 6000
    tok = raw_tokens(len(DRAWN_LENGTHS), L, 1)
    lengths = np.array(DRAWN_LENGTHS, dtype=np.int32)
    props = [1.0] * len(DENOISERS)
    c = UL2Collator(DENOISERS, props, seed=SEED, **BIG)
    assert max(c.tokens_len) == 4096
    tab = host_tables(DENOISERS, props, BIG)
    tokens = strided(tok)
    assert tokens.stride(0) != L
    for step in (0, 1):
        got = on_host(c(tokens, torch.from_numpy(lengths).cuda()))
        want = ul2_ref.collate(tok, lengths, tab, seed=SEED, step=step, **BIG)
        assert_equal(got, want, f"step {step}")
        if step == 0:   # what this batch is meant to exercise (a changed draw must not lose it silently)
            assert set(want["denoiser"].tolist()) == set(range(len(DENOISERS)))
            n = np.minimum(lengths, np.array(tab["tokens_len"])[want["denoiser"]])
            assert (n == 4096).any() and (lengths > n).sum() >= 4 and (lengths == n).sum() >= 4
            assert want["status"][0] & 8 == 0
    assert int(c.step.item()) == 2


# (denoiser, n, the term of spans = max(1, min(max_spans, num_sentinels, rint(noise / mu), noise, n - noise)) that decides)
CLAMPS = [
    (6, 300, "max_spans"),        # 45 noise tokens, rint(45 / 3) = 15 > 7
    (0, 2311, "num_sentinels"),   # 347 noise tokens, rint(347 / 3) = 116 > 100
    (0, 257, "rint"),             # 39 noise tokens in 13 spans
    (7, 10, "n - noise"),         # 9 noise tokens, 1 non-noise token
    (4, 11, "one"),               # 2 noise tokens, rint(2 / 64) = 0
    (0, 2, "noise >= 1"),         # rint(0.3) = 0 noise tokens -> 1
    (7, 3, "noise <= n - 1"),     # rint(2.7) = 3 noise tokens -> 2
    (2, 2, "S head 0"),           # the S-denoiser with rint(2 / 4) = 0 leading tokens: every token is noise
    (2, 2601, "S"),
]


@pytest.mark.parametrize("d, n, which", CLAMPS)
def test_span_count_clamps(d, n, which):
    from flasht5_amd import UL2Collator
    dn = DENOISERS[d]
    if dn["max_spans"] > 1:
        noise, spans = ul2_ref.span_counts(n, dn["mu"], dn["r"], dn["max_spans"], 100)
        free = int(round(min(max(int(round(n * dn["r"])), 1), n - 1) / dn["mu"]))
        want_spans = {"max_spans": dn["max_spans"], "num_sentinels": 100, "rint": free, "n - noise": n - noise, "one": 1}.get(which)
        if want_spans is not None:
            assert spans == want_spans and (which == "rint" or free != spans), (noise, spans, free)
        if which == "noise >= 1":
            assert int(round(n * dn["r"])) == 0 and noise == 1
        if which == "noise <= n - 1":
            assert int(round(n * dn["r"])) == n and noise == n - 1
    props = [float(i == d) for i in range(len(DENOISERS))]
    c = UL2Collator(DENOISERS, props, seed=SEED + 1, **BIG)
    tok = raw_tokens(2, n + 5, 2)
    lengths = np.array([n, n], dtype=np.int32)
    got = on_host(c(strided(tok), torch.from_numpy(lengths).cuda()))
    want = ul2_ref.collate(tok, lengths, host_tables(DENOISERS, props, BIG), seed=SEED + 1, step=0, **BIG)
    assert_equal(got, want, which)
    assert (want["denoiser"] == d).all() and want["status"][0] == 0
    if which == "S head 0":
        assert want["input_ids"][0, :3].tolist() == [31992, 32099, 1]


SMALL = dict(max_length=16, max_labels_length=16, **VOCAB)


def _mask(n, noise_at):
    m = np.zeros((1, n), dtype=np.uint8)
    m[0, noise_at] = 1
    return m


STATUS_CASES = [
    # (bit, n_b, the raw token to plant at column 3 (None: none), the noise positions of the given mask)
    (1, 30, None, [5]),                      # 29 kept tokens: the encoder side does not fit into 16 columns
    (2, 30, None, list(range(1, 30))),       # 29 noise tokens: the decoder side does not fit
    (4, 8, 0, [2, 3]),                       # a raw pad token
    (4, 8, 32000, [5]),                      # a raw token at the low end of the sentinel range
    (8, 1, None, []),
    (8, 0, None, []),
    (0, 8, 31999, [2, 3]),                   # (just below the sentinel range: nothing to report)
]


@pytest.mark.parametrize("bit, n, plant, noise_at", STATUS_CASES)
def test_each_status_bit_alone(bit, n, plant, noise_at):
    from flasht5_amd import UL2Collator
    dens, props = DENOISERS[:1], [1.0]
    c = UL2Collator(dens, props, seed=0, **SMALL)
    tok = raw_tokens(1, 32, 3, eos_every=1000)
    if plant is not None:
        tok[0, 3] = plant
    lengths = np.array([n], dtype=np.int32)
    mask = _mask(32, noise_at)
    den = np.zeros(1, dtype=np.int32)
    out = c(strided(tok), torch.from_numpy(lengths).cuda(), noise_mask=torch.from_numpy(mask).cuda(), denoiser=torch.from_numpy(den).cuda())
    got = on_host(out)
    want = ul2_ref.collate(tok, lengths, host_tables(dens, props, SMALL), seed=0, step=0, noise_mask=mask, denoiser=den, **SMALL)
    assert_equal(got, want, f"bit {bit}")
    assert got["status"][0] == bit and got["status"][1] == (bit != 0)
    if bit == 0:
        c.check(out)
    else:
        with pytest.raises(RuntimeError, match={1: "encoder side", 2: "decoder side", 4: "raw token", 8: "fewer than 2"}[bit]):
            c.check(out)
    if bit == 1:
        assert got["enc_len"][0] == 16 and got["input_ids"][0, 15] == 1
    if bit == 2:
        assert got["dec_len"][0] == 16 and got["labels"][0, 15] == 1
    if bit == 8:
        assert got["input_ids"][0, :4].tolist() == [31990, 31991, 1, 0] and got["labels"][0, :2].tolist() == [1, -100]
    assert int(c.step.item()) == 1   # (given-mask mode draws nothing, the counter still counts calls)


def test_nothing_is_written_outside_the_outputs():
    """the C ABI on caller-owned buffers that carry a guard tail of sentinels: rows that are cut on both sides, rows with
    lengths the contract clamps (negative, beyond L) and a denoiser index out of range leave every guard element untouched,
    write every element in front of it, and equal the restatement on the clamped inputs"""
    import ctypes
    from flasht5_amd import _lib
    from flasht5_amd.ul2 import ul2_tables
    GUARD, SENT = 64, 0x5A
    dens, props = DENOISERS[:4], [1.0] * 4
    B, L, ML, MD = 6, 600, 16, 24
    args = dict(max_length=ML, max_labels_length=MD, **VOCAB)
    tab_dev = ul2_tables(dens, props, max_length=ML, max_labels_length=MD, sentinel_first_id=32099, num_sentinels=100, device="cuda")
    tok = raw_tokens(B, L, 6)
    lengths = np.array([600, -4, 9999, 300, 1, 64], dtype=np.int32)
    mask = (np.random.default_rng(8).random((B, L)) < 0.4).astype(np.uint8)
    den = np.array([0, 1, 2, 77, -3, 3], dtype=np.int32)
    shapes = dict(input_ids=(B * ML, torch.int64), labels=(B * MD, torch.int64), attention_mask=(B * ML, torch.uint8),
                  decoder_attention_mask=(B * MD, torch.uint8), enc_len=(B, torch.int32), dec_len=(B, torch.int32),
                  denoiser=(B, torch.int32), status=(4, torch.int32))
    step = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    tokens = strided(tok)
    for given in (True, False):
        bufs = {k: torch.full((n + GUARD,), SENT, dtype=dt, device="cuda") for k, (n, dt) in shapes.items()}
        p = _lib.Ul2Params()
        p.B, p.L, p.max_length, p.max_labels_length, p.num_denoisers, p.num_sentinels, p.random_chunk = B, L, ML, MD, 4, 100, 1
        p.sentinel_first_id, p.eos_token_id, p.pad_token_id, p.seed = 32099, 1, 0, 99
        p.tokens, p.tokens_stride, p.step = tokens.data_ptr(), tokens.stride(0), step.data_ptr()
        n_dev = torch.from_numpy(lengths).cuda()
        p.lengths = n_dev.data_ptr()
        for k in ("mu", "r", "max_spans", "tokens_len", "prefix_off", "prefix_ids", "cum_prop"):
            setattr(p, k, getattr(tab_dev, k).data_ptr())
        if given:
            m_dev, d_dev = torch.from_numpy(mask).cuda(), torch.from_numpy(den).cuda()
            p.noise_mask, p.noise_mask_stride, p.denoiser_in = m_dev.data_ptr(), L, d_dev.data_ptr()
        for k, t in bufs.items():
            setattr(p, k, t.data_ptr())
        _lib.check(_lib.load().fat5_ul2_collate(ctypes.byref(p), _lib.stream_ptr(tokens.device)), "fat5_ul2_collate")
        torch.cuda.synchronize()
        want = ul2_ref.collate(tok, lengths, host_tables(dens, props, args), seed=99, step=5, noise_mask=mask if given else None,
                               denoiser=den if given else None, **args)
        for k, (n, _) in shapes.items():
            h = bufs[k].cpu().numpy()
            assert (h[n:] == SENT).all(), (given, k)
            assert np.array_equal(h[:n], want[k].reshape(-1).astype(h.dtype)), (given, k)
        assert want["status"][0] & 8 and (not given or want["status"][0] & 3 == 3)   # (drawn rows are cut to tokens_len first)


def test_captured_call_draws_anew_at_every_replay():
    from flasht5_amd import UL2Collator
    args = dict(max_length=160, max_labels_length=160, **VOCAB)
    props = [1.0, 1.0, 2.0, 0.5, 0.5, 0.5, 0.5, 0.0]
    c = UL2Collator(DENOISERS, props, seed=SEED + 2, **args)
    B, L = 8, 400
    tok = raw_tokens(B, L, 4)
    lengths = np.array([400, 150, 11, 64, 200, 90, 399, 30], dtype=np.int32)
    tokens, n_dev = strided(tok), torch.from_numpy(lengths).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c(tokens, n_dev)     # (uploads the tables, warms the allocator)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s = int(c.step.item())
    assert s == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = c(tokens, n_dev)
    tab = host_tables(DENOISERS, props, args)
    seen = []
    for k in range(2):
        g.replay()
        seen.append(on_host(out))
        assert_equal(seen[-1], ul2_ref.collate(tok, lengths, tab, seed=SEED + 2, step=s + k, **args), f"replay {k}")
    assert int(c.step.item()) == s + 2
    assert not np.array_equal(seen[0]["input_ids"], seen[1]["input_ids"]) and not np.array_equal(seen[0]["labels"], seen[1]["labels"])
    assert 7 not in seen[0]["denoiser"] and 7 not in seen[1]["denoiser"]   # (proportion 0)


def test_model_loss_on_a_collated_batch():
    """a two-layer FAT5 on the collator's batch: finite, and the bits of the loss on the host-restated batch"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, UL2Collator
    args = dict(max_length=64, max_labels_length=64, sentinel_first_id=127, num_sentinels=20, eos_token_id=1, pad_token_id=0)
    dens = [dict(mu=3.0, r=0.15, max_spans=20, prefix_ids=[100, 101]), dict(mu=4.0, r=0.0, max_spans=1, prefix_ids=[102]),
            dict(mu=3.0, r=0.5, max_spans=20, prefix_ids=[103])]
    props = [1.0, 1.0, 1.0]
    c = UL2Collator(dens, props, seed=SEED + 3, **args)
    B, L = 6, 120
    tok = np.random.default_rng(5).integers(2, 100, size=(B, L)).astype(np.int64)
    lengths = np.array([120, 40, 11, 64, 100, 25], dtype=np.int32)
    out = c(strided(tok), torch.from_numpy(lengths).cuda())
    want = ul2_ref.collate(tok, lengths, host_tables(dens, props, args), seed=SEED + 3, step=0, **args)
    assert_equal(on_host(out), want)
    c.check(out)
    cfg = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=2, num_decoder_layers=2,
                     relative_attention_max_distance=64, max_sequence_length=64)
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(cfg).cuda().bfloat16()
    with torch.no_grad():
        loss = model(out["input_ids"], out["labels"], attention_mask=out["attention_mask"],
                     decoder_attention_mask=out["decoder_attention_mask"])
        up = {k: torch.from_numpy(want[k]).cuda() for k in ("input_ids", "labels", "attention_mask", "decoder_attention_mask")}
        loss_host = model(up["input_ids"], up["labels"], attention_mask=up["attention_mask"],
                          decoder_attention_mask=up["decoder_attention_mask"])
    assert torch.isfinite(loss).item()
    assert torch.equal(loss, loss_host), (loss.item(), loss_host.item())
