"""GPU tests of generation's vocabulary-row kernels at their tile and load seams (tests/vocab_seams.py): `sample_logits`,
`speculative_accept` with sampling, `beam_step` (raw and logits_normalized), `process_logits` (the plain and the EXT instance)
and greedy `speculative_accept`, each at vocabulary sizes equal to and one either side of a chunk (8), a wave's span (512), a tile
(4096; 2048 for the argmax), a slice (8192) or the register limit (32768), on three load paths -- (a) aligned with a row stride
that is a multiple of 8, (b) an odd row stride, (c) a view one element into a buffer --, with every decision on a planted index
J(V) and NaN in the padding behind V (a read past V shows in the result).  Every kernel also gets one call at V = 2^20 and one at
2^20 + 1 that must be refused before any launch.

Each result is compared with its restatement exactly as the kernel's own test compares it (test_sampling_gpu.py,
test_spec_sample_gpu.py, test_beam_gpu.py, test_logits_proc_gpu.py, test_speculative_gpu.py).  tests/test_vocab_seams_cpu.py proves
that no case here is ambiguous, so there is no skip branch: every row of every call is held to the restatement.  The
`[vocab-seams] ...` lines name what each kernel met."""
import ctypes
import math

import pytest
import torch

import spec_ref as G
import spec_sample_ref as R
import vocab_seams as vs
from sampling_ref import draw

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = math.nan
NINF = float("-inf")
GUARD = 3
STATE = ("running_scores", "running_seqs", "cache_row_batch", "finished_seqs", "finished_scores", "finished_flags", "finished_lens",
         "heuristic", "status")
SEEN = {f: set() for f in vs.FAMILIES}   # family -> (path, seam class, dtype) met by a launch of this session
RAN = {f: set() for f in vs.FAMILIES}    # family -> (V, path) that passed


def _note(f, V, path, dtype):
    RAN[f].add((V, path))
    for name, at in vs.seam_classes(f).items():
        if V in at:
            SEEN[f].add((path, name, dtype))


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _placed(x, path):
    """x on the device on load path `path`, NaN behind every row; the kernel's `vec` condition holds on path (a) alone"""
    view, buf = vs.place(x, path, NAN, DEV)
    strides_ok = all(s % 8 == 0 for s in view.stride()[:-1])
    assert (view.data_ptr() % 16 == 0 and strides_ok) == vs.vec_expected(path) and view.stride(-1) == 1
    return view, buf


def _params(f, extra=()):
    return [pytest.param(V, p, id=f"V{V}-{p}") for V in list(vs.sizes(f)) + list(extra) for p in vs.PATHS]


# ------------------------------------------------------------------------------------------------------------------ sample_logits
def _run_sample_call(c, path, one_row=False):
    from flasht5_amd import sample_logits
    e = vs.sample_expected(c)
    V, B = c["x"].shape[0], len(c["us"])
    view, buf = _placed(c["x"].expand(1 if one_row else B, V), path)
    u = torch.tensor(c["us"], dtype=torch.float32, device=DEV)
    if one_row:   # (B = 1: one call per uniform over the same row)
        outs = [sample_logits(view, c["T"], c["top_k"], c["top_p"], uniforms=u[b:b + 1], return_aux=True) for b in range(B)]
        tok, aux = torch.cat([o[0] for o in outs]).cpu(), torch.cat([o[1] for o in outs]).cpu()
    else:
        tok, aux = (t.cpu() for t in sample_logits(view, c["T"], c["top_k"], c["top_p"], uniforms=u, return_aux=True))
    what = (V, path, c["kind"])
    assert vs.padding_untouched(view, buf, NAN), what
    for b in range(B):
        assert aux[b, 2].item() == c["us"][b], what
        assert tok[b].item() == e["tokens"][b], what + (b, tok[b].item(), e["tokens"][b])
        if e["degenerate"]:
            continue
        assert tok[b].item() in draw(e["r"], c["us"][b], 0.0 if c["exact"] else vs.TOL), what + (b,)
        assert aux[b, 0].item() == e["tau"], what + (b, aux[b].tolist(), e["tau"])
        assert aux[b, 3].item() == e["kept"], what + (b, aux[b].tolist(), e["kept"])
        assert abs(aux[b, 1].item() - e["ratio"]) <= 1e-5, what + (b, aux[b].tolist(), e["ratio"])
    return B


@pytest.mark.parametrize("V, path", _params("sample"))
def test_sample_logits(V, path):
    dtype = vs.dtype_for("sample", V, path)
    rows = sum(_run_sample_call(c, path) for c in vs.sample_calls(V, dtype))
    _note("sample", V, path, dtype)
    print(f"[vocab-seams] sample_logits V={V} path ({path}) {str(dtype)[6:]}: {rows} rows, all held to the restatement")


def test_sample_logits_at_the_largest_vocabulary():
    from flasht5_amd import _lib, sample_logits
    calls = vs.sample_calls(vs.MAX_V, torch.float32, kinds=vs.SAMPLE_BIG_KINDS)
    assert len(calls) == len(vs.SAMPLE_BIG_KINDS)
    for c in calls:
        _run_sample_call(c, "a", one_row=True)
    V = vs.MAX_V + 1
    x = torch.zeros(2, V, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="outside"):
        sample_logits(x, 1.0, 0, 1.0)
    tok = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    p = _lib.SampleParams()
    p.B, p.V, p.dtype, p.logits, p.row_stride, p.temperature, p.top_p, p.tokens = 2, V, _lib.FAT5_BF16, x.data_ptr(), V, 1.0, 1.0, tok.data_ptr()
    assert _lib.load().fat5_sample_logits(ctypes.byref(p), _lib.stream_ptr(x.device)) != 0
    torch.cuda.synchronize()
    assert tok.tolist() == [-7, -7]


# ------------------------------------------------------------------------------------------------------------------ sampled verification
def _spec_tensors(ln, path):
    lab_buf = torch.full((ln["labels"].shape[0], ln["labels"].shape[1] + 2 * GUARD), -7, dtype=torch.long, device=DEV)
    labels = lab_buf[:, GUARD:-GUARD]
    labels.copy_(ln["labels"])
    logits, lbuf = _placed(ln["logits"], path)
    t = dict(logits=logits, draft=ln["draft"].to(DEV), cache_seqlens=ln["cache_seqlens"].to(DEV), labels=labels, tok=ln["tok"].to(DEV),
             seen_eos=ln["seen_eos"].to(DEV), limit=ln["limit"], draft_seqlens=ln["draft_seqlens"].to(DEV))
    return t, lab_buf, (logits, lbuf)


def _run_spec_sample(ln, path, sampling, with_q, hook):
    from flasht5_amd import speculative_accept
    t, lab_buf, lg = _spec_tensors(ln, path)
    q = _placed(ln["draft_logits"], path) if with_q else None
    na, nn, sampled, aux = speculative_accept(
        t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"], draft_seqlens=t["draft_seqlens"],
        eos_token_id=R.EOS, sampling=sampling, draft_logits=None if q is None else q[0], uniforms=ln["uniforms"].to(DEV) if hook else None,
        return_sampled=True, return_aux=True)
    torch.cuda.synchronize()
    got = {k: t[k].cpu() for k in ("labels", "tok", "cache_seqlens", "draft_seqlens", "seen_eos")}
    got.update(n_accepted=na.cpu(), n_new=nn.cpu(), sampled=sampled.cpu(), aux=aux.cpu(), draft=t["draft"].cpu())
    guards = lab_buf.cpu()
    assert bool((guards[:, :GUARD] == -7).all()) and bool((guards[:, -GUARD:] == -7).all()), "guard columns"
    assert vs.padding_untouched(*lg, NAN) and (q is None or vs.padding_untouched(*q, NAN))
    return got


def _check_spec_sample(V, path, dtype, gamma, warpers, philox=True):
    import test_spec_sample_gpu as T   # (its per-row comparison and its bookkeeping check, as they stand)
    M = gamma + 1
    ln = vs.spec_sample_case(V, dtype, gamma)
    B = ln["logits"].shape[0]
    tally = T._Tally()
    for Tm, k, p in warpers:
        sampling = (Tm, k, p, R.SEED + k, R.OFFSET)
        cache = {}

        def dist_of(name, b, i, cache=cache, Tm=Tm, k=k, p=p):
            if (name, b, i) not in cache:
                cache[name, b, i] = R.dist(ln[name][b, i], Tm, k, p)
            return cache[name, b, i]
        for with_q, hook in ((True, True), (False, True)) + (((True, False),) if philox else ()):
            got = _run_spec_sample(ln, path, sampling, with_q, hook)
            for b in range(B):
                want_u = ln["uniforms"][b].tolist() if hook else R.round_uniforms(sampling[3], R.OFFSET, vs.SPEC_OLDS[b], b, M)
                assert got["aux"][b].tolist() == [list(w) for w in want_u], (b, hook)
                T._check_row(tally, lambda i, b=b: dist_of("logits", b, i), (lambda i, b=b: dist_of("draft_logits", b, i)) if with_q else None,
                             ln["draft"][b].tolist(), got["aux"][b].tolist(), got["sampled"][b], V)
            T._bookkeeping_is_exact(ln, got, V)
            if hook and V > 1:   # the planted row: the first draft rejected, the residual draw on the planted index
                assert got["sampled"][3].tolist() == [ln["star"]] + [-1] * gamma, (with_q, got["sampled"][3].tolist(), ln["star"])
    assert tally.ambiguous * 4 <= tally.rows, (tally.ambiguous, tally.rows)
    return tally


@pytest.mark.parametrize("V, path", _params("spec_sample"))
def test_sampled_verification(V, path):
    dtype = vs.dtype_for("spec_sample", V, path)
    gamma = (4, 1)[(vs.sizes("spec_sample").index(V) + vs.PATHS.index(path)) % 2]   # (every size meets both over its paths)
    tally = _check_spec_sample(V, path, dtype, gamma, vs.SPEC_WARPERS)
    _note("spec_sample", V, path, dtype)
    print(f"[vocab-seams] spec_accept_sampled V={V} path ({path}) {str(dtype)[6:]} gamma={gamma}: {tally.rows} rows checked, "
          f"{tally.ambiguous} of the random rows ambiguous")


def test_sampled_verification_at_the_largest_vocabulary():
    from flasht5_amd import speculative_accept
    _check_spec_sample(vs.MAX_V, "a", torch.bfloat16, 1, vs.SPEC_WARPERS[:1], philox=False)
    ln = vs.spec_sample_case(9, torch.bfloat16, 1)
    t, _, _ = _spec_tensors(ln, "a")
    big = torch.zeros(4, 2, vs.MAX_V + 1, dtype=torch.bfloat16, device=DEV)
    before = {k: t[k].clone() for k in ("labels", "tok", "cache_seqlens", "seen_eos")}
    with pytest.raises(ValueError, match="outside"):
        speculative_accept(big, t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"], sampling=(1.0, 0, 1.0, 1))
    with pytest.raises(ValueError, match="outside"):
        speculative_accept(big, t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"])
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], before[k]) for k in before)


# ------------------------------------------------------------------------------------------------------------------ beam_step
def _close(got, want):
    """test_beam_gpu.py's bound on a score whose lse is not exact in fp32"""
    return bool(((got - want).abs() <= 1e-5 * want.abs().clamp(min=1.0)).all())


def _run_beam(V, k, path, dtype, items=vs.BEAM_ITEMS):
    from flasht5_amd.beam import beam_step, new_state
    c = vs.beam_case(V, k, dtype, items)
    B, L = len(items), vs.BEAM_MAX_LENGTH + 1
    for norm in (False, True):
        want = vs.beam_expected(c, norm)
        st = new_state(B, k, L, L, DEV)
        lens = torch.zeros(B * k, dtype=torch.int32, device=DEV)
        for s, x in enumerate(c["steps"], 1):
            view, buf = _placed(x, path)
            lens.fill_(s)
            beam_step(view, st, lens, vs.BEAM_MAX_LENGTH, 1.0, False, logits_normalized=norm)
            torch.cuda.synchronize()
            tok_ref, ref = want[s - 1]
            what = (V, k, path, "normalized" if norm else "raw", s)
            assert vs.padding_untouched(view, buf, NAN), what
            assert torch.equal(st.tokens.cpu(), tok_ref), what + (st.tokens.cpu().view(B, k), tok_ref.view(B, k))
            for name in STATE:
                got = getattr(st, name).cpu().view(B, -1)
                exp = ref[name].view(B, -1)
                for it, item in enumerate(items):
                    if norm or vs.BEAM_EXACT[item] or not got.dtype.is_floating_point:
                        assert torch.equal(got[it], exp[it]), what + (item, name, got[it], exp[it])
                    else:
                        assert _close(got[it], exp[it]), what + (item, name, got[it], exp[it])


@pytest.mark.parametrize("V, path", [pytest.param(V, p, id=f"V{V}-{p}") for V in vs.beam_sizes() for p in vs.PATHS])
def test_beam_step(V, path):
    dtype = vs.dtype_for("beam", V, path)
    for k in vs.beam_ks(V):
        _run_beam(V, k, path, dtype)
    _note("beam", V, path, dtype)
    print(f"[vocab-seams] beam_step V={V} path ({path}) {str(dtype)[6:]}: k in {vs.beam_ks(V)}, raw and normalized, two steps")


def test_beam_step_at_the_largest_vocabulary():
    from flasht5_amd.beam import beam_step, new_state
    _run_beam(vs.MAX_V, 2, "a", torch.float16, items=("tie",))
    st = new_state(1, 2, 7, 7, DEV)
    before = {name: getattr(st, name).clone() for name in STATE}
    with pytest.raises(ValueError, match="outside"):
        beam_step(torch.zeros(2, vs.MAX_V + 1, dtype=torch.float16, device=DEV), st, torch.ones(2, dtype=torch.int32, device=DEV), 6)
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(st, name), before[name]) for name in STATE)


# ------------------------------------------------------------------------------------------------------------------ process_logits
OUT_FILL = -7.0


def _out_view(rows, V, aligned):
    """an fp32 output of row stride a multiple of 4 on an aligned base (16-byte stores), or one element into such a buffer"""
    stride = (V // 4 + 1) * 4 + 4
    buf = torch.full((rows * stride + 16,), OUT_FILL, dtype=torch.float32, device=DEV)
    view = buf.as_strided((rows, V), (stride, 1), 0 if aligned else 1)
    assert (view.data_ptr() % 16 == 0 and stride % 4 == 0) == aligned
    return view, buf


def _process_c_abi(c, x, out, log_softmax):
    """fat5_process_logits through the C ABI: `out` is the caller's (rows, V) fp32 view, or `x` itself (in place)"""
    from flasht5_amd import _lib
    from flasht5_amd.logits_process import pack_bad_words
    cfg = c["cfg"]
    rows, V = x.shape
    seq, lens = c["seqs"].to(DEV), c["lens"].to(DEV)
    keep = [seq, lens]
    p = _lib.LogitsParams()
    p.rows, p.V, p.dtype, p.log_softmax = rows, V, _lib.dtype_code(x.dtype), int(log_softmax)
    p.logits, p.row_stride, p.out, p.out_stride = x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0)
    p.sequences, p.seq_stride, p.seq_len, p.lengths = seq.data_ptr(), seq.stride(0), seq.shape[1], lens.data_ptr()
    p.repetition_penalty, p.no_repeat_ngram_size = cfg["repetition_penalty"], cfg["no_repeat_ngram_size"]
    p.min_length, p.eos_token_id = cfg["min_length"], cfg["eos_token_id"]
    if cfg["suppress_tokens"]:
        sup = torch.tensor(cfg["suppress_tokens"], dtype=torch.int32, device=DEV)
        keep.append(sup)
        p.n_suppress, p.suppress_tokens = sup.numel(), sup.data_ptr()
    if c["ext"]:
        enc = c["enc"].to(DEV)
        bad = pack_bad_words(cfg["bad_words_ids"], torch.device(DEV, torch.cuda.current_device()), cfg["eos_token_id"])
        keep += [enc, bad]
        p.encoder_repetition_penalty, p.encoder_no_repeat_ngram_size = cfg["encoder_repetition_penalty"], cfg["encoder_no_repeat_ngram_size"]
        p.encoder_input_ids, p.encoder_stride, p.encoder_rows, p.encoder_len = enc.data_ptr(), enc.stride(0), enc.shape[0], enc.shape[1]
        p.rows_per_encoder_row, p.prompt_length = 1, 1
        p.bad_words_ids, p.bad_words_offsets = bad.ids.data_ptr(), bad.offsets.data_ptr()
        p.n_bad_words, p.n_bad_word_ids = bad.offsets.numel() - 1, bad.ids.numel()
        p.forced_tokens, p.forced_bos_token_id = _lib.FAT5_FORCED_BOS, cfg["forced_bos_token_id"]
    _lib.check(_lib.load().fat5_process_logits(ctypes.byref(p), _lib.stream_ptr(x.device)), "fat5_process_logits")
    torch.cuda.synchronize()
    del keep


def _compare_logits(y, want, rows_kind, what):
    """test_logits_proc_gpu.py's comparisons: bitwise without log_softmax and on exact-lse rows, else the bans exactly and the
    finite values within 1e-5 (relative)"""
    y = y.cpu()
    assert torch.equal(y == NINF, want == NINF), what
    if rows_kind != "mass":
        assert torch.equal(_bits(y), _bits(want)), what + ((_bits(y) != _bits(want)).nonzero()[:8],)
        return
    fin = torch.isfinite(want)
    err = ((y - want).abs() / want.abs().clamp(min=1.0))[fin].max().item()
    assert err <= 1e-5, what + (err,)
    assert torch.equal(_bits(y)[~fin], _bits(want)[~fin]), what


def _run_logits(V, path, dtype):
    from flasht5_amd import process_logits
    for ext in (False, True):
        for rows_kind in ("plain", "exact", "mass"):
            c = vs.logits_case(V, dtype, ext, rows_kind)
            ls = rows_kind != "plain"
            want = vs.logits_expected(c, log_softmax=ls)
            what = (V, path, "ext" if ext else "plain", rows_kind)
            x, xbuf = _placed(c["x"], path)
            kw = dict(c["cfg"], log_softmax=ls)
            if ext:
                kw.update(encoder_input_ids=c["enc"].to(DEV))
            y = process_logits(x, c["seqs"].to(DEV), c["lens"].to(DEV), **kw)
            _compare_logits(y, want, rows_kind, what + ("wrapper",))
            for aligned in (True, False):   # the output's 16-byte stores, decided apart from the input's loads
                out, obuf = _out_view(x.shape[0], V, aligned)
                _process_c_abi(c, x, out, ls)
                _compare_logits(out, want, rows_kind, what + ("out aligned" if aligned else "out misaligned",))
                assert vs.padding_untouched(out, obuf, OUT_FILL), what
            assert vs.padding_untouched(x, xbuf, NAN), what
    # one in-place fp32 call: every edit is computed from the input value, the padding behind V stays NaN
    c = vs.logits_case(V, torch.float32, True, "plain")
    x, xbuf = _placed(c["x"], path)
    _process_c_abi(c, x, x, False)
    _compare_logits(x, vs.logits_expected(c), "plain", (V, path, "in place"))
    assert vs.padding_untouched(x, xbuf, NAN), (V, path, "in place")


@pytest.mark.parametrize("V, path", _params("logits"))
def test_process_logits(V, path):
    dtype = vs.dtype_for("logits", V, path)
    _run_logits(V, path, dtype)
    _note("logits", V, path, dtype)
    print(f"[vocab-seams] process_logits V={V} path ({path}) {str(dtype)[6:]}: plain and EXT, three row kinds, wrapper + two output "
          "alignments, one in-place fp32 call")


def test_process_logits_at_the_largest_vocabulary():
    from flasht5_amd import process_logits
    V = vs.MAX_V
    c = vs.logits_case(V, torch.bfloat16, True, "mass")
    x, xbuf = _placed(c["x"][:1], "a")
    c1 = dict(c, seqs=c["seqs"][:1], lens=c["lens"][:1], enc=c["enc"][:1], x=c["x"][:1])   # (row 0 alone: one row at this size)
    y = process_logits(x, c1["seqs"].to(DEV), c1["lens"].to(DEV), log_softmax=True, encoder_input_ids=c1["enc"].to(DEV), **c["cfg"])
    _compare_logits(y, vs.logits_expected(c1, log_softmax=True), "mass", (V, "wrapper"))
    assert vs.padding_untouched(x, xbuf, NAN)
    with pytest.raises(ValueError, match="outside"):
        process_logits(torch.zeros(1, V + 1, dtype=torch.bfloat16, device=DEV), c1["seqs"].to(DEV), c1["lens"].to(DEV), min_length=3)


# ------------------------------------------------------------------------------------------------------------------ greedy verification
def _run_argmax(ln, path):
    from flasht5_amd import speculative_accept
    t, lab_buf, lg = _spec_tensors(ln, path)
    na, nn = speculative_accept(t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"],
                                draft_seqlens=t["draft_seqlens"], eos_token_id=vs.ARGMAX_EOS)
    torch.cuda.synchronize()
    got = {k: t[k].cpu() for k in ("labels", "tok", "cache_seqlens", "draft_seqlens", "seen_eos")}
    got["n_accepted"], got["n_new"] = na.cpu(), nn.cpu()
    want = vs.argmax_expected(ln)
    for k in G.OUTPUTS:
        assert torch.equal(got[k], want[k]), (path, k, got[k].tolist(), want[k].tolist())
    guards = lab_buf.cpu()
    assert bool((guards[:, :GUARD] == -7).all()) and bool((guards[:, -GUARD:] == -7).all()), "guard columns"
    assert vs.padding_untouched(*lg, NAN)


@pytest.mark.parametrize("V, path", _params("argmax"))
def test_greedy_verification_argmax(V, path):
    dtype = vs.dtype_for("argmax", V, path)
    ln = vs.argmax_case(V, dtype)
    _run_argmax(ln, path)
    _note("argmax", V, path, dtype)
    print(f"[vocab-seams] spec_accept (argmax) V={V} path ({path}) {str(dtype)[6:]}: {ln['logits'].shape[0] * ln['logits'].shape[1]} rows, "
          f"{-(-V // vs.slice_of('argmax'))} slice(s)")


def test_greedy_verification_at_the_largest_vocabulary():
    _run_argmax(vs.argmax_case(vs.MAX_V, torch.bfloat16, plain_rows=1), "a")   # (the refusal at 2^20 + 1: with the sampled verification)


# ------------------------------------------------------------------------------------------------------------------ what ran
KERNELS = dict(sample="sample_logits_kernel<DT, 8 | 0>", spec_sample="spec_warp_kernel<DT, 8 | 0> + spec_sample_accept_kernel<DT>",
               beam="beam_topk_kernel<DT>", logits="process_logits_kernel<DT, false | true>", argmax="spec_argmax_kernel<DT> + spec_accept_kernel")


def test_zz_coverage():
    """one line per kernel: on paths (a), (b) and (c) every seam class was met, and on path (a) by every dtype (of the families
    whose cases all ran and passed in this session; a selection with -k prints what it met and asserts nothing)"""
    for f in vs.FAMILIES:
        seen = SEEN[f]
        if not seen:
            continue
        if len(RAN[f]) < len(vs.sizes(f)) * len(vs.PATHS):
            print(f"[vocab-seams] {KERNELS[f]}: {len(RAN[f])} of {len(vs.sizes(f)) * len(vs.PATHS)} cases ran")
            continue
        classes = list(vs.seam_classes(f))
        paths = {p: sorted({c for q, c, _ in seen if q == p}) for p in vs.PATHS}
        on_a = {c: sorted({str(d)[6:] for q, k, d in seen if q == "a" and k == c}) for c in classes}
        print(f"[vocab-seams] {KERNELS[f]}: " + "; ".join(f"({p}) {', '.join(paths[p])}" for p in vs.PATHS)
              + " | dtypes on (a): " + "; ".join(f"{c} {'/'.join(on_a[c])}" for c in classes))
        for p in vs.PATHS:
            assert paths[p] == sorted(classes), (f, p, paths[p])
        for c in classes:
            assert len(on_a[c]) == 3, (f, c, on_a[c])
