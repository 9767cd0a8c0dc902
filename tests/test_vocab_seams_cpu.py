"""What tests/test_vocab_seams_gpu.py rests on, proved without a GPU: the seam table of tests/vocab_seams.py is the kernels' own
(the constants are read out of the four headers), every case is sensitive to every planted index it names (replacing that one
input element by the row's background value changes the restatement's expected output, and a tie resolved to the other index
changes the pick), and nothing in the sampler's cases is ambiguous: every top-p margin is at least 100 * TOL and every injected
uniform lies at least 100 * TOL * S_kept inside its token's interval -- or, on the rows whose kept masses are all exactly 2^40
(an all-equal row, the kept maxima of the adjacent-values and signed-zero rows, whose intervals are narrower than that at large
V), the draw is integer arithmetic in the kernel and in the restatement alike and is compared with tolerance zero.  So the GPU test
has no skip branch."""
import math
import os
import re

import pytest
import torch

import sampling_ref as S
import spec_ref as G
import spec_sample_ref as R
import vocab_seams as vs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flasht5_amd", "csrc")
NINF = float("-inf")


# ------------------------------------------------------------------------------------------------------------------ the table
def _constants(*headers):
    """every `constexpr int NAME = <integer expression over earlier names>;` of the headers, evaluated"""
    env = {}
    for h in headers:
        with open(os.path.join(CSRC, h)) as f:
            for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", f.read()):
                e = re.sub(r"[A-Za-z_]\w*", lambda m: str(env[m.group(0)]), expr)
                assert re.fullmatch(r"[0-9\s*/+\-<>()]+", e), (name, expr)
                env[name] = int(eval(e, {"__builtins__": {}}))
    return env


def test_the_table_is_the_headers():
    c = _constants("sample_kernels.h", "beam_kernels.h", "logits_kernels.h", "spec_kernels.h")
    assert c["SAMPLE_THREADS"] == vs.THREADS["sample"] == vs.THREADS["spec_sample"]
    assert c["BEAM_TOPK_THREADS"] == vs.THREADS["beam"] and c["LOGITS_THREADS"] == vs.THREADS["logits"]
    assert c["SPEC_THREADS"] == vs.THREADS["argmax"]
    assert c["SAMPLE_TILE"] == vs.tile("sample") == c["SAMPLE_THREADS"] * vs.ELEMS
    assert c["BEAM_TILE"] == vs.tile("beam") and c["LOGITS_TILE"] == vs.tile("logits") and c["SPEC_TILE"] == vs.tile("argmax")
    assert c["SAMPLE_REG_TILES"] == vs.SAMPLE_REG_TILES and c["SAMPLE_REG_TILES"] * c["SAMPLE_TILE"] == vs.reg_limit("sample")
    assert c["SPEC_SLICE_TILES"] == vs.SPEC_SLICE_TILES and c["SPEC_SLICE"] == vs.slice_of("argmax")
    assert c["SAMPLE_MAX_V"] == c["LOGITS_MAX_V"] == c["SPEC_MAX_V"] == vs.MAX_V
    # the layout every kernel shares: thread t owns [8t, 8t + 8) of a tile, 16-byte loads under `vec && j0 + 8 <= V`
    for h in ("sample_kernels.h", "beam_kernels.h", "logits_kernels.h", "spec_kernels.h"):
        with open(os.path.join(CSRC, h)) as f:
            src = f.read()
        assert re.search(r"tid \* 8", src) and re.search(r"vec && j0 \+ 8 <= V", src), h


def test_the_sizes_and_the_planted_indices():
    t4096 = [7, 8, 9, 511, 512, 513, 4095, 4096, 4097]
    assert vs.sizes("sample") == vs.sizes("spec_sample") == [1] + t4096 + [32767, 32768, 32769, 32776]
    assert vs.sizes("beam") == vs.sizes("logits") == [2] + t4096
    assert vs.sizes("argmax") == [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193, 16385]
    assert vs.planted("sample", 32776) == [0, 7, 8, 511, 512, 4095, 4096, 8191, 32767, 32768, 32775]   # (V - 9 and V - 8 are 32767, 32768)
    assert vs.planted("argmax", 16385) == [0, 7, 8, 511, 512, 2047, 2048, 4095, 8191, 8192, 16376, 16377, 16384]
    assert vs.planted("beam", 9) == [0, 1, 7, 8] and vs.planted("logits", 2) == [0, 1] and vs.planted("sample", 1) == [0]
    big = vs.planted("sample", vs.MAX_V)
    assert big[-3:] == [vs.MAX_V - 9, vs.MAX_V - 8, vs.MAX_V - 1] and 32768 in big and 8191 in big


def test_the_dtype_rotation_and_the_load_paths():
    for f in vs.FAMILIES:
        for name, at in vs.seam_classes(f).items():   # on path (a) every dtype meets every seam class
            assert {vs.dtype_for(f, V, "a") for V in at} == set(vs.DTYPES), (f, name)
        for V in vs.sizes(f):
            assert len({vs.dtype_for(f, V, p) for p in vs.PATHS}) == 3
            sa, oa = vs.layout(V, "a")
            sb, ob = vs.layout(V, "b")
            sc, oc = vs.layout(V, "c")
            assert sa % 8 == 0 and sa >= V + 8 and oa == 0 and sb % 2 == 1 and sb >= V + 8 and ob == 0 and sc % 8 == 0 and oc == 1
    x = torch.arange(2 * 3 * 9, dtype=torch.float32).view(2, 3, 9)
    for p in vs.PATHS:
        view, buf = vs.place(x, p, math.nan)
        assert torch.equal(view, x) and view.stride(2) == 1 and view.stride(0) == 3 * view.stride(1)
        assert vs.padding_untouched(view, buf, math.nan)
        aligned = view.data_ptr() % 16 == 0 and view.stride(1) % 8 == 0 and view.stride(0) % 8 == 0
        assert aligned == vs.vec_expected(p), p
        buf[-1] = 0.0
        assert not vs.padding_untouched(view, buf, math.nan)


# ------------------------------------------------------------------------------------------------------------------ the sampler
def _check_sample_call(c, V, sensitive=True):
    e = vs.sample_expected(c)
    what = (V, c["kind"])
    if e["degenerate"]:
        assert c["kind"] in ("nan-after-inf", "inf-after-finite", "nan-last", "all-ninf"), what
        for j in c["planted"] if V > 1 else []:
            x = c["x"].clone()
            x[j] = c["bg"][j]
            assert not vs.same_sample(e, vs.sample_expected(c, x)), what + (j,)
        return
    assert e["margin"] >= vs.WIDE, what + (e["margin"],)
    if c["exact"]:
        assert e["ones"], what
    else:
        assert all(e["wide"]), what + (e["wide"],)
    assert all(e["r"]["kept"][t] for t in e["tokens"])
    if c["kind"] == "draw":     # one uniform per planted index, each token that index, everything kept
        assert e["tokens"][:len(c["planted"])] == c["planted"] and e["kept"] == V and e["ratio"] == 1.0, what
    if c["kind"].startswith("topk") and 0 < c["top_k"] < V:   # all ties of the k-th value are kept
        kth = sorted(S.scaled(c["x"], 1.0).tolist(), reverse=True)[c["top_k"] - 1]
        assert e["tau"] == kth and e["kept"] == int((c["x"].float() >= kth).sum()) >= c["top_k"], what
    for j in c["planted"] if sensitive else []:
        x = c["x"].clone()
        x[j] = c["bg"][j]
        assert not vs.same_sample(e, vs.sample_expected(c, x)), what + (j,)


@pytest.mark.parametrize("dtype", vs.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("V", vs.sizes("sample"))
def test_sampler_cases_are_unambiguous_and_sensitive(V, dtype):
    calls = vs.sample_calls(V, dtype)
    kinds = [c["kind"] for c in calls]
    assert len(set(kinds)) == len(kinds) and {"draw", "equal", "adjacent-hi", "zeros-p", "zeros-k1", "lowbins-all", "nan-after-inf"} <= set(kinds)
    if V > 2:
        assert {f"topk{k}" for k in (1, 2, V - 1, V, V + 1)} <= set(kinds)
    for c in calls:
        assert c["x"].dtype == dtype and c["x"].shape == (V,) and len(c["us"]) >= 2
        _check_sample_call(c, V)
    taus = {k: vs.sample_expected(c)["tau"] for k, c in zip(kinds, calls) if k.startswith(("negative", "positive"))}
    for name in ("negative", "positive"):   # tau is the row maximum, the row minimum and a value between them
        x = next(c for c in calls if c["kind"] == f"{name}-tau-1")["x"].float()
        assert taus[f"{name}-tau-1"] == x.max() and taus[f"{name}-tau0"] == x.min(), (V, name)
        assert V < 8 or x.min() < taus[f"{name}-taumid"] < x.max(), (V, name)
    if dtype == torch.float32 and V > 1:    # two values adjacent in fp32: the last pass of the radix select decides
        x = next(c for c in calls if c["kind"] == "adjacent-lo")["x"]
        hi, lo = x.max(), x[x > -1.0].min()
        assert S.scaled(x, 1.0).dtype.itemsize == 4 and hi.view(torch.int32) - lo.view(torch.int32) == 1


def test_sampler_cases_at_the_largest_vocabulary():
    calls = vs.sample_calls(vs.MAX_V, torch.float32, kinds=vs.SAMPLE_BIG_KINDS)
    assert [c["kind"] for c in calls] == list(vs.SAMPLE_BIG_KINDS)
    for c in calls:
        _check_sample_call(c, vs.MAX_V, sensitive=c["kind"] == "draw")


# ------------------------------------------------------------------------------------------------------------------ the argmax
@pytest.mark.parametrize("V", vs.sizes("argmax") + [vs.MAX_V])
def test_argmax_cases_are_sensitive(V):
    ln = vs.argmax_case(V, vs.dtype_for("argmax", V, "a"), plain_rows=1 if V == vs.MAX_V else None)
    want = vs.argmax_expected(ln)
    M = ln["logits"].shape[1]
    assert want["n_accepted"].tolist() == [M - 1] * ln["logits"].shape[0] and want["n_new"].tolist() == [M] * ln["logits"].shape[0]
    assert V == vs.MAX_V or {j for _, _, j in ln["planted"]} >= set(vs.planted("argmax", V))   # every planted index is some position's argmax
    if V == 1:
        return   # (one token: nothing else can be picked)
    for b, i, j in ln["planted"]:
        x = ln["logits"].clone()
        x[b, i, j] = ln["bg"][j]
        assert not G.same(want, vs.argmax_expected(ln, x)), (V, b, i, j)
    assert not G.same(want, vs.argmax_expected(ln, mutant="tie_highest")), V   # the other index of a tie is another pick


# ------------------------------------------------------------------------------------------------------------------ the logits processors
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("V", vs.sizes("logits") + [vs.MAX_V])
def test_logits_cases_are_sensitive(V, ext):
    for rows in ("plain", "exact", "mass"):
        c = vs.logits_case(V, vs.dtype_for("logits", V, "a"), ext, rows)
        ls = rows != "plain"
        want = vs.logits_expected(c, log_softmax=ls)
        x32 = c["x"].float()
        if rows == "exact":   # the lse is the row maximum exactly, so the comparison is bitwise
            assert torch.equal(vs.proc_ref.lse_rows(x32), x32.max(-1, keepdim=True).values)
        edited = 0
        for j in c["planted"]:
            x = c["x"].clone()
            x[0, j] = c["bg"][0, j]
            moved = not torch.equal(vs.logits_expected(c, x, log_softmax=ls)[0, j], want[0, j])
            plain = x32[0, j] - (vs.proc_ref.lse_rows(x32)[0, 0] if ls else 0.0)
            edit = not torch.equal(want[0, j], plain)          # a penalty or a ban landed on the planted index
            assert moved or (edit and want[0, j] == NINF), (V, rows, j)
            edited += edit
        assert edited == len(c["planted"]), (V, rows)          # every planted index of row 0 carries an edit
        assert want[0, V - 1] == NINF                           # eos = V - 1 under min_length
        last = c["x"].clone()                                   # ... and row 2, past min_length, carries element V - 1 through (V >= 9)
        last[2, V - 1] = c["bg"][2, V - 1]
        assert len(c["planted"]) <= 2 or want[2, V - 1] != NINF and not torch.equal(vs.logits_expected(c, last, log_softmax=ls)[2, V - 1], want[2, V - 1])
        if ext:   # the forced row: 0 at the planted id, -inf elsewhere
            t = c["cfg"]["forced_bos_token_id"]
            assert want[1, t] == 0.0 and int((want[1] == NINF).sum()) == V - 1


# ------------------------------------------------------------------------------------------------------------------ the beam step
def _same_steps(a, b):
    return all(torch.equal(x[0], y[0]) and all(torch.equal(x[1][n], y[1][n]) for n in x[1]) for x, y in zip(a, b))


BEAM_CASES = [(V, k, vs.BEAM_ITEMS) for V in vs.beam_sizes() for k in vs.beam_ks(V)] + [(vs.MAX_V, 2, ("tie",))]


@pytest.mark.parametrize("V, k, items", BEAM_CASES, ids=[f"V{V}-k{k}" for V, k, _ in BEAM_CASES])
def test_beam_cases_are_sensitive(V, k, items):
    c = vs.beam_case(V, k, vs.dtype_for("beam", V, "a"), items)
    for it, name in enumerate(items):   # an exact item: every row's log_softmax is x - max, exactly
        x = c["steps"][0][it * k].float()
        if vs.BEAM_EXACT[name]:
            assert torch.equal(torch.log_softmax(x, -1), x - x.max())
    for norm in (False, True):
        want = vs.beam_expected(c, norm)
        run1 = want[0][1]["running_seqs"][:, :, 1]
        for it, name in enumerate(items):
            for j in c["planted"][name]:
                x = c["steps"][0].clone()
                x[it * k, j] = c["bg"][name][j]
                assert not _same_steps(want[:1], vs.beam_expected(c, norm, x)[:1]), (V, k, norm, name, j)
        # the threshold tie: the running beams hold the FIRST tied indices in vocabulary order, never a later one in their place
        m = len(c["planted"]["tie"])
        got = [t for t in run1[items.index("tie")].tolist() if t in c["tied"]]
        assert got[:m] == c["tied"][:m], (V, k, got, c["tied"])
        # the twin item: two beams leave step 1 with one score, and step 2 takes every tie between them from the lower beam first
        if "twin" in items and V > 2:
            it = items.index("twin")
            rs = want[0][1]["running_scores"][it]
            assert rs[0] == rs[1], (V, k, rs)
            parents = want[1][1]["cache_row_batch"].view(len(items), k, -1)[it, :, 1].tolist()
            assert parents[0] == it * k and it * k + 1 in parents, (V, k, parents)


# ------------------------------------------------------------------------------------------------------------------ the sampled verification
@pytest.mark.parametrize("gamma", [1, 4])
@pytest.mark.parametrize("V", vs.sizes("spec_sample"))
def test_sampled_verification_cases(V, gamma):
    dtype = vs.dtype_for("spec_sample", V, "a")
    ln = vs.spec_sample_case(V, dtype, gamma)
    L = vs.planted("spec_sample", V)
    assert set(ln["draft"].flatten().tolist()) <= set(L) and ln["logits"].shape == (4, gamma + 1, V)
    if V == 1:
        return
    star, d = ln["star"], ln["d"]
    for T, k, p in vs.SPEC_WARPERS:
        P = R.dist(ln["logits"][3, 0], T, k, p)
        for Q in (R.dist(ln["draft_logits"][3, 0], T, k, p), R.one_hot(V, d)):
            assert P["margin"] >= vs.WIDE and Q["margin"] >= vs.WIDE
            assert R.accept_margin(P, Q, d, 0.9) < -vs.WIDE                      # the first draft is rejected, far from the boundary
            assert R.residual_draw(P, Q, 0.5, vs.WIDE) == {star}                 # and the residual draw lands on the planted index
        x = ln["logits"].clone()
        x[3, :, star] = ln["bg"][star]
        args = (ln["draft"], ln["cache_seqlens"], ln["labels"], ln["tok"], ln["seen_eos"], ln["limit"], ln["draft_seqlens"])
        kw = dict(sampling=(T, k, p, 7), uniforms=ln["uniforms"])
        want = R.accept_sampled_ref(ln["logits"][3:], *[a[3:] if torch.is_tensor(a) else a for a in args], **{**kw, "uniforms": ln["uniforms"][3:]})
        other = R.accept_sampled_ref(x[3:], *[a[3:] if torch.is_tensor(a) else a for a in args], **{**kw, "uniforms": ln["uniforms"][3:]})
        assert want["sampled"][0, 0] == star and want["n"][0] == 0 and other["sampled"][0, 0] != star
