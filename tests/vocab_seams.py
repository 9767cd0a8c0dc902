"""The seam table of generation's vocabulary-row kernels and the cases built on it (CPU only; nothing here imports the package).

Five kernel families walk one logits row per workgroup with one layout: thread t owns elements [8t, 8t + 8) of every tile, a
16-byte load where `vec` is set and j0 + 8 <= V, element loads otherwise, block scans carried from tile to tile.

    family        kernel (csrc header)                                              threads / tile   further structure
    sample        sample_logits_kernel<DT, NREG>      (sample_kernels.h)            512 / 4096       register-resident up to 32768
    spec_sample   spec_warp_kernel + spec_sample_accept_kernel (spec_sample_kernels.h)  512 / 4096   the same parts, the same limit
    beam          beam_topk_kernel                    (beam_kernels.h)              512 / 4096       V >= 2
    logits        process_logits_kernel<DT, EXT>      (logits_kernels.h)            512 / 4096       V >= 2, vec and vec_out apart
    argmax        spec_argmax_kernel + spec_accept_kernel (spec_kernels.h)          256 / 2048       slices of 4 tiles = 8192

Everything below is derived from five constants (threads, ELEMS, SAMPLE_REG_TILES, SPEC_SLICE_TILES, MAX_V);
tests/test_vocab_seams_cpu.py reads the same constants out of the headers, so a retuned kernel fails the table and does not move
its seams off the tested sizes.  `sizes(f)` are the vocabulary sizes at a chunk, a wave's span, a tile, a slice and the register
limit (and one either side); `planted(f, V)` the indices J(V): the first and last element of a thread, a wave, a tile, a slice
and the register-resident part, and the elements of the ragged tail.  `layout` gives the three load paths: (a) an aligned base and
a row stride that is a multiple of 8 (16-byte loads, a ragged last chunk wherever V % 8 != 0), (b) an odd row stride, (c) a view
that starts one element into such a buffer (element loads for the whole row in both).

The case builders give CPU tensors in which every decision is made on a planted index and nothing is ambiguous, and the
`*_expected` functions restate them with the modules the kernels' own tests use (sampling_ref, spec_sample_ref, beam_ref,
logits_proc_ref, logits_proc_ext_ref, spec_ref).  test_vocab_seams_cpu.py proves the cases sensitive and unambiguous without a
GPU; test_vocab_seams_gpu.py runs the kernels on them."""
import math

import numpy as np
import torch

import beam_ref
import logits_proc_ext_ref as ext_ref
import logits_proc_ref as proc_ref
import sampling_ref as S
import spec_ref as G
import spec_sample_ref as R

ELEMS = 8               # elements per thread and tile
SAMPLE_REG_TILES = 8    # register-resident tiles of the sampler and the sampled verification
SPEC_SLICE_TILES = 4    # tiles per slice of the argmax
MAX_V = 1 << 20         # SAMPLE_MAX_V = LOGITS_MAX_V = SPEC_MAX_V
THREADS = dict(sample=512, spec_sample=512, beam=512, logits=512, argmax=256)
MIN_V = dict(sample=1, spec_sample=1, beam=2, logits=2, argmax=1)
FAMILIES = tuple(THREADS)
TOL = 4e-6              # tests/test_sampling_gpu.py's TOL: the sampler's __expf against exp in fp64, relative to S
WIDE = 100 * TOL        # every top-p margin and every injected uniform here keeps this distance from its boundary
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
PATHS = ("a", "b", "c")
NINF = float("-inf")


# ------------------------------------------------------------------------------------------------------------------ the table
def tile(f):
    return THREADS[f] * ELEMS


def slice_of(f):
    return tile(f) * SPEC_SLICE_TILES if f == "argmax" else None


def reg_limit(f):
    return tile(f) * SAMPLE_REG_TILES if f in ("sample", "spec_sample") else None


def seam_classes(f):
    """seam class -> the sizes at it: the seam and one either side (the register limit adds the first size whose last chunk is
    whole again; the slices add a third slice with one element)"""
    c = dict(chunk=[ELEMS - 1, ELEMS, ELEMS + 1], wave=[64 * ELEMS - 1, 64 * ELEMS, 64 * ELEMS + 1],
             tile=[tile(f) - 1, tile(f), tile(f) + 1])
    if slice_of(f):
        c["slice"] = [slice_of(f) - 1, slice_of(f), slice_of(f) + 1, 2 * slice_of(f) + 1]
    if reg_limit(f):
        c["reg"] = [reg_limit(f) - 1, reg_limit(f), reg_limit(f) + 1, reg_limit(f) + ELEMS]
    return c


def sizes(f):
    return [MIN_V[f]] + [v for vs in seam_classes(f).values() for v in vs]


def planted(f, V):
    """J(V), sorted"""
    t = tile(f)
    j = {0, ELEMS - 1, ELEMS, 64 * ELEMS - 1, 64 * ELEMS, t - 1, t, 2 * t - 1, V - 9, V - 8, V - 1}
    if slice_of(f):
        j |= {slice_of(f) - 1, slice_of(f)}
    if reg_limit(f):
        j |= {reg_limit(f) - 1, reg_limit(f)}
    return sorted(i for i in j if 0 <= i < V)


def layout(V, path):
    """(row stride, offset of the first row in its buffer), in elements"""
    mult8 = (V // 8 + 1) * 8 + 8          # the next multiple of 8 above V, plus 8
    if path == "a":
        return mult8, 0
    if path == "b":
        return V + 9 - V % 2, 0           # odd
    return mult8, 1


def vec_expected(path):
    return path == "a"


def dtype_for(f, V, path):
    """the dtype rotates with the size and the path, so that on path (a) the three sizes of every seam class meet all three"""
    s = sizes(f)
    i = s.index(V) if V in s else V % 3
    return DTYPES[(i + PATHS.index(path)) % 3]


def place(x, path, fill, device="cpu"):
    """x (..., V) -> (view of that shape on `device` laid out for `path`, its buffer): rows one after the other with the
    path's stride, every element outside the view holding `fill`"""
    V = x.shape[-1]
    rows = x.numel() // V
    stride, off = layout(V, path)
    buf = torch.full((rows * stride + 16,), fill, dtype=x.dtype, device=device)
    shape = tuple(x.shape)
    strides = [stride, 1] if len(shape) > 1 else [1]
    for n in reversed(shape[1:-1]):
        strides.insert(0, strides[0] * n)
    view = buf.as_strided(shape, strides, off)
    view.copy_(x.to(device))
    return view, buf


def padding_untouched(view, buf, fill):
    """whether every element of `buf` outside `view` still holds `fill` (NaN compares as equal to NaN)"""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask.as_strided(tuple(view.shape), view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    rest = buf[mask]
    return bool(torch.isnan(rest).all()) if isinstance(fill, float) and math.isnan(fill) else bool((rest == fill).all())


def _grid(V):
    """a coarse value grid, exact in bf16 and fp16: 0, 0.25, .. 1.75 by index"""
    return 0.25 * (torch.arange(V) % 8).float()


def _exact(x, dtype):
    """x (fp32) in `dtype`; every value the builders write is representable, so nothing is rounded"""
    y = x.to(dtype, copy=True)
    fin = torch.isfinite(x)
    assert torch.equal(y.float()[fin], x[fin]), "a case value is not exact in " + str(dtype)
    return y


# ------------------------------------------------------------------------------------------------------------------ the sampler
def _significant_groups(x):
    """the value groups of row x (fp32, T = 1) in ascending order and their cumulative share of the mass"""
    xd = S.scaled(x, 1.0).astype(np.float64)
    e = np.exp(xd - xd[np.isfinite(xd)].max())
    vals, inv = np.unique(xd, return_inverse=True)
    mass = np.bincount(inv.reshape(-1), weights=e, minlength=len(vals))
    return vals, np.cumsum(mass) / mass.sum(), mass / mass.sum()


def top_p_for(x, which):
    """the top_p (an fp32 value) that puts (1 - p) S at the middle of a value group's mass, so that tau is that group's value:
    which = -1 the highest group, -2 the one below it, 0 the lowest, "mid" the middle one -- of the groups holding >= 1e-3 of S"""
    vals, C, share = _significant_groups(x)
    idx = np.nonzero(share >= 1e-3)[0]
    i = int(idx[len(idx) // 2] if which == "mid" else idx[max(which, -len(idx))])
    lo = C[i - 1] if i > 0 else 0.0
    return float(np.float32(1.0 - (lo + C[i]) / 2))


def _mid_uniform(r, j):
    """the fp32 uniform at the middle of token j's prefix interval in the restated row r"""
    P = np.cumsum(r["e"])
    return float(np.float32((P[j] - r["e"][j] / 2) / P[-1]))


def _sample_call(kind, x, bg, plant, dtype, top_k=0, top_p=1.0, T=1.0, us=None, exact=False):
    c = dict(kind=kind, x=x if x.dtype == dtype else _exact(x, dtype), bg=bg if bg.dtype == dtype else _exact(bg, dtype),
             planted=list(plant), T=T, top_k=int(top_k), exact=exact)
    top_p = c["top_p"] = top_p_for(c["x"], top_p[1]) if isinstance(top_p, tuple) else top_p   # ("tau", which): see top_p_for
    if us is None:   # one uniform per kept planted index, at the middle of its interval
        r = S.restate(S.scaled(c["x"], T), c["top_k"], top_p)
        us = [_mid_uniform(r, j) for j in plant if r["kept"][j] and r["e"][j] > 0]
        c["planted"] = [j for j in plant if r["kept"][j]]   # (the call names the planted indices its filters keep)
    us = [float(np.float32(u)) for u in us]
    c["us"] = us if len(us) > 1 else us * 2   # (two rows at least: one row alone has no row stride)
    return c


SAMPLE_BIG_KINDS = ("draw", "topk3", f"topk{MAX_V - 1}", "negative-taumid", "lowbins-p", "nan-after-inf")   # what runs at V = 2^20


class _Calls(list):
    def __init__(self, kinds):
        super().__init__()
        self.kinds = kinds

    def add(self, kind, *a, **kw):
        if self.kinds is None or kind in self.kinds:
            self.append(_sample_call(kind, *a, **kw))


def sample_calls(V, dtype, f="sample", kinds=None):
    """the sampler's calls at one size (kinds: only these): each one logits row, run as len(us) equal rows with one injected
    uniform each"""
    L = planted(f, V)
    n = len(L)
    g = _grid(V)
    boost = float(max(2, round(math.log(V / n))))
    low = -20.0 - g
    out = _Calls(kinds)
    # 1. a draw on every seam element: the mass sits on J(V), one uniform per planted index
    x = low.clone()
    x[L] = 0.0
    out.add("draw", x, low, L, dtype)
    # 2. top-k: the k-th largest value on several planted indices of different threads, waves and tiles
    x = low.clone()
    above = [L[1], L[-2]] if n >= 4 else []
    ties = [j for j in L if j not in above]
    x[ties] = 4.0
    for j, v in zip(above, (6.0, 5.0)):
        x[j] = v
    for k in sorted({1, 2, len(above) + 1, V - 1, V, V + 1} - {0, -1}):
        out.add(f"topk{k}", x, low, L, dtype, top_k=k)
    # 3. top-p and the radix passes
    eq = torch.full((V,), 1.5)
    out.add("equal", eq, low, L, dtype, top_p=0.5, exact=True)
    one = torch.ones(1, dtype=dtype)
    below = (one.view(torch.int32 if dtype == torch.float32 else torch.int16) - 1).view(dtype)   # the value under 1.0 in dtype
    x = _exact(low, dtype)
    x[L[0::2]] = one
    x[L[1::2]] = below
    out.add("adjacent-hi", x, low, L, dtype, top_p=("tau", -1), exact=True)
    if n > 1:
        out.add("adjacent-lo", x, low, L, dtype, top_p=("tau", -2))
    x = low.clone()
    x[L[0::2]] = -0.0
    x[L[1::2]] = 0.0
    out.add("zeros-p", x, low, L, dtype, top_p=("tau", -1), exact=True)
    out.add("zeros-k1", x, low, L, dtype, top_k=1, exact=True)
    neg = -1.0 - boost - g
    xn = neg.clone()
    xn[L] = -1.0
    pos = 0.25 + g
    xp = pos.clone()
    xp[L] = 2.0 + boost
    for name, x, bg in (("negative", xn, neg), ("positive", xp, pos)):
        for which in (-1, 0, "mid"):
            out.add(f"{name}-tau{which}", x, bg, L, dtype, top_p=("tau", which))
    x = xn.clone()   # -inf entries and one finite entry at the bottom of the format: the lowest bins are in play
    free = [j for j in list(range(min(V, 64))) + list(range(max(V - 64, 64), V)) if j not in L]
    for j in [j for j in free if j % 8 == 3] + [j for j in free if j % 8 == 5][:1]:
        x[j] = NINF if j % 8 == 3 else (-65504.0 if dtype == torch.float16 else -3e38)
    x = x.to(dtype)
    for name, k, p in (("lowbins-p", 0, ("tau", "mid")), ("lowbins-k", V - 1, 1.0), ("lowbins-all", 0, 1.0)):
        if name != "lowbins-k" or k >= 1:
            out.add(name, x, neg, L, dtype, top_k=k, top_p=p)
    # 4. degenerate rows: the first NaN / +inf on a later tile than another candidate
    mid, last = L[n // 2], L[-1]
    for name, put, win in (("nan-after-inf", ((L[0], math.inf), (last, math.nan), (mid, math.nan)), mid),
                           ("inf-after-finite", ((L[0], 5.0), (last, math.inf), (mid, math.inf)), mid),
                           ("nan-last", ((last, math.nan),), last), ("all-ninf", (), None)):
        x = torch.full((V,), NINF) if name == "all-ninf" else low.clone()
        for j, v in put:
            x[j] = v
        out.add(name, x.to(dtype), _exact(low, dtype), [] if win is None else [win], dtype, top_k=5, top_p=0.5, T=0.9, us=[0.3, 0.6])
    return out


def sample_expected(c, x=None):
    """the restatement of one call (x: another row in place of the call's): per uniform the token, and tau, the kept count and
    S_kept / S; `wide[b]`: the uniform lies at least WIDE * S_kept inside its token's interval"""
    xs = S.scaled(c["x"] if x is None else x, c["T"])
    if np.isnan(xs).any() or (xs == np.inf).any() or (xs == -np.inf).all():
        return dict(degenerate=True, tokens=[S.argmax_rule(xs)] * len(c["us"]), margin=math.inf)
    r = S.restate(xs, c["top_k"], c["top_p"])
    toks = [min(S.draw(r, u)) for u in c["us"]]
    wide = [S.draw(r, u, WIDE) == {j} for u, j in zip(c["us"], toks)]
    ones = bool((r["e"][r["kept"]] == 1.0).all())   # every kept mass is exactly 2^40: the draw is integer arithmetic on both sides
    return dict(degenerate=False, r=r, tokens=toks, wide=wide, ones=ones, tau=r["tau"], kept=int(r["kept"].sum()), ratio=r["ratio"],
                margin=r["margin"])


def same_sample(a, b):
    if a["degenerate"] or b["degenerate"]:
        return a["degenerate"] == b["degenerate"] and a["tokens"] == b["tokens"]
    return a["tokens"] == b["tokens"] and a["tau"] == b["tau"] and a["kept"] == b["kept"] and abs(a["ratio"] - b["ratio"]) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ the argmax
PEAK = 8.0
GAMMA = 4
ARGMAX_EOS = 3   # (no planted index at any size of the table, so no row is cut at an EOS)


def argmax_case(V, dtype, gamma=GAMMA, plain_rows=None):
    """one greedy verification call: every position of every row has its maximum on a planted index, and every draft agrees, so
    all M argmaxes of a row reach the outputs.  -> spec_ref.inputs' dict plus `bg` (V,), `planted` [(b, i, j)] and `ties`"""
    L = planted("argmax", V)
    n, M = len(L), gamma + 1
    bg = -1.0 - 0.25 * ((torch.arange(V) + 3) % 8).float()   # (its own maximum sits on index 5, no planted index)
    nplain = -(-n // M) if plain_rows is None else plain_rows   # (all of J(V) takes ceil(n / M) rows)
    B = nplain + 2
    x = bg.repeat(B, M, 1)
    plant, want = [], torch.zeros(B, M, dtype=torch.long)
    for b in range(nplain):                      # every planted index is the maximum of some position
        for i in range(M):
            j = L[(b * M + i) % n]
            x[b, i, j] = PEAK
            plant.append((b, i, j))
            want[b, i] = j
    b = nplain                                   # the maximum twice, in different tiles and slices: the lower index
    for i in range(M):
        lo, hi = sorted((L[i % n], L[(i + max(n // 2, 1)) % n]))
        x[b, i, lo] = x[b, i, hi] = PEAK
        plant.append((b, i, lo))
        want[b, i] = lo
    b = nplain + 1
    mid, last = L[n // 2], L[-1]
    s, t = slice_of("argmax"), tile("argmax")
    z = s - 1 if V > s else (t - 1 if V > t else max(V - 2, 0))
    x[b, 0, L[0]], x[b, 0, last] = math.inf, math.nan          # a NaN in a later slice against +inf in an earlier one
    x[b, 1, mid], x[b, 1, last] = math.nan, math.nan           # two NaNs in different slices
    x[b, 2] = -1.0
    x[b, 2, z] = -0.0                                          # -0.0 against +0.0 across a slice boundary
    if z + 1 < V:
        x[b, 2, z + 1] = 0.0
    x[b, 3, mid], x[b, 3, last] = math.inf, math.inf           # two +inf
    x[b, 4, last] = PEAK
    for i, j in enumerate((last, mid, z, mid, last)):
        plant.append((b, i, j))
        want[b, i] = j
    g = torch.Generator().manual_seed(V)
    lens = torch.full((B,), 3 + M, dtype=torch.int32)
    return dict(logits=x.to(dtype), draft=want[:, :gamma].clone(), cache_seqlens=lens, labels=torch.randint(2, 100, (B, G.NCOLS), generator=g),
                tok=torch.randint(2, 100, (B,), generator=g), seen_eos=torch.zeros(B, dtype=torch.bool), limit=G.NCOLS - 1,
                draft_seqlens=lens.clone(), bg=bg.to(dtype), planted=plant, argmax=want, tie_row=nplain)


def argmax_expected(ln, logits=None, mutant=None):
    return G.accept_ref(ln["logits"] if logits is None else logits, ln["draft"], ln["cache_seqlens"], ln["labels"], ln["tok"],
                        ln["seen_eos"], ln["limit"], ln["draft_seqlens"], ARGMAX_EOS, mutant)


# ------------------------------------------------------------------------------------------------------------------ the logits processors
def logits_case(V, dtype, ext, rows="plain"):
    """one process_logits call of three rows whose edits fall on J(V): row 0 with the whole sequence (below min_length: eos =
    V - 1 banned), row 1 with the start token alone (the forced row of the EXT instance), row 2 three tokens longer than row 0
    and past min_length, so that element V - 1 itself comes through.  rows: "plain" (ordinary values), "exact" (the row lse is
    its maximum, exactly) or "mass" (the mass sits on J(V)).
    -> dict(x, bg, seqs, lens, cfg (the processors), enc (the encoder ids or None), planted)"""
    L = planted("logits", V)
    n = len(L)
    j = torch.arange(V)
    if rows == "plain":
        bg = ((j * 7) % 16 - 8).float() * 0.25
        x = bg.clone()
        for i, t in enumerate(L):
            x[t] = (3.0 + 0.25 * i) * (-1) ** i
    elif rows == "exact":
        bg = -120.0 - (j % 32).float()
        x = bg.clone()
        for i, t in enumerate(L):
            x[t] = -104.0 - i
        x[L[n // 2]] = 2.0
    else:
        bg = -30.0 - _grid(V)
        x = bg.clone()
        x[L] = 0.0
    seq0 = [0, L[-1]] + L[1:-1] + [0, L[n // 2], 0]
    Ls = len(seq0) + 3
    seqs = torch.full((3, Ls), L[0], dtype=torch.int64)
    seqs[0, :len(seq0)] = seqs[2, :len(seq0)] = torch.tensor(seq0)
    seqs[1, 0] = 0
    seqs[2, len(seq0):] = L[1 % n]   # (not the start token: the n-gram that bans V - 1 in row 0 does not end row 2)
    lens = torch.tensor([len(seq0), 1, Ls], dtype=torch.int32)
    cfg = dict(repetition_penalty=1.5, no_repeat_ngram_size=2, min_length=len(seq0) + 2, eos_token_id=V - 1,
               suppress_tokens=[L[1 % n]] if n > 3 else None)
    enc = None
    if ext:
        e = [L[2 % n], 0, L[3 % n]] + L[::-1]
        enc = torch.tensor([e, e[::-1], e], dtype=torch.int64)
        cfg.update(encoder_repetition_penalty=1.25, encoder_no_repeat_ngram_size=2, bad_words_ids=[[L[4 % n]], [0, L[5 % n]]],
                   forced_bos_token_id=L[n // 2])
    x1, bg1 = (x.flip(0), bg.flip(0)) if rows == "plain" else (x, bg)
    return dict(x=_exact(torch.stack([x, x1, x]), dtype), bg=_exact(torch.stack([bg, bg1, bg]), dtype),
                seqs=seqs, lens=lens, cfg=cfg, enc=enc, planted=L, ext=ext, rows=rows)


def logits_expected(c, x=None, log_softmax=False):
    x = c["x"] if x is None else x
    if c["ext"]:
        return ext_ref.process(x, c["seqs"], c["lens"], log_softmax=log_softmax, encoder_input_ids=c["enc"], **c["cfg"])
    return proc_ref.process(x, c["seqs"], c["lens"], log_softmax=log_softmax, **c["cfg"])


# ------------------------------------------------------------------------------------------------------------------ the beam step
BEAM_ITEMS = ("distinct", "tie", "twin", "mass")   # the batch items of a beam case, by the row kind of step 1
BEAM_EXACT = dict(distinct=True, tie=True, twin=False, mass=False)   # the item's lse is exact in fp32 (its decisions are in all four)
BEAM_STEP2 = dict(distinct="tie", tie="distinct", twin="distinct", mass="mass")
BEAM_MAX_LENGTH = 6
BEAM_KS = (2, 4, 16)


def beam_sizes():
    """the table's sizes, and V = 2k (Kr >= V takes everything) and 2k + 1 for every beam count"""
    return sorted(set(sizes("beam")) | {2 * k + d for k in BEAM_KS for d in (0, 1)})


def beam_ks(V):
    return list(BEAM_KS) if V in sizes("beam") else [k for k in BEAM_KS if V in (2 * k, 2 * k + 1)]


def _beam_rows(V, k):
    L = planted("beam", V)
    Kr = min(2 * k, V)
    j = torch.arange(V)
    low = -150.0 - (j % 32).float()
    rows, plant = {}, {}
    # Kr distinct top scores on J(V), the best on the highest index
    x = low.clone()
    order = L[::-1][:Kr]
    for i, t in enumerate(order):
        x[t] = 2.0 if i == 0 else -104.0 - i
    rows["distinct"], plant["distinct"] = x, order[:k]
    # a threshold tie: scores strictly above (three; one with two beams, where three would fill both running beams) on indices
    # outside J(V), then one value on up to nine planted indices
    free = [t for t in range(2, min(V, 40)) if t not in L][:min(3, k - 1)]
    above = free if free else [L[-1]]
    tied = [t for t in L if t not in above and t != beam_ref.EOS][:9]   # (an EOS candidate leaves the running beams)
    x = low.clone()
    for i, t in enumerate(above):
        x[t] = 2.0 if i == 0 else -103.0 - i
    x[tied] = -110.0
    rows["tie"], plant["tie"] = x, tied[:max(0, min(k - len(above), len(tied)))]
    # the maximum twice: two beams leave step 1 with one running score
    x = low.clone()
    x[L[0]] = x[L[-1]] = 2.0
    rows["twin"], plant["twin"] = x, sorted({L[0], L[-1]})
    # the mass on J(V): background <= -30, planted entries 0; a dropped element moves the lse by ln(n / (n - 1)) at least
    x = -30.0 - _grid(V)
    x[L] = 0.0
    rows["mass"], plant["mass"] = x, L[:k]
    return rows, plant, tied, low


def beam_case(V, k, dtype, items=BEAM_ITEMS):
    """two steps of len(items) batch items: step 1 (beam 0 alone is live, so its row's list decides the step) with one item per
    row kind, step 2 (every beam live, reached from step 1's state) with one row on every beam of an item: the twin item's two
    best beams then tie on every candidate and the lower beam * V + token wins.
    -> dict(steps [(B * k, V) in dtype, ..], planted {item: [j]} (the indices whose pick reaches the outputs), tied, bg {item: (V,)})"""
    rows, plant, tied, low = _beam_rows(V, k)
    step1 = torch.stack([rows[name] for name in items for _ in range(k)])
    step2 = torch.stack([rows[BEAM_STEP2[name]] for name in items for _ in range(k)])
    mass_bg = -30.0 - _grid(V)
    return dict(steps=[_exact(step1, dtype), _exact(step2, dtype)], planted=plant, tied=tied, k=k, V=V, items=tuple(items),
                bg={name: _exact(mass_bg if name == "mass" else low, dtype) for name in items})


def beam_expected(c, normalized, step1=None):
    """beam_ref's (tokens, state) after each step, from the start state (normalized: the rows taken as log-probabilities)"""
    k = c["k"]
    L = BEAM_MAX_LENGTH + 1
    st = beam_ref.init(len(c["items"]), k, L, L)
    out = []
    for s, x in enumerate(c["steps"], 1):
        x = step1 if (s == 1 and step1 is not None) else x
        if normalized:
            tok = proc_ref.beam_step_normalized(st, x, s, BEAM_MAX_LENGTH)
        else:
            tok, _ = beam_ref.step(st, x, s, BEAM_MAX_LENGTH)
        out.append((tok.clone(), {name: t.clone() for name, t in st.items()}))
    return out


# ------------------------------------------------------------------------------------------------------------------ the sampled verification
# a top-k and a top-p setting of spec_sample_ref.GRID.  Both keep few tokens: on a flat row of n kept tokens a draw lies within
# TOL * S of a prefix boundary with probability about 2 * TOL * n, a quarter at n = 32768, and such rows only count as ambiguous
SPEC_WARPERS = [(0.7, 50, 1.0), (2.0, 0, 0.05)]
SPEC_OLDS = (3, 10, 0, 5)


def spec_sample_case(V, dtype, gamma):
    """spec_sample_ref's grid generator at one size (three rows), every draft a planted index, and a fourth row whose first
    draft is rejected (u1 = 0.9 against P(d) < 0.2) and whose residual mass sits on one planted index"""
    L = planted("spec_sample", V)
    n, M = len(L), gamma + 1
    ln = R.inputs(dict(id=f"seam-V{V}-{str(dtype)[6:]}-g{gamma}", V=V, dtype=dtype, gamma=gamma, pad=0), near=gamma > 1)
    for b in range(3):
        for i in range(gamma):
            ln["draft"][b, i] = L[(b * gamma + i) % n]
    low = -30.0 - _grid(V)
    star, d = L[-1], L[0]
    p = low.clone()
    p[d] = -2.0
    p[star] = 0.0
    q = low.clone()
    q[d] = 0.0
    ln["logits"] = torch.cat([ln["logits"], _exact(p, dtype).expand(1, M, V)])
    ln["draft_logits"] = torch.cat([ln["draft_logits"], _exact(q, dtype).expand(1, gamma, V)])
    ln["draft"] = torch.cat([ln["draft"], torch.full((1, gamma), d, dtype=torch.long)])
    u = torch.tensor([0.25, 0.9, 0.5]).expand(1, M, 3)
    ln["uniforms"] = torch.cat([ln["uniforms"], u]).contiguous()
    lens = torch.tensor([o + M for o in SPEC_OLDS], dtype=torch.int32)
    g = torch.Generator().manual_seed(V + gamma)
    ln.update(cache_seqlens=lens, draft_seqlens=lens.clone(), labels=torch.randint(2, 100, (4, R.NCOLS), generator=g),
              tok=torch.randint(2, 100, (4,), generator=g), seen_eos=torch.zeros(4, dtype=torch.bool), star=star, d=d, bg=_exact(low, dtype))
    return ln
