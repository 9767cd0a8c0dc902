"""A plain-Python restatement of the draft-verification rule of speculative greedy decoding (include/fat5.h, fat5_spec_accept;
flasht5_amd/speculative.py), the mutants a test of it must tell from the truth, and the case list both test files use
(tests/test_speculative_cpu.py proves without a GPU that every mutant differs from the restatement on at least one of these
cases; tests/test_speculative_gpu.py compares the kernel with the restatement on the same cases, exactly: every output is an
integer).  CPU only; nothing here imports the package."""
import math
import zlib

import torch

EOS = 1

MUTANTS = (
    "n_off_by_one",         # one more draft accepted than agrees
    "eos_ignored",          # the candidates are not cut after the first EOS
    "limit_ignored",        # the candidates are not cut to the free columns
    "frozen_advanced",      # a row with seen_eos set on entry is treated as live
    "bonus_from_previous",  # the bonus token is a_{n-1} instead of a_n
    "draft_len_kept",       # draft_seqlens is not rolled back
    "tie_highest",          # the highest index among equal maxima
)


def argmax_row(x, highest=False):
    """the first NaN, else the first +inf, else the lowest (mutant: highest) index among equal maxima (-0 equals +0)"""
    x = x.float()
    nan = torch.isnan(x).nonzero()
    if len(nan):
        return int(nan[0])
    inf = (x == math.inf).nonzero()
    if len(inf):
        return int(inf[0])
    at = (x == x.max()).nonzero()
    return int(at[-1] if highest else at[0])


def accept_ref(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens=None, eos=EOS, mutant=None):
    """-> dict of NEW tensors: labels, tok, cache_seqlens, draft_seqlens (or None), seen_eos, n_accepted, n_new"""
    assert mutant is None or mutant in MUTANTS
    B, M, V = logits.shape
    gamma, ncols = M - 1, labels.shape[1]
    out = dict(labels=labels.clone(), tok=tok.clone(), cache_seqlens=cache_seqlens.clone(), seen_eos=seen_eos.clone(),
               draft_seqlens=None if draft_seqlens is None else draft_seqlens.clone(),
               n_accepted=torch.zeros(B, dtype=torch.int32), n_new=torch.zeros(B, dtype=torch.int32))
    for b in range(B):
        a = [argmax_row(logits[b, i], highest=mutant == "tie_highest") for i in range(M)]
        d = [int(t) for t in draft[b]]
        n = 0
        while n < gamma and a[n] == d[n]:
            n += 1
        if mutant == "n_off_by_one":
            n = min(n + 1, gamma)
        bonus = a[n - 1] if mutant == "bonus_from_previous" and n > 0 else a[n]
        cand = d[:n] + [bonus]
        if eos in cand and mutant != "eos_ignored":
            cand = cand[:cand.index(eos) + 1]
        old = int(cache_seqlens[b]) - M
        lim = min(int(limit[b]) if torch.is_tensor(limit) else int(limit), ncols - 1)
        room = lim - old if 0 <= old < lim else 0
        if mutant == "limit_ignored":
            room = len(cand) if old >= 0 else 0
        cand = cand[:room]
        frozen = bool(seen_eos[b]) and mutant != "frozen_advanced"
        if frozen:
            cand = []
        c = len(cand)
        for j, t in enumerate(cand):
            if old + 1 + j < ncols:   # (only the limit mutant can get here with a column outside)
                out["labels"][b, old + 1 + j] = t
        out["cache_seqlens"][b] = old + c
        if draft_seqlens is not None and mutant != "draft_len_kept":
            out["draft_seqlens"][b] = old + c
        if not frozen:
            if c:
                out["tok"][b] = cand[-1]
            if (c and cand[-1] == eos) or old < 0 or old + c >= lim:
                out["seen_eos"][b] = True
        out["n_accepted"][b] = min(n, c)
        out["n_new"][b] = c
    return out


OUTPUTS = ("labels", "tok", "cache_seqlens", "draft_seqlens", "seen_eos", "n_accepted", "n_new")


def same(x, y):
    """whether two results of accept_ref (or the kernel's outputs in the same dict) are equal in every tensor"""
    return all((x[k] is None and y[k] is None) or torch.equal(x[k], y[k]) for k in OUTPUTS)


# ------------------------------------------------------------------------------------------------------------------- the cases
NCOLS = 40
PEAK = 8.0   # the planted maximum; the noise under it is 0.25 * randn clipped to [-2, 2]
V_BIG = 32128 + 3


def _row(n, gamma, old=3, frozen=False, a=None, d=None, special=None):
    """a row whose target argmaxes `a` (drawn by inputs() when None) agree with the drafts on exactly the first n"""
    return dict(n=n, old=old, frozen=frozen, a=a, d=d, special=special)


def _build_cases():
    out = []

    def add(name, V, dtype, gamma, rows, limit=NCOLS - 1, pad=0):
        out.append(dict(id=f"{name}-V{V}-{str(dtype)[6:]}-g{gamma}", V=V, dtype=dtype, gamma=gamma, rows=rows, limit=limit, pad=pad))

    # B = 3 with n = 0, a middle value and gamma, at every V, dtype and gamma (V_BIG: a tail that is no multiple of the 16-byte width)
    for V in (1, 7, 512, V_BIG):
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            for gamma in (1, 4, 15):
                add("mixed", V, dtype, gamma, [_row(0, gamma, old=3), _row(gamma // 2, gamma, old=10), _row(gamma, gamma, old=0)])
    # row and batch strides that are not the contiguous ones (pad elements after every row, 3 rows of slack per batch element):
    # a multiple of 8 keeps the 16-byte path with a ragged tail, an odd one takes the element path
    for V, pad, dtype in ((V_BIG, 5, torch.bfloat16), (V_BIG, 5, torch.float32), (V_BIG, 5, torch.float16), (V_BIG, 2, torch.bfloat16),
                          (512, 8, torch.bfloat16), (7, 1, torch.float32)):
        add(f"stride{pad}", V, dtype, 4, [_row(1, 4), _row(4, 4, old=7), _row(2, 4, old=20)], pad=pad)
    g, V, bf = 4, 512, torch.bfloat16
    # exact ties: the maximum sits at two or three indices; the lowest is the argmax, and the draft names it
    add("ties", V, bf, g, [_row(g, g, special=dict(kind="tie", at=(0, 2, 4))), _row(2, g, special=dict(kind="tie", at=(2,))),
                           _row(0, g, special=dict(kind="tie", at=(0,)))])
    add("ties", V_BIG, torch.float32, g, [_row(g, g, special=dict(kind="tie", at=(1, 4))), _row(1, g), _row(0, g)])
    add("zeros", 7, torch.float16, g, [_row(g, g, special=dict(kind="zeros", at=(0, 1, 2, 3, 4))), _row(1, g), _row(0, g)])
    # a NaN row (with a +inf in front of it: the NaN wins) and a +inf row (two of them: the first wins)
    add("naninf", V, bf, g, [_row(g, g, special=dict(kind="nan", at=(1, 4))), _row(g, g, special=dict(kind="inf", at=(0, 3))),
                             _row(1, g, special=dict(kind="nan", at=(1,)))])
    add("naninf", V_BIG, torch.float16, g, [_row(2, g, special=dict(kind="nan", at=(2,))), _row(g, g, special=dict(kind="inf", at=(4,))),
                                            _row(0, g, special=dict(kind="inf", at=(0,)))])
    # EOS as the first, a middle and the bonus token (the drafts agree past it: what follows an EOS is cut)
    add("eos", V, bf, g, [_row(g, g, a=[EOS, 5, 6, 7, 8]), _row(g, g, a=[5, 6, EOS, 7, 8], old=9), _row(2, g, a=[5, 6, EOS, 7, 8], old=20)])
    add("eos-bonus-last", V, bf, g, [_row(g, g, a=[5, 6, 7, 8, EOS]), _row(0, g, a=[EOS, 6, 7, 8, 9]), _row(3, g, a=[5, EOS, 7, 8, 9])])
    # the limit reached in the middle of a round, exactly at its end, and one column before it
    add("limit", V, bf, g, [_row(g, g, old=36), _row(g, g, old=34), _row(g, g, old=33)])
    add("limit-rows", V, bf, g, [_row(g, g, old=3), _row(2, g, old=17), _row(0, g, old=29)], limit=[5, 20, 30])
    add("limit-eos", V, bf, g, [_row(g, g, old=37, a=[5, EOS, 7, 8, 9]), _row(g, g, old=38, a=[EOS, 6, 7, 8, 9]), _row(1, g, old=37)])
    # a frozen row between two live ones; a frozen row that would have accepted everything
    add("frozen", V, bf, g, [_row(2, g), _row(g, g, old=12, frozen=True), _row(g, g, old=30)])
    # a draft id equal to V (and one below 0) where the target's choice would otherwise be met
    add("draft-oob", V, bf, g, [_row(g, g, d={0: V}), _row(g, g, d={2: -1}, old=8), _row(g, g, d={4 - 1: V + 7}, old=1)])
    add("draft-oob", 1, torch.float32, g, [_row(g, g, d={0: 1}), _row(g, g, d={2: 1}, old=8), _row(g, g, old=1)])
    # lengths and limits that make no sense: nothing is written, the lengths are restored, the row is marked done
    add("garbage", V, bf, g, [_row(g, g, old=-9), _row(g, g, old=NCOLS + 100), _row(g, g, old=5)], limit=[39, 39, 10 ** 6])
    add("garbage-limit", V, bf, g, [_row(g, g, old=38), _row(g, g, old=39), _row(g, g, old=0)], limit=[-3, 10 ** 6, 0])
    return out


CASES = _build_cases()


def inputs(case):
    """the call of `case` as CPU tensors: logits (B, M, V) in the case's dtype, draft, cache_seqlens (advanced by M), labels,
    tok, seen_eos, limit (an int or a (B,) int32 tensor) and draft_seqlens"""
    g = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    V, gamma, rows = case["V"], case["gamma"], case["rows"]
    B, M = len(rows), gamma + 1
    logits = (0.25 * torch.randn(B, M, V, generator=g)).clamp(-2, 2)
    draft = torch.zeros(B, gamma, dtype=torch.long)
    lens = torch.zeros(B, dtype=torch.int32)
    labels = torch.randint(2, 100, (B, NCOLS), generator=g)   # (what a wrong write would overwrite is never 0)
    tok = torch.randint(2, 100, (B,), generator=g)
    seen = torch.zeros(B, dtype=torch.bool)
    for b, r in enumerate(rows):
        a = r["a"]
        if a is None:   # distinct from EOS wherever the vocabulary allows it
            a = [int(t) for t in torch.randint(2, V, (M,), generator=g)] if V > 2 else [0] * M
        sp = r["special"] or {}
        for i in range(M):
            logits[b, i, a[i]] = PEAK
            if i in sp.get("at", ()):
                if sp["kind"] == "tie":      # the same value again at higher indices
                    for j in {min(V - 1, a[i] + 1), V - 1}:
                        logits[b, i, j] = PEAK
                elif sp["kind"] == "zeros":  # a row of zeros of both signs: index 0
                    logits[b, i] = 0.0
                    logits[b, i, 0::2] = -0.0
                    a[i] = 0
                elif sp["kind"] == "nan":    # a +inf in front of the first NaN, a second NaN behind it
                    j = V // 2
                    logits[b, i, j], logits[b, i, 0], logits[b, i, V - 1] = math.nan, math.inf, math.nan
                    a[i] = j
                elif sp["kind"] == "inf":    # two +inf above the planted peak
                    j = V // 3
                    logits[b, i, j], logits[b, i, V - 1] = math.inf, math.inf
                    a[i] = j
        n = r["n"]
        for i in range(gamma):
            draft[b, i] = a[i]
        if n < gamma:
            draft[b, n] = (a[n] + 1) % V if V > 1 else V   # (V = 1: the only id that differs lies outside the vocabulary)
        for i, t in (r["d"] or {}).items():
            draft[b, i] = t
        lens[b] = r["old"] + M
        seen[b] = r["frozen"]
    limit = case["limit"]
    if isinstance(limit, list):
        limit = torch.tensor([max(-2 ** 31, min(2 ** 31 - 1, v)) for v in limit], dtype=torch.int32)
    return dict(logits=logits.to(case["dtype"]), draft=draft, cache_seqlens=lens, labels=labels, tok=tok, seen_eos=seen, limit=limit,
                draft_seqlens=lens.clone())


def reference(case, ln, mutant=None):
    return accept_ref(ln["logits"], ln["draft"], ln["cache_seqlens"], ln["labels"], ln["tok"], ln["seen_eos"], ln["limit"],
                      ln["draft_seqlens"], EOS, mutant)
