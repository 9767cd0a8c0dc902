"""An fp64 restatement of the verification rule of speculative sampling (include/fat5.h, fat5_spec_accept_sampled;
flasht5_amd/speculative.py), the mutants a test of it must tell from the truth, and the case list both test files use
(tests/test_spec_sample_cpu.py proves without a GPU that every mutant differs from the restatement on at least one of these
cases; tests/test_spec_sample_gpu.py compares the kernels with the restatement on the same cases).  The distributions come from
sampling_ref.restate, the plain draw from sampling_ref.draw, the uniforms from sampling_ref.philox4x32_10 and the bookkeeping
from spec_ref.accept_ref.  CPU only; nothing here imports the package.

    P_i = warped distribution of logits[b, i], Q_i of draft_logits[b, i] (one-hot at d_i without draft_logits); a degenerate
          row is one-hot at torch.argmax's index
    (u0, u1, u2) of chunk row i: words 0, 1, 2 of Philox(key = seed, counter = (offset + old + 1 + i, b, 0)), (w >> 8) * 2^-24
    draft i is accepted iff all before it were, 0 <= d_i < V and u1 * Q_i(d_i) < P_i(d_i)
    after n = gamma accepted drafts: the plain draw from P_gamma with u0; otherwise the residual draw with u2 over
          r_j = floor(max(0, P_n(j) - Q_n(j)) * 2^40), and over P_n when their sum is 0"""
import math
import zlib

import numpy as np
import torch

import sampling_ref as S
import spec_ref as G

EOS = G.EOS
ONE = 1 << 40
DRAFT_KEY = 0x9E3779B97F4A7C15

MUTANTS = (
    "accept_u_from_w0",     # the acceptance uniform is u0
    "counter_i",            # the counter is offset + i instead of offset + old + 1 + i
    "counter_old_plus_i",   # the counter is offset + old + i
    "row_word_bM_plus_i",   # the Philox row word is b * M + i instead of b
    "residual_unclipped",   # the residual is P - Q, not clipped at 0 (the scan runs over signed values)
    "residual_from_p",      # after a rejection the token is drawn from P_n
    "bonus_u2",             # the token after gamma accepted drafts is drawn with u2
    "q_zero_rejects",       # a draft with Q(d) = 0 is rejected whatever P(d)
    "draft_oob_accepted",   # a draft outside [0, V) counts as accepted
    "no_r0_fallback",       # with no residual mass the token is index 0 instead of a draw from P_n
)


# ------------------------------------------------------------------------------------------------------------ the distributions
def dist(row, temperature, top_k, top_p):
    """the warped distribution of one logits row (a torch tensor of any float dtype): dict(p (fp64, sums to 1), r (the restated
    row, None when degenerate), margin (of the top-p decision, relative to S))"""
    x = S.scaled(row, temperature)
    if np.isnan(x).any() or (x == np.inf).any() or (x == -np.inf).all():
        p = np.zeros(x.shape[0])
        p[S.argmax_rule(x)] = 1.0
        return dict(p=p, r=None, margin=math.inf)
    r = S.restate(x, top_k, top_p)
    return dict(p=r["e"] / r["e"].sum(), r=r, margin=r["margin"])


def one_hot(V, d):
    q = np.zeros(V)
    if 0 <= d < V:
        q[d] = 1.0
    return dict(p=q, r=None, margin=math.inf)


def uniforms(seed, counter, row):
    """(u0, u1, u2) of one Philox block (exact: 24-bit integers times 2^-24)"""
    ctr = int(counter) & 0xFFFFFFFFFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = S.philox4x32_10((ctr & S.MASK, ctr >> 32, int(row) & S.MASK, 0), (seed & S.MASK, seed >> 32))
    return tuple((v >> 8) * 2.0 ** -24 for v in w[:3])


def round_uniforms(seed, offset, old, b, M, mutant=None):
    """the (M, 3) uniforms of batch row b whose length before the chunk was `old`"""
    out = []
    for i in range(M):
        ctr = offset + old + 1 + i
        if mutant == "counter_i":
            ctr = offset + i
        elif mutant == "counter_old_plus_i":
            ctr = offset + old + i
        out.append(uniforms(seed, ctr, b * M + i if mutant == "row_word_bM_plus_i" else b))
    return out


# ------------------------------------------------------------------------------------------------------------------ the draws
def _target(u, total):
    t = math.floor(u * total) if u >= 0 else 0   # (u NaN or negative: 0, as in the sampler)
    return min(t, total - 1)


def plain_draw(P, u, tol=0.0):
    """the sampler's inverse-CDF token(s) from a distribution of dist(): sampling_ref.draw, or the one-hot index"""
    if P["r"] is None:
        return {int(np.argmax(P["p"]))}
    return S.draw(P["r"], u, tol)


def residual(P, Q, mutant=None):
    """r_j as Python-exact integers (int64 array; signed only under the unclipped mutant)"""
    diff = P["p"] - Q["p"]
    if mutant != "residual_unclipped":
        diff = np.maximum(diff, 0.0)
    return np.trunc(diff * float(ONE)).astype(np.int64)


def residual_draw(P, Q, u, tol=0.0, mutant=None):
    """the token(s) of the residual draw: the first j whose inclusive prefix of r exceeds min(floor(u R), R - 1); with tol > 0
    every j with r_j > 0 whose prefix interval lies within tol (in units of probability: tol * 2^40) of the target -- the r_j
    are differences of two distributions that each carry the sampler's relative error, so their prefixes carry an absolute
    one.  R = 0: the draw from P"""
    if mutant == "residual_from_p":
        return plain_draw(P, u, tol)
    r = residual(P, Q, mutant)
    R = int(np.maximum(r, 0).sum())
    if R == 0:
        return {0} if mutant == "no_r0_fallback" else plain_draw(P, u, tol)
    pre = np.cumsum(r)
    t = _target(u, R)
    if tol == 0.0:
        return {int(np.argmax(pre > t))}
    ok = (r > 0) & (pre - r <= t + tol * ONE) & (pre > t - tol * ONE)
    return set(np.nonzero(ok)[0].tolist())


def accept_margin(P, Q, d, u1):
    """P(d) - u1 * Q(d): the draft is accepted iff this is > 0"""
    return float(P["p"][d]) - u1 * float(Q["p"][d])


# ---------------------------------------------------------------------------------------------------------------- one batch row
def verify_row(dists_p, dists_q, d, u, V, mutant=None):
    """dists_p(i), dists_q(i): callables giving the distributions of chunk row i (dists_q None: one-hot drafts); d: the gamma
    drafts; u: (M, 3).  -> (n, token, sampled (M,) list)"""
    gamma = len(d)
    n = 0
    while n < gamma:
        di = int(d[n])
        if not 0 <= di < V:
            if mutant == "draft_oob_accepted":
                n += 1
                continue
            break
        P = dists_p(n)
        Q = dists_q(n) if dists_q is not None else one_hot(V, di)
        u1 = u[n][0] if mutant == "accept_u_from_w0" else u[n][1]
        if mutant == "q_zero_rejects" and Q["p"][di] == 0.0:
            break
        if not accept_margin(P, Q, di, u1) > 0:
            break
        n += 1
    P = dists_p(n)
    if n == gamma:
        token = min(plain_draw(P, u[n][2] if mutant == "bonus_u2" else u[n][0]))
    else:
        Q = dists_q(n) if dists_q is not None else one_hot(V, int(d[n]))
        token = min(residual_draw(P, Q, u[n][2], 0.0, mutant))
    return n, token, [int(t) for t in d[:n]] + [token] + [-1] * (gamma - n)


def bookkeep(rows, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens=None, eos=EOS, V=2):
    """spec_ref.accept_ref's bookkeeping for given per-row results: rows[b] = (n, token).  accept_ref derives n from argmaxes, so
    it is fed one-hot rows whose argmaxes are the candidates, and a draft that differs from the token at position n.  (A draft
    id outside [0, V) among the accepted ones -- the mutant alone -- is shown to it as 0.)"""
    B, gamma = draft.shape
    Vf = max([V, 2] + [t + 1 for _, t in rows])
    fake = torch.zeros(B, gamma + 1, Vf)
    d2 = draft.clone()
    for b, (n, t) in enumerate(rows):
        for i in range(n):
            if not 0 <= int(d2[b, i]) < Vf:
                d2[b, i] = 0
            fake[b, i, int(d2[b, i])] = 1.0
        fake[b, n, t] = 1.0
        if n < gamma:
            d2[b, n] = (t + 1) % Vf
    out = G.accept_ref(fake, d2, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens, eos)
    return out


def rows_from_sampled(sampled, seen_eos):
    """(n, token) per batch row from the kernel's `sampled` (B, M): frozen rows (all -1) count as (0, 0)"""
    out = []
    for b in range(sampled.shape[0]):
        s = [int(t) for t in sampled[b]]
        if bool(seen_eos[b]):
            assert all(t == -1 for t in s), s
            out.append((0, 0))
            continue
        n = s.index(-1) - 1 if -1 in s else len(s) - 1
        assert n >= 0 and all(t == -1 for t in s[n + 1:]), s
        out.append((n, s[n]))
    return out


def accept_sampled_ref(logits, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens=None, eos=EOS, *, sampling,
                       draft_logits=None, uniforms=None, mutant=None):
    """the whole call -> spec_ref.accept_ref's dict of NEW tensors, with `sampled` (B, M) int64 and `n` (B,) beside them"""
    assert mutant is None or mutant in MUTANTS
    temperature, top_k, top_p, seed = sampling[:4]
    offset = sampling[4] if len(sampling) > 4 else 0
    B, M, V = logits.shape
    rows, sampled = [], torch.full((B, M), -1, dtype=torch.int64)
    for b in range(B):
        if bool(seen_eos[b]):
            rows.append((0, 0))
            continue
        old = int(cache_seqlens[b]) - M
        u = uniforms[b].tolist() if uniforms is not None else round_uniforms(seed, offset, old, b, M, mutant)
        cp, cq = {}, {}

        def dp(i, b=b, c=cp):
            if i not in c:
                c[i] = dist(logits[b, i], temperature, top_k, top_p)
            return c[i]

        def dq(i, b=b, c=cq):
            if i not in c:
                c[i] = dist(draft_logits[b, i], temperature, top_k, top_p)
            return c[i]
        n, t, s = verify_row(dp, dq if draft_logits is not None else None, draft[b].tolist(), u, V, mutant)
        rows.append((n, t))
        sampled[b] = torch.tensor(s)
    out = bookkeep(rows, draft, cache_seqlens, labels, tok, seen_eos, limit, draft_seqlens, eos, V)
    out["sampled"] = sampled
    out["n"] = torch.tensor([n for n, _ in rows], dtype=torch.int32)
    return out


OUTPUTS = G.OUTPUTS + ("sampled",)


def same(x, y):
    return all((x[k] is None and y[k] is None) or torch.equal(x[k], y[k]) for k in OUTPUTS)


# ------------------------------------------------------------------------------------------------------------------- the cases
NCOLS = G.NCOLS
V_TAIL = 32128 + 3     # a tail that is no multiple of the 16-byte width
V_LONG = 32768 + 11    # just past the register-resident limit
GRID = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.5, 50, 0.9), (1.0, 1, 1.0), (2.0, 0, 0.05)]   # the sampler tests' warpers
SEED, OFFSET = 0x1234567890ABCDEF, 5
OLDS = (3, 10, 0)


def _build_cases():
    out = []
    for V in (1, 7, 512, V_TAIL, V_LONG):
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            for gamma in (1, 4, 15):
                out.append(dict(id=f"grid-V{V}-{str(dtype)[6:]}-g{gamma}", V=V, dtype=dtype, gamma=gamma, pad=0))
    # padded row and batch strides, as spec_ref's stride cases: a multiple of 8 keeps the 16-byte path, an odd one leaves it
    for V, pad, dtype in ((V_TAIL, 5, torch.bfloat16), (V_TAIL, 5, torch.float32), (V_TAIL, 5, torch.float16), (V_TAIL, 2, torch.bfloat16),
                          (V_LONG, 5, torch.bfloat16), (512, 8, torch.bfloat16), (7, 1, torch.float32)):
        out.append(dict(id=f"stride{pad}-V{V}-{str(dtype)[6:]}-g4", V=V, dtype=dtype, gamma=4, pad=pad))
    return out


CASES = _build_cases()
SMALL_CASES = [c for c in CASES if c["V"] <= 512]   # what the CPU test restates in full


def inputs(case, near=False):
    """the call of `case` as CPU tensors (B = 3): logits (B, M, V) and draft_logits (B, gamma, V) = randn * 2.5 in the case's
    dtype (near: the drafter's rows are the target's plus randn * 0.3), drafts drawn from the drafter's rows by argmax of
    logits + Gumbel noise, lengths (advanced by M), labels, tok, seen_eos, limit, draft_seqlens and hook uniforms (B, M, 3)"""
    g = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    V, gamma = case["V"], case["gamma"]
    B, M = 3, gamma + 1
    logits = (torch.randn(B, M, V, generator=g) * 2.5).to(case["dtype"])
    if near:
        dl = (logits[:, :gamma].float() + 0.3 * torch.randn(B, gamma, V, generator=g)).to(case["dtype"])
    else:
        dl = (torch.randn(B, gamma, V, generator=g) * 2.5).to(case["dtype"])
    gum = -torch.log(-torch.log(torch.rand(B, gamma, V, generator=g).clamp_min(1e-20)))
    draft = (dl.float() + gum).argmax(-1)
    lens = torch.tensor([o + M for o in OLDS], dtype=torch.int32)
    labels = torch.randint(2, 100, (B, NCOLS), generator=g)
    tok = torch.randint(2, 100, (B,), generator=g)
    return dict(logits=logits, draft_logits=dl, draft=draft, cache_seqlens=lens, labels=labels, tok=tok,
                seen_eos=torch.zeros(B, dtype=torch.bool), limit=NCOLS - 1, draft_seqlens=lens.clone(),
                uniforms=torch.rand(B, M, 3, generator=g))


def hand_cases():
    """small hand-made calls (V = 12, fp32) that the random grid cannot be relied on to produce: forced decisions through the
    uniforms hook.  -> list of (id, kwargs for accept_sampled_ref)"""
    V, gamma = 12, 3
    M = gamma + 1
    g = torch.Generator().manual_seed(99)
    logits = torch.randn(2, M, V, generator=g) * 2.0
    base = dict(cache_seqlens=torch.tensor([3 + M, 9 + M], dtype=torch.int32), labels=torch.randint(2, 100, (2, NCOLS), generator=g),
                tok=torch.randint(2, 100, (2,), generator=g), seen_eos=torch.zeros(2, dtype=torch.bool), limit=NCOLS - 1,
                draft_seqlens=torch.tensor([3 + M, 9 + M], dtype=torch.int32))
    am = logits.argmax(-1)
    out = []
    # P = Q bitwise and the rejection forced by u1 = 1: no residual mass, the fallback draws from P_n
    u = torch.rand(2, M, 3, generator=g)
    u[:, 0, 1] = 1.0
    out.append(("r0-fallback", dict(base, logits=logits, draft=am[:, :gamma].clone(), draft_logits=logits[:, :gamma].clone(),
                                    sampling=(1.0, 0, 1.0, 7), uniforms=u)))
    # a draft outside the drafter's kept set (top_k = 2 of a drafter that prefers other tokens) but inside the target's: Q = 0 < P
    dl = logits[:, :gamma].clone()
    dl[torch.arange(2)[:, None], torch.arange(gamma)[None, :], am[:, :gamma]] = -30.0
    u = torch.tensor([0.1, 0.999, 0.9]).expand(2, M, 3).contiguous()   # (all accepted: the bonus is drawn with u0, far from u2)
    out.append(("q-zero", dict(base, logits=logits, draft=am[:, :gamma].clone(), draft_logits=dl, sampling=(1.0, 2, 1.0, 7),
                               uniforms=u)))
    # draft ids V and -1 where everything else would be accepted (u1 = 0)
    d = am[:, :gamma].clone()
    d[0, 1], d[1, 0] = V, -1
    out.append(("draft-oob", dict(base, logits=logits, draft=d, draft_logits=None, sampling=(1.0, 0, 1.0, 7),
                                  uniforms=torch.zeros(2, M, 3))))
    # Philox: rows at different lengths, with and without the drafter's logits (several seeds: some accept, some reject)
    for seed in (1, 2, 3):
        for with_q in (True, False):
            dq = (logits[:, :gamma] + 0.5 * torch.randn(2, gamma, V, generator=g)) if with_q else None
            out.append((f"philox-s{seed}-{'q' if with_q else 'onehot'}",
                        dict(base, logits=logits, draft=am[:, :gamma].clone(), draft_logits=dq, sampling=(1.0, 9, 0.95, seed, 11))))
    return out
