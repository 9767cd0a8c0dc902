"""Speculative sampling on the GPU: the verification kernels (csrc/spec_sample_kernels.h through `speculative_accept(...,
sampling=...)`) against the fp64 restatement of tests/spec_sample_ref.py on its case list, the edge cases through the uniforms
hook (exact), the law of the first emitted token (chi-square, acceptance rate), one captured round replayed while the lengths
grow, and the model level: a loop driven through the public pieces and restated round by round from its own logits,
`generate(do_sample=True, assistant_model=... / prompt_lookup_num_tokens=...)` bitwise against that loop and against its
graph=True run, top_k = 1 against plain greedy, the acceptance of a model drafting for itself, and the other modes.

Tolerance (the sampler tests' TOL, for their reason: the kernel's e_j are fp32 __expf values, its sums exact): a row whose
top-p threshold lies within TOL * S of a cumulative mass is ambiguous and skipped; an acceptance decision is checked up to TOL
in u1 * Q(d) - P(d) (a draft outside the target's kept set is rejected exactly); a drawn token may be either neighbour of a boundary within TOL of the target.  At most a quarter of the
checked rows may be ambiguous (skipped, decided within TOL, or with more than one admissible token).

The `[spec-sample] ...` lines are what DESIGN 4.19 records."""
import math

import numpy as np
import pytest
import torch

import spec_ref as G
import spec_sample_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 3
TOL = 4e-6  # (__expf: exp2 of a rounded product, a few fp32 ulps of e_j; the sums themselves are exact)
STATE = ("labels", "tok", "cache_seqlens", "draft_seqlens", "seen_eos")


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _padded(x, pad, fill=50.0):
    """a (B, rows, V) tensor on the device inside a buffer with `pad` elements after every row and three rows of slack per batch
    element (large values: reading the slack shows)"""
    B, rows, V = x.shape
    buf = torch.full((B, rows + 3, V + pad), fill, dtype=x.dtype, device=DEV)
    view = buf[:, :rows, :V]
    view.copy_(x)
    return view


def _device_call(ln, pad=0, draft=None, with_q=True):
    lab_buf = torch.full((ln["labels"].shape[0], ln["labels"].shape[1] + 2 * GUARD), -7, dtype=torch.long, device=DEV)
    labels = lab_buf[:, GUARD:-GUARD]
    labels.copy_(ln["labels"])
    lim = ln["limit"].to(DEV) if torch.is_tensor(ln["limit"]) else ln["limit"]
    t = dict(logits=_padded(ln["logits"], pad), draft=(ln["draft"] if draft is None else draft).to(DEV),
             cache_seqlens=ln["cache_seqlens"].to(DEV), labels=labels, tok=ln["tok"].to(DEV), seen_eos=ln["seen_eos"].to(DEV), limit=lim,
             draft_seqlens=None if ln.get("draft_seqlens") is None else ln["draft_seqlens"].to(DEV),
             draft_logits=_padded(ln["draft_logits"], pad) if with_q and ln.get("draft_logits") is not None else None)
    return t, lab_buf


def _run(ln, sampling, pad=0, draft=None, with_q=True, uniforms=None):
    from flasht5_amd import speculative_accept
    t, lab_buf = _device_call(ln, pad, draft, with_q)
    na, nn, sampled, aux = speculative_accept(
        t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"], draft_seqlens=t["draft_seqlens"],
        eos_token_id=R.EOS, sampling=sampling, draft_logits=t["draft_logits"], uniforms=None if uniforms is None else uniforms.to(DEV),
        return_sampled=True, return_aux=True)
    torch.cuda.synchronize()
    got = {k: (None if t[k] is None else t[k].cpu()) for k in STATE}
    got.update(n_accepted=na.cpu(), n_new=nn.cpu(), sampled=sampled.cpu(), aux=aux.cpu(), draft=t["draft"].cpu())
    guards = lab_buf.cpu()
    assert bool((guards[:, :GUARD] == -7).all()) and bool((guards[:, -GUARD:] == -7).all()), "guard columns"
    return got


def _bookkeeping_is_exact(ln, got, V):
    """labels, tok, both lengths, seen_eos and both counters equal spec_ref.accept_ref fed the kernel's own per-row tokens"""
    rows = R.rows_from_sampled(got["sampled"], ln["seen_eos"])
    want = R.bookkeep(rows, got["draft"], ln["cache_seqlens"], ln["labels"], ln["tok"], ln["seen_eos"], ln["limit"],
                      ln.get("draft_seqlens"), R.EOS, V)
    for k in G.OUTPUTS:
        assert (want[k] is None and got[k] is None) or torch.equal(got[k], want[k]), (k, got[k], want[k])
    return rows


class _Tally:
    def __init__(self):
        self.rows = self.ambiguous = 0


def _check_row(tally, dp, dq, d, u, sampled_row, V):
    """one batch row of one call against the restatement: dp(i) / dq(i) restate chunk row i (dq None: one-hot drafts), u (M, 3)
    the uniforms the kernel used, sampled_row its per-row tokens"""
    gamma = len(d)
    s = [int(t) for t in sampled_row]
    n = s.index(-1) - 1 if -1 in s else gamma
    tally.rows += 1
    doubtful = False
    for i in range(n + 1):
        P = dp(i)
        Q = None
        if i < gamma:   # (a draft id outside the vocabulary: the all-zero one-hot, or the drafter's row as it is)
            Q = dq(i) if dq is not None else R.one_hot(V, d[i])
        if P["margin"] < TOL or (Q is not None and Q["margin"] < TOL):
            tally.ambiguous += 1     # a top-p decision within rounding: nothing behind it can be held to the restatement
            return
        in_range = i < gamma and 0 <= d[i] < V
        if i < n:        # the kernel accepted draft i
            assert s[i] == d[i] and in_range, (i, s, d)
            m = R.accept_margin(P, Q, d[i], u[i][1])
            assert m > -TOL, (i, m)
            doubtful |= abs(m) <= TOL and P["p"][d[i]] > 0   # (P(d) = 0 is a fact of the kept set, not of rounding)
        elif n < gamma:  # the kernel rejected draft n and drew from the residual
            if in_range:
                m = R.accept_margin(P, Q, d[i], u[i][1])
                assert m < TOL, (i, m)
                doubtful |= abs(m) <= TOL and P["p"][d[i]] > 0   # (P(d) = 0 is a fact of the kept set, not of rounding)
            ok = R.residual_draw(P, Q, u[i][2], TOL)
            assert s[i] in ok, (i, s[i], sorted(ok)[:8])
            doubtful |= len(ok) > 1
        else:            # every draft accepted: the plain draw with u0
            ok = R.plain_draw(P, u[i][0], TOL)
            assert s[i] in ok, (i, s[i], sorted(ok)[:8])
            doubtful |= len(ok) > 1
        assert 0 <= s[i] < V and P["p"][s[i]] > 0, (i, s)   # whatever is emitted is a token the target keeps
    tally.ambiguous += bool(doubtful)


@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_kernel_against_the_restatement(case):
    V, gamma, M = case["V"], case["gamma"], case["gamma"] + 1
    ln = R.inputs(case, near=gamma > 1)
    tally = _Tally()
    for T, k, p in R.GRID:
        sampling = (T, k, p, R.SEED + k, R.OFFSET)
        cache = {}

        def dist_of(name, b, i, cache=cache, T=T, k=k, p=p):
            if (name, b, i) not in cache:
                cache[name, b, i] = R.dist(ln[name][b, i], T, k, p)
            return cache[name, b, i]
        for with_q in (True, False):
            for hook in (False, True):
                got = _run(ln, sampling, case["pad"], with_q=with_q, uniforms=ln["uniforms"] if hook else None)
                # every uniform is the Python Philox value, bitwise (or the hook's)
                for b in range(3):
                    want_u = ln["uniforms"][b].tolist() if hook else R.round_uniforms(sampling[3], R.OFFSET, R.OLDS[b], b, M)
                    assert got["aux"][b].tolist() == [list(w) for w in want_u], (b, hook)
                    _check_row(tally, lambda i, b=b: dist_of("logits", b, i), (lambda i, b=b: dist_of("draft_logits", b, i)) if with_q else None,
                               ln["draft"][b].tolist(), got["aux"][b].tolist(), got["sampled"][b], V)
                _bookkeeping_is_exact(ln, got, V)
            # the second call: drafts built from the first call's tokens, and the hook's u1 forcing exactly n = 0, gamma // 2 and
            # gamma accepted drafts per row (0 accepts whatever P(d) > 0, +inf rejects): that pins the bookkeeping
            want_n = [0, gamma // 2, gamma]
            d2 = ln["logits"][:, :gamma].float().argmax(-1)
            d2 = torch.where(got["sampled"][:, :gamma] >= 0, got["sampled"][:, :gamma], d2)
            u2 = ln["uniforms"].clone()
            for b, n in enumerate(want_n):
                u2[b, :n, 1] = 0.0
                u2[b, n:, 1] = math.inf
            got2 = _run(ln, sampling, case["pad"], draft=d2, with_q=with_q, uniforms=u2)
            rows = _bookkeeping_is_exact(ln, got2, V)
            assert [n for n, _ in rows] == want_n, (rows, want_n)
    print(f"[spec-sample] {case['id']}: {tally.rows} rows checked, {tally.ambiguous} ambiguous")
    assert tally.ambiguous * 4 <= tally.rows, (tally.ambiguous, tally.rows)


# ------------------------------------------------------------------------------------------------------------------ edge cases
EV, EG = 16, 4   # the edge cases' vocabulary and gamma


def _edge_base(seed=0, B=3):
    g = torch.Generator().manual_seed(seed)
    M = EG + 1
    lens = torch.tensor([3, 10, 0][:B], dtype=torch.int32) + M
    logits, dl = torch.randn(B, M, EV, generator=g) * 2.0, torch.randn(B, EG, EV, generator=g) * 2.0
    # EOS is drawn only where a case plants it: a mass of about 1e-7, yet above the 2^-40 below which a fixed-point mass is 0
    logits[..., R.EOS] = dl[..., R.EOS] = -12.0
    return dict(logits=logits, draft_logits=dl,
                draft=torch.randint(2, EV, (B, EG), generator=g), cache_seqlens=lens, labels=torch.randint(2, 100, (B, R.NCOLS), generator=g),
                tok=torch.randint(2, 100, (B,), generator=g), seen_eos=torch.zeros(B, dtype=torch.bool), limit=R.NCOLS - 1,
                draft_seqlens=lens.clone(), uniforms=torch.rand(B, M, 3, generator=g))


def _forced(u, ns):
    """the hook's u1 set so that exactly ns[b] drafts are accepted (where P(d) > 0): 0 accepts, +inf rejects"""
    u = u.clone()
    for b, n in enumerate(ns):
        u[b, :n, 1] = 0.0
        u[b, n:, 1] = math.inf
    return u


def _exact(ln, sampling=(1.0, 0, 1.0, 3), with_q=True, uniforms=None):
    """the kernel equals the restatement in every output, exactly (the hook's uniforms keep every decision away from rounding)"""
    u = ln["uniforms"] if uniforms is None else uniforms
    got = _run(ln, sampling, with_q=with_q, uniforms=u)
    want = R.accept_sampled_ref(ln["logits"], ln["draft"], ln["cache_seqlens"], ln["labels"], ln["tok"], ln["seen_eos"], ln["limit"],
                                ln.get("draft_seqlens"), R.EOS, sampling=sampling, draft_logits=ln["draft_logits"] if with_q else None,
                                uniforms=u)
    for k in R.OUTPUTS:
        assert (want[k] is None and got[k] is None) or torch.equal(got[k], want[k]), (k, got[k], want[k])
    return got


def test_edge_eos_as_an_accepted_draft_as_the_residual_token_and_as_the_bonus():
    ln = _edge_base(1)
    ln["draft"][0, 1] = R.EOS                 # row 0: EOS is the second of four accepted drafts
    ln["logits"][1, 2, R.EOS] = 40.0          # row 1: two accepted, the third rejected, the residual is all but EOS-only
    ln["draft"][1, 2] = 5
    ln["logits"][2, EG, R.EOS] = 40.0         # row 2: everything accepted, the bonus is EOS
    ln["draft"][2] = torch.tensor([4, 5, 6, 7])
    got = _exact(ln, uniforms=_forced(ln["uniforms"], [4, 2, 4]))
    assert got["n_new"].tolist() == [2, 3, 5] and got["seen_eos"].tolist() == [True, True, True]
    assert got["sampled"][1, 2] == R.EOS and got["sampled"][2, EG] == R.EOS and got["n_accepted"].tolist() == [2, 2, 4]


def test_edge_limit_frozen_and_garbage():
    ln = _edge_base(2)
    ln["cache_seqlens"] = torch.tensor([36, 12, 30], dtype=torch.int32) + EG + 1
    ln["draft_seqlens"] = ln["cache_seqlens"].clone()
    ln["seen_eos"][1] = True                  # a frozen row between two live ones
    got = _exact(ln, uniforms=_forced(ln["uniforms"], [4, 4, 1]))   # row 0: the limit in mid-round (three columns left)
    assert got["n_new"].tolist() == [3, 0, 2] and got["cache_seqlens"].tolist() == [39, 12, 32] and got["sampled"][1].tolist() == [-1] * 5
    assert got["seen_eos"].tolist() == [True, True, False]
    for lens, limit in (([-9, R.NCOLS + 100, 5], [39, 39, 10 ** 6]), ([38, 39, 0], [-3, 10 ** 6, 0])):
        ln = _edge_base(3)
        ln["cache_seqlens"] = torch.tensor(lens, dtype=torch.int32) + EG + 1
        ln["draft_seqlens"] = ln["cache_seqlens"].clone()
        ln["limit"] = torch.tensor(limit, dtype=torch.int32)
        _exact(ln, uniforms=_forced(ln["uniforms"], [4, 4, 4]))
        _exact(ln, with_q=False, sampling=(0.8, 5, 0.9, 11))


def test_edge_draft_ids_outside_the_vocabulary():
    ln = _edge_base(4)
    ln["draft"][0, 1], ln["draft"][1, 0], ln["draft"][2, 3] = EV, -1, EV + 7
    for with_q in (True, False):
        got = _exact(ln, with_q=with_q, uniforms=_forced(ln["uniforms"], [4, 4, 4]))
        assert [n for n, _ in R.rows_from_sampled(got["sampled"], ln["seen_eos"])] == [1, 0, 3]
        assert bool((got["sampled"] < EV).all())


def test_edge_drafts_outside_a_kept_set():
    ln = _edge_base(5)
    order = ln["logits"].argsort(-1, descending=True)
    # outside the target's kept set (top_k = 3: its fifth choice): rejected even with u1 = 0, and never emitted
    ln["draft"][0] = order[0, :EG, 4]
    # outside the drafter's kept set but inside the target's (the target's first choice, which the drafter puts last): accepted
    # even with u1 just below 1
    ln["draft"][1] = order[1, :EG, 0]
    ln["draft_logits"][1, torch.arange(EG), ln["draft"][1]] = -30.0
    ln["draft"][2] = order[2, :EG, 0]
    u = ln["uniforms"].clone()
    u[0, :, 1] = 0.0
    u[1, :, 1] = 1.0 - 2.0 ** -24
    u[2, :, 1] = 0.0
    got = _exact(ln, sampling=(1.0, 3, 1.0, 3), uniforms=u)
    assert [n for n, _ in R.rows_from_sampled(got["sampled"], ln["seen_eos"])] == [0, 4, 4]
    assert got["sampled"][0, 0] != ln["draft"][0, 0]


def test_edge_p_equal_to_q_bitwise_always_accepts():
    ln = _edge_base(6)
    ln["draft_logits"] = ln["logits"][:, :EG].clone()
    ln["draft"] = ln["logits"][:, :EG].argmax(-1)    # (a token every warper keeps)
    u = ln["uniforms"].clone()
    u[:, :, 1] = 1.0 - 2.0 ** -24     # the largest u1 the Philox path can give
    for sampling in ((1.0, 0, 1.0, 3), (0.7, 5, 0.9, 3)):
        got = _exact(ln, sampling=sampling, uniforms=u)
        assert got["n_accepted"].tolist() == [EG] * 3
    u[:, 0, 1] = 1.0                  # (only the hook can say 1: rejected, no residual mass, the fallback draws from P_0)
    got = _exact(ln, uniforms=u)
    assert got["n_accepted"].tolist() == [0, 0, 0]


def test_edge_degenerate_rows():
    nan, inf = float("nan"), float("inf")
    for where in ("target", "drafter", "both"):
        ln = _edge_base(7)
        rows = [ln["logits"]] * (where != "drafter") + [ln["draft_logits"]] * (where != "target")
        for x in rows:
            x[0, 1, 9], x[0, 1, 3], x[0, 1, 12] = nan, inf, nan     # the first NaN wins: one-hot at 9
            x[1, 0, 6], x[1, 0, 11] = inf, inf                       # the first +inf: one-hot at 6
            x[2, 2] = -inf                                            # only -inf: one-hot at 0
        ln["draft"][0, 1], ln["draft"][1, 0], ln["draft"][2, 2] = 9, 6, 0
        for ns in ([4, 4, 4], [1, 0, 2]):
            _exact(ln, uniforms=_forced(ln["uniforms"], ns))
        got = _exact(ln)       # (the random uniforms decide)
        assert bool((got["sampled"] < EV).all())
        _exact(ln, with_q=False)


def test_edge_top_k_one_is_the_greedy_kernel():
    from flasht5_amd import speculative_accept
    for case in (c for c in G.CASES if c["id"].startswith(("mixed-V512", "eos-V512", "limit-V512", "frozen-V512"))):
        ln = G.inputs(case)            # (rows with a unique maximum)
        want = G.reference(case, ln)
        for with_q in (False, True):
            dl = None
            if with_q:                 # a drafter that would have proposed these drafts under top_k = 1
                dl = torch.randn(ln["logits"].shape[0], case["gamma"], case["V"]).to(case["dtype"])
                dl.scatter_(2, ln["draft"].clamp(0, case["V"] - 1).unsqueeze(-1), 30.0)
            t = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ln.items()}
            na, nn = speculative_accept(t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"],
                                        draft_seqlens=t["draft_seqlens"], sampling=(0.9, 1, 1.0, 5), draft_logits=None if dl is None else dl.to(DEV))
            got = {k: t[k].cpu() for k in STATE}
            got.update(n_accepted=na.cpu(), n_new=nn.cpu())
            assert G.same(got, want), (case["id"], with_q)


# ------------------------------------------------------------------------------------------------------------------------ law
def _bound(dof):
    """the 0.999 chi-square quantile by the Wilson-Hilferty approximation (as tests/test_sampling_gpu.py computes it)"""
    return dof * (1 - 2 / (9 * dof) + 3.09 * (2 / (9 * dof)) ** 0.5) ** 3


@pytest.mark.parametrize("which", ["same", "near", "far", "onehot"])
def test_law_of_the_first_emitted_token(which):
    from flasht5_amd import sample_logits, speculative_accept
    g = torch.Generator().manual_seed(5)
    V, N, T, top_p, seed = 200, 1 << 14, 0.8, 0.95, 4242
    p_row = (torch.randn(V, generator=g) * 1.5).bfloat16()
    q_row = dict(same=p_row, near=(p_row.float() + 0.4 * torch.randn(V, generator=g)).bfloat16(),
                 far=(torch.randn(V, generator=g) * 1.5).bfloat16(), onehot=(torch.randn(V, generator=g) * 1.5).bfloat16())[which]
    other = (torch.randn(V, generator=g) * 1.5).bfloat16()      # chunk row 1: never reaches the first emitted token
    logits = torch.stack((p_row, other)).to(DEV).expand(N, 2, V)
    dl = q_row.to(DEV).expand(N, 1, V)
    lens = (torch.arange(N, dtype=torch.int32, device=DEV) % 7) + 2      # (old; the drafter sits at the same lengths)
    draft = sample_logits(dl[:, 0], T, 0, top_p, seed=seed ^ R.DRAFT_KEY, offsets=lens + 1).unsqueeze(1)
    labels = torch.zeros(N, 12, dtype=torch.long, device=DEV)
    tok = torch.zeros(N, dtype=torch.long, device=DEV)
    seen = torch.zeros(N, dtype=torch.bool, device=DEV)
    cs = lens + 2
    na, nn = speculative_accept(logits, draft, cs, labels, tok, seen, 11, sampling=(T, 0, top_p, seed),
                                draft_logits=None if which == "onehot" else dl)
    first = labels.gather(1, (lens.long() + 1).unsqueeze(1))[:, 0].cpu().numpy()
    accepted = (na.cpu().numpy() >= 1)
    P, Q = R.dist(p_row, T, 0, top_p), R.dist(q_row, T, 0, top_p)
    a = float((Q["p"] * P["p"]).sum()) if which == "onehot" else float(np.minimum(P["p"], Q["p"]).sum())
    prob = P["p"]
    cnt = np.bincount(first, minlength=V)
    assert cnt[prob == 0].sum() == 0
    big = prob * N >= 5
    exp, obs = prob[big] * N, cnt[big]
    rest_e, rest_o = N - exp.sum(), N - obs.sum()
    chi2 = float(((obs - exp) ** 2 / exp).sum() + ((rest_o - rest_e) ** 2 / rest_e if rest_e >= 5 else 0.0))
    dof = int(big.sum())
    rate = float(accepted.mean())
    print(f"[spec-sample] law {which}: chi2 {chi2:.1f} (dof {dof}, bound {_bound(dof):.1f}), acceptance {rate:.4f} against {a:.4f}")
    assert chi2 < _bound(dof), (chi2, _bound(dof), dof)
    assert abs(rate - a) <= 5 * math.sqrt(a * (1 - a) / N), (rate, a)


# --------------------------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_while_the_lengths_grow_equals_eager():
    from flasht5_amd import speculative_accept
    case = next(c for c in R.CASES if c["id"] == "grid-V512-bfloat16-g4")
    ln = R.inputs(case, near=True)
    M = case["gamma"] + 1
    ln["cache_seqlens"] = torch.tensor([0, 2, 20], dtype=torch.int32)   # (before the chunk step)
    ln["draft_seqlens"] = ln["cache_seqlens"].clone()
    ln["limit"] = torch.tensor([39, 39, 27], dtype=torch.int32)
    keys = ("logits", "draft_logits", "draft", "cache_seqlens", "draft_seqlens", "labels", "tok", "seen_eos", "limit")

    def fresh():
        return {k: ln[k].to(DEV).clone() for k in keys}

    def one(t, seed):
        t["cache_seqlens"].add_(M)
        t["draft_seqlens"].add_(M)
        return speculative_accept(t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"],
                                  draft_seqlens=t["draft_seqlens"], sampling=(0.9, 50, 0.95, seed), draft_logits=t["draft_logits"],
                                  return_sampled=True)

    def rounds(seed):
        e, out = fresh(), []
        for _ in range(6):
            r = one(e, seed)
            out.append([x.cpu().clone() for x in (e["labels"], e["tok"], e["cache_seqlens"], e["draft_seqlens"], e["seen_eos"], *r)])
        return out
    eager, again, other = rounds(7), rounds(7), rounds(8)
    assert all(torch.equal(a, b) for x, y in zip(eager, again) for a, b in zip(x, y))          # the same seed: the same bits
    assert any(not torch.equal(a, b) for x, y in zip(eager, other) for a, b in zip(x, y))      # another seed differs
    assert eager[0][2].tolist() != eager[-1][2].tolist()                                        # the lengths grew
    t = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = one(t, 7)
    for i in range(6):
        graph.replay()
        torch.cuda.synchronize()
        now = [x.cpu() for x in (t["labels"], t["tok"], t["cache_seqlens"], t["draft_seqlens"], t["seen_eos"], *r)]
        assert all(torch.equal(a, b) for a, b in zip(now, eager[i])), f"replay {i}"
    del graph


# ---------------------------------------------------------------------------------------------------------------- model level
T_MAX = 16
SAMPLING = (0.9, 20, 0.95)


def _model(seed=0, vocab=512, layers=2):
    """test_speculative_gpu.py's small model, restated"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=layers,
                   relative_attention_max_distance=64, max_sequence_length=128, attention_type="fat5_rpe")
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


class _Setup:
    def __init__(self):
        self.m = _model(seed=11).to(DEV).bfloat16()
        self.other = _model(seed=12, layers=1).to(DEV).bfloat16()
        with torch.no_grad():      # logits with a spread worth sampling from (the initial lm_head gives a nearly flat row)
            self.m.lm_head.weight.mul_(6.0)
            self.other.lm_head.weight.mul_(6.0)
        V = self.m.config.vocab_size
        g = torch.Generator().manual_seed(5)
        ids = torch.randint(2, V, (4, 33), generator=g)
        ids[:, 17:33] = ids[:, 1:17]          # (a repeated stretch: the lookup finds something)
        self.ids = ids.to(DEV)
        self.prompt = torch.tensor([[0, 5, 7], [0, 5, 9], [0, 5, 11], [0, 5, 13]]).to(DEV)


@pytest.fixture(scope="module")
def su():
    return _Setup()


def _loop(m, ids, prompt, gamma, sampling, assistant=None, lookup_ngram=None, keep=None):
    """the rounds of `generate(do_sample=True, ...)` driven from outside through the public pieces (`draft_tokens` or
    `prompt_lookup_draft`, `decode_chunk`, `speculative_accept`); `keep` collects every round's inputs and outputs on the host"""
    from flasht5_amd import prompt_lookup_draft, speculative_accept
    from flasht5_amd.speculative import draft_tokens
    B, P = prompt.shape
    V = m.config.vocab_size
    state = m.init_decode_state(ids, max_length=T_MAX + gamma + 1, prompt_length=P)
    dstate = None if assistant is None else assistant.init_decode_state(ids, max_length=T_MAX + gamma + 1, prompt_length=P)
    labels = torch.zeros((B, P + T_MAX), dtype=torch.long, device=DEV)
    labels[:, :P] = prompt
    tok = prompt[:, P - 1].clone()
    seen = torch.zeros((B,), dtype=torch.bool, device=DEV)
    draft = torch.zeros((B, gamma), dtype=torch.long, device=DEV)
    if P > 1:
        m.decode_chunk(state, prompt[:, :P - 1], logits="none")
        if dstate is not None:
            assistant.decode_chunk(dstate, prompt[:, :P - 1], logits="none")
    dl, drafted, accepted, rounds = None, 0, 0, 0
    while not bool(seen.all()):
        live = int((~seen).sum())
        if assistant is not None:
            dl = draft_tokens(assistant, dstate, tok, draft, sampling=sampling, draft_logits=dl)
            drafted += live * gamma
        else:
            _, n_prop = prompt_lookup_draft(ids.to(torch.int64), labels, state.cache_seqlens, tok, seen, gamma, lookup_ngram, None, V, out=draft)
            drafted += int(n_prop.sum())
        state.steps = 0
        before = state.cache_seqlens.cpu().clone()
        logits = m.decode_chunk(state, torch.cat((tok.unsqueeze(1), draft), 1), logits="all")
        was_seen = seen.cpu().clone()
        na, nn, sampled, aux = speculative_accept(logits, draft, state.cache_seqlens, labels, tok, seen, P - 1 + T_MAX,
                                                  draft_seqlens=None if dstate is None else dstate.cache_seqlens, sampling=sampling,
                                                  draft_logits=dl, return_sampled=True, return_aux=True)
        accepted += int((na if assistant is not None else torch.minimum(na, n_prop)).sum())
        rounds += 1
        assert rounds <= T_MAX
        if keep is not None:
            keep.append(dict(logits=logits.cpu(), draft_logits=None if dl is None else dl.cpu().clone(), draft=draft.cpu().clone(),
                             old=before, seen=was_seen, sampled=sampled.cpu(), aux=aux.cpu(), n_new=nn.cpu()))
    return labels, state.cache_seqlens.cpu(), dict(rounds=rounds, drafted=drafted, accepted=accepted)


@pytest.mark.parametrize("drafter", ["assistant", "lookup"])
def test_the_replayed_loop_is_what_the_restatement_gives_and_generate_equals_it(su, drafter):
    from flasht5_amd.generation import finish_labels
    gamma, seed = 4, 2024
    sampling = SAMPLING + (seed,)
    kw = dict(assistant=su.other) if drafter == "assistant" else dict(lookup_ngram=2)
    keep = []
    labels, lens, st = _loop(su.m, su.ids, su.prompt, gamma, sampling, keep=keep, **kw)
    V, M = su.m.config.vocab_size, gamma + 1
    tally = _Tally()
    for rnd in keep:
        for b in range(su.ids.shape[0]):
            if bool(rnd["seen"][b]):
                assert rnd["sampled"][b].tolist() == [-1] * M and int(rnd["n_new"][b]) == 0
                continue
            want_u = R.round_uniforms(seed, 0, int(rnd["old"][b]), b, M)
            assert rnd["aux"][b].tolist() == [list(w) for w in want_u]
            cache = {}

            def dist_of(x, i, cache=cache, b=b):
                if (id(x), i) not in cache:
                    cache[id(x), i] = R.dist(x[b, i], *SAMPLING)
                return cache[id(x), i]
            dq = None if rnd["draft_logits"] is None else (lambda i, x=rnd["draft_logits"]: dist_of(x, i))
            _check_row(tally, lambda i, x=rnd["logits"]: dist_of(x, i), dq, rnd["draft"][b].tolist(), rnd["aux"][b].tolist(),
                       rnd["sampled"][b], V)
    print(f"[spec-sample] model loop, {drafter}: {st}, {tally.rows} rows restated, {tally.ambiguous} ambiguous")
    assert tally.ambiguous * 4 <= tally.rows, (tally.ambiguous, tally.rows)
    L = int(lens.max())
    want = finish_labels(labels[:, :L + 1])
    gkw = dict(assistant_model=su.other, num_assistant_tokens=gamma) if drafter == "assistant" else dict(prompt_lookup_num_tokens=gamma)
    for graph in (False, True):
        got, gst = su.m.generate(su.ids, max_length=T_MAX, do_sample=True, temperature=SAMPLING[0], top_k=SAMPLING[1], top_p=SAMPLING[2],
                                 seed=seed, decoder_input_ids=su.prompt, graph=graph, return_stats=True, **gkw)
        assert torch.equal(got, want), (drafter, graph)
        assert gst == st, (gst, st)


def test_top_k_one_equals_plain_greedy_on_decisive_models():
    import test_speculative_gpu as TG
    t5 = TG._Setup("t5_rpe", 4)
    for name in ("same", "half"):
        for graph in (False, True):
            got, st = t5.m.generate(t5.ids, max_length=TG.T_MAX, assistant_model=t5.assistants[name], num_assistant_tokens=4, graph=graph,
                                    do_sample=True, top_k=1, seed=9, return_stats=True)
            assert torch.equal(got, t5.plain), (name, graph)
            print(f"[spec-sample] top_k 1, decisive, drafted by {name}, graph {graph}: {st}")
    got = t5.m.generate(t5.ids, max_length=TG.T_MAX, prompt_lookup_num_tokens=4, do_sample=True, top_k=1, seed=9, decoder_input_ids=t5.prompt)
    assert torch.equal(got, t5.plain_prompt)


def test_a_model_drafting_for_itself_has_most_drafts_accepted(su):
    """the chunk step and the one-row step differ by rounding only, so TV(p, q) is near 0; a counter or key mix-up drives the
    acceptance towards sum p^2 instead, a few percent here"""
    got, st = su.m.generate(su.ids, max_length=T_MAX, do_sample=True, temperature=SAMPLING[0], top_k=SAMPLING[1], top_p=SAMPLING[2], seed=31,
                            assistant_model=su.m, num_assistant_tokens=4, return_stats=True)
    print(f"[spec-sample] self-drafting: {st}, acceptance {st['accepted'] / max(1, st['drafted']):.3f}")
    assert st["accepted"] * 2 >= st["drafted"] > 0, st


@pytest.mark.parametrize("mode", ["prompt", "padding", "fp8"])
@pytest.mark.parametrize("drafter", ["assistant", "lookup"])
def test_other_modes_eager_equals_graph(su, mode, drafter):
    gamma = 4
    kw = dict(max_length=T_MAX, do_sample=True, temperature=SAMPLING[0], top_k=SAMPLING[1], top_p=SAMPLING[2], seed=77, return_stats=True)
    kw.update(dict(assistant_model=su.other, num_assistant_tokens=gamma) if drafter == "assistant" else dict(prompt_lookup_num_tokens=gamma))
    ids = su.ids
    if mode == "prompt":
        kw["decoder_input_ids"] = su.prompt
    elif mode == "padding":
        mask = torch.ones_like(ids)
        mask[1, 20:] = 0
        mask[3, 9:] = 0
        kw["attention_mask"] = mask
    else:
        kw["kv_cache_dtype"] = "fp8"
    eager, st = su.m.generate(ids, **kw)
    graphed, gst = su.m.generate(ids, graph=True, **kw)
    assert torch.equal(eager, graphed) and st == gst, (mode, drafter)
    P = 3 if mode == "prompt" else 1
    assert set(st) == {"rounds", "drafted", "accepted"} and all(type(v) is int for v in st.values())
    assert 0 <= st["accepted"] <= st["drafted"] <= st["rounds"] * gamma * ids.shape[0]
    assert 1 <= st["rounds"] <= T_MAX and eager.shape[1] <= P + T_MAX
    print(f"[spec-sample] {mode}, {drafter}: {st}")
