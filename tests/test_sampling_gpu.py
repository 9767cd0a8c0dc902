"""GPU tests of sampling: `sample_logits` (fat5_sample_logits) against the fp64 restatement in tests/sampling_ref.py -- the kept set
(aux tau and count), the Philox uniform bitwise, the inverse-CDF token with injected uniforms --, a chi-square test of 2^15 draws,
the edges (-inf never drawn, top_k = 1 / tiny top_p = argmax, degenerate rows, batch independence, determinism under graph
replay), and generation: eager == graph, top_k = 1 == greedy, and an eager decode_step loop restated with the kernel's u.

Tolerance: the kernel's e_j are fp32 __expf values and its masses exact sums of them truncated to 2^-40, so a top-p decision may
differ from the fp64 restatement only where the threshold lies within TOL * S of a cumulative mass (`margin` in the
restatement), and a token only where u * S_kept lies within TOL * S_kept of a prefix boundary (either neighbour is accepted)."""
import numpy as np
import pytest
import torch

from sampling_ref import argmax_rule, draw, restate, scaled, uniform

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 4e-6  # (__expf: exp2 of a rounded product, a few fp32 ulps of e_j; the sums themselves are exact)


def _rows(B, V, dtype, stride, g):
    buf = (torch.randn(B, stride, generator=g) * 2.5).to(dtype)
    return buf.to(DEV)[:, :V]


@pytest.mark.parametrize("V", [1, 7, 1000, 32128, 250112])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_exact_against_the_restatement(B, V, dtype):
    from flasht5_amd import sample_logits
    if B == 64 and V == 250112 and dtype != torch.bfloat16:
        pytest.skip("(the long row is covered in bf16 at B = 64)")
    g = torch.Generator().manual_seed(B * 31 + V + len(str(dtype)))
    stride = V + 8 * (1 + V % 3) if V % 2 else V + 8  # (row strides != V; odd V takes the element-load path)
    logits = _rows(B, V, dtype, stride, g)
    host = logits.cpu()
    grid = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.5, 50, 0.9), (1.0, 1, 1.0), (2.0, 0, 0.05)]
    rows = range(B) if B <= 5 else range(0, B, 9)
    ambiguous = 0
    for T, k, p in grid:
        seed = 1000 + k
        offs = torch.arange(B, dtype=torch.int32, device=DEV) * 3 + 17
        tok, aux = sample_logits(logits, T, k, p, seed=seed, offsets=offs, offset=5, return_aux=True)
        u = torch.rand(B, generator=g)
        tok_u, aux_u = sample_logits(logits, T, k, p, uniforms=u.to(DEV), return_aux=True)
        tok, aux, tok_u, aux_u = tok.cpu(), aux.cpu(), tok_u.cpu(), aux_u.cpu()
        for b in rows:
            r = restate(scaled(host[b], T), k, p)
            assert aux[b, 2].item() == uniform(seed, 5 + 3 * b + 17, b), (b, "u")
            assert aux_u[b, 2].item() == u[b].item()
            assert 0 <= tok[b] < V and r["kept"][tok[b]], (T, k, p, b)
            if r["margin"] < TOL:
                ambiguous += 1
                continue
            assert aux[b, 0].item() == r["tau"], (T, k, p, b, aux[b], r["tau"])
            assert aux[b, 3].item() == r["kept"].sum(), (T, k, p, b)
            assert abs(aux[b, 1].item() - r["ratio"]) <= 1e-5
            assert tok[b].item() in draw(r, aux[b, 2].item(), TOL), (T, k, p, b)
            assert tok_u[b].item() in draw(r, u[b].item(), TOL), (T, k, p, b)
    assert ambiguous <= len(grid) * len(rows) // 4  # (only top-p rows can be ambiguous; most are checked)


def test_distribution_chi_square():
    from flasht5_amd import sample_logits
    g = torch.Generator().manual_seed(5)
    V, N = 200, 1 << 15
    row = (torch.randn(V, generator=g) * 1.5).bfloat16()
    logits = row.to(DEV).expand(N, V)  # (a row-broadcast view: stride(0) = 0, copied by the wrapper)
    offs = torch.arange(N, dtype=torch.int32, device=DEV)
    tok = sample_logits(logits, 0.8, 0, 0.95, seed=77, offsets=offs).cpu()
    r = restate(scaled(row, 0.8), 0, 0.95)
    prob = r["e"] / r["e"].sum()
    cnt = np.bincount(tok.numpy(), minlength=V)
    assert cnt[~r["kept"]].sum() == 0
    big = prob * N >= 5
    exp = prob[big] * N
    obs = cnt[big]
    rest_e, rest_o = N - exp.sum(), N - obs.sum()
    chi2 = float(((obs - exp) ** 2 / exp).sum() + ((rest_o - rest_e) ** 2 / rest_e if rest_e >= 5 else 0.0))
    dof = int(big.sum())
    # (a fixed seed: deterministic; the bound is the 0.999 quantile, by the Wilson-Hilferty approximation)
    bound = dof * (1 - 2 / (9 * dof) + 3.09 * (2 / (9 * dof)) ** 0.5) ** 3
    assert chi2 < bound, (chi2, bound, dof)


def test_edges():
    from flasht5_amd import sample_logits
    g = torch.Generator().manual_seed(9)
    B, V = 64, 32128
    x = torch.randn(B, V, generator=g).bfloat16()
    x[:, ::3] = -float("inf")
    x[:, 1] = 40.0  # (a unique maximum)
    xd = x.to(DEV)
    for seed in range(4):
        tok = sample_logits(xd, 1.0, 0, 1.0, seed=seed).cpu()
        assert (tok % 3 != 0).all()  # -inf never drawn
    am = x.float().argmax(-1)
    assert torch.equal(sample_logits(xd, 1.3, 1, 1.0, seed=3).cpu(), am)
    assert torch.equal(sample_logits(xd, 1.0, 0, 1e-6, seed=3).cpu(), am)
    # degenerate rows: the argmax rule, inside [0, V)
    d = torch.randn(6, 1000, generator=g)
    d[0, 17] = float("nan"); d[0, 500] = float("nan")
    d[1, 3] = float("inf"); d[1, 9] = float("nan")
    d[2, 40] = float("inf"); d[2, 41] = float("inf")
    d[3] = -float("inf")
    d[4, 999] = float("nan")
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        tok, aux = sample_logits(d.to(dt).to(DEV), 0.9, 5, 0.5, seed=1, return_aux=True)
        tok = tok.cpu()
        for b in range(5):
            assert tok[b].item() == argmax_rule(d[b].to(dt).float().numpy()), (dt, b)
        assert 0 <= tok[5] < 1000
    # batch independence: row b at B = 64 == the same row alone at B = 1 with the same counter and row index
    offs = torch.arange(B, dtype=torch.int32, device=DEV)
    y = torch.randn(B, V, generator=g).bfloat16().to(DEV)
    full = sample_logits(y, 0.9, 50, 0.9, seed=11, offsets=offs).cpu()
    r = restate(scaled(y[0].cpu(), 0.9), 50, 0.9)
    one = sample_logits(y[:1], 0.9, 50, 0.9, seed=11, offsets=offs[:1]).cpu()
    assert one[0] == full[0]
    assert r["kept"][full[0]]


@pytest.mark.parametrize("B, V", [(64, 32128), (16, 250112)])
def test_top_k_off_is_exact_and_bitwise_stable(B, V):
    # top_k = 0 skips the radix select, so the kept-mass pass follows the maximum's broadcast directly: every row must still
    # match the restatement, and 20 reruns must give the same bits (tokens and aux)
    from flasht5_amd import sample_logits
    g = torch.Generator().manual_seed(B + V)
    logits = (torch.randn(B, V, generator=g) * 2).bfloat16().to(DEV)
    host = logits.cpu()
    offs = torch.arange(B, dtype=torch.int32, device=DEV)
    for p in (1.0, 0.9):
        tok0, aux0 = sample_logits(logits, 0.8, 0, p, seed=21, offsets=offs, return_aux=True)
        for _ in range(20):
            tok, aux = sample_logits(logits, 0.8, 0, p, seed=21, offsets=offs, return_aux=True)
            assert torch.equal(tok, tok0) and torch.equal(aux, aux0)
        tok0, aux0 = tok0.cpu(), aux0.cpu()
        checked = 0
        for b in range(B):
            r = restate(scaled(host[b], 0.8), 0, p)
            if r["margin"] < TOL:
                continue
            assert aux0[b, 0].item() == r["tau"] and aux0[b, 3].item() == r["kept"].sum(), (p, b)
            assert abs(aux0[b, 1].item() - r["ratio"]) <= 1e-5, (p, b)
            assert tok0[b].item() in draw(r, aux0[b, 2].item(), TOL), (p, b)
            checked += 1
        assert checked >= 3 * B // 4


def test_deterministic_and_graph_replay():
    from flasht5_amd import sample_logits
    g = torch.Generator().manual_seed(3)
    for V in (32128, 250112):
        x = torch.randn(16, V, generator=g).bfloat16().to(DEV)
        offs = torch.arange(16, dtype=torch.int32, device=DEV)
        a = sample_logits(x, 0.8, 50, 0.9, seed=5, offsets=offs)
        b = sample_logits(x, 0.8, 50, 0.9, seed=5, offsets=offs)
        c = sample_logits(x, 0.8, 0, 1.0, seed=6, offsets=offs)
        c2 = sample_logits(x, 0.8, 0, 1.0, seed=7, offsets=offs)
        assert torch.equal(a, b)
        assert not torch.equal(c, c2)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            sample_logits(x, 0.8, 50, 0.9, seed=5, offsets=offs)  # (warm-up outside the capture)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = sample_logits(x, 0.8, 50, 0.9, seed=5, offsets=offs)
        for _ in range(3):
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)
        offs.add_(1)  # (the counter lives on the device: a replay after the increment draws new uniforms)
        gr.replay()
        assert torch.equal(out, sample_logits(x, 0.8, 50, 0.9, seed=5, offsets=offs))


def _model(autocast):
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    torch.manual_seed(0)
    c = FAT5Config(vocab_size=512, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=256)
    m = FAT5ForConditionalGeneration(c).to(DEV)
    if not autocast:
        m = m.bfloat16()
    return m.eval()


@pytest.mark.parametrize("autocast", [False, True])
def test_generate_sampling(autocast):
    from flasht5_amd import sample_logits
    m = _model(autocast)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(2, 512, (5, 40), generator=g).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        kw = dict(max_length=24, do_sample=True, temperature=1.5, top_k=0, top_p=0.95, seed=123)
        eager = m.generate(ids, **kw)
        graph = m.generate(ids, graph=True, **kw)
        assert torch.equal(eager, graph)
        other = m.generate(ids, **dict(kw, seed=124))
        assert not torch.equal(eager, other)
        torch.manual_seed(42)
        s1 = m.generate(ids, max_length=24, do_sample=True)
        torch.manual_seed(42)
        s2 = m.generate(ids, max_length=24, do_sample=True, graph=True)
        assert torch.equal(s1, s2)
        # top_k = 1 == greedy wherever the maximum is unique (top-k keeps every logit tied with the k-th largest, as HF's
        # TopKLogitsWarper does, and bf16 logits tie at the maximum now and then: from a row's first tie on, either may differ)
        greedy = m.generate(ids, max_length=24)
        assert torch.equal(m.generate(ids, max_length=24, top_k=None, temperature=0.0), greedy)  # (greedy ignores them)
        samp = m.generate(ids, max_length=24, do_sample=True, top_k=1, seed=9, graph=True)
        state = m.init_decode_state(ids, max_length=24)
        tok = torch.zeros(5, dtype=torch.long, device=DEV)
        upto = torch.full((5,), greedy.shape[1] - 1, dtype=torch.long)
        for t in range(greedy.shape[1] - 1):
            logits = m.decode_step(state, tok)
            ties = ((logits == logits.max(-1, keepdim=True).values).sum(-1) > 1).cpu()
            upto = torch.where(ties & (upto == greedy.shape[1] - 1), torch.full_like(upto, t), upto)
            tok = logits.argmax(-1)
        assert (upto == greedy.shape[1] - 1).sum() >= 3, upto
        for b in range(5):
            assert torch.equal(samp[b, :upto[b] + 1], greedy[b, :upto[b] + 1]), (b, upto[b])
        # an eager decode_step loop with the restatement fed the kernel's u gives generate's tokens
        state = m.init_decode_state(ids, max_length=24)
        tok = torch.zeros(5, dtype=torch.long, device=DEV)
        steps = eager.shape[1] - 1
        for t in range(steps):
            logits = m.decode_step(state, tok)
            _, aux = sample_logits(logits, 1.5, 0, 0.95, seed=123, offsets=state.cache_seqlens, return_aux=True)
            host = logits.float().cpu()
            nxt = []
            for b in range(5):
                r = restate(scaled(host[b].to(logits.dtype), 1.5), 0, 0.95)
                cand = draw(r, aux[b, 2].item(), TOL)
                j = eager[b, t + 1].item()
                live = not (eager[b, :t + 1] == 1).any()  # (finish_labels zeroes everything after a row's first 1)
                if live and t + 1 < eager.shape[1] - 1:
                    assert j in cand, (t, b, j, cand)
                nxt.append(j if j in cand else min(cand))
            tok = torch.tensor(nxt, device=DEV)
