"""Prompt-lookup speculative decoding on the GPU: the lookup kernel (csrc/lookup_kernels.h through `prompt_lookup_draft`) exactly
against the restatement of tests/lookup_ref.py on its case list (every output is an integer: torch.equal, no tolerance), with
padded row strides, guard columns around the draft and sentinels behind every row; reruns; one captured launch replayed while
the sequences change; and the model level: `generate(prompt_lookup_num_tokens=...)` on decisive models must equal plain greedy
`generate` exactly and return the statistics the CPU simulation of tests/lookup_ref.py derives, and on a model with a random
lm_head every produced token must lie within the decode path's logit bound of the teacher-forced maximum.

The `[prompt-lookup] ...` lines (acceptance per setting, the worst logit gap) are what DESIGN 4.18 records."""
import pytest
import torch

import lookup_ref as R
import spec_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 3                          # guard columns on either side of every row of the draft
SRC_PAD, LAB_PAD = 5, 3            # slack elements behind every row of source and of labels


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _device_call(case, ln):
    """the case's tensors on the device, every one a view with a padded row stride: what lies behind a row of source is the
    row's pending token (a scan that ran on would find it), behind a row of labels an id a wrong read would propose"""
    B, L_src = ln["source"].shape
    ncols, gamma = ln["labels"].shape[1], case["gamma"]
    src_buf = ln["tok"].view(B, 1).repeat(1, L_src + SRC_PAD).to(DEV)
    source = src_buf[:, :L_src]
    source.copy_(ln["source"])
    lab_buf = torch.full((B, ncols + LAB_PAD), 9, dtype=torch.long, device=DEV)
    labels = lab_buf[:, :ncols]
    labels.copy_(ln["labels"])
    out_buf = torch.full((B, gamma + 2 * GUARD), -7, dtype=torch.long, device=DEV)
    t = dict(source=source, labels=labels, cache_seqlens=ln["cache_seqlens"].to(DEV), tok=ln["tok"].to(DEV), seen_eos=ln["seen_eos"].to(DEV),
             src_seqlens=None if ln["src_seqlens"] is None else ln["src_seqlens"].to(DEV), out=out_buf[:, GUARD:GUARD + gamma])
    return t, out_buf


def _run(case, t):
    from flasht5_amd import prompt_lookup_draft
    return prompt_lookup_draft(t["source"], t["labels"], t["cache_seqlens"], t["tok"], t["seen_eos"], case["gamma"], case["N"],
                               src_seqlens=t["src_seqlens"], vocab_size=case["V"], out=t["out"])


@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_kernel_equals_the_restatement(case):
    ln = R.inputs(case)
    want_draft, want_n = R.reference(case, ln)
    t, out_buf = _device_call(case, ln)
    before = {k: v.clone() for k, v in t.items() if v is not None and k != "out"}
    draft, n = _run(case, t)
    torch.cuda.synchronize()
    assert draft.data_ptr() == t["out"].data_ptr() and n.dtype == torch.int32 and draft.dtype == torch.int64
    assert torch.equal(draft.cpu(), want_draft), f"{case['id']}: draft: got {draft.tolist()} want {want_draft.tolist()}"
    assert torch.equal(n.cpu(), want_n), f"{case['id']}: n_proposed: got {n.tolist()} want {want_n.tolist()}"
    g = case["gamma"]
    assert bool((out_buf[:, :GUARD] == -7).all()) and bool((out_buf[:, GUARD + g:] == -7).all()), f"{case['id']}: guard columns"
    assert all(torch.equal(v, t[k]) for k, v in before.items()), f"{case['id']}: an input was written"
    first = out_buf.clone()
    draft2, n2 = _run(case, t)
    assert torch.equal(out_buf, first) and torch.equal(n2, n), f"{case['id']}: a second run gives other bits"


def test_kernel_without_out_and_with_one_row():
    """out=None returns a new contiguous tensor; B = 1 and a batch of rows taken with a step"""
    from flasht5_amd import prompt_lookup_draft
    case = next(c for c in R.CASES if c["id"].startswith("random-g4-N3-L600"))
    ln = R.inputs(case)
    for rows in (slice(0, 3), slice(0, 1), slice(0, 3, 2)):
        sub = {k: (v[rows].clone() if torch.is_tensor(v) else v) for k, v in ln.items()}
        want = R.reference(case, sub)
        src, lab = ln["source"].to(DEV)[rows], ln["labels"].to(DEV)[rows]   # (a stepped slice: the row stride is twice the width)
        d = {k: sub[k].to(DEV) for k in ("cache_seqlens", "tok", "seen_eos", "src_seqlens")}
        draft, n = prompt_lookup_draft(src, lab, d["cache_seqlens"], d["tok"], d["seen_eos"], case["gamma"], case["N"],
                                       src_seqlens=d["src_seqlens"], vocab_size=case["V"])
        assert draft.is_contiguous() and R.same((draft.cpu(), n.cpu()), want)
    z = lambda *s, dt=torch.long: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    draft, n = prompt_lookup_draft(z(0, 5), z(0, 12), z(0, dt=torch.int32), z(0), z(0, dt=torch.bool), 4)
    assert draft.shape == (0, 4) and n.shape == (0,)
    with pytest.raises(ValueError, match="labels must be on"):
        prompt_lookup_draft(z(2, 5), torch.zeros(2, 12, dtype=torch.long), z(2, dt=torch.int32), z(2), z(2, dt=torch.bool), 4)


def test_twenty_reruns_give_the_same_bits():
    for name in ("random-g4-N16-L4099", "random-g15-N3-L4099", "many-g4-N1"):
        case = next(c for c in R.CASES if c["id"].startswith(name))
        t, out_buf = _device_call(case, R.inputs(case))
        _, n = _run(case, t)
        first, first_n = out_buf.clone(), n.clone()
        for _ in range(20):
            out_buf[:, GUARD:GUARD + case["gamma"]] = -1
            _, n = _run(case, t)
            assert torch.equal(out_buf, first) and torch.equal(n, first_n), name


def test_graph_replay_while_the_sequences_change():
    """one captured launch; between the replays labels, tok, the lengths, the source lengths and the finished rows change in
    place, and every replay equals the restatement of the state it ran on"""
    case = next(c for c in R.CASES if c["id"].startswith("random-g4-N3-L600"))
    ln = R.inputs(case)
    t, out_buf = _device_call(case, ln)
    _run(case, t)   # (warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        draft, n = _run(case, t)
    seen_drafts = set()
    for i in range(6):
        now = dict(ln)
        now["cache_seqlens"] = (ln["cache_seqlens"] - 5 * i).clamp(min=0)
        now["tok"] = (ln["tok"] + i) % 3 + 2
        now["labels"] = ln["labels"].roll(i, 1)
        now["src_seqlens"] = (ln["src_seqlens"] - 37 * i).clamp(min=0)
        now["seen_eos"] = torch.tensor([i == 4, False, i == 2])
        for k in ("cache_seqlens", "tok", "labels", "src_seqlens", "seen_eos"):
            t[k].copy_(now[k])
        out_buf[:, GUARD:GUARD + case["gamma"]] = -1
        graph.replay()
        torch.cuda.synchronize()
        want = R.reference(case, now)
        assert R.same((draft.cpu(), n.cpu()), want), f"replay {i}: got {draft.tolist()} {n.tolist()} want {want[0].tolist()} {want[1].tolist()}"
        seen_drafts.add(str(want[0].tolist()))
    assert len(seen_drafts) >= 4   # (the replays did not all compute the same thing)
    del graph


# ---------------------------------------------------------------------------------------------------------------- model level
VOCAB, B, L, T_MAX = 128, 4, 33, 20


def _model(seed=0, **kw):
    """the small model of the CPU tests: d_model 64, 2 heads of 64, 1 encoder and 2 decoder layers, vocabulary 128"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    c = FAT5Config(vocab_size=VOCAB, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=64, attention_type="fat5_rpe", **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c).to(DEV).bfloat16()


def _sigma(seed, eos_after=None):
    """a permutation of the ids with EOS (1) a fixed point, so that no chain reaches it; eos_after=(t, k): the chain from token t
    reaches EOS with its k-th token instead (EOS then leads to where that token led)"""
    others = torch.tensor([0] + list(range(2, VOCAB)))
    sigma = torch.arange(VOCAB)
    sigma[others] = others[torch.randperm(VOCAB - 1, generator=torch.Generator().manual_seed(1000 + seed))]
    if eos_after is not None:
        t, k = eos_after
        for _ in range(k - 1):
            t = int(sigma[t])
        sigma[1], sigma[t] = sigma[t].clone(), 1
    assert sorted(sigma.tolist()) == list(range(VOCAB))
    return sigma


def _decisive(m, sigma):
    """lm_head row sigma(t) is token t's embedding, so the next token is sigma(current token).  At d_model 64 the margin of that
    choice is small (a row that attends to five encoder positions loses it), so the decoder's attention output projections are
    halved first: every kernel still runs on the same shapes, and the token's own embedding dominates the residual stream"""
    with torch.no_grad():
        if not getattr(m, "_damped", False):
            for blk in m.decoder.block:
                blk.self_attention_layer.self_attention.o.weight.mul_(0.5)
                blk.cross_attention_layer.cross_attention.o.weight.mul_(0.5)
            m._damped = True
        m.lm_head.weight[sigma.to(DEV)] = m.shared.weight


def _chain(sigma, t, n):
    out = []
    for _ in range(n):
        t = int(sigma[t])
        out.append(t)
    return out


class _Setup:
    def __init__(self):
        self.sigma = _sigma(3)
        self.m = _model(seed=3)
        _decisive(self.m, self.sigma)
        g = torch.Generator().manual_seed(103)
        self.random = torch.randint(2, VOCAB, (B, L), generator=g)
        self.prompt = torch.tensor([[0, 5, t] for t in (7, 11, 13, 17)])
        chain0 = torch.tensor(_chain(self.sigma, 0, L))
        self.sources = {
            "unrelated": (self.random, None, None),
            "chain": (chain0.repeat(B, 1), None, None),
            "half": (torch.stack([chain0 if b % 2 == 0 else self.random[b] for b in range(B)]), None, None),
            # the copy starts at column 12: row 0 sees all of it, row 3 its first tokens, rows 1 and 2 none of it
            "hidden": (torch.cat((self.random[:, :12], chain0[:L - 12].repeat(B, 1)), 1), torch.tensor([33, 10, 5, 16], dtype=torch.int32), None),
            "prompt": (torch.stack([torch.tensor(_chain(self.sigma, int(self.prompt[b, 2]), L)) if b != 1 else self.random[b] for b in range(B)]),
                       None, self.prompt),
        }
        self.sources["fp8"] = self.sources["half"]


@pytest.fixture(scope="module")
def t5():
    return _Setup()


def _mask(lens):
    return None if lens is None else (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).long().to(DEV)


@pytest.mark.parametrize("setting", ["unrelated", "chain", "half", "hidden", "prompt", "fp8"])
def test_generate_with_the_lookup_equals_plain_greedy(t5, setting):
    ids, lens, prompt = t5.sources[setting]
    kw = dict(max_length=T_MAX, attention_mask=_mask(lens))
    if prompt is not None:
        kw["decoder_input_ids"] = prompt.to(DEV)
    if setting == "fp8":
        kw["kv_cache_dtype"] = "fp8"
    plain = t5.m.generate(ids.to(DEV), **kw)
    cpu_prompt = prompt if prompt is not None else torch.zeros((B, 1), dtype=torch.long)
    assert torch.equal(plain.cpu(), R.greedy_chain(t5.sigma, cpu_prompt, T_MAX)), "the model is not decisive"   # (the premise)
    assert plain.shape[1] == cpu_prompt.shape[1] + T_MAX and not bool((plain[:, 1:-1] == 1).any())
    for gamma in (1, 4):
        for N in (1, 2, 3):
            _, _, want = R.simulate_generate(t5.sigma, ids, lens, cpu_prompt, T_MAX, gamma, N, accept=spec_ref.accept_ref)
            for graph in (False, True):
                got, st = t5.m.generate(ids.to(DEV), graph=graph, prompt_lookup_num_tokens=gamma, max_matching_ngram_size=N,
                                        return_stats=True, **kw)
                assert torch.equal(got, plain), (setting, gamma, N, graph)
                assert set(st) == {"rounds", "drafted", "accepted"} and all(type(v) is int for v in st.values())
                assert st == want, (setting, gamma, N, graph, st, want)
            print(f"[prompt-lookup] {setting} gamma {gamma} N {N}: {want} for {T_MAX} tokens of {B} rows")
    if setting == "chain":     # every draft is right: gamma + 1 tokens per round, but for the first round of an empty key's luck
        assert want["accepted"] == want["drafted"] and want["rounds"] <= T_MAX // 4 + 1
    if setting == "hidden":    # rows 1 and 2 must not see the copy behind their lengths: the simulation would differ if they did
        _, _, seeing = R.simulate_generate(t5.sigma, ids, None, cpu_prompt, T_MAX, 4, 3)
        assert seeing["rounds"] <= want["rounds"] and seeing["accepted"] > want["accepted"]
    tensor = t5.m.generate(ids.to(DEV), prompt_lookup_num_tokens=4, **kw)   # (no stats: the tensor alone)
    assert torch.is_tensor(tensor) and torch.equal(tensor, plain)


def test_eos_inside_a_copied_continuation():
    """every row's chain is in its source; row 0's reaches EOS with its 6th token, in the middle of a copied continuation: the row
    ends there, the others run on to max_length"""
    sigma = _sigma(3, eos_after=(7, 6))
    m = _model(seed=3)
    _decisive(m, sigma)
    prompt = torch.tensor([[0, 5, t] for t in (7, 13, 17, 19)])   # (the chains of 13, 17 and 19 do not pass through 7's)
    ids = torch.stack([torch.tensor(_chain(sigma, int(prompt[b, 2]), L)) for b in range(B)])
    assert int(ids[0, 5]) == 1 and not bool((ids[1:, :T_MAX] == 1).any())
    plain = m.generate(ids.to(DEV), max_length=T_MAX, decoder_input_ids=prompt.to(DEV))
    assert torch.equal(plain.cpu(), R.greedy_chain(sigma, prompt, T_MAX))
    assert plain[0, 3:9].tolist() == ids[0, :6].tolist() and bool((plain[0, 9:] == 0).all())
    for graph in (False, True):
        got, st = m.generate(ids.to(DEV), max_length=T_MAX, decoder_input_ids=prompt.to(DEV), graph=graph, prompt_lookup_num_tokens=4,
                             max_matching_ngram_size=2, return_stats=True)
        assert torch.equal(got, plain), graph
        _, _, want = R.simulate_generate(sigma, ids, None, prompt, T_MAX, 4, 2, accept=spec_ref.accept_ref)
        assert st == want and st["accepted"] >= T_MAX, (st, want)


def _loop(m, ids, gamma, N, mask=None):
    """the rounds of `generate(prompt_lookup_num_tokens=...)` driven from outside through the public pieces; returns the raw
    labels, the final lengths and the counters"""
    from flasht5_amd import prompt_lookup_draft, speculative_round
    n_rows = ids.shape[0]
    state = m.init_decode_state(ids, max_length=T_MAX + gamma + 1, prompt_length=1)
    labels = torch.zeros((n_rows, 1 + T_MAX), dtype=torch.long, device=DEV)
    tok = torch.zeros((n_rows,), dtype=torch.long, device=DEV)
    seen = torch.zeros((n_rows,), dtype=torch.bool, device=DEV)
    rounds = proposed = accepted = 0
    while not bool(seen.all()):
        draft, n_prop = prompt_lookup_draft(ids, labels, state.cache_seqlens, tok, seen, gamma, N, vocab_size=VOCAB)
        na, _ = speculative_round(m, state, tok, draft, labels, seen, T_MAX)
        rounds, proposed, accepted = rounds + 1, proposed + int(n_prop.sum()), accepted + int(torch.minimum(na, n_prop).sum())
        assert rounds <= T_MAX
    return labels, state.cache_seqlens.cpu(), (rounds, proposed, accepted)


def test_random_lm_head_stays_within_the_logit_bound():
    """random lm_head: a chunk step and a one-row step round differently, so plain greedy is no exact reference.  Along the
    output the teacher-forced logits Z of the training forward must put every produced token within
    2 * 0.02 * max(1, max|Z|) of the row maximum (the decode path's logit bound, DESIGN 4.10, once for each side); no position is
    left out"""
    from flasht5_amd.generation import finish_labels
    LOGIT_BOUND = 0.02
    m = _model(seed=11)
    ids = torch.randint(2, VOCAB, (B, L), generator=torch.Generator().manual_seed(5)).to(DEV)
    worst = 0.0
    for gamma, N in ((4, 2), (15, 1)):
        labels, lens, (rounds, proposed, accepted) = _loop(m, ids, gamma, N)
        n_cols = int(lens.max())
        with torch.no_grad():
            Z = m.lm_head(m.decoder(labels[:, :n_cols], encoder_hidden_states=m.encoder(ids))).float()   # Z[:, t] chooses column t + 1
        for b in range(B):
            for t in range(int(lens[b])):
                z = Z[b, t]
                gap = float(z.max() - z[labels[b, t + 1]]) / max(1.0, float(z.abs().max()))
                worst = max(worst, gap)
                assert gap <= 2 * LOGIT_BOUND, (gamma, N, b, t, gap)
        print(f"[prompt-lookup] random lm_head, gamma {gamma} N {N}: {rounds} rounds, {proposed} proposed, {accepted} accepted, "
              f"{int(lens.sum())} tokens, worst gap {worst:.3e} of the bound {2 * LOGIT_BOUND:.1e}")
        got = m.generate(ids, max_length=T_MAX, prompt_lookup_num_tokens=gamma, max_matching_ngram_size=N)
        assert torch.equal(got, finish_labels(labels[:, :n_cols + 1]))


def test_the_default_path_issues_no_lookup(t5, monkeypatch):
    """prompt_lookup_num_tokens=None: `generate` never reaches the op; with a value it does, once per round"""
    from flasht5_amd import prompt_lookup
    calls = []
    real = prompt_lookup.lookup_draft_op

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(prompt_lookup, "lookup_draft_op", counting)
    ids = t5.sources["chain"][0].to(DEV)
    for kw in (dict(), dict(graph=True), dict(prompt_lookup_num_tokens=None, max_matching_ngram_size=3), dict(do_sample=True, seed=1),
               dict(num_beams=2), dict(assistant_model=t5.m, num_assistant_tokens=2)):
        t5.m.generate(ids, max_length=6, **kw)
        assert not calls, kw
    _, st = t5.m.generate(ids, max_length=6, prompt_lookup_num_tokens=2, return_stats=True)
    assert len(calls) == st["rounds"] >= 1
