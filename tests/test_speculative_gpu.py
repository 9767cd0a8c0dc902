"""Speculative greedy decoding on the GPU: the verification kernel (csrc/spec_kernels.h through `speculative_accept`) exactly
against the restatement of tests/spec_ref.py on its case list (every output is an integer: torch.equal, no tolerance), one
captured round replayed while the lengths grow, and the model level: `generate(assistant_model=...)` on decisive models must
equal plain greedy `generate` exactly, scripted drafts through `speculative_round` must take the number of rounds the host
derives from the plain run, and on a non-decisive model every produced token must lie within the decode path's logit bound of the
teacher-forced maximum.

The `[speculative] ...` lines (acceptance per case, the worst logit gap) are what DESIGN 4.15 records."""
import math

import pytest
import torch

import spec_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 3   # guard columns on either side of every row of labels


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _device_call(case, ln):
    """the case's tensors on the device: logits with the case's row padding and three rows of slack per batch element, labels
    inside a buffer with GUARD columns before and after"""
    B, M, V = ln["logits"].shape
    rs = V + case["pad"]
    buf = torch.full((B, M + 3, rs), 50.0, dtype=case["dtype"], device=DEV)   # (above the planted peak: reading the slack shows)
    logits = buf[:, :M, :V]
    logits.copy_(ln["logits"])
    lab_buf = torch.full((B, R.NCOLS + 2 * GUARD), -7, dtype=torch.long, device=DEV)
    labels = lab_buf[:, GUARD:GUARD + R.NCOLS]
    labels.copy_(ln["labels"])
    lim = ln["limit"].to(DEV) if torch.is_tensor(ln["limit"]) else ln["limit"]
    t = dict(logits=logits, draft=ln["draft"].to(DEV), cache_seqlens=ln["cache_seqlens"].to(DEV), labels=labels, tok=ln["tok"].to(DEV),
             seen_eos=ln["seen_eos"].to(DEV), limit=lim, draft_seqlens=ln["draft_seqlens"].to(DEV))
    return t, lab_buf


def _run(case, ln):
    from flasht5_amd import speculative_accept
    t, lab_buf = _device_call(case, ln)
    na, nn = speculative_accept(t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"],
                                draft_seqlens=t["draft_seqlens"], eos_token_id=R.EOS)
    torch.cuda.synchronize()
    got = {k: t[k].cpu() for k in ("labels", "tok", "cache_seqlens", "draft_seqlens", "seen_eos")}
    got["n_accepted"], got["n_new"] = na.cpu(), nn.cpu()
    return got, lab_buf.cpu()


@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_kernel_equals_the_restatement(case):
    ln = R.inputs(case)
    want = R.reference(case, ln)
    got, lab_buf = _run(case, ln)
    for k in R.OUTPUTS:
        assert torch.equal(got[k], want[k]), f"{case['id']}: {k}: got {got[k].tolist()} want {want[k].tolist()}"
    assert got["n_accepted"].dtype == got["n_new"].dtype == torch.int32
    assert bool((lab_buf[:, :GUARD] == -7).all()) and bool((lab_buf[:, GUARD + R.NCOLS:] == -7).all()), f"{case['id']}: guard columns"
    again, lab_again = _run(case, ln)
    assert R.same(got, again) and torch.equal(lab_buf, lab_again), f"{case['id']}: a second run gives other bits"


def test_kernel_without_the_optional_tensors_and_with_the_sliced_batch():
    """draft_seqlens=None and an int limit; B = 1; and a batch of rows taken with a step (batch stride twice the contiguous one)"""
    from flasht5_amd import speculative_accept
    case = next(c for c in R.CASES if c["id"].startswith("mixed-V512-bfloat16-g4"))
    ln = R.inputs(case)
    for rows in (slice(0, 1), slice(0, 3, 2)):
        sub = {k: (v[rows].clone() if torch.is_tensor(v) else v) for k, v in ln.items()}
        sub["draft_seqlens"] = None
        want = R.accept_ref(sub["logits"], sub["draft"], sub["cache_seqlens"], sub["labels"], sub["tok"], sub["seen_eos"], sub["limit"])
        lg = ln["logits"].to(DEV)[rows]
        t = {k: sub[k].to(DEV) for k in ("draft", "cache_seqlens", "labels", "tok", "seen_eos")}
        na, nn = speculative_accept(lg, t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], sub["limit"])
        got = {k: t[k].cpu() for k in t if k != "draft"}
        got.update(n_accepted=na.cpu(), n_new=nn.cpu(), draft_seqlens=None)
        assert R.same(got, want)


def test_graph_replay_while_the_lengths_grow_equals_eager():
    """one captured round (the chunk step's `cache_seqlens += M`, then the kernel) replayed six times against six eager rounds:
    the rows advance by different amounts per round, one freezes at an EOS and one at its limit"""
    from flasht5_amd import speculative_accept
    case = next(c for c in R.CASES if c["id"].startswith("eos-V512"))
    ln = R.inputs(case)
    M = case["gamma"] + 1
    ln["cache_seqlens"] = torch.tensor([0, 2, 20], dtype=torch.int32)   # (before the chunk step)
    ln["draft_seqlens"] = ln["cache_seqlens"].clone()
    ln["limit"] = torch.tensor([39, 39, 27], dtype=torch.int32)
    ln["seen_eos"][:] = False
    for b in (1, 2):   # rows 1 and 2 go on: their third choice is no EOS any more (row 1 accepts 4 a round, row 2 accepts 2)
        ln["logits"][b, 2, R.EOS] = 0.0
        ln["logits"][b, 2, 9] = R.PEAK
    ln["draft"][1, 2] = 9

    def fresh():
        return {k: (v.to(DEV).clone() if torch.is_tensor(v) else v) for k, v in ln.items()}

    def one(t):
        t["cache_seqlens"].add_(M)
        t["draft_seqlens"].add_(M)
        return speculative_accept(t["logits"], t["draft"], t["cache_seqlens"], t["labels"], t["tok"], t["seen_eos"], t["limit"],
                                  draft_seqlens=t["draft_seqlens"])

    e, eager = fresh(), []
    for _ in range(6):
        na, nn = one(e)
        eager.append([x.cpu().clone() for x in (e["labels"], e["tok"], e["cache_seqlens"], e["draft_seqlens"], e["seen_eos"], na, nn)])
    assert eager[0][2].tolist() != eager[-1][2].tolist() and eager[-1][4].tolist() == [True, False, True]
    w = fresh()
    one(w)   # (warm-up on a copy)
    t = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        na, nn = one(t)
    for i in range(6):
        graph.replay()
        torch.cuda.synchronize()
        now = [x.cpu() for x in (t["labels"], t["tok"], t["cache_seqlens"], t["draft_seqlens"], t["seen_eos"], na, nn)]
        assert all(torch.equal(a, b) for a, b in zip(now, eager[i])), f"replay {i}"
    del graph


def test_operator_rejections_on_the_gpu():
    from flasht5_amd import speculative_accept
    z = lambda *s, dt=torch.long: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    lg = torch.zeros(2, 5, 16, device=DEV)
    with pytest.raises(ValueError, match="labels must be on"):
        speculative_accept(lg, z(2, 4), z(2, dt=torch.int32), torch.zeros(2, 12, dtype=torch.long), z(2), z(2, dt=torch.bool), 11)
    with pytest.raises(ValueError, match="draft must be"):   # (the shape first, the device second)
        speculative_accept(lg, torch.zeros(2, 3, dtype=torch.long), z(2, dt=torch.int32), z(2, 12), z(2), z(2, dt=torch.bool), 11)
    na, nn = speculative_accept(lg[:0], z(0, 4), z(0, dt=torch.int32), z(0, 12), z(0), z(0, dt=torch.bool), 11)
    assert na.shape == nn.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- model level
def _model(kind, seed=0, vocab=512):
    """test_decode_chunk_gpu.py's small model, restated"""
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    kw = dict(attention_type="fat5_rpe")
    if kind == "rope":
        kw = dict(position_encoding_type="RoPE")
    c = FAT5Config(vocab_size=vocab, d_model=256, d_kv=64, d_ff=512, num_heads=4, num_layers=2, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=128, **kw)
    torch.manual_seed(seed)
    return FAT5ForConditionalGeneration(c)


def _sigma(V, seed):
    return torch.randperm(V, generator=torch.Generator().manual_seed(1000 + seed))


def _decisive(m, sigma):
    """test_decode_chunk_gpu.py's construction, restated: lm_head row sigma(t) is token t's embedding, so the next token is
    sigma(current token)"""
    with torch.no_grad():
        m.lm_head.weight[sigma] = m.shared.weight


def _half(sigma, seed):
    """a permutation that agrees with sigma on about half the ids: the values at the other ids are rotated among themselves"""
    out = sigma.clone()
    other = (torch.rand(len(sigma), generator=torch.Generator().manual_seed(seed)) < 0.5).nonzero()[:, 0]
    out[other] = sigma[other.roll(1)]
    return out


T_MAX = 16


class _Setup:
    """a decisive target, its three decisive assistants (other weights: seed + 50), inputs, and the plain greedy outputs"""

    def __init__(self, kind, B):
        self.seed = 3
        self.m = _model(kind, seed=self.seed).to(DEV).bfloat16()
        V = self.m.config.vocab_size
        self.sigma = _sigma(V, self.seed)
        _decisive(self.m, self.sigma)
        self.assistants = {}
        for name, sg in (("same", self.sigma), ("other", _sigma(V, self.seed + 1)), ("half", _half(self.sigma, 77))):
            a = _model(kind, seed=self.seed + 50).to(DEV).bfloat16()
            _decisive(a, sg)
            self.assistants[name] = a
        self.ids = torch.randint(2, V, (B, 33), generator=torch.Generator().manual_seed(100 + self.seed)).to(DEV)
        inv = torch.argsort(self.sigma)
        # a prompt of 3 tokens per row; row 1 ends in the token whose second successor is EOS, so it stops early
        last = [7, int(inv[inv[1]]), 11, 13][:B]
        assert all(t > 1 for t in last)
        self.prompt = torch.tensor([[0, 5, t] for t in last]).to(DEV)
        self.plain = self.m.generate(self.ids, max_length=T_MAX)
        self.plain_prompt = self.m.generate(self.ids, max_length=T_MAX, decoder_input_ids=self.prompt)


@pytest.fixture(scope="module")
def t5():
    return _Setup("t5_rpe", 4)


@pytest.fixture(scope="module")
def rope():
    return _Setup("rope", 1)


def test_the_prompted_rows_are_ragged(t5):
    """the premise of the model-level cases: row 1 reaches EOS two tokens after the prompt, the others go on"""
    out = t5.plain_prompt
    assert out[1, 3:5].tolist() == [int(t5.sigma[t5.prompt[1, 2]]), 1] and bool((out[1, 5:] == 0).all())
    assert out.shape[1] > 8 and not bool((out[0, 3:6] == 1).any())


@pytest.mark.parametrize("gamma", [1, 4])
@pytest.mark.parametrize("which", ["same", "other", "half"])
def test_generate_with_an_assistant_equals_plain_greedy(t5, which, gamma):
    a = t5.assistants[which]
    for graph in (False, True):
        got, st = t5.m.generate(t5.ids, max_length=T_MAX, assistant_model=a, num_assistant_tokens=gamma, graph=graph, return_stats=True)
        assert torch.equal(got, t5.plain), (which, gamma, graph)
        gotp, stp = t5.m.generate(t5.ids, max_length=T_MAX, assistant_model=a, num_assistant_tokens=gamma, graph=graph,
                                  decoder_input_ids=t5.prompt, return_stats=True)
        assert torch.equal(gotp, t5.plain_prompt), (which, gamma, graph, "prompt")
        print(f"[speculative] {which} gamma {gamma} graph {graph}: {st} prompted {stp}")
        for s, out, P in ((st, got, 1), (stp, gotp, 3)):
            T = out.shape[1] - P
            assert set(s) == {"rounds", "drafted", "accepted"} and all(type(v) is int for v in s.values())
            assert 0 <= s["accepted"] <= s["drafted"] <= s["rounds"] * gamma * t5.ids.shape[0]
            if which == "same":      # every draft agrees: the longest row gains gamma + 1 tokens per round
                assert s["rounds"] == math.ceil(T / (gamma + 1))
            elif which == "other":   # two random permutations agree on an id with probability 1 / 512
                assert s["accepted"] * 4 <= s["drafted"] and s["rounds"] >= T - 2
            else:
                assert 0 < s["accepted"] < s["drafted"]
    plain = t5.m.generate(t5.ids, max_length=T_MAX, assistant_model=a, num_assistant_tokens=gamma)   # (no stats: the tensor alone)
    assert torch.is_tensor(plain) and torch.equal(plain, t5.plain)


@pytest.mark.parametrize("which", ["same", "half"])
def test_rope_at_one_row_equals_plain_greedy(rope, which):
    a = rope.assistants[which]
    for graph in (False, True):
        got = rope.m.generate(rope.ids, max_length=T_MAX, assistant_model=a, num_assistant_tokens=4, graph=graph)
        assert torch.equal(got, rope.plain), (which, graph)
        got = rope.m.generate(rope.ids, max_length=T_MAX, assistant_model=a, num_assistant_tokens=4, graph=graph,
                              decoder_input_ids=rope.prompt)
        assert torch.equal(got, rope.plain_prompt), (which, graph, "prompt")


def _loop(m, ids, prompt, gamma, drafter, assistant=None):
    """the rounds of `generate(assistant_model=...)` driven from outside through the public pieces: `drafter(lens) -> (B, gamma)`
    scripts the drafts (None: the assistant drafts); returns the raw labels, the final lengths and per-round counters"""
    from flasht5_amd import speculative_round
    from flasht5_amd.speculative import draft_tokens
    B, P = prompt.shape
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
    rounds = []
    while not bool(seen.all()):
        live = (~seen).cpu()
        if drafter is not None:
            draft.copy_(drafter(state.cache_seqlens.cpu()))
        else:
            draft_tokens(assistant, dstate, tok, draft)
        na, nn = speculative_round(m, state, tok, draft, labels, seen, P - 1 + T_MAX, draft_state=dstate)
        rounds.append((live, na.cpu(), nn.cpu()))
        assert len(rounds) <= T_MAX
        if dstate is not None:
            assert torch.equal(dstate.cache_seqlens, state.cache_seqlens)
    return labels, state.cache_seqlens.cpu(), rounds


@pytest.mark.parametrize("gamma", [1, 4])
def test_scripted_drafts_through_speculative_round(t5, gamma):
    from flasht5_amd.generation import finish_labels
    m, P = t5.m, 3
    V = m.config.vocab_size
    want = t5.plain_prompt
    T = want.shape[1] - P
    # the greedy continuation of every row, unfinished: one more token than the run under test may produce
    cont = m.generate(t5.ids, max_length=T_MAX + 1, decoder_input_ids=t5.prompt).cpu()
    cont = torch.cat((cont, torch.zeros(cont.shape[0], gamma + 2, dtype=torch.long)), 1)

    def following(lens, shift):   # row b's pending token is column lens[b]: the drafts are the columns behind it
        return torch.stack([(cont[b, int(n) + 1:int(n) + 1 + gamma] + shift) % V for b, n in enumerate(lens)])

    total = torch.tensor([want[b, P:].tolist().index(1) + 1 for b in range(want.shape[0])])   # the tokens every row gains in all
    assert int(total.max()) == T

    labels, lens, rounds = _loop(m, t5.ids, t5.prompt, gamma, lambda lens: following(lens, 0))
    assert torch.equal(finish_labels(labels[:, :P + T]), want)
    assert len(rounds) == math.ceil(T / (gamma + 1))
    done = torch.zeros_like(total)
    for live, na, nn in rounds:   # every round a row takes gamma drafts and the bonus, or what is left of its sequence
        assert torch.equal(nn.long(), (total - done).clamp(max=gamma + 1)), (nn, total, done)
        assert bool((na >= nn - 1).all()) and bool((na <= nn).all()) and bool((na[nn == gamma + 1] == gamma).all())
        done += nn
    assert torch.equal(done, total) and torch.equal(lens.long(), total + P - 1)

    labels, lens, rounds = _loop(m, t5.ids, t5.prompt, gamma, lambda lens: following(lens, 1))
    assert torch.equal(finish_labels(labels[:, :P + T]), want)
    assert len(rounds) == T and all(int(na.sum()) == 0 for _, na, _ in rounds)
    assert all(bool((nn[live] == 1).all()) for live, _, nn in rounds)


def test_non_decisive_model_stays_within_the_logit_bound():
    """random lm_head: a chunk step and a one-row step round differently, so plain greedy is no exact reference.  Along the
    speculative output the teacher-forced logits Z of the training forward must put every produced token within
    2 * 0.02 * max(1, max|Z|) of the row maximum (the decode path's logit bound, once for each side); no position is left out"""
    from flasht5_amd.generation import finish_labels
    LOGIT_BOUND = 0.02
    m = _model("t5_rpe", seed=11).to(DEV).bfloat16()
    other = _model("t5_rpe", seed=12).to(DEV).bfloat16()
    ids = torch.randint(2, m.config.vocab_size, (4, 33), generator=torch.Generator().manual_seed(5)).to(DEV)
    prompt = torch.zeros((4, 1), dtype=torch.long, device=DEV)
    worst = 0.0
    for name, a in (("itself", m), ("other", other)):   # (its own drafter: nearly every draft accepted; another model: nearly none)
        labels, lens, rounds = _loop(m, ids, prompt, 4, None, assistant=a)
        acc, new = sum(int(na.sum()) for _, na, _ in rounds), sum(int(nn.sum()) for _, _, nn in rounds)
        L = int(lens.max())
        with torch.no_grad():
            Z = m.lm_head(m.decoder(labels[:, :L], encoder_hidden_states=m.encoder(ids))).float()   # Z[:, t] chooses column t + 1
        for b in range(4):
            for t in range(int(lens[b])):
                z = Z[b, t]
                gap = float(z.max() - z[labels[b, t + 1]]) / max(1.0, float(z.abs().max()))
                worst = max(worst, gap)
                assert gap <= 2 * LOGIT_BOUND, (name, b, t, gap)
        print(f"[speculative] non-decisive, drafted by {name}: {len(rounds)} rounds, {acc} drafts accepted, {new} tokens, "
              f"worst gap {worst:.3e} of the bound {2 * LOGIT_BOUND:.1e}")
        got = m.generate(ids, max_length=T_MAX, assistant_model=a, num_assistant_tokens=4)
        assert torch.equal(got, finish_labels(labels[:, :L + 1]))
        if name == "itself":
            assert acc >= new // 2, (acc, new)
