"""A plain-Python restatement of the prompt-lookup drafting rule of speculative greedy decoding (include/fat5.h,
fat5_lookup_draft; flasht5_amd/prompt_lookup.py), the mutants a test of it must tell from the truth, and the case list both test
files use (tests/test_prompt_lookup_cpu.py proves without a GPU that every mutant differs from the restatement on at least one of
these cases; tests/test_prompt_lookup_gpu.py compares the kernel with the restatement on the same cases, exactly: every output is
an integer).  CPU only; nothing here imports the package."""
import zlib

import torch

MUTANTS = (
    "latest_position",      # within one sequence the largest position wins instead of the smallest
    "own_first",            # at equal match length the own sequence beats the source
    "shortest_first",       # the smallest match length >= 1 wins
    "across_seam",          # a match in the own sequence runs on backwards into the end of the source
    "read_past",            # the continuation is read past Ls (into the padding) and past len (into stale labels)
    "pending_from_labels",  # the pending token is labels[b, len] instead of tok[b]
    "frozen_proposes",      # a row with seen_eos set is treated as live
    "m_uncapped",           # the match length is not capped at N
    "filler_zero",          # the draft is filled with 0 instead of tok[b]
    "oov_kept",             # an id outside [0, V) is not cut
)


def lookup_ref(source, src_seqlens, labels, cache_seqlens, tok, seen_eos, gamma, N, V=None, mutant=None):
    """-> (draft (B, gamma) int64, n_proposed (B,) int32), new tensors.  src_seqlens may be None (every row L_src long), V may be
    None (no id is cut)"""
    assert mutant is None or mutant in MUTANTS
    B, L_src = source.shape
    ncols = labels.shape[1]
    draft = torch.zeros((B, gamma), dtype=torch.int64)
    n_proposed = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        ln, pending = int(cache_seqlens[b]), int(tok[b])
        filler = 0 if mutant == "filler_zero" else pending
        draft[b] = filler
        frozen = bool(seen_eos[b]) and mutant != "frozen_proposes"
        if frozen or not 0 <= ln <= ncols - 1:
            continue
        row = [int(t) for t in labels[b]]
        s = row[:ln] + [row[ln] if mutant == "pending_from_labels" else pending]
        Ls = L_src if src_seqlens is None else max(0, min(L_src, int(src_seqlens[b])))
        full = [int(t) for t in source[b]]
        x = full[:Ls]
        cap_n = 10 ** 9 if mutant == "m_uncapped" else N

        def match(seq, e, cap):
            m = 0
            while m < cap and seq[e - m] == s[ln - m]:
                m += 1
            return m

        cands = []   # (m, from the source, e)
        for e in range(0, Ls - 1):
            m = match(x, e, min(cap_n, e + 1, ln + 1))
            if m >= 1:
                cands.append((m, 1, e))
        for e in range(0, ln):
            if mutant == "across_seam":
                m = match(x + s, Ls + e, min(cap_n, Ls + e + 1, ln + 1))
            else:
                m = match(s, e, min(cap_n, e + 1))
            if m >= 1:
                cands.append((m, 0, e))
        if not cands:
            continue
        key = lambda c: (c[0] if mutant != "shortest_first" else -c[0], c[1] if mutant != "own_first" else -c[1],  # noqa: E731
                         -c[2] if mutant != "latest_position" else c[2])
        m, from_source, e = max(cands, key=key)
        if from_source:
            seq = full if mutant == "read_past" else x
        else:
            seq = s + row[ln + 1:] if mutant == "read_past" else s
        cont = seq[e + 1:e + 1 + gamma]
        c = 0
        for t in cont:
            if V is not None and not 0 <= t < V and mutant != "oov_kept":
                break
            c += 1
        for j in range(c):
            draft[b, j] = cont[j]
        n_proposed[b] = c
    return draft, n_proposed


# ------------------------------------------------------------------------------------------------------------------- the cases
NCOLS = 40
NCOLS_BIG = 1100
V = 512
PAD_ID = 7   # the padding of `source` alternates the row's pending token with this id: a scan or a read past Ls finds them


def _row(src, own, tok, frozen=False, length=None, src_len=None):
    """src: the row's valid source tokens; own: labels[b, :len]; length / src_len: what the length vectors hold when it is not
    len(own) / len(src) (values that make no sense included)"""
    return dict(src=list(src), own=list(own), tok=tok, frozen=frozen, length=len(own) if length is None else length,
                src_len=len(src) if src_len is None else src_len)


def _build_cases():
    out = []

    def add(name, rows, gamma=4, N=2, L_src=None, ncols=NCOLS, vocab=V, seqlens=True, random=None):
        if L_src is None:
            L_src = max(len(r["src"]) for r in rows)
        out.append(dict(id=f"{name}-g{gamma}-N{N}-L{L_src}-c{ncols}-V{vocab}-{'lens' if seqlens else 'nolens'}", gamma=gamma, N=N, L_src=L_src,
                        ncols=ncols, V=vocab, seqlens=seqlens, rows=rows, random=random))

    u = [30, 31, 32, 33, 34, 35, 36]   # a source that shares nothing with the own sequences below
    # a match only in the source, only in the own sequence (its continuation ends in the pending token), in both at equal m
    where = [_row([5, 6, 7, 8, 9, 10, 11], [0, 20, 6], 7), _row(u, [0, 5, 6, 7, 8, 5, 6], 7),
             _row([5, 6, 7, 40, 41, 42, 43], [0, 6, 7, 50, 51, 6], 7)]
    for gamma in (1, 4, 15):
        add("where", where, gamma=gamma)
    add("where", where, N=1)
    add("where", where, N=16, seqlens=False)
    # different match lengths: the own sequence wins with 3 against 1, the source with 3 against 2, and at 2 against 2
    add("lengths", [_row([9, 7, 40, 41, 42, 43], [0, 5, 6, 7, 50, 51, 52, 5, 6], 7), _row([5, 6, 7, 40, 41, 42], [0, 9, 6, 7, 50, 5, 6], 7),
                    _row([9, 6, 7, 40, 41, 42], [0, 9, 6, 7, 50, 8, 6], 7)], N=3)
    # several candidates at the same m: the earliest, in the source and in the own sequence; N = 1 with the token everywhere
    many = [_row([6, 7, 10, 6, 7, 11, 6, 7, 12], [0, 9, 6], 7), _row(u, [0, 6, 7, 20, 6, 7, 21, 6], 7),
            _row([7, 7, 7, 8, 7, 9], [0, 7, 3, 7], 7)]
    add("many", many)
    add("many", many, N=1)
    add("many", many, N=3, gamma=15)
    # the only continuation is the last source token; a match at e = Ls - 1 is no candidate (alone, and beside an own match);
    # the rows are shorter than L_src, so what lies behind them is padding
    ends = [_row([30, 31, 6, 7, 99], [0, 9, 6], 7), _row([30, 31, 32, 6, 7], [0, 9, 6], 7),
            _row([30, 31, 32, 6, 7], [0, 6, 7, 50, 51, 6], 7)]
    add("ends", ends, L_src=7)
    add("ends", ends, L_src=7, gamma=1)
    add("ends", ends, L_src=9, gamma=15, N=3)
    # len = 0 (the start token alone), a key shorter than N, and an empty / one-token / two-token source
    add("short", [_row([9, 0, 5, 6, 8, 4, 3], [], 0), _row([9, 0, 5, 6, 8, 4, 3], [0], 5), _row([0, 5, 6, 8, 4, 3, 2], [0, 5], 6)], N=16)
    add("short", [_row([], [0, 5, 6, 5], 6), _row([], [], 0), _row([], [0, 4, 4], 4)], L_src=0, seqlens=False)
    add("short", [_row([6], [0, 6, 9], 6), _row([5], [], 5), _row([0], [0, 4, 4], 4)], L_src=1)
    add("short", [_row([6, 8], [0, 3], 6), _row([5, 5], [], 5), _row([4, 6], [0, 4, 5], 6)], L_src=2, seqlens=False)
    # an id >= V and a negative id inside a continuation, from the source and from the own sequence; the same without a V
    oov = [_row([6, 7, 8, 600, 9, 10], [0, 9, 6], 7), _row([6, 7, -3, 8, 9, 10], [0, 9, 6], 7), _row(u, [0, 6, 7, 8, V, 6], 7)]
    add("oov", oov)
    add("oov", oov, vocab=None)
    add("oov", oov, vocab=601, gamma=15)
    # a frozen row with a perfect match between two live ones
    add("frozen", [where[0], dict(where[2], frozen=True), where[1]])
    # the match length is capped at N: two source positions tie at N = 2 (the earlier wins) though the later one matches 3
    add("cap", [_row([9, 6, 7, 20, 5, 6, 7, 21], [0, 5, 6], 7), _row(u, [0, 9, 6, 7, 20, 5, 6, 7, 21, 5, 6], 7),
                _row([6, 7, 20, 5, 6, 7, 21], [0, 5, 6], 7)])
    # the seam: own position 0 continues the key only if the end of the source is glued in front of it
    add("seam", [_row([50, 51, 4, 5], [6, 30, 31, 5, 6, 40, 4, 5], 6), _row([50, 4, 5, 6], [5, 6, 30, 31, 4], 5),
                 _row([4, 5], [6, 30, 6, 31, 4, 5], 6)], N=3)
    # lengths that make no sense: nothing is proposed and nothing is read; src_seqlens below 0 and beyond L_src are clamped
    add("garbage", [_row(where[0]["src"], [0, 20, 6], 7, length=-5), _row(where[0]["src"], [0, 20, 6], 7, length=NCOLS),
                    _row(where[0]["src"], [0, 20, 6], 7, length=NCOLS + 100)])
    add("garbage-src", [_row([5, 6, 7, 8], [0, 20, 6], 7, src_len=-3), _row([5, 6, 7, 8, 9, 10, 11], [0, 20, 6], 7, src_len=10 ** 6),
                        _row([5, 6, 7], [0, 20, 6, 7, 21, 6], 7, src_len=-2 ** 31)], L_src=7)
    add("full", [_row(u, [0] + [3 + (i * i) % 5 for i in range(NCOLS - 2)], 4), _row(u, [0] * (NCOLS - 1), 0, length=NCOLS - 1),
                 _row([3, 4, 5, 6, 7, 8, 9], [0, 3], 4, length=NCOLS)], gamma=15, N=16)
    # random rows over a small alphabet: many matches of every length; long sources take several passes of the workgroup, with
    # a ragged tail, and the key is planted near the end of one row so that the winner lies in a late pass
    for L_src, ncols, gamma, N, seqlens in ((7, NCOLS, 4, 2, True), (600, NCOLS, 4, 3, True), (600, NCOLS, 15, 16, False),
                                            (4099, NCOLS, 4, 16, True), (4099, NCOLS, 1, 1, False), (4099, NCOLS_BIG, 15, 3, True),
                                            (600, NCOLS_BIG, 4, 16, False), (2, NCOLS_BIG, 15, 2, True)):
        add("random", None, gamma=gamma, N=N, L_src=L_src, ncols=ncols, seqlens=seqlens, random=True)
    return out


CASES = _build_cases()


def _random_rows(case, g):
    L_src, ncols, N = case["L_src"], case["ncols"], case["N"]
    rows = []
    for b in range(3):
        alphabet = (3, 4, 24)[b]   # (24: long matches are rare, so the planted key below is the winner)
        length = int(torch.randint(ncols // 2, ncols, (1,), generator=g)) if b else ncols - 1
        own = [0] + [int(t) for t in torch.randint(2, 2 + alphabet, (length - 1,), generator=g)]
        tok = int(torch.randint(2, 2 + alphabet, (1,), generator=g))
        Ls = L_src if not case["seqlens"] or b == 0 else int(torch.randint(L_src // 2, L_src + 1, (1,), generator=g))
        src = [int(t) for t in torch.randint(2, 2 + alphabet, (Ls,), generator=g)]
        if b == 2 and Ls >= 40:   # the last min(N, 8) tokens of the own sequence, pending token included, two positions before the end
            key = (own + [tok])[-min(N, 8):]
            src[Ls - 2 - len(key):Ls - 2] = key
        rows.append(_row(src, own, tok))
    return rows


def inputs(case):
    """the call of `case` as CPU tensors: source (B, L_src), src_seqlens ((B,) int32 or None), labels (B, ncols), cache_seqlens,
    tok, seen_eos.  What lies behind a row's length is never neutral: the padding of source alternates the pending token with
    PAD_ID, labels goes on with ids a wrong read would propose"""
    g = torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))
    rows = _random_rows(case, g) if case["random"] else case["rows"]
    B, L_src, ncols = len(rows), case["L_src"], case["ncols"]
    source = torch.zeros((B, L_src), dtype=torch.int64)
    labels = torch.randint(2, 100, (B, ncols), generator=g)
    lens = torch.zeros((B,), dtype=torch.int32)
    src_lens = torch.zeros((B,), dtype=torch.int32)
    tok = torch.zeros((B,), dtype=torch.int64)
    seen = torch.zeros((B,), dtype=torch.bool)
    for b, r in enumerate(rows):
        n = len(r["src"])
        assert n <= L_src and len(r["own"]) <= ncols and (case["seqlens"] or n == L_src), case["id"]
        source[b, :n] = torch.tensor(r["src"], dtype=torch.int64)
        source[b, n::2] = r["tok"]
        source[b, n + 1::2] = PAD_ID
        labels[b, :len(r["own"])] = torch.tensor(r["own"], dtype=torch.int64)
        lens[b] = r["length"]
        src_lens[b] = max(-2 ** 31, min(2 ** 31 - 1, r["src_len"]))
        tok[b] = r["tok"]
        seen[b] = r["frozen"]
    return dict(source=source, src_seqlens=src_lens if case["seqlens"] else None, labels=labels, cache_seqlens=lens, tok=tok, seen_eos=seen)


def reference(case, ln, mutant=None):
    return lookup_ref(ln["source"], ln["src_seqlens"], ln["labels"], ln["cache_seqlens"], ln["tok"], ln["seen_eos"], case["gamma"],
                      case["N"], case["V"], mutant)


def same(x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


# --------------------------------------------------------------------------------------------- the loop of `generate`, on the CPU
def simulate_generate(sigma, input_ids, src_lens, prompt, max_length, gamma, N, eos=1, accept=None):
    """`generate(prompt_lookup_num_tokens=gamma, max_matching_ngram_size=N)` for a model whose next token is sigma[current token]
    (a permutation chain), with `lookup_ref` for the lookup kernel and `accept` (tests/spec_ref.py's accept_ref; None: the same
    rule written out here) for the verification -> (raw labels (B, P + max_length), lengths, dict(rounds, drafted, accepted))"""
    B, P = prompt.shape
    Vn = len(sigma)
    labels = torch.zeros((B, P + max_length), dtype=torch.int64)
    labels[:, :P] = prompt
    tok = prompt[:, P - 1].clone()
    lens = torch.full((B,), P - 1, dtype=torch.int32)
    seen = torch.zeros((B,), dtype=torch.bool)
    limit = P - 1 + max_length
    stats = dict(rounds=0, drafted=0, accepted=0)
    for _ in range(max_length):
        draft, n_prop = lookup_ref(input_ids, src_lens, labels, lens, tok, seen, gamma, N, Vn)
        live = ~seen
        chunk = torch.cat((tok.unsqueeze(1), draft), 1)
        logits = torch.zeros((B, gamma + 1, Vn))
        logits.scatter_(2, sigma[chunk].unsqueeze(2), 1.0)   # the target's choice after chunk row i is sigma[chunk[i]]
        if accept is not None:
            r = accept(logits, draft, lens + (gamma + 1), labels, tok, seen, limit, None, eos)
            labels, tok, lens, seen, n_acc = r["labels"], r["tok"], r["cache_seqlens"], r["seen_eos"], r["n_accepted"]
        else:
            n_acc = torch.zeros((B,), dtype=torch.int32)
            for b in range(B):
                if seen[b]:
                    continue
                a = [int(sigma[t]) for t in chunk[b]]
                n = 0
                while n < gamma and a[n] == int(draft[b, n]):
                    n += 1
                cand = [int(t) for t in draft[b, :n]] + [a[n]]
                if eos in cand:
                    cand = cand[:cand.index(eos) + 1]
                old = int(lens[b])
                cand = cand[:max(0, limit - old)]
                for j, t in enumerate(cand):
                    labels[b, old + 1 + j] = t
                lens[b] = old + len(cand)
                if cand:
                    tok[b] = cand[-1]
                if (cand and cand[-1] == eos) or old + len(cand) >= limit:
                    seen[b] = True
                n_acc[b] = min(n, len(cand))
        stats["rounds"] += 1
        stats["drafted"] += int(n_prop[live].sum())
        stats["accepted"] += int(torch.minimum(n_acc, n_prop)[live].sum())
        if bool(seen.all()):
            break
    return labels, lens, stats


def greedy_chain(sigma, prompt, max_length, eos=1):
    """plain greedy `generate` for the same model, finished as `finish_labels` does: (B, P + steps)"""
    B, P = prompt.shape
    labels = torch.zeros((B, P + max_length), dtype=torch.int64)
    labels[:, :P] = prompt
    tok = prompt[:, P - 1].clone()
    seen = torch.zeros((B,), dtype=torch.bool)
    steps = 0
    for t in range(max_length):
        tok = sigma[tok]
        labels[:, P + t] = tok
        seen |= tok == eos
        steps += 1
        if bool(seen.all()):
            break
    return finish(labels[:, :P + steps], eos)


def finish(labels, eos=1):
    labels = labels.clone()
    labels[:, -1] = eos
    first = (labels == eos).long().argmax(-1, keepdim=True)
    keep = torch.arange(labels.shape[1]).unsqueeze(0) <= first
    return labels.masked_fill(~keep, 0)
