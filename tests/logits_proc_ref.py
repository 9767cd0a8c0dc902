"""A plain-torch (CPU, fp32) restatement of the logits processors as include/fat5.h states them (fat5_process_logits): HF's
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor and SuppressTokensLogitsProcessor in
HF's order, over a fixed-size sequence buffer with a per-row length -- plus a beam step that takes processed log-probabilities
(tests/beam_ref.py's `step` applies log_softmax itself and cannot be fed processed rows) and the greedy / beam loops over them.

    y = process(logits, sequences, lengths, repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=5, suppress_tokens=[3])
"""
import torch

import beam_ref

NEG = beam_ref.NEG
EOS = beam_ref.EOS


def process_row(x, seq, s, V, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, eos_token_id=1, suppress_tokens=None):
    """x: (V,) fp32 (already normalised when the caller wants that); seq: a list of ints; s: the clamped length"""
    y = x.clone()
    tok = [t if 0 <= t < V else -1 for t in seq[:s]]  # (outside the vocabulary: "no token")
    theta = torch.tensor(float(repetition_penalty), dtype=torch.float32)
    if float(repetition_penalty) != 1.0:
        for t in sorted({t for t in tok if t >= 0}):
            y[t] = x[t] * theta if bool(x[t] < 0) else x[t] / theta
    n = int(no_repeat_ngram_size)
    if n > 0 and s >= n:
        tail = tok[s - n + 1:s]
        for i in range(0, s - n + 1):
            if tok[i:i + n - 1] == tail and tok[i + n - 1] >= 0:
                y[tok[i + n - 1]] = float("-inf")
    if s < int(min_length):
        y[eos_token_id] = float("-inf")
    for t in (suppress_tokens if suppress_tokens is not None else []):
        if 0 <= int(t) < V:
            y[int(t)] = float("-inf")
    return y


def lse_rows(x):
    """the kernel's log-sum-exp in fp32 (max + log(sum exp(x - max))); the summation order is the kernel's own, so this agrees
    with it to rounding, and exactly where every partial sum is exact"""
    m = x.max(-1, keepdim=True).values
    return m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))


def process(logits, sequences, lengths, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, eos_token_id=1,
            suppress_tokens=None, log_softmax=False, lse=None):
    """(rows, V) any float dtype -> (rows, V) fp32; `lse` (rows, 1): use these values instead of lse_rows (exactness tests)"""
    x = logits.detach().float().cpu()
    rows, V = x.shape
    if log_softmax:
        x = x - (lse_rows(x) if lse is None else lse.float().cpu().view(rows, 1))
    seqs = sequences.cpu().tolist()
    L = sequences.shape[1]
    sup = None if suppress_tokens is None else [int(t) for t in (suppress_tokens.cpu().tolist() if torch.is_tensor(suppress_tokens)
                                                               else suppress_tokens)]
    out = torch.empty_like(x)
    for r in range(rows):
        s = min(max(int(lengths[r]), 0), L)
        out[r] = process_row(x[r], seqs[r], s, V, repetition_penalty, no_repeat_ngram_size, min_length, eos_token_id, sup)
    return out


def beam_step_normalized(st, logp, s, max_length, length_penalty=1.0, early_stopping=False):
    """beam_ref.step over rows that are log-probabilities already (processed, not renormalised): score = running + logp.
    In place; returns the next tokens (B * k,)"""
    rs = st["running_scores"]
    B, k = rs.shape
    V = logp.shape[-1]
    K = 2 * k
    top = beam_ref._top
    cand = (logp.float().cpu().view(B, k, V) + rs[:, :, None]).reshape(B, k * V)
    ti = top(cand, K)
    score = cand.gather(1, ti)
    parent, tok = ti // V, ti % V
    hits = (tok == EOS) | (s >= max_length)
    v = score + hits.to(torch.float32) * NEG
    ri = top(v, k)
    f = score / (float(s) ** length_penalty)
    full = st["finished_flags"].all(-1, keepdim=True) & (early_stopping is True)
    f = f + full.to(torch.float32) * NEG
    f = f + (~st["heuristic"]).unsqueeze(1).to(torch.float32) * NEG
    did = hits & (torch.arange(K) < k).unsqueeze(0)
    f = f + (~did).to(torch.float32) * NEG
    merged = torch.cat([st["finished_scores"], f], 1)
    fi = top(merged, k)
    run_old, tab_old = st["running_seqs"], st["cache_row_batch"].view(B, k, -1)
    cand_seq = run_old.gather(1, parent[:, :, None].expand(B, K, run_old.shape[2])).clone()
    cand_seq[:, :, s] = tok
    t = s - 1
    new_run = cand_seq.gather(1, ri[:, :, None].expand(B, k, run_old.shape[2]))
    rp = parent.gather(1, ri)
    new_tab = tab_old.gather(1, rp[:, :, None].expand(B, k, tab_old.shape[2])).clone()
    new_tab[:, :, t] = (torch.arange(B).unsqueeze(1) * k + rp).to(torch.int32)
    new_tab[:, :, t + 1:] = tab_old[:, :, t + 1:]
    new_run[:, :, s + 1:] = run_old[:, :, s + 1:]
    m_seq = torch.cat([st["finished_seqs"], cand_seq], 1)
    new_fin = m_seq.gather(1, fi[:, :, None].expand(B, k, m_seq.shape[2]))
    new_fs = merged.gather(1, fi)
    new_ff = torch.cat([st["finished_flags"], did], 1).gather(1, fi)
    new_fl = torch.cat([st["finished_lens"], torch.full((B, K), s, dtype=torch.int32)], 1).gather(1, fi)
    new_rs = v.gather(1, ri)
    hyp = max_length if (early_stopping == "never" and length_penalty > 0.0) else s
    best = new_rs[:, :1] / (hyp ** length_penalty)
    worst = torch.where(new_ff, new_fs.min(1, keepdim=True).values, torch.tensor(NEG))
    heur = st["heuristic"] & (best > worst).any(-1)
    st.update(running_scores=new_rs, running_seqs=new_run, cache_row_batch=new_tab.reshape(B * k, -1), finished_seqs=new_fin,
              finished_scores=new_fs, finished_flags=new_ff, finished_lens=new_fl, heuristic=heur,
              status=(heur.int() | (new_ff.all(1).int() << 1) | (hits.all(1).int() << 2)).to(torch.int32))
    return tok.gather(1, ri).reshape(B * k)


def beam_search(next_logits, B, k, max_length, proc, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                log_softmax=torch.log_softmax):
    """beam_ref.beam_search with the processors `proc` (process' keyword arguments) applied to log_softmax(logits), HF's order"""
    st = beam_ref.init(B, k, max_length + 1, max_length + 1)
    for s in range(1, max_length + 1):
        seqs = st["running_seqs"].reshape(B * k, -1)
        logp = log_softmax(next_logits(seqs[:, :s]).float().cpu(), -1)
        y = process(logp, seqs, torch.full((B * k,), s, dtype=torch.int32), **proc)
        beam_step_normalized(st, y, s, max_length, length_penalty, early_stopping)
        if not beam_ref.keep_going(st, early_stopping):
            break
    R = num_return_sequences
    T = int(st["finished_lens"][:, :R].max())
    return st["finished_seqs"][:, :R].reshape(B * R, -1)[:, :T + 1], st["finished_scores"][:, :R].reshape(B * R)


def greedy(next_logits, B, max_length, proc):
    """the greedy loop of flasht5_amd.generation.generate over a logits callable: (B, steps + 1) int64 before finish_labels"""
    labels = torch.zeros(B, max_length + 1, dtype=torch.int64)
    seen = torch.zeros(B, dtype=torch.bool)
    steps = 0
    for s in range(1, max_length + 1):
        y = process(next_logits(labels[:, :s]), labels, torch.full((B,), s, dtype=torch.int32), **proc)
        nxt = y.argmax(-1)
        labels[:, s] = nxt
        seen |= nxt == EOS
        steps = s
        if bool(seen.all()):
            break
    return labels[:, :steps + 1]
