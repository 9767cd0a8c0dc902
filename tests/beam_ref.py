"""A plain-torch (CPU, fp32) restatement of HF's vectorized beam search (transformers 5.x `GenerationMixin._beam_search`:
_get_top_k_continuations, _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic,
_beam_search_has_unfinished_sequences) with one EOS id (1), decoder prompt = the start token 0, max_new_tokens = max_length, no
logits processors, and the fixed tie order of include/fat5.h (every top-k is a stable descending sort: on an equal score the
lower index wins).  Its state is the beam-step kernel's (flasht5_amd/beam.py BeamState), so a test can feed both the same logits.

    st = init(B, k, seq_len, capacity)
    tokens, amb = step(st, logits, s, max_length, length_penalty, early_stopping)     # s: tokens fed so far (1, 2, ...)
    seqs, scores = beam_search(next_logits, B, k, max_length, ...)                    # the whole loop over a logits callable

`amb[b]` marks a batch item whose step came within `tol` (relative) + `atol` (absolute) of a tie in one of its decisions (the top-K selection, the running
selection, the finished merge, the heuristic): another fp32 evaluation order may decide it differently."""
import torch

EOS = 1
NEG = -1.0e9


def init(B, k, seq_len, capacity):
    rs = torch.full((B, k), NEG, dtype=torch.float32)
    rs[:, 0] = 0.0
    return dict(running_scores=rs, running_seqs=torch.zeros(B, k, seq_len, dtype=torch.int64),
                cache_row_batch=torch.zeros(B * k, capacity, dtype=torch.int32),
                finished_seqs=torch.zeros(B, k, seq_len, dtype=torch.int64), finished_scores=torch.full((B, k), NEG),
                finished_flags=torch.zeros(B, k, dtype=torch.bool), finished_lens=torch.zeros(B, k, dtype=torch.int32),
                heuristic=torch.ones(B, dtype=torch.bool), status=torch.zeros(B, dtype=torch.int32))


def _top(x, n):
    """indices of the n largest entries per row, ties to the lower index"""
    return torch.sort(x, dim=1, descending=True, stable=True).indices[:, :n]


def _near(x, idx, n, tol, atol=0.0, src=None):
    """per row: do the first n + 1 entries of x in the order idx hold two neighbours within tol?  `src` (same shape as x): the
    logits row of each entry -- two equal entries of one row are one logit value, ranked by token everywhere, so not a near-tie"""
    sel = idx[:, :n + 1] if idx.shape[1] > n else idx
    v = x.gather(1, sel)
    if v.shape[1] < 2:
        return torch.zeros(x.shape[0], dtype=torch.bool)
    d = (v[:, :-1] - v[:, 1:]).abs()
    # (two entries that both carry a -1e9 penalty are equal on both sides: the penalty absorbs the rounding of the rest)
    penalised = (v[:, :-1] <= 0.1 * NEG) & (v[:, 1:] <= 0.1 * NEG)
    near = (d <= tol * v[:, :-1].abs().clamp(min=1.0) + atol) & ~penalised
    if src is not None:
        s = src.gather(1, sel)
        near &= ~((d == 0) & (s[:, :-1] == s[:, 1:]))
    return near.any(1)


def step(st, logits, s, max_length, length_penalty=1.0, early_stopping=False, tol=0.0, atol=0.0):
    """one step in place; returns (tokens (B * k,) int64, amb (B,) bool)"""
    rs = st["running_scores"]
    B, k = rs.shape
    V = logits.shape[-1]
    K = 2 * k
    x = logits.float().cpu().view(B, k, V)
    cand = (torch.log_softmax(x, -1) + rs[:, :, None]).reshape(B, k * V)  # (HF's op; the kernel forms x - lse, within an ulp)
    ti = _top(cand, K)
    check = tol > 0 or atol > 0
    row_of = (torch.arange(k * V) // V).unsqueeze(0).expand(B, k * V)
    amb = _near(cand, _top(cand, min(K + 1, k * V)), K, tol, atol, row_of) if check else torch.zeros(B, dtype=torch.bool)
    score = cand.gather(1, ti)
    parent, tok = ti // V, ti % V
    hits = (tok == EOS) | (s >= max_length)
    # running beams (HF: topk_log_probs + hits * -1e9, top k)
    v = score + hits.to(torch.float32) * NEG
    ri = _top(v, k)
    if check:
        amb |= _near(v, _top(v, K), k, tol, atol, parent)
    # finished merge (HF's additions, in HF's order, then cat(old, new) and the top k)
    f = score / (float(s) ** length_penalty)
    full = st["finished_flags"].all(-1, keepdim=True) & (early_stopping is True)
    f = f + full.to(torch.float32) * NEG
    f = f + (~st["heuristic"]).unsqueeze(1).to(torch.float32) * NEG
    did = hits & (torch.arange(K) < k).unsqueeze(0)
    f = f + (~did).to(torch.float32) * NEG
    merged = torch.cat([st["finished_scores"], f], 1)
    fi = _top(merged, k)
    if check:
        amb |= _near(merged, _top(merged, k + K), k, tol, atol / abs(float(s) ** length_penalty))
    # sequences: the K candidates' rows (parent row, token at column s), then the gathers
    run_old, tab_old = st["running_seqs"], st["cache_row_batch"].view(B, k, -1)
    cand_seq = run_old.gather(1, parent[:, :, None].expand(B, K, run_old.shape[2])).clone()
    cand_seq[:, :, s] = tok
    t = s - 1
    new_run = cand_seq.gather(1, ri[:, :, None].expand(B, k, run_old.shape[2]))
    rp = parent.gather(1, ri)
    new_tab = tab_old.gather(1, rp[:, :, None].expand(B, k, tab_old.shape[2])).clone()
    new_tab[:, :, t] = (torch.arange(B).unsqueeze(1) * k + rp).to(torch.int32)
    new_tab[:, :, t + 1:] = tab_old[:, :, t + 1:]  # (columns past t are not touched)
    new_run[:, :, s + 1:] = run_old[:, :, s + 1:]
    m_seq = torch.cat([st["finished_seqs"], cand_seq], 1)
    new_fin = m_seq.gather(1, fi[:, :, None].expand(B, k, m_seq.shape[2]))
    new_fs = merged.gather(1, fi)
    new_ff = torch.cat([st["finished_flags"], did], 1).gather(1, fi)
    new_fl = torch.cat([st["finished_lens"], torch.full((B, K), s, dtype=torch.int32)], 1).gather(1, fi)
    new_rs = v.gather(1, ri)
    # the heuristic at cur_len = s + 1
    hyp = max_length if (early_stopping == "never" and length_penalty > 0.0) else s
    best = new_rs[:, :1] / (hyp ** length_penalty)
    worst = torch.where(new_ff, new_fs.min(1, keepdim=True).values, torch.tensor(NEG))
    cmp = best > worst
    if check:
        amb |= ((best - worst).abs() <= tol * best.abs().clamp(min=1.0) + atol).any(1)
    heur = st["heuristic"] & cmp.any(-1)
    st.update(running_scores=new_rs, running_seqs=new_run, cache_row_batch=new_tab.reshape(B * k, -1), finished_seqs=new_fin,
              finished_scores=new_fs, finished_flags=new_ff, finished_lens=new_fl, heuristic=heur,
              status=(heur.int() | (new_ff.all(1).int() << 1) | (hits.all(1).int() << 2)).to(torch.int32))
    return tok.gather(1, ri).reshape(B * k), amb


def keep_going(st, early_stopping):
    """HF's _beam_search_has_unfinished_sequences over the whole batch"""
    s = st["status"]
    improve = bool((s & 1).ne(0).any())
    full = bool((s & 2).ne(0).all()) and early_stopping is True
    return improve and not full and not bool((s & 4).ne(0).all())


def beam_search(next_logits, B, k, max_length, length_penalty=1.0, early_stopping=False, num_return_sequences=1, tol=0.0,
                atol=0.0):
    """the whole loop: next_logits(prefix (B * k, cur_len) int64) -> (B * k, V) logits of the next position.  Returns
    (sequences (B * R, 1 + T) int64, 0 past each hypothesis's end; scores (B * R,) fp32; ambiguous: any step of any item came
    within tol of a tie)"""
    st = init(B, k, max_length + 1, max_length + 1)
    ambiguous = False
    for s in range(1, max_length + 1):
        prefix = st["running_seqs"][:, :, :s].reshape(B * k, s)
        _, amb = step(st, next_logits(prefix), s, max_length, length_penalty, early_stopping, tol, atol)
        ambiguous = ambiguous or bool(amb.any())
        if not keep_going(st, early_stopping):
            break
    R = num_return_sequences
    T = int(st["finished_lens"][:, :R].max())
    return st["finished_seqs"][:, :R].reshape(B * R, -1)[:, :T + 1], st["finished_scores"][:, :R].reshape(B * R), ambiguous
