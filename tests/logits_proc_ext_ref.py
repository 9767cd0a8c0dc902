"""A plain-torch (CPU, fp32) restatement of the ten logits processors as include/fat5.h states them (fat5_process_logits with its
appended fields), built on tests/logits_proc_ref.py's `process_row`: HF's EncoderRepetitionPenalty, RepetitionPenalty,
NoRepeatNGram, EncoderNoRepeatNGram, NoBadWords, MinLength, MinNewTokensLength, ForcedBOSToken, ForcedEOSToken and SuppressTokens
processors in HF's order, over a fixed-size sequence buffer with a per-row length, a per-row encoder length and a per-row
decoder-prompt length -- plus the greedy / beam loops over them.

    y = process(logits, sequences, lengths, encoder_no_repeat_ngram_size=3, encoder_input_ids=ids, bad_words_ids=[[5, 6]],
                min_new_tokens=4, forced_eos_token_id=1, max_new_tokens=12)
"""
import torch

import beam_ref
import logits_proc_ref as base

NINF = float("-inf")
EOS = base.EOS


def kept_bad_words(bad_words_ids, eos_token_id=1):
    """HF drops a sequence equal to [eos]"""
    return [list(w) for w in (bad_words_ids or []) if list(w) != [eos_token_id]]


def process_row(x, seq, s, V, enc=(), P=1, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, eos_token_id=1,
                suppress_tokens=None, encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0, bad_words_ids=None,
                min_new_tokens=0, forced_bos_token_id=None, forced_eos_token_id=None, max_new_tokens=0):
    """x: (V,) fp32; seq: a list of ints; s: the clamped length; enc: the row's encoder ids (inside its mask); P: its decoder
    prompt length"""
    e = [t if 0 <= t < V else -1 for t in enc]
    tok = [t if 0 <= t < V else -1 for t in seq[:s]]
    # 1. the encoder repetition penalty, on the input values: p = fp32(1 / phi), the division in double as HF forms it
    x1 = x.clone()
    if float(encoder_repetition_penalty) != 1.0:
        p = torch.tensor(1 / float(encoder_repetition_penalty), dtype=torch.float32)
        for t in sorted({t for t in e if t >= 0}):
            x1[t] = x[t] * p if bool(x[t] < 0) else x[t] / p
    # 2, 3, 6. repetition penalty (over the encoder-penalised values), n-grams, min_length
    y = base.process_row(x1, seq, s, V, repetition_penalty, no_repeat_ngram_size, min_length, eos_token_id, None)
    # 4. encoder n-grams
    n = int(encoder_no_repeat_ngram_size)
    if n > 0 and s >= n - 1:
        tail = tok[s - n + 1:s]
        for i in range(0, len(e) - n + 1):
            if e[i:i + n - 1] == tail and e[i + n - 1] >= 0:
                y[e[i + n - 1]] = NINF
    # 5. bad words
    for w in kept_bad_words(bad_words_ids, eos_token_id):
        L = len(w)
        if L == 1 or (s >= L and tok[s - (L - 1):s] == w[:-1]):
            if 0 <= w[-1] < V:
                y[w[-1]] = NINF
    # 7. min_new_tokens
    if s - P < int(min_new_tokens):
        y[eos_token_id] = NINF
    # 8, 9. the forced tokens (the later one decides)
    forced = None
    if forced_bos_token_id is not None and s == 1:
        forced = forced_bos_token_id
    if forced_eos_token_id is not None and s - P == int(max_new_tokens) - 1:
        forced = forced_eos_token_id
    if forced is not None:
        y = torch.full_like(y, NINF)
        y[forced] = 0.0
    # 10. suppress_tokens
    for t in (suppress_tokens if suppress_tokens is not None else []):
        if 0 <= int(t) < V:
            y[int(t)] = NINF
    return y


def process(logits, sequences, lengths, log_softmax=False, lse=None, encoder_input_ids=None, encoder_lengths=None,
            rows_per_encoder_row=1, prompt_length=1, prompt_lengths=None, suppress_tokens=None, **proc):
    """(rows, V) any float dtype -> (rows, V) fp32.  Row r reads encoder row r // rows_per_encoder_row, its first
    clamp(encoder_lengths[...], 0, L_enc) ids, and the prompt length prompt_lengths[r] (prompt_length when None)"""
    x = logits.detach().float().cpu()
    rows, V = x.shape
    if log_softmax:
        x = x - (base.lse_rows(x) if lse is None else lse.float().cpu().view(rows, 1))
    seqs = sequences.cpu().tolist()
    L = sequences.shape[1]
    sup = None if suppress_tokens is None else [int(t) for t in (suppress_tokens.cpu().tolist() if torch.is_tensor(suppress_tokens)
                                                               else suppress_tokens)]
    encs = None if encoder_input_ids is None else encoder_input_ids.cpu().tolist()
    out = torch.empty_like(x)
    for r in range(rows):
        s = min(max(int(lengths[r]), 0), L)
        enc = ()
        if encs is not None:
            er = r // rows_per_encoder_row
            el = len(encs[er]) if encoder_lengths is None else min(max(int(encoder_lengths[er]), 0), len(encs[er]))
            enc = encs[er][:el]
        P = int(prompt_length) if prompt_lengths is None else int(prompt_lengths[r])
        out[r] = process_row(x[r], seqs[r], s, V, enc, P, suppress_tokens=sup, **proc)
    return out


def greedy(next_logits, B, max_length, proc, **ctx):
    """logits_proc_ref.greedy with the ten processors (`proc`) and the call's context (`ctx`: encoder_input_ids, ...)"""
    labels = torch.zeros(B, max_length + 1, dtype=torch.int64)
    seen = torch.zeros(B, dtype=torch.bool)
    steps = 0
    for s in range(1, max_length + 1):
        y = process(next_logits(labels[:, :s]), labels, torch.full((B,), s, dtype=torch.int32), max_new_tokens=max_length, **proc, **ctx)
        nxt = y.argmax(-1)
        labels[:, s] = nxt
        seen |= nxt == EOS
        steps = s
        if bool(seen.all()):
            break
    return labels[:, :steps + 1]


def beam_search(next_logits, B, k, max_length, proc, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                process_fn=None, **ctx):
    """logits_proc_ref.beam_search with the ten processors; `process_fn(logp, seqs, s)` replaces the restatement (the test
    that chains HF's classes by hand passes one)"""
    st = beam_ref.init(B, k, max_length + 1, max_length + 1)
    for s in range(1, max_length + 1):
        seqs = st["running_seqs"].reshape(B * k, -1)
        logp = torch.log_softmax(next_logits(seqs[:, :s]).float().cpu(), -1)
        if process_fn is not None:
            y = process_fn(logp, seqs, s)
        else:
            y = process(logp, seqs, torch.full((B * k,), s, dtype=torch.int32), rows_per_encoder_row=k, max_new_tokens=max_length,
                        **proc, **ctx)
        base.beam_step_normalized(st, y, s, max_length, length_penalty, early_stopping)
        if not beam_ref.keep_going(st, early_stopping):
            break
    R = num_return_sequences
    T = int(st["finished_lens"][:, :R].max())
    return st["finished_seqs"][:, :R].reshape(B * R, -1)[:, :T + 1], st["finished_scores"][:, :R].reshape(B * R)
