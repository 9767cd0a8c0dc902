"""Speculative decoding benchmark: tokens per second of greedy `generate(graph=True)` against `generate(graph=True,
assistant_model=...)` on the same inputs.

Target: FAT5-base in bf16; drafter: the same configuration with half the layers (encoder and decoder), other weights.  Both are
made decisive (tests/test_speculative_gpu.py's construction: lm_head row sigma(t) is token t's embedding, scaled embeddings, so
the next token is sigma(current token)), and the drafter's permutation agrees with the target's on a chosen share of the ids:
that share controls the acceptance, which a random drafter would leave near zero.  sigma keeps EOS out of every chain, so each
run produces exactly NEW tokens per row.  L_enc = 512, B in {1, 8}, gamma in {2, 4, 8}, agreement in {1.0, 0.8, 0.5}.

Per line: the median and the spread (max - min) of REPS repeats of the whole call, (plain, speculative) alternating inside one
process after a warm-up of both, timed with device events; tokens per second of both; accepted / drafted and the rounds of the
speculative run; and whether the two outputs are equal.  The condition a gain is expected under,
    (gamma + 1) draft steps + one chunk step  <  (mean accepted + 1) target steps,
is reported beside every line from graph replays of the three steps timed on their own (`lhs_ms`, `rhs_ms`).
The log goes to --log (default profiles/speculative_bench.log); one JSON line is printed at the end.

--lookup: the prompt-lookup drafter (`generate(prompt_lookup_num_tokens=gamma)`) instead of the model drafter, on
the same target.  The greedy output is the target's permutation chain from the start token; a chosen share of it (the first
share * 16 tokens of every 16) is written into input_ids, so that share of the output can be copied from the encoder input and
the rest cannot.  B in {1, 8}, gamma in {2, 4, 8}, share in {1.0, 0.5, 0.0}, max_matching_ngram_size 2; the same alternation
with plain greedy `generate(graph=True)`; the lookup launch's own time and both sides of
    one lookup launch + one chunk step  <  (mean accepted + 1) target steps
from graph replays timed alone.  The log goes to profiles/prompt_lookup_bench.log."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration  # noqa: E402
from flasht5_amd.generation import _capture_call, decode_chunk, decode_step, init_decode_state  # noqa: E402

REPS = 5
NEW = 64
L_ENC = 512
EMBED_SCALE = 8.0   # the residual stream is then dominated by the token's embedding: the construction stays decisive at 12 layers

_log = None


def say(line):
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def sigma_without_eos(V, seed):
    """a permutation of the ids with sigma(1) = 1: no other token leads to EOS"""
    s = torch.randperm(V, generator=torch.Generator().manual_seed(seed))
    at = int((s == 1).nonzero()[0])
    s[at], s[1] = s[1].clone(), 1
    return s


def agreeing(sigma, share, seed):
    """a permutation equal to sigma on about `share` of the ids (the others' values rotated among themselves), sigma(1) = 1 kept"""
    out = sigma.clone()
    other = (torch.rand(len(sigma), generator=torch.Generator().manual_seed(seed)) >= share).nonzero()[:, 0]
    other = other[other != 1]
    if len(other) > 1:
        out[other] = sigma[other.roll(1)]
    return out


def decisive(model, sigma):
    with torch.no_grad():
        model.shared.weight.mul_(EMBED_SCALE)
        model.lm_head.weight[sigma] = model.shared.weight


def set_sigma(model, sigma):
    with torch.no_grad():
        model.lm_head.weight[sigma] = model.shared.weight


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def med_spread(ts):
    return statistics.median(ts), max(ts) - min(ts)


def step_times(model, assistant, ids, gamma, it=50):
    """graph replays of one target step, one drafter step and one target chunk step of gamma + 1 rows, in ms (the lengths are
    reset between replays, so every replay sees the same caches)"""
    B = ids.shape[0]
    out = []
    tok = torch.full((B,), 5, dtype=torch.long, device="cuda")
    chunk = torch.full((B, gamma + 1), 5, dtype=torch.long, device="cuda")
    for m, fn in ((model, lambda st: decode_step(model, st, tok)), (assistant, lambda st: decode_step(assistant, st, tok)),
                  (model, lambda st: decode_chunk(model, st, chunk, logits="all"))):
        st = init_decode_state(m, ids, NEW + gamma + 1)
        st.cache_seqlens.fill_(NEW // 2)

        def one(st=st, fn=fn):
            st.steps = 0
            fn(st)
            st.cache_seqlens.fill_(NEW // 2)
        one()
        g = _capture_call(one)
        for _ in range(3):
            g.replay()
        ms, _ = timed(lambda: [g.replay() for _ in range(it)])
        out.append(ms / it)
        del g
    return out


def lookup_time(ids, gamma, ngram, V, it=200):
    """graph replays of the lookup launch alone, in ms: sequences half full, every row live"""
    from flasht5_amd import prompt_lookup_draft
    B = ids.shape[0]
    labels = torch.randint(2, V, (B, 1 + NEW), device="cuda")
    lens = torch.full((B,), NEW // 2, dtype=torch.int32, device="cuda")
    tok = ids[:, 200].clone()
    seen = torch.zeros((B,), dtype=torch.bool, device="cuda")
    draft = torch.zeros((B, gamma), dtype=torch.long, device="cuda")
    one = lambda: prompt_lookup_draft(ids, labels, lens, tok, seen, gamma, ngram, vocab_size=V, out=draft)  # noqa: E731
    one()
    g = _capture_call(one)
    for _ in range(3):
        g.replay()
    ms, _ = timed(lambda: [g.replay() for _ in range(it)])
    del g
    return ms / it


def copy_inputs(sigma, B, V, share, seed):
    """random input_ids with `share` of the greedy output (the chain from the start token 0) written into them, in runs"""
    ids = torch.randint(2, V, (B, L_ENC), generator=torch.Generator().manual_seed(seed))
    t = 0
    for k in range(NEW):
        t = int(sigma[t])
        if k % 16 < round(16 * share):
            ids[:, 100 + k] = t
    return ids.cuda()


def main_lookup(path, quick):
    global _log
    NGRAM = 2
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    _log = open(path, "w")
    base = FAT5Config()
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(base).cuda().bfloat16().eval()
    V = base.vocab_size
    sigma = sigma_without_eos(V, 1000)
    decisive(model, sigma)
    say(f"# prompt lookup: target {base.num_decoder_layers} + {base.num_layers} layers, bf16, L_enc {L_ENC}, {NEW} new tokens, "
        f"max_matching_ngram_size {NGRAM}, graph=True, {REPS} alternating repeats (median, spread = max - min)")
    rows = {}
    with torch.no_grad():
        for B in ((1,) if quick else (1, 8)):
            for gamma in ((4,) if quick else (2, 4, 8)):
                probe = copy_inputs(sigma, B, V, 1.0, B)
                t_step, _, t_chunk = step_times(model, model, probe, gamma)
                t_lookup = lookup_time(probe, gamma, NGRAM, V)
                for share in ((1.0,) if quick else (1.0, 0.5, 0.0)):
                    ids = copy_inputs(sigma, B, V, share, B)
                    plain = lambda: model.generate(ids, max_length=NEW, graph=True)  # noqa: E731
                    spec = lambda: model.generate(ids, max_length=NEW, graph=True, prompt_lookup_num_tokens=gamma,  # noqa: E731
                                                  max_matching_ngram_size=NGRAM, return_stats=True)
                    ref, (got, st) = plain(), spec()   # warm-up of both
                    tp, ts = [], []
                    for _ in range(REPS):
                        tp.append(timed(plain)[0])
                        ts.append(timed(spec)[0])
                    (mp, sp), (ms, ss) = med_spread(tp), med_spread(ts)
                    T = ref.shape[1] - 1
                    mean_acc = st["accepted"] / max(1, st["rounds"] * B)
                    lhs, rhs = t_lookup + t_chunk, (mean_acc + 1) * t_step
                    faster = max(ts) < min(tp)
                    rows[f"B{B}_g{gamma}_c{share}"] = dict(
                        plain_ms=round(mp, 2), plain_spread_ms=round(sp, 2), spec_ms=round(ms, 2), spec_spread_ms=round(ss, 2),
                        plain_tok_s=round(B * T / mp * 1e3, 1), spec_tok_s=round(B * (got.shape[1] - 1) / ms * 1e3, 1),
                        accepted=st["accepted"], drafted=st["drafted"], rounds=st["rounds"], same_tokens=bool(torch.equal(ref, got)),
                        step_ms=round(t_step, 3), lookup_ms=round(t_lookup, 4), chunk_ms=round(t_chunk, 3), lhs_ms=round(lhs, 3),
                        rhs_ms=round(rhs, 3), expected=lhs < rhs, faster=faster)
                    say(f"B={B} gamma={gamma} copy={share:.1f}: plain {mp:8.2f} ms (spread {sp:6.2f}) {B * T / mp * 1e3:8.1f} tok/s | "
                        f"lookup {ms:8.2f} ms (spread {ss:6.2f}) {B * (got.shape[1] - 1) / ms * 1e3:8.1f} tok/s | "
                        f"accepted {st['accepted']} / drafted {st['drafted']} in {st['rounds']} rounds | same tokens {torch.equal(ref, got)} | "
                        f"lookup {t_lookup * 1e3:5.1f} us + chunk = {lhs:6.3f} ms {'<' if lhs < rhs else '>='} (acc+1) steps {rhs:6.3f} ms | "
                        f"{'faster' if faster else 'NOT faster'}")
    say(json.dumps(rows))
    _log.close()


def main():
    global _log
    assert torch.cuda.is_available(), "this benchmark needs the GPU (there is no CPU path)"
    if "--lookup" in sys.argv:
        path = os.path.join(ROOT, "profiles", "prompt_lookup_bench.log")
        if "--log" in sys.argv:
            path = sys.argv[sys.argv.index("--log") + 1]
        return main_lookup(path, "--quick" in sys.argv)
    path = os.path.join(ROOT, "profiles", "speculative_bench.log")
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    _log = open(path, "w")
    quick = "--quick" in sys.argv
    base = FAT5Config()
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(base).cuda().bfloat16().eval()
    torch.manual_seed(1)
    half = FAT5Config(num_layers=base.num_layers // 2, num_decoder_layers=base.num_decoder_layers // 2)
    assistant = FAT5ForConditionalGeneration(half).cuda().bfloat16().eval()
    V = base.vocab_size
    sigma = sigma_without_eos(V, 1000)
    decisive(model, sigma)
    decisive(assistant, sigma)
    say(f"# target {base.num_decoder_layers} + {base.num_layers} layers, drafter {half.num_decoder_layers} + {half.num_layers}, bf16, "
        f"L_enc {L_ENC}, {NEW} new tokens, graph=True, {REPS} alternating repeats (median, spread = max - min)")
    rows = {}
    with torch.no_grad():
        for B in ((1,) if quick else (1, 8)):
            ids = torch.randint(2, V, (B, L_ENC), generator=torch.Generator().manual_seed(B)).cuda()
            for gamma in ((4,) if quick else (2, 4, 8)):
                t_step, t_draft, t_chunk = step_times(model, assistant, ids, gamma)
                for share in ((1.0,) if quick else (1.0, 0.8, 0.5)):
                    set_sigma(assistant, agreeing(sigma, share, 7))
                    plain = lambda: model.generate(ids, max_length=NEW, graph=True)  # noqa: E731
                    spec = lambda: model.generate(ids, max_length=NEW, graph=True, assistant_model=assistant,  # noqa: E731
                                                  num_assistant_tokens=gamma, return_stats=True)
                    ref, (got, st) = plain(), spec()   # warm-up of both
                    tp, ts = [], []
                    for _ in range(REPS):
                        tp.append(timed(plain)[0])
                        ts.append(timed(spec)[0])
                    (mp, sp), (ms, ss) = med_spread(tp), med_spread(ts)
                    T = ref.shape[1] - 1
                    mean_acc = st["accepted"] / max(1, st["rounds"] * B)
                    lhs, rhs = (gamma + 1) * t_draft + t_chunk, (mean_acc + 1) * t_step
                    faster = max(ts) < min(tp)
                    rows[f"B{B}_g{gamma}_a{share}"] = dict(
                        plain_ms=round(mp, 2), plain_spread_ms=round(sp, 2), spec_ms=round(ms, 2), spec_spread_ms=round(ss, 2),
                        plain_tok_s=round(B * T / mp * 1e3, 1), spec_tok_s=round(B * (got.shape[1] - 1) / ms * 1e3, 1),
                        accepted=st["accepted"], drafted=st["drafted"], rounds=st["rounds"], same_tokens=bool(torch.equal(ref, got)),
                        step_ms=round(t_step, 3), draft_step_ms=round(t_draft, 3), chunk_ms=round(t_chunk, 3), lhs_ms=round(lhs, 3),
                        rhs_ms=round(rhs, 3), expected=lhs < rhs, faster=faster)
                    say(f"B={B} gamma={gamma} agree={share:.1f}: plain {mp:8.2f} ms (spread {sp:6.2f}) {B * T / mp * 1e3:8.1f} tok/s | "
                        f"speculative {ms:8.2f} ms (spread {ss:6.2f}) {B * (got.shape[1] - 1) / ms * 1e3:8.1f} tok/s | "
                        f"accepted {st['accepted']} / drafted {st['drafted']} in {st['rounds']} rounds | same tokens {torch.equal(ref, got)} | "
                        f"(g+1) draft + chunk {lhs:6.3f} ms {'<' if lhs < rhs else '>='} (acc+1) steps {rhs:6.3f} ms | "
                        f"{'faster' if faster else 'NOT faster'}")
    say(json.dumps(rows))
    _log.close()


if __name__ == "__main__":
    main()
