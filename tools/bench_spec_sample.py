"""Speculative-sampling benchmark: the verification call alone, and sampled generation end to end.

Verification: `speculative_accept(..., sampling=...)` (fat5_spec_accept_sampled: two launches) at (B, V) = (1, 32128) and
(64, 32128), gamma = 4, bf16, temperature 0.7, top_k 50, top_p 0.9, with and without the drafter's logits; beside it, in the same
run and on the same logits, the greedy `speculative_accept` (fat5_spec_accept: two launches) and ONE `sample_logits` launch over B
rows and over B * (gamma + 1) rows.  The drafter's rows are the target's plus noise (sigma 0.3) and the drafts are drawn from them,
so a round both accepts and rejects.  Every call is captured in a graph together with the reset of the state it rolls back (the
lengths and seen_eos: two small copies, timed alone as `reset`), replayed IT times between device events after a warm-up;
the median and the spread (max - min) of REPS such measurements are reported, in microseconds.

End to end: FAT5-base in bf16 (random weights), L_enc = 512, 64 new tokens, B in {1, 8}, gamma = 4, graph=True:
`generate(do_sample=True)` plain, with the model drafting for itself (`assistant_model=model`: the acceptance a perfect drafter
gets, at the cost of a full-size drafter) and with the prompt lookup (random inputs whose second half repeats the first: sampled
text rarely continues a copy, so few drafts are proposed).  Median and spread of REPS alternating repeats of the whole call, in ms
per produced token and row, with the acceptance beside it.

The log goes to --log (default profiles/spec_sample_bench.log); one JSON line is printed at the end."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, sample_logits, speculative_accept  # noqa: E402
from flasht5_amd.speculative import DRAFT_KEY  # noqa: E402

REPS, IT = 5, 100
NEW, L_ENC, GAMMA = 64, 512, 4
WARP = (0.7, 50, 0.9)

_log = None


def say(line):
    print(line, flush=True)
    if _log is not None:
        _log.write(line + "\n")
        _log.flush()


def replay_us(fn):
    """median and spread of REPS measurements of IT replays of `fn` captured in a graph, in microseconds per replay"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(IT):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / IT * 1e3)
    del g
    return statistics.median(ts), max(ts) - min(ts)


def verification(rows):
    M = GAMMA + 1
    for B, V in ((1, 32128), (64, 32128)):
        g = torch.Generator().manual_seed(B)
        logits = (torch.randn(B, M, V, generator=g) * 3).bfloat16().cuda()
        dl = (logits[:, :GAMMA].float() + 0.3 * torch.randn(B, GAMMA, V, generator=g).cuda()).bfloat16()
        offs = torch.arange(B, dtype=torch.int32, device="cuda")
        draft = torch.stack([sample_logits(dl[:, i], *WARP, seed=7 ^ DRAFT_KEY, offsets=offs + i) for i in range(GAMMA)], 1)
        lens0 = torch.full((B,), 20 + M, dtype=torch.int32, device="cuda")
        lens, dlens = lens0.clone(), lens0.clone()
        labels = torch.zeros(B, 128, dtype=torch.long, device="cuda")
        tok = torch.zeros(B, dtype=torch.long, device="cuda")
        seen = torch.zeros(B, dtype=torch.bool, device="cuda")
        flat = logits.reshape(B * M, V)
        offs_all = torch.arange(B * M, dtype=torch.int32, device="cuda")

        def reset():
            lens.copy_(lens0)
            dlens.copy_(lens0)
            seen.zero_()

        def sampled(with_q):
            reset()
            return speculative_accept(logits, draft, lens, labels, tok, seen, 127, draft_seqlens=dlens, sampling=WARP + (7,),
                                      draft_logits=dl if with_q else None)

        def greedy():
            reset()
            return speculative_accept(logits, draft, lens, labels, tok, seen, 127, draft_seqlens=dlens)
        na, _ = sampled(True)
        na1, _ = sampled(False)
        acc = (float(na.float().mean()), float(na1.float().mean()))
        t = dict(reset=replay_us(reset), sampled_q=replay_us(lambda: sampled(True)), sampled_onehot=replay_us(lambda: sampled(False)),
                 greedy=replay_us(greedy), sample_B=replay_us(lambda: sample_logits(logits[:, 0], *WARP, seed=7, offsets=offs)),
                 sample_BM=replay_us(lambda: sample_logits(flat, *WARP, seed=7, offsets=offs_all)))
        rows[f"verify_B{B}_V{V}"] = {k: (round(v[0], 2), round(v[1], 2)) for k, v in t.items()}
        rows[f"verify_B{B}_V{V}"]["mean_accepted"] = (round(acc[0], 2), round(acc[1], 2))
        say(f"verification B={B} V={V} gamma={GAMMA} bf16 (us, median (spread)): " +
            " | ".join(f"{k} {v[0]:7.2f} ({v[1]:5.2f})" for k, v in t.items()) +
            f" | mean accepted drafts {acc[0]:.2f} with logits, {acc[1]:.2f} one-hot")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def end_to_end(rows, quick):
    base = FAT5Config()
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(base).cuda().bfloat16().eval()
    V = base.vocab_size
    kw = dict(max_length=NEW, graph=True, do_sample=True, temperature=WARP[0], top_k=WARP[1], top_p=WARP[2], seed=11, return_stats=True)
    with torch.no_grad():
        for B in ((1,) if quick else (1, 8)):
            ids = torch.randint(2, V, (B, L_ENC), generator=torch.Generator().manual_seed(B))
            ids[:, L_ENC // 2:] = ids[:, :L_ENC // 2]
            ids = ids.cuda()
            calls = dict(plain=lambda: (model.generate(ids, **{k: v for k, v in kw.items() if k != "return_stats"}), None),
                         self_drafted=lambda: model.generate(ids, assistant_model=model, num_assistant_tokens=GAMMA, **kw),
                         lookup=lambda: model.generate(ids, prompt_lookup_num_tokens=GAMMA, **kw))
            outs = {k: f() for k, f in calls.items()}   # warm-up of all three
            ts = {k: [] for k in calls}
            for _ in range(REPS):
                for k, f in calls.items():
                    ts[k].append(timed(f)[0])
            for k in calls:
                out, st = outs[k]
                toks = int((out[:, 1:] != 0).sum())    # produced tokens over all rows (what follows an EOS is 0)
                med, spread = statistics.median(ts[k]), max(ts[k]) - min(ts[k])
                rows[f"e2e_B{B}_{k}"] = dict(ms=round(med, 2), spread_ms=round(spread, 2), tokens=toks, ms_per_token_row=round(med / (toks / B), 4),
                                             stats=st)
                say(f"end to end B={B} {k:12s}: {med:8.2f} ms (spread {spread:6.2f}), {toks} tokens, {med / (toks / B):7.4f} ms per token and row"
                    + ("" if st is None else f" | accepted {st['accepted']} / drafted {st['drafted']} in {st['rounds']} rounds"))


def main():
    global _log
    assert torch.cuda.is_available(), "this benchmark needs the GPU (there is no CPU path)"
    path = os.path.join(ROOT, "profiles", "spec_sample_bench.log")
    if "--log" in sys.argv:
        path = sys.argv[sys.argv.index("--log") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    _log = open(path, "w")
    say(f"# speculative sampling: temperature {WARP[0]}, top_k {WARP[1]}, top_p {WARP[2]}, gamma {GAMMA}, bf16; graph replays, "
        f"{REPS} repeats (median, spread = max - min)")
    rows = {}
    verification(rows)
    if "--no-e2e" not in sys.argv:
        end_to_end(rows, "--quick" in sys.argv)
    say(json.dumps(rows))
    _log.close()


if __name__ == "__main__":
    main()
