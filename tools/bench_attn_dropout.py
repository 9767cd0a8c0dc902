"""Attention dropout (p = 0.1, the family of csrc/attn_dropout_kernels.h) against the same call at p = 0 (the tuned bodies): forward
and backward of `flash_attention_v2_rpe1d` at (4, 12, S, 64) bf16 with the T5 table, S = 512 and 2048, not causal and causal.
Warm-up, device events around `iters` back-to-back EAGER calls (call times: host path and kernels; at S = 512 the p = 0 calls
are bound by the host path), the median of `rounds` rounds, the two variants interleaved round by round.  Then a FAT5-base
`GraphedTrainStep` replay (B = 4, 1024 encoder + 512 decoder tokens, fuse_norm_linear, AdamWScale: bench.py's cfg5 step) with
attention_dropout_rate 0 and 0.1, the two captured steps interleaved the same way (device time: a replay has no host path).
One JSON line per problem:  python tools/bench_attn_dropout.py [--rounds 7] [--iters 200] [--step-iters 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flasht5_amd import flash_attention_v2_rpe1d  # noqa: E402

B, H, D, RADIUS, P = 4, 12, 64, 128, 0.1


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 2048])
    args = ap.parse_args()
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    for S in args.lengths:
        for causal in (False, True):
            g = torch.Generator(device="cuda").manual_seed(S)
            # the model's layout: (B, S, H, D) storage viewed as (B, H, S, D)
            q, k, v, do = (torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16().permute(0, 2, 1, 3) for _ in range(4))
            q, k, v = (t.requires_grad_() for t in (q, k, v))
            r1 = (torch.randn(H, 2 * RADIUS + 1, device="cuda", generator=g) * 0.5).requires_grad_()
            fns = {}
            for name, kw in (("p0", {}), ("drop", dict(dropout_p=P, dropout_seed=1234, dropout_step=step, dropout_site=0))):
                fwd = lambda kw=kw: flash_attention_v2_rpe1d(q, k, v, r1, RADIUS, causal, 0.125, **kw)
                o = fwd()
                bwd = lambda o=o: torch.autograd.grad(o, (q, k, v, r1), do, retain_graph=True)
                fns[name] = (fwd, bwd)
                for _ in range(3):  # warm-up
                    fwd()
                    bwd()
            torch.cuda.synchronize()
            times = {(n, s): [] for n in fns for s in ("fwd", "bwd")}
            for _ in range(args.rounds):
                for name, (fwd, bwd) in fns.items():
                    times[name, "fwd"].append(timed(fwd, args.iters))
                    times[name, "bwd"].append(timed(bwd, args.iters))
            med = {f"{n}_{s}_us": round(statistics.median(t), 1) for (n, s), t in times.items()}
            med.update(S=S, causal=causal, p=P, fwd_slowdown=round(med["drop_fwd_us"] / med["p0_fwd_us"], 2),
                       bwd_slowdown=round(med["drop_bwd_us"] / med["p0_bwd_us"], 2))
            print(json.dumps(med), flush=True)
    train_steps(args)


def train_steps(args):
    from flasht5_amd import AdamWScale, FAT5Config, FAT5ForConditionalGeneration, GraphedTrainStep
    steps = {}
    for name, rate in (("p0", 0.0), ("drop", P)):
        cfg = FAT5Config(attention_dropout_rate=rate, dropout_seed=1234, fuse_norm_linear=True)
        torch.manual_seed(0)
        m = FAT5ForConditionalGeneration(cfg).cuda().bfloat16()
        fn = GraphedTrainStep(m, AdamWScale(m.parameters(), lr=1e-3, kahan_sum=True, max_grad_norm=1.0), warmup=2)
        ids, labels = torch.randint(0, cfg.vocab_size, (4, 1024), device="cuda"), torch.randint(0, cfg.vocab_size, (4, 512), device="cuda")
        for _ in range(5):  # two eager calls, the capture, two replays
            fn(ids, labels)
        steps[name] = (lambda fn=fn, ids=ids, labels=labels: fn(ids, labels))
    torch.cuda.synchronize()
    times = {n: [] for n in steps}
    for _ in range(args.rounds):
        for name, fn in steps.items():
            times[name].append(timed(fn, args.step_iters) / 1e3)
    med = {f"{n}_step_ms": round(statistics.median(t), 2) for n, t in times.items()}
    med.update(what="FAT5-base GraphedTrainStep replay, B = 4, 1024 + 512 tokens", p=P, step_slowdown=round(med["drop_step_ms"] / med["p0_step_ms"], 2))
    print(json.dumps(med), flush=True)


if __name__ == "__main__":
    main()
