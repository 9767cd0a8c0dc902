"""Local (window = 127) against full attention: forward and backward of `flash_attention_v2_rpe1d` at (4, 12, S, 64) bf16,
S = 512, 2048, 8192.  Warm-up, device events around `iters` back-to-back calls, the median of `rounds` rounds, the two variants
interleaved round by round.  One JSON line per length:  python tools/bench_local.py [--rounds 7] [--iters 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flasht5_amd import flash_attention_v2_rpe1d  # noqa: E402

B, H, D, RADIUS, WINDOW = 4, 12, 64, 128, 127


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lengths", type=int, nargs="+", default=[512, 2048, 8192])
    args = ap.parse_args()
    for S in args.lengths:
        g = torch.Generator(device="cuda").manual_seed(S)
        # the model's layout: (B, S, H, D) storage viewed as (B, H, S, D)
        q, k, v, do = (torch.randn(B, S, H, D, device="cuda", generator=g).bfloat16().permute(0, 2, 1, 3) for _ in range(4))
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        r1 = (torch.randn(H, 2 * RADIUS + 1, device="cuda", generator=g) * 0.5).requires_grad_()
        fns = {}
        for name, window in (("full", None), ("local", WINDOW)):
            fwd = lambda window=window: flash_attention_v2_rpe1d(q, k, v, r1, RADIUS, False, 0.125, window=window)
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
        med.update(S=S, window=WINDOW, fwd_speedup=round(med["full_fwd_us"] / med["local_fwd_us"], 2),
                   bwd_speedup=round(med["full_bwd_us"] / med["local_bwd_us"], 2), work_ratio=round((2 * WINDOW + 1) / S, 3))
        print(json.dumps(med), flush=True)


if __name__ == "__main__":
    main()
