"""Transient-global (window = 127, one global key per 16 tokens) against local (window = 127) and full attention: forward and
backward of `flash_attention_v2_rpe1d` at (4, 12, S, 64) bf16, S = 2048, 8192, 16384.  The method of tools/bench_local.py: warm-up,
device events around `iters` back-to-back calls, the median of `rounds` rounds, the three variants interleaved round by round.  The
global keys are given tensors: the operator is timed, not the model's aggregate step.
One JSON line per length:  python tools/bench_tglobal.py [--rounds 7] [--iters 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flasht5_amd import flash_attention_v2_rpe1d  # noqa: E402
from bench_local import timed  # noqa: E402

B, H, D, RADIUS, WINDOW = 4, 12, 64, 128, 127


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lengths", type=int, nargs="+", default=[2048, 8192, 16384])
    args = ap.parse_args()
    for S in args.lengths:
        g = torch.Generator(device="cuda").manual_seed(S)
        # the model's layout: (B, S, H, D) storage viewed as (B, H, S, D)
        mk = lambda n: torch.randn(B, n, H, D, device="cuda", generator=g).bfloat16().permute(0, 2, 1, 3)
        q, k, v, do, gk, gv = mk(S), mk(S), mk(S), mk(S), mk(S // 16), mk(S // 16)
        q, k, v, gk, gv = (t.requires_grad_() for t in (q, k, v, gk, gv))
        r1, g1 = ((torch.randn(H, 2 * RADIUS + 1, device="cuda", generator=g) * 0.5).requires_grad_() for _ in range(2))
        variants = {"full": ({}, (q, k, v, r1)), "local": (dict(window=WINDOW), (q, k, v, r1)),
                    "tglobal": (dict(window=WINDOW, global_kv=(gk, gv), global_rpe1d=g1, global_radius=RADIUS), (q, k, v, gk, gv, r1, g1))}
        fns = {}
        for name, (kw, leaves) in variants.items():
            fwd = lambda kw=kw: flash_attention_v2_rpe1d(q, k, v, r1, RADIUS, False, 0.125, **kw)
            o = fwd()
            bwd = lambda o=o, leaves=leaves: torch.autograd.grad(o, leaves, do, retain_graph=True)
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
        # scores a row visits: the band's 2 w + 1 (interior rows), plus S / 16 global keys
        band, glob = 2 * WINDOW + 1, S // 16
        med.update(S=S, window=WINDOW, global_work_ratio=round(glob / band, 3))
        for s in ("fwd", "bwd"):
            med[f"{s}_cost_over_local"] = round(med[f"tglobal_{s}_us"] / med[f"local_{s}_us"] - 1, 3)
            med[f"{s}_speedup_over_full"] = round(med[f"full_{s}_us"] / med[f"tglobal_{s}_us"], 2)
            med[f"{s}_ps_per_score_local"] = round(med[f"local_{s}_us"] * 1e6 / (B * H * S * band), 3)
            med[f"{s}_ps_per_score_global"] = round((med[f"tglobal_{s}_us"] - med[f"local_{s}_us"]) * 1e6 / (B * H * S * glob), 3)
        print(json.dumps(med), flush=True)


if __name__ == "__main__":
    main()
