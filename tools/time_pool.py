"""Time sequence pooling: B = 32 rows of L = 512 tokens, d = 768, bf16, lengths uniform in [32, 512], the <eos> last in
each row; modes "eos" and "mean", forward and backward.

  kernel: `fat5::seq_pool_fwd` / `fat5::seq_pool_bwd` on the padded layout with seqlens.  `--chain` launches are captured in one
          graph and the graph is replayed `--calls` times between two device events: microseconds per launch, with no host in
          the figure.  Medians over `--rounds` rounds.
  torch:  the formulation the reference uses on the same inputs, forward and backward through autograd, on the host clock around
          one call that ends in a device synchronise (its own synchronisation included: "eos" reads the <eos> counts back).
            "eos":  ids.eq(eos) -> unique_consecutive(mask.sum(1)) checked on the host -> hidden[mask].view(B, -1, d)[:, -1]
            "mean": (hidden * mask).sum(1) / lengths over the padded layout, fp32 accumulation

Both give the same result: the script checks that before it times anything ("eos" bit for bit, "mean" within bf16 rounding).  One
JSON line at the end; `--log` keeps a copy."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import sequence_pool  # noqa: E402
from flasht5_amd.pooling import MODES  # noqa: E402

EOS = 1


def torch_eos(hidden, ids):
    mask = ids.eq(EOS)
    if len(torch.unique_consecutive(mask.sum(1))) > 1:   # (the reference's host check)
        raise ValueError("All examples must have the same number of <eos> tokens.")
    B, _, d = hidden.shape
    return hidden[mask, :].view(B, -1, d)[:, -1, :]


def torch_mean(hidden, valid, lengths):
    return ((hidden.float() * valid.unsqueeze(-1)).sum(1) / lengths.unsqueeze(-1)).to(hidden.dtype)


def device_us(fn, chain, calls, rounds):
    """fn() launched `chain` times inside one graph; microseconds per launch over `calls` replays, one figure per round"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (calls * chain) * 1e3)
    return out


def host_us(fn, calls, rounds):
    """the host clock around one fn() and a synchronise; microseconds per call, one median of `calls` per round"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        out.append(statistics.median(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pool needs the GPU: a CPU run measures nothing")
    B, L, d = a.batch, a.length, a.width
    g = torch.Generator().manual_seed(a.seed)
    lengths = torch.randint(min(32, L), L + 1, (B,), generator=g)
    ids = torch.randint(2, 30000, (B, L), generator=g)
    ids[torch.arange(B), lengths - 1] = EOS
    hidden = torch.randn(B, L, d, generator=g).bfloat16().cuda().requires_grad_(True)
    ids, seqlens = ids.cuda(), lengths.to(torch.int32).cuda()
    valid = torch.arange(L, device="cuda").unsqueeze(0) < seqlens.unsqueeze(1)
    flen = seqlens.float()
    dp = torch.randn(B, d, generator=g).bfloat16().cuda()

    res = dict(tool="time_pool", batch=B, length=L, width=d, dtype="bf16", tokens=int(lengths.sum()), chain=a.chain, calls=a.calls, rounds=a.rounds)
    for mode in ("eos", "mean"):
        ref_fn = (lambda: torch_eos(hidden, ids)) if mode == "eos" else (lambda: torch_mean(hidden, valid, flen))
        pooled, position, found = sequence_pool(hidden, mode, seqlens=seqlens, input_ids=ids, eos_token_id=EOS)
        want = ref_fn()
        (dh,) = torch.autograd.grad(pooled, hidden, dp)
        (dh_want,) = torch.autograd.grad(want, hidden, dp)
        if mode == "eos":
            assert torch.equal(pooled, want) and torch.equal(dh, dh_want) and found.tolist() == [1] * B
        else:
            for got, ref in ((pooled, want), (dh, dh_want)):
                got, ref = got.detach().float(), ref.detach().float()
                assert float((got - ref).abs().max()) <= 2.0 ** -7 * max(float(ref.abs().max()), 1e-6)
        h = hidden.detach()
        code = MODES[mode]
        fwd = device_us(lambda: torch.ops.fat5.seq_pool_fwd(h, None, seqlens, ids if mode == "eos" else None, code, EOS), a.chain, a.calls, a.rounds)
        bwd = device_us(lambda: torch.ops.fat5.seq_pool_bwd(dp, position, None, seqlens, code, B, L), a.chain, a.calls, a.rounds)

        def torch_step():
            torch.autograd.grad(ref_fn(), hidden, dp)

        t_fwd = host_us(lambda: ref_fn(), a.calls, a.rounds)
        t_both = host_us(torch_step, a.calls, a.rounds)
        res[mode] = dict(kernel_fwd_us=round(statistics.median(fwd), 2), kernel_fwd_min_max=[round(min(fwd), 2), round(max(fwd), 2)],
                         kernel_bwd_us=round(statistics.median(bwd), 2), kernel_bwd_min_max=[round(min(bwd), 2), round(max(bwd), 2)],
                         torch_fwd_us=round(statistics.median(t_fwd), 1), torch_fwd_bwd_us=round(statistics.median(t_both), 1))
    line = json.dumps(res)
    print(line, flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
