"""Decode kernel with bf16 caches against FP8 (e4m3) caches, on the same build: fat5_attn_decode graph-replayed on the grid of
DESIGN 4.10 -- H = 12, D = 64, bf16 activations, (B, L, H, D) caches, B in {1, 16, 64}, L in {128, 512, 1024, 4096} keys (the cache
holds L - 1 rows and the step appends one), T5 bias on.

Per shape both variants are captured once and then timed in alternating repeats (bf16, fp8, bf16, fp8, ...: REPEATS blocks of ITERS
replays each, device events around a block), so a drift of the clocks hits both alike; reported are the median and the spread
(min .. max) of the block means.  Bytes moved: the K and V rows read (2 B H L D elements of 2 bytes, or of 1 byte plus 2 B H L
fp32 scales), q and o, the workspace written and read; GB/s is bytes / median.  fp8/bf16 below 1 means the FP8 cache is faster.
Writes profiles/decode_fp8_bench.log and prints one JSON line at the end."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import _lib, flash_attn_with_kvcache, quantize_kv  # noqa: E402
from flasht5_amd.positional_encoding import rpe1d_from_table  # noqa: E402

H, D, R = 12, 64, 128
REPEATS, ITERS = 7, 40


def capture(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def block(g):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e-3


def main():
    lines, rows = [], {}
    gen = torch.Generator().manual_seed(0)
    rpe = rpe1d_from_table(torch.randn(32, H, generator=gen) * 0.5, bidirectional=False, num_buckets=32, max_distance=R).cuda()

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# decode kernel, bf16 vs FP8 (e4m3) KV cache; H={H} D={D} bias on; {REPEATS} alternating blocks of {ITERS} graph replays; "
        f"{torch.cuda.get_device_name(0)}")
    say("#   B     L | bf16 us median (min..max)    GB/s | fp8 us median (min..max)     GB/s | fp8/bf16 time | bytes fp8/bf16")
    for B in (1, 16, 64):
        for L in (128, 512, 1024, 4096):
            kc = torch.randn(B, L, H, D, device="cuda", dtype=torch.bfloat16)
            vc = torch.randn(B, L, H, D, device="cuda", dtype=torch.bfloat16)
            (kb, ks), (vb, vs) = quantize_kv(kc), quantize_kv(vc)
            q, kn, vn = (torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16) for _ in range(3))
            lens = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
            g16 = capture(lambda: flash_attn_with_kvcache(q, kc, vc, kn, vn, lens, 0.125, rpe, R))
            g8 = capture(lambda: flash_attn_with_kvcache(q, kb, vb, kn, vn, lens, 0.125, rpe, R, k_scale=ks, v_scale=vs))
            t16, t8 = [], []
            for _ in range(REPEATS):
                t16.append(block(g16))
                t8.append(block(g8))
            p = _lib.DecodeParams()
            p.B, p.H, p.D, p.capacity = B, H, D, L
            ws = _lib.load().fat5_attn_decode_workspace_bytes(p)
            other = 2 * B * H * D * 2 + 2 * ws
            n16 = 2 * B * H * L * D * 2 + other
            n8 = 2 * B * H * L * (D + 4) + other
            m16, m8 = statistics.median(t16), statistics.median(t8)
            rows[f"B{B}_L{L}"] = {"bf16_us": round(m16 * 1e6, 2), "bf16_min_us": round(min(t16) * 1e6, 2), "bf16_max_us": round(max(t16) * 1e6, 2),
                                  "bf16_GBs": round(n16 / m16 / 1e9, 1), "fp8_us": round(m8 * 1e6, 2), "fp8_min_us": round(min(t8) * 1e6, 2),
                                  "fp8_max_us": round(max(t8) * 1e6, 2), "fp8_GBs": round(n8 / m8 / 1e9, 1),
                                  "fp8_over_bf16": round(m8 / m16, 3), "bytes_ratio": round(n8 / n16, 3)}
            say(f"  {B:3d} {L:5d} | {m16 * 1e6:8.2f} ({min(t16) * 1e6:8.2f}..{max(t16) * 1e6:8.2f}) {n16 / m16 / 1e9:7.1f} | "
                f"{m8 * 1e6:8.2f} ({min(t8) * 1e6:8.2f}..{max(t8) * 1e6:8.2f}) {n8 / m8 / 1e9:7.1f} | {m8 / m16:13.3f} | {n8 / n16:.3f}")
            del g16, g8, kc, vc, kb, vb
    out = os.environ.get("FAT5_BENCH_LOG", os.path.join(ROOT, "profiles", "decode_fp8_bench.log"))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"decode_fp8": rows}))


if __name__ == "__main__":
    main()
