"""Rotary position embedding bandwidth benchmark: q | k | v rotated in ONE fat5_rope_apply launch, forward and backward (the
conjugate rotation), bf16, at cfg2's attention shape (4, 512, 12, 64) and at (8, 2048, 16, 128).

Bytes model per pass: read + write of q, k and v (2 * 3 * B * S * H * D * 2 B) plus the two tables once (2 * S * D / 2 * 2 B).
Prints event-timed us (host path included: custom op + ctypes), graph-replayed us (the launches alone, back to back) and the
fraction of 8 TB/s of the graph-replayed time; one JSON line at the end.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` (tools/README.md)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd.rotary import rotary, rotary_tables  # noqa: E402

PEAK = 8e12


def ev(fn, it=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def gv(fn, it=50):
    """the same calls captured in a HIP graph (no Python / ctypes / allocator time between launches)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(it):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def main():
    out = {}
    for B, S, H, D in ((4, 512, 12, 64), (8, 2048, 16, 128)):
        cos, sin, _, _ = rotary_tables(D, S, dtype=torch.bfloat16, device="cuda")
        # the module's layout: (B, S, H, D) projections
        qkv = [torch.randn(B, S, H, D, device="cuda").bfloat16() for _ in range(3)]
        nbytes = 2 * 3 * B * S * H * D * 2 + 2 * S * (D // 2) * 2
        rec = {"bytes": nbytes}
        for name, conj in (("fwd", False), ("bwd", True)):
            fn = lambda: rotary(qkv, cos, sin, None, None, 1, False, conj, None, 0)  # noqa: E731
            te, tg = ev(fn), gv(fn)
            rec.update({f"{name}_us": round(te * 1e6, 1), f"{name}_graph_us": round(tg * 1e6, 1),
                        f"{name}_graph_TBs": round(nbytes / tg / 1e12, 2), f"{name}_frac_8TBs": round(nbytes / tg / PEAK, 3)})
            print(f"rope q|k|v ({B},{S},{H},{D}) bf16 {name}: {te * 1e6:7.1f} us event-timed | graph {tg * 1e6:7.1f} us "
                  f"{nbytes / tg / 1e12:5.2f} TB/s = {nbytes / tg / PEAK:.3f} of 8 TB/s  ({nbytes / 1e6:.1f} MB)", flush=True)
        out[f"rope_{B}x{S}x{H}x{D}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
