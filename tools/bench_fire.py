"""FIRE position-bias benchmark: the HIP producer (fat5_fire_fwd) and its parameter-gradient backward (fat5_fire_bwd) against the
reference formula run eagerly in torch on the same GPU, at H = 12, W = 32, bf16 bias, S in {512, 2048, 8192}.

The eager producer restates the reference's FIRE.apply_fire (src/utils/positional_encoding.py:341-417: fp32 positions, log
transform, Linear(1, W) -> ReLU -> Linear(W, H) over every (i, j), permute, cast to bf16); it is not imported.  Its backward is
autograd's.  Roofline per pass (2 FLOP per FMA, 8 TB/s, 157 TF/s fp32): forward max(H S^2 2 B / 8 TB/s, S^2 (2W + 2HW) / 157 TF/s),
backward max(the same bytes read, S^2 (4HW + 6W) / 157 TF/s).  Prints event-timed us (host path included), graph-replayed us
(launches alone), the fraction of the bound, peak extra memory (torch allocator) and one JSON line at the end.  Kernel times: run
it under `rocprofv3 --kernel-trace --stats` (tools/README.md)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd.fire import FIRE, fire_bwd  # noqa: E402

BW, FL = 8e12, 157.3e12
H, W = 12, 32


def ev(fn, it=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def gv(fn, it=20):
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
    del g
    return s.elapsed_time(e) / it * 1e-3


def eager_fire(m, S):
    """the reference formula, eager torch (fp32), cast to bf16 like FIRE.forward"""
    pos = torch.arange(S, dtype=torch.float32, device="cuda")
    rel = pos[:, None] - pos[None, :]
    thr = torch.abs(m.L_multiplier * m.init_L)
    pn = torch.max(pos, thr)[:, None]
    rel = torch.sign(rel) * torch.log(torch.abs(m.c * rel) + 1)
    pn = torch.log(torch.abs(m.c * pn) + 1) + m.eps
    return m.mlp((rel / pn).unsqueeze(-1)).unsqueeze(0).permute(0, 3, 1, 2).contiguous().to(torch.bfloat16)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del out
    return p


def main():
    torch.manual_seed(0)
    m = FIRE(H, W, 0.1, 128).cuda()
    params = [p for p in m.parameters() if p.requires_grad]
    out = {}
    for S in (512, 2048, 8192):
        P = S * S
        nbytes = H * P * 2
        b_fwd = max(nbytes / BW, P * (2 * W + 2 * H * W) / FL)
        b_bwd = max(nbytes / BW, P * (4 * H * W + 6 * W) / FL)
        rec = {"bytes": nbytes, "fwd_bound_us": round(b_fwd * 1e6, 1), "bwd_bound_us": round(b_bwd * 1e6, 1)}
        fwd = lambda: m.compute_bias(S, S, "cuda", torch.bfloat16)  # noqa: E731
        G = torch.randn(H, S, S, device="cuda").bfloat16()
        f = [t.detach().float().contiguous().reshape(-1) for t in (m.mlp[0].weight, m.mlp[0].bias, m.mlp[2].bias, m.c, m.L_multiplier,
                                                                   m.init_L)]
        w2 = m.mlp[2].weight.detach().float().contiguous()
        bwd = lambda: fire_bwd(G, f[0], f[1], w2, f[2], f[3], f[4], f[5], 1e-6)  # noqa: E731
        te, tg = ev(fwd), gv(fwd)
        be, bg = ev(bwd), gv(bwd)
        rec.update({"fwd_us": round(te * 1e6, 1), "fwd_graph_us": round(tg * 1e6, 1), "fwd_frac_bound": round(b_fwd / tg, 3),
                    "bwd_us": round(be * 1e6, 1), "bwd_graph_us": round(bg * 1e6, 1), "bwd_frac_bound": round(b_bwd / bg, 3),
                    "fwd_peak_extra_MB": round(peak(fwd) / 1e6, 1), "out_MB": round(nbytes / 1e6, 1)})
        # eager reference: forward alone, and forward + autograd backward with the same upstream gradient
        gb = G.unsqueeze(0)
        eager_ok = True
        try:
            with torch.no_grad():
                ee = ev(lambda: eager_fire(m, S), it=5)
            ep = peak(lambda: eager_fire(m, S))

            def eager_fb():
                b = eager_fire(m, S)
                torch.autograd.grad(b, params, gb)
            eb = ev(eager_fb, it=3)
            epb = peak(eager_fb)
            rec.update({"eager_fwd_us": round(ee * 1e6, 1), "eager_fwd_bwd_us": round(eb * 1e6, 1),
                        "eager_fwd_peak_extra_MB": round(ep / 1e6, 1), "eager_fwd_bwd_peak_extra_MB": round(epb / 1e6, 1),
                        "fwd_speedup_vs_eager": round(ee / te, 1)})
        except torch.cuda.OutOfMemoryError:
            eager_ok = False
            torch.cuda.empty_cache()
        print(f"FIRE S={S} H={H} W={W} bf16: fwd {te * 1e6:8.1f} us (graph {tg * 1e6:8.1f}, bound {b_fwd * 1e6:6.1f}: "
              f"{b_fwd / tg:.2f})  bwd {be * 1e6:8.1f} us (graph {bg * 1e6:8.1f}, bound {b_bwd * 1e6:6.1f}: {b_bwd / bg:.2f})  "
              f"peak extra {rec['fwd_peak_extra_MB']} MB (out {rec['out_MB']} MB)"
              + (f"  | eager fwd {rec['eager_fwd_us']:.1f} us, fwd+bwd {rec['eager_fwd_bwd_us']:.1f} us, peak "
                 f"{rec['eager_fwd_peak_extra_MB']} / {rec['eager_fwd_bwd_peak_extra_MB']} MB, fwd speedup {rec['fwd_speedup_vs_eager']}x"
                 if eager_ok else "  | eager: out of memory"), flush=True)
        out[f"fire_S{S}"] = rec
        del G
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
