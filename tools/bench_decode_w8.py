"""Cached greedy decoding with 16-bit decoder weights against FP8 (e4m3) weights (`weight_dtype="fp8"`), on the same build.

End to end: one decoding step (`generation._step`: decoder pass, lm_head, argmax, bookkeeping) captured in a HIP graph per variant,
L_enc = 512, bf16; FAT5-base at B in {1, 16, 64} and one wide configuration (d_model 2048, d_ff 5120, 32 heads of 64, 24 decoder
layers, 2 encoder layers -- the encoder is not part of a step) at B = 1.  Both graphs are timed in alternating repeats (default, fp8,
default, fp8, ...: REPEATS blocks of ITERS replays each, device events around a block, the cache lengths reset before every block), so
a drift of the clocks hits both alike; reported are the median and the spread (min .. max) of the block means, in ms per token.

Per kernel: `w8_linear` (plain instance) against `F.linear` in bf16 at (R, K, N) in {1, 16, 64} x {(768, 2304), (768, 4096),
(2048, 768), (768, 32768)}, timed the same way; GB/s counts the weight bytes (N K, or 2 N K), the scales, x and y.
Writes profiles/decode_w8_bench.log and prints one JSON line at the end.  `--kernel-only` / `--e2e-only` run one half,
`--quick` only FAT5-base at B = 1 of the second."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, generation, quantize_weight, w8_linear  # noqa: E402

REPEATS, ITERS = 7, 40
L_ENC = 512


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


def block(g, before=None):
    if before is not None:
        before()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e-3


def alternate(ga, gb, before_a=None, before_b=None):
    ta, tb = [], []
    for _ in range(REPEATS):
        ta.append(block(ga, before_a))
        tb.append(block(gb, before_b))
    return ta, tb


def fmt(t, unit):
    return f"{statistics.median(t) * unit:9.3f} ({min(t) * unit:9.3f}..{max(t) * unit:9.3f})"


def step_graph(model, ids, weight_dtype):
    """one captured decoding step of a fresh state -> (graph, reset, the tensors the graph uses): `reset` puts the cache lengths
    back to one token"""
    B = ids.shape[0]
    state = model.init_decode_state(ids, max_length=ITERS + 16, weight_dtype=weight_dtype)
    labels = torch.zeros((B, state.capacity), dtype=torch.long, device="cuda")
    tok = torch.zeros((B,), dtype=torch.long, device="cuda")
    eos = torch.zeros((B,), dtype=torch.bool, device="cuda")
    generation._step(model, state, tok, labels, eos)   # (step 0 eager, as generate does)
    g = generation._capture_call(lambda: generation._step(model, state, tok, labels, eos))

    def reset():
        state.cache_seqlens.fill_(1)
    # (the graph reads and writes these tensors by address: whoever replays it keeps them alive)
    return g, reset, (state, labels, tok, eos)


def e2e(say):
    rows = {}
    say("# ms per token of one graph-replayed greedy step; default = 16-bit weights (library GEMMs), fp8 = weight_dtype='fp8'")
    say("# model        B | default ms median (min..max)     | fp8 ms median (min..max)         | fp8/default")
    wide = dict(d_model=2048, d_ff=5120, num_heads=32, d_kv=64, num_layers=2, num_decoder_layers=24)
    quick = "--quick" in sys.argv   # (FAT5-base at B = 1 alone)
    for name, cfg, batches in (("FAT5-base", {}, (1,) if quick else (1, 16, 64)),) + (() if quick else (("wide-2048", wide, (1,)),)):
        torch.manual_seed(0)
        model = FAT5ForConditionalGeneration(FAT5Config(**cfg)).bfloat16().cuda().eval()
        V = model.lm_head.weight.shape[0]
        for B in batches:
            ids = torch.randint(2, V, (B, L_ENC), device="cuda")
            with torch.no_grad():
                g16, r16, s16 = step_graph(model, ids, None)
                g8, r8, s8 = step_graph(model, ids, "fp8")
                t16, t8 = alternate(g16, g8, r16, r8)
            m16, m8 = statistics.median(t16), statistics.median(t8)
            rows[f"{name}_B{B}"] = {"default_ms": round(m16 * 1e3, 4), "default_min_ms": round(min(t16) * 1e3, 4),
                                    "default_max_ms": round(max(t16) * 1e3, 4), "fp8_ms": round(m8 * 1e3, 4),
                                    "fp8_min_ms": round(min(t8) * 1e3, 4), "fp8_max_ms": round(max(t8) * 1e3, 4),
                                    "fp8_over_default": round(m8 / m16, 3)}
            say(f"  {name:10s} {B:3d} | {fmt(t16, 1e3)} | {fmt(t8, 1e3)} | {m8 / m16:.3f}")
            del g16, g8, s16, s8
        del model
        torch.cuda.empty_cache()
    return rows


def kernels(say):
    rows = {}
    say("# w8_linear (plain) against F.linear in bf16; us per call, graph-replayed")
    say("#   R     K      N | F.linear us median (min..max)    GB/s | w8_linear us median (min..max)   GB/s | w8/bf16")
    for K, N in ((768, 2304), (768, 4096), (2048, 768), (768, 32768)):
        W = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
        w8, sc = quantize_weight(W)
        for R in (1, 16, 64):
            x = torch.randn(R, K, device="cuda", dtype=torch.bfloat16)
            g16 = capture(lambda: F.linear(x, W))
            g8 = capture(lambda: w8_linear(x, w8, sc))
            t16, t8 = alternate(g16, g8)
            io = 2 * R * K + 2 * R * N
            n16, n8 = 2 * N * K + io, N * K + 4 * N + io
            m16, m8 = statistics.median(t16), statistics.median(t8)
            rows[f"R{R}_K{K}_N{N}"] = {"bf16_us": round(m16 * 1e6, 2), "bf16_GBs": round(n16 / m16 / 1e9, 1), "w8_us": round(m8 * 1e6, 2),
                                       "w8_min_us": round(min(t8) * 1e6, 2), "w8_max_us": round(max(t8) * 1e6, 2),
                                       "w8_GBs": round(n8 / m8 / 1e9, 1), "w8_over_bf16": round(m8 / m16, 3)}
            say(f"  {R:3d} {K:5d} {N:6d} | {fmt(t16, 1e6)} {n16 / m16 / 1e9:7.1f} | {fmt(t8, 1e6)} {n8 / m8 / 1e9:7.1f} | {m8 / m16:.3f}")
            del g16, g8
    return rows


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# FP8 decoder weights; {REPEATS} alternating blocks of {ITERS} graph replays; {torch.cuda.get_device_name(0)}")
    res = {}
    if "--e2e-only" not in sys.argv:
        res["kernel"] = kernels(say)
    if "--kernel-only" not in sys.argv:
        res["end_to_end"] = e2e(say)
    out = os.environ.get("FAT5_BENCH_LOG", os.path.join(ROOT, "profiles", "decode_w8_bench.log"))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"decode_w8": res}))


if __name__ == "__main__":
    main()
