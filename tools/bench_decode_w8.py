"""Cached greedy decoding with 16-bit decoder weights against FP8 (e4m3) weights (`weight_dtype="fp8"`), on the same build.

End to end: one decoding step (`generation._step`: decoder pass, lm_head, argmax, bookkeeping) captured in a HIP graph per variant,
L_enc = 512, bf16; FAT5-base at B in {1, 16, 64} and one wide configuration (d_model 2048, d_ff 5120, 32 heads of 64, 24 decoder
layers, 2 encoder layers -- the encoder is not part of a step) at B = 1.  Both graphs are timed in alternating repeats (default, fp8,
default, fp8, ...: REPEATS blocks of ITERS replays each, device events around a block, the cache lengths reset before every block), so
a drift of the clocks hits both alike; reported are the median and the spread (min .. max) of the block means, in ms per token.

Per kernel: `w8_linear` (plain instance), kernel="rows" and kernel="matrix", against `F.linear` in bf16 at (R, K, N) in
{1, 9, 16, 64, 128} x {(768, 2304), (768, 4096), (2048, 768), (768, 32768)}, the three graphs taking turns the same way; the end-to-end
table has a `weight_kernel="matrix"` column at B > 8.  The matrix kernel is accepted against the row kernel of the same run: its
min..max over the blocks must lie wholly below the row kernel's ("below rows" / "below fp8"); GB/s counts the weight bytes (N K, or 2 N K), the scales, x and y.
Writes profiles/decode_w8_bench.log and prints one JSON line at the end.  `--kernel-only` / `--e2e-only` run one half,
`--quick` only FAT5-base at B = 1 of the second.

`--mxfp4` runs the MXFP4 tables instead and writes profiles/decode_w4_bench.log: per launch, the FAT5-base projections
and lm_head at R in {1, 8, 16, 64} with four alternating graphs (F.linear in bf16, w8_linear rows, w8_linear matrix, w4_linear; GB/s
of the MXFP4 column counts N K 17 / 32 weight bytes, x and y), and end to end a FAT5-base step at B in {1, 8, 64} with the columns
default, fp8, fp8 + weight_kernel="matrix" and mxfp4.  No ratio is asserted: the table says what was measured."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, generation, quantize_weight, w8_linear  # noqa: E402
from flasht5_amd import quantize_weight_mxfp4, w4_linear  # noqa: E402

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


def alternate(graphs, befores=None):
    """the block means of every graph, the graphs taking turns block by block -> one list of REPEATS times per graph"""
    befores = befores or [None] * len(graphs)
    times = [[] for _ in graphs]
    for _ in range(REPEATS):
        for t, g, before in zip(times, graphs, befores):
            t.append(block(g, before))
    return times


def fmt(t, unit):
    return f"{statistics.median(t) * unit:9.3f} ({min(t) * unit:9.3f}..{max(t) * unit:9.3f})"


def step_graph(model, ids, weight_dtype, weight_kernel=None):
    """one captured decoding step of a fresh state -> (graph, reset, the tensors the graph uses): `reset` puts the cache lengths
    back to one token"""
    B = ids.shape[0]
    state = model.init_decode_state(ids, max_length=ITERS + 16, weight_dtype=weight_dtype, weight_kernel=weight_kernel)
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
    say("# matrix = weight_dtype='fp8', weight_kernel='matrix' (B > 8: the MFMA kernel in every projection); accepted where its")
    say("# min..max lies wholly below fp8's")
    say("# model        B | default ms median (min..max)     | fp8 ms median (min..max)         | fp8/default | matrix ms median "
        "(min..max)      | matrix/fp8 | below fp8")
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
                if B > 8:
                    gm, rm, sm = step_graph(model, ids, "fp8", "matrix")
                    t16, t8, tm = alternate([g16, g8, gm], [r16, r8, rm])
                else:
                    (t16, t8), tm = alternate([g16, g8], [r16, r8]), None
            m16, m8 = statistics.median(t16), statistics.median(t8)
            rows[f"{name}_B{B}"] = {"default_ms": round(m16 * 1e3, 4), "default_min_ms": round(min(t16) * 1e3, 4),
                                    "default_max_ms": round(max(t16) * 1e3, 4), "fp8_ms": round(m8 * 1e3, 4),
                                    "fp8_min_ms": round(min(t8) * 1e3, 4), "fp8_max_ms": round(max(t8) * 1e3, 4),
                                    "fp8_over_default": round(m8 / m16, 3)}
            line = f"  {name:10s} {B:3d} | {fmt(t16, 1e3)} | {fmt(t8, 1e3)} | {m8 / m16:.3f}"
            if tm is not None:
                mm = statistics.median(tm)
                rows[f"{name}_B{B}"].update(matrix_ms=round(mm * 1e3, 4), matrix_min_ms=round(min(tm) * 1e3, 4),
                                            matrix_max_ms=round(max(tm) * 1e3, 4), matrix_over_fp8=round(mm / m8, 3),
                                            matrix_below_fp8=max(tm) < min(t8))
                line += f"       | {fmt(tm, 1e3)} | {mm / m8:.3f}      | {'yes' if max(tm) < min(t8) else 'NO'}"
                del gm, sm
            say(line)
            del g16, g8, s16, s8
        del model
        torch.cuda.empty_cache()
    return rows


def kernels(say):
    rows = {}
    say("# w8_linear (plain), kernel='rows' and kernel='matrix', against F.linear in bf16; us per call, graph-replayed")
    say("#   R     K      N | F.linear us median (min..max)    GB/s | rows us median (min..max)        GB/s | rows/bf16 | matrix us "
        "median (min..max)      GB/s | matrix/bf16 | matrix/rows | below rows")
    for K, N in ((768, 2304), (768, 4096), (2048, 768), (768, 32768)):
        W = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
        w8, sc = quantize_weight(W)
        for R in (1, 9, 16, 64, 128):
            x = torch.randn(R, K, device="cuda", dtype=torch.bfloat16)
            g16 = capture(lambda: F.linear(x, W))
            g8 = capture(lambda: w8_linear(x, w8, sc))
            gm = capture(lambda: w8_linear(x, w8, sc, kernel="matrix"))
            t16, t8, tm = alternate([g16, g8, gm])
            io = 2 * R * K + 2 * R * N
            n16, n8 = 2 * N * K + io, N * K + 4 * N + io
            m16, m8, mm = statistics.median(t16), statistics.median(t8), statistics.median(tm)
            rows[f"R{R}_K{K}_N{N}"] = {"bf16_us": round(m16 * 1e6, 2), "bf16_GBs": round(n16 / m16 / 1e9, 1), "w8_us": round(m8 * 1e6, 2),
                                       "w8_min_us": round(min(t8) * 1e6, 2), "w8_max_us": round(max(t8) * 1e6, 2),
                                       "w8_GBs": round(n8 / m8 / 1e9, 1), "w8_over_bf16": round(m8 / m16, 3),
                                       "matrix_us": round(mm * 1e6, 2), "matrix_min_us": round(min(tm) * 1e6, 2),
                                       "matrix_max_us": round(max(tm) * 1e6, 2), "matrix_over_bf16": round(mm / m16, 3),
                                       "matrix_over_rows": round(mm / m8, 3), "matrix_below_rows": max(tm) < min(t8)}
            say(f"  {R:3d} {K:5d} {N:6d} | {fmt(t16, 1e6)} {n16 / m16 / 1e9:7.1f} | {fmt(t8, 1e6)} {n8 / m8 / 1e9:7.1f} | {m8 / m16:.3f}"
                f"     | {fmt(tm, 1e6)} {n8 / mm / 1e9:7.1f} | {mm / m16:.3f}       | {mm / m8:.3f}       | "
                f"{'yes' if max(tm) < min(t8) else 'NO'}")
            del g16, g8, gm
    return rows


def kernels_w4(say):
    rows = {}
    say("# per launch, us median (min..max) of graph replays: F.linear bf16 | w8_linear rows | w8_linear matrix | w4_linear (MXFP4) GB/s")
    say("#   R     K      N | bf16                              | fp8 rows                          | fp8 matrix                        "
        "| mxfp4                                GB/s | mxfp4/rows | mxfp4/matrix | mxfp4/bf16")
    for K, N in ((768, 768), (768, 2304), (768, 4096), (2048, 768), (768, 32128)):   # o / cross q, qkv, [wi_0; wi_1], wo, lm_head
        W = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
        w8, sc = quantize_weight(W)
        q4, e8 = quantize_weight_mxfp4(W)
        for R in (1, 8, 16, 64):
            x = torch.randn(R, K, device="cuda", dtype=torch.bfloat16)
            graphs = [capture(lambda: F.linear(x, W)), capture(lambda: w8_linear(x, w8, sc)),
                      capture(lambda: w8_linear(x, w8, sc, kernel="matrix")), capture(lambda: w4_linear(x, q4, e8))]
            t16, t8, tm, t4 = alternate(graphs)
            m16, m8, mm, m4 = (statistics.median(t) for t in (t16, t8, tm, t4))
            n4 = N * K * 17 // 32 + 2 * R * K + 2 * R * N
            rows[f"R{R}_K{K}_N{N}"] = {"bf16_us": round(m16 * 1e6, 2), "rows_us": round(m8 * 1e6, 2), "matrix_us": round(mm * 1e6, 2),
                                       "mxfp4_us": round(m4 * 1e6, 2), "mxfp4_min_us": round(min(t4) * 1e6, 2),
                                       "mxfp4_max_us": round(max(t4) * 1e6, 2), "mxfp4_GBs": round(n4 / m4 / 1e9, 1)}
            say(f"  {R:3d} {K:5d} {N:6d} | {fmt(t16, 1e6)} | {fmt(t8, 1e6)} | {fmt(tm, 1e6)} | {fmt(t4, 1e6)} {n4 / m4 / 1e9:7.1f} | "
                f"{m4 / m8:.3f}      | {m4 / mm:.3f}        | {m4 / m16:.3f}")
            del graphs
    return rows


def e2e_w4(say):
    rows = {}
    say("# ms per token of one graph-replayed greedy FAT5-base step, median (min..max): default (16-bit) | fp8 | fp8 matrix (B > 8) | mxfp4")
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).bfloat16().cuda().eval()
    V = model.lm_head.weight.shape[0]
    for B in (1, 8, 64):
        ids = torch.randint(2, V, (B, L_ENC), device="cuda")
        variants = [(None, None), ("fp8", None)] + ([("fp8", "matrix")] if B > 8 else []) + [("mxfp4", None)]
        with torch.no_grad():
            built = [step_graph(model, ids, wd, wk) for wd, wk in variants]
        times = alternate([b[0] for b in built], [b[1] for b in built])
        med = [statistics.median(t) for t in times]
        names = ["default", "fp8"] + (["matrix"] if B > 8 else []) + ["mxfp4"]
        rows[f"B{B}"] = {f"{n}_ms": round(m * 1e3, 4) for n, m in zip(names, med)}
        rows[f"B{B}"].update(mxfp4_min_ms=round(min(times[-1]) * 1e3, 4), mxfp4_max_ms=round(max(times[-1]) * 1e3, 4))
        say(f"  B {B:3d} | " + " | ".join(f"{n} {fmt(t, 1e3)}" for n, t in zip(names, times)) +
            f" | mxfp4/fp8 {med[-1] / med[1]:.3f} | mxfp4/default {med[-1] / med[0]:.3f}")
        del built
    return rows


def main_w4():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# MXFP4 decoder weights; {REPEATS} alternating blocks of {ITERS} graph replays; {torch.cuda.get_device_name(0)}")
    res = {}
    if "--e2e-only" not in sys.argv:
        res["kernel"] = kernels_w4(say)
    if "--kernel-only" not in sys.argv:
        res["end_to_end"] = e2e_w4(say)
    out = os.environ.get("FAT5_BENCH_LOG", os.path.join(ROOT, "profiles", "decode_w4_bench.log"))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"decode_w4": res}))


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
    main_w4() if "--mxfp4" in sys.argv else main()
