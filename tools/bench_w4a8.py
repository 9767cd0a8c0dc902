"""The encoder's linears with 16-bit weights against MXFP4 weights on the block-scaled MFMA (W4A8), on the same build.

Per launch, bf16, at the FAT5-base encoder shapes (K, N) in {(768, 2304), (768, 768), (768, 4096), (2048, 768)} and R in
{4096, 32768}: `F.linear` on the 16-bit weight (the library GEMM: today's encoder path), `w4_linear` (the skinny MXFP4 kernel, which
accepts these row counts), `quantize_activation_mxfp8` alone, `w4a8_matmul` alone on rows quantised beforehand, and `w4a8_linear`
(the two launches together).  End to end: one encoder forward of FAT5-base at B x 512 for B in {8, 64}, 16-bit against
`encoder_weight_dtype="mxfp4"`.  Every variant is captured in a HIP graph and the graphs are timed in alternating repeats (REPEATS
blocks of ITERS replays each, device events around a block), so a drift of the clocks hits all alike; reported are the median and
the spread (min .. max) of the block means.  TFLOP/s counts 2 R K N over the median.  No ratio is asserted: the table says what was
measured.  Writes profiles/encoder_w4a8_bench.log (or $FAT5_BENCH_LOG) and prints one JSON line at the end.
`--padded` measures instead the padded encoder pass of generation (16-bit and MXFP4) and one padded `generate` call, eagerly."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, generation  # noqa: E402
from flasht5_amd import quantize_activation_mxfp8, quantize_weight_mxfp4, w4_linear, w4a8_linear, w4a8_matmul  # noqa: E402

REPEATS, ITERS = 7, 20
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


def block(g):
    """the mean time of ITERS runs of g: a captured graph's replays, or a callable's eager calls"""
    run = getattr(g, "replay", g)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e-3


def alternate(graphs):
    """the block means of every graph, the graphs taking turns block by block -> one list of REPEATS times per graph"""
    times = [[] for _ in graphs]
    for _ in range(REPEATS):
        for t, g in zip(times, graphs):
            t.append(block(g))
    return times


def fmt(t, unit):
    return f"{statistics.median(t) * unit:9.2f} ({min(t) * unit:9.2f}..{max(t) * unit:9.2f})"


@torch.no_grad()
def kernels(say):
    rows = {}
    say("# per launch, us median (min..max) of graph replays: F.linear bf16 | w4_linear | quantiser | w4a8_matmul | w4a8_linear (both)")
    say("#     R     K     N | bf16                            TFLOP/s | w4_linear                       | mx8 quantiser                   "
        "| w4a8 GEMM                       TFLOP/s | w4a8 pair                       | pair/bf16 | pair/w4_linear")
    for K, N in ((768, 2304), (768, 768), (768, 4096), (2048, 768)):   # qkv, o, [wi_0; wi_1], wo
        W = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
        q4, e8 = quantize_weight_mxfp4(W)
        for R in (4096, 32768):
            x = torch.randn(R, K, device="cuda", dtype=torch.bfloat16)
            a8, ax = quantize_activation_mxfp8(x)
            graphs = [capture(lambda: F.linear(x, W)), capture(lambda: w4_linear(x, q4, e8)), capture(lambda: quantize_activation_mxfp8(x)),
                      capture(lambda: w4a8_matmul(a8, ax, q4, e8, torch.bfloat16)), capture(lambda: w4a8_linear(x, q4, e8))]
            times = alternate(graphs)
            m16, m4, mq, mg, mp = (statistics.median(t) for t in times)
            flop = 2.0 * R * K * N
            rows[f"R{R}_K{K}_N{N}"] = {"bf16_us": round(m16 * 1e6, 2), "w4_linear_us": round(m4 * 1e6, 2), "quant_us": round(mq * 1e6, 2),
                                       "gemm_us": round(mg * 1e6, 2), "pair_us": round(mp * 1e6, 2),
                                       "pair_min_us": round(min(times[4]) * 1e6, 2), "pair_max_us": round(max(times[4]) * 1e6, 2)}
            say(f"  {R:5d} {K:5d} {N:5d} | {fmt(times[0], 1e6)} {flop / m16 / 1e12:7.1f} | {fmt(times[1], 1e6)} | {fmt(times[2], 1e6)} | "
                f"{fmt(times[3], 1e6)} {flop / mg / 1e12:7.1f} | {fmt(times[4], 1e6)} | {mp / m16:.3f}     | {mp / m4:.3f}")
            del graphs
    return rows


@torch.no_grad()
def e2e(say):
    rows = {}
    say("# ms of one graph-replayed FAT5-base encoder forward at B x 512, median (min..max): 16-bit | encoder_weight_dtype='mxfp4'")
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).bfloat16().cuda().eval()
    model.quantize_encoder_weights_mxfp4()
    V = model.lm_head.weight.shape[0]
    for B in (8, 64):
        ids = torch.randint(2, V, (B, L_ENC), device="cuda")
        graphs = [capture(lambda: generation.encode(model, ids)), capture(lambda: generation.encode(model, ids, None, "mxfp4"))]
        t16, t4 = alternate(graphs)
        m16, m4 = statistics.median(t16), statistics.median(t4)
        rows[f"B{B}"] = {"default_ms": round(m16 * 1e3, 4), "mxfp4_ms": round(m4 * 1e3, 4), "mxfp4_min_ms": round(min(t4) * 1e3, 4),
                         "mxfp4_max_ms": round(max(t4) * 1e3, 4)}
        say(f"  B {B:3d} | default {fmt(t16, 1e3)} | mxfp4 {fmt(t4, 1e3)} | mxfp4/default {m4 / m16:.3f}")
        del graphs
    return rows


@torch.no_grad()
def padded(say):
    """`--padded`: the padded encoder pass of generation and one whole padded `generate`, eagerly (the pass builds its indices from
    the host lengths with two host-to-device copies, which a graph does not capture): REPEATS alternating blocks of ITERS
    `generation.encode` calls at B = 8 x 512 with ragged lengths, device events around a block; then REPEATS
    `generate(graph=True, max_length=32)` calls, a host clock around each call and its synchronise"""
    import time
    say("# ms of one eager padded FAT5-base generation.encode at B 8 x 512 (lengths 512 .. 64), median (min..max): 16-bit | mxfp4")
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).bfloat16().cuda().eval()
    model.quantize_encoder_weights_mxfp4()
    B = 8
    ids = torch.randint(2, model.lm_head.weight.shape[0], (B, L_ENC), device="cuda")
    lens = torch.tensor([L_ENC - 64 * b for b in range(B)], device="cuda")
    mask = torch.arange(L_ENC, device="cuda").unsqueeze(0) < lens.unsqueeze(1)
    pad, _ = generation.check_padding(ids, mask)

    calls = [lambda: generation.encode(model, ids, pad), lambda: generation.encode(model, ids, pad, "mxfp4")]
    for fn in calls:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t16, t4 = alternate(calls)
    say(f"  B {B:3d} | default {fmt(t16, 1e3)} | mxfp4 {fmt(t4, 1e3)}")
    gen = []
    for i in range(REPEATS + 1):   # (the first call is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, attention_mask=mask, max_length=32, graph=True)
        torch.cuda.synchronize()
        if i:
            gen.append(time.perf_counter() - t0)
    say(f"# ms of one padded generate(graph=True, max_length=32) call, {out.shape[1] - 1} steps: {fmt(gen, 1e3)}")
    return {"encode_default_ms": round(statistics.median(t16) * 1e3, 4), "encode_mxfp4_ms": round(statistics.median(t4) * 1e3, 4),
            "generate_ms": round(statistics.median(gen) * 1e3, 4)}


def main():
    log = open(os.environ.get("FAT5_BENCH_LOG", os.path.join(ROOT, "profiles", "encoder_w4a8_bench.log")), "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")   # (line by line: a run that ends early leaves what it measured)
        log.flush()
    say(f"# MXFP4 encoder weights (W4A8); {REPEATS} alternating blocks of {ITERS} graph replays; {torch.cuda.get_device_name(0)}")
    res = {}
    if "--padded" in sys.argv:
        res["padded"] = padded(say)
    else:
        if "--e2e-only" not in sys.argv:
            res["kernel"] = kernels(say)
        if "--kernel-only" not in sys.argv:
            res["end_to_end"] = e2e(say)
    log.close()
    print(json.dumps({"encoder_w4a8": res}))


if __name__ == "__main__":
    main()
