"""Time one optimizer step over FAT5-base's parameter tensors, in bf16 and in fp32: `flasht5_amd.Adafactor` eagerly and
as one replay of a captured step (`graph_advance()` + replay: what `GraphedTrainStep` pays), against
`transformers.optimization.Adafactor` on the same device and on copies of the same tensors -- the code a user runs today; it
cannot be captured, its `_get_lr` reads RMS(p) on the host -- and, for scale, `AdamWScale`'s eager step.

Alternating blocks: each of 7 rounds times every variant once (device events around `calls` back-to-back steps, host enqueue time
included, all warmed up); reported are the median and min..max of the 7 block means, in milliseconds per step, and the optimizer
state each class holds (sum of `nbytes`).  `--log FILE` keeps a copy of the output."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from transformers.optimization import Adafactor as HFAdafactor  # noqa: E402

from flasht5_amd import Adafactor, AdamWScale, FAT5Config, FAT5ForConditionalGeneration  # noqa: E402

ROUNDS = 7


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n  # ms per step


def state_bytes(opt):
    return sum(v.nbytes for st in opt.state.values() for v in st.values() if torch.is_tensor(v))


def params_like(shapes, dtype, g):
    ps = [torch.nn.Parameter((torch.randn(s, generator=g, device="cuda") * 0.05).to(dtype)) for s in shapes]
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g, device="cuda") * 1e-2).to(dtype)
    return ps


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_adafactor needs the GPU: a CPU run measures nothing")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in FAT5ForConditionalGeneration(FAT5Config()).parameters()]
    numel = sum(torch.Size(s).numel() for s in shapes)
    say(f"FAT5-base: {len(shapes)} parameter tensors, {numel / 1e6:.1f} M elements; ms per optimizer step, median [min .. max] of {ROUNDS} block means")
    for dtype in (torch.bfloat16, torch.float32):
        g = torch.Generator(device="cuda").manual_seed(0)
        sets = {k: params_like(shapes, dtype, g) for k in ("fused", "graph", "hf", "adamw")}
        opts = {"fused": Adafactor(sets["fused"]), "graph": Adafactor(sets["graph"]), "hf": HFAdafactor(sets["hf"]),
                "adamw": AdamWScale(sets["adamw"], lr=1e-3)}
        opts["graph"].init_state()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opts["graph"].step()

        def replay():
            opts["graph"].graph_advance()
            graph.replay()
        variants = {"flasht5_amd.Adafactor eager": (opts["fused"].step, 10), "flasht5_amd.Adafactor graph replay": (replay, 10),
                    "transformers Adafactor eager": (opts["hf"].step, 3), "AdamWScale eager": (opts["adamw"].step, 10)}
        for fn, _ in variants.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, (fn, n) in variants.items():
                times[k].append(timed(fn, n))
        for k, v in times.items():
            say(f"{str(dtype)[6:]:9s}{k:36s} {statistics.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]")
        ok = max(times["flasht5_amd.Adafactor eager"]) < min(times["transformers Adafactor eager"])
        say(f"{str(dtype)[6:]:9s}fused eager min..max wholly below transformers': {ok}")
        say(f"{str(dtype)[6:]:9s}optimizer state: flasht5_amd.Adafactor {state_bytes(opts['fused']) / 2 ** 20:.1f} MiB, transformers Adafactor "
            f"{state_bytes(opts['hf']) / 2 ** 20:.1f} MiB, AdamWScale {state_bytes(opts['adamw']) / 2 ** 20:.1f} MiB "
            f"(parameters {sum(p.nbytes for p in sets['fused']) / 2 ** 20:.1f} MiB)")
        del graph
        opts["graph"].release_captured_step()
        del sets, opts, variants, replay
        torch.cuda.empty_cache()
    if "--log" in sys.argv:
        with open(sys.argv[sys.argv.index("--log") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
