"""Sampling benchmark: the one-launch sampler (fat5_sample_logits) and sampled generation.

Kernel alone, bf16 logits, B in {1, 16, 64} x V in {32128, 250112} x {top_k = 50; top_p = 0.9; both}, temperature 0.7;
graph-replayed, device-event timed after a warm-up.  Bytes = B V 2 (the row read once; every later pass of a register-resident row
reads registers, a longer row re-reads L2).  Beside it, on the same logits: `logits.argmax(-1)` and a torch-eager restatement of
HF's warpers (temperature, top-k via topk, top-p via sort + softmax + cumsum + scatter, softmax, multinomial), both graph-replayed.

End to end, FAT5-base in bf16, L_enc = 512, 64 new tokens forced (no early stop), B in {1, 16, 64}: ms per token of graph-replayed
cached decoding, greedy against sampling (temperature 0.7, top_k 50, top_p 0.9) -- the setup of DESIGN section 4.10's end-to-end
row, timed the same way (without generate's per-token host read of the stop flag).  Prints one JSON line at the end."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import sample_logits, FAT5Config, FAT5ForConditionalGeneration  # noqa: E402
from flasht5_amd import generation  # noqa: E402

MODES = {"top_k50": (50, 1.0), "top_p0.9": (0, 0.9), "both": (50, 0.9)}
T = 0.7


def graph_time(fn, it=50):
    """mean device time of one replay of `fn` captured in a graph (after an eager warm-up)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def ev_time(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3


def eager_sample(logits, k, p):
    """HF's warpers restated in torch eager, then multinomial"""
    x = logits.float() / T
    if k:
        kth = torch.topk(x, k, dim=-1).values[:, -1:]
        x = x.masked_fill(x < kth, -float("inf"))
    if p < 1.0:
        sx, si = torch.sort(x, dim=-1)
        cum = sx.softmax(-1).cumsum(-1)
        rm = cum <= 1 - p
        rm[:, -1] = False
        x = x.scatter(1, si, sx.masked_fill(rm, -float("inf")))
    return torch.multinomial(x.softmax(-1), 1)[:, 0]  # (torch's default generator: the one a graph capture can advance)


def kernel_rows():
    rows = {}
    for B in (1, 16, 64):
        for V in (32128, 250112):
            logits = torch.randn(B, V, device="cuda").bfloat16() * 3
            offs = torch.arange(B, dtype=torch.int32, device="cuda")
            t_arg = graph_time(lambda: logits.argmax(-1))
            for name, (k, p) in MODES.items():
                t_s = graph_time(lambda: sample_logits(logits, T, k, p, seed=1, offsets=offs))
                t_e = graph_time(lambda: eager_sample(logits, k, p))
                key = f"B{B}_V{V}_{name}"
                rows[key] = {"sample_us": round(t_s * 1e6, 2), "GBs": round(B * V * 2 / t_s / 1e9, 1),
                             "argmax_us": round(t_arg * 1e6, 2), "eager_us": round(t_e * 1e6, 2),
                             "speedup_vs_eager": round(t_e / t_s, 2)}
                print(f"B={B:3d} V={V:6d} {name:9s}: sampler {t_s * 1e6:8.2f} us ({B * V * 2 / t_s / 1e9:6.1f} GB/s) | "
                      f"argmax {t_arg * 1e6:7.2f} us | eager warpers + multinomial {t_e * 1e6:8.2f} us ({t_e / t_s:5.1f}x)",
                      flush=True)
    return rows


def e2e_rows(new_tokens=64, L_enc=512):
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).cuda().bfloat16().eval()
    rows = {}
    sampling = (T, 50, 0.9, 1234)
    for B in (1, 16, 64):
        ids = torch.randint(2, 32768, (B, L_enc), device="cuda")
        out = {}
        with torch.no_grad():
            def cached(step):
                state = model.init_decode_state(ids, max_length=new_tokens)
                labels = torch.zeros((B, state.capacity), dtype=torch.long, device="cuda")
                tok = torch.zeros((B,), dtype=torch.long, device="cuda")
                eos = torch.zeros((B,), dtype=torch.bool, device="cuda")
                step(model, state, tok, labels, eos)  # (step 0 eager, as generate does)
                g = generation._capture_call(lambda: step(model, state, tok, labels, eos))
                torch.cuda.synchronize()
                return ev_time(lambda: [g.replay() for _ in range(new_tokens - 1)]) / (new_tokens - 1)

            def sample_step(model, state, tok, labels, eos):
                generation._step(model, state, tok, labels, eos, sampling=sampling)

            cached(generation._step)  # warm-up
            for rep in range(3):  # (alternated: greedy, sampling, greedy, ...)
                out.setdefault("greedy_ms", []).append(cached(generation._step) * 1e3)
                out.setdefault("sample_ms", []).append(cached(sample_step) * 1e3)
        g_ms, s_ms = min(out["greedy_ms"]), min(out["sample_ms"])
        rows[f"B{B}"] = {"greedy_ms_per_token": round(g_ms, 4), "sample_ms_per_token": round(s_ms, 4),
                         "overhead_pct": round((s_ms / g_ms - 1) * 100, 2),
                         "greedy_all": [round(v, 4) for v in out["greedy_ms"]], "sample_all": [round(v, 4) for v in out["sample_ms"]]}
        print(f"B={B:3d}: greedy {g_ms:.4f} ms/token, sampling {s_ms:.4f} ms/token ({(s_ms / g_ms - 1) * 100:+.2f} %)", flush=True)
    return rows


if __name__ == "__main__":
    res = {"kernel": kernel_rows()}
    if "--kernel-only" not in sys.argv:
        res["end_to_end"] = e2e_rows()
    print(json.dumps(res))
