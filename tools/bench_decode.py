"""Decode benchmark: the split-KV decode kernel (fat5_attn_decode) and cached greedy generation.

Kernel alone, H = 12, D = 64, bf16, (B, L, H, D) caches, B in {1, 16, 64}, L in {128, 512, 1024, 4096} keys (the cache holds L - 1
rows and the step appends one), T5 bias on; graph-replayed, device-event timed after a warm-up.  Bytes moved = 2 B H L D 2 (K and V)
+ q and o + the workspace written and read; the fraction is against 8 TB/s (spec) and ~6.3 TB/s (achievable).  Beside it, what a user
could run before: fat5_attn_fwd at M = 1 without bias (the cross-attention shape) and flash_attention_v2_rpe1d causal on M = N = L
(what a cache-less decoder pays per layer for its last row).

End to end, FAT5-base in bf16, L_enc = 512, 64 new tokens forced (no early stop), B in {1, 16, 64}: ms per token and tokens/s of
the reference's recompute algorithm (the whole decoder over every token so far at each step, the encoder output reused as the
reference reuses it; the lm_head on the last row only, which favours it), of cached eager decoding and of cached decoding replayed from a HIP graph.  The cached paths are timed without `generate`'s
per-token host read of the stop flag (one small device-to-host copy and synchronisation per token), so their ms per token is slightly
optimistic against `generate()` as users call it.  Prints one JSON line at the end.
Kernel times: run it under `rocprofv3 --kernel-trace --stats` (tools/README.md)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import flash_attn_with_kvcache, flash_attention_v2_bias, flash_attention_v2_rpe1d  # noqa: E402
from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration  # noqa: E402
from flasht5_amd import generation  # noqa: E402
from flasht5_amd.positional_encoding import rpe1d_from_table  # noqa: E402

SPEC, ACHIEVABLE = 8e12, 6.3e12
H, D, R = 12, 64, 128


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


def ev_time(fn, it=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(it):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def kernel_rows():
    from flasht5_amd import _lib
    rows = {}
    g = torch.Generator().manual_seed(0)
    rpe = rpe1d_from_table(torch.randn(32, H, generator=g) * 0.5, bidirectional=False, num_buckets=32, max_distance=R).cuda()
    for B in (1, 16, 64):
        for L in (128, 512, 1024, 4096):
            kc = torch.randn(B, L, H, D, device="cuda", dtype=torch.bfloat16)
            vc = torch.randn(B, L, H, D, device="cuda", dtype=torch.bfloat16)
            q, kn, vn = (torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16) for _ in range(3))
            lens = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
            t_dec = graph_time(lambda: flash_attn_with_kvcache(q, kc, vc, kn, vn, lens, 0.125, rpe, R))
            p = _lib.DecodeParams()
            p.B, p.H, p.D, p.capacity = B, H, D, L
            ws = _lib.load().fat5_attn_decode_workspace_bytes(p)
            nbytes = 2 * B * H * L * D * 2 + 2 * B * H * D * 2 + 2 * ws
            qh, kh, vh = q.transpose(1, 2), kc.transpose(1, 2), vc.transpose(1, 2)  # (B, H, ., D) views
            t_fwd1 = graph_time(lambda: flash_attention_v2_bias(qh, kh, vh, None, False, 0.125))
            qf = torch.randn(B, H, L, D, device="cuda", dtype=torch.bfloat16)
            t_full = graph_time(lambda: flash_attention_v2_rpe1d(qf, kh, vh, rpe, R, True, 0.125)) if B * L <= 16 * 4096 else None
            rows[f"B{B}_L{L}"] = {
                "decode_us": round(t_dec * 1e6, 2), "GBs": round(nbytes / t_dec / 1e9, 1),
                "frac_spec": round(nbytes / t_dec / SPEC, 3), "frac_achievable": round(nbytes / t_dec / ACHIEVABLE, 3),
                "fwd_m1_us": round(t_fwd1 * 1e6, 2), "causal_full_us": None if t_full is None else round(t_full * 1e6, 2)}
            print(f"B={B:3d} L={L:5d}: decode {t_dec * 1e6:8.2f} us ({nbytes / t_dec / 1e9:7.1f} GB/s, "
                  f"{nbytes / t_dec / ACHIEVABLE:5.1%} of 6.3 TB/s) | fat5_attn_fwd M=1 {t_fwd1 * 1e6:8.2f} us | "
                  f"causal M=N=L {'-' if t_full is None else f'{t_full * 1e6:9.2f} us'}", flush=True)
            del kc, vc, qf
    return rows


def e2e_rows(new_tokens=64, L_enc=512):
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).cuda().bfloat16().eval()
    rows = {}
    for B in (1, 16, 64):
        ids = torch.randint(2, 32768, (B, L_enc), device="cuda")
        out = {}
        with torch.no_grad():
            enc = model.encoder(ids)

            def recompute():
                labels = torch.zeros(B, 1, dtype=torch.long, device="cuda")
                for _ in range(new_tokens):
                    lg = model.lm_head(model.decoder(labels, encoder_hidden_states=enc)[:, -1:])[:, -1]
                    labels = torch.cat([labels, lg.argmax(-1, keepdim=True)], -1)

            def cached(graph):
                state = model.init_decode_state(ids, max_length=new_tokens)
                labels = torch.zeros((B, state.capacity), dtype=torch.long, device="cuda")
                tok = torch.zeros((B,), dtype=torch.long, device="cuda")
                eos = torch.zeros((B,), dtype=torch.bool, device="cuda")
                generation._step(model, state, tok, labels, eos)  # (step 0 eager in both modes, as generate does)
                g = generation._capture_call(lambda: generation._step(model, state, tok, labels, eos)) if graph else None
                torch.cuda.synchronize()
                t = ev_time(lambda: [g.replay() if graph else generation._step(model, state, tok, labels, eos)
                                     for _ in range(new_tokens - 1)])
                return t / (new_tokens - 1)

            recompute()  # warm-up
            out["recompute_ms_per_token"] = ev_time(recompute) / new_tokens * 1e3
            cached(False)
            out["cached_eager_ms_per_token"] = cached(False) * 1e3
            out["cached_graph_ms_per_token"] = cached(True) * 1e3
        for k in list(out):
            out[k.replace("ms_per_token", "tokens_per_s")] = round(B / (out[k] * 1e-3), 1)
            out[k] = round(out[k], 3)
        rows[f"B{B}"] = out
        print(f"B={B:3d}: " + ", ".join(f"{k} {v}" for k, v in out.items()), flush=True)
    return rows


if __name__ == "__main__":
    res = {"kernel": kernel_rows()}
    if "--kernel-only" not in sys.argv:
        res["end_to_end"] = e2e_rows()
    print(json.dumps(res))
