"""Chunk decode benchmark: one fat5_attn_decode_chunk launch of M query rows against (a) M graph-replayed one-row launches (the only
cached path before the chunk kernel) and (b) the training forward at M x L; and `generate` with a 32-token decoder prompt against a
prefill by 31 `decode_step`s.

Kernel: H = 12, D = 64, bf16, (B, L, H, D) caches, T5 bias, append; B in {1, 16, 64}, L in {128, 512, 1024} keys after the append (the
cache holds L - M rows), M in {2, 4, 8, 16, 64}.  Every figure is a graph replay timed with device events after a warm-up, taken
REPS times with (chunk, one-row) alternating inside one process; the table gives the median and the spread (max - min) of each, and
`faster` says whether the chunk's slowest repeat beats the one-row path's fastest one.  (b) reads host-side lengths and does not
append, so it is a comparison of the attention arithmetic only.
End to end: FAT5-base in bf16, L_enc = 512, B in {1, 16}, a 32-token prompt and 32 new tokens: the time until the first new token's
logits exist, prefilled by one `decode_chunk` of 31 tokens or by 31 eager `decode_step`s, and the whole `generate` call.
Prints one JSON line at the end."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import flash_attn_with_kvcache, flash_attn_with_kvcache_chunk, flash_attention_v2_rpe1d  # noqa: E402
from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration  # noqa: E402
from flasht5_amd.positional_encoding import rpe1d_from_table  # noqa: E402

H, D, R = 12, 64, 128
REPS = 5


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


def replay_time(g, it):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def med_spread(ts):
    return statistics.median(ts), max(ts) - min(ts)


def kernel_rows(Bs, Ls, Ms, it):
    rows = {}
    gen = torch.Generator().manual_seed(0)
    rpe = rpe1d_from_table(torch.randn(32, H, generator=gen) * 0.5, bidirectional=False, num_buckets=32, max_distance=R).cuda()
    rn = lambda *s: torch.randn(*s, device="cuda", dtype=torch.bfloat16)  # noqa: E731
    for B in Bs:
        for L in Ls:
            for M in Ms:
                kc, vc, q, kn, vn = rn(B, L, H, D), rn(B, L, H, D), rn(B, M, H, D), rn(B, M, H, D), rn(B, M, H, D)
                lens = torch.full((B,), L - M, dtype=torch.int32, device="cuda")
                lens_i = [torch.full((B,), L - M + i, dtype=torch.int32, device="cuda") for i in range(M)]
                g_chunk = capture(lambda: flash_attn_with_kvcache_chunk(q, kc, vc, kn, vn, lens, 0.125, True, rpe, R))
                g_rows = capture(lambda: [flash_attn_with_kvcache(q[:, i:i + 1], kc, vc, kn[:, i:i + 1], vn[:, i:i + 1], lens_i[i], 0.125,
                                                                  rpe, R) for i in range(M)])
                qh, kh, vh = q.transpose(1, 2), kc.transpose(1, 2), vc.transpose(1, 2)
                g_fwd = capture(lambda: flash_attention_v2_rpe1d(qh, kh, vh, rpe, R, True, 0.125))
                tc, tr = [], []
                for _ in range(REPS):   # (alternating, in one process)
                    tc.append(replay_time(g_chunk, it))
                    tr.append(replay_time(g_rows, it))
                tf = replay_time(g_fwd, it)
                (mc, sc), (mr, sr) = med_spread(tc), med_spread(tr)
                faster = max(tc) < min(tr)
                rows[f"B{B}_L{L}_M{M}"] = {"chunk_us": round(mc * 1e6, 2), "chunk_spread_us": round(sc * 1e6, 2),
                                           "one_row_x_M_us": round(mr * 1e6, 2), "one_row_spread_us": round(sr * 1e6, 2),
                                           "fwd_MxL_us": round(tf * 1e6, 2), "speedup": round(mr / mc, 2), "faster": faster}
                print(f"B={B:3d} L={L:5d} M={M:3d}: chunk {mc * 1e6:8.2f} us (spread {sc * 1e6:5.2f}) | {M} one-row launches "
                      f"{mr * 1e6:8.2f} us (spread {sr * 1e6:5.2f}) | x{mr / mc:5.2f} {'faster' if faster else 'NOT faster'} | "
                      f"training forward M x L {tf * 1e6:8.2f} us", flush=True)
                del g_chunk, g_rows, g_fwd, kc, vc
    return rows


def e2e_rows(Bs, P=32, new_tokens=32, L_enc=512):
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).cuda().bfloat16().eval()
    rows = {}
    for B in Bs:
        ids = torch.randint(2, 32768, (B, L_enc), device="cuda")
        prompt = torch.randint(2, 32768, (B, P), device="cuda")
        prompt[:, 0] = 0

        def prefill(chunk):
            state = model.init_decode_state(ids, max_length=new_tokens, prompt_length=P)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            if chunk:
                model.decode_chunk(state, prompt[:, :P - 1], logits="none")
            else:
                for t in range(P - 1):
                    model.decode_step(state, prompt[:, t])
            model.decode_step(state, prompt[:, P - 1])
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e)

        def whole():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            model.generate(ids, max_length=new_tokens, graph=True, decoder_input_ids=prompt, suppress_tokens=[1])  # (no early stop)
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e)

        with torch.no_grad():
            prefill(True), prefill(False), whole()   # warm-up
            tc, ts = [], []
            for _ in range(REPS):
                tc.append(prefill(True))
                ts.append(prefill(False))
            tw = [whole() for _ in range(3)]
        (mc, sc), (ms, ss) = med_spread(tc), med_spread(ts)
        rows[f"B{B}"] = {"first_token_chunk_ms": round(mc, 3), "chunk_spread_ms": round(sc, 3), "first_token_steps_ms": round(ms, 3),
                         "steps_spread_ms": round(ss, 3), "generate_ms": round(statistics.median(tw), 3)}
        print(f"B={B:3d}: prompt of {P}: first new token after {mc:8.3f} ms with one chunk (spread {sc:.3f}), {ms:8.3f} ms with "
              f"{P - 1} decode_steps (spread {ss:.3f}); generate(+{new_tokens} tokens, graph) {statistics.median(tw):8.3f} ms", flush=True)
    return rows


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU (there is no CPU path)"
    quick = "--quick" in sys.argv
    res = {"kernel": kernel_rows((1, 16, 64), (128, 512, 1024), (2, 4, 8, 16, 64), 20 if quick else 200)}
    if "--kernel-only" not in sys.argv:
        res["end_to_end"] = e2e_rows((1, 16))
    print(json.dumps(res))
