"""Beam-search benchmark: generate(num_beams=4) on the beam-step kernel and the indexed decode reads, against greedy decoding at
B * k rows and against an eager HF-style loop over the same decode step.

FAT5-base, bf16, L_enc = 512, random weights (EOS rarely ends a run: the steps actually run are reported), max_length new tokens.
  - graph:   one captured step (decode step + beam step) replayed per token, timed with device events over the steps, without
             generate's per-token host read of the stop flag;
  - generate: `generate(num_beams=4, graph=True)` end to end (encoder, capture, host reads) divided by its steps;
  - greedy:  the cached greedy step at B * 4 rows, graph-replayed (the same decode work with an argmax instead of the beam step);
  - hf_eager: the decode step on duplicated cross caches (B * k rows, no cache_batch_idx), torch bookkeeping (log_softmax, topk
             of 2k, gathers, the finished merge, the heuristic) and a per-layer index_select reorder of every self-attention cache,
             eagerly, with one host read per token as HF's loop has.
Stage-1 roofline: B * k * V * elem bytes of logits read once per step; the fraction is against 6.3 TB/s (achievable).
Decode kernel with and without the row map at tools/bench_decode.py's shapes (H 12, D 64, bf16, T5 bias, append).
Kernel times: run `--quick` under `rocprofv3 --kernel-trace --stats` (tools/README.md).  Prints one JSON line at the end."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration, flash_attn_with_kvcache  # noqa: E402
from flasht5_amd import generation  # noqa: E402
from flasht5_amd.beam import new_state, keep_going  # noqa: E402
from flasht5_amd.positional_encoding import rpe1d_from_table  # noqa: E402

ACHIEVABLE = 6.3e12


def graph_time(fn, it=50):
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


def decode_kernel_rows(Bs, Ls):
    H, D, R = 12, 64, 128
    g = torch.Generator().manual_seed(0)
    rpe = rpe1d_from_table(torch.randn(32, H, generator=g), bidirectional=False, num_buckets=32, max_distance=R).cuda()
    rows = []
    for B in Bs:
        for L in Ls:
            kc = torch.randn(B, L, H, D, dtype=torch.bfloat16, device="cuda")
            vc = torch.randn(B, L, H, D, dtype=torch.bfloat16, device="cuda")
            q, kn, vn = (torch.randn(B, 1, H, D, dtype=torch.bfloat16, device="cuda") for _ in range(3))
            lens = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
            k = 4 if B % 4 == 0 else 1  # (parents inside groups of 4 rows, as beams of one input)
            table = ((torch.arange(B, device="cuda") // k) * k).int().unsqueeze(1) + torch.randint(0, k, (B, L), device="cuda").int()
            plain = graph_time(lambda: flash_attn_with_kvcache(q, kc, vc, kn, vn, lens, 0.125, rpe, R))
            mapped = graph_time(lambda: flash_attn_with_kvcache(q, kc, vc, kn, vn, lens, 0.125, rpe, R, cache_row_batch=table))
            rows.append(dict(B=B, L=L, plain_us=round(plain * 1e6, 2), row_map_us=round(mapped * 1e6, 2),
                             ratio=round(mapped / plain, 3)))
            print(f"[decode] B {B:3d} L {L:5d}: plain {plain * 1e6:7.2f} us  row map {mapped * 1e6:7.2f} us  ({mapped / plain:.3f}x)",
                  flush=True)
    return rows


def _hf_eager_step(model, state, tok, st, k, max_length, s):
    """the decode step on duplicated cross caches, then HF's bookkeeping in torch and the per-layer cache reorder"""
    logits = generation.decode_step(model, state, tok).float()
    B = st["rs"].shape[0]
    V = logits.shape[-1]
    lp = torch.log_softmax(logits, -1).view(B, k, V) + st["rs"][:, :, None]
    top, idx = lp.view(B, k * V).topk(2 * k)
    parent, nxt = idx // V, idx % V
    hits = (nxt == 1) | (s >= max_length)
    v = top + hits.float() * -1e9
    ri = v.topk(k).indices
    f = top / float(s) + (~st["unsat"]).float()[:, None] * -1e9 + (~(hits & (torch.arange(2 * k, device=v.device) < k))).float() * -1e9
    merged = torch.cat([st["fs"], f], 1)
    fi = merged.topk(k).indices
    seqs = st["seq"].gather(1, parent[:, :, None].expand(-1, -1, st["seq"].shape[2])).clone()
    seqs[:, :, s] = nxt
    st["fin"] = torch.cat([st["fin"], seqs], 1).gather(1, fi[:, :, None].expand(-1, -1, seqs.shape[2]))
    st["fs"] = merged.gather(1, fi)
    st["seq"] = seqs.gather(1, ri[:, :, None].expand(-1, -1, seqs.shape[2]))
    st["rs"] = v.gather(1, ri)
    best = st["rs"][:, :1] / float(s)
    st["unsat"] = st["unsat"] & (best > st["fs"].min(1, keepdim=True).values).any(-1)
    beam_idx = ((torch.arange(B, device=v.device)[:, None] * k) + parent.gather(1, ri)).view(-1)
    for kc, vc in zip(state.self_k, state.self_v):  # (HF's _reorder_cache: index_select per layer)
        kc.copy_(kc.index_select(0, beam_idx))
        vc.copy_(vc.index_select(0, beam_idx))
    tok.copy_(st["seq"][:, :, s].reshape(-1))
    return bool(st["unsat"].any())  # (one host read per token, as HF's loop)


def run(Bs, k, max_length, L_enc, quick):
    torch.manual_seed(0)
    c = FAT5Config(num_layers=12, num_decoder_layers=12, attention_type="fat5_rpe")
    m = FAT5ForConditionalGeneration(c).cuda().bfloat16().eval()
    V = c.vocab_size
    out = []
    for B in Bs:
        ids = torch.randint(2, V, (B, L_enc), device="cuda")
        row = dict(B=B, k=k, L_enc=L_enc, max_length=max_length)
        with torch.no_grad():
            # graph-replayed beam step, no host reads
            state = generation.init_decode_state(m, ids, max_length, num_beams=k)
            bs = new_state(B, k, max_length + 1, state.capacity, "cuda")
            bs.cache_row_batch = state.row_batch
            tok = torch.zeros(B * k, dtype=torch.long, device="cuda")
            opts = (max_length, 1.0, False)
            generation._beam_step(m, state, tok, bs, opts)
            g = generation._capture_call(lambda: generation._beam_step(m, state, tok, bs, opts))
            steps = max_length - 1
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(steps):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            row["graph_ms_per_token"] = round(s.elapsed_time(e) / steps, 4)
            del g
            if quick:
                out.append(row)
                continue
            # generate end to end
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seqs = m.generate(ids, max_length=max_length, graph=True, num_beams=k)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ran = int(seqs.shape[1] - 1)
            row["generate_ms_per_token"] = round(wall * 1e3 / max(1, ran), 4)
            row["generate_longest_hypothesis"] = ran
            # greedy at B * k rows, graph-replayed
            ids_k = ids.repeat_interleave(k, 0)
            gst = generation.init_decode_state(m, ids_k, max_length)
            gtok = torch.zeros(B * k, dtype=torch.long, device="cuda")
            labels = torch.zeros(B * k, gst.capacity, dtype=torch.long, device="cuda")
            seen = torch.zeros(B * k, dtype=torch.bool, device="cuda")
            generation._step(m, gst, gtok, labels, seen)
            g = generation._capture_call(lambda: generation._step(m, gst, gtok, labels, seen))
            s.record()
            for _ in range(steps):
                g.replay()
            e.record()
            torch.cuda.synchronize()
            row["greedy_Bk_graph_ms_per_token"] = round(s.elapsed_time(e) / steps, 4)
            del g
            # HF-style eager loop on the same decode step
            hst = generation.init_decode_state(m, ids, max_length)
            hst.cross_k = [t.repeat_interleave(k, 0).contiguous() for t in hst.cross_k]
            hst.cross_v = [t.repeat_interleave(k, 0).contiguous() for t in hst.cross_v]
            hst.self_k = [torch.zeros((B * k,) + t.shape[1:], dtype=t.dtype, device="cuda") for t in hst.self_k]
            hst.self_v = [torch.zeros((B * k,) + t.shape[1:], dtype=t.dtype, device="cuda") for t in hst.self_v]
            hst.cache_seqlens = torch.zeros(B * k, dtype=torch.int32, device="cuda")
            rs = torch.full((B, k), -1e9, device="cuda")
            rs[:, 0] = 0
            hs = dict(rs=rs, fs=torch.full((B, k), -1e9, device="cuda"), unsat=torch.ones(B, dtype=torch.bool, device="cuda"),
                      seq=torch.zeros(B, k, max_length + 1, dtype=torch.long, device="cuda"),
                      fin=torch.zeros(B, k, max_length + 1, dtype=torch.long, device="cuda"))
            htok = torch.zeros(B * k, dtype=torch.long, device="cuda")
            _hf_eager_step(m, hst, htok, hs, k, max_length, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(2, max_length + 1):
                _hf_eager_step(m, hst, htok, hs, k, max_length, i)
            torch.cuda.synchronize()
            row["hf_eager_ms_per_token"] = round((time.perf_counter() - t0) * 1e3 / (max_length - 1), 4)
            # stage-1 roofline
            row["stage1_logit_bytes"] = B * k * V * 2
            row["stage1_roofline_us"] = round(B * k * V * 2 / ACHIEVABLE * 1e6, 2)
        print(f"[beam] {row}", flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--max-length", type=int, default=64)
    ap.add_argument("--l-enc", type=int, default=512)
    ap.add_argument("--quick", action="store_true", help="graph-replayed beam steps only (for a rocprofv3 run)")
    ap.add_argument("--no-decode-kernel", action="store_true")
    a = ap.parse_args()
    Bs = [int(x) for x in a.batches.split(",")]
    res = dict(beam=run(Bs, a.beams, a.max_length, a.l_enc, a.quick))
    if not a.quick and not a.no_decode_kernel:
        res["decode_kernel"] = decode_kernel_rows([1, 16, 64], [128, 512, 1024, 4096])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
