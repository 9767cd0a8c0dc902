"""Logits-processor benchmark: the one-launch kernel (fat5_process_logits) and generation with processors.

Kernel alone, bf16 logits, (rows, V) in {(1, 32128), (64, 32128), (64, 250112)} x s in {64, 512}, all four processors on
(theta 1.2, n 3, min_length above s, 100 suppressed ids), with and without log_softmax; graph-replayed, device-event timed,
median of the repetitions.  Beside it, alternated in the same process, the only other form that keeps the step capturable: the
same semantics in torch ops over the whole fixed-size sequence buffer with masks (`torch_process`, checked against the kernel
before it is timed), captured the same way.  Roofline: rows V (e + 4) bytes, the read twice with log_softmax, at 6.3 TB/s.

End to end, FAT5-base in bf16, L_enc = 512, 64 new tokens forced (no early stop): ms per token of graph-replayed cached decoding
with n = 3, theta = 1.2, min_length = 30 against the same step without processors -- greedy and sampled at B in {1, 16, 64}, beam
search (k = 4) at B in {1, 16} -- alternated, tools/bench_sample.py's and bench_beam.py's method.  Prints one JSON line at the end.

`--ext`: the same shapes with the six further processors (L_enc 512, encoder n = 3, phi = 1.2, 16 bad-word sequences,
min_new_tokens above s, a forced EOS that does not fire) next to the launch with only the old four arguments, alternated, and
the end-to-end rows with them ("*_ext").  `--kernel-only` leaves the end-to-end part out; the "kernel" rows of a
`--kernel-only` run of this file at two commits, alternated in one session, compare the old-argument launch across them."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import process_logits, FAT5Config, FAT5ForConditionalGeneration  # noqa: E402
from flasht5_amd import generation  # noqa: E402
from flasht5_amd.beam import new_state  # noqa: E402

ACHIEVABLE = 6.3e12
NINF = float("-inf")


def torch_process(logits, seqs, lens, theta, n, m, eos, sup, log_softmax):
    """fat5.h's semantics in torch ops with static shapes (nothing depends on a host-side length, so it can be captured): the
    whole (rows, L) buffer is processed and positions past the length are sent to a spare column V.  theta: a 0-dim fp32 device
    tensor (a Python scalar divisor becomes a multiplication by its reciprocal on the GPU, which is not the IEEE quotient)"""
    rows, V = logits.shape
    L = seqs.shape[1]
    x = logits.float()
    if log_softmax:
        x = torch.log_softmax(x, -1)
    xp = torch.cat([x, x.new_zeros(rows, 1)], 1)
    pos = torch.arange(L, device=x.device).unsqueeze(0)
    ln = lens.long().clamp(0, L).unsqueeze(1)
    ok = (pos < ln) & (seqs >= 0) & (seqs < V)
    tok = torch.where(ok, seqs, torch.full_like(seqs, V))
    g = xp.gather(1, tok)
    y = xp.scatter(1, tok, torch.where(g < 0, g * theta, g / theta))
    if n > 0:
        W = L - n + 1
        tail_idx = (ln - (n - 1) + torch.arange(n - 1, device=x.device).unsqueeze(0)).clamp(0, L - 1)
        tail = tok.gather(1, tail_idx)
        match = (pos[:, :W] <= ln - n)
        for j in range(n - 1):
            match = match & (tok[:, j:j + W] == tail[:, j:j + 1])
        y = y.scatter(1, torch.where(match, tok[:, n - 1:], torch.full_like(tok[:, n - 1:], V)), NINF)
    y[:, eos] = torch.where(ln[:, 0] < m, torch.full_like(y[:, eos], NINF), y[:, eos])
    if sup is not None:
        y = y.index_fill(1, sup, NINF)  # (sup: int64 here; an indexed assignment would synchronise inside a capture)
    return y[:, :V]


def _graph(fn):
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


def _time(g, it=50):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e-3


def kernel_rows(reps=7):
    rows_out = {}
    theta, n = 1.2, 3
    for rows, V in ((1, 32128), (64, 32128), (64, 250112)):
        for s in (64, 512):
            L = s + 1
            g0 = torch.Generator().manual_seed(rows + V + s)
            logits = (torch.randn(rows, V, generator=g0) * 3).bfloat16().cuda()
            seqs = torch.randint(0, 2000, (rows, L), generator=g0).cuda()
            lens = torch.full((rows,), s, dtype=torch.int32, device="cuda")
            sup = torch.arange(32000, 32100, dtype=torch.int32, device="cuda")
            m = s + 1
            sup_l = sup.long()
            theta_t = torch.tensor(theta, dtype=torch.float32, device="cuda")
            for ls in (False, True):
                kern = lambda: process_logits(logits, seqs, lens, repetition_penalty=theta, no_repeat_ngram_size=n, min_length=m,  # noqa: E731
                                              suppress_tokens=sup, log_softmax=ls)
                base = lambda: torch_process(logits, seqs, lens, theta_t, n, m, 1, sup_l, ls)  # noqa: E731
                a, b = kern(), base()
                if ls:
                    fin = torch.isfinite(b)
                    assert torch.equal(torch.isfinite(a), fin) and (a[fin] - b[fin]).abs().max() <= 1e-4, "baseline != kernel"
                else:
                    assert torch.equal(a, b), f"baseline != kernel at {int((a != b).sum())} entries"
                gk, gb = _graph(kern), _graph(base)
                tk, tb = [], []
                for _ in range(reps):  # (alternated)
                    tk.append(_time(gk))
                    tb.append(_time(gb))
                del gk, gb
                t_k, t_b = statistics.median(tk), statistics.median(tb)
                nbytes = rows * V * (2 * (2 if ls else 1) + 4)
                key = f"rows{rows}_V{V}_s{s}_{'logsoftmax' if ls else 'plain'}"
                rows_out[key] = {"kernel_us": round(t_k * 1e6, 2), "torch_masked_us": round(t_b * 1e6, 2),
                                 "ratio": round(t_b / t_k, 2), "roofline_us": round(nbytes / ACHIEVABLE * 1e6, 2),
                                 "GBs": round(nbytes / t_k / 1e9, 1), "kernel_min_max_us": [round(min(tk) * 1e6, 2), round(max(tk) * 1e6, 2)]}
                print(f"{key:40s}: kernel {t_k * 1e6:8.2f} us ({nbytes / t_k / 1e9:7.1f} GB/s, roofline {nbytes / ACHIEVABLE * 1e6:6.2f} us)"
                      f" | torch masked ops {t_b * 1e6:8.2f} us ({t_b / t_k:5.1f}x)", flush=True)
    return rows_out


def ext_kernel_rows(reps=7, L_enc=512):
    """the launch with all ten processors against the launch with the old four, same rows, alternated"""
    from flasht5_amd import pack_bad_words
    rows_out = {}
    theta, n = 1.2, 3
    for rows, V in ((1, 32128), (64, 32128), (64, 250112)):
        for s in (64, 512):
            L = s + 1
            g0 = torch.Generator().manual_seed(rows + V + s)
            logits = (torch.randn(rows, V, generator=g0) * 3).bfloat16().cuda()
            seqs = torch.randint(0, 2000, (rows, L), generator=g0).cuda()
            enc = torch.randint(0, 2000, (rows, L_enc), generator=g0).cuda()
            lens = torch.full((rows,), s, dtype=torch.int32, device="cuda")
            sup = torch.arange(32000, 32100, dtype=torch.int32, device="cuda")
            bad = pack_bad_words([[int(t) for t in torch.randint(2, 2000, (1 + i % 3,), generator=g0)] for i in range(16)], "cuda")
            old = dict(repetition_penalty=theta, no_repeat_ngram_size=n, min_length=s + 1, suppress_tokens=sup)
            new = dict(old, encoder_repetition_penalty=1.2, encoder_no_repeat_ngram_size=3, encoder_input_ids=enc, bad_words_ids=bad,
                       min_new_tokens=s + 1, forced_eos_token_id=1, max_new_tokens=4095)
            for ls in (False, True):
                g_old = _graph(lambda: process_logits(logits, seqs, lens, log_softmax=ls, **old))
                g_new = _graph(lambda: process_logits(logits, seqs, lens, log_softmax=ls, **new))
                t_old, t_new = [], []
                for _ in range(reps):  # (alternated)
                    t_old.append(_time(g_old))
                    t_new.append(_time(g_new))
                del g_old, g_new
                key = f"rows{rows}_V{V}_s{s}_{'logsoftmax' if ls else 'plain'}"
                us = lambda v: round(v * 1e6, 2)  # noqa: E731
                rows_out[key] = {"old4_us": us(statistics.median(t_old)), "old4_min_max_us": [us(min(t_old)), us(max(t_old))],
                                 "ext10_us": us(statistics.median(t_new)), "ext10_min_max_us": [us(min(t_new)), us(max(t_new))]}
                print(f"{key:40s}: old four {rows_out[key]['old4_us']:8.2f} us {rows_out[key]['old4_min_max_us']} | all ten "
                      f"{rows_out[key]['ext10_us']:8.2f} us {rows_out[key]['ext10_min_max_us']}", flush=True)
    return rows_out


PROC = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=30, eos_token_id=1, suppress_tokens=None)
EXT = "--ext" in sys.argv


def _ext_proc(ids, k=1):
    """PROC plus the six further processors, as `generate` hands them to the step"""
    from flasht5_amd import pack_bad_words
    proc = dict(PROC, encoder_repetition_penalty=1.2, encoder_no_repeat_ngram_size=3, min_new_tokens=30, forced_eos_token_id=1,
                bad_words_ids=pack_bad_words([[5 + i, 9 + i] for i in range(16)], ids.device), encoder_input_ids=ids,
                rows_per_encoder_row=k, max_new_tokens=64)
    return proc


def _replay_ms(g, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(steps):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def e2e_rows(new_tokens=64, L_enc=512, reps=3):
    torch.manual_seed(0)
    model = FAT5ForConditionalGeneration(FAT5Config()).cuda().bfloat16().eval()
    sampling = (0.7, 50, 0.9, 1234)
    out = {}
    with torch.no_grad():
        for B in (1, 16, 64):
            ids = torch.randint(2, 32768, (B, L_enc), device="cuda")

            def cached(step):
                state = model.init_decode_state(ids, max_length=new_tokens)
                labels = torch.zeros((B, state.capacity), dtype=torch.long, device="cuda")
                tok = torch.zeros((B,), dtype=torch.long, device="cuda")
                eos = torch.zeros((B,), dtype=torch.bool, device="cuda")
                step(model, state, tok, labels, eos)
                g = generation._capture_call(lambda: step(model, state, tok, labels, eos))
                return _replay_ms(g, new_tokens - 1)

            steps = {
                "greedy": lambda m, st, t, lb, e: generation._step(m, st, t, lb, e),
                "greedy_proc": lambda m, st, t, lb, e: generation._step(m, st, t, lb, e, PROC),
                "sample": lambda m, st, t, lb, e: generation._step(m, st, t, lb, e, None, sampling),
                "sample_proc": lambda m, st, t, lb, e: generation._step(m, st, t, lb, e, PROC, sampling),
            }
            if EXT:
                ext = _ext_proc(ids)
                steps["greedy_ext"] = lambda m, st, t, lb, e: generation._step(m, st, t, lb, e, ext)
                steps["sample_ext"] = lambda m, st, t, lb, e: generation._step(m, st, t, lb, e, ext, sampling)
            cached(steps["greedy"])  # warm-up
            ms = {k: [] for k in steps}
            for _ in range(reps):  # (alternated)
                for k, f in steps.items():
                    ms[k].append(cached(f))
            row = {k: round(statistics.median(v), 4) for k, v in ms.items()}
            row["greedy_overhead_pct"] = round((row["greedy_proc"] / row["greedy"] - 1) * 100, 2)
            row["sample_overhead_pct"] = round((row["sample_proc"] / row["sample"] - 1) * 100, 2)
            if EXT:
                row["greedy_ext_overhead_pct"] = round((row["greedy_ext"] / row["greedy"] - 1) * 100, 2)
                row["sample_ext_overhead_pct"] = round((row["sample_ext"] / row["sample"] - 1) * 100, 2)
            row["all"] = {k: [round(x, 4) for x in v] for k, v in ms.items()}
            out[f"B{B}"] = row
            print(f"B={B:3d}: {row}", flush=True)
        k = 4
        for B in (1, 16):
            ids = torch.randint(2, 32768, (B, L_enc), device="cuda")

            def beam(proc):
                state = generation.init_decode_state(model, ids, new_tokens, num_beams=k)
                bs = new_state(B, k, new_tokens + 1, state.capacity, "cuda")
                bs.cache_row_batch = state.row_batch
                tok = torch.zeros(B * k, dtype=torch.long, device="cuda")
                opts = (new_tokens, 1.0, False)
                generation._beam_step(model, state, tok, bs, opts, proc)
                g = generation._capture_call(lambda: generation._beam_step(model, state, tok, bs, opts, proc))
                return _replay_ms(g, new_tokens - 1)

            beam(None)
            ms = {"beam": [], "beam_proc": []}
            if EXT:
                ms["beam_ext"] = []
            for _ in range(reps):
                ms["beam"].append(beam(None))
                ms["beam_proc"].append(beam(PROC))
                if EXT:
                    ms["beam_ext"].append(beam(_ext_proc(ids, k)))
            row = {k_: round(statistics.median(v), 4) for k_, v in ms.items()}
            row["beam_overhead_pct"] = round((row["beam_proc"] / row["beam"] - 1) * 100, 2)
            if EXT:
                row["beam_ext_overhead_pct"] = round((row["beam_ext"] / row["beam"] - 1) * 100, 2)
            row["all"] = {k_: [round(x, 4) for x in v] for k_, v in ms.items()}
            out[f"beam_B{B}_k{k}"] = row
            print(f"beam B={B:3d} k={k}: {row}", flush=True)
    return out


if __name__ == "__main__":
    res = {"kernel": kernel_rows()}
    if EXT:
        res["kernel_ext"] = ext_kernel_rows()
    if "--kernel-only" not in sys.argv:
        res["end_to_end"] = e2e_rows()
    print(json.dumps(res))
