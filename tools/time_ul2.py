"""Time the UL2 collator: B = 64 rows of L = 2048 raw tokens, max_length = max_labels_length = 1024, the denoiser
set of the reference's train_flash_t5.py (max_spans 1024).

  device: one `UL2Collator` call -- two launches, the output allocations and the counter's in-place add -- (a) eager, the host
          clock around `--calls` calls that end in a device synchronise, (b) captured in a graph and replayed, device events
          around `--calls` replays.  Medians over `--rounds` rounds, in microseconds per call.
  host:   the plain-loop restatement of the contract (tests/ul2_ref.py) on the same batch, one call, in seconds.  It is the
          tests' oracle, written for reading, not for speed: the figure says what a per-example Python collator costs, not what
          the best host code could do.

Both produce the same batch: the script checks that before it times anything.  One JSON line at the end; `--log` keeps a copy."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from flasht5_amd import UL2Collator  # noqa: E402
from flasht5_amd.ul2 import _host_tables  # noqa: E402
import ul2_ref  # noqa: E402

DENOISERS = [dict(mu=mu, r=r, max_spans=ms, prefix_ids=p) for mu, r, ms, p in (
    (3.0, 0.15, 1024, [31990, 31991]), (8.0, 0.15, 1024, [31990, 31991]), (4.0, 0.0, 1, [31992]), (3.0, 0.5, 1024, [31993, 31994]),
    (8.0, 0.15, 1024, [31993, 31994]), (64.0, 0.15, 1024, [31993, 31994]), (64.0, 0.5, 1024, [31993, 31994]))]
PROPORTIONS = [0.165, 0.165, 0.34, 0.0825, 0.0825, 0.0825, 0.0825]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=2048)
    ap.add_argument("--max-length", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ul2 needs the GPU: a CPU run measures nothing")
    args = dict(max_length=a.max_length, max_labels_length=a.max_length, sentinel_first_id=32099, num_sentinels=100, eos_token_id=1,
                pad_token_id=0)
    rng = np.random.default_rng(a.seed)
    tok = rng.integers(2, 31000, size=(a.batch, a.length)).astype(np.int64)
    lengths = rng.integers(a.length // 8, a.length + 1, size=a.batch).astype(np.int32)
    tokens, n_dev = torch.from_numpy(tok).cuda(), torch.from_numpy(lengths).cuda()
    c = UL2Collator(DENOISERS, PROPORTIONS, seed=a.seed, **args)
    tab = _host_tables(DENOISERS, PROPORTIONS, args["max_length"], args["max_labels_length"], args["sentinel_first_id"], args["num_sentinels"])

    out = c(tokens, n_dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = ul2_ref.collate(tok, lengths, tab, seed=a.seed, step=0, **args)
    host_s = time.perf_counter() - t0
    for k in ("input_ids", "labels", "enc_len", "dec_len", "denoiser", "status"):
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    flags = int(want["status"][0])

    for _ in range(20):
        c(tokens, n_dev)
    torch.cuda.synchronize()
    eager = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            c(tokens, n_dev)
        torch.cuda.synchronize()
        eager.append((time.perf_counter() - t0) / a.calls * 1e6)

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c(tokens, n_dev)
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    graph = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        graph.append(e0.elapsed_time(e1) / a.calls * 1e3)

    res = dict(tool="time_ul2", batch=a.batch, length=a.length, max_length=a.max_length, tokens_len=tab["tokens_len"], status_flags=flags,
               eager_us_per_call=round(statistics.median(eager), 2), eager_us_min_max=[round(min(eager), 2), round(max(eager), 2)],
               graph_us_per_call=round(statistics.median(graph), 2), graph_us_min_max=[round(min(graph), 2), round(max(graph), 2)],
               host_restatement_s=round(host_s, 3), calls=a.calls, rounds=a.rounds)
    line = json.dumps(res)
    print(line, flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
