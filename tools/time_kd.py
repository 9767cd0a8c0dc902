"""Time the distillation loss at (4096, 32768) bf16: `fat5_kd_fwd_bwd` (one launch, in place) against the eager
PyTorch composition (two log-softmaxes, kl_div, cross_entropy, z-loss and their autograd) on the same GPU, against `fat5_ce_fwd_bwd`
at the same shape (two row streams where the distillation kernel moves three) and against its own two launches.  Width 32776
stands beside 32768 because `fat5_ce_fwd_bwd` changes kernels there (it holds a row of up to 32768 16-bit columns in registers);
the distillation kernel reads its rows twice at every width.

Device events around `calls` back-to-back calls, every shape warmed up, the variants alternated inside each of 7 rounds: median
[min, max] in microseconds per call.  `--log FILE` keeps a copy of the output."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from flasht5_amd import distillation as KD  # noqa: E402
from flasht5_amd.cross_entropy_loss import cross_entropy_fwd_bwd_  # noqa: E402

ROWS, ALPHA, T, SM, ZS = 4096, 0.5, 2.0, 0.1, 1e-4
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)


def make(V):
    s = (torch.randn(ROWS, V, generator=g) * 2).bfloat16().to(dev)
    t = (torch.randn(ROWS, V, generator=g) * 2).bfloat16().to(dev)
    y = torch.randint(0, V, (ROWS,), generator=g).to(dev)
    return s, t, y


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per call


def eager(s, t, y):
    s = s.detach().requires_grad_()
    sf, tf = s.float(), t.float()
    kd = F.kl_div(F.log_softmax(sf / T, -1), F.log_softmax(tf / T, -1), reduction="none", log_target=True).sum(-1)
    lse = torch.logsumexp(sf, -1)
    ce = F.cross_entropy(sf, y, reduction="none", label_smoothing=SM) + ZS * lse * lse
    loss = ((1 - ALPHA) * ce + ALPHA * T * T * kd).mean()
    loss.backward()
    return loss


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_kd needs the GPU: a CPU run measures nothing")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    variants = {}
    dl = torch.full((1,), 1.0 / ROWS, device=dev)
    outs = [torch.empty(ROWS, device=dev) for _ in range(7)]
    for V in (32768, 32776):
        s, t, y = make(V)
        buf = s.clone()
        cfg = (ALPHA, T, SM, 1.0, ZS, -100)
        variants[f"kd_fwd_bwd V={V}"] = (lambda buf=buf, t=t, y=y: KD.distillation_fwd_bwd_(buf, t, y, dl.expand(ROWS), *outs, *cfg), 50)
        variants[f"ce_fwd_bwd V={V}"] = (lambda buf=buf, y=y: cross_entropy_fwd_bwd_(buf, y, dl.expand(ROWS), outs[0], outs[2], outs[4], SM, 1.0, ZS, -100), 50)
        if V == 32768:
            def two(s=s, t=t, y=y, buf=buf):
                o = KD.distillation_fwd(s, t, y, *cfg)
                KD._launch("fat5_kd_bwd", s, t, y, cfg, dlosses=dl.expand(ROWS), lse=o[4], lse_s=o[5], lse_t=o[6], dlogits=buf)
            variants["kd two launches V=32768"] = (two, 50)
            variants["eager composition V=32768"] = (lambda s=s, t=t, y=y: eager(s, t, y), 5)
    for fn, _ in variants.values():   # warm-up of every shape
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(7):
        for k, (fn, n) in variants.items():
            times[k].append(timed(fn, n))
    say(f"rows {ROWS}, bf16, alpha {ALPHA}, T {T}, smoothing {SM}, z {ZS}; us per call, median [min, max] of 7 rounds")
    for k, v in times.items():
        V = int(k.split("V=")[1])
        streams = 3 if k.startswith("kd_fwd_bwd") else 2 if k.startswith("ce") else 0
        bw = f"  {streams * ROWS * V * 2 / statistics.median(v) / 1e6:.2f} TB/s of its {streams} row streams" if streams else ""
        say(f"{k:32s} {statistics.median(v):9.1f} [{min(v):9.1f}, {max(v):9.1f}]{bw}")
    torch.cuda.reset_peak_memory_stats()
    s, t, y = make(32768)
    base = torch.cuda.memory_allocated()
    eager(s, t, y)
    say(f"eager composition: peak memory above its inputs {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB "
        f"(inputs: {2 * ROWS * 32768 * 2 / 2 ** 20:.0f} MiB; the fused launch allocates nothing)")
    if "--log" in sys.argv:
        with open(sys.argv[sys.argv.index("--log") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
