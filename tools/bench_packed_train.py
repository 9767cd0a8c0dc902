"""Padded against packed training steps: FAT5-base, bf16, the eager `train_step` with AdamWScale, B = 16,
L_enc = 1024, L_dec = 256, encoder and decoder lengths drawn once, uniformly from [L / 8, L], under a fixed seed.

  padded: `train_step(model, ids, labels)` -- the step of before: no mask, every padded position computed (and attended);
  packed: `train_step(model, ids, labels, attention_mask=..., decoder_attention_mask=...)` -- the valid tokens only; the step
          includes the planner's two launches per side and the forward's one host read.

One process, both forms warmed up, then timed in alternating rounds (host clock around a device synchronise); the medians over
the rounds are reported as ms per step and valid tokens (encoder + decoder) per second.  `--steps` steps per round, `--rounds`
rounds, `--layers` to shrink the model for a rehearsal.  One JSON line at the end; a log copy goes to `--log`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from flasht5_amd import AdamWScale, FAT5Config, FAT5ForConditionalGeneration, train_step  # noqa: E402


def make_batch(cfg, B, l_enc, l_dec, seed):
    g = torch.Generator().manual_seed(seed)
    enc_lens = torch.randint(l_enc // 8, l_enc + 1, (B,), generator=g)
    dec_lens = torch.randint(l_dec // 8, l_dec + 1, (B,), generator=g)
    ids = torch.randint(1, cfg.vocab_size, (B, l_enc), generator=g)
    labels = torch.randint(1, cfg.vocab_size, (B, l_dec), generator=g)
    am = torch.arange(l_enc).unsqueeze(0) < enc_lens.unsqueeze(1)
    dm = torch.arange(l_dec).unsqueeze(0) < dec_lens.unsqueeze(1)
    ids = ids.masked_fill(~am, cfg.pad_token_id)
    labels = labels.masked_fill(~dm, -100)
    return ids.cuda(), labels.cuda(), am.cuda(), dm.cuda(), int(enc_lens.sum()), int(dec_lens.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--enc", type=int, default=1024)
    ap.add_argument("--dec", type=int, default=256)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_packed_train needs the GPU: a CPU run measures nothing")

    cfg = FAT5Config(num_layers=a.layers, num_decoder_layers=a.layers)
    torch.manual_seed(a.seed)
    model = FAT5ForConditionalGeneration(cfg).cuda().bfloat16()
    opt = AdamWScale(model.parameters(), lr=1e-4, max_grad_norm=1.0)
    ids, labels, am, dm, n_enc, n_dec = make_batch(cfg, a.batch, a.enc, a.dec, a.seed)
    valid = n_enc + n_dec
    forms = {
        "padded": lambda: train_step(model, ids, labels, opt, max_grad_norm=None),
        "packed": lambda: train_step(model, ids, labels, opt, max_grad_norm=None, attention_mask=am, decoder_attention_mask=dm),
    }
    lines = [f"FAT5-base ({a.layers} + {a.layers} layers) bf16 eager train_step, B = {a.batch}, L_enc = {a.enc}, L_dec = {a.dec}; valid tokens "
             f"{n_enc} of {a.batch * a.enc} (encoder), {n_dec} of {a.batch * a.dec} (decoder); {a.rounds} alternating rounds of {a.steps} steps"]
    print(lines[0], flush=True)
    for fn in forms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps)
            assert torch.isfinite(loss).item(), name
    out = {"valid_tokens": valid, "padded_positions": a.batch * (a.enc + a.dec)}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"ms_per_step": round(med * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2), "max_ms": round(max(ts) * 1e3, 2),
                     "valid_tokens_per_s": round(valid / med)}
        lines.append(f"{name}: median {med * 1e3:8.2f} ms / step (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}), "
                     f"{valid / med:,.0f} valid tokens / s")
        print(lines[-1], flush=True)
    out["packed_over_padded_time"] = round(out["packed"]["ms_per_step"] / out["padded"]["ms_per_step"], 3)
    lines.append(f"packed / padded step time: {out['packed_over_padded_time']:.3f}")
    print(lines[-1], flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
