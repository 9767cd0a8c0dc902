"""Generate tests/golden/fire.npz from the IMPORTED reference (build container only).

    python tests/golden/make_golden_fire.py

Imports /root/reference (read-only), builds its `FIRE` module on the CPU in fp32, sets the case's parameters, runs `apply_fire`
and autograd with a seeded upstream gradient, and stores arrays only: the parameters, the bias, the upstream gradient and the
reference gradients of the six parameters (init_L's is zero: it is not trainable).  Cases:
  * t128_tie   S = 256, default T = 128 (row 128 ties with the threshold)
  * zero_b1    some mlp.0.bias entries exactly zero (relu'(0) = 0 on the diagonal)
  * neg_c_lm   negative c and negative L_multiplier
  * w8_h6      W = 8, H = 6
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.utils.positional_encoding import FIRE  # noqa: E402

# name: (S, H, W, init_L, c, L_multiplier, zero_b1)
CASES = {
    "t128_tie": (256, 2, 32, 128, 0.1, 1.0, False),
    "zero_b1": (64, 4, 16, 24, 0.1, 1.0, True),
    "neg_c_lm": (96, 4, 32, 40, -0.3, -0.75, False),
    "w8_h6": (48, 6, 8, 16, 0.25, 1.0, False),
}


def main():
    out = {}
    for idx, (name, (S, H, W, init_L, c, lm, zero_b1)) in enumerate(CASES.items()):
        torch.manual_seed(1000 + idx)
        m = FIRE(num_heads=H, mlp_width=W, init_c=0.1, init_L=init_L)
        with torch.no_grad():
            m.c.fill_(c)
            m.L_multiplier.fill_(lm)
            if zero_b1:
                m.mlp[0].bias[::3] = 0.0
        bias = m.apply_fire(S, "cpu")  # (1, H, S, S) fp32
        # (bf16-representable values, stored as raw bf16 bits: half the bytes, and exact in every dtype the kernels take)
        g = torch.randn(bias.shape, generator=torch.Generator().manual_seed(2000 + idx)).bfloat16().float()
        bias.backward(g)
        arrays = {
            "w1": m.mlp[0].weight, "b1": m.mlp[0].bias, "w2": m.mlp[2].weight, "b2": m.mlp[2].bias,
            "c": m.c, "L_multiplier": m.L_multiplier, "init_L": m.init_L.float(),
            "bias": bias,
        }
        for k, v in arrays.items():
            out[f"{name}__{k}"] = v.detach().numpy().astype(np.float32)
        out[f"{name}__dbias"] = g.bfloat16().view(torch.int16).numpy().view(np.uint16)
        for k, p in (("w1", m.mlp[0].weight), ("b1", m.mlp[0].bias), ("w2", m.mlp[2].weight), ("b2", m.mlp[2].bias),
                     ("c", m.c), ("L_multiplier", m.L_multiplier)):
            out[f"{name}__grad_{k}"] = p.grad.detach().numpy().astype(np.float32)
        out[f"{name}__meta"] = np.array([S, H, W, m.eps], dtype=np.float64)
    path = os.path.join(HERE, "fire.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
