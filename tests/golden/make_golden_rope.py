"""Generate tests/golden/rope_tables.npz from the IMPORTED reference (build container only).

    python tests/golden/make_golden_rope.py

Imports /root/reference (read-only) and runs its `RotaryPositionalEncoding._update_cos_sin_cache` -- the table code needs torch
and einops only, not flash_attn -- and stores the tables it builds (cos, sin and, with xPos, cos_k / sin_k) as arrays.  Only the
tables are stored: the rotation oracle is a few lines of eager torch in tests/test_rope_gpu.py.  16-bit tables are stored as raw
bits (uint16).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.utils.positional_encoding import RotaryPositionalEncoding  # noqa: E402

# name: (dim, rows, base, scale_base, dtype)  -- dim = int(d_kv * rotary_emb_fraction)
CASES = {
    "bf16_d64": (64, 1024, 10000.0, None, torch.bfloat16),
    "fp16_d64_half": (32, 512, 10000.0, None, torch.float16),
    "bf16_d64_xpos": (64, 1024, 10000.0, 512, torch.bfloat16),
    "fp32_d64": (64, 512, 10000.0, None, torch.float32),
    "bf16_d128": (128, 2048, 10000.0, None, torch.bfloat16),
}
CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def raw(t):
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.contiguous().view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def main():
    out = {}
    for name, (dim, rows, base, scale_base, dtype) in CASES.items():
        m = RotaryPositionalEncoding(dim, rows, base=base, interleaved=False, scale_base=scale_base)
        m._update_cos_sin_cache(rows, device=torch.device("cpu"), dtype=dtype)
        out[f"{name}__meta"] = np.array([dim, rows, base, -1 if scale_base is None else scale_base, CODES[dtype]], dtype=np.float64)
        out[f"{name}__cos"], out[f"{name}__sin"] = raw(m._cos_cached), raw(m._sin_cached)
        if scale_base is not None:
            out[f"{name}__cos_k"], out[f"{name}__sin_k"] = raw(m._cos_k_cached), raw(m._sin_k_cached)
    np.savez_compressed(os.path.join(HERE, "rope_tables.npz"), **out)
    print("wrote rope_tables.npz:", ", ".join(CASES))


if __name__ == "__main__":
    main()
