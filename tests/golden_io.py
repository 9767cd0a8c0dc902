"""Loader for the committed golden fixtures (tests/golden/*.npz)."""
import os
import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}


def _t(a, dtype=None):
    if a.dtype == np.uint16:  # raw bf16 bits
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(a.copy())


class ieee_sqrt:
    """`with ieee_sqrt():` -- fp32 CPU `Tensor.sqrt` correctly rounded (numpy's, the hardware instruction).  torch computes it
    with MKL's vector math, accurate to 1 ulp and rounded differently on different CPU vendors; the fp32 AdamWScale parameters of
    adamw_scale.portable.npz are frozen under this context (reference and oracle alike, tests/golden/make_golden.py --portable),
    so their bits are the same on every host."""

    def __enter__(self):
        self.orig = orig = torch.Tensor.sqrt

        def sqrt(t):
            if t.dtype == torch.float32 and t.device.type == "cpu":
                return torch.from_numpy(np.sqrt(t.detach().numpy()))
            return orig(t)
        torch.Tensor.sqrt = sqrt

    def __exit__(self, *exc):
        torch.Tensor.sqrt = self.orig
        return False


def load(name):
    """<name>.npz, with the arrays of <name>.portable.npz laid over it when that file exists: the values the oracle tests compare
    bit for bit / to 1e-6, re-frozen so that every x86 host reproduces them (tests/golden/make_golden.py --portable)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {k: z[k] for k in z.files}
    portable = os.path.join(GOLDEN, name + ".portable.npz")
    if os.path.exists(portable):
        p = np.load(portable)
        out.update({k: p[k] for k in p.files})
    return out


def load_attn(name):
    z = load(name)
    B, H, M, N, D, causal, dt = (int(x) for x in z["meta"])
    dtype = DTYPES[dt]
    out = {"B": B, "H": H, "M": M, "N": N, "D": D, "causal": bool(causal), "dtype": dtype,
           "sm_scale": float(z["sm_scale"][0])}
    for key in z:
        if key in ("meta", "sm_scale"):
            continue
        out[key] = _t(z[key])
    if dtype == torch.float32:  # cfg1: inputs stored as bf16 bits, used as fp32
        for key in ("q", "k", "v", "bias", "do"):
            if key in out:
                out[key] = out[key].float()
    out.setdefault("bias", None)
    return out


ATTN_CASES = [
    "attn_t164_nc_1h_bf16", "attn_t164_nc_1h_fp16", "attn_t100_c_bh_bf16", "attn_t100_c_bh_fp16",
    "attn_mgtn_nc_bh_bf16", "attn_mgtn_c_1h_fp16", "attn_nobias_c_bf16", "attn_11_nc_bf16",
    "attn_d128_nc_bf16", "attn_d32_c_fp16",
]
TRITON_CASES = ["triton_t80_nc_1h_fp16", "triton_t80_c_bh_fp16", "triton_t100_nc_1h_fp16",
                "triton_d128_nc_1h_fp16", "triton_d32_c_1h_fp16", "triton_mgtn_nc_bh_fp16"]  # (round 3: D = 128, D = 32, M > N per-batch bias)
