"""Host-only: where the 64-row dQ body takes its resident K / V form (fat5_attn_bwd_kvres, "kvres" of the Python describe() dicts; csrc/attn_dispatch.h,
BwdLayout::kvres).
The rule: the 64-row dQ body runs (alone or inside the one-launch backward), head_dim 64, bias none or T5, its operands are staged through LDS, and a
workgroup has at most 16 key steps (512 keys).  Legal means taken; FAT5_V_KVRES_ON / _OFF force / forbid it inside what is legal."""
import pytest


def _d(**kw):
    from flasht5_amd import _lib as L
    return L.describe(**kw)


def test_kvres_rule():
    from flasht5_amd import _lib as L
    if L.load().fat5_chip_cus() != 256:  # (which shapes take the 64-row body at all follows the chip's size, as in test_dispatch_rules_are_pinned)
        pytest.skip("dispatch rules are pinned for a 256-CU device (MI355X) or no device at all")
    rpe = dict(bias_mode=L.BIAS_RPE1D, radius=128, need_dbias=True)
    F = L.V_FUSED64_ON
    cases = [
        (dict(B=4, H=12, M=512, N=512, **rpe), "1"),                        # the benchmark's shape, plain call
        (dict(B=4, H=12, M=512, N=512), "1"),                               # ... without bias
        (dict(B=4, H=12, M=512, N=512, causal=True, **rpe), "1"),           # ... causal (the table carries the mask)
        (dict(B=16, H=12, M=512, N=512, **rpe), "1"),                       # several rounds of workgroups: the form follows the body, not the grid
        (dict(B=4, H=12, M=512, N=512, dtype=L.FAT5_F16, **rpe), "1"),
        (dict(B=4, H=12, M=512, N=512, variant=L.V_KVRES_OFF, **rpe), "0"),
        (dict(B=4, H=12, M=512, N=512, variant=L.V_KVRES_ON, **rpe), "1"),
        (dict(B=1, H=2, M=256, N=512, variant=F, **rpe), "1"),              # 16 steps: the last slot
        (dict(B=1, H=2, M=256, N=513, variant=F, **rpe), "0"),              # 17 steps
        (dict(B=1, H=2, M=256, N=544, variant=F | L.V_KVRES_ON, **rpe), "0"),   # ... forcing changes nothing: the form does not exist there
        (dict(B=1, H=2, M=64, N=32, variant=F, **rpe), "1"),
        (dict(B=1, H=2, M=2048, N=500, variant=F), "1"),
        (dict(B=1, H=2, M=512, N=512, variant=F, bias_mode=L.BIAS_RPE1D, radius=512, need_dbias=True), "0"),            # radius 512: the operands are not staged
        (dict(B=1, H=2, M=512, N=512, variant=F | L.V_KVRES_ON, bias_mode=L.BIAS_RPE1D, radius=512, need_dbias=True), "0"),
        (dict(B=1, H=2, M=512, N=512, variant=F, bias_mode=L.BIAS_RPE1D, radius=16, need_dbias=True), "1"),
        (dict(B=1, H=2, M=512, N=512, variant=L.V_Q64_ON | L.V_FUSED64_OFF, **rpe), "1"),   # the stand-alone dQ kernel takes the form as well
        (dict(B=1, H=2, M=512, N=512, variant=L.V_Q64_OFF | L.V_FUSED64_OFF, **rpe), "0"),  # the 32-row body has no such form
        (dict(B=4, H=12, M=2048, N=2048, **rpe), "0"),
        (dict(B=4, H=12, M=512, N=512, bias_mode=L.BIAS_DENSE, need_dbias=True), "0"),
        (dict(B=4, H=12, M=512, N=512, D=128), "0"),
    ]
    for kw, want in cases:
        d = _d(**kw)
        assert d["kvres"] == want, (kw, d)
        if want == "1":
            assert d["dq"] == "64row", (kw, d)


def test_kvres_changes_neither_workspace_nor_launch_count():
    """the form is a property of the dQ workgroups alone: same workspace, same launches, same other fields with the bit on and off"""
    import ctypes
    from flasht5_amd import _lib as L
    rpe = dict(bias_mode=L.BIAS_RPE1D, radius=128, need_dbias=True)
    for kw in (dict(B=4, H=12, M=512, N=512, **rpe), dict(B=2, H=3, M=300, N=200), dict(B=1, H=2, M=512, N=160, causal=True, **rpe)):
        on, off = _d(variant=L.V_FUSED64_ON | L.V_KVRES_ON, **kw), _d(variant=L.V_FUSED64_ON | L.V_KVRES_OFF, **kw)
        assert on.pop("kvres") == "1" and off.pop("kvres") == "0"
        assert on == off


def test_the_describe_text_keeps_its_fields():
    """kvres travels through a call of its own: the text of fat5_attn_describe has the fields it had (tests/dispatch_snapshot.txt records them)"""
    import ctypes
    from flasht5_amd import _lib as L
    p = L.AttnParams()
    p.B, p.H, p.M, p.N, p.D = 4, 12, 512, 512, 64
    p.dtype, p.sm_scale = L.FAT5_BF16, 0.125
    buf = ctypes.create_string_buffer(256)
    L.check(L.load().fat5_attn_describe(ctypes.byref(p), buf, 256), "fat5_attn_describe")
    keys = [kv.split("=")[0] for kv in buf.value.decode().split()]
    assert keys == ["fwd", "dq", "dkdv", "fused", "dbias", "qdiag"], keys
    assert L.load().fat5_attn_bwd_kvres(ctypes.byref(p)) == 1
    p.N = 544
    assert L.load().fat5_attn_bwd_kvres(ctypes.byref(p)) == 0
    p.D = 7   # (invalid parameters: 0, like fat5_attn_bwd_launches)
    assert L.load().fat5_attn_bwd_kvres(ctypes.byref(p)) == 0
