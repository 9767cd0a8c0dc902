"""CPU tests of the rotary position embedding: the host table builder against the reference's tables (tests/golden/rope_tables.npz,
tests/golden/make_golden_rope.py), the C ABI's argument checks (all before any launch: fake, aligned pointers are enough) and the
ctypes mirror of fat5_rope_params."""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_io import GOLDEN

DTYPES = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def _tensor(a, dtype):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


def _bits(t):
    return t.view(torch.int16).to(torch.int32) if t.element_size() == 2 else t.view(torch.int32)


def _same(mine, ref):
    """bit for bit (torch's CPU cos / sin give these tables the same bits on its scalar, AVX2 and AVX-512 code paths)"""
    assert mine.dtype == ref.dtype and mine.shape == ref.shape
    assert torch.equal(_bits(mine), _bits(ref)), int((_bits(mine) != _bits(ref)).sum())


def test_host_tables_match_reference():
    from flasht5_amd.rotary import rotary_tables
    z = np.load(os.path.join(GOLDEN, "rope_tables.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    assert len(names) == 5
    for name in names:
        dim, rows, base, scale_base, code = z[f"{name}__meta"].tolist()
        dtype = DTYPES[int(code)]
        cos, sin, cos_k, sin_k = rotary_tables(int(dim), int(rows), base, None if scale_base < 0 else scale_base, dtype)
        assert cos.shape == (int(rows), int(dim) // 2)
        _same(cos, _tensor(z[f"{name}__cos"], dtype))
        _same(sin, _tensor(z[f"{name}__sin"], dtype))
        if scale_base < 0:
            assert cos_k is None and sin_k is None
        else:
            _same(cos_k, _tensor(z[f"{name}__cos_k"], dtype))
            _same(sin_k, _tensor(z[f"{name}__sin_k"], dtype))


def test_bf16_positions_are_quantised_like_the_reference():
    """the reference's positions are arange(seqlen) in the tables' dtype: in bf16, 255..261 -> 255, 256, 256, 258, 260, 260, 260"""
    from flasht5_amd.rotary import rotary_tables
    cos, sin, _, _ = rotary_tables(2, 300, dtype=torch.bfloat16)  # inv_freq = [1]: sin[p] = sin(position)
    pos = torch.arange(300, dtype=torch.bfloat16).float()
    assert pos[255:262].tolist() == [255, 256, 256, 258, 260, 260, 260]
    assert torch.equal(sin[:, 0], torch.sin(pos).to(torch.bfloat16))
    assert torch.equal(sin[256], sin[257]) and not torch.equal(sin[257], sin[258])


def test_module_buffers_and_signature():
    from flasht5_amd import RotaryPositionalEncoding
    m = RotaryPositionalEncoding(64, 1024, 10000.0, False, 512)
    assert torch.allclose(m.inv_freq, 1.0 / 10000.0 ** (torch.arange(0, 64, 2).float() / 64))
    assert torch.allclose(m.scale, (torch.arange(0, 64, 2).float() + 0.4 * 64) / (1.4 * 64))
    assert RotaryPositionalEncoding(32, 16).scale is None
    assert "inv_freq" not in m.state_dict()  # (non-persistent, as in the reference: RoPE checkpoints carry no table)


def test_sizeof_rope_params_matches_mirror(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_rope_params() == ctypes.sizeof(_lib.RopeParams)
    assert "fat5_rope_apply" in _lib.EXPORTS and "fat5_sizeof_rope_params" in _lib.EXPORTS


def _good():
    from flasht5_amd import _lib
    p = _lib.RopeParams()
    p.B, p.S, p.H, p.D, p.rd = 2, 128, 12, 64, 64
    p.dtype, p.n_tensors, p.n_q, p.table_rows = _lib.FAT5_BF16, 3, 1, 1024
    p.cos, p.sin = 0x10000, 0x20000
    for i in range(3):
        p.x[i], p.y[i] = 0x100000 * (i + 1), 0x100000 * (i + 4)
        for d, s in enumerate((128 * 12 * 64, 12 * 64, 64)):
            p.x_stride[i][d] = p.y_stride[i][d] = s
    return p


@pytest.mark.parametrize("what,mutate,msg", [
    ("odd rd", lambda p: setattr(p, "rd", 31), b"rd 31"),
    ("oversized rd", lambda p: setattr(p, "rd", 66), b"rd 66"),
    ("zero rd", lambda p: setattr(p, "rd", 0), b"rd 0"),
    ("positions beyond the table", lambda p: setattr(p, "table_rows", 127), b"beyond the table"),
    ("keys beyond the table", lambda p: setattr(p, "S_k", 2048), b"beyond the table"),
    ("null x", lambda p: p.x.__setitem__(1, None), b"null or unaligned"),
    ("null y", lambda p: p.y.__setitem__(2, None), b"null or unaligned"),
    ("misaligned x", lambda p: p.x.__setitem__(0, 0x100008), b"null or unaligned"),
    ("misaligned stride", lambda p: p.x_stride[1].__setitem__(1, 12 * 64 + 4), b"multiples of 8"),
    ("null table", lambda p: setattr(p, "sin", None), b"null cos / sin"),
    ("half an xPos pair", lambda p: setattr(p, "cos_k", 0x30000), b"go together"),
    ("dtype", lambda p: setattr(p, "dtype", 7), b"dtype 7"),
    ("head_dim", lambda p: setattr(p, "D", 48), b"head_dim 48"),
    ("tensor count", lambda p: setattr(p, "n_tensors", 4), b"n_tensors 4"),
])
def test_bad_rope_arguments_are_rejected_without_gpu(lib, what, mutate, msg):
    p = _good()
    mutate(p)
    assert lib.fat5_rope_apply(ctypes.byref(p), None) == -1, what
    assert msg in lib.fat5_last_error(), (what, lib.fat5_last_error())


def test_empty_problem_is_a_no_op(lib):
    p = _good()
    p.B = 0
    assert lib.fat5_rope_apply(ctypes.byref(p), None) == 0
    p = _good()
    p.S = 0
    assert lib.fat5_rope_apply(ctypes.byref(p), None) == 0


def test_python_checks_without_gpu():
    from flasht5_amd import apply_rotary_emb
    from flasht5_amd.rotary import rotary_tables
    cos, sin, _, _ = rotary_tables(64, 16, dtype=torch.bfloat16)
    x = torch.zeros(1, 32, 2, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="beyond the table"):
        apply_rotary_emb(x, cos, sin)
    with pytest.raises(ValueError, match="rotated width"):
        apply_rotary_emb(torch.zeros(1, 8, 2, 32, dtype=torch.bfloat16), cos, sin)


def test_tensors_of_one_table_group_must_share_their_length():
    """the kernel bounds every tensor of a table group (q | k and v) by one sequence length: unequal lengths, or packed buffers whose
    widths are not their tensor counts x heads x head_dim, are rejected before any launch (CPU tensors: nothing reaches a device)"""
    from flasht5_amd import apply_rotary_emb_qkv, apply_rotary_emb_packed
    from flasht5_amd.rotary import rotary_tables, _launch
    cos, sin, _, _ = rotary_tables(64, 512, dtype=torch.bfloat16)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16)  # noqa: E731
    q = z(2, 64, 4, 64)
    with pytest.raises(ValueError, match="share their sequence length"):
        apply_rotary_emb_qkv(q, z(2, 96, 4, 64), z(2, 80, 4, 64), cos, sin)  # v shorter than k
    with pytest.raises(ValueError, match="share their sequence length"):
        apply_rotary_emb_qkv(q, z(2, 96, 4, 64), z(2, 128, 4, 64), cos, sin)  # v longer than k
    with pytest.raises(ValueError, match="batch"):
        apply_rotary_emb_qkv(q, z(1, 96, 4, 64), z(1, 96, 4, 64), cos, sin)
    with pytest.raises(ValueError, match="same number of tokens"):
        cu = torch.tensor([0, 10, 30], dtype=torch.int32)
        apply_rotary_emb_qkv(z(30, 4, 64), z(30, 4, 64), z(31, 4, 64), cos, sin, cu_seqlens=cu, max_seqlen=20)
    # packed: q and the k | v buffer in one group (nq = 2) with different lengths; a buffer narrower / wider than its tensors
    with pytest.raises(ValueError, match="share their sequence length"):
        apply_rotary_emb_packed((z(2, 64, 4 * 64), z(2, 96, 2 * 4 * 64)), (1, 2), 4, cos, sin, nq=2)
    with pytest.raises(ValueError, match="buffer widths"):
        apply_rotary_emb_packed((z(2, 64, 4 * 64), z(2, 96, 4 * 64)), (1, 2), 4, cos, sin, nq=1)
    with pytest.raises(ValueError, match="buffer widths"):
        apply_rotary_emb_packed((z(2, 64, 3 * 4 * 64 + 8),), (3,), 4, cos, sin)
    # the launcher itself (the custom ops' common path) checks the same, and that outputs match their inputs
    with pytest.raises(ValueError, match="share their sequence length"):
        _launch([q, z(2, 96, 4, 64), z(2, 80, 4, 64)], [q, q, q], cos, sin, None, None, 1, False, False, None, 0)
    with pytest.raises(ValueError, match="input's shape"):
        _launch([q], [z(2, 63, 4, 64)], cos, sin, None, None, 1, False, False, None, 0)
