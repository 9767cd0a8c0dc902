"""CPU tests of chunked KV-cache attention and decoder prompts: the C ABI's argument checks of fat5_attn_decode_chunk (all before any
launch: fake, aligned pointers are enough), the ctypes mirror, the workspace query, the custom op's fake implementation, the
Python-side rejections of the operator, of `decode_chunk` and of `generate(decoder_input_ids=...)` (before the encoder runs), and
what tests/test_decode_chunk_gpu.py rests on: the fp64 restatement equals the one-row restatement row by row, and its bound tells
every applicable mutant from the truth on that file's own inputs."""
import ctypes

import pytest
import torch

import decode_chunk_fp64 as C
import decode_fp64 as F
from test_decode_chunk_gpu import CASES, inputs, reference

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch)
DETECTED = {name: [0, 0] for name in C.MUTANTS}   # [cases where it applied, cases where the bound caught it]


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.DecodeChunkParams()
    B, H, M, D, cap = 2, 4, 5, 64, 256
    p.B, p.H, p.M, p.D, p.dtype, p.capacity, p.N, p.causal = B, H, M, D, _lib.FAT5_BF16, cap, 0, 1
    p.cache_seqlens = BASE
    p.sm_scale = 0.125
    for i, f in enumerate(("q", "k_cache", "v_cache", "k_new", "v_new", "o", "lse")):
        setattr(p, f, BASE + 65536 * (i + 1))
    for f in ("q", "o", "k_new", "v_new"):
        getattr(p, f + "_stride")[:] = (M * H * D, H * D, D)
    p.k_cache_stride[:] = (cap * H * D, H * D, D)
    p.v_cache_stride[:] = (cap * H * D, H * D, D)
    p.num_splits = 1  # (no workspace needed unless a case asks for one)
    for k, v in kw.items():
        if k.endswith("_stride"):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    return p


def test_struct_size_matches_library(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_decode_chunk_params() == ctypes.sizeof(_lib.DecodeChunkParams)
    for name in ("fat5_attn_decode_chunk", "fat5_attn_decode_chunk_workspace_bytes", "fat5_sizeof_decode_chunk_params"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_constants_restated():
    assert (C.CHUNK_TQ, C.CHUNK_MAX_M) == (4, 1024) and C.CHUNK_MAX_M >= 512
    assert (F.groups(64), F.wg_pass(64), F.groups(128), F.wg_pass(128)) == (32, 128, 16, 64)
    from flasht5_amd.decode import MAX_CHUNK
    assert MAX_CHUNK == C.CHUNK_MAX_M


@pytest.mark.parametrize("bad, msg", [
    (dict(D=32), "head_dim"), (dict(D=96), "head_dim"), (dict(dtype=0), "dtype"), (dict(dtype=5), "dtype"),
    (dict(B=0), "B 0"), (dict(H=0), "H 0"), (dict(M=0), "M 0"), (dict(M=1025), "M 1025"), (dict(capacity=-1), "capacity"),
    (dict(causal=2), "causal"), (dict(num_splits=129), "num_splits"), (dict(num_splits=-1), "num_splits"),
    (dict(bias_mode=2, rpe_radius=0, rpe1d=BASE), "rpe_radius"), (dict(bias_mode=2, rpe_radius=2049, rpe1d=BASE), "rpe_radius"),
    (dict(bias_mode=2, rpe_radius=16, rpe1d=None), "needs rpe1d"), (dict(bias_mode=1), "bias_mode"),
    (dict(v_new=None), "both"), (dict(k_new=None), "both"), (dict(cache_seqlens=None), "needs cache_seqlens"),
    (dict(cache_seqlens=None, k_new=None, v_new=None, N=300), "N 300"), (dict(cache_seqlens=BASE + 2), "cache_seqlens misaligned"),
    (dict(q=None), "q:"), (dict(q=BASE + 8), "unaligned"), (dict(k_cache=BASE + 2), "k_cache"), (dict(o=None), "o:"),
    (dict(k_new=BASE + 4, v_new=BASE), "k_new"),
    (dict(q_stride=(5 * 4 * 64, 4 * 64, 60)), "multiples"), (dict(q_stride=(5 * 4 * 64, 4 * 64 + 4, 64)), "multiples"),
    (dict(k_cache_stride=(256 * 256, 256, 65)), "multiples"), (dict(v_new_stride=(3, 256, 64)), "multiples"),
    (dict(o_stride=(1280, 256, 63)), "multiples"), (dict(sm_scale=float("inf")), "sm_scale"), (dict(sm_scale=float("nan")), "sm_scale"),
    (dict(lse=BASE + 2), "lse misaligned"),
])
def test_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_attn_decode_chunk(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()
    assert "attn_decode_chunk" in lib.fat5_last_error().decode()


def test_null_params(lib):
    assert lib.fat5_attn_decode_chunk(None, None) == -1 and lib.fat5_attn_decode_chunk_workspace_bytes(None) == 0


def test_workspace_checked(lib):
    p = _params(num_splits=8)
    need = lib.fat5_attn_decode_chunk_workspace_bytes(ctypes.byref(p))
    assert need == 2 * 4 * 5 * 8 * (64 + 2) * 4  # [B][H][M][splits] (max, sum) + o[D], fp32
    assert lib.fat5_attn_decode_chunk(ctypes.byref(p), None) == -3
    assert "workspace" in lib.fat5_last_error().decode()
    p.workspace, p.workspace_bytes = BASE + (1 << 22), need - 16
    assert lib.fat5_attn_decode_chunk(ctypes.byref(p), None) == -3
    p.workspace, p.workspace_bytes = BASE + (1 << 22) + 8, need
    assert lib.fat5_attn_decode_chunk(ctypes.byref(p), None) == -3


def test_split_policy_is_host_known(lib):
    # one split (no workspace) when the capacity holds one workgroup pass; never more than 128; fewer as the chunk brings more tiles
    assert lib.fat5_attn_decode_chunk_workspace_bytes(ctypes.byref(_params(num_splits=0, capacity=33))) == 0
    last = None
    for M in (1, 4, 64, 1024):
        n = lib.fat5_attn_decode_chunk_workspace_bytes(ctypes.byref(_params(num_splits=0, B=1, M=M, capacity=1 << 16)))
        splits = n // (4 * M * (64 + 2) * 4) if n else 1
        assert 1 <= splits <= 128 and (last is None or splits <= last)
        last = splits
    assert last == 1   # 256 tiles * 4 heads: enough workgroups without a split


def test_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import decode  # noqa: F401  (registers the op)
    with FakeTensorMode():
        B, M, H, D, cap = 3, 5, 6, 64, 40
        q = torch.empty(B, M, H, D, dtype=torch.bfloat16)
        kc = torch.empty(B, H, cap, D, dtype=torch.bfloat16).transpose(1, 2)
        vc = torch.empty(B, cap, H, D, dtype=torch.bfloat16)
        lens = torch.empty(B, dtype=torch.int32)
        o, lse = torch.ops.fat5.attn_decode_chunk(q, kc, vc, q, q, lens, 0.125, True, None, 0, True, 0)
        assert o.shape == (B, M, H, D) and o.dtype == torch.bfloat16 and o.is_contiguous()
        assert lse.shape == (B, H, M) and lse.dtype == torch.float32 and lse.is_contiguous()
        o, lse = torch.ops.fat5.attn_decode_chunk(q, kc, vc, None, None, None, 0.125, False, None, 0, False, 0)
        assert o.shape == (B, M, H, D) and lse.numel() == 0
    schema = str(torch.ops.fat5.attn_decode_chunk.default._schema)
    assert "Tensor(a1!) k_cache" in schema and "Tensor(a2!) v_cache" in schema   # (the cache mutation is declared)


def test_python_rejections():
    import flasht5_amd
    from flasht5_amd.decode import flash_attn_with_kvcache_chunk
    assert flasht5_amd.flash_attn_with_kvcache_chunk is flash_attn_with_kvcache_chunk
    bf = torch.bfloat16
    q = torch.zeros(2, 3, 4, 64, dtype=bf)
    kc = torch.zeros(2, 16, 4, 64, dtype=bf)
    with pytest.raises(RuntimeError, match="forward only"):
        flash_attn_with_kvcache_chunk(q.clone().requires_grad_(), kc, kc)
    # shape / dtype / bias checks come before the device check: reachable on any host
    cases = [
        (dict(q=torch.zeros(2, 4, 64, dtype=bf)), ValueError, r"\(B, M, H, D\)"),
        (dict(q=torch.zeros(2, 1025, 4, 64, dtype=bf)), ValueError, "M <= 1024"),
        (dict(q=q.float(), k_cache=kc.float(), v_cache=kc.float()), TypeError, "fp16 or bf16"),
        (dict(q=q.half()), ValueError, "dtype mismatch"),
        (dict(q=torch.zeros(2, 3, 4, 32, dtype=bf), k_cache=torch.zeros(2, 16, 4, 32, dtype=bf),
              v_cache=torch.zeros(2, 16, 4, 32, dtype=bf)), ValueError, "head_dim"),
        (dict(k_cache=torch.zeros(2, 16, 3, 64, dtype=bf)), ValueError, "k_cache must be"),
        (dict(k_cache=torch.zeros(3, 16, 4, 64, dtype=bf)), ValueError, "k_cache must be"),
        (dict(v_cache=torch.zeros(2, 17, 4, 64, dtype=bf)), ValueError, "capacities"),
        (dict(k=q), ValueError, "both k and v"),
        (dict(k=q, v=q), ValueError, "needs cache_seqlens"),
        (dict(k=q[:, :2], v=q[:, :2], cache_seqlens=3), ValueError, r"k must be \(2, 3, 4, 64\)"),
        (dict(k=q, v=q, cache_seqlens=torch.zeros(3, dtype=torch.int32)), ValueError, "2 lengths"),
        (dict(rpe1d=torch.zeros(4, 257), rpe_radius=0), ValueError, "rpe_radius 0"),
        (dict(rpe1d=torch.zeros(4, 129), rpe_radius=128), ValueError, r"\(4, 257\)"),
        (dict(rpe1d=torch.zeros(3, 257), rpe_radius=128), ValueError, "rpe1d must be"),
        (dict(rpe1d=torch.zeros(4, 257, dtype=torch.float64), rpe_radius=128), ValueError, "rpe1d must be"),
        (dict(), ValueError, "GPU"),
    ]
    for kw, exc, msg in cases:
        args = dict(q=q, k_cache=kc, v_cache=kc)
        args.update(kw)
        with pytest.raises(exc, match=msg):
            flash_attn_with_kvcache_chunk(**args)


def _small_config(**kw):
    from flasht5_amd import FAT5Config
    base = dict(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                relative_attention_max_distance=64, max_sequence_length=64)
    base.update(kw)
    return FAT5Config(**base)


class _EncoderRan(Exception):
    pass


def _no_encoder(m):
    def boom(*a, **k):
        raise _EncoderRan()
    m.encoder.forward = boom
    return m


def test_generate_rejections_come_before_the_encoder():
    from flasht5_amd import FAT5ForConditionalGeneration
    m = _no_encoder(FAT5ForConditionalGeneration(_small_config()))
    ids = torch.zeros(2, 4, dtype=torch.long)
    ok = torch.tensor([[0, 5, 6], [0, 7, 8]])
    with pytest.raises(_EncoderRan):   # (a valid prompt gets as far as the encoder)
        m.generate(ids, decoder_input_ids=ok)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(ids, decoder_input_ids=ok, num_beams=2)
    with pytest.raises(ValueError, match="EOS"):
        m.generate(ids, decoder_input_ids=torch.tensor([[0, 5, 6], [0, 1, 8]]))
    with pytest.raises(ValueError, match="3 rows"):
        m.generate(ids, decoder_input_ids=torch.zeros(3, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m.generate(ids, decoder_input_ids=torch.tensor([[0, 5], [0, 128]]))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        m.generate(ids, decoder_input_ids=torch.tensor([[0, 5], [0, -1]]))
    for bad in (torch.zeros(2, 0, dtype=torch.long), torch.zeros(2, dtype=torch.long), torch.zeros(2, 2, dtype=torch.int32), [[0], [0]]):
        with pytest.raises(ValueError, match=r"\(B, P\) int64"):
            m.generate(ids, decoder_input_ids=bad)
    # the processors' 4096 columns count the prompt
    with pytest.raises(ValueError, match="4096 sequence columns"):
        m.generate(ids, max_length=4094, decoder_input_ids=ok, repetition_penalty=1.2)
    with pytest.raises(_EncoderRan):
        m.generate(ids, max_length=4093, decoder_input_ids=ok, repetition_penalty=1.2)
    # ... and so do the rotary tables (64 rows here)
    r = _no_encoder(FAT5ForConditionalGeneration(_small_config(position_encoding_type="RoPE")))
    with pytest.raises(ValueError, match="rotary tables"):
        r.generate(ids, max_length=62, decoder_input_ids=ok)
    with pytest.raises(_EncoderRan):
        r.generate(ids, max_length=61, decoder_input_ids=ok)
    with pytest.raises(ValueError, match="rotary tables"):
        r.init_decode_state(ids, max_length=60, prompt_length=5)


def test_decode_chunk_host_refusals():
    from flasht5_amd import FAT5ForConditionalGeneration
    from flasht5_amd.generation import DecodeState
    m = FAT5ForConditionalGeneration(_small_config())
    z = torch.zeros(2, 8, 2, 64)
    state = DecodeState(torch.zeros(2, 3, 64), [z, z], [z, z], [z, z], [z, z], torch.full((2,), 6, dtype=torch.int32), None, 8, steps=6)
    with pytest.raises(ValueError, match="the chunk brings 3"):
        m.decode_chunk(state, torch.zeros(2, 3, dtype=torch.long))
    assert state.steps == 6
    with pytest.raises(ValueError, match=r"\(B, M\)"):
        m.decode_chunk(state, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError, match="logits"):
        m.decode_chunk(state, torch.zeros(2, 2, dtype=torch.long), logits="first")
    state.row_batch = torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="beam-search state"):
        m.decode_chunk(state, torch.zeros(2, 2, dtype=torch.long))
    attn = m.decoder.block[0].self_attention_layer.self_attention
    with pytest.raises(ValueError, match="one query row"):
        attn.forward_decode(torch.zeros(2, 2, 64), z, z, torch.zeros(2, dtype=torch.int32), cache_row_batch=state.row_batch)


# ---------------------------------------------------------------------------------------- the restatement, the bound, the mutants
@pytest.mark.parametrize("bias", [True, False])
def test_rows_equal_the_one_row_restatement(bias):
    """causal append: row i is decode_fp64.decode_ref at lens + i with new row i and the caches after the rows before it -- overflow
    (rows that no longer fit), a full cache, a length past the capacity and a negative one included"""
    g = torch.Generator().manual_seed(3)
    B, M, H, D, cap, R = 5, 6, 2, 64, 40, 8
    for lens in ([0, 17, 37, 40, 45], [-2, 34, 35, 39, 1]):
        rn = lambda *s: torch.randn(*s, generator=g).bfloat16()  # noqa: E731
        q, kn, vn, kc, vc = rn(B, M, H, D), rn(B, M, H, D), rn(B, M, H, D), rn(B, cap, H, D), rn(B, cap, H, D)
        rpe = torch.randn(H, 2 * R + 1, generator=g) if bias else None
        ref = C.chunk_ref(q, kc, vc, kn, vn, lens, 0.125, True, rpe, R if bias else 0)
        k, v = kc, vc
        for i in range(M):
            # (decode_ref clamps its lengths as the kernel does; a negative length stays at 0 + i for the rows that follow)
            li = [max(0, n) + i for n in lens]
            one = F.decode_ref(q[:, i], k, v, kn[:, i], vn[:, i], li, 0.125, rpe, R if bias else 0)
            assert float((one["o"] - ref["o"][:, i]).abs().max()) <= 1e-12
            fin = torch.isfinite(one["lse"])
            assert torch.equal(torch.isfinite(ref["lse"][:, i]), fin) and float((one["lse"] - ref["lse"][:, i])[fin].abs().max()) <= 1e-12
            for name in ("absv", "smag", "bmag", "srange"):
                assert float((one[name] - ref[name][:, i]).abs().max()) <= 1e-12, name
            k, v = one["kc"], one["vc"]
        assert torch.equal(k, ref["kc"]) and torch.equal(v, ref["vc"])


def test_no_append_is_bottom_right_aligned():
    """without an append p_i = L - M + i: causal rows equal one-row calls over the first p_i + 1 keys; rows at negative positions are empty"""
    g = torch.Generator().manual_seed(4)
    B, M, H, D, cap, R = 2, 7, 2, 64, 30, 4
    rn = lambda *s: torch.randn(*s, generator=g).bfloat16()  # noqa: E731
    q, kc, vc = rn(B, M, H, D), rn(B, cap, H, D), rn(B, cap, H, D)
    rpe = torch.randn(H, 2 * R + 1, generator=g)
    lens = [4, 29]
    ref = C.chunk_ref(q, kc, vc, None, None, lens, 0.125, True, rpe, R)
    for i in range(M):
        li = [max(0, n - M + i + 1) for n in lens]
        one = F.decode_ref(q[:, i], kc, vc, None, None, li, 0.125, rpe, R)
        assert float((one["o"] - ref["o"][:, i]).abs().max()) <= 1e-12
        assert torch.equal(torch.isfinite(ref["lse"][:, i]), torch.isfinite(one["lse"]))
    assert ref["nvis"][0][:3] == [0, 0, 0] and ref["nvis"][0][3] == 1 and bool((ref["o"][0, :3] == 0).all())
    full = C.chunk_ref(q, kc, vc, None, None, None, 0.125, False)
    assert full["L"] == [cap, cap] and full["nvis"][1] == [cap] * M


def test_the_case_table_is_what_the_issue_asks_for():
    TQ = C.CHUNK_TQ
    assert {c["D"] for c in CASES} == {64, 128} and {c["dtype"] for c in CASES} == {torch.bfloat16, torch.float16}
    for D in (64, 128):
        P = F.wg_pass(D)
        edge = [c for c in CASES if c["kind"] == "edge" and c["D"] == D]
        assert {c["M"] for c in edge} == {1, TQ - 1, TQ, TQ + 1, 2 * TQ + 1}
        for M in (1, TQ - 1, TQ, TQ + 1, 2 * TQ + 1):
            assert {(c["lens"][0] + M) - P for c in edge if c["M"] == M} == {-1, 0, 1}
        assert {c["splits"] for c in CASES if c["kind"] == "split" and c["D"] == D} == {1, 2, 3}
    for c in CASES:
        assert c["lens"] is None or c["lens"][0] != c["lens"][1]
        if c["kind"] == "split":
            assert all((n + c["M"]) % 2 and (n + c["M"]) % 3 for n in c["lens"])
    kinds = {c["kind"] for c in CASES}
    assert kinds == {"edge", "split", "empty", "radius1", "cross", "cross-bias", "masked", "overflow"}
    assert any(c["lens"] is None for c in CASES if c["kind"] == "cross")
    assert all(c["M"] > max(c["lens"]) for c in CASES if c["kind"] == "masked")
    over = [n for c in CASES if c["kind"] == "overflow" for n in c["lens"]]
    assert any(n < 0 for n in over) and any(n == 40 for n in over) and any(n > 40 for n in over) and any(0 < n < 40 for n in over)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_applicable_mutant_violates_the_bound(case):
    ln = inputs(case)
    ref = reference(case, ln)
    bo, bl = C.chunk_bound(ref, case["dtype"], case["D"], case["splits"])
    # correct arithmetic satisfies the bound: the fp64 result rounded once to the storage dtype
    ro, rl, same = C.ratios(ref["o"].to(case["dtype"]), ref["lse"].float(), ref, bo, bl)
    assert same and ro <= 1.0 and rl <= 1.0, (case["id"], ro, rl)
    for name, mutant in C.MUTANTS.items():
        mut = reference(case, ln, mutant)
        if not mut["applied"]:
            continue
        caught = not C.within(mut["o"], mut["lse"], ref, bo, bl)
        DETECTED[name][0] += 1
        DETECTED[name][1] += caught
        assert caught, f"{case['id']}: the bound does not see the mutant '{name}'"


def test_zz_every_mutant_applied_and_was_caught():
    """(runs last) per mutant: the cases where it applied, and where the bound caught it -- all of them"""
    if sum(a for a, _ in DETECTED.values()) == 0:
        return  # (the mutant test was deselected in this session)
    for name, (applied, caught) in DETECTED.items():
        print(f"[decode-chunk] mutant '{name}': applied in {applied} cases, caught in {caught}")
    for name, (applied, caught) in DETECTED.items():
        assert applied >= 3 and caught == applied, (name, applied, caught)
