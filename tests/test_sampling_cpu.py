"""CPU tests of sampling: the Python Philox4x32-10 against the Random123 known-answer vectors, the fp64 restatement's kept set
against HF's warpers, the C ABI's rejections of fat5_sample_logits (before any launch: fake, aligned pointers are enough), the
ctypes mirror, the custom op's fake implementation and the host-side validation of the sampling arguments of `generate`."""
import ctypes

import numpy as np
import pytest
import torch

from sampling_ref import philox4x32_10, restate, scaled, uniform

BASE = 1 << 20  # (never dereferenced: every call below is rejected before a launch, or is a B == 0 no-op)


def test_philox_known_answers():
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    assert uniform(0, 0, 0) == (0x6627E8D5 >> 8) * 2.0 ** -24


def test_restatement_kept_set_matches_hf():
    tr = pytest.importorskip("transformers")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    g = torch.Generator().manual_seed(0)
    V, rows = 1000, 6
    checked = 0
    for T in (0.5, 1.0, 1.7):
        for k in (0, 1, 50, V):
            for p in (0.05, 0.9, 1.0):
                logits = torch.randn(rows, V, generator=g) * 3
                s = TemperatureLogitsWarper(T)(None, logits.clone())
                if k:
                    s = TopKLogitsWarper(k)(None, s)
                s = TopPLogitsWarper(p)(None, s)
                for b in range(rows):
                    r = restate(scaled(logits[b], T), k, p)
                    if r["margin"] < 1e-4:  # (a top-p boundary within HF's fp32 cumsum rounding: either answer is right)
                        continue
                    hf = torch.isfinite(s[b]).numpy()
                    assert np.array_equal(r["kept"], hf), (T, k, p, b)
                    checked += 1
    assert checked > 0.9 * 3 * 4 * 3 * rows


def test_restatement_ties_at_the_threshold_are_kept():
    x = np.array([3.0, 1.0, 2.0, 2.0, 2.0, 0.0], dtype=np.float32)
    assert restate(x, 2, 1.0)["kept"].tolist() == [True, False, True, True, True, False]
    assert restate(x, 0, 1e-6)["kept"].tolist() == [True, False, False, False, False, False]


@pytest.fixture(scope="module")
def lib():
    from flasht5_amd import _lib
    return _lib.load()


def _params(**kw):
    from flasht5_amd import _lib
    p = _lib.SampleParams()
    p.B, p.V, p.dtype, p.top_k = 4, 32128, _lib.FAT5_BF16, 50
    p.logits, p.row_stride = BASE, 32128
    p.temperature, p.top_p = 0.7, 0.9
    p.seed, p.offset = 1, 0
    p.tokens = BASE + 4096
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_struct_size_matches_library(lib):
    from flasht5_amd import _lib
    assert lib.fat5_sizeof_sample_params() == ctypes.sizeof(_lib.SampleParams)
    assert "fat5_sample_logits" in _lib.EXPORTS and "fat5_sizeof_sample_params" in _lib.EXPORTS


@pytest.mark.parametrize("bad, msg", [
    (dict(B=-1), "B -1"), (dict(V=0), "V 0"), (dict(V=(1 << 20) + 1), "V 1048577"), (dict(dtype=7), "dtype"),
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(top_k=-1), "top_k"), (dict(top_p=0.0), "top_p"),
    (dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(row_stride=100), "row_stride"),
    (dict(logits=None), "logits"), (dict(logits=BASE + 1), "logits"), (dict(tokens=None), "tokens"), (dict(tokens=BASE + 4), "tokens"),
    (dict(offsets=BASE + 2), "offsets"), (dict(uniforms=BASE + 1), "uniforms"), (dict(aux=BASE + 2), "aux"),
])
def test_rejects_before_launch(lib, bad, msg):
    p = _params(**bad)
    assert lib.fat5_sample_logits(ctypes.byref(p), None) == -1
    assert msg in lib.fat5_last_error().decode()


def test_empty_batch_is_a_no_op(lib):
    assert lib.fat5_sample_logits(ctypes.byref(_params(B=0)), None) == 0


def test_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flasht5_amd import sampling  # noqa: F401  (registers the op)
    with FakeTensorMode():
        logits = torch.empty(5, 32128, dtype=torch.bfloat16)
        tok, aux = torch.ops.fat5.sample_logits(logits, 0.7, 50, 0.9, 3, 0, None, None, True)
        assert tok.shape == (5,) and tok.dtype == torch.int64
        assert aux.shape == (5, 4) and aux.dtype == torch.float32
        tok, aux = torch.ops.fat5.sample_logits(logits, 1.0, 0, 1.0, 3, 0, None, None, False)
        assert aux.numel() == 0


def test_python_rejections():
    from flasht5_amd import sample_logits
    x = torch.zeros(2, 10)
    for kw, exc, msg in [
        (dict(temperature=0.0), ValueError, "temperature"), (dict(top_k=-1), ValueError, "top_k"), (dict(top_k=2.5), ValueError, "top_k"),
        (dict(top_p=0.0), ValueError, "top_p"), (dict(top_p=1.01), ValueError, "top_p"),
        (dict(offsets=torch.zeros(3, dtype=torch.int32)), ValueError, r"offsets must be \(2,\)"),
        (dict(), ValueError, "GPU"),
    ]:
        with pytest.raises(exc, match=msg):
            sample_logits(x, **kw)
    with pytest.raises(ValueError, match=r"\(B, V\)"):
        sample_logits(torch.zeros(10))
    with pytest.raises(TypeError, match="dtype"):
        sample_logits(torch.zeros(2, 10, dtype=torch.float64))


def _small_model():
    from flasht5_amd import FAT5Config, FAT5ForConditionalGeneration
    c = FAT5Config(vocab_size=128, d_model=64, d_kv=64, d_ff=128, num_heads=2, num_layers=1, num_decoder_layers=2,
                   relative_attention_max_distance=64, max_sequence_length=64)
    return FAT5ForConditionalGeneration(c)


@pytest.mark.parametrize("kw, msg", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(top_k=-3), "top_k"),
    (dict(top_k=True), "top_k"), (dict(top_p=0.0), "top_p"), (dict(top_p=2.0), "top_p"),
])
def test_generate_validates_sampling_arguments_before_the_encoder(kw, msg):
    m = _small_model()
    m.encoder.forward = None  # (reaching the encoder would raise a TypeError instead)
    with pytest.raises(ValueError, match=msg):
        m.generate(torch.zeros(1, 4, dtype=torch.long), do_sample=True, **kw)


def test_greedy_generate_neither_checks_nor_uses_sampling_arguments():
    m = _small_model()

    class Reached(Exception):
        pass

    def enc(*a, **k):
        raise Reached()
    m.encoder.forward = enc  # (the first device work: reaching it means no sampling argument was rejected)
    for kw in (dict(top_k=None), dict(temperature=0.0, top_p=5.0), dict(top_k=-1)):
        with pytest.raises(Reached):
            m.generate(torch.zeros(1, 4, dtype=torch.long), **kw)
