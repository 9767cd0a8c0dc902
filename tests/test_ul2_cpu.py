"""CPU tests of the UL2 collator: the host restatement of the contract (tests/ul2_ref.py) against the reference
collator's recorded runs (tests/golden/ul2_collator.npz, made by tests/golden/make_golden_ul2.py), `ul2_lengths` against the
reference's recorded optima, the library's exports and descriptor size, every host check, and the uniformity of the contract's
random segmentation."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import ul2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ul2_collator.npz")))


def fixture_tables(fx):
    """the fixture's denoisers as the host tables of flasht5_amd.ul2 (any object with these keys serves the restatement)"""
    D = len(fx["den_mu"])
    return dict(mu=[float(x) for x in fx["den_mu"]], r=[float(x) for x in fx["den_r"]], max_spans=[int(x) for x in fx["den_max_spans"]],
                tokens_len=[int(x) for x in fx["optimal_len"][0, :, 0]], prefix_off=[int(x) for x in fx["prefix_off"]],
                prefix_ids=[int(x) for x in fx["prefix_ids"]], cum_prop=[(i + 1) / D for i in range(D)])


def fixture_args(fx):
    first, count, eos, pad = (int(x) for x in fx["vocab"])
    ml, mll = (int(x) for x in fx["settings"][0])
    return dict(max_length=ml, max_labels_length=mll, sentinel_first_id=first, num_sentinels=count, eos_token_id=eos, pad_token_id=pad)


def fixture_denoisers(fx):
    off = fx["prefix_off"]
    return [dict(mu=float(fx["den_mu"][d]), r=float(fx["den_r"][d]), max_spans=int(fx["den_max_spans"][d]),
                 prefix_ids=[int(x) for x in fx["prefix_ids"][off[d]:off[d + 1]]]) for d in range(len(off) - 1)]


def test_restatement_reproduces_the_reference(fx):
    """given-mask mode on the recorded masks: input_ids and labels bit-equal on every recorded case, nothing flagged"""
    assert len(fx["lengths"]) >= 1000
    got = ul2_ref.collate(fx["tokens"], fx["lengths"], fixture_tables(fx), seed=0, step=0, noise_mask=fx["mask"], denoiser=fx["denoiser"],
                          **fixture_args(fx))
    assert np.array_equal(got["input_ids"], fx["ref_input_ids"].astype(np.int64))
    assert np.array_equal(got["labels"], fx["ref_labels"].astype(np.int64))
    assert got["status"][0] == 0 and got["status"][1] == 0
    assert np.array_equal(got["attention_mask"], fx["ref_input_ids"] != fixture_args(fx)["pad_token_id"])
    assert np.array_equal(got["decoder_attention_mask"], fx["ref_labels"] != -100)


def test_span_counts_equal_the_recorded_masks(fx):
    """(noise, spans) of the contract = the noise tokens and noise runs of the mask the reference drew; the S-denoiser's mask itself"""
    tab, a = fixture_tables(fx), fixture_args(fx)
    half_even = 0
    for n, d, m in zip(fx["lengths"], fx["denoiser"], fx["mask"]):
        n, d = int(n), int(d)
        m = m[:n].astype(bool)
        if tab["max_spans"][d] == 1:
            mask, _ = ul2_ref.draw_mask(n, tab["mu"][d], tab["r"][d], 1, a["num_sentinels"], 0, 0, 0)
            assert mask == list(m), (n, d)
            continue
        runs = int(m[0]) + int(np.count_nonzero(m[1:] & ~m[:-1]))
        assert ul2_ref.span_counts(n, tab["mu"][d], tab["r"][d], tab["max_spans"][d], a["num_sentinels"]) == (int(m.sum()), runs), (n, d)
        assert not m[0]    # (the layout starts with non-noise)
        half_even += tab["r"][d] == 0.5 and n % 2 == 1
    assert half_even > 100   # (the sweep crossed the n * 0.5 ties)


def test_cases_the_reference_raises_on_are_flagged(fx):
    """the reference's own optimum for mu = 64, r = 0.15 is one column too long for max_length: the contract cuts and sets bit 1"""
    tab, a = fixture_tables(fx), fixture_args(fx)
    assert len(fx["raised_lengths"]) >= 1
    for row in range(len(fx["raised_lengths"])):
        d = int(fx["raised_denoiser"][row])
        # any mask of the contract has the same stream lengths: draw one
        got = ul2_ref.collate(fx["raised_tokens"][row:row + 1], fx["raised_lengths"][row:row + 1], dict(tab, cum_prop=[float(i >= d) for i in range(len(tab["mu"]))]),
                              seed=5, step=row, **a)
        assert got["denoiser"][0] == d
        assert got["status"][0] == 1 and got["enc_len"][0] == a["max_length"]
        assert got["input_ids"][0, -1] == a["eos_token_id"]


def test_ul2_lengths_equal_the_recorded_optima(fx):
    from flasht5_amd.ul2 import ul2_lengths, _host_tables
    longest = int(np.diff(fx["prefix_off"]).max())
    for s, (ml, mll) in enumerate(fx["settings"]):
        for d in range(len(fx["den_mu"])):
            want = tuple(int(x) for x in fx["optimal_len"][s, d])
            assert ul2_lengths(int(ml), int(mll), float(fx["den_r"][d]), float(fx["den_mu"][d]), longest) == want, (s, d)
    a = fixture_args(fx)
    host = _host_tables(fixture_denoisers(fx), [1.0] * len(fx["den_mu"]), a["max_length"], a["max_labels_length"], a["sentinel_first_id"], a["num_sentinels"])
    assert host["tokens_len"] == [int(x) for x in fx["optimal_len"][0, :, 0]]
    assert host["prefix_off"] == [int(x) for x in fx["prefix_off"]] and host["prefix_ids"] == [int(x) for x in fx["prefix_ids"]]
    assert host["cum_prop"][-1] == pytest.approx(1.0) and all(x < y for x, y in zip(host["cum_prop"], host["cum_prop"][1:]))


def test_exports_and_sizeof():
    from flasht5_amd import _lib
    import flasht5_amd
    lib = _lib.load()
    assert {"fat5_ul2_collate", "fat5_sizeof_ul2_params"} <= set(_lib.EXPORTS)
    assert lib.fat5_sizeof_ul2_params() == ctypes.sizeof(_lib.Ul2Params)
    for name in ("ul2_lengths", "ul2_tables", "ul2_collate", "UL2Collator"):
        assert hasattr(flasht5_amd, name)
    # the descriptor is checked before anything is launched (no GPU needed)
    assert lib.fat5_ul2_collate(None, None) == -1
    p = _lib.Ul2Params()
    assert lib.fat5_ul2_collate(ctypes.byref(p), None) == -1 and b"ul2_collate" in lib.fat5_last_error()
    p.B, p.L, p.max_length, p.max_labels_length, p.num_denoisers, p.num_sentinels = 1, 8, 8, 8, 1, 100
    assert lib.fat5_ul2_collate(ctypes.byref(p), None) == -1 and b"tokens" in lib.fat5_last_error()
    p.num_denoisers = 257
    assert lib.fat5_ul2_collate(ctypes.byref(p), None) == -1 and b"num_denoisers" in lib.fat5_last_error()


GOOD = dict(max_length=64, max_labels_length=64, sentinel_first_id=32099, num_sentinels=100, eos_token_id=1, pad_token_id=0, seed=0)
DEN = dict(mu=3.0, r=0.15, max_spans=100, prefix_ids=[31990])


@pytest.mark.parametrize("denoiser, kwargs, match", [
    (dict(DEN, mu=0.5), {}, "mu"),
    (dict(DEN, mu=float("nan")), {}, "mu"),
    (dict(DEN, r=1.0), {}, "r ="),
    (dict(DEN, r=-0.1), {}, "r ="),
    (dict(DEN, max_spans=0), {}, "max_spans"),
    (dict(DEN, prefix_ids=[32000]), {}, "sentinel range"),
    (dict(DEN, prefix_ids=[32099]), {}, "sentinel range"),
    (dict(DEN, prefix_ids=[-3]), {}, "negative"),
    (DEN, dict(max_length=5000, max_labels_length=5000), "4096"),
    (DEN, dict(max_length=1), "prefix"),
    (DEN, dict(max_length=2), "at least 2 tokens"),
    (DEN, dict(max_labels_length=0), "at least 1"),
    (DEN, dict(num_sentinels=0), "num_sentinels"),
    (DEN, dict(sentinel_first_id=50), "below 0"),
])
def test_host_checks_of_the_denoisers(denoiser, kwargs, match):
    from flasht5_amd import UL2Collator
    with pytest.raises(ValueError, match=match):
        UL2Collator([denoiser], [1.0], **dict(GOOD, **kwargs))


def test_host_checks_of_the_proportions():
    from flasht5_amd import UL2Collator
    for props in ([1.0, 1.0], [-1.0], [0.0], [float("nan")]):
        with pytest.raises(ValueError, match="proportions"):
            UL2Collator([DEN], props, **GOOD)
    with pytest.raises(ValueError, match="denoisers"):
        UL2Collator([], [], **GOOD)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        UL2Collator([DEN], [1.0], **GOOD)(torch.zeros(2, 16, dtype=torch.int64), torch.full((2,), 16, dtype=torch.int32))
    # no device is touched by the constructor.  63 columns behind the prefix: n = 69 has rint(10.35) = 10 noise tokens in
    # rint(3.33) = 3 spans, 59 + 3 + 1 = 63 columns; n = 70 has rint(10.5) = 10 (half to even), 60 + 3 + 1 = 64
    assert UL2Collator([DEN], [1.0], **GOOD).tokens_len == [69]


def test_host_checks_of_a_call():
    """dtypes and shapes before devices: a CPU tensor of the right kind is refused as not being on the device"""
    from flasht5_amd.ul2 import ul2_collate, UL2Tables
    a = {k: v for k, v in GOOD.items()}
    tokens, lengths = torch.zeros(2, 16, dtype=torch.int64), torch.full((2,), 16, dtype=torch.int32)
    step = torch.zeros(1, dtype=torch.int64)
    tab = UL2Tables(*(torch.zeros(1) for _ in range(7)))
    call = lambda t=tokens, n=lengths, **kw: ul2_collate(t, n, tab, step, **dict(a, **kw))   # noqa: E731
    with pytest.raises(ValueError, match=r"\(B, L\)"):
        call(t=tokens[0])
    with pytest.raises(ValueError, match="int64"):
        call(t=tokens.int())
    with pytest.raises(ValueError, match="at least one row"):
        call(t=tokens[:0])
    with pytest.raises(RuntimeError, match="HIP device"):
        call()


def chi2_quantile(p_upper, k):
    """the chi-square quantile with upper tail p_upper at k degrees of freedom"""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p_upper, k))
    except ImportError:   # Wilson-Hilferty: chi2_k ~ k (1 - 2/(9k) + z sqrt(2/(9k)))^3, z the normal quantile (by bisection on erfc)
        lo, hi = 0.0, 10.0
        for _ in range(80):
            z = (lo + hi) / 2
            lo, hi = (z, hi) if 0.5 * math.erfc(z / math.sqrt(2)) > p_upper else (lo, z)
        return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


def test_segmentation_is_uniform():
    """all C(5, 2) = 10 compositions of 6 into 3 positive parts over 20,000 rows of one fixed seed: Pearson's statistic stays below
    the chi-square quantile (9 degrees of freedom) at p = 1e-4"""
    rows, seed, step, stream = 20000, 20240517, 3, 1
    # the restatement's segmentation, the Philox words of all rows at once: positions 0 .. 4 are lanes 0 .. 3 of block 0 and lane 0 of block 1
    r = np.arange(rows)
    w0, w1 = ul2_ref.words(0, r, stream, step, seed), ul2_ref.words(1, r, stream, step, seed)
    keys = np.stack([(w0[i].astype(np.uint64) << np.uint64(32)) | np.uint64(i) for i in range(4)] + [(w1[0].astype(np.uint64) << np.uint64(32)) | np.uint64(4)], axis=1)
    counts = {}
    for b in range(rows):
        cuts = sorted(int(k) & 0xFFFFFFFF for k in sorted(keys[b])[:2])
        parts = (cuts[0] + 1, cuts[1] - cuts[0], 6 - cuts[1] - 1)
        counts[parts] = counts.get(parts, 0) + 1
        if b < 50:   # (the vectorised keys are the restatement's)
            assert list(parts) == ul2_ref.segmentation(6, 3, b, stream, step, seed)
    assert len(counts) == 10 and all(min(c) >= 1 and sum(c) == 6 for c in counts)
    expect = rows / 10
    stat = sum((c - expect) ** 2 / expect for c in counts.values())
    bound = chi2_quantile(1e-4, 9)
    assert 33.0 < bound < 34.5   # (33.72 exactly)
    print(f"Pearson statistic {stat:.2f}, bound {bound:.2f}")
    assert stat < bound
