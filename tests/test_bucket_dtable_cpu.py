"""Host-only: which reduction forms the T5 table gradient (fat5_attn_describe `dtable=`).  The bucket-run form
(csrc/reduce_kernels.h: drpe_runs_reduce_kernel) is taken where the call asks for the (num_buckets, H) table only and hands
over a host copy of the bucket map whose every id occupies one contiguous run; everything else keeps the per-diagonal
reduction and its bucket scan."""
import ctypes

import pytest

from flasht5_amd import _lib
from flasht5_amd import positional_encoding as pe


def _t5_map(md=128, radius=None, bidir=True, nb=32):
    R = pe.rpe_radius(md) if radius is None else radius
    return [int(x) for x in pe._bucket_index_cpu(R, bidir, nb, md)], R


def _desc(bucket, R, **kw):
    args = dict(B=4, H=12, M=512, N=512, bias_mode=_lib.BIAS_RPE1D, radius=R, need_dbias=True, bucket=bucket)
    args.update(kw)
    return _lib.describe(**args)


@pytest.mark.parametrize("md,radius,bidir", [(128, None, True), (128, 512, True), (32, None, True), (128, None, False)])
def test_t5_maps_take_the_run_form(md, radius, bidir):
    bucket, R = _t5_map(md, radius, bidir)
    assert _desc(bucket, R)["dtable"] == "runs"
    assert _desc(bucket, R, variant=_lib.V_DTABLE_RUNS_ON)["dtable"] == "runs"
    assert _desc(bucket, R, variant=_lib.V_DTABLE_RUNS_OFF)["dtable"] == "scan"
    # the choice of the reduction does not move the kernel bodies
    d_on, d_off = _desc(bucket, R), _desc(bucket, R, variant=_lib.V_DTABLE_RUNS_OFF)
    assert {k: v for k, v in d_on.items() if k != "dtable"} == {k: v for k, v in d_off.items() if k != "dtable"}


def test_cfg2_dispatch():
    bucket, R = _t5_map()
    d = _desc(bucket, R)
    assert d["dtable"] == "runs" and d["fused"] == "1"


def test_fallbacks():
    bucket, R = _t5_map()
    # a bucket id in two places: not a sequence of runs
    bad = list(bucket)
    bad[0], bad[R] = bad[R], bad[0]
    assert _desc(bad, R)["dtable"] == "scan"
    # ids outside [0, num_buckets) are left out of the table in either form; they do not break a run
    assert _desc([-1] + bucket[1:], R)["dtable"] == "runs"
    # more buckets than the kernel's argument block holds
    many = list(range(2 * R + 1))
    assert _desc(many, R, num_buckets=2 * R + 1)["dtable"] == "scan"
    assert _desc(many[:129] + [128] * (2 * R + 1 - 129), R, num_buckets=129)["dtable"] == "scan"
    assert _desc(many[:128] + [127] * (2 * R + 1 - 128), R, num_buckets=128)["dtable"] == "runs"
    # no host map, or the (H, 2R+1) generator's gradient asked for: no table-only call, no dtable entry
    assert "dtable" not in _lib.describe(B=4, H=12, M=512, N=512, bias_mode=_lib.BIAS_RPE1D, radius=R, need_dbias=True)
    p = _lib.AttnParams()
    p.B, p.H, p.M, p.N, p.D, p.dtype = 4, 12, 512, 512, 64, _lib.FAT5_BF16
    p.sm_scale, p.bias_mode, p.rpe_radius, p.rpe1d = 0.125, _lib.BIAS_RPE1D, R, 16
    host = (ctypes.c_int32 * len(bucket))(*bucket)
    p.rpe_bucket, p.drpe_table, p.rpe_num_buckets, p.rpe_bucket_host = 16, 16, 32, ctypes.addressof(host)
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().fat5_attn_describe(ctypes.byref(p), buf, 256), "describe")
    assert "dtable=runs" in buf.value.decode()
    p.drpe1d = 16  # both gradients: the per-diagonal sums are an output, so the per-diagonal reduction runs
    _lib.check(_lib.load().fat5_attn_describe(ctypes.byref(p), buf, 256), "describe")
    assert "dtable" not in buf.value.decode()


def test_the_host_copy_of_a_cached_map():
    import torch
    dev = torch.device("cpu")
    idx = pe.bucket_index32(128, True, 32, 128, dev)
    host = pe.host_bucket_map(idx)
    assert host is not None and host.dtype == torch.int32 and torch.equal(host, idx)
    assert pe.host_bucket_map(idx.clone()) is None
