import os
import sys

# fp32 CPU matmuls (the attention oracle against the golden fixtures) round differently with the code path MKL picks for the
# host's CPU.  The fixtures are frozen under MKL's conditional-numerical-reproducibility mode COMPATIBLE
# (tests/golden/make_golden.py), which takes the same path on every x86 CPU; it must be set before MKL is first called, i.e.
# before torch computes anything.  (fp32 sqrt is not covered by it: see golden_io.ieee_sqrt.)
os.environ["MKL_CBWR"] = "COMPATIBLE"

import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def pytest_collection_modifyitems(config, items):
    if _has_gpu():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
