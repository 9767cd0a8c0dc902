"""CPU test: the attention dispatch policy answers a few thousand problems exactly as tests/dispatch_snapshot.txt records
(kernel bodies, launch count and workspace size through the public host-only calls; grid and format: tools/dispatch_snapshot.py).
test_dispatch_rules_are_pinned (test_host_cpu.py) pins the MEASURED decisions one by one; this one keeps an edit of the policy code
from moving any other shape, workspace offset or launch count unnoticed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_matches_snapshot():
    from flasht5_amd import _lib as L
    if L.load().fat5_chip_cus() != 256:  # (the thresholds are rounds of the chip, as in test_dispatch_rules_are_pinned)
        pytest.skip("the dispatch snapshot holds for a 256-CU device (MI355X) or no device at all")
    spec = importlib.util.spec_from_file_location("dispatch_snapshot", os.path.join(ROOT, "tools", "dispatch_snapshot.py"))
    snap = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(snap)
    assert len(snap.cases()) >= 3000
    bad = snap.compare(L.load())
    assert not bad, f"{len(bad)} case(s) differ from the snapshot, the first:\n" + "\n".join(
        f"{lab}\n  snapshot: {w}\n  library:  {g}" for lab, w, g in bad[:5])
