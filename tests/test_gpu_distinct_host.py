"""GPU: SimpleEdgeStream::distinct and getVertices on the C++ host mirror
(tests/cpp/test_distinct.cpp -> gelly_streaming.hpp -> libgs_summary.so), against the
reference's pinned outputs (TestDistinct.java, TestGetVertices.java)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def test_distinct_on_host_mirror():
    exe = os.path.join(BIN, "test_distinct")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestDistinct.test", "TestGetVertices.test", "Distinct.getVertices.doubledStream",
                 "Distinct.values.firstKept", "Distinct.timestamps.firstKept", "Distinct.idempotent",
                 "Distinct.twoFolds.newEdges", "Distinct.twoFolds.newVertices", "Distinct.twoFolds.size",
                 "Distinct.twoFolds.edges"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout
