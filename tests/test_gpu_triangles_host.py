"""GPU: the WindowTriangles and ExactTriangleCount drivers of the C++ host mirror
(tests/cpp/test_triangles.cpp -> gelly_streaming.hpp -> libgs_summary.so), against the
reference's pinned outputs."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def test_triangles_on_host_mirror():
    exe = os.path.join(BIN, "test_triangles")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("WindowTrianglesITCase.test", "ExactTriangleCount.defaultStream", "ExactTriangleCount.batchings"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout
