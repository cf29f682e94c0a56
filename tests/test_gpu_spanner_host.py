"""GPU: AdjacencyListGraph and Spanner of the C++ host mirror (tests/cpp/test_spanner.cpp ->
gelly_streaming.hpp -> libgs_summary.so), against the reference's pinned sequences and the
sequential restatement, and the SpannerExample program on its default stream."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def test_spanner_on_host_mirror():
    exe = os.path.join(BIN, "test_spanner")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("AdjacencyListGraphTest.testBoundedBFS", "AdjacencyListGraphTest.testAddEdge",
                 "SpannerExample.defaultStream", "Spanner.aggregate.windowsOfFour", "Spanner.aggregate.spansTheStream",
                 "CombineSpanners.reduce.moreVertices", "CombineSpanners.reduce.fewerVertices",
                 "CombineSpanners.reduce.tie"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout


def test_spanner_example_default_stream():
    exe = os.path.join(BIN, "spanner_example")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # FlattenSet: one (src, trg) line per kept edge; one window holds the whole default stream
    want = [(1, 4), (2, 3), (3, 4), (4, 5), (4, 7), (5, 6), (6, 8), (7, 8), (8, 9)]
    assert r.stdout.splitlines() == ["(%d,%d)" % e for e in want]
