"""GPU: SimpleEdgeStream's continuous degree and count calls on the C++ host mirror
(tests/cpp/test_degstream.cpp -> gelly_streaming.hpp -> libgs_summary.so) and the
degree_distribution example program, against the reference's pinned outputs
(tests/golden/degree_pins.json)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def _pins():
    with open(os.path.join(ROOT, "tests", "golden", "degree_pins.json")) as f:
        return json.load(f)


def test_degree_streams_on_host_mirror():
    exe = os.path.join(BIN, "test_degstream")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("TestGetDegrees.testGetDegrees stream", "TestGetDegrees.testGetInDegrees stream",
                 "TestGetDegrees.testGetOutDegrees stream", "getDegreeStream arrival order",
                 "TestNumberOfEntities.testNumberOfVertices stream", "TestNumberOfEntities.testNumberOfEdges stream",
                 "SimpleEdgeStream last values", "SimpleEdgeStream.empty streams",
                 "DegreeDistribution.DEGREES_RESULT stream", "DegreeDistribution.DEGREES_RESULT_ZERO stream",
                 "degreeDistributionStream deletion count"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout


def test_degree_distribution_example(tmp_path):
    exe = os.path.join(BIN, "degree_distribution")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    pins = _pins()
    # the example's default data is DEGREES_DATA
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split("\n")[:-1] == pins["degrees_result"]["text"].split("\n")
    path = tmp_path / "events.txt"
    path.write_text(pins["degrees_data_zero"]["text"] + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split("\n")[:-1] == pins["degrees_result_zero"]["text"].split("\n")
    r = subprocess.run([exe, str(tmp_path / "missing.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot read" in r.stderr
