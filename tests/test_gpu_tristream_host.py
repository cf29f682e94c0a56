"""GPU: ExactTriangleCount's continuous stream on the C++ host mirror (tests/cpp/test_tristream.cpp
-> gelly_streaming.hpp -> libgs_summary.so) and the exact_triangle_count example program, against
the sequence derived from the reference's code (tests/golden/tristream_pins.json)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def _pins():
    with open(os.path.join(ROOT, "tests", "golden", "tristream_pins.json")) as f:
        return json.load(f)


def test_triangle_stream_on_host_mirror():
    exe = os.path.join(BIN, "test_tristream")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("ExactTriangleCount.stream built-in stream", "ExactTriangleCount.stream batch 1, 4 and n",
                 "ExactTriangleCount.stream last values == run", "ExactTriangleCount.stream repeated edge and loop",
                 "ExactTriangleCount.stream empty stream"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout
    # the program's literal is the pins' derived sequence
    with open(os.path.join(ROOT, "tests", "cpp", "test_tristream.cpp")) as f:
        text = f.read()
    lit = ", ".join("{%d, %d}" % (k, v) for k, v in _pins()["derived"]["tuples"])
    assert "want = {%s};" % lit in text


def test_exact_triangle_count_example(tmp_path):
    exe = os.path.join(BIN, "exact_triangle_count")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    pins = _pins()
    # the example's default data is the built-in stream
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split("\n")[:-1] == ["(%d,%d)" % (k, v) for k, v in pins["derived"]["tuples"]]
    case = pins["test_intersection"]["cases"][0]
    path = tmp_path / "edges.txt"
    path.write_text("% a comment line\n" + "".join("%d %d\n" % (s, d) for s, d in case["as_stream"]))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split("\n")[:-1] == ["(%d,%d)" % (k, v) for k, v in case["expected_tuples"]]
    r = subprocess.run([exe, str(tmp_path / "missing.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot read" in r.stderr
