"""GPU: TriangleEstimate and BroadcastTriangleCount of the C++ host mirror
(tests/cpp/test_trisample.cpp -> gelly_streaming.hpp -> libgs_summary.so) against the sequential
definition of csrc/gs_trisample_seq.hpp on the reference's default stream at 256 samples and on
K16, at several batch sizes, and the broadcast_triangle_count example program on its built-in
stream and on a file (the K5 pin of tests/golden/trisample_pins.json)."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def test_trisample_on_host_mirror():
    exe = os.path.join(BIN, "test_trisample")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("BroadcastTriangleCount.defaultStream", "BroadcastTriangleCount.defaultStream.estimate",
                 "BroadcastTriangleCount.defaultStream.batch7", "BroadcastTriangleCount.k16",
                 "TriangleEstimate.accessors", "BroadcastTriangleCount.k16.batch1", "BroadcastTriangleCount.k5Pin",
                 "BroadcastTriangleCount.rejectsTwoVertices"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout


def test_example_program_default_stream_and_file(tmp_path):
    exe = os.path.join(BIN, "broadcast_triangle_count")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    # the built-in stream (2000 edges, 1000 vertices, 10000 samples): rows "(edges,estimate)", edge counts ascending
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(x) for x in re.fullmatch(r"\((\d+),(-?\d+)\)", line).groups()) for line in r.stdout.splitlines()]
    assert rows and all(a[0] < b[0] for a, b in zip(rows[:-1], rows[1:])) and rows[-1][0] <= 2000
    assert all(a[1] != b[1] for a, b in zip(rows[:-1], rows[1:]))  # a row only when the estimate changes
    # the K5 pin from a tab-separated file, folded three arrivals at a time
    with open(os.path.join(ROOT, "tests", "golden", "trisample_pins.json")) as f:
        pin = json.load(f)["k5_twice"]
    k5 = [(a, b) for a in range(5) for b in range(a + 1, 5)] * 2
    path = tmp_path / "k5.txt"
    path.write_text("".join("%d\t%d\n" % e for e in k5))
    r = subprocess.run([exe, str(path), str(pin["vertices"]), str(pin["samples"]), "3"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["(%d,%d)" % tuple(x) for x in pin["rows"]]
    assert subprocess.run([exe, "one-argument"], capture_output=True, text=True, timeout=120).returncode == 1
