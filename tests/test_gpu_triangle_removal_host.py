"""GPU: the SlidingWindowTriangles driver of the C++ host mirror
(tests/cpp/test_triangle_removal.cpp -> gelly_streaming.hpp -> libgs_summary.so) on the
reference's 19 pinned edges: the pinned WindowTriangles rows with size == slide, a brute-force
count per union of two panes with size == 2 slide, and the refusal of size % slide != 0."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def test_the_program_holds_the_pinned_edges():
    """The rows in the C++ source are tests/golden/triangle_pins.json's triangles_data."""
    with open(os.path.join(ROOT, "tests", "golden", "triangle_pins.json")) as f:
        pins = json.load(f)
    with open(os.path.join(ROOT, "tests", "cpp", "test_triangle_removal.cpp")) as f:
        text = f.read()
    block = text[text.index("rows[19][3]"):text.index("for (const auto& r : rows)")]
    rows = [[int(x) for x in m] for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", block)]
    assert rows == [list(e) for e in pins["triangles_data"]["edges"]]


def test_sliding_window_triangles_on_host_mirror():
    exe = os.path.join(BIN, "test_triangle_removal")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("sizeEqualsSlide", "equalsWindowTriangles", "bruteForceHasTheFourWindows", "twoPanes", "gap",
                 "sizeNotAMultipleOfSlide"):
        assert "PASS SlidingWindowTriangles." + name in r.stdout
    assert "0 failure(s)" in r.stdout
