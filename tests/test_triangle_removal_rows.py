"""CPU: the removal arithmetic of the triangle summary (csrc/gs_triangle_rows.hpp: the pair
lookup, the age test, the stamp rebase at the fold number's wrap, the vanished-row test) and a
host removal composed of it, against brute force in a stand-alone program built with the address
and undefined-behaviour sanitizers (tests/cpp/triangle_removal_sanitize.cpp). The header is the
one the kernels include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_removal_arithmetic_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "triangle_removal_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "triangle_removal_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_kernels_use_the_checked_functions():
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_triangle_k.hip")) as f:
        text = f.read()
    for fn in ("tri_pair_at(", "tri_is_old(", "tri_rebase(", "tri_row_gone("):
        assert fn in text, fn
