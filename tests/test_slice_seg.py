"""CPU: the window slices' segmented-combine operator and tile / carry arithmetic
(csrc/gs_slice_seg.hpp) against brute force in a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/cpp/slice_seg_sanitize.cpp). The header is the one the
kernels include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_arithmetic_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "slice_seg_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "slice_seg_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_kernels_include_the_checked_header():
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_slice_k.hip")) as f:
        text = f.read()
    assert '#include "gs_slice_seg.hpp"' in text
    for fn in ("seg_combine<", "seg_push<", "seg_identity<", "slice_op<", "slice_emit(", "slice_closed(",
               "slice_out_rank(", "slice_fixup(", "slice_fixup_rank(", "slice_tile_begin(", "slice_tile_end(",
               "slice_tiles(", "slice_edge_of(", "slice_key_is_src("):
        assert fn in text, fn
