"""CPU: the k-spanner summary's sequential definitions (csrc/gs_spanner_seq.hpp: status bytes,
the traversal predicate, the capacity arithmetic, the step rule, within, the fold and the fold by
rounds) against brute force in a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/cpp/spanner_seq_sanitize.cpp). The header is the one the
kernels include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")


def test_sequential_definitions_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "spanner_seq_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "spanner_seq_sanitize.cpp"), "-o", exe],
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
    with open(os.path.join(CSRC, "gs_spanner.hpp")) as f:
        assert '#include "gs_spanner_seq.hpp"' in f.read()
    with open(os.path.join(CSRC, "gs_spanner_k.hip")) as f:
        text = f.read()
    assert '#include "gs_spanner.hpp"' in text and '#include "gs_triangle_rows.hpp"' in text
    for fn in ("sp_traversable(", "sp_round_verdict(", "sp_pick_side(", "sp_set_slots(", "sp_hash(", "sp_stamp(",
               "kSpDead", "kSpannerLdsSet", "tri_row(", "tri_has_pair(", "tri_pair_lower("):
        assert fn in text, fn
    with open(os.path.join(CSRC, "gs_spanner.cpp")) as f:
        host = f.read()
    for fn in ("sp_clamp_set(", "sp_slow_round(", "kSpMaxGen", "kSpannerMaxK"):
        assert fn in host, fn
    # the header itself reads standard headers only (and the HIP runtime under a HIP compiler)
    with open(os.path.join(CSRC, "gs_spanner_seq.hpp")) as f:
        incs = [l.split()[1] for l in f.read().splitlines() if l.startswith("#include")]
    assert all(i.startswith("<") for i in incs), incs
