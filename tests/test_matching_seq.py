"""CPU: the weighted matching summary's rules header (csrc/gs_matching_seq.hpp: the wrapping
acceptance test, the state record, the cells, the may-accept rule, the phase functions of a
round, the sequential definition and the fold by rounds) in a stand-alone program built with the
address and undefined-behaviour sanitizers (tests/cpp/matching_seq_sanitize.cpp): mt_fold_seq
against a brute-force scan of M, mt_fold_rounds against mt_fold_seq under every tuning. The
header is the one the kernels include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gelly-streaming_amd", "csrc")


def test_rules_and_round_scheme_under_address_and_undefined_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "matching_seq_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + CSRC,
                            os.path.join(ROOT, "tests", "cpp", "matching_seq_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_kernels_and_host_include_the_checked_header():
    with open(os.path.join(CSRC, "gs_matching.hpp")) as f:
        hpp = f.read()
    assert '#include "gs_matching_seq.hpp"' in hpp and '#include "gs_distinct.hpp"' in hpp
    with open(os.path.join(CSRC, "gs_matching_k.hip")) as f:
        text = f.read()
    assert '#include "gs_matching.hpp"' in text and '#include "gs_scan.hpp"' in text
    for fn in ("mt_ph_reset(", "mt_ph_seed(", "mt_ph_pass(", "mt_ph_lower(", "mt_ph_remain(", "mt_ph_commit(",
               "mt_event_rows(", "mt_weight_safe(", "mt_vertex_init(", "block_excl_scan<", "block_count_to<"):
        assert fn in text, fn
    with open(os.path.join(CSRC, "gs_matching.cpp")) as f:
        host = f.read()
    assert '#include "gs_matching.hpp"' in host
    for fn in ("kMatchingRoundCap", "kMatchingTailThreshold", "kMatchingIterCap", "kMatchingMaxIterCap", "kMtMaxFold",
               "mt_wrap_add(", "launch_dist_vertices(", "launch_tile_scan("):
        assert fn in host, fn
    # the phase functions are made of the rules
    with open(os.path.join(CSRC, "gs_matching_seq.hpp")) as f:
        seq = f.read()
    for fn in ("mt_accepts(", "mt_cells(", "mt_collision_sum(", "mt_lower_bound(", "mt_may_accept("):
        assert seq.count(fn) >= 2, fn
    assert "inline uint64_t mt_fold_seq(" in seq and "inline uint64_t mt_fold_rounds(" in seq
    # no second open-addressing insert: the vertex table is the distinct streams'
    assert "atomicCAS" not in text and "atomicCAS" not in host
    # the header itself reads standard headers only (and the HIP runtime under a HIP compiler)
    incs = [l.split()[1] for l in seq.splitlines() if l.startswith("#include")]
    assert all(i.startswith("<") for i in incs), incs
